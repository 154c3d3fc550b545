/*
 * mamba_hip.h — C ABI of the MI355X many-chain MCMC engine (libmambahip.so).
 *
 * Drop-in boundary: this library replaces, for the supported
 * lowered models, everything Mamba.jl runs under `pmap2(mcmc_worker!, lsts)`
 * in `mcmc_master!`:
 *   /root/reference/src/model/mcmc.jl:36-59   mcmc_master!  (chain fan-out)
 *   /root/reference/src/model/mcmc.jl:62-83   mcmc_worker!  (per-chain loop, keep rule)
 *   /root/reference/src/model/simulation.jl:93-107  sample!(m)  (block sweep)
 *   /root/reference/src/samplers/{amwg,amm,nuts,slice}.jl  (block updates)
 *   /root/reference/src/model/simulation.jl:47-90   logpdf! / gradlogpdf!
 * A Julia `ccall` shim binds these symbols from a specialised
 * mcmc_master!; unsupported models/schemes return MMB_E_UNSUPPORTED so the
 * shim can fall back to the Julia path.
 *
 * Conventions: every function returns 0 on success or a negative MMB_E* code
 * (message via mmb_last_error); nothing throws across the ABI.  All real
 * arrays are FP64 (Mamba is Float64-only, src/Mamba.jl:57-58).  Host buffers
 * are caller-owned; device memory is owned by the engine.  An engine is used by
 * one host thread at a time (one engine per GPU; multi-GPU = one process per
 * GPU, each with its own shard of global chain ids).
 */
#ifndef MAMBA_HIP_H
#define MAMBA_HIP_H

#if !defined(__HIPCC_RTC__)
#include <stddef.h>
#include <stdint.h>
#else  /* hipRTC (node-IR specialisation): fixed-width types from its runtime header */
typedef __hip_internal::int8_t int8_t;
typedef __hip_internal::uint8_t uint8_t;
typedef __hip_internal::int16_t int16_t;
typedef __hip_internal::uint16_t uint16_t;
typedef __hip_internal::int32_t int32_t;
typedef __hip_internal::uint32_t uint32_t;
typedef __hip_internal::int64_t int64_t;
typedef __hip_internal::uint64_t uint64_t;
typedef __UINTPTR_TYPE__ uintptr_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MMB_ABI_VERSION 10
#define MMB_MAX_BLOCKS 8
#define MMB_MAX_NODES_PER_BLOCK 4

/* ---- error codes ---- */
#define MMB_OK 0
#define MMB_E_ARG (-1)         /* invalid argument (ArgumentError in mcmc.jl:22-25, amwg.jl:37-42) */
#define MMB_E_UNSUPPORTED (-2) /* model/scheme not lowered to a kernel: fall back to Julia */
#define MMB_E_HIP (-3)         /* HIP runtime error */
#define MMB_E_STATE (-4)       /* call out of order (e.g. run before init) */
#define MMB_E_NOMEM (-5)
#define MMB_E_COMM (-6)        /* RCCL error in a cross-GPU collective (mmb_comm_*, mmb_gr_allreduce) */
/* Slice shrinkage bound: the reference shrinks until it accepts (slice.jl:78-88,103-113); a
 * kernel must end, so an update still rejecting after this many candidates stops and mmb_run
 * returns MMB_E_STATE (only a degenerate target, e.g. an infinite width, gets there). */
#define MMB_SLICE_MAX_SHRINK 100000

/* ---- lowered model kinds ---- */
typedef enum {
  MMB_MODEL_LINE = 1,    /* doc/tutorial/line.jl:5-25   y ~ IsoNormal(xmat*beta, sqrt(s2)) */
  MMB_MODEL_RATS = 2,    /* doc/examples/rats.jl:48-97  hierarchical growth model */
  MMB_MODEL_LOGISTIC = 3, /* build-defined:  y ~ Bernoulli(invlogit(X*beta)) */
  MMB_MODEL_IR = 4        /* generic node IR: created by mmb_create_ir */
} mmb_model_kind;

/* node ids (Stochastic nodes that can appear in a sampling block) */
enum { MMB_LINE_BETA = 0, MMB_LINE_S2 = 1,
       MMB_LINE_Y = 2 /* the observed node: valid in the node lists of mmb_draws_logpdf, mmb_draws_predict and their kin only */ };
enum {
  MMB_RATS_S2_C = 0, MMB_RATS_ALPHA = 1, MMB_RATS_MU_ALPHA = 2, MMB_RATS_S2_ALPHA = 3,
  MMB_RATS_BETA = 4, MMB_RATS_MU_BETA = 5, MMB_RATS_S2_BETA = 6
};
enum { MMB_LOGISTIC_BETA = 0 };

/* ---- sampler kinds (src/samplers/{amwg,amm,nuts,slice,hmc,mala}.jl) ---- */
typedef enum {
  MMB_SAMPLER_AMWG = 1,  /* src/samplers/amwg.jl:47-61 */
  MMB_SAMPLER_AMM = 2,   /* src/samplers/amm.jl:45-59    */
  MMB_SAMPLER_NUTS = 3,  /* src/samplers/nuts.jl:47-56 */
  MMB_SAMPLER_SLICE = 4, /* src/samplers/slice.jl:47-58 */
  MMB_SAMPLER_GIBBS = 5, /* user Sampler(params, f): conjugate full conditional of the block's node,
                            e.g. doc/tutorial/line.jl:27-45 */
  MMB_SAMPLER_HMC = 6,   /* src/samplers/hmc.jl:47-65 */
  MMB_SAMPLER_MALA = 7,  /* src/samplers/mala.jl:43-58 */
  MMB_SAMPLER_RWM = 8,   /* src/samplers/rwm.jl:49-71 (additive: the ABI version is unchanged) */
  MMB_SAMPLER_DGS = 9,   /* src/samplers/dgs.jl:56-126: discrete Gibbs sampling of one discrete node-IR node
                            (additive: the ABI version is unchanged) */
  MMB_SAMPLER_SLICESIMPLEX = 10, /* src/samplers/slicesimplex.jl:24-122: slice sampling of one Dirichlet node-IR node
                                    on its simplex; mmb_block_spec.scale in (0, 1], no tune state (additive too) */
  /* The binary samplers of one Bernoulli or DiscreteUniform(0, 1) node-IR node of 1..32 elements (additive too).
   * BMG / BMC3: k is an int in mmb_block_spec.nsteps (form = MMB_BINARY_K_INT), or index lists in tuning, one
   * 32-bit mask per list (bit i = element i + 1) stored as a double, 1..MMB_BINARY_MAX_LISTS of them
   * (form = MMB_BINARY_K_LISTS); no tune state.  BIA: epsilon in epsilon, decay in beta, target in target,
   * the initial A[dim] then D[dim] in tuning; tune row [iter, A[dim], D[dim]]. */
  MMB_SAMPLER_BMG = 11,  /* src/samplers/bmg.jl:57-101: binary Metropolised Gibbs */
  MMB_SAMPLER_BMC3 = 12, /* src/samplers/bmc3.jl:57-65: binary MC3 */
  MMB_SAMPLER_BIA = 13,  /* src/samplers/bia.jl:70-119: binary individual adaptation */
  /* BHMC of one such node (additive too): traveltime in mmb_block_spec.scale, finite, > 0 and
   * <= MMB_BHMC_MAX_TRAVELTIME; refresh in form (0: the reference, the velocity is never redrawn; 1: it is
   * redrawn at the start of every update).  Tune row [position[dim], velocity[dim], wallhits, wallcrosses,
   * initialised]; a chain whose `initialised` is 0 draws its particle at its first update. */
  MMB_SAMPLER_BHMC = 14, /* src/samplers/bhmc.jl:35-122: binary Hamiltonian Monte Carlo */
  /* ABC of one or more continuous node-IR nodes (additive too; node-IR models only).  Packed into the fields of
   * mmb_block_spec:
   *   form       proposal | kernel << 8 | randeps << 16   (proposal, kernel: mmb_rwm_proposal; randeps 0 or 1)
   *   batchsize  maxdraw, 1..MMB_ABC_MAX_DRAW          nsteps   nsim, 1..MMB_ABC_MAX_NSIM
   *   beta       decay in [0, 1]                       epsilon  the target tolerance, finite and > 0
   *   transform  1                                     tuning   scale[dim] (finite, >= 0), then the summary codes
   *                                                             (mmb_abc_summary, 1..MMB_ABC_MAX_SUMMARY of them)
   * The data nodes are the block's terms that are not its params (mmb_ir_block.term with trans == 0), in term
   * order: at least one, at most MMB_ABC_MAX_DATA, each a Normal, MvNormal, Bernoulli, Binomial, Poisson,
   * Exponential or Uniform node.  Each contributes its summary (the listed statistics in the listed order;
   * MMB_ABC_IDENTITY, which may only stand alone: its elements) and the summaries are concatenated: T = their
   * total length, 1..MMB_ABC_MAX_T.  MMB_ABC_VAR and MMB_ABC_STD need nodes of >= 2 elements.
   * Tune row [initialised, Tsim[nsim][T], epsilon[nsim], epsilonprime[nsim]], length 1 + nsim (T + 2); a chain
   * whose `initialised` is 0 simulates its first Tsim at its first update (abc.jl:47-83). */
  MMB_SAMPLER_ABC = 15   /* src/samplers/abc.jl:23-147: approximate Bayesian computation */
} mmb_sampler_kind;
typedef enum {
  MMB_ABC_IDENTITY = 0, MMB_ABC_SUM = 1, MMB_ABC_MEAN = 2, MMB_ABC_VAR = 3, MMB_ABC_STD = 4, MMB_ABC_MINIMUM = 5,
  MMB_ABC_MAXIMUM = 6
} mmb_abc_summary;
#define MMB_ABC_MAX_DRAW 1024
#define MMB_ABC_MAX_NSIM 8
#define MMB_ABC_MAX_T 32
#define MMB_ABC_MAX_DATA 16
#define MMB_ABC_MAX_SUMMARY 8
typedef enum { MMB_BINARY_K_INT = 0, MMB_BINARY_K_LISTS = 1 } mmb_binary_form;
#define MMB_BINARY_MAX_LISTS 64
#define MMB_BINARY_MAX 32
/* 128 pi: an update has at most dim (floor(traveltime / pi) + 2) wall events, so the cap bounds it by 4160 */
#define MMB_BHMC_MAX_TRAVELTIME 402.1238596594935

typedef enum { MMB_ADAPT_ALL = 0, MMB_ADAPT_BURNIN = 1, MMB_ADAPT_NONE = 2 } mmb_adapt;
typedef enum { MMB_SLICE_MULTIVARIATE = 0, MMB_SLICE_UNIVARIATE = 1 } mmb_slice_form;
/* RWM proposal(0.0, 1.0): Normal or a SymDistributionType (src/distributions/extensions.jl:51-53);
 * the standard variates are drawn as csrc/symdist.h says */
typedef enum {
  MMB_RWM_NORMAL = 0, MMB_RWM_SYMUNIFORM = 1, MMB_RWM_SYMTRIANGULAR = 2, MMB_RWM_EPANECHNIKOV = 3,
  MMB_RWM_BIWEIGHT = 4, MMB_RWM_TRIWEIGHT = 5, MMB_RWM_COSINE = 6
} mmb_rwm_proposal;

/* One sampling block = one Sampler in Model.samplers (src/Mamba.jl:119-124). */
/* Gradient of a NUTS / HMC / MALA block.  The reference differentiates logpdf! with Calculus
 * (gradlogpdf!(m, x, block, transform; dtype = :forward), simulation.jl:47-51): forward
 * differences with epsilon = sqrt(eps()) * max(1, |x_i|), non-finite entries -> 0.
 *   MMB_GRAD_DEFAULT  the model's default: forward differences on line and the node IR (the
 *                     reference's), the analytic gradient kernel on logistic (configs[3]) --
 *                     C callers only; the Python mirror and the Julia shim pass FORWARD or
 *                     ANALYTIC explicitly, so the substitution is never implicit
 *   MMB_GRAD_FORWARD  forward differences (line, node IR, logistic: p + 1 log-density columns
 *                     per gradient through the batched MFMA kernel, ABI 9)
 *   MMB_GRAD_ANALYTIC the hand-derived gradient (line, logistic; node IR: MMB_E_ARG) */
typedef enum { MMB_GRAD_DEFAULT = 0, MMB_GRAD_FORWARD = 1, MMB_GRAD_ANALYTIC = 2 } mmb_gradient;

typedef struct {
  int32_t sampler;                         /* mmb_sampler_kind */
  int32_t nnodes;                          /* number of nodes in `params` */
  int32_t nodes[MMB_MAX_NODES_PER_BLOCK];  /* node ids in block (params) order */
  int32_t adapt;                           /* AMWG/AMM: mmb_adapt (default :all) */
  int32_t form;                            /* Slice: mmb_slice_form (default Multivariate); RWM: mmb_rwm_proposal;
                                              BMG/BMC3: mmb_binary_form; BHMC: refresh (0 or 1);
                                              ABC: proposal | kernel << 8 | randeps << 16 */
  int32_t transform;                       /* Slice: transform flag (default false); AMWG/AMM/NUTS/RWM use true */
  int32_t batchsize;                       /* AMWG batchsize (default 50); ABC maxdraw */
  double target;                           /* AMWG target (0.44) / NUTS target (0.6) / BIA target (0.45) */
  double beta;                             /* AMM beta (0.05); BIA decay (0.55); ABC decay (1.0) */
  double scale;                            /* AMM scale (2.38); SliceSimplex scale in (0, 1]; BHMC traveltime */
  int32_t dim;                             /* unlisted block length (checked by mmb_create) */
  int32_t ntuning;                         /* length of `tuning` */
  const double* tuning;                    /* AMWG sigma[dim] | Slice width[dim] | RWM scale[dim] | AMM Sigma[dim*dim] col-major
                                              | HMC/MALA Sigma[dim*dim] col-major, or none (SigmaL = I)
                                              | BMG/BMC3 list masks | BIA A[dim], D[dim]
                                              | ABC scale[dim], summary codes */
  double epsilon;                          /* HMC/MALA step size (hmc.jl:13, mala.jl:12); BIA epsilon (bia.jl:21); ABC epsilon */
  int32_t nsteps;                          /* HMC leapfrog steps L (hmc.jl:13); BMG/BMC3 int k; ABC nsim */
  int32_t gradient;                        /* NUTS/HMC/MALA logpdfgrad! (sampler.jl:97-111): mmb_gradient */
} mmb_block_spec;

typedef struct {
  int32_t model;                           /* mmb_model_kind */
  int32_t nblocks;
  mmb_block_spec blocks[MMB_MAX_BLOCKS];   /* Model.samplers, in sweep order */
  int32_t nobs;                            /* logistic: N (rows of X) */
  int32_t ncoef;                           /* logistic: p (columns of X) */
  double prior_sd;                         /* logistic: beta ~ MvNormal(p, prior_sd) */
  int32_t reserved[8];
} mmb_model_spec;

/* ---- generic node IR (ABI version 3) ----------------------------------
 * A Mamba Model DAG (src/model/model.jl:5-27, src/model/dependent.jl:75-152) lowered by the
 * host (mamba.jl_amd/ir.py; a Julia shim would walk m.nodes the same way):
 *   - Logical nodes are inlined into the expressions of their Stochastic children;
 *   - Stochastic nodes that no sampling block updates are fixed: values in the data pool;
 *   - the sampled ones own slots [off, off+len) of the chain state (P = nvalues);
 *   - each node's distribution parameters are stack-code expressions evaluated per element i
 *     of the node (elementwise broadcast, src/distributions/distributionstruct.jl:142-158).
 * Block ids in mmb_block_spec.nodes index `nodes`. */
typedef enum {
  MMB_IR_NORMAL = 1,      /* Normal(mu, sigma)                          RealDistribution      */
  MMB_IR_ISONORMAL = 2,   /* MvNormal(mu[], sigma) (PDMats ScalMat)     node-level density    */
  MMB_IR_INVGAMMA = 3,    /* InverseGamma(shape, scale)                 PositiveDistribution  */
  MMB_IR_GAMMA = 4,       /* Gamma(shape, scale)                        PositiveDistribution  */
  MMB_IR_EXPONENTIAL = 5, /* Exponential(scale)                         PositiveDistribution  */
  MMB_IR_UNIFORM = 6,     /* Uniform(a, b), constant bounds lo/hi       bounded (affine logit) */
  MMB_IR_BETA = 7,        /* Beta(a, b)                                 UnitDistribution      */
  MMB_IR_BINOMIAL = 8,    /* Binomial(n, p)     observed, or sampled by a DGS block (n data, max n <= 31:
                             lo = 0, hi = max n, cterm = the lchoose table below) */
  MMB_IR_POISSON = 9,     /* Poisson(lambda)    fixed (observed) nodes only (infinite support) */
  MMB_IR_BERNOULLI = 10,  /* Bernoulli(p)       observed, or sampled by a DGS block (lo = 0, hi = 1) */
  MMB_IR_LOGICAL = 11,    /* Logical: expr[0] is the value (monitored logicals) */
  MMB_IR_CATEGORICAL = 12,     /* Categorical(p), support 1..K: no parameter expression; cterm = pool offset of
                                  the K probabilities (shared by every element), lo = 1, hi = K */
  MMB_IR_DISCRETEUNIFORM = 13, /* DiscreteUniform(a, b), constant integer bounds lo / hi */
  MMB_IR_DIRICHLET = 14        /* Dirichlet(alpha): one node is one distribution of 2 <= len <= 32 elements, a
                                  node-level density; no parameter expression; cterm = pool offset of
                                  alpha[len], then lmnB = sum lgamma(alpha_i) - lgamma(sum alpha_i) */
} mmb_ir_family;
/* A sampled Dirichlet node is updated by a SliceSimplex block only, and such a block holds exactly one
 * Dirichlet node.  Its support is the probability vectors: every x_i >= 0 and |sum x - 1| <=
 * MMB_SIMPLEX_TOL; off it the log density is -Inf.
 * Categorical(P) with P a sampled Dirichlet node reads its probabilities from the chain state:
 * cterm = MMB_IR_CAT_STATE(off) <= -2, off = the first state slot of P, and hi = len(P). */
#define MMB_SIMPLEX_TOL 1e-8
#define MMB_SIMPLEX_MAX 32
#define MMB_IR_CAT_STATE(off) (-2 - (off))
/* A sampled discrete node (Bernoulli, Binomial, Categorical, DiscreteUniform) is updated by a DGS block, or, when
 * it is binary (Bernoulli, DiscreteUniform(0, 1)) and has at most MMB_BINARY_MAX elements, by a BMG, BMC3, BIA or
 * BHMC block; each such block holds exactly one such node.  Its support is the integers lo..hi (Binomial: 0..n_i of
 * element i), at most MMB_DGS_MAX_SUPPORT values.  Off the support its log density is -Inf. */
#define MMB_DGS_MAX_SUPPORT 32

/* expression code: one int32 word per op, op << 24 | arg; a push spills the previous top */
enum {
  MMB_IR_OP_END = 0,
  MMB_IR_OP_CONST = 1,  /* push consts[arg] */
  MMB_IR_OP_VAL = 2,    /* push state[arg] */
  MMB_IR_OP_VALI = 3,   /* push state[arg + i] */
  MMB_IR_OP_VALG = 4,   /* push state[arg + (int)pool[w + i]], w = the next code word */
  MMB_IR_OP_DATA = 5,   /* push pool[arg + i] */
  MMB_IR_OP_DATAS = 6,  /* push pool[arg] */
  MMB_IR_OP_VALV = 7,   /* push state[arg + (int)state[w + i] - 1], w = the next code word: x[T] with T a
                           sampled discrete node (state slots w .. w + len - 1) whose support lies in 1..len(x) */
  MMB_IR_OP_DATAV = 8,  /* push pool[arg + (int)state[w + i] - 1], w = the next code word */
  MMB_IR_OP_ADD = 16, MMB_IR_OP_SUB = 17, MMB_IR_OP_MUL = 18, MMB_IR_OP_DIV = 19,
  MMB_IR_OP_NEG = 32, MMB_IR_OP_EXP = 33, MMB_IR_OP_LOG = 34, MMB_IR_OP_SQRT = 35,
  MMB_IR_OP_INVLOGIT = 36, MMB_IR_OP_LOGIT = 37, MMB_IR_OP_ABS = 38
};
#define MMB_IR_MAX_STACK 16
#define MMB_IR_MAX_TERMS 16
#define MMB_IR_MAX_VALUES 512
#define MMB_IR_MAX_RED 8        /* reductions per Gibbs block (ABI 10) */

typedef struct {
  int32_t family;    /* mmb_ir_family */
  int32_t fixed;     /* 1: values in the pool at `off` (not sampled) */
  int32_t off, len;  /* state slots (or pool offset) */
  int32_t expr[3];   /* code offsets of the distribution parameters (Distributions order), -1 none */
  int32_t cterm;     /* pool offset of a per-element constant (log binomial coefficient,
                        -lgamma(k+1)) or -1.  Sampled Binomial: a table of lchoose(n_i, k), k = 0..hi, per
                        element i, at cterm + i (hi + 1) + k (0 where k > n_i).  Categorical: the K probabilities,
                        or MMB_IR_CAT_STATE(off): they are state slots off .. off + K - 1 (a sampled Dirichlet
                        node).  Dirichlet: alpha[len], lmnB */
  double lo, hi;     /* Uniform bounds; sampled discrete nodes and Categorical / DiscreteUniform: the support */
} mmb_ir_node;

/* logpdf!(m, x, block, transform) terms (simulation.jl:77-90): params \ targets in block
 * order, then targets in topological order; trans = node is a block param (evaluated with
 * the block's transform) */
typedef struct {
  int32_t nterms;
  int32_t term[MMB_IR_MAX_TERMS];
  int32_t trans[MMB_IR_MAX_TERMS];
  /* ABI 10: a Gibbs block (a user Sampler(params, f) closure, src/samplers/sampler.jl:20-24, in the
   * style of doc/tutorial/line.jl:27-45 and INTEGRATION.md §3) whose closure returns
   * rand(Family(p0, p1)) of one scalar node, traced like the node functions:
   *   gibbs_family  MMB_IR_NORMAL    value = p0 + p1 * z         (rand(Normal(mu, sigma)))
   *                 MMB_IR_INVGAMMA  value = p1 / G, G ~ Gamma(p0) (rand(InverseGamma(shape, scale)))
   *                 MMB_IR_GAMMA     value = p1 * G, G ~ Gamma(p0) (rand(Gamma(shape, scale)))
   *                 0: not a Gibbs block
   *   gibbs_expr    p0, p1: scalar expressions (evaluated at element 0)
   *   nred          reductions evaluated before them: red_expr[r] summed over elements
   *                 0 .. red_len[r] - 1 (sum(x), sumabs2(x) in the closure); the parameter
   *                 expressions read reduction r as value slot nvalues + r (MMB_IR_OP_VAL)
   * Draws: z is normal #0 of the block's MMB_SUB_NORMAL stream, G Marsaglia-Tsang on its
   * MMB_SUB_GAMMA_N / MMB_SUB_GAMMA_U streams (mmb_math.h), as the hand-lowered Gibbs blocks. */
  int32_t gibbs_family;
  int32_t gibbs_expr[2];
  int32_t nred;
  int32_t red_expr[MMB_IR_MAX_RED];
  int32_t red_len[MMB_IR_MAX_RED];
} mmb_ir_block;

typedef struct {
  int32_t nvalues;              /* P */
  int32_t nnodes;
  const mmb_ir_node* nodes;
  int32_t ncode;
  const int32_t* code;
  int32_t nconst;
  const double* consts;
  int64_t npool;
  const double* pool;           /* data, fixed node values, gather indices (0-based), cterms */
  int32_t nmon;
  const int32_t* mon;           /* monitored node ids in Chains order, each contributing len values */
  int32_t stack;                /* max expression stack depth (<= MMB_IR_MAX_STACK) */
  mmb_ir_block blocks[MMB_MAX_BLOCKS];  /* one per sampling block of the spec */
} mmb_ir_model;

/* Arguments of one mcmc window (mcmc.jl:36-83). */
typedef struct {
  int64_t iters;        /* window = iter+1 : iter+iters  (mcmc_master! `window`) */
  int64_t burnin;       /* keep iteration i iff i > burnin && (i-burnin) % thin == 0 (mcmc.jl:76) */
  int64_t thin;
  int64_t model_burnin; /* Model.burnin: gate for adapt=:burnin (amwg.jl:55) and NUTS (nuts.jl:52) */
  double* draws;        /* host out, Mamba Chains order n_kept x p_mon x K (iteration fastest) or NULL */
  int32_t keep_device;  /* nonzero: keep this window's draws on the device (mmb_get_draws / GR) */
  int32_t time_kernels; /* nonzero: bracket each kernel launch with HIP events (mmb_kernel_time) */
} mmb_run_args;

typedef struct mmb_engine mmb_engine;

/* Engine lifetime ---------------------------------------------------------------- */
int mmb_abi_version(void);
int mmb_create(const mmb_model_spec* spec, int device, mmb_engine** out);
/* Node-IR model (spec->model == MMB_MODEL_IR): the IR is copied and validated (every code
 * word, slot and pool range against the node lengths) before anything touches the device.
 * Replaces the same fan-out as mmb_create for any Model lowered to the IR. */
int mmb_create_ir(const mmb_model_spec* spec, const mmb_ir_model* ir, int device, mmb_engine** out);
void mmb_destroy(mmb_engine* e);
const char* mmb_last_error(const mmb_engine* e); /* e may be NULL: last global error */

/* setinputs! (initialization.jl:30-40): named data arrays.
 * line: "x"(5), "y"(5); rats: "y"(150, rat-major), "x"(5); logistic: "X"(N*p row-major), "y"(N) */
int mmb_set_data(mmb_engine* e, const char* name, const double* x, int64_t n);

/* setinits! (initialization.jl:20-28): K chains, `init` is K x P row-major (chain-major),
 * P = mmb_num_values(); global chain ids are chain_offset .. chain_offset+K-1 (they key the
 * Philox streams, so a chain's trajectory does not depend on how chains are sharded). */
int mmb_num_values(const mmb_engine* e);
int mmb_num_monitored(const mmb_engine* e);
/* K, the engine's chain count after mmb_init_chains (0 before): the length of every per-chain
 * table the engine hands out (mmb_chain_order).  ABI 10. */
int64_t mmb_num_chains(const mmb_engine* e);
int mmb_init_chains(mmb_engine* e, const double* init, int64_t K, int64_t chain_offset, uint64_t seed);

/* mcmc_worker! loop for all chains of this engine (mcmc.jl:62-83). */
int mmb_run(mmb_engine* e, const mmb_run_args* args);
int64_t mmb_iter(const mmb_engine* e);              /* Model.iter after the last window */
/* Restore Model.iter when resuming from a checkpoint (read(name, ModelChains) followed by
 * mcmc(mc, iters), fileio.jl:3-11 + mcmc.jl:3-16).  Philox streams are keyed by
 * (seed, global chain id, iteration), so values + tune + iter + seed reproduce the
 * uninterrupted trajectory exactly.  Call after mmb_init_chains; iter >= 0. */
int mmb_set_iter(mmb_engine* e, int64_t iter);

/* ModelState / gettune / settune! (mcmc.jl:56,82; simulation.jl:3-28):
 * values: K x P row-major.  tune: K x mmb_tune_len() doubles in the canonical layout
 * (DESIGN.md §tune layout; ints stored exactly as doubles). */
int mmb_get_values(mmb_engine* e, double* values);
int mmb_set_values(mmb_engine* e, const double* values);
int64_t mmb_tune_len(const mmb_engine* e);
int mmb_get_tune(mmb_engine* e, double* tune);
int mmb_set_tune(mmb_engine* e, const double* tune);

/* Draws of the last window kept on device (keep_device=1), host copy in Mamba order. */
int64_t mmb_num_kept(const mmb_engine* e);
int mmb_get_draws(mmb_engine* e, double* draws);
/* Allocate the device draw buffer for windows keeping up to nkept iterations now, so a
 * later mmb_run does not allocate inside a timed or latency-sensitive window (mmb_run grows
 * the buffer itself when a window needs more).  nkept >= 0. */
int mmb_reserve_draws(mmb_engine* e, int64_t nkept);

/* Gelman-Rubin sufficient statistics of the device-kept draws (gelmandiag.jl:3-60).
 * mmb_gr_range: per monitored param [min, max] over local chains/draws (for link()).
 * mmb_gr_partials: per-chain mean/covariance reduced over local chains, after optional
 * log/logit link (link_kind per param: 0 none, 1 log, 2 logit) and shift `shift[p]`;
 * out has mmb_gr_len() doubles: these are summed across GPUs (RCCL all-reduce).
 * mmb_gr_partials and mmb_gr_allreduce serve at most 64 monitored values; a model that
 * monitors more gets MMB_E_UNSUPPORTED (mmb_gr_range has no such limit). */
int mmb_gr_range(mmb_engine* e, double* minmax /* 2*p */);
int64_t mmb_gr_len(const mmb_engine* e);
int mmb_gr_partials(mmb_engine* e, const int32_t* link_kind, const double* shift, double* out);

/* The one cross-GPU exchange (gelmandiag.jl:11-25), over RCCL/xGMI, inside the
 * library so a ccall caller reaches it (SURVEY §8b mmb_gr_allreduce).  Chains never interact
 * while sampling (mcmc.jl:48-52), so this is the only collective.
 * A communicator spans the engines (one per GPU) of every participating process:
 *   one process driving all GPUs (Julia threads / async streams):
 *       mmb_comm_init(engines, ngpu, ngpu, 0, NULL, &c)          -> ncclCommInitAll
 *   one process per GPU (torchrun-style, or Julia workers):
 *       rank 0: mmb_comm_id(id); the caller broadcasts the MMB_COMM_ID_BYTES bytes;
 *       every process: mmb_comm_init(&e, 1, nranks, rank, id, &c) -> ncclCommInitRank
 *   (nlocal engines of one process take ranks rank0 .. rank0+nlocal-1 of nranks).
 * mmb_range_allreduce: global [min, max] per monitored param (one MAX all-reduce of
 *   (-min, max)), for link() (chains.jl:237-246) and the shift.
 * mmb_gr_allreduce: mmb_gr_partials of every local engine (same link/shift on every rank),
 *   summed over all ranks by one SUM all-reduce of mmb_gr_len doubles; out = global sums,
 *   from which the host evaluates the PSRF as gelmandiag.jl:26-60 (mamba.jl_amd/gelman.py
 *   psrf_from_sums).  Every rank must call each collective (RCCL semantics).
 * Errors are reported through mmb_last_error(engines[0]). */
#define MMB_COMM_ID_BYTES 128
typedef struct mmb_comm mmb_comm;
int mmb_comm_id(uint8_t* id /* MMB_COMM_ID_BYTES */);
int mmb_comm_init(mmb_engine** engines, int nlocal, int nranks, int rank0, const uint8_t* id, mmb_comm** out);
int mmb_range_allreduce(mmb_comm* c, double* minmax /* 2*p: [min, max] per param */);
int mmb_gr_allreduce(mmb_comm* c, const int32_t* link_kind, const double* shift, double* out);
void mmb_comm_destroy(mmb_comm* c);

/* Posterior summaries of the device-kept draws, pooled over chains.
 * mmb_chain_summary replaces the per-element work of summarystats(c; etype=:bm)
 * (/root/reference/src/output/stats.jl:85-94) and mcse_bm (src/output/mcse.jl:10-19):
 * per local chain k and monitored param j, out[(k*p + j)*MMB_SUMMARY_FIELDS + f] =
 *   [sum x', sum x'^2, sum d_b, sum d_b^2, #full batches, head sum, head count,
 *    tail sum, tail count, 0]    with x' = x - shift[j],
 * where batches are runs of `batch_size` consecutive elements of vec(x) (chains
 * concatenated; local chain k sits at position chain_base + k: the global chain id for a
 * pooled multi-GPU summary, k for this engine alone), d_b = batch mean - shift[j] for the batches lying
 * wholly in the chain, and head/tail are the chain's pieces of batches shared with the
 * previous/next chain (joined by the host, across GPUs too).
 * mmb_order_hist: one radix-select pass for quantile(c) (stats.jl:73-80): for each of
 * `ntargets` key prefixes (order-preserving uint64 key of the double, bits above digit
 * 56-8*pass), counts[t*256 + d] = #draws of `param` whose key matches prefix t and whose
 * digit is d. */
#define MMB_SUMMARY_FIELDS 10
#define MMB_ORDER_MAX_TARGETS 16
int mmb_chain_summary(mmb_engine* e, const double* shift /* p */, int64_t batch_size, int64_t chain_base,
                      double* out /* K x p x MMB_SUMMARY_FIELDS */);
int mmb_order_hist(mmb_engine* e, int param, int ntargets, const uint64_t* prefix, int pass,
                   uint64_t* counts /* ntargets x 256 */);

/* Highest-posterior-density interval of one monitored param, pooled over chains: hpd(x; alpha)
 * (src/output/stats.jl:54-74) sorts the N pooled draws, takes a = y[1:m] and
 * b = y[N-m+1:N], m = max(1, ceil(alpha N)), and returns [a[i], b[i]] at the first minimum of b - a.
 * Only the m smallest and the m largest values are looked at, so the device sorts those alone
 * (hpd.hip).  The caller selects the thresholds lo = y[m-1], hi = y[N-m] (0-based) with
 * mmb_order_hist, then:
 * mmb_hpd_collect (stats.jl:54-74, the tails of y = sort(x)): one pass over the kept draws of
 *   `param` appends the values strictly below lo to the engine's "below" buffer and those
 *   strictly above hi to its "above" buffer, in the order of the radix select's key (which puts
 *   -0.0 below +0.0), unsorted.  counts = the two numbers found.  Nothing is written past `cap`
 *   elements of either buffer (the buffers grow to cap on demand; a correct call passes m - 1); a
 *   count above cap is MMB_E_ARG and leaves the engine without tails.
 * mmb_hpd_get_tails (stats.jl:54-74): copies the first nbelow / nabove elements of the two
 *   buffers out, for the all-gather of a sharded summary; the counts are the caller's, as
 *   mmb_hpd_collect returned them, and at most the buffers' capacity (elements past the last
 *   collect's counts hold whatever earlier calls left there).  Sorted once mmb_hpd_gap ran.
 * mmb_hpd_set_tails (stats.jl:54-74): the inverse: uploads tails (the pooled ones of every rank)
 *   as the engine's tails, in any order.
 * mmb_hpd_gap (stats.jl:58-63): sorts both tails ascending on the device (LSD radix sort on the
 *   64-bit key), then takes the first minimum of d[i] = b[i] - a[i], i < m, over the virtual arrays
 *   a = sorted below, then copies of lo;  b = copies of hi, then sorted above (each m long; the
 *   copies are never stored).  out = [a[i], b[i]], *index = i (0-based).  `total` is N, the pooled
 *   number of draws: 1 <= m <= total, both counts <= m - 1, and lo <= hi unless the tails overlap
 *   (2m > total); else MMB_E_ARG.  Needs tails (mmb_hpd_collect or mmb_hpd_set_tails): else
 *   MMB_E_STATE.
 * NaN draws: the key puts them at the extremes; the interval is then unspecified. */
int mmb_hpd_collect(mmb_engine* e, int param, double lo, double hi, int64_t cap, int64_t counts[2]);
int mmb_hpd_get_tails(mmb_engine* e, double* below, int64_t nbelow, double* above, int64_t nabove);
int mmb_hpd_set_tails(mmb_engine* e, const double* below, int64_t nbelow, const double* above, int64_t nabove);
int mmb_hpd_gap(mmb_engine* e, int64_t m, int64_t total, double lo, double hi, double out[2], int64_t* index);

/* Model log densities of the device-kept draws (modelstats.hip): logpdf(mc, nodekeys) and the pieces of
 * dic(mc) (/root/reference/src/output/modelstats.jl:3-68).  `nodes` lists 1 <= nnodes <= MMB_IR_MAX_TERMS
 * Stochastic node ids of the model (line: MMB_LINE_BETA / _S2 / _Y; node IR: indices of mmb_ir_model.nodes;
 * a Logical or an id out of range is MMB_E_ARG).  For kept row i and local chain k,
 *   lp[i,k] = sum over the list, in list order, of logpdf(node) with the node's parameters evaluated on
 *   that draw's values (mapreduce(+), modelstats.jl:63: no early exit; sampled nodes untransformed),
 * each term by the sweep kernel's own node log density (support -> -Inf, per-element constants, lane
 * partials in element order and the group sum), so it has the bits the sampler computes for that state.
 * Node IR: every sampled node that a requested node's parameter expressions read (getsimkeys,
 * modelstats.jl:107-132; Logicals are inlined, so a monitored Logical is recomputed from its parents, not
 * relisted from the chain), and a requested node that is itself sampled, must be monitored: else MMB_E_ARG,
 * the message naming the first missing node id.  Hand-lowered rats (3 of 65 values monitored) and
 * logistic: MMB_E_UNSUPPORTED.  Without device-kept draws: MMB_E_STATE.  All validation precedes any
 * launch; none of these calls touches chain state, tune, iteration counter, draws, hpd tails or chain order.
 * mmb_draws_logpdf (modelstats.jl:30-68): out[i + nkept*k], the value array of the n x 1 x K Chains.
 * mmb_draws_deviance (modelstats.jl:7-8): per local chain k, with D = -2 lp,
 *   out[2k] = sum_i (D[i,k] - shift), out[2k+1] = sum_i (D[i,k] - shift)^2, in row order; the n x K values
 *   stay on the device.  Non-finite values propagate.  Additive across chains and GPUs for a common shift.
 * mmb_logpdf_at (modelstats.jl:15-25): the same sum at one point x (pmon values in monitored-column
 *   order, e.g. the posterior means), by the same kernel on a one-row, one-chain buffer. */
int mmb_draws_logpdf(mmb_engine* e, int nnodes, const int32_t* nodes,
                     double* out /* nkept x K, Chains order: out[i + nkept*k] */);
int mmb_draws_deviance(mmb_engine* e, int nnodes, const int32_t* nodes, double shift, double* out /* K x 2 */);
int mmb_logpdf_at(mmb_engine* e, int nnodes, const int32_t* nodes,
                  const double* x /* pmon, one point in monitored-column order */, double* lp);

/* Posterior predictive draws of the observed nodes on the device-kept draws (predict.hip):
 * predict(mc, nodekeys) (src/output/modelstats.jl:71-102).  `nodes` lists 1 <= nnodes <= MMB_IR_MAX_TERMS
 * observed (fixed) Stochastic node ids (line: MMB_LINE_Y only; node IR: indices of mmb_ir_model.nodes);
 * P is the summed length of the listed nodes, column j counting their elements in list order.  For kept
 * row i and local chain k the value of column j is one variate of the node's distribution, its parameters
 * evaluated on that draw as mmb_draws_logpdf evaluates them, and it is a pure function of (seed,
 * chain_offset + k, iteration start + i*thin, node id n, element e): it does not depend on sharding, row
 * chunking, tile size or call order.  Philox counter and key as everywhere (mmb_math.h): key = seed,
 * ctr.w = global chain id, ctr.z = (uint32)(start + i*thin), ctr.y = block*16 + substream, with blocks no
 * sampler uses (those are < 8): the node block PB(n) = 256 + n and, for the gamma-based families, the
 * element block GB(n, e) = (n + 1)*65536 + e (n < 4095 and 2*len <= 65536, else MMB_E_UNSUPPORTED).
 *   Normal, IsoNormal  a + b z, z = normal #e of (PB, MMB_SUB_NORMAL)
 *   Bernoulli          u < p ? 1 : 0, u = uniform #e of (PB, MMB_SUB_UNIFORM); Exponential(t) -t log1p(-u);
 *   Uniform(lo, hi)    lo + (hi - lo) u
 *   Binomial(n, p)     trials in ceil(n/512) chunks of at most 512, chunk c with uniform #(c*len + e), each
 *                      by sequential-search inversion on min(p, 1 - p) (mirrored for p > 1/2), summed;
 *                      n an integer in [0, 2^20], else NaN
 *   Poisson(lambda)    max(1, ceil(lambda/256)) equal pieces, piece c with uniform #(c*len + e), each by
 *                      sequential-search inversion (at most 4096 steps), summed; more than 64 pieces: NaN
 *   Gamma(k, t) t G(k), InverseGamma(a, b) b / G(a), Beta(a, b) G1/(G1 + G2) with G1 = G(a) on GB(n, e) and
 *                      G2 = G(b) on GB(n, len + e); G = mmb_gamma_any on MMB_SUB_GAMMA_N / _U from index 0
 * A parameter that is not finite or outside the family's domain (sigma < 0, p outside [0, 1], lambda < 0,
 * shape or scale <= 0, hi < lo) gives NaN for that element and draws nothing: every loop ends on any draws.
 * Validation as mmb_draws_logpdf's (unmonitored parent: MMB_E_ARG naming the node id; hand-lowered rats
 * and logistic: MMB_E_UNSUPPORTED; no device-kept draws: MMB_E_STATE), and: a listed node that is not
 * observed is MMB_E_ARG; thin >= 1, start >= 0, 0 <= i0 < i1 <= mmb_num_kept, else MMB_E_ARG; a result tile
 * of 8 chains that does not fit the LDS beside the state images is MMB_E_UNSUPPORTED.  All of it precedes any
 * launch; none of these calls touches chain state, tune, iteration counter, draws, hpd tails or chain order.
 * mmb_draws_predict: rows [i0, i1) of the kept draws, out[(i - i0) + (i1 - i0)*(j + P*k)]; row i always has
 *   iteration start + i*thin (i the kept-row index), so a window equals the same rows of the full call.
 * mmb_draws_predict_moments: over all kept rows, out[(k*P + j)*2] = sum_i (yhat - shift[j]) and
 *   out[(k*P + j)*2 + 1] = sum_i (yhat - shift[j])^2 in row order; the values stay on the device.
 *   Non-finite values propagate.  Additive across chains and GPUs for a common shift.
 * mmb_predict_width: P of a node list (after the same validation). */
int mmb_draws_predict(mmb_engine* e, int nnodes, const int32_t* nodes, uint64_t seed, int64_t start, int64_t thin,
                      int64_t i0, int64_t i1, double* out /* (i1-i0) x P x K, Chains order */);
int mmb_draws_predict_moments(mmb_engine* e, int nnodes, const int32_t* nodes, uint64_t seed, int64_t start,
                              int64_t thin, const double* shift /* P */, double* out /* K x P x 2 */);
int mmb_predict_width(mmb_engine* e, int nnodes, const int32_t* nodes, int64_t* P);

/* Upload draws: the inverse of mmb_get_draws. `draws` is nkept x p x K column-major (the
 * Chains value layout, iteration fastest); it is transposed into the device draw buffer, which
 * grows by mmb_reserve_draws' rule, and becomes the engine's kept window (mmb_num_kept ==
 * nkept), so every device summary runs on it: a Chains read back from a file, or a series chosen
 * by a test.  Needs mmb_init_chains and nkept >= 1. */
int mmb_set_draws(mmb_engine* e, const double* draws, int64_t nkept);

/* Per-chain convergence diagnostics of the device-kept draws (diag.hip): the per-element work of
 * autocor / changerate (/root/reference/src/output/stats.jl:3-39), gewekediag
 * (src/output/gewekediag.jl) and mcse (src/output/mcse.jl:3-46), per local chain k and monitored
 * param j.  Windows are 0-based half-open ranges [i0, i1) of the kept draws, 0 <= i0 < i1 <=
 * mmb_num_kept, n_w = i1 - i0; outputs are C row-major.  The window mean is taken on x - x[i0] and
 * every sum of products on z = x - mean, so a series of equal elements gives gamma(l) = 0
 * exactly (mcse 0; autocorrelation and Geweke z then 0/0 = NaN, as in the reference).
 * mmb_chain_autocov: out[(k*p + j)*(2 + nlags) + f] = [mean, gamma(0), gamma(lags[0]), ...] with
 *   gamma(l) = sum_t z_t z_{t+l} / n_w (StatsBase autocov(x, lags; demean=true)), all lags in
 *   one sweep.  0 <= nlags <= MMB_DIAG_MAX_LAGS, each lag in 1 .. n_w - 1 (else MMB_E_ARG, "lags
 *   must be less than the sample length").
 * mmb_chain_mcse: out[(k*p + j)*MMB_MCSE_FIELDS + f] = [mean, gamma(0), mcse, terms].
 *   MMB_MCSE_IMSE / MMB_MCSE_IPSE follow mcse_imse / mcse_ipse (mcse.jl:21-46) statement for
 *   statement on the window's series (m = div(n_w - 2, 2), the running min of IMSE, Ghat > 0 ||
 *   break; n_w >= 2); terms = lag pairs added in the loop.  MMB_MCSE_BM is mcse_bm(x;
 *   size=batch_size) of the window alone (batches start at i0, the remainder is dropped;
 *   n_w < 2*batch_size is MMB_E_ARG with the reference's message); terms = batches.
 *   batch_size is ignored by the other two.
 *   The one departure from the reference: where `value` is negative its sqrt throws a
 *   DomainError; a kernel over thousands of chains cannot throw for one of them and writes NaN
 *   for that (chain, param).
 * mmb_change_counts: out[j], j < p = the number of (local chain, i >= 1) with x[i] != x[i-1] for
 *   param j over all kept draws; out[p] = the number with any param changed (stats.jl:19-39).
 *   Exact integer counts, additive across GPUs. */
#define MMB_DIAG_MAX_LAGS 16
#define MMB_MCSE_FIELDS 4
#define MMB_MCSE_BM 0
#define MMB_MCSE_IMSE 1
#define MMB_MCSE_IPSE 2
int mmb_chain_autocov(mmb_engine* e, int64_t i0, int64_t i1, int nlags, const int64_t* lags,
                      double* out /* K x p x (2 + nlags) */);
int mmb_chain_mcse(mmb_engine* e, int64_t i0, int64_t i1, int etype, int64_t batch_size,
                   double* out /* K x p x MMB_MCSE_FIELDS */);
int mmb_change_counts(mmb_engine* e, int64_t* out /* p + 1 */);

/* Partials of the two remaining per-chain convergence diagnostics, heideldiag
 * (src/output/heideldiag.jl:3-27) and rafterydiag (src/output/rafterydiag.jl:3-47), on
 * the device-kept draws: per local chain k and monitored param j, n = mmb_num_kept, C row-major.
 * The closing formulas are the host's (mamba.jl_amd/diag.py).
 * mmb_chain_cvm: the Cramer-von Mises sums of heideldiag.jl:11-16 on the suffix windows [s, n) of
 *   `nstarts` 0-based, strictly increasing starts, 1 <= nstarts <= MMB_HEIDEL_MAX_STARTS, 0 <= s < n
 *   (else MMB_E_ARG): out[((k*p + j)*nstarts + q)*2 + f] = [mean_s, W_s] with mean_s the window
 *   mean (x[s_0] + the index-order sum of x - x[s_0], over m = n - s) and
 *   W_s = (sum_{t=1..m} B_t^2) / m^2,  B_t = sum_{u<=t} (x_{s+u-1} - mean_s):
 *   `sum(Bsq) / m` of heideldiag.jl:15-16 without its 1 / S0.  B is accumulated on the centred
 *   values, so a series of equal elements gives W = 0 exactly.  All starts are served by one pair
 *   of sweeps over the rows.
 * mmb_chain_mcse_from: mmb_chain_mcse with a window start per (chain, param), i0[k*p + j], and the
 *   common end i1 (the halfwidth of heideldiag.jl:24 on each series' chosen window).  Every
 *   element is validated as mmb_chain_mcse validates its window; the message names the first
 *   offending (chain, param).  Equal starts give mmb_chain_mcse's output bit for bit.
 * mmb_chain_raftery: 0 < q < 1, 3 <= n < 2^31.  out[(k*p + j)*MMB_RAFTERY_FIELDS + f] =
 *   [threshold, kthin, ntest, n00, n10, n01, n11, bic].  threshold is Julia 0.5 quantile(x, q)
 *   (rafterydiag.jl:13): index = 1 + (n-1)q, lo = floor, hi = ceil, h = index - lo, the value a if
 *   index == lo, else (1-h)*a + h*b (rounded products, then their sum) with a, b the exact order
 *   statistics of rank lo-1 and hi-1.  kthin, ntest and bic are those at which the loop of
 *   rafterydiag.jl:17-33 on dichot = x <= threshold stops (the first bic < 0); n_ab counts
 *   test_t = a, test_{t+1} = b in that thinned series: [n00, n10, n01, n11] = tranfinal[1..4]
 *   of rafterydiag.jl:34.  Counts are exact integers.
 *   A second departure, next to the NaN-for-DomainError one above: a series for which ntest falls
 *   below 3 before bic turns negative ends the reference in a DomainError from log(-1); here it
 *   gets kthin = NaN, bic = NaN and zero counts (ntest is the length that was too short). */
#define MMB_HEIDEL_MAX_STARTS 16
#define MMB_RAFTERY_FIELDS 8
int mmb_chain_cvm(mmb_engine* e, int nstarts, const int64_t* starts, double* out /* K x p x nstarts x 2 */);
int mmb_chain_mcse_from(mmb_engine* e, const int64_t* i0 /* K x p */, int64_t i1, int etype, int64_t batch_size,
                        double* out /* K x p x MMB_MCSE_FIELDS */);
int mmb_chain_raftery(mmb_engine* e, double q, double* out /* K x p x MMB_RAFTERY_FIELDS */);

/* Timing / sync (bench.py roofline) */
int mmb_sync(mmb_engine* e);
/* Device time of the last mmb_run window's kernel launches (time_kernels nonzero).  A sweep window
 * may run as chain parts on streams of their own, whose launches overlap (MMB_SWEEP_PARTS):
 * total_ms is the time during which at least one sweep launch of the window was in flight -- the
 * union of the launches' [start, end] intervals, not their sum -- so it never exceeds the window's
 * wall time; with one part that is the sum as before.  launches counts every part's launches;
 * units (chain-updates) does not depend on the parts.  (Logistic windows: the summed
 * gradient-kernel time of their parts.) */
int mmb_kernel_time(const mmb_engine* e, double* total_ms, int64_t* launches, int64_t* units);
int mmb_state_bytes(const mmb_engine* e, double* bytes_per_chain_update);
/* Gradient evaluations (logpdf!+gradlogpdf! calls, sampler.jl:97-119) in the last mmb_run,
 * summed over chains; counted on device by the batched-gradient (logistic) engine, 0 else. */
int mmb_grad_evals(mmb_engine* e, int64_t* n);
/* NUTS tree statistics since mmb_init_chains, all NUTS blocks and chains: out[0] = completed
 * updates, out[1] = updates stopped by the depth cap MMB_NUTS_MAX_DEPTH (30: 2^30 leapfrogs
 * in one update, beyond any run that finishes) while the
 * reference's unbounded doubling loop (nuts.jl:106-125) would have continued, out[2] = sum of
 * final tree depths j.  out[1] == 0 means the cap never changed a draw. */
int mmb_nuts_stats(mmb_engine* e, int64_t out[3]);
/* Node-IR kernel specialisation.  mmb_create_ir writes the lowered model as
 * HIP source -- node log densities (dependent.jl:207-213 -> distributionstruct.jl:136-168) and
 * block logpdf! term lists (simulation.jl:77-90) as straight-line code -- and compiles it with
 * hipRTC (code objects cached by source hash: MMB_JIT_CACHE, else <library dir>/jit), replacing
 * the per-op interpreter; the same operations in the same order, so results are bit-identical.
 * On any failure, or with MMB_IR_JIT=0, the interpreter kernel runs.
 * mmb_ir_jit_info: 1 if the engine runs the specialised kernel, 0 if the interpreter; `buf`
 * receives the reason / cache status.  mmb_ir_jit_prebuild: validate and compile into the cache
 * without a device (build step).  mmb_ir_jit_source_text: the generated source (returns its
 * length; copies up to n - 1 bytes). */
int mmb_ir_jit_info(const mmb_engine* e, char* buf, int64_t n);
int mmb_ir_jit_prebuild(const mmb_model_spec* spec, const mmb_ir_model* ir, char* info, int64_t n);
int mmb_ir_jit_source_text(const mmb_model_spec* spec, const mmb_ir_model* ir, char* buf, int64_t n);
/* AMM factorization statistics since mmb_init_chains, per sampling block b (zero rows for
 * non-AMM blocks), summed over the engine's chains: out[b*MMB_AMM_STATS + i] =
 *   i = 0  adaptive updates, i.e. cholfact(Hermitian(Sigma), Val{true}) calls (amm.jl:81-87)
 *   i = 1  of them with rank(F) == n, i.e. SigmaLm replaced (amm.jl:88-90)
 *   i = 2  sum of rank(F) (dpstf2's pivots taken before its ajj <= 0 stop)
 *   i = 3  sum of factorization steps the device executed for the update's chain group:
 *          min(rank + 1, n) per chain, the max over the two chains of a wavefront on the
 *          32-lane kernels (both chains step together), the chain's own count elsewhere
 *   i = 4  updates whose optimistic factorization pass was redone by the checked pass
 * Diagnostics only (the bench reports the full-rank fraction and mean steps of its timed
 * window); no draw depends on them. */
#define MMB_AMM_STATS 5
int mmb_amm_stats(mmb_engine* e, int64_t* out /* MMB_MAX_BLOCKS x MMB_AMM_STATS */);

/* AMWG path counter since init_chains: out[0] = block updates that ran amwg_sub! one coordinate
 * at a time (samplers.h amwg) instead of the lane-parallel decision of every coordinate, which
 * is taken when each coordinate's accept test is certain under the logpdf's rounding bound
 * (rats alpha / beta; the environment variable MMB_AMWG_EXACT=1 forces the sequential loop,
 * MMB_SLICE_EXACT=1 the one-candidate-at-a-time Slice shrink loop of the rats scalar blocks).
 * Both paths give the same draws; diagnostics only. */
int mmb_amwg_stats(mmb_engine* e, int64_t* out /* 1 */);

/* RWM counters since mmb_init_chains, per sampling block b (zero rows for the other blocks), summed
 * over the engine's chains: out[2 b] = block updates, out[2 b + 1] = accepted ones (rwm.jl:67-70).
 * A user sizes `scale` from this acceptance rate (RWM does not adapt).  BMG, BMC3 and BIA blocks fill
 * their rows the same way (a BMG block of one element has no accept step: every update counts as
 * accepted), and so do BHMC blocks, whose accepts are the updates that ran to traveltime (the others
 * stalled and changed nothing), and ABC blocks, whose accepts are the updates that took a
 * candidate.  Diagnostics only. */
int mmb_rwm_stats(mmb_engine* e, int64_t* out /* MMB_MAX_BLOCKS x 2 */);

/* The lane-group slot -> chain table the next window will run with (K entries; the identity
 * when no ordering applies).  The 32-lane sweep kernels (rats, node IR) pair chains whose
 * pivoted Cholesky stops alike in one wavefront; the table sorts the chains by their AMM blocks'
 * factor-valid flags (slow classes first; MMB_ORDER_MODE 0 ascending, 2 balanced workgroups),
 * computed on the device right after each window (and before one that follows a host write of
 * the tune state).  Results do not depend on it (every chain keeps its own state, draws column
 * and Philox id); diagnostics.  Writes mmb_num_chains(e) entries. */
int mmb_chain_order(mmb_engine* e, int32_t* slot_to_chain);

/* Diagnostics: the device's 32-lane pivoted Cholesky of the AMM update (cholfact(Hermitian(S),
 * :U, Val{true}) = LAPACK dpstf2 for n < 64, amm.jl:87) on n caller-supplied d x d matrices,
 * 1 <= d <= 30, packed lower triangle S[c][tri(i) + k] (i >= k, 480 doubles per matrix).  Out per
 * matrix: info[c] = {rank, redone} (redone: the optimistic pass was redone by the checked
 * one), pos[c][32] each element's pivot position (-1 past d) and, on full rank, L[c][480] the
 * factor in position form: element e's row at tri(pos[e]) + k, k = 0..pos[e].  Runs on `device`
 * outside any engine. */
int mmb_debug_pchol(int device, int64_t n, int d, const double* S, double* L, int32_t* pos, int32_t* info);

#ifdef __cplusplus
}
#endif
#endif /* MAMBA_HIP_H */
