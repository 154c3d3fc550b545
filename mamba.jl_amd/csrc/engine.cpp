// engine.cpp — host side of libmambahip.so: the C ABI of include/mamba_hip.h.
//
// mmb_run is mcmc_master!/mcmc_worker! (src/model/mcmc.jl:36-83) for every chain of
// this engine's shard: it launches the fused sweep kernel over windows of iterations
// on the engine's stream and copies the kept draws out in Mamba's Chains order.
#include "engine.h"

#include <cstdarg>
#include <type_traits>

thread_local std::string g_last_error;

int fail(mmb_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  if (e) e->err = buf;
  return code;
}

int node_dim(const mmb_model_spec& s, const mmb_ir_model* ir, int node, bool* positive) {
  bool pos = false;
  int d = -1;
  if (s.model == MMB_MODEL_IR) {
    // sampled nodes only: not fixed, not Logical; a discrete family only where a DGS block (or, a binary
    // node, a BMG, BMC3 or BIA block) samples it, a Dirichlet node only where a SliceSimplex block does
    // (ir_validate and create_impl check both)
    if (ir && node >= 0 && node < ir->nnodes) {
      const mmb_ir_node& n = ir->nodes[node];
      const bool ok = !n.fixed && ((n.family >= MMB_IR_NORMAL && n.family <= MMB_IR_BETA) || ir_dgs_family(n.family) ||
                                   n.family == MMB_IR_DIRICHLET);
      d = ok ? n.len : -1;
    }
  } else if (s.model == MMB_MODEL_LINE) {
    if (node == MMB_LINE_BETA) d = 2;
    else if (node == MMB_LINE_S2) { d = 1; pos = true; }
  } else if (s.model == MMB_MODEL_RATS) {
    static const int dims[7] = {1, 30, 1, 1, 30, 1, 1};
    static const int posv[7] = {1, 0, 0, 1, 0, 0, 1};
    if (node >= 0 && node < 7) { d = dims[node]; pos = posv[node]; }
  } else if (s.model == MMB_MODEL_LOGISTIC) {
    if (node == MMB_LOGISTIC_BETA) d = s.ncoef;
  }
  if (positive) *positive = pos;
  return d;
}

static int chol_lower(int d, const double* A, double* L) {  // A column-major
  for (int i = 0; i < d * d; ++i) L[i] = 0.0;
  for (int j = 0; j < d; ++j) {
    double s = A[j * d + j];
    for (int k = 0; k < j; ++k) s -= L[j * d + k] * L[j * d + k];
    if (!(s > 0.0)) return -1;
    double ljj = std::sqrt(s);
    L[j * d + j] = ljj;
    for (int i = j + 1; i < d; ++i) {
      double t = A[j * d + i];
      for (int k = 0; k < j; ++k) t -= L[i * d + k] * L[j * d + k];
      L[i * d + j] = t / ljj;
    }
  }
  return 0;
}

// C linkage comes from the extern "C" declarations in include/mamba_hip.h.

int mmb_abi_version(void) { return MMB_ABI_VERSION; }

const char* mmb_last_error(const mmb_engine* e) {
  if (e && !e->err.empty()) return e->err.c_str();
  return g_last_error.c_str();
}

// An ABC block's spec (mamba_hip.h MMB_SAMPLER_ABC) checked against the lowered model, and its device table
// [T, ns, nd, codes[ns], then per data node (node id, first statistic)] (samplers.h abc).  Returns the reason
// for a refusal, or null.
static const char* abc_family_name(int fam) {
  switch (fam) {
    case MMB_IR_GAMMA: return "Gamma";
    case MMB_IR_INVGAMMA: return "InverseGamma";
    case MMB_IR_BETA: return "Beta";
    case MMB_IR_CATEGORICAL: return "Categorical";
    case MMB_IR_DISCRETEUNIFORM: return "DiscreteUniform";
    case MMB_IR_DIRICHLET: return "Dirichlet";
    default: return "this family";
  }
}
static const char* abc_table(const mmb_block_spec& s, const mmb_ir_node* nodes, int nnodes, const mmb_ir_block& IB, int d,
                             std::vector<int32_t>& tab) {
  static thread_local char msg[160];
  const int prop = s.form & 0xff, kern = (s.form >> 8) & 0xff;
  if (s.form < 0 || (s.form >> 17) != 0 || prop > MMB_RWM_COSINE || kern > MMB_RWM_COSINE)
    return "ABC form is proposal | kernel << 8 | randeps << 16 with proposal and kernel in 0..6";
  if (!(s.beta >= 0.0 && s.beta <= 1.0)) return "decay is not in [0, 1]";
  if (!(std::isfinite(s.epsilon) && s.epsilon > 0.0)) return "epsilon is not finite and > 0";
  if (s.batchsize < 1 || s.batchsize > MMB_ABC_MAX_DRAW) return "maxdraw is not in 1..1024";
  if (s.nsteps < 1 || s.nsteps > MMB_ABC_MAX_NSIM) return "nsim is not in 1..8";
  if (s.transform != 1) return "ABC unlists its nodes with transform (transform = 1)";
  const int ns = s.ntuning - d;
  if (s.dim != d || ns < 1 || ns > MMB_ABC_MAX_SUMMARY || !s.tuning)
    return "ABC tuning is scale[dim] followed by 1..8 summary codes";
  for (int i = 0; i < d; ++i)
    if (!(std::isfinite(s.tuning[i]) && s.tuning[i] >= 0.0)) return "ABC scale must be finite and >= 0";
  bool var = false;
  for (int q = 0; q < ns; ++q) {
    const double cd = s.tuning[d + q];
    if (!(cd >= MMB_ABC_IDENTITY && cd <= MMB_ABC_MAXIMUM) || cd != std::floor(cd)) return "unknown summary code";
    if (cd == MMB_ABC_IDENTITY && ns != 1) return "the identity summary may only stand alone";
    var = var || cd == MMB_ABC_VAR || cd == MMB_ABC_STD;
  }
  for (int a = 0; a < s.nnodes; ++a)
    if (ir_dgs_family(nodes[s.nodes[a]].family) || nodes[s.nodes[a]].family == MMB_IR_POISSON)
      return "ABC samples continuous nodes";
  tab.assign(3 + ns, 0);
  for (int q = 0; q < ns; ++q) tab[3 + q] = (int32_t)s.tuning[d + q];
  const bool ident = tab[3] == MMB_ABC_IDENTITY;
  int T = 0, nd = 0;
  for (int t = 0; t < IB.nterms && t < MMB_IR_MAX_TERMS; ++t) {
    if (IB.trans[t]) continue;
    const int n = IB.term[t];
    if (n < 0 || n >= nnodes) return "ABC: a term of the block is not a node";
    const mmb_ir_node& N = nodes[n];
    if (!mmb_abc_data_family(N.family)) {
      snprintf(msg, sizeof msg, "ABC cannot simulate data node %d: %s data nodes are not supported", n,
               abc_family_name(N.family));
      return msg;
    }
    if (var && N.len < 2) return "the var and std summaries need data nodes of >= 2 elements";
    if (nd == MMB_ABC_MAX_DATA) return "ABC: at most 16 data nodes";
    tab.push_back(n);
    tab.push_back(T);
    T += ident ? N.len : ns;
    if (T > MMB_ABC_MAX_T) return "the total summary length is not in 1..32";
    ++nd;
  }
  if (nd < 1) return "ABC needs at least one data node among the block's targets";
  tab[0] = T;
  tab[1] = ns;
  tab[2] = nd;
  return nullptr;
}

int create_impl(const mmb_model_spec* spec, const mmb_ir_model* ir, int device, mmb_engine** out) {
  if (!spec || !out) return fail(nullptr, MMB_E_ARG, "null argument");
  *out = nullptr;
  if (spec->nblocks < 1 || spec->nblocks > MMB_MAX_BLOCKS)
    return fail(nullptr, MMB_E_ARG, "nblocks must be in 1..%d", MMB_MAX_BLOCKS);
  mmb_engine* e = new mmb_engine();
  e->spec = *spec;
  e->model = spec->model;
  if (e->model == MMB_MODEL_RATS) {
    e->P = 65; e->pmon = 3; e->VS = Mdl<MMB_MODEL_RATS>::VS;
    e->DP = Mdl<MMB_MODEL_RATS>::DP; e->TP = Mdl<MMB_MODEL_RATS>::TP;
  } else if (e->model == MMB_MODEL_LINE) {
    e->P = 3; e->pmon = 3; e->VS = Mdl<MMB_MODEL_LINE>::VS;
    e->DP = Mdl<MMB_MODEL_LINE>::DP; e->TP = Mdl<MMB_MODEL_LINE>::TP;
  } else if (e->model == MMB_MODEL_IR) {
    if (!ir) {
      delete e;
      return fail(nullptr, MMB_E_ARG, "node-IR models are created with mmb_create_ir");
    }
    e->P = ir->nvalues;
    e->pmon = 0;
    for (int q = 0; q < ir->nmon; ++q) e->pmon += ir->nodes[ir->mon[q]].len;
    e->VS = (ir_state_len(spec, ir) + 7) / 8 * 8;  // + the Gibbs blocks' reduction slots; 64-byte rows
    e->DP = Mdl<MMB_MODEL_IR>::DP; e->TP = Mdl<MMB_MODEL_IR>::TP;
    e->ir_nodes.assign(ir->nodes, ir->nodes + ir->nnodes);
    e->ir_code.assign(ir->code, ir->code + ir->ncode);
    e->ir_const.assign(ir->consts, ir->consts + ir->nconst);
    e->ir_pool.assign(ir->pool, ir->pool + ir->npool);
    e->ir_mon.assign(ir->mon, ir->mon + ir->nmon);
    e->ir_blocks.assign(ir->blocks, ir->blocks + spec->nblocks);
    e->ir_stack = ir->stack;
    e->have_data = true;  // the pool carries the data
  } else if (e->model == MMB_MODEL_LOGISTIC) {
    if (spec->ncoef < 1 || spec->ncoef > MMB_LG_DV || spec->nobs < 1 || !(spec->prior_sd > 0.0)) {
      delete e;
      return fail(nullptr, MMB_E_ARG, "logistic: need 1 <= ncoef <= %d, nobs >= 1, prior_sd > 0", MMB_LG_DV);
    }
    const int k0 = spec->blocks[0].sampler;
    if (spec->nblocks != 1 || !(k0 == MMB_SAMPLER_NUTS || k0 == MMB_SAMPLER_HMC || k0 == MMB_SAMPLER_MALA)) {
      delete e;
      return fail(nullptr, MMB_E_UNSUPPORTED,
                  "logistic: only the [NUTS(:beta)], [HMC(:beta, ...)] and [MALA(:beta, ...)] schemes are lowered");
    }
    e->P = spec->ncoef; e->pmon = spec->ncoef; e->VS = MMB_LG_DV; e->DP = MMB_LG_DV; e->TP = 0;
    e->lg_N = spec->nobs; e->lg_p = spec->ncoef; e->lg_rps = mmb_lg_rps(spec->nobs);
  } else {
    delete e;
    return fail(nullptr, MMB_E_UNSUPPORTED, "unknown model kind %d", spec->model);
  }
  for (int b = 0; b < spec->nblocks; ++b) {
    const mmb_block_spec& s = spec->blocks[b];
    BlockHost h;
    h.spec = s;
    if (s.nnodes < 1 || s.nnodes > MMB_MAX_NODES_PER_BLOCK) {
      delete e;
      return fail(nullptr, MMB_E_ARG, "block %d: bad node count", b);
    }
    int d = 0, nvec = 0;
    for (int a = 0; a < s.nnodes; ++a) {
      for (int a2 = 0; a2 < a; ++a2)
        if (s.nodes[a2] == s.nodes[a]) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: repeated node", b);
        }
      int nd = node_dim(*spec, ir, s.nodes[a], nullptr);
      if (nd < 0) {
        delete e;
        return fail(nullptr, MMB_E_ARG, "block %d: node id %d invalid for model", b, s.nodes[a]);
      }
      if (nd > 1) nvec++;
      d += nd;
    }
    if (s.dim != 0 && s.dim != d) {
      delete e;
      return fail(nullptr, MMB_E_ARG, "block %d: dim %d != unlisted length %d", b, s.dim, d);
    }
    h.d = d;
    h.T = tri(d);
    // (a DGS block never unlists its node into lanes: it visits the elements one by one)
    if (e->model == MMB_MODEL_IR && d > Mdl<MMB_MODEL_IR>::DMAX && s.sampler != MMB_SAMPLER_DGS) {
      delete e;
      return fail(nullptr, MMB_E_UNSUPPORTED, "node IR: block %d has %d elements (max %d)", b, d,
                  Mdl<MMB_MODEL_IR>::DMAX);
    }
    if (e->model == MMB_MODEL_RATS && nvec > 0 && (s.nnodes != 1)) {
      delete e;
      return fail(nullptr, MMB_E_UNSUPPORTED, "rats: alpha/beta must form their own block");
    }
    if (s.ntuning > 0) h.tuning.assign(s.tuning, s.tuning + s.ntuning);
    // logpdfgrad! scheme of gradient samplers (mmb_gradient): forward differences where the
    // model supports them (line, node IR), the analytic gradient on line and logistic
    if (s.sampler == MMB_SAMPLER_NUTS || s.sampler == MMB_SAMPLER_HMC || s.sampler == MMB_SAMPLER_MALA) {
      const int gr = s.gradient;
      // logistic: the reference's default dtype=:forward (Calculus forward differences,
      // simulation.jl:47-51) runs as p + 1 log-density columns per request through the batched
      // MFMA kernel (logistic.hip lg_grad_kernel<.., LPONLY>, lg_assemble_fd)
      if (e->model == MMB_MODEL_LOGISTIC) e->lg_fd = gr == MMB_GRAD_FORWARD;
      const bool ok = gr == MMB_GRAD_DEFAULT || gr == MMB_GRAD_FORWARD ||
                      (gr == MMB_GRAD_ANALYTIC && e->model != MMB_MODEL_IR);
      if (!ok) {
        delete e;
        return fail(nullptr, MMB_E_ARG, "block %d: gradient %d is not available for this model", b, gr);
      }
    }
    switch (s.sampler) {
      case MMB_SAMPLER_AMWG:
        if (!(s.ntuning == 1 || s.ntuning == d)) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "length(sigma) differs from variate length %d", d);
        }
        if (s.batchsize <= 0) { delete e; return fail(nullptr, MMB_E_ARG, "batchsize must be positive"); }
        break;
      case MMB_SAMPLER_AMM: {
        if (s.ntuning != d * d) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "Sigma dimension differs from variate length %d", d);
        }
        h.sigl.resize((size_t)d * d);
        if (chol_lower(d, s.tuning, h.sigl.data())) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "AMM Sigma is not positive definite");
        }
        h.sigl_diag = true;
        for (int i = 0; i < d; ++i)
          for (int k = 0; k < i; ++k)
            if (h.sigl[i * d + k] != 0.0) h.sigl_diag = false;
        break;
      }
      case MMB_SAMPLER_SLICE:
        if (!(s.ntuning == 1 || s.ntuning == d)) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "length(width) differs from variate length %d", d);
        }
        break;
      case MMB_SAMPLER_GIBBS:
        // node IR: a lowered closure (mmb_ir_block.gibbs_*, checked by ir_validate) of one scalar node
        if (e->model == MMB_MODEL_IR && d != 1) {
          delete e;
          return fail(nullptr, MMB_E_UNSUPPORTED, "node IR: a Gibbs closure block draws one scalar node");
        }
        if (s.nnodes != 1) {
          delete e;
          return fail(nullptr, MMB_E_UNSUPPORTED, "Gibbs: one node per block");
        }
        break;
      case MMB_SAMPLER_NUTS:
        if (e->model == MMB_MODEL_RATS) {
          delete e;
          return fail(nullptr, MMB_E_UNSUPPORTED, "NUTS for the rats model is not lowered in this version");
        }
        break;
      case MMB_SAMPLER_HMC:
      case MMB_SAMPLER_MALA:  // validate(v) (hmc.jl:33-42, mala.jl:28-37)
        if (e->model == MMB_MODEL_RATS) {
          delete e;
          return fail(nullptr, MMB_E_UNSUPPORTED, "HMC/MALA for the rats model is not lowered in this version");
        }
        if (s.ntuning != 0) {
          if (s.ntuning != d * d) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "Sigma dimension differs from variate length %d", d);
          }
          h.sigl.resize((size_t)d * d);
          if (chol_lower(d, s.tuning, h.sigl.data())) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "PosDefException: Sigma is not positive definite");
          }
        }
        break;
      case MMB_SAMPLER_RWM:  // validate(v) (rwm.jl:39-44); the host broadcasts a scalar scale
        if (s.dim != d || s.ntuning != d) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "length(scale) differs from variate length %d", d);
        }
        for (int i = 0; i < d; ++i)
          if (!(std::isfinite(s.tuning[i]) && s.tuning[i] >= 0.0)) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "block %d: RWM scale[%d] must be finite and >= 0", b, i);
          }
        if (s.form < MMB_RWM_NORMAL || s.form > MMB_RWM_COSINE) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: unknown RWM proposal %d", b, s.form);
        }
        break;
      case MMB_SAMPLER_DGS:  // dgs.jl:56-80: one discrete node per block (the host splits DGS([a, b]))
        if (e->model != MMB_MODEL_IR) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: DGS samples discrete nodes of node-IR models only", b);
        }
        if (s.nnodes != 1 || !ir_dgs_family(ir->nodes[s.nodes[0]].family)) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: a DGS block holds one Bernoulli, Binomial, Categorical or "
                      "DiscreteUniform node", b);
        }
        break;
      case MMB_SAMPLER_SLICESIMPLEX:  // slicesimplex.jl:24-58: one Dirichlet node per block (the host splits the keys)
        if (e->model != MMB_MODEL_IR) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: SliceSimplex samples Dirichlet nodes of node-IR models only", b);
        }
        if (s.nnodes != 1 || ir->nodes[s.nodes[0]].family != MMB_IR_DIRICHLET || d < 2 || d > MMB_SIMPLEX_MAX) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: a SliceSimplex block holds one Dirichlet node of 2..%d elements", b,
                      MMB_SIMPLEX_MAX);
        }
        if (!(s.scale > 0.0 && s.scale <= 1.0)) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: scale is not in (0, 1]", b);
        }
        if (s.transform != 0) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: SliceSimplex moves on the simplex itself (transform = 0)", b);
        }
        e->ssx_kmax = std::max(e->ssx_kmax, d);
        break;
      case MMB_SAMPLER_BMG:
      case MMB_SAMPLER_BMC3:
      case MMB_SAMPLER_BIA:
      case MMB_SAMPLER_BHMC: {  // bmg.jl:26-37, bmc3.jl:26-37, bia.jl:36-50, bhmc.jl:30 (validate): one binary node per block
        const char* nm = binary_name(s.sampler);
        if (e->model != MMB_MODEL_IR) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: %s samples binary nodes of node-IR models only", b, nm);
        }
        if (s.nnodes != 1) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: a %s block holds exactly one node (one joint step over its "
                      "elements)", b, nm);
        }
        if (!ir_binary_node(ir->nodes[s.nodes[0]])) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: %s samples a Bernoulli or DiscreteUniform(0, 1) node; node %d "
                      "is not binary", b, nm, s.nodes[0]);
        }
        if (d < 1 || d > MMB_BINARY_MAX) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: a %s block holds a node of 1..%d elements", b, nm, MMB_BINARY_MAX);
        }
        const double all = d >= 32 ? 4294967295.0 : (double)((1u << d) - 1u);
        if (s.sampler == MMB_SAMPLER_BHMC) {
          // the cap bounds an update's wall events (samplers.h bhmc): a documented refusal
          if (!(std::isfinite(s.scale) && s.scale > 0.0 && s.scale <= MMB_BHMC_MAX_TRAVELTIME)) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "block %d: traveltime is not finite, > 0 and <= %g (128 pi)", b,
                        (double)MMB_BHMC_MAX_TRAVELTIME);
          }
          if (s.form != 0 && s.form != 1) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "block %d: refresh is 0 or 1", b);
          }
        } else if (s.sampler != MMB_SAMPLER_BIA && s.form == MMB_BINARY_K_INT) {
          if (s.nsteps < 1 || s.nsteps > d) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "block %d: k exceeds variate length %d", b, d);
          }
        } else if (s.sampler != MMB_SAMPLER_BIA && s.form == MMB_BINARY_K_LISTS) {
          if (s.ntuning < 1 || s.ntuning > MMB_BINARY_MAX_LISTS) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "block %d: k holds 1..%d index lists", b, MMB_BINARY_MAX_LISTS);
          }
          for (int i = 0; i < s.ntuning; ++i)
            if (!(s.tuning[i] >= 1.0 && s.tuning[i] <= all && s.tuning[i] == std::floor(s.tuning[i]))) {
              delete e;
              return fail(nullptr, MMB_E_ARG, "block %d: indices in k exceed variate length %d", b, d);
            }
        } else if (s.sampler != MMB_SAMPLER_BIA) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: unknown form %d of k", b, s.form);
        } else {
          if (!(s.epsilon > 0.0 && s.epsilon < 0.5)) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "block %d: epsilon is not in (0, 0.5)", b);
          }
          if (s.ntuning != 2 * d) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "block %d: A and D must contain %d probabilities each", b, d);
          }
          for (int i = 0; i < 2 * d; ++i)
            if (!(s.epsilon < s.tuning[i] && s.tuning[i] < 1.0 - s.epsilon)) {
              delete e;
              return fail(nullptr, MMB_E_ARG, "block %d: %s must contain %d probabilities in (%g, %g)", b,
                          i < d ? "A" : "D", d, s.epsilon, 1.0 - s.epsilon);
            }
          if (!(s.beta > 0.5 && s.beta <= 1.0)) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "block %d: decay is not in (0.5, 1]", b);
          }
          if (!(s.target > 0.0 && s.target < 1.0)) {
            delete e;
            return fail(nullptr, MMB_E_ARG, "block %d: target is not in (0, 1)", b);
          }
        }
        break;
      }
      case MMB_SAMPLER_ABC: {  // abc.jl:23-51: the packing is documented at MMB_SAMPLER_ABC (mamba_hip.h)
        const char* why = e->model != MMB_MODEL_IR ? "ABC samples the nodes of node-IR models only"
                                                   : abc_table(s, ir->nodes, ir->nnodes, ir->blocks[b], d, h.abc_tab);
        if (why) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: %s", b, why);
        }
        break;
      }
      default:
        delete e;
        return fail(nullptr, MMB_E_ARG, "unknown sampler kind %d", s.sampler);
    }
    if (e->model == MMB_MODEL_IR && s.sampler != MMB_SAMPLER_SLICESIMPLEX)
      for (int a = 0; a < s.nnodes; ++a)
        if (ir->nodes[s.nodes[a]].family == MMB_IR_DIRICHLET) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: Dirichlet node %d can be sampled by a SliceSimplex block only", b,
                      s.nodes[a]);
        }
    if (e->model == MMB_MODEL_IR && s.sampler != MMB_SAMPLER_DGS && !binary_kind(s.sampler))
      for (int a = 0; a < s.nnodes; ++a)
        if (ir_dgs_family(ir->nodes[s.nodes[a]].family)) {
          delete e;
          return fail(nullptr, MMB_E_ARG, "block %d: discrete node %d can be sampled by a DGS block only", b, s.nodes[a]);
        }
    h.tune_len = s.sampler == MMB_SAMPLER_ABC ? tune_len_of(s.sampler, d, s.nsteps, h.abc_tab[0])
                                              : tune_len_of(s.sampler, d);
    e->kinds |= 1u << s.sampler;
    e->blocks.push_back(std::move(h));
  }
  hipError_t st = hipSetDevice(device);
  if (st != hipSuccess) {
    delete e;
    return fail(nullptr, MMB_E_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(st));
  }
  e->device = device;
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&e->ev0) != hipSuccess || hipEventCreate(&e->ev1) != hipSuccess) {
    delete e;
    return fail(nullptr, MMB_E_HIP, "stream/event creation failed");
  }
  if (e->model == MMB_MODEL_IR) {  // device copies of the IR tables (read-only for every launch)
    bool ok = true;
    auto up = [&](auto& dst, const auto& v) {
      using T = typename std::remove_reference<decltype(v)>::type::value_type;
      if (!ok) return;
      ok = dst.alloc(v.size()) == hipSuccess &&
           (v.empty() || hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
    };
    {  // device code: every expression with its leaf+binop pairs fused (ir_fuse), padded
       // with END words (the interpreter fetches one word ahead, ir.h ev)
      std::vector<mmb_ir_node> nodes(e->ir_nodes);
      std::vector<mmb_ir_block> blocks(e->ir_blocks);
      std::vector<int32_t> code;
      ir_fuse(e->ir_code, nodes, blocks, code);
      code.resize(code.size() + 2, 0);
      up(e->d_ir_nodes, nodes);
      up(e->d_ir_code, code);
      up(e->d_ir_blocks, blocks);
    }
    up(e->d_ir_const, e->ir_const);
    up(e->d_ir_pool, e->ir_pool);
    up(e->d_ir_mon, e->ir_mon);
    // AMWG blocks whose logpdf! separates by coordinate: lane-parallel decisions in the specialised
    // kernel (MMB_IR_SEP=0 keeps every block on amwg_sub!'s sequential loop)
    const char* se = std::getenv("MMB_IR_SEP");
    const bool sep_on = !(se && std::string(se) == "0");
    for (size_t b = 0; sep_on && b < e->blocks.size(); ++b) {
      BlockHost& h = e->blocks[b];
      std::vector<int32_t> tab;
      if (h.spec.sampler == MMB_SAMPLER_AMWG &&
          ir_sep_table(e->ir_nodes, e->ir_code, e->ir_pool, e->ir_blocks[b], h.spec, e->P, tab, &h.sep_eps))
        up(h.sep_d, tab);
    }
    for (auto& h : e->blocks)
      if (h.spec.sampler == MMB_SAMPLER_ABC) up(h.sep_d, h.abc_tab);
    if (!ok) {
      mmb_destroy(e);
      return fail(nullptr, MMB_E_HIP, "node IR upload failed");
    }
  }
  *out = e;
  return 0;
}

int mmb_create(const mmb_model_spec* spec, int device, mmb_engine** out) {
  if (spec && spec->model == MMB_MODEL_IR)
    return fail(nullptr, MMB_E_ARG, "node-IR models are created with mmb_create_ir");
  return create_impl(spec, nullptr, device, out);
}

// drops the per-chain device state (the next mmb_init_chains, mmb_destroy)
static void free_dev(mmb_engine* e) {
  for (auto& h : e->blocks) static_cast<BlockChainBufs&>(h) = BlockChainBufs();
  static_cast<ChainBufs&>(*e) = ChainBufs();
  e->cperm_identity = true;
  e->order_fresh = false;
  e->draws_cap = 0;
}

void mmb_destroy(mmb_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
#ifdef MMB_WAVE_TIMES
  // rats: two chains per wave, four waves per workgroup
  if (e->model == MMB_MODEL_RATS)
    mmb_wave_times_dump((int)((e->K + 1) / 2), e->sw_resident > 0 ? 4 * e->sw_resident : 4096);
#endif
  if (e->jit_mod && std::getenv("MMB_IR_JIT_PROF") && std::atoi(std::getenv("MMB_IR_JIT_PROF")) == 1) {
    // phase timers of a profiling specialised kernel (ir_jit.cpp): the static kernels' names
    hipDeviceptr_t p = nullptr;
    size_t nb = 0;
    unsigned long long h[32] = {};
    if (hipModuleGetGlobal(&p, &nb, e->jit_mod, "mmb_prof") == hipSuccess && nb >= sizeof h &&
        hipMemcpyDtoH(h, p, sizeof h) == hipSuccess) {
      const char* names[] = {"amm:prep", "amm:load m/fl/Mv", "amm:proposal", "amm:logf x2+accept", "amm:moments+Sigma",
                             "amm:pchol", "amm:store", "gibbs", "iteration", "count", "pchol:steps",
                             "pchol:carry", "pchol:writeback", "amwg", "slice", "draws"};
      for (int i = 0; i < 16; ++i) fprintf(stderr, "MMB_PROF %-22s %llu\n", names[i], h[i]);
    }
  }
#ifdef MMB_PHASE_PROF
  mmb_prof_dump();
  mmb_prof_dump_line();
#endif
  // every buffer goes here, before the streams, the events and the module
  free_dev(e);
  for (BlockHost& h : e->blocks) h.sep_d.reset();
  static_cast<EngineBufs&>(*e) = EngineBufs();
  for (hipEvent_t ev : e->lg_cev)
    if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : e->lg_join)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& pool : e->evpoolx)
    for (hipEvent_t ev : pool) (void)hipEventDestroy(ev);
  for (hipStream_t q : e->lg_streamx)
    if (q) (void)hipStreamDestroy(q);
  for (hipEvent_t ev : e->sw_join)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& pool : e->sw_evpoolx)
    for (hipEvent_t ev : pool) (void)hipEventDestroy(ev);
  for (hipStream_t q : e->sw_streamx)
    if (q) (void)hipStreamDestroy(q);
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  for (hipEvent_t ev : e->evpool) (void)hipEventDestroy(ev);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  if (e->jit_mod) (void)hipModuleUnload(e->jit_mod);
  delete e;
}

int mmb_set_data(mmb_engine* e, const char* name, const double* x, int64_t n) {
  if (!e || !name || !x) return fail(e, MMB_E_ARG, "null argument");
  std::string nm(name);
  if (e->model == MMB_MODEL_LINE) {
    if (n != 5) return fail(e, MMB_E_ARG, "line: %s must have 5 elements", name);
    if (nm == "x") e->x.assign(x, x + 5);
    else if (nm == "y") e->y.assign(x, x + 5);
    else return fail(e, MMB_E_ARG, "line: unknown input %s", name);
  } else if (e->model == MMB_MODEL_LOGISTIC) {
    if (nm == "X") {
      if (n != (int64_t)e->lg_N * e->lg_p) return fail(e, MMB_E_ARG, "logistic: X must be nobs x ncoef");
      e->X.assign(x, x + n);
    } else if (nm == "y") {
      if (n != e->lg_N) return fail(e, MMB_E_ARG, "logistic: y must have nobs elements");
      for (int64_t i = 0; i < n; ++i)
        if (!(x[i] == 0.0 || x[i] == 1.0)) return fail(e, MMB_E_ARG, "logistic: y must be 0/1");
      e->y.assign(x, x + n);
    } else {
      return fail(e, MMB_E_ARG, "logistic: unknown input %s", name);
    }
    e->have_data = !e->X.empty() && !e->y.empty();
    if (e->have_data) {  // padded device copies: X [Np][64], y [Np]
      const size_t Np = (size_t)MMB_LG_NG * MMB_LG_NS * e->lg_rps;
      std::vector<double> hx(Np * MMB_LG_DV, 0.0), hy(Np, 0.0);
      for (int i = 0; i < e->lg_N; ++i) {
        for (int k = 0; k < e->lg_p; ++k) {
          hx[(size_t)i * MMB_LG_DV + k] = e->X[(size_t)i * e->lg_p + k];
        }
        hy[i] = e->y[i];
      }
      HIPCHK(e, hipSetDevice(e->device));
      if (!e->lg_X) HIPCHK(e, e->lg_X.alloc(hx.size()));
      if (!e->lg_y) HIPCHK(e, e->lg_y.alloc(hy.size()));
      HIPCHK(e, hipMemcpy(e->lg_X, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(e, hipMemcpy(e->lg_y, hy.data(), hy.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return 0;
  } else if (e->model == MMB_MODEL_RATS) {
    if (nm == "y") {
      if (n != 150) return fail(e, MMB_E_ARG, "rats: y must have 150 elements");
      e->y.assign(x, x + 150);
    } else if (nm == "x") {
      if (n != 5) return fail(e, MMB_E_ARG, "rats: x must have 5 elements");
      e->x.assign(x, x + 5);
    } else {
      return fail(e, MMB_E_ARG, "rats: unknown input %s", name);
    }
  }
  e->have_data = !e->x.empty() && !e->y.empty();
  if (e->have_data && e->model == MMB_MODEL_RATS) {
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->d_data) HIPCHK(e, e->d_data.alloc(150));
    HIPCHK(e, hipMemcpy(e->d_data, e->y.data(), 150 * sizeof(double), hipMemcpyHostToDevice));
  }
  return 0;
}

int mmb_num_values(const mmb_engine* e) { return e ? e->P : MMB_E_ARG; }
int mmb_num_monitored(const mmb_engine* e) { return e ? e->pmon : MMB_E_ARG; }
int64_t mmb_num_chains(const mmb_engine* e) { return e ? e->K : MMB_E_ARG; }
int64_t mmb_iter(const mmb_engine* e) { return e ? e->iter : MMB_E_ARG; }
int mmb_set_iter(mmb_engine* e, int64_t iter) {
  if (!e) return fail(e, MMB_E_ARG, "null engine");
  if (!e->d_vals) return fail(e, MMB_E_STATE, "mmb_init_chains not called");
  if (iter < 0 || iter > 0xffffffffLL) return fail(e, MMB_E_ARG, "iteration out of range");
  e->iter = iter;
  ++e->xepoch;
  return 0;
}
int64_t mmb_num_kept(const mmb_engine* e) { return e ? e->n_kept : MMB_E_ARG; }

// canonical values (K x P) <-> device layout
static void to_device_layout(const mmb_engine* e, const double* v, double* dv) {
  if (e->model == MMB_MODEL_RATS) {
    std::fill(dv, dv + e->VS, 0.0);
    for (int i = 0; i < 30; ++i) { dv[i] = v[1 + i]; dv[32 + i] = v[33 + i]; }
    dv[64] = v[0]; dv[65] = v[31]; dv[66] = v[32]; dv[67] = v[63]; dv[68] = v[64];
  } else if (e->model == MMB_MODEL_LOGISTIC || e->model == MMB_MODEL_IR) {
    std::fill(dv, dv + e->VS, 0.0);
    for (int i = 0; i < e->P; ++i) dv[i] = v[i];
  } else {
    dv[0] = v[0]; dv[1] = v[1]; dv[2] = v[2]; dv[3] = 0.0;
  }
}
static void from_device_layout(const mmb_engine* e, const double* dv, double* v) {
  if (e->model == MMB_MODEL_RATS) {
    for (int i = 0; i < 30; ++i) { v[1 + i] = dv[i]; v[33 + i] = dv[32 + i]; }
    v[0] = dv[64]; v[31] = dv[65]; v[32] = dv[66]; v[63] = dv[67]; v[64] = dv[68];
  } else if (e->model == MMB_MODEL_LOGISTIC || e->model == MMB_MODEL_IR) {
    for (int i = 0; i < e->P; ++i) v[i] = dv[i];
  } else {
    v[0] = dv[0]; v[1] = dv[1]; v[2] = dv[2];
  }
}

int mmb_set_values(mmb_engine* e, const double* values) {
  if (!e || !values) return fail(e, MMB_E_ARG, "null argument");
  if (!e->d_vals) return fail(e, MMB_E_STATE, "mmb_init_chains not called");
  constexpr unsigned kDiscreteKinds = (1u << MMB_SAMPLER_DGS) | (1u << MMB_SAMPLER_BMG) | (1u << MMB_SAMPLER_BMC3) |
                                      (1u << MMB_SAMPLER_BIA) | (1u << MMB_SAMPLER_BHMC);
  if (e->model == MMB_MODEL_IR && (e->kinds & kDiscreteKinds)) {
    // sampled discrete nodes: every value inside its support, which is what bounds the state-indexed
    // gathers x[T] (ir.h ev) and the constant-table lookups of the kernels (a binary block's node: 0 or
    // 1, validatebinary)
    for (const mmb_ir_node& N : e->ir_nodes) {
      if (N.fixed || !ir_dgs_family(N.family)) continue;
      for (int64_t k = 0; k < e->K; ++k)
        for (int i = 0; i < N.len; ++i) {
          const double x = values[k * e->P + N.off + i];
          double hi = N.hi;
          if (N.family == MMB_IR_BINOMIAL) {  // (one DATA / DATAS word: ir_validate)
            const int w = e->ir_code[N.expr[0]];
            hi = e->ir_pool[(w & 0xffffff) + ((int)((uint32_t)w >> 24) == MMB_IR_OP_DATA ? i : 0)];
          }
          if (!(x >= N.lo && x <= hi && x == std::floor(x)))
            return fail(e, MMB_E_ARG, "chain %lld: value %g of discrete node element %d is outside its support %g..%g",
                        (long long)k, x, i, N.lo, hi);
        }
    }
  }
  if (e->model == MMB_MODEL_IR && (e->kinds & (1u << MMB_SAMPLER_SLICESIMPLEX))) {
    // sampled Dirichlet nodes: a probability vector (validatesimplex, sampler.jl:80-82; the support of
    // ir_math.h mmb_ir_dirichlet_lp), so that a SliceSimplex update starts inside its first simplex
    for (const mmb_ir_node& N : e->ir_nodes) {
      if (N.fixed || N.family != MMB_IR_DIRICHLET) continue;
      for (int64_t k = 0; k < e->K; ++k) {
        double sum = 0.0;
        bool neg = false;
        for (int i = 0; i < N.len; ++i) {
          const double x = values[k * e->P + N.off + i];
          sum += x;
          neg = neg || !(x >= 0.0);
        }
        if (neg || !(std::fabs(sum - 1.0) <= MMB_SIMPLEX_TOL))
          return fail(e, MMB_E_ARG, "chain %lld: variate is not a probability vector (Dirichlet node at value slot %d)",
                      (long long)k, N.off);
      }
    }
  }
  ++e->xepoch;
  std::vector<double> h((size_t)e->K * e->VS);
  for (int64_t k = 0; k < e->K; ++k) to_device_layout(e, values + k * e->P, h.data() + k * e->VS);
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipMemcpy(e->d_vals, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

int mmb_get_values(mmb_engine* e, double* values) {
  if (!e || !values) return fail(e, MMB_E_ARG, "null argument");
  if (!e->d_vals) return fail(e, MMB_E_STATE, "mmb_init_chains not called");
  std::vector<double> h((size_t)e->K * e->VS);
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipMemcpy(h.data(), e->d_vals, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t k = 0; k < e->K; ++k) from_device_layout(e, h.data() + k * e->VS, values + k * e->P);
  return 0;
}

static int upload_blocks(mmb_engine* e) {
  std::vector<DBlock> db(e->blocks.size());
  for (size_t b = 0; b < e->blocks.size(); ++b) {
    BlockHost& h = e->blocks[b];
    DBlock& d = db[b];
    std::memset(&d, 0, sizeof d);
    d.kind = h.spec.sampler;
    d.nn = h.spec.nnodes;
    d.d = h.d;
    d.transform = h.spec.sampler == MMB_SAMPLER_SLICE ? h.spec.transform : binary_kind(h.spec.sampler) ? 0 : 1;
    const bool abc = h.spec.sampler == MMB_SAMPLER_ABC;
    d.form = h.spec.form;
    d.adapt = abc ? h.spec.nsteps : h.spec.adapt;  // ABC: nsim (maxdraw in batchsize, samplers.h abc)
    d.batchsize = h.spec.batchsize;
    // BMG / BMC3: the int k, or the number of index lists (their masks: d.width)
    if (h.spec.sampler == MMB_SAMPLER_BMG || h.spec.sampler == MMB_SAMPLER_BMC3)
      d.batchsize = h.spec.form == MMB_BINARY_K_LISTS ? (int32_t)h.tuning.size() : h.spec.nsteps;
    d.sigl_diag = h.sigl_diag;
    // forward differences (the reference's default) unless the analytic gradient was asked for
    d.fdgrad = h.spec.gradient != MMB_GRAD_ANALYTIC ? 1 : 0;
    for (int a = 0; a < 4; ++a) d.nodes[a] = a < h.spec.nnodes ? h.spec.nodes[a] : -1;
    // line: element -> value index (beta -> 0,1; s2 -> 2)
    int o = 0;
    for (int a = 0; a < h.spec.nnodes && o < 4; ++a) {
      int n = h.spec.nodes[a];
      if (e->model == MMB_MODEL_LINE) {
        if (n == MMB_LINE_BETA) { d.emap[o++] = 0; if (o < 4) d.emap[o++] = 1; }
        else d.emap[o++] = 2;
      } else {
        d.emap[o++] = n;
      }
    }
    d.target = h.spec.target;
    d.beta = h.spec.beta;
    d.scale = (h.spec.sampler == MMB_SAMPLER_BIA || abc) ? h.spec.epsilon : h.spec.scale;
    d.width0 = h.tuning.empty() ? 0.0 : h.tuning[0];
    d.width = (h.spec.sampler == MMB_SAMPLER_SLICE && h.tuning.size() > 1) ? h.width.get() : nullptr;
    if ((h.spec.sampler == MMB_SAMPLER_BMG || h.spec.sampler == MMB_SAMPLER_BMC3) && h.spec.form == MMB_BINARY_K_LISTS)
      d.width = h.width.get();
    d.sigl = h.sigl_d;
    d.t_sigma = h.sigma; d.t_accept = h.accept; d.t_m = h.m; d.t_flags = h.flags;
    d.t_Mv = h.Mv; d.t_Mvv = h.Mvv; d.t_Mv_alt = h.Mv_alt; d.t_Mvv_alt = h.Mvv_alt; d.t_Ls = h.Ls; d.t_piv = h.piv; d.t_xnext = h.xnext; d.t_xtag = h.xtag; d.t_nuts = h.nuts; d.t_nfr = h.nfr;
    d.t_astat = h.astat;
    d.t_hmc = h.hmc;
    d.ir_blk = (int32_t)b;
    d.gibbs_a = __builtin_nan("");
    if (e->model == MMB_MODEL_IR && h.spec.sampler == MMB_SAMPLER_GIBBS) {
      // a constant Gamma shape (the expression is one CONST word): the sweep kernel draws the
      // variate with every block's draws of a batch of iterations at once (samplers.h predraw)
      const mmb_ir_block& IB = e->ir_blocks[b];
      const int pc = IB.gibbs_expr[0];
      if (IB.gibbs_family != MMB_IR_NORMAL && pc >= 0 && pc + 1 < (int)e->ir_code.size() &&
          (int)((uint32_t)e->ir_code[pc] >> 24) == MMB_IR_OP_CONST && e->ir_code[pc + 1] == MMB_IR_OP_END) {
        const double a = e->ir_const[e->ir_code[pc] & 0xffffff];
        if (a >= 1.0) d.gibbs_a = a;  // (predraw replays Marsaglia-Tsang, a >= 1; smaller: mmb_gamma_any)
      }
      d.gibbs_fam = IB.gibbs_family;
    }
    d.sep = h.sep_d;
    d.sep_eps = h.sep_eps;
  }
  if (!e->d_blocks) HIPCHK(e, e->d_blocks.alloc(MMB_MAX_BLOCKS));
  HIPCHK(e, hipMemcpy(e->d_blocks, db.data(), db.size() * sizeof(DBlock), hipMemcpyHostToDevice));
  return 0;
}

int mmb_init_chains(mmb_engine* e, const double* init, int64_t K, int64_t chain_offset, uint64_t seed) {
  if (!e || !init) return fail(e, MMB_E_ARG, "null argument");
  if (K < 1 || K > (int64_t)1 << 30) return fail(e, MMB_E_ARG, "K out of range");
  if (chain_offset < 0 || chain_offset + K > ((int64_t)1 << 32))
    return fail(e, MMB_E_ARG, "global chain ids must fit in 32 bits");
  if (!e->have_data) return fail(e, MMB_E_STATE, "inputs must be set before inits");
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  free_dev(e);
  e->K = K;
  e->chain_offset = chain_offset;
  e->seed = seed;
  e->iter = 0;
  e->n_kept = 0;
  HIPCHK(e, e->d_vals.alloc((size_t)K * e->VS));
  e->slice_overflows = 0;
  HIPCHK(e, e->d_nstat.alloc(8));
  HIPCHK(e, e->d_nstat.zero(8));
  const size_t DP = e->DP, TP = e->TP;
  for (auto& h : e->blocks) {
    HIPCHK(e, h.m.alloc(K));
    HIPCHK(e, h.flags.alloc(K));
    HIPCHK(e, h.m.zero(K));
    HIPCHK(e, h.flags.zero(K));
    if (h.spec.sampler == MMB_SAMPLER_AMWG) {
      HIPCHK(e, h.sigma.alloc(K * DP));
      HIPCHK(e, h.accept.alloc(K * DP));
      std::vector<double> sg(K * DP, 0.0);
      for (int64_t k = 0; k < K; ++k)
        for (int i = 0; i < h.d; ++i) sg[k * DP + i] = h.tuning.size() == 1 ? h.tuning[0] : h.tuning[i];
      HIPCHK(e, hipMemcpy(h.sigma, sg.data(), sg.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(e, h.accept.zero(K * DP));
    } else if (h.spec.sampler == MMB_SAMPLER_AMM) {
      HIPCHK(e, h.Mv.alloc(K * DP));
      HIPCHK(e, h.Mvv.alloc(K * TP));
      HIPCHK(e, h.Ls.alloc(K * TP));
      HIPCHK(e, h.piv.alloc(K * DP));
      HIPCHK(e, h.Mv.zero(K * DP));
      HIPCHK(e, h.Mvv.zero(K * TP));
      HIPCHK(e, h.Ls.zero(K * TP));
      if (amm_posform(e)) {  // the kernels of samplers.h amm's lazy factor store
        HIPCHK(e, h.Mv_alt.alloc(K * DP));
        HIPCHK(e, h.Mvv_alt.alloc(K * TP));
        HIPCHK(e, h.Mv_alt.zero(K * DP));
        HIPCHK(e, h.Mvv_alt.zero(K * TP));
      }
      std::vector<uint8_t> pv(K * DP);
      for (int64_t k = 0; k < K; ++k)
        for (size_t i = 0; i < DP; ++i) pv[k * DP + i] = (uint8_t)i;
      HIPCHK(e, hipMemcpy(h.piv, pv.data(), pv.size(), hipMemcpyHostToDevice));
      HIPCHK(e, h.xnext.alloc(K * DP));
      HIPCHK(e, h.xtag.alloc(K));
      HIPCHK(e, h.xtag.fill_bytes(0xff, K));  // -1: no carried proposal
      HIPCHK(e, h.astat.alloc(K * MMB_AMM_STAT_STRIDE));
      HIPCHK(e, h.astat.zero(K * MMB_AMM_STAT_STRIDE));
      HIPCHK(e, h.sigl_d.alloc((size_t)h.d * h.d));
      HIPCHK(e, hipMemcpy(h.sigl_d, h.sigl.data(), h.sigl.size() * sizeof(double), hipMemcpyHostToDevice));
    } else if (h.spec.sampler == MMB_SAMPLER_RWM) {
      HIPCHK(e, h.sigma.alloc(K * DP));
      std::vector<double> sg(K * DP, 0.0);
      for (int64_t k = 0; k < K; ++k)
        for (int i = 0; i < h.d; ++i) sg[k * DP + i] = h.tuning[i];
      HIPCHK(e, hipMemcpy(h.sigma, sg.data(), sg.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(e, h.astat.alloc(K * MMB_AMM_STAT_STRIDE));
      HIPCHK(e, h.astat.zero(K * MMB_AMM_STAT_STRIDE));
    } else if (h.spec.sampler == MMB_SAMPLER_ABC) {
      // scale in sigma (as RWM's); the canonical tune row in hmc, zeroed: every chain simulates its first Tsim
      // at its first update
      HIPCHK(e, h.sigma.alloc(K * DP));
      std::vector<double> sg(K * DP, 0.0);
      for (int64_t k = 0; k < K; ++k)
        for (int i = 0; i < h.d; ++i) sg[k * DP + i] = h.tuning[i];
      HIPCHK(e, hipMemcpy(h.sigma, sg.data(), sg.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(e, h.hmc.alloc((size_t)K * h.tune_len));
      HIPCHK(e, h.hmc.zero((size_t)K * h.tune_len));
      HIPCHK(e, h.astat.alloc(K * MMB_AMM_STAT_STRIDE));
      HIPCHK(e, h.astat.zero(K * MMB_AMM_STAT_STRIDE));
    } else if (h.spec.sampler == MMB_SAMPLER_NUTS) {
      HIPCHK(e, h.nuts.alloc(K * 8));
      HIPCHK(e, h.nuts.zero(K * 8));
      if (e->model == MMB_MODEL_LINE) {
        const size_t fr = (size_t)NutsFrames<Mdl<MMB_MODEL_LINE>::G * Mdl<MMB_MODEL_LINE>::R>::DBL;
        HIPCHK(e, h.nfr.alloc(K * fr));
      } else if (e->model == MMB_MODEL_IR) {
        const size_t fr = (size_t)NutsFrames<Mdl<MMB_MODEL_IR>::G * Mdl<MMB_MODEL_IR>::R>::DBL;
        HIPCHK(e, h.nfr.alloc(K * fr));
      }
    } else if (h.spec.sampler == MMB_SAMPLER_HMC || h.spec.sampler == MMB_SAMPLER_MALA) {
      HIPCHK(e, h.hmc.alloc(K * 2));
      std::vector<double> t(K * 2);
      for (int64_t k = 0; k < K; ++k) { t[2 * k] = h.spec.epsilon; t[2 * k + 1] = (double)h.spec.nsteps; }
      HIPCHK(e, hipMemcpy(h.hmc, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
      if (!h.sigl.empty()) {
        HIPCHK(e, h.sigl_d.alloc((size_t)h.d * h.d));
        HIPCHK(e, hipMemcpy(h.sigl_d, h.sigl.data(), h.sigl.size() * sizeof(double), hipMemcpyHostToDevice));
      }
    } else if (h.spec.sampler == MMB_SAMPLER_SLICE && h.tuning.size() > 1) {
      HIPCHK(e, h.width.alloc(h.tuning.size()));
      HIPCHK(e, hipMemcpy(h.width, h.tuning.data(), h.tuning.size() * sizeof(double), hipMemcpyHostToDevice));
    } else if (binary_kind(h.spec.sampler)) {
      HIPCHK(e, h.astat.alloc(K * MMB_AMM_STAT_STRIDE));
      HIPCHK(e, h.astat.zero(K * MMB_AMM_STAT_STRIDE));
      if (h.spec.sampler == MMB_SAMPLER_BIA) {  // A in sigma, D in accept, iter in m (zeroed above)
        HIPCHK(e, h.sigma.alloc(K * DP));
        HIPCHK(e, h.accept.alloc(K * DP));
        std::vector<double> ta(K * DP, 0.0), td(K * DP, 0.0);
        for (int64_t k = 0; k < K; ++k)
          for (int i = 0; i < h.d; ++i) {
            ta[k * DP + i] = h.tuning[i];
            td[k * DP + i] = h.tuning[h.d + i];
          }
        HIPCHK(e, hipMemcpy(h.sigma, ta.data(), ta.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(h.accept, td.data(), td.size() * sizeof(double), hipMemcpyHostToDevice));
      } else if (h.spec.sampler == MMB_SAMPLER_BHMC) {
        // position in sigma, velocity in accept, wallhits and wallcrosses in hmc, initialised in m (zeroed
        // above: every chain draws its particle at its first update)
        HIPCHK(e, h.sigma.alloc(K * DP));
        HIPCHK(e, h.accept.alloc(K * DP));
        HIPCHK(e, h.hmc.alloc(K * 2));
        HIPCHK(e, h.sigma.zero(K * DP));
        HIPCHK(e, h.accept.zero(K * DP));
        HIPCHK(e, h.hmc.zero(K * 2));
      } else if (h.spec.form == MMB_BINARY_K_LISTS) {
        HIPCHK(e, h.width.alloc(h.tuning.size()));
        HIPCHK(e, hipMemcpy(h.width, h.tuning.data(), h.tuning.size() * sizeof(double), hipMemcpyHostToDevice));
      }
    }
  }
  if (e->model == MMB_MODEL_LOGISTIC) {
    HIPCHK(e, e->lg_vec.alloc((size_t)K * MMB_LG_NVEC * MMB_LG_DV));
    HIPCHK(e, e->lg_vec.zero((size_t)K * MMB_LG_NVEC * MMB_LG_DV));
    HIPCHK(e, e->lg_sc.alloc((size_t)K * MMB_LG_NSC));
    HIPCHK(e, e->lg_iv.alloc((size_t)K * MMB_LG_NIV));
    HIPCHK(e, e->lg_iv.zero((size_t)K * MMB_LG_NIV));
    HIPCHK(e, e->lg_itc.alloc((size_t)K));
    HIPCHK(e, e->lg_frames.alloc((size_t)K * NutsFrames<MMB_LG_DV>::DBL));
    HIPCHK(e, e->lg_pos.alloc((size_t)K * MMB_LG_DV));
    HIPCHK(e, e->lg_gpart.alloc((size_t)MMB_LG_NG * MMB_LG_NS * K * MMB_LG_DV));
    HIPCHK(e, e->lg_lpart.alloc((size_t)MMB_LG_NG * MMB_LG_NS * K * (e->lg_fd ? e->lg_p + 1 : 1)));
    HIPCHK(e, e->lg_count.alloc(2 * MMB_LG_SPLIT_MAX));
    HIPCHK(e, e->lg_s2c.alloc((size_t)2 * K));
    HIPCHK(e, e->lg_ngrad.alloc(1));
    if (!e->lg_hcount) HIPCHK(e, e->lg_hcount.alloc(2 * MMB_LG_SPLIT_MAX));
    for (hipEvent_t& ev : e->lg_cev)
      if (!ev) HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    for (hipEvent_t& ev : e->lg_join)
      if (!ev) HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    for (hipStream_t& q : e->lg_streamx)
      if (!q) HIPCHK(e, hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
  }
  int rc = upload_blocks(e);
  if (rc) return rc;
  return mmb_set_values(e, init);
}

static int64_t kept_upto(int64_t t, int64_t burnin, int64_t thin) {
  return t > burnin ? (t - burnin) / thin : 0;
}

void fill_args(const mmb_engine* e, SweepArgs& A) {
  std::memset(&A, 0, sizeof A);
  A.K = (int32_t)e->K;
  A.chain_offset = (uint32_t)e->chain_offset;
  A.seed = e->seed;
  A.nb = (int32_t)e->blocks.size();
  A.vals = e->d_vals;
  A.xepoch = e->xepoch;
  A.nuts_stat = e->d_nstat;
  A.ig_c = 0.001 * std::log(0.001) - std::lgamma(0.001);
  A.blocks = e->d_blocks;
  A.cperm = e->cperm_identity ? nullptr : e->d_cperm.get();
  A.wg_offset = 0;  // one part: every workgroup (mmb_run deals them to parts)
  A.wg_stride = 1;
  {  // MMB_AMWG_EXACT=1: AMWG updates by amwg_sub!'s sequential loop; 2: wide AMWG band.
     // MMB_SLICE_EXACT=1: Slice shrink candidates one at a time.  MMB_AMWG_PROBE=1: tests only.
    const char* ae = std::getenv("MMB_AMWG_EXACT");
    const int v = ae ? std::atoi(ae) : 0;
    A.amwg_exact = (v == 1 || v == 2) ? v : 0;
    const char* se = std::getenv("MMB_SLICE_EXACT");
    A.slice_exact = (se && std::atoi(se) == 1) ? 1 : 0;
    const char* ap = std::getenv("MMB_AMWG_PROBE");
    A.amwg_probe = (ap && std::atoi(ap) == 1) ? 1 : 0;
  }
  if (e->model == MMB_MODEL_IR) {
    A.ir_nodes = e->d_ir_nodes; A.ir_code = e->d_ir_code; A.ir_const = e->d_ir_const;
    A.ir_pool = e->d_ir_pool; A.ir_blocks = e->d_ir_blocks; A.ir_mon = e->d_ir_mon;
    A.ir_nmon = (int32_t)e->ir_mon.size();
    A.ir_pmon = e->pmon;
    A.ir_vs = e->VS;
    A.ir_red0 = e->P;  // Gibbs reduction slots follow the values
    A.ir_npool = (int32_t)e->ir_pool.size();
    // AMM scratch mat[TP] | z2 | vv | mv | ia (+ pchol32's reciprocal slot), the state (and its
    // candidate copy), the expression stack (ir.h Mdl::load; interpreter: Mdl<IR>::AMM_DBL, TP = 528)
    A.ir_amm = (e->kinds & (1u << MMB_SAMPLER_AMM)) ? (int32_t)(e->TP + 4 * Mdl<MMB_MODEL_IR>::DP + 2) : 0;
    A.ir_lds = A.ir_amm + (e->ir_noprop ? 1 : 2) * e->VS +
               (e->jit_fn ? e->ir_stack_dbl : (e->ir_stack + 1) * Mdl<MMB_MODEL_IR>::G);
    // SliceSimplex vertex rows (samplers.h slice_simplex), last, so that every other scheme's layout stays
    A.ir_ssx = e->ssx_kmax * Mdl<MMB_MODEL_IR>::G;
    A.ir_lds += A.ir_ssx;
  } else if (e->model == MMB_MODEL_RATS) {
    double s = 0.0;
    for (int i = 0; i < 5; ++i) s += e->x[i];
    A.xbar = s / 5.0;
    for (int i = 0; i < 5; ++i) A.xm[i] = e->x[i] - A.xbar;
    A.data0 = e->d_data;
  } else {
    for (int i = 0; i < 5; ++i) { A.lx[i] = e->x[i]; A.ly[i] = e->y[i]; }
  }
}

// Chain parts of a window (mmb_run).  A launch of the rats kernels ends in a tail: its wavefronts
// fall into duration classes, two per resident slot, and the slots that drew the short ones idle
// until the last wave is done (busy 84-86 % of a launch's span), and the next
// launch waits on the stream for that last wave although it depends on its own chains only.  So the
// workgroups are dealt round-robin to `parts` parts over the one sorted slot -> chain table (the
// same class mix in each, slow classes first), every part a sequence of launches on its own
// stream: a part's launch n + 1 waits for its own launch n, and the other parts' resident launches
// fill the slots its tail frees.  Results do not depend on the parts (every index of the kernel
// is the chain's own).  The 32-lane kernels only (rats and the node IR; the line and logistic paths
// have no parts): MMB_SWEEP_PARTS=1..4 forces the count; unset, MMB_SWEEP_PARTS_DEFAULT parts when
// each part still has a workgroup for every resident workgroup slot of the device, else one.
// Default 2 (16384 rats chains, 400 steps: 1.45-1.46e8 chain-updates/s vs 1.32-1.33e8 on one
// stream; 3 parts as fast, 4 slower than one).
constexpr int MMB_SWEEP_PARTS_DEFAULT = 2;
static int sweep_parts(mmb_engine* e, const SweepArgs& A, int* parts) {
  *parts = 1;
  if (!(e->model == MMB_MODEL_RATS || e->model == MMB_MODEL_IR)) return 0;
  int nwg = 0, per_cu = 0;
  if (e->jit_fn) {  // specialised node-IR kernel: the interpreter's launch shape (mmb_run)
    const int per_block = 128 / Mdl<MMB_MODEL_IR>::G;
    nwg = (A.K + per_block - 1) / per_block;
    if (!e->sw_resident) {
      const size_t lds = (size_t)per_block * Mdl<MMB_MODEL_IR>::lds_stride(A) * sizeof(double);
      HIPCHK(e, hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, e->jit_fn, 128, lds));
    }
  } else {
    hipError_t st = mmb_sweep_shape(e->model, e->kinds, A, &nwg, e->sw_resident ? nullptr : &per_cu);
    if (st != hipSuccess) return fail(e, MMB_E_HIP, "sweep shape: %s", hipGetErrorString(st));
  }
  if (!e->sw_resident) {
    int cus = 0;
    HIPCHK(e, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
    e->sw_resident = std::max(1, per_cu * cus);
  }
  int p = 1;
  const char* s = std::getenv("MMB_SWEEP_PARTS");
  if (s && std::atoi(s) >= 1) {
    p = std::min(std::atoi(s), MMB_SWEEP_PARTS_MAX);
  } else {
    p = MMB_SWEEP_PARTS_DEFAULT;
    while (p > 1 && nwg / p < e->sw_resident) --p;
  }
  *parts = std::max(1, std::min(p, nwg));  // a part past the last workgroup would launch nothing
  return 0;
}

static int iters_per_launch_one(const mmb_engine* e) {
  // rats: 20 (16384 chains: ~2.5 ms launches; 16 was 0.5-0.9 % over 8 and 6 % over 4 in the
  // round-4 A/B, the launch tail amortised; round 5: 20 as fast as 16 and 32 over 400 steps, and a
  // 20-iteration window runs as one launch: 1.226e8 vs 1.21e8 for 10 + 10); line: 256 (an
  // iteration of the quad kernel is ~8 us, so 64 per launch left a launch gap every ~0.5 ms)
  return e->model == MMB_MODEL_RATS ? 20 : e->model == MMB_MODEL_IR ? 16 : e->model == MMB_MODEL_LINE ? 256 : 64;
}

static int iters_per_launch(const mmb_engine* e, int parts, int64_t iters) {
  const char* s = std::getenv("MMB_ITERS_PER_LAUNCH");
  if (s && std::atoi(s) > 0) return std::atoi(s);
  const int W = iters_per_launch_one(e);
  // chain parts fill each other's launch tails only from a part's second launch on (all parts'
  // first launches start together), so a window that would be a single launch runs as two:
  // 16384 rats chains, 20 iterations, 2 parts: 10 + 10 1.25-1.28e8 chain-updates/s, 20 1.21e8
  if (parts > 1 && iters > 1) return (int)std::min<int64_t>(W, (iters + 1) / 2);
  return W;
}


// Wavefront pairing of the 32-lane kernels (two chains per wavefront step together): a chain whose
// AMM moment matrix is indefinite stops its pivoted Cholesky after a few pivots every update
// (the amm.jl:102 alias leaves about half the chains so, persistently), but its
// wavefront runs until the partner chain has finished.  Before a window the engine orders the
// chains by class -- for each AMM block, whether the chain has a valid factor (flags bit 2) --
// so chains that stop alike share wavefronts; the kernel maps lane-group slot -> chain through
// the table (sweep.h), and every chain keeps its own state, draws column and Philox id, so the
// results are identical for any order.  The table is a stable counting sort computed on the
// device (sweep.hip order_chains_kernel), queued on the engine stream behind the previous
// window: no synchronisation, no copy and no host work per call.  MMB_ORDER_CHAINS=0 keeps the
// identity.
static int order_chains(mmb_engine* e) {
  e->cperm_identity = true;
  if (!(e->model == MMB_MODEL_RATS || e->model == MMB_MODEL_IR) || e->K < 4) return 0;
  const char* env = std::getenv("MMB_ORDER_CHAINS");
  if (env && std::string(env) == "0") return 0;
  OrderArgs oa;
  std::memset(&oa, 0, sizeof oa);
  for (const BlockHost& h : e->blocks)
    if (h.spec.sampler == MMB_SAMPLER_AMM && h.flags && oa.nblk < MMB_ORDER_BLOCKS) oa.flags[oa.nblk++] = h.flags;
  if (oa.nblk == 0) return 0;
  if (!e->d_cperm) HIPCHK(e, e->d_cperm.alloc((size_t)e->K));
  oa.K = (int32_t)e->K;
  oa.perm = e->d_cperm;
  // chains per workgroup of the 32-lane sweep kernels (sweep.hip launch: rats 256 threads, node IR 128)
  oa.cpw = e->model == MMB_MODEL_RATS ? 8 : 4;
  {
    // default 1, slow classes first: the launch's second dispatch round then ends on the fast
    // ones (20-iteration windows: 1.17-1.18e8 -> 1.20-1.21e8 chain-updates/s; balanced
    // workgroups, mode 2, 1.12-1.13e8)
    const char* om = std::getenv("MMB_ORDER_MODE");
    oa.mode = om ? std::atoi(om) : 1;
    if (oa.mode < 0 || oa.mode > 2) oa.mode = 1;
  }
  hipError_t st = mmb_launch_order_chains(oa, e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "order_chains launch: %s", hipGetErrorString(st));
  e->cperm_identity = false;
  return 0;
}

static int64_t order_every() {
  const char* s = std::getenv("MMB_ORDER_EVERY");
  return (s && std::atoi(s) > 0) ? std::atoi(s) : 64;
}

// Launch widths of a window: ceil(iters / W) launches of equal length (+-1), so a window of 20
// iterations at W = 16 runs 10 + 10 instead of 16 + 4 (a short launch pays the launch tail on
// few iterations)
static int launch_width(int64_t iters, int W, int64_t li) {
  const int64_t nl = (iters + W - 1) / W;
  const int64_t q = iters / nl, r = iters % nl;
  return (int)(q + (li < r ? 1 : 0));
}


// Config-4 window: ctl / grad kernel pairs until no chain requests a gradient.  The
// request count is read back every LG_CHECK steps (pinned host words, one check behind the
// launches); surplus pairs after the last chain finished are no-ops (the grad kernel exits on
// count 0, idle chains return).
//
// The chains run as independent parts (default 3, MMB_LG_SPLIT=1..4), each on its own stream
// with its own request list, partial buffers and count words: a step is a latency-bound control
// kernel (one wave per chain, little arithmetic) behind an MFMA gradient kernel, and the other
// part's gradient kernel fills the GPU while one part is in its control kernel (and the window's
// tail, where few chains still run, overlaps across the parts).  Every chain keeps its own state,
// Philox id and draws column, so the draws are identical for any split.
#ifndef MMB_LG_FOLD_MIN
#define MMB_LG_FOLD_MIN 1024  // chains: 16 tiles x 32 groups = 512 workgroups
#endif
static int run_logistic(mmb_engine* e, const mmb_run_args* a, double* draws, int64_t kept0, int64_t nk,
                        bool want) {
  constexpr int LG_CHECK = 8;
  const BlockHost& h = e->blocks[0];
  LgArgs A0;
  std::memset(&A0, 0, sizeof A0);
  A0.K = (int32_t)e->K; A0.p = e->lg_p; A0.N = e->lg_N; A0.rps = e->lg_rps;
  A0.Np = MMB_LG_NG * MMB_LG_NS * e->lg_rps;
  A0.chain_offset = (uint32_t)e->chain_offset;
  A0.seed = e->seed;
  A0.iter0 = e->iter;
  A0.it_end = e->iter + a->iters;
  A0.burnin = a->burnin; A0.thin = a->thin; A0.model_burnin = a->model_burnin; A0.kept_origin = kept0;
  A0.prior_sd = e->spec.prior_sd;
  A0.target = h.spec.target;
  A0.X = e->lg_X; A0.y = e->lg_y;
  A0.vals = e->d_vals; A0.vec = e->lg_vec; A0.sc = e->lg_sc; A0.iv = e->lg_iv; A0.itc = e->lg_itc;
  A0.kind = h.spec.sampler;
  A0.frames = e->lg_frames; A0.tm = h.m; A0.tflags = h.flags;
  A0.tune = A0.kind == MMB_SAMPLER_NUTS ? h.nuts.get() : h.hmc.get();
  const int tune_w = A0.kind == MMB_SAMPLER_NUTS ? 8 : 2;
  A0.sigl = h.sigl_d;
  A0.draws = draws;
  A0.Kd = (int32_t)e->K;
  A0.pos = e->lg_pos; A0.gpart = e->lg_gpart; A0.lpart = e->lg_lpart; A0.count = e->lg_count; A0.s2c = e->lg_s2c;
  A0.ngrad = e->lg_ngrad;
  A0.nstat = e->d_nstat;
  A0.fd = e->lg_fd ? 1 : 0;
  A0.nv = e->lg_fd ? e->lg_p + 1 : 1;
  // default 3 parts: 1.34e6 chain-updates/s on config 4 vs 1.28e6 (2), 1.11e6 (4), 1.12e6 (1)
  int nh = 3;
  if (const char* hs = std::getenv("MMB_LG_SPLIT")) nh = std::max(1, std::min(MMB_LG_SPLIT_MAX, std::atoi(hs)));
  if (e->K < 32 * nh) nh = 1;
  struct Half {
    LgArgs A;
    hipStream_t st;
    std::vector<hipEvent_t>* ev;
    int64_t s = 0;
    int nbound = 0;
    bool done = false;
  } H[MMB_LG_SPLIT_MAX];
  for (int i = 0; i < nh; ++i) {
    // chains [b, b + k) of the engine: every per-chain array offset by b rows, the partial and
    // request buffers split in proportion (each half indexes them with its own K)
    const int64_t b = e->K * i / nh, k = e->K * (i + 1) / nh - b;
    LgArgs& A = H[i].A;
    A = A0;
    A.K = (int32_t)k;
    A.Kv = k * A.nv;
    A.chain_offset = (uint32_t)(e->chain_offset + b);
    A.vals += b * MMB_LG_DV; A.vec += b * MMB_LG_NVEC * MMB_LG_DV; A.sc += b * MMB_LG_NSC;
    A.iv += b * MMB_LG_NIV; A.itc += b; A.frames += b * NutsFrames<MMB_LG_DV>::DBL;
    A.tune += b * tune_w; A.tm += b; A.tflags += b;
    if (A.draws) A.draws += b;
    A.pos += b * MMB_LG_DV;
    A.gpart += (size_t)MMB_LG_NG * MMB_LG_NS * b * MMB_LG_DV;
    A.lpart += (size_t)MMB_LG_NG * MMB_LG_NS * b * A.nv;
    A.count += 2 * i;
    A.s2c += 2 * b;
    H[i].st = i == 0 ? e->stream : e->lg_streamx[i - 1];
    H[i].ev = i == 0 ? &e->evpool : &e->evpoolx[i - 1];
    H[i].nbound = (int)k;
  }
  HIPCHK(e, hipMemsetAsync(e->lg_ngrad, 0, sizeof(unsigned long long), e->stream));
  e->kernel_ms = 0.0;
  e->launches = 0;
  e->units = 0;
  e->lg_steps = 0;
  if (a->iters > 0) {
    // every update needs >= 1 gradient; a NUTS tree has <= 2^depth leaves and nutsepsilon
    // <= 4001; HMC needs L + 1 gradients per update, MALA 2
    int64_t per = (1LL << MMB_NUTS_MAX_DEPTH) + 2, extra = 4002;
    if (A0.kind != MMB_SAMPLER_NUTS) {
      std::vector<double> th;
      int rc = d2h(e, th, h.hmc, e->K * 2);
      if (rc) return rc;
      double lmax = 0.0;
      for (int64_t k = 0; k < e->K; ++k) lmax = std::max(lmax, th[k * 2 + 1]);
      per = A0.kind == MMB_SAMPLER_MALA ? 2 : (int64_t)std::max(lmax, 0.0) + 1;
      extra = 0;
    }
    const int64_t cap = a->iters * per + extra + 4 * LG_CHECK;
    HIPCHK(e, hipMemsetAsync(e->lg_count, 0, 2 * MMB_LG_SPLIT_MAX * sizeof(int32_t), e->stream));
    // every return from here on -- the error paths included -- leaves no part kernel running:
    // an early return drains the part streams (the next mmb_run / mmb_set_* on the engine stream
    // may reset lg_count or touch lg_vec / vals, which a still-running part would use)
    struct PartDrain {
      Half* H;
      int nh;
      bool armed = true;
      ~PartDrain() {
        if (armed)
          for (int i = 0; i < nh; ++i) (void)hipStreamSynchronize(H[i].st);
      }
    } drain{H, nh};
    if (nh > 1) {  // fork: the part streams start behind everything queued on the engine stream
      HIPCHK(e, hipEventRecord(e->lg_join[0], e->stream));
      for (int i = 1; i < nh; ++i) HIPCHK(e, hipStreamWaitEvent(H[i].st, e->lg_join[0], 0));
    }
    for (int i = 0; i < nh; ++i) {
      hipError_t st = mmb_lg_launch_ctl(H[i].A, 1, 0, H[i].A.K, 0, H[i].st);
      if (st != hipSuccess) return fail(e, MMB_E_HIP, "lg_ctl launch: %s", hipGetErrorString(st));
    }
    for (int live = nh; live > 0;) {
      for (int i = 0; i < nh; ++i) {
        Half& q = H[i];
        if (q.done) continue;
        const LgArgs& A = q.A;
        const int64_t s = q.s;
        const int par = (int)(s & 1);
        std::vector<hipEvent_t>& ev = *q.ev;
        if (a->time_kernels) {
          while ((int64_t)ev.size() < 2 * (s + 1)) {
            hipEvent_t x;
            HIPCHK(e, hipEventCreate(&x));
            ev.push_back(x);
          }
          HIPCHK(e, hipEventRecord(ev[2 * s], q.st));
        }
        // group mode once the step is wide enough to fill the GPU with one workgroup per
        // (group, 64-chain tile): half the partial traffic; one workgroup per sub-range below
        // that, where a step's latency is what counts
        const int fold = (int64_t)q.nbound * A.nv * nh >= MMB_LG_FOLD_MIN ? 1 : 0;
        hipError_t st = mmb_lg_launch_grad(A, par, q.nbound, fold, q.st);
        if (st != hipSuccess) return fail(e, MMB_E_HIP, "lg_grad launch: %s", hipGetErrorString(st));
        if (a->time_kernels) HIPCHK(e, hipEventRecord(ev[2 * s + 1], q.st));
        st = mmb_lg_launch_ctl(A, 0, par ^ 1, q.nbound, fold, q.st);
        if (st != hipSuccess) return fail(e, MMB_E_HIP, "lg_ctl launch: %s", hipGetErrorString(st));
        q.s = s + 1;
        if (q.s % LG_CHECK == 0) {
          // two readbacks in flight: wait for the one issued LG_CHECK steps ago, so the
          // stream still holds LG_CHECK queued steps while the host decides (the count is
          // non-increasing, so the older value is still a bound on the running chains)
          const int j = (int)((q.s / LG_CHECK) & 1);
          int32_t* hc = e->lg_hcount + 2 * i;
          hipEvent_t* cev = e->lg_cev + 2 * i;
          HIPCHK(e, hipMemcpyAsync(hc + j, A.count + (q.s & 1), sizeof(int32_t), hipMemcpyDeviceToHost, q.st));
          HIPCHK(e, hipEventRecord(cev[j], q.st));
          const int jw = q.s >= 2 * LG_CHECK ? j ^ 1 : j;  // the first check waits for its own copy
          HIPCHK(e, hipEventSynchronize(cev[jw]));         // (short windows end without surplus)
          if (hc[jw] == 0) {
            q.done = true;
            --live;
          } else {
            q.nbound = hc[jw];
          }
        }
        if (q.s > cap) return fail(e, MMB_E_STATE, "logistic window did not terminate");
      }
    }
    for (int i = 1; i < nh; ++i) {  // join: later work on the engine stream sees every part's results
      HIPCHK(e, hipEventRecord(e->lg_join[i], H[i].st));
      HIPCHK(e, hipStreamWaitEvent(e->stream, e->lg_join[i], 0));
    }
    drain.armed = false;  // joined: the engine stream orders everything after the parts
    int64_t steps = 0;
    for (int i = 0; i < nh; ++i) steps = std::max(steps, H[i].s);
    e->lg_steps = steps;
    if (a->time_kernels) {
      // summed gradient-kernel durations of all parts (they may overlap in time)
      for (int i = 0; i < nh; ++i) {
        HIPCHK(e, hipStreamSynchronize(H[i].st));
        for (int64_t t = 0; t < H[i].s; ++t) {
          float ms = 0.f;
          HIPCHK(e, hipEventElapsedTime(&ms, (*H[i].ev)[2 * t], (*H[i].ev)[2 * t + 1]));
          e->kernel_ms += ms;
        }
      }
    }
    e->launches = 0;
    for (int i = 0; i < nh; ++i) e->launches += H[i].s;
    e->units = a->iters * e->K;
  }
  e->iter += a->iters;
  e->n_kept = want ? nk : 0;
  if (a->draws && nk > 0) {
    std::vector<double> hd((size_t)nk * e->pmon * e->K);
    HIPCHK(e, hipMemcpyAsync(hd.data(), e->d_draws, hd.size() * sizeof(double), hipMemcpyDeviceToHost,
                             e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int64_t i = 0; i < nk; ++i)
      for (int j = 0; j < e->pmon; ++j)
        for (int64_t k = 0; k < e->K; ++k)
          a->draws[i + nk * (j + (int64_t)e->pmon * k)] = hd[(i * e->pmon + j) * e->K + k];
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

int mmb_run(mmb_engine* e, const mmb_run_args* a) {
  if (!e || !a) return fail(e, MMB_E_ARG, "null argument");
  if (!e->d_vals) return fail(e, MMB_E_STATE, "mmb_init_chains not called");
  if (a->iters < 0 || a->thin < 1 || a->burnin < 0)
    return fail(e, MMB_E_ARG, "iters >= 0, thin >= 1, burnin >= 0 required");
  if (e->iter + a->iters > 0xffffffffLL) return fail(e, MMB_E_ARG, "iteration counter overflow");
  HIPCHK(e, hipSetDevice(e->device));
  const int64_t it0 = e->iter;
  const int64_t kept0 = kept_upto(it0, a->burnin, a->thin);
  const int64_t nk = kept_upto(it0 + a->iters, a->burnin, a->thin) - kept0;
  const bool want = (a->draws != nullptr) || a->keep_device;
  if (want && nk > 0) {
    size_t need = (size_t)nk * e->pmon * e->K;
    if (need > e->draws_cap) {
      e->draws_cap = 0;
      HIPCHK(e, e->d_draws.alloc(need));
      e->draws_cap = need;
    }
  }
  if (e->model == MMB_MODEL_LOGISTIC) return run_logistic(e, a, (want && nk > 0) ? e->d_draws.get() : nullptr, kept0, nk, want);
  if (a->iters > 0 && !e->order_fresh) {  // else computed right after a previous window
    int orc = order_chains(e);
    if (orc) return orc;
    e->order_iter = it0;
  }
  SweepArgs A;
  fill_args(e, A);
  A.burnin = a->burnin;
  A.thin = a->thin;
  A.model_burnin = a->model_burnin;
  A.kept_origin = kept0;
  A.draws = (want && nk > 0) ? e->d_draws.get() : nullptr;
  int np = 1;
  {
    int rc = sweep_parts(e, A, &np);
    if (rc) return rc;
  }
  const int W = iters_per_launch(e, np, a->iters);
  e->kernel_ms = 0.0;
  e->launches = 0;
  e->units = 0;
  const int64_t nl = a->iters > 0 ? (a->iters + W - 1) / W : 0;
  hipStream_t pst[MMB_SWEEP_PARTS_MAX];
  std::vector<hipEvent_t>* pev[MMB_SWEEP_PARTS_MAX];
  for (int p = 0; p < np; ++p) {
    if (p > 0 && !e->sw_streamx[p - 1])
      HIPCHK(e, hipStreamCreateWithFlags(&e->sw_streamx[p - 1], hipStreamNonBlocking));
    pst[p] = p == 0 ? e->stream : e->sw_streamx[p - 1];
    pev[p] = p == 0 ? &e->evpool : &e->sw_evpoolx[p - 1];
    if (a->time_kernels) {
      while ((int64_t)pev[p]->size() < 2 * nl) {
        hipEvent_t ev;
        HIPCHK(e, hipEventCreate(&ev));
        pev[p]->push_back(ev);
      }
    }
  }
  if (np > 1)
    for (int p = 0; p < np; ++p)
      if (!e->sw_join[p]) HIPCHK(e, hipEventCreateWithFlags(&e->sw_join[p], hipEventDisableTiming));
  // every return from here on -- the error paths included -- leaves no part kernel running: the
  // engine stream alone orders whatever the caller does next
  struct PartDrain {
    hipStream_t* st;
    int n;
    bool armed = true;
    ~PartDrain() {
      if (armed)
        for (int p = 1; p < n; ++p) (void)hipStreamSynchronize(st[p]);
    }
  } drain{pst, np};
#ifdef MMB_WAVE_TIMES
  if (nl > 0) mmb_wave_times_reset(e->stream);
#endif
  if (np > 1 && nl > 0) {  // fork: the part streams start behind everything queued on the engine stream
    HIPCHK(e, hipEventRecord(e->sw_join[0], e->stream));
    for (int p = 1; p < np; ++p) HIPCHK(e, hipStreamWaitEvent(pst[p], e->sw_join[0], 0));
  }
  for (int64_t done = 0, li = 0, w = 0; done < a->iters; done += w, ++li) {
    w = launch_width(a->iters, W, li);
    A.iter0 = it0 + done;
    A.n_iters = w;
    // launch li of every part: part p holds workgroups p, p + np, ... of the one slot -> chain
    // table (the same class mix in every part), and its launch li + 1 waits for its own launch li only
    for (int p = 0; p < np; ++p) {
      A.wg_offset = p;
      A.wg_stride = np;
      if (a->time_kernels) HIPCHK(e, hipEventRecord((*pev[p])[2 * li], pst[p]));
      hipError_t st;
      if (e->jit_fn) {  // node IR, specialised kernel: the interpreter's launch shape (4 chains / 128 threads)
        const int per_block = 128 / Mdl<MMB_MODEL_IR>::G;
        const int nwg = (A.K + per_block - 1) / per_block;
        const unsigned grid = (unsigned)((nwg - p + np - 1) / np);
        const size_t lds = (size_t)per_block * Mdl<MMB_MODEL_IR>::lds_stride(A) * sizeof(double);
        void* args[] = {(void*)&A};
        st = hipModuleLaunchKernel(e->jit_fn, grid, 1, 1, 128, 1, 1, (unsigned)lds, pst[p], args, nullptr);
      } else {
        st = mmb_launch_sweep(e->model, e->kinds, A, pst[p]);
      }
      if (st != hipSuccess) return fail(e, MMB_E_HIP, "sweep launch: %s", hipGetErrorString(st));
      if (a->time_kernels) HIPCHK(e, hipEventRecord((*pev[p])[2 * li + 1], pst[p]));
      e->launches += 1;
    }
    e->units += (int64_t)w * e->K;
  }
  if (np > 1 && nl > 0) {  // join: later work on the engine stream sees every part's results
    for (int p = 1; p < np; ++p) {
      HIPCHK(e, hipEventRecord(e->sw_join[p], pst[p]));
      HIPCHK(e, hipStreamWaitEvent(e->stream, e->sw_join[p], 0));
    }
  }
  drain.armed = false;  // joined: the engine stream orders everything after the parts
  if (a->iters > 0 && (!e->order_fresh || it0 + a->iters - e->order_iter >= order_every())) {
    // the next window's order from this window's final flags, queued behind its last launch so
    // it runs while the host is between windows (a host write of the tune state invalidates it).
    // The classes persist -- a chain's factor-valid flag is set by its first full-rank update and
    // kept -- so a table less than MMB_ORDER_EVERY iterations old is kept: any table gives the
    // same results, only the pairing could lag a class change (the kernel is ~21 us, ~1 % of a
    // 20-iteration window)
    int orc = order_chains(e);
    if (orc) return orc;
    e->order_fresh = true;
    e->order_iter = it0 + a->iters;
  }
  if (a->time_kernels && nl > 0) {
    // device time of the window's launches, read after the window (no per-launch sync): the time
    // during which at least one launch was in flight.  One part's launches follow each other on
    // their stream, so that is their sum; launches of different parts overlap (their sum could
    // exceed the wall time), so it is the union of the [start, end] intervals on the clock of the
    // window's first event.
    std::vector<std::pair<float, float>> iv;
    for (int p = 0; p < np; ++p) {
      HIPCHK(e, hipEventSynchronize((*pev[p])[2 * nl - 1]));
      for (int64_t li = 0; li < nl; ++li) {
        float t0 = 0.f, dt = 0.f;
        HIPCHK(e, hipEventElapsedTime(&dt, (*pev[p])[2 * li], (*pev[p])[2 * li + 1]));
        if (np == 1) {
          e->kernel_ms += dt;
          continue;
        }
        if (p > 0 || li > 0) HIPCHK(e, hipEventElapsedTime(&t0, (*pev[0])[0], (*pev[p])[2 * li]));
        iv.emplace_back(t0, t0 + dt);
      }
    }
    std::sort(iv.begin(), iv.end());
    for (size_t i = 0; i < iv.size();) {
      float hi = iv[i].second;
      size_t j = i + 1;
      for (; j < iv.size() && iv[j].first <= hi; ++j) hi = std::max(hi, iv[j].second);
      e->kernel_ms += hi - iv[i].first;
      i = j;
    }
  }
  e->iter = it0 + a->iters;
  e->n_kept = want ? nk : 0;
  if ((e->kinds & (1u << MMB_SAMPLER_SLICE)) && a->iters > 0) {
    unsigned long long ov = 0;
    HIPCHK(e, hipMemcpyAsync(&ov, e->d_nstat + 3, sizeof ov, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (ov != e->slice_overflows) {
      const unsigned long long n = ov - e->slice_overflows;
      e->slice_overflows = ov;
      return fail(e, MMB_E_STATE, "Slice: %llu update(s) in iterations %lld..%lld still rejected after %d shrink "
                  "steps (the reference would loop forever; check the widths and the target's support)",
                  n, (long long)it0 + 1, (long long)e->iter, MMB_SLICE_MAX_SHRINK);
    }
  }
  if (a->draws && nk > 0) {
    std::vector<double> h((size_t)nk * e->pmon * e->K);
    HIPCHK(e, hipMemcpyAsync(h.data(), e->d_draws, h.size() * sizeof(double), hipMemcpyDeviceToHost,
                             e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    // Mamba Chains value: n x p x m, column-major (iteration fastest)
    for (int64_t i = 0; i < nk; ++i)
      for (int j = 0; j < e->pmon; ++j)
        for (int64_t k = 0; k < e->K; ++k)
          a->draws[i + nk * (j + (int64_t)e->pmon * k)] = h[(i * e->pmon + j) * e->K + k];
  }
  return 0;
}

int mmb_reserve_draws(mmb_engine* e, int64_t nkept) {
  if (!e || nkept < 0) return fail(e, MMB_E_ARG, "null engine or nkept < 0");
  if (!e->d_vals) return fail(e, MMB_E_STATE, "mmb_init_chains not called");
  const size_t need = (size_t)nkept * e->pmon * e->K;
  if (need > e->draws_cap) {
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // the old buffer may still be read by a kernel
    e->draws_cap = 0;
    e->n_kept = 0;  // the kept draws (if any) went with the old buffer
    HIPCHK(e, e->d_draws.alloc(need));
    e->draws_cap = need;
  }
  return 0;
}

int mmb_get_draws(mmb_engine* e, double* draws) {
  if (!e || !draws) return fail(e, MMB_E_ARG, "null argument");
  const int64_t nk = e->n_kept;
  if (nk == 0) return 0;
  std::vector<double> h((size_t)nk * e->pmon * e->K);
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipMemcpy(h.data(), e->d_draws, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < nk; ++i)
    for (int j = 0; j < e->pmon; ++j)
      for (int64_t k = 0; k < e->K; ++k)
        draws[i + nk * (j + (int64_t)e->pmon * k)] = h[(i * e->pmon + j) * e->K + k];
  return 0;
}

int mmb_set_draws(mmb_engine* e, const double* draws, int64_t nkept) {
  if (!e || !draws) return fail(e, MMB_E_ARG, "null argument");
  if (nkept < 1) return fail(e, MMB_E_ARG, "nkept must be >= 1");
  const int rc = mmb_reserve_draws(e, nkept);   // mmb_init_chains called; grows the buffer
  if (rc != 0) return rc;
  // Chains value (n x p x m column-major) -> device layout draws[(i*p + j)*K + k]
  std::vector<double> h((size_t)nkept * e->pmon * e->K);
  for (int64_t k = 0; k < e->K; ++k)
    for (int j = 0; j < e->pmon; ++j)
      for (int64_t i = 0; i < nkept; ++i)
        h[(i * e->pmon + j) * e->K + k] = draws[i + nkept * (j + (int64_t)e->pmon * k)];
  HIPCHK(e, hipSetDevice(e->device));
  e->n_kept = 0;
  HIPCHK(e, hipMemcpyAsync(e->d_draws, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->n_kept = nkept;
  return 0;
}

// ---------------------------------------------------------------- timing
int mmb_sync(mmb_engine* e) {
  if (!e) return fail(e, MMB_E_ARG, "null argument");
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

int mmb_kernel_time(const mmb_engine* e, double* total_ms, int64_t* launches, int64_t* units) {
  if (!e) return MMB_E_ARG;
  if (total_ms) *total_ms = e->kernel_ms;
  if (launches) *launches = e->launches;
  if (units) *units = e->units;
  return 0;
}

// Algorithmic HBM bytes per chain-update (B = 2*S_state + S_draw/thin is
// reported by bench.py; this returns 2*S_state with the minimal state: FP64 values,
// packed symmetric matrices, int32 counters, one byte per pivot index).
int mmb_state_bytes(const mmb_engine* e, double* bytes) {
  if (!e || !bytes) return MMB_E_ARG;
  double s = 8.0 * e->P;
  for (auto& h : e->blocks) {
    switch (h.spec.sampler) {
      case MMB_SAMPLER_AMWG: s += 8.0 * h.d * 2 + 4.0 * h.d * 0 + 4.0; break;  // sigma, accept, m
      case MMB_SAMPLER_AMM: s += 8.0 * (h.d + 2.0 * h.T) + 1.0 * h.d + 4.0; break;  // Mv, Mvv, L, piv, m
      case MMB_SAMPLER_NUTS: s += 8.0 * 7 + 4.0; break;
      case MMB_SAMPLER_HMC: s += 8.0 * 2; break;   // epsilon, L (read only)
      case MMB_SAMPLER_MALA: s += 8.0; break;
      case MMB_SAMPLER_RWM: s += 8.0 * h.d; break;  // scale (read only)
      case MMB_SAMPLER_DGS: break;  // no tune state; the masses stay in registers (samplers.h dgs)
      case MMB_SAMPLER_SLICESIMPLEX: break;  // no tune state; the vertex matrix lives in LDS within one update
      case MMB_SAMPLER_BIA: s += 8.0 * h.d * 2 + 4.0; break;  // A, D, iter
      case MMB_SAMPLER_BHMC: s += 8.0 * h.d * 2 + 8.0 * 2 + 4.0; break;  // position, velocity, the counters, initialised
      case MMB_SAMPLER_ABC: s += 8.0 * h.d + 8.0 * h.tune_len; break;     // scale, the tune row
      case MMB_SAMPLER_BMG:
      case MMB_SAMPLER_BMC3: break;  // no tune state
      default: break;
    }
  }
  *bytes = 2.0 * s;
  return 0;
}


// the engine's counter words (d_nstat, zeros before mmb_init_chains): NUTS {updates, depth-cap hits,
// depth sum}, [3] Slice overflows, [5] the AMWG count
static int nstat_read(mmb_engine* e, unsigned long long (&v)[8]) {
  std::memset(v, 0, sizeof v);
  if (!e->d_nstat) return 0;
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipMemcpyAsync(v, e->d_nstat, sizeof v, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

int mmb_nuts_stats(mmb_engine* e, int64_t* out) {
  if (!e || !out) return fail(e, MMB_E_ARG, "null argument");
  unsigned long long v[8];
  if (int rc = nstat_read(e, v)) return rc;
  for (int i = 0; i < 3; ++i) out[i] = (int64_t)v[i];
  return 0;
}

int mmb_amwg_stats(mmb_engine* e, int64_t* out) {
  if (!e || !out) return fail(e, MMB_E_ARG, "null argument");
  unsigned long long v[8];
  if (int rc = nstat_read(e, v)) return rc;
  out[0] = (int64_t)v[5];
  return 0;
}

// out[b * width + i]: the first `width` words of block b's astat rows summed over the chains, for the
// blocks of sampler `kind` (RWM: and the BMG, BMC3, BIA, BHMC and ABC blocks, which count updates and accepts alike)
static int astat_sums(mmb_engine* e, int kind, int width, int64_t* out) {
  if (!e || !out) return fail(e, MMB_E_ARG, "null argument");
  for (int i = 0; i < MMB_MAX_BLOCKS * width; ++i) out[i] = 0;
  if (e->K == 0) return 0;
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  std::vector<uint64_t> h;
  for (size_t b = 0; b < e->blocks.size(); ++b) {
    const int bk = e->blocks[b].spec.sampler;
    if (!e->blocks[b].astat || !(bk == kind || (kind == MMB_SAMPLER_RWM && (binary_kind(bk) || bk == MMB_SAMPLER_ABC)))) continue;
    int rc = d2h(e, h, e->blocks[b].astat, (size_t)e->K * MMB_AMM_STAT_STRIDE);
    if (rc) return rc;
    for (int64_t k = 0; k < e->K; ++k)
      for (int i = 0; i < width; ++i) out[b * width + i] += (int64_t)h[k * MMB_AMM_STAT_STRIDE + i];
  }
  return 0;
}

int mmb_amm_stats(mmb_engine* e, int64_t* out) { return astat_sums(e, MMB_SAMPLER_AMM, MMB_AMM_STATS, out); }
int mmb_rwm_stats(mmb_engine* e, int64_t* out) { return astat_sums(e, MMB_SAMPLER_RWM, 2, out); }

int mmb_chain_order(mmb_engine* e, int32_t* slot_to_chain) {
  if (!e || !slot_to_chain) return fail(e, MMB_E_ARG, "null argument");
  if (e->K == 0) return 0;
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (e->cperm_identity || !e->d_cperm) {
    for (int64_t k = 0; k < e->K; ++k) slot_to_chain[k] = (int32_t)k;
    return 0;
  }
  HIPCHK(e, hipMemcpy(slot_to_chain, e->d_cperm, (size_t)e->K * sizeof(int32_t), hipMemcpyDeviceToHost));
  return 0;
}

int mmb_debug_pchol(int device, int64_t n, int d, const double* S, double* L, int32_t* pos, int32_t* info) {
  if (n < 1 || d < 1 || d > 30 || !S || !L || !pos || !info)
    return fail(nullptr, MMB_E_ARG, "mmb_debug_pchol: n >= 1, 1 <= d <= 30 and non-null buffers required");
  constexpr int TP = 480;
  // the caller's current device is restored on return, and the probe runs on a private stream
  // (no device-wide synchronisation of whatever else the caller has queued)
  int dev0 = 0;
  hipError_t st = hipGetDevice(&dev0);
  if (st == hipSuccess) st = hipSetDevice(device);
  if (st == hipSuccess) {  // (the buffers go before the caller's device is restored)
    DevBuf<double> dS, dL;
    DevBuf<int32_t> dpos, dinfo;
    hipStream_t ps = nullptr;
    st = hipStreamCreateWithFlags(&ps, hipStreamNonBlocking);
    if (st == hipSuccess) st = dS.alloc((size_t)n * TP);
    if (st == hipSuccess) st = dL.alloc((size_t)n * TP);
    if (st == hipSuccess) st = dpos.alloc((size_t)n * 32);
    if (st == hipSuccess) st = dinfo.alloc((size_t)n * 2);
    if (st == hipSuccess) st = hipMemcpyAsync(dS, S, (size_t)n * TP * sizeof(double), hipMemcpyHostToDevice, ps);
    if (st == hipSuccess) st = hipMemsetAsync(dL, 0, (size_t)n * TP * sizeof(double), ps);
    if (st == hipSuccess) st = mmb_launch_pchol_probe((int)n, d, dS, dL, dpos, dinfo, ps);
    if (st == hipSuccess) st = hipMemcpyAsync(L, dL, (size_t)n * TP * sizeof(double), hipMemcpyDeviceToHost, ps);
    if (st == hipSuccess) st = hipMemcpyAsync(pos, dpos, (size_t)n * 32 * sizeof(int32_t), hipMemcpyDeviceToHost, ps);
    if (st == hipSuccess) st = hipMemcpyAsync(info, dinfo, (size_t)n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ps);
    if (st == hipSuccess) st = hipStreamSynchronize(ps);
    if (ps) {
      (void)hipStreamSynchronize(ps);  // (an error path: nothing in flight may use the buffers)
      (void)hipStreamDestroy(ps);
    }
  }
  (void)hipSetDevice(dev0);
  if (st != hipSuccess) return fail(nullptr, MMB_E_HIP, "mmb_debug_pchol: %s", hipGetErrorString(st));
  return 0;
}

int mmb_grad_evals(mmb_engine* e, int64_t* n) {
  if (!e || !n) return fail(e, MMB_E_ARG, "null argument");
  *n = 0;
  if (e->model != MMB_MODEL_LOGISTIC || !e->lg_ngrad) return 0;
  unsigned long long v = 0;
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipMemcpyAsync(&v, e->lg_ngrad, sizeof v, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  *n = (int64_t)v;
  return 0;
}
