// engine.h — what the host units of libmambahip.so share: the engine's state and its helpers.
//
//   engine.cpp       lifecycle, data, values, mmb_init_chains, the window runners (mmb_run), draws, getters
//   engine_ir.cpp    node IR: validation, expression fusing, separable AMWG tables, the specialised kernel
//   engine_tune.cpp  the canonical tune row (mmb_get_tune / mmb_set_tune)
//   engine_post.cpp  everything computed on the device-kept draws
//   engine_comm.cpp  the RCCL collective
//
// Comments in the kernel headers that say engine.cpp mean the engine_*.cpp units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device.h"
#include "models.h"
#include "nuts.h"
#include "logistic.h"
#include "ir.h"
#include "ir_jit.h"
#include "devbuf.h"
#include "launch.h"

// chain parts of a sweep window (mmb_run): the engine stream and three more, as many streams as a
// process has hardware queues by default (streams that share a queue serialise)
constexpr int MMB_SWEEP_PARTS_MAX = 4;

// A block's per-chain device state: allocated by mmb_init_chains, dropped as one group by the next
// mmb_init_chains and by mmb_destroy (free_dev)
struct BlockChainBufs {
  DevBuf<double> sigma, accept, Mv, Mvv, Ls;
  // AMM second moment buffers (32-lane kernels that carry proposals; DBlock::t_Mv_alt): chain k's
  // current Mv / Mvv are in these when its m is odd.  Null: one buffer
  DevBuf<double> Mv_alt, Mvv_alt;
  DevBuf<double> nuts, nfr, width, sigl_d;
  DevBuf<double> hmc;  // HMC/MALA [K][2] epsilon, L; ABC [K][tune_len] the canonical tune row
  DevBuf<int32_t> m, flags;
  DevBuf<uint8_t> piv;
  DevBuf<double> xnext;    // AMM carried next proposal [K][DP] (samplers.h amm)
  DevBuf<int64_t> xtag;    // AMM [K] tag of the carried proposal
  DevBuf<uint64_t> astat;  // AMM [K][MMB_AMM_STAT_STRIDE] factorization counters (mmb_amm_stats);
                           // RWM, BMG, BMC3, BIA, BHMC, ABC: the same rows, [0] updates, [1] accepts (mmb_rwm_stats)
};

struct BlockHost : BlockChainBufs {
  mmb_block_spec spec;
  std::vector<double> tuning;
  int d = 0, T = 0, tune_len = 0;
  std::vector<double> sigl;  // AMM chol(Sigma) lower row-major
  bool sigl_diag = false;
  DevBuf<int32_t> sep_d;  // node-IR AMWG: coordinate -> element-term table (ir_sep_table), engine lifetime;
                          // ABC: the block's table (abc_tab)
  double sep_eps = 0.0;
  std::vector<int32_t> abc_tab;  // ABC: [T, ns, nd, codes[ns], then per data node (node id, first statistic)]
};

// The engine's per-chain device state: dropped as one group like the blocks' (free_dev)
struct ChainBufs {
  DevBuf<double> d_vals;
  DevBuf<DBlock> d_blocks;
  // logistic (config 4): the NUTS machine state (logistic.h)
  DevBuf<double> lg_vec, lg_sc, lg_frames, lg_pos, lg_gpart, lg_lpart;
  DevBuf<int32_t> lg_iv, lg_count, lg_s2c;
  DevBuf<int64_t> lg_itc;
  DevBuf<unsigned long long> lg_ngrad;
  DevBuf<int32_t> d_cperm;  // lane-group slot -> chain of the 32-lane sweep kernels (order_chains)
  DevBuf<unsigned long long> d_nstat;  // NUTS {updates, depth-cap hits, depth sum}, Slice overflows
                                       // since init_chains
  DevBuf<double> d_draws;  // draws of the last window (draws_cap doubles)
};

// Device state that lives as long as the engine (mmb_destroy drops the group)
struct EngineBufs {
  DevBuf<double> d_data;
  DevBuf<double> lg_X, lg_y;  // logistic: padded X/y
  DevBuf<int32_t, true> lg_hcount;  // pinned: the request-count readbacks (run_logistic)
  // hpd tails (mmb_hpd_*): keys of the draws below / above the thresholds, a sort buffer as large and
  // the sort's tile histograms, all for hpd_cap keys; grown on demand
  DevBuf<uint64_t> hpd_below, hpd_above, hpd_tmp;
  DevBuf<unsigned int> hpd_tilehist;
  DevBuf<unsigned long long> hpd_words;  // meta, ghist, gap partials and result (HPD_WORDS)
  // node IR (MMB_MODEL_IR): device tables of the lowered model
  DevBuf<mmb_ir_node> d_ir_nodes;
  DevBuf<int32_t> d_ir_code, d_ir_mon;
  DevBuf<double> d_ir_const, d_ir_pool;
  DevBuf<mmb_ir_block> d_ir_blocks;
};

struct mmb_engine : ChainBufs, EngineBufs {
  mmb_model_spec spec{};
  int device = 0;
  hipStream_t stream = nullptr;
  int model = 0;
  int P = 0, pmon = 0, VS = 0, DP = 0, TP = 0;
  std::vector<BlockHost> blocks;
  unsigned kinds = 0;  // bitmask of sampler kinds in the scheme
  // data
  std::vector<double> x, y, X;
  bool have_data = false;
  // chains
  int64_t K = 0, chain_offset = 0;
  uint64_t seed = 0;
  int64_t iter = 0;
  // logistic (config 4)
  int lg_N = 0, lg_p = 0, lg_rps = 0;
  bool lg_fd = false;  // forward-difference gradient (MMB_GRAD_FORWARD): p + 1 columns per request
  hipEvent_t lg_cev[2 * MMB_LG_SPLIT_MAX] = {};  // request-count readbacks in flight, 2 per part (run_logistic)
  hipStream_t lg_streamx[MMB_LG_SPLIT_MAX - 1] = {};   // the streams of parts 1.. (part 0: the engine stream)
  hipEvent_t lg_join[MMB_LG_SPLIT_MAX] = {};          // fork / join of the streams
  std::vector<hipEvent_t> evpoolx[MMB_LG_SPLIT_MAX - 1];  // kernel timing events of parts 1..
  int64_t lg_steps = 0;  // gradient steps of the last window
  // sweep parts (mmb_run): the streams of parts 1.. (part 0: the engine stream), created on first use
  hipStream_t sw_streamx[MMB_SWEEP_PARTS_MAX - 1] = {};
  hipEvent_t sw_join[MMB_SWEEP_PARTS_MAX] = {};           // [0] fork, [i] join of part i
  std::vector<hipEvent_t> sw_evpoolx[MMB_SWEEP_PARTS_MAX - 1];  // kernel timing events of parts 1..
  int sw_resident = 0;  // workgroups of the sweep kernel the device holds at once (0: not asked yet)
  bool cperm_identity = true;
  bool order_fresh = false;    // d_cperm holds a table computed after a window (a host write of the
                               // tune state clears it)
  int64_t order_iter = 0;      // the iteration whose flags d_cperm was computed from
  unsigned long long slice_overflows = 0;  // d_nstat[3] as last reported by mmb_run
  int64_t xepoch = 0;  // bumped by every host write of chain state: invalidates carried AMM proposals
  // draws of the last window
  size_t draws_cap = 0;
  int64_t n_kept = 0;
  // hpd tails (mmb_hpd_*)
  int64_t hpd_cap = 0;
  int64_t hpd_n[2] = {0, 0};                // keys held: below, above
  uint64_t hpd_varying[2] = {0, 0};         // bits in which each buffer's keys differ (sort passes to run)
  bool hpd_have = false, hpd_sorted = false;
  // node IR (MMB_MODEL_IR): host copies of the lowered model
  std::vector<mmb_ir_node> ir_nodes;
  std::vector<int32_t> ir_code, ir_mon;
  std::vector<double> ir_const, ir_pool;
  std::vector<mmb_ir_block> ir_blocks;
  int ir_stack = 0;
  // node IR specialised kernel (ir_jit.cpp): null when the interpreter kernel runs
  hipModule_t jit_mod = nullptr;
  hipFunction_t jit_fn = nullptr;
  bool ir_noprop = false;  // specialised AMM + Gibbs kernel: no candidate copy of the state (ir.h NOPROP)
  int ir_stack_dbl = 0;    // specialised kernel's expression-stack LDS doubles
  int ssx_kmax = 0;        // elements of the widest SliceSimplex block (0: none)
  std::string jit_info;
  // timing
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> evpool;  // 2 per launch when time_kernels
  double kernel_ms = 0.0;
  int64_t launches = 0, units = 0;
  std::string err;
};

#pragma GCC visibility push(hidden)  // shared by the units, not exported

extern thread_local std::string g_last_error;  // engine.cpp

// records the message (mmb_last_error) and returns `code`
int fail(mmb_engine* e, int code, const char* fmt, ...);

#define HIPCHK(e, call)                                                                  \
  do {                                                                                   \
    hipError_t _st = (call);                                                             \
    if (_st != hipSuccess)                                                               \
      return fail((e), MMB_E_HIP, "%s failed: %s", #call, hipGetErrorString(_st));       \
  } while (0)

template <class T>
static int d2h(mmb_engine* e, std::vector<T>& h, const DevBuf<T>& d, size_t n) {
  h.resize(n);
  HIPCHK(e, hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return 0;
}
template <class T>
static int h2d(mmb_engine* e, const DevBuf<T>& d, const std::vector<T>& h) {
  HIPCHK(e, hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

static inline int tri(int i) { return i * (i + 1) / 2; }

// families a DGS block may sample (dgs.jl:6-8 DGSUnivariateDistribution, without the hypergeometrics)
static inline bool ir_dgs_family(int fam) {
  return fam == MMB_IR_BINOMIAL || fam == MMB_IR_BERNOULLI || fam == MMB_IR_CATEGORICAL ||
         fam == MMB_IR_DISCRETEUNIFORM;
}

// the binary samplers (bmg.jl, bmc3.jl, bia.jl, bhmc.jl) and the nodes they may sample: Bernoulli, DiscreteUniform(0, 1)
static inline bool binary_kind(int kind) {
  return kind == MMB_SAMPLER_BMG || kind == MMB_SAMPLER_BMC3 || kind == MMB_SAMPLER_BIA || kind == MMB_SAMPLER_BHMC;
}
static inline const char* binary_name(int kind) {
  return kind == MMB_SAMPLER_BMG ? "BMG" : kind == MMB_SAMPLER_BMC3 ? "BMC3" : kind == MMB_SAMPLER_BIA ? "BIA" : "BHMC";
}
static inline bool ir_binary_node(const mmb_ir_node& n) {
  return n.family == MMB_IR_BERNOULLI || (n.family == MMB_IR_DISCRETEUNIFORM && n.lo == 0.0 && n.hi == 1.0);
}

// the 32-lane kernels keep the AMM factor in position form on the device (engine_tune.cpp)
static inline bool amm_posform(const mmb_engine* e) { return e->model == MMB_MODEL_RATS || e->model == MMB_MODEL_IR; }

// engine.cpp
int node_dim(const mmb_model_spec& s, const mmb_ir_model* ir, int node, bool* positive);
int create_impl(const mmb_model_spec* spec, const mmb_ir_model* ir, int device, mmb_engine** out);
void fill_args(const mmb_engine* e, SweepArgs& A);

// engine_ir.cpp
void ir_expr_slots(const std::vector<int32_t>& code, const std::vector<double>& pool, int pc, int i,
                   std::vector<int>& slots, bool* dyn = nullptr);
bool ir_sep_table(const std::vector<mmb_ir_node>& nodes, const std::vector<int32_t>& code,
                  const std::vector<double>& pool, const mmb_ir_block& IB, const mmb_block_spec& s,
                  int nvalues, std::vector<int32_t>& tab, double* epsf);
void ir_fuse(const std::vector<int32_t>& code, std::vector<mmb_ir_node>& nodes,
             std::vector<mmb_ir_block>& blocks, std::vector<int32_t>& out);
int ir_state_len(const mmb_model_spec* spec, const mmb_ir_model* ir);

// engine_tune.cpp
int tune_len_of(int kind, int d, int nsim = 0, int nstat = 0);

// engine_post.cpp
int gr_width_check(mmb_engine* e);

#pragma GCC visibility pop
