// modelstats.hip — model log densities of the device-kept draws.
//
// logpdf(mc, nodekeys) (src/output/modelstats.jl:30-68) relists every kept draw into the model
// and sums logpdf(m[key]) over the node list (mapreduce(+), modelstats.jl:63: a plain sum in list
// order, no early exit, sampled nodes untransformed); dic (modelstats.jl:3-12) needs the mean and
// the variance of D = -2 lp over all draws and the density at the posterior means
// (modelstats.jl:15-25).  Here, for kept row i and local chain k:
//
//   lp[i*K + k] = sum over the node list of logpdf(node | the draw's values)
//
// ms_ir_kernel (node-IR models): the interpreter's ev / node_lp (ir.h) on the draw instead of the
//   chain state, so a node's term has the bits the sweep kernel computes for the same state.  The
//   draw buffer is draws[(i*pmon + j)*K + k], chain fastest: one chain's row is a stride-K gather,
//   so a workgroup takes a TILE of T consecutive chains of one row at a time.  Its 128 threads
//   load the columns the requested nodes read (`col`: monitored column -> `slot`: state slot; T
//   consecutive chains of one column are T*8 contiguous bytes) and write them transposed into T
//   per-chain state images in LDS (stride S doubles, S odd: the transposed writes of one column
//   spread over the banks).  The four 32-lane groups then evaluate the tile's chains one after
//   another (group g: chains g, g + 4, ...), vals = the chain's image, each group with an
//   expression stack of its own.  Chains past K are loaded as chain K - 1 and not stored: every
//   group makes the same trips (the butterflies and wave barriers need all lanes).
//   LDS per workgroup = (T*S + 4*(stack + 1)*32) doubles; the host picks T = 32, 16 or 8 as the
//   largest that keeps it within MS_LDS_BYTES (64 KiB: two workgroups per CU stay resident, and
//   no opt-in for a larger dynamic allocation is needed).  The launch arguments and the load phase are
//   in modelstats.h: predict.hip tiles the same way.
//
// ms_line_kernel (hand-lowered line): one thread per (row, chain), three coalesced loads; terms
//   y = Mdl<line>::ylp, beta = the prior as Mdl<line>::logf forms it, s2 = d_iglogpdf(ig_c, s2, 0).
//
// ms_deviance_kernel: per chain, [sum_i (D - c), sum_i (D - c)^2] with D = -2 lp, in row order,
//   continued over row chunks (the n x K values stay on the device; non-finite values propagate).
#include "modelstats.h"
#include "launch.h"

#define MS_DEV_THREADS 64   // deviance reduction: one wavefront per workgroup spreads few chains over the CUs
#define MS_DEV_ROWS 16      // its loads in flight per thread

// LDS doubles of a workgroup with a tile of T chains
static size_t ms_lds_doubles(int T, int S, int stack) { return (size_t)T * S + (size_t)MS_GROUPS * (stack + 1) * 32; }

__global__ __launch_bounds__(MS_THREADS) void ms_ir_kernel(const SweepArgs A, const MsArgs M) {
  extern __shared__ double ms_lds[];
  using MI = Mdl<MMB_MODEL_IR>;
  const int t = (int)threadIdx.x;
  const int grp = t >> 5;
  const Grp<32> g;
  double* img = ms_lds;
  double* stk = ms_lds + (size_t)M.T * M.S + (size_t)grp * (M.stack + 1) * 32;
  const int T = M.T;
  const int64_t ktiles = ((int64_t)M.K + T - 1) / T;
  const int64_t ntiles = M.n * ktiles;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t i = tile / ktiles;
    const int64_t k0 = (tile - i * ktiles) * T;
    ms_load_tile(M, i, k0, t, img);
    __syncthreads();
    for (int c = grp; c < T; c += MS_GROUPS) {
      const double* vals = img + (size_t)c * M.S;
      double lp = 0.0;
      for (int a = 0; a < M.nnodes; ++a) lp += MI::template node_lp<true>(A, M.nodes[a], vals, stk, g, 0);
      const int64_t k = k0 + c;
      if (g.lane == 0 && k < M.K) M.lp[(size_t)i * M.K + k] = lp;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void ms_line_kernel(const SweepArgs A, const MsArgs M) {
  using ML = Mdl<MMB_MODEL_LINE>;
  const int64_t total = M.n * M.K;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t i = idx / M.K, k = idx - i * M.K;
    const double* row = M.draws + (size_t)i * 3 * M.K + k;
    ML::St s;
    s.v[0] = row[0];
    s.v[1] = row[(size_t)M.K];
    s.v[2] = row[(size_t)2 * M.K];
    double lp = 0.0;
    for (int a = 0; a < M.nnodes; ++a) {
      double term;
      if (M.nodes[a] == MMB_LINE_BETA) {
        if (!isfinite(s.v[0]) || !isfinite(s.v[1])) term = -__builtin_inf();
        else term = d_iso(2, sqrt(1000.0), s.v[0] * s.v[0] + s.v[1] * s.v[1]);
      } else if (M.nodes[a] == MMB_LINE_S2) {
        term = d_iglogpdf(A.ig_c, s.v[2], 0);
      } else {
        term = ML::ylp(A, s);
      }
      lp += term;
    }
    M.lp[idx] = lp;
  }
}

// acc[2k], acc[2k+1] += the rows' (D - c), (D - c)^2 of chain k, in row order
__global__ __launch_bounds__(MS_DEV_THREADS) void ms_deviance_kernel(int64_t rows, int K, const double* __restrict__ lp,
                                                                     double shift, double* __restrict__ acc) {
  const int64_t k = (int64_t)blockIdx.x * MS_DEV_THREADS + threadIdx.x;
  if (k >= K) return;
  double s1 = acc[2 * k], s2 = acc[2 * k + 1];
  // MS_DEV_ROWS loads in flight per thread, then the adds in row order (one thread per chain is few
  // wavefronts: without the batch every add waited for its own load)
  int64_t i = 0;
  for (; i + MS_DEV_ROWS <= rows; i += MS_DEV_ROWS) {
    double v[MS_DEV_ROWS];
#pragma unroll
    for (int u = 0; u < MS_DEV_ROWS; ++u) v[u] = lp[(size_t)(i + u) * K + k];
#pragma unroll
    for (int u = 0; u < MS_DEV_ROWS; ++u) {
      const double d = -2.0 * v[u] - shift;
      s1 += d;
      s2 += d * d;
    }
  }
  for (; i < rows; ++i) {
    const double d = -2.0 * lp[(size_t)i * K + k] - shift;
    s1 += d;
    s2 += d * d;
  }
  acc[2 * k] = s1;
  acc[2 * k + 1] = s2;
}

// ---------------------------------------------------------------- host side
// The tile of a node-IR model with `nvalues` values and expression stack depth `stack`: T chains, image
// stride S (nvalues rounded up to odd).  Returns 0 when not even 8 chains fit.
int mmb_modelstats_tile(int nvalues, int stack, int* S) {
  *S = nvalues | 1;
  for (int T = 32; T >= 8; T >>= 1)
    if (ms_lds_doubles(T, *S, stack) * sizeof(double) <= MS_LDS_BYTES) return T;
  return 0;
}

// lp[i*K + k], i < n, of the rows of `draws` ([n][pmon][K]).  Line: nodes are MMB_LINE_* ids.  Node IR: node
// ids of A's tables; col / slot (device, ncols entries) name the monitored columns to load and their state
// slots, every slot < nvalues <= MMB_IR_MAX_VALUES.
hipError_t mmb_launch_modelstats(int model, const SweepArgs& A, int nvalues, int stack, int64_t n, int K, int pmon,
                                 const double* draws, int nnodes, const int32_t* nodes, const int32_t* col,
                                 const int32_t* slot, int ncols, double* lp, hipStream_t st) {
  if (n < 1 || K < 1 || nnodes < 1 || nnodes > MMB_IR_MAX_TERMS) return hipErrorInvalidValue;
  MsArgs M{};
  M.n = n;
  M.K = K;
  M.pmon = pmon;
  M.draws = draws;
  M.lp = lp;
  M.nnodes = nnodes;
  for (int a = 0; a < nnodes; ++a) M.nodes[a] = nodes[a];
  if (model == MMB_MODEL_LINE) {
    if (pmon != 3) return hipErrorInvalidValue;
    int64_t blocks = (n * K + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(ms_line_kernel, dim3((unsigned)blocks), dim3(256), 0, st, A, M);
    return hipGetLastError();
  }
  if (model != MMB_MODEL_IR) return hipErrorInvalidValue;
  if (nvalues < 1 || nvalues > MMB_IR_MAX_VALUES || stack < 1 || stack > MMB_IR_MAX_STACK || ncols < 0)
    return hipErrorInvalidValue;
  M.col = col;
  M.slot = slot;
  M.ncols = ncols;
  M.stack = stack;
  M.T = mmb_modelstats_tile(nvalues, stack, &M.S);
  if (M.T == 0) return hipErrorInvalidValue;
  const int64_t ntiles = n * (((int64_t)K + M.T - 1) / M.T);
  int64_t blocks = ntiles < 4096 ? ntiles : 4096;
  const size_t lds = ms_lds_doubles(M.T, M.S, stack) * sizeof(double);
  hipLaunchKernelGGL(ms_ir_kernel, dim3((unsigned)blocks), dim3(MS_THREADS), lds, st, A, M);
  return hipGetLastError();
}

hipError_t mmb_launch_deviance(int64_t rows, int K, const double* lp, double shift, double* acc, hipStream_t st) {
  if (rows < 1 || K < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ms_deviance_kernel, dim3((unsigned)((K + MS_DEV_THREADS - 1) / MS_DEV_THREADS)), dim3(MS_DEV_THREADS), 0,
                     st, rows, K, lp, shift, acc);
  return hipGetLastError();
}
