// predict.hip — posterior predictive draws of the observed nodes on the device-kept draws.
//
// predict(mc, nodekeys) (src/output/modelstats.jl:71-102) relists every kept draw into the model and
// draws rand(m[key]) of each listed output node.  Here, for kept row i, local chain k and column j
// (the listed nodes' elements in list order, P in all),
//
//   yhat[(i*P + j)*K + k] = one variate of the node's distribution with its parameters evaluated on
//                           the draw, on the streams of predict_math.h: a pure function of (seed,
//                           chain_offset + k, the row's iteration, node id, element)
//
// so the values do not depend on sharding, row chunking, tile size or call order.
//
// pr_ir_kernel (node-IR models) tiles like ms_ir_kernel (modelstats.h): a workgroup of 128 threads
//   takes T consecutive chains of one row, loads the columns the listed nodes' parameter expressions
//   read into T per-chain state images in LDS, then its four 32-lane groups walk the tile's chains
//   (group g: chains g, g + 4, ...) with the lanes over a node's elements: the lane evaluates the
//   parameters with the interpreter's ev on the image, exactly as node_lp does, and draws.  Lanes
//   hold different columns of one chain and the output is chain-fastest, so a store from the lanes
//   would be a lone 8-byte write a stride of K apart.  The results are staged in LDS instead, a tile
//   [T][P] of stride RS (P rounded up to odd), and written out the way the loads came in: thread t
//   takes chain t % T, so T chains of one column are T*8 contiguous bytes.  Chains past K are
//   loaded as chain K - 1, skipped by the groups (no cross-lane operation here) and not stored.
//   LDS per workgroup = (T*S + T*RS + 4*(stack + 1)*32) doubles within MS_LDS_BYTES; the host
//   picks the largest T of 32 / 16 / 8 that fits.
//
// pr_line_kernel (hand-lowered line): one thread per (row, chain); three coalesced loads, mu_i as
//   Mdl<line>::ylp forms it, sigma = sqrt(s2); the five normals are both halves of pairs 0 and 1
//   and the first of pair 2 (three Philox blocks); five coalesced stores.
//
// pr_moments_kernel: per (chain, column), [sum_i (yhat - shift_j), sum_i (yhat - shift_j)^2] in
//   row order, continued over row chunks (ms_deviance_kernel's scheme; non-finite values propagate).
#include "modelstats.h"
#include "predict_math.h"
#include "launch.h"

#define PR_MOM_THREADS 64
#define PR_MOM_ROWS 16  // loads in flight per thread

struct PrArgs {
  double* out;                      // [n][P][K]
  int32_t P, RS;                    // result columns; stride of the result tile (doubles, odd)
  int32_t col0[MMB_IR_MAX_TERMS];   // first result column of list entry a
  uint64_t seed;
  int64_t it0, thin;                // iteration of row i of this launch: it0 + i*thin
};

static size_t pr_lds_doubles(int T, int S, int RS, int stack) {
  return (size_t)T * S + (size_t)T * RS + (size_t)MS_GROUPS * (stack + 1) * 32;
}

__global__ __launch_bounds__(MS_THREADS) void pr_ir_kernel(const SweepArgs A, const MsArgs M, const PrArgs R) {
  extern __shared__ double pr_lds[];
  using MI = Mdl<MMB_MODEL_IR>;
  const int t = (int)threadIdx.x;
  const int grp = t >> 5, lane = t & 31;
  const int T = M.T;
  double* img = pr_lds;
  double* res = pr_lds + (size_t)T * M.S;
  double* stk = res + (size_t)T * R.RS + (size_t)grp * (M.stack + 1) * 32;
  const int64_t ktiles = ((int64_t)M.K + T - 1) / T;
  const int64_t ntiles = M.n * ktiles;
  const int lc = t % T, cs = t / T, cstep = MS_THREADS / T;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t i = tile / ktiles;
    const int64_t k0 = (tile - i * ktiles) * T;
    const uint32_t iter = (uint32_t)(R.it0 + i * R.thin);
    ms_load_tile(M, i, k0, t, img);
    __syncthreads();
    for (int c = grp; c < T; c += MS_GROUPS) {
      const int64_t k = k0 + c;
      if (k >= M.K) break;
      const double* vals = img + (size_t)c * M.S;
      double* rc = res + (size_t)c * R.RS;
      const uint32_t chain = A.chain_offset + (uint32_t)k;
      for (int a = 0; a < M.nnodes; ++a) {
        const int n = M.nodes[a];
        const mmb_ir_node& N = ir_const_ref(A.ir_nodes, n);
        const int fam = N.family, len = N.len;
        const bool iso = fam == MMB_IR_ISONORMAL;
        const double sig = iso ? MI::ev(A, N.expr[1], 0, vals, stk, lane) : 0.0;
        for (int e = lane; e < len; e += 32) {
          const double pa = N.expr[0] >= 0 ? MI::ev(A, N.expr[0], e, vals, stk, lane) : 0.0;
          const double pb = iso ? sig : (N.expr[1] >= 0 ? MI::ev(A, N.expr[1], e, vals, stk, lane) : 0.0);
          rc[R.col0[a] + e] = mmb_pr_elem(fam, pa, pb, R.seed, chain, iter, n, e, len);
        }
      }
    }
    __syncthreads();
    {
      const int64_t k = k0 + lc;
      if (k < M.K) {
        double* dst = R.out + (size_t)i * R.P * M.K + k;
        const double* src = res + (size_t)lc * R.RS;
        for (int q = cs; q < R.P; q += cstep) dst[(size_t)q * M.K] = src[q];
      }
    }
    // the next tile's load writes the images only, and its barrier stands before the next result writes
  }
}

__global__ __launch_bounds__(256) void pr_line_kernel(const SweepArgs A, const MsArgs M, const PrArgs R) {
  const int64_t total = M.n * M.K;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t i = idx / M.K, k = idx - i * M.K;
    const double* row = M.draws + (size_t)i * 3 * M.K + k;
    const double b0 = row[0], b1 = row[(size_t)M.K], s2 = row[(size_t)2 * M.K];
    const double sig = sqrt(s2);
    const mmb_rng s = mmb_rng_make(R.seed, A.chain_offset + (uint32_t)k, (uint32_t)(R.it0 + i * R.thin),
                                   mmb_pr_block(MMB_LINE_Y), MMB_SUB_NORMAL);
    double z[6];
    mmb_normal_pair(&s, 0, &z[0], &z[1]);
    mmb_normal_pair(&s, 1, &z[2], &z[3]);
    mmb_normal_pair(&s, 2, &z[4], &z[5]);
    double* dst = R.out + (size_t)i * 5 * M.K + k;
#pragma unroll
    for (int e = 0; e < 5; ++e) {
      const double mu = b0 + A.lx[e] * b1;
      const bool ok = isfinite(mu) && isfinite(sig) && sig >= 0.0;
      dst[(size_t)e * M.K] = ok ? mu + sig * z[e] : __builtin_nan("");
    }
  }
}

// acc[(k*P + j)*2], [.. + 1] += the rows' (yhat - shift[j]), (yhat - shift[j])^2 of chain k, in row order
__global__ __launch_bounds__(PR_MOM_THREADS) void pr_moments_kernel(int64_t rows, int K, int P,
                                                                    const double* __restrict__ yhat,
                                                                    const double* __restrict__ shift,
                                                                    double* __restrict__ acc) {
  const int64_t idx = (int64_t)blockIdx.x * PR_MOM_THREADS + threadIdx.x;
  if (idx >= (int64_t)K * P) return;
  const int64_t j = idx / K, k = idx - j * K;   // chain fastest: a wavefront's loads are contiguous
  const double sh = shift[j];
  double* a = acc + ((size_t)k * P + j) * 2;
  double s1 = a[0], s2 = a[1];
  const double* col = yhat + (size_t)j * K + k;
  const size_t rs = (size_t)P * K;
  int64_t i = 0;
  for (; i + PR_MOM_ROWS <= rows; i += PR_MOM_ROWS) {
    double v[PR_MOM_ROWS];
#pragma unroll
    for (int u = 0; u < PR_MOM_ROWS; ++u) v[u] = col[(size_t)(i + u) * rs];
#pragma unroll
    for (int u = 0; u < PR_MOM_ROWS; ++u) {
      const double d = v[u] - sh;
      s1 += d;
      s2 += d * d;
    }
  }
  for (; i < rows; ++i) {
    const double d = col[(size_t)i * rs] - sh;
    s1 += d;
    s2 += d * d;
  }
  a[0] = s1;
  a[1] = s2;
}

// ---------------------------------------------------------------- host side
// The tile of a node-IR model with `nvalues` values, stack depth `stack` and P result columns: T chains,
// image stride S, result stride RS (both rounded up to odd).  Returns 0 when not even 8 chains fit.
int mmb_predict_tile(int nvalues, int stack, int P, int* S, int* RS) {
  *S = nvalues | 1;
  *RS = P | 1;
  for (int T = 32; T >= 8; T >>= 1)
    if (pr_lds_doubles(T, *S, *RS, stack) * sizeof(double) <= MS_LDS_BYTES) return T;
  return 0;
}

// yhat[(i*P + j)*K + k], i < n, of the rows of `draws` ([n][pmon][K]); row i has iteration it0 + i*thin.
// Line: the node list is {MMB_LINE_Y}, P = 5.  Node IR: as mmb_launch_modelstats, col0[a] the first
// result column of nodes[a]; the caller has checked that a tile fits (mmb_predict_tile).
hipError_t mmb_launch_predict(int model, const SweepArgs& A, int nvalues, int stack, int64_t n, int K, int pmon,
                              const double* draws, int nnodes, const int32_t* nodes, const int32_t* col0, int P,
                              const int32_t* col, const int32_t* slot, int ncols, uint64_t seed, int64_t it0,
                              int64_t thin, double* yhat, hipStream_t st) {
  if (n < 1 || K < 1 || P < 1 || nnodes < 1 || nnodes > MMB_IR_MAX_TERMS) return hipErrorInvalidValue;
  MsArgs M{};
  M.n = n;
  M.K = K;
  M.pmon = pmon;
  M.draws = draws;
  M.nnodes = nnodes;
  PrArgs R{};
  R.out = yhat;
  R.P = P;
  R.seed = seed;
  R.it0 = it0;
  R.thin = thin;
  for (int a = 0; a < nnodes; ++a) {
    M.nodes[a] = nodes[a];
    R.col0[a] = col0[a];
  }
  if (model == MMB_MODEL_LINE) {
    if (pmon != 3 || P != 5 || nnodes != 1 || nodes[0] != MMB_LINE_Y) return hipErrorInvalidValue;
    int64_t blocks = (n * K + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(pr_line_kernel, dim3((unsigned)blocks), dim3(256), 0, st, A, M, R);
    return hipGetLastError();
  }
  if (model != MMB_MODEL_IR) return hipErrorInvalidValue;
  if (nvalues < 1 || nvalues > MMB_IR_MAX_VALUES || stack < 1 || stack > MMB_IR_MAX_STACK || ncols < 0)
    return hipErrorInvalidValue;
  M.col = col;
  M.slot = slot;
  M.ncols = ncols;
  M.stack = stack;
  M.T = mmb_predict_tile(nvalues, stack, P, &M.S, &R.RS);
  if (M.T == 0) return hipErrorInvalidValue;
  const int64_t ntiles = n * (((int64_t)K + M.T - 1) / M.T);
  const int64_t blocks = ntiles < 4096 ? ntiles : 4096;
  const size_t lds = pr_lds_doubles(M.T, M.S, R.RS, stack) * sizeof(double);
  hipLaunchKernelGGL(pr_ir_kernel, dim3((unsigned)blocks), dim3(MS_THREADS), lds, st, A, M, R);
  return hipGetLastError();
}

hipError_t mmb_launch_predict_moments(int64_t rows, int K, int P, const double* yhat, const double* shift, double* acc,
                                      hipStream_t st) {
  if (rows < 1 || K < 1 || P < 1) return hipErrorInvalidValue;
  const int64_t blocks = ((int64_t)K * P + PR_MOM_THREADS - 1) / PR_MOM_THREADS;
  hipLaunchKernelGGL(pr_moments_kernel, dim3((unsigned)blocks), dim3(PR_MOM_THREADS), 0, st, rows, K, P, yhat, shift,
                     acc);
  return hipGetLastError();
}
