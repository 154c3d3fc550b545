// modelstats.h — what the kernels over the device-kept draws share (modelstats.hip: log densities,
// predict.hip: posterior predictive draws): the launch arguments of a node list and the load phase
// that tiles draw rows into per-chain state images in LDS (layout: modelstats.hip's header).
#pragma once
#include "sweep.h"

#define MS_THREADS 128
#define MS_GROUPS (MS_THREADS / 32)
#define MS_LDS_BYTES 65536

struct MsArgs {
  int64_t n;             // rows of `draws`
  int32_t K, pmon;       // chains, monitored columns
  const double* draws;   // [n][pmon][K]
  double* lp;            // [n][K]
  int32_t nnodes;
  int32_t nodes[MMB_IR_MAX_TERMS];
  // node IR
  const int32_t* col;    // [ncols] monitored column
  const int32_t* slot;   // [ncols] its state slot
  int32_t ncols;
  int32_t T, S;          // tile chains, image stride (doubles)
  int32_t stack;         // expression stack depth
};

// Row i, chains k0 .. k0 + T - 1 (past K: chain K - 1) of the columns `col` into the T images at `img`,
// column q at state slot `slot[q]`; thread t takes chain t % T (T consecutive chains of one column
// are T*8 contiguous bytes).  The caller synchronises the workgroup before the images are read.
__device__ __forceinline__ void ms_load_tile(const MsArgs& M, int64_t i, int64_t k0, int t, double* img) {
  const int T = M.T;
  const int lc = t % T, cs = t / T, cstep = MS_THREADS / T;
  int64_t k = k0 + lc;
  if (k > M.K - 1) k = M.K - 1;
  const double* row = M.draws + (size_t)i * M.pmon * M.K + k;
  double* dst = img + (size_t)lc * M.S;
  for (int q = cs; q < M.ncols; q += cstep) dst[M.slot[q]] = row[(size_t)M.col[q] * M.K];
}
