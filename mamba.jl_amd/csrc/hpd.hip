// hpd.hip — highest-posterior-density intervals of the device-kept draws.
//
// hpd(x; alpha) (src/output/stats.jl:54-74) sorts the N pooled draws of a param, takes the m
// smallest a = y[1:m] and the m largest b = y[N-m+1:N], m = max(1, ceil(alpha N)), and returns
// [a[i], b[i]] at the first minimum of b - a.  The two thresholds y[m-1] and y[N-m] come from the
// radix select (summary.hip os_hist_kernel); this file does the rest, on the select's
// order-preserving 64-bit key (order_key.h):
//
// hpd_collect_kernel: one streaming pass over the param's n x K draws (os_hist_kernel's access
//   pattern).  Keys strictly below key(lo) are appended to `below`, keys strictly above key(hi) to
//   `above`, each at most m - 1 of them, unsorted.  A workgroup takes HPD_ROWS rows of its 256 chains
//   at a time; its wavefronts count their hits with ballots and ONE atomic add per buffer claims the
//   workgroup's slots (the two counters are the pass's only contended words: at one add per
//   wavefront and 8 rows the pass ran at the counters' rate, 13 times the select's pass);
//   a slot at or past `cap` is never written (the count still grows: the host reports the
//   overflow).  It also keeps the OR and the AND of the stored keys: a key byte in which they agree
//   is the same in every key, and the sort skips its pass (posterior tails share their top bytes).
//
// hpd_sort_*: LSD radix sort, 8 bits per pass, of one buffer, stable and exact.  Per pass
//   count:   a workgroup histograms the digit of its tile of HPD_TILE keys -> tilehist[d][tile],
//            and adds it to the pass's totals ghist[d];
//   scan:    workgroup d turns row d into scatter offsets: (keys of smaller digits) + (keys of
//            digit d in earlier tiles);
//   scatter: a key's slot = that offset + its rank among the tile's keys of the same digit, in
//            tile order: (such keys in earlier 64-key units, a prefix over LDS counts) + (such keys
//            in lower lanes of its unit, from eight ballots that intersect to the lanes holding
//            the same digit).
//
// hpd_gap_kernel / hpd_gap_final_kernel: d[i] = b[i] - a[i] over the virtual arrays
//   a = sorted below, then copies of lo;  b = copies of hi, then sorted above  (m each; the copies
//   are never stored), reduced to the minimum with the lowest index on ties (lexicographic on
//   (d, i)), in two stages so that the result does not depend on the launch shape.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "order_key.h"
#include "launch.h"

#define HPD_THREADS 256
#define HPD_ROWS 16                                 // rows a thread has in flight in the collect pass
// keys per thread of a sort tile: 16 makes tiles of 4096 keys.  Every tile adds its 256 digit counts
// to the pass's 256 totals and owns a column of tilehist, so smaller tiles (4 keys per thread were
// tried) spend the count kernel on those contended adds and strided stores, not on reading keys
#define HPD_TILE_KEYS 16
#define HPD_TILE (HPD_THREADS * HPD_TILE_KEYS)      // keys per sort tile
#define HPD_UNITS (HPD_TILE / 64)                   // 64-key units (one wavefront load) per tile
#define HPD_GAP_BLOCKS 256
// meta words: the two counts, then OR and AND of the stored keys of each buffer
#define HPD_META 6

static_assert(HPD_THREADS == 256, "one thread per radix bin");

// ---------------------------------------------------------------- collect
__global__ void hpd_meta_init_kernel(unsigned long long* __restrict__ meta) {
  if (threadIdx.x < HPD_META) meta[threadIdx.x] = (threadIdx.x == 3 || threadIdx.x == 5) ? ~0ull : 0ull;
}

// store the lane's taken keys of HPD_ROWS rows from slot `base` on: a key's slot is base + (taken keys
// of earlier rows) + (taken keys of lower lanes in its row)
__device__ __forceinline__ void hpd_store(const uint64_t (&key)[HPD_ROWS], const bool (&take)[HPD_ROWS],
                                          uint64_t* __restrict__ buf, int64_t cap, unsigned long long base, int lane,
                                          uint64_t& bor, uint64_t& band) {
  const unsigned long long lower = (1ull << lane) - 1ull;
#pragma unroll
  for (int u = 0; u < HPD_ROWS; ++u) {
    const unsigned long long mask = __ballot(take[u]);
    if (take[u]) {
      const unsigned long long slot = base + (unsigned long long)__popcll(mask & lower);
      if (slot < (unsigned long long)cap) {   // never past the capacity the caller gave
        buf[slot] = key[u];
        bor |= key[u];
        band &= key[u];
      }
    }
    base += (unsigned long long)__popcll(mask);
  }
}

__device__ __forceinline__ uint64_t hpd_wave_or(uint64_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, s);
  return v;
}

__global__ __launch_bounds__(HPD_THREADS) void hpd_collect_kernel(int P, int j, int64_t n, int K,
                                                                  const double* __restrict__ draws, uint64_t klo,
                                                                  uint64_t khi, int64_t cap,
                                                                  uint64_t* __restrict__ below,
                                                                  uint64_t* __restrict__ above,
                                                                  unsigned long long* __restrict__ meta) {
  // the wavefronts' hit counts of the round and the slots the workgroup claimed, by round parity:
  // a wavefront may start the next round while another still reads this one's
  __shared__ unsigned int wtot[2][2][HPD_THREADS / 64];
  __shared__ unsigned long long wbase[2][2];
  const size_t stride = (size_t)P * K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t bor = 0ull, band = ~0ull, aor = 0ull, aand = ~0ull;
  int par = 0;
  // every thread of the workgroup makes the same trips (barriers and ballots need them all): a
  // chain past K or a row past n is masked, not skipped
  for (int64_t i0 = (int64_t)blockIdx.y * HPD_ROWS; i0 < n; i0 += (int64_t)gridDim.y * HPD_ROWS) {
    for (int64_t k0 = (int64_t)blockIdx.x * HPD_THREADS; k0 < K; k0 += (int64_t)gridDim.x * HPD_THREADS) {
      const int64_t k = k0 + threadIdx.x;
      uint64_t key[HPD_ROWS];
      bool lo[HPD_ROWS], hi[HPD_ROWS];
      unsigned nlo = 0u, nhi = 0u;
#pragma unroll
      for (int u = 0; u < HPD_ROWS; ++u) {
        const bool ok = k < K && i0 + u < n;
        key[u] = ok ? os_key(draws[(size_t)(i0 + u) * stride + (size_t)j * K + (size_t)k]) : 0ull;
        lo[u] = ok && key[u] < klo;
        hi[u] = ok && key[u] > khi;
      }
#pragma unroll
      for (int u = 0; u < HPD_ROWS; ++u) {
        nlo += (unsigned)__popcll(__ballot(lo[u]));
        nhi += (unsigned)__popcll(__ballot(hi[u]));
      }
      if (lane == 0) {
        wtot[par][0][wave] = nlo;
        wtot[par][1][wave] = nhi;
      }
      __syncthreads();
      if (threadIdx.x < 2) {                   // one atomic add per buffer claims the workgroup's slots
        unsigned tot = 0u;
#pragma unroll
        for (int w = 0; w < HPD_THREADS / 64; ++w) tot += wtot[par][threadIdx.x][w];
        wbase[par][threadIdx.x] = tot ? atomicAdd(&meta[threadIdx.x], (unsigned long long)tot) : 0ull;
      }
      __syncthreads();
      unsigned long long blo = wbase[par][0], bhi = wbase[par][1];
#pragma unroll
      for (int w = 0; w < HPD_THREADS / 64; ++w) {
        blo += w < wave ? wtot[par][0][w] : 0u;
        bhi += w < wave ? wtot[par][1][w] : 0u;
      }
      hpd_store(key, lo, below, cap, blo, lane, bor, band);
      hpd_store(key, hi, above, cap, bhi, lane, aor, aand);
      par ^= 1;
    }
  }
  bor = hpd_wave_or(bor);
  band = ~hpd_wave_or(~band);
  aor = hpd_wave_or(aor);
  aand = ~hpd_wave_or(~aand);
  if (lane == 0) {
    if (bor) atomicOr(&meta[2], (unsigned long long)bor);
    if (~band) atomicAnd(&meta[3], (unsigned long long)band);
    if (aor) atomicOr(&meta[4], (unsigned long long)aor);
    if (~aand) atomicAnd(&meta[5], (unsigned long long)aand);
  }
}

// ---------------------------------------------------------------- sort
__global__ __launch_bounds__(HPD_THREADS) void hpd_sort_count_kernel(const uint64_t* __restrict__ src, int64_t n,
                                                                     int shift, int64_t ntiles,
                                                                     unsigned int* __restrict__ tilehist,
                                                                     unsigned long long* __restrict__ ghist) {
  __shared__ unsigned int h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * HPD_TILE;
#pragma unroll
  for (int q = 0; q < HPD_TILE_KEYS; ++q) {
    const int64_t i = t0 + q * HPD_THREADS + threadIdx.x;
    if (i < n) atomicAdd(&h[(unsigned)(src[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  const unsigned v = h[threadIdx.x];
  tilehist[(size_t)threadIdx.x * ntiles + blockIdx.x] = v;
  if (v) atomicAdd(&ghist[threadIdx.x], (unsigned long long)v);
}

// workgroup d: tilehist[d][*] (counts) -> exclusive offsets, from the number of keys with a smaller digit
__global__ __launch_bounds__(HPD_THREADS) void hpd_sort_scan_kernel(int64_t ntiles, unsigned int* __restrict__ tilehist,
                                                                    const unsigned long long* __restrict__ ghist) {
  __shared__ unsigned long long s[HPD_THREADS];
  const int d = (int)blockIdx.x, t = (int)threadIdx.x;
  s[t] = t < d ? ghist[t] : 0ull;
  __syncthreads();
  for (int w = HPD_THREADS / 2; w >= 1; w >>= 1) {
    if (t < w) s[t] += s[t + w];
    __syncthreads();
  }
  unsigned long long carry = s[0];
  __syncthreads();
  unsigned int* row = tilehist + (size_t)d * ntiles;
  for (int64_t c0 = 0; c0 < ntiles; c0 += HPD_THREADS) {
    const int64_t c = c0 + t;
    const unsigned long long x = c < ntiles ? row[c] : 0u;
    s[t] = x;
    __syncthreads();
    for (int w = 1; w < HPD_THREADS; w <<= 1) {     // inclusive scan of the chunk
      const unsigned long long add = t >= w ? s[t - w] : 0ull;
      __syncthreads();
      s[t] += add;
      __syncthreads();
    }
    if (c < ntiles) row[c] = (unsigned int)(carry + s[t] - x);
    carry += s[HPD_THREADS - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(HPD_THREADS) void hpd_sort_scatter_kernel(const uint64_t* __restrict__ src,
                                                                       uint64_t* __restrict__ dst, int64_t n, int shift,
                                                                       int64_t ntiles,
                                                                       const unsigned int* __restrict__ tileoff) {
  // keys of digit d in unit u of the tile, then their exclusive prefix over the units
  __shared__ unsigned short cnt[HPD_UNITS][256];
  __shared__ unsigned int base[256];
  for (int q = threadIdx.x; q < HPD_UNITS * 256; q += HPD_THREADS) cnt[q >> 8][q & 255] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  const int64_t t0 = (int64_t)blockIdx.x * HPD_TILE;
  uint64_t key[HPD_TILE_KEYS];
  unsigned rank[HPD_TILE_KEYS];
#pragma unroll
  for (int q = 0; q < HPD_TILE_KEYS; ++q) {
    const int64_t i = t0 + q * HPD_THREADS + threadIdx.x;
    const bool ok = i < n;
    key[q] = ok ? src[i] : 0ull;
    const unsigned dg = (unsigned)(key[q] >> shift) & 255u;
    unsigned long long peers = __ballot(ok);        // the unit's lanes holding the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (dg >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    rank[q] = (unsigned)__popcll(peers & lower);
    if (ok && rank[q] == 0u) cnt[q * (HPD_THREADS / 64) + wave][dg] = (unsigned short)__popcll(peers);
  }
  __syncthreads();
  {
    const int d = (int)threadIdx.x;
    unsigned acc = 0u;
#pragma unroll
    for (int u = 0; u < HPD_UNITS; ++u) {
      const unsigned c = cnt[u][d];
      cnt[u][d] = (unsigned short)acc;
      acc += c;
    }
    base[d] = tileoff[(size_t)d * ntiles + blockIdx.x];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < HPD_TILE_KEYS; ++q) {
    const int64_t i = t0 + q * HPD_THREADS + threadIdx.x;
    if (i < n) {
      const unsigned dg = (unsigned)(key[q] >> shift) & 255u;
      const int64_t slot = (int64_t)base[dg] + cnt[q * (HPD_THREADS / 64) + wave][dg] + rank[q];
      if (slot < n) dst[slot] = key[q];             // holds by construction; the bound costs nothing
    }
  }
}

// ---------------------------------------------------------------- gap
__device__ __forceinline__ double hpd_gap_a(int64_t i, const uint64_t* __restrict__ below, int64_t nb, double lo) {
  return i < nb ? os_unkey(below[i]) : lo;
}

__device__ __forceinline__ double hpd_gap_b(int64_t i, const uint64_t* __restrict__ above, int64_t na, int64_t m,
                                            double hi) {
  return i < m - na ? hi : os_unkey(above[i - (m - na)]);
}

// (d, i) precedes (bd, bi): smaller d, or equal d at a lower index; bi < 0: nothing yet
__device__ __forceinline__ bool hpd_gap_less(double d, int64_t i, double bd, int64_t bi) {
  return i >= 0 && (bi < 0 || d < bd || (d == bd && i < bi));
}

__device__ __forceinline__ void hpd_gap_block_min(double& bd, int64_t& bi, double* sd, long long* si) {
  const int t = (int)threadIdx.x;
  sd[t] = bd;
  si[t] = bi;
  __syncthreads();
  for (int w = HPD_THREADS / 2; w >= 1; w >>= 1) {
    if (t < w && hpd_gap_less(sd[t + w], si[t + w], sd[t], si[t])) {
      sd[t] = sd[t + w];
      si[t] = si[t + w];
    }
    __syncthreads();
  }
  bd = sd[0];
  bi = si[0];
}

__global__ __launch_bounds__(HPD_THREADS) void hpd_gap_kernel(const uint64_t* __restrict__ below, int64_t nb,
                                                              const uint64_t* __restrict__ above, int64_t na, int64_t m,
                                                              double lo, double hi, double* __restrict__ part_d,
                                                              long long* __restrict__ part_i) {
  __shared__ double sd[HPD_THREADS];
  __shared__ long long si[HPD_THREADS];
  double bd = 0.0;
  int64_t bi = -1;
  for (int64_t i = (int64_t)blockIdx.x * HPD_THREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * HPD_THREADS) {
    const double d = hpd_gap_b(i, above, na, m, hi) - hpd_gap_a(i, below, nb, lo);
    if (hpd_gap_less(d, i, bd, bi)) {
      bd = d;
      bi = i;
    }
  }
  hpd_gap_block_min(bd, bi, sd, si);
  if (threadIdx.x == 0) {
    part_d[blockIdx.x] = bd;
    part_i[blockIdx.x] = bi;
  }
}

// res = [a[i], b[i]] as doubles, then i as a 64-bit integer
__global__ __launch_bounds__(HPD_THREADS) void hpd_gap_final_kernel(const uint64_t* __restrict__ below, int64_t nb,
                                                                    const uint64_t* __restrict__ above, int64_t na,
                                                                    int64_t m, double lo, double hi, int nparts,
                                                                    const double* __restrict__ part_d,
                                                                    const long long* __restrict__ part_i,
                                                                    double* __restrict__ res) {
  __shared__ double sd[HPD_THREADS];
  __shared__ long long si[HPD_THREADS];
  const int t = (int)threadIdx.x;
  double bd = t < nparts ? part_d[t] : 0.0;
  int64_t bi = t < nparts ? part_i[t] : -1;
  hpd_gap_block_min(bd, bi, sd, si);
  if (t == 0) {
    const bool found = bi >= 0 && bi < m;
    res[0] = found ? hpd_gap_a(bi, below, nb, lo) : lo;
    res[1] = found ? hpd_gap_b(bi, above, na, m, hi) : hi;
    ((long long*)res)[2] = found ? bi : -1;
  }
}

// ---------------------------------------------------------------- host side
// os_key / os_unkey (order_key.h) for the host: thresholds, uploaded and downloaded tails
uint64_t mmb_hpd_key(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof u);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

double mmb_hpd_unkey(uint64_t key) {
  const uint64_t u = (key >> 63) ? key & 0x7fffffffffffffffull : ~key;
  double x;
  memcpy(&x, &u, sizeof x);
  return x;
}

int64_t mmb_hpd_tiles(int64_t n) { return (n + HPD_TILE - 1) / HPD_TILE; }

// meta: HPD_META words (counts, OR / AND of the stored keys); below / above hold `cap` keys each
hipError_t mmb_launch_hpd_collect(int P, int j, int64_t n, int K, const double* draws, double lo, double hi,
                                  int64_t cap, uint64_t* below, uint64_t* above, unsigned long long* meta,
                                  hipStream_t st) {
  if (cap < 0 || n < 1 || K < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hpd_meta_init_kernel, dim3(1), dim3(64), 0, st, meta);
  // os_hist_kernel's shape: ~1024 workgroups striding over the rows
  int gx = (K + HPD_THREADS - 1) / HPD_THREADS;
  if (gx > 64) gx = 64;
  int64_t gy = 1024 / gx;
  const int64_t groups = (n + HPD_ROWS - 1) / HPD_ROWS;
  if (gy > groups) gy = groups;
  if (gy < 1) gy = 1;
  hipLaunchKernelGGL(hpd_collect_kernel, dim3(gx, (unsigned)gy), dim3(HPD_THREADS), 0, st, P, j, n, K, draws,
                     mmb_hpd_key(lo), mmb_hpd_key(hi), cap, below, above, meta);
  return hipGetLastError();
}

// Sorts keys[0, n) ascending, through tmp[0, n).  `varying`: the bits in which the keys differ (OR ^ AND);
// a pass whose byte is the same in every key is skipped.  tilehist: 256 * mmb_hpd_tiles(n) words, ghist: 256.
// *in_tmp = 1 when the sorted keys ended in tmp (the caller swaps the two buffers).
hipError_t mmb_launch_hpd_sort(uint64_t* keys, uint64_t* tmp, int64_t n, uint64_t varying, unsigned int* tilehist,
                               unsigned long long* ghist, int* in_tmp, hipStream_t st) {
  *in_tmp = 0;
  if (n < 2) return hipSuccess;
  if (n > 0xffffffffll) return hipErrorInvalidValue;   // the scatter offsets are 32-bit
  const int64_t ntiles = mmb_hpd_tiles(n);
  uint64_t *src = keys, *dst = tmp;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 8 * pass;
    if (((varying >> shift) & 255ull) == 0ull) continue;
    hipError_t e = hipMemsetAsync(ghist, 0, 256 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hpd_sort_count_kernel, dim3((unsigned)ntiles), dim3(HPD_THREADS), 0, st, src, n, shift, ntiles,
                       tilehist, ghist);
    hipLaunchKernelGGL(hpd_sort_scan_kernel, dim3(256), dim3(HPD_THREADS), 0, st, ntiles, tilehist, ghist);
    hipLaunchKernelGGL(hpd_sort_scatter_kernel, dim3((unsigned)ntiles), dim3(HPD_THREADS), 0, st, src, dst, n, shift,
                       ntiles, tilehist);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    uint64_t* t = src;
    src = dst;
    dst = t;
  }
  *in_tmp = src == tmp;
  return hipSuccess;
}

// part_d / part_i: HPD_GAP_BLOCKS words each; res: 3 words ([a[i], b[i]] doubles, i int64)
hipError_t mmb_launch_hpd_gap(const uint64_t* below, int64_t nb, const uint64_t* above, int64_t na, int64_t m,
                              double lo, double hi, double* part_d, long long* part_i, double* res, hipStream_t st) {
  if (m < 1 || nb < 0 || na < 0 || nb > m || na > m) return hipErrorInvalidValue;
  int64_t nparts = (m + HPD_THREADS - 1) / HPD_THREADS;
  if (nparts > HPD_GAP_BLOCKS) nparts = HPD_GAP_BLOCKS;
  hipLaunchKernelGGL(hpd_gap_kernel, dim3((unsigned)nparts), dim3(HPD_THREADS), 0, st, below, nb, above, na, m, lo, hi,
                     part_d, part_i);
  hipLaunchKernelGGL(hpd_gap_final_kernel, dim3(1), dim3(HPD_THREADS), 0, st, below, nb, above, na, m, lo, hi,
                     (int)nparts, part_d, part_i, res);
  return hipGetLastError();
}
