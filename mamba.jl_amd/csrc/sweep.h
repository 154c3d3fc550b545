// sweep.h — the fused block-sweep kernel: one launch advances every chain of the
// shard through `n_iters` iterations of sample!(m) (simulation.jl:93-107), i.e.
// mcmc_worker!'s loop body (mcmc.jl:74-80) including the keep rule and the
// Chains write sim[i,:,1] = unlist(m, true) (mcmc.jl:76-77).
//
// Per chain, per iteration: values are held in registers; AMWG/AMM tune state
// and the AMM moment/factor matrices are streamed from/to HBM (chain-major,
// element fastest, coalesced per lane group); the AMM covariance and its
// pivoted Cholesky factor are staged in LDS.  Shared by sweep.hip (the static
// kernels) and the node-IR JIT kernel (engine.cpp ir_jit_source, compiled by hipRTC).
#pragma once
#include "samplers.h"
#include "ir.h"

#ifdef MMB_PHASE_PROF
extern __device__ unsigned long long mmb_prof[32];
#endif
#ifdef MMB_WAVE_TIMES
// diagnostics: per wave slot of the shard, over the launches of the last mmb_run window (all
// parts): first start, last end and summed residency on the 100 MHz constant clock (engine.cpp
// clears them before a window and dumps the occupancy summary at mmb_destroy)
#define MMB_WT_MAX 65536
extern __device__ unsigned long long mmb_wt[3 * MMB_WT_MAX];
#endif

#ifndef MMB_SWEEP_WAVES
#define MMB_SWEEP_WAVES 4  // rats: min waves per SIMD the register allocator must allow
#endif
// Occupancy target per model: rats runs 8192 waves and is latency-bound (4 waves/SIMD
// measured 12 % faster than 3 despite spills); line has 64 waves in all, so it keeps the
// whole register budget (no spills).
#ifndef MMB_IR_WAVES
#define MMB_IR_WAVES 2  // node IR: min waves per SIMD (register budget 512 / waves)
#endif
template <int MODEL>
constexpr int sweep_waves() {
  return MODEL == MMB_MODEL_RATS ? MMB_SWEEP_WAVES : MODEL == MMB_MODEL_IR ? MMB_IR_WAVES : 1;
}

// KINDS: bitmask (1 << mmb_sampler_kind) of the sampler kinds present in the scheme; the
// other block paths are compiled out (register/SGPR allocation is per kernel).
template <int MODEL, unsigned KINDS>
__device__ __forceinline__ void sweep_body(const SweepArgs& A) {
  using M = Mdl<MODEL>;
  using S = Smp<M>;
  constexpr int G = M::G;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  if constexpr ((KINDS >> MMB_SAMPLER_AMM) & 1u) {  // moment-update slot table (before any exit)
    S::ik_fill();
    __syncthreads();
  }
#ifdef MMB_IR_POOL_LDS
  if constexpr (MODEL == MMB_MODEL_IR) {  // node-IR specialised kernel: the data pool in LDS (ir_jit.cpp)
    double* ps = mmb_ir_pool_s();
    for (int t = (int)threadIdx.x; t < MMB_IR_POOL_LDS; t += (int)blockDim.x) ps[t] = A.ir_pool[t];
    __syncthreads();
  }
#endif
  // workgroup of the shard: the engine may run the shard as parts, each a launch of its own that
  // holds every wg_stride-th workgroup (engine.cpp mmb_run); offset 0, stride 1: all of them
  const unsigned wg = blockIdx.x * (unsigned)A.wg_stride + (unsigned)A.wg_offset;
  const int slot = (int)((wg * blockDim.x + threadIdx.x) / G);
#ifdef MMB_WAVE_TIMES
  const uint64_t _wt0 = __builtin_amdgcn_s_memrealtime();
  const int _wid = (int)((wg * blockDim.x + threadIdx.x) >> 6);  // the wave's slot in the shard, not the launch
#endif
  if (slot >= A.K) return;  // whole lane groups exit together
  // chain of this lane group: the engine may order the chains so that chains whose pivoted
  // Cholesky stops early share wavefronts (engine.cpp order_chains); every index below --
  // state, tune, draws column, Philox chain id -- is the chain's own, so results do not depend
  // on the order
  const int c = A.cperm != nullptr ? A.cperm[slot] : slot;
  Grp<G> g;
  double* lds = smem + (size_t)(threadIdx.x / G) * M::lds_stride(A);
  typename M::St s;
  typename M::Lc l;
  M::load(A, c, g.lane, s, l, lds);
  const uint32_t chain = A.chain_offset + (uint32_t)c;
#ifdef MMB_PHASE_PROF
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < 16; ++i) mmb_prof_lds()[i] = 0;
#endif
  // state-independent draws (32-lane groups): one pass draws them for the next Q = max(1, 32 / nb)
  // iterations, block b of the batch's iteration j in lane j * nb + b (samplers.h predraw).  A
  // batch starts at the launch's step 0 and on every Q-th step after it, so no draw crosses a
  // launch; what a batch draws past the launch's last iteration is dropped.  pre0 = (step % Q) * nb,
  // kept by addition: it wraps when another iteration's nb lanes would not fit the 32.
  constexpr bool PREDRAW = G == 32 && (KINDS & ((1u << MMB_SAMPLER_GIBBS) | (1u << MMB_SAMPLER_AMM))) != 0u;
  int pre0 = 0;
  double pre = 0.0;
  // rats: the vector blocks' scalar constants, formed by one lane-parallel pass when a block
  // needs one whose variance node was written since the last pass (models.h prep_pass); all
  // stale here, so no value crosses a launch
  typename M::PrepCache pk = M::prep_cache(lds);
  // AMM lazy factor store (samplers.h amm): set by an update whose chain has to rebuild the factor
  // of the update before; the block loop then visits the block a second time at once, so the
  // rebuild runs through the one copy of the factorization
  bool amm_rec = false;
  for (int step = 0; step < A.n_iters; ++step) {
    const int64_t it = A.iter0 + 1 + step;
#ifdef MMB_PHASE_PROF
    const uint64_t _it0 = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (PREDRAW) {
      // (one step in Q; marked so for the block placement: the pass sits out of the iteration's
      // straight line, which also keeps sweep_kernel<rats, Gibbs+AMM> at its 198 spilled VGPRs
      // against 207 unmarked)
      if (__builtin_expect(pre0 == 0, 0)) {
        MMB_PROF_START
        pre = S::predraw(A, chain, it, g);
        MMB_PROF_MARK(15, g.lane)
      }
    }
    for (int b = 0; b < A.nb; ++b) {
      // descriptor read through the constant address space: uniform scalar loads (s_load,
      // scalar cache) instead of vector loads that wait on the vector memory path
      const DBlock& B = mmb_block(A.blocks, b);
      const mmb_rng rn = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_NORMAL);
      const mmb_rng ru = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_UNIFORM);
      const bool adapt = B.adapt == MMB_ADAPT_ALL ? true
                         : B.adapt == MMB_ADAPT_BURNIN ? (it <= A.model_burnin) : false;
      switch (B.kind) {
        case MMB_SAMPLER_AMWG:
          if constexpr ((KINDS >> MMB_SAMPLER_AMWG) & 1u) {
            MMB_PROF_START
            S::amwg(A, B, c, rn, ru, adapt, s, l, g, pk);
            MMB_PROF_MARK(13, g.lane)
          }
          break;
        case MMB_SAMPLER_AMM:
          if constexpr ((KINDS >> MMB_SAMPLER_AMM) & 1u) S::amm(A, B, c, chain, it, b, rn, ru, adapt, s, l, g, lds,
                                                                        G == 32 ? S::lane_value(pre, pre0 + b) : 0.0, pk,
                                                                        amm_rec);
          break;
        case MMB_SAMPLER_SLICE:
          if constexpr ((KINDS >> MMB_SAMPLER_SLICE) & 1u) {
            MMB_PROF_START
            if (B.form == MMB_SLICE_UNIVARIATE) S::slice_uni(A, B, ru, s, l, g, lds);
            else S::slice_multi(A, B, ru, s, l, g, lds);
            MMB_PROF_MARK(14, g.lane)
          }
          break;
        case MMB_SAMPLER_NUTS:
          if constexpr ((KINDS >> MMB_SAMPLER_NUTS) & 1u) S::nuts(A, B, c, it, b, s, g);
          break;
        case MMB_SAMPLER_HMC:
          if constexpr ((KINDS >> MMB_SAMPLER_HMC) & 1u) S::template hmc<false>(A, B, c, rn, ru, s, g);
          break;
        case MMB_SAMPLER_MALA:
          if constexpr ((KINDS >> MMB_SAMPLER_MALA) & 1u) S::template hmc<true>(A, B, c, rn, ru, s, g);
          break;
        case MMB_SAMPLER_RWM:
          if constexpr ((KINDS >> MMB_SAMPLER_RWM) & 1u) S::rwm(A, B, c, chain, it, b, rn, ru, s, l, g, pk);
          break;
        case MMB_SAMPLER_DGS:
          if constexpr ((KINDS >> MMB_SAMPLER_DGS) & 1u)
            S::template dgs<((KINDS >> MMB_SAMPLER_SLICESIMPLEX) & 1u) != 0u>(A, B, ru, s, g);
          break;
        case MMB_SAMPLER_SLICESIMPLEX:
          if constexpr ((KINDS >> MMB_SAMPLER_SLICESIMPLEX) & 1u) {
            const mmb_rng rs = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_SIMPLEX);
            S::slice_simplex(A, B, ru, rs, s, g, M::ssx_rows(A, lds));
          }
          break;
        case MMB_SAMPLER_BMG:
        case MMB_SAMPLER_BMC3:
        case MMB_SAMPLER_BIA:
          if constexpr ((KINDS >> MMB_SAMPLER_BMG) & 1u) {
            const mmb_rng rb = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_BINARY);
            if (B.kind == MMB_SAMPLER_BMG) S::bmg(A, B, c, ru, rb, s, l, g);
            else if (B.kind == MMB_SAMPLER_BMC3) S::bmc3(A, B, c, ru, rb, s, l, g);
            else S::bia(A, B, c, ru, rb, s, l, g);
          }
          break;
        case MMB_SAMPLER_BHMC:
          if constexpr ((KINDS >> MMB_SAMPLER_BHMC) & 1u) {
            const mmb_rng ri = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_INIT);
            S::bhmc(A, B, c, rn, ri, s, l, g);
          }
          break;
        case MMB_SAMPLER_ABC:
          if constexpr ((KINDS >> MMB_SAMPLER_ABC) & 1u) S::abc(A, B, c, chain, it, b, rn, ru, s, g);
          break;
        case MMB_SAMPLER_GIBBS: if constexpr ((KINDS >> MMB_SAMPLER_GIBBS) & 1u) {
          const mmb_rng gn = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_GAMMA_N);
          const mmb_rng gu = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_GAMMA_U);
          MMB_PROF_START
          M::gibbs(A, B, s, l, g, &rn, &gn, &gu, G == 32 ? S::lane_value(pre, pre0 + b) : 0.0);
          MMB_PROF_MARK(7, g.lane)
        }
          break;
        default:
          break;
      }
      M::prep_wrote(pk, B);
      if constexpr (S::CARRY && ((KINDS >> MMB_SAMPLER_AMM) & 1u) != 0u) {
        if (__builtin_expect(__ballot(amm_rec) != 0, 0)) --b;  // (wave-uniform; rare: a rounding event)
      }
    }
#ifdef MMB_PHASE_PROF
    if ((threadIdx.x & 63) == 0) {
      mmb_prof_lds()[8] += __builtin_amdgcn_s_memtime() - _it0;
      mmb_prof_lds()[9] += 1;
    }
#endif
    pre0 += A.nb;
    if (pre0 + A.nb > 32) pre0 = 0;
    if (A.draws && it > A.burnin && (it - A.burnin) % A.thin == 0) {
      const int64_t row = (it - A.burnin) / A.thin - 1 - A.kept_origin;
      M::write_draws(A, s, g, row, c);
    }
  }
  M::store(A, c, g.lane, s);
#ifdef MMB_WAVE_TIMES
  if ((threadIdx.x & 63) == 0 && _wid < MMB_WT_MAX) {  // (a wave slot's launches follow each other: no race)
    const uint64_t _wt1 = __builtin_amdgcn_s_memrealtime();
    if (mmb_wt[3 * _wid] == 0) mmb_wt[3 * _wid] = _wt0;
    mmb_wt[3 * _wid + 1] = _wt1;
    mmb_wt[3 * _wid + 2] += _wt1 - _wt0;
  }
#endif
#ifdef MMB_PHASE_PROF
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < 16; ++i) atomicAdd(&mmb_prof[i], mmb_prof_lds()[i]);
#endif
}

#ifndef MMB_RATS_BLOCK
#define MMB_RATS_BLOCK 256  // rats: threads per workgroup (8 chains)
#endif
template <int MODEL, unsigned KINDS>
__global__ __launch_bounds__(MODEL == MMB_MODEL_RATS && MMB_RATS_BLOCK > 256 ? MMB_RATS_BLOCK : 256,
                             sweep_waves<MODEL>()) void sweep_kernel(const SweepArgs A) {
  sweep_body<MODEL, KINDS>(A);
}

constexpr unsigned K_ALL = (1u << MMB_SAMPLER_AMWG) | (1u << MMB_SAMPLER_AMM) |
                         (1u << MMB_SAMPLER_SLICE) | (1u << MMB_SAMPLER_GIBBS);
constexpr unsigned K_GRAD = (1u << MMB_SAMPLER_NUTS) | (1u << MMB_SAMPLER_HMC) | (1u << MMB_SAMPLER_MALA);
constexpr unsigned K_ALL_GRAD = K_ALL | K_GRAD;
constexpr unsigned K_GIBBS_AMM = (1u << MMB_SAMPLER_AMM) | (1u << MMB_SAMPLER_GIBBS);
constexpr unsigned K_SLICE_AMWG = (1u << MMB_SAMPLER_AMWG) | (1u << MMB_SAMPLER_SLICE);
constexpr unsigned K_IR = (1u << MMB_SAMPLER_AMWG) | (1u << MMB_SAMPLER_AMM) | (1u << MMB_SAMPLER_SLICE) |
                         (1u << MMB_SAMPLER_GIBBS) | K_GRAD;
// RWM is compiled only into kernels of their own, which schemes that hold an RWM block take
// (sweep.hip): the instantiations above keep their masks, and so their code
constexpr unsigned K_RWM = 1u << MMB_SAMPLER_RWM;
// DGS likewise (node-IR models only): one more instantiation, which also holds RWM, so that a scheme
// may mix DGS blocks with every other kind
constexpr unsigned K_DGS = 1u << MMB_SAMPLER_DGS;
// SliceSimplex likewise: the instantiation that schemes with such a block take holds every other kind
constexpr unsigned K_SIMPLEX = 1u << MMB_SAMPLER_SLICESIMPLEX;
// The binary samplers BMG, BMC3 and BIA likewise: one instantiation for the three, which holds every other kind
constexpr unsigned K_BIN = (1u << MMB_SAMPLER_BMG) | (1u << MMB_SAMPLER_BMC3) | (1u << MMB_SAMPLER_BIA);
// BHMC likewise: one further instantiation, which holds every other kind
constexpr unsigned K_BHMC = 1u << MMB_SAMPLER_BHMC;
// ABC likewise: one further instantiation, which holds every other kind
constexpr unsigned K_ABC = 1u << MMB_SAMPLER_ABC;

