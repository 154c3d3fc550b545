// samplers.h — block updates of src/samplers/{amwg,amm,slice}.jl for one chain
// advanced by a group of G lanes (element e of the block vector in lane e % G,
// register slot e / G).  RNG consumption follows mmb_math.h's documented layout and
// is mirrored draw for draw by oracle/oracle.c.
#pragma once
#include "models.h"
#include "hmc.h"
#include "nuts.h"

// Whether model M evaluates logpdf! in the chain state itself (Mdl<MMB_MODEL_IR>::NOPROP in the
// specialised AMM / Gibbs kernels); false for models without the member.  amm() keeps a copy of
// the old value only for these: the copy would serve every model (same products), but the line
// and rats kernels are tuned to their register budgets, and with the split their instruction
// streams are the ones they had (compared function by function in the device assembly of
// sweep.hip) -- the simpler form's register cost in them has not been measured.
template <class M, class = void>
struct mmb_noprop {
  static constexpr bool value = false;
};
template <class M>
struct mmb_noprop<M, decltype((void)M::NOPROP)> {
  static constexpr bool value = M::NOPROP;
};

template <class M>
struct Smp {
  static constexpr int G = M::G, R = M::R, DMAX = M::DMAX, DP = M::DP, TP = M::TP;
  static constexpr int NT = (TP + G - 1) / G;  // packed-triangle slots per lane
  using St = typename M::St;
  using Lc = typename M::Lc;

  // ---------------------------------------------------------------- batched draws
  // Variates that do not depend on the chain state -- per block of an iteration its Gibbs
  // variate (Mdl::gibbs_draw_kind: Gamma(a) by Marsaglia-Tsang or a standard normal) or its
  // AMM accept uniform -- drawn for Q = max(1, 32 / nb) consecutive iterations in one pass
  // (32-lane groups): lane l holds block l % nb of iteration it + l / nb, lanes from Q * nb on
  // draw nothing that is used.  They depend only on (seed, chain, iteration, block, substream)
  // and the block descriptors, so the pass fills the lanes one iteration leaves idle with the
  // following iterations' draws and the sweep runs it on every Q-th iteration (sweep.h).  Same
  // substreams, counters and operations as the per-block draws of each iteration
  // (mmb_gamma_mt is replayed in full whenever its first attempt does not accept), so the
  // values are bit-identical to drawing them inside the blocks.
  __device__ __forceinline__ static double predraw(const SweepArgs& A, uint32_t chain, int64_t it,
                                                   const Grp<G>& g) {
    // q = lane / nb capped at Q - 1, by uniform steps over the batch's iterations (no per-lane
    // division); a lane past the batch then has bl >= nb, matches no block and keeps kind 0
    int q = 0;
    for (int t = A.nb; A.nb > 0 && t + A.nb <= 32; t += A.nb) q += g.lane >= t ? 1 : 0;
    const int bl = g.lane - q * A.nb;
    int kind = 0;  // 0 none, 1 Gamma(a), 2 normal, 3 uniform
    double a = 0.0;
    for (int b = 0; b < A.nb; ++b) {
      const DBlock& B = mmb_block(A.blocks, b);
      double ab = 0.0;
      int k = 0;
      if (B.kind == MMB_SAMPLER_GIBBS) k = M::gibbs_draw_kind(B, &ab);
      else if (B.kind == MMB_SAMPLER_AMM) k = 3;
      kind = bl == b ? k : kind;
      a = bl == b ? ab : a;
    }
    const uint32_t b = (uint32_t)bl;
    const uint32_t itq = (uint32_t)(it + (int64_t)q);  // the iteration's own Philox key (64-bit sum, then cut)
    const mmb_rng rn = mmb_rng_make(A.seed, chain, itq, b, kind == 1 ? MMB_SUB_GAMMA_N : MMB_SUB_NORMAL);
    const mmb_rng ru = mmb_rng_make(A.seed, chain, itq, b, kind == 1 ? MMB_SUB_GAMMA_U : MMB_SUB_UNIFORM);
    const double x = mmb_normal(&rn, 0u);
    const double u = mmb_uniform(&ru, 0u);
    if (kind != 1) return kind == 2 ? x : u;
    // mmb_gamma_mt's first attempt (normal #0, uniform #0)
    const double d = a - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    double v = 1.0 + c * x;
    bool ok = false;
    double r = 0.0;
    if (v > 0.0) {
      v = v * v * v;
      const double x2 = x * x;
      if (u < 1.0 - 0.0331 * (x2 * x2)) ok = true;
      else if (mmb_log(u) < 0.5 * x2 + d * (1.0 - v + mmb_log(v))) ok = true;
      r = d * v;
    }
    if (!ok) {
      uint32_t kn = 0, ku = 0;
      r = mmb_gamma_mt(a, &rn, &ru, &kn, &ku);
    }
    return r;
  }
  // value of lane b (group-relative, wave-uniform b) of each 32-lane group
  __device__ __forceinline__ static double lane_value(double v, int b) {
    const uint64_t u = mmb_d2u(v);
    const int lo = (int)(uint32_t)u, hi = (int)(uint32_t)(u >> 32);
    const uint32_t lo0 = (uint32_t)__builtin_amdgcn_readlane(lo, b), hi0 = (uint32_t)__builtin_amdgcn_readlane(hi, b);
    const uint32_t lo1 = (uint32_t)__builtin_amdgcn_readlane(lo, b + 32), hi1 = (uint32_t)__builtin_amdgcn_readlane(hi, b + 32);
    const bool up = (threadIdx.x & 32) != 0;
    return mmb_u2d((uint64_t)(up ? lo1 : lo0) | ((uint64_t)(up ? hi1 : hi0) << 32));
  }

  // ---------------------------------------------------------------- AMWG
  // amwg_sub! decided for every coordinate at once (blocks whose logpdf is a butterfly over
  // per-lane terms that only the lane's own element changes: M::AMWG_SEP).  Coordinate j's
  // step compares its uniform with exp(delta_j), delta_j = logf(state with x_j') - logf0, two
  // rounded evaluations whose states differ only in lane j's terms; in exact arithmetic the
  // difference is d_j = (tp_j' - tp_j) - 0.5 invv (ts_j' - ts_j) whatever the other
  // coordinates' accept history.  Each rounded logf is within 9 u (sum_i |tp_i| + |yk| +
  // invv sum_i |ts_i|) of its exact value (a depth-5 tree sum, then three roundings), so
  // |delta_j - d_j| <= eps_j with the factor of 128 u taken below; a decision is CERTAIN
  // when the uniform is outside [exp(d_j - eps_j), exp(d_j + eps_j)] widened by the
  // (sub-ulp) error of mmb_exp.  All certain: x_j' where accepted -- the same values and
  // accept counts as the sequential loop, bit for bit, since certain decisions are its
  // decisions.  Any uncertain lane, a non-finite term or bound: false, and the caller runs
  // the sequential loop (RNG draws are the same precomputed z / uown either way).
  // The model gives, per lane j, d_j and the magnitude epsm_j its rounding band scales with
  // (M::amwg_dm: rats models.h, the node IR's separable blocks ir.h), and the band's relative
  // factor (M::amwg_epsf).
  __device__ __forceinline__ static bool amwg_lanes(const DBlock& B, const typename M::Prep& pc, const St& s,
                                                    const Lc& l, const Grp<G>& g, double* x, const double* z,
                                                    const double* uown, double* acc, double ad,
                                                    const SweepArgs& A) {
    const bool in = g.lane < B.d;
    const double x1 = x[0] + z[0];  // the sequential loop's x[r] += z[r]
    double del, epsm;
    bool bad;
    M::amwg_dm(A, B, pc, s, l, g, x[0], x1, del, epsm, bad);
    // (amwg_exact = 2, tests: a 2^30 times wider band, so that many updates fall back)
    const double eps = (A.amwg_exact == 2 ? 0x1p30 * M::amwg_epsf(B) : M::amwg_epsf(B)) * epsm;
    const double lo = del - eps, hi = del + eps;
    const double ue = uown[0];  // in [0, 1)
    const bool acc_c = lo >= 700.0 || (lo > -700.0 && ue < mmb_exp(lo) * (1.0 - 0x1p-48));
    const bool rej_c = (hi <= -700.0 && ue >= 1e-300) ||
                       (hi > -700.0 && hi < 700.0 && ue >= mmb_exp(hi) * (1.0 + 0x1p-48));
    bad = bad || !isfinite(eps);
    const bool unsure = in && (bad || !(acc_c || rej_c));
    const uint64_t bal = __ballot(unsure);
    const bool any = (threadIdx.x & 32) ? (bal >> 32) != 0 : (uint32_t)bal != 0;
    if (any) return false;
    if (in && acc_c) {
      x[0] = x1;
      acc[0] += ad;
    }
    return true;
  }

  // amwg.jl:68-115 (sample!, setadapt!, amwg_sub!).
  __device__ __forceinline__ static void amwg(const SweepArgs& A, const DBlock& B, int c, const mmb_rng& rn,
                              const mmb_rng& ru, bool adapt, St& s, const Lc& l, const Grp<G>& g,
                              typename M::PrepCache& pk) {
    const int d = B.d;
    double x[R], sig[R], acc[R], z[R];
    M::unlist(B, s, g.lane, x);
    int m = B.t_m[c];
    int fl = B.t_flags[c];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int e = r * G + g.lane;
      sig[r] = e < d ? B.t_sigma[(size_t)c * DP + e] : 0.0;
      acc[r] = e < d ? B.t_accept[(size_t)c * DP + e] : 0.0;
    }
    if (adapt && !(fl & 1)) {  // setadapt!: accept[:] = 0, m = 0
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.0;
      m = 0;
    }
    fl = adapt ? (fl | 1) : (fl & ~1);
    const double ad = adapt ? 1.0 : 0.0;
    if (adapt) m += 1;
    const typename M::Prep pc = M::prep(B, s, g, pk);
    // the proposal normals and (lane groups) the accept uniforms of every element at once,
    // element e on its own lane: the same Philox draws (index e) the sequential loop below
    // consumes, so the values are bit-identical; each step then takes its uniform from lane e
    // (readlane) instead of every lane recomputing it (-~60 VALU per coordinate)
    double uown[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int e = r * G + g.lane;
      z[r] = e < d ? sig[r] * mmb_normal(&rn, 2u * (uint32_t)e) : 0.0;
      uown[r] = (G > 1 && e < d) ? mmb_uniform(&ru, (uint32_t)e) : 0.0;
    }
    bool seq = true;
    if constexpr (M::AMWG_SEP && G == 32 && R == 1) {
      if (M::AMWG_PROBE && A.amwg_probe != 0 && M::amwg_sep(B)) {
        // test-only (MMB_AMWG_PROBE=1, rats): uniforms a few ulps to 2^-12 off each coordinate's
        // accept threshold exp(d_j) (mmb_math.h mmb_amwg_probe_factor; the oracle draws the same),
        // so both the lane-parallel decision and its sequential fallback meet near-ties
        double del, em;
        bool bd;
        M::amwg_dm(A, B, pc, s, l, g, x[0], x[0] + z[0], del, em, bd);
        uown[0] = g.lane < d ? mmb_amwg_probe_uniform(del, &ru, (uint32_t)g.lane) : 0.0;
      }
      if (A.amwg_exact != 1 && M::amwg_sep(B)) {
        seq = !amwg_lanes(B, pc, s, l, g, x, z, uown, acc, ad, A);
        if (seq && g.lane == 0) atomicAdd(&A.nuts_stat[5], 1ull);
      }
    }
    if (seq) {  // amwg_sub!: one coordinate at a time, the block's logpdf at every proposal
      double logf0 = M::logf_p(A, B, pc, s, l, g, x);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        for (int ln = 0; ln < G; ++ln) {
          int e = r * G + ln;
          if (e >= d) break;
          bool own = g.lane == ln;
          double xo = x[r];
          if (own) x[r] += z[r];
          double lpp = M::logf_p(A, B, pc, s, l, g, x);
          const double ue = G == 32 ? lane_value(uown[r], ln) : mmb_uniform(&ru, (uint32_t)e);
          if (ue < mmb_exp(lpp - logf0)) {
            logf0 = lpp;
            if (own) acc[r] += ad;
          } else if (own) {
            x[r] = xo;
          }
        }
      }
    }
    if (adapt && m % B.batchsize == 0) {  // amwg.jl:74-79 ((m/b)^-0.5 as 1/sqrt(m/b))
      double q = (double)m / (double)B.batchsize;
      double delta = 1.0 / sqrt(q);
      if (0.01 < delta) delta = 0.01;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double eps = (acc[r] / (double)m < B.target) ? -delta : delta;
        sig[r] *= mmb_exp(eps);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int e = r * G + g.lane;
      if (e < d) {
        B.t_sigma[(size_t)c * DP + e] = sig[r];
        B.t_accept[(size_t)c * DP + e] = acc[r];
      }
    }
    if (g.lane == 0) { B.t_m[c] = m; B.t_flags[c] = fl; }
    M::relist(B, s, g, x);
  }

  // ---------------------------------------------------------------- RWM
  // rwm.jl:65-71 (sample!): x = v + scale .* rand(proposal(0.0, 1.0), n), accepted iff
  // rand() < exp(logpdf!(block, x) - logpdf!(block, v)); both log densities are evaluated at every
  // update (the reference caches nothing) and nothing adapts.  v is unlisted with transform
  // (rwm.jl:52).  A NaN ratio rejects and +inf accepts by the comparison itself.  Element e's
  // variate is drawn by the lane that owns it: normal #e of the block's MMB_SUB_NORMAL stream, or
  // symdist.h's variate of coordinate e on MMB_SUB_PROPOSAL; the accept uniform is #0 of
  // MMB_SUB_UNIFORM.  Tune: scale[d] per chain (RWMTune.scale, B.t_sigma); the update and accept
  // counts (mmb_rwm_stats) are added by lane 0 with no-return atomics, as amm_count's.
  __device__ __forceinline__ static void rwm(const SweepArgs& A, const DBlock& B, int c, uint32_t chain, int64_t it,
                                             int b, const mmb_rng& rn, const mmb_rng& ru, St& s, const Lc& l,
                                             const Grp<G>& g, typename M::PrepCache& pk) {
    const int d = B.d;
    const mmb_rng rp = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_PROPOSAL);
    double v[R], x[R];
    M::unlist(B, s, g.lane, v);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int e = r * G + g.lane;
      double sc = 0.0, z = 0.0;
      if (e < d) {
        sc = B.t_sigma[(size_t)c * DP + e];
        z = B.form == MMB_RWM_NORMAL ? mmb_normal(&rn, (uint32_t)e) : mmb_symdist(B.form, &rp, (uint32_t)e);
      }
      x[r] = v[r] + sc * z;
    }
    const typename M::Prep pc = M::prep(B, s, g, pk);
    double lx, lv;
    M::logf_p2(A, B, pc, s, l, g, x, v, lx, lv);
    const bool acc = mmb_uniform(&ru, 0u) < mmb_exp(lx - lv);
    if (acc) {
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = x[r];
    }
    if (g.lane == 0 && B.t_astat != nullptr) {
      uint64_t* a = B.t_astat + (size_t)c * MMB_AMM_STAT_STRIDE;
      (void)__hip_atomic_fetch_add(a + 0, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (acc) (void)__hip_atomic_fetch_add(a + 1, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    M::relist(B, s, g, v);
  }

  // ---------------------------------------------------------------- DGS
  // dgs.jl:56-126 (DGS(params), sample!, mass): the full conditional of each element of the block's
  // one discrete node, by enumeration of the element's support (node-IR models; M::dgs_* in ir.h).
  // Elements are updated in order and each sees the earlier ones' new values.  For element e, the
  // k-th support value (ascending) is written into the state and mass_k = exp(logpdf(d_e, s_k) +
  // logpdf(model, targets)) is evaluated by all 32 lanes (the targets' element terms lane-parallel,
  // M::dgs_lp); lane k keeps mass_k in a register -- at most 32 masses, one per lane, nothing goes
  // to memory.  Then, the same on every lane, psum = mass_0 + mass_1 + ... in k order,
  // probs_k = psum > 0 ? mass_k / psum : 1 / n (dgs.jl:119-121), and the value is the smallest k
  // whose running sum probs_0 + ... + probs_k exceeds u (the last value if none does), u = uniform #e
  // of the block's MMB_SUB_UNIFORM stream: rand(Categorical(probs)) by inversion.  No tune state.
  // A psum that is not finite (a mass overflowed to +Inf, or a NaN log density) has no probability
  // vector: the reference throws inside Categorical(probs); here the element keeps the value it had
  // before the update.  u is indexed by the element, so that draws nothing out of order.
  // SX: the kernel also holds SliceSimplex, so a target may read a sampled Dirichlet node (ir.h elem_lp)
  template <bool SX = false>
  __device__ __forceinline__ static void dgs(const SweepArgs& A, const DBlock& B, const mmb_rng& ru, St& s,
                                             const Grp<G>& g) {
    static_assert(G == 32, "DGS keeps one mass per lane of a 32-lane group");
    const int len = M::dgs_elems(s, B);
    for (int e = 0; e < len; ++e) {
      double lo;
      const int n = M::dgs_support(A, B, s, e, g.lane, &lo);
      const double old = M::dgs_get(B, s, e);
      double mass = 0.0;
      for (int k = 0; k < n; ++k) {
        M::dgs_set(B, s, e, lo + (double)k, g.lane);
        const double m = mmb_exp(M::template dgs_lp<SX>(A, B, s, g, e, lo + (double)k));
        mass = g.lane == k ? m : mass;
      }
      double psum = 0.0;
      for (int k = 0; k < n; ++k) psum = psum + lane_value(mass, k);
      const double u = mmb_uniform(&ru, (uint32_t)e);
      double v = old;
      if (isfinite(psum)) {
        const double unif = 1.0 / (double)n;
        double cum = 0.0;
        int pick = n - 1;
        bool found = false;
        for (int k = 0; k < n; ++k) {
          cum = cum + (psum > 0.0 ? lane_value(mass, k) / psum : unif);
          if (!found && cum > u) {
            pick = k;
            found = true;
          }
        }
        v = lo + (double)pick;
      }
      M::dgs_set(B, s, e, v, g.lane);
    }
  }

  // ---------------------------------------------------------------- BMG, BMC3, BIA
  // The binary samplers (bmg.jl:57-101, bmc3.jl:57-65, bia.jl:70-119) of the block's one Bernoulli or
  // DiscreteUniform(0, 1) node of n = B.d <= 32 elements (node-IR models), element i on lane i.
  // logf(x) is M::logf: logpdf!(block, x), the node's own term and its targets in the block's term
  // order, with the early exit on a non-finite running sum; the targets' element terms are evaluated
  // by all 32 lanes.  The two chains of a wave take their branches on their own, and every cross-lane
  // step (the 32-wide shuffles, lane_value, the DPP sums inside logf) stays within the chain's own 32
  // lanes.  Element sets are 32-bit masks, bit i for element i.  rb is the block's MMB_SUB_BINARY
  // stream, ru its MMB_SUB_UNIFORM stream.  Updates and accepts are counted as RWM's (mmb_rwm_stats).
  //
  // The index set (randind; the reference's StatsBase.sample cannot be restated):
  //   int k    a partial Fisher-Yates shuffle of 0..n-1, position p on lane p: for j = 0..k-1,
  //            r = j + min(floor(u_j (n - j)), n - j - 1), u_j = uniform #j of rb, swap positions j and r;
  //            the set is the first k positions
  //   lists    list number min(floor(u_0 m), m - 1) of the m lists (B.width: one mask per list)
  __device__ __forceinline__ static uint32_t bin_index_set(const DBlock& B, const mmb_rng& rb, const Grp<G>& g) {
    const int n = B.d < 32 ? B.d : 32;
    const uint32_t all = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
    if (B.form == MMB_BINARY_K_LISTS) {
      const int m = B.batchsize;
      int q = (int)(mmb_uniform(&rb, 0u) * (double)m);
      q = q < m - 1 ? q : m - 1;
      q = q > 0 ? q : 0;
      return (uint32_t)B.width[q] & all;
    }
    const int k = B.batchsize < n ? B.batchsize : n;
    int perm = g.lane;
    uint32_t set = 0u;
    for (int j = 0; j < k; ++j) {
      const int left = n - j;
      int t = (int)(mmb_uniform(&rb, (uint32_t)j) * (double)left);
      t = t < left - 1 ? t : left - 1;
      const int r = j + (t > 0 ? t : 0);
      const int pr = __shfl(perm, r, 32), pj = __shfl(perm, j, 32);
      perm = g.lane == j ? pr : (g.lane == r ? pj : perm);
      set |= 1u << (uint32_t)(pr & 31);
    }
    return set & all;
  }
  __device__ __forceinline__ static void bin_count(const DBlock& B, int c, bool acc, const Grp<G>& g) {
    if (g.lane == 0 && B.t_astat != nullptr) {
      uint64_t* a = B.t_astat + (size_t)c * MMB_AMM_STAT_STRIDE;
      (void)__hip_atomic_fetch_add(a + 0, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (acc) (void)__hip_atomic_fetch_add(a + 1, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // t_i summed over the elements i of `set` in ascending order, t_i on lane i
  __device__ __forceinline__ static double bin_set_sum(double t, uint32_t set) {
    double q = 0.0;
    for (uint32_t rem = set; rem != 0u; rem &= rem - 1u) q = q + __shfl(t, (int)__builtin_ctz(rem), 32);
    return q;
  }

  // BMC3 (bmc3.jl:57-65): the elements of the index set are flipped, and the candidate x is accepted iff
  // u < exp(logf(x) - logf(v)), u = uniform #0 of ru.  Two evaluations of logf.  A NaN ratio rejects.
  __device__ __forceinline__ static void bmc3(const SweepArgs& A, const DBlock& B, int c, const mmb_rng& ru,
                                              const mmb_rng& rb, St& s, const Lc& l, const Grp<G>& g) {
    static_assert(G == 32 && R == 1, "the binary samplers keep one element per lane of a 32-lane group");
    double v[R], x[R];
    M::unlist(B, s, g.lane, v);
    const uint32_t set = bin_index_set(B, rb, g);
    x[0] = ((set >> (uint32_t)g.lane) & 1u) != 0u ? 1.0 - v[0] : v[0];
    const double lx = M::logf(A, B, s, l, g, x);
    const double lv = M::logf(A, B, s, l, g, v);
    const bool acc = mmb_uniform(&ru, 0u) < mmb_exp(lx - lv);
    if (acc) v[0] = x[0];
    bin_count(B, c, acc, g);
    M::relist(B, s, g, v);
  }

  // BMG's pbernoulli! (bmg.jl:62-77) at x, lf = logf(x): for each i of the set, ascending,
  // p_i = invlogit(logf(x | x_i = 1) - logf(x | x_i = 0)), replaced by 0.5 unless 0 < p_i < 1 (a NaN
  // fails that test too).  One of the two configurations is x itself, so each i costs one evaluation
  // of logf, at x with element i flipped; the reference evaluates both, which gives the same values
  // because logf is a deterministic function of the state.  Lane i keeps p_i in a register, as DGS
  // keeps its masses; nothing goes to memory.
  __device__ static double bmg_probs(const SweepArgs& A, const DBlock& B, const St& s, const Lc& l, const Grp<G>& g,
                                     const double* x, double lf, uint32_t set) {
    double p = 0.5;
    for (uint32_t rem = set; rem != 0u; rem &= rem - 1u) {
      const int i = (int)__builtin_ctz(rem);
      const double xi = __shfl(x[0], i, 32);
      double y[R];
      y[0] = g.lane == i ? 1.0 - x[0] : x[0];
      const double lo = M::logf(A, B, s, l, g, y);
      const double pi = mmb_invlogit(xi == 1.0 ? lf - lo : lo - lf);
      p = g.lane == i ? ((0.0 < pi && pi < 1.0) ? pi : 0.5) : p;
    }
    return p;
  }
  // BMG (bmg.jl:57-101): theta_i = (uniform #(1 + i) of ru < p_i) for i in the set, y = x with theta
  // written in, qy = sum_i log(y_i == 1 ? p_i : 1 - p_i) with p at x, qx the same for x with p at y (both
  // over the set in ascending order), accepted iff u < exp((logf(y) - qy) - (logf(x) - qx)), u = uniform
  // #0 of ru.  n = 1 takes the reference's direct branch: theta is the new value, no accept step (counted
  // as accepted).  k + 1 evaluations of logf for x and k + 1 for y: 2k + 2 against the reference's 4k + 2.
  __device__ __forceinline__ static void bmg(const SweepArgs& A, const DBlock& B, int c, const mmb_rng& ru,
                                             const mmb_rng& rb, St& s, const Lc& l, const Grp<G>& g) {
    static_assert(G == 32 && R == 1, "the binary samplers keep one element per lane of a 32-lane group");
    double v[R], y[R];
    M::unlist(B, s, g.lane, v);
    const uint32_t set = bin_index_set(B, rb, g);
    const bool in = ((set >> (uint32_t)g.lane) & 1u) != 0u;
    const double lfx = M::logf(A, B, s, l, g, v);
    const double px = bmg_probs(A, B, s, l, g, v, lfx, set);
    const double theta = mmb_uniform(&ru, 1u + (uint32_t)g.lane) < px ? 1.0 : 0.0;
    y[0] = in ? theta : v[0];
    bool acc = true;
    if (B.d > 1) {
      const double qy = bin_set_sum(y[0] == 1.0 ? mmb_log(px) : mmb_log(1.0 - px), set);
      const double lfy = M::logf(A, B, s, l, g, y);
      const double py = bmg_probs(A, B, s, l, g, y, lfy, set);
      const double qx = bin_set_sum(v[0] == 1.0 ? mmb_log(py) : mmb_log(1.0 - py), set);
      acc = mmb_uniform(&ru, 0u) < mmb_exp((lfy - qy) - (lfx - qx));
    }
    if (acc) v[0] = y[0];
    bin_count(B, c, acc, g);
    M::relist(B, s, g, v);
  }

  // BIA (bia.jl:70-119).  Lane j proposes for element j with u_j = uniform #j of rb: a 0 becomes 1 iff
  // u_j < A_j (added), a 1 becomes 0 iff u_j < D_j (deleted); q_ratio is the product over j ascending of
  // D_j / A_j (added), A_j / D_j (deleted), 1 (kept); alpha = min(1, exp(logf(x) - logf(v)) q_ratio).
  // Then A_j and D_j adapt (bia.jl:101-111; every j, whether it moved or not), with iter^(-decay) as
  // exp(-decay log(iter)), and the proposal is accepted iff uniform #0 of ru < alpha.  The adaptation
  // never switches off (the reference has no adapt flag here).  Tune per chain: iter (B.t_m), A
  // (B.t_sigma), D (B.t_accept); epsilon = B.scale, decay = B.beta, target = B.target.
  // A NaN alpha would turn every A_j and D_j into NaN in the reference (0 * NaN) and the sampler would
  // be dead from then on; here it rejects and leaves the tune row, iter included, as it was.
  __device__ __forceinline__ static void bia(const SweepArgs& A, const DBlock& B, int c, const mmb_rng& ru,
                                             const mmb_rng& rb, St& s, const Lc& l, const Grp<G>& g) {
    static_assert(G == 32 && R == 1, "the binary samplers keep one element per lane of a 32-lane group");
    const int d = B.d < 32 ? B.d : 32;
    const bool in = g.lane < d;
    double v[R], x[R];
    M::unlist(B, s, g.lane, v);
    const size_t at = (size_t)c * DP + (size_t)g.lane;
    const double Aj = in ? B.t_sigma[at] : 0.5, Dj = in ? B.t_accept[at] : 0.5;
    const int iter = B.t_m[c] + 1;
    const double eps = B.scale;
    const double uj = mmb_uniform(&rb, (uint32_t)g.lane);
    const bool add = in && v[0] == 0.0 && uj < Aj;
    const bool del = in && v[0] != 0.0 && uj < Dj;
    x[0] = add ? 1.0 : (del ? 0.0 : v[0]);
    const double f = add ? Dj / Aj : (del ? Aj / Dj : 1.0);
    double q = 1.0;
    for (int j = 0; j < d; ++j) q = q * lane_value(f, j);
    const double lx = M::logf(A, B, s, l, g, x);
    const double lv = M::logf(A, B, s, l, g, v);
    const double r = mmb_exp(lx - lv) * q;
    bool acc = false;
    if (r == r) {
      const double alpha = r < 1.0 ? r : 1.0;
      const double gn = mmb_exp(-B.beta * mmb_log((double)iter));
      if (in) {
        const double ca = mmb_log((Aj - eps) / (1.0 - Aj - eps)) + gn * (add ? 1.0 : 0.0) * (alpha - B.target);
        const double ea = mmb_exp(ca);
        B.t_sigma[at] = (ea * (1.0 - eps) + eps) / (1.0 + ea);
        const double cd = mmb_log((Dj - eps) / (1.0 - Dj - eps)) + gn * (del ? 1.0 : 0.0) * (alpha - B.target);
        const double ed = mmb_exp(cd);
        B.t_accept[at] = (ed * (1.0 - eps) + eps) / (1.0 + ed);
      }
      if (g.lane == 0) B.t_m[c] = iter;
      acc = mmb_uniform(&ru, 0u) < alpha;
    }
    if (acc) v[0] = x[0];
    bin_count(B, c, acc, g);
    M::relist(B, s, g, v);
  }

  // ---------------------------------------------------------------- BHMC
  // Binary Hamiltonian Monte Carlo (bhmc.jl:50-122) of the block's one Bernoulli or DiscreteUniform(0, 1)
  // node of n = B.d <= 32 elements, element i on lane i.  The sampler's state is a particle: lane i keeps
  // position_i, velocity_i and the side S_i of its wall (as x_i = 1 for S_i = +1, 0 for -1) in registers
  // for the whole update; the per-element arithmetic is bhmc.h's.  Tune per chain: position (B.t_sigma),
  // velocity (B.t_accept), wallhits and wallcrosses (B.t_hmc, doubles: exact to 2^53, so they do not wrap
  // at 2^31), initialised (B.t_m).  traveltime = B.scale, refresh = B.form.
  //
  // A chain that is not initialised draws its particle first: position_i = normal #i, velocity_i = normal
  // #(32 + i) of ri, the block's MMB_SUB_INIT stream (the reference's randn(n) when the tune is built,
  // bhmc.jl:17).  With refresh, velocity_i = normal #i of rn, the block's MMB_SUB_NORMAL stream, at the
  // start of every update (an extension: the reference never redraws it).  The sides come from the
  // position (bhmc.jl:58), not from the node's value; S_i = -1 for position_i <= 0.
  //
  // One wall event: the walltimes lane-parallel, the last-hit guard on lane j, a (min, lowest index)
  // reduction over the chain's 32 lanes (lanes >= n hold +Inf), one mmb_sincos of the move time, the move
  // lane-parallel, and on lane j the bounce.  Of the two configurations at a wall one is the current S,
  // whose logf is carried: one evaluation of logf at the start and one per event (the reference: two per
  // event; the same values, logf being a deterministic function of the state).  logf itself is evaluated
  // by all 32 lanes.  The two chains of a wave run their own event counts, and every cross-lane step (the
  // DPP stages of the reduction, the 32-wide shuffles, the ballot of grp_any, the DPP sums inside logf)
  // stays within the chain's own 32 lanes.
  //
  // The loop ends by construction: an element hits its wall once per pi of time, so an update has at most
  // n (floor(traveltime / pi) + 1) events, and the loop makes at most cap = n (floor(traveltime / pi) + 2)
  // trips, the last of which has to be the final partial move.  A stall -- a zero move time (the
  // reference's error), a NaN among the walltimes, or cap trips without reaching traveltime -- ends the
  // update with the node's value and the whole tune row as they were before it.  Updates are counted as
  // RWM's, an accept being an update that ran to traveltime (mmb_rwm_stats).
  template <int S_>
  __device__ __forceinline__ static void bhmc_amin_stage(double& key, int& idx) {
    const double ok = Grp<G>::template other_d<S_>(key);
    const int oi = Grp<G>::template other_i<S_>(idx);
    const bool take = (ok < key) || (ok == key && oi < idx);
    key = take ? ok : key;
    idx = take ? oi : idx;
  }
  __device__ static void bhmc(const SweepArgs& A, const DBlock& B, int c, const mmb_rng& rn, const mmb_rng& ri, St& s,
                              const Lc& l, const Grp<G>& g) {
    static_assert(G == 32 && R == 1, "the binary samplers keep one element per lane of a 32-lane group");
    const int n = B.d < 32 ? B.d : 32;
    const bool in = g.lane < n;
    const size_t at = (size_t)c * DP + (size_t)g.lane;
    const double T = B.scale;
    double v[R], x[R];
    M::unlist(B, s, g.lane, v);
    double pos, vel;
    if (B.t_m[c] == 0) {
      pos = mmb_normal(&ri, (uint32_t)g.lane);
      vel = mmb_normal(&ri, 32u + (uint32_t)g.lane);
    } else {
      pos = in ? B.t_sigma[at] : 0.0;
      vel = in ? B.t_accept[at] : 0.0;
    }
    if (B.form != 0) vel = mmb_normal(&rn, (uint32_t)g.lane);
    x[0] = (in && pos > 0.0) ? 1.0 : 0.0;
    double lf = M::logf(A, B, s, l, g, x);
    const int cap = n * ((int)floor(T / MMB_BHMC_PI) + 2);
    double total = 0.0;
    int j = -1, hits = 0, crosses = 0;
    bool done = false;
#pragma unroll 1
    for (int ev = 0; ev < cap; ++ev) {
      double wt = mmb_bhmc_walltime(vel, pos);
      if (g.lane == j) wt = mmb_bhmc_guard(wt);
      wt = in ? wt : __builtin_inf();
      if (grp_any(wt != wt)) break;
      double mt = wt;
      int jj = g.lane;
      bhmc_amin_stage<0>(mt, jj); bhmc_amin_stage<1>(mt, jj); bhmc_amin_stage<2>(mt, jj);
      bhmc_amin_stage<3>(mt, jj); bhmc_amin_stage<4>(mt, jj);
      if (mt == 0.0) break;
      j = jj;
      if (mt == __builtin_inf()) mt = MMB_BHMC_PI;
      total = total + mt;
      const bool last = total >= T;
      if (last) mt = mt - (total - T);
      double sn, cs, a1, b1;
      mmb_sincos(mt, &sn, &cs);
      mmb_bhmc_move(vel, pos, sn, cs, &a1, &b1);
      vel = a1;
      pos = b1;
      if (last) {
        done = true;
        break;
      }
      ++hits;
      if (g.lane == j) pos = 0.0;
      double y[R];
      y[0] = g.lane == j ? 1.0 - x[0] : x[0];
      const double lo = M::logf(A, B, s, l, g, y);
      const double xj = __shfl(x[0], j, 32), vj = __shfl(vel, j, 32);
      int crossed;
      const double vn = mmb_bhmc_bounce(vj, xj == 1.0 ? lf - lo : lo - lf, &crossed);
      if (g.lane == j) vel = vn;
      if (crossed) {
        x[0] = y[0];
        lf = lo;
        ++crosses;
      }
    }
    if (done) {
      if (in) {
        B.t_sigma[at] = pos;
        B.t_accept[at] = vel;
        v[0] = pos > 0.0 ? 1.0 : 0.0;
      }
      if (g.lane == 0) {
        B.t_m[c] = 1;
        B.t_hmc[2 * (size_t)c] = B.t_hmc[2 * (size_t)c] + (double)hits;
        B.t_hmc[2 * (size_t)c + 1] = B.t_hmc[2 * (size_t)c + 1] + (double)crosses;
      }
    }
    bin_count(B, c, done, g);
    M::relist(B, s, g, v);
  }

  // ---------------------------------------------------------------- ABC
  // Approximate Bayesian computation (abc.jl:36-144) of the block's continuous nodes, d = B.d <= 32
  // coordinates unlisted with transform, coordinate e on lane e (node-IR models).  No likelihood is
  // evaluated: up to maxdraw = B.batchsize rounds of propose, simulate nsim = B.adapt data sets from the
  // block's data nodes at the candidate, summarise them, measure the distance to the observed summaries,
  // weight by the kernel density (abc.h), accept or reject.  proposal = B.form & 0xff, kernel =
  // (B.form >> 8) & 0xff, randeps = bit 16, epsilon = B.scale, decay = B.beta, scale[d] per chain in
  // B.t_sigma.  B.sep is the block's table (engine.cpp abc_table): [T, ns, nd, codes[ns], then per data
  // node (node id, first statistic)].  Tune per chain: B.t_hmc, the canonical row [initialised,
  // Tsim[nsim][T], epsilon[nsim], epsilonprime[nsim]].
  //
  // Summaries (abc_stats): element e of a data node sits on lane e % 32 in ascending e -- the observed
  // value, or the variate mmb_pr_elem_on draws at the parameters the node's expressions give on the
  // candidate state (s.prop), on the streams of (block, draw k, simulation i, data slot j), abc.h
  // mmb_abc_block.  sum: lane partials in element order, then the 32-lane butterfly (g.sum); mean:
  // sum / n; var: a second pass over the elements, the partials of (x - mean)^2 summed likewise, over
  // n - 1; std: sqrt(var); minimum / maximum: lane partials from +-Inf, the butterfly with "the partner's
  // value if it is smaller (larger) or NaN", then lane 0's result for every lane (the sign of a zero
  // tie is lane 0's).  identity: the node's elements.  Statistic t of the concatenated summaries sits on
  // lane t.  A lane's first element is kept in a register for the second pass; later ones (nodes of
  // more than 32 elements) are formed again, which gives the same bits: every variate is a function of
  // its key.  distance: sqrt of g.sum over the lanes' (Tsim_t - Tobs_t)^2, lanes >= T adding 0.
  //
  // The candidate's Tsim1[i] (statistic t on lane t), epsilon1[i] and epsilonprime1[i] (on lane i) stay
  // in registers and reach the tune row only on accept.  The two chains of a wave leave the draw loop
  // at their own k; every cross-lane step (DPP stages, 32-wide shuffles) stays within the chain's own 32
  // lanes, and every branch around one is uniform over those 32 lanes.
  __device__ __forceinline__ static double abc_jmax(double a, double b) {  // Julia max(a, b): NaN propagates
    if (isnan(a)) return a;
    if (isnan(b)) return b;
    return b > a ? b : a;
  }
  template <int S_>
  __device__ __forceinline__ static void abc_minmax_stage(double& lo, double& hi) {
    const double ol = Grp<G>::template other_d<S_>(lo);
    const double oh = Grp<G>::template other_d<S_>(hi);
    lo = (ol < lo || ol != ol) ? ol : lo;
    hi = (oh > hi || oh != oh) ? oh : hi;
  }
  template <bool SIM>
  __device__ __forceinline__ static double abc_elem(const SweepArgs& A, const mmb_ir_node& N, int e, double sig,
                                                    const double* vals, const St& s, const mmb_rng& sn,
                                                    const mmb_rng& su, int lane) {
    if constexpr (!SIM) {
      (void)sig; (void)sn; (void)su; (void)lane;
      return (N.fixed ? A.ir_pool + N.off : vals + N.off)[e];
    } else {
      const double pa = N.expr[0] >= 0 ? M::ev(A, N.expr[0], e, vals, s.stk, lane) : 0.0;
      const double pb = N.family == MMB_IR_ISONORMAL
                            ? sig
                            : (N.expr[1] >= 0 ? M::ev(A, N.expr[1], e, vals, s.stk, lane) : 0.0);
      return mmb_pr_elem_on(N.family, pa, pb, &sn, &su, e, N.len);
    }
  }
  // the concatenated summaries, statistic t on lane t (0 on lanes >= T): observed (SIM = false), or
  // simulated for draw k, simulation i, on the state `vals`: the chain state itself for the observed values
  // and the first update's simulation (k = 0; the reference simulates from the model as it stands, not from
  // the relisted invlink(link(value))), the candidate state for k >= 1
  template <bool SIM>
  __device__ __noinline__ static double abc_stats(const SweepArgs& A, const DBlock& B, const St& s, const double* vals,
                                                  const Grp<G>& g, uint32_t chain, uint32_t it, int b, int k, int i) {
    const int32_t* tab = B.sep;
    const int ns = tab[1], nd = tab[2];
    const int32_t* codes = tab + 3;
    const int32_t* dn = tab + 3 + ns;
    bool need_var = false, need_mm = false;
    for (int q = 0; q < ns; ++q) {
      need_var = need_var || codes[q] == MMB_ABC_VAR || codes[q] == MMB_ABC_STD;
      need_mm = need_mm || codes[q] == MMB_ABC_MINIMUM || codes[q] == MMB_ABC_MAXIMUM;
    }
    double ts = 0.0;
    for (int j = 0; j < nd; ++j) {
      const mmb_ir_node& N = M::node_ref(A, dn[2 * j]);
      const int t0 = dn[2 * j + 1], n = N.len;
      const uint32_t blk = mmb_abc_block(b, k, i, j);
      const mmb_rng sn = mmb_rng_make(A.seed, chain, it, blk, MMB_SUB_ABC_N);
      const mmb_rng su = mmb_rng_make(A.seed, chain, it, blk, MMB_SUB_ABC_U);
      double sig = 0.0;
      if (SIM && N.family == MMB_IR_ISONORMAL) sig = M::ev(A, N.expr[1], 0, vals, s.stk, g.lane);
      const double x0 = g.lane < n ? abc_elem<SIM>(A, N, g.lane, sig, vals, s, sn, su, g.lane) : 0.0;
      if (codes[0] == MMB_ABC_IDENTITY) {  // n <= 32 here: T <= 32
        const double xv = __shfl(x0, (g.lane - t0) & 31, 32);
        ts = (g.lane >= t0 && g.lane < t0 + n) ? xv : ts;
        continue;
      }
      double ps = 0.0, lo = __builtin_inf(), hi = -__builtin_inf();
      for (int e = g.lane; e < n; e += G) {
        const double xe = e == g.lane ? x0 : abc_elem<SIM>(A, N, e, sig, vals, s, sn, su, g.lane);
        ps = ps + xe;
        lo = (xe < lo || xe != xe) ? xe : lo;
        hi = (xe > hi || xe != xe) ? xe : hi;
      }
      const double sum = g.sum(ps);
      const double mean = sum / (double)n;
      double var = 0.0;
      if (need_var) {
        double pq = 0.0;
        for (int e = g.lane; e < n; e += G) {
          const double xe = e == g.lane ? x0 : abc_elem<SIM>(A, N, e, sig, vals, s, sn, su, g.lane);
          const double dv = xe - mean;
          pq = pq + dv * dv;
        }
        var = g.sum(pq) / (double)(n - 1);
      }
      if (need_mm) {
        abc_minmax_stage<0>(lo, hi); abc_minmax_stage<1>(lo, hi); abc_minmax_stage<2>(lo, hi);
        abc_minmax_stage<3>(lo, hi); abc_minmax_stage<4>(lo, hi);
        lo = __shfl(lo, 0, 32);
        hi = __shfl(hi, 0, 32);
      }
      for (int q = 0; q < ns; ++q) {
        const int cd = codes[q];
        const double sv = cd == MMB_ABC_SUM ? sum : cd == MMB_ABC_MEAN ? mean : cd == MMB_ABC_VAR ? var
                          : cd == MMB_ABC_STD ? sqrt(var) : cd == MMB_ABC_MINIMUM ? lo : hi;
        ts = g.lane == t0 + q ? sv : ts;
      }
    }
    return ts;
  }
  // logpdf(model, params, transform) (abc.jl:41, 103-104): the block's own nodes' terms in term order, with
  // logpdf!'s early exit on a non-finite running sum; x is written into the candidate state first, where
  // the data nodes' parameter expressions then read it
  __device__ __noinline__ static double abc_prior(const SweepArgs& A, const DBlock& B, const St& s, const Grp<G>& g,
                                                  const double* x) {
    M::put(B, s, g.lane, x, s.prop, nullptr);
    const mmb_ir_block& IB = M::block_ref(A, B.ir_blk);
    double lp = 0.0;
    for (int t = 0; t < IB.nterms; ++t) {
      if (!IB.trans[t]) continue;
      lp += M::template node_lp<false>(A, IB.term[t], s.prop, s.stk, g, B.transform);
      if (!isfinite(lp)) break;
    }
    return lp;
  }
  __device__ __forceinline__ static double abc_dist(double ts, double tobs, int T, const Grp<G>& g) {
    const double df = g.lane < T ? ts - tobs : 0.0;
    return sqrt(g.sum(df * df));
  }
  __device__ static void abc(const SweepArgs& A, const DBlock& B, int c, uint32_t chain, int64_t it, int b,
                             const mmb_rng& rn, const mmb_rng& ru, St& s, const Grp<G>& g) {
    static_assert(G == 32 && R == 1, "ABC keeps one statistic per lane of a 32-lane group");
    const int T = B.sep[0];
    const int d = B.d, nsim = B.adapt, maxdraw = B.batchsize;
    const int prop = B.form & 0xff, kern = (B.form >> 8) & 0xff;
    const bool randeps = ((B.form >> 16) & 1) != 0;
    const double eps = B.scale, decay = B.beta;
    const uint32_t itk = (uint32_t)it;
    double* row = B.t_hmc + (size_t)c * (size_t)(1 + nsim * (T + 2));
    double* rowe = row + 1 + nsim * T;
    const mmb_rng rp = mmb_rng_make(A.seed, chain, itk, (uint32_t)b, MMB_SUB_PROPOSAL);
    double v[R], x[R];
    M::unlist(B, s, g.lane, v);
    const double lp0 = abc_prior(A, B, s, g, v);
    const double tobs = abc_stats<false>(A, B, s, s.cur, g, chain, itk, b, 0, 0);
    const bool first = row[0] == 0.0;
    double pi0 = 0.0, e0 = 0.0;  // e0: the current epsilon[i] on lane i
#pragma unroll 1
    for (int i = 0; i < nsim; ++i) {
      double ts, ei, epi, perr = 1.0, dd;
      if (first) {  // abc.jl:63-83
        ts = abc_stats<true>(A, B, s, s.cur, g, chain, itk, b, 0, i);
        dd = abc_dist(ts, tobs, T, g);
        ei = decay > 0.0 ? abc_jmax(eps, dd) : eps;
        epi = ei;
        if (randeps) {
          const mmb_rng se = mmb_rng_make(A.seed, chain, itk, mmb_abc_block(b, 0, i, 16), MMB_SUB_ABC_U);
          epi = -ei * mmb_log1p(-mmb_uniform(&se, 0u));
          perr = mmb_abc_exp_pdf(ei, epi);
        }
        if (g.lane < T) row[1 + i * T + g.lane] = ts;
        if (g.lane == i) {  // (the lanes that store them on accept: same lane, same address, program order)
          rowe[i] = ei;
          rowe[nsim + i] = epi;
        }
      } else {  // abc.jl:86-93
        ts = g.lane < T ? row[1 + i * T + g.lane] : 0.0;
        ei = rowe[i];
        epi = rowe[nsim + i];
        dd = abc_dist(ts, tobs, T, g);
        if (randeps) perr = mmb_abc_exp_pdf(ei, epi);
      }
      pi0 = pi0 + mmb_abc_kernel_pdf(kern, epi, dd) * perr;
      e0 = g.lane == i ? ei : e0;
    }
    double ts1[MMB_ABC_MAX_NSIM];
#pragma unroll
    for (int i = 0; i < MMB_ABC_MAX_NSIM; ++i) ts1[i] = 0.0;
    double e1 = 0.0, ep1 = 0.0;  // the candidate's epsilon1[i], epsilonprime1[i] on lane i
    bool acc = false;
#pragma unroll 1
    for (int k = 1; k <= maxdraw; ++k) {
      double sc = 0.0, z = 0.0;
      if (g.lane < d) {
        const uint32_t q = (uint32_t)(k - 1) * (uint32_t)d + (uint32_t)g.lane;
        sc = B.t_sigma[(size_t)c * DP + g.lane];
        z = prop == MMB_RWM_NORMAL ? mmb_normal(&rn, q) : mmb_symdist(prop, &rp, q);
      }
      x[0] = v[0] + sc * z;
      const double lp1 = abc_prior(A, B, s, g, x);
      if (lp1 == -__builtin_inf()) continue;
      double pi1 = 0.0;
#pragma unroll
      for (int i = 0; i < MMB_ABC_MAX_NSIM; ++i) {
        if (i < nsim) {
          ts1[i] = abc_stats<true>(A, B, s, s.prop, g, chain, itk, b, k, i);
          const double dd = abc_dist(ts1[i], tobs, T, g);
          const double eo = __shfl(e0, i, 32);
          const double ei = (1.0 - decay) * eo + decay * abc_jmax(eps, jmin(dd, eo));  // abc.jl:119-120
          double epi = ei, perr = 1.0;
          if (randeps) {
            const mmb_rng se = mmb_rng_make(A.seed, chain, itk, mmb_abc_block(b, k, i, 16), MMB_SUB_ABC_U);
            epi = -ei * mmb_log1p(-mmb_uniform(&se, 0u));
            perr = mmb_abc_exp_pdf(ei, epi);
          }
          pi1 = pi1 + mmb_abc_kernel_pdf(kern, epi, dd) * perr;
          e1 = g.lane == i ? ei : e1;
          ep1 = g.lane == i ? epi : ep1;
        }
      }
      if (mmb_uniform(&ru, (uint32_t)(k - 1)) < pi1 / pi0 * mmb_exp(lp1 - lp0)) {
        acc = true;
        break;
      }
    }
    if (acc) {
      v[0] = x[0];
#pragma unroll
      for (int i = 0; i < MMB_ABC_MAX_NSIM; ++i)
        if (i < nsim && g.lane < T) row[1 + i * T + g.lane] = ts1[i];
      if (g.lane < nsim) {
        rowe[g.lane] = e1;
        rowe[nsim + g.lane] = ep1;
      }
    }
    if (first && g.lane == 0) row[0] = 1.0;
    bin_count(B, c, acc, g);
    M::relist(B, s, g, v);
  }

  // ---------------------------------------------------------------- SliceSimplex
  // slicesimplex.jl:86-122 (sample!, makefirstsimplex, shrinksimplex) for the block's one Dirichlet node
  // of k = B.d <= 32 elements (node-IR models; M::ssx_* in ir.h), the reference's linear solves
  // replaced by their closed form.  Lane i owns element i and row i of the k x k
  // vertex matrix V (LDS, column j at V[32 j + lane]: a column read touches 32 distinct banks), so
  // the products V xb, the first simplex and the shrink are lane-local; xb_j, bc_i come from lane j
  // by lane_value.  Every sum runs in index order from 0.0.
  //   draw r        w_j = e_j / (e_0 + ... + e_{k-1}), e_j = -log(1 - u), u = uniform #(32 r + j) of the
  //                 block's MMB_SUB_SIMPLEX stream: rand(Dirichlet(1, ..., 1))
  //   p0            logf(v) + log(uniform #0 of MMB_SUB_UNIFORM)
  //   first simplex V0 = I, columns j >= 1 moved towards column 0 by 1 - scale; V = V0 + v - V0 w (draw 0);
  //                 bx = w: the barycentric coordinates of v in V (V w = v by construction)
  //   candidate r   x = V xb, xb = draw r; rejected iff some x_i < 0 or > 1 (a ballot) or logf(x) < p0
  //                 (evaluated for an in-box x only; a NaN accepts, as in the reference)
  //   shrink        bc = xb; for every i with bc_i < bx_i (the set is fixed first), ascending, t = bc_i now:
  //                 V[:, j] += t (V[:, i] - V[:, j]) for j != i, and both bc and bx become
  //                 b_j / (1 - t) (j != i), (b_i - t) / (1 - t): the coordinates of x and of v in the new V
  // After MMB_SLICE_MAX_SHRINK rejected candidates the update stops as Slice does (slice_overflow).
  // The two chains of a wave leave the candidate loop on their own; every cross-lane step inside it
  // (DPP sums, lane_value, the ballot) stays within the chain's own 32 lanes.  No tune state.
  __device__ __forceinline__ static double ssx_draw(const mmb_rng& rs, uint32_t r, int k, const Grp<G>& g) {
    const double e = g.lane < k ? -mmb_log(1.0 - mmb_uniform(&rs, 32u * r + (uint32_t)g.lane)) : 0.0;
    double sum = 0.0;
    for (int j = 0; j < k; ++j) sum = sum + lane_value(e, j);
    return e / sum;
  }
  __device__ static void slice_simplex(const SweepArgs& A, const DBlock& B, const mmb_rng& ru, const mmb_rng& rs,
                                       St& s, const Grp<G>& g, double* V) {
    static_assert(G == 32 && R == 1, "SliceSimplex keeps one row of the vertex matrix per lane of a 32-lane group");
    const int k = B.d < G ? B.d : G, lane = g.lane;
    double v[R];
    M::unlist(B, s, lane, v);  // (0 on the lanes past k)
    const double p0 = M::ssx_logf(A, B, s, g, v) + mmb_log(mmb_uniform(&ru, 0u));
    double bx = ssx_draw(rs, 0u, k, g);
    {
      const double c = 1.0 - B.scale, ii0 = lane == 0 ? 1.0 : 0.0;
      double dot = 0.0;
      for (int j = 0; j < k; ++j) {
        const double iij = lane == j ? 1.0 : 0.0;
        const double v0 = iij + c * (ii0 - iij);
        V[32 * j + lane] = v0;
        dot = dot + v0 * lane_value(bx, j);
      }
      for (int j = 0; j < k; ++j) V[32 * j + lane] = (V[32 * j + lane] + v[0]) - dot;
    }
    bool hit = false;
    for (uint32_t r = 1; r <= (uint32_t)MMB_SLICE_MAX_SHRINK; ++r) {
      const double xb = ssx_draw(rs, r, k, g);
      double x[R];
      {
        double acc = 0.0;
        for (int j = 0; j < k; ++j) acc = acc + V[32 * j + lane] * lane_value(xb, j);
        x[0] = acc;
      }
      bool rej = grp_any(lane < k && (x[0] < 0.0 || x[0] > 1.0));
      if (!rej) rej = M::ssx_logf(A, B, s, g, x) < p0;
      if (!rej) {
        v[0] = x[0];
        hit = true;
        break;
      }
      const unsigned long long bal = __ballot(lane < k && xb < bx);
      const uint32_t shr = (uint32_t)((threadIdx.x & 32) != 0 ? (bal >> 32) : bal);
      double bc = xb;
      for (int i = 0; i < k; ++i) {
        if (((shr >> i) & 1u) == 0u) continue;
        const double t = lane_value(bc, i), om = 1.0 - t;
        const double vi = V[32 * i + lane];
        for (int j = 0; j < k; ++j) {
          if (j == i) continue;
          const double vj = V[32 * j + lane];
          V[32 * j + lane] = vj + t * (vi - vj);
        }
        bc = lane == i ? (bc - t) / om : bc / om;
        bx = lane == i ? (bx - t) / om : bx / om;
      }
    }
    if (!hit) slice_overflow(A, g);
    M::relist(B, s, g, v);
  }

  // ---------------------------------------------------------------- pivoted Cholesky
  // cholfact(Hermitian(S), Val{true}) restated in LAPACK dpstf2('U', tol = 0) op order
  // (oracle.c orc_pchol): pivot = first maximum of the remaining diagonal in position
  // order, stop when it is <= 0 or NaN, row J as a dot product then scaled by ONE/AJJ.
  // The dot product runs on two accumulators (even / odd k) summed at the end (the
  // oracle does the same).  S: packed symmetric in LDS (`mat`, slot(i,k)); the pivot's
  // factor row is broadcast through `prow` (contiguous LDS) each step.  On full rank the
  // factor is written back in place: L[i][step k] -> slot(i, piv[k]), L[i][pos_i] ->
  // slot(i,i).  pk[] receives the pivot order.  Returns the rank (group-uniform).
  // One lane per chain holds every row (line: G = 1, R = 3); 32-lane groups with one row per
  // lane (rats, the node IR) take pchol32 below, amm() decides.
  __device__ __forceinline__ static int pchol(int d, double* mat, double* prow, int* pks,
                                              const Grp<G>& g) {
    static_assert(G == 1, "pchol()'s pivot search walks the rows of one lane; lane groups use pchol32");
    double diag0[R], work[R], Lrow[R][DMAX];
    bool done[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int e = r * G + g.lane;
      done[r] = !(e < d);
      diag0[r] = e < d ? mat[mmb_tri(e) + e] : 0.0;
      work[r] = 0.0;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) Lrow[r][k] = 0.0;
    }
    int rank = d;
    bool live = true;
#pragma unroll
    for (int j = 0; j < DMAX; ++j) {
      if (live && j < d) {
        // ---- pivot: first maximum of the remaining diagonal in position order ----
        double dl[R];
#pragma unroll
        for (int r = 0; r < R; ++r) dl[r] = diag0[r] - work[r];
        // dpstf2's position swaps replayed from the pivot history
        int perm[DMAX];
#pragma unroll
        for (int t = 0; t < DMAX; ++t) perm[t] = t;
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
          if (k < j) {
            int q = pks[k];
            int qpos = k;
#pragma unroll
            for (int t = 0; t < DMAX; ++t) qpos = (t >= k && perm[t] == q) ? t : qpos;
            int tmp = perm[k];
#pragma unroll
            for (int t = 0; t < DMAX; ++t) perm[t] = (t == qpos) ? tmp : perm[t];
            perm[k] = q;
          }
        }
        // fold in position order: first strict maximum (oracle.c orc_pchol)
        int best = -1;
        double bv = 0.0;
#pragma unroll
        for (int t = 0; t < DMAX; ++t) {
          if (t >= j && t < d) {
            int e = perm[t];
            double de = dl[0];
#pragma unroll
            for (int r = 1; r < R; ++r) de = (e == r) ? dl[r] : de;
            if (best < 0) { best = e; bv = de; }
            else if (de > bv) { best = e; bv = de; }
          }
        }
        const int p = best;
        const double val = bv;
        if (!(val > 0.0)) {
          rank = j;
          live = false;
        } else {
          if (g.lane == 0) pks[j] = p;
          const double ajj = sqrt(val);
          const double rinv = 1.0 / ajj;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            if (r * G + g.lane == p) {
              done[r] = true;
              Lrow[r][j] = ajj;
#pragma unroll
              for (int k = 0; k + 1 < j; k += 2)
                *(double2*)(prow + k) = make_double2(Lrow[r][k], Lrow[r][k + 1]);
              if (j & 1) prow[j - 1] = Lrow[r][j - 1];
            }
          }
          grp_sync();
#pragma unroll
          for (int r = 0; r < R; ++r) {
            int e = r * G + g.lane;
            if (!done[r]) {
              double t0 = 0.0, t1 = 0.0;
#pragma unroll
              for (int k = 0; k + 1 < j; k += 2) {
                const double2 pp = *(const double2*)(prow + k);
                t0 = fma(Lrow[r][k], pp.x, t0);
                t1 = fma(Lrow[r][k + 1], pp.y, t1);
              }
              if (j & 1) t0 = fma(Lrow[r][j - 1], prow[j - 1], t0);
              double lij = (mat[mmb_slot(e, p)] - (t0 + t1)) * rinv;
              Lrow[r][j] = lij;
              work[r] = work[r] + lij * lij;
            }
          }
          grp_sync();
        }
      }
    }
    if (rank == d) {  // write the factor back in slot form
#pragma unroll
      for (int r = 0; r < R; ++r) {
        int e = r * G + g.lane;
        if (e < d) {
          bool before = true;
#pragma unroll
          for (int k = 0; k < DMAX; ++k) {
            if (k < d) {
              const int q = pks[k];
              if (q == e) {
                mat[mmb_tri(e) + e] = Lrow[r][k];
                before = false;
              } else if (before) {
                mat[mmb_slot(e, q)] = Lrow[r][k];
              }
            }
          }
        }
      }
    }
    return rank;
  }

  // Exact pivot choice for the rare cases the fast search hands over (ties of the high
  // words, NaN candidates): replays dpstf2's position swaps from the pivot history and
  // takes the first maximum in position order.  Out of line: it is shared by every
  // unrolled step instead of being inlined 30 times.
  __device__ __forceinline__ static int pivot_exact(double dl, bool done, const int* pks, int j,
                                                              int d, int* perm, double* val) {
    const int lane = (int)(threadIdx.x & (G - 1));
    if (lane == 0) {
      for (int t = 0; t < d; ++t) perm[t] = t;
      for (int k = 0; k < j; ++k) {
        int q = pks[k], qpos = k;
        for (int t = k; t < d; ++t) if (perm[t] == q) qpos = t;
        int tmp = perm[k]; perm[k] = q; perm[qpos] = tmp;
      }
    }
    grp_sync();
    int mypos = 0x7fffffff;
    for (int t = j; t < d; ++t) if (perm[t] == lane) mypos = t;
    grp_sync();
    double key = done ? -__builtin_inf()
                      : (isnan(dl) ? (mypos == j ? __builtin_inf() : -__builtin_inf()) : dl);
    int pi = (done ? 0x7fff : mypos) << 16 | lane;
    Grp<G> g;
    g.argmax(key, pi);
    const int p = pi & 0xffff;
    *val = g.bcast(dl, p);
    return p;
  }

  // group max of an int over the 32 lanes: four row stages (DPP folded into v_max_i32)
  // and one permlane16 swap whose two outputs are the two rows of each half
  __device__ __forceinline__ static int gmax_i32(int x) {
    x = max(x, dpp_i<MMB_DPP_XOR1>(x));
    x = max(x, dpp_i<MMB_DPP_XOR2>(x));
    x = max(x, dpp_i<MMB_DPP_HMIRROR>(x));
    x = max(x, dpp_i<MMB_DPP_MIRROR>(x));
    auto r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
    return max((int)r[0], (int)r[1]);
  }

  // pchol for 32-lane groups with one row per lane (rats), same results as pchol():
  // * the pivot lane computes sqrt / reciprocal of its remaining diagonal by the in-range
  //   sequences of device.h (bit-identical to sqrt() and 1.0 / x there) and publishes the
  //   reciprocal through LDS together with its factor row.  In the optimistic pass it takes
  //   the reciprocal from the root's half-reciprocal (mmb_rcp_seeded: no v_rcp_f64, one Newton
  //   step less), and the last step publishes no reciprocal;
  // * the search reduces the high words of the positive candidates as int32 (one DPP
  //   max per stage); a unique maximal high word is the unique maximum.  High-word ties
  //   and NaN candidates go to pivot_exact (dpstf2's first maximum in position order).
  // Measured (rats sweep, 16384 chains): 0.255 -> 0.248 ms; the factorization is bound by
  // its f64 work per step (sqrt, reciprocal, dot product), not by the pivot search.
  // rn1 != null: also returns in *ynext this lane's row of SigmaLm z2' for the next
  // iteration (z2' = the second normal of each element's pair from rn1), formed from the
  // factor rows still in registers: P L z2' (amm.jl:74), row e = sum_k L[pos e][k] z2'[k],
  // k ascending -- the order of the direct matvec in amm().
  //
  // On full rank the factor is left in `mat` in POSITION form (row at pivot position t, i.e.
  // row piv[t] of P'L... stored at tri(t) .. tri(t) + t, step order), and *pos receives this
  // lane's position; amm() stores it with the position bytes (the host converts to the
  // canonical slot form + pivot order, engine.cpp).  wb = false skips that write-back.
  __device__ __forceinline__ static int pchol32(int d, double* mat, double* prow, int* pks, const Grp<G>& g,
                                                int* pos_out, const DBlock* NB = nullptr,
                                                const SweepArgs& A = SweepArgs{}, int c = 0, uint32_t chain = 0,
                                                int64_t it = 0, int b = 0, int m = 0, int* redo = nullptr,
                                                bool wb = true) {
    // a block as wide as the model's DMAX (rats: both 30-d blocks) runs a copy with d a
    // compile-time constant: no per-step scalar test and branch of j against d (9.58e7 ->
    // 9.90e7 rats chain-updates/s, A/B on one box, parity unchanged)
    if (d == DMAX)
      return pchol32_impl<true>(d, mat, prow, pks, pos_out, NB, A.seed, A.xepoch, c, chain, it, b, m, redo, wb);
    return pchol32_impl<false>(d, mat, prow, pks, pos_out, NB, A.seed, A.xepoch, c, chain, it, b, m, redo, wb);
  }
  template <bool FULLD>
  __device__ __forceinline__ static int pchol32_impl(int d_arg, double* mat, double* prow, int* pks, int* pos_out,
                                                     const DBlock* NB, uint64_t seed, int64_t xepoch, int c,
                                                     uint32_t chain, int64_t it, int b, int m,
                                                     int* redo_out, bool wb) {
    const int d = FULLD ? DMAX : d_arg;
    const Grp<G> g;
    constexpr int RI = DMAX;  // prow[RI]: the pivot's reciprocal
    const int lane = g.lane;
    const bool hi_half = (threadIdx.x & 32) != 0;
    const bool inb = lane < d;
    const int lc = inb ? lane : 0;
    const double diag0 = inb ? mat[mmb_tri(lane) + lane] : 0.0;
    double work = 0.0;
    double Lrow[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) Lrow[k] = 0.0;
    MMB_PROF_START
    bool done = !inb;
    int rank = d;
    int pe = 0;  // this lane's pivot position
    bool live = true;
    // the factorization's epilogue (carried proposal, write-back)
    auto tail = [&]() __attribute__((always_inline)) -> int {
      MMB_PROF_MARK(10, lane)
      // carried proposal of the next iteration (see amm): formed here, where the factor rows are
      // still in registers; skipped when the next proposal would need an older factor
      if (NB != nullptr && (rank == d || m <= 2 * d)) {
        const mmb_rng rn1 = mmb_rng_make(seed, chain, (uint32_t)(it + 1), (uint32_t)b, MMB_SUB_NORMAL);
        double z1n = 0.0, z2n = 0.0;
        if (inb) mmb_normal_pair(&rn1, (uint32_t)lane, &z1n, &z2n);
        double a = 0.0;
        if (inb) a = fma(NB->sigl[lane * d + lane], z1n, a);
        if (m > 2 * d) {
          // rows are zero past the lane's own step, so the full sweep adds exact zeros
          double y = 0.0;
          // z2'[k] lives in lane k: rows 0 / 1 of the group exchange theirs (permlane16 swap),
          // then each product takes z2'[k] from lane k % 16 of the row (DPP64 row_newbcast)
          const double zs = swap16_d(z2n);
          const bool row0 = (lane & 16) == 0;
          const double zA = row0 ? z2n : zs, zB = row0 ? zs : z2n;
#pragma unroll
          for (int k = 0; k < DMAX; ++k) fmac_rowbc_n(y, k < 16 ? zA : zB, Lrow[k], k & 15);
          a = NB->beta * a + (1.0 - NB->beta) * y;
        }
        if (inb) NB->t_xnext[(size_t)c * DP + lane] = a;
        if (lane == 0) NB->t_xtag[c] = (xepoch << 32) | (int64_t)(uint32_t)(it + 1);  // xtag()
      }
      MMB_PROF_MARK(11, lane)
      // (wb, wave-uniform: false when the caller will not read the factor from `mat`, amm()'s
      // lazy factor store; `mat` then still holds Sigma)
      if (wb && rank == d && inb) {  // the factor in position form: row at position pe at tri(pe) + k
        // one store per k from every lane, no exec-mask change: entries past the row's end
        // (k > pe, exact zeros) go to the lane's own dummy slot in the idle pivot-row buffer
        const int base = mmb_tri(pe);
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
          double* dst = k <= pe ? mat + base + k : prow + lane;
          *dst = Lrow[k];
        }
      }
      MMB_PROF_MARK(12, lane)
      *pos_out = pe;
      return rank;
    };
    // Two passes over the same Sigma (mat is only read until the write-back):
    // * the optimistic pass takes, per chain, the lane whose candidate dl = diag0 - work has
    //   the largest int32 high word (the lowest such lane on a tie) as the pivot and stops
    //   when every candidate is negative.  It never branches on the pivot search; whether a
    //   step was outside what that rule decides exactly -- a high-word tie, a NaN or >= 2^700
    //   candidate, or a maximum below 2^-700 (then the in-range square root / reciprocal of
    //   device.h would not be the IEEE ones) -- is checked once, after its last step;
    // * only if so (rare), the whole factorization is redone by the checked pass: the same
    //   steps, with dpstf2's exact choice (pivot_exact: first maximum in position order, its
    //   rank test) and sqrt() / division wherever a step needs them.
    // Both give dpstf2's pivots and bits.  A lane that is done (its row finished) or out of
    // range carries work = +inf, so its candidate is -inf and its key negative with no
    // per-step select.  The row update of lij is the !done select only; the dot product runs
    // on every lane (a DPP source lane must be active).
    if (!inb) work = __builtin_inf();
    // LDS byte address of mat (32-bit local address space)
    const uint32_t mat_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double*)mat;
    int hmask = hi_half ? -1 : 0;
    asm volatile("" : "+v"(hmask));  // keep it a VGPR (not a scalar lane mask + select)
    constexpr int KEY_LO = 0x14300000;     // high word of 2^-700
    constexpr double BIG = 0x1p700;
    // CHECKED is a template constant: two inlined copies of the pass (one copy branching per step
    // on a run-time flag was tried and dropped).  The optimistic pass (!CHECKED)
    // * keeps no per-step bookkeeping of whether its choices were dpstf2's: everything that could
    //   make them differ is visible after the loop (see the check below the step loop; the round-3
    //   per-step check cost scalar work in every step);
    // * keeps no done flag: a lane is done iff its work is +inf (pivots set it; an undone lane
    //   whose sum of squares overflowed counts as done too, which only a chain that cannot reach
    //   full rank can meet -- its rank then disagrees with its steps and the check redoes it).
    // Returns whether the pass has to be redone (the checked pass: never).
    auto pass = [&](auto checked_c) __attribute__((always_inline)) -> bool {
      constexpr bool CHECKED = decltype(checked_c)::value;
      // optimistic pass: this lane's candidate when it was taken as the pivot (until then a value
      // the post-loop check passes)
      double apiv = 1.5;
      double inf_s = __builtin_inf();
      asm volatile("" : "+s"(inf_s));  // +inf in an SGPR pair: one v_mov_b64 per pivot
#pragma unroll
      for (int j = 0; j < DMAX; ++j) {
        if (live && j < d) {
          const double dl = diag0 - work;
          const int key = (int)(mmb_d2u(dl) >> 32);
          const int mx = gmax_i32(key);
          const uint64_t eq = __ballot(key == mx);
          uint32_t elo = (uint32_t)eq, ehi = (uint32_t)(eq >> 32);
          int p = 0;
          // one compare for the stop and the pivot mask (pos = the complement mask)
          const uint64_t negm = __ballot(mx < 0);
          bool pos = mmb_inverse_ballot(~negm);  // dpstf2's ajj <= 0 stop
          bool fast = true;
          if constexpr (!CHECKED) {
            // p = plo in the lower chain, phi in the upper one, as plo ^ ((plo ^ phi) & hmask)
            const int plo = __builtin_ctz(elo | 0x80000000u), phi = __builtin_ctz(ehi | 0x80000000u);
            p = plo ^ ((plo ^ phi) & hmask);
          } else {
            const uint64_t act = __builtin_amdgcn_read_exec();
            const uint64_t bad = __ballot(!(dl < BIG));      // NaN, +inf or >= 2^700
            const uint64_t big = __ballot(key >= KEY_LO);    // candidates >= 2^-700
            const uint64_t neg = __ballot(mx < 0);
            // per chain (32-bit half): inactive, or stopping, or a unique maximum >= 2^-700
            uint32_t alo = (uint32_t)act, ahi = (uint32_t)(act >> 32);
            uint32_t nlo = (uint32_t)neg, nhi = (uint32_t)(neg >> 32), blo = (uint32_t)big, bhi = (uint32_t)(big >> 32);
            asm("" : "+s"(elo), "+s"(ehi), "+s"(alo), "+s"(ahi));
            asm("" : "+s"(nlo), "+s"(nhi), "+s"(blo), "+s"(bhi));
            const bool ok_lo = alo == 0 || nlo != 0 || ((elo & (elo - 1)) == 0 && blo != 0);
            const bool ok_hi = ahi == 0 || nhi != 0 || ((ehi & (ehi - 1)) == 0 && bhi != 0);
            fast = bad == 0 && ok_lo && ok_hi;
            if (fast) {
              const int plo = __builtin_ctz(elo | 0x80000000u), phi = __builtin_ctz(ehi | 0x80000000u);
              p = plo ^ ((plo ^ phi) & hmask);
            } else {
              double val;
              p = pivot_exact(dl, done, pks, j, d, (int*)prow, &val);
              pos = val > 0.0;
            }
          }
          // optimistic pass: no branch on the stop either -- a chain whose candidates are all
          // negative runs this step on a garbage pivot (one of its done / out-of-range lanes,
          // whose -inf keys are the largest negative ones) and stops after it; a stopped
          // chain's factor is never used (rank < d) and its done set is unchanged
          if (CHECKED && !pos) {
            live = false;  // rank = pivots taken, counted after the loop
          } else {
            // optimistic pass: the pivot is the lane holding the maximal high word (unique, or
            // the pass is redone; a stopping chain's garbage step may take several of its done /
            // out-of-range -inf lanes, which changes nothing that is used), and a stopping
            // chain's step takes no pivot (its done lanes keep pe and row)
            const bool piv = CHECKED ? lane == p : mmb_inverse_ballot(eq & ~negm);
            if (piv) {
              if constexpr (CHECKED) pks[j] = p;  // (only the checked pass replays it)
              else apiv = dl;
              if (j + 1 < d) {  // the last step has no rows left to update: no readers
#pragma unroll
                for (int k = 0; k + 1 < j; k += 2) *(double2*)(prow + k) = make_double2(Lrow[k], Lrow[k + 1]);
                if (j & 1) prow[j - 1] = Lrow[j - 1];
              }
              double ajj;
              if constexpr (!CHECKED) {
                // IEEE sqrt in the fast range; the reciprocal seeded from its half-reciprocal is
                // 1.0 / ajj except on the candidates the post-loop check sends to the checked pass
                // (device.h).  Running the prefix on every lane ahead of the search, in the DPP
                // stages' wait states, was measured slower than this.
                double sg, sh;
                mmb_sqrt_prefix(dl, &sg, &sh);
                ajj = mmb_sqrt_finish(dl, sg, sh);
                if (j + 1 < d) prow[RI] = mmb_rcp_seeded(ajj, sh);  // (last step: no readers)
              } else {
                double rinv;
                if (fast) {
                  mmb_sqrt_rcp_inrange(dl, &ajj, &rinv);  // IEEE results in the fast range (device.h)
                } else {
                  ajj = sqrt(dl);
                  rinv = 1.0 / ajj;
                }
                prow[RI] = rinv;
              }
              Lrow[j] = ajj;
              pe = j;
              work = inf_s;
              if constexpr (CHECKED) done = true;
            }
            grp_sync();
            if (j + 1 < d) {  // (j = d - 1: every lane is done)
              // pivot row: lane l of each 16-lane row reads elements l and 16 + l, then every
              // product takes element k from lane k % 16 of its row by a DPP64 row_newbcast operand
              double t0 = 0.0, t1 = 0.0;
              // Sigma(lc, p) at byte 8 slot = 4 a (a + 1) + 8 b, a = max, b = min
              const int sa = max(lc, p), sb = min(lc, p);
              int sq, ad;  // sa (sa + 1) in one instruction; byte address by two shift-adds
              asm("v_mad_u32_u24 %0, %1, %1, %1" : "=v"(sq) : "v"(sa));
              asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(ad) : "v"(sb), "v"(mat_lds));
              asm("v_lshl_add_u32 %0, %1, 2, %0" : "+v"(ad) : "v"(sq));
              double sig = *(const __attribute__((address_space(3))) double*)(uintptr_t)(uint32_t)ad;
              double rinv = prow[RI];
              double pA = prow[lane & 15];
              double pB = j > 16 ? prow[16 + (lane & 15)] : 0.0;
              asm volatile("" : "+v"(sig), "+v"(rinv), "+v"(pA));
              if (j > 16) asm volatile("" : "+v"(pB));
              if (j > 0) {
#pragma unroll
                for (int k = 0; k < j; ++k) {
                  const double src = k < 16 ? pA : pB;
                  if (k & 1) fmac_rowbc_ld(t1, src, Lrow[k], k & 15);
                  else fmac_rowbc_ld(t0, src, Lrow[k], k & 15);
                }
              }
              const double lij = (sig - (t0 + t1)) * rinv;
              const bool keep = CHECKED ? done : work == inf_s;  // done lanes keep their rows
              // done lanes carry work = +inf, which absorbs lij^2: no select for work
              work = work + lij * lij;
              if (!keep) Lrow[j] = lij;
            }
            grp_sync();
            if (!CHECKED) live = live && pos;
          }
        }
      }
      if constexpr (CHECKED) {
        return false;
      } else {
        // What the optimistic choices could get wrong, checked once after the loop:
        // * a pivot outside the in-range square root's domain [2^-700, 2^700] -- a tiny or zero
        //   maximum, a huge or +inf one, a positive NaN key (it would have been the maximum);
        // * a pivot whose seeded reciprocal may differ from 1.0 / ajj (device.h mmb_rcp_seeded_doubt:
        //   a significand within 64 ulps of a binade boundary);
        // * a NaN candidate that never became a pivot (dpstf2 may stop on it; its work stays NaN
        //   to the end because NaN + x = NaN and only pivots reset work);
        // * a high-word tie: every lane holding the maximal key became a pivot at that step, so
        //   the chain has more done lanes than steps that took pivots (pe values 0..max_pe, each
        //   taken once when exact: done == max_pe + 1).
        // On a tie the rows the pass computed after it are garbage; the redo replaces them.
        done = work == inf_s;
        const bool inr = apiv >= 0x1p-700 && apiv <= 0x1p700 && !mmb_rcp_seeded_doubt(apiv);
        uint64_t need = __ballot(inb && (done ? !inr : isnan(diag0 - work)));
        const uint64_t dn = __ballot(done && inb);
        const int mpe = gmax_i32((done && inb) ? pe : -1);
        const uint64_t act = __builtin_amdgcn_read_exec();
        const int m0 = __builtin_amdgcn_readlane(mpe, 0), m1 = __builtin_amdgcn_readlane(mpe, 32);
        if ((uint32_t)act != 0u && __builtin_popcount((uint32_t)dn) != m0 + 1) need |= 1ull;
        if ((act >> 32) != 0u && __builtin_popcount((uint32_t)(dn >> 32)) != m1 + 1) need |= 1ull << 32;
        return need != 0;
      }
    };
    // rare (a few per thousand factorizations): redo with dpstf2's exact decisions, the same
    // unrolled steps inline (an out-of-line redo and a compact-loop redo were both measured
    // slower: the call forces the live factor rows through scratch); marked unlikely so the
    // block placement moves the checked pass out of the hot code
    if (__builtin_expect(pass(mmb_bc<false>{}), 0)) {
      if (redo_out) *redo_out = 1;
      work = inb ? 0.0 : __builtin_inf();
#pragma unroll
      for (int k = 0; k < DMAX; ++k) Lrow[k] = 0.0;
      done = !inb;
      pe = 0;
      live = true;
      (void)pass(mmb_bc<true>{});
    }
    const uint64_t dn = __ballot(done && inb);
    rank = __builtin_popcount(hi_half ? (uint32_t)(dn >> 32) : (uint32_t)dn);  // pivots taken
    return tail();
  }

  // (i, k) of every packed slot, i << 8 | k, one table per workgroup in LDS (filled once per
  // launch by ik_fill): the moment update reads it instead of inverting tri() per slot
  static constexpr bool IKTAB = (G == 32);
  __device__ __forceinline__ static uint16_t* ik_table() {
    __shared__ uint16_t tab[IKTAB ? TP : 1];
    return tab;
  }
  __device__ __forceinline__ static void ik_fill() {
    if constexpr (IKTAB) {
      for (int t = (int)threadIdx.x; t < TP; t += (int)blockDim.x) {
        int i, k;
        slot_ik(t, i, k);
        ik_table()[t] = (uint16_t)(i << 8 | k);
      }
    }
  }
  // (i, k) of packed slot s = tri(i) + k: float square root estimate, integer correction
  __device__ __forceinline__ static void slot_ik(int s, int& i, int& k) {
    int ii = (int)((sqrtf((float)(8 * s + 1)) - 1.0f) * 0.5f);
    ii += (mmb_tri(ii + 1) <= s) ? 1 : 0;
    ii -= (mmb_tri(ii) > s) ? 1 : 0;
    i = ii;
    k = s - mmb_tri(ii);
  }

  // AMM factorization counters of one update (mmb_amm_stats): rank(F) == n (amm.jl:88), the
  // rank, the factorization steps the group executed (min(rank + 1, n) per chain; on the 32-lane
  // kernels the two chains of a wave step together, so the wave's count is the larger one) and
  // whether the optimistic pass was redone.  Diagnostics: lane 0 of the group, 20 bytes.
  __device__ __forceinline__ static void amm_count(const DBlock& B, int c, int d, int rank, int redo,
                                                   const Grp<G>& g) {
    const int st = rank < d ? rank + 1 : d;
    int ws = st;
    if constexpr (G == 32) {
      const uint64_t act = __builtin_amdgcn_read_exec();  // the upper group may have exited (c >= K)
      const int s0 = __builtin_amdgcn_readlane(st, 0), s1 = __builtin_amdgcn_readlane(st, 32);
      ws = max((uint32_t)act != 0u ? s0 : 0, (act >> 32) != 0u ? s1 : 0);
    }
    if (g.lane == 0) {
      // no-return atomics: fire-and-forget, no HBM round trip on the update's path (a plain
      // load-add-store would wait for the load)
      uint64_t* a = B.t_astat + (size_t)c * MMB_AMM_STAT_STRIDE;
      (void)__hip_atomic_fetch_add(a + 0, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (rank == d) (void)__hip_atomic_fetch_add(a + 1, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(a + 2, (uint64_t)rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(a + 3, (uint64_t)ws, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (redo) (void)__hip_atomic_fetch_add(a + 4, (uint64_t)redo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }

  // ---------------------------------------------------------------- AMM
  // amm.jl:66-108.  LDS per chain: mat[TP] | z2[DP] | vv[DP] | mv[DP] | ia[2*DP ints]
  // (rats: then the vector blocks' scalar constants, models.h prep_pass, which nothing here touches)
  // Carried proposal (32-lane groups, diagonal SigmaL): the proposal of the NEXT iteration,
  // x' - v = SigmaL z1' [beta * . + (1 - beta) SigmaLm z2'] (amm.jl:72-76), depends only on
  // that iteration's draws (Philox keyed by the iteration), the tune m after this update and
  // the factor this update computes -- and v is unchanged in between (only this block samples
  // its nodes).  So it is formed right after the factorization, with the factor rows still in
  // registers (no pivot decode), and carried through HBM (t_xnext, 30 doubles) instead of
  // re-reading the factor (465 doubles) next time.  Same operations in the same order, so the
  // draws are bit-identical; the tag (host epoch, iteration) makes any host write of the chain
  // state or a skipped update fall back to the direct path.
  static constexpr bool CARRY = (G == 32 && R == 1);
  // factor storage on device: position form + position bytes (pchol32) or slot form + pivot
  // order (pchol); the host converts to the canonical slot form (engine.cpp mmb_get_tune)
  static constexpr bool POSFORM = (G == 32 && R == 1);
  __device__ __forceinline__ static int64_t xtag(const SweepArgs& A, int64_t it) {
    return (A.xepoch << 32) | (int64_t)(uint32_t)it;
  }
  __device__ __forceinline__ static void amm(const SweepArgs& A, const DBlock& B, int c, uint32_t chain,
                             int64_t it, int b, const mmb_rng& rn,
                             const mmb_rng& ru, bool adapt, St& s, const Lc& l, const Grp<G>& g,
                             double* lds, double upre, typename M::PrepCache& pk, bool& rec) {
    const int d = B.d;
    const int T = mmb_tri(d);
    double* mat = lds;
    double* z2s = lds + TP;
    double* vvs = z2s + DP;
    double* mvs = vvs + DP;
    int* ia = (int*)(mvs + DP);  // piv / pos scratch (2*DP ints)
    MMB_PROF_START
    int m, fl;
    int* pks = (int*)z2s;  // pivot order (group-uniform values), LDS
    const bool carry = CARRY && B.t_xtag != nullptr && B.sigl_diag;
    bool lazy = false;
    // Lazy factor store (carried proposals, two moment buffers).  Within a launch nothing reads
    // t_Ls / t_piv of a chain whose update was full rank: the next proposal is the carry and the
    // next full-rank update overwrites them.  So a full-rank update whose successor runs in this
    // launch and adapts (both wave-uniform, known before the factorization) keeps its factor in
    // registers only -- no LDS write-back, no store -- and marks the chain (flag bit 4, STALE).
    // The one reader left is a marked chain whose NEXT update is rank deficient (amm.jl:88-90
    // keeps the older SigmaLm; a rounding event).  That update returns rec = true and the sweep
    // runs the block again at once (sweep.h: the block loop re-enters this one copy of the code):
    // the second visit (`recover`) does nothing but rebuild Sigma of the update before from the
    // other moment buffer, by the operations of the moment update's Sigma line, factorize it
    // again (the same bits) and store that factor; no proposal, no carry, no counters.  A wave
    // partner that does not recover rides along on whatever its `mat` holds and stores nothing.
    // The launch's last iteration always stores, so no mark crosses a launch.
    constexpr int STALE = 16;
    if constexpr (CARRY)
      lazy = carry && B.t_Mv_alt != nullptr && it != A.iter0 + A.n_iters &&
             (B.adapt == MMB_ADAPT_ALL || (B.adapt == MMB_ADAPT_BURNIN && it + 1 <= A.model_burnin));
    bool recover = false;  // wave-uniform
    if constexpr (CARRY) recover = __ballot(rec) != 0;
    if (__builtin_expect(recover, 0)) {
      // Sigma(m - 1) = cc (Mvv - Mv Mv') from the buffer of the other parity, p and cc of m - 1
      // (a marked chain's previous update was full rank, so it was not the fresh one)
      m = B.t_m[c];
      fl = B.t_flags[c];
      const int mp = m - 1;
      const double pp = (double)mp / ((double)mp + 1.0);
      const double ccp = (B.scale * B.scale / (double)d) / pp;
      const double* MvvP = ((mp & 1) ? B.t_Mvv_alt : B.t_Mvv) + (size_t)c * TP;
      const double* MvP = ((mp & 1) ? B.t_Mv_alt : B.t_Mv) + (size_t)c * DP;
      double* mvp = (double*)ia;  // the pivot-row buffer, idle between factorizations
      if (rec && g.lane < d) mvp[g.lane] = MvP[g.lane];
      grp_sync();
      if (rec) {
        for (int t = g.lane; t < TP; t += G) {
          int i, k;
          slot_ik(t, i, k);
          mat[t] = ccp * (MvvP[t] - mvp[k] * mvp[i]);
        }
      }
      M::stash(lds, s, g.lane);
      grp_sync();
    } else {
    double v[R], x[R], z1[R], z2[R], mv[R];
    M::unlist(B, s, g.lane, v);
    m = B.t_m[c];
    fl = B.t_flags[c];
    // two moment buffers (DBlock::t_Mv_alt): the current Mv is in the copy of m's parity; both
    // loads are issued with the load of m (no address that waits for it)
    const bool dual = CARRY && B.t_Mv_alt != nullptr;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int e = r * G + g.lane;
      mv[r] = e < d ? B.t_Mv[(size_t)c * DP + e] : 0.0;
      if constexpr (CARRY) {
        const double alt = (dual && e < d) ? B.t_Mv_alt[(size_t)c * DP + e] : 0.0;
        mv[r] = (dual && (m & 1)) ? alt : mv[r];
      }
    }
    const bool fresh = adapt && !(fl & 1);
    bool carried = false;
    if constexpr (CARRY) carried = B.t_xtag != nullptr && !fresh && B.t_xtag[c] == xtag(A, it);
    if (fresh) {  // setadapt!: m = 0, Mv = v (aliased), Mvv = v v', SigmaLm = 0
      m = 0;
      fl = (fl | 2) & ~4;
#pragma unroll
      for (int r = 0; r < R; ++r) mv[r] = v[r];
    }
    fl = adapt ? (fl | 1) : (fl & ~1);
    MMB_PROF_MARK(1, g.lane)
    // proposal: x = SigmaL * z1 [; x = beta*x + (1-beta)*SigmaLm*z2]; x += v
    if (carried) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int e = r * G + g.lane;
        x[r] = e < d ? B.t_xnext[(size_t)c * DP + e] : 0.0;
      }
    } else {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int e = r * G + g.lane;
      if (e < d) mmb_normal_pair(&rn, (uint32_t)e, &z1[r], &z2[r]);
      else { z1[r] = 0.0; z2[r] = 0.0; }
    }
    if (!B.sigl_diag) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        int e = r * G + g.lane;
        if (e < d) vvs[e] = z1[r];
      }
      grp_sync();
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int e = r * G + g.lane;
      double a = 0.0;
      if (e < d) {
        if (B.sigl_diag) {
          a = fma(B.sigl[e * d + e], z1[r], a);
        } else {
          for (int k = 0; k <= e; ++k) a = fma(B.sigl[e * d + k], vvs[k], a);
        }
      }
      x[r] = a;
    }
    if (m > 2 * d) {
      double y[R];
#pragma unroll
      for (int r = 0; r < R; ++r) y[r] = 0.0;
      if (fl & 4) {
        grp_sync();
        const double* Ls = B.t_Ls + (size_t)c * TP;
        double lt[NT];  // all loads issued before the first use (one HBM latency, not NT)
#pragma unroll
        for (int u = 0; u < NT; ++u) lt[u] = (u * G + g.lane < T) ? Ls[u * G + g.lane] : 0.0;
#pragma unroll
        for (int u = 0; u < NT; ++u)
          if (u * G + g.lane < T) mat[u * G + g.lane] = lt[u];
        if constexpr (POSFORM) {
          // position form: this lane's row starts at tri(pos e); y = sum_{k <= pos e} L z2s[k]
          // in k order (the diagonal last), as the slot-form matvec below
          const int e = g.lane;
          const int pe = e < d ? (int)B.t_piv[(size_t)c * DP + e] : 0;
          if (e < d) z2s[e] = z2[0];
          grp_sync();
          const double* row = mat + mmb_tri(pe);
          double a = 0.0;
#pragma unroll
          for (int k = 0; k < DMAX; ++k)
            if (k < d) a = k <= pe ? fma(row[k], z2s[k], a) : a;
          if (e < d) y[0] = a;
        } else {
        // pivot order: the chain's DP bytes as DP/4 words in registers (uniform per group),
        // so the matvec's LDS reads are independent of each other (no ia[k] -> mat chain)
        uint32_t pw[DP / 4];
        const uint32_t* pvw = (const uint32_t*)(B.t_piv + (size_t)c * DP);
#pragma unroll
        for (int w = 0; w < DP / 4; ++w) pw[w] = pvw[w];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          int e = r * G + g.lane;
          if (e < d) z2s[e] = z2[r];
        }
        grp_sync();
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int e = r * G + g.lane;
          int pe = 0;  // position of e in the pivot order
#pragma unroll
          for (int k = 0; k < DMAX; ++k)
            if (k < d && (int)((pw[k >> 2] >> (8 * (k & 3))) & 0xffu) == e) pe = k;
          double a = 0.0;
#pragma unroll
          for (int k = 0; k < DMAX; ++k) {
            if (k < d) {
              const int q = (int)((pw[k >> 2] >> (8 * (k & 3))) & 0xffu);
              const double m_ = mat[mmb_slot(e, q)];
              const double z_ = z2s[k];
              a = (k < pe) ? fma(m_, z_, a) : a;
            }
          }
          if (e < d) y[r] = fma(mat[mmb_tri(e) + e], z2s[pe], a);
        }
        }  // !POSFORM
      }
#pragma unroll
      for (int r = 0; r < R; ++r) x[r] = B.beta * x[r] + (1.0 - B.beta) * y[r];
    }
    }  // !carried
#pragma unroll
    for (int r = 0; r < R; ++r) x[r] = x[r] + v[r];
    MMB_PROF_MARK(2, g.lane)
    const typename M::Prep pc = M::prep(B, s, g, pk);
    MMB_PROF_MARK(0, g.lane)
    double lx, lv;
    M::logf_p2(A, B, pc, s, l, g, x, v, lx, lv);
    const double ua = G == 32 ? upre : mmb_uniform(&ru, 0u);  // predraw() for 32-lane groups
    if (ua < mmb_exp(lx - lv)) {
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = x[r];
    }
    MMB_PROF_MARK(3, g.lane)
    if (!adapt) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        int e = r * G + g.lane;
        if (e < d) ((dual && (m & 1)) ? B.t_Mv_alt : B.t_Mv)[(size_t)c * DP + e] = mv[r];
      }
      if (g.lane == 0) { B.t_m[c] = m; B.t_flags[c] = fl; }
      grp_sync();
      M::relist(B, s, g, v);
      return;
    }
    {  // amm.jl:81-91
      m += 1;
      const double p = (double)m / ((double)m + 1.0);
      const double q = 1.0 - p;
      // fresh, models that evaluate logpdf! in the state itself (mmb_noprop): mv is still setadapt!'s
      // copy of the unlisted old value, kept for Mvv = v_old v_old' below
      double vkeep[R];
      if constexpr (mmb_noprop<M>::value) {
#pragma unroll
        for (int r = 0; r < R; ++r) vkeep[r] = mv[r];
      }
      if (fl & 2) {
#pragma unroll
        for (int r = 0; r < R; ++r) mv[r] = p * v[r] + q * v[r];
        fl &= ~2;
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) mv[r] = p * mv[r] + q * v[r];
      }
      grp_sync();
      // (v[e], Mv[e]) pairs interleaved over the vvs|mvs scratch: one 16-byte read per index
      double2* vm = (double2*)vvs;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        int e = r * G + g.lane;
        if (e < d) vm[e] = make_double2(v[r], mv[r]);
      }
      const double cc = (B.scale * B.scale / (double)d) / p;
      // two moment buffers: read Mvv(m - 1) from the copy of that parity, write Mvv(m) to the other
      double* Mvv = ((dual && ((m - 1) & 1)) ? B.t_Mvv_alt : B.t_Mvv) + (size_t)c * TP;
      double* Mvv_w = ((dual && (m & 1)) ? B.t_Mvv_alt : B.t_Mvv) + (size_t)c * TP;
      // fresh: Mvv = v_old v_old' was formed before the proposal; v_old is still unlist()
      // of the state `s`, so recompute it from s here (same products).  Not so where logf_p2 has
      // written invlink(v_old) into the state itself (the node IR's NOPROP layout): under a log or
      // logit link unlist() of that is link(invlink(link(state))), a rounding away from v_old.
      double vold[R];
      if (fresh) {
        if constexpr (mmb_noprop<M>::value) {
#pragma unroll
          for (int r = 0; r < R; ++r) vold[r] = vkeep[r];
        } else {
          M::unlist(B, s, g.lane, vold);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          int e = r * G + g.lane;
          if (e < d) z2s[e] = vold[r];
        }
      }
      grp_sync();
      // the lane's own Mvv slots straight into registers, all loads in flight at once.  Slots
      // T <= t < TP are the row's padding (never read as Mvv / Sigma): they are updated like the
      // others from stale scratch, so no slot needs a branch (rats: NT * G == TP exactly), and
      // the new values are stored after the slot loop -- an HBM store between two uses of the
      // loaded values would make every use wait for the stores before it (vmcnt(0)).
      double lt[NT];
#pragma unroll
      for (int u = 0; u < NT; ++u) lt[u] = (!fresh && u * G + g.lane < TP) ? Mvv[u * G + g.lane] : 0.0;
      // slot t = u G + lane: HBM and LDS addresses are the lane's base + a constant per u
      // (immediate offsets), the fresh / steady choice is made once outside the slot loop
      double* const Mvv_l = Mvv_w + g.lane;
      double* const mat_l = mat + g.lane;
      auto slots = [&](auto fresh_c) {
        constexpr bool FRESH = decltype(fresh_c)::value;
        // opaque once per update: the table reads can be issued together (one LDS wait), but
        // not hoisted out of the iteration loop (2 * NT ints live across it: spills)
        int li0 = g.lane;
        asm volatile("" : "+v"(li0));
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          const int t = u * G + g.lane;
          if ((u + 1) * G <= TP || t < TP) {
            int i, k;
            if constexpr (IKTAB) {
              const int li = li0;
              const int w = ik_table()[li + u * G];
              i = w >> 8;
              k = w & 255;
            } else {
              int ti = t;
              asm volatile("" : "+v"(ti));
              slot_ik(ti, i, k);
            }
            const double2 a = vm[k], bi = vm[i];
            const double old = FRESH ? z2s[i] * z2s[k] : lt[u];
            const double nv = p * old + (q * a.x) * bi.x;
            lt[u] = nv;
            mat_l[u * G] = cc * (nv - a.y * bi.y);
          }
        }
      };
      if (fresh) slots(mmb_bc<true>{});
      else slots(mmb_bc<false>{});
#pragma unroll
      for (int u = 0; u < NT; ++u)
        if ((u + 1) * G <= TP || u * G + g.lane < TP) Mvv_l[u * G] = lt[u];
      grp_sync();
      // everything but the factorization is finished first; the chain state is parked
      // in LDS so the Cholesky's register footprint does not stack on top of it
#pragma unroll
      for (int r = 0; r < R; ++r) {
        int e = r * G + g.lane;
        if (e < d) ((dual && (m & 1)) ? B.t_Mv_alt : B.t_Mv)[(size_t)c * DP + e] = mv[r];
      }
      if (g.lane == 0) { B.t_m[c] = m; B.t_flags[c] = fl; }
      M::relist(B, s, g, v);
      M::stash(lds, s, g.lane);
      grp_sync();
      MMB_PROF_MARK(4, g.lane)
    }
    }  // !recover
    int rank;
    int redo = 0;
    int pe = 0;
    if constexpr (G == 32 && R == 1)
      rank = pchol32(d, mat, (double*)ia, pks, g, &pe, (carry && !recover) ? &B : nullptr, A, c, chain, it, b, m, &redo,
                     !lazy || recover);
    else
      rank = pchol(d, mat, (double*)ia, pks, g);
    grp_sync();
    MMB_PROF_MARK(5, g.lane)
    if (!recover && B.t_astat != nullptr) amm_count(B, c, d, rank, redo, g);
    if (rank == d && (recover ? rec : !lazy)) {
      double* Ls = B.t_Ls + (size_t)c * TP;
#pragma unroll
      for (int u = 0; u < NT; ++u)
        if (u * G + g.lane < T) Ls[u * G + g.lane] = mat[u * G + g.lane];
      uint8_t* pv = B.t_piv + (size_t)c * DP;
      if constexpr (POSFORM) {
        if (g.lane < d) pv[g.lane] = (uint8_t)pe;  // position of element lane
      } else {
        for (int k = g.lane; k < d; k += G) pv[k] = (uint8_t)pks[k];
      }
    }
    if constexpr (!CARRY) {
      if (rank == d && g.lane == 0) B.t_flags[c] = fl | 4;
    } else {
      if (recover) {
        if (rec && g.lane == 0) B.t_flags[c] = (fl | 4) & ~STALE;
        rec = false;
      } else {
        if (rank == d && g.lane == 0) B.t_flags[c] = lazy ? (fl | 4 | STALE) : ((fl | 4) & ~STALE);
        rec = (fl & STALE) != 0 && rank < d;  // the caller runs the block again at once
      }
    }
    M::unstash(lds, s, g.lane);
    grp_sync();
    MMB_PROF_MARK(6, g.lane)
  }

  // ---------------------------------------------------------------- Slice
  // The reference shrinks until it accepts (slice.jl:78-88,103-113); a kernel must end, so
  // after MMB_SLICE_MAX_SHRINK rejections the update stops, the chain-update is counted in
  // stat[3] and mmb_run fails with MMB_E_STATE (never a silent out-of-slice draw).  Only a
  // degenerate target gets there (e.g. an infinite width: every candidate is NaN, -Inf).
  __device__ __forceinline__ static void slice_overflow(const SweepArgs& A, const Grp<G>& g) {
    if (g.lane == 0) atomicAdd(&A.nuts_stat[3], 1ull);
  }
  __device__ __forceinline__ static double width(const DBlock& B, int e) {
    return B.width ? B.width[e] : B.width0;
  }
  // The sequential uniforms of a lane group's update (Slice, univariate) 32 at a time: lane j of
  // the group draws index base + j (the same Philox draws, bit-identical), a step takes its index
  // from its lane (ds_bpermute: the two groups of a wave may be at different indices); a group
  // that runs past the window refills it.  Replaces one all-lane Philox per draw.
  struct UWin {
    double u;
    uint32_t base;
  };
  __device__ __forceinline__ static double uwin_next(const mmb_rng& ru, UWin& w, uint32_t k, const Grp<G>& g) {
    if (k - w.base >= (uint32_t)G) {  // group-uniform
      w.base = k;
      w.u = mmb_uniform(&ru, k + (uint32_t)g.lane);
    }
    const int src = (int)(threadIdx.x & 63 & ~(G - 1)) + (int)(k - w.base);
    return __shfl(w.u, src, 64);
  }
  // slice.jl:66-92 (Univariate) with the shrink loop's candidates evaluated four at a time
  // (models with M::SLICE_CAND: lanes 8q .. 8q+7 of the chain evaluate candidate q).  Given that
  // every earlier candidate was rejected, the candidates of a coordinate are fixed in advance:
  // candidate j = lo + (up - lo) * u_j, then lo or up moves to it by its side of the current
  // value -- the loop's arithmetic on its uniforms, independent of the logpdf values.  A round
  // forms the next four on every lane, evaluates them at once (exact logf values: the model's
  // evaluator sums the same tree), and takes the first that the loop would accept; the uniform
  // index, the logf0 carried to the next coordinate and the overflow case follow the loop.  The
  // draws are the sequential loop's, bit for bit.
  __device__ __forceinline__ static void slice_uni_cand(const SweepArgs& A, const DBlock& B, const mmb_rng& ru,
                                                        St& s, const Lc& l, const Grp<G>& g, double* lds) {
    constexpr int SD = M::SLICE_CAND_D;
    constexpr int NC = M::SLICE_NC, LPC = 32 / NC;  // candidates per round, lanes per candidate
    constexpr uint32_t LEAD = NC == 2 ? 0x00010001u : NC == 4 ? 0x01010101u : 0x11111111u;  // group leaders' ballot bits
    static_assert(MMB_SLICE_MAX_SHRINK % NC == 0, "rounds of candidates end at the cap");
    const int d = B.d;
    double x[R];
    M::unlist(B, s, g.lane, x);
    typename M::SCtx cx;
    M::slice_cand_prep(A, B, s, l, g, lds, cx);
    double logf0 = M::slice_logf0(A, B, s, l, g, x, cx);  // logf, reusing the prep's sums
    double lo = 0.0, up = 0.0;
    if (g.lane < d) {
      const double w = width(B, g.lane);
      lo = x[0] - w * mmb_uniform(&ru, (uint32_t)g.lane);
      up = lo + w;
    }
    typename M::SMemo memo;
    double xu[SD], lou[SD], upu[SD];  // element values and intervals, group-uniform
#pragma unroll
    for (int a = 0; a < SD; ++a) {
      xu[a] = a < d ? g.bcast(x[0], a) : 0.0;
      lou[a] = a < d ? g.bcast(lo, a) : 0.0;
      upu[a] = a < d ? g.bcast(up, a) : 0.0;
    }
    uint32_t k = (uint32_t)d;
    UWin uw{0.0, 0xffffffffu - (uint32_t)G};
    const int q = g.lane / LPC;
    const int gbase = (int)(threadIdx.x & 63) & ~(G - 1);
    for (int e = 0; e < d; ++e) {
      const double p0 = logf0 + mmb_log(uwin_next(ru, uw, k++, g));
      double xo = xu[0], lo_ = lou[0], up_ = upu[0];
#pragma unroll
      for (int a = 1; a < SD; ++a)
        if (a == e) { xo = xu[a]; lo_ = lou[a]; up_ = upu[a]; }
      double xn = 0.0, lfn = 0.0;
      // candidate j (from 1) takes uniform k + j - 1
      for (uint32_t j0 = 0;; j0 += NC) {
        double cand[NC];
#pragma unroll
        for (int t = 0; t < NC; ++t) {
          const double cv = lo_ + (up_ - lo_) * uwin_next(ru, uw, k + j0 + (uint32_t)t, g);
          cand[t] = cv;
          if (cv < xo) lo_ = cv;
          else up_ = cv;
        }
        double mine = cand[0];
#pragma unroll
        for (int t = 1; t < NC; ++t) mine = q == t ? cand[t] : mine;
        double xv[SD];
#pragma unroll
        for (int a = 0; a < SD; ++a) xv[a] = a == e ? mine : xu[a];
        const double lp = M::slice_cand_logf(A, B, s, cx, xv, g.lane, memo);
        const bool hit = !(lp < p0) && j0 + (uint32_t)q + 1u <= (uint32_t)MMB_SLICE_MAX_SHRINK;
        const uint64_t bal = __ballot(hit && (g.lane & (LPC - 1)) == 0);
        const uint32_t hb = (uint32_t)(bal >> gbase) & LEAD;  // candidate q -> bit LPC q
        if (hb != 0u) {
          const int qs = __builtin_ctz(hb) / LPC;
          xn = cand[0];
#pragma unroll
          for (int t = 1; t < NC; ++t) xn = qs == t ? cand[t] : xn;
          lfn = __shfl(lp, gbase + LPC * qs, 64);
          k += j0 + (uint32_t)qs + 1u;
          break;
        }
        if (j0 + (uint32_t)NC >= (uint32_t)MMB_SLICE_MAX_SHRINK) {  // every candidate up to the cap rejected:
          xn = lo_ + (up_ - lo_) * uwin_next(ru, uw, k + j0 + (uint32_t)NC, g);  // the loop's last draw
          lfn = __shfl(lp, gbase + LPC * (NC - 1), 64);                           // logf of the cap-th
          k += j0 + (uint32_t)NC + 1u;
          slice_overflow(A, g);
          break;
        }
      }
#pragma unroll
      for (int a = 0; a < SD; ++a) xu[a] = a == e ? xn : xu[a];
      logf0 = lfn;
      if (g.lane == e) x[0] = xn;
    }
    M::relist(B, s, g, x);
  }
  // slice.jl:66-92 (Univariate)
  __device__ __forceinline__ static void slice_uni(const SweepArgs& A, const DBlock& B, const mmb_rng& ru, St& s,
                                   const Lc& l, const Grp<G>& g, double* lds) {
    if constexpr (M::SLICE_CAND && G == 32 && R == 1) {
      if (A.slice_exact == 0 && M::slice_cand_ok(B)) {
        slice_uni_cand(A, B, ru, s, l, g, lds);
        return;
      }
    }
    const int d = B.d;
    double x[R], lo[R], up[R];
    M::unlist(B, s, g.lane, x);
    double logf0 = M::logf(A, B, s, l, g, x);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int e = r * G + g.lane;
      if (e < d) {
        double w = width(B, e);
        lo[r] = x[r] - w * mmb_uniform(&ru, (uint32_t)e);
        up[r] = lo[r] + w;
      } else { lo[r] = 0.0; up[r] = 0.0; }
    }
    uint32_t k = (uint32_t)d;
    UWin uw{0.0, 0xffffffffu - (uint32_t)G};  // empty window: the first draw fills it
    auto next_u = [&](uint32_t kk) __attribute__((always_inline)) -> double {
      if constexpr (G == 32) return uwin_next(ru, uw, kk, g);
      else return mmb_uniform(&ru, kk);
    };
#pragma unroll
    for (int r = 0; r < R; ++r) {
      for (int ln = 0; ln < G; ++ln) {
        int e = r * G + ln;
        if (e >= d) break;
        bool own = g.lane == ln;
        double p0 = logf0 + mmb_log(next_u(k++));
        double xo = x[r];
        double u = next_u(k++);
        if (own) x[r] = lo[r] + (up[r] - lo[r]) * u;
        bool hit = false;
        for (int guard = 0; guard < MMB_SLICE_MAX_SHRINK; ++guard) {
          logf0 = M::logf(A, B, s, l, g, x);
          if (!(logf0 < p0)) { hit = true; break; }
          if (own) {
            double value = x[r];
            if (value < xo) lo[r] = value;
            else up[r] = value;
          }
          u = next_u(k++);
          if (own) x[r] = lo[r] + (up[r] - lo[r]) * u;
        }
        if (!hit) slice_overflow(A, g);
      }
    }
    M::relist(B, s, g, x);
  }
  // slice.jl:95-117 (Multivariate), candidates four at a time as slice_uni_cand: candidate 1 is
  // w u + lo per element, candidate j > 1 moves each lo / up to candidate j - 1's element by its
  // side of the current value and draws lo + (up - lo) u, uniforms 1 + 2d + (j - 2) d + e
  __device__ __forceinline__ static void slice_multi_cand(const SweepArgs& A, const DBlock& B, const mmb_rng& ru,
                                                          St& s, const Lc& l, const Grp<G>& g, double* lds) {
    constexpr int SD = M::SLICE_CAND_D;
    const int d = B.d;
    double v[R];
    M::unlist(B, s, g.lane, v);
    UWin uw{0.0, 0xffffffffu - (uint32_t)G};
    typename M::SCtx cx;
    M::slice_cand_prep(A, B, s, l, g, lds, cx);
    const double p0 = M::slice_logf0(A, B, s, l, g, v, cx) + mmb_log(uwin_next(ru, uw, 0u, g));
    typename M::SMemo memo;
    double vu[SD], lo[SD], up[SD], x1[SD];
#pragma unroll
    for (int a = 0; a < SD; ++a) {
      vu[a] = a < d ? g.bcast(v[0], a) : 0.0;
      lo[a] = up[a] = x1[a] = 0.0;
      if (a < d) {
        const double w = width(B, a);
        lo[a] = vu[a] - w * uwin_next(ru, uw, 1u + (uint32_t)a, g);
        up[a] = lo[a] + w;
        x1[a] = w * uwin_next(ru, uw, 1u + (uint32_t)d + (uint32_t)a, g) + lo[a];
      }
    }
    constexpr int NC = M::SLICE_NC, LPC = 32 / NC;
    constexpr uint32_t LEAD = NC == 2 ? 0x00010001u : NC == 4 ? 0x01010101u : 0x11111111u;
    const int q = g.lane / LPC;
    const int gbase = (int)(threadIdx.x & 63) & ~(G - 1);
    double prev[SD], xn[SD];
    // candidate j > 1 from candidate j - 1 (the loop's shrink and redraw)
    auto next = [&](const double* pv, uint32_t j, double* out) __attribute__((always_inline)) {
      const uint32_t kk = 1u + 2u * (uint32_t)d + (j - 2u) * (uint32_t)d;
#pragma unroll
      for (int a = 0; a < SD; ++a) {
        if (a < d) {
          if (pv[a] < vu[a]) lo[a] = pv[a];
          else up[a] = pv[a];
          out[a] = lo[a] + (up[a] - lo[a]) * uwin_next(ru, uw, kk + (uint32_t)a, g);
        } else {
          out[a] = 0.0;
        }
      }
    };
    for (uint32_t j0 = 0;; j0 += NC) {
      double cand[NC][SD];
#pragma unroll
      for (int t = 0; t < NC; ++t) {
        if (j0 + (uint32_t)t == 0u) {
#pragma unroll
          for (int a = 0; a < SD; ++a) cand[t][a] = x1[a];
        } else {
          next(t == 0 ? prev : cand[t - 1], j0 + (uint32_t)t + 1u, cand[t]);
        }
      }
#pragma unroll
      for (int a = 0; a < SD; ++a) prev[a] = cand[NC - 1][a];
      double xv[SD];
#pragma unroll
      for (int a = 0; a < SD; ++a) {
        xv[a] = cand[0][a];
#pragma unroll
        for (int t = 1; t < NC; ++t) xv[a] = q == t ? cand[t][a] : xv[a];
      }
      const double lp = M::slice_cand_logf(A, B, s, cx, xv, g.lane, memo);
      const bool hit = !(lp < p0) && j0 + (uint32_t)q + 1u <= (uint32_t)MMB_SLICE_MAX_SHRINK;
      const uint64_t bal = __ballot(hit && (g.lane & (LPC - 1)) == 0);
      const uint32_t hb = (uint32_t)(bal >> gbase) & LEAD;
      if (hb != 0u) {
        const int qs = __builtin_ctz(hb) / LPC;
#pragma unroll
        for (int a = 0; a < SD; ++a) {
          xn[a] = cand[0][a];
#pragma unroll
          for (int t = 1; t < NC; ++t) xn[a] = qs == t ? cand[t][a] : xn[a];
        }
        break;
      }
      if (j0 + (uint32_t)NC >= (uint32_t)MMB_SLICE_MAX_SHRINK) {  // the cap: the loop's last shrink and draw
        next(prev, j0 + (uint32_t)NC + 1u, xn);
        slice_overflow(A, g);
        break;
      }
    }
    double x[R];
    x[0] = 0.0;
#pragma unroll
    for (int a = 0; a < SD; ++a)
      if (g.lane == a && a < d) x[0] = xn[a];
    M::relist(B, s, g, x);
  }
  // slice.jl:95-117 (Multivariate)
  __device__ __forceinline__ static void slice_multi(const SweepArgs& A, const DBlock& B, const mmb_rng& ru, St& s,
                                     const Lc& l, const Grp<G>& g, double* lds) {
    if constexpr (M::SLICE_CAND && G == 32 && R == 1) {
      if (A.slice_exact == 0 && M::slice_cand_ok(B)) {
        slice_multi_cand(A, B, ru, s, l, g, lds);
        return;
      }
    }
    const int d = B.d;
    double v[R], x[R], lo[R], up[R];
    M::unlist(B, s, g.lane, v);
    uint32_t k = 0;
    double p0 = M::logf(A, B, s, l, g, v) + mmb_log(mmb_uniform(&ru, k++));
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int e = r * G + g.lane;
      if (e < d) {
        double w = width(B, e);
        lo[r] = v[r] - w * mmb_uniform(&ru, 1u + (uint32_t)e);
        up[r] = lo[r] + w;
        x[r] = w * mmb_uniform(&ru, 1u + (uint32_t)d + (uint32_t)e) + lo[r];
      } else { lo[r] = up[r] = x[r] = 0.0; }
    }
    k = 1u + 2u * (uint32_t)d;
    bool hit = false;
    for (int guard = 0; guard < MMB_SLICE_MAX_SHRINK; ++guard) {
      if (!(M::logf(A, B, s, l, g, x) < p0)) { hit = true; break; }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        int e = r * G + g.lane;
        if (e < d) {
          double value = x[r];
          if (value < v[r]) lo[r] = value;
          else up[r] = value;
          x[r] = lo[r] + (up[r] - lo[r]) * mmb_uniform(&ru, k + (uint32_t)e);
        }
      }
      k += (uint32_t)d;
    }
    if (!hit) slice_overflow(A, g);
    M::relist(B, s, g, x);
  }

  // ---------------------------------------------------------------- NUTS
  // sample!(v::NUTSVariate) with the model gradient computed inline (nuts.h machine).
  // Model path: adapts iff iter <= burnin (nuts.jl:52).
  __device__ __forceinline__ static void nuts(const SweepArgs& A, const DBlock& B, int c, int64_t it, int b,
                                              St& s, const Grp<G>& g) {
    using NU = Nuts<G, R>;
    typename NU::St S;
    const double* tn = B.t_nuts + (size_t)c * 8;
    S.t_eps = tn[0]; S.t_epsbar = tn[1]; S.t_Hbar = tn[2]; S.t_mu = tn[3];
    S.t_alpha = tn[4]; S.t_nalpha = tn[5];
    S.t_m = B.t_m[c];
    S.t_flags = B.t_flags[c];
    M::unlist(B, s, g.lane, S.v);
    S.pc = NPC_BEGIN;
    const uint32_t chain = A.chain_offset + (uint32_t)c;
    typename NU::Env E;
    E.d = B.d;
    E.lane = g.lane;
    E.adapt = it <= A.model_burnin;
    E.target = B.target;
    E.rn = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_NORMAL);
    E.ru = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_UNIFORM);
    E.ri = mmb_rng_make(A.seed, chain, (uint32_t)it, (uint32_t)b, MMB_SUB_INIT);
    E.F = B.t_nfr + (size_t)c * NutsFrames<NU::DV>::DBL;
    E.stat = A.nuts_stat;
    while (NU::advance(S, E, g)) S.lf = M::logf_grad(A, B, s, S.x, S.g);
    double* tw = B.t_nuts + (size_t)c * 8;
    if (g.lane == 0) {
      tw[0] = S.t_eps; tw[1] = S.t_epsbar; tw[2] = S.t_Hbar; tw[3] = S.t_mu;
      tw[4] = S.t_alpha; tw[5] = S.t_nalpha;
      B.t_m[c] = S.t_m;
      B.t_flags[c] = S.t_flags;
    }
    M::relist(B, s, g, S.v);
  }

  // ---------------------------------------------------------------- HMC / MALA
  // sample!(v::HMCVariate) (hmc.jl:72-111) / sample!(v::MALAVariate) (mala.jl:67-86), hmc.h
  // machines with the model gradient computed inline; tune (epsilon, L) is per chain.
  template <bool MALA>
  __device__ __forceinline__ static void hmc(const SweepArgs& A, const DBlock& B, int c, const mmb_rng& rn,
                                             const mmb_rng& ru, St& s, const Grp<G>& g) {
    using HM = Hmc<G, R>;
    typename HM::St S;
    typename HM::Env E;
    const double* th = B.t_hmc + (size_t)c * 2;
    E.d = B.d;
    E.lane = g.lane;
    E.eps = th[0];
    E.L = (int)th[1];
    E.sigl = B.sigl;
    E.rn = rn;
    E.ru = ru;
    M::unlist(B, s, g.lane, S.v);
    S.pc = HPC_BEGIN;
    if (MALA) {
      while (HM::advance_mala(S, E, g)) S.lf = M::logf_grad(A, B, s, S.x, S.g);
    } else {
      while (HM::advance_hmc(S, E, g)) S.lf = M::logf_grad(A, B, s, S.x, S.g);
    }
    M::relist(B, s, g, S.v);
  }
};
