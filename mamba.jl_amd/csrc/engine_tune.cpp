// engine_tune.cpp — the canonical tune row: its length per block and the two directions between it
// and the device's tune state (mmb_get_tune / mmb_set_tune).
#include "engine.h"

int tune_len_of(int kind, int d, int nsim, int nstat) {
  switch (kind) {
    case MMB_SAMPLER_AMWG: return 2 + 2 * d;
    case MMB_SAMPLER_AMM: return 4 + 2 * d + 2 * tri(d);
    case MMB_SAMPLER_NUTS: return 9;
    case MMB_SAMPLER_HMC: return 2;   // [epsilon, L]     (HMCTune, hmc.jl:5-10)
    case MMB_SAMPLER_MALA: return 1;  // [epsilon]        (MALATune, mala.jl:5-9)
    case MMB_SAMPLER_RWM: return d;   // scale[d]         (RWMTune, rwm.jl:5-9)
    case MMB_SAMPLER_DGS: return 0;   // no tuning state  (DGSTune holds only the mass function, dgs.jl:12-26)
    case MMB_SAMPLER_SLICESIMPLEX: return 0;  // none either (SliceSimplexTune: logf and the constant scale)
    case MMB_SAMPLER_BMG: return 0;           // none (BMGTune: logf and the constant k, bmg.jl:7-16)
    case MMB_SAMPLER_BMC3: return 0;          // none (BMC3Tune likewise, bmc3.jl:7-16)
    case MMB_SAMPLER_BIA: return 1 + 2 * d;   // [iter, A[d], D[d]]  (BIATune, bia.jl:5-25)
    case MMB_SAMPLER_BHMC: return 2 * d + 3;  // [position[d], velocity[d], wallhits, wallcrosses, initialised]
                                              // (BHMCTune, bhmc.jl:5-19)
    case MMB_SAMPLER_ABC: return 1 + nsim * (nstat + 2);  // [initialised, Tsim[nsim][T], epsilon[nsim],
                                                          // epsilonprime[nsim]]  (ABCTune, abc.jl:5-18)
    default: return 0;
  }
}

int64_t mmb_tune_len(const mmb_engine* e) {
  if (!e) return MMB_E_ARG;
  int64_t n = 0;
  for (auto& h : e->blocks) n += h.tune_len;
  return n;
}

// ---------------------------------------------------------------- tune (canonical layout)

// The 32-lane factorization (samplers.h pchol32: rats, node IR) keeps the AMM factor in
// POSITION form on device -- row at pivot position t at tri(t) + k, k = 0..t, plus one byte per
// element holding its position -- while the canonical tune layout (and the oracle) use the slot
// form L[e][step k] -> slot(e, piv[k]), diagonal at slot(e, e), plus the pivot order.
static int slot_(int i, int k) { return i >= k ? tri(i) + k : tri(k) + i; }
// position form (lp, pos) -> slot form (ls, piv); one chain, d x d
static void pos_to_slot(int d, const double* lp, const uint8_t* pos, double* ls, uint8_t* piv) {
  for (int e = 0; e < d; ++e) piv[pos[e] < d ? pos[e] : e] = (uint8_t)e;
  for (int e = 0; e < d; ++e) {
    const int pe = pos[e] < d ? pos[e] : e;
    for (int k = 0; k < pe; ++k) ls[slot_(e, piv[k])] = lp[tri(pe) + k];
    ls[slot_(e, e)] = lp[tri(pe) + pe];
  }
}
static void slot_to_pos(int d, const double* ls, const uint8_t* piv, double* lp, uint8_t* pos) {
  for (int k = 0; k < d; ++k) pos[piv[k] < d ? piv[k] : k] = (uint8_t)k;
  for (int e = 0; e < d; ++e) {
    const int pe = pos[e];
    for (int k = 0; k < pe; ++k) lp[tri(pe) + k] = ls[slot_(e, piv[k])];
    lp[tri(pe) + pe] = ls[slot_(e, e)];
  }
}

int mmb_get_tune(mmb_engine* e, double* tune) {
  if (!e || !tune) return fail(e, MMB_E_ARG, "null argument");
  if (!e->d_vals) return fail(e, MMB_E_STATE, "mmb_init_chains not called");
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  const int64_t TL = mmb_tune_len(e), K = e->K;
  const size_t DP = e->DP, TP = e->TP;
  int64_t off = 0;
  for (auto& h : e->blocks) {
    std::vector<int32_t> m, fl;
    int rc;
    if ((rc = d2h(e, m, h.m, K)) || (rc = d2h(e, fl, h.flags, K))) return rc;
    if (h.spec.sampler == MMB_SAMPLER_AMWG) {
      std::vector<double> sg, ac;
      if ((rc = d2h(e, sg, h.sigma, K * DP)) || (rc = d2h(e, ac, h.accept, K * DP))) return rc;
      for (int64_t k = 0; k < K; ++k) {
        double* t = tune + k * TL + off;
        t[0] = (fl[k] & 1) ? 1.0 : 0.0;
        t[1] = m[k];
        for (int i = 0; i < h.d; ++i) { t[2 + i] = sg[k * DP + i]; t[2 + h.d + i] = ac[k * DP + i]; }
      }
    } else if (h.spec.sampler == MMB_SAMPLER_AMM) {
      std::vector<double> mv, mvv, ls;
      std::vector<uint8_t> pv;
      if ((rc = d2h(e, mv, h.Mv, K * DP)) || (rc = d2h(e, mvv, h.Mvv, K * TP)) ||
          (rc = d2h(e, ls, h.Ls, K * TP)) || (rc = d2h(e, pv, h.piv, K * DP)))
        return rc;
      if (h.Mv_alt) {  // two moment buffers: chain k's current ones are those of m[k]'s parity
        std::vector<double> mva, mvva;
        if ((rc = d2h(e, mva, h.Mv_alt, K * DP)) || (rc = d2h(e, mvva, h.Mvv_alt, K * TP))) return rc;
        for (int64_t k = 0; k < K; ++k) {
          if (!(m[k] & 1)) continue;
          std::copy(&mva[k * DP], &mva[k * DP] + DP, &mv[k * DP]);
          std::copy(&mvva[k * TP], &mvva[k * TP] + TP, &mvv[k * TP]);
        }
      }
      for (int64_t k = 0; k < K; ++k) {
        double* t = tune + k * TL + off;
        t[0] = (fl[k] & 1) ? 1.0 : 0.0;
        t[1] = m[k];
        t[2] = (fl[k] & 4) ? 1.0 : 0.0;
        t[3] = (fl[k] & 2) ? 1.0 : 0.0;
        double* p = t + 4;
        for (int i = 0; i < h.d; ++i) p[i] = mv[k * DP + i];
        p += h.d;
        for (int s = 0; s < h.T; ++s) p[s] = mvv[k * TP + s];
        p += h.T;
        if (amm_posform(e)) {
          std::vector<uint8_t> piv(h.d);
          std::fill(p, p + h.T, 0.0);
          pos_to_slot(h.d, &ls[k * TP], &pv[k * DP], p, piv.data());
          p += h.T;
          for (int i = 0; i < h.d; ++i) p[i] = piv[i];
        } else {
          for (int s = 0; s < h.T; ++s) p[s] = ls[k * TP + s];
          p += h.T;
          for (int i = 0; i < h.d; ++i) p[i] = pv[k * DP + i];
        }
      }
    } else if (h.spec.sampler == MMB_SAMPLER_NUTS) {
      std::vector<double> nt;
      if ((rc = d2h(e, nt, h.nuts, K * 8))) return rc;
      for (int64_t k = 0; k < K; ++k) {  // [adapt, m, eps, epsbar, Hbar, mu, alpha, nalpha, init]
        double* t = tune + k * TL + off;
        t[0] = (fl[k] & 1) ? 1.0 : 0.0;
        t[1] = m[k];
        for (int i = 0; i < 6; ++i) t[2 + i] = nt[k * 8 + i];
        t[8] = (fl[k] & 8) ? 1.0 : 0.0;
      }
    } else if (h.spec.sampler == MMB_SAMPLER_HMC || h.spec.sampler == MMB_SAMPLER_MALA) {
      std::vector<double> th;
      if ((rc = d2h(e, th, h.hmc, K * 2))) return rc;
      for (int64_t k = 0; k < K; ++k)
        for (int i = 0; i < h.tune_len; ++i) tune[k * TL + off + i] = th[k * 2 + i];
    } else if (h.spec.sampler == MMB_SAMPLER_RWM) {
      std::vector<double> sg;
      if ((rc = d2h(e, sg, h.sigma, K * DP))) return rc;
      for (int64_t k = 0; k < K; ++k)
        for (int i = 0; i < h.d; ++i) tune[k * TL + off + i] = sg[k * DP + i];
    } else if (h.spec.sampler == MMB_SAMPLER_BIA) {
      std::vector<double> ta, td;
      if ((rc = d2h(e, ta, h.sigma, K * DP)) || (rc = d2h(e, td, h.accept, K * DP))) return rc;
      for (int64_t k = 0; k < K; ++k) {
        double* t = tune + k * TL + off;
        t[0] = m[k];
        for (int i = 0; i < h.d; ++i) { t[1 + i] = ta[k * DP + i]; t[1 + h.d + i] = td[k * DP + i]; }
      }
    } else if (h.spec.sampler == MMB_SAMPLER_ABC) {  // the device keeps the canonical row
      std::vector<double> tr;
      if ((rc = d2h(e, tr, h.hmc, K * h.tune_len))) return rc;
      for (int64_t k = 0; k < K; ++k)
        for (int i = 0; i < h.tune_len; ++i) tune[k * TL + off + i] = tr[k * h.tune_len + i];
    } else if (h.spec.sampler == MMB_SAMPLER_BHMC) {
      std::vector<double> tp, tv, tc;
      if ((rc = d2h(e, tp, h.sigma, K * DP)) || (rc = d2h(e, tv, h.accept, K * DP)) || (rc = d2h(e, tc, h.hmc, K * 2)))
        return rc;
      for (int64_t k = 0; k < K; ++k) {
        double* t = tune + k * TL + off;
        for (int i = 0; i < h.d; ++i) { t[i] = tp[k * DP + i]; t[h.d + i] = tv[k * DP + i]; }
        t[2 * h.d] = tc[k * 2];
        t[2 * h.d + 1] = tc[k * 2 + 1];
        t[2 * h.d + 2] = m[k] != 0 ? 1.0 : 0.0;
      }
    }
    off += h.tune_len;
  }
  return 0;
}

int mmb_set_tune(mmb_engine* e, const double* tune) {
  if (!e || !tune) return fail(e, MMB_E_ARG, "null argument");
  if (!e->d_vals) return fail(e, MMB_E_STATE, "mmb_init_chains not called");
  const int64_t TL = mmb_tune_len(e), K = e->K;
  const size_t DP = e->DP, TP = e->TP;
  // validate every row before any device state changes: a valid AMM factor (t[2] != 0) needs
  // its pivot order to be a permutation of 0..d-1 (it indexes the caller's row and the device
  // factor); an invalid one is stored with identity positions whatever its pivot bytes hold
  for (int64_t off = 0, b = 0; b < (int64_t)e->blocks.size(); off += e->blocks[b].tune_len, ++b) {
    const auto& h = e->blocks[b];
    if (h.spec.sampler == MMB_SAMPLER_BIA) {  // bia.jl:41-44: the update takes logs of A - epsilon, 1 - A - epsilon
      for (int64_t k = 0; k < K; ++k) {
        const double* t = tune + k * TL + off;
        bool ok = t[0] >= 0.0 && t[0] < 2147483647.0 && t[0] == (double)(int64_t)t[0];
        for (int i = 0; i < 2 * h.d; ++i) ok = ok && h.spec.epsilon < t[1 + i] && t[1 + i] < 1.0 - h.spec.epsilon;
        if (!ok)
          return fail(e, MMB_E_ARG, "block %d chain %lld: a BIA tune row is [iter, A, D] with iter >= 0 and A, D in "
                      "(epsilon, 1 - epsilon)", (int)b + 1, (long long)k);
      }
      continue;
    }
    if (h.spec.sampler == MMB_SAMPLER_BHMC) {  // the counters are whole numbers a double holds exactly
      for (int64_t k = 0; k < K; ++k) {
        const double* t = tune + k * TL + off + 2 * h.d;
        bool ok = t[2] == 0.0 || t[2] == 1.0;
        for (int i = 0; i < 2; ++i) ok = ok && t[i] >= 0.0 && t[i] < 9007199254740992.0 && t[i] == std::floor(t[i]);
        if (!ok)
          return fail(e, MMB_E_ARG, "block %d chain %lld: a BHMC tune row is [position, velocity, wallhits, wallcrosses, "
                      "initialised] with whole counters >= 0 and initialised 0 or 1", (int)b + 1, (long long)k);
      }
      continue;
    }
    if (h.spec.sampler == MMB_SAMPLER_ABC) {
      for (int64_t k = 0; k < K; ++k) {
        const double t0 = tune[k * TL + off];
        if (!(t0 == 0.0 || t0 == 1.0))
          return fail(e, MMB_E_ARG, "block %d chain %lld: an ABC tune row is [initialised, Tsim, epsilon, epsilonprime] "
                      "with initialised 0 or 1", (int)b + 1, (long long)k);
      }
      continue;
    }
    if (h.spec.sampler != MMB_SAMPLER_AMM) continue;
    for (int64_t k = 0; k < K; ++k) {
      const double* t = tune + k * TL + off;
      if (t[2] == 0.0) continue;
      const double* pv = t + 4 + h.d + 2 * h.T;
      uint32_t seen = 0;
      for (int i = 0; i < h.d; ++i) {
        const double v = pv[i];
        if (!(v >= 0.0 && v < h.d) || v != (double)(int)v || (seen >> (int)v & 1u))
          return fail(e, MMB_E_ARG, "block %d chain %lld: AMM pivot order is not a permutation of 0..%d",
                      (int)b + 1, (long long)k, h.d - 1);
        seen |= 1u << (int)v;
      }
    }
  }
  ++e->xepoch;
  e->order_fresh = false;  // the factor-valid flags change
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  int64_t off = 0;
  for (auto& h : e->blocks) {
    std::vector<int32_t> m(K, 0), fl(K, 0);
    int rc;
    if (h.spec.sampler == MMB_SAMPLER_AMWG) {
      std::vector<double> sg(K * DP, 0.0), ac(K * DP, 0.0);
      for (int64_t k = 0; k < K; ++k) {
        const double* t = tune + k * TL + off;
        fl[k] = t[0] != 0.0 ? 1 : 0;
        m[k] = (int32_t)t[1];
        for (int i = 0; i < h.d; ++i) { sg[k * DP + i] = t[2 + i]; ac[k * DP + i] = t[2 + h.d + i]; }
      }
      if ((rc = h2d(e, h.sigma, sg)) || (rc = h2d(e, h.accept, ac))) return rc;
    } else if (h.spec.sampler == MMB_SAMPLER_AMM) {
      std::vector<double> mv(K * DP, 0.0), mvv(K * TP, 0.0), ls(K * TP, 0.0);
      std::vector<uint8_t> pv(K * DP, 0);
      for (int64_t k = 0; k < K; ++k) {
        const double* t = tune + k * TL + off;
        fl[k] = (t[0] != 0.0 ? 1 : 0) | (t[2] != 0.0 ? 4 : 0) | (t[3] != 0.0 ? 2 : 0);
        m[k] = (int32_t)t[1];
        const double* p = t + 4;
        for (int i = 0; i < h.d; ++i) mv[k * DP + i] = p[i];
        p += h.d;
        for (int s = 0; s < h.T; ++s) mvv[k * TP + s] = p[s];
        p += h.T;
        const bool valid = t[2] != 0.0;
        if (amm_posform(e)) {
          std::vector<uint8_t> piv(h.d);
          for (int i = 0; i < h.d; ++i) piv[i] = valid ? (uint8_t)p[h.T + i] : (uint8_t)i;
          slot_to_pos(h.d, p, piv.data(), &ls[k * TP], &pv[k * DP]);
        } else {
          for (int s = 0; s < h.T; ++s) ls[k * TP + s] = p[s];
          p += h.T;
          for (int i = 0; i < h.d; ++i) pv[k * DP + i] = valid ? (uint8_t)p[i] : (uint8_t)i;
        }
      }
      if ((rc = h2d(e, h.Mv, mv)) || (rc = h2d(e, h.Mvv, mvv)) || (rc = h2d(e, h.Ls, ls)) ||
          (rc = h2d(e, h.piv, pv)))
        return rc;
      // two moment buffers: both get the row, so the one of the chain's m holds it
      if (h.Mv_alt && ((rc = h2d(e, h.Mv_alt, mv)) || (rc = h2d(e, h.Mvv_alt, mvv)))) return rc;
    } else if (h.spec.sampler == MMB_SAMPLER_NUTS) {
      std::vector<double> nt(K * 8, 0.0);
      for (int64_t k = 0; k < K; ++k) {
        const double* t = tune + k * TL + off;
        fl[k] = (t[0] != 0.0 ? 1 : 0) | (t[8] != 0.0 ? 8 : 0);
        m[k] = (int32_t)t[1];
        for (int i = 0; i < 6; ++i) nt[k * 8 + i] = t[2 + i];
      }
      if ((rc = h2d(e, h.nuts, nt))) return rc;
    } else if (h.spec.sampler == MMB_SAMPLER_HMC || h.spec.sampler == MMB_SAMPLER_MALA) {
      std::vector<double> th(K * 2);
      for (int64_t k = 0; k < K; ++k) {
        const double* t = tune + k * TL + off;
        th[k * 2] = t[0];
        th[k * 2 + 1] = h.tune_len > 1 ? t[1] : (double)h.spec.nsteps;
      }
      if ((rc = h2d(e, h.hmc, th))) return rc;
    } else if (h.spec.sampler == MMB_SAMPLER_RWM) {
      std::vector<double> sg(K * DP, 0.0);
      for (int64_t k = 0; k < K; ++k)
        for (int i = 0; i < h.d; ++i) sg[k * DP + i] = tune[k * TL + off + i];
      if ((rc = h2d(e, h.sigma, sg))) return rc;
    } else if (h.spec.sampler == MMB_SAMPLER_BIA) {
      std::vector<double> ta(K * DP, 0.0), td(K * DP, 0.0);
      for (int64_t k = 0; k < K; ++k) {
        const double* t = tune + k * TL + off;
        m[k] = (int32_t)t[0];
        for (int i = 0; i < h.d; ++i) { ta[k * DP + i] = t[1 + i]; td[k * DP + i] = t[1 + h.d + i]; }
      }
      if ((rc = h2d(e, h.sigma, ta)) || (rc = h2d(e, h.accept, td))) return rc;
    } else if (h.spec.sampler == MMB_SAMPLER_ABC) {
      std::vector<double> tr((size_t)K * h.tune_len);
      for (int64_t k = 0; k < K; ++k)
        for (int i = 0; i < h.tune_len; ++i) tr[k * h.tune_len + i] = tune[k * TL + off + i];
      if ((rc = h2d(e, h.hmc, tr))) return rc;
    } else if (h.spec.sampler == MMB_SAMPLER_BHMC) {
      std::vector<double> tp(K * DP, 0.0), tv(K * DP, 0.0), tc(K * 2, 0.0);
      for (int64_t k = 0; k < K; ++k) {
        const double* t = tune + k * TL + off;
        for (int i = 0; i < h.d; ++i) { tp[k * DP + i] = t[i]; tv[k * DP + i] = t[h.d + i]; }
        tc[k * 2] = t[2 * h.d];
        tc[k * 2 + 1] = t[2 * h.d + 1];
        m[k] = t[2 * h.d + 2] != 0.0 ? 1 : 0;
      }
      if ((rc = h2d(e, h.sigma, tp)) || (rc = h2d(e, h.accept, tv)) || (rc = h2d(e, h.hmc, tc))) return rc;
    }
    if ((rc = h2d(e, h.m, m)) || (rc = h2d(e, h.flags, fl))) return rc;
    off += h.tune_len;
  }
  return 0;
}
