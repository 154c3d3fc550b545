// engine_post.cpp — everything computed on the device-kept draws: Gelman-Rubin partials, summaries and
// order statistics, hpd, model statistics, posterior prediction and the per-chain diagnostics.
#include "engine.h"
#include "predict_math.h"

// ---------------------------------------------------------------- Gelman-Rubin partials
int64_t mmb_gr_len(const mmb_engine* e) {
  if (!e) return MMB_E_ARG;
  const int64_t p = e->pmon;
  return 1 + p + p * p + p * p + 3 * p;
}

int mmb_gr_range(mmb_engine* e, double* minmax) {
  if (!e || !minmax) return fail(e, MMB_E_ARG, "null argument");
  if (e->n_kept < 1) return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  HIPCHK(e, hipSetDevice(e->device));
  DevBuf<double> d;
  HIPCHK(e, d.alloc(2 * e->pmon));
  hipError_t st = mmb_launch_gr_range(e->pmon, e->n_kept, (int)e->K, e->d_draws, d, e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "gr_range: %s", hipGetErrorString(st));
  HIPCHK(e, hipMemcpyAsync(minmax, d, 2 * e->pmon * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

// gr.hip holds a chain's p x p covariance in thread-owned pairs: p <= mmb_gr_pmax()
int gr_width_check(mmb_engine* e) {
  if (e->pmon > mmb_gr_pmax())
    return fail(e, MMB_E_UNSUPPORTED, "Gelman-Rubin sums (gelmandiag, cor) serve at most %d monitored values; "
                "this model monitors %d", mmb_gr_pmax(), e->pmon);
  return 0;
}

int mmb_gr_partials(mmb_engine* e, const int32_t* link, const double* shift, double* out) {
  if (!e || !link || !shift || !out) return fail(e, MMB_E_ARG, "null argument");
  if (int rc = gr_width_check(e)) return rc;
  if (e->n_kept < 2) return fail(e, MMB_E_STATE, "need >= 2 device-kept draws per chain");
  HIPCHK(e, hipSetDevice(e->device));
  const int p = e->pmon;
  const int64_t L = mmb_gr_len(e);
  DevBuf<int32_t> dl;
  DevBuf<double> ds, dout;
  HIPCHK(e, dl.alloc(p));
  HIPCHK(e, ds.alloc(p));
  HIPCHK(e, dout.alloc(L));
  HIPCHK(e, hipMemcpyAsync(dl, link, p * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(ds, shift, p * sizeof(double), hipMemcpyHostToDevice, e->stream));
  hipError_t st = mmb_launch_gr_stats(p, e->n_kept, (int)e->K, e->d_draws, dl, ds, dout, e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "gr_stats: %s", hipGetErrorString(st));
  HIPCHK(e, hipMemcpyAsync(out, dout, L * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

// ---------------------------------------------------------------- posterior summaries
int mmb_chain_summary(mmb_engine* e, const double* shift, int64_t batch_size, int64_t chain_base, double* out) {
  if (!e || !shift || !out) return fail(e, MMB_E_ARG, "null argument");
  if (batch_size < 1) return fail(e, MMB_E_ARG, "batch size must be positive");
  if (chain_base < 0) return fail(e, MMB_E_ARG, "chain_base must be >= 0");
  if (e->n_kept < 1) return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  HIPCHK(e, hipSetDevice(e->device));
  const int p = e->pmon;
  const size_t nout = (size_t)e->K * p * MMB_SUMMARY_FIELDS;
  DevBuf<double> ds, dout;
  HIPCHK(e, ds.alloc(p));
  HIPCHK(e, dout.alloc(nout));
  HIPCHK(e, hipMemcpyAsync(ds, shift, p * sizeof(double), hipMemcpyHostToDevice, e->stream));
  hipError_t st = mmb_launch_chain_summary(p, e->n_kept, (int)e->K, chain_base, batch_size, e->d_draws, ds,
                                           dout, e->stream);
  if (st == hipSuccess) st = hipMemcpyAsync(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "chain_summary: %s", hipGetErrorString(st));
  return 0;
}

int mmb_order_hist(mmb_engine* e, int param, int ntargets, const uint64_t* prefix, int pass, uint64_t* counts) {
  if (!e || !prefix || !counts) return fail(e, MMB_E_ARG, "null argument");
  if (param < 0 || param >= e->pmon) return fail(e, MMB_E_ARG, "param %d out of range", param);
  if (ntargets < 1 || ntargets > MMB_ORDER_MAX_TARGETS) return fail(e, MMB_E_ARG, "1 <= ntargets <= %d",
                                                                      MMB_ORDER_MAX_TARGETS);
  if (pass < 0 || pass > 7) return fail(e, MMB_E_ARG, "pass must be 0..7");
  if (e->n_kept < 1) return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  HIPCHK(e, hipSetDevice(e->device));
  DevBuf<uint64_t> dp;
  DevBuf<unsigned long long> dc;
  HIPCHK(e, dp.alloc(ntargets));
  HIPCHK(e, dc.alloc((size_t)ntargets * 256));
  hipError_t st = hipMemcpyAsync(dp, prefix, ntargets * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream);
  if (st == hipSuccess)
    st = mmb_launch_order_hist(e->pmon, param, e->n_kept, (int)e->K, e->d_draws, ntargets, dp, pass, dc, e->stream);
  if (st == hipSuccess)
    st = hipMemcpyAsync(counts, dc, (size_t)ntargets * 256 * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "order_hist: %s", hipGetErrorString(st));
  return 0;
}

// ---------------------------------------------------------------- hpd (stats.jl:54-74)
// hpd_words: the collect pass's counts and key bits, the sort's digit totals, the gap's partials and result
constexpr int HPD_W_META = 0, HPD_W_GHIST = 8, HPD_W_PARTD = 264, HPD_W_PARTI = 520, HPD_W_RES = 776,
              HPD_WORDS = 784;
constexpr int64_t HPD_MAX_KEYS = 0xffffffffll;  // the sort's scatter offsets are 32-bit

// room for `cap` keys in each tail and in the sort buffer; growing drops the tails held
static int hpd_reserve(mmb_engine* e, int64_t cap) {
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->hpd_words) HIPCHK(e, e->hpd_words.alloc(HPD_WORDS));
  if (cap <= e->hpd_cap) return 0;
  HIPCHK(e, hipStreamSynchronize(e->stream));  // the old buffers may still be read by a kernel
  e->hpd_cap = 0;
  e->hpd_have = false;
  // every old buffer goes before a new one is allocated
  e->hpd_below.reset(), e->hpd_above.reset(), e->hpd_tmp.reset(), e->hpd_tilehist.reset();
  hipError_t st = e->hpd_below.alloc((size_t)cap);
  if (st == hipSuccess) st = e->hpd_above.alloc((size_t)cap);
  if (st == hipSuccess) st = e->hpd_tmp.alloc((size_t)cap);
  if (st == hipSuccess) st = e->hpd_tilehist.alloc((size_t)256 * mmb_hpd_tiles(cap));
  if (st != hipSuccess)
    return fail(e, st == hipErrorOutOfMemory ? MMB_E_NOMEM : MMB_E_HIP, "hpd buffers for %lld values: %s",
                (long long)cap, hipGetErrorString(st));
  e->hpd_cap = cap;
  return 0;
}

int mmb_hpd_collect(mmb_engine* e, int param, double lo, double hi, int64_t cap, int64_t counts[2]) {
  if (!e || !counts) return fail(e, MMB_E_ARG, "null argument");
  if (param < 0 || param >= e->pmon) return fail(e, MMB_E_ARG, "param %d out of range", param);
  if (cap < 0 || cap > HPD_MAX_KEYS) return fail(e, MMB_E_ARG, "cap must be 0 .. %lld", (long long)HPD_MAX_KEYS);
  if (lo != lo || hi != hi) return fail(e, MMB_E_ARG, "a threshold is NaN");
  if (e->n_kept < 1) return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  e->hpd_have = e->hpd_sorted = false;
  if (int rc = hpd_reserve(e, cap)) return rc;
  unsigned long long* meta = e->hpd_words + HPD_W_META;
  unsigned long long h[6] = {};
  hipError_t st = mmb_launch_hpd_collect(e->pmon, param, e->n_kept, (int)e->K, e->d_draws, lo, hi, cap, e->hpd_below,
                                         e->hpd_above, meta, e->stream);
  if (st == hipSuccess) st = hipMemcpyAsync(h, meta, sizeof h, hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "hpd_collect: %s", hipGetErrorString(st));
  counts[0] = (int64_t)h[0];
  counts[1] = (int64_t)h[1];
  if (counts[0] > cap || counts[1] > cap)
    return fail(e, MMB_E_ARG, "hpd_collect: %lld draws below lo and %lld above hi, room for %lld each (lo and hi "
                "must be the order statistics m - 1 and N - m, cap = m - 1)", (long long)counts[0],
                (long long)counts[1], (long long)cap);
  for (int b = 0; b < 2; ++b) {
    e->hpd_n[b] = counts[b];
    e->hpd_varying[b] = counts[b] > 0 ? (uint64_t)(h[2 + 2 * b] ^ h[3 + 2 * b]) : 0;
  }
  e->hpd_have = true;
  return 0;
}

int mmb_hpd_get_tails(mmb_engine* e, double* below, int64_t nbelow, double* above, int64_t nabove) {
  if (!e || (nbelow > 0 && !below) || (nabove > 0 && !above)) return fail(e, MMB_E_ARG, "null argument");
  if (nbelow < 0 || nabove < 0) return fail(e, MMB_E_ARG, "counts must be >= 0");
  if (nbelow > e->hpd_cap || nabove > e->hpd_cap)
    return fail(e, MMB_E_ARG, "counts %lld, %lld exceed the tail buffers' %lld", (long long)nbelow, (long long)nabove,
                (long long)e->hpd_cap);
  if (nbelow + nabove == 0) return 0;
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<uint64_t> kb((size_t)nbelow), ka((size_t)nabove);
  hipError_t st = hipSuccess;
  if (nbelow > 0)
    st = hipMemcpyAsync(kb.data(), e->hpd_below, kb.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess && nabove > 0)
    st = hipMemcpyAsync(ka.data(), e->hpd_above, ka.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "hpd_get_tails: %s", hipGetErrorString(st));
  for (int64_t i = 0; i < nbelow; ++i) below[i] = mmb_hpd_unkey(kb[(size_t)i]);
  for (int64_t i = 0; i < nabove; ++i) above[i] = mmb_hpd_unkey(ka[(size_t)i]);
  return 0;
}

int mmb_hpd_set_tails(mmb_engine* e, const double* below, int64_t nbelow, const double* above, int64_t nabove) {
  if (!e || (nbelow > 0 && !below) || (nabove > 0 && !above)) return fail(e, MMB_E_ARG, "null argument");
  if (nbelow < 0 || nabove < 0) return fail(e, MMB_E_ARG, "counts must be >= 0");
  if (nbelow > HPD_MAX_KEYS || nabove > HPD_MAX_KEYS)
    return fail(e, MMB_E_ARG, "at most %lld values per tail", (long long)HPD_MAX_KEYS);
  e->hpd_have = e->hpd_sorted = false;
  if (int rc = hpd_reserve(e, std::max(nbelow, nabove))) return rc;
  const double* src[2] = {below, above};
  const int64_t cnt[2] = {nbelow, nabove};
  uint64_t* dst[2] = {e->hpd_below, e->hpd_above};
  std::vector<uint64_t> keys[2];
  hipError_t st = hipSuccess;
  for (int b = 0; b < 2 && st == hipSuccess; ++b) {
    keys[b].resize((size_t)cnt[b]);
    uint64_t bor = 0, band = ~0ull;
    for (int64_t i = 0; i < cnt[b]; ++i) {
      const uint64_t k = mmb_hpd_key(src[b][i]);
      keys[b][(size_t)i] = k;
      bor |= k;
      band &= k;
    }
    e->hpd_varying[b] = cnt[b] > 0 ? bor ^ band : 0;
    if (cnt[b] > 0)
      st = hipMemcpyAsync(dst[b], keys[b].data(), keys[b].size() * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream);
  }
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);  // the host copies go out of scope
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "hpd_set_tails: %s", hipGetErrorString(st));
  e->hpd_n[0] = nbelow;
  e->hpd_n[1] = nabove;
  e->hpd_have = true;
  return 0;
}

int mmb_hpd_gap(mmb_engine* e, int64_t m, int64_t total, double lo, double hi, double out[2], int64_t* index) {
  if (!e || !out || !index) return fail(e, MMB_E_ARG, "null argument");
  if (m < 1 || m > total) return fail(e, MMB_E_ARG, "need 1 <= m <= total, got m = %lld, total = %lld", (long long)m,
                                      (long long)total);
  if (lo != lo || hi != hi) return fail(e, MMB_E_ARG, "a threshold is NaN");
  if (lo > hi && m <= total - m)
    return fail(e, MMB_E_ARG, "lo = %g > hi = %g although the tails do not overlap (2 m <= total)", lo, hi);
  if (!e->hpd_have) return fail(e, MMB_E_STATE, "no tails: call mmb_hpd_collect or mmb_hpd_set_tails first");
  if (e->hpd_n[0] > m - 1 || e->hpd_n[1] > m - 1)
    return fail(e, MMB_E_ARG, "the tails hold %lld and %lld values, more than m - 1 = %lld", (long long)e->hpd_n[0],
                (long long)e->hpd_n[1], (long long)(m - 1));
  HIPCHK(e, hipSetDevice(e->device));
  hipError_t st = hipSuccess;
  if (!e->hpd_sorted) {
    DevBuf<uint64_t>* buf[2] = {&e->hpd_below, &e->hpd_above};
    for (int b = 0; b < 2 && st == hipSuccess; ++b) {
      int in_tmp = 0;
      st = mmb_launch_hpd_sort(*buf[b], e->hpd_tmp, e->hpd_n[b], e->hpd_varying[b], e->hpd_tilehist,
                               e->hpd_words + HPD_W_GHIST, &in_tmp, e->stream);
      if (st == hipSuccess && in_tmp) std::swap(*buf[b], e->hpd_tmp);  // equal capacities: the buffers trade places
    }
    if (st != hipSuccess) {
      e->hpd_have = false;  // a buffer may be half sorted
      return fail(e, MMB_E_HIP, "hpd sort: %s", hipGetErrorString(st));
    }
    e->hpd_sorted = true;
  }
  unsigned long long h[3] = {};
  double* res = (double*)(e->hpd_words + HPD_W_RES);
  st = mmb_launch_hpd_gap(e->hpd_below, e->hpd_n[0], e->hpd_above, e->hpd_n[1], m, lo, hi,
                          (double*)(e->hpd_words + HPD_W_PARTD), (long long*)(e->hpd_words + HPD_W_PARTI), res,
                          e->stream);
  if (st == hipSuccess) st = hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "hpd_gap: %s", hipGetErrorString(st));
  memcpy(out, h, 2 * sizeof(double));
  *index = (int64_t)h[2];
  return 0;
}

// ---------------------------------------------------------------- model statistics (modelstats.jl)
// The plan of a node list: validated ids and, for node-IR models, the monitored columns to load and the
// state slots they fill.  getsimkeys (modelstats.jl:107-132) relists the sampled nodes the requested nodes
// depend on through Logicals; here that is the read set of their parameter expressions (Logicals are
// inlined): the VAL / VALI / VALG words over every element, VALG through the gather indices in the pool.
struct MsPlan {
  std::vector<int32_t> col, slot;
};

static int ms_plan(mmb_engine* e, int nnodes, const int32_t* nodes, bool need_draws, MsPlan& pl,
                   const char* what = "logpdf") {
  if (e->model == MMB_MODEL_RATS)
    return fail(e, MMB_E_UNSUPPORTED, "%s: the hand-lowered rats model monitors 3 of its 65 values (s2_c, mu_beta, "
                "alpha0): alpha and beta are not in the chains, so the nodes cannot be relisted from the draws "
                "(use the node-IR rats model with alpha, beta and the hyper-parameters monitored)", what);
  if (e->model == MMB_MODEL_LOGISTIC)
    return fail(e, MMB_E_UNSUPPORTED, "%s: the logistic model evaluates its likelihood through its own batched "
                "engine; its model statistics are not lowered yet", what);
  if (!e->d_vals || (need_draws && e->n_kept < 1))
    return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  if (nnodes < 1 || nnodes > MMB_IR_MAX_TERMS) return fail(e, MMB_E_ARG, "1 <= nnodes <= %d", MMB_IR_MAX_TERMS);
  if (e->model == MMB_MODEL_LINE) {
    for (int a = 0; a < nnodes; ++a)
      if (nodes[a] < 0 || nodes[a] > MMB_LINE_Y)
        return fail(e, MMB_E_ARG, "node id %d is not a Stochastic node of the line model", nodes[a]);
    return 0;
  }
  const int NN = (int)e->ir_nodes.size();
  std::vector<int> colstart(NN, -1);  // first monitored column of a node, -1: not monitored
  int c0 = 0;
  for (int32_t nid : e->ir_mon) {
    colstart[nid] = c0;
    c0 += e->ir_nodes[nid].len;
  }
  auto sampled = [&](const mmb_ir_node& N) { return !N.fixed && N.family != MMB_IR_LOGICAL; };
  std::vector<char> need(NN, 0);
  for (int a = 0; a < nnodes; ++a) {
    const int nid = nodes[a];
    if (nid < 0 || nid >= NN || e->ir_nodes[nid].family == MMB_IR_LOGICAL)
      return fail(e, MMB_E_ARG, "node id %d is not a Stochastic node of the model", nid);
    const mmb_ir_node& N = e->ir_nodes[nid];
    if (sampled(N)) need[nid] = 1;
    std::vector<int> slots;
    if (const int po = mmb_ir_cat_state(N.family, N.cterm); po >= 0)  // Categorical(P) reads P's slots
      for (int i = 0; i < (int)N.hi; ++i) slots.push_back(po + i);
    for (int k = 0; k < 3; ++k) {
      if (N.expr[k] < 0) continue;
      const int ne = (N.family == MMB_IR_ISONORMAL && k == 1) ? 1 : N.len;
      for (int i = 0; i < ne; ++i) ir_expr_slots(e->ir_code, e->ir_pool, N.expr[k], i, slots);
    }
    for (int s : slots) {
      int owner = -1;
      for (int q = 0; q < NN; ++q) {
        const mmb_ir_node& Q = e->ir_nodes[q];
        if (sampled(Q) && s >= Q.off && s < Q.off + Q.len) owner = q;
      }
      if (owner < 0) return fail(e, MMB_E_ARG, "node id %d reads value slot %d, which no sampled node owns", nid, s);
      need[owner] = 1;
    }
  }
  for (int q = 0; q < NN; ++q)
    if (need[q] && colstart[q] < 0)
      return fail(e, MMB_E_ARG, "node id %d is not monitored: the requested nodes need its draws", q);
  for (int q = 0; q < NN; ++q) {
    if (!need[q]) continue;
    const mmb_ir_node& Q = e->ir_nodes[q];
    for (int i = 0; i < Q.len; ++i) {
      pl.col.push_back(colstart[q] + i);
      pl.slot.push_back(Q.off + i);
    }
  }
  return 0;
}

// lp of the n x K rows of `draws` into d_lp ([n][K], device), rows [r0, r0 + rows)
static hipError_t ms_launch(mmb_engine* e, const SweepArgs& A, const MsPlan& pl, const int32_t* d_col,
                            const int32_t* d_slot, int64_t rows, int K, const double* draws, int nnodes,
                            const int32_t* nodes, double* d_lp) {
  return mmb_launch_modelstats(e->model, A, e->P, e->ir_stack, rows, K, e->pmon, draws, nnodes, nodes, d_col, d_slot,
                               (int)pl.col.size(), d_lp, e->stream);
}

// rows of the device lp scratch per pass: the n x K values are formed (and, for the deviance, reduced) in
// chunks of at most this many doubles
constexpr int64_t MS_CHUNK = 8ll << 20;

// shared body: out_lp (host, Chains order out[i + n*k]) and / or acc (host, K x 2 deviance sums with `shift`)
static int ms_run(mmb_engine* e, const char* what, int nnodes, const int32_t* nodes, int64_t n, int K,
                  const double* draws, double* out_lp, double shift, double* acc) {
  MsPlan pl;
  if (int rc = ms_plan(e, nnodes, nodes, true, pl)) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  SweepArgs A;
  fill_args(e, A);
  const int64_t crows = std::max<int64_t>(1, std::min<int64_t>(n, MS_CHUNK / K));
  DevBuf<int32_t> d_tab;
  DevBuf<double> d_lp, d_acc;
  const size_t nc = pl.col.size();
  hipError_t st = hipSuccess;
  if (nc) {
    st = d_tab.alloc(2 * nc);
    if (st == hipSuccess)
      st = hipMemcpyAsync(d_tab, pl.col.data(), nc * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess)
      st = hipMemcpyAsync(d_tab + nc, pl.slot.data(), nc * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
  }
  if (st == hipSuccess) st = d_lp.alloc((size_t)crows * K);
  if (st == hipSuccess && acc) {
    st = d_acc.alloc((size_t)2 * K);
    if (st == hipSuccess) st = hipMemsetAsync(d_acc, 0, (size_t)2 * K * sizeof(double), e->stream);
  }
  std::vector<double> h;
  if (out_lp) h.resize((size_t)crows * K);
  for (int64_t r0 = 0; r0 < n && st == hipSuccess; r0 += crows) {
    const int64_t rows = std::min(crows, n - r0);
    st = ms_launch(e, A, pl, d_tab, d_tab ? d_tab + nc : nullptr, rows, K,
                   draws + (size_t)r0 * e->pmon * K, nnodes, nodes, d_lp);
    if (st == hipSuccess && acc) st = mmb_launch_deviance(rows, K, d_lp, shift, d_acc, e->stream);
    if (st == hipSuccess && out_lp) {
      st = hipMemcpyAsync(h.data(), d_lp, (size_t)rows * K * sizeof(double), hipMemcpyDeviceToHost, e->stream);
      if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
      if (st == hipSuccess)
        for (int64_t i = 0; i < rows; ++i)
          for (int64_t k = 0; k < K; ++k) out_lp[(r0 + i) + n * k] = h[(size_t)i * K + k];
    }
  }
  if (st == hipSuccess && acc)
    st = hipMemcpyAsync(acc, d_acc, (size_t)2 * K * sizeof(double), hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "%s: %s", what, hipGetErrorString(st));
  return 0;
}

int mmb_draws_logpdf(mmb_engine* e, int nnodes, const int32_t* nodes, double* out) {
  if (!e || !nodes || !out) return fail(e, MMB_E_ARG, "null argument");
  return ms_run(e, "draws_logpdf", nnodes, nodes, e->n_kept, (int)e->K, e->d_draws, out, 0.0, nullptr);
}

int mmb_draws_deviance(mmb_engine* e, int nnodes, const int32_t* nodes, double shift, double* out) {
  if (!e || !nodes || !out) return fail(e, MMB_E_ARG, "null argument");
  return ms_run(e, "draws_deviance", nnodes, nodes, e->n_kept, (int)e->K, e->d_draws, nullptr, shift, out);
}

int mmb_logpdf_at(mmb_engine* e, int nnodes, const int32_t* nodes, const double* x, double* lp) {
  if (!e || !nodes || !x || !lp) return fail(e, MMB_E_ARG, "null argument");
  {  // validated before anything is allocated (ms_run validates again on the same arguments)
    MsPlan pl;
    if (int rc = ms_plan(e, nnodes, nodes, true, pl)) return rc;
  }
  HIPCHK(e, hipSetDevice(e->device));
  DevBuf<double> d_x;  // a one-row, one-chain draw buffer
  HIPCHK(e, d_x.alloc((size_t)e->pmon));
  hipError_t st = hipMemcpyAsync(d_x, x, (size_t)e->pmon * sizeof(double), hipMemcpyHostToDevice, e->stream);
  int rc = 0;
  if (st != hipSuccess) rc = fail(e, MMB_E_HIP, "logpdf_at: %s", hipGetErrorString(st));
  else rc = ms_run(e, "logpdf_at", nnodes, nodes, 1, 1, d_x, lp, 0.0, nullptr);
  (void)hipStreamSynchronize(e->stream);  // (nothing in flight reads d_x when it goes)
  return rc;
}

// ---------------------------------------------------------------- posterior prediction (modelstats.jl:71-102)
// The plan of a predict call: the node list's plan (ms_plan), the first result column of every list
// entry and the result width P.  Everything is validated here, before any launch.
struct PrPlan {
  MsPlan ms;
  std::vector<int32_t> col0;
  int P = 0;
};

static int pr_plan(mmb_engine* e, int nnodes, const int32_t* nodes, PrPlan& pl) {
  if (int rc = ms_plan(e, nnodes, nodes, true, pl.ms, "predict")) return rc;
  if (e->model == MMB_MODEL_LINE) {
    if (nnodes != 1 || nodes[0] != MMB_LINE_Y)
      return fail(e, MMB_E_ARG, "predict: y (MMB_LINE_Y) is the only observed node of the line model");
    pl.col0.assign(1, 0);
    pl.P = 5;
    return 0;
  }
  int64_t P = 0;
  for (int a = 0; a < nnodes; ++a) {
    const mmb_ir_node& N = e->ir_nodes[nodes[a]];
    if (!N.fixed) return fail(e, MMB_E_ARG, "node id %d is not an observed Stochastic node of the model", nodes[a]);
    if (N.family == MMB_IR_CATEGORICAL || N.family == MMB_IR_DISCRETEUNIFORM || N.family == MMB_IR_DIRICHLET)
      return fail(e, MMB_E_UNSUPPORTED, "predict: node id %d: Categorical, DiscreteUniform and Dirichlet variates are "
                  "not lowered", nodes[a]);
    const bool gam = N.family == MMB_IR_GAMMA || N.family == MMB_IR_INVGAMMA || N.family == MMB_IR_BETA;
    if (gam && !mmb_pr_gblock_ok(nodes[a], N.len))
      return fail(e, MMB_E_UNSUPPORTED, "predict: node id %d (length %d) does not fit the element blocks of the "
                  "gamma streams (node id < 4095, 2 * length <= 65536)", nodes[a], N.len);
    pl.col0.push_back((int32_t)P);
    P += N.len;
  }
  int S, RS;
  if (P > MMB_IR_MAX_VALUES * 4 || mmb_predict_tile(e->P, e->ir_stack, (int)P, &S, &RS) == 0)
    return fail(e, MMB_E_UNSUPPORTED, "predict: a tile of 8 chains (%d state values and %lld predicted values each) "
                "does not fit the 64 KiB of LDS: predict fewer nodes per call", e->P, (long long)P);
  pl.P = (int)P;
  return 0;
}

// doubles of the device scratch of predicted values per pass; MMB_PREDICT_CHUNK_ROWS (tests) caps its rows
constexpr int64_t PR_CHUNK = 8ll << 20;

// shared body over the kept rows [i0, i1): out (host, Chains order, (i1 - i0) x P x K) and / or acc (host,
// K x P x 2 sums about `shift`, P values)
static int pr_run(mmb_engine* e, const char* what, int nnodes, const int32_t* nodes, uint64_t seed, int64_t start,
                  int64_t thin, int64_t i0, int64_t i1, double* out, const double* shift, double* acc) {
  PrPlan pl;
  if (int rc = pr_plan(e, nnodes, nodes, pl)) return rc;
  if (thin < 1 || start < 0) return fail(e, MMB_E_ARG, "%s: thin >= 1 and start >= 0", what);
  if (i0 < 0 || i1 <= i0 || i1 > e->n_kept)
    return fail(e, MMB_E_ARG, "window [%lld, %lld) is not inside the %lld kept draws", (long long)i0, (long long)i1,
                (long long)e->n_kept);
  HIPCHK(e, hipSetDevice(e->device));
  SweepArgs A;
  fill_args(e, A);
  const int K = (int)e->K, P = pl.P;
  const int64_t nw = i1 - i0;
  int64_t crows = std::max<int64_t>(1, std::min<int64_t>(nw, PR_CHUNK / ((int64_t)P * K)));
  if (const char* s = std::getenv("MMB_PREDICT_CHUNK_ROWS")) crows = std::max<int64_t>(1, std::min<int64_t>(crows, std::atoll(s)));
  DevBuf<int32_t> d_tab;
  DevBuf<double> d_y, d_acc, d_shift;
  const size_t nc = pl.ms.col.size();
  const size_t nacc = (size_t)2 * K * P;
  hipError_t st = hipSuccess;
  if (nc) {
    st = d_tab.alloc(2 * nc);
    if (st == hipSuccess)
      st = hipMemcpyAsync(d_tab, pl.ms.col.data(), nc * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess)
      st = hipMemcpyAsync(d_tab + nc, pl.ms.slot.data(), nc * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
  }
  if (st == hipSuccess) st = d_y.alloc((size_t)crows * P * K);
  if (st == hipSuccess && acc) {
    st = d_acc.alloc(nacc);
    if (st == hipSuccess) st = hipMemsetAsync(d_acc, 0, nacc * sizeof(double), e->stream);
    if (st == hipSuccess) st = d_shift.alloc((size_t)P);
    if (st == hipSuccess) st = hipMemcpyAsync(d_shift, shift, (size_t)P * sizeof(double), hipMemcpyHostToDevice, e->stream);
  }
  std::vector<double> h;
  if (out) h.resize((size_t)crows * P * K);
  for (int64_t r0 = i0; r0 < i1 && st == hipSuccess; r0 += crows) {
    const int64_t rows = std::min(crows, i1 - r0);
    st = mmb_launch_predict(e->model, A, e->P, e->ir_stack, rows, K, e->pmon, e->d_draws + (size_t)r0 * e->pmon * K,
                            nnodes, nodes, pl.col0.data(), P, d_tab, d_tab ? d_tab + nc : nullptr, (int)nc, seed,
                            start + r0 * thin, thin, d_y, e->stream);
    if (st == hipSuccess && acc) st = mmb_launch_predict_moments(rows, K, P, d_y, d_shift, d_acc, e->stream);
    if (st == hipSuccess && out) {
      st = hipMemcpyAsync(h.data(), d_y, (size_t)rows * P * K * sizeof(double), hipMemcpyDeviceToHost, e->stream);
      if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
      if (st == hipSuccess)
        for (int64_t i = 0; i < rows; ++i)
          for (int64_t j = 0; j < P; ++j)
            for (int64_t k = 0; k < K; ++k) out[(r0 - i0 + i) + nw * (j + (int64_t)P * k)] = h[((size_t)i * P + j) * K + k];
    }
  }
  if (st == hipSuccess && acc) st = hipMemcpyAsync(acc, d_acc, nacc * sizeof(double), hipMemcpyDeviceToHost, e->stream);
  const hipError_t sy = hipStreamSynchronize(e->stream);  // also after a failure: nothing is freed under a kernel
  if (st == hipSuccess) st = sy;
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "%s: %s", what, hipGetErrorString(st));
  return 0;
}

int mmb_predict_width(mmb_engine* e, int nnodes, const int32_t* nodes, int64_t* P) {
  if (!e || !nodes || !P) return fail(e, MMB_E_ARG, "null argument");
  PrPlan pl;
  if (int rc = pr_plan(e, nnodes, nodes, pl)) return rc;
  *P = pl.P;
  return 0;
}

int mmb_draws_predict(mmb_engine* e, int nnodes, const int32_t* nodes, uint64_t seed, int64_t start, int64_t thin,
                      int64_t i0, int64_t i1, double* out) {
  if (!e || !nodes || !out) return fail(e, MMB_E_ARG, "null argument");
  return pr_run(e, "draws_predict", nnodes, nodes, seed, start, thin, i0, i1, out, nullptr, nullptr);
}

int mmb_draws_predict_moments(mmb_engine* e, int nnodes, const int32_t* nodes, uint64_t seed, int64_t start,
                              int64_t thin, const double* shift, double* out) {
  if (!e || !nodes || !shift || !out) return fail(e, MMB_E_ARG, "null argument");
  return pr_run(e, "draws_predict_moments", nnodes, nodes, seed, start, thin, 0, e->n_kept, nullptr, shift, out);
}

// ---------------------------------------------------------------- per-chain diagnostics
static int diag_window(mmb_engine* e, int64_t i0, int64_t i1) {
  if (i0 < 0 || i1 <= i0 || i1 > e->n_kept)
    return fail(e, MMB_E_ARG, "window [%lld, %lld) is not inside the %lld kept draws", (long long)i0, (long long)i1,
                (long long)e->n_kept);
  return 0;
}

// launch (on the engine's stream) into a device buffer of `nout` doubles, copy back
template <class Launch>
static int diag_run(mmb_engine* e, const char* what, size_t nout, double* out, Launch launch) {
  HIPCHK(e, hipSetDevice(e->device));
  DevBuf<double> dout;
  HIPCHK(e, dout.alloc(nout));
  hipError_t st = launch(dout.get());
  if (st == hipSuccess) st = hipMemcpyAsync(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "%s: %s", what, hipGetErrorString(st));
  return 0;
}

int mmb_chain_autocov(mmb_engine* e, int64_t i0, int64_t i1, int nlags, const int64_t* lags, double* out) {
  if (!e || !out || (nlags > 0 && !lags)) return fail(e, MMB_E_ARG, "null argument");
  if (e->n_kept < 1) return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  if (int rc = diag_window(e, i0, i1)) return rc;
  if (nlags < 0 || nlags > MMB_DIAG_MAX_LAGS) return fail(e, MMB_E_ARG, "0 <= nlags <= %d", MMB_DIAG_MAX_LAGS);
  for (int q = 0; q < nlags; ++q)
    if (lags[q] < 1 || lags[q] >= i1 - i0)
      return fail(e, MMB_E_ARG, "lags must be less than the sample length (lag %lld, window of %lld)",
                  (long long)lags[q], (long long)(i1 - i0));
  const int p = e->pmon;
  return diag_run(e, "chain_autocov", (size_t)e->K * p * (2 + nlags), out, [&](double* dout) {
    return mmb_launch_chain_autocov(p, (int)e->K, i0, i1, nlags, lags, e->d_draws, dout, e->stream);
  });
}

// the window and method checks of mmb_chain_mcse
static int mcse_window(mmb_engine* e, int64_t i0, int64_t i1, int etype, int64_t batch_size) {
  if (int rc = diag_window(e, i0, i1)) return rc;
  const int64_t nw = i1 - i0;
  if (etype == MMB_MCSE_BM) {
    if (batch_size < 1) return fail(e, MMB_E_ARG, "batch size must be positive");
    if (nw / batch_size < 2)   // mcse.jl:13-16
      return fail(e, MMB_E_ARG, "iterations are < %lld and batch size is > %lld", (long long)(2 * batch_size),
                  (long long)(nw / 2));
  } else if (etype == MMB_MCSE_IMSE || etype == MMB_MCSE_IPSE) {
    if (nw < 2) return fail(e, MMB_E_ARG, "lags must be less than the sample length (lag 1, window of 1)");
  } else {
    return fail(e, MMB_E_ARG, "unsupported mcse method %d", etype);
  }
  return 0;
}

int mmb_chain_mcse(mmb_engine* e, int64_t i0, int64_t i1, int etype, int64_t batch_size, double* out) {
  if (!e || !out) return fail(e, MMB_E_ARG, "null argument");
  if (e->n_kept < 1) return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  if (int rc = mcse_window(e, i0, i1, etype, batch_size)) return rc;
  const int p = e->pmon;
  return diag_run(e, "chain_mcse", (size_t)e->K * p * MMB_MCSE_FIELDS, out, [&](double* dout) {
    return mmb_launch_chain_mcse(p, (int)e->K, i0, i1, etype, batch_size, e->d_draws, dout, e->stream);
  });
}

// heideldiag.jl:11-16 on every candidate window at once
int mmb_chain_cvm(mmb_engine* e, int nstarts, const int64_t* starts, double* out) {
  if (!e || !out || !starts) return fail(e, MMB_E_ARG, "null argument");
  if (e->n_kept < 1) return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  if (nstarts < 1 || nstarts > MMB_HEIDEL_MAX_STARTS)
    return fail(e, MMB_E_ARG, "1 <= nstarts <= %d", MMB_HEIDEL_MAX_STARTS);
  for (int q = 0; q < nstarts; ++q) {
    if (starts[q] < 0 || starts[q] >= e->n_kept)
      return fail(e, MMB_E_ARG, "start %lld is not inside the %lld kept draws", (long long)starts[q],
                  (long long)e->n_kept);
    if (q > 0 && starts[q] <= starts[q - 1]) return fail(e, MMB_E_ARG, "starts must be strictly increasing");
  }
  const int p = e->pmon;
  return diag_run(e, "chain_cvm", (size_t)e->K * p * nstarts * 2, out, [&](double* dout) {
    return mmb_launch_chain_cvm(p, (int)e->K, e->n_kept, nstarts, starts, e->d_draws, dout, e->stream);
  });
}

// heideldiag.jl:24: mcse of each series' own window
int mmb_chain_mcse_from(mmb_engine* e, const int64_t* i0, int64_t i1, int etype, int64_t batch_size, double* out) {
  if (!e || !out || !i0) return fail(e, MMB_E_ARG, "null argument");
  if (e->n_kept < 1) return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  const int p = e->pmon;
  const size_t nel = (size_t)e->K * p;
  for (size_t q = 0; q < nel; ++q)
    if (int rc = mcse_window(e, i0[q], i1, etype, batch_size)) {
      const std::string why = e->err;
      return fail(e, rc, "%s (chain %lld, param %d)", why.c_str(), (long long)(q / p), (int)(q % p));
    }
  HIPCHK(e, hipSetDevice(e->device));
  DevBuf<int64_t> di;
  HIPCHK(e, di.alloc(nel));
  hipError_t st = hipMemcpyAsync(di, i0, nel * sizeof(int64_t), hipMemcpyHostToDevice, e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "chain_mcse_from: %s", hipGetErrorString(st));
  return diag_run(e, "chain_mcse_from", nel * MMB_MCSE_FIELDS, out, [&](double* dout) {
    return mmb_launch_chain_mcse_from(p, (int)e->K, di, i1, etype, batch_size, e->d_draws, dout, e->stream);
  });
}

// rafterydiag.jl:13-34; the quantile index is Julia 0.5 quantile's, split here
int mmb_chain_raftery(mmb_engine* e, double q, double* out) {
  if (!e || !out) return fail(e, MMB_E_ARG, "null argument");
  if (e->n_kept < 1) return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  if (!(q > 0.0 && q < 1.0)) return fail(e, MMB_E_ARG, "q is not in (0, 1)");
  const int64_t n = e->n_kept;
  if (n < 3 || n > 0x7fffffffll)
    return fail(e, MMB_E_ARG, "the Raftery-Lewis counts need 3 <= kept draws < 2^31, got %lld", (long long)n);
  const double index = 1.0 + (double)(n - 1) * q;
  const double lo = floor(index);
  const double h = index - lo;
  const int interp = index != lo;
  const int64_t rlo = (int64_t)lo - 1;
  if (rlo < 0 || rlo + interp >= n) return fail(e, MMB_E_ARG, "quantile index %g outside 1 .. %lld", index, (long long)n);
  const int p = e->pmon;
  return diag_run(e, "chain_raftery", (size_t)e->K * p * MMB_RAFTERY_FIELDS, out, [&](double* dout) {
    return mmb_launch_chain_raftery(p, (int)e->K, n, rlo, interp, h, e->d_draws, dout, e->stream);
  });
}

int mmb_change_counts(mmb_engine* e, int64_t* out) {
  if (!e || !out) return fail(e, MMB_E_ARG, "null argument");
  if (e->n_kept < 1) return fail(e, MMB_E_STATE, "no device-kept draws (run with keep_device=1)");
  HIPCHK(e, hipSetDevice(e->device));
  const size_t nb = (size_t)(e->pmon + 1) * sizeof(unsigned long long);
  DevBuf<unsigned long long> dc;
  HIPCHK(e, dc.alloc((size_t)e->pmon + 1));
  hipError_t st = mmb_launch_change_counts(e->pmon, (int)e->K, e->n_kept, e->d_draws, dc, e->stream);
  if (st == hipSuccess) st = hipMemcpyAsync(out, dc, nb, hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  if (st != hipSuccess) return fail(e, MMB_E_HIP, "change_counts: %s", hipGetErrorString(st));
  return 0;
}
