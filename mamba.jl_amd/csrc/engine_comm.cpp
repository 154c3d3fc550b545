// engine_comm.cpp — the one collective of the path: Gelman-Rubin sums across GPUs over RCCL.
#include "engine.h"

#include <rccl/rccl.h>

// ---------------------------------------------------------------- cross-GPU Gelman-Rubin (RCCL)
// The one collective of the path (gelmandiag.jl:11-25): each local engine reduces
// its kept draws to the mmb_gr_len sufficient statistics on device (gr.hip), then one SUM
// all-reduce over RCCL/xGMI, in place in a per-engine device buffer; the global [min, max]
// used for link() and the shift is one MAX all-reduce of (-min, max).
// the agreement slot's value outside an agreement: flag 2 = "this rank could not stage" (comm_agree)
static const double kAgreeFailed[4] = {2.0, 0.0, 0.0, 0.0};

struct mmb_comm {
  std::vector<mmb_engine*> eng;
  std::vector<ncclComm_t> comm;
  std::vector<DevBuf<double>> buf;  // per local engine: [L stats | 2p range | p shift | p link (int32) | 4 agree]
  int p = 0;
  int64_t L = 0;
  double agree[4] = {0.0, 0.0, 0.0, 0.0};  // comm_agree's contribution (outlives its async H2D copies)
};

#define NCCLCHK(e, x)                                                                 \
  do {                                                                                \
    ncclResult_t r_ = (x);                                                            \
    if (r_ != ncclSuccess) return fail((e), MMB_E_COMM, "%s: %s", #x, ncclGetErrorString(r_)); \
  } while (0)

__global__ void mmb_negate_mins(double* mm, int p) {
  const int j = (int)threadIdx.x;
  if (j < p) mm[2 * j] = -mm[2 * j];
}

int mmb_comm_id(uint8_t* id) {
  if (!id) return fail(nullptr, MMB_E_ARG, "null argument");
  ncclUniqueId u;
  NCCLCHK(nullptr, ncclGetUniqueId(&u));
  std::memcpy(id, u.internal, MMB_COMM_ID_BYTES);
  return 0;
}

void mmb_comm_destroy(mmb_comm* c) {
  if (!c) return;
  for (size_t i = 0; i < c->eng.size(); ++i) {
    (void)hipSetDevice(c->eng[i]->device);
    if (c->comm[i]) (void)ncclCommDestroy(c->comm[i]);
    c->buf[i].reset();
  }
  delete c;
}

int mmb_comm_init(mmb_engine** engines, int nlocal, int nranks, int rank0, const uint8_t* id, mmb_comm** out) {
  if (!engines || !out || nlocal < 1) return fail(nullptr, MMB_E_ARG, "null argument or nlocal < 1");
  *out = nullptr;
  mmb_engine* e0 = engines[0];
  if (!e0) return fail(nullptr, MMB_E_ARG, "null engine");
  if (nranks < nlocal || rank0 < 0 || rank0 + nlocal > nranks)
    return fail(e0, MMB_E_ARG, "ranks %d..%d outside 0..%d", rank0, rank0 + nlocal - 1, nranks - 1);
  if (nlocal < nranks && !id) return fail(e0, MMB_E_ARG, "ranks span processes: pass the mmb_comm_id bytes of rank 0");
  for (int i = 0; i < nlocal; ++i) {
    if (!engines[i]) return fail(e0, MMB_E_ARG, "null engine %d", i);
    if (engines[i]->pmon != e0->pmon) return fail(e0, MMB_E_ARG, "engines monitor different parameter counts");
    for (int k = 0; k < i; ++k)
      if (engines[k]->device == engines[i]->device) return fail(e0, MMB_E_ARG, "two local engines on device %d", engines[i]->device);
  }
  mmb_comm* c = new mmb_comm;
  c->eng.assign(engines, engines + nlocal);
  c->comm.assign(nlocal, nullptr);
  c->buf.resize(nlocal);
  c->p = e0->pmon;
  c->L = mmb_gr_len(e0);
  const size_t nbuf = (size_t)c->L + 4 * (size_t)c->p + 4;
  for (int i = 0; i < nlocal; ++i) {
    // the agreement slot starts (and is left after every agreement) holding the failure flag, so
    // a rank that cannot stage its contribution still contributes "failed" (comm_agree)
    if (hipSetDevice(engines[i]->device) != hipSuccess || c->buf[i].alloc(nbuf) != hipSuccess ||
        hipMemcpy(c->buf[i] + (nbuf - 4), kAgreeFailed, sizeof kAgreeFailed, hipMemcpyHostToDevice) != hipSuccess) {
      mmb_comm_destroy(c);
      return fail(e0, MMB_E_HIP, "comm buffer allocation failed");
    }
  }
  ncclResult_t r;
  if (nlocal == nranks && !id) {
    std::vector<int> devs(nlocal);
    for (int i = 0; i < nlocal; ++i) devs[i] = engines[i]->device;
    r = ncclCommInitAll(c->comm.data(), nlocal, devs.data());
  } else {
    ncclUniqueId u;
    std::memcpy(u.internal, id, MMB_COMM_ID_BYTES);
    r = ncclGroupStart();
    for (int i = 0; r == ncclSuccess && i < nlocal; ++i) {
      (void)hipSetDevice(engines[i]->device);
      r = ncclCommInitRank(&c->comm[i], nranks, u, rank0 + i);
    }
    ncclResult_t r2 = ncclGroupEnd();
    if (r == ncclSuccess) r = r2;
  }
  if (r != ncclSuccess) {
    mmb_comm_destroy(c);
    return fail(e0, MMB_E_COMM, "RCCL communicator init (%d local of %d ranks): %s", nlocal, nranks,
                ncclGetErrorString(r));
  }
  *out = c;
  return 0;
}

static int comm_sync(mmb_comm* c) {
  for (mmb_engine* e : c->eng) {
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  return 0;
}

// One in-place all-reduce of n doubles at offset off of every local engine's buffer, grouped.
// ncclGroupEnd is called whatever happens inside the group, so a failed call never leaves the
// thread's RCCL group open for later collectives.
static ncclResult_t grouped_allreduce(mmb_comm* c, size_t off, size_t n, ncclRedOp_t op) {
  ncclResult_t r = ncclGroupStart();
  if (r != ncclSuccess) return r;
  for (size_t i = 0; r == ncclSuccess && i < c->eng.size(); ++i)
    r = ncclAllReduce(c->buf[i] + off, c->buf[i] + off, n, ncclDouble, op, c->comm[i], c->eng[i]->stream);
  const ncclResult_t r2 = ncclGroupEnd();
  return r != ncclSuccess ? r : r2;
}

// Agreement step before a data collective.  Every local engine contributes (flag, -n_kept,
// n_kept) to one MAX all-reduce, where flag = 1 if this process cannot take part (too few kept
// draws on some local engine) and 2 if it could not even stage its contribution: the slot holds
// 2 outside an agreement (set at comm init and re-armed after every readback), so an engine whose
// staging copy fails contributes the failure flag, never a stale "agree" of an earlier call.  A process whose precondition fails therefore still enters the
// collective, and every rank sees the same verdict: all fail together (MMB_E_STATE for too few
// draws, MMB_E_ARG when the ranks kept different numbers of draws, which would otherwise give
// a silently wrong PSRF) or all proceed with the common n_kept.
// A local HIP failure while staging the contribution does not skip the collective (the peers
// are already waiting in it): the process always joins the all-reduce and the sync, and reports
// its error afterwards (as mmb_gr_allreduce does for launch failures).
static int comm_agree(mmb_comm* c, int64_t need, int64_t* nkept) {
  mmb_engine* e0 = c->eng[0];
  const size_t off = (size_t)c->L + 4 * (size_t)c->p;
  int64_t lo = INT64_MAX, hi = -1;
  for (mmb_engine* e : c->eng) { lo = std::min(lo, e->n_kept); hi = std::max(hi, e->n_kept); }
  c->agree[0] = lo < need ? 1.0 : 0.0;
  c->agree[1] = -(double)lo;
  c->agree[2] = (double)hi;
  c->agree[3] = 0.0;
  int lrc = 0;
  // MMB_TEST_COMM_STAGE_FAIL=1 (tests only): skip the staging copy as if it had failed
  const char* tf = std::getenv("MMB_TEST_COMM_STAGE_FAIL");
  const bool inject = tf && std::atoi(tf) == 1;
  for (size_t i = 0; i < c->eng.size(); ++i) {
    hipError_t st = hipSetDevice(c->eng[i]->device);
    if (st == hipSuccess && inject) st = hipErrorUnknown;
    if (st == hipSuccess)
      st = hipMemcpyAsync(c->buf[i] + off, c->agree, sizeof(c->agree), hipMemcpyHostToDevice, c->eng[i]->stream);
    if (st != hipSuccess && !lrc) lrc = fail(e0, MMB_E_HIP, "agreement staging: %s", hipGetErrorString(st));
  }
  const ncclResult_t r = grouped_allreduce(c, off, 4, ncclMax);
  double all[4] = {2.0, 0.0, 0.0, 0.0};
  hipError_t st = hipSetDevice(e0->device);
  if (st == hipSuccess) st = hipMemcpyAsync(all, c->buf[0] + off, sizeof(all), hipMemcpyDeviceToHost, e0->stream);
  for (size_t i = 0; i < c->eng.size(); ++i)  // re-arm: the slot holds the failure flag again
    if (hipSetDevice(c->eng[i]->device) == hipSuccess)
      (void)hipMemcpyAsync(c->buf[i] + off, kAgreeFailed, sizeof kAgreeFailed, hipMemcpyHostToDevice, c->eng[i]->stream);
  const int rc = comm_sync(c);
  if (r != ncclSuccess) return fail(e0, MMB_E_COMM, "agreement all-reduce: %s", ncclGetErrorString(r));
  if (lrc)
    return fail(e0, MMB_E_HIP, "%s (the agreement all-reduce saw flag %.0f: every rank fails this collective)",
                g_last_error.c_str(), all[0]);
  if (st != hipSuccess) return fail(e0, MMB_E_HIP, "agreement readback: %s", hipGetErrorString(st));
  if (rc) return rc;
  if (all[0] >= 2.0)
    return fail(e0, MMB_E_COMM, "another rank could not stage its agreement contribution; collective skipped");
  if (all[0] != 0.0)
    return fail(e0, MMB_E_STATE, "need >= %lld device-kept draws per chain on every rank (this process: %lld)",
                (long long)need, (long long)lo);
  if (-all[1] != all[2])
    return fail(e0, MMB_E_ARG, "ranks kept different numbers of draws (%.0f .. %.0f)", -all[1], all[2]);
  *nkept = (int64_t)all[2];
  return 0;
}

int mmb_range_allreduce(mmb_comm* c, double* minmax) {
  if (!c || !minmax) return fail(nullptr, MMB_E_ARG, "null argument");
  mmb_engine* e0 = c->eng[0];
  const int p = c->p;
  int64_t nk = 0;
  int rc = comm_agree(c, 1, &nk);
  if (rc) return rc;
  for (size_t i = 0; i < c->eng.size(); ++i) {
    mmb_engine* e = c->eng[i];
    HIPCHK(e0, hipSetDevice(e->device));
    double* mm = c->buf[i] + c->L;
    hipError_t st = mmb_launch_gr_range(p, nk, (int)e->K, e->d_draws, mm, e->stream);
    if (st == hipSuccess) {
      hipLaunchKernelGGL(mmb_negate_mins, dim3(1), dim3(((p + 63) / 64) * 64), 0, e->stream, mm, p);
      st = hipGetLastError();
    }
    // a local launch failure after the agreement still joins the all-reduce below (its peers
    // are already committed to it); the error is reported afterwards
    if (st != hipSuccess) rc = fail(e0, MMB_E_HIP, "gr_range: %s", hipGetErrorString(st));
  }
  const ncclResult_t r = grouped_allreduce(c, (size_t)c->L, 2 * (size_t)p, ncclMax);
  if (r != ncclSuccess) return fail(e0, MMB_E_COMM, "range all-reduce: %s", ncclGetErrorString(r));
  if (rc) return rc;
  HIPCHK(e0, hipSetDevice(e0->device));
  HIPCHK(e0, hipMemcpyAsync(minmax, c->buf[0] + c->L, 2 * p * sizeof(double), hipMemcpyDeviceToHost, e0->stream));
  rc = comm_sync(c);
  if (rc) return rc;
  for (int j = 0; j < p; ++j) minmax[2 * j] = -minmax[2 * j];
  return 0;
}

int mmb_gr_allreduce(mmb_comm* c, const int32_t* link, const double* shift, double* out) {
  if (!c || !link || !shift || !out) return fail(nullptr, MMB_E_ARG, "null argument");
  mmb_engine* e0 = c->eng[0];
  const int p = c->p;
  // every rank holds the same model, so all refuse alike before any collective
  if (int wrc = gr_width_check(e0)) return wrc;
  int64_t nk = 0;
  int rc = comm_agree(c, 2, &nk);
  if (rc) return rc;
  for (size_t i = 0; i < c->eng.size(); ++i) {
    mmb_engine* e = c->eng[i];
    HIPCHK(e0, hipSetDevice(e->device));
    double* ds = c->buf[i] + c->L + 2 * p;
    int32_t* dl = (int32_t*)(ds + p);
    hipError_t st = hipMemcpyAsync(ds, shift, p * sizeof(double), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(dl, link, p * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = mmb_launch_gr_stats(p, nk, (int)e->K, e->d_draws, dl, ds, c->buf[i], e->stream);
    if (st != hipSuccess) rc = fail(e0, MMB_E_HIP, "gr_stats: %s", hipGetErrorString(st));
  }
  const ncclResult_t r = grouped_allreduce(c, 0, (size_t)c->L, ncclSum);
  if (r != ncclSuccess) return fail(e0, MMB_E_COMM, "Gelman-Rubin all-reduce: %s", ncclGetErrorString(r));
  if (rc) { (void)comm_sync(c); return rc; }
  HIPCHK(e0, hipSetDevice(e0->device));
  HIPCHK(e0, hipMemcpyAsync(out, c->buf[0], c->L * sizeof(double), hipMemcpyDeviceToHost, e0->stream));
  // the host copies of link/shift must outlive the async H2D copies: wait before returning
  return comm_sync(c);
}
