"""mcmc() driver, Engine wrapper and Chains container.

Mirrors src/model/mcmc.jl: `mcmc(m, inputs, inits, iters; burnin, thin, chains)`
(mcmc.jl:19-33) and the restart form `mcmc(mc, iters)` (mcmc.jl:3-16).  The chain
fan-out (`pmap2(mcmc_worker!, ...)`, mcmc.jl:52) is one HIP engine per GPU holding a
contiguous shard of global chain ids; draws come back in Mamba's Chains layout
(n x p x chains, src/output/chains.jl:5-11).
"""
import ctypes as C

import numpy as np

from . import abi
from .samplers import ArgumentError


class Engine:
    """One libmambahip engine (one GPU, one shard of chains)."""

    def __init__(self, model, device=0):
        self.lib = abi.lib()
        self.model = model
        self.spec = model.spec()
        h = C.c_void_p()
        if model.kind == abi.MMB_MODEL_IR:  # generic node IR (ir.py)
            self.ir = model.ir()
            rc = self.lib.mmb_create_ir(C.byref(self.spec), C.byref(self.ir), int(device), C.byref(h))
        else:
            rc = self.lib.mmb_create(C.byref(self.spec), int(device), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"mmb_create failed ({abi.ERRORS.get(rc, rc)}): "
                               f"{self.lib.mmb_last_error(None).decode()}")
        self.h = h
        for name, arr in zip(model.input_names, model.data_arrays()):
            self._chk(self.lib.mmb_set_data(self.h, name.encode(), abi.dptr(arr), arr.size))
        self.P = self.lib.mmb_num_values(self.h)
        self.pmon = self.lib.mmb_num_monitored(self.h)
        self.K = 0

    def _chk(self, rc):
        return abi.check(rc, self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.mmb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def init_chains(self, init, chain_offset=0, seed=1):
        init = np.ascontiguousarray(init, dtype=np.float64)
        self.K = init.shape[0]
        self.chain_offset = int(chain_offset)
        self.seed = int(seed)
        self._chk(self.lib.mmb_init_chains(self.h, abi.dptr(init), self.K, int(chain_offset),
                                           C.c_uint64(int(seed))))

    def run(self, iters, burnin=0, thin=1, model_burnin=None, draws=True, keep_device=False,
            time_kernels=False):
        a = abi.RunArgs()
        a.iters, a.burnin, a.thin = int(iters), int(burnin), int(thin)
        a.model_burnin = int(burnin if model_burnin is None else model_burnin)
        a.keep_device = int(keep_device)
        a.time_kernels = int(time_kernels)
        it0 = self.iter
        kept = lambda t: (t - burnin) // thin if t > burnin else 0  # noqa: E731
        nk = kept(it0 + iters) - kept(it0)
        out = None
        if draws and nk > 0:
            out = np.empty((nk, self.pmon, self.K), order="F")
            a.draws = abi.dptr(out)
        self._chk(self.lib.mmb_run(self.h, C.byref(a)))
        return out

    def reserve_draws(self, nkept):
        """Allocate the device draw buffer for windows keeping up to `nkept` iterations now
        (mmb_reserve_draws), so a later run does not allocate inside a timed window."""
        self._chk(self.lib.mmb_reserve_draws(self.h, int(nkept)))

    @property
    def iter(self):
        return self.lib.mmb_iter(self.h)

    def set_iter(self, it):
        self._chk(self.lib.mmb_set_iter(self.h, int(it)))

    def values(self):
        v = np.empty((self.K, self.P))
        self._chk(self.lib.mmb_get_values(self.h, abi.dptr(v)))
        return v

    def set_values(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        self._chk(self.lib.mmb_set_values(self.h, abi.dptr(v)))

    def tune(self):
        n = self.lib.mmb_tune_len(self.h)
        t = np.empty((self.K, max(n, 1)))
        if n > 0:
            self._chk(self.lib.mmb_get_tune(self.h, abi.dptr(t)))
        return t[:, :n]

    def set_tune(self, t):
        t = np.ascontiguousarray(t, dtype=np.float64)
        if t.size:
            self._chk(self.lib.mmb_set_tune(self.h, abi.dptr(t)))

    def num_kept(self):
        return self.lib.mmb_num_kept(self.h)

    def draws(self):
        nk = self.num_kept()
        out = np.empty((nk, self.pmon, self.K), order="F")
        if nk:
            self._chk(self.lib.mmb_get_draws(self.h, abi.dptr(out)))
        return out

    def sync(self):
        self._chk(self.lib.mmb_sync(self.h))

    def kernel_time(self):
        ms = C.c_double()
        n = C.c_int64()
        u = C.c_int64()
        self.lib.mmb_kernel_time(self.h, C.byref(ms), C.byref(n), C.byref(u))
        return ms.value, n.value, u.value

    def grad_evals(self):
        n = C.c_int64()
        self._chk(self.lib.mmb_grad_evals(self.h, C.byref(n)))
        return n.value

    def nuts_stats(self):
        """NUTS tree statistics since init_chains (mmb_nuts_stats): completed updates,
        updates stopped by the depth cap (reference: unbounded), mean final tree depth."""
        v = (C.c_int64 * 3)()
        self._chk(self.lib.mmb_nuts_stats(self.h, v))
        return {"updates": v[0], "depth_cap_hits": v[1], "depth_sum": v[2]}

    def amm_stats(self):
        """AMM factorization counters since init_chains (mmb_amm_stats), one dict per AMM block
        (keyed by block index): adaptive updates (cholfact calls, amm.jl:87), full-rank ones
        (rank(F) == n: SigmaLm replaced, amm.jl:88-90), the rank sum, the factorization steps
        the device executed (per wavefront of two chains on the 32-lane kernels) and the updates
        whose optimistic pass was redone by the checked one."""
        v = (C.c_int64 * (abi.MMB_MAX_BLOCKS * abi.MMB_AMM_STATS))()
        self._chk(self.lib.mmb_amm_stats(self.h, v))
        out = {}
        for b, blk in enumerate(self.model.samplers):
            if getattr(blk, "kind", None) != abi.MMB_SAMPLER_AMM:
                continue
            r = v[b * abi.MMB_AMM_STATS:(b + 1) * abi.MMB_AMM_STATS]
            out[b] = {"updates": r[0], "full_rank": r[1], "rank_sum": r[2], "steps_sum": r[3], "redo": r[4]}
        return out

    def rwm_stats(self):
        """RWM counters since init_chains (mmb_rwm_stats), one dict per RWM block (keyed by block
        index), summed over the chains: block updates and accepted ones (rwm.jl:67-70).  RWM does
        not adapt: size `scale` from this acceptance rate."""
        v = (C.c_int64 * (abi.MMB_MAX_BLOCKS * 2))()
        self._chk(self.lib.mmb_rwm_stats(self.h, v))
        out = {}
        for b, blk in enumerate(self.model.samplers):
            if getattr(blk, "kind", None) != abi.MMB_SAMPLER_RWM:
                continue
            out[b] = {"updates": v[2 * b], "accepts": v[2 * b + 1],
                      "rate": v[2 * b + 1] / v[2 * b] if v[2 * b] else float("nan")}
        return out

    def accept_stats(self):
        """Update and accept counters since init_chains of every block that has a Metropolis accept step
        and counts it (mmb_rwm_stats): RWM, BMG, BMC3, BIA, BHMC and ABC blocks, one dict per block keyed by block
        index, summed over the chains.  A BMG block of one element has no accept step (bmg.jl:83-84):
        every update counts as accepted.  A BHMC block's accepts are the updates that ran to traveltime:
        updates - accepts of them stalled and left the chain as it was.  An ABC block's accepts are the updates
        that took one of their candidates."""
        kinds = (abi.MMB_SAMPLER_RWM, abi.MMB_SAMPLER_BMG, abi.MMB_SAMPLER_BMC3, abi.MMB_SAMPLER_BIA,
                 abi.MMB_SAMPLER_BHMC, abi.MMB_SAMPLER_ABC)
        v = (C.c_int64 * (abi.MMB_MAX_BLOCKS * 2))()
        self._chk(self.lib.mmb_rwm_stats(self.h, v))
        return {b: {"updates": v[2 * b], "accepts": v[2 * b + 1],
                    "rate": v[2 * b + 1] / v[2 * b] if v[2 * b] else float("nan")}
                for b, blk in enumerate(self.model.samplers) if getattr(blk, "kind", None) in kinds}

    def bhmc_stats(self):
        """Per BHMC block (keyed by block index): `wallhits` and `wallcrosses` (BHMCTune, bhmc.jl:10-11), one
        entry per chain, since the chain's particle was drawn; read from the tune rows."""
        t = self.tune()
        out, off = {}, 0
        for b, blk in enumerate(self.model.samplers):
            d = self.model.block_dim(blk)
            if blk.kind == abi.MMB_SAMPLER_BHMC:
                out[b] = {"wallhits": t[:, off + 2 * d].astype(np.int64),
                          "wallcrosses": t[:, off + 2 * d + 1].astype(np.int64)}
            off += blk.tune_len(d)
        return out

    def amwg_stats(self):
        """AMWG block updates since init_chains that ran the sequential coordinate loop
        (mmb_amwg_stats) rather than the lane-parallel decision of every coordinate."""
        v = (C.c_int64 * 1)()
        self._chk(self.lib.mmb_amwg_stats(self.h, v))
        return {"sequential_updates": v[0]}

    def chain_order(self):
        """The lane-group slot -> chain table of the last window (mmb_chain_order): the 32-lane
        kernels pair chains whose AMM factorization stops alike; results do not depend on it."""
        out = np.empty(self.K, dtype=np.int32)
        if self.K:
            self._chk(self.lib.mmb_chain_order(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def ir_jit(self):
        """Node-IR engines: (True, info) when the specialised kernel runs (mmb_create_ir compiled
        the model with hipRTC or found it in the cache), (False, reason) for the interpreter."""
        buf = C.create_string_buffer(4096)
        r = self.lib.mmb_ir_jit_info(self.h, buf, len(buf))
        if r < 0:
            self._chk(r)
        return bool(r), buf.value.decode()

    def state_bytes(self):
        b = C.c_double()
        self.lib.mmb_state_bytes(self.h, C.byref(b))
        return b.value

    # Gelman-Rubin partial sums of the device-kept draws (for the cross-GPU all-reduce)
    def gr_range(self):
        mm = np.empty(2 * self.pmon)
        self._chk(self.lib.mmb_gr_range(self.h, abi.dptr(mm)))
        return mm.reshape(self.pmon, 2)

    def gr_partials(self, link, shift):
        link = np.ascontiguousarray(link, dtype=np.int32)
        shift = np.ascontiguousarray(shift, dtype=np.float64)
        out = np.empty(self.lib.mmb_gr_len(self.h))
        self._chk(self.lib.mmb_gr_partials(self.h, link.ctypes.data_as(C.POINTER(C.c_int32)),
                                           abi.dptr(shift), abi.dptr(out)))
        return out

    # posterior-summary partials of the device-kept draws (summary.py pools them)
    def chain_summary(self, shift, batch_size=100, chain_base=0):
        shift = np.ascontiguousarray(shift, dtype=np.float64)
        out = np.empty((self.K, self.pmon, abi.MMB_SUMMARY_FIELDS))
        self._chk(self.lib.mmb_chain_summary(self.h, abi.dptr(shift), int(batch_size), int(chain_base),
                                             abi.dptr(out)))
        return out

    def order_hist(self, param, prefixes, npass):
        pre = np.ascontiguousarray(prefixes, dtype=np.uint64)
        out = np.empty((pre.size, 256), dtype=np.uint64)
        u64 = C.POINTER(C.c_uint64)
        self._chk(self.lib.mmb_order_hist(self.h, int(param), int(pre.size), pre.ctypes.data_as(u64), int(npass),
                                          out.ctypes.data_as(u64)))
        return out

    # hpd (stats.jl:54-74) on the device-kept draws: summary.hpd_sharded drives these
    def hpd_collect(self, param, lo, hi, cap):
        """Collect the kept draws of `param` strictly below `lo` and strictly above `hi` into the
        engine's two tail buffers (mmb_hpd_collect), at most `cap` each: (n_below, n_above).  A
        count above `cap` is an error, and nothing is written past `cap`."""
        counts = (C.c_int64 * 2)()
        self._chk(self.lib.mmb_hpd_collect(self.h, int(param), float(lo), float(hi), int(cap), counts))
        return int(counts[0]), int(counts[1])

    def hpd_get_tails(self, nbelow, nabove):
        """The first `nbelow` / `nabove` values of the tail buffers (mmb_hpd_get_tails), as collected:
        unsorted until hpd_gap has run."""
        below, above = np.empty(int(nbelow)), np.empty(int(nabove))
        self._chk(self.lib.mmb_hpd_get_tails(self.h, abi.dptr(below), below.size, abi.dptr(above), above.size))
        return below, above

    def hpd_set_tails(self, below, above):
        """Upload tails (the pooled ones of every rank) as the engine's tails (mmb_hpd_set_tails)."""
        below = np.ascontiguousarray(below, dtype=np.float64).reshape(-1)
        above = np.ascontiguousarray(above, dtype=np.float64).reshape(-1)
        self._chk(self.lib.mmb_hpd_set_tails(self.h, abi.dptr(below), below.size, abi.dptr(above), above.size))

    def hpd_gap(self, m, total, lo, hi):
        """Sort the tails on the device and take the first minimum of b - a over a = sorted below
        padded with `lo` and b = `hi` padding then sorted above, `m` each (mmb_hpd_gap; `total` the
        pooled number of draws): (array [a[i], b[i]], i)."""
        out = np.empty(2)
        idx = C.c_int64()
        self._chk(self.lib.mmb_hpd_gap(self.h, int(m), int(total), float(lo), float(hi), abi.dptr(out), C.byref(idx)))
        return out, int(idx.value)

    # model log densities of the device-kept draws (modelstats.py maps names and closes dic)
    def _node_list(self, nodes):
        ids = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        return ids, ids.ctypes.data_as(C.POINTER(C.c_int32))

    def draws_logpdf(self, nodes):
        """n x K: the sum of the listed nodes' log densities at every kept draw (mmb_draws_logpdf,
        modelstats.jl:30-68); `nodes` are engine node ids, summed in list order."""
        ids, p = self._node_list(nodes)
        out = np.empty((max(self.num_kept(), 0), self.K), order="F")
        self._chk(self.lib.mmb_draws_logpdf(self.h, int(ids.size), p, abi.dptr(out)))
        return out

    def draws_deviance(self, nodes, shift):
        """K x 2: per chain [sum_i (D - shift), sum_i (D - shift)^2] of D = -2 logpdf over the kept
        draws, in row order (mmb_draws_deviance); the n x K values stay on the device."""
        ids, p = self._node_list(nodes)
        out = np.empty((self.K, 2))
        self._chk(self.lib.mmb_draws_deviance(self.h, int(ids.size), p, float(shift), abi.dptr(out)))
        return out

    def logpdf_at(self, nodes, x):
        """The listed nodes' log density at one point `x` (pmon values in monitored-column order),
        by the kernel of draws_logpdf on a one-row buffer (mmb_logpdf_at, modelstats.jl:15-25)."""
        ids, p = self._node_list(nodes)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if x.size != self.pmon:
            raise ArgumentError(f"the point must have {self.pmon} values, got {x.size}")
        lp = C.c_double()
        self._chk(self.lib.mmb_logpdf_at(self.h, int(ids.size), p, abi.dptr(x), C.byref(lp)))
        return lp.value

    # posterior predictive draws of the observed nodes (modelstats.py maps names and closes the moments)
    def predict_width(self, nodes):
        """P: the summed length of the listed observed nodes (mmb_predict_width)."""
        ids, p = self._node_list(nodes)
        P = C.c_int64()
        self._chk(self.lib.mmb_predict_width(self.h, int(ids.size), p, C.byref(P)))
        return int(P.value)

    def draws_predict(self, nodes, seed, start, thin, i0=0, i1=None):
        """(i1 - i0) x P x K: one variate of every element of the listed observed nodes at the kept
        draws [i0, i1) (default: all), parameters evaluated on the draw (mmb_draws_predict,
        modelstats.jl:71-102).  Kept row i has iteration start + i * thin; a value is a function of
        (seed, global chain id, iteration, node id, element) only."""
        ids, p = self._node_list(nodes)
        i1 = self.num_kept() if i1 is None else int(i1)
        P = self.predict_width(ids)
        out = np.empty((max(i1 - int(i0), 0), P, self.K), order="F")
        self._chk(self.lib.mmb_draws_predict(self.h, int(ids.size), p, C.c_uint64(int(seed)), int(start), int(thin),
                                             int(i0), i1, abi.dptr(out)))
        return out

    def draws_predict_moments(self, nodes, seed, start, thin, shift):
        """K x P x 2: per chain and predicted column [sum_i (yhat - shift_j), sum_i (yhat - shift_j)^2]
        over the kept draws, in row order (mmb_draws_predict_moments); the values stay on the device."""
        ids, p = self._node_list(nodes)
        P = self.predict_width(ids)
        shift = np.ascontiguousarray(shift, dtype=np.float64).reshape(-1)
        if shift.size != P:
            raise ArgumentError(f"the shift must have {P} values, got {shift.size}")
        out = np.empty((self.K, P, 2))
        self._chk(self.lib.mmb_draws_predict_moments(self.h, int(ids.size), p, C.c_uint64(int(seed)), int(start),
                                                     int(thin), abi.dptr(shift), abi.dptr(out)))
        return out

    def set_draws(self, value):
        """Upload `value` (n x p x chains, the Chains layout) as the device-kept draws
        (mmb_set_draws, the inverse of `draws`): the device summaries then run on it."""
        v = np.asarray(value, dtype=np.float64)
        if v.ndim != 3 or v.shape[1] != self.pmon or v.shape[2] != self.K or v.shape[0] < 1:
            raise ArgumentError(f"draws must be n x {self.pmon} x {self.K} with n >= 1, got {v.shape}")
        v = np.asfortranarray(v)
        self._chk(self.lib.mmb_set_draws(self.h, abi.dptr(v), v.shape[0]))

    # per-chain diagnostics of the device-kept draws (diag.py applies the closing formulas)
    def chain_autocov(self, i0, i1, lags):
        """K x p x (2 + nlags): [mean, gamma(0), gamma(lags[0]), ...] of the kept draws [i0, i1)."""
        lg = np.ascontiguousarray(lags, dtype=np.int64).reshape(-1)
        out = np.empty((self.K, self.pmon, 2 + lg.size))
        self._chk(self.lib.mmb_chain_autocov(self.h, int(i0), int(i1), int(lg.size),
                                             lg.ctypes.data_as(C.POINTER(C.c_int64)), abi.dptr(out)))
        return out

    def chain_mcse(self, i0, i1, etype, batch_size=100):
        """K x p x [mean, gamma(0), mcse, terms] of the kept draws [i0, i1); etype "bm", "imse"
        or "ipse" (or its MMB_MCSE_* code).  NaN where the reference's sqrt would throw."""
        if not isinstance(etype, (int, np.integer)):
            from .diag import etype_code
            etype = etype_code(etype)
        out = np.empty((self.K, self.pmon, abi.MMB_MCSE_FIELDS))
        self._chk(self.lib.mmb_chain_mcse(self.h, int(i0), int(i1), int(etype), int(batch_size), abi.dptr(out)))
        return out

    def chain_cvm(self, starts):
        """K x p x nstarts x [mean, W] of the suffix windows [s, n) of the kept draws, for 0-based
        strictly increasing `starts`: W = sum_t B_t^2 / m^2 of heideldiag.jl:14-16 (no 1 / S0)."""
        st = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
        out = np.empty((self.K, self.pmon, st.size, 2))
        self._chk(self.lib.mmb_chain_cvm(self.h, int(st.size), st.ctypes.data_as(C.POINTER(C.c_int64)),
                                         abi.dptr(out)))
        return out

    def chain_mcse_from(self, i0, i1, etype, batch_size=100):
        """chain_mcse with a window start per (chain, param): `i0` is K x p, the end `i1` common."""
        if not isinstance(etype, (int, np.integer)):
            from .diag import etype_code
            etype = etype_code(etype)
        i0 = np.ascontiguousarray(i0, dtype=np.int64)
        if i0.shape != (self.K, self.pmon):
            raise ArgumentError(f"window starts must be {self.K} x {self.pmon}, got {i0.shape}")
        out = np.empty((self.K, self.pmon, abi.MMB_MCSE_FIELDS))
        self._chk(self.lib.mmb_chain_mcse_from(self.h, i0.ctypes.data_as(C.POINTER(C.c_int64)), int(i1), int(etype),
                                               int(batch_size), abi.dptr(out)))
        return out

    def chain_raftery(self, q):
        """K x p x [threshold, kthin, ntest, n00, n10, n01, n11, bic] (rafterydiag.jl:13-34) of the
        kept draws; kthin NaN where the thinned series ran out before bic turned negative."""
        out = np.empty((self.K, self.pmon, abi.MMB_RAFTERY_FIELDS))
        self._chk(self.lib.mmb_chain_raftery(self.h, float(q), abi.dptr(out)))
        return out

    def change_counts(self):
        """p + 1 exact counts over this engine's chains of (chain, i >= 1) with x[i] != x[i-1]:
        per param, then with any param changed."""
        out = np.zeros(self.pmon + 1, dtype=np.int64)
        self._chk(self.lib.mmb_change_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out


class Chains:
    """Chains / ModelChains (src/output/chains.jl:5-11, modelchains.jl): value is
    n x p x chains, names the monitored nodes, range = start:thin:stop."""

    def __init__(self, value, names, start, thin, chains, model=None, engine=None):
        self.value = value
        self.names = list(names)
        self.start, self.thin = int(start), int(thin)
        self.chains = np.asarray(chains)
        self.model = model
        self.engine = engine

    @property
    def range(self):
        n = self.value.shape[0]
        return range(self.start, self.start + n * self.thin, self.thin)

    def __getitem__(self, name):
        return self.value[:, self.names.index(name), :]

    def _device_engine(self):
        eng = self.engine
        if eng is None or eng.h is None or eng.num_kept() != self.value.shape[0] or self.value.shape[0] == 0:
            raise ArgumentError("summaries run on the device-kept draws: sample with keep_device=True "
                                "(the engine holds the last window's draws)")
        return eng

    def summarystats(self, batch_size=100):
        """summarystats(c; etype=:bm) (stats.jl:85-94): p x [Mean, SD, Naive SE, MCSE, ESS]."""
        from .summary import summarystats_sharded
        return summarystats_sharded(self._device_engine(), batch_size)

    def quantile(self, q=(0.025, 0.25, 0.5, 0.75, 0.975)):
        """quantile(c; q) (stats.jl:73-80), pooled over iterations and chains: p x len(q)."""
        from .summary import quantile_sharded
        return quantile_sharded(self._device_engine(), q)

    def hpd(self, alpha=0.05):
        """hpd(c; alpha) (stats.jl:66-74): the highest-posterior-density interval of each monitored
        param, draws pooled over iterations and chains: (p x 2 array, ["95% Lower", "95% Upper"]).
        The tails are sorted on the device; only the result leaves it.  NaN draws are not
        detected: the result is then unspecified."""
        from .summary import hpd_labels, hpd_sharded
        return hpd_sharded(self._device_engine(), alpha), hpd_labels(alpha)

    def describe(self, q=(0.025, 0.25, 0.5, 0.75, 0.975), batch_size=100):
        """describe(c) (stats.jl:42-52): summarystats and quantiles per monitored name."""
        ss = self.summarystats(batch_size)
        qs = self.quantile(q)
        labels = ["Mean", "SD", "Naive SE", "MCSE", "ESS"]
        return {nm: {**{lb: float(ss[j, i]) for i, lb in enumerate(labels)},
                     **{f"{100 * x}%": float(qs[j, t]) for t, x in enumerate(q)}}
                for j, nm in enumerate(self.names)}

    def upload(self):
        """Put `value` on the engine as its device-kept draws (Engine.set_draws), so the device
        summaries and diagnostics run on chains that were read back from a file.  Explicit:
        `read` itself uploads nothing."""
        eng = self.engine
        if eng is None or eng.h is None or eng.K == 0:
            raise ArgumentError("upload needs an engine with initialised chains (read(name, model=...))")
        eng.set_draws(self.value)
        return self

    def autocor(self, lags=(1, 5, 10, 50), relative=True):
        """autocor(c; lags, relative) (stats.jl:3-13) per chain: (p x nlags x chains, labels).
        As in the reference, `relative` multiplies the lags by `thin` and otherwise a lag that
        is not a multiple of `thin` is an ArgumentError; the resulting lags are then used as
        INDEX lags of the kept series.  With thin > 1 "Lag L" is therefore the correlation of
        kept draws L rows apart, i.e. L * thin sampler iterations apart."""
        from .diag import autocor
        return autocor(self._device_engine(), lags, self.thin, relative)

    def changerate(self):
        """changerate(c) (stats.jl:19-39): the p + 1 rates [names..., Multivariate], 3 decimals."""
        from .diag import changerate_sharded
        return changerate_sharded(self._device_engine())

    def gewekediag(self, first=0.1, last=0.5, etype="imse", batch_size=100):
        """gewekediag(c; first, last, etype) (gewekediag.jl:3-31): p x 2 x chains,
        [round(z, 3), round(1 - erf(|z|/sqrt(2)), 4)].  One departure from the reference: where
        an IMSE / IPSE `value` is negative the reference's sqrt throws a DomainError; here that
        (chain, param) gets NaN."""
        from .diag import gewekediag
        return gewekediag(self._device_engine(), first, last, etype, batch_size)

    def mcse(self, etype="imse", batch_size=100):
        """mcse(x, etype) (mcse.jl:3-46) of each chain's kept series: p x chains.  NaN where the
        reference's sqrt of a negative IMSE / IPSE `value` would throw a DomainError."""
        from .diag import mcse
        return mcse(self._device_engine(), etype, batch_size)

    def heideldiag(self, alpha=0.05, eps=0.1, etype="imse", batch_size=100):
        """heideldiag(c; alpha, eps, etype) (heideldiag.jl:3-41): p x 6 x chains, [Burn-in,
        Stationarity, p-value, Mean, Halfwidth, Test], Burn-in counted from `start` as the
        reference counts it from start(c.range).  Departures: fewer than 10 kept draws are an
        ArgumentError (the reference's step is then 0 and it never returns for a series that
        does not converge at once), and NaN stands where the sqrt of a negative IMSE / IPSE
        `value` would throw a DomainError."""
        from .diag import heideldiag
        return heideldiag(self._device_engine(), alpha, eps, etype, batch_size, self.start)

    def rafterydiag(self, q=0.025, r=0.005, s=0.95, eps=0.001):
        """rafterydiag(c; q, r, s, eps) (rafterydiag.jl:3-61): p x 5 x chains, [Thinning, Burn-in,
        Total, Nmin, Dependence Factor], with `start` and `thin` where the reference takes
        start(c.range) and step(range).  Departure: a series whose thinned test sequence falls
        below 3 elements before bic turns negative gets NaN (the reference ends in a DomainError
        from log(-1))."""
        from .diag import rafterydiag
        return rafterydiag(self._device_engine(), q, r, s, eps, self.start, self.thin)

    def cor(self):
        """cor(c) (stats.jl:15-17): the p x p correlation matrix of the draws pooled over chains."""
        from .gelman import cor_sharded
        return cor_sharded(self._device_engine())

    def logpdf(self, nodekeys=None):
        """logpdf(mc[, nodekeys]) (modelstats.jl:28-51): the summed log density of the listed
        Stochastic nodes (default: all) at every kept draw, a Chains n x 1 x chains named
        ["logpdf"].  Every sampled node the list needs must be monitored."""
        from .modelstats import logpdf
        return logpdf(self, nodekeys)

    def dic(self):
        """dic(mc) (modelstats.jl:3-12): (2 x 2 [DIC, Effective Parameters] for pD and pV, row
        labels, column labels), from the deviance of the output nodes on the device-kept draws."""
        from .modelstats import dic
        return dic(self)


    def predict(self, nodekeys=None, seed=None, rows=None):
        """predict(mc[, nodekeys]) (modelstats.jl:71-102): posterior predictive draws of the observed
        output nodes (default: all of them) at every kept draw, a Chains n x P x chains named like
        names(m, nodekeys).  `seed` defaults to the seed of the chains; `rows` = (i0, i1) restricts
        the call to the kept rows [i0, i1), whose values equal those rows of the full call."""
        from .modelstats import predict
        return predict(self, nodekeys, seed, rows)

    def predict_summary(self, nodekeys=None, seed=None):
        """(P x 2 [Mean, SD] of the predicted values pooled over draws and chains, names, column
        labels): the moments are reduced on the device, the predicted values never leave it."""
        from .modelstats import predict_summary
        return predict_summary(self, nodekeys, seed)


def mcmc(model, inputs, inits, iters, burnin=0, thin=1, chains=1, verbose=False, device=0,
         chain_offset=0, seed=1, keep_device=False):
    """mcmc(m, inputs, inits, iters; burnin, thin, chains) (mcmc.jl:19-33)."""
    if not iters > burnin:
        raise ArgumentError("burnin is greater than or equal to iters")
    model.setinputs(inputs)
    init = model.init_matrix(inits, chains)
    model.burnin = burnin
    eng = Engine(model, device)
    eng.init_chains(init, chain_offset=chain_offset, seed=seed)
    draws = eng.run(iters, burnin=burnin, thin=thin, model_burnin=burnin, keep_device=keep_device)
    if draws is None:
        draws = np.empty((0, eng.pmon, eng.K))
    model.iter = eng.iter
    return Chains(draws, model.monitor_names, burnin + thin, thin,
                  np.arange(chain_offset + 1, chain_offset + chains + 1), model, eng)


def mcmc_restart(mc, iters, verbose=False):
    """mcmc(mc::ModelChains, iters) (mcmc.jl:3-16): continue from model.states."""
    eng, model = mc.engine, mc.model
    last = mc.range[-1] if mc.value.shape[0] else mc.start - mc.thin
    if last != (model.iter // mc.thin) * mc.thin:
        raise ArgumentError("chain is missing its last iteration")
    draws = eng.run(iters, burnin=last, thin=mc.thin, model_burnin=model.burnin)
    model.iter = eng.iter
    value = np.concatenate([mc.value, draws], axis=0) if draws is not None else mc.value
    return Chains(value, mc.names, mc.start, mc.thin, mc.chains, model, eng)


_CKPT_KIND = "mamba_amd.ModelChains/1"


def write(name, c):
    """write(name, c::AbstractChains) (fileio.jl:10-12): save the chains and, for a
    ModelChains with a live engine, the resumable model state (ModelState values + tune,
    Model.iter, Philox seed, global chain offset, Model.burnin).  The file is a plain
    .npz (no pickled objects): `read(name, model=...)` restores an engine on any device
    and `mcmc_restart` then continues exactly where the writer stopped."""
    arrays = dict(kind=np.array(_CKPT_KIND), value=np.asarray(c.value, dtype=np.float64),
                  names=np.array(c.names, dtype=np.str_), start=np.int64(c.start),
                  thin=np.int64(c.thin), chains=np.asarray(c.chains, dtype=np.int64))
    eng = c.engine
    if eng is not None and getattr(eng, "h", None) is not None and eng.K > 0:
        arrays.update(values=eng.values(), tune=eng.tune(), iter=np.int64(eng.iter),
                      seed=np.uint64(eng.seed), chain_offset=np.int64(eng.chain_offset),
                      model_burnin=np.int64(getattr(c.model, "burnin", 0)))
    with open(name, "wb") as f:  # np.savez would append ".npz" to a bare name
        np.savez(f, **arrays)


def read(name, model=None, device=0):
    """read(name, ModelChains) (fileio.jl:3-8): load chains written by `write`.  With
    `model` (the same Model, inputs set, as the writer's: closures are not serialised),
    the saved state is restored into a new engine on `device`, ready for
    `mcmc_restart(mc, iters)`.  Raises TypeError if the file holds no chains."""
    with np.load(name, allow_pickle=False) as z:
        if "kind" not in z.files or str(z["kind"]) != _CKPT_KIND:
            raise TypeError(f'read("{name}", ModelChains): not a chains file')
        d = {k: z[k] for k in z.files}
    eng = None
    if model is not None:
        if "values" not in d:
            raise ArgumentError("file holds no model state to resume from")
        vals = d["values"]
        eng = Engine(model, device)
        if vals.shape[1] != eng.P:
            eng.close()
            raise ArgumentError(f"saved state has {vals.shape[1]} values per chain, model has {eng.P}")
        eng.init_chains(vals, chain_offset=int(d["chain_offset"]), seed=int(d["seed"]))
        eng.set_tune(d["tune"])
        eng.set_iter(int(d["iter"]))
        model.burnin = int(d["model_burnin"])
        model.iter = int(d["iter"])
    return Chains(d["value"], [str(x) for x in d["names"]], int(d["start"]), int(d["thin"]),
                  d["chains"], model, eng)
