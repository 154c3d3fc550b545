"""hpd (src/output/stats.jl:54-74), the host half: mamba.jl_amd/summary.py hpd_sharded against the
np.sort restatement tests/hpd_ref.py, fed by an engine-shaped host shard (tests/test_summary.py's,
with numpy hpd_collect / hpd_gap restating the contracts of include/mamba_hip.h mmb_hpd_*); the
sharded path at world size 2 over gloo with the rank boundary inside the chains; and the C ABI's
argument checks, which need no device.  The device kernels are checked in tests/test_gpu_hpd.py.
Every comparison is exact: the same doubles, one IEEE subtraction."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import hpd_ref
from test_summary import HostSummaryShard, _free_port, _keys

ALPHAS = (1e-9, 0.05, 0.3, 0.5, 0.7, 0.999)


class HostHpdShard(HostSummaryShard):
    """HostSummaryShard plus the hpd entry points (mmb_hpd_collect / get_tails / set_tails / gap)."""

    def hpd_collect(self, param, lo, hi, cap):
        x = self.d[:, param, :].ravel()
        k = _keys(x)
        below, above = x[k < _keys(lo)[0]], x[k > _keys(hi)[0]]
        if below.size > cap or above.size > cap:
            raise RuntimeError("count above capacity")
        self.tails = (below, above)
        return below.size, above.size

    def hpd_get_tails(self, nbelow, nabove):
        return self.tails[0][:nbelow].copy(), self.tails[1][:nabove].copy()

    def hpd_set_tails(self, below, above):
        self.tails = (np.asarray(below, dtype=np.float64), np.asarray(above, dtype=np.float64))

    def hpd_gap(self, m, total, lo, hi):
        below, above = self.tails
        assert 1 <= m <= total and below.size <= m - 1 and above.size <= m - 1
        assert lo <= hi or 2 * m > total
        a = np.concatenate([np.sort(below), np.full(m - below.size, lo)])
        b = np.concatenate([np.full(m - above.size, hi), np.sort(above)])
        i = int(np.argmin(b - a))
        return np.array([a[i], b[i]]), i


@functools.lru_cache(maxsize=None)
def draws(name):
    v = hpd_ref.INPUTS[name]()
    v.setflags(write=False)
    return v


def test_inputs_are_what_the_tests_need():
    """The properties the inputs are chosen for, on the reference."""
    v = draws("small")
    assert v.shape == (41, 3, 67) and hpd_ref.hpd_count(0.05, v.shape[0] * v.shape[2]) == 138
    y = np.sort(v[:, 1, :].ravel())
    assert (y == y[137]).sum() > 50 and (y == y[2747 - 138]).sum() > 50           # ties at both thresholds
    assert len({int(b) for b in _keys(v[:, 2, :].ravel()) >> np.uint64(56)}) > 60   # the top key byte varies
    f = draws("flat")
    assert (f[:, 0, :] == -2.5).all() and set(np.unique(f[:, 1, :])) == {1.0, 2.0}
    z = f[:, 2, :][f[:, 2, :] == 0.0]
    assert np.signbit(z).any() and not np.signbit(z).all()
    b = draws("big")
    m = hpd_ref.hpd_count(0.05, b.shape[0] * b.shape[2])
    _, idx = hpd_ref.hpd(b, 0.05)
    assert m == 5140 and 0 < idx[0] < m - 1 and idx[1] == 0 and idx[2] == m - 1


def test_hpd_count_is_the_reference_double_product(mamba):
    hc = mamba.summary.hpd_count
    assert hc(0.05, 2747) == 138 and hc(0.999, 2747) == 2745
    assert hc(0.07, 100) == 8            # 0.07 * 100.0 = 7.000000000000001: ceil of the double product
    assert hc(1e-9, 2747) == hc(0.0, 2747) == hc(-3.0, 2747) == 1
    assert hc(0.5, 7) == 4


@pytest.mark.parametrize("name", ["small", "flat", "big"])
@pytest.mark.parametrize("alpha", ALPHAS + (0.0, -1.0))
def test_hpd_host_logic(mamba, name, alpha):
    """Thresholds, collect, padding with ties, overlapping tails (alpha > 0.5), alpha <= 0."""
    v = draws(name)
    got, idx = mamba.summary.hpd_sharded(HostHpdShard(v), alpha, return_index=True)
    ref, ridx = hpd_ref.hpd(v, alpha)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(idx, ridx)
    if alpha <= 0:
        np.testing.assert_array_equal(got, np.stack([v.min(axis=(0, 2)), v.max(axis=(0, 2))], axis=1))


def test_hpd_argument_errors_and_labels(mamba):
    shard = HostHpdShard(draws("small"))
    for bad in (1.0, 1.5, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(mamba.ArgumentError, match="alpha"):
            mamba.summary.hpd_sharded(shard, bad)
    lab = mamba.summary.hpd_labels
    assert lab(0.05) == ["95% Lower", "95% Upper"]
    assert lab(0.1)[0] == "90% Lower" and lab(0.01)[1] == "99% Upper" and lab(0.025)[0] == "97.5% Lower"
    # Chains.hpd: values and labels, through the same host logic
    v = draws("small")
    ch = mamba.Chains(v, ["a", "b", "c"], 1, 1, np.arange(1, v.shape[2] + 1), None, None)
    with pytest.raises(mamba.ArgumentError, match="device-kept"):
        ch.hpd()


# ---- sharded: world size 2 over gloo -----------------------------------------------------
def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import torch
        import _mamba_path
        mb = _mamba_path.load()
        v = hpd_ref.input_small()
        lo, hi = (0, 30) if rank == 0 else (30, v.shape[2])   # uneven; the boundary is inside the chains
        shard = HostHpdShard(v[:, :, lo:hi], chain_offset=lo)

        def ar_sum(x):
            t = torch.tensor(np.asarray(x, dtype=np.float64))
            dist.all_reduce(t)
            return t.numpy()

        def gather(obj):
            out = [None] * world
            dist.all_gather_object(out, obj)
            return out

        res = {a: mb.summary.hpd_sharded(shard, a, allreduce_sum=ar_sum, allgather=gather, return_index=True)
               for a in ALPHAS}
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


def test_sharded_hpd_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    v = hpd_ref.input_small()
    for a in ALPHAS:
        ref, ridx = hpd_ref.hpd(v, a)
        for rank in (0, 1):                      # both ranks, exactly the unsharded reference
            np.testing.assert_array_equal(got[rank][a][0], ref)
            np.testing.assert_array_equal(got[rank][a][1], ridx)


# ---- the C ABI without a device ----------------------------------------------------------
def test_hpd_abi_without_a_device(mamba):
    lib = mamba.abi.lib()
    assert lib.mmb_abi_version() == mamba.abi.MMB_ABI_VERSION == 10
    two = (C.c_double * 2)()
    cnt = (C.c_int64 * 2)()
    idx = C.c_int64()
    assert lib.mmb_hpd_collect(None, 0, 0.0, 1.0, 1, cnt) == -1
    assert lib.mmb_hpd_get_tails(None, two, 1, two, 1) == -1
    assert lib.mmb_hpd_set_tails(None, two, 1, two, 1) == -1
    assert lib.mmb_hpd_gap(None, 1, 2, 0.0, 1.0, two, C.byref(idx)) == -1
    assert b"null" in lib.mmb_last_error(None)
    for name in ("hpd_collect", "hpd_get_tails", "hpd_set_tails", "hpd_gap"):
        assert callable(getattr(mamba.Engine, name))
    assert callable(mamba.Chains.hpd) and callable(mamba.hpd_sharded)
