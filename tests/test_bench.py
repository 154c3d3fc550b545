"""bench.py's plain run and --dump-outputs: the result line's timing fields, what a plain run
leaves out, and the dumped arrays against the same run made directly on an Engine."""
import json
import os
import sys

import numpy as np
import pytest


class _FakeEngine:
    """values() / draws() of an engine after a kept window (no device)."""

    def __init__(self, K, P, nk, pmon):
        rng = np.random.default_rng(3)
        self.v = rng.normal(size=(K, P))
        self.d = np.asfortranarray(rng.normal(size=(nk, pmon, K)))

    def values(self):
        return self.v

    def draws(self):
        return self.d


def _load(path, sfx=""):
    return {n: np.load(os.path.join(path, n + sfx + ".npy")) for n in ("values", "draws", "chains")}


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    eng = _FakeEngine(K=200, P=7, nk=5, pmon=3)
    bench.dump_outputs(eng, str(tmp_path / "all"), 0)
    a = _load(str(tmp_path / "all"))
    assert all(x.dtype == np.float64 for x in a.values())
    np.testing.assert_array_equal(a["chains"], np.arange(200))
    np.testing.assert_array_equal(a["values"], eng.v)
    np.testing.assert_array_equal(a["draws"], eng.d)
    # over the budget: whole chains of a fixed seeded sample, the same from call to call
    per_chain = 8 * (7 + 5 * 3 + 1)
    monkeypatch.setattr(bench, "DUMP_BYTES", 50 * per_chain + 17)
    bench.dump_outputs(eng, str(tmp_path / "s1"), 0)
    bench.dump_outputs(eng, str(tmp_path / "s2"), 1)
    s1, s2 = _load(str(tmp_path / "s1")), _load(str(tmp_path / "s2"), "_rank1")
    idx = s1["chains"].astype(int)
    assert len(idx) == 50 and len(set(idx)) == 50 and np.all(np.diff(idx) > 0)
    assert sum(x.nbytes for x in s1.values()) <= bench.DUMP_BYTES
    np.testing.assert_array_equal(s1["values"], eng.v[idx])
    np.testing.assert_array_equal(s1["draws"], eng.d[:, :, idx])
    for n in s1:
        np.testing.assert_array_equal(s1[n], s2[n])


@pytest.mark.gpu
def test_bench_plain_run_line_and_dumped_outputs(mamba, tmp_path, capsys, monkeypatch):
    """A plain run (in this process: bench.main) times exactly --steps steps, reports ms_per_step
    consistent with its throughput, leaves the --full extras out, and --dump-outputs holds, bit for
    bit, the chain state and kept draws of the same run sequence made directly on an Engine."""
    import bench
    mb = mamba
    K, steps, warmup, pre, thin = 256, 6, 2, 128, 2
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    out_dir = str(tmp_path / "dump")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                                      "--chains", str(K), "--dump-outputs", out_dir])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == warmup
    assert out["unit"] == "chain-updates/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["ms_per_step"] > 0
    np.testing.assert_allclose(out["value"], K / (out["ms_per_step"] * 1e-3), rtol=1e-9)
    for k in ("cpu_baseline", "gelman_rubin_psrf"):
        assert k not in out
    assert "collective" not in out["config"]
    got = _load(out_dir)
    assert all(x.dtype == np.float64 for x in got.values())
    m = mb.rats()
    m.setinputs(mb.model.RATS_DATA)
    m.setsamplers(mb.model.rats_scheme_gibbs_amm())
    eng = mb.Engine(m, device=0)
    eng.init_chains(mb.model.rats_init_ls(K, seed=1000), chain_offset=0, seed=20261015)
    eng.run(pre, burnin=0, thin=thin, model_burnin=0, draws=False, keep_device=False)
    eng.run(warmup, burnin=0, thin=thin, model_burnin=0, draws=False, keep_device=False)
    eng.reserve_draws(steps // thin + 1)
    eng.run(steps, burnin=pre + warmup, thin=thin, model_burnin=0, draws=False, keep_device=True)
    v, d = eng.values(), eng.draws()
    eng.close()
    assert d.shape == (steps // thin, 3, K)
    np.testing.assert_array_equal(got["chains"], np.arange(K))
    np.testing.assert_array_equal(got["values"], v)
    np.testing.assert_array_equal(got["draws"], d)
