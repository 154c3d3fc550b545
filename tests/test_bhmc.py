"""BHMC without a device: the public constructor and every refusal, the lowered block spec, the engine's own
validation, csrc/bhmc.h against libm, and the plain-Python restatement (tests/bhmc_ref.py) against closed forms."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import bhmc_ref as hr
import binary_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi


def lowered(mamba, D, scheme, K=4, prior="bernoulli", mixed=False):
    m, inputs, inits = br.model(mamba.ir, D, prior, mixed)
    m.setinputs(inputs).setsamplers(scheme)
    return m, m.init_matrix(inits(K), K)


def flat(ir, n):
    """(model, inits(K)) of one Bernoulli(0.5) node of n elements with no targets: logf is n log(0.5) everywhere."""
    m = ir.Model(gamma=ir.Stochastic(1, lambda: ir.Bernoulli(0.5)))
    return m, lambda K: [{"gamma": [float((k >> (j % 5)) & 1) for j in range(n)]} for k in range(K)]


# ------------------------------------------------------------------ 1. constructor and validation
def test_abi_constants(mamba):
    a = mamba.abi
    assert a.MMB_SAMPLER_BHMC == 14 and a.MMB_ABI_VERSION == 10
    assert a.MMB_BHMC_MAX_TRAVELTIME == 128.0 * PI
    assert (a.MMB_SUB_NORMAL, a.MMB_SUB_INIT) == (hr.SUB_NORMAL, hr.SUB_INIT) == (0, 4)
    hdr = open(os.path.join(ROOT, "include", "mamba_hip.h")).read()
    assert re.search(r"\bMMB_SAMPLER_BHMC = 14\b", hdr) and re.search(r"#define MMB_ABI_VERSION 10\b", hdr)
    val = float(re.search(r"#define MMB_BHMC_MAX_TRAVELTIME (\S+)", hdr).group(1))
    assert val == 128.0 * PI
    mh = open(os.path.join(ROOT, "mamba.jl_amd", "csrc", "mmb_math.h")).read()
    assert re.search(r"#define MMB_SUB_INIT 4u\b", mh) and re.search(r"#define MMB_SUB_NORMAL 0u\b", mh)
    bh = open(os.path.join(ROOT, "mamba.jl_amd", "csrc", "bhmc.h")).read()
    assert float(re.search(r"#define MMB_BHMC_PI (\S+)", bh).group(1)) == PI
    assert float(re.search(r"#define MMB_BHMC_NEARZERO (\S+)", bh).group(1)) == hr.NEARZERO == 1e4 * np.finfo(float).eps
    assert "MMB_SAMPLER_BHMC = Int32(14)" in open(os.path.join(ROOT, "julia", "MambaHIP.jl")).read()


def test_constructor(mamba):
    a = mamba.abi
    s = mamba.BHMC("gamma", 2.5 * PI)
    assert (s.kind, s.adapt, s.tuning, s.params, s.scale, s.form, s.traveltime, s.refresh) == \
        (a.MMB_SAMPLER_BHMC, a.MMB_ADAPT_NONE, None, ["gamma"], 2.5 * PI, 0, 2.5 * PI, False)
    s = mamba.BHMC(["gamma"], 3, refresh=True)
    assert (s.scale, s.form, s.refresh) == (3.0, 1, True)
    assert repr(s) == "BHMC(['gamma'])" and s.name == "BHMC"
    assert [s.tune_len(d) for d in (1, 3, 32)] == [5, 9, 67]
    with pytest.raises(mamba.ArgumentError, match="one joint move"):
        mamba.BHMC(["a", "b"], 1.0)
    with pytest.raises(mamba.ArgumentError, match="refresh is True or False"):
        mamba.BHMC("g", 1.0, refresh=1)
    with pytest.raises(mamba.ArgumentError, match="traveltime is a number"):
        mamba.BHMC("g", "long")
    with pytest.raises(TypeError):
        mamba.BHMC("g")  # the reference has no default traveltime either


@pytest.mark.parametrize("make", ["line", "rats", "logistic"])
def test_non_ir_models_refuse(mamba, make):
    m = mamba.logistic(20, 3, 10.0) if make == "logistic" else getattr(mamba, make)()
    node = {"line": "beta", "rats": "alpha", "logistic": "beta"}[make]
    with pytest.raises(mamba.ArgumentError, match="node-IR"):
        m.setsamplers([mamba.BHMC(node, 1.0)])


def test_family_and_length_refusals(mamba):
    ir = mamba.ir
    with pytest.raises(mamba.ArgumentError, match="BHMC: node beta is not a Bernoulli"):
        lowered(mamba, br.MIX, [mamba.BHMC("beta", 1.0), mamba.DGS("gamma"), mamba.Slice("s2", 1.0)], mixed=True)
    for dist, init in ((lambda: ir.DiscreteUniform(0, 2), 1), (lambda: ir.DiscreteUniform(1, 2), 1),
                       (lambda: ir.Categorical([0.5, 0.5]), 1)):
        m = ir.Model(t=ir.Stochastic(1, dist)).setsamplers([mamba.BHMC("t", 1.0)])
        with pytest.raises(mamba.ArgumentError, match="BHMC: node t is not a Bernoulli"):
            m.init_matrix([{"t": [init, init]}], 1)
    m = ir.Model(t=ir.Stochastic(1, lambda n: ir.Binomial(n, 0.5))).setinputs({"n": [1.0, 1.0]})
    m.setsamplers([mamba.BHMC("t", 1.0)])
    with pytest.raises(mamba.ArgumentError, match="BHMC: node t is not a Bernoulli"):
        m.init_matrix([{"t": [0, 1]}], 1)
    m, inits = flat(ir, 33)
    m.setsamplers([mamba.BHMC("gamma", 1.0)])
    with pytest.raises(mamba.ArgumentError, match="at most 32 elements"):
        m.init_matrix(inits(1), 1)
    m, inits = flat(ir, 32)
    m.setsamplers([mamba.BHMC("gamma", 64.5 * PI)])  # the doc demo's (2 p + 0.5) pi at p = 32
    m.init_matrix(inits(1), 1)
    # a binary node may sit in a DGS, BMG, BMC3, BIA or BHMC block; another kind refuses it in its own words
    for s in (mamba.DGS("gamma"), mamba.BMG("gamma"), mamba.BMC3("gamma"), mamba.BIA("gamma"), mamba.BHMC("gamma", 1.0)):
        lowered(mamba, br.S3, [s])
    with pytest.raises(mamba.ArgumentError, match="discrete node gamma"):
        lowered(mamba, br.S3, [mamba.Slice("gamma", 1.0)])


def test_traveltime_refusals(mamba):
    """Finite, > 0 and <= 128 pi, checked once the node's length is known (with the 1..32 elements)."""
    for T in (30.5 * PI, 128.0 * PI, 1e-3):  # pollution.jl's, the cap itself, a short one
        lowered(mamba, br.S3, [mamba.BHMC("gamma", T)])
    for T in (0.0, -1.0, math.inf, math.nan, np.nextafter(128.0 * PI, math.inf), 1e9):
        with pytest.raises(mamba.ArgumentError, match="traveltime is not finite, > 0 and <= 128 pi"):
            lowered(mamba, br.S3, [mamba.BHMC("gamma", T)])


def test_inits_are_binary(mamba):
    for prior in ("bernoulli", "uniform"):
        m, inputs, inits = br.model(mamba.ir, br.S3, prior)
        m.setinputs(inputs).setsamplers([mamba.BHMC("gamma", 2.5 * PI)])
        for v in (2.0, 0.5, -1.0):
            bad = inits(2)
            bad[1]["gamma"] = [v, 0.0, 1.0]
            with pytest.raises(mamba.ArgumentError, match=r"discrete node gamma \(chain 2\) is outside its support"):
                m.init_matrix(bad, 2)


def test_lowered_block_spec_and_tune_len(mamba):
    a = mamba.abi
    m, V = lowered(mamba, br.S6, [mamba.BHMC("gamma", 12.5 * PI, refresh=True)])
    assert V.shape == (4, 6) and set(np.unique(V)) <= {0.0, 1.0}
    b = m.spec().blocks[0]
    assert (b.sampler, b.nnodes, b.dim, b.form, b.scale, b.ntuning, b.transform) == (14, 1, 6, 1, 12.5 * PI, 0, 0)
    I = m.ir()
    assert (I.nodes[1].family, I.nodes[1].fixed, I.nodes[1].len) == (a.MMB_IR_BERNOULLI, 0, 6)
    assert [I.blocks[0].term[t] for t in range(I.blocks[0].nterms)] == [1, 0]  # the node, then its target
    m, _ = lowered(mamba, br.S32, [mamba.BHMC("gamma", 2.5 * PI)], prior="uniform")
    b = m.spec().blocks[0]
    assert (b.sampler, b.dim, b.form, b.scale) == (14, 32, 0, 2.5 * PI)
    assert (m.ir().nodes[1].family, m.ir().nodes[1].hi) == (a.MMB_IR_DISCRETEUNIFORM, 1.0)
    # the canonical row [position[d], velocity[d], wallhits, wallcrosses, initialised]: the source's table, the host's
    # mirror of it and the restatement's row agree (mmb_tune_len needs an engine, and an engine a device)
    src = open(os.path.join(ROOT, "mamba.jl_amd", "csrc", "engine_tune.cpp")).read()
    assert re.search(r"case MMB_SAMPLER_BHMC: return 2 \* d \+ 3;", src)
    mix = [mamba.RWM("beta", 0.3), mamba.Slice("s2", 1.0, transform=True), mamba.BHMC("gamma", 2.5 * PI)]
    m, _ = lowered(mamba, br.MIX, mix, mixed=True)
    assert [s.tune_len(m.block_dim(s)) for s in m.samplers] == [3, 0, 9]
    assert hr.tune_offset(hr.spec("MIX", True, False), 2) == 3 and hr.tune_offset(hr.spec("MIX", True, True), 0) == 0
    out = hr.bhmc_step(lambda x: 0.0, 3, [0.0] * 9, 2.5 * PI, False, lambda k: 1.0 + k, lambda k: 0.0, hr.BDec(), hr.PyOps())
    assert out.done and len(out.row) == 9 and out.row[8] == 1.0


def test_engine_validation(mamba):
    """mmb_ir_jit_prebuild validates the IR and the block specs like mmb_create_ir and needs no device: the test models
    pass and the specialised kernel declines them naming BHMC; mmb_create_ir refuses what the host refuses."""
    lib, a = mamba.abi.lib(), mamba.abi
    buf = C.create_string_buffer(512)
    for dn, Tpi, mixed, first in hr.REPLAY_CASES:
        bl = [mamba.BHMC("gamma", Tpi * PI)]
        ot = [mamba.RWM("beta", 0.3), mamba.Slice("s2", 1.0, transform=True)] if mixed else []
        m, _ = lowered(mamba, hr.DATA[dn], bl + ot if first else ot + bl, prior=br.prior_of(dn), mixed=mixed)
        spec, I = m.spec(), m.ir()
        rc = lib.mmb_ir_jit_prebuild(C.byref(spec), C.byref(I), buf, 512)
        assert rc == -2 and b"BHMC" in buf.value, (dn, rc, buf.value, lib.mmb_last_error(None))
    # a Binomial node patched into a BHMC block: refused by name
    ir = mamba.ir
    m = ir.Model(t=ir.Stochastic(1, lambda n: ir.Binomial(n, 0.5))).setinputs({"n": [1.0, 1.0]})
    m.setsamplers([mamba.DGS("t")]).init_matrix([{"t": [0, 1]}], 1)
    spec, I = m.spec(), m.ir()
    spec.blocks[0].sampler, spec.blocks[0].scale = a.MMB_SAMPLER_BHMC, 1.0
    rc = lib.mmb_ir_jit_prebuild(C.byref(spec), C.byref(I), buf, 512)
    msg = lib.mmb_last_error(None).decode()
    assert rc == -1 and "BHMC" in msg and "not binary" in msg, msg

    def rc_of(spec, I):
        h = C.c_void_p()
        rc = lib.mmb_create_ir(C.byref(spec), C.byref(I), 0, C.byref(h))
        assert not h.value
        return rc, lib.mmb_last_error(None).decode()
    for field, val, want in [("scale", 0.0, "traveltime is not finite"), ("scale", -2.0, "traveltime is not finite"),
                             ("scale", math.nan, "traveltime is not finite"), ("scale", math.inf, "traveltime is not"),
                             ("scale", 403.0, "traveltime is not finite"), ("form", 2, "refresh is 0 or 1")]:
        m, _ = lowered(mamba, br.S3, [mamba.BHMC("gamma", 2.5 * PI)])
        spec, I = m.spec(), m.ir()
        setattr(spec.blocks[0], field, val)
        rc, msg = rc_of(spec, I)
        assert rc == -1 and want in msg, (field, val, msg)


# ------------------------------------------------------------------ 2. csrc/bhmc.h against libm
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return hr.host_lib(tmp_path_factory.mktemp("bhmc_host"))


def test_header_atan2_against_libm(host):
    """mmb_atan2 against numpy.arctan2: 20000 points per quadrant with magnitudes from 1e-300 to 1e300 and 20000 more
    with both magnitudes below 4, the axes, signed zeros, infinities and NaN.  At most 2 ulps: fdlibm's documented bound
    below 1 ulp plus libm's own (measured: 1.0)."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for sy, sx in itertools.product((1.0, -1.0), repeat=2):
        for wide in (True, False):
            y = sy * (10.0 ** rng.uniform(-300, 300, 20000) if wide else rng.uniform(0, 4, 20000))
            x = sx * (10.0 ** rng.uniform(-300, 300, 20000) if wide else rng.uniform(0, 4, 20000))
            got = np.array([host.h_atan2(a, b) for a, b in zip(y, x)])
            ref = np.arctan2(y, x)
            ulps = np.abs(got - ref) / np.spacing(np.abs(ref))
            assert np.all(np.signbit(got) == np.signbit(ref))
            worst = max(worst, float(ulps.max()))
    print(f"mmb_atan2: worst {worst} ulps")
    assert worst <= 2.0
    special = [0.0, -0.0, 1.0, -1.0, 1e-300, -1e300, 5e-324, math.inf, -math.inf, math.nan]
    for a, b in itertools.product(special, repeat=2):
        g, r = host.h_atan2(a, b), float(np.arctan2(a, b))
        if r != r:
            assert g != g, (a, b, g)
        else:
            assert abs(g - r) <= 2.0 * np.spacing(abs(r)) and math.copysign(1.0, g) == math.copysign(1.0, r), (a, b, g, r)


def test_header_sincos_against_libm(host):
    """mmb_sincos against numpy on 20000 points of [0, pi] and 0, pi / 2, pi: 2e-15 absolute, the bound of test_math's
    sincos test (measured: 1.2e-16)."""
    rng = np.random.default_rng(6)
    s, c, worst = C.c_double(), C.c_double(), 0.0
    for x in list(rng.uniform(0.0, PI, 20000)) + [0.0, PI / 2.0, PI]:
        host.h_sincos(x, C.byref(s), C.byref(c))
        worst = max(worst, abs(s.value - math.sin(x)), abs(c.value - math.cos(x)))
    print(f"mmb_sincos: worst {worst:.3e}")
    assert worst <= 2e-15
    host.h_sincos(0.0, C.byref(s), C.byref(c))
    assert (s.value, c.value) == (0.0, 1.0)
    host.h_sincos(PI, C.byref(s), C.byref(c))
    assert c.value == -1.0 and abs(s.value - math.sin(PI)) <= 1e-25  # the double nearest pi lies 1.22e-16 below pi


def test_header_elements_against_restatement(host):
    """walltime, guard, move and bounce of the header against the restatement's: the same decisions, values to 1e-15."""
    rng = np.random.default_rng(7)
    H, P, d = hr.HostOps(host), hr.PyOps(), hr.BDec()
    for v, p in rng.standard_normal((2000, 2)):
        assert abs(H.walltime(v, p) - P.walltime(v, p)) <= 4e-16 * PI
        s, c = P.sincos(abs(p) % PI)
        assert H.move(v, p, s, c) == P.move(v, p, s, c)
        for dl in (0.0, 0.3 * p, -5.0, math.inf, -math.inf, math.nan):
            assert H.bounce(v, dl, d) == P.bounce(v, dl, d)
    assert H.walltime(1.0, 0.0) == 0.0 and H.walltime(-1.0, 0.0) == 0.0 and H.walltime(0.0, 1.0) == PI / 2
    assert math.isnan(H.walltime(math.nan, 1.0)) and math.isnan(H.walltime(1.0, math.nan))
    for w in (0.0, 1e-13, 2.0 * PI, 2.0 * PI - 1e-13):
        assert H.guard(w, d) == math.inf == P.guard(w, d)
    for w in (1e-11, 1.0, PI, math.inf):
        assert H.guard(w, d) == w == P.guard(w, d)
    assert math.isnan(H.guard(math.nan, d))
    assert H.bounce(0.0, math.inf, d) == (-0.0, False) and H.bounce(-2.0, -math.inf, d) == (-math.inf, True)
    assert d.nears == []


# ------------------------------------------------------------------ 3. the restatement alone
@pytest.mark.parametrize("n,Tpi", [(1, 2.5), (3, 2.5), (3, 6.5), (32, 2.5)])
def test_flat_density_is_a_rigid_rotation(oracle, n, Tpi):
    """A flat log density crosses every wall at unchanged speed: m updates rotate the particle by m T, so position =
    b0 cos(m T) + a0 sin(m T), velocity = a0 cos(m T) - b0 sin(m T), and wallhits == wallcrosses == the sign changes of
    the closed form.  Tolerance 1e-12 of the particle's size: each event's rotation is good to a few ulps, and there
    are at most 5 x 96 of them."""
    z, T, m = oracle.L.orc_normal, Tpi * PI, 5
    logf = lambda x: n * math.log(0.5)  # noqa: E731
    most = 0
    for chain in range(5):
        b0 = [z(hr.SEED, chain, 1, 0, hr.SUB_INIT, i) for i in range(n)]
        a0 = [z(hr.SEED, chain, 1, 0, hr.SUB_INIT, 32 + i) for i in range(n)]
        row, d = [0.0] * (2 * n + 3), hr.BDec()
        for it in range(1, m + 1):
            o = hr.bhmc_step(logf, n, row, T, False, lambda k: z(hr.SEED, chain, it, 0, hr.SUB_INIT, k), None, d, hr.PyOps())
            assert o.done and o.hits == o.crosses <= hr.event_bound(n, T)
            most = max(most, o.hits)
            row = o.row
            assert o.value == [1.0 if p > 0.0 else 0.0 for p in row[:n]]
        want = [b * math.cos(m * T) + a * math.sin(m * T) for a, b in zip(a0, b0)] + \
               [a * math.cos(m * T) - b * math.sin(m * T) for a, b in zip(a0, b0)]
        assert hr.row_gap(row, want, n) <= 1e-12
        count = sum(hr.sign_changes(b, a, m * T) for a, b in zip(a0, b0))
        assert row[2 * n] == row[2 * n + 1] == count
        assert d.nears == []
    print(f"n = {n}, T = {Tpi} pi: most events in an update {most}, bound {hr.event_bound(n, T)}")
    if (n, Tpi) == (3, 6.5):
        assert most == hr.event_bound(n, T) == 21  # the bound is reached


def test_energy_invariant(oracle):
    """sum(position^2 + velocity^2) / 2 - logf(S) is conserved by every update without refresh (binary_ref's S6, 10
    updates of about 78 events from the chain's own draw): to 1e-11 of its size."""
    sp = hr.spec("S6")
    node = sp.blocks[0][1]
    init = [1.0, 0.0, 1.0, 1.0, 0.0, 0.0]
    worst = []

    def each(st, pre, out, zi, zr):
        lf = lambda x: node.logf(st, x)  # noqa: E731
        if pre[-1] == 0.0:
            pre = [zi(i) for i in range(6)] + [zi(32 + i) for i in range(6)] + [0.0, 0.0, 1.0]
        e0, e1 = hr.energy(lf, pre, 6), hr.energy(lf, out.row, 6)
        assert out.done and out.hits <= hr.event_bound(6, 12.5 * PI)
        worst.append(abs(e1 - e0) / abs(e0))
    for chain in range(3):
        hr.forward(oracle.L.orc_normal, sp, hr.SEED, init, chain, 10, 12.5 * PI, False, each=each)
    print(f"energy drift: worst {max(worst):.2e} (relative)")
    assert max(worst) <= 1e-11


def test_exact_posterior_with_refresh(oracle):
    """refresh=True is Pakman & Paninski's algorithm and targets the posterior: S3's three coupled indicators, 1024
    independent chains, T = 3.5 pi, the 12th draw of each: the 8 state frequencies within 5 standard errors
    sqrt(p (1 - p) / 1024) of the enumerated posterior.  refresh=False (the reference) is not tested against the
    posterior: its velocity is never redrawn and it does not target it."""
    K, iters, T = 1024, 12, 3.5 * PI
    sp = hr.spec("S3")
    code = []
    for chain in range(K):
        vals = hr.forward(oracle.L.orc_normal, sp, hr.SEED, [0.0, 0.0, 0.0], chain, iters, T, True)[0]
        code.append(int(vals[-1][0] * 4 + vals[-1][1] * 2 + vals[-1][2]))
    states = list(itertools.product([0.0, 1.0], repeat=3))
    lp = [br.logpdf_gamma_y(br.S3, list(g))[0] for g in states]
    w = [math.exp(x - max(lp)) for x in lp]
    post = [x / math.fsum(w) for x in w]
    freq = np.bincount(code, minlength=8) / K
    for s, (p, f) in enumerate(zip(post, freq)):
        print(f"state {states[s]}: posterior {p:.5f}, frequency {f:.5f}, {abs(f - p) / math.sqrt(p * (1 - p) / K):.2f} se")
    for p, f in zip(post, freq):
        assert abs(f - p) <= 5.0 * math.sqrt(p * (1.0 - p) / K)


def _inits(mamba, dn, mixed):
    m, inputs, inits = br.model(mamba.ir, hr.DATA[dn], br.prior_of(dn), mixed)
    others = [mamba.RWM("beta", 0.3), mamba.Slice("s2", 1.0, transform=True)] if mixed else []
    m.setinputs(inputs).setsamplers([mamba.BHMC("gamma", 1.0)] + others)
    return m.init_matrix(hr.inits_of(dn, inits)(hr.K_REPLAY), hr.K_REPLAY)


@pytest.mark.parametrize("refresh", [False, True])
def test_restatement_meets_no_threshold_and_summation_gap(mamba, oracle, refresh):
    """On the GPU replay's seed, chain count and iterations the restatement alone (MIX with beta and s2 held at their
    inits) meets no decision within DELTA of its threshold, and no stall except on EDGE, which is there for them.
    The same runs measure the summation gap: every update is repeated from its own pre-update row with the log
    densities summed naively in reversed term order in place of math.fsum; the largest row_gap is what
    bhmc_ref.SUMMATION_GAP records (and the replay allows 100 times it)."""
    gaps = []
    for dn, Tpi, mixed, first in hr.REPLAY_CASES:
        if not first:
            continue
        V = _inits(mamba, dn, mixed)
        sp, spn = hr.spec(dn, mixed), hr.spec(dn, mixed, naive=True)
        n, T = hr.DATA[dn].n, Tpi * PI
        near = stalls = infspeed = 0
        for chain in range(hr.K_REPLAY):
            def each(st, pre, out, zi, zr):
                o2 = hr.bhmc_step(lambda x: spn.blocks[0][1].logf(st, x), n, pre, T, refresh, zi, zr, hr.BDec(), hr.PyOps())
                assert (o2.done, o2.hits, o2.crosses, o2.value) == (out.done, out.hits, out.crosses, out.value)
                gaps.append(hr.row_gap(o2.row, out.row, n))
            _, _, nr, outs = hr.forward(oracle.L.orc_normal, sp, hr.SEED, V[chain], chain, hr.ITERS_REPLAY, T, refresh,
                                        each=each)
            near += nr
            stalls += sum(not o.done for o in outs)
            infspeed += sum(o.infspeed for o in outs)
            assert all(o.hits <= hr.event_bound(n, T) for o in outs)
        print(f"{dn} refresh={refresh}: {near} near decisions, {stalls} stalls, {infspeed} crossings at infinite speed")
        assert near == 0
        if dn == "EDGE":
            assert stalls > 0 and infspeed > 0
        else:
            assert stalls == 0
    print(f"summation gap: worst {max(gaps):.3e}; recorded {hr.SUMMATION_GAP:.3e}")
    assert max(gaps) <= hr.SUMMATION_GAP <= 4.0 * max(max(gaps), 1e-16)
