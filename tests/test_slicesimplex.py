"""SliceSimplex / Dirichlet on the host: constructors, the node-IR lowering and its checks, the engine's
validation of the lowered tables, and the restatement (tests/slicesimplex_ref.py) on its own."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import slicesimplex_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -2  # include/mamba_hip.h MMB_E_ARG, MMB_E_UNSUPPORTED
SEED = 11  # the GPU tests' seed (tests/test_gpu_slicesimplex.py)


@pytest.fixture(scope="module")
def mb():
    import _mamba_path
    return _mamba_path.load()


@pytest.fixture(scope="module")
def prim():
    import oracle_lib
    return ref.Prim(oracle_lib.Oracle().L)


def compiled(mb, name, scheme, K=2):
    m, inputs, inits = getattr(ref, "model" + name)(mb.ir)
    m.setinputs(inputs).setsamplers(scheme)
    return m, m.init_matrix(inits(K), K)


# ---------------------------------------------------------------- constructors
@pytest.mark.parametrize("scale", [0.0, -0.5, 1.0000001, 2, float("nan"), float("inf"), "x"])
def test_scale_outside_unit_interval(mb, scale):
    with pytest.raises(mb.ArgumentError, match=re.escape("scale is not in (0, 1]")):
        mb.SliceSimplex("P", scale=scale)


def test_constructor_fields(mb):
    s = mb.SliceSimplex("P")
    assert (s.kind, s.params, s.scale, s.tuning, s.adapt) == (10, ["P"], 1.0, None, mb.abi.MMB_ADAPT_NONE)
    assert mb.SliceSimplex(["a", "b"], scale=0.75).scale == 0.75
    assert repr(mb.SliceSimplex("P", scale=0.5)) == "SliceSimplex(['P'])"


def test_constants_agree_with_the_headers(mb):
    a = mb.abi
    h = open(os.path.join(ROOT, "include", "mamba_hip.h")).read()
    mm = open(os.path.join(ROOT, "mamba.jl_amd", "csrc", "mmb_math.h")).read()
    assert int(re.search(r"MMB_SAMPLER_SLICESIMPLEX = (\d+)", h).group(1)) == a.MMB_SAMPLER_SLICESIMPLEX == 10
    assert int(re.search(r"MMB_IR_DIRICHLET = (\d+)", h).group(1)) == a.MMB_IR_DIRICHLET == 14
    assert int(re.search(r"#define MMB_SIMPLEX_MAX (\d+)", h).group(1)) == a.MMB_SIMPLEX_MAX == 32
    assert float(re.search(r"#define MMB_SIMPLEX_TOL (\S+)", h).group(1)) == a.MMB_SIMPLEX_TOL == ref.SIMPLEX_TOL
    assert int(re.search(r"#define MMB_SUB_SIMPLEX (\d+)u", mm).group(1)) == a.MMB_SUB_SIMPLEX == ref.SUB_SIMPLEX == 6
    assert int(re.search(r"#define MMB_SUB_UNIFORM (\d+)u", mm).group(1)) == ref.SUB_UNIFORM
    assert int(re.search(r"#define MMB_SLICE_MAX_SHRINK (\d+)", h).group(1)) == ref.MAX_SHRINK
    assert 32 * ref.MAX_SHRINK + 31 < 2 ** 32  # the draws' uniform index at the cap
    assert a.MMB_ABI_VERSION == 10  # additive


def test_line_and_rats_refuse(mb):
    for m in (mb.line(), mb.rats()):
        with pytest.raises(mb.ArgumentError, match="node-IR models"):
            m.setsamplers([mb.SliceSimplex("s2" if m.kind == mb.abi.MMB_MODEL_LINE else "s2_c")])


# ---------------------------------------------------------------- ir.Dirichlet / ir.Categorical(P)
@pytest.mark.parametrize("alpha", [[1.0, 0.0], [1.0, -2.0], [float("nan"), 1.0], [float("inf"), 1.0]])
def test_dirichlet_alpha_must_be_positive(mb, alpha):
    with pytest.raises(mb.ArgumentError, match="alpha must be positive"):
        mb.ir.Dirichlet(alpha)
    m = mb.ir.Model(P=mb.ir.Stochastic(1, lambda a: mb.ir.Dirichlet(a)))  # as a data vector: checked at lowering
    m.setinputs({"a": alpha}).setsamplers([mb.SliceSimplex("P")])
    with pytest.raises(mb.ArgumentError, match="alpha must be positive"):
        m.init_matrix([{"P": [0.5, 0.5]}], 1)


def test_dirichlet_alpha_expression_refused(mb):
    with pytest.raises(mb.ArgumentError, match="constant list or a data vector"):
        mb.ir.Dirichlet(mb.ir.Ref("a") + 1.0)


@pytest.mark.parametrize("k", [1, 33])
def test_dirichlet_length_limits(mb, k):
    m = mb.ir.Model(P=mb.ir.Stochastic(1, lambda: mb.ir.Dirichlet([1.0] * k)))
    m.setsamplers([mb.SliceSimplex("P")])
    with pytest.raises(mb.ArgumentError, match="32 elements"):  # (33: the block limit of every sampler says it first)
        m.init_matrix([{"P": [1.0 / k] * k}], 1)


def test_dirichlet_alpha_length_must_match(mb):
    m = mb.ir.Model(P=mb.ir.Stochastic(1, lambda: mb.ir.Dirichlet([1.0, 1.0, 1.0])))
    m.setsamplers([mb.SliceSimplex("P")])
    with pytest.raises(mb.ArgumentError, match="alpha has 3 elements, the node 2"):
        m.init_matrix([{"P": [0.5, 0.5]}], 1)


def test_arrays_of_dirichlets_refused(mb):
    m = mb.ir.Model(P=mb.ir.Stochastic(2, lambda: mb.ir.Dirichlet([1.0] * 4)))
    m.setsamplers([mb.SliceSimplex("P")])
    with pytest.raises(mb.ArgumentError, match="arrays of Dirichlets are not lowered"):
        m.init_matrix([{"P": [0.25] * 4}], 1)


def test_dirichlet_only_by_slicesimplex_and_back(mb):
    ir = mb.ir
    m = ir.Model(P=ir.Stochastic(1, lambda: ir.Dirichlet([1.0, 1.0])), z=ir.Stochastic(lambda: ir.Normal(0, 1)))
    for bad in (mb.Slice("P", 1.0), mb.AMWG("P", 0.1), mb.RWM("P", 0.1), mb.AMM("P", np.eye(2))):
        m.setsamplers([bad, mb.Slice("z", 1.0)])
        with pytest.raises(mb.ArgumentError, match="Dirichlet node P cannot be sampled by .*: use SliceSimplex"):
            m.init_matrix([{"P": [0.5, 0.5], "z": 0.0}], 1)
    m.setsamplers([mb.SliceSimplex("P"), mb.SliceSimplex("z")])
    with pytest.raises(mb.ArgumentError, match="SliceSimplex: node z is not a Dirichlet node"):
        m.init_matrix([{"P": [0.5, 0.5], "z": 0.0}], 1)


@pytest.mark.parametrize("P", [[0.5, 0.6], [1.5, -0.5], [0.5, 0.5 + 3e-8], [float("nan"), 0.5], [1.0]])
def test_inits_must_be_probability_vectors(mb, P):
    m, inputs, inits = ref.modelC(mb.ir)
    m.setinputs(inputs).setsamplers(mb.ir.eyes_scheme())
    bad = [dict(d) for d in inits(3)]
    bad[2]["P"] = P  # every chain is checked, not the first only
    with pytest.raises(mb.ArgumentError, match="variate is not a probability vector"):
        m.init_matrix(bad, 3)
    m.init_matrix(inits(3), 3)


def test_categorical_p_must_be_data_or_a_sampled_dirichlet(mb):
    ir = mb.ir
    with pytest.raises(mb.ArgumentError, match="constant list, a data vector or a sampled Dirichlet node"):
        ir.Categorical(ir.Ref("P") * 0.5)
    m = ir.Model(T=ir.Stochastic(1, lambda q: ir.Categorical(q), False),
                 q=ir.Stochastic(1, lambda: ir.Beta(1.0, 1.0)))
    m.setsamplers([mb.Slice("q", 0.5)])
    with pytest.raises(mb.ArgumentError, match="the sampled node q is not a Dirichlet node"):
        m.init_matrix([{"T": [1.0, 2.0], "q": [0.4, 0.6]}], 1)
    m = ir.Model(T=ir.Stochastic(1, lambda w: ir.Categorical(w), False), w=ir.Logical(1, lambda q: q * 1.0),
                 q=ir.Stochastic(1, lambda: ir.Dirichlet([1.0, 1.0])))
    m.setsamplers([mb.SliceSimplex("q")])
    with pytest.raises(mb.ArgumentError, match="constant list, a data vector or a sampled Dirichlet node"):
        m.init_matrix([{"T": [1.0, 2.0], "q": [0.4, 0.6]}], 1)


def test_observed_categorical_range_follows_len_p(mb):
    m, inputs, inits = ref.modelA(mb.ir)
    m.setsamplers([mb.SliceSimplex("P")])
    bad = inits(1)
    bad[0]["T"] = [1.0, 4.0]
    with pytest.raises(mb.ArgumentError, match=r"integers in 1\.\.3"):
        m.init_matrix(bad, 1)


# ---------------------------------------------------------------- the lowering
def test_state_read_categorical_encoding_and_targets(mb):
    m, _ = compiled(mb, "C", mb.ir.eyes_scheme())
    I, a = m.ir(), mb.abi
    T, P = I.nodes[m.order.index("T")], I.nodes[m.order.index("P")]
    assert (P.family, P.fixed, P.len) == (a.MMB_IR_DIRICHLET, 0, 2) and list(P.expr) == [-1, -1, -1]
    assert (T.family, T.cterm, T.lo, T.hi) == (a.MMB_IR_CATEGORICAL, -2 - P.off, 1.0, 2.0) and list(T.expr) == [-1] * 3
    pool = np.ctypeslib.as_array(I.pool, shape=(I.npool,))
    assert list(pool[P.cterm:P.cterm + 3]) == [1.0, 1.0, 0.0]  # alpha, lmnB = 2 lgamma(1) - lgamma(2)
    assert m.samplers[3].targets == ["T"] and m.parents["T"] == {"P"}
    B = I.blocks[3]
    assert [m.order[B.term[t]] for t in range(B.nterms)] == ["P", "T"]
    assert m.support["T"] == (1, 2) and m.discrete == ["T"] and m.simplex == ["P"]
    assert set(m.no_predict) == {"T", "P"}


def test_pool_table_categorical_is_unchanged(mb):
    import dgs_ref
    m, inputs, inits = dgs_ref.model2(mb.ir)
    m.setinputs(inputs).setsamplers([mb.DGS("T")])
    m.init_matrix(inits(1), 1)
    I = m.ir()
    T = I.nodes[m.order.index("T")]
    pool = np.ctypeslib.as_array(I.pool, shape=(I.npool,))
    assert T.cterm >= 0 and list(pool[T.cterm:T.cterm + 3]) == dgs_ref.M2_P and m.no_predict == {}


def test_lmnb_in_the_pool(mb):
    m, _ = compiled(mb, "B", [mb.SliceSimplex("P", scale=0.5)])
    I = m.ir()
    P = I.nodes[m.order.index("P")]
    pool = np.ctypeslib.as_array(I.pool, shape=(I.npool,))
    assert list(pool[P.cterm:P.cterm + 32]) == ref.MB_ALPHA
    want = math.fsum(math.lgamma(x) for x in ref.MB_ALPHA) - math.lgamma(math.fsum(ref.MB_ALPHA))
    assert pool[P.cterm + 32] == want == ref.specB().blocks[0][1].lmnb


def test_two_keys_lower_to_one_block_per_node(mb):
    ir = mb.ir
    m = ir.Model(
        Tb=ir.Stochastic(1, lambda b: ir.Categorical(b), False),
        Ta=ir.Stochastic(1, lambda a: ir.Categorical(a), False),
        y=ir.Stochastic(1, lambda a, z: ir.Normal(a[1] + z, 1.0), False),
        a=ir.Stochastic(1, lambda: ir.Dirichlet([1.0, 2.0])),
        z=ir.Stochastic(lambda: ir.Normal(0, 1)),
        b=ir.Stochastic(1, lambda: ir.Dirichlet([3.0, 1.0, 1.0])))
    m.setsamplers([mb.Slice("z", 1.0), mb.SliceSimplex(["b", "a"], scale=0.6)])
    assert [(s.kind, s.params, s.scale) for s in m.samplers[1:]] == [(10, ["b"], 0.6), (10, ["a"], 0.6)]
    m.init_matrix([{"Ta": [1.0, 2.0], "Tb": [3.0, 1.0], "y": [0.1, 0.2], "a": [0.5, 0.5], "z": 0.0,
                    "b": [0.2, 0.3, 0.5]}], 1)
    I = m.ir()
    terms = [[m.order[I.blocks[b].term[t]] for t in range(I.blocks[b].nterms)] for b in range(3)]
    assert terms == [["z", "y"], ["b", "Tb"], ["a", "Ta", "y"]]  # the node, then its targets in topological order
    sp = m.spec()
    assert [(sp.blocks[b].sampler, sp.blocks[b].nnodes, sp.blocks[b].scale, sp.blocks[b].dim) for b in (1, 2)] == \
        [(10, 1, 0.6, 3), (10, 1, 0.6, 2)]


# ---------------------------------------------------------------- the engine's validation (no device needed)
def engine_verdict(mb, m, ir_model=None):
    """(code, message) of the engine's node-IR validation, reached through the entry point that returns the
    specialised kernel's source: a valid model with a Dirichlet node is declined there, with the reason."""
    lib = mb.abi.lib()
    sp, I = m.spec(), ir_model if ir_model is not None else m.ir()
    buf = C.create_string_buffer(1 << 12)
    rc = lib.mmb_ir_jit_source_text(C.byref(sp), C.byref(I), buf, 1 << 12)
    return rc, lib.mmb_last_error(None).decode()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_engine_accepts_and_the_generator_declines(mb, name):
    scheme = {"A": [mb.SliceSimplex("P")], "B": [mb.SliceSimplex("P", scale=0.5)], "C": mb.ir.eyes_scheme()}[name]
    m, _ = compiled(mb, name, scheme)
    rc, msg = engine_verdict(mb, m)
    assert rc == E_UNSUPPORTED and "declines schemes with SliceSimplex blocks" in msg, msg


def test_engine_checks_the_lowered_tables(mb):
    m, _ = compiled(mb, "C", mb.ir.eyes_scheme())
    I = m.ir()
    T, P = I.nodes[m.order.index("T")], I.nodes[m.order.index("P")]
    pool = np.ctypeslib.as_array(I.pool, shape=(I.npool,))

    def broken(msg):
        rc, got = engine_verdict(mb, m, I)
        assert rc == E_ARG and msg in got, got

    keep = T.cterm
    T.cterm = keep - 1  # slots that are not one Dirichlet node's
    broken("slots of one sampled Dirichlet node of length K")
    T.cterm = keep
    T.hi = 3.0  # K differs from len(P)
    broken("slots of one sampled Dirichlet node of length K")
    T.hi = 2.0
    pool[P.cterm] = 0.0
    broken("alpha[0] must be positive")
    pool[P.cterm] = 1.0
    keep = P.cterm
    P.cterm = I.npool - 2  # alpha[2] and lmnB would end past the pool
    broken("needs alpha[len] and lmnB in the pool")
    P.cterm = keep
    I.blocks[3].term[0], I.blocks[3].term[1] = I.blocks[3].term[1], I.blocks[3].term[0]
    broken("its terms are its node, then the node's targets")
    I.blocks[3].term[0], I.blocks[3].term[1] = I.blocks[3].term[1], I.blocks[3].term[0]
    keep = I.blocks[1].term[2]  # [Slice(lambda0, theta)]: lambda0, theta, y
    I.blocks[1].term[2] = m.order.index("T")  # only DGS and SliceSimplex blocks evaluate such a term
    broken("is a term of SliceSimplex and DGS blocks only")
    I.blocks[1].term[2] = keep
    sp = m.spec()
    rc = mb.abi.lib().mmb_ir_jit_source_text(C.byref(sp), C.byref(I), None, 0)
    assert rc == E_UNSUPPORTED  # restored: valid again


# ---------------------------------------------------------------- the restatement on its own
SOLVE_WORST = {"A": 1.94e-14, "B": 1.35e-12}  # measured: the runs below


@pytest.mark.parametrize("name,K,iters", [("A", 8, 200), ("B", 4, 100)])
def test_closed_form_equals_the_solves(mb, prim, name, K, iters):
    """bx after the first simplex and after every shrink against numpy.linalg.solve(V, v), on the GPU tests'
    runs of models A and B.  Measured worst |difference|: 1.94e-14 on A (k = 3, 5840 solves), 1.35e-12 on
    B (k = 32, 8078 solves); the bound is 100 times that.  No update meets the threshold band: the
    condition under which the GPU replays allow at most 2 skips."""
    spec = getattr(ref, "spec" + name)()
    _, _, inits = getattr(ref, "model" + name)(mb.ir)
    solve, near, cands = [], 0, 0
    for c, d in enumerate(inits(K)):
        rows, n, cd = ref.forward(prim, spec, SEED, d["P"], c, iters, solve)
        near += n
        cands += cd
        last = np.array(rows[-1])
        assert last.min() >= 0.0 and abs(last.sum() - 1.0) < 1e-13
    print(f"model {name}: worst |bx - solve(V, v)| {max(solve):.3e} over {len(solve)} solves, "
          f"{cands / (K * iters) - 1.0:.2f} shrinks per update, {near} threshold updates")
    assert max(solve) <= 100.0 * SOLVE_WORST[name]
    assert near == 0


@pytest.mark.parametrize("reverse", [False, True])
def test_no_threshold_updates_on_model_c(mb, prim, reverse):
    """Model C's SliceSimplex block alone (the other blocks' nodes held at a mixed assignment of T), at its
    block index in either scheme order, with the GPU tests' seed and chains: no threshold update."""
    spec = ref.specC(reverse)
    n = len(ref.MC_Y)
    row = [0.0] * (n + 7)
    row[:n] = [1.0, 1.0, 2.0, 2.0, 1.0, 2.0]
    row[n:n + 2] = [0.5, 0.5]
    near = 0
    for c in range(4):
        _, nr, _ = ref.forward(prim, spec, SEED, row, c, 200)
        near += nr
    assert near == 0


def test_restatement_is_stationary_on_model_a(prim):
    """1024 independent chains of the restatement, 30 updates, the last draw only: each coordinate's mean
    within 5 standard errors sqrt(var / 1024) of the exact posterior Dirichlet(alpha + counts)."""
    K, spec = 1024, ref.specA()
    last = np.array([ref.forward(prim, spec, SEED, p, c, 30)[0][-1] for c, p in enumerate(ref._simplex_inits(3, K))])
    a0 = math.fsum(ref.MA_POST)
    for i, a in enumerate(ref.MA_POST):
        mean, var = a / a0, a * (a0 - a) / (a0 * a0 * (a0 + 1.0))
        z = (last[:, i].mean() - mean) / math.sqrt(var / K)
        print(f"P[{i + 1}]: mean {last[:, i].mean():.5f}, exact {mean:.5f}, z = {z:+.2f}")
        assert abs(z) <= 5.0


def test_shrink_keeps_v_inside_and_contracts(prim):
    """After every shrink v = V bx still holds to rounding and bx stays a probability vector."""
    node = ref.specA(0.75).blocks[0][1]
    v = [0.2, 0.5, 0.3]
    key = (SEED, 0, 1, 0)
    bx = ref.draw(prim, key, 0, 3)
    V = ref.first_simplex(v, bx, node.scale)
    np.testing.assert_allclose(ref.matvec(V, bx), v, atol=1e-15)
    np.testing.assert_allclose(V.sum(axis=0), 1.0, atol=1e-15)  # every vertex is on the plane sum = 1
    for r in range(1, 6):
        vol0 = abs(np.linalg.det(V))
        V, bx = ref.shrink(V, bx, ref.draw(prim, key, r, 3))
        assert bx.min() >= 0.0 and abs(bx.sum() - 1.0) < 1e-14
        np.testing.assert_allclose(ref.matvec(V, bx), v, atol=1e-15)
        assert abs(np.linalg.det(V)) < vol0
