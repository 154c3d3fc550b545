"""BHMC (src/samplers/bhmc.jl:50-122) restated in plain Python: the checker of tests/test_gpu_bhmc.py, in the style of
tests/binary_ref.py, whose models, BNode and DELTA it shares.

One update of a chain's particle, tune row [position[n], velocity[n], wallhits, wallcrosses, initialised]:

    initialise  a row whose `initialised` is 0: position_i = normal #i, velocity_i = normal #(32 + i) of the
                block's SUB_INIT stream of (seed, global chain, iteration, block)
    refresh     (an extension) velocity_i = normal #i of the block's SUB_NORMAL stream, at the start of every update
    sides       S_i = +1 iff position_i > 0, else -1; the configuration x_i = (S_i + 1) / 2
    event loop  walltime_i = phi > 0 ? pi - phi : -phi, phi = atan2(position_i, velocity_i); the element j that hit
                last gets +Inf within 1e4 eps of 0 or 2 pi; (movetime, j) = the minimum, ties to the lowest index; an
                Inf movetime is pi; totaltime += movetime, and once totaltime >= traveltime the move is cut to end at
                traveltime and is the last; every element rotates by movetime; at a wall position_j = 0,
                v2 = velocity_j^2 + sign(velocity_j) 2 (logf(x | x_j = 1) - logf(x | x_j = 0)), v2 > 0 crosses at
                sqrt(v2), anything else (a NaN too) reflects
    stall       a zero movetime, a NaN walltime, or cap = n (floor(traveltime / pi) + 2) trips of the loop without
                reaching traveltime: the update ends with the value and the whole row as they were
    value       x_i = 1 iff position_i > 0

Of the two configurations at a wall one is the current one, whose logf is carried (as the device does); the values
are those of the reference's two evaluations because logf is a function of the state.

The arithmetic comes from an `ops` object: PyOps is math.atan2 / sin / cos, the reference for the replay; HostOps calls
csrc/bhmc.h compiled by the host C compiler, which is the text the kernels compile, so with a log-density difference
that is exactly 0 on both sides (a flat density) its rows are the device's bit for bit.

Decisions (PyOps) go through BDec: the arg-min, totaltime >= traveltime, v2 > 0 and the final sign are "near" within
DELTA of their thresholds (binary_ref's reasoning: the log densities are within about 1e-10 of exact, the angles
within a few ulps); the two last-hit guards compare against 1e4 eps, far below DELTA, and are near only within DELTA
relative to that: the guarded element's position is the exact zero written at its hit, so its walltime is an exact 0
on both sides and the guard's outcome is no rounding question.  At a near decision the device may go either way:
the replay explores both and counts a skip.
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import binary_ref as br
from dgs_ref import DELTA, normal_lp

SUB_NORMAL, SUB_INIT = 0, 4
NEARZERO = 1e4 * 2.220446049250313e-16
INF = math.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def event_cap(n, T):
    return n * (int(math.floor(T / math.pi)) + 2)


def event_bound(n, T):
    """An element meets its wall once per pi of time: at most n (floor(T / pi) + 1) events in an update."""
    return n * (int(math.floor(T / math.pi)) + 1)


class BDec(br.Dec):
    def lt(self, u, t, delta=DELTA):
        natural = u < t
        if not abs(u - t) <= delta:
            return natural
        i = len(self.nears)
        self.nears.append(self.forced[i] if i < len(self.forced) else natural)
        return self.nears[i]


def explore(step, forced=()):
    d = BDec(forced)
    outs = [step(d)]
    for i in range(len(forced), len(d.nears)):
        outs += explore(step, tuple(d.nears[:i]) + (not d.nears[i],))
    return outs


def sign(x):
    return 1.0 if x > 0.0 else (-1.0 if x < 0.0 else x)


class PyOps:
    def walltime(self, v, p):
        phi = math.atan2(p, v)
        return math.pi - phi if phi > 0.0 else -phi

    def guard(self, w, dec):
        if dec.lt(abs(w), NEARZERO, DELTA * NEARZERO) or dec.lt(abs(w - 2.0 * math.pi), NEARZERO, DELTA * NEARZERO):
            return INF
        return w

    def sincos(self, t):
        return math.sin(t), math.cos(t)

    def move(self, a, b, s, c):
        return a * c - b * s, a * s + b * c

    def bounce(self, v, dl, dec):
        sg = sign(v)
        v2 = v * v + sg * 2.0 * dl
        if dec.lt(0.0, v2):
            return math.sqrt(v2) * sg, True
        return v * -1.0, False


HOST_SRC = r"""
#include "bhmc.h"
double h_atan2(double y, double x) { return mmb_atan2(y, x); }
void h_sincos(double x, double* s, double* c) { mmb_sincos(x, s, c); }
double h_walltime(double v, double p) { return mmb_bhmc_walltime(v, p); }
double h_guard(double w) { return mmb_bhmc_guard(w); }
void h_move(double a, double b, double s, double c, double* a1, double* b1) { mmb_bhmc_move(a, b, s, c, a1, b1); }
double h_bounce(double v, double dl, int* crossed) { return mmb_bhmc_bounce(v, dl, crossed); }
"""


def host_lib(tmp):
    """csrc/bhmc.h compiled by the host C compiler as tests/test_rwm.py compiles symdist.h."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler: the oracle itself could not have been built")
    src, so = os.path.join(str(tmp), "bhmc_host.c"), os.path.join(str(tmp), "libbhmchost.so")
    with open(src, "w") as f:
        f.write(HOST_SRC)
    subprocess.run([cc, "-O2", "-std=c99", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, "mamba.jl_amd", "csrc"), src, "-o", so, "-lm"], check=True)
    L = C.CDLL(so)
    D, PD = C.c_double, C.POINTER(C.c_double)
    for name, res, args in [("h_atan2", D, [D, D]), ("h_sincos", None, [D, PD, PD]), ("h_walltime", D, [D, D]),
                            ("h_guard", D, [D]), ("h_move", None, [D, D, D, D, PD, PD]),
                            ("h_bounce", D, [D, D, C.POINTER(C.c_int)])]:
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


class HostOps:
    """The per-element functions of csrc/bhmc.h; its comparisons are the header's own (no near band)."""

    def __init__(self, L):
        self.L = L

    def walltime(self, v, p):
        return self.L.h_walltime(v, p)

    def guard(self, w, dec):
        return self.L.h_guard(w)

    def sincos(self, t):
        s, c = C.c_double(), C.c_double()
        self.L.h_sincos(t, C.byref(s), C.byref(c))
        return s.value, c.value

    def move(self, a, b, s, c):
        a1, b1 = C.c_double(), C.c_double()
        self.L.h_move(a, b, s, c, C.byref(a1), C.byref(b1))
        return a1.value, b1.value

    def bounce(self, v, dl, dec):
        cr = C.c_int()
        return self.L.h_bounce(v, dl, C.byref(cr)), bool(cr.value)


class Out:
    """One update's outcome: value (None: stalled, the node keeps its value), the new row, the events."""

    def __init__(self, value, done, row, hits, crosses, why="", infspeed=0):
        self.value, self.done, self.row, self.hits, self.crosses, self.why = value, done, row, hits, crosses, why
        self.infspeed = infspeed  # wall crossings that left at infinite speed


def bhmc_step(logf, n, row, T, refresh, zi, zr, dec, ops):
    """logf(x) -> logpdf!(block, x); row the pre-update tune row; zi(k) / zr(k) normal #k of the block's SUB_INIT /
    SUB_NORMAL stream."""
    pos, vel = [float(v) for v in row[:n]], [float(v) for v in row[n:2 * n]]
    if row[2 * n + 2] == 0.0:
        pos, vel = [zi(i) for i in range(n)], [zi(32 + i) for i in range(n)]
    if refresh:
        vel = [zr(i) for i in range(n)]
    x = [1.0 if p > 0.0 else 0.0 for p in pos]
    lf = logf(x)
    total, j, hits, crosses, done, why, infspeed = 0.0, -1, 0, 0, False, "cap", 0
    for _ in range(event_cap(n, T)):
        w = [ops.walltime(vel[i], pos[i]) for i in range(n)]
        if j >= 0:
            w[j] = ops.guard(w[j], dec)
        if any(t != t for t in w):
            why = "nan"
            break
        jj = 0
        for k in range(1, n):
            if dec.lt(w[k], w[jj]):
                jj = k
        mt = w[jj]
        if mt == 0.0:
            why = "zero"
            break
        j = jj
        if mt == INF:
            mt = math.pi
        total = total + mt
        last = not dec.lt(total, T)
        if last:
            mt = mt - (total - T)
        s, c = ops.sincos(mt)
        for i in range(n):
            vel[i], pos[i] = ops.move(vel[i], pos[i], s, c)
        if last:
            done = True
            break
        hits += 1
        pos[j] = 0.0
        y = list(x)
        y[j] = 1.0 - x[j]
        lo = logf(y)
        vel[j], crossed = ops.bounce(vel[j], lf - lo if x[j] == 1.0 else lo - lf, dec)
        if crossed:
            x, lf = y, lo
            crosses += 1
            infspeed += math.isinf(vel[j])
    if not done:
        return Out(None, False, [float(v) for v in row], hits, crosses, why, infspeed)
    value = [1.0 if dec.lt(0.0, p) else 0.0 for p in pos]
    return Out(value, True, pos + vel + [row[2 * n] + hits, row[2 * n + 1] + crosses, 1.0], hits, crosses, "", infspeed)


def row_gap(have, want, n):
    """Largest |have - want| over the 2 n positions and velocities, relative to the largest magnitude among want's
    (the particle's size: an element near its wall has a position near 0, so elementwise ratios say nothing).
    Entries equal on both sides (infinities too) or NaN on both count 0; otherwise a non-finite entry counts Inf."""
    scale = max([abs(v) for v in want[:2 * n] if math.isfinite(v)] + [1e-300])
    gap = 0.0
    for h, w in zip(have[:2 * n], want[:2 * n]):
        if h == w or (h != h and w != w):
            continue
        gap = max(gap, abs(h - w) / scale if math.isfinite(h) and math.isfinite(w) else INF)
    return gap


def energy(logf, row, n):
    pos, vel = row[:n], row[n:2 * n]
    return 0.5 * math.fsum(p * p + v * v for p, v in zip(pos, vel)) - logf([1.0 if p > 0.0 else 0.0 for p in pos])


def sign_changes(b0, a0, t):
    """Sign changes of b0 cos s + a0 sin s = r sin(s + phi0) over 0 < s <= t, phi0 = atan2(b0, a0)."""
    phi0 = math.atan2(b0, a0)
    return int(math.floor((t + phi0) / math.pi)) - int(math.floor(phi0 / math.pi))


# ------------------------------------------------------------------ models
# binary_ref's S3, S6, S32, S1 and MIX, and EDGE: S3 with its second column scaled by 1e200, so that gamma_2 = 1 puts
# every mean beyond the range of a double's square: logf = -Inf there.  At gamma_2's wall the log-density difference is
# -Inf: coming from the 0 side (velocity > 0) v2 = -Inf reflects, coming from the 1 side (velocity < 0) v2 = +Inf
# crosses at infinite speed, after which Inf - Inf in the next moves gives NaN walltimes and the update stalls.  With
# gamma_2 = 1 every other element's difference is -Inf - -Inf = NaN, which reflects.
EDGE = br.Data(3, 101, [0.35, -0.3, 0.25], {0, 2}, scale=[1.0, 1e200, 1.0])
DATA = dict(S3=br.S3, S6=br.S6, S32=br.S32, S1=br.S1, MIX=br.MIX, EDGE=EDGE)

# The replay cases of tests/test_gpu_bhmc.py: (data, traveltime / pi, mixed, BHMC block first); 8 chains, 25 iterations
K_REPLAY, ITERS_REPLAY, SEED = 8, 25, 11
REPLAY_CASES = [("S6", 12.5, False, True), ("S32", 2.5, False, True), ("S1", 2.5, False, True),
                ("MIX", 2.5, True, True), ("MIX", 2.5, True, False), ("EDGE", 2.5, False, True)]
# measured by tests/test_bhmc.py::test_summation_gap over these cases, refresh both ways: the largest gap between
# the restatement with its log densities summed by math.fsum and summed naively in reversed term order, one update
# from the same row; the replay allows 100 times it (the device's summation order is a third one)
SUMMATION_GAP = 2.4e-13
POS_TOL = 100.0 * SUMMATION_GAP


def logf_of(D, mixed=False, naive=False):
    """binary_ref.logf_of; naive: the same terms summed one by one in reversed order, not by math.fsum."""
    if not naive:
        return br.logf_of(D, mixed)

    def rsum(ts):
        s = 0.0
        for t in reversed(list(ts)):
            s = s + t
        return s

    def logf(st):
        g = st["gamma"]
        coef = st["beta"] if mixed else D.b0
        sd = math.sqrt(st["s2"][0]) if mixed else 1.0
        terms = [math.log(0.5)] * D.n
        on = [j for j in range(D.n) if g[j] != 0.0]
        for i in range(br.NOBS):
            terms.append(normal_lp(D.y[i], rsum(D.X[j][i] * coef[j] * g[j] for j in on), sd))
        return rsum(terms)
    return logf


def spec(dn, mixed=False, first=True, naive=False):
    D = DATA[dn]
    sp = br.spec(D, "bhmc", 1, mixed, first)
    node = next(w for k, w in sp.blocks if k == "bin")
    node._logf = logf_of(D, mixed, naive)
    return sp


def inits_of(dn, inits):
    """EDGE: chains start with gamma_2 = 0 (a finite log density); BHMC itself never reads the node's value."""
    def f(K):
        out = inits(K)
        if dn == "EDGE":
            for d in out:
                d["gamma"][1] = 0.0
        return out
    return f


def tune_offset(sp, bhmc_block):
    """Offset of the BHMC block's row in the chain's tune row: MIX's RWM(beta) block holds scale[3], Slice nothing."""
    off = 0
    for b, (kind, what) in enumerate(sp.blocks):
        if b == bhmc_block:
            return off
        off += 3 if what == ["beta"] else 0
    raise ValueError(bhmc_block)


class Replay:
    """Replays every update of the BHMC block from the device's own pre-update row: draws[t, column, chain] (thin 1,
    burnin 0, every sampled node monitored), tunes[t][chain] the chain's whole tune row before iteration t + 1
    (t = 0: after init_chains) and tunes[t + 1] after it."""

    def __init__(self, orc_normal, sp, seed, T, refresh, chain_offset=0, ops=None):
        self.z, self.sp, self.seed, self.T, self.refresh, self.off = orc_normal, sp, seed, T, refresh, chain_offset
        self.ops = ops or PyOps()
        self.b = next(b for b, (k, _) in enumerate(sp.blocks) if k == "bin")
        self.node = sp.blocks[self.b][1]
        self.toff = tune_offset(sp, self.b)
        self.skips = self.updates = self.done = self.stalls = self.events = self.infspeed = 0
        self.mismatch, self.gap, self.why = [], 0.0, {}
        self.helper = br.Replay(None, sp, seed)

    def step(self, st, row, c, it):
        n = self.node.n
        zi = lambda k: self.z(self.seed, self.off + c, it, self.b, SUB_INIT, k)  # noqa: E731
        zr = lambda k: self.z(self.seed, self.off + c, it, self.b, SUB_NORMAL, k)  # noqa: E731
        logf = lambda x: self.node.logf(st, x)  # noqa: E731
        return explore(lambda d: bhmc_step(logf, n, row, self.T, self.refresh, zi, zr, d, self.ops))

    def chain(self, c, init_row, draws, tunes, it0=0):
        n, w = self.node.n, 2 * self.node.n + 3
        st = self.helper.state(init_row)
        for t in range(draws.shape[0]):
            dev = self.helper.state(draws[t, :, c])
            for b, (kind, what) in enumerate(self.sp.blocks):
                if kind != "bin":
                    for nm in what:
                        st[nm] = list(dev[nm])
                    continue
                self.updates += 1
                pre = [float(v) for v in tunes[t][c][self.toff:self.toff + w]]
                have = [float(v) for v in tunes[t + 1][c][self.toff:self.toff + w]]
                got = dev[what.name]
                outs = self.step(st, pre, c, it0 + t + 1)
                ok = [o for o in outs if (o.value if o.done else st[what.name]) == got and o.row[2 * n:] == have[2 * n:]]
                if not ok:
                    self.mismatch.append((c, it0 + t + 1, got, have[2 * n:], outs[0].value, outs[0].row[2 * n:], outs[0].why))
                    hit = outs[0]
                else:
                    hit = min(ok, key=lambda o: row_gap(have, o.row, n))
                    if hit is not outs[0]:
                        self.skips += 1
                    self.gap = max(self.gap, row_gap(have, hit.row, n))
                self.done += hit.done
                self.stalls += not hit.done
                self.events += hit.hits
                self.infspeed += hit.infspeed
                if not hit.done:
                    self.why[hit.why] = self.why.get(hit.why, 0) + 1
                st[what.name] = list(got)
        return st

    def run(self, init, draws, tunes, it0=0):
        for c in range(draws.shape[2]):
            self.chain(c, init[c], draws, tunes, it0)
        return self


def forward(orc_normal, sp, seed, init_row, chain, iters, T, refresh, ops=None, row=None, each=None):
    """The restatement alone on a binary-only scheme from a fresh (uninitialised) row: (value rows, tune rows after
    each update, near decisions met, outcomes); each(st, pre_row, out): a hook after every update."""
    R = Replay(orc_normal, sp, seed, T, refresh, ops=ops)
    n = R.node.n
    st = R.helper.state(init_row)
    row = [0.0] * (2 * n + 3) if row is None else list(row)
    near, values, rows, outs = 0, [], [], []
    for t in range(iters):
        d = BDec()
        zi = lambda k: orc_normal(seed, chain, t + 1, R.b, SUB_INIT, k)  # noqa: E731
        zr = lambda k: orc_normal(seed, chain, t + 1, R.b, SUB_NORMAL, k)  # noqa: E731
        o = bhmc_step(lambda x: R.node.logf(st, x), n, row, T, refresh, zi, zr, d, R.ops)
        if each is not None:
            each(st, row, o, zi, zr)
        near += len(d.nears)
        if o.done:
            st[R.node.name] = list(o.value)
        row = list(o.row)
        values.append(list(st[R.node.name]))
        rows.append(row)
        outs.append(o)
    return values, rows, near, outs
