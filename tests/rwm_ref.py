"""Restatement of the RWM block update (src/samplers/rwm.jl:65-71) -- the checker of RWM.

Plain Python on the oracle library's primitives only (orc_uniform, orc_normal, orc_sincos2pi,
orc_exp, orc_log: the kernels' own Philox streams and elementary functions).  One update of
block b, chain c (global id), iteration it:

    v    = the block's values unlisted with transform (log of positive nodes)
    x[k] = v[k] + scale[k] * r[k]                         one multiply, one add
    r[k] = normal #k of MMB_SUB_NORMAL (Normal), else symdist(kind, k) on MMB_SUB_PROPOSAL
    accept iff uniform #0 of MMB_SUB_UNIFORM < exp(logpdf!(x) - logpdf!(v))

The two log densities are the oracle's block_logpdf on a TWIN model -- the same model with every
RWM block replaced by AMWG(params, 1.0), which has the same term list and transform = true -- so
they are the oracle's own bits, which the AMWG parity tests assert are the kernels' bits.  Links
are restated from csrc/ir_math.h on orc_log / orc_exp and IEEE operations: identity, log
(positive nodes), logit (Beta: log(x / (1 - x)), 1 / (exp(-y) + 1)) and affine logit (Uniform(lo, hi):
logit((x - lo) / (hi - lo)), (hi - lo) invlogit(y) + lo).
"""
import ctypes as C

import numpy as np

SUB_NORMAL, SUB_UNIFORM, SUB_PROPOSAL = 0, 1, 5
TWOPI_HI = 6.28318530717958623200e+00
NORMAL, SYMUNIFORM, SYMTRIANGULAR, EPANECHNIKOV, BIWEIGHT, TRIWEIGHT, COSINE = range(7)


def symdist(L, kind, seed, chain, it, block, k):
    """Standard variate of coordinate k (csrc/symdist.h restated): u_j = uniform #(8k + j)."""
    u = lambda j: L.orc_uniform(seed, chain, it, block, SUB_PROPOSAL, 8 * k + j)  # noqa: E731
    if kind == SYMUNIFORM:
        return 2.0 * u(0) - 1.0
    if kind == SYMTRIANGULAR:
        return u(0) - u(1)
    if kind in (EPANECHNIKOV, BIWEIGHT, TRIWEIGHT):
        m = kind - EPANECHNIKOV + 1  # the (m + 1)-th smallest of 2m + 1 uniforms
        return 2.0 * sorted(u(j) for j in range(2 * m + 1))[m] - 1.0
    if kind == COSINE:
        u0 = u(0)
        lo, hi = 0.0, 1.0
        s, c = C.c_double(), C.c_double()
        for _ in range(53):
            w = 0.5 * (lo + hi)
            L.orc_sincos2pi(w, C.byref(s), C.byref(c))
            if w - s.value / TWOPI_HI < u0:
                lo = w
            else:
                hi = w
        return 2.0 * (0.5 * (lo + hi)) - 1.0
    raise ValueError(kind)


def cdf(kind, z):
    """Closed-form cdf of the standard SymDistributionType on [-1, 1]."""
    z = np.asarray(z, dtype=np.float64)
    if kind == SYMUNIFORM:
        return (z + 1.0) / 2.0
    if kind == SYMTRIANGULAR:
        return np.where(z < 0.0, (1.0 + z) ** 2 / 2.0, 1.0 - (1.0 - z) ** 2 / 2.0)
    if kind == EPANECHNIKOV:
        return 0.5 + (3.0 * z - z ** 3) / 4.0
    if kind == BIWEIGHT:
        return 0.5 + (15.0 * z - 10.0 * z ** 3 + 3.0 * z ** 5) / 16.0
    if kind == TRIWEIGHT:
        return 0.5 + (35.0 * z - 35.0 * z ** 3 + 21.0 * z ** 5 - 5.0 * z ** 7) / 32.0
    if kind == COSINE:
        return 0.5 * (1.0 + z + np.sin(np.pi * z) / np.pi)
    raise ValueError(kind)


def link(L, kind, x, lo, hi):
    """mmb_ir_link restated (kind 0 identity, 1 log, 2 logit, 3 affine logit)."""
    x, lo, hi = np.float64(x), np.float64(lo), np.float64(hi)
    with np.errstate(all="ignore"):
        if kind == 1:
            return L.orc_log(x)
        if kind == 2:
            return L.orc_log(x / (np.float64(1.0) - x))
        if kind == 3:
            t = (x - lo) / (hi - lo)
            return L.orc_log(t / (np.float64(1.0) - t))
    return float(x)


def invlink(L, kind, y, lo, hi):
    """mmb_ir_invlink restated."""
    lo, hi = np.float64(lo), np.float64(hi)
    with np.errstate(all="ignore"):
        if kind == 1:
            return L.orc_exp(y)
        if kind == 2:
            return float(np.float64(1.0) / (np.float64(L.orc_exp(-y)) + np.float64(1.0)))
        if kind == 3:
            return float((hi - lo) * (np.float64(1.0) / (np.float64(L.orc_exp(-y)) + np.float64(1.0))) + lo)
    return float(y)


def twin_scheme(mb, scheme):
    """The scheme with each RWM block replaced by AMWG(params, 1.0)."""
    return [mb.AMWG(list(s.params), 1.0) if s.kind == mb.abi.MMB_SAMPLER_RWM else s for s in scheme]


class Restatement:
    """RWM updates of `model` (whose RWM blocks the twin holds as AMWG blocks) on canonical value
    rows [K, P].  `scales`: per RWM block index, [K, d] (the tune rows)."""

    def __init__(self, oracle, mb, model, twin, seed, chain_offset=0):
        self.L, self.mb, self.m, self.twin = oracle.L, mb, model, twin
        self.seed, self.off = int(seed), int(chain_offset)
        oracle._ir(twin)
        self.spec = twin.spec()
        self.arrs, self.ptrs, self.ns = oracle._data(twin)
        self.oracle = oracle
        self.blocks = []
        a = mb.abi
        for b, s in enumerate(model.samplers):
            idx, pos = [], []          # pos: per element (link kind, lo, hi)
            for p in s.params:
                n = model.nodes[p]
                tr = getattr(model, "traced", None)
                fam = tr[p].fam if tr is not None and p in tr else None
                lk = (1 if n.positive else 0, 0.0, 0.0)
                if fam == a.MMB_IR_BETA:
                    lk = (2, 0.0, 0.0)
                elif fam == a.MMB_IR_UNIFORM:
                    N = model.ir().nodes[n.id]     # the node named p: its id, checked against its layout
                    assert (N.family, N.off, N.len, N.fixed) == (fam, n.offset, n.dim, 0), p
                    lk = (3, float(N.lo), float(N.hi))
                idx += list(range(n.offset, n.offset + n.dim))
                pos += [lk] * n.dim
            self.blocks.append((s, np.array(idx), pos))
        self.updates = {b: 0 for b, s in enumerate(model.samplers) if s.kind == mb.abi.MMB_SAMPLER_RWM}
        self.accepts = dict(self.updates)
        self.chain_accepts = {}  # (block, chain) -> accepted updates

    def scales0(self, K):
        out = {}
        for b, (s, idx, _) in enumerate(self.blocks):
            if s.kind == self.mb.abi.MMB_SAMPLER_RWM:
                out[b] = np.tile(s.spec_tuning(len(idx)), (K, 1))
        return out

    def logpdf(self, values, b, x):
        dp = C.POINTER(C.c_double)
        self.oracle._ir(self.twin)  # (the oracle holds one lowered IR at a time)
        xx = np.ascontiguousarray(x, dtype=np.float64)
        return self.L.orc_block_logpdf(C.byref(self.spec), self.ptrs, self.ns, values.ctypes.data_as(dp), b,
                                       xx.ctypes.data_as(dp))

    def update(self, row, b, chain, it, scale):
        """One RWM update of block b on the value row (in place).  Returns whether it accepted."""
        s, idx, pos = self.blocks[b]
        L, d = self.L, len(idx)
        v = np.array([link(L, p[0], row[i], p[1], p[2]) for i, p in zip(idx, pos)])
        g = self.off + chain
        x = np.empty(d)
        for k in range(d):
            r = (L.orc_normal(self.seed, g, it, b, SUB_NORMAL, k) if s.form == NORMAL
                 else symdist(L, s.form, self.seed, g, it, b, k))
            x[k] = v[k] + scale[k] * r
        lx = self.logpdf(row, b, x)
        lv = self.logpdf(row, b, v)
        acc = L.orc_uniform(self.seed, g, it, b, SUB_UNIFORM, 0) < L.orc_exp(lx - lv)
        self.updates[b] += 1
        self.accepts[b] += int(acc)
        self.chain_accepts[(b, chain)] = self.chain_accepts.get((b, chain), 0) + int(acc)
        if acc:
            v = x
        for q, (i, p) in enumerate(zip(idx, pos)):
            row[i] = invlink(L, p[0], v[q], p[1], p[2])
        return acc

    def monitored(self, row):
        """sim[i, :, 1] = unlist(m, true) of one chain: the monitored columns of a value row."""
        m = self.m
        col = {}
        for n in m.nodes.values():
            for i in range(n.dim):
                col[n.name if n.dim == 1 else f"{n.name}[{i + 1}]"] = row[n.offset + i]
                col[f"{n.name}[{i + 1}]"] = row[n.offset + i]
        out = []
        for name in m.monitor_names:
            if name in col:
                out.append(col[name])
            elif name == "alpha0":  # rats.jl:65-67: mu_alpha - xbar * mu_beta
                inp = m.inputs
                xbar = float(inp["xbar"][0]) if "xbar" in inp else float(np.sum(inp["x"]) / 5.0)
                out.append(col["mu_alpha"] - xbar * col["mu_beta"])
            else:
                raise NotImplementedError(f"monitored column {name}")
        return out

    def run(self, values, iters, burnin=0, thin=1, scales=None, it0=0, nblocks=None):
        """Sweeps of a scheme whose (first `nblocks`) blocks are all RWM, on values [K, P] in place.
        Returns the kept draws [n, p, K] (Chains order)."""
        K = values.shape[0]
        scales = self.scales0(K) if scales is None else scales
        nb = len(self.blocks) if nblocks is None else nblocks
        for b in range(nb):
            if self.blocks[b][0].kind != self.mb.abi.MMB_SAMPLER_RWM:
                raise NotImplementedError("the restatement sweeps RWM blocks only")
        kept = []
        for it in range(it0 + 1, it0 + iters + 1):
            for c in range(K):
                for b in range(nb):
                    self.update(values[c], b, c, it, scales[b][c])
            if it > burnin and (it - burnin) % thin == 0:
                kept.append([self.monitored(values[c]) for c in range(K)])
        if not kept:
            return None
        return np.asfortranarray(np.transpose(np.array(kept), (0, 2, 1)))

    def stats(self):
        return {b: {"updates": self.updates[b], "accepts": self.accepts[b]} for b in self.updates}

    def tune(self, scales, K):
        """The engine's tune rows [K, tune_len] of an all-RWM scheme."""
        return np.concatenate([scales[b] for b in sorted(scales)], axis=1) if scales else np.zeros((K, 0))
