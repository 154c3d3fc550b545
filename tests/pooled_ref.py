"""pooled_ref.py -- extended-precision restatement of the pooled post-processing kernels
(TEST INFRASTRUCTURE ONLY): the Gelman-Rubin sums and the range of gr.hip, the per-chain summary
partials and the order statistics of summary.hip, on an n x p x K draw array.

Independent of the product and of the other restatements: plain numpy in np.longdouble (64-bit
mantissa on x86-64; the module refuses to load where it is narrower), nothing imported from
mamba.jl_amd or oracle/.  tests/test_pooled_ref.py pins it on the CPU against hand-computable
cases, oracle/summary_ref.py, gelman.gelmandiag and the host shard of tests/test_summary.py before
tests/test_gpu_pooled.py holds the device kernels to it.

Every sum comes with its SCALE: the sum of the absolute values of the terms that were added, the
quantity a floating-point summation error is proportional to (|fl(sum t) - sum t| <= (N - 1) u
sum |t| for N terms in any order, u = 2^-53).  The device tests ask |got - ref| <= 1e-10 scale.
How far down "the terms" go is stated per function; the rule is that a term is a quantity the
kernel obtains with a relative error of a few u, so that the bound is sound for a correct kernel
(1e-10 is about 2^20 u: room for sums of 2^15 terms and the few roundings per term) while a wrong
term, a dropped or doubled element or a wrong divisor moves an entry by far more than 1e-10 of it.

The crafted inputs of the device tests live here too (the *_inputs functions), so that the CPU
test can assert their stated properties and both files see the same arrays.
"""
import itertools

import numpy as np

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise ImportError("pooled_ref needs an extended-precision np.longdouble (64-bit mantissa)")


# ------------------------------------------------------------------ Gelman-Rubin sums (gr.hip)
def link(x, kind):
    """Mamba's link on float64 draws, in extended precision: log x, log(x / (1 - x)) (utils.jl:67)."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    if kind == 1:
        return np.log(x)
    if kind == 2:
        return np.log(x / (LD(1) - x))
    return x


def link_kinds(mm):
    """link(c) (chains.jl:237-246) from a p x 2 [min, max] table: 1 (log) when the minimum is
    positive, 2 (logit) when the maximum is also below one, 0 (identity) otherwise."""
    return np.array([0 if not lo > 0.0 else (2 if hi < 1.0 else 1) for lo, hi in np.asarray(mm)], dtype=np.int32)


def mid_shift(x, kinds):
    """The shift gelmandiag takes: the link of the mid-range, in float64 (the host's expression)."""
    mm = minmax(x)
    mid = 0.5 * (mm[:, 0] + mm[:, 1])
    sh = mid.copy()
    k = np.asarray(kinds)
    sh[k == 1] = np.log(mid[k == 1])
    sh[k == 2] = np.log(mid[k == 2] / (1.0 - mid[k == 2]))
    return sh


def gr_sums(x, kinds, shift):
    """(L, scale): the L-vector [m, sum phi (p), sum phi phi' (p p), sum S2 (p p), sum s2^2 (p),
    sum s2 phi (p), sum s2 phi^2 (p)] of include/mamba_hip.h mmb_gr_partials, sums over chains of
    phi_k = mean_k - shift and S2_k = the chain's covariance (divisor n - 1) of the linked draws
    y, both np.longdouble; and per entry the scale of the module docstring.

    Terms.  A chain mean is a sum of n terms y_i / n (the y carry the link's rounding, relative),
    phi adds the term -shift: A_kj = sum_i |y_ijk| / n + |shift_j| is the scale of phi_kj, and
    phi may be far smaller than it (a level of 1e8 under a shift of 1e8).  Products of phi take the
    products of these scales.  The covariance is two-pass: its terms are the products d_ij d_il /
    (n - 1) of the deviations d = y - mean; an error dm of the mean enters S2 only as n dm_j dm_l /
    (n - 1), second order in u, because the deviations about the exact mean sum to zero.  So
      sum phi: sum_k A_kj;  sum phi phi': sum_k A_kj A_kl;  sum S2: sum_k sum_i |d_ij d_il| / (n - 1);
      sum s2^2: sum_k s2_kj^2;  sum s2 phi: sum_k s2_kj A_kj;  sum s2 phi^2: sum_k s2_kj A_kj^2
    (s2 is a sum of positive terms: it is its own scale).  Entry 0 counts chains and is exact."""
    x = np.asarray(x, dtype=np.float64)
    n, p, K = x.shape
    y = np.stack([link(x[:, j, :], int(kinds[j])) for j in range(p)], axis=1)       # n x p x K
    sh = np.asarray(shift, dtype=np.float64).astype(LD)
    # centred on the first linked draw before anything is summed (a level of 1e8 keeps its spread
    # well inside the 64-bit mantissa)
    c = y[0, :, 0].copy()
    yc = y - c[None, :, None]
    meanc = yc.sum(0) / LD(n)                                                        # p x K
    phi = meanc + (c - sh)[:, None]
    A = np.abs(y).sum(0) / LD(n) + np.abs(sh)[:, None]
    d = yc - meanc[None]
    S2 = np.einsum("ijk,ilk->jlk", d, d) / LD(n - 1)                                 # p x p x K
    S2a = np.einsum("ijk,ilk->jlk", np.abs(d), np.abs(d)) / LD(n - 1)
    s2 = np.einsum("jjk->jk", S2)
    L = np.concatenate([[LD(K)], phi.sum(1), np.einsum("jk,lk->jl", phi, phi).ravel(), S2.sum(2).ravel(),
                        (s2 * s2).sum(1), (s2 * phi).sum(1), (s2 * phi * phi).sum(1)])
    scale = np.concatenate([[LD(0)], A.sum(1), np.einsum("jk,lk->jl", A, A).ravel(), S2a.sum(2).ravel(),
                            (s2 * s2).sum(1), (s2 * A).sum(1), (s2 * A * A).sum(1)])
    return L, scale


def minmax(x):
    """p x 2 [min, max] of each column over iterations and chains (float64, exact)."""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([x.min(axis=(0, 2)), x.max(axis=(0, 2))], axis=1)


# ------------------------------------------------------------------ chain summaries (summary.hip)
FIELDS = ("s1", "q", "B1", "B2", "nfull", "hsum", "hcnt", "tsum", "tcnt", "pad")


def chain_partials(x, kg, bs, shift):
    """(out, scale), both K x p x 10 np.longdouble: the fields [s1, q, B1, B2, nfull, hsum, hcnt,
    tsum, tcnt, 0] of mmb_chain_summary for chains with global ids kg (chain kg occupies the flat
    positions kg n .. kg n + n - 1 of vec(x); batch b the positions b bs .. b bs + bs - 1).
    With x' = x - shift: s1 = sum x', q = sum x'^2; over the batches lying wholly inside the
    chain B1 = sum d_b, B2 = sum d_b^2, d_b = (sum of the batch's x') / bs, nfull their number;
    the piece of a batch begun in an earlier chain is the head (hsum, hcnt), the piece of one that
    runs on into the next chain the tail (tsum, tcnt); a chain lying inside one batch without
    starting it is all head.

    Terms.  x' is one IEEE subtraction, relative error u whatever cancels in it, so the terms are
    the x' themselves: scale s1 = sum |x'|, q = sum x'^2, B1 = sum_b (sum |x'|) / bs,
    B2 = sum_b ((sum |x'|) / bs)^2, hsum / tsum = sum |x'| over the piece.  The counts are exact
    integers (scale 0)."""
    x = np.asarray(x, dtype=np.float64)
    n, p, K = x.shape
    bs = int(bs)
    xs = x.astype(LD) - np.asarray(shift, dtype=np.float64).astype(LD)[None, :, None]
    out = np.zeros((K, p, 10), dtype=LD)
    scale = np.zeros((K, p, 10), dtype=LD)
    for k in range(K):
        v = xs[:, :, k]                                                  # n x p
        a = np.abs(v)
        t0 = int(kg[k]) * n
        out[k, :, 0], scale[k, :, 0] = v.sum(0), a.sum(0)
        out[k, :, 1] = scale[k, :, 1] = (v * v).sum(0)
        first = -(-t0 // bs) * bs - t0                                   # offset of the first batch start >= t0
        starts = np.unique(np.concatenate([[0], np.arange(first, n, bs)])).astype(np.int64)
        ends = np.append(starts[1:], n)
        seg = np.add.reduceat(v, starts, axis=0)                         # nseg x p
        sega = np.add.reduceat(a, starts, axis=0)
        for s, (i0, i1) in enumerate(zip(starts, ends)):
            begins = (t0 + i0) % bs == 0
            closes = (t0 + i1) % bs == 0
            if begins and closes:
                continue
            f = 5 if not begins else 7                                   # head / tail: [sum, count]
            out[k, :, f], scale[k, :, f] = seg[s], sega[s]
            out[k, :, f + 1] = i1 - i0
        full = ((t0 + starts) % bs == 0) & ((t0 + ends) % bs == 0)
        db, da = seg[full] / LD(bs), sega[full] / LD(bs)
        out[k, :, 2], scale[k, :, 2] = db.sum(0), da.sum(0)
        out[k, :, 3], scale[k, :, 3] = (db * db).sum(0), (da * da).sum(0)
        out[k, :, 4] = int(full.sum())
    return out, scale


def summarystats(x, bs):
    """p x 5 float64 [Mean, SD, Naive SE, MCSE, ESS] of summarystats(c; etype=:bm)
    (stats.jl:85-94, mcse.jl:10-19) from np.longdouble sums over vec(x) (chains concatenated):
    SD = sqrt(sum (x - mean)^2 / (N - 1)), Naive SE = SD / sqrt(N), MCSE = the same standard error
    of the means of the N // bs full batches, ESS = min((SD / MCSE)^2, n); N // bs < 2 is an
    error there and a ValueError here.  A constant column gives SD = MCSE = 0 and ESS NaN."""
    x = np.asarray(x, dtype=np.float64)
    n, p, K = x.shape
    N, m = n * K, (n * K) // int(bs)
    if m < 2:
        raise ValueError(f"iterations are < {2 * bs} and batch size is > {N // 2}")
    out = np.empty((p, 5))
    for j in range(p):
        # centred on the first draw before anything is summed: the spread of a column at 1e9 would
        # otherwise sit in the last bits even of a 64-bit mantissa
        c = LD(x[0, j, 0])
        v = x[:, j, :].ravel(order="F").astype(LD) - c
        mu = v.sum() / LD(N)
        sd = np.sqrt(((v - mu) ** 2).sum() / LD(N - 1))
        mb = v[:m * bs].reshape(m, bs).sum(1) / LD(bs)
        mcse = np.sqrt(((mb - mb.sum() / LD(m)) ** 2).sum() / LD(m - 1)) / np.sqrt(LD(m))
        with np.errstate(invalid="ignore", divide="ignore"):
            ess = np.minimum((sd / mcse) ** 2, LD(n))
        out[j] = [c + mu, sd, sd / np.sqrt(LD(N)), mcse, ess]
    return out


# ------------------------------------------------------------------ order statistics
def order_stats(x, j, ranks):
    """The 0-based order statistics `ranks` of column j pooled over iterations and chains."""
    v = np.sort(np.asarray(x, dtype=np.float64)[:, j, :].ravel())
    return v[np.asarray(ranks, dtype=np.int64)]


def quantile_ranks(N, q):
    """The 0-based ranks Julia 0.5's quantile! reads for probabilities q of N sorted values."""
    index = 1.0 + (N - 1) * np.asarray(q, dtype=np.float64)
    return sorted(set((np.floor(index).astype(np.int64) - 1).tolist())
                  | set((np.ceil(index).astype(np.int64) - 1).tolist()))


def quantile(x, q):
    """p x len(q): quantile(c; q) (stats.jl:73-80) by Julia 0.5 Base.quantile! on the pooled sorted
    column, in float64 and in the host's own expression -- index = 1 + (N - 1) q, lo = floor,
    h = index - lo, v[lo] where the index is integral, else (1 - h) v[lo] + h v[hi] -- so that the
    comparison is exact."""
    x = np.asarray(x, dtype=np.float64)
    n, p, K = x.shape
    N = n * K
    q = np.asarray(q, dtype=np.float64)
    index = 1.0 + (N - 1) * q
    lo = np.floor(index).astype(np.int64)
    hi = np.ceil(index).astype(np.int64)
    h = index - lo
    out = np.empty((p, q.size))
    for j in range(p):
        v = np.sort(x[:, j, :].ravel())
        for t in range(q.size):
            a, b = v[lo[t] - 1], v[hi[t] - 1]
            out[j, t] = a if index[t] == lo[t] else (1.0 - h[t]) * a + h[t] * b
    return out


# ------------------------------------------------------------------ crafted inputs: Gelman-Rubin sums
GR_SMALL_MAX, GR_BIG_MAX, GR_BIG_CHAINS, GR_TI = 4, 64, 16, 32          # gr.hip's constants
GR_SHAPES = [(p, K) for p in (1, 2, 4) for K in (2, 255, 257)] + [(5, 15), (5, 17), (64, 33)]
GR_LENGTHS = (2, 31, 33, 65)
CONSTANT_CHAIN = 1


def gr_kinds(p, K, n):
    """Link kinds 0, 1, 2 in rotation across the columns; the rotation's start moves with K and n, so
    that a single column (p = 1) sees every kind over the lengths."""
    return np.array([(j + K + GR_LENGTHS.index(n)) % 3 for j in range(p)], dtype=np.int32)


def gr_level(j, n):
    """Identity columns alternate between level 0 and level 1e8 (unit spread on both)."""
    return 1e8 if (j // 3 + GR_LENGTHS.index(n)) % 2 == 1 else 0.0


def gr_inputs(p, K, n):
    """(x, kinds): logit columns uniform in (0, 1) with values 5e-10 from either end, log columns
    10^U(-300, 300) with 1e-300 and 1e300 themselves, identity columns N(level, 1); chain
    CONSTANT_CHAIN repeats its first draw (S2 = 0)."""
    rng = np.random.default_rng(1000 * p + 7 * K + n)
    kinds = gr_kinds(p, K, n)
    x = np.empty((n, p, K))
    for j in range(p):
        if kinds[j] == 2:
            c = rng.uniform(0.0, 1.0, (n, K))
            c[0, 0], c[n - 1, 0] = 5e-10, 1.0 - 5e-10          # chain 0: not the constant one
        elif kinds[j] == 1:
            c = 10.0 ** rng.uniform(-300.0, 300.0, (n, K))
            c[0, 0], c[n - 1, 0] = 1e-300, 1e300
        else:
            c = gr_level(j, n) + rng.normal(size=(n, K))
        x[:, j, :] = c
    x[:, :, CONSTANT_CHAIN] = x[0, :, CONSTANT_CHAIN]
    return x, kinds


def gr_end_to_end_inputs(p):
    """(x, kinds) for gelmandiag(transform=True) and cor: n = 50, K = 20, chains on their own levels
    (the between-chain variance is not a rounding residue), every column's spread comparable to its
    level.  p = 3: [logit, log, identity].  p = 6 adds a positive column whose minimum is exactly
    0.0 (identity, not log), a column in (0, 1] whose maximum is exactly 1.0 (log, not logit) and
    an all-negative one."""
    n, K = 50, 20
    rng = np.random.default_rng(60 + p)
    off = rng.normal(size=(p, K)) * 0.3
    z = rng.normal(size=(n, p, K)) + off[None]
    x = np.empty((n, p, K))
    x[:, 0] = 1.0 / (1.0 + np.exp(-z[:, 0]))                  # (0, 1): logit
    x[:, 1] = np.exp(1.0 + z[:, 1])                           # positive, above one too: log
    x[:, 2] = z[:, 2] + 0.5                                   # mixed signs: identity
    kinds = [2, 1, 0]
    if p == 6:
        x[:, 3] = np.abs(z[:, 3])
        x[7, 3, 4] = 0.0                                      # minimum exactly 0.0: identity
        x[:, 4] = 1.0 / (1.0 + np.exp(-z[:, 4]))
        x[11, 4, 9] = 1.0                                     # maximum exactly 1.0: log
        x[:, 5] = -np.exp(0.3 * z[:, 5])                      # all negative: identity
        kinds += [0, 1, 0]
    return x, np.array(kinds, dtype=np.int32)


# ------------------------------------------------------------------ crafted inputs: chain summaries
SS_THREADS, SS_U = 256, 16                                              # summary.hip's constants
SS_SHAPES = [(p, K) for p in (1, 3, 64) for K in (1, 255, 257)]
SS_LENGTHS = (1, 15, 16, 17, 100)
SS_BASES = (0, 7)
SS_COLUMNS = ("level 1e9", "constant", "ties")


def ss_column(j, n):
    return SS_COLUMNS[(j + n) % 3]


def ss_inputs(p, K, n):
    """Columns in rotation (the rotation's start moves with n, so p = 1 sees every kind over the
    lengths): 1e9 + N(0, 1e-3); the constant 2.5; N(0.3, 1) rounded to halves (heavy ties, both
    signs)."""
    rng = np.random.default_rng(5000 * p + 11 * K + n)
    x = np.empty((n, p, K))
    for j in range(p):
        kind = ss_column(j, n)
        if kind == "level 1e9":
            x[:, j, :] = 1e9 + rng.normal(0.0, 1e-3, (n, K))
        elif kind == "constant":
            x[:, j, :] = 2.5
        else:
            x[:, j, :] = np.round(rng.normal(0.3, 1.0, (n, K)) * 2.0) / 2.0
    return x


def ss_batch_sizes(n, K):
    """1, n, n + 1, a prime that divides neither n nor n K, and one well above n."""
    prime = next(q for q in (3, 5, 7, 11, 13, 17, 19) if n % q and (n * K) % q and q not in (n, n + 1))
    return sorted({1, n, n + 1, prime, 2 * n + 3})


SS_TABLE_BS = (7, 60, 100)        # N = 540: 77, 9 and 5 batches; 7 and 100 straddle the chains
SS_TABLE_BS_TOO_BIG = 271         # 540 // 271 = 1 batch: an ArgumentError
SS_TABLE_SPLIT = 4                # two shards: chains [0, 4) and [4, 9); flat 240 is inside a batch of 7 and of 100


def ss_table_inputs(constant):
    """n = 60, K = 9 for the summarystats tables: the three column kinds (the constant one only on
    request) and a plain N(-4, 2) column."""
    n, K = 60, 9
    rng = np.random.default_rng(77)
    cols = [1e9 + rng.normal(0.0, 1e-3, (n, K)), np.round(rng.normal(0.3, 1.0, (n, K)) * 2.0) / 2.0,
            rng.normal(-4.0, 2.0, (n, K))]
    if constant:
        cols.insert(1, np.full((n, K), 2.5))
    return np.stack(cols, axis=1)


# ------------------------------------------------------------------ crafted inputs: order statistics, range
TINY = 5e-324                                                           # the smallest subnormal
Q12 = (0.013, 0.11, 0.19, 0.27, 0.36, 0.44, 0.52, 0.61, 0.69, 0.78, 0.86, 0.987)
Q_ENDS = (0.0, 0.5, 1.0)
OS_BIG_K = 16384 + 257                       # os_hist_kernel's grid covers 64 x 256 chains per stride


def os_inputs(infinite):
    """n = 37, K = 11, four columns: mixed signs; all equal; three distinct values; and one holding
    -0.0, +0.0, the smallest subnormals of both signs, +-1.7e308 and (on request) +-inf among
    N(0, 1) draws."""
    n, K = 37, 11
    rng = np.random.default_rng(31)
    x = np.empty((n, 4, K))
    x[:, 0] = rng.normal(0.0, 3.0, (n, K))
    x[:, 1] = -7.25
    x[:, 2] = rng.choice([-1.5, 0.0, 2.0 ** -40], size=(n, K))
    c = rng.normal(size=(n, K))
    special = [-0.0, 0.0, -TINY, TINY, -1.7e308, 1.7e308, -0.0, 0.0] + ([-np.inf, np.inf] if infinite else [])
    c.flat[rng.choice(n * K, len(special), replace=False)] = special
    x[:, 3] = c
    return x


def os_big_inputs(n):
    """One column, OS_BIG_K chains: N(0, 1), the chains past the first 16384 lifted by 10 -- the top
    order statistics all come from chains only the second stride of the chain loop reaches."""
    x = np.random.default_rng(90 + n).normal(size=(n, 1, OS_BIG_K))
    x[:, :, 16384:] += 10.0
    return x


def os_wide_inputs():
    """n = 9, K = 5, 64 columns N(j, 1): no two columns share an order statistic."""
    x = np.random.default_rng(64).normal(size=(9, 64, 5))
    return x + np.arange(64.0)[None, :, None]


def range_inputs(p, n, K):
    """N(0, 1) with -0.0 / +0.0 columns, a column reaching +-inf and plain ones, as far as p allows."""
    x = np.random.default_rng(p + n + K).normal(size=(n, p, K))
    x[0, 0, 0] = np.inf
    if n * K > 1:
        x[n - 1, 0, K - 1] = -np.inf
    if p > 1:
        x[:, 1, :] = np.where(np.arange(n * K).reshape(n, K) % 2 == 0, -0.0, 0.0)
    if p > 2:
        x[:, 2, :] = -np.abs(x[:, 2, :])
        x[0, 2, 0] = -0.0                             # maximum -0.0 over negative values
    return x


def wide_inputs():
    """n = 40, K = 5, 66 columns (the node-IR rats model with every node monitored): N(j - 30, 1 + j / 10)."""
    j = np.arange(66.0)
    return np.random.default_rng(66).normal(size=(40, 66, 5)) * (1.0 + j / 10.0)[None, :, None] + (j - 30.0)[None, :, None]


def all_gr_cases():
    return [(p, K, n) for (p, K), n in itertools.product(GR_SHAPES, GR_LENGTHS)]
