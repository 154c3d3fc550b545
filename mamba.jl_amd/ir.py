"""Generic node IR: Mamba Model DAGs lowered for the HIP engine.

Mirrors the reference's model specification API (src/model/dependent.jl:75-152,
src/model/model.jl:5-27):

    model = ir.Model(
        r=ir.Stochastic(1, lambda alpha0, alpha1, x1, b, n:
                        ir.Binomial(n, ir.invlogit(alpha0 + alpha1 * x1 + b)), False),
        b=ir.Stochastic(1, lambda s2: ir.Normal(0, ir.sqrt(s2)), False),
        alpha0=ir.Stochastic(lambda: ir.Normal(0, 1000)), ...)

Each node function names its parents by argument name, like a Julia closure
(src/utils.jl:3-43).  It is traced once with symbolic arguments, so it is written
vectorised: arithmetic broadcasts elementwise over the node's elements (a Stochastic(1, ...)
node with a univariate distribution is elementwise, distributionstruct.jl:142-158),
`mu[batch]` gathers with a 1-based data index vector, `beta[2]` is element 2 (1-based).
Logical nodes are inlined into their Stochastic children; Stochastic nodes that no sampling
block updates are fixed (observed) and their values (from the inits, as in the reference)
go to the data pool.  The lowering produces the mmb_ir_model of include/mamba_hip.h:
per-node stack code, the block term lists of logpdf! (simulation.jl:77-90: params \\ targets
in block order, then targets in topological order) and the monitored nodes.

Supported: Normal, MvNormal(mu, sigma) (isotropic), InverseGamma, Gamma, Exponential,
Uniform (constant bounds), Beta for sampled nodes; Binomial, Poisson, Bernoulli, Categorical,
DiscreteUniform for fixed nodes; + - * / neg abs exp log sqrt invlogit logit, x**2; blocks of
<= 32 elements.

Binary nodes (src/samplers/bmg.jl, bmc3.jl, bia.jl): a Bernoulli or DiscreteUniform(0, 1) node of at most 32
elements may instead be sampled by one `BMG`, `BMC3`, `BIA` or `BHMC` (bhmc.jl) block, which holds that node alone.

Discrete nodes (src/samplers/dgs.jl): a Bernoulli, Binomial (n data), Categorical(p) (p a constant
list or a data vector shared by every element, support 1..K) or DiscreteUniform(a, b) (constant
integer bounds) node may be sampled, by a `DGS` block only; Poisson stays observed (infinite
support).  A sampled element's support holds at most 32 values (one mass per lane of the chain's
32-lane group): Binomial n <= 31, K <= 32, b - a <= 31.  DGS(["a", "b"]) becomes one device block
per node, in order (the reference loops over its keys, dgs.jl:61-80); a DGS node may be longer
than 32 elements.  `x[T]` with T a sampled discrete node gathers by the state (x a sampled node or
a data vector; T's support within 1..len(x), T as long as the expression).

Probability vectors (src/samplers/slicesimplex.jl): `Dirichlet(alpha)` (alpha a constant list or a data
vector, every alpha_i > 0) is one distribution over the 2..32 elements of a Stochastic(1, ...) node; a
sampled one is updated by a `SliceSimplex` block only, and its initial values are probability vectors.
SliceSimplex(["a", "b"]) becomes one device block per node, in order.  `Categorical(P)` with P such a
sampled node reads its probabilities from the chain state (K = len(P)), so mixture weights are
learnt (doc/examples/eyes.jl).  Arrays of Dirichlets (doc/examples/asthma.jl) are not lowered.

User Gibbs blocks (ABI 10): `Sampler(params, f)` (src/samplers/sampler.jl:20-24) whose closure
returns `rand(Normal(mu, sigma))`, `rand(InverseGamma(shape, scale))` or `rand(Gamma(shape,
scale))` for one scalar node -- the conjugate full conditionals of doc/tutorial/line.jl:38-45
and INTEGRATION.md §3 -- traced like the node functions, with `sum(x)`, `sumabs2(x)`, `mean(x)`
and `length(x)` over node / data expressions:

    Gibbs_s2_c = ir.Sampler(["s2_c"], lambda alpha, beta, s2_c, y, rat, Xm:
        ir.rand(ir.InverseGamma(0.001 + ir.length(y) / 2,
                                0.001 + ir.sumabs2(y - (alpha[rat] + beta[rat] * Xm)) / 2)))
The topological order of targets is deterministic (declaration order breaks ties); the
reference's depends on Dict hashing (model.jl:112-120), which only changes summation order.
"""
import builtins
import ctypes as C
import inspect
import math

import numpy as np

from . import abi
from .model import Model as _BaseModel, Node
from .samplers import ArgumentError

# ------------------------------------------------------------------ expressions


def _e(x):
    if isinstance(x, Expr):
        return x
    if isinstance(x, (int, float, np.integer, np.floating)):
        return Const(float(x))
    raise ArgumentError(f"unsupported value in a node expression: {x!r}")


class Expr:
    def __add__(s, o): return Bin("+", s, _e(o))
    def __radd__(s, o): return Bin("+", _e(o), s)
    def __sub__(s, o): return Bin("-", s, _e(o))
    def __rsub__(s, o): return Bin("-", _e(o), s)
    def __mul__(s, o): return Bin("*", s, _e(o))
    def __rmul__(s, o): return Bin("*", _e(o), s)
    def __truediv__(s, o): return Bin("/", s, _e(o))
    def __rtruediv__(s, o): return Bin("/", _e(o), s)
    def __neg__(s): return Un("neg", s)
    def __abs__(s): return Un("abs", s)

    def __pow__(s, k):
        if k == 2:
            return Bin("*", s, s)
        raise ArgumentError("only x**2 is supported in node expressions")


class Const(Expr):
    def __init__(s, v):
        s.v = v


class Ref(Expr):
    """A closure argument: a node or an input, elementwise."""

    def __init__(s, name):
        s.name = name

    def __getitem__(s, idx):
        if isinstance(idx, Ref):
            return Gather(s.name, idx.name)
        if isinstance(idx, (int, np.integer)) and idx >= 1:
            return Elem(s.name, int(idx))
        raise ArgumentError("index a node with a 1-based integer or a data index vector")


class Elem(Expr):
    def __init__(s, name, k):
        s.name, s.k = name, k


class Gather(Expr):
    def __init__(s, name, idx):
        s.name, s.idx = name, idx


class Bin(Expr):
    def __init__(s, op, a, b):
        s.op, s.a, s.b = op, a, b


class Un(Expr):
    def __init__(s, op, a):
        s.op, s.a = op, a


class Reduce(Expr):
    """sum over the elements of an expression (a Gibbs closure's reductions)."""

    def __init__(s, a):
        s.a = a


class Len(Expr):
    """length(x): the element count of an expression, a constant once node lengths are known."""

    def __init__(s, a):
        s.a = a


class RedSlot(Expr):
    """Reduction k of a Gibbs block: value slot nvalues + k of the state row (lowering only)."""

    def __init__(s, k):
        s.k = k


class Rand:
    """rand(d): the value a Gibbs closure returns."""

    def __init__(s, dist):
        if not isinstance(dist, Dist):
            raise ArgumentError("rand() takes a distribution")
        s.dist = dist


def sum(x): return Reduce(_e(x))                    # noqa: A001 -- Julia's sum(x) in closures
def sumabs2(x): return Reduce(Bin("*", _e(x), _e(x)))  # Julia sumabs2(x) = sum(abs2, x)
def length(x): return Len(_e(x))
def mean(x): return Bin("/", sum(x), length(x))     # Julia mean(x) = sum(x) / length(x)
def rand(d): return Rand(d)


def exp(x): return Un("exp", _e(x))
def log(x): return Un("log", _e(x))
def sqrt(x): return Un("sqrt", _e(x))
def invlogit(x): return Un("invlogit", _e(x))   # src/utils.jl:64
def logit(x): return Un("logit", _e(x))         # src/utils.jl:67


# ------------------------------------------------------------------ distributions

class Dist:
    def __init__(s, fam, *params):
        s.fam = fam
        s.params = [_e(p) for p in params]


def Normal(mu=0.0, sigma=1.0): return Dist(abi.MMB_IR_NORMAL, mu, sigma)
def InverseGamma(shape=1.0, scale=1.0): return Dist(abi.MMB_IR_INVGAMMA, shape, scale)
def Gamma(shape=1.0, scale=1.0): return Dist(abi.MMB_IR_GAMMA, shape, scale)
def Exponential(scale=1.0): return Dist(abi.MMB_IR_EXPONENTIAL, scale)
def Uniform(a=0.0, b=1.0): return Dist(abi.MMB_IR_UNIFORM, a, b)
def Beta(a=1.0, b=1.0): return Dist(abi.MMB_IR_BETA, a, b)
def Binomial(n, p): return Dist(abi.MMB_IR_BINOMIAL, n, p)
def Poisson(lam): return Dist(abi.MMB_IR_POISSON, lam)
def Bernoulli(p): return Dist(abi.MMB_IR_BERNOULLI, p)


def Categorical(p):
    """Categorical(p): support 1..K; p a list of K constants, a data vector (an input) or a sampled
    Dirichlet node (its K elements, read from the chain state), the same for every element of the node."""
    d = Dist(abi.MMB_IR_CATEGORICAL)
    if isinstance(p, Ref):
        d.p = p
    elif isinstance(p, Expr):
        raise ArgumentError("Categorical(p): p is a constant list, a data vector or a sampled Dirichlet node")
    else:
        d.p = np.atleast_1d(np.asarray(p, dtype=np.float64)).ravel()
    return d


def Dirichlet(alpha):
    """Dirichlet(alpha): alpha a list of constants or a data vector (an input), every alpha_i > 0; the
    node's 2..32 elements are one probability vector."""
    d = Dist(abi.MMB_IR_DIRICHLET)
    if isinstance(alpha, Ref):
        d.alpha = alpha
    elif isinstance(alpha, Expr):
        raise ArgumentError("Dirichlet(alpha): alpha is a constant list or a data vector")
    else:
        d.alpha = np.atleast_1d(np.asarray(alpha, dtype=np.float64)).ravel()
        _check_alpha(d.alpha)
    return d


def _check_alpha(a):
    if a.size < 1 or not np.all(np.isfinite(a)) or np.any(a <= 0.0):
        raise ArgumentError("Dirichlet(alpha): every alpha must be positive")


def DiscreteUniform(a, b):
    """DiscreteUniform(a, b): the integers a..b, constant bounds."""
    for v in (a, b):
        if isinstance(v, Expr) or isinstance(v, bool) or v != int(v):
            raise ArgumentError("DiscreteUniform(a, b): constant integer bounds")
    if int(b) < int(a):
        raise ArgumentError("DiscreteUniform(a, b): a <= b")
    d = Dist(abi.MMB_IR_DISCRETEUNIFORM)
    d.lo, d.hi = int(a), int(b)
    return d


def MvNormal(mu, sigma):
    """MvNormal(mu, sigma) / MvNormal(k, sigma) (zero mean): isotropic ScalMat covariance."""
    if isinstance(mu, (int, np.integer)) and not isinstance(mu, bool):
        mu = 0.0
    return Dist(abi.MMB_IR_ISONORMAL, mu, sigma)


_SAMPLEABLE = {abi.MMB_IR_NORMAL, abi.MMB_IR_ISONORMAL, abi.MMB_IR_INVGAMMA, abi.MMB_IR_GAMMA,
               abi.MMB_IR_EXPONENTIAL, abi.MMB_IR_UNIFORM, abi.MMB_IR_BETA}
_GIBBS_FAMILIES = {abi.MMB_IR_NORMAL, abi.MMB_IR_INVGAMMA, abi.MMB_IR_GAMMA}


def Sampler(params, f):
    """Sampler(params, f) (src/samplers/sampler.jl:20-24): a user block update whose closure f
    names its arguments after nodes and inputs (like a node function, src/utils.jl:3-43) and
    returns rand(Normal | InverseGamma | Gamma) of the block's one scalar node.  The closure is
    traced here; the node IR lowers it to a Gibbs block (mmb_ir_block.gibbs_*)."""
    from .samplers import Sampler as _S
    s = _S(params, abi.MMB_SAMPLER_GIBBS, abi.MMB_ADAPT_NONE, None)
    if not callable(f):
        raise ArgumentError("Sampler(params, f): f must be a function")
    s.f = f
    s.argnames = list(inspect.signature(f).parameters)
    out = f(*[Ref(a) for a in s.argnames])
    if not isinstance(out, Rand) or out.dist.fam not in _GIBBS_FAMILIES:
        raise ArgumentError("a node-IR Sampler closure must return rand(Normal | InverseGamma | Gamma)")
    s.traced = out.dist
    return s
_DISCRETE = {abi.MMB_IR_BINOMIAL, abi.MMB_IR_POISSON, abi.MMB_IR_BERNOULLI, abi.MMB_IR_CATEGORICAL,
             abi.MMB_IR_DISCRETEUNIFORM}
# DGSUnivariateDistribution (dgs.jl:6-8) without the two hypergeometrics
_DGS_FAMILIES = _DISCRETE - {abi.MMB_IR_POISSON}
_POSITIVE = {abi.MMB_IR_INVGAMMA, abi.MMB_IR_GAMMA, abi.MMB_IR_EXPONENTIAL}


def _isprobvec(v):
    """The support of a Dirichlet node (csrc/ir_math.h mmb_ir_dirichlet_lp): every entry >= 0 and
    |sum - 1| <= MMB_SIMPLEX_TOL; a NaN fails."""
    v = np.asarray(v, dtype=np.float64)
    return bool(np.all(v >= 0.0) and abs(float(v.sum()) - 1.0) <= abi.MMB_SIMPLEX_TOL)


# ------------------------------------------------------------------ nodes

class _NodeDef:
    def __init__(self, kind, args, monitor):
        if args and callable(args[0]):
            dim, f, rest = 0, args[0], args[1:]
        elif len(args) >= 2 and callable(args[1]):
            dim, f, rest = int(args[0]), args[1], args[2:]
        else:
            raise ArgumentError(f"{kind}([dim,] f[, monitor])")
        if rest:
            monitor = rest[0]
        self.kind, self.dim, self.f = kind, dim, f
        self.monitor = bool(monitor)
        self.argnames = list(inspect.signature(f).parameters)


def Stochastic(*args, monitor=True):
    """Stochastic(f[, monitor]) / Stochastic(d, f[, monitor]) (dependent.jl:137-152)."""
    return _NodeDef("stochastic", args, monitor)


def Logical(*args, monitor=True):
    """Logical(f[, monitor]) / Logical(d, f[, monitor]) (dependent.jl:75-88)."""
    return _NodeDef("logical", args, monitor)


# ------------------------------------------------------------------ model

class Model(_BaseModel):
    """Model(; nodes...) (model.jl:5-27) lowered to the node IR at setinits (init_matrix)."""

    def __init__(self, **nodes):
        super().__init__(abi.MMB_MODEL_IR, [], 0, [], [])
        self.defs = dict(nodes)
        self.order = list(nodes)
        self.traced = {}
        for name, d in self.defs.items():
            if not isinstance(d, _NodeDef):
                raise ArgumentError(f"node {name} must be a Stochastic or Logical")
            out = d.f(*[Ref(a) for a in d.argnames])
            if d.kind == "stochastic":
                if not isinstance(out, Dist):
                    raise ArgumentError(f"Stochastic node {name} must return a distribution")
            else:
                out = _e(out)
            self.traced[name] = out
        self.stoch = [n for n in self.order if self.defs[n].kind == "stochastic"]
        # Stochastic nodes are the candidate block parameters (dims known at setinits)
        self.nodes = {n: Node(n, i, 0, 0, self.traced[n].fam in _POSITIVE) for i, n in enumerate(self.order)
                      if self.defs[n].kind == "stochastic"}
        self.compiled = False
        self.inputs = {}

    # setsamplers! is checked once the node lengths are known (init_matrix)
    def setsamplers(self, samplers):
        # DGS(["a", "b"]) updates its keys one after another (dgs.jl:61-80): one device block per node,
        # in order, so that a block's terms are the node and that node's targets (dgs.jl:109-126 mass)
        # SliceSimplex(["a", "b"]) likewise (slicesimplex.jl:37-54)
        split = []
        for s in samplers:
            if s.kind == abi.MMB_SAMPLER_DGS and len(s.params) != 1:
                from .samplers import DGS
                split += [DGS(p) for p in s.params]
            elif s.kind == abi.MMB_SAMPLER_SLICESIMPLEX and len(s.params) != 1:
                from .samplers import SliceSimplex
                split += [SliceSimplex(p, scale=s.scale) for p in s.params]
            else:
                split.append(s)
        samplers = split
        for s in samplers:
            if s.kind == abi.MMB_SAMPLER_GIBBS and getattr(s, "traced", None) is None:
                raise ArgumentError("on the node IR a Gibbs block is a traced closure: ir.Sampler(params, f) "
                                    "returning rand(Normal | InverseGamma | Gamma)")
            if s.kind == abi.MMB_SAMPLER_GIBBS and len(s.params) != 1:
                raise ArgumentError("a node-IR Sampler closure updates one node")
            for p in s.params:
                if p not in self.nodes:
                    raise ArgumentError(f"{p} is not a Stochastic node of this model")
        if not 1 <= len(samplers) <= abi.MMB_MAX_BLOCKS:
            raise ArgumentError(f"need 1..{abi.MMB_MAX_BLOCKS} sampling blocks")
        self.samplers = list(samplers)
        self.compiled = False
        return self

    def setinputs(self, inputs):
        self.inputs = {k: np.atleast_1d(np.asarray(v, dtype=np.float64)).ravel(order="F") for k, v in inputs.items()}
        self.compiled = False
        return self

    def data_arrays(self):
        return []

    def block_dim(self, s):
        return builtins.sum(self.lens[p] for p in s.params)

    # ---- setinits!: node lengths, layout, lowering ----
    def init_matrix(self, inits, chains):
        if isinstance(inits, np.ndarray):
            if not self.compiled:
                raise ArgumentError("a node-IR model needs dict inits (node lengths) before a value matrix")
            return super().init_matrix(inits, chains)
        if len(inits) < chains:
            raise ArgumentError("fewer initial values than chains")
        self._compile(inits[0])
        for k in range(chains):  # sampled discrete nodes start inside their supports (they index x[T])
            for n in self.discrete:
                v = self._initval(inits[k], n)
                lo, hi = self.support[n]
                if v.size != self.lens[n] or np.any(v != np.round(v)) or np.any(v < lo) or np.any(v > hi):
                    raise ArgumentError(f"initial value of discrete node {n} (chain {k + 1}) is outside its support")
        for k in range(chains):  # sampled Dirichlet nodes start on the simplex (validatesimplex, sampler.jl:80-82)
            for n in self.simplex:
                v = self._initval(inits[k], n)
                if v.size != self.lens[n] or not _isprobvec(v):
                    raise ArgumentError(f"variate is not a probability vector (node {n}, chain {k + 1})")
        for k in range(1, chains):  # fixed (observed) nodes are data: equal in every chain
            for n in self.fixed:
                if not np.array_equal(self._initval(inits[k], n), self.fixed_vals[n]):
                    raise ArgumentError(f"fixed node {n} differs between chains' inits")
        return super().init_matrix([{p: inits[k][p] for p in self.params} for k in range(chains)], chains)

    def _initval(self, d, n):
        if n not in d:
            raise ArgumentError(f"missing initial value for node : {n}")
        return np.atleast_1d(np.asarray(d[n], dtype=np.float64)).ravel(order="F")

    def _compile(self, init0):
        if not self.samplers:
            raise ArgumentError("no samplers set (setsamplers!)")
        inblock = {p for s in self.samplers for p in s.params}
        self.params = [n for n in self.stoch if n in inblock]
        self.fixed = [n for n in self.stoch if n not in inblock]
        self.lens = {}
        for n in self.stoch:
            v = self._initval(init0, n)
            if self.defs[n].dim == 0 and v.size != 1:
                raise ArgumentError(f"incompatible initial value for node : {n}")
            self.lens[n] = v.size
        self.fixed_vals = {n: self._initval(init0, n) for n in self.fixed}
        binary = (abi.MMB_SAMPLER_BMG, abi.MMB_SAMPLER_BMC3, abi.MMB_SAMPLER_BIA, abi.MMB_SAMPLER_BHMC)
        by_dgs = {p for s in self.samplers if s.kind == abi.MMB_SAMPLER_DGS or s.kind in binary for p in s.params}
        for s in self.samplers:
            for n in s.params:
                fam = self.traced[n].fam
                if s.kind == abi.MMB_SAMPLER_DGS:
                    if fam not in _DGS_FAMILIES:
                        raise ArgumentError(f"DGS: node {n} is not a Bernoulli, Binomial, Categorical or "
                                            "DiscreteUniform node")
                elif s.kind in binary:
                    # validatebinary's domain: Bernoulli, or DiscreteUniform(0, 1) (bmg.jl:26-37, bia.jl:49)
                    d = self.traced[n]
                    if not (fam == abi.MMB_IR_BERNOULLI or
                            (fam == abi.MMB_IR_DISCRETEUNIFORM and (d.lo, d.hi) == (0, 1))):
                        raise ArgumentError(f"{s.name}: node {n} is not a Bernoulli or DiscreteUniform(0, 1) node")
                elif s.kind == abi.MMB_SAMPLER_SLICESIMPLEX:
                    if fam != abi.MMB_IR_DIRICHLET:
                        raise ArgumentError(f"SliceSimplex: node {n} is not a Dirichlet node")
                elif fam == abi.MMB_IR_DIRICHLET:
                    raise ArgumentError(f"Dirichlet node {n} cannot be sampled by {s!r}: use SliceSimplex")
                elif fam in _DISCRETE:
                    raise ArgumentError(f"discrete node {n} cannot be sampled by {s!r}: use DGS")
                elif s.kind == abi.MMB_SAMPLER_ABC and fam not in _SAMPLEABLE:
                    raise ArgumentError(f"ABC: node {n} is not a continuous sampleable node")
                elif fam not in _SAMPLEABLE:
                    raise ArgumentError(f"node {n}: its distribution family cannot be sampled by these samplers")
        self.discrete = [n for n in self.params if n in by_dgs]
        self.simplex = [n for n in self.params if self.traced[n].fam == abi.MMB_IR_DIRICHLET]
        # state layout: sampled nodes in declaration order
        off = 0
        self.nodes = {}
        for i, n in enumerate(self.order):
            if n in self.params:
                self.nodes[n] = Node(n, i, off, self.lens[n], self.traced[n].fam in _POSITIVE)
                off += self.lens[n]
        self.nvalues = off
        if not 1 <= off <= abi.MMB_IR_MAX_VALUES:
            raise ArgumentError(f"node IR: 1..{abi.MMB_IR_MAX_VALUES} sampled values")
        for s in self.samplers:
            d = self.block_dim(s)
            if d > 32 and s.kind != abi.MMB_SAMPLER_DGS:  # (DGS visits its elements one by one)
                raise ArgumentError(f"node IR: blocks of at most 32 elements (block {s.params} has {d})")
            if s.kind == abi.MMB_SAMPLER_GIBBS and d != 1:
                raise ArgumentError(f"node IR: a Sampler closure draws one scalar node ({s.params[0]} has {d})")
            s.validate(d)
        _Lowering(self).run()
        self.compiled = True

    def spec(self):
        if not self.compiled:
            raise ArgumentError("node-IR model: call init_matrix (setinits!) first")
        return super().spec()

    def stats_table(self):
        if not self.compiled:
            raise ArgumentError("node-IR model: call init_matrix (setinits!) first")
        return self._stats

    def ir(self):
        if not self.compiled:
            raise ArgumentError("node-IR model: call init_matrix (setinits!) first")
        return self._ir


class _Lowering:
    """Model -> mmb_ir_model (include/mamba_hip.h)."""

    def __init__(self, m):
        self.m = m
        self.code, self.consts, self.pool = [], [], []
        self.pool_of = {}
        self.depth = 1
        self.fixed_reads = set()  # fixed (observed) Stochastic nodes some node's expressions read

    # -- pool / const helpers
    def const(self, v):
        self.consts.append(float(v))
        return len(self.consts) - 1

    @staticmethod
    def word(opc, arg):
        """One code word: opcode in the top byte, operand (pool / value / constant offset) in
        the low 24 bits; a larger operand would carry into the opcode, so it is refused."""
        if not 0 <= arg < 1 << 24:
            raise ArgumentError(f"node IR operand {arg} does not fit in 24 bits (pool or model too large)")
        return opc << 24 | arg

    def put(self, key, arr):
        if key in self.pool_of:
            return self.pool_of[key]
        off = len(self.pool)
        self.pool.extend(float(a) for a in np.asarray(arr, dtype=np.float64).ravel())
        self.pool_of[key] = off
        return off

    def kind(self, name):
        m = self.m
        if name in m.defs:
            if m.defs[name].kind == "logical":
                return "logical"
            return "param" if name in m.params else "fixed"
        if name in m.inputs:
            return "data"
        raise ArgumentError(f"{name} is neither a node nor an input")

    def length(self, e, seen=()):
        """Broadcast length of an expression (1 = scalar)."""
        if isinstance(e, (Const, Elem, Reduce, Len, RedSlot)):
            return 1
        if isinstance(e, Ref):
            k = self.kind(e.name)
            if k == "logical":
                if e.name in seen:
                    raise ArgumentError(f"cycle through logical {e.name}")
                return self.length(self.m.traced[e.name], seen + (e.name,))
            if k == "data":
                return self.m.inputs[e.name].size
            return self.m.lens[e.name]
        if isinstance(e, Gather):
            return self.m.inputs[e.idx].size if e.idx in self.m.inputs else self.length(Ref(e.idx))
        if isinstance(e, Bin):
            a, b = self.length(e.a, seen), self.length(e.b, seen)
            if a != 1 and b != 1 and a != b:
                raise ArgumentError("length mismatch in a node expression")
            return max(a, b)
        return self.length(e.a, seen)

    def host_value(self, e, n):
        """Numeric value of a data/constant-only expression (length n), else None."""
        if isinstance(e, Const):
            return np.full(n, e.v)
        if isinstance(e, Ref):
            k = self.kind(e.name)
            if k == "data":
                v = self.m.inputs[e.name]
                return np.full(n, v[0]) if v.size == 1 else v.copy()
            if k == "fixed":
                v = self.m.fixed_vals[e.name]
                return np.full(n, v[0]) if v.size == 1 else v.copy()
            if k == "logical":
                return self.host_value(self.m.traced[e.name], n)
            return None
        if isinstance(e, Bin):
            a, b = self.host_value(e.a, n), self.host_value(e.b, n)
            if a is None or b is None:
                return None
            return {"+": a + b, "-": a - b, "*": a * b, "/": a / b}[e.op]
        if isinstance(e, Un):
            a = self.host_value(e.a, n)
            if a is None:
                return None
            return {"neg": -a, "abs": np.abs(a), "exp": np.exp(a), "log": np.log(a), "sqrt": np.sqrt(a),
                    "invlogit": 1.0 / (np.exp(-a) + 1.0), "logit": np.log(a / (1.0 - a))}[e.op]
        return None

    # -- code emission for an expression evaluated at elements 0..n-1
    def emit(self, e, n, sp, refs):
        op = abi.IR_OP
        m = self.m

        def push(word):
            self.code.append(word)
            self.depth = max(self.depth, sp + 1)
            return sp + 1

        if isinstance(e, Const):
            return push(self.word(op["const"], self.const(e.v)))
        if isinstance(e, RedSlot):  # a Gibbs block's reduction: value slot nvalues + k
            return push(self.word(op["val"], m.nvalues + e.k))
        if isinstance(e, (Reduce, Len)):
            raise ArgumentError("sum / length appear only in a Sampler closure's distribution parameters")
        if isinstance(e, Elem):
            k = self.kind(e.name)
            ln = self.length(Ref(e.name))
            if not 1 <= e.k <= ln:
                raise ArgumentError(f"{e.name}[{e.k}] out of range")
            if k == "param":
                refs.add(e.name)
                return push(self.word(op["val"], (m.nodes[e.name].offset + e.k - 1)))
            if k in ("fixed", "data"):
                if k == "fixed":
                    self.fixed_reads.add(e.name)
                v = m.fixed_vals[e.name] if k == "fixed" else m.inputs[e.name]
                return push(self.word(op["datas"], self.put(("elem", e.name, e.k), v[e.k - 1:e.k])))
            raise ArgumentError("element of a logical: index its parents instead")
        if isinstance(e, Ref):
            k = self.kind(e.name)
            if k == "logical":
                ln = self.length(e)
                if ln not in (1, n):
                    raise ArgumentError(f"logical {e.name} has length {ln}, expected 1 or {n}")
                return self.emit(m.traced[e.name], n, sp, refs)
            ln = self.length(e)
            if ln not in (1, n):
                raise ArgumentError(f"{e.name} has length {ln}, expected 1 or {n}")
            if k == "param":
                refs.add(e.name)
                o = m.nodes[e.name].offset
                return push(self.word(op["val"] if ln == 1 else op["vali"], o))
            if k == "fixed":
                self.fixed_reads.add(e.name)
            v = m.fixed_vals[e.name] if k == "fixed" else m.inputs[e.name]
            o = self.put(("v", e.name), v)
            return push(self.word(op["datas"] if ln == 1 else op["data"], o))
        if isinstance(e, Gather) and e.idx in m.defs and e.idx in getattr(m, "discrete", ()):
            # x[T], T a sampled discrete node: the index is state (MMB_IR_OP_VALV / _DATAV)
            if m.lens[e.idx] != n:
                raise ArgumentError(f"gather index {e.idx} has length {m.lens[e.idx]}, expected {n}")
            k = self.kind(e.name)
            if k == "logical":
                raise ArgumentError("gather from a logical: gather its parents instead")
            ln = self.length(Ref(e.name))
            lo, hi = self.support_bounds(e.idx)
            if lo < 1 or hi > ln:
                raise ArgumentError(f"{e.name}[{e.idx}]: the support {lo}..{hi} of {e.idx} must lie in 1..{ln}")
            refs.add(e.idx)
            if k == "param":
                refs.add(e.name)
                sp2 = push(self.word(op["valv"], m.nodes[e.name].offset))
            else:
                if k == "fixed":
                    self.fixed_reads.add(e.name)
                v = m.fixed_vals[e.name] if k == "fixed" else m.inputs[e.name]
                sp2 = push(self.word(op["datav"], self.put(("v", e.name), v)))
            self.code.append(m.nodes[e.idx].offset)
            return sp2
        if isinstance(e, Gather):
            if e.idx not in m.inputs:
                raise ArgumentError(f"gather index {e.idx} must be an input (data) vector or a sampled discrete node")
            idx = m.inputs[e.idx]
            if idx.size != n:
                raise ArgumentError(f"gather index {e.idx} has length {idx.size}, expected {n}")
            k = self.kind(e.name)
            ln = self.length(Ref(e.name))
            if np.any(idx != np.round(idx)) or idx.min() < 1 or idx.max() > ln:
                raise ArgumentError(f"{e.name}[{e.idx}]: indices must be integers in 1..{ln}")
            if k == "param":
                refs.add(e.name)
                w = self.put(("idx", e.idx), idx - 1.0)
                sp2 = push(self.word(op["valg"], m.nodes[e.name].offset))
                self.code.append(w)
                return sp2
            if k in ("fixed", "data"):
                if k == "fixed":
                    self.fixed_reads.add(e.name)
                v = m.fixed_vals[e.name] if k == "fixed" else m.inputs[e.name]
                return push(self.word(op["data"], self.put(("g", e.name, e.idx), v[(idx - 1).astype(int)])))
            raise ArgumentError("gather from a logical: gather its parents instead")
        if isinstance(e, Bin):
            sp = self.emit(e.a, n, sp, refs)
            sp = self.emit(e.b, n, sp, refs)
            self.code.append(op[e.op] << 24)
            return sp - 1
        sp = self.emit(e.a, n, sp, refs)
        self.code.append(op[e.op] << 24)
        return sp

    def cat_p(self, name):
        """The probability vector of Categorical node `name` (a constant list or a data vector), checked
        as Distributions' isprobvec does."""
        p = self.m.traced[name].p
        if isinstance(p, Ref):
            if self.kind(p.name) != "data":
                raise ArgumentError(f"Categorical p of {name} must be a constant list, a data vector or a sampled "
                                    "Dirichlet node")
            p = self.m.inputs[p.name]
        if p.size < 1 or not np.all(np.isfinite(p)) or np.any(p < 0.0) or \
                abs(float(p.sum()) - 1.0) > math.sqrt(np.finfo(float).eps):
            raise ArgumentError(f"Categorical p of {name} is not a probability vector")
        return p

    def cat_state(self, name):
        """The sampled Dirichlet node that Categorical node `name` reads its probabilities from, or None
        (a constant list or a data vector: cat_p)."""
        p = self.m.traced[name].p
        if not isinstance(p, Ref) or p.name not in self.m.defs or self.kind(p.name) != "param":
            return None
        if self.m.traced[p.name].fam != abi.MMB_IR_DIRICHLET:
            raise ArgumentError(f"Categorical p of {name}: the sampled node {p.name} is not a Dirichlet node")
        return p.name

    def dirichlet_alpha(self, name):
        a = self.m.traced[name].alpha
        if isinstance(a, Ref):
            if self.kind(a.name) != "data":
                raise ArgumentError(f"Dirichlet alpha of {name} must be a constant list or a data vector")
            a = self.m.inputs[a.name]
            _check_alpha(a)
        return a

    def binomial_n(self, name):
        dist, ln = self.m.traced[name], self.m.lens[name]
        nn = self.host_value(dist.params[0], ln)
        if nn is None:
            raise ArgumentError(f"Binomial n of {name} must be data")
        return nn

    def support_bounds(self, name):
        """(lo, hi) of discrete node `name` over all its elements (integers)."""
        dist = self.m.traced[name]
        if dist.fam == abi.MMB_IR_BERNOULLI:
            return 0, 1
        if dist.fam == abi.MMB_IR_BINOMIAL:
            nn = self.binomial_n(name)
            if np.any(nn != np.round(nn)) or nn.min() < 0:
                raise ArgumentError(f"Binomial n of {name} must be non-negative integers")
            return 0, int(nn.max())
        if dist.fam == abi.MMB_IR_CATEGORICAL:
            P = self.cat_state(name)
            return 1, int(self.m.lens[P] if P is not None else self.cat_p(name).size)
        return dist.lo, dist.hi

    def expr(self, e, n, refs):
        start = len(self.code)
        self.emit(e, n, 0, refs)
        self.code.append(0)  # END
        return start

    # -- Gibbs closure blocks (ABI 10)
    def resolve(self, e, reds):
        """A closure expression with length() replaced by its constant, each sum() by a reduction
        slot (appended to `reds`), and constant subexpressions folded (+ - * / neg abs: the same
        IEEE operations the device would perform, so a constant Gamma shape is one CONST word)."""
        if isinstance(e, Len):
            return Const(float(self.length(e.a)))
        if isinstance(e, Reduce):
            if reds is None:
                raise ArgumentError("a sum() inside a sum() is not supported")
            reds.append(self.resolve(e.a, None))
            if len(reds) > abi.MMB_IR_MAX_RED:
                raise ArgumentError(f"at most {abi.MMB_IR_MAX_RED} sum()s per Sampler closure")
            return RedSlot(len(reds) - 1)
        if isinstance(e, Bin):
            a, b = self.resolve(e.a, reds), self.resolve(e.b, reds)
            if isinstance(a, Const) and isinstance(b, Const):
                x, y = np.float64(a.v), np.float64(b.v)
                with np.errstate(all="ignore"):
                    return Const(float({"+": x + y, "-": x - y, "*": x * y, "/": x / y}[e.op]))
            return Bin(e.op, a, b)
        if isinstance(e, Un):
            a = self.resolve(e.a, reds)
            if isinstance(a, Const) and e.op in ("neg", "abs"):
                return Const(-a.v if e.op == "neg" else abs(a.v))
            return Un(e.op, a)
        return e

    def gibbs(self, blk, s):
        m = self.m
        dist = s.traced
        if dist.fam not in _GIBBS_FAMILIES or len(dist.params) != 2:
            raise ArgumentError("a node-IR Sampler closure must return rand(Normal | InverseGamma | Gamma)")
        for a in s.argnames:
            self.kind(a)  # every closure argument is a node or an input
        reds = []
        ps = [self.resolve(p, reds) for p in dist.params]
        refs = set()
        for k, p in enumerate(ps):
            if self.length(p) != 1:
                raise ArgumentError(f"Sampler({s.params}): distribution parameter {k + 1} is not a scalar "
                                    "(reduce it with sum / sumabs2 / mean)")
        blk.gibbs_family = dist.fam
        blk.nred = len(reds)
        for r, x in enumerate(reds):
            n = self.length(x)
            blk.red_expr[r] = self.expr(x, n, refs)
            blk.red_len[r] = n
        for k, p in enumerate(ps):
            blk.gibbs_expr[k] = self.expr(p, 1, refs)

    def cat_table(self, n, N, refs):
        """cterm of Categorical node n: its probability table in the pool, or the state slots of the
        sampled Dirichlet node it reads (which makes n a target of that node)."""
        P = self.cat_state(n)
        if P is None:
            N.cterm = self.put(("catp", n), self.cat_p(n))
        else:
            refs.add(P)
            N.cterm = -2 - self.m.nodes[P].offset  # MMB_IR_CAT_STATE(off), include/mamba_hip.h
            self.m.no_predict[n] = f"a Categorical that reads the sampled node {P}"

    def run(self):
        m = self.m
        m.support = {}
        m.no_predict = {}
        ids = {n: i for i, n in enumerate(m.order)}
        nodes = (abi.IrNode * len(m.order))()
        parents = {}
        simulated_only = set()
        for n in m.order:
            N = nodes[ids[n]]
            N.expr[0] = N.expr[1] = N.expr[2] = -1
            N.cterm = -1
            N.lo = N.hi = 0.0
            d = m.defs[n]
            refs = set()
            if d.kind == "logical":
                e = m.traced[n]
                N.family, N.fixed, N.off = abi.MMB_IR_LOGICAL, 0, 0
                N.len = self.length(e)
                N.expr[0] = self.expr(e, N.len, refs)
                continue
            dist = m.traced[n]
            ln = m.lens[n]
            N.family, N.len = dist.fam, ln
            if n in m.params:
                N.fixed, N.off = 0, m.nodes[n].offset
            else:
                N.fixed, N.off = 1, self.put(("v", n), m.fixed_vals[n])
            ps = dist.params
            if dist.fam == abi.MMB_IR_ISONORMAL:
                N.expr[0] = self.expr(ps[0], ln, refs)
                if self.length(ps[1]) != 1:
                    raise ArgumentError(f"MvNormal sigma of {n} must be a scalar")
                N.expr[1] = self.expr(ps[1], 1, refs)
            elif dist.fam == abi.MMB_IR_BINOMIAL and n in m.params:
                # sampled: n as one data word, so that the engine can check every element's support
                nn = self.binomial_n(n)
                N.expr[0] = len(self.code)
                self.code += [self.word(abi.IR_OP["data"], self.put(("binn", n), nn)), 0]
                N.expr[1] = self.expr(ps[1], ln, refs)
            else:
                for k, p in enumerate(ps):
                    N.expr[k] = self.expr(p, ln, refs)
            if dist.fam == abi.MMB_IR_UNIFORM:
                lo, hi = self.host_value(ps[0], 1), self.host_value(ps[1], 1)
                if lo is None or hi is None:
                    if n in m.params:
                        raise ArgumentError(f"Uniform bounds of {n} must be constants or data")
                    # an observed Uniform node whose bounds read sampled nodes has no constant support to
                    # evaluate its density on: only ABC blocks, which simulate it from the bound expressions
                    # and never evaluate its density, may hold it as a target (checked below)
                    simulated_only.add(n)
                    N.lo = N.hi = float("nan")
                else:
                    N.lo, N.hi = float(lo[0]), float(hi[0])
            if dist.fam in _DISCRETE and n in m.params:
                # sampled by a DGS block: the support lo..hi, at most one value per lane of the group
                if dist.fam == abi.MMB_IR_POISSON:
                    raise ArgumentError(f"Poisson node {n} cannot be sampled (infinite support): observed only")
                lo, hi = self.support_bounds(n)
                if hi - lo + 1 > abi.MMB_DGS_MAX_SUPPORT:
                    raise ArgumentError(f"discrete node {n}: a support of {hi - lo + 1} values exceeds the "
                                        f"{abi.MMB_DGS_MAX_SUPPORT} that DGS enumerates")
                N.lo, N.hi = float(lo), float(hi)
                m.support[n] = (lo, hi)
                if dist.fam == abi.MMB_IR_BINOMIAL:
                    nn = self.binomial_n(n)
                    m.support[n] = (0, nn)
                    # lchoose(n_i, k), k = 0..max n, per element (0 past n_i: off the support)
                    N.cterm = self.put(("ct", n), [
                        math.lgamma(a + 1) - math.lgamma(k + 1) - math.lgamma(a - k + 1) if k <= a else 0.0
                        for a in nn for k in range(hi + 1)])
                elif dist.fam == abi.MMB_IR_CATEGORICAL:
                    self.cat_table(n, N, refs)
            elif dist.fam in (abi.MMB_IR_CATEGORICAL, abi.MMB_IR_DISCRETEUNIFORM):
                lo, hi = self.support_bounds(n)
                N.lo, N.hi = float(lo), float(hi)
                x = m.fixed_vals[n]
                if np.any(x != np.round(x)) or x.min() < lo or x.max() > hi:
                    raise ArgumentError(f"{n}: observations must be integers in {lo}..{hi}")
                if dist.fam == abi.MMB_IR_CATEGORICAL:
                    self.cat_table(n, N, refs)
            elif dist.fam == abi.MMB_IR_DIRICHLET:
                # one Dirichlet over the node's elements: alpha[len], then lmnB, in the pool
                if d.dim != 1:
                    raise ArgumentError(f"Dirichlet node {n}: one Dirichlet is a Stochastic(1, ...) vector node "
                                        "(arrays of Dirichlets are not lowered)")
                al = self.dirichlet_alpha(n)
                if al.size != ln:
                    raise ArgumentError(f"Dirichlet node {n}: alpha has {al.size} elements, the node {ln}")
                if not 2 <= ln <= abi.MMB_SIMPLEX_MAX:
                    raise ArgumentError(f"Dirichlet node {n}: 2..{abi.MMB_SIMPLEX_MAX} elements (it has {ln})")
                lmnb = math.fsum(math.lgamma(a) for a in al) - math.lgamma(math.fsum(al))
                N.cterm = self.put(("diralpha", n), list(al) + [lmnb])
                m.no_predict[n] = "a Dirichlet node"
                if n not in m.params and not _isprobvec(m.fixed_vals[n]):
                    raise ArgumentError(f"{n}: the observed value is not a probability vector")
            elif dist.fam in _DISCRETE:
                x = m.fixed_vals[n]
                if np.any(x != np.round(x)) or x.min() < 0:
                    raise ArgumentError(f"{n}: discrete observations must be non-negative integers")
                if dist.fam == abi.MMB_IR_BINOMIAL:
                    nn = self.host_value(ps[0], ln)
                    if nn is None:
                        raise ArgumentError(f"Binomial n of {n} must be data")
                    if np.any(x > nn):
                        raise ArgumentError(f"{n}: Binomial observations exceed n")
                    ct = [math.lgamma(a + 1) - math.lgamma(k + 1) - math.lgamma(a - k + 1) for a, k in zip(nn, x)]
                    N.cterm = self.put(("ct", n), ct)
                elif dist.fam == abi.MMB_IR_POISSON:
                    N.cterm = self.put(("ct", n), [-math.lgamma(k + 1) for k in x])
                elif np.any((x != 0) & (x != 1)):
                    raise ArgumentError(f"{n}: Bernoulli observations must be 0/1")
            parents[n] = refs
        node_fixed_reads = set(self.fixed_reads)  # (the Gibbs closures below read observed nodes too)
        # targets (stochastic children through logicals) and topological order
        children = {n: [c for c in m.stoch if n in parents[c]] for n in m.stoch}
        indeg = {n: builtins.sum(1 for p in parents[n] if p != n) for n in m.stoch}
        topo, ready = [], [n for n in m.stoch if indeg[n] == 0]
        while ready:
            ready.sort(key=lambda x: ids[x])
            n = ready.pop(0)
            topo.append(n)
            for c in children[n]:
                if c != n:
                    indeg[c] -= 1
                    if indeg[c] == 0:
                        ready.append(c)
        if len(topo) != len(m.stoch):
            raise ArgumentError("the model graph has a cycle")
        ir = abi.IrModel()
        for b, s in enumerate(m.samplers):
            targets = {c for p in s.params for c in children[p]}
            for t in sorted(targets & simulated_only):
                if s.kind != abi.MMB_SAMPLER_ABC:
                    raise ArgumentError(f"Uniform bounds of {t} must be constants or data: {s!r} evaluates its "
                                        "density (only ABC blocks, which simulate it, take such a node)")
            terms = [p for p in s.params if p not in targets] + [t for t in topo if t in targets]
            if len(terms) > abi.MMB_IR_MAX_TERMS:
                raise ArgumentError("too many nodes in one block's logpdf!")
            ir.blocks[b].nterms = len(terms)
            for t, nm in enumerate(terms):
                ir.blocks[b].term[t] = ids[nm]
                ir.blocks[b].trans[t] = int(nm in s.params)
            s.targets = [t for t in topo if t in targets]
            if s.kind == abi.MMB_SAMPLER_ABC:  # abc.jl:49-51: the data nodes, in the block's term order
                s.resolve_abc([(t, m.traced[t].fam, m.lens[t]) for t in terms if t not in s.params])
            if s.kind == abi.MMB_SAMPLER_GIBBS:
                self.gibbs(ir.blocks[b], s)
        mon, names = [], []
        for n in m.order:
            d = m.defs[n]
            if not d.monitor:
                continue
            N = nodes[ids[n]]
            mon.append(ids[n])
            names += [n] if (d.dim == 0 and N.len == 1) else [f"{n}[{i + 1}]" for i in range(N.len)]
        if self.depth > abi.MMB_IR_MAX_STACK:
            raise ArgumentError("node expression too deep")
        if not self.code:  # a model whose families take no parameter expression (Dirichlet, Categorical):
            self.code.append(0)  # the engine asks for a code table, one END word
        m.monitor_names = names
        m.topo = topo
        # the node table of the model statistics (Model.keys, modelstats.py): an output node is an
        # observed Stochastic node that no other node reads
        m.parents = parents
        m._stats = {"stoch": list(m.stoch), "output": [n for n in m.fixed if n not in node_fixed_reads],
                    "parents": parents, "sampled": set(m.params),
                    "monitored": {n for n in m.params if m.defs[n].monitor}, "ids": {n: ids[n] for n in m.stoch},
                    "names": {n: [n] if (m.defs[n].dim == 0 and nodes[ids[n]].len == 1)
                              else [f"{n}[{i + 1}]" for i in range(nodes[ids[n]].len)] for n in m.stoch},
                    "observed": {n: np.array(m.fixed_vals[n], dtype=np.float64).ravel() for n in m.fixed}}
        keep = {"nodes": nodes, "code": np.asarray(self.code, dtype=np.int32),
                "consts": np.asarray(self.consts + [0.0], dtype=np.float64),
                "pool": np.asarray(self.pool + [0.0], dtype=np.float64),
                "mon": np.asarray(mon + [0], dtype=np.int32)}
        ir.nvalues = m.nvalues
        ir.nnodes = len(m.order)
        ir.nodes = nodes
        ir.ncode = len(self.code)
        ir.code = keep["code"].ctypes.data_as(C.POINTER(C.c_int32))
        ir.nconst = len(self.consts)
        ir.consts = keep["consts"].ctypes.data_as(C.POINTER(C.c_double))
        ir.npool = len(self.pool)
        ir.pool = keep["pool"].ctypes.data_as(C.POINTER(C.c_double))
        ir.nmon = len(mon)
        ir.mon = keep["mon"].ctypes.data_as(C.POINTER(C.c_int32))
        ir.stack = self.depth
        m._ir, m._ir_keep = ir, keep


# ------------------------------------------------------------------ reference examples

def line_model():
    """doc/tutorial/line.jl:5-25 written in the IR (mu = xmat * beta as beta[1] + beta[2] x)."""
    return Model(
        y=Stochastic(1, lambda mu, s2: MvNormal(mu, sqrt(s2)), False),
        mu=Logical(1, lambda x, beta: beta[1] + beta[2] * x, False),
        beta=Stochastic(1, lambda: MvNormal(2, math.sqrt(1000))),
        s2=Stochastic(lambda: InverseGamma(0.001, 0.001)))


def rats_model():
    """doc/examples/rats.jl:48-97 (y rat-major, 1-based `rat` index, Xm = x[week] - xbar)."""
    return Model(
        y=Stochastic(1, lambda alpha, beta, rat, Xm, s2_c: MvNormal(alpha[rat] + beta[rat] * Xm, sqrt(s2_c)),
                     False),
        alpha=Stochastic(1, lambda mu_alpha, s2_alpha: Normal(mu_alpha, sqrt(s2_alpha)), False),
        alpha0=Logical(lambda mu_alpha, xbar, mu_beta: mu_alpha - xbar * mu_beta),
        mu_alpha=Stochastic(lambda: Normal(0.0, 1000), False),
        s2_alpha=Stochastic(lambda: InverseGamma(0.001, 0.001), False),
        beta=Stochastic(1, lambda mu_beta, s2_beta: Normal(mu_beta, sqrt(s2_beta)), False),
        mu_beta=Stochastic(lambda: Normal(0.0, 1000)),
        s2_beta=Stochastic(lambda: InverseGamma(0.001, 0.001), False),
        s2_c=Stochastic(lambda: InverseGamma(0.001, 0.001)))


def rats_scheme_gibbs_amm():
    """The headline Gibbs + AMM scheme (BASELINE configs[2]; the hand-lowered
    model.rats_scheme_gibbs_amm) with its conjugate blocks as the user closures of INTEGRATION.md
    §3 -- Sampler(params, f) in the style of doc/tutorial/line.jl:27-45 -- traced into node-IR
    Gibbs blocks: s2_c | alpha, beta, y; mu_alpha | alpha, s2_alpha (prior Normal(0, 1000));
    s2_alpha | alpha, mu_alpha (prior InverseGamma(0.001, 0.001)); mu_beta, s2_beta alike."""
    from .samplers import AMM
    s2_c = Sampler(["s2_c"], lambda alpha, beta, y, rat, Xm:
                   rand(InverseGamma(0.001 + length(y) / 2,
                                     0.001 + sumabs2(y - (alpha[rat] + beta[rat] * Xm)) / 2)))
    # prec = 1 / 1000^2 + length(x) / s2; rand(Normal(sum(x) / s2 / prec, sqrt(1 / prec)))
    mu_alpha = Sampler(["mu_alpha"], lambda alpha, s2_alpha:
                       rand(Normal(sum(alpha) / s2_alpha / (1 / 1000**2 + length(alpha) / s2_alpha),
                                   sqrt(1 / (1 / 1000**2 + length(alpha) / s2_alpha)))))
    s2_alpha = Sampler(["s2_alpha"], lambda alpha, mu_alpha:
                       rand(InverseGamma(0.001 + length(alpha) / 2, 0.001 + sumabs2(alpha - mu_alpha) / 2)))
    mu_beta = Sampler(["mu_beta"], lambda beta, s2_beta:
                      rand(Normal(sum(beta) / s2_beta / (1 / 1000**2 + length(beta) / s2_beta),
                                  sqrt(1 / (1 / 1000**2 + length(beta) / s2_beta)))))
    s2_beta = Sampler(["s2_beta"], lambda beta, mu_beta:
                      rand(InverseGamma(0.001 + length(beta) / 2, 0.001 + sumabs2(beta - mu_beta) / 2)))
    return [s2_c, AMM("alpha", np.eye(30)), mu_alpha, s2_alpha, AMM("beta", 0.01 * np.eye(30)), mu_beta, s2_beta]


def rats_inits_ls(chains, seed=1):
    """model.rats_init_ls (per-rat least-squares fits + jitter, the headline's inits) as the node
    IR's per-chain dict inits."""
    from .model import rats_init_ls, RATS_Y
    v = rats_init_ls(chains, seed=seed)  # [s2_c, alpha(30), mu_alpha, s2_alpha, beta(30), mu_beta, s2_beta]
    return [{"y": RATS_Y, "s2_c": v[k, 0], "alpha": v[k, 1:31], "mu_alpha": v[k, 31], "s2_alpha": v[k, 32],
             "beta": v[k, 33:63], "mu_beta": v[k, 63], "s2_beta": v[k, 64]} for k in range(chains)]


def rats_inputs():
    from .model import RATS_DATA
    x = np.asarray(RATS_DATA["x"])
    xbar = x.mean()
    i = np.arange(150)
    return {"y": RATS_DATA["y"], "rat": i // 5 + 1.0, "Xm": x[i % 5] - xbar, "xbar": xbar}


SEEDS = {  # doc/examples/seeds.jl:4-12
    "r": [10, 23, 23, 26, 17, 5, 53, 55, 32, 46, 10, 8, 10, 8, 23, 0, 3, 22, 15, 32, 3],
    "n": [39, 62, 81, 51, 39, 6, 74, 72, 51, 79, 13, 16, 30, 28, 45, 4, 12, 41, 30, 51, 7],
    "x1": [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    "x2": [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1]}


def seeds_model():
    """doc/examples/seeds.jl:16-56 (random-effect logistic regression, Binomial)."""
    return Model(
        r=Stochastic(1, lambda alpha0, alpha1, x1, alpha2, x2, alpha12, b, n:
                     Binomial(n, invlogit(alpha0 + alpha1 * x1 + alpha2 * x2 + alpha12 * x1 * x2 + b)), False),
        b=Stochastic(1, lambda s2: Normal(0, sqrt(s2)), False),
        alpha0=Stochastic(lambda: Normal(0, 1000)),
        alpha1=Stochastic(lambda: Normal(0, 1000)),
        alpha2=Stochastic(lambda: Normal(0, 1000)),
        alpha12=Stochastic(lambda: Normal(0, 1000)),
        s2=Stochastic(lambda: InverseGamma(0.001, 0.001)))


def seeds_inits():
    """doc/examples/seeds.jl:60-65"""
    r = SEEDS["r"]
    return [{"r": r, "alpha0": 0, "alpha1": 0, "alpha2": 0, "alpha12": 0, "s2": 0.01, "b": [0.0] * 21},
            {"r": r, "alpha0": 0, "alpha1": 0, "alpha2": 0, "alpha12": 0, "s2": 1, "b": [0.0] * 21}]


PUMPS = {"y": [5, 1, 5, 14, 3, 19, 1, 1, 4, 22],                       # doc/examples/pumps.jl:4-8
         "t": [94.3, 15.7, 62.9, 126, 5.24, 31.4, 1.05, 1.05, 2.1, 10.5]}


def pumps_model():
    """doc/examples/pumps.jl:12-39 (Gamma-Poisson hierarchical model)."""
    return Model(
        y=Stochastic(1, lambda theta, t: Poisson(theta * t), False),
        theta=Stochastic(1, lambda alpha, beta: Gamma(alpha, 1 / beta)),
        alpha=Stochastic(lambda: Exponential(1.0)),
        beta=Stochastic(lambda: Gamma(0.1, 1.0)))


SURGICAL = {"r": [0, 18, 8, 46, 8, 13, 9, 31, 14, 8, 29, 24],        # doc/examples/surgical.jl:4-8
            "n": [47, 148, 119, 810, 211, 196, 148, 215, 207, 97, 256, 360]}


def surgical_model():
    """doc/examples/surgical.jl:12-41 (random-effects logistic, Logical p and pop_mean)."""
    return Model(
        r=Stochastic(1, lambda n, p: Binomial(n, p), False),
        p=Logical(1, lambda b: invlogit(b)),
        b=Stochastic(1, lambda mu, s2: Normal(mu, sqrt(s2)), False),
        mu=Stochastic(lambda: Normal(0, 1000)),
        pop_mean=Logical(lambda mu: invlogit(mu)),
        s2=Stochastic(lambda: InverseGamma(0.001, 0.001)))


DYES_Y = [1545, 1440, 1440, 1520, 1580, 1540, 1555, 1490, 1560, 1495, 1595, 1550, 1605, 1510, 1560,
          1445, 1440, 1595, 1465, 1545, 1595, 1630, 1515, 1635, 1625, 1520, 1455, 1450, 1480, 1445]


def dyes_model():
    """doc/examples/dyes.jl:22-45 (variance components, MvNormal with a batch gather)."""
    return Model(
        y=Stochastic(1, lambda mu, batch, s2_within: MvNormal(mu[batch], sqrt(s2_within)), False),
        mu=Stochastic(1, lambda theta, s2_between: Normal(theta, sqrt(s2_between))),
        theta=Stochastic(lambda: Normal(0, 1000)),
        s2_within=Stochastic(lambda: InverseGamma(0.001, 0.001)),
        s2_between=Stochastic(lambda: InverseGamma(0.001, 0.001)))


def dyes_inputs():
    return {"y": DYES_Y, "batch": np.repeat(np.arange(1, 7), 5).astype(float)}


SALM = {"y": [15, 21, 29, 16, 18, 21, 16, 26, 33, 27, 41, 60, 33, 38, 41, 20, 27, 42],  # 3 x 6, column-major
        "x": [0.0, 10, 33, 100, 333, 1000],                                            # doc/examples/salm.jl:4-11
        "dose": np.repeat(np.arange(1, 7), 3).astype(float)}                          # column index of y[i, j]


def salm_model():
    """doc/examples/salm.jl:15-47 (Poisson log-linear dose response with plate effects; the
    node `lambda` is `lam` here, a Python keyword)."""
    return Model(
        y=Stochastic(2, lambda alpha, beta, gamma, x, dose, lam:
                     Poisson(exp(alpha + beta * log(x[dose] + 10) + gamma * x[dose] + lam)), False),
        alpha=Stochastic(lambda: Normal(0, 1000)),
        beta=Stochastic(lambda: Normal(0, 1000)),
        gamma=Stochastic(lambda: Normal(0, 1000)),
        lam=Stochastic(2, lambda s2: Normal(0, sqrt(s2)), False),
        s2=Stochastic(lambda: InverseGamma(0.001, 0.001)))


def salm_inits():
    """doc/examples/salm.jl:51-56"""
    y = SALM["y"]
    return [{"y": y, "alpha": 0, "beta": 0, "gamma": 0, "s2": 10, "lam": np.zeros(18)},
            {"y": y, "alpha": 1, "beta": 1, "gamma": 0.01, "s2": 1, "lam": np.zeros(18)}]


BLOCKER = {  # doc/examples/blocker.jl:4-17
    "rt": [3, 7, 5, 102, 28, 4, 98, 60, 25, 138, 64, 45, 9, 57, 25, 33, 28, 8, 6, 32, 27, 22],
    "nt": [38, 114, 69, 1533, 355, 59, 945, 632, 278, 1916, 873, 263, 291, 858, 154, 207, 251, 151, 174, 209,
           391, 680],
    "rc": [3, 14, 11, 127, 27, 6, 152, 48, 37, 188, 52, 47, 16, 45, 31, 38, 12, 6, 3, 40, 43, 39],
    "nc": [39, 116, 93, 1520, 365, 52, 939, 471, 282, 1921, 583, 266, 293, 883, 147, 213, 122, 154, 134, 218,
           364, 674]}


def blocker_model():
    """doc/examples/blocker.jl:21-64 (random-effects meta-analysis of 22 trials)."""
    return Model(
        rc=Stochastic(1, lambda mu, nc: Binomial(nc, invlogit(mu)), False),
        rt=Stochastic(1, lambda mu, delta, nt: Binomial(nt, invlogit(mu + delta)), False),
        mu=Stochastic(1, lambda: Normal(0, 1000), False),
        delta=Stochastic(1, lambda d, s2: Normal(d, sqrt(s2)), False),
        delta_new=Stochastic(lambda d, s2: Normal(d, sqrt(s2))),
        d=Stochastic(lambda: Normal(0, 1000)),
        s2=Stochastic(lambda: InverseGamma(0.001, 0.001)))


def blocker_inits():
    """doc/examples/blocker.jl:68-73"""
    b = BLOCKER
    return [{"rc": b["rc"], "rt": b["rt"], "d": 0, "delta_new": 0, "s2": 1, "mu": np.zeros(22), "delta": np.zeros(22)},
            {"rc": b["rc"], "rt": b["rt"], "d": 2, "delta_new": 2, "s2": 10, "mu": np.full(22, 2.0),
             "delta": np.full(22, 2.0)}]


EYES_Y = [529.0, 530.0, 532.0, 533.1, 533.4, 533.6, 533.7, 534.1, 534.8, 535.3,   # doc/examples/eyes.jl:4-13
          535.4, 535.9, 536.1, 536.3, 536.4, 536.6, 537.0, 537.4, 537.5, 538.3,
          538.5, 538.6, 539.4, 539.6, 540.4, 540.8, 542.0, 542.8, 543.0, 543.5,
          543.8, 543.9, 545.3, 546.2, 548.8, 548.7, 548.9, 549.0, 549.4, 549.9,
          550.6, 551.2, 551.4, 551.5, 551.6, 552.8, 552.9, 553.2]


def eyes_model(monitor_all=False):
    """doc/examples/eyes.jl:17-61 (two-component normal mixture with the weight P ~ Dirichlet(alpha)
    sampled).  The reference's lambda = [lambda0; lambda0 + theta] indexed by T is written
    lambda0 + theta * (T - 1) -- the same two values, bit for bit, for T in {1, 2} -- and monitored as the
    Logical `lam` = lambda0 + theta * step, step = [0, 1] (`lambda` is a Python keyword).
    `monitor_all` also monitors T, lambda0 and theta, which the example does not."""
    mon = bool(monitor_all)
    return Model(
        y=Stochastic(1, lambda lambda0, theta, T, s2: Normal(lambda0 + theta * (T - 1), sqrt(s2)), False),
        T=Stochastic(1, lambda P: Categorical(P), mon),
        P=Stochastic(1, lambda alpha: Dirichlet(alpha)),
        lam=Logical(1, lambda lambda0, theta, step: lambda0 + theta * step),
        lambda0=Stochastic(lambda: Normal(0.0, 1000.0), mon),
        theta=Stochastic(lambda: Uniform(0.0, 1000.0), mon),
        s2=Stochastic(lambda: InverseGamma(0.001, 0.001)))


def eyes_inputs():
    return {"alpha": [1.0, 1.0], "step": [0.0, 1.0]}


def eyes_inits(y=None):
    """doc/examples/eyes.jl:65-70 (`y`: other observations than the example's 48)."""
    y = EYES_Y if y is None else list(y)
    return [{"y": y, "T": [1.0] * len(y), "P": [0.5, 0.5], "lambda0": 535, "theta": 5, "s2": 10},
            {"y": y, "T": [1.0] * len(y), "P": [0.5, 0.5], "lambda0": 550, "theta": 1, "s2": 1}]


def eyes_scheme():
    """doc/examples/eyes.jl:74-77"""
    from .samplers import DGS, Slice, SliceSimplex
    return [DGS("T"), Slice(["lambda0", "theta"], [5.0, 1.0]), Slice("s2", 2.0, transform=True),
            SliceSimplex("P", scale=0.75)]


def line_abc_model():
    """doc/examples/line_abc.jl:13-20 written in the IR (xmat * beta as beta[1] + beta[2] x, inlined into y)."""
    return Model(
        y=Stochastic(1, lambda x, beta, s2: MvNormal(beta[1] + beta[2] * x, sqrt(s2)), False),
        beta=Stochastic(1, lambda: MvNormal(2, math.sqrt(100))),
        s2=Stochastic(lambda: InverseGamma(0.01, 0.01)))


def line_abc_inputs():
    """doc/examples/line_abc.jl:4-7 (y is the observed node's initial value: line_abc_inits)."""
    return {"x": [1.0, 2.0, 3.0, 4.0, 5.0]}


def line_abc_inits(chains, seed=1):
    """doc/examples/line_abc.jl:24-31: beta ~ Normal(0, 1), s2 ~ Gamma(1, 1) per chain."""
    rng = np.random.default_rng(seed)
    return [{"y": [1.0, 3.0, 3.0, 3.0, 5.0], "beta": rng.normal(0.0, 1.0, 2), "s2": float(rng.gamma(1.0, 1.0))}
            for _ in range(chains)]


def line_abc_scheme(maxdraw=100, nsim=3):
    """doc/examples/line_abc.jl:35-48: summary1 = identity, summary2 = x -> [mean(x); sqrt(var(x))]."""
    from .samplers import ABC, Epanechnikov
    return [ABC("beta", [0.5, 0.25], "identity", 0.5, kernel="Normal", maxdraw=maxdraw, nsim=nsim),
            ABC("s2", 0.5, ("mean", "std"), 0.1, kernel=Epanechnikov, maxdraw=maxdraw, nsim=nsim)]
