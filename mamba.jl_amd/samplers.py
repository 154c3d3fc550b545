"""Sampler constructors mirroring Mamba.jl's model-based sampler API.

Each constructor returns a `Sampler` (src/Mamba.jl:119-124: params, eval, tune,
targets) whose `eval` is a lowered HIP block update instead of a Julia closure.
Argument meaning, defaults and validation errors follow the reference:

  AMWG(params, sigma; adapt=:all, batchsize=50, target=0.44)   src/samplers/amwg.jl:47-61
  AMM(params, Sigma; adapt=:all, beta=0.05, scale=2.38)        src/samplers/amm.jl:45-59
  NUTS(params; dtype=:forward, target=0.6)                     src/samplers/nuts.jl:47-56
  Slice(params, width, Univariate|Multivariate; transform=false) src/samplers/slice.jl:47-58
  HMC(params, epsilon, L[, Sigma]; dtype=:forward)            src/samplers/hmc.jl:47-65
  MALA(params, epsilon[, Sigma]; dtype=:forward)              src/samplers/mala.jl:43-58
  RWM(params, scale, proposal=Normal)                          src/samplers/rwm.jl:49-63
  DGS(params)  -- discrete Gibbs sampling of discrete nodes      src/samplers/dgs.jl:56-80
                  (node-IR models; no tuning, nothing adapts)
  SliceSimplex(params, scale=1.0)  -- slice sampling of Dirichlet nodes on the simplex
                  (node-IR models; no tuning, nothing adapts)   src/samplers/slicesimplex.jl:24-58
  BMG(params, k=1), BMC3(params, k=1)  -- binary Metropolised Gibbs and binary MC3 on one Bernoulli
                  node (node-IR models; no tuning)            src/samplers/bmg.jl:42-50, bmc3.jl:42-50
  BIA(params, A, D, epsilon, decay=0.55, target=0.45)  -- binary individual adaptation; A and D
                  always adapt (node-IR models)               src/samplers/bia.jl:18-24, bia.jl:55-63
  BHMC(params, traveltime, refresh=False)  -- binary Hamiltonian Monte Carlo on one Bernoulli node
                  (node-IR models; the particle is the tune state)      src/samplers/bhmc.jl:35-43
  ABC(params, scale, summary, epsilon, kernel=SymUniform, dist=None, proposal=Normal, maxdraw=1, nsim=1,
      decay=1.0, randeps=False)  -- approximate Bayesian computation: no likelihood, the block's data
                  nodes are simulated and summarised (node-IR models)   src/samplers/abc.jl:23-29
  Gibbs(params)  -- a user `Sampler(params, f)` whose f is the node's conjugate full
                    conditional (doc/tutorial/line.jl:27-45); lowered per model.
"""
import math

import numpy as np

from . import abi

Univariate = "Univariate"
Multivariate = "Multivariate"

# RWM proposals: Normal and the SymDistributionTypes (src/distributions/extensions.jl:51-53)
Normal, SymUniform, SymTriangularDist = "Normal", "SymUniform", "SymTriangularDist"
Epanechnikov, Biweight, Triweight, Cosine = "Epanechnikov", "Biweight", "Triweight", "Cosine"
RWM_PROPOSALS = {Normal: abi.MMB_RWM_NORMAL, SymUniform: abi.MMB_RWM_SYMUNIFORM,
                 SymTriangularDist: abi.MMB_RWM_SYMTRIANGULAR, Epanechnikov: abi.MMB_RWM_EPANECHNIKOV,
                 Biweight: abi.MMB_RWM_BIWEIGHT, Triweight: abi.MMB_RWM_TRIWEIGHT, Cosine: abi.MMB_RWM_COSINE}


class ArgumentError(ValueError):
    """Julia ArgumentError raised by the reference's validators."""


def _params(params):
    if isinstance(params, str):
        return [params]
    return list(params)


def _adapt(adapt):
    adapt = str(adapt).lstrip(":")
    if adapt not in ("all", "burnin", "none"):
        raise ArgumentError("adapt must be one of :all, :burnin, or :none")
    return {"all": abi.MMB_ADAPT_ALL, "burnin": abi.MMB_ADAPT_BURNIN, "none": abi.MMB_ADAPT_NONE}[adapt]


class Sampler:
    def __init__(self, params, kind, adapt=abi.MMB_ADAPT_ALL, tuning=None, **kw):
        self.params = _params(params)
        self.kind = kind
        self.adapt = adapt
        self.tuning = None if tuning is None else np.atleast_1d(np.asarray(tuning, dtype=np.float64))
        self.form = kw.pop("form", abi.MMB_SLICE_MULTIVARIATE)
        self.transform = int(kw.pop("transform", False))
        self.batchsize = int(kw.pop("batchsize", 50))
        self.target = float(kw.pop("target", 0.44))
        self.beta = float(kw.pop("beta", 0.05))
        self.scale = float(kw.pop("scale", 2.38))
        self.epsilon = float(kw.pop("epsilon", 0.0))
        self.nsteps = int(kw.pop("nsteps", 0))
        self.gradient = int(kw.pop("gradient", abi.MMB_GRAD_DEFAULT))
        if kw:
            raise ArgumentError(f"unsupported sampler arguments {sorted(kw)}")
        self.targets = []

    def validate(self, dim):
        """validate(v) (amwg.jl:37-42, amm.jl:35-40, slice.jl:37-42)"""
        t = self.tuning
        if self.kind == abi.MMB_SAMPLER_AMWG and not (t.size == 1 or t.size == dim):
            raise ArgumentError(f"length(sigma) differs from variate length {dim}")
        if self.kind == abi.MMB_SAMPLER_AMM and t.size != dim * dim:
            raise ArgumentError(f"Sigma dimension differs from variate length {dim}")
        if self.kind == abi.MMB_SAMPLER_SLICE and not (t.size == 1 or t.size == dim):
            raise ArgumentError(f"length(width) differs from variate length {dim}")
        if self.kind in (abi.MMB_SAMPLER_HMC, abi.MMB_SAMPLER_MALA) and t is not None and t.size != dim * dim:
            raise ArgumentError(f"Sigma dimension differs from variate length {dim}")
        if self.kind == abi.MMB_SAMPLER_RWM and not (t.size == 1 or t.size == dim):  # rwm.jl:39-44
            raise ArgumentError(f"length(scale) differs from variate length {dim}")
        if self.kind in (abi.MMB_SAMPLER_BMG, abi.MMB_SAMPLER_BMC3):  # bmg.jl:26-37, bmc3.jl:26-37
            if isinstance(self.k, int):
                if self.k > dim:
                    raise ArgumentError(f"k exceeds variate length {dim}")
            elif max(max(ix) for ix in self.k) > dim:
                raise ArgumentError(f"indices in k exceed variate length {dim}")
            self.tuning = None if isinstance(self.k, int) else np.array(
                [float(sum({1 << (i - 1) for i in ix})) for ix in self.k])
        if self.kind == abi.MMB_SAMPLER_BIA:  # bia.jl:18-24 (defaults), bia.jl:36-50 (validate)
            a, dd, eps = self.bia
            eps = 0.01 / dim if eps is None else float(eps)
            a = np.full(dim, 1.0 / dim) if a is None else np.atleast_1d(np.asarray(a, dtype=np.float64)).ravel()
            dd = np.full(dim, 1.0 / dim) if dd is None else np.atleast_1d(np.asarray(dd, dtype=np.float64)).ravel()
            if not 0.0 < eps < 0.5:
                raise ArgumentError("epsilon is not in (0, 0.5)")
            for nm, v in (("A", a), ("D", dd)):
                if not (v.size == dim and np.all((eps < v) & (v < 1.0 - eps))):
                    raise ArgumentError(f"{nm} must contain {dim} probabilities in ({eps}, {1.0 - eps})")
            if not 0.5 < self.beta <= 1.0:
                raise ArgumentError("decay is not in (0.5, 1]")
            if not 0.0 < self.target < 1.0:
                raise ArgumentError("target is not in (0, 1)")
            self.epsilon = eps
            self.tuning = np.concatenate([a, dd])
        if self.kind == abi.MMB_SAMPLER_BHMC:
            if not 1 <= dim <= abi.MMB_BINARY_MAX:
                raise ArgumentError(f"a BHMC block holds a node of 1..{abi.MMB_BINARY_MAX} elements")
            # an update has at most dim (floor(traveltime / pi) + 2) wall events: the cap keeps that bounded
            if not (math.isfinite(self.scale) and 0.0 < self.scale <= abi.MMB_BHMC_MAX_TRAVELTIME):
                raise ArgumentError("traveltime is not finite, > 0 and <= 128 pi")

        if self.kind == abi.MMB_SAMPLER_ABC and not (self.abc_scale.size == 1 or self.abc_scale.size == dim):
            raise ArgumentError(f"length(scale) differs from variate length {dim}")

    def resolve_abc(self, data):
        """The block's data nodes, known once the model is lowered (ir.py): `data` lists (name, family, length)
        in the block's term order.  Checks them (abc.jl:49-58 and the documented caps) and fixes T."""
        if not data:
            raise ArgumentError(f"ABC({self.params}) needs at least one data node: a stochastic node among the "
                                "block's targets that is not one of its params")
        if len(data) > abi.MMB_ABC_MAX_DATA:
            raise ArgumentError(f"ABC({self.params}): at most {abi.MMB_ABC_MAX_DATA} data nodes")
        ident = self.abc_codes[0] == abi.MMB_ABC_IDENTITY
        needs2 = any(c in (abi.MMB_ABC_VAR, abi.MMB_ABC_STD) for c in self.abc_codes)
        T = 0
        for name, fam, ln in data:
            if fam not in ABC_DATA_FAMILIES:
                raise ArgumentError(f"ABC cannot simulate data node {name}: {ABC_REFUSED_FAMILIES.get(fam, 'such')} "
                                    "data nodes are not supported")
            if needs2 and ln < 2:
                raise ArgumentError(f"the var and std summaries need data nodes of >= 2 elements ({name} has {ln})")
            T += ln if ident else len(self.abc_codes)
        if not 1 <= T <= abi.MMB_ABC_MAX_T:
            raise ArgumentError(f"the total summary length {T} is not in 1..{abi.MMB_ABC_MAX_T}")
        self.abc_data, self.abc_T = [d[0] for d in data], T

    def spec_tuning(self, dim):
        """`tuning` as the block spec carries it: RWM's scalar scale is broadcast to the variate length
        (the engine takes scale[dim]); every other kind passes its vector as it is."""
        if self.kind == abi.MMB_SAMPLER_RWM and self.tuning.size == 1:
            return np.full(dim, self.tuning[0])
        if self.kind == abi.MMB_SAMPLER_ABC:  # scale[dim], then the summary codes
            sc = np.full(dim, self.abc_scale[0]) if self.abc_scale.size == 1 else self.abc_scale
            return np.concatenate([sc, np.asarray(self.abc_codes, dtype=np.float64)])
        return self.tuning

    def tune_len(self, dim):
        """Length of the block's canonical tune row (csrc/engine_tune.cpp tune_len_of) for a variate of
        `dim` elements."""
        tri = dim * (dim + 1) // 2
        if self.kind == abi.MMB_SAMPLER_ABC:  # [initialised, Tsim[nsim][T], epsilon[nsim], epsilonprime[nsim]]
            if getattr(self, "abc_T", None) is None:
                raise ArgumentError("an ABC block's tune row is known once its model has its initial values")
            return 1 + self.nsteps * (self.abc_T + 2)
        return {abi.MMB_SAMPLER_AMWG: 2 + 2 * dim, abi.MMB_SAMPLER_AMM: 4 + 2 * dim + 2 * tri, abi.MMB_SAMPLER_NUTS: 9,
                abi.MMB_SAMPLER_HMC: 2, abi.MMB_SAMPLER_MALA: 1, abi.MMB_SAMPLER_RWM: dim,
                abi.MMB_SAMPLER_BIA: 1 + 2 * dim, abi.MMB_SAMPLER_BHMC: 2 * dim + 3}.get(self.kind, 0)

    def __repr__(self):
        return f"{self.name}({self.params})"

    @property
    def name(self):
        return {1: "AMWG", 2: "AMM", 3: "NUTS", 4: "Slice", 5: "Gibbs", 6: "HMC", 7: "MALA", 8: "RWM", 9: "DGS",
                10: "SliceSimplex", 11: "BMG", 12: "BMC3", 13: "BIA", 14: "BHMC", 15: "ABC"}[self.kind]


def AMWG(params, sigma, adapt="all", batchsize=50, target=0.44):
    return Sampler(params, abi.MMB_SAMPLER_AMWG, _adapt(adapt), sigma, batchsize=batchsize,
                   target=target)


def AMM(params, Sigma, adapt="all", beta=0.05, scale=2.38):
    S = np.asarray(Sigma, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ArgumentError("Sigma must be a square matrix")
    # column-major, as Julia stores it
    return Sampler(params, abi.MMB_SAMPLER_AMM, _adapt(adapt), S.ravel(order="F"), beta=beta,
                   scale=scale)


def NUTS(params, dtype="forward", target=0.6):
    return Sampler(params, abi.MMB_SAMPLER_NUTS, abi.MMB_ADAPT_BURNIN, None, target=target,
                   gradient=_dtype(dtype))


def _dtype(dtype):
    """logpdfgrad! scheme (sampler.jl:97-111 -> simulation.jl:47-51, Calculus): "forward" (the
    reference's default) -> MMB_GRAD_FORWARD: Calculus forward differences on every model (line
    and the node IR inline; logistic as p + 1 log-density columns per request through the MFMA
    gradient kernel, lg_grad_kernel's LPONLY form, bit-exact vs the oracle), so a reference-default
    NUTS(:beta) on logistic runs on the GPU with the reference's own gradient; "analytic" -> the
    hand-derived gradient (line, logistic: the config-4 kernel's batched MFMA gradient).
    Calculus' :central / :complex are not on the device."""
    d = str(dtype).lstrip(":")
    if d == "forward":
        return abi.MMB_GRAD_FORWARD
    if d == "analytic":
        return abi.MMB_GRAD_ANALYTIC
    if d in ("central", "complex"):
        raise ArgumentError(f"dtype :{d} is not supported on the device (forward or analytic)")
    raise ArgumentError(f"unsupported dtype {dtype}")


def _sigma(Sigma):
    if Sigma is None:
        return None  # SigmaL = I (UniformScaling)
    S = np.asarray(Sigma, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ArgumentError("Sigma must be a square matrix")
    return S.ravel(order="F")


def HMC(params, epsilon, L, Sigma=None, dtype="forward"):
    """HMC(params, epsilon, L[, Sigma]; dtype) -- hmc.jl:47-55; tune [epsilon, L] (HMCTune)."""
    g = _dtype(dtype)
    if int(L) != L:
        raise ArgumentError("L must be an integer")
    return Sampler(params, abi.MMB_SAMPLER_HMC, abi.MMB_ADAPT_NONE, _sigma(Sigma), epsilon=epsilon,
                   nsteps=int(L), gradient=g)


def MALA(params, epsilon, Sigma=None, dtype="forward"):
    """MALA(params, epsilon[, Sigma]; dtype) -- mala.jl:43-51; tune [epsilon] (MALATune)."""
    g = _dtype(dtype)
    return Sampler(params, abi.MMB_SAMPLER_MALA, abi.MMB_ADAPT_NONE, _sigma(Sigma), epsilon=epsilon, gradient=g)


def Slice(params, width, form=Multivariate, transform=False):
    f = {Univariate: abi.MMB_SLICE_UNIVARIATE, Multivariate: abi.MMB_SLICE_MULTIVARIATE}.get(form)
    if f is None:
        raise ArgumentError("form must be Univariate or Multivariate")
    return Sampler(params, abi.MMB_SAMPLER_SLICE, abi.MMB_ADAPT_NONE, width, form=f,
                   transform=transform)


def RWM(params, scale, proposal=Normal):
    """RWM(params, scale; proposal=Normal) -- rwm.jl:49-63; tune scale[d] (RWMTune), no adaptation.
    `proposal`: Normal or a SymDistributionType name, in any letter case."""
    names = {k.lower(): v for k, v in RWM_PROPOSALS.items()}
    form = names.get(str(proposal).lstrip(":").lower())
    if form is None:
        raise ArgumentError(f"unsupported proposal {proposal}: one of {', '.join(RWM_PROPOSALS)}")
    sc = np.atleast_1d(np.asarray(scale, dtype=np.float64))
    if sc.ndim != 1 or not (np.isfinite(sc).all() and (sc >= 0.0).all()):
        raise ArgumentError("scale must be a finite non-negative scalar or vector")
    return Sampler(params, abi.MMB_SAMPLER_RWM, abi.MMB_ADAPT_NONE, sc, form=form, transform=True)


def DGS(params):
    """DGS(params) -- dgs.jl:56-80: each element of each discrete node of `params` is drawn from its full
    conditional, enumerated over the element's support (Bernoulli, Binomial, Categorical,
    DiscreteUniform; at most 32 values).  Node-IR models only.  The reference updates the keys one
    after another (dgs.jl:61-80), so a node-IR model lowers DGS(["a", "b"]) into one device block
    per node, in order (ir.Model.setsamplers).  No tuning state."""
    return Sampler(params, abi.MMB_SAMPLER_DGS, abi.MMB_ADAPT_NONE, None)


def SliceSimplex(params, scale=1.0):
    """SliceSimplex(params; scale=1.0) -- slicesimplex.jl:24-58: each Dirichlet node of `params` is updated
    by slice sampling on its simplex, the first simplex shrunk by `scale` in (0, 1] (validate,
    slicesimplex.jl:24-27).  Node-IR models only; like DGS, a node-IR model lowers
    SliceSimplex(["a", "b"]) into one device block per node, in order (slicesimplex.jl:37-54).  No tuning
    state, nothing adapts."""
    try:
        sc = float(scale)
    except (TypeError, ValueError):
        raise ArgumentError("scale is not in (0, 1]") from None
    if not 0.0 < sc <= 1.0:
        raise ArgumentError("scale is not in (0, 1]")
    return Sampler(params, abi.MMB_SAMPLER_SLICESIMPLEX, abi.MMB_ADAPT_NONE, None, scale=sc)


def _binary(name, kind, params, k):
    params = _params(params)
    if len(params) != 1:
        raise ArgumentError(f"{name}({params}) is one joint step over all the listed nodes in the reference, which a "
                            f"block of one node cannot restate: give {name} one node (one block per node is a "
                            "different sampler)")
    if isinstance(k, (int, np.integer)) and not isinstance(k, bool):
        k = int(k)
        if k < 1:
            raise ArgumentError("k must be at least 1")
        s = Sampler(params, kind, abi.MMB_ADAPT_NONE, None, form=abi.MMB_BINARY_K_INT, nsteps=k)
    else:
        try:
            ok = all(float(i) == int(i) and not isinstance(i, bool) for ix in k for i in ix)
            k = [[int(i) for i in ix] for ix in k]
        except (TypeError, ValueError):
            ok = False
        if not ok or any(len(ix) == 0 for ix in k):
            raise ArgumentError("k is an int or a list of non-empty lists of 1-based indices")
        if not 1 <= len(k) <= abi.MMB_BINARY_MAX_LISTS:
            raise ArgumentError(f"k holds 1..{abi.MMB_BINARY_MAX_LISTS} index lists")
        if min(min(ix) for ix in k) < 1:
            raise ArgumentError("indices in k start at 1")
        s = Sampler(params, kind, abi.MMB_ADAPT_NONE, None, form=abi.MMB_BINARY_K_LISTS)
    s.k = k
    return s


def BMG(params, k=1):
    """BMG(params; k=1) -- bmg.jl:42-50: binary Metropolised Gibbs on the one Bernoulli (or DiscreteUniform(0, 1))
    node of `params`, 1..32 elements.  k is the number of elements drawn without replacement for each
    update, or a list of 1-based index lists of which one is drawn (BMGForm, bmg.jl:5).  Node-IR models
    only.  No tuning state."""
    return _binary("BMG", abi.MMB_SAMPLER_BMG, params, k)


def BMC3(params, k=1):
    """BMC3(params; k=1) -- bmc3.jl:42-50: binary MC3, the elements of the drawn index set are flipped together;
    k as for BMG (BMC3Form, bmc3.jl:5).  Node-IR models only.  No tuning state."""
    return _binary("BMC3", abi.MMB_SAMPLER_BMC3, params, k)


def BIA(params, A=None, D=None, epsilon=None, decay=0.55, target=0.45):
    """BIA(params; A, D, epsilon, decay=0.55, target=0.45) -- bia.jl:55-63: binary individual adaptation.  The
    defaults are the reference's (bia.jl:18-24): A = D = 1 / n and epsilon = 0.01 / n for a node of n
    elements, so they and validate (bia.jl:36-50) are resolved once n is known (setinits); the
    default A = 1 / n does not pass validate for n = 1, as in the reference.  A and D adapt at every
    update; tune row [iter, A[n], D[n]].  Node-IR models only."""
    params = _params(params)
    if len(params) != 1:
        raise ArgumentError(f"BIA({params}) is one joint step over all the listed nodes in the reference, which a "
                            "block of one node cannot restate: give BIA one node")
    try:
        s = Sampler(params, abi.MMB_SAMPLER_BIA, abi.MMB_ADAPT_NONE, None, beta=decay, target=target)
    except (TypeError, ValueError):
        raise ArgumentError("decay and target are numbers") from None
    s.bia = (A, D, epsilon)
    return s


def BHMC(params, traveltime, refresh=False):
    """BHMC(params, traveltime) -- bhmc.jl:35-43: binary Hamiltonian Monte Carlo on the one Bernoulli (or
    DiscreteUniform(0, 1)) node of `params`, 1..32 elements.  The sampler's state is a particle (position and
    velocity per element), drawn once at the chain's first update and moved on from where the last update left
    it; the node's value is the side of each element's wall.  `traveltime` is finite, > 0 and at most 128 pi
    (the cap bounds an update's wall events; checked once the node's length is known).  refresh=False is the
    reference, which never redraws the velocity and so does not target the exact posterior; refresh=True (an
    extension: Pakman & Paninski's algorithm) redraws it at the start of every update.  Tune row
    [position[n], velocity[n], wallhits, wallcrosses, initialised].  Node-IR models only."""
    params = _params(params)
    if len(params) != 1:
        raise ArgumentError(f"BHMC({params}) is one joint move over all the listed nodes in the reference, which a "
                            "block of one node cannot restate: give BHMC one node")
    if isinstance(refresh, (bool, np.bool_)):
        refresh = bool(refresh)
    else:
        raise ArgumentError("refresh is True or False")
    try:
        s = Sampler(params, abi.MMB_SAMPLER_BHMC, abi.MMB_ADAPT_NONE, None, form=int(refresh), scale=traveltime)
    except (TypeError, ValueError):
        raise ArgumentError("traveltime is a number") from None
    s.traveltime, s.refresh = s.scale, refresh
    return s


ABC_SUMMARIES = {"identity": abi.MMB_ABC_IDENTITY, "sum": abi.MMB_ABC_SUM, "mean": abi.MMB_ABC_MEAN,
                 "var": abi.MMB_ABC_VAR, "std": abi.MMB_ABC_STD, "minimum": abi.MMB_ABC_MINIMUM,
                 "maximum": abi.MMB_ABC_MAXIMUM}
ABC_DATA_FAMILIES = (abi.MMB_IR_NORMAL, abi.MMB_IR_ISONORMAL, abi.MMB_IR_BERNOULLI, abi.MMB_IR_BINOMIAL,
                     abi.MMB_IR_POISSON, abi.MMB_IR_EXPONENTIAL, abi.MMB_IR_UNIFORM)
ABC_REFUSED_FAMILIES = {abi.MMB_IR_GAMMA: "Gamma", abi.MMB_IR_INVGAMMA: "InverseGamma", abi.MMB_IR_BETA: "Beta",
                        abi.MMB_IR_CATEGORICAL: "Categorical", abi.MMB_IR_DISCRETEUNIFORM: "DiscreteUniform",
                        abi.MMB_IR_DIRICHLET: "Dirichlet"}


def ABC(params, scale, summary, epsilon, kernel=SymUniform, dist=None, proposal=Normal, maxdraw=1, nsim=1, decay=1.0,
        randeps=False):
    """ABC(params, scale, summary, epsilon; kernel, dist, proposal, maxdraw, nsim, decay, randeps) -- abc.jl:23-147:
    approximate Bayesian computation on the continuous nodes of `params` (unlisted with transform).  Up to
    `maxdraw` candidates theta0 + scale .* rand(proposal(0, 1)) per update; for each, `nsim` data sets are
    simulated from the block's data nodes (the stochastic nodes among its targets that are not params),
    summarised, and weighed by kernel(0, tolerance) at the distance sqrt(sumabs2(Tsim - Tobs)) to the observed
    summaries; the tolerance decreases towards `epsilon` at rate `decay`, and with `randeps` is drawn from
    Exponential(tolerance).  `summary`: a name or a tuple of names out of identity (alone), sum, mean, var, std,
    minimum, maximum -- each data node's summary is the listed statistics, and the nodes' summaries are
    concatenated (at most 32 values).  `dist`: None, the reference's default.  `kernel`, `proposal`: Normal or a
    SymDistributionType name.  Tune row [initialised, Tsim[nsim][T], epsilon[nsim], epsilonprime[nsim]].
    Node-IR models only."""
    names = {k.lower(): v for k, v in RWM_PROPOSALS.items()}
    try:
        decay = float(decay)
    except (TypeError, ValueError):
        raise ArgumentError("decay is not in [0, 1]") from None
    if not 0.0 <= decay <= 1.0:
        raise ArgumentError("decay is not in [0, 1]")
    if dist is not None:
        raise ArgumentError("dist: only None, the reference's default sqrt(sumabs2(Tsim - Tobs)), is supported")
    kern = names.get(str(kernel).lstrip(":").lower())
    if kern is None:
        raise ArgumentError(f"unsupported kernel {kernel}: one of {', '.join(RWM_PROPOSALS)}")
    prop = names.get(str(proposal).lstrip(":").lower())
    if prop is None:
        raise ArgumentError(f"unsupported proposal {proposal}: one of {', '.join(RWM_PROPOSALS)}")
    if not isinstance(randeps, (bool, np.bool_)):
        raise ArgumentError("randeps is True or False")
    try:
        eps = float(epsilon)
    except (TypeError, ValueError):
        raise ArgumentError("epsilon is not finite and > 0") from None
    if not (math.isfinite(eps) and eps > 0.0):
        raise ArgumentError("epsilon is not finite and > 0")
    for nm, val, cap in (("maxdraw", maxdraw, abi.MMB_ABC_MAX_DRAW), ("nsim", nsim, abi.MMB_ABC_MAX_NSIM)):
        if isinstance(val, (bool, np.bool_)) or not isinstance(val, (int, np.integer)) or not 1 <= val <= cap:
            raise ArgumentError(f"{nm} is not an integer in 1..{cap}")
    codes = []
    for nm in ([summary] if isinstance(summary, str) else list(summary)):
        cd = ABC_SUMMARIES.get(str(nm).lstrip(":").lower()) if isinstance(nm, str) else None
        if cd is None:
            raise ArgumentError(f"unsupported summary {nm}: one of {', '.join(ABC_SUMMARIES)}")
        codes.append(cd)
    if not 1 <= len(codes) <= abi.MMB_ABC_MAX_SUMMARY:
        raise ArgumentError(f"summary lists 1..{abi.MMB_ABC_MAX_SUMMARY} statistics")
    if abi.MMB_ABC_IDENTITY in codes and len(codes) != 1:
        raise ArgumentError("the identity summary may only stand alone")
    try:
        sc = np.atleast_1d(np.asarray(scale, dtype=np.float64))
    except (TypeError, ValueError):
        raise ArgumentError("scale must be a finite non-negative scalar or vector") from None
    if sc.ndim != 1 or sc.size < 1 or not (np.isfinite(sc).all() and (sc >= 0.0).all()):
        raise ArgumentError("scale must be a finite non-negative scalar or vector")
    s = Sampler(params, abi.MMB_SAMPLER_ABC, abi.MMB_ADAPT_NONE, sc, form=prop | kern << 8 | int(bool(randeps)) << 16,
                transform=True, batchsize=int(maxdraw), nsteps=int(nsim), beta=decay, epsilon=eps)
    s.abc_scale, s.abc_codes, s.abc_T, s.abc_data = sc, codes, None, None
    s.maxdraw, s.nsim, s.decay, s.randeps = int(maxdraw), int(nsim), decay, bool(randeps)
    s.kernel, s.proposal = kern, prop
    return s


def Gibbs(params):
    return Sampler(params, abi.MMB_SAMPLER_GIBBS, abi.MMB_ADAPT_NONE, None)
