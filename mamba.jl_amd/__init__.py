"""mamba_amd — MI355X-native many-chain MCMC engine for Mamba.jl's sampler hot path.

Python host mirror of the reference's model-based sampler API (src/samplers/*.jl,
src/model/mcmc.jl) over the C ABI of include/mamba_hip.h (libmambahip.so).  Every
sampling call runs the hand-written HIP kernels; there is no CPU fallback.

The package directory is `mamba.jl_amd/`; import it as `mamba_amd` via
`_mamba_path.load()` (the dot in the directory name is not importable directly).
"""
from . import abi, diag, gelman, ir, model, modelstats, samplers, summary  # noqa: F401
from .gelman import (Comm, cor_from_sums, cor_sharded, gelmandiag, gelmandiag_rccl, gelmandiag_sharded,  # noqa: F401
                     psrf_from_sums)
from .diag import (autocor, changerate_sharded, geweke_windows, geweke_z, gewekediag, heideldiag,  # noqa: F401
                   pcramer, rafterydiag)
from .summary import hpd_sharded, pool_summary, quantile_sharded, summarystats_sharded  # noqa: F401
from .modelstats import dic, dic_sharded, logpdf, logpdf_sharded  # noqa: F401
from .modelstats import predict, predict_moments_sharded, predict_sharded, predict_summary  # noqa: F401
from .mcmc import Chains, Engine, mcmc, mcmc_restart, read, write  # noqa: F401
from .model import line, logistic, rats  # noqa: F401
from .samplers import (ABC, AMM, AMWG, BHMC, BIA, BMC3, BMG, DGS, HMC, MALA, NUTS, RWM, ArgumentError, Gibbs, Multivariate, Sampler,  # noqa: F401
                       Slice, SliceSimplex, Univariate)
from .samplers import (Biweight, Cosine, Epanechnikov, Normal, SymTriangularDist, SymUniform,  # noqa: F401
                       Triweight)

__version__ = "0.1.0"
