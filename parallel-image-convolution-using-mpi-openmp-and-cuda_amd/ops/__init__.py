"""Stencil operators: native HIP/CPU dispatch and the NumPy oracle."""
from .stencil import Engine, StableInfo, convolve, convolve_until_stable, image_geometry, residual  # noqa: F401
from .stencil import BatchEngine, convolve_batch, convolve_batch_until_stable, residual_batch  # noqa: F401
from .stencil import convolve_many, convolve_many_until_stable, residual_many, size_buckets  # noqa: F401
from .stencil import unsharp, unsharp_batch, unsharp_many  # noqa: F401
from .reference import numpy_convolve, numpy_decimate, numpy_residual, numpy_step, numpy_unsharp  # noqa: F401
from .pyramid import Pyramid, pyramid, pyramid_sizes  # noqa: F401
