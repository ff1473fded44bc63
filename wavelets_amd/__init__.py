"""wavelets_amd - MI355X-native a-trous wavelet engine with the ``watroo`` Python API.

    from wavelets_amd import AtrousTransform, B3spline, Triangle, Coefficients, denoise, wow

mirrors ``from watroo import ...`` (/root/reference/watroo/__init__.py:1-2).  The arithmetic
runs in hand-written HIP kernels (wavelets_amd/csrc) behind the C ABI of
include/watroo_hip.h; see DESIGN.md and INTEGRATION.md.
"""
from .wavelets import *  # noqa: F401,F403
from .wavelets import atrous_convolution, sdev_loc, AbstractScalingFunction  # noqa: F401
from .utils import *  # noqa: F401,F403
from .sequence import map_frames, denoise_many, wow_many, transform_many  # noqa: F401  (sequences of frames: double-buffered over PCIe)

from .batch import transform_stack, denoise_stack, wow_stack, enhance_stack, richardson_lucy_stack  # noqa: F401  (stacks of same-shape frames: one launch per pass)
from .signals import transform_signals, denoise_signals, signals_eligible  # noqa: F401  (stacks of 1-D signals of one length: a workgroup per signal, the scales in LDS)
from .along import transform_along, denoise_along, along_eligible  # noqa: F401  (the 1-D transform along any axis of an array: a tile of neighbouring signals per workgroup)
from .wow_signals import wow_signals, wow_along, wow_signals_eligible  # noqa: F401  (wow of stacks of 1-D signals and along an axis: the per-scale loop of a signal in one launch)
from .cubes import transform_cube, denoise_cube, wow_cube, cube_eligible, cube64_eligible, wow_cube_eligible  # noqa: F401  ((Z, Y, X) cubes, float32 and float64 / integer: the x, y and z filters and the detail of a scale in one launch; wow's whitening of a scale in one more)
from .rng import normal_frames  # noqa: F401  (seeded standard-normal frames, filled on the GPU)
from . import resident  # noqa: F401  (transform_stack / denoise_stack from a device array to a device array: no PCIe crossing)
from .resident import DeviceArray  # noqa: F401

__version__ = '0.1.0'
