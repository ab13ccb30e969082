"""jello_amd -- MI355X (gfx950) compute backend for the Jello/Vello 2D renderer hot path.

Python here is only glue for tests and benchmarks: the product is ``libjello_hip.so`` (HIP kernels
behind the C ABI of ``include/jello_hip.h``) plus ``libjello_host.so`` (the C++ mirror of Jello's
Scene / encoding / renderer recording surface).  See DESIGN.md and INTEGRATION.md.
"""
from ._lib import build, lib_paths, load_host, HostLibraryMissing  # noqa: F401
from .scene import (  # noqa: F401
    Scene, Path, Brush, Stroke, dash, Color, ColorStop, RenderParams, BumpSizes, Fill, Join, Cap, Mix, Compose, Extend, Aa,
)
from .engine import (  # noqa: F401
    Host, Recording, Engine, ImageFormat, Surface, YuvLayout, YuvMatrix, YuvRange, YuvTransfer, BlurEdge, blur_taps, ResampleFilter, resample_taps, MorphOp, MorphEdge, WarpFilter, WarpEdge, warp_plan, warp_bounds, ConvolveEdge, ConvolveMode, convolve_weights, LightKind, LightSource, lighting_plan, lighting_tables, TurbulenceKind, turbulence_plan, turbulence_tables, DisplaceChannel, displace_offset, ShadowFlags, shadow_plan, shadow_bounds, box_shadow_geometry, perspective_plan, perspective_bounds, ColorSpace, ColorFunc, color_tables, composite_clip, DistanceWhich, DistanceEdge, DistanceFlags, distance_plan, LoadAlpha, ChromaFilter, load_texels, load_yuv_codes, STAGE_NAMES, CMD,
)
from .engine import StatsWhat, StatsPopulation, StatsTransfer, stats_plan, stats_codes  # noqa: F401,E402
from .imagecalls import LUT3D_MIN_SIZE, LUT3D_MAX_SIZE, lut3d_identity, lut3d_texels  # noqa: F401,E402
from . import colorfilter  # noqa: F401,E402
from . import convolution  # noqa: F401,E402
from . import distance  # noqa: F401,E402
from . import lighting  # noqa: F401,E402
from . import lut3d  # noqa: F401,E402
from . import perspective  # noqa: F401,E402
from . import stats  # noqa: F401,E402
