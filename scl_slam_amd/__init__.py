"""scl_slam_amd -- MI355X-native Scan Context loop-closure engine (host-side Python mirror).

The product is the C-ABI shared library ``scl_slam_amd/lib/libscl_engine.so`` (HIP kernels
for gfx950 + host engine, see ``include/scl_engine.h``).  This package is a thin ctypes
binding over it that mirrors the reference's plugin interface (``scan_descriptor``,
include/descriptor.h:21-36) so tests and benchmarks read like the reference's call sites.
There is no CPU fallback: importing works anywhere, creating an engine needs a HIP device.
"""
from ._native import load_library, LIB_PATH, NativeLibraryError  # noqa: F401
from .engine import (  # noqa: F401
    SclConfig, SclError, ScanContextEngine, ScanContextDescriptor, IcpParams, QUERY_STAGED,
    RegistrationEval, RegistrationPlaneEval, PgoParams, PgoResult, MapStats, MAP_RECORD,
)
from .m2dp import M2dpConfig, M2dpEngine, M2dpError  # noqa: F401
from .fpfh import FpfhConfig, FpfhEngine, FpfhError  # noqa: F401
from .grsd import GrsdConfig, GrsdEngine, GrsdError  # noqa: F401

__all__ = [
    "load_library", "LIB_PATH", "NativeLibraryError", "SclConfig", "SclError",
    "ScanContextEngine", "ScanContextDescriptor", "IcpParams", "QUERY_STAGED", "RegistrationEval", "RegistrationPlaneEval",
    "PgoParams", "PgoResult", "MapStats", "MAP_RECORD",
    "M2dpConfig", "M2dpEngine", "M2dpError", "FpfhConfig", "FpfhEngine", "FpfhError",
    "GrsdConfig", "GrsdEngine", "GrsdError",
]
