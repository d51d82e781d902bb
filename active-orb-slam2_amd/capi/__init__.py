"""ctypes binding of the C ABI declared in include/aos2.h (lib/libaos2.so, built by csrc/Makefile).

This is plumbing: numpy arrays in, numpy arrays out, every call goes through the extern "C" entry
points a C++/cgo/JNI caller would use.  There is no Python or CPU fallback: a missing library
raises LibraryMissing, a missing GPU surfaces as AosError(AOS2_ERR_NO_DEVICE).

_abi declares the ABI (checked against the header by tests/test_capi_layout_cpu.py), _core loads the library and holds the bench
harness, _build the pieces the argument builders share; the other modules wrap one section of the header each.  This file is the
flat surface: every public name, and the private ones that tests and tools use.
"""
import ctypes as C  # noqa: F401

from ._abi import *  # noqa: F401,F403
from ._abi import (_LbaProblem, _LbaResult, _LbaSystem, _LbaTrial, _LocalMapGraph, _PnpResult, _PosePassCase,  # noqa: F401
                   _SvcMotionsOut)
from ._core import (AosError, Graph, LibraryMissing, Runner, _check, _p, bind_to_device_node, device_count, device_local_cpus,  # noqa: F401
                    hip_runtime, host_empty, lib, lib_path, recording)
from .extractor import *  # noqa: F401,F403
from .frames import *  # noqa: F401,F403
from .kfdb import *  # noqa: F401,F403
from .local_map import *  # noqa: F401,F403
from .local_map import _kf_culling_view, _local_map_delta, _local_map_graph, _normal_depth_args  # noqa: F401
from .matcher import *  # noqa: F401,F403
from .optimisers import *  # noqa: F401,F403
from .optimisers import _GBA_SENTINEL_INT, _essential_graph_args, _sim3_opt_args, _sim3_opt_steps_args  # noqa: F401
from .planner import *  # noqa: F401,F403
from .solvers import *  # noqa: F401,F403
from .solvers import _init_args, _pnp_args, _sim3_args  # noqa: F401
from .taps import *  # noqa: F401,F403
