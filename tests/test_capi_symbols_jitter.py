"""The library exports the jitter of the per-column parameters and the getter of the ocean rows, on a machine without a GPU; both
refuse what they can refuse without a handle."""
import ctypes as C

import numpy as np

import samsim_amd
from samsim_amd.capi import JitterInfo, JitterSpec, JitterTerm


def test_library_exports_jitter_and_get_ocean():
    so = samsim_amd.load()
    assert so.samsim_abi_version() == 6
    for name in ("samsim_jitter", "samsim_get_ocean"):
        assert hasattr(so, name), name
    jitter, get_ocean = so.samsim_jitter, so.samsim_get_ocean
    jitter.argtypes, jitter.restype = [C.c_void_p, C.POINTER(JitterSpec), C.POINTER(JitterInfo)], C.c_int
    get_ocean.argtypes, get_ocean.restype = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p], C.c_int
    spec = JitterSpec.make([JitterTerm.make("dT2m", 0.0, 0.9, 0.1)])
    info = JitterInfo(-7)
    assert jitter(None, C.byref(spec), C.byref(info)) == -1 and jitter(None, None, None) == -1
    assert info.n_written == -7
    buf = np.full(4, -7.0)
    assert get_ocean(None, 0, 4, buf.ctypes.data, buf.ctypes.data) == -1 and (buf == -7.0).all()
