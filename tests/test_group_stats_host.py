"""Per-group ensemble statistics without a GPU: the boundary (header, exported symbols, ctypes mirror, Fortran binding, ABI
number).  The numbers themselves are checked on the GPU (tests/test_gpu_group_stats.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi
from samsim_amd import testcases as tcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("samsim_set_groups", "samsim_get_group_stats", "samsim_get_group_profile_stats")


def header():
    return open(os.path.join(ROOT, "include", "samsim.h")).read()


def test_header_declares_the_three_functions_and_the_two_constants():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+samsim_set_groups\s*\(\s*samsim_handle\s*\*\s*h\s*,\s*int32_t\s+ngroups\s*,\s*const\s+int32_t\s*\*\s*group_of_column\s*\)", text)
    assert re.search(r"\bint\s+samsim_get_group_stats\s*\(\s*samsim_handle\s*\*\s*h\s*,\s*int32_t\s+nslots\s*,\s*const\s+int32_t\s*\*\s*slots\s*,"
                     r"\s*samsim_stat\s*\*\s*out\s*\)", text)
    assert re.search(r"\bint\s+samsim_get_group_profile_stats\s*\(\s*samsim_handle\s*\*\s*h\s*,\s*const\s+samsim_profile_request\s*\*\s*rq\s*,"
                     r"\s*int32_t\s+group\s*,\s*samsim_stat\s*\*\s*out\s*\)", text)
    assert re.search(r"^#define SAMSIM_MAX_GROUPS\s+1024\s*$", text, re.M)
    assert re.search(r"^#define SAMSIM_GROUP_SCRATCH_BYTES\s+\(16ull << 20\)\s*$", text, re.M)


def test_python_mirror_matches_the_header():
    value = int(re.search(r"^#define SAMSIM_MAX_GROUPS\s+(\d+)", header(), re.M).group(1))
    assert capi.MAX_GROUPS == value == 1024
    for method in ("set_groups", "group_stats"):
        assert callable(getattr(capi.Solver, method))


def test_fortran_host_binds_the_three_names():
    text = open(os.path.join(ROOT, "host", "capi_binding.f90")).read()
    for name in NAMES:
        assert re.search(rf"FUNCTION\s+{name}\s*\(.*BIND\(C,\s*name='{name}'\)", text), name


def test_library_exports_them_and_the_abi_version_stays_6():
    lib = samsim_amd.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.samsim_abi_version() == 6 and capi.ABI_VERSION == 6
    assert "#define SAMSIM_ABI_VERSION 6" in header()


def test_null_handle_is_refused_before_any_device_work():
    """no handle, no device: each of the three calls answers SAMSIM_ERR_ARG from its argument checks"""
    lib = samsim_amd.load()
    lab = np.zeros(4, dtype=np.int32)
    slots = (C.c_int32 * 1)(0)
    out = np.zeros(4, dtype=capi.STAT_DTYPE)
    rq = capi.ProfileRequest()
    rq.struct_size = C.sizeof(capi.ProfileRequest)
    lib.samsim_set_groups.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.samsim_get_group_stats.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.samsim_get_group_profile_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert lib.samsim_set_groups(None, 1, lab.ctypes.data) == -1
    assert lib.samsim_get_group_stats(None, 1, C.addressof(slots), out.ctypes.data) == -1
    assert lib.samsim_get_group_profile_stats(None, C.addressof(rq), 0, out.ctypes.data) == -1


def test_without_a_gpu_the_calls_never_reach_a_device():
    """on a machine without a GPU there is no handle to label: hip_solver fails with -4 as it always did"""
    lib = samsim_amd.load()
    lib.samsim_device_count.restype = C.c_int
    if lib.samsim_device_count() > 0:
        pytest.skip("a GPU is present")
    cfg, _ = tcs.testcase1(1)
    with pytest.raises(samsim_amd.SamsimError) as e:
        samsim_amd.hip_solver(cfg, 4)
    assert e.value.code == -4


def test_python_mirror_derives_ngroups_and_refuses_labels_without_a_group():
    """Solver.set_groups on a Solver without a handle whose raw call records its arguments: ngroups defaults to max(label) + 1,
    labels that are all -1 need an explicit ngroups, None removes the labels"""
    seen = []

    class Recorder(capi.Solver):
        def __init__(self):
            self.ncol, self.ngroups = 6, 0

        def set_groups_raw(self, ngroups, labels):
            seen.append((ngroups, None if labels is None else labels.copy()))

        def close(self):
            pass
    s = Recorder()
    s.set_groups([0, 2, -1, 1, 2, 0])
    assert seen[-1][0] == 3 and seen[-1][1].dtype == np.int32 and seen[-1][1].tolist() == [0, 2, -1, 1, 2, 0]
    s.set_groups([0, 0, 0, 0, 0, 0], ngroups=5)
    assert seen[-1][0] == 5
    with pytest.raises(ValueError):
        s.set_groups([-1] * 6)
    s.set_groups([-1] * 6, ngroups=2)
    assert seen[-1][0] == 2
    s.set_groups(None)
    assert seen[-1] == (0, None)
