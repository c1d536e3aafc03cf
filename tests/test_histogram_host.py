"""Ensemble histograms without a GPU: the boundary (header, exported symbols, ctypes mirror, Fortran binding, ABI number), the
host-side quantile brackets and the numpy reference itself.  The counts are checked on the GPU (tests/test_gpu_histogram.py)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi
from tests import hist_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("samsim_get_histogram", "samsim_get_profile_histogram")


def header():
    return open(os.path.join(ROOT, "include", "samsim.h")).read()


def test_header_declares_both_functions_the_struct_and_the_two_constants():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+samsim_get_histogram\s*\(\s*samsim_handle\s*\*\s*h\s*,\s*int32_t\s+slot\s*,\s*const\s+samsim_hist_bins\s*\*\s*vb\s*,"
                     r"\s*int32_t\s+by_group\s*,\s*int64_t\s*\*\s*counts\s*\)", text)
    assert re.search(r"\bint\s+samsim_get_profile_histogram\s*\(\s*samsim_handle\s*\*\s*h\s*,\s*const\s+samsim_profile_request\s*\*\s*rq\s*,"
                     r"\s*const\s+samsim_hist_bins\s*\*\s*vb\s*,\s*int32_t\s+group\s*,\s*int64_t\s*\*\s*counts\s*\)", text)
    assert re.search(r"typedef\s+struct\s+samsim_hist_bins\s*\{\s*int32_t\s+struct_size\s*;\s*int32_t\s+nvbins\s*;\s*double\s+v0\s*,\s*dv\s*;\s*\}"
                     r"\s*samsim_hist_bins\s*;", text)
    assert re.search(r"^#define SAMSIM_HIST_MAX_VBINS\s+254\s*$", text, re.M)
    m = re.search(r"^#define SAMSIM_HIST_SCRATCH_BYTES\s+\((\d+)ull << 20\)\s*$", text, re.M)
    assert m and 1 <= int(m.group(1)) <= 16


def test_python_mirror_matches_the_header():
    value = int(re.search(r"^#define SAMSIM_HIST_MAX_VBINS\s+(\d+)", header(), re.M).group(1))
    assert capi.HIST_MAX_VBINS == value == 254
    assert [n for n, _ in capi.HistBins._fields_] == ["struct_size", "nvbins", "v0", "dv"]
    assert [t for _, t in capi.HistBins._fields_] == [C.c_int32, C.c_int32, C.c_double, C.c_double]
    assert C.sizeof(capi.HistBins) == 24 and capi.HistBins.v0.offset == 8 and capi.HistBins.dv.offset == 16
    vb = capi.hist_bins(30, -1.5, 0.25)
    assert (vb.struct_size, vb.nvbins, vb.v0, vb.dv) == (24, 30, -1.5, 0.25)
    for method in ("histogram", "histogram_raw", "profile_histogram", "profile_histogram_raw"):
        assert callable(getattr(capi.Solver, method))


def test_fortran_host_binds_both_names():
    text = open(os.path.join(ROOT, "host", "capi_binding.f90")).read()
    for name in NAMES:
        assert re.search(rf"FUNCTION\s+{name}\s*\(.*BIND\(C,\s*name='{name}'\)", text), name
    driver = open(os.path.join(ROOT, "host", "host_driver.f90")).read()
    assert re.search(r"NAMELIST\s*/samsim_run/[^/]*\bhist_bins\b[^/]*\bhist_max\b", driver, re.S)


def test_library_exports_them_and_the_abi_version_stays_6():
    lib = samsim_amd.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.samsim_abi_version() == 6 and capi.ABI_VERSION == 6
    assert "#define SAMSIM_ABI_VERSION 6" in header()


def test_null_handle_is_refused_before_any_device_work():
    """no handle, no device: each of the two calls answers SAMSIM_ERR_ARG from its argument checks"""
    lib = samsim_amd.load()
    vb = capi.hist_bins(8, 0.0, 1.0)
    rq = capi.ProfileRequest()
    rq.struct_size, rq.nbins, rq.narrays = C.sizeof(capi.ProfileRequest), 4, 1
    out = np.zeros(64, dtype=np.int64)
    lib.samsim_get_histogram.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.samsim_get_profile_histogram.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert lib.samsim_get_histogram(None, 0, C.addressof(vb), 0, out.ctypes.data) == -1
    assert lib.samsim_get_profile_histogram(None, C.addressof(rq), C.addressof(vb), -1, out.ctypes.data) == -1


def order_statistic(data, q):
    r = max(1, math.ceil(q * len(data)))
    return np.sort(data)[r - 1]


def test_quantile_bracket_contains_the_exact_order_statistic():
    rng = np.random.default_rng(7)
    nv, v0, dv = 12, -0.5, 0.125
    for data in (rng.normal(0.2, 0.4, 1001), rng.uniform(-0.4, 0.9, 64), np.full(17, 0.25), rng.normal(0.2, 3.0, 500)):
        counts = hr.histogram_reference(data, nv, v0, dv)
        assert counts.sum() == len(data)
        for q in (0.0, 0.05, 0.5, 0.95, 1.0):
            lo, hi = capi.quantile_bracket(counts, v0, dv, q)
            x = order_statistic(data, q)
            assert lo <= x < hi, (q, lo, x, hi)
            assert hi == np.inf or lo == -np.inf or hi - lo == pytest.approx(dv)
    E = hr.edges(nv, v0, dv)
    assert np.array_equal(capi.hist_edges(nv, v0, dv), E)
    # a value on an edge belongs to the bin that begins there
    counts = hr.histogram_reference(np.array([E[3]]), nv, v0, dv)
    assert capi.quantile_bracket(counts, v0, dv, 0.5) == (E[3], E[4])


def test_quantile_bracket_outer_entries_are_unbounded():
    nv, v0, dv = 4, 0.0, 1.0
    low = np.array([5, 0, 0, 0, 0, 0])
    high = np.array([0, 0, 0, 0, 0, 3])
    assert capi.quantile_bracket(low, v0, dv, 0.5) == (-np.inf, 0.0)
    assert capi.quantile_bracket(high, v0, dv, 0.5) == (4.0, np.inf)
    both = np.array([1, 0, 2, 0, 0, 1])
    assert capi.quantile_bracket(both, v0, dv, 0.0) == (-np.inf, 0.0)
    assert capi.quantile_bracket(both, v0, dv, 0.5) == (1.0, 2.0)
    assert capi.quantile_bracket(both, v0, dv, 1.0) == (4.0, np.inf)


def test_quantile_bracket_refuses_an_empty_row_and_a_bad_q():
    with pytest.raises(ValueError):
        capi.quantile_bracket(np.zeros(6, dtype=np.int64), 0.0, 1.0, 0.5)
    for q in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            capi.quantile_bracket(np.array([0, 1, 2, 0]), 0.0, 1.0, q)


def test_numpy_reference_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    nv, v0, dv = 23, -0.3, 0.07
    E = [v0 + j * dv for j in range(nv + 1)]                 # python floats: the product is rounded, then the sum
    assert E == list(hr.edges(nv, v0, dv))
    v = rng.uniform(E[0] - 0.2, E[-1] + 0.2, 1000)
    v[10], v[11], v[12], v[13], v[14], v[15] = E[5], E[0] - 1.0, E[-1], E[-1] + 3.0, float("nan"), E[0]
    want = np.zeros(nv + 2, dtype=np.int64)
    for x in v:
        want[sum(1 for e in E if e <= x)] += 1
    got = hr.histogram_reference(v, nv, v0, dv)
    assert got.dtype == np.int64 and np.array_equal(got, want) and got.sum() == 1000
    idx = hr.entries(v, nv, v0, dv)
    assert idx[10] == 6 and idx[11] == 0 and idx[12] == nv + 1 and idx[13] == nv + 1 and idx[14] == 0 and idx[15] == 1
    assert got[0] > 1 and got[-1] > 2 and (got[1:-1] > 0).all()
    # per group, with stopped columns left out
    status = np.zeros(1000, dtype=np.int32)
    status[::97] = 99
    labels = (np.arange(1000) % 4).astype(np.int32)
    labels[::13] = -1
    per = hr.scalar_histogram_reference(v, status, nv, v0, dv, labels, 4)
    assert per.shape == (4, nv + 2) and per.sum() == ((status == 0) & (labels >= 0)).sum()
    assert np.array_equal(per[2], hr.histogram_reference(v[(status == 0) & (labels == 2)], nv, v0, dv))
    assert hr.scalar_histogram_reference(v, status, nv, v0, dv).sum() == (status == 0).sum()
