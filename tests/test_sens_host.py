"""Ensemble sensitivities without a GPU: the boundary (header, exported symbols, ctypes mirror, Fortran binding, ABI number), the
host helpers that turn second moments into slopes and correlations, and the extended-precision reference itself.  The moments are
checked on the GPU (tests/test_gpu_sens.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bench
import samsim_amd
from samsim_amd import capi
from samsim_amd.capi import A, S, State
from tests import sens_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("samsim_get_covariance", "samsim_get_profile_regression")


def header():
    return open(os.path.join(ROOT, "include", "samsim.h")).read()


def test_reference_equals_numpy_cov_on_random_data():
    rng = np.random.default_rng(3)
    rows = rng.normal(size=(5, 1000)) * np.array([1.0, 1e-3, 50.0, 1.0, 7.0])[:, None] + np.array([0.0, 270.0, -3.0, 1e4, 0.5])[:, None]
    rows[3] = 0.4 * rows[0] - 2.0 * rows[2] + rows[3]
    n, mean, cov = sr.covariance_matrix(rows)
    want = np.cov(rows, bias=True)
    assert n == 1000 and np.allclose(mean.astype(np.float64), rows.mean(axis=1), rtol=1e-13, atol=0.0)
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    assert (np.abs(cov.astype(np.float64) - want) <= 1e-12 * scale).all() and np.array_equal(cov, cov.T)
    k, mx, my, vx, vy, c = sr.pair_moments(rows[0], rows[3])
    assert k == 1000 and float(c) == float(cov[0, 3]) and float(vx) == float(cov[0, 0]) and float(vy) == float(cov[3, 3])
    assert sr.pair_moments([], []) == (0, 0, 0, 0, 0, 0)
    assert sr.covariance_matrix([np.zeros(0), np.zeros(0)])[0] == 0


def test_reference_reproduces_the_sensitivities_of_the_committed_ensemble():
    """sheba_ensemble_80.npz, 256 members 200 days from open water: the signal the device-side reductions are for"""
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80.npz")
    assert st.ncol == 256
    full = State.empty(st.ncol, st.nlayer)
    full.lay[:4] = st.lay
    full.scal[:] = st.scal
    full.scal[S["dT2m"]], full.scal[S["precip_scale"]] = pert
    full.n_active[:] = st.n_active
    status = np.zeros(st.ncol, dtype=np.int32)
    n, mean, cov = sr.covariance_reference(full, status, ["thickness", "thick_snow", "dT2m", "precip_scale"])
    r = capi.correlation(cov.astype(np.float64))
    print("correlations", r[0, 3], r[1, 3], r[0, 2])
    assert n == 256 and round(r[0, 3], 3) == -0.988 and round(r[1, 3], 4) == 0.9996 and round(r[0, 2], 2) == 0.17
    q = sr.profile_regression_reference(full, status, ["S_bu"], "precip_scale", axis="layer", origin="top")["S_bu"]
    _, rho = capi.slope_and_correlation(q)
    assert st.n_active.min() == 80 and np.array_equal(q["count"], np.full(80, 256))
    print("S_bu against precip_scale by layer", np.round(rho, 2))
    # +0.57 in the top layer, -0.95 and -0.98 where the interior begins (layers 38 and 39), below -0.94 down to layer 64, -0.22 in
    # layer 71 where the bottom layers begin: a profile of sensitivities
    assert [round(float(rho[k]), 2) for k in (0, 37, 38, 70)] == [0.57, -0.95, -0.98, -0.22]
    assert rho[37:64].max() < -0.94 and rho[37:64].min() > -0.995 and np.abs(rho[71:]).max() < 0.15
    # the per-bin moments of the predictor are those of the contributing columns
    k, mx, my, vx, vy, c = sr.pair_moments(pert[1], full.arr("S_abs")[0] / full.arr("m")[0])
    assert (q["count"][0], q["mean_x"][0], q["var_x"][0], q["cov"][0]) == (k, float(mx), float(vx), float(c))


def test_pair_stat_is_48_bytes_in_the_header_s_field_order():
    text = header()
    body = text[text.index("typedef struct samsim_pair_stat {"):text.index("} samsim_pair_stat;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, decl in re.findall(r"(int64_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), ctype) for n in decl.split(",")]
    assert [n for n, _ in fields] == [n for n, _ in capi.PairStat._fields_] == list(capi.PAIR_STAT_DTYPE.names)
    assert [t for _, t in fields] == ["int64_t"] + ["double"] * 5
    assert [t for _, t in capi.PairStat._fields_] == [C.c_int64] + [C.c_double] * 5
    assert C.sizeof(capi.PairStat) == capi.PAIR_STAT_DTYPE.itemsize == 48
    assert [capi.PAIR_STAT_DTYPE.fields[n][1] for n in capi.PAIR_STAT_DTYPE.names] == [getattr(capi.PairStat, n).offset for n in capi.PAIR_STAT_DTYPE.names]
    assert int(re.search(r"^#define SAMSIM_SENS_MAX_SLOTS\s+(\d+)\s*$", text, re.M).group(1)) == capi.SENS_MAX_SLOTS == 8
    m = re.search(r"^#define SAMSIM_SENS_SCRATCH_BYTES\s+\((\d+)ull << 20\)\s*$", text, re.M)
    assert m and 1 <= int(m.group(1)) <= 16
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+samsim_get_covariance\s*\(\s*samsim_handle\s*\*\s*h\s*,\s*int32_t\s+nslots\s*,\s*const\s+int32_t\s*\*\s*slots\s*,"
                     r"\s*int32_t\s+group\s*,\s*int64_t\s*\*\s*count\s*,\s*double\s*\*\s*mean\s*,\s*double\s*\*\s*cov\s*\)", text)
    assert re.search(r"\bint\s+samsim_get_profile_regression\s*\(\s*samsim_handle\s*\*\s*h\s*,\s*const\s+samsim_profile_request\s*\*\s*rq\s*,"
                     r"\s*int32_t\s+predictor_slot\s*,\s*int32_t\s+group\s*,\s*samsim_pair_stat\s*\*\s*out\s*\)", text)
    for method in ("covariance", "covariance_raw", "profile_regression", "profile_regression_raw"):
        assert callable(getattr(capi.Solver, method))


def test_host_helpers_on_a_hand_made_case():
    cov = np.array([[4.0, -3.0], [-3.0, 9.0]])
    assert np.array_equal(capi.correlation(cov), np.array([[1.0, -0.5], [-0.5, 1.0]]))
    assert np.array_equal(capi.correlation(np.array([[0.0, 0.0], [0.0, 9.0]])), np.array([[0.0, 0.0], [0.0, 1.0]]))
    with pytest.raises(ValueError):
        capi.correlation(np.zeros((2, 3)))
    q = np.zeros(4, dtype=capi.PAIR_STAT_DTYPE)
    q[0] = (10, 1.0, 2.0, 4.0, 9.0, -3.0)
    q[1] = (10, 1.0, 2.0, 0.0, 9.0, 0.0)          # the predictor does not vary: no slope, no correlation
    q[2] = (10, 1.0, 2.0, 4.0, 0.0, 0.0)          # the value does not vary: slope 0, no correlation
    slope, rho = capi.slope_and_correlation(q)   # q[3]: an empty bin
    assert slope.tolist() == [-0.75, 0.0, 0.0, 0.0] and rho.tolist() == [-0.5, 0.0, 0.0, 0.0]


def test_fortran_host_binds_both_names():
    text = open(os.path.join(ROOT, "host", "capi_binding.f90")).read()
    for name in NAMES:
        assert re.search(rf"FUNCTION\s+{name}\s*\(.*BIND\(C,\s*name='{name}'\)", text), name
    assert re.search(r"TYPE,\s*BIND\(C\)\s*::\s*samsim_pair_stat", text)
    driver = open(os.path.join(ROOT, "host", "host_driver.f90")).read()
    assert re.search(r"NAMELIST\s*/samsim_run/[^/]*\bsens\b", driver, re.S)


def test_library_exports_them_and_the_abi_version_stays_6():
    lib = samsim_amd.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.samsim_abi_version() == 6 and capi.ABI_VERSION == 6
    assert "#define SAMSIM_ABI_VERSION 6" in header()


def test_null_arguments_are_refused_before_any_device_work():
    """no handle, no device: each of the two calls answers SAMSIM_ERR_ARG from its argument checks"""
    lib = samsim_amd.load()
    rq = capi.ProfileRequest()
    rq.struct_size, rq.nbins, rq.narrays = C.sizeof(capi.ProfileRequest), 4, 1
    slots, count, out = (C.c_int32 * 2)(0, 1), C.c_int64(0), np.zeros(64)
    lib.samsim_get_covariance.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.samsim_get_profile_regression.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    assert lib.samsim_get_covariance(None, 2, C.addressof(slots), -1, C.addressof(count), out.ctypes.data, out.ctypes.data) == -1
    assert lib.samsim_get_profile_regression(None, C.addressof(rq), 0, -1, out.ctypes.data) == -1
