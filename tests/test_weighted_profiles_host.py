"""Weighted profile statistics and weighted covariances without a GPU: the reference of the GPU tests
(tests/weighted_profile_reference.py) against a brute-force triple loop on a hand-made State, unit weights against the unweighted
profile reference, and the boundary (header, exported symbols, ctypes wrappers, Fortran binding, ABI number).  The reductions
themselves are checked on the GPU (tests/test_gpu_weighted_profiles.py)."""
import ctypes as C
import math
import os
import re

import numpy as np

import samsim_amd
from samsim_amd import capi
from samsim_amd.capi import A, State
from tests import weighted_profile_reference as wpr
from tests.profile_reference import profile_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("samsim_get_weighted_profile_stats", "samsim_get_weighted_covariance")
NCOL, NLAYER = 7, 6
DZ, NBINS = 0.25, 8


def header():
    return open(os.path.join(ROOT, "include", "samsim.h")).read()


def hand_made():
    """seven columns of up to six layers: column 2 is stopped, column 4 has weight 0, column 5 has no active layer; thicknesses are
    multiples of 1/16 m (every depth is exact) and no column is thicker than 1.6875 m, so the last depth bin [1.75, 2) stays empty"""
    st = State.empty(NCOL, NLAYER)
    rng = np.random.default_rng(11)
    st.n_active[:] = [6, 3, 5, 4, 6, 0, 2]
    st.arr("thick")[:] = rng.integers(1, 5, size=(NLAYER, NCOL)) / 16.0
    st.arr("T")[:] = -rng.uniform(1.0, 20.0, size=(NLAYER, NCOL))
    st.arr("m")[:] = rng.uniform(50.0, 200.0, size=(NLAYER, NCOL))
    st.arr("S_abs")[:] = st.arr("m") * rng.uniform(1.0, 9.0, size=(NLAYER, NCOL))
    st.arr("m")[1, 0] = 0.0                                              # the stored S_bu is the value there
    st.arr("S_bu")[:] = 33.0
    st.arr("psi_l")[:] = rng.uniform(0.0, 0.4, size=(NLAYER, NCOL))
    status = np.array([0, 0, 99, 0, 0, 0, 0], dtype=np.int32)
    w = np.array([0.5, 2.0, 1.0, 0.125, 0.0, 3.0, 1e-3])
    labels = np.array([0, 1, 0, 0, 0, 1, -1], dtype=np.int32)
    assert float(st.arr("thick").sum(0).max()) <= 1.75
    return st, status, w, labels


def layer_value(st, name, k, c):
    if name != "S_bu":
        return float(st.arr(name)[k, c])
    m = float(st.arr("m")[k, c])
    return float(st.arr("S_abs")[k, c]) / m if m != 0.0 else float(st.arr("S_bu")[k, c])


def brute_force(st, status, w, labels, group, name, axis, origin, nbins, z0, dz):
    """per bin the list of (column, v, w) over the counting columns that contribute: loops over bins, columns and layers"""
    per_bin = []
    for b in range(nbins):
        members = []
        for c in range(st.ncol):
            if status[c] != 0 or not w[c] > 0.0 or (group is not None and labels[c] != group):
                continue
            na = int(st.n_active[c])
            if axis == "layer":
                k = b + 1 if origin == "top" else na - b
                if 1 <= k <= na:
                    members.append((c, layer_value(st, name, k - 1, c), w[c]))
                continue
            H = 0.0
            for k in range(na):
                H += float(st.arr("thick")[k, c])
            e0, e1 = z0 + b * dz, z0 + (b + 1) * dz
            Z, L, W = 0.0, 0.0, 0.0
            for k in range(na):
                Zn = Z + float(st.arr("thick")[k, c])
                lo, hi = (Z, Zn) if origin == "top" else (H - Zn, H - Z)
                o = max(0.0, min(hi, e1) - max(lo, e0))
                L += o
                W += o * layer_value(st, name, k, c)
                Z = Zn
            if L > 0.0:
                members.append((c, W / L, w[c]))
        per_bin.append(members)
    return per_bin


def test_reference_against_a_triple_loop_on_a_hand_made_state():
    st, status, w, labels = hand_made()
    seen_empty = seen_subset = 0
    for axis, nbins, kw in (("layer", NLAYER, {}), ("depth", NBINS, dict(z0=0.0, dz=DZ))):
        for origin in ("top", "bottom"):
            for group in (None, 0):
                names = ["T", "S_bu", "psi_l", "thick"]
                ref, who = wpr.weighted_profile_reference(st, status, w, names, labels, group, axis=axis, origin=origin, nbins=nbins, **kw)
                ok = wpr.counting(status, w, labels, group)
                assert not ok[2] and not ok[4] and ok[0]
                for name in names:
                    brute = brute_force(st, status, w, labels, group, name, axis, origin, nbins, kw.get("z0", 0.0), kw.get("dz", 1.0))
                    for b, members in enumerate(brute):
                        r = ref[name][b]
                        assert [c for c, _, _ in members] == who[name][b].tolist(), (axis, origin, group, name, b)
                        assert r["count"] == len(members)
                        if not members:
                            assert r.tobytes() == np.zeros((), dtype=capi.WSTAT_DTYPE).tobytes()
                            seen_empty += 1
                            continue
                        seen_subset += len(members) < ok.sum()
                        vs, ws = [v for _, v, _ in members], [x for _, _, x in members]
                        W = math.fsum(ws)
                        mean = math.fsum(x * v for v, x in zip(vs, ws)) / W
                        var = math.fsum(x * (v - mean) ** 2 for v, x in zip(vs, ws)) / W
                        assert r["sum_w"] == W and r["sum_w2"] == math.fsum(x * x for x in ws)
                        assert r["min"] == min(vs) and r["max"] == max(vs)
                        assert abs(r["mean"] - mean) <= 1e-14 * max(1.0, abs(mean)), (axis, origin, group, name, b)
                        assert abs(r["var"] - var) <= 1e-13 * max(1e-3, var), (axis, origin, group, name, b)
    assert seen_empty > 0 and seen_subset > 0
    # the weighting matters: a weighted mean is not the plain one
    ref, _ = wpr.weighted_profile_reference(st, status, w, ["T"], axis="layer", origin="top", nbins=NLAYER)
    plain = profile_reference(st, np.where(wpr.counting(status, w), 0, 1), ["T"], axis="layer", origin="top", nbins=NLAYER)
    assert ref["T"]["mean"][0] != plain["T"]["mean"][0] and ref["T"]["count"][0] == plain["T"]["count"][0] == 4


def test_unit_weights_reproduce_the_profile_reference():
    st, status, _, labels = hand_made()
    w = np.ones(NCOL)
    for axis, nbins, kw in (("layer", NLAYER, {}), ("depth", NBINS, dict(z0=0.0, dz=DZ))):
        for origin in ("top", "bottom"):
            names = ["T", "S_bu", "thick"]
            ref, _ = wpr.weighted_profile_reference(st, status, w, names, axis=axis, origin=origin, nbins=nbins, **kw)
            plain = profile_reference(st, status, names, axis=axis, origin=origin, nbins=nbins, **kw)
            for n in names:
                assert np.array_equal(ref[n]["count"], plain[n]["count"]) and (ref[n]["count"] > 0).any()
                assert (ref[n]["count"] == 0).any() or axis == "layer"      # (two columns hold all six layers)
                assert np.array_equal(ref[n]["min"], plain[n]["min"]) and np.array_equal(ref[n]["max"], plain[n]["max"])
                assert np.array_equal(ref[n]["sum_w"], plain[n]["count"].astype(np.float64))
                assert np.array_equal(ref[n]["sum_w2"], plain[n]["count"].astype(np.float64))
                assert (np.abs(ref[n]["mean"] - plain[n]["mean"]) <= 1e-14 * np.maximum(1.0, np.abs(plain[n]["mean"]))).all()
                assert (np.abs(np.sqrt(ref[n]["var"]) - plain[n]["std"]) <= 1e-12 * np.maximum(1e-3, plain[n]["std"])).all()


def test_covariance_reference_against_loops_and_numpy():
    rng = np.random.default_rng(5)
    n = 40
    rows = rng.normal(size=(3, n)) * np.array([1.0, 1e-2, 30.0])[:, None] + np.array([0.0, 270.0, -3.0])[:, None]
    rows[2] += 5.0 * rows[0]
    w = rng.uniform(0.0, 2.0, size=n)
    w[3] = 0.0
    ok = np.ones(n, dtype=bool)
    ok[7] = False
    cnt, sw, sw2, mean, cov = wpr.weighted_covariance_reference(rows, w, ok)
    use = [c for c in range(n) if ok[c] and w[c] > 0.0]
    assert cnt == len(use) == n - 2 and sw == math.fsum(w[c] for c in use) and sw2 == math.fsum(w[c] * w[c] for c in use)
    for i in range(3):
        mi = math.fsum(w[c] * rows[i, c] for c in use) / sw
        assert abs(float(mean[i]) - mi) <= 1e-14 * max(1.0, abs(mi))
        for j in range(3):
            mj = math.fsum(w[c] * rows[j, c] for c in use) / sw
            cij = math.fsum(w[c] * (rows[i, c] - mi) * (rows[j, c] - mj) for c in use) / sw
            sc = math.sqrt(float(cov[i, i]) * float(cov[j, j]))
            assert abs(float(cov[i, j]) - cij) <= 1e-12 * sc, (i, j)
    want = np.cov(rows[:, use], bias=True, aweights=w[use])
    assert (np.abs(cov.astype(np.float64) - want) <= 1e-12 * np.sqrt(np.outer(np.diag(want), np.diag(want)))).all()
    assert np.array_equal(cov, cov.T)
    # a column that does not count changes nothing; nothing counting gives zeros
    rows2 = rows.copy()
    rows2[:, 3], rows2[:, 7] = 1e9, -1e9
    again = wpr.weighted_covariance_reference(rows2, w, ok)
    assert again[0] == cnt and np.array_equal(again[3], mean) and np.array_equal(again[4], cov)
    none = wpr.weighted_covariance_reference(rows, np.zeros(n), ok)
    assert none[:3] == (0, 0.0, 0.0) and not none[3].any() and not none[4].any()


def test_header_wrappers_and_binding_declare_the_two_calls():
    text = header()
    assert "#define SAMSIM_ABI_VERSION 6" in text and capi.ABI_VERSION == 6
    m = re.search(r"^#define SAMSIM_WPROFILE_SCRATCH_BYTES\s+\((\d+)ull << 20\)", text, re.M)
    assert m and 1 <= int(m.group(1)) <= 16
    weights_block = text[text.index("samsim_get_weighted_histogram.  Edges"):text.index("#define SAMSIM_WEIGHT_SLOT")]
    scope = weights_block[weights_block.index("Not in scope."):weights_block.index("Errors, all found")]
    assert "beyond the regression identity" not in scope and "weighted\n *     covariances;" not in scope
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+samsim_get_weighted_profile_stats\s*\(\s*samsim_handle\s*\*\s*h\s*,\s*const\s+samsim_profile_request\s*\*\s*rq\s*,"
                     r"\s*int32_t\s+group\s*,\s*samsim_wstat\s*\*\s*out\s*\)", code)
    assert re.search(r"\bint\s+samsim_get_weighted_covariance\s*\(\s*samsim_handle\s*\*\s*h\s*,\s*int32_t\s+nslots\s*,\s*const\s+int32_t\s*\*\s*slots\s*,"
                     r"\s*int32_t\s+group\s*,\s*int64_t\s*\*\s*count\s*,\s*double\s*\*\s*sum_w\s*,\s*double\s*\*\s*sum_w2\s*,\s*double\s*\*\s*mean\s*,"
                     r"\s*double\s*\*\s*cov\s*\)", code)
    for method in ("weighted_profile_stats", "weighted_profile_stats_raw", "weighted_covariance", "weighted_covariance_raw"):
        assert callable(getattr(capi.Solver, method)), method
    binding = open(os.path.join(ROOT, "host", "capi_binding.f90")).read()
    for name in NAMES:
        assert re.search(rf"FUNCTION\s+{name}\s*\([^)]*\)\s*(&\s*)?BIND\(C,\s*name='{name}'\)", binding), name


def test_library_exports_them_and_refuses_null_arguments():
    """no handle, no device: each of the two calls answers SAMSIM_ERR_ARG from its argument checks and writes nothing"""
    lib = samsim_amd.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.samsim_abi_version() == 6
    rq = capi.ProfileRequest()
    rq.struct_size, rq.nbins, rq.narrays = C.sizeof(capi.ProfileRequest), 4, 1
    slots, count, out = (C.c_int32 * 2)(0, 1), C.c_int64(-7), np.full(64, -77.0)
    lib.samsim_get_weighted_profile_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.samsim_get_weighted_covariance.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    assert lib.samsim_get_weighted_profile_stats(None, C.addressof(rq), -1, out.ctypes.data) == -1
    p = out.ctypes.data
    assert lib.samsim_get_weighted_covariance(None, 2, C.addressof(slots), -1, C.addressof(count), p, p + 8, p + 16, p + 64) == -1
    assert count.value == -7 and (out == -77.0).all()
