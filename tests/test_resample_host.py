"""The posterior draw without a GPU (samsim_resample, samsim_get_offspring, samsim_get_ancestors): the header, the ctypes mirror, the
Fortran binding and the library's symbols agree, the calls refuse what they can refuse without a handle, the plain C++ part of
samsim_amd/csrc/samsim_resample.h -- the functions the kernels call, compiled by g++ -- equals the numpy restatement
(tests/resample_reference.py), the grid rule tiles the blocks once, the scratch layout stays within the constant, and the
restatement has the properties a resampler must have."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi
from samsim_amd.capi import ResampleInfo, ResampleSpec
from tests import resample_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("samsim_resample", "samsim_get_offspring", "samsim_get_ancestors")
U0_LAST = 1.0 - 2.0 ** -53                    # the largest offset below 1


def code_of_header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "samsim.h")).read(), flags=re.S)


def fields_of(code, name):
    body = code[code.index("typedef struct %s {" % name):code.index("} %s;" % name)]
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
    out = []
    for ctype, decl in re.findall(r"\b(int32_t|int64_t|uint64_t|double)\s+([^;]+);", body):
        out += [(n.strip(), ctypes_of[ctype]) for n in decl.split(",")]
    return out


@pytest.fixture(scope="module")
def lib():
    h = rr.helper()
    assert h is not None, "needs g++, as tests/test_host_logic.py does"
    return h


def test_header_declares_the_functions_and_constants():
    code = " ".join(code_of_header().split())
    for decl in ("int samsim_resample(samsim_handle *h, const samsim_resample_spec *spec, samsim_resample_info *info );",
                 "int samsim_get_offspring(samsim_handle *h, int64_t col0, int64_t ncols, double *out );",
                 "int samsim_get_ancestors(samsim_handle *h, int64_t k0, int64_t nk, int64_t *out );"):
        assert decl in code, decl
    assert re.search(r"#define SAMSIM_OFFSPRING_SLOT 0x50000\b", code)
    assert re.search(r"#define SAMSIM_RESAMPLE_MAX_DRAWS 4194304\b", code) and capi.RESAMPLE_MAX_DRAWS == 4194304
    assert "#define SAMSIM_RESAMPLE_SCRATCH_BYTES (64ull << 10)" in code
    assert "enum samsim_resample_kind { SAMSIM_RESAMPLE_SYSTEMATIC = 0, SAMSIM_RESAMPLE_STRATIFIED = 1 };" in code
    assert capi.RESAMPLE_KINDS == {"systematic": 0, "stratified": 1} == rr.KINDS
    assert "#define SAMSIM_ABI_VERSION 6" in code and capi.ABI_VERSION == 6
    assert capi.offspring_slot() == 0x50000 > capi.weight_slot() and capi._slot(capi.offspring_slot()) == 0x50000


def test_struct_layouts_match_the_ctypes_mirrors():
    code = code_of_header()
    assert fields_of(code, "samsim_resample_spec") == list(ResampleSpec._fields_) and C.sizeof(ResampleSpec) == 40
    assert fields_of(code, "samsim_resample_info") == list(ResampleInfo._fields_) and C.sizeof(ResampleInfo) == 48
    s = ResampleSpec.make(1000, u0=0.25, group=2)
    assert (s.struct_size, s.kind, s.group, s.reserved, s.m, s.u0, s.seed) == (40, 0, 2, 0, 1000, 0.25, 0)
    s = ResampleSpec.make(7, "stratified", seed=(1 << 64) - 1)
    assert (s.kind, s.group, s.m, s.u0, s.seed) == (1, -1, 7, 0.0, (1 << 64) - 1)


def test_fortran_binding_names_every_symbol():
    binding = open(os.path.join(ROOT, "host", "capi_binding.f90")).read()
    for name in FUNCTIONS:
        assert re.search(r"BIND\(C,\s*NAME\s*=\s*['\"]%s['\"]\)" % name, binding, re.I), name
    for name in ("samsim_resample_spec", "samsim_resample_info"):
        assert re.search(r"TYPE,\s*BIND\(C\)\s*::\s*%s\b" % name, binding, re.I), name
    assert re.search(r"SAMSIM_OFFSPRING_SLOT\s*=\s*%d_c_int32_t" % 0x50000, binding)
    for name in ("SAMSIM_RESAMPLE_SYSTEMATIC = 0", "SAMSIM_RESAMPLE_STRATIFIED = 1", "SAMSIM_RESAMPLE_MAX_DRAWS = 4194304_c_int64_t"):
        assert name in binding, name


def test_library_exports_and_refuses_without_a_handle():
    so = samsim_amd.load()
    assert so.samsim_abi_version() == 6
    vp, i64 = C.c_void_p, C.c_int64
    sig = {"samsim_resample": [vp, C.POINTER(ResampleSpec), C.POINTER(ResampleInfo)], "samsim_get_offspring": [vp, i64, i64, vp],
           "samsim_get_ancestors": [vp, i64, i64, vp]}
    assert sorted(sig) == sorted(FUNCTIONS)
    f = {}
    for name, args in sig.items():
        f[name] = getattr(so, name)
        f[name].argtypes, f[name].restype = args, C.c_int
    spec, info = ResampleSpec.make(16), ResampleInfo(-7, -7, -7, -7, -7, -77.0)
    assert f["samsim_resample"](None, C.byref(spec), C.byref(info)) == -1
    assert f["samsim_resample"](None, None, None) == -1
    assert f["samsim_resample"](None, None, C.byref(info)) == -1
    assert (info.n_pos, info.m_drawn, info.n_survivors, info.max_offspring, info.argmax_offspring, info.sum_w) == (-7, -7, -7, -7, -7, -77.0)
    out, idx = np.full(8, -77.0), np.full(8, -77, dtype=np.int64)
    assert f["samsim_get_offspring"](None, 0, 4, out.ctypes.data) == -1
    assert f["samsim_get_ancestors"](None, 0, 4, idx.ctypes.data) == -1
    assert (out == -77.0).all() and (idx == -77).all()


# ------------------------------------------------------------------------------------------- the functions the kernels call
def test_the_mixer_equals_the_reference(lib):
    rng = np.random.default_rng(5)
    n = 100_000
    seed = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    k = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    seed[:4] = (0, 0, (1 << 64) - 1, (1 << 64) - 1)
    k[:4] = (0, (1 << 64) - 1, 0, (1 << 64) - 1)
    got = np.zeros(n, dtype=np.uint64)
    lib.h_mixes(n, seed.ctypes.data, k.ctypes.data, got.ctypes.data)
    assert np.array_equal(got, rr.mix(seed, k))
    for i in range(200):
        assert int(got[i]) == rr.mix_int(int(seed[i]), int(k[i])) == lib.h_mix(int(seed[i]), int(k[i]))
    # splitmix64 seeded with 0: its first outputs, as published with the generator
    assert [rr.mix_int(0, i) for i in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    u = rr.offset(seed, k)
    assert (u >= 0.0).all() and (u < 1.0).all() and lib.h_offset(int(seed[9]), int(k[9])) == u[9]
    assert 0.49 < u.mean() < 0.51


def random_cases(rng, n):
    """(t, m, u0, seed): m over the whole range, t within [0, m] -- integers, near-integers and the two ends among them"""
    m = np.where(rng.uniform(size=n) < 0.5, rng.integers(1, 200, n), rng.integers(1, capi.RESAMPLE_MAX_DRAWS + 1, n)).astype(np.int64)
    t = rng.uniform(size=n) * m
    how = rng.integers(0, 8, n)
    t = np.where(how == 0, np.floor(t), t)
    t = np.where(how == 1, np.nextafter(np.floor(t), np.inf), t)
    t = np.where(how == 2, np.maximum(np.nextafter(np.floor(t), -np.inf), 0.0), t)
    t[:3], m[:3] = (0.0, 5.0, 4194304.0), (5, 5, 4194304)                # t = 0, t = m
    t = np.minimum(t, m.astype(np.float64))
    u0 = rng.uniform(size=n)
    u0[rng.uniform(size=n) < 0.1] = 0.0
    u0[rng.uniform(size=n) < 0.1] = U0_LAST
    u0[rng.uniform(size=n) < 0.1] = 0.73
    seed = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return t, m, u0, seed


def test_both_counts_equal_the_reference(lib):
    rng = np.random.default_rng(6)
    n = 100_000
    t, m, u0, seed = random_cases(rng, n)
    got = np.zeros(n, dtype=np.int64)
    for kind in (rr.SYSTEMATIC, rr.STRATIFIED):
        lib.h_counts(kind, n, t.ctypes.data, m.ctypes.data, u0.ctypes.data, seed.ctypes.data, got.ctypes.data)
        if kind == rr.SYSTEMATIC:
            want = [rr.count_systematic(float(t[i]), int(m[i]), float(u0[i])) for i in range(n)]
        else:
            want = [rr.count_stratified(float(t[i]), int(m[i]), int(seed[i])) for i in range(n)]
        assert got.tolist() == want, kind
        assert (got >= 0).all() and (got <= m).all() and (got[t >= m] == m[t >= m]).all() and (got[t == 0.0] == 0).all()
    # the ends, one by one
    for m1 in (1, 64, 4194304):
        for u in (0.0, 0.73, U0_LAST):
            assert lib.h_count_systematic(0.0, m1, u) == 0 and lib.h_count_systematic(float(m1), m1, u) == m1
            assert lib.h_count_systematic(np.nextafter(float(m1), 0.0), m1, u) == (m1 if u < U0_LAST else m1 - 1)
        assert lib.h_count_stratified(0.0, m1, 99) == 0 and lib.h_count_stratified(float(m1), m1, 99) == m1
    assert lib.h_count_systematic(0.5, 4, 0.5) == 0 and lib.h_count_systematic(np.nextafter(0.5, 1.0), 4, 0.5) == 1
    assert lib.h_count_systematic(1.0, 4, 0.0) == 1 and lib.h_count_systematic(np.nextafter(1.0, 2.0), 4, 0.0) == 2


def test_both_counts_do_not_decrease_and_the_row_form_is_the_scalar_one(lib):
    rng = np.random.default_rng(7)
    n = 100_000
    for m in (1, 63, 4197, 210_004, capi.RESAMPLE_MAX_DRAWS):
        t = np.sort(rng.uniform(size=n)) * m
        t[:n // 4] = np.sort(np.round(t[:n // 4]))                        # exact integers among them
        t = np.sort(np.minimum(t, float(m)))
        t[0], t[-1] = 0.0, float(m)
        mm = np.full(n, m, dtype=np.int64)
        got = np.zeros(n, dtype=np.int64)
        for kind, u0, seed in ((0, 0.0, 0), (0, 0.73, 0), (0, U0_LAST, 0), (1, 0.0, 12345), (1, 0.0, (1 << 64) - 1)):
            uu, ss = np.full(n, u0), np.full(n, seed, dtype=np.uint64)
            lib.h_counts(kind, n, t.ctypes.data, mm.ctypes.data, uu.ctypes.data, ss.ctypes.data, got.ctypes.data)
            assert (np.diff(got) >= 0).all() and got[0] == 0 and got[-1] == m, (m, kind, u0, seed)
            assert np.array_equal(got, rr.counts(t, m, kind, u0, seed)), (m, kind, u0, seed)


def test_the_grid_rule_tiles_the_blocks_once(lib):
    max_ncol = lib.h_layout(10)
    assert max_ncol == ((1 << 32) - 1) // (8 * capi.NSCAL) and lib.h_layout(8) == rr.GRID == 1024
    edges = [1, 2, 63, 64, 65, 4197, 70001, 1023 * 64, 1023 * 64 + 1, 65536, 65537, 2 * 65536 - 1, 2 * 65536, 2 * 65536 + 1, 1 << 20,
             (1 << 20) + 1, 3 * 65536 + 64, max_ncol - 64, max_ncol - 1, max_ncol]
    out = (C.c_int64 * 3)()
    for ncol in edges:
        lib.h_grid(ncol, out)
        nblk, per, ranges = out[0], out[1], out[2]
        assert (nblk, per, ranges) == rr.grid_rule(ncol), ncol
        assert nblk == -(-ncol // 64) and per == -(-nblk // 1024) and 1 <= ranges <= 1024, ncol
        # range g owns [g * per, min((g + 1) * per, nblk)): none empty, no gap, no overlap, the last ends at nblk
        assert (ranges - 1) * per < nblk <= ranges * per, ncol
    assert rr.grid_rule(70001) == (1094, 2, 547) and rr.grid_rule(4197) == (66, 1, 66)


def test_the_scratch_layout_stays_within_the_constant(lib):
    sums, bases, total, part, result, nbytes, sz_part, sz_result, grid, bound = (lib.h_layout(i) for i in range(10))
    assert bound == 64 << 10 and nbytes == lib.h_scratch_bytes() <= bound
    assert sums == 0 and bases >= sums + 8 * grid and total >= bases + 8 * grid and part >= total + 8
    assert result >= part + sz_part * grid and nbytes >= result + sz_result
    assert sz_result == C.sizeof(ResampleInfo) and all(at % 8 == 0 for at in (bases, total, part, result))


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n", [4197, 70001])
def test_the_reference_has_the_properties_of_a_resampler(n):
    rng = np.random.default_rng(n)
    w = np.where(rng.uniform(size=n) < 0.2, 0.0, rng.exponential(1.0, n))
    status = np.zeros(n, dtype=np.int32)
    cases = [("systematic", u0, 0) for u0 in (0.0, 0.73, U0_LAST)] + [("stratified", 0.0, 2024)]
    for m in (1, 63, n, 3 * n + 1):
        for kind, u0, seed in cases:
            r = rr.resample(w, status, None, None, m, kind, u0, seed)
            N, anc, C_, W = r["offspring"], r["ancestors"], r["C"], r["W"]
            assert (np.diff(C_) >= 0.0).all() and C_[-1] == W and C_[0] == w[0]
            assert N.sum() == m == anc.size == r["info"]["m_drawn"] and (N >= 0).all()
            assert (np.diff(anc) >= 0).all() and np.array_equal(np.bincount(anc, minlength=n), N)
            assert (N[w == 0.0] == 0).all() and r["info"]["n_pos"] == (w > 0).sum()
            dev = np.abs(N - m * w / W).max()
            assert dev <= 1.0 if kind == "systematic" else dev < 2.0, (m, kind, u0, dev)
            assert r["info"]["max_offspring"] == N.max() and N[r["info"]["argmax_offspring"]] == N.max()
            assert (N[:r["info"]["argmax_offspring"]] < N.max()).all() and r["info"]["n_survivors"] == (N >= 1).sum()
    # unit weights, as many draws as columns: every column exactly once
    one = np.ones(n)
    for kind, u0, seed in (("systematic", 0.5, 0), ("stratified", 0.0, 7)):
        r = rr.resample(one, status, None, None, n, kind, u0, seed)
        assert (r["offspring"] == 1.0).all() and np.array_equal(r["ancestors"], np.arange(n)) and r["W"] == float(n)


def test_the_reference_on_hand_made_rows():
    status = np.array([0, 0, 7, 0, 0, 0], dtype=np.int32)
    w = np.array([1.0, 0.0, 5.0, 2.0, np.nan, 1.0])                      # the stopped column and the NaN do not count
    r = rr.resample(w, status, None, None, 8, "systematic", 0.5)
    assert r["W"] == 4.0 and r["C"].tolist() == [1.0, 1.0, 1.0, 3.0, 3.0, 4.0]
    assert r["offspring"].tolist() == [2.0, 0.0, 0.0, 4.0, 0.0, 2.0] and r["ancestors"].tolist() == [0, 0, 3, 3, 3, 3, 5, 5]
    assert r["info"] == dict(n_pos=3, m_drawn=8, n_survivors=3, max_offspring=4, argmax_offspring=3, sum_w=4.0)
    r = rr.resample(w, status, None, None, 2, "systematic", 0.0)         # points 0 and 1: t = 0.5, 1.5, 2
    assert r["ancestors"].tolist() == [0, 3]
    lab = np.array([0, 0, 0, 1, 1, 0], dtype=np.int32)
    r = rr.resample(w, status, lab, 1, 3, "stratified", seed=5)
    assert r["ancestors"].tolist() == [3, 3, 3] and r["info"]["n_pos"] == 1
    for bad in (np.zeros(6), np.array([1.0, np.inf, 1.0, 1.0, 1.0, 1.0])):
        r = rr.resample(bad, status, None, None, 5)
        assert r["info"]["m_drawn"] == 0 and not r["offspring"].any() and r["ancestors"].size == 0
        assert r["info"]["max_offspring"] == 0 and r["info"]["argmax_offspring"] == 0 and r["info"]["sum_w"] == r["W"]
