"""The device-side copy of columns without a GPU (samsim_copy_columns, samsim_apply_resample, samsim_get_copy_plan): the header, the
ctypes mirror, the Fortran binding and the library's symbols agree, the calls refuse what they can refuse without a handle, the plain
C++ part of samsim_amd/csrc/samsim_copy.h -- the functions the kernels call, compiled by g++, walked range by range as the kernels
walk them -- equals the numpy rule of tests/copy_reference.py, the grid rule tiles the blocks once, the scratch layout stays within
the constant, and the rule has the properties an in-place copy needs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi
from samsim_amd.capi import ApplyInfo
from tests import copy_reference as cr
from tests import resample_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("samsim_copy_columns", "samsim_apply_resample", "samsim_get_copy_plan")


def code_of_header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "samsim.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    h = cr.helper()
    assert h is not None, "needs g++, as tests/test_host_logic.py does"
    return h


def test_header_declares_the_functions_and_constants():
    code = " ".join(code_of_header().split())
    for decl in ("int samsim_copy_columns(samsim_handle *h, int64_t n, const int64_t *src , const int64_t *dst , int32_t what);",
                 "int samsim_apply_resample(samsim_handle *h, int32_t what, samsim_apply_info *info );",
                 "int samsim_get_copy_plan(samsim_handle *h, int64_t k0, int64_t nk, int64_t *src , int64_t *dst );"):
        assert decl in code, decl
    for name, value in (("SAMSIM_COPY_FORCING", 1), ("SAMSIM_COPY_TRACKS", 2), ("SAMSIM_COPY_SCORES", 4)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), code), name
    assert (capi.COPY_FORCING, capi.COPY_TRACKS, capi.COPY_SCORES) == (1, 2, 4)
    assert capi.copy_what() == 0 and capi.copy_what(True, True, True) == 7 and capi.copy_what(tracks=True) == 2
    assert "#define SAMSIM_COPY_SCRATCH_BYTES (64ull << 10)" in code and capi.COPY_SCRATCH_BYTES == 64 << 10
    assert "#define SAMSIM_ABI_VERSION 6" in code and capi.ABI_VERSION == 6
    # the draw's own comment points here instead of ruling the copy out
    text = open(os.path.join(ROOT, "include", "samsim.h")).read()
    draw = text[text.index("/* Posterior draws:"):text.index("#define SAMSIM_OFFSPRING_SLOT")]
    scope = draw[draw.index("Not in scope."):draw.index("Errors, all found")]
    assert "samsim_apply_resample" in scope and "device-side copy" not in scope


def test_struct_layout_matches_the_ctypes_mirror():
    code = code_of_header()
    body = code[code.index("typedef struct samsim_apply_info {"):code.index("} samsim_apply_info;")]
    names = []
    for decl in re.findall(r"\bint64_t\s+([^;]+);", body):
        names += [n.strip() for n in decl.split(",")]
    assert [(n, C.c_int64) for n in names] == list(ApplyInfo._fields_) and C.sizeof(ApplyInfo) == 32
    assert names == ["n_pool", "n_free", "n_copies", "n_sources"]


def test_fortran_binding_names_every_symbol():
    binding = open(os.path.join(ROOT, "host", "capi_binding.f90")).read()
    for name in FUNCTIONS:
        assert re.search(r"BIND\(C,\s*NAME\s*=\s*['\"]%s['\"]\)" % name, binding, re.I), name
    assert re.search(r"TYPE,\s*BIND\(C\)\s*::\s*samsim_apply_info\b", binding, re.I)
    assert "SAMSIM_COPY_FORCING = 1, SAMSIM_COPY_TRACKS = 2, SAMSIM_COPY_SCORES = 4" in binding


def test_the_makefile_builds_the_new_source():
    mk = open(os.path.join(ROOT, "samsim_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "samsim_copy.hip" in srcs and srcs[-1] == "samsim_capi.cpp"
    assert re.search(r"kernel-resource-usage -c -x hip samsim_copy\.hip", mk)
    # the step kernel does not see the copy
    kernels = open(os.path.join(ROOT, "samsim_amd", "csrc", "samsim_kernels.hip")).read()
    assert "samsim_copy" not in kernels


def test_library_exports_and_refuses_without_a_handle():
    so = samsim_amd.load()
    assert so.samsim_abi_version() == 6
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    sig = {"samsim_copy_columns": [vp, i64, vp, vp, i32], "samsim_apply_resample": [vp, i32, C.POINTER(ApplyInfo)],
           "samsim_get_copy_plan": [vp, i64, i64, vp, vp]}
    assert sorted(sig) == sorted(FUNCTIONS)
    f = {}
    for name, args in sig.items():
        f[name] = getattr(so, name)
        f[name].argtypes, f[name].restype = args, C.c_int
    src, dst = np.array([1, 2], dtype=np.int64), np.array([3, 4], dtype=np.int64)
    info = ApplyInfo(-7, -7, -7, -7)
    assert f["samsim_copy_columns"](None, 2, src.ctypes.data, dst.ctypes.data, 0) == -1
    assert f["samsim_copy_columns"](None, 2, None, None, 99) == -1
    assert f["samsim_apply_resample"](None, 0, C.byref(info)) == -1
    assert f["samsim_apply_resample"](None, 8, None) == -1
    assert f["samsim_get_copy_plan"](None, 0, 2, src.ctypes.data, dst.ctypes.data) == -1
    assert (info.n_pool, info.n_free, info.n_copies, info.n_sources) == (-7, -7, -7, -7)
    assert src.tolist() == [1, 2] and dst.tolist() == [3, 4]


# ------------------------------------------------------------------------------------------- the functions the kernels call
def helper_plan(lib, pool, N):
    n = N.size
    pool8 = np.ascontiguousarray(pool, dtype=np.uint8)
    Nd = np.ascontiguousarray(N, dtype=np.float64)
    src, dst = np.full(max(1, n), -7, dtype=np.int64), np.full(max(1, n), -7, dtype=np.int64)
    out = np.zeros(5, dtype=np.int64)
    ok = lib.h_plan(n, pool8.ctypes.data, Nd.ctypes.data, src.ctypes.data, dst.ctypes.data, out.ctypes.data)
    return ok, src, dst, out


def check_against_rule(lib, status, lab, group, N, what):
    r = cr.plan(N, status, lab, group)
    pool = cr.pool_of(status, lab, group)
    ok, src, dst, out = helper_plan(lib, pool, N)
    assert out.tolist() == [r["info"]["n_pool"], r["info"]["n_free"], r["info"]["n_copies"], r["info"]["n_sources"], r["n_bad"]], what
    assert bool(ok) == r["balanced"], what
    if ok:
        k = r["info"]["n_copies"]
        assert np.array_equal(src[:k], r["src"]) and np.array_equal(dst[:k], r["dst"]), what
        assert (src[k:] == -7).all() and (dst[k:] == -7).all(), what
    else:
        assert (src == -7).all() and (dst == -7).all(), what
    return r


def balanced_offspring(rng, pool, heavy=0):
    """an offspring row that sums to the pool size over the pool: a multinomial draw, `heavy` members with most of the weight"""
    idx = np.flatnonzero(pool)
    N = np.zeros(pool.size, dtype=np.int64)
    if idx.size:
        w = rng.exponential(1.0, idx.size)
        if heavy:
            w[rng.choice(idx.size, heavy, replace=False)] *= 50.0 * idx.size
        N[idx] = rng.multinomial(idx.size, w / w.sum())
    return N


@pytest.mark.parametrize("ncol", [1, 63, 64, 65, 300, 4197, 70001, 2 * 65536 + 1])
def test_the_plan_of_random_offspring_rows_equals_the_rule(lib, ncol):
    rng = np.random.default_rng(ncol)
    status = np.where(rng.uniform(size=ncol) < 0.02, 7, 0).astype(np.int32)
    lab = rng.integers(-1, 3, ncol).astype(np.int32)
    for group in (None, 1):
        pool = cr.pool_of(status, lab, group)
        for heavy in (0, 2):
            if heavy > pool.sum():
                continue
            N = balanced_offspring(rng, pool, heavy)
            r = check_against_rule(lib, status, lab, group, N, (ncol, group, heavy))
            assert r["balanced"] and r["info"]["n_copies"] == (np.maximum(N - 1, 0)).sum()
            if heavy and pool.sum() > 200:
                assert (N - 1 >= 64).any()                              # the write's cooperative path has work at this size
        # rows that do not balance: a draw of another size, and a drawn column that stopped
        N = balanced_offspring(rng, pool)
        if pool.sum() >= 2:
            c = int(np.flatnonzero(pool)[0])
            more = N.copy()
            more[c] += 1
            assert not check_against_rule(lib, status, lab, group, more, "m + 1")["balanced"]
            drawn = np.flatnonzero(N >= 1)
            st2 = status.copy()
            st2[drawn[0]] = 5
            r = check_against_rule(lib, st2, lab, group, N, "stopped survivor")
            assert not r["balanced"] and r["n_bad"] == 1


def test_the_edges_of_the_rule(lib):
    ncol = 64 * 3 + 37                                                    # a ragged last block
    status, one = np.zeros(ncol, dtype=np.int32), np.ones(ncol, dtype=np.int64)
    r = check_against_rule(lib, status, None, None, one, "all ones")
    assert r["balanced"] and r["info"] == dict(n_pool=ncol, n_free=0, n_copies=0, n_sources=0)
    for best in (0, 63, 64, ncol - 1):                                    # one family of everything, at the lanes that matter
        N = np.zeros(ncol, dtype=np.int64)
        N[best] = ncol
        r = check_against_rule(lib, status, None, None, N, ("one family", best))
        assert r["balanced"] and (r["src"] == best).all() and r["dst"].tolist() == [c for c in range(ncol) if c != best]
        assert r["info"] == dict(n_pool=ncol, n_free=ncol - 1, n_copies=ncol - 1, n_sources=1)
    # an empty pool: nothing to do, and that balances
    r = check_against_rule(lib, np.full(ncol, 3, dtype=np.int32), None, None, np.zeros(ncol, dtype=np.int64), "empty pool")
    assert r["balanced"] and r["info"] == dict(n_pool=0, n_free=0, n_copies=0, n_sources=0)
    # no draw (every offspring 0) over a pool that is not empty does not balance
    assert not check_against_rule(lib, status, None, None, np.zeros(ncol, dtype=np.int64), "no draw")["balanced"]
    # the last column alone is free, its copy comes from the first
    N = one.copy()
    N[0], N[-1] = 2, 0
    r = check_against_rule(lib, status, None, None, N, "last column")
    assert r["src"].tolist() == [0] and r["dst"].tolist() == [ncol - 1]
    # column by column
    pool = np.array([1, 1, 1, 1, 0, 0, 0], dtype=np.uint8)
    off = np.array([0.0, 1.0, 2.0, 65.0, 0.0, 1.0, 9.0])
    surplus, free_, source, bad = np.zeros(7, dtype=np.int64), *(np.zeros(7, dtype=np.uint8) for _ in range(3))
    lib.h_columns(7, pool.ctypes.data, off.ctypes.data, surplus.ctypes.data, free_.ctypes.data, source.ctypes.data, bad.ctypes.data)
    assert surplus.tolist() == [0, 0, 1, 64, 0, 0, 0] and free_.tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert source.tolist() == [0, 0, 1, 1, 0, 0, 0] and bad.tolist() == [0, 0, 0, 0, 0, 1, 1]


def test_the_grid_rule_and_the_scratch_layout(lib):
    part, free_, copies, result, nbytes, sz_part, sz_result, grid, bound, max_ncol, sz_info, piece, max_nlayer = (lib.h_layout(i) for i in range(13))
    assert grid == cr.GRID == rr.GRID == 1024 and bound == 64 << 10 and nbytes == lib.h_scratch_bytes() <= bound
    assert part == 0 and free_ >= part + sz_part * grid and copies >= free_ + 8 * grid and result >= copies + 8 * grid
    assert nbytes >= result + sz_result and sz_info == C.sizeof(ApplyInfo) and sz_result == sz_info + 8
    assert all(at % 8 == 0 for at in (free_, copies, result))
    out = (C.c_int64 * 3)()
    for ncol in (1, 63, 64, 65, 300, 4197, 70001, 65536, 65537, 1 << 20, (1 << 20) + 1, max_ncol - 1, max_ncol):
        lib.h_grid(ncol, out)
        assert (out[0], out[1], out[2]) == cr.grid_rule(ncol) == rr.grid_rule(ncol), ncol
        assert (out[2] - 1) * out[1] < out[0] <= out[2] * out[1] and 1 <= out[2] <= 1024, ncol
    assert cr.grid_rule(70001) == (1094, 2, 547)
    # a piece of the pair list is one launch of the layer kernel: within 2^30 threads, and never empty
    for nlayer in (3, 12, 80, max_nlayer):
        e = lib.h_piece_entries(nlayer)
        assert e >= 1 and e * capi.NARR * nlayer <= piece == 1 << 30 < (e + 1) * capi.NARR * nlayer


# ------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n", [4197, 70001])
def test_the_rule_has_the_properties_of_an_in_place_copy(n):
    rng = np.random.default_rng(n)
    w = np.where(rng.uniform(size=n) < 0.2, 0.0, rng.exponential(1.0, n))
    status = np.zeros(n, dtype=np.int32)
    status[[5, n - 1]] = 7
    lab = (np.arange(n) % 3).astype(np.int32)
    for group in (None, 1):
        pool = cr.pool_of(status, lab, group)
        for kind, u0, seed in (("systematic", 0.73, 0), ("stratified", 0.0, 2024)):
            N = rr.resample(w, status, lab, group, int(pool.sum()), kind, u0, seed)["offspring"]
            r = cr.plan(N, status, lab, group)
            src, dst = r["src"], r["dst"]
            assert r["balanced"] and src.size == dst.size > 100
            assert (np.diff(dst) > 0).all() and (np.diff(src) >= 0).all()
            assert not np.intersect1d(src, dst).size
            assert np.array_equal(np.bincount(src, minlength=n), np.maximum(N - 1, 0).astype(np.int64))
            assert pool[src].all() and pool[dst].all() and (N[dst] == 0).all() and (N[src] >= 2).all()
            # after the copy every pool column holds a drawn member, and member c is held N_c times
            holds = np.arange(n)
            holds[dst] = src
            assert np.array_equal(np.bincount(holds[pool], minlength=n), N.astype(np.int64))
            # a draw of another size does not balance
            N2 = rr.resample(w, status, lab, group, int(pool.sum()) + 1, kind, u0, seed)["offspring"]
            assert not cr.plan(N2, status, lab, group)["balanced"]
