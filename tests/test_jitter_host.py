"""The rejuvenation of the resampled ensemble without a GPU (samsim_jitter, samsim_get_ocean): the header, the ctypes mirror and the
Makefile agree; samsim_amd/csrc/samsim_jitter.h -- the functions the kernel calls, compiled alone by g++ -- equals the numpy rule of
tests/jitter_reference.py bit for bit in its integer part and within 4 ulp in its deviate; the deviates are standard normal and
uncorrelated across targets and columns at bounds that follow from the sample size; the value rule on hand-made cases; the checks of a
spec in the documented order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from samsim_amd import capi
from samsim_amd.capi import JT, JitterInfo, JitterSpec, JitterTerm
from tests import jitter_reference as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NCOL = ((1 << 32) - 1) // (8 * capi.NSCAL)
INF = np.inf


@pytest.fixture(scope="module")
def lib():
    h = jr.helper()
    assert h is not None, "needs g++, as tests/test_host_logic.py does"
    return h


def code_of_header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "samsim.h")).read(), flags=re.S)


# ------------------------------------------------------------------------------------------------ header, mirror, Makefile
def test_header_declares_the_functions_and_constants(lib):
    code = " ".join(code_of_header().split())
    for decl in ("int samsim_jitter(samsim_handle *h, const samsim_jitter_spec *spec, samsim_jitter_info *info );",
                 "int samsim_get_ocean(samsim_handle *h, int64_t col0, int64_t ncols, double *dfl_q_bottom , double *S_bu_bottom );",
                 "#define SAMSIM_JITTER_MAX_TERMS 4", "#define SAMSIM_JITTER_MAX_ATTEMPTS 32", "#define SAMSIM_OCEAN_SLOT(i) (0x60000 + (i))",
                 "enum samsim_jitter_target { SAMSIM_JT_DT2M = 0, SAMSIM_JT_PRECIP_SCALE, SAMSIM_JT_DFL_Q_BOTTOM, SAMSIM_JT_S_BU_BOTTOM };",
                 "enum samsim_jitter_which { SAMSIM_JITTER_POOL = 0, SAMSIM_JITTER_COPIES = 1 };",
                 "#define SAMSIM_ABI_VERSION 6"):
        assert decl in code, decl
    assert capi.JITTER_TARGETS == ["dT2m", "precip_scale", "dfl_q_bottom", "S_bu_bottom"] and capi.JITTER_WHICH == {"pool": 0, "copies": 1}
    assert capi.ocean_slot("dfl_q_bottom") == 0x60000 and capi.ocean_slot("S_bu_bottom") == 0x60001 == lib.h_layout(12)
    assert capi.jitter_slot("dT2m") == capi.S["dT2m"] and capi.jitter_slot(3) == 0x60001
    assert (lib.h_layout(10), lib.h_layout(11)) == (capi.JITTER_MAX_TERMS, capi.JITTER_MAX_ATTEMPTS) == (4, 32)


def test_struct_layout_matches_the_ctypes_mirror(lib):
    assert (lib.h_layout(7), lib.h_layout(8), lib.h_layout(9)) == (C.sizeof(JitterTerm), C.sizeof(JitterSpec), C.sizeof(JitterInfo)) == (48, 216, 72)
    code = code_of_header()
    for name, cls in (("samsim_jitter_term", JitterTerm), ("samsim_jitter_spec", JitterSpec), ("samsim_jitter_info", JitterInfo)):
        body = code[code.index("typedef struct %s {" % name) + len("typedef struct %s {" % name):code.index("} %s;" % name)]
        names = []
        for decl in re.findall(r"\b(?:int32_t|int64_t|uint64_t|double|samsim_jitter_term)\s+([^;]+);", body):
            names += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(",")]
        assert names == [n for n, _ in cls._fields_], name
    assert JitterSpec.term.offset == 24 and JitterTerm.centre.offset == 8 and JitterInfo.n_hi.offset == 40


def test_the_makefile_builds_the_new_source():
    mk = open(os.path.join(ROOT, "samsim_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "samsim_jitter.hip" in srcs and srcs[-1] == "samsim_capi.cpp"
    assert re.search(r"kernel-resource-usage -c -x hip samsim_jitter\.hip", mk)
    kernels = open(os.path.join(ROOT, "samsim_amd", "csrc", "samsim_kernels.hip")).read()
    assert "samsim_jitter" not in kernels                                 # the step kernel does not see the jitter
    # the mixer is reused, not restated
    text = open(os.path.join(ROOT, "samsim_amd", "csrc", "samsim_jitter.h")).read()
    assert "0x9E37" not in text and "rs_offset(" in text and "sp_log(" in text


def test_the_grid_rule_and_the_scratch_layout(lib):
    part, result, nbytes, sz, grid, bound, max_ncol = (lib.h_layout(i) for i in range(7))
    assert grid == jr.GRID == 4096 and bound == capi.JITTER_SCRATCH_BYTES and max_ncol == MAX_NCOL
    assert part == 0 and sz == 72 and result >= part + sz * grid and result % 8 == 0 and result + sz <= nbytes <= bound
    out = (C.c_int64 * 3)()
    for n in (1, 63, 64, 65, 300, 4197, 70001, 4096 * 64, 4096 * 64 + 1, 1 << 20, max_ncol):
        lib.h_grid(n, out)
        assert (out[0], out[1], out[2]) == jr.grid_rule(n), n
        assert (out[2] - 1) * out[1] < out[0] <= out[2] * out[1] and 1 <= out[2] <= grid, n


# --------------------------------------------------------------------------------------------------------- the integer part
def test_mix_and_uniforms_equal_the_numpy_restatement_bit_for_bit(lib):
    n = 100000
    rng = np.random.default_rng(20261021)
    seed = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    col = rng.integers(0, MAX_NCOL, n).astype(np.uint64)
    col[:1000] = MAX_NCOL - 1                                             # the shift by 8 stays inside 64 bits
    col[1000:1100] = 0
    seed[:10] = np.uint64((1 << 64) - 1)
    seed[10:20] = 0
    target = rng.integers(0, 4, n).astype(np.int32)
    attempt = rng.integers(0, 32, n).astype(np.int32)
    attempt[:500] = 31
    k, x, y = np.zeros(n, dtype=np.uint64), np.zeros(n), np.zeros(n)
    lib.h_uniforms(n, seed.ctypes.data, col.ctypes.data, target.ctypes.data, attempt.ctypes.data, k.ctypes.data, x.ctypes.data, y.ctypes.data)
    want_k = jr.key(col, target, attempt)
    assert np.array_equal(k, want_k) and int(k.max()) < 1 << 32 and int(k.max()) >> 8 == MAX_NCOL - 1
    assert np.array_equal(k >> np.uint64(8), col) and np.array_equal((k >> np.uint64(6)) & np.uint64(3), target.astype(np.uint64))
    assert np.array_equal((k >> np.uint64(1)) & np.uint64(31), attempt.astype(np.uint64)) and not (k & np.uint64(1)).any()
    m = np.zeros(n, dtype=np.uint64)
    lib.h_mix(n, seed.ctypes.data, k.ctypes.data, m.ctypes.data)
    assert np.array_equal(m, jr.mix(seed, k))
    assert [capi.mix64(int(seed[i]), int(k[i])) for i in range(0, n, 997)] == [int(v) for v in m[::997]]
    assert x.view(np.uint64).tobytes() == jr.uniform(seed, k).view(np.uint64).tobytes()
    assert y.view(np.uint64).tobytes() == jr.uniform(seed, k | np.uint64(1)).view(np.uint64).tobytes()
    assert (x >= -1.0).all() and (x < 1.0).all() and (x * 2.0 ** 52 == np.rint(x * 2.0 ** 52)).all()
    assert capi.rs_offset(int(seed[77]), int(k[77])) == (x[77] + 1.0) / 2.0


# --------------------------------------------------------------------------------------------------------------- the deviate
N_STAT = 1 << 20
SEED = 0x5A17C0DE


@pytest.fixture(scope="module")
def deviates(lib):
    cols = np.arange(N_STAT, dtype=np.int64)
    return [jr.deviate(SEED, cols, t) for t in range(4)]


def test_the_compiled_deviate_is_the_numpy_rule_within_4_ulp(deviates):
    cols = np.arange(1 << 18, dtype=np.int64)
    worst = 0.0
    for t in range(4):
        eps, att = deviates[t][0][:cols.size], deviates[t][1][:cols.size]
        want, want_att = jr.deviate_numpy(SEED, cols, t)
        assert np.array_equal(att, want_att)
        ulp = np.abs(eps - want) / np.spacing(np.abs(want))
        worst = max(worst, float(ulp.max()))
    print("deviate against the rule with np.log: worst", worst, "ulp")
    assert worst <= 4.0
    # columns at the end of the range, another seed
    cols = np.arange(MAX_NCOL - 5000, MAX_NCOL, dtype=np.int64)
    eps, att = jr.deviate((1 << 64) - 3, cols, 3)
    want, want_att = jr.deviate_numpy((1 << 64) - 3, cols, 3)
    assert np.array_equal(att, want_att) and (np.abs(eps - want) <= 4.0 * np.spacing(np.abs(want))).all()


def test_the_deviates_are_standard_normal_and_uncorrelated(deviates):
    """z-scores at 5: the bounds follow from N (the mean of N unit normals has deviation 1/sqrt(N), their variance sqrt(2/N), the
    sample correlation of independent ones 1/sqrt(N)); they are not measurements"""
    n = float(N_STAT)
    e = [d[0] for d in deviates]
    for t in range(4):
        mean, var = float(e[t].mean()), float(e[t].var())
        print("target", t, "mean", mean, "var", var, "max attempts", int(deviates[t][1].max()), "mean attempts", float(deviates[t][1].mean()))
        assert abs(mean) < 5.0 / np.sqrt(n) and abs(var - 1.0) < 5.0 * np.sqrt(2.0 / n)
        r = float(np.corrcoef(e[t][:-1], e[t][1:])[0, 1])                 # neighbouring columns
        assert abs(r) < 5.0 / np.sqrt(n), (t, r)
        assert deviates[t][1].max() <= 20 and deviates[t][1].min() >= 1   # no column needs more than 20 attempts
        assert 1.2 < deviates[t][1].mean() < 1.35                         # 4 / pi = 1.273
    for a in range(4):
        for b in range(a + 1, 4):
            r = float(np.corrcoef(e[a], e[b])[0, 1])
            assert abs(r) < 5.0 / np.sqrt(n), (a, b, r)
    # the key is the seed as well: another seed, another stream
    other = jr.deviate(SEED + 1, np.arange(4096), 0)[0]
    assert not (other == e[0][:4096]).any()


# ------------------------------------------------------------------------------------------------------------ the value rule
def both(term, theta, eps):
    v1, lo1, hi1 = jr.value_compiled(term, theta, eps)
    v2, lo2, hi2 = jr.value(term, theta, eps)
    assert v1.view(np.uint64).tobytes() == np.asarray(v2, dtype=np.float64).view(np.uint64).tobytes()
    assert np.array_equal(lo1, lo2) and np.array_equal(hi1, hi2)
    return v1, lo1, hi1


def test_the_value_rule_on_hand_made_cases(lib, deviates):
    eps = deviates[0][0][:1000]
    theta = np.linspace(-3.0, 7.0, 1000)
    # sigma = 0 and shrink = 0: the centre exactly
    v, lo, hi = both(JitterTerm.make("dT2m", 1.0 / 3.0, 0.0, 0.0), theta, eps)
    assert (v == 1.0 / 3.0).all() and not lo.any() and not hi.any()
    # theta = 0, centre = 0, sigma = 1, infinite bounds: the deviate exactly
    v, lo, hi = both(JitterTerm.make("precip_scale", 0.0, 0.37, 1.0), np.zeros(1000), eps)
    assert v.view(np.uint64).tobytes() == eps.view(np.uint64).tobytes() and not lo.any() and not hi.any()
    # shrink = 1 and sigma = 0 around centre 0: the value itself
    v, _, _ = both(JitterTerm.make("dT2m", 0.0, 1.0, 0.0), theta, eps)
    assert (v == theta).all()
    # every operation is rounded on its own
    t = JitterTerm.make("dfl_q_bottom", 0.1, 0.7, 0.3)
    v, _, _ = both(t, theta, eps)
    want = [(0.1 + 0.7 * (float(th) - 0.1)) + 0.3 * float(e) for th, e in zip(theta, eps)]
    assert v.tolist() == want
    # both clamps with their counts; a value on a bound is not counted
    t = JitterTerm.make("S_bu_bottom", 0.0, 1.0, 0.0, 1.0, 5.0)
    v, lo, hi = both(t, np.array([-2.0, 1.0, 3.0, 5.0, 5.5, 0.999]), np.zeros(6))
    assert v.tolist() == [1.0, 1.0, 3.0, 5.0, 5.0, 1.0] and lo.tolist() == [True, False, False, False, False, True]
    assert hi.tolist() == [False, False, False, False, True, False]
    t = JitterTerm.make("dT2m", 0.0, 1.0, 2.0, -1.0, 1.0)
    v, lo, hi = both(t, np.zeros(1000), eps)
    assert (v >= -1.0).all() and (v <= 1.0).all() and lo.sum() == (2.0 * eps < -1.0).sum() > 100 and hi.sum() == (2.0 * eps > 1.0).sum() > 100
    # NaN stays NaN and counts nowhere; an infinite value is clamped
    v, lo, hi = both(JitterTerm.make("dT2m", 0.0, 1.0, 1.0, -1.0, 1.0), np.array([np.nan, 0.0, INF, -INF]), np.array([0.0, np.nan, 0.0, 0.0]))
    assert np.isnan(v[:2]).all() and v[2:].tolist() == [1.0, -1.0] and lo.tolist() == [False, False, False, True] and hi.tolist() == [False, False, True, False]


def test_which_columns_are_written():
    status = np.array([0, 0, 7, 0, 0, 3], dtype=np.int32)
    lab = np.array([1, 2, 1, -1, 1, 1], dtype=np.int32)
    assert jr.written("pool", 6, status).tolist() == [True, True, False, True, True, False]
    assert jr.written("pool", 6, status, lab, 1).tolist() == [True, False, False, False, True, False]
    assert jr.written("copies", 6, status, lab, None, [1, 2, 4]).tolist() == [False, True, False, False, True, False]
    rows = {0: np.arange(6.0)}
    new, info = jr.apply([JitterTerm.make(0, 0.0, 1.0, 1.0)], rows, 5, "pool", status, lab, 1)
    eps = jr.deviate(5, [0, 4], 0)[0]
    assert info == {"n_written": 2, "n_lo": [0], "n_hi": [0]} and new[0].tolist() == [0.0 + eps[0], 1.0, 2.0, 3.0, 4.0 + eps[1], 5.0]


def test_liu_west():
    a, h = capi.liu_west(0.98)
    assert a == (3 * 0.98 - 1) / (2 * 0.98) and h == np.sqrt(1.0 - a * a) and abs(a * a + h * h - 1.0) < 1e-15
    assert capi.liu_west(1.0) == (1.0, 0.0)
    with pytest.raises(ValueError):
        capi.liu_west(0.2)


# ------------------------------------------------------------------------------------------------------- the checks of a spec
def check(lib, spec, have_q=True, have_s=True, group_ok=True, plan_n=5):
    return lib.h_check(C.byref(spec), int(have_q), int(have_s), int(group_ok), plan_n)


def good_terms():
    return [JitterTerm.make("dT2m", 0.1, 0.9, 0.2, -3.0, 3.0), JitterTerm.make("precip_scale", 1.0, 0.99, 0.05, 0.0, INF),
            JitterTerm.make("dfl_q_bottom", 0.0, 1.0, 0.0), JitterTerm.make("S_bu_bottom", 34.0, 0.5, 1.0, 0.0, 40.0)]


def test_the_spec_checks_in_the_documented_order(lib):
    ARG, ABI = -1, -6
    assert check(lib, JitterSpec.make(good_terms())) == 0
    assert check(lib, JitterSpec.make(good_terms()[:1], "copies")) == 0
    assert lib.h_check(None, 1, 1, 1, 5) == ARG
    # the struct size comes before everything a spec holds
    bad = JitterSpec.make(good_terms(), 7)
    bad.struct_size -= 8
    bad.nterms = 9
    assert check(lib, bad) == ABI
    bad.struct_size += 8
    assert check(lib, bad) == ARG
    for which in (-1, 2):
        assert check(lib, JitterSpec.make(good_terms(), which)) == ARG
    for n in (0, -1, 5):
        s = JitterSpec.make(good_terms())
        s.nterms = n
        assert check(lib, s) == ARG, n
    # per term: each fault alone, in each position
    def with_term(i, **kw):
        terms = good_terms()
        for k, v in kw.items():
            setattr(terms[i], k, v)
        return JitterSpec.make(terms)
    nan = float("nan")
    faults = [dict(target=4), dict(target=-1), dict(reserved=1), dict(centre=nan), dict(centre=INF), dict(shrink=nan), dict(sigma=INF),
              dict(shrink=-0.01), dict(shrink=1.01), dict(sigma=-1e-300), dict(lo=nan), dict(hi=nan), dict(lo=2.0, hi=1.0)]
    for i in range(4):
        for f in faults:
            assert check(lib, with_term(i, **f)) == ARG, (i, f)
    assert check(lib, with_term(1, target=JT["dT2m"])) == ARG            # a target listed twice
    assert check(lib, with_term(3, lo=-0.5)) == ARG                      # a negative salinity below
    assert check(lib, with_term(2, lo=-0.5)) == 0                        # the flux offset may be negative
    assert check(lib, with_term(0, lo=-INF, hi=INF)) == 0 and check(lib, with_term(0, lo=1.0, hi=1.0)) == 0
    assert check(lib, with_term(0, shrink=0.0, sigma=0.0)) == 0
    # terms beyond nterms are not looked at
    s = with_term(3, target=99)
    s.nterms = 3
    assert check(lib, s) == 0
    # then the rows, the group, the plan
    assert check(lib, JitterSpec.make(good_terms()), have_q=False) == ARG and check(lib, JitterSpec.make(good_terms()), have_s=False) == ARG
    assert check(lib, JitterSpec.make(good_terms()[:2]), have_q=False, have_s=False) == 0
    assert check(lib, JitterSpec.make(good_terms(), group=3), group_ok=False) == ARG
    assert check(lib, JitterSpec.make(good_terms(), group=3), group_ok=True) == 0
    assert check(lib, JitterSpec.make(good_terms(), "copies", group=3)) == ARG      # the plan carries the group of its draw
    assert check(lib, JitterSpec.make(good_terms(), "copies"), plan_n=-1) == ARG    # no plan applied yet
    assert check(lib, JitterSpec.make(good_terms(), "copies"), plan_n=0) == 0
    assert check(lib, JitterSpec.make(good_terms(), "copies"), group_ok=False) == 0  # -1 needs no labels: the caller's answer is not asked
