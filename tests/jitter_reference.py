"""TEST INFRASTRUCTURE: what samsim_jitter (include/samsim.h) must equal.

helper() compiles samsim_amd/csrc/samsim_jitter.h -- the functions the kernel calls -- alone with g++ and exposes the mixer, the
uniforms, the deviate, the value rule and the checks of a spec through ctypes.  Beside it the rule in numpy: the integer part (mix,
key, uniforms), the deviate with np.log in the place of the library's logarithm, the value rule, and which columns a call writes.
apply() is the reference of the GPU tests: the compiled deviate and the numpy value rule on downloaded rows, status and labels."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from samsim_amd.capi import JITTER_MAX_ATTEMPTS, JITTER_MAX_TERMS, JitterSpec, JitterTerm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "samsim_amd", "csrc")
GRID = 4096                                   # ranges at most (DEV_JT_GRID)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)

HELPER_CPP = r'''#include "samsim_jitter.h"
extern "C" {
void h_mix(long n, const unsigned long long *seed, const unsigned long long *k, unsigned long long *out) {
  for (long i = 0; i < n; ++i) out[i] = rs_mix(seed[i], k[i]);
}
// the point (x, y) of attempt a of (seed, column, target), and its key
void h_uniforms(long n, const unsigned long long *seed, const unsigned long long *col, const int *target, const int *attempt,
                unsigned long long *key, double *x, double *y) {
  for (long i = 0; i < n; ++i) {
    key[i] = jt_key(col[i], target[i], attempt[i]);
    x[i] = jt_uniform(seed[i], key[i]);
    y[i] = jt_uniform(seed[i], key[i] | 1);
  }
}
void h_deviate(long n, unsigned long long seed, const long long *col, int target, double *eps, int *attempts) {
  for (long i = 0; i < n; ++i) eps[i] = jt_deviate(seed, (unsigned long long)col[i], target, &attempts[i]);
}
void h_value(const samsim_jitter_term *t, long n, const double *theta, const double *eps, double *v, unsigned char *lo, unsigned char *hi) {
  for (long i = 0; i < n; ++i) {
    const JtValue r = jt_value(*t, theta[i], eps[i]);
    v[i] = r.v; lo[i] = r.lo; hi[i] = r.hi;
  }
}
int h_check(const samsim_jitter_spec *spec, int have_dfl_q, int have_S_bu, int group_ok, long long plan_n) {
  return jt_check(spec, have_dfl_q != 0, have_S_bu != 0, group_ok != 0, plan_n);
}
void h_grid(long long n, long long *out) { const JtGrid g = jt_grid(n); out[0] = g.nblk; out[1] = g.per; out[2] = g.ranges; }
long long h_layout(int i) {
  const long long at[] = {(long long)DEV_JT_PART_AT, (long long)DEV_JT_RESULT_AT, (long long)DEV_JT_BYTES, (long long)sizeof(JtCounts),
                          (long long)DEV_JT_GRID, (long long)SAMSIM_JITTER_SCRATCH_BYTES, (long long)SAMSIM_MAX_NCOL,
                          (long long)sizeof(samsim_jitter_term), (long long)sizeof(samsim_jitter_spec), (long long)sizeof(samsim_jitter_info),
                          (long long)SAMSIM_JITTER_MAX_TERMS, (long long)SAMSIM_JITTER_MAX_ATTEMPTS, (long long)SAMSIM_OCEAN_SLOT(1)};
  return at[i];
}
}
'''


@functools.lru_cache(maxsize=None)
def helper():
    """samsim_jitter.h as a small shared library, or None where there is no g++"""
    if shutil.which("g++") is None:
        return None
    d = tempfile.mkdtemp(prefix="samsim_jitter_")
    src, so = os.path.join(d, "helper.cpp"), os.path.join(d, "libhelper.so")
    with open(src, "w") as f:
        f.write(HELPER_CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, src, "-o", so])
    lib = C.CDLL(so)
    i64, u64, vp = C.c_int64, C.c_uint64, C.c_void_p
    lib.h_mix.argtypes, lib.h_mix.restype = [C.c_long, vp, vp, vp], None
    lib.h_uniforms.argtypes, lib.h_uniforms.restype = [C.c_long, vp, vp, vp, vp, vp, vp, vp], None
    lib.h_deviate.argtypes, lib.h_deviate.restype = [C.c_long, u64, vp, C.c_int, vp, vp], None
    lib.h_value.argtypes, lib.h_value.restype = [C.POINTER(JitterTerm), C.c_long, vp, vp, vp, vp, vp], None
    lib.h_check.argtypes, lib.h_check.restype = [C.POINTER(JitterSpec), C.c_int, C.c_int, C.c_int, i64], C.c_int
    lib.h_grid.argtypes, lib.h_grid.restype = [i64, vp], None
    lib.h_layout.argtypes, lib.h_layout.restype = [C.c_int], i64
    return lib


# ------------------------------------------------------------------------------------------------- the compiled functions
def deviate(seed, cols, target):
    """(eps float64, attempts int32) of the columns `cols` for (seed, target): jt_deviate of the header, compiled for the host"""
    cols = np.ascontiguousarray(cols, dtype=np.int64)
    eps, att = np.zeros(cols.size), np.zeros(cols.size, dtype=np.int32)
    helper().h_deviate(cols.size, int(seed) & (2 ** 64 - 1), cols.ctypes.data, int(target), eps.ctypes.data, att.ctypes.data)
    return eps, att


def value_compiled(term, theta, eps):
    """(v, lo, hi) of jt_value of the header for a JitterTerm"""
    theta, eps = np.ascontiguousarray(theta, dtype=np.float64), np.ascontiguousarray(eps, dtype=np.float64)
    v, lo, hi = np.zeros(theta.size), np.zeros(theta.size, dtype=np.uint8), np.zeros(theta.size, dtype=np.uint8)
    helper().h_value(C.byref(term), theta.size, theta.ctypes.data, eps.ctypes.data, v.ctypes.data, lo.ctypes.data, hi.ctypes.data)
    return v, lo.astype(bool), hi.astype(bool)


# ------------------------------------------------------------------------------------------------------ the rule in numpy
def mix(seed, k):
    """the splitmix64 finaliser of seed + (k + 1) * 0x9E3779B97F4A7C15, uint64 arrays in wrapping arithmetic"""
    seed, k = np.asarray(seed, dtype=np.uint64), np.asarray(k, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = seed + (k + np.uint64(1)) * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def key(col, target, attempt):
    col, target, attempt = (np.asarray(a, dtype=np.uint64) for a in (col, target, attempt))
    return (col << np.uint64(8)) | (target << np.uint64(6)) | (attempt << np.uint64(1))


def uniform(seed, k):
    """2 * ((mix >> 11) * 2^-53) - 1: exact"""
    return 2.0 * ((mix(seed, k) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0


def deviate_numpy(seed, cols, target):
    """(eps, attempts): the rule with np.log in the place of the library's logarithm"""
    cols = np.asarray(cols, dtype=np.uint64)
    eps, att = np.zeros(cols.size), np.full(cols.size, JITTER_MAX_ATTEMPTS, dtype=np.int32)
    open_ = np.ones(cols.size, dtype=bool)
    for a in range(JITTER_MAX_ATTEMPTS):
        idx = np.flatnonzero(open_)
        if not idx.size:
            break
        k = key(cols[idx], target, a)
        x, y = uniform(seed, k), uniform(seed, k | np.uint64(1))
        s = x * x + y * y
        ok = (s > 0.0) & (s < 1.0)
        at = idx[ok]
        eps[at] = x[ok] * np.sqrt((-2.0 * np.log(s[ok])) / s[ok])
        att[at] = a + 1
        open_[at] = False
    return eps, att


def value(term, theta, eps):
    """(v, lo, hi): centre + shrink * (theta - centre), + sigma * eps, the two bounds; every operation rounded on its own"""
    theta, eps = np.asarray(theta, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = theta - term.centre
        p = term.shrink * d
        v = term.centre + p
        e = term.sigma * eps
        v = v + e
        lo = v < term.lo
        hi = ~lo & (v > term.hi)
    return np.where(lo, term.lo, np.where(hi, term.hi, v)), lo, hi


def written(which, ncol, status, labels=None, group=None, plan_dst=None):
    """bool [ncol]: the columns a call writes.  "pool": status 0 and the label passes the group; "copies": the destinations of the
    stored plan whose status is 0 now"""
    run = np.asarray(status) == 0
    if which in ("copies", 1):
        w = np.zeros(ncol, dtype=bool)
        w[np.asarray(plan_dst, dtype=np.int64)] = True
        return w & run
    if group is not None and group >= 0:
        run = run & (np.asarray(labels) == group)
    return run


def apply(terms, rows, seed, which, status, labels=None, group=None, plan_dst=None):
    """(new rows {target: float64 [ncol]}, info) of jitter(terms, which, seed, group) on the rows {target: float64 [ncol]}: the compiled
    deviate of the header and the numpy value rule"""
    ncol = np.asarray(status).size
    w = written(which, ncol, status, labels, group, plan_dst)
    cols = np.flatnonzero(w)
    out, n_lo, n_hi = {}, [], []
    for t in terms:
        eps, _ = deviate(seed, cols, t.target)
        v, lo, hi = value(t, np.asarray(rows[t.target])[cols], eps)
        new = np.array(rows[t.target], dtype=np.float64)
        new[cols] = v
        out[t.target] = new
        n_lo.append(int(lo.sum()))
        n_hi.append(int(hi.sum()))
    return out, {"n_written": int(cols.size), "n_lo": n_lo, "n_hi": n_hi}


def grid_rule(n):
    """(nblk, per, ranges) of the n entries a call walks"""
    nblk = (n + 63) // 64
    per = (nblk + GRID - 1) // GRID
    return nblk, per, ((nblk + per - 1) // per if per else 0)


assert JITTER_MAX_TERMS == 4
