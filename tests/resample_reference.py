"""TEST INFRASTRUCTURE: numpy restatement of samsim_resample (include/samsim.h), operation by operation.

The cumulative weight is np.cumsum per range (np.cumsum adds sequentially) on top of the ranges' bases, themselves a sequential sum;
the mixer of the stratified offsets is uint64 arithmetic; the point counts K(t) are math.ceil / math.floor (count_systematic,
count_stratified) and, for whole rows, the same operations through np.ceil / np.floor (counts).  helper() compiles the plain C++ part
of samsim_amd/csrc/samsim_resample.h -- the functions the kernels call -- for the host with g++."""
import ctypes as C
import functools
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "samsim_amd", "csrc")
GRID = 1024                                   # ranges at most (DEV_RS_GRID)
M64 = (1 << 64) - 1
SYSTEMATIC, STRATIFIED = 0, 1
KINDS = {"systematic": SYSTEMATIC, "stratified": STRATIFIED}

HELPER_CPP = r'''#include "samsim_resample.h"
extern "C" {
unsigned long long h_mix(unsigned long long seed, unsigned long long k) { return rs_mix(seed, k); }
double h_offset(unsigned long long seed, unsigned long long k) { return rs_offset(seed, k); }
long long h_count_systematic(double t, long long m, double u0) { return rs_count_systematic(t, m, u0); }
long long h_count_stratified(double t, long long m, unsigned long long seed) { return rs_count_stratified(t, m, seed); }
void h_counts(int kind, long n, const double *t, const long long *m, const double *u0, const unsigned long long *seed, long long *out) {
  for (long i = 0; i < n; ++i) out[i] = kind == 0 ? rs_count_systematic(t[i], m[i], u0[i]) : rs_count_stratified(t[i], m[i], seed[i]);
}
void h_mixes(long n, const unsigned long long *seed, const unsigned long long *k, unsigned long long *out) {
  for (long i = 0; i < n; ++i) out[i] = rs_mix(seed[i], k[i]);
}
void h_grid(long long ncol, long long *out) { const RsGrid g = rs_grid(ncol); out[0] = g.nblk; out[1] = g.per; out[2] = g.ranges; }
long long h_scratch_bytes(void) { return (long long)rs_scratch_bytes(); }
long long h_layout(int i) {
  const long long at[] = {(long long)DEV_RS_SUMS_AT, (long long)DEV_RS_BASES_AT, (long long)DEV_RS_TOTAL_AT, (long long)DEV_RS_PART_AT,
                          (long long)DEV_RS_RESULT_AT, (long long)DEV_RS_BYTES, (long long)sizeof(RsPartial), (long long)sizeof(RsResult),
                          (long long)DEV_RS_GRID, (long long)SAMSIM_RESAMPLE_SCRATCH_BYTES, (long long)SAMSIM_MAX_NCOL};
  return at[i];
}
}
'''


@functools.lru_cache(maxsize=None)
def helper():
    """the plain C++ part of samsim_resample.h as a small shared library, or None where there is no g++.  -ffp-contract=off as the
    library is built"""
    if shutil.which("g++") is None:
        return None
    d = tempfile.mkdtemp(prefix="samsim_resample_")
    src, so = os.path.join(d, "helper.cpp"), os.path.join(d, "libhelper.so")
    with open(src, "w") as f:
        f.write(HELPER_CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, src, "-o", so])
    lib = C.CDLL(so)
    u64, i64, dbl, vp = C.c_uint64, C.c_int64, C.c_double, C.c_void_p
    lib.h_mix.argtypes, lib.h_mix.restype = [u64, u64], u64
    lib.h_offset.argtypes, lib.h_offset.restype = [u64, u64], dbl
    lib.h_count_systematic.argtypes, lib.h_count_systematic.restype = [dbl, i64, dbl], i64
    lib.h_count_stratified.argtypes, lib.h_count_stratified.restype = [dbl, i64, u64], i64
    lib.h_counts.argtypes, lib.h_counts.restype = [C.c_int, C.c_long, vp, vp, vp, vp, vp], None
    lib.h_mixes.argtypes, lib.h_mixes.restype = [C.c_long, vp, vp, vp], None
    lib.h_grid.argtypes, lib.h_grid.restype = [i64, vp], None
    lib.h_scratch_bytes.argtypes, lib.h_scratch_bytes.restype = [], i64
    lib.h_layout.argtypes, lib.h_layout.restype = [C.c_int], i64
    return lib


def grid_rule(ncol):
    """(nblk, per, ranges): the 64-column blocks, the blocks per range and the ranges -- the grid rule of samsim_select_columns"""
    nblk = (ncol + 63) // 64
    per = (nblk + GRID - 1) // GRID
    return nblk, per, (nblk + per - 1) // per


def mix(seed, k):
    """the splitmix64 finaliser of seed + (k + 1) * 0x9E3779B97F4A7C15 in wrapping 64-bit arithmetic; uint64 arrays or ints"""
    with np.errstate(over="ignore"):
        z = np.asarray(seed, dtype=np.uint64) + (np.asarray(k, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def mix_int(seed, k):
    """mix in Python integers"""
    z = (seed + (k + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def offset(seed, k):
    """u(k) = (mix(seed, k) >> 11) * 2^-53, in [0, 1)"""
    return (mix(seed, k) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def count_systematic(t, m, u0):
    """K(t) of SAMSIM_RESAMPLE_SYSTEMATIC for one t: m from t >= m on, else min(max(ceil(t - u0), 0), m), the difference rounded"""
    if t >= m:
        return m
    return min(max(math.ceil(t - u0), 0), m)


def count_stratified(t, m, seed):
    """K(t) of SAMSIM_RESAMPLE_STRATIFIED for one t: m from t >= m on, else f + (u(f) < t - f), f = floor(t)"""
    if t >= m:
        return m
    f = math.floor(t)
    u = float(mix_int(seed, f) >> 11) * 2.0 ** -53
    return f + (1 if u < t - f else 0)


def counts(t, m, kind, u0=0.0, seed=0):
    """K(t) of a whole row t (float64, within [0, m]): int64"""
    t = np.asarray(t, dtype=np.float64)
    full = t >= m
    tt = np.where(full, 0.0, t)
    if kind == SYSTEMATIC:
        k = np.clip(np.ceil(tt - np.float64(u0)), 0.0, float(m)).astype(np.int64)
    else:
        f = np.floor(tt)
        k = f.astype(np.int64) + (offset(seed, f.astype(np.uint64)) < tt - f)
    return np.where(full, np.int64(m), k).astype(np.int64)


def terms_of(w, status, labels=None, group=None):
    """the columns' terms: w where the column counts (status 0, the label of the group, w > 0), else +0.0"""
    w = np.asarray(w, dtype=np.float64)
    ok = np.asarray(status) == 0
    if group is not None and group >= 0:
        ok = ok & (np.asarray(labels) == group)
    with np.errstate(invalid="ignore"):
        ok = ok & (w > 0.0)
    return np.where(ok, w, 0.0), ok


def cumulative(terms):
    """(C, W): the inclusive prefix sum of the terms in the header's bracketing -- sequential inside a range from 0.0, the ranges'
    bases B_{g+1} = B_g + T_g sequential from 0.0, C_c = B_g + L_c -- and W = B_G"""
    n = terms.size
    _, per, ranges = grid_rule(n)
    span = per * 64
    C_ = np.empty(n)
    B = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for g in range(ranges):
            L = np.cumsum(terms[g * span:(g + 1) * span])
            C_[g * span:g * span + L.size] = np.float64(B) + L
            B = float(np.float64(B) + L[-1])
    return C_, B


def resample(w, status, labels, group, m, kind="systematic", u0=0.0, seed=0):
    """dict(offspring float64 [ncol], ancestors int64 [m_drawn], info dict, C, W) of samsim_resample for the weight row w"""
    kind = KINDS[kind] if isinstance(kind, str) else kind
    terms, ok = terms_of(w, status, labels, group)
    C_, W = cumulative(terms)
    n = terms.size
    if W > 0.0 and math.isfinite(W):
        t = (C_ / np.float64(W)) * np.float64(m)
        K = counts(t, m, kind, u0, seed)
        N = np.diff(K, prepend=np.int64(0))
    else:
        N = np.zeros(n, dtype=np.int64)
    info = dict(n_pos=int(ok.sum()), m_drawn=int(N.sum()), n_survivors=int((N >= 1).sum()), max_offspring=int(N.max()),
                argmax_offspring=int(np.argmax(N)), sum_w=float(W))
    return dict(offspring=N.astype(np.float64), ancestors=np.repeat(np.arange(n, dtype=np.int64), np.maximum(N, 0)), info=info, C=C_, W=W)
