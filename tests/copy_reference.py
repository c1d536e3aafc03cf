"""TEST INFRASTRUCTURE: what samsim_copy_columns and samsim_apply_resample (include/samsim.h) must equal.

plan() is the header's rule for the pair list in numpy.  host_route() is the route through the host the copy is defined by, as a
function of a Solver: get_columns of the sources, set_state at each destination, set_status with the sources' status, the tracer
amounts, and -- where asked for -- the track and score rows.  (The perturbation slots SAMSIM_COPY_FORCING adds have no setter for a
window of columns; tests/test_gpu_copy_columns.py checks them against the source's own continuation.)  helper() compiles the plain
C++ part of samsim_amd/csrc/samsim_copy.h -- the functions the kernels call -- for the host with g++ and walks it range by range."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from samsim_amd.capi import NARR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "samsim_amd", "csrc")
GRID = 1024                                   # ranges at most (DEV_CP_GRID)

HELPER_CPP = r'''#include "samsim_copy.h"
extern "C" {
void h_grid(long long ncol, long long *out) { const CpGrid g = cp_grid(ncol); out[0] = g.nblk; out[1] = g.per; out[2] = g.ranges; }
// the rule of one column: surplus, free, source, bad
void h_columns(long n, const unsigned char *pool, const double *offspring, long long *surplus, unsigned char *free_, unsigned char *source,
               unsigned char *bad) {
  for (long i = 0; i < n; ++i) {
    const CpColumn c = cp_column(pool[i] != 0, offspring[i]);
    surplus[i] = c.surplus; free_[i] = c.free; source[i] = c.source; bad[i] = c.bad;
  }
}
// the plan as the three kernels form it, range by range: the counts, the scan, the write.  Returns 1 when the plan balances; the
// lists are written only then.  out = n_pool, n_free, n_copies, n_sources, n_bad
int h_plan(long long ncol, const unsigned char *pool, const double *offspring, long long *src, long long *dst, long long *out) {
  const CpGrid g = cp_grid(ncol);
  CpPartial part[DEV_CP_GRID];
  long long at_free[DEV_CP_GRID], at_copies[DEV_CP_GRID];
  CpResult r = {0, 0, 0, 0, 0};
  for (int w = 0; w < g.ranges; ++w) {
    CpPartial q = {0, 0, 0, 0, 0};
    const long long c0 = (long long)w * g.per * 64, c1 = c0 + g.per * 64 < ncol ? c0 + g.per * 64 : ncol;
    for (long long c = c0; c < c1; ++c) {
      const CpColumn k = cp_column(pool[c] != 0, offspring[c]);
      q.n_pool += pool[c] != 0; q.n_free += k.free; q.n_copies += k.surplus; q.n_sources += k.source; q.n_bad += k.bad;
    }
    part[w] = q;
    at_free[w] = r.n_free; at_copies[w] = r.n_copies;
    r.n_pool += q.n_pool; r.n_free += q.n_free; r.n_copies += q.n_copies; r.n_sources += q.n_sources; r.n_bad += q.n_bad;
  }
  out[0] = r.n_pool; out[1] = r.n_free; out[2] = r.n_copies; out[3] = r.n_sources; out[4] = r.n_bad;
  if (!cp_balanced(r)) return 0;
  for (int w = 0; w < g.ranges; ++w) {
    long long f = at_free[w], k = at_copies[w];
    const long long c0 = (long long)w * g.per * 64, c1 = c0 + g.per * 64 < ncol ? c0 + g.per * 64 : ncol;
    for (long long c = c0; c < c1; ++c) {
      const CpColumn q = cp_column(pool[c] != 0, offspring[c]);
      if (q.free) dst[f++] = c;
      for (long long j = 0; j < q.surplus; ++j) src[k++] = c;
    }
  }
  return 1;
}
long long h_scratch_bytes(void) { return (long long)cp_scratch_bytes(); }
long long h_piece_entries(long long nlayer) { return (long long)cp_piece_entries((size_t)nlayer); }
long long h_layout(int i) {
  const long long at[] = {(long long)DEV_CP_PART_AT, (long long)DEV_CP_FREE_AT, (long long)DEV_CP_COPIES_AT, (long long)DEV_CP_RESULT_AT,
                          (long long)DEV_CP_BYTES, (long long)sizeof(CpPartial), (long long)sizeof(CpResult), (long long)DEV_CP_GRID,
                          (long long)SAMSIM_COPY_SCRATCH_BYTES, (long long)SAMSIM_MAX_NCOL, (long long)sizeof(samsim_apply_info),
                          (long long)DEV_CP_PIECE_THREADS, (long long)SAMSIM_MAX_NLAYER};
  return at[i];
}
}
'''


@functools.lru_cache(maxsize=None)
def helper():
    """the plain C++ part of samsim_copy.h as a small shared library, or None where there is no g++"""
    if shutil.which("g++") is None:
        return None
    d = tempfile.mkdtemp(prefix="samsim_copy_")
    src, so = os.path.join(d, "helper.cpp"), os.path.join(d, "libhelper.so")
    with open(src, "w") as f:
        f.write(HELPER_CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, src, "-o", so])
    lib = C.CDLL(so)
    i64, vp = C.c_int64, C.c_void_p
    lib.h_grid.argtypes, lib.h_grid.restype = [i64, vp], None
    lib.h_columns.argtypes, lib.h_columns.restype = [C.c_long, vp, vp, vp, vp, vp, vp], None
    lib.h_plan.argtypes, lib.h_plan.restype = [i64, vp, vp, vp, vp, vp], C.c_int
    lib.h_scratch_bytes.argtypes, lib.h_scratch_bytes.restype = [], i64
    lib.h_piece_entries.argtypes, lib.h_piece_entries.restype = [i64], i64
    lib.h_layout.argtypes, lib.h_layout.restype = [C.c_int], i64
    return lib


def grid_rule(ncol):
    """(nblk, per, ranges): the grid rule of samsim_select_columns"""
    nblk = (ncol + 63) // 64
    per = (nblk + GRID - 1) // GRID
    return nblk, per, (nblk + per - 1) // per


def pool_of(status, labels=None, group=None):
    """the columns with status 0 whose label passes the group"""
    pool = np.asarray(status) == 0
    if group is not None and group >= 0:
        pool = pool & (np.asarray(labels) == group)
    return pool


def plan(offspring, status, labels=None, group=None):
    """dict(src, dst, info, n_bad, balanced) of samsim_apply_resample for the offspring row of a draw over `group`: the header's rule"""
    N = np.asarray(offspring).astype(np.int64)
    ncol = N.size
    pool = pool_of(status, labels, group)
    dst = np.nonzero(pool & (N == 0))[0].astype(np.int64)
    src = np.repeat(np.arange(ncol, dtype=np.int64), np.where(pool, np.maximum(N - 1, 0), 0).astype(np.int64))
    n_bad = int((~pool & (N >= 1)).sum())
    info = dict(n_pool=int(pool.sum()), n_free=int(dst.size), n_copies=int(src.size), n_sources=int((pool & (N >= 2)).sum()))
    return dict(src=src, dst=dst, info=info, n_bad=n_bad, balanced=dst.size == src.size and n_bad == 0)


def host_route(g, src, dst, tracks=False, scores=False):
    """the route through the host that defines copy_columns(src, dst, tracks=tracks, scores=scores) without forcing, on the Solver g"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    st, (status, step, layer) = g.get_columns(src, NARR, with_status=True)
    # (the row getters once for the whole handle, then the sources' columns of what they returned: a window of one column is a 2D copy
    # of as many pieces as it has rows)
    bgc = trk = sco = None
    if getattr(g, "n_bgc", 0):
        whole = g.get_tracer_state()[0]
        bgc = [np.ascontiguousarray(whole[..., c:c + 1]) for c in src]
    if tracks:
        whole = [g.tracks(t) for t in range(g.ntracks)]
        trk = [[{f: r[c:c + 1].copy() for f, r in whole[t].items()} for t in range(g.ntracks)] for c in src]
    if scores:
        whole = g.scores()
        sco = [{f: r[c:c + 1].copy() for f, r in whole.items()} for c in src]
    for j, d in enumerate(dst):
        d = int(d)
        g.set_state(st.window(j, 1), d)
        g.set_status(status[j:j + 1], step[j:j + 1], layer[j:j + 1], col0=d)
        if bgc is not None:
            g.set_tracer_state(bgc[j], d)
        if tracks:
            for t in range(g.ntracks):
                g.set_track_state(t, trk[j][t], d)
        if scores:
            g.set_score_state(sco[j], d)


def everything(g, tracks=False, scores=False):
    """what the getters return of the whole handle, as bytes: the state (fifteen arrays, every scalar row, N_active), the status
    triple and the work counters; the track and score rows where asked for"""
    s, (status, step, layer) = g.get_state(), g.get_status()
    out = dict(scal=s.scal.view(np.uint64).copy(), n_active=s.n_active.copy(), status=status, step=step, layer=layer,
               work=np.array(g.get_work()))
    out["lay"] = s.lay.view(np.uint64).copy()
    if tracks:
        for t in range(g.ntracks):
            for f, r in g.tracks(t).items():
                out["track%d.%s" % (t, f)] = r.view(np.uint64).copy()
    if scores:
        for f, r in g.scores().items():
            out["score." + f] = r.view(np.uint64).copy()
    return out


def differing(a, b):
    """the names of the entries of two everything() that differ, with the columns that do"""
    return {k: np.unique(np.nonzero(a[k] != b[k])[-1])[:8].tolist() for k in a if not np.array_equal(a[k], b[k])}
