"""samsim_select_columns / samsim_get_columns on the GPU: which columns a predicate holds for, and the state of scattered columns.
Every comparison is equality of integers or of bytes against the numpy restatement of the header (tests/select_reference.py)
applied to get_state(), get_status(), the labels and tracks() of the same handle."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bench
import samsim_amd
from samsim_amd import capi
from samsim_amd import testcases as tcs
from samsim_amd.capi import A, NARR, NPROG, NSCAL, S, SELECT_MAX_OUT, Selection, State, TF, TrackSpec, hist_edges, track_slot
from tests import select_reference as sr
from tests.helpers import ROOT, golden
from tests.test_gpu_profile_stats import ensemble

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "host", "samsim_host.x")
SLOTS = ("thick_snow", "m_snow", "T_top", "N_active")
STOPPED = (5, 40000, 70000)
INF = float("inf")


@functools.lru_cache(maxsize=None)
def melting():
    """70 001 columns of the day-345 ensemble after 200 steps: more 64-column blocks than any grid of 1 024 waves, a ragged last
    block, three stopped columns.  Computed once, left unchanged (labels and tracks are removed again by whoever sets them)"""
    g = ensemble("sheba_ensemble_80_day345.npz", 70001, 200, corrupt=STOPPED)
    status = g.get_status()
    assert np.nonzero(status[0])[0].tolist() == list(STOPPED)
    return g, g.get_state(), status


@functools.lru_cache(maxsize=None)
def winter():
    """1 001 columns of the day-75 ensemble after 100 steps: 19-22 active layers of 80, so the lanes of a block end at different
    layers and S_bu is refreshed only where layers are active; three stopped columns"""
    g = ensemble("sheba_ensemble_80_day75.npz", 1001, 100, corrupt=(5, 400, 900))
    status = g.get_status()
    assert np.nonzero(status[0])[0].tolist() == [5, 400, 900]
    return g, status


def bounds(s, ok, name):
    """the 10 % and 90 % quantiles of a slot over the running columns"""
    q10, q90 = np.quantile(sr.slot_values(name, s)[ok], [0.1, 0.9])
    return float(q10), float(q90)


def same(got, want):
    (gi, gn), (wi, wn) = got, want
    return gi.dtype == np.int64 and gn == wn and gi.tobytes() == wi.tobytes()


# ------------------------------------------------------------------------------------------------------------ 1
def test_ascending_indices_and_exact_count():
    """One term per slot with the bounds [q10, q90) of the running columns.  thick_snow and m_snow are spread over this ensemble
    (56 051 and 56 049 of 69 998 running columns match on an MI355X) and their selections must be neither empty nor everything,
    else the test proves nothing.  T_top and N_active are not: 69 725 running columns of the melting ensemble hold T_top = 0.0 and
    all of them N_active = nlayer (tests/test_gpu_histogram.py meets the same), so q10 == q90 = v and [v, v) is empty for any
    implementation -- lo >= hi, which the header allows and which must match nothing on the device as well.  For these two the test
    also takes [v, the next double above v): it must match exactly the columns that hold v (69 725 and 69 998), which is asserted
    to be some, and that term is the one the ANDed selections use (55 503 matches for two terms and for four)."""
    g, s, (status, _, _) = melting()
    ok = status == 0
    terms, spread = [], []
    for name in SLOTS:
        lo, hi = bounds(s, ok, name)
        for term in [(name, lo, hi)] + ([] if hi > lo else [(name, lo, float(np.nextafter(hi, INF)))]):
            want = sr.select_reference(s, status, [term])
            got = g.select([term])
            print(name, "lo", term[1], "hi", term[2], "matches", want[1], "of", int(ok.sum()))
            assert same(got, want), term
            assert (np.diff(got[0]) > 0).all()
            again = g.select([term])
            assert again[1] == got[1] and again[0].tobytes() == got[0].tobytes()
        if hi > lo:
            spread.append(name)
            assert 0 < want[1] < ok.sum(), name              # else the test proves nothing
        else:
            assert g.select([(name, lo, hi)])[1] == 0 and want[1] > 0, name
        terms.append(term)
    assert {"thick_snow", "m_snow"} <= set(spread)
    for t in (terms[:2], terms):
        want = sr.select_reference(s, status, t)
        print(len(t), "terms ANDed:", want[1])
        assert 0 < want[1] < ok.sum() and same(g.select(t), want), len(t)
    idx, n = g.select(())
    assert n == g.ensemble_stats(["m_snow"])["m_snow"].count == ok.sum() and np.array_equal(idx, np.nonzero(ok)[0])


# ------------------------------------------------------------------------------------------------------------ 2
def test_truncation():
    g, s, (status, _, _) = melting()
    lo, hi = bounds(s, status == 0, "m_snow")
    sel = Selection.make([("m_snow", lo, hi)])
    full, n_match = g.select_raw(sel, SELECT_MAX_OUT)
    assert n_match == full.size > 65
    for max_out in (0, 1, 63, 64, 65, n_match - 1, n_match, n_match + 1):
        buf = np.full(n_match + 8, -77, dtype=np.int64)      # the sentinel
        idx, n = g.select_raw(sel, max_out, out=buf)
        k = min(max_out, n_match)
        assert n == n_match and idx.size == k, max_out
        assert buf[:k].tobytes() == full[:k].tobytes() and (buf[k:] == -77).all(), max_out


# ------------------------------------------------------------------------------------------------------------ 3
def test_status_modes():
    g, s, (status, _, _) = melting()
    code = int(status[STOPPED[0]])
    assert code != 0 and (status[list(STOPPED)] == code).all()
    idx, n = g.select((), status="stopped")
    assert idx.tolist() == list(STOPPED) and n == 3
    idx, n = g.select((), status=code)
    assert idx.tolist() == list(STOPPED) and n == 3
    idx, n = g.select((), status=code + 1)
    assert idx.size == 0 and n == 0
    for max_out in (1000, SELECT_MAX_OUT):
        idx, n = g.select((), status="any", max_out=max_out)
        assert n == g.ncol and np.array_equal(idx, np.arange(g.ncol)[:max_out])
    idx, n = g.select((), status="running")
    assert n == g.ncol - 3 and not np.isin(list(STOPPED), idx).any()
    # a stopped column is tested on the values it froze with
    t = [("N_active", -INF, INF)]
    assert same(g.select(t, status="stopped"), sr.select_reference(s, status, t, mode="stopped")) and g.select(t, status="stopped")[1] == 3


# ------------------------------------------------------------------------------------------------------------ 4
def test_agreement_with_the_histogram():
    g, s, (status, _, _) = melting()
    lo, hi = bounds(s, status == 0, "m_snow")
    nv, v0, dv = 30, lo, (hi - lo) / 30
    E = hist_edges(nv, v0, dv)
    hist = g.histogram("m_snow", nv, v0, dv)
    for j in range(nv):
        assert g.select([("m_snow", E[j], E[j + 1])], max_out=0)[1] == hist[j + 1], j
    assert g.select([("m_snow", E[nv], INF)], max_out=0)[1] == hist[nv + 1] > 0      # (no m_snow of this ensemble is +inf)
    assert (hist[1:-1] > 0).sum() >= 3                       # entry 0 is not compared: it also holds NaNs


# ------------------------------------------------------------------------------------------------------------ 5
def test_groups():
    g, s, (status, _, _) = melting()
    c = np.arange(g.ncol)
    lab = (c % 9).astype(np.int32)
    lab[::11] = -1
    lo, hi = bounds(s, status == 0, "m_snow")
    t = [("m_snow", lo, hi)]
    assert Selection.make((), group=3).group == 3
    f = g._f("select_columns")
    n = C.c_int64(-7)
    assert f(g._h, C.byref(Selection.make((), group=0)), 0, None, C.byref(n)) == -1 and n.value == -7   # no labels
    try:
        g.set_groups(lab, ngroups=9)
        before = g.select(t, group=3)
        assert 0 < before[1] < (lab == 3).sum() and same(before, sr.select_reference(s, status, t, group=3, labels=lab))
        assert g.select((), group=3)[1] == g.group_stats(["m_snow"])["m_snow"]["count"][3] == ((lab == 3) & (status == 0)).sum()
        lab2 = (lab + 5) % 9
        lab2[lab2 == 3] = 4
        lab2[c % 7 == 0] = -1
        lab2 = np.where(lab == 3, 3, lab2).astype(np.int32)
        assert np.array_equal(lab2 == 3, lab == 3) and (lab2 != lab).sum() > g.ncol // 2
        g.set_groups(lab2, ngroups=9)
        after = g.select(t, group=3)
        assert after[1] == before[1] and after[0].tobytes() == before[0].tobytes()
        assert not same(g.select(t, group=4), sr.select_reference(s, status, t, group=4, labels=lab))
        assert f(g._h, C.byref(Selection.make((), group=9)), 0, None, C.byref(n)) == -1
    finally:
        g.set_groups(None)


# ------------------------------------------------------------------------------------------------------------ 6
def test_track_slots():
    g = ensemble("sheba_ensemble_80_day345.npz", 5003, 0, corrupt=(70,))
    g.set_tracks([TrackSpec.make("ice_thickness")], every=50)
    g.step(200)
    s, status = g.get_state(), g.get_status()[0]
    rows = {0: g.tracks(0)}
    slot = track_slot(0, TF["MAX"])
    x = rows[0]["MAX"][status == 0]
    lo, hi = (float(q) for q in np.quantile(x, [0.25, 0.75]))
    want = sr.select_reference(s, status, [(slot, lo, hi)], tracks=rows)
    assert 0 < want[1] < x.size and same(g.select([(slot, lo, hi)]), want)
    both = [(slot, lo, hi), ("m_snow", -INF, float(np.median(s.sc("m_snow"))))]
    assert same(g.select(both), sr.select_reference(s, status, both, tracks=rows))
    g.set_tracks(None)
    n = C.c_int64(-7)
    assert g._f("select_columns")(g._h, C.byref(Selection.make([(slot, lo, hi)])), 0, None, C.byref(n)) == -1 and n.value == -7
    g.close()


# ------------------------------------------------------------------------------------------------------------ 7
def scattered(ncol, stopped, rng):
    """a permutation of 300 positions: the first and the last column, both sides of a 64-block boundary, the stopped columns, one
    duplicate"""
    must = sorted({0, ncol - 1, 63, 64, 127, 128, *stopped})
    rest = rng.choice(np.setdiff1d(np.arange(ncol), must), 300 - len(must) - 1, replace=False)
    cols = np.concatenate([must, rest, [int(rest[0])]]).astype(np.int64)
    cols = cols[rng.permutation(cols.size)]
    assert cols.size == 300 and np.unique(cols).size == 299 and (np.diff(cols) < 0).any()
    return cols


def check_columns(g, cols, status3):
    for narr in (NARR, NPROG):
        got, (st, sp, ly) = g.get_columns(cols, narr=narr, with_status=True)
        want = g.get_state(narr=narr)
        assert got.lay.shape == (narr, g.nlayer, cols.size) and got.scal.shape == (NSCAL, cols.size)
        assert got.lay.tobytes() == np.ascontiguousarray(want.lay[..., cols]).tobytes(), narr
        assert got.scal.tobytes() == np.ascontiguousarray(want.scal[..., cols]).tobytes(), narr
        assert got.n_active.tobytes() == np.ascontiguousarray(want.n_active[cols]).tobytes(), narr
        for a, b in zip((st, sp, ly), status3):
            assert a.dtype == b.dtype and a.tobytes() == np.ascontiguousarray(b[cols]).tobytes()
        plain = g.get_columns(cols, narr=narr)
        assert plain.lay.tobytes() == got.lay.tobytes() and plain.scal.tobytes() == got.scal.tobytes()


def test_get_columns_against_get_state():
    rng = np.random.default_rng(14)
    g, _, status3 = melting()
    check_columns(g, scattered(g.ncol, STOPPED, rng), status3)
    # winter() has not read its state: run in file order, get_columns comes first, on rows that no get_state has clamped or
    # refreshed on the device since the last step, and get_state after it returns the same bytes
    g, status3 = winter()
    cols = scattered(g.ncol, (5, 400, 900), rng)
    check_columns(g, cols, status3)
    na = g.get_state().n_active
    assert 19 <= na[status3[0] == 0].min() < na[status3[0] == 0].max() <= 22 and len(set(na[cols[:64]].tolist())) > 1


def test_get_columns_of_an_upload_and_of_a_stale_s_bu_row():
    """A handle never stepped returns the upload, negative S_abs and all: nothing is clamped, nothing is refreshed.  Whether a
    stepped handle holds an S_bu row that differs from S_abs / m cannot be read through the ABI (samsim_get_state refreshes the row
    before it returns it), so the test plants one: columns uploaded into a stepped handle keep their uploaded S_bu row on the device
    -- here 123.0 -- and a negative S_abs (no clamp in a column uploaded since the last step), and get_columns must return the
    quotient S_abs / m, not the stored 123.0, and leave the row to a later get_state, which returns the same bytes."""
    g = ensemble("sheba_ensemble_80_day75.npz", 1001, 0)
    up = g.get_state()
    up.arr("S_abs")[0, ::3] = -0.25
    up.arr("S_abs")[5, 1::7] = -1.0e-3
    up.arr("S_bu")[:] = 123.0
    g.set_state(up)
    cols = scattered(g.ncol, (5, 400, 900), np.random.default_rng(15))
    for narr in (NARR, NPROG):
        got = g.get_columns(cols, narr=narr)
        assert got.lay.tobytes() == np.ascontiguousarray(up.lay[:narr][..., cols]).tobytes()
        assert got.n_active.tobytes() == np.ascontiguousarray(up.n_active[cols]).tobytes()
        assert got.scal[:S["dT2m"]].tobytes() == np.ascontiguousarray(up.scal[:S["dT2m"]][..., cols]).tobytes()
    assert (g.get_columns(cols).arr("S_abs") < 0).any()
    g.step(20)
    win = g.get_state(64, 3)
    assert g.get_status()[0][65] == 0 and win.n_active[1] >= 6 and (win.arr("m")[:win.n_active[1], 1] != 0.0).all()
    win.arr("S_abs")[0] = -0.25
    win.arr("S_bu")[:] = 123.0
    g.set_state(win, 64)
    cols = np.array([66, 0, 65, 64, 1000, 65], dtype=np.int64)
    got = g.get_columns(cols)
    na = int(win.n_active[1])
    assert (got.arr("S_bu")[:na, 2] != 123.0).all() and (got.arr("S_bu")[na:, 2] == 123.0).all()     # column 65: the stored row is 123.0
    assert got.arr("S_abs")[0, 2] == -0.25 and got.arr("S_bu")[0, 2] == -0.25 / win.arr("m")[0, 1] < 0.0   # no clamp, the quotient
    want = g.get_state()
    assert got.lay.tobytes() == np.ascontiguousarray(want.lay[..., cols]).tobytes()
    g.close()


# ------------------------------------------------------------------------------------------------------------ 8
def test_get_columns_and_select_leave_the_ensemble_alone():
    a = ensemble("sheba_ensemble_80_day345.npz", 5003, 0, corrupt=(70,))
    b = ensemble("sheba_ensemble_80_day345.npz", 5003, 0, corrupt=(70,))
    cols = scattered(a.ncol, (70,), np.random.default_rng(16))
    for _ in range(3):
        a.step(20)
        idx, n = a.select([("m_snow", 0.0, INF), ("N_active", 1.0, INF)], status="any")
        assert n > 0
        a.get_columns(cols)
        a.get_columns(idx[:500], narr=NPROG, with_status=True)
        b.step(20)
    sa, sb = a.get_state(), b.get_state()
    assert sa.lay.tobytes() == sb.lay.tobytes() and sa.scal.tobytes() == sb.scal.tobytes() and sa.n_active.tobytes() == sb.n_active.tobytes()
    for x, y in zip(a.get_status(), b.get_status()):
        assert x.tobytes() == y.tobytes()
    ca, cb = a.get_clock(), b.get_clock()
    assert bytes(ca) == bytes(cb) and ca.step == cb.step and a.get_work() == b.get_work()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------ 9
def test_pieces():
    """The second of the issue's two ways (tests/test_gpu_large_handle.py shows no build with a smaller SAMSIM_STAGE_MAX_BYTES, a
    plain define of the header): SAMSIM_SELECT_MAX_OUT scattered columns of a 20-layer, 300 000-column handle, 15 x 20 x 262 144 x 8 B
    = 629 MB through the 256 MiB staging buffer in three pieces.  The handle is never stepped and holds a value of its own in every
    element (exact integers), so any position that takes its element from another column, layer or array shows.  1 000 sampled
    positions and both sides of both piece boundaries are held against get_state."""
    ncol, N = 300000, 20
    cfg, _ = tcs.testcase4(1, nlayer=N, n_top=5, n_bottom=5)
    g = samsim_amd.hip_solver(cfg, ncol)
    st = State.empty(ncol, N)
    st.lay[:] = (np.arange(NARR * N, dtype=np.float64) * float(1 << 20)).reshape(NARR, N, 1) + np.arange(ncol, dtype=np.float64)
    st.scal[:] = -(np.arange(NSCAL, dtype=np.float64) * float(1 << 20)).reshape(NSCAL, 1) - np.arange(ncol, dtype=np.float64)
    st.n_active[:] = 1 + np.arange(ncol) % N
    g.set_state(st)
    rng = np.random.default_rng(17)
    cols = rng.permutation(ncol)[:SELECT_MAX_OUT].astype(np.int64)
    stage = int(re.search(r"^#define SAMSIM_STAGE_MAX_BYTES \((\d+)ull << 20\)", open(os.path.join(ROOT, "include", "samsim.h")).read(),
                          re.M).group(1)) << 20
    piece = (stage // (NARR * N * 8)) & ~63
    assert 2 * piece < cols.size <= 3 * piece              # three pieces
    got = g.get_columns(cols)
    want = g.get_state()
    pos = np.unique(np.concatenate([rng.integers(0, cols.size, 1000), [0, piece - 1, piece, 2 * piece - 1, 2 * piece, cols.size - 1]]))
    assert got.lay[..., pos].tobytes() == want.lay[..., cols[pos]].tobytes()
    assert got.scal[..., pos].tobytes() == want.scal[..., cols[pos]].tobytes()
    assert got.n_active[pos].tobytes() == want.n_active[cols[pos]].tobytes()
    # and every position against the value it must hold
    assert np.array_equal(got.lay[0, 0], cols.astype(np.float64)) and np.array_equal(got.lay[NARR - 1, N - 1] - float((NARR * N - 1) << 20), cols)
    assert np.array_equal(got.lay - got.lay[0, 0], np.broadcast_to((np.arange(NARR * N, dtype=np.float64) * float(1 << 20)).reshape(NARR, N, 1),
                                                                got.lay.shape))
    g.close()


# ------------------------------------------------------------------------------------------------------------ 10
def test_errors():
    g, status3 = winter()
    sel_f, get_f = g._f("select_columns"), g._f("get_columns")
    out, n = np.full(16, -77, dtype=np.int64), C.c_int64(-7)

    def select(sel, max_out=16, cols=out, nm=n, h=None):
        return sel_f(g._h if h is None else h, C.byref(sel) if sel is not None else None, max_out,
                     cols.ctypes.data if cols is not None else None, C.byref(nm) if nm is not None else None)

    def made(**k):
        sel = Selection.make([("m_snow", 0.0, 1.0), ("T_top", -1.0, 1.0)])
        for name, v in k.items():
            setattr(sel, name, v)
        return sel

    def term(i, **k):
        sel = made()
        for name, v in k.items():
            setattr(sel.terms[i], name, v)
        return sel
    good = made()
    bad_size = made(struct_size=good.struct_size - 8)
    # in the order of the header: NULL pointers, the struct size, then the SAMSIM_ERR_ARG list
    assert select(good, h=C.c_void_p()) == -1 and select(None) == -1 and select(good, nm=None) == -1
    assert select(bad_size, nm=None) == -1                                  # a NULL pointer is found before the struct size
    assert select(bad_size) == -6
    bad_size.nterms = 9
    assert select(bad_size) == -6                                           # ... and the struct size before nterms
    assert select(made(nterms=-1)) == -1 and select(made(nterms=capi.SELECT_MAX_TERMS + 1)) == -1
    for i in (0, 1):
        for slot in (NSCAL, -2, track_slot(0, 0)):                          # (no tracks are set on this handle)
            assert select(term(i, slot=slot)) == -1, (i, slot)
        assert select(term(i, reserved=1)) == -1
        assert select(term(i, lo=float("nan"))) == -1 and select(term(i, hi=float("nan"))) == -1
    assert select(term(3, slot=NSCAL, reserved=1, lo=float("nan"))) == 0    # a term beyond nterms is not looked at
    assert select(made(group=-2)) == -1 and select(made(group=0)) == -1     # (no labels are set on this handle)
    assert select(made(status_mode=-1)) == -1 and select(made(status_mode=4)) == -1
    for mode in (0, 1, 3):
        assert select(made(status_mode=mode, code=99)) == -1, mode
    assert select(made(status_mode=2, code=99)) == 0
    assert select(made(reserved=1)) == -1
    assert select(good, max_out=-1) == -1 and select(good, max_out=SELECT_MAX_OUT + 1) == -1 and select(good, max_out=1, cols=None) == -1
    assert select(good, max_out=0, cols=None) == 0
    n.value = -7
    out[:] = -77
    for bad in (made(reserved=1), made(group=0)):
        assert select(bad) == -1 and n.value == -7 and (out == -77).all()       # a refused call writes nothing
    # lo >= hi and infinite bounds are no errors
    one = Selection.make([("m_snow", 2.0, 1.0)])
    assert select(one) == 0 and n.value == 0
    one.terms[0].lo, one.terms[0].hi = -INF, INF
    assert select(one) == 0 and n.value == g.ncol - 3 and out.tolist() == [0, 1, 2, 3, 4, 6] + list(range(7, 17))

    # samsim_get_columns
    ncols = 8
    cols = np.array([3, 1000, 0, 64, 63, 3, 900, 5], dtype=np.int64)
    st = State.empty(ncols, g.nlayer)
    st.lay[:], st.scal[:], st.n_active[:] = -77.0, -77.0, -77
    stat, step, lay = np.full(ncols, -77, dtype=np.int32), np.full(ncols, -77, dtype=np.int64), np.full(ncols, -77, dtype=np.int32)

    def get(n_=ncols, c=cols, h=None, s="default", **k):
        soa = st._c()
        for name, v in k.items():
            setattr(soa, name, v)
        return get_f(g._h if h is None else h, n_, c.ctypes.data if c is not None else None,
                     C.byref(soa) if s == "default" else None, stat.ctypes.data, step.ctypes.data, lay.ctypes.data)

    def untouched():
        return (st.lay == -77.0).all() and (st.scal == -77.0).all() and (st.n_active == -77).all() and (stat == -77).all() \
            and (step == -77).all() and (lay == -77).all()
    refusals = [dict(h=C.c_void_p()), dict(c=None), dict(s=None), dict(lay=None), dict(scal=None), dict(n_active=None),
                dict(nlayer=g.nlayer - 1), dict(narr=NARR - 1), dict(narr=0), dict(n_=0, ncol=0), dict(n_=-1, ncol=-1),
                dict(n_=SELECT_MAX_OUT + 1, ncol=SELECT_MAX_OUT + 1), dict(ncol=ncols - 1), dict(ncol=ncols + 1),
                dict(c=np.array([3, 1000, 0, 64, 63, 3, g.ncol, 5], dtype=np.int64)),
                dict(c=np.array([3, 1000, 0, 64, 63, 3, 900, -1], dtype=np.int64))]
    for r in refusals:
        assert get(**r) == -1, r
        assert untouched(), r
    # after all refusals a good call still succeeds, and so does a good selection
    assert get() == 0 and not untouched()
    want = g.get_state()
    assert st.lay.tobytes() == np.ascontiguousarray(want.lay[..., cols]).tobytes() and stat.tobytes() == status3[0][cols].tobytes()
    assert step.tobytes() == status3[1][cols].tobytes() and lay.tobytes() == status3[2][cols].tobytes()
    idx, nm = g.select([("m_snow", -INF, INF)], status="any")
    assert nm == idx.size > 0


# ------------------------------------------------------------------------------------------------------------ 11
@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran host not built (no flang)")
def test_fortran_host_member_files(tmp_path):
    """members_thinner / members_max in &samsim_run: the four dat_ens_members*.dat files hold the columns Solver.select returns for an
    identically set up handle and, at the printed precision (ES16.8), what Solver.get_columns returns for them; without the key no new
    file appears and dat_ensemble.dat keeps its bytes.

    Testcase 4 with 96 perturbed columns, as test_fortran_host_track_file sets it up, but restarted from a checkpoint of the day-75
    ensemble and run 100 steps, through one output point (n_time_out of the fixture's clock is 8 565 of 8 640).  From open water the
    thickness slot -- the vital sign of the last output point -- is 0.0 in every column at 600 steps, past the first output point and
    still after 43 300 steps (five output points, measured on an MI355X): no threshold splits that ensemble.  The day-75 members hold
    96 distinct values between 0.18 m and 0.21 m."""
    from samsim_amd import checkpoint
    sheba = golden("sheba_forcing.npz")
    keys = (("fl_sw", "flux_sw"), ("fl_lw", "flux_lw"), ("T2m", "T2m"), ("precip", "precip"))
    ncol, nsteps = 96, 100
    z, st, clock, _ = bench.load_ensemble("sheba_ensemble_80_day75.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    assert clock["n_time_out"] + nsteps > cfg.i_time_out > clock["n_time_out"]      # an output point lies inside the run
    total = clock["step"] + nsteps

    def fresh():
        g = samsim_amd.hip_solver(cfg, ncol)
        g.set_forcing(*[sheba[k] for k, _ in keys], *tcs.ensemble_perturbation(ncol))
        return g
    g = fresh()
    g.set_state(State(bench.tile(st.lay, ncol), bench.tile(st.scal, ncol), bench.tile(st.n_active, ncol).astype(np.int32)))
    g.set_clock(**clock)
    chk = tmp_path / "day75.chk"
    checkpoint.save(g, str(chk))
    g.close()
    g = fresh()                                              # what the host does: the forcing, then the checkpoint
    checkpoint.load(g, str(chk))
    g.step(nsteps)
    thick = g.get_state().sc("thickness")
    thr = float(np.median(thick)) + 1e-9
    idx_all, n_match = g.select([("thickness", -INF, thr)])
    print("thickness", thick.min(), "..", thick.max(), "distinct", np.unique(thick).size, "threshold", thr, "matches", n_match)
    assert ncol // 4 <= n_match <= 3 * ncol // 4
    members_max = n_match - 5                                # below the number of matches: the cap is exercised
    idx = idx_all[:members_max]
    want = g.get_columns(idx)
    g.close()

    def run(d, extra, ok=True):
        (d / "output").mkdir(parents=True)
        for key, name in keys:
            np.savetxt(d / f"{name}.txt.input", sheba[key], fmt="%.17e")
        (d / "samsim.nml").write_text(f"&samsim_run testcase=4, ncol={ncol}, perturb=.true., max_steps={total}, restart_in='{chk}'{extra} /\n"
                                      f"&samsim_flags Nlayer={cfg.nlayer}, N_top={cfg.n_top}, N_bottom={cfg.n_bottom} /\n")
        r = subprocess.run([HOST], cwd=d, capture_output=True, text=True, timeout=900)
        assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-2000:]
        return (d / "output") if ok else r
    with_members = run(tmp_path / "members", f", members_thinner={thr!r}, members_max={members_max}")
    plain = run(tmp_path / "plain", "")
    new = ["dat_ens_members.dat", "dat_ens_members_S_bu.dat", "dat_ens_members_T.dat", "dat_ens_members_thick.dat"]
    assert sorted(set(os.listdir(with_members)) - set(os.listdir(plain))) == new
    assert (plain / "dat_ensemble.dat").read_bytes() == (with_members / "dat_ensemble.dat").read_bytes()

    def printed(got, want):
        """ES16.8 prints nine digits: half a unit of the ninth"""
        tol = 0.5e-8 * 10.0 ** math.floor(math.log10(abs(want))) * (1.0 + 1e-6) if want != 0.0 else 0.0
        return abs(got - want) <= tol
    f = np.loadtxt(with_members / "dat_ens_members.dat", ndmin=2)
    assert f.shape == (members_max, 5) and f[:, 0].astype(np.int64).tolist() == idx.tolist()
    assert f[:, 1].astype(np.int32).tolist() == want.n_active.tolist()
    for j in range(members_max):
        assert all(printed(a, b) for a, b in zip(f[j, 2:], (want.sc("thickness")[j], want.sc("thick_snow")[j], want.sc("T_top")[j]))), j
    for name in ("T", "S_bu", "thick"):
        p = np.loadtxt(with_members / f"dat_ens_members_{name}.dat", ndmin=2)
        assert p.shape == (members_max, cfg.nlayer)
        w = want.arr(name).T
        bad = [(j, k) for j in range(members_max) for k in range(cfg.nlayer) if not printed(p[j, k], w[j, k])]
        assert not bad, (name, bad[:5])
    r = run(tmp_path / "negative", ", members_thinner=-0.5", ok=False)
    assert "members_thinner" in r.stdout and not os.listdir(tmp_path / "negative" / "output")
    r = run(tmp_path / "toomany", f", members_thinner=0.5, members_max={SELECT_MAX_OUT + 1}", ok=False)
    assert "members_max" in r.stdout
