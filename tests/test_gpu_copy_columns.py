"""Whole columns copied in place on the GPU (samsim_copy_columns, samsim_apply_resample, samsim_get_copy_plan): the step that puts the
copies of a posterior draw where the dropped members were.  The oracle is the library itself: a second handle built the same way takes
the route through the host the header defines the copy by (tests/copy_reference.host_route: get_columns, set_state, set_status, the
tracer, track and score setters), and every comparison is byte for byte -- there is nothing to tolerate.  The plan is compared with
the numpy rule of tests/copy_reference.plan applied to the downloaded offspring row, status and labels of the same handle.

The large handle (70 001 columns, 12 layers, never stepped: 1 094 blocks, per = 2, a ragged last block, three stopped columns, the
last column among them) is the one of tests/test_gpu_resample.py with every column made different from every other; the tests that
write to it upload its state again first."""
import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi, testcases as tcs
from samsim_amd.capi import NPROG, S, ApplyInfo, SamsimError, TrackSpec
from tests import copy_reference as cr
from tests.test_gpu_group_stats import labels_of_test_1
from tests.test_gpu_profile_stats import ensemble
from tests.test_gpu_weights import BUOY, J_SUM, scored_ensemble, snapshot

pytestmark = pytest.mark.gpu
NCOL = 70001
STOPPED = (5, 40000, 70000)
BEST = 45678
R_RAND, R_ONE, R_DEG, R_ID = "energy_stored", "fl_rest", "melt_err", "freshwater"
DT2M = S["dT2m"]
# the pair list of the byte-for-byte tests, on 300 columns (four blocks of 64 and a ragged one of 44): source 10 three times -- into
# lane 63 of its own block, lane 0 of the next and the last column of the ragged block --, the stopped column 200, and 250 into lane 1
SRC = np.array([10, 10, 10, 200, 250], dtype=np.int64)
DST = np.array([63, 64, 299, 130, 1], dtype=np.int64)
STOP = (200, 7, 2, 5)                          # column, code, step, layer


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def state_bytes(g):
    """the ensemble as the getters return it: state, status triple, work"""
    return cr.everything(g)


def same(a, b, what):
    d = cr.differing(a, b)
    assert not d, (what, d)


def small_pair(tracks_and_scores=False):
    """two handles of the day-200 ensemble tiled to 300 columns, 80 layers, three steps on, column 200 stopped"""
    out = []
    for _ in range(2):
        g = ensemble("sheba_ensemble_80.npz", 300, 0)
        if tracks_and_scores:
            g.set_tracks([TrackSpec.make("ice_thickness"), TrackSpec.make("scalar", "T_top")], 1)
        g.step(3)
        assert not g.get_status()[0].any()
        if tracks_and_scores:
            g.set_sensors(BUOY)
            g.score(g.sensor_values([77])[:, 0])
        c, code, step, layer = STOP
        g.set_status(np.array([code], dtype=np.int32), np.array([step], dtype=np.int64), np.array([layer], dtype=np.int32), col0=c)
        out.append(g)
    return out


# ------------------------------------------------------------------------------------- 1: equal to the host route, byte for byte
@pytest.mark.parametrize("rows", [False, True])
def test_the_copy_equals_the_route_through_the_host(rows):
    a, b = small_pair(rows)
    a.copy_columns(SRC, DST, tracks=rows, scores=rows)
    cr.host_route(b, SRC, DST, tracks=rows, scores=rows)
    ea, eb = cr.everything(a, rows, rows), cr.everything(b, rows, rows)
    same(ea, eb, "after the copy")
    # the copy of the stopped column is stopped, with the same step and layer; the others run
    c, code, step, layer = STOP
    assert (ea["status"][130], ea["step"][130], ea["layer"][130]) == (code, step, layer) and np.flatnonzero(ea["status"]).tolist() == [130, c]
    # and it is a copy: the bytes get_columns forms for the sources
    got = a.get_columns(DST)
    want = a.get_columns(SRC)
    assert got.lay.tobytes() == want.lay.tobytes() and got.n_active.tobytes() == want.n_active.tobytes()
    assert got.scal[:DT2M].tobytes() == want.scal[:DT2M].tobytes() and got.scal[DT2M:].tobytes() != want.scal[DT2M:].tobytes()
    if rows:
        assert ea["score.J_SUM"][DST[0]] == ea["score.J_SUM"][SRC[0]] != 0 and ea["track0.N"].view(np.float64)[DST[0]] == 3.0
    for g in (a, b):
        g.step(5)
    same(cr.everything(a, rows, rows), cr.everything(b, rows, rows), "five steps later")
    assert np.flatnonzero(a.get_status()[0]).tolist() == [130, c]
    a.close()
    b.close()


def test_the_copy_of_a_stale_s_bu_row_and_an_uploaded_negative_s_abs():
    """as tests/test_gpu_select.py plants them for the gather: columns uploaded into a stepped handle keep their uploaded S_bu row
    (123.0) and a negative S_abs (no clamp since the upload); the copy carries the quotient over the active layers, the stored row
    below them and the negative value, as get_columns forms them"""
    a, b = small_pair()
    for g in (a, b):
        win = g.get_state(64, 3)
        assert win.n_active[1] >= 6 and (win.arr("m")[:win.n_active[1], 1] != 0.0).all()
        win.arr("S_abs")[0] = -0.25
        win.arr("S_bu")[:] = 123.0
        g.set_state(win, 64)
    src, dst = np.array([65, 65, 10], dtype=np.int64), np.array([5, 290, 66], dtype=np.int64)
    na, m0 = int(win.n_active[1]), win.arr("m")[0, 1]
    a.copy_columns(src, dst)
    cr.host_route(b, src, dst)
    same(state_bytes(a), state_bytes(b), "after the copy")
    got = a.get_columns(np.array([5, 290, 65]))
    assert (got.arr("S_bu")[:na] != 123.0).all() and (got.arr("S_bu")[na:] == 123.0).all()
    assert (got.arr("S_abs")[0] == -0.25).all() and (got.arr("S_bu")[0] == -0.25 / m0).all()
    for g in (a, b):
        g.step(5)
    same(state_bytes(a), state_bytes(b), "five steps later")
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 2: a copy continues as its source
def test_a_copy_with_its_forcing_continues_as_its_source():
    g = ensemble("sheba_ensemble_80.npz", 300, 3)
    src, dst = np.array([10, 20, 20], dtype=np.int64), np.array([70, 299, 21], dtype=np.int64)
    before = g.get_state()
    assert u64(before.scal[DT2M:, src]).tobytes() != u64(before.scal[DT2M:, dst]).tobytes()
    g.copy_columns(src[:1], dst[:1])                                      # without the flag: the slot keeps its perturbations
    s = g.get_state()
    assert u64(s.scal[DT2M:]).tobytes() == u64(before.scal[DT2M:]).tobytes()
    assert u64(s.scal[:DT2M, 70]).tobytes() == u64(before.scal[:DT2M, 10]).tobytes()
    g.copy_columns(src, dst, forcing=True)
    s = g.get_state()
    assert u64(s.scal[:, dst]).tobytes() == u64(before.scal[:, src]).tobytes()
    g.step(5)
    s = g.get_state()
    assert not g.get_status()[0].any()
    # the criterion of tests/test_gpu_ensemble_io.py for a restart from a full state: the prognostic arrays, the scalars, N_active
    assert u64(s.lay[:NPROG][..., dst]).tobytes() == u64(s.lay[:NPROG][..., src]).tobytes()
    assert u64(s.scal[:, dst]).tobytes() == u64(s.scal[:, src]).tobytes()
    assert np.array_equal(s.n_active[dst], s.n_active[src])
    assert u64(s.lay[:NPROG][..., 70]).tobytes() != u64(s.lay[:NPROG][..., 71]).tobytes()
    g.close()


# ------------------------------------------------------------------------------------------------- 3: nothing else is written
def columns_of(snap, ncol, keep):
    """the snapshot of tests/test_gpu_weights.py restricted to the columns `keep`"""
    def rows(b, dtype):
        return np.frombuffer(b, dtype=dtype).reshape(-1, ncol)[:, keep].tobytes()
    out = dict(lay=rows(snap["lay"], np.uint64), scal=rows(snap["scal"], np.uint64), n_active=rows(snap["n_active"], np.int32),
               status=rows(snap["status"], np.int32), err_step=rows(snap["err_step"], np.int64), err_layer=rows(snap["err_layer"], np.int32),
               functionals=rows(snap["functionals"], np.uint64), clock=snap["clock"], work=snap["work"], output=snap["output"])
    for name in ("tracks", "scores"):
        out[name] = {f: rows(b, np.uint64) for f, b in snap[name].items()}
    return out


def test_nothing_but_the_destinations_is_written():
    ncol = 300
    lab = (np.arange(ncol) % 3).astype(np.int32)
    handles = [scored_ensemble(ncol, (5,), lab, 3, 77)[0] for _ in range(2)]
    keep = np.setdiff1d(np.arange(ncol), DST)
    for g in handles:
        g.set_weights(J_SUM, "gauss", 50.0)
        g.resample(ncol - 1)
    g = handles[0]
    before = snapshot(g)
    w, N, anc = g.weights(), g.offspring(), g.ancestors()
    groups = [g.select(group=k, status="any")[0] for k in range(3)]
    for h in handles:
        h.copy_columns(SRC, DST, tracks=True, scores=True)
    after = snapshot(g)
    assert columns_of(after, ncol, keep) == columns_of(before, ncol, keep)
    assert columns_of(after, ncol, DST) != columns_of(before, ncol, DST)
    assert g.weights().tobytes() == w.tobytes() and g.offspring().tobytes() == N.tobytes() and g.ancestors().tobytes() == anc.tobytes()
    assert all(np.array_equal(g.select(group=k, status="any")[0], groups[k]) for k in range(3))
    # two handles given the same call hold the same bytes
    assert snapshot(handles[1]) == after
    for h in handles:
        h.close()


# ------------------------------------------------------------------------------------------- 4, 5, 6: the plan, on the large handle
@pytest.fixture(scope="module")
def big():
    assert cr.grid_rule(NCOL) == (1094, 2, 547) and NCOL % 64 != 0 and STOPPED[-1] == NCOL - 1
    rng = np.random.default_rng(23)
    cfg, st = tcs.testcase4(NCOL, nlayer=12, n_top=4, n_bottom=4)
    ident = np.arange(NCOL, dtype=np.float64)
    st.sc(R_RAND)[:] = np.where(rng.uniform(size=NCOL) < 0.2, 0.0, rng.exponential(1.0, NCOL))
    st.sc(R_ONE)[:] = 1.0
    st.sc(R_DEG)[:] = 1.0 + rng.uniform(0.001, 5.0, NCOL)
    st.sc(R_DEG)[BEST] = 0.5
    st.sc(R_ID)[:] = ident
    st.arr("T")[:] = -ident[None, :] / NCOL - np.arange(12)[:, None]        # every column different in every layer
    st.arr("flush_h")[:] = ident[None, :]                                   # and in the last of the fifteen arrays
    st.n_active[:] = 3 + (np.arange(NCOL) % 9)
    g = samsim_amd.hip_solver(cfg, NCOL)
    lab = labels_of_test_1(NCOL)
    g.set_groups(lab, ngroups=11)
    g.set_clock()
    lab.setflags(write=False)
    return dict(g=g, st=st, lab=lab)


def fresh(big):
    """the large handle with its state as built, three columns stopped and no resample rows"""
    g = big["g"]
    g.set_state(big["st"])
    for c in STOPPED:
        g.set_status(np.array([7], dtype=np.int32), col0=c)
    g.clear_resample()
    status = g.get_status()[0]
    assert sorted(np.flatnonzero(status)) == list(STOPPED)
    return g, status


def check_apply(g, status, lab, group, what):
    """apply the rows in force: plan and info against the rule, the destinations hold the sources' bytes, nothing else moved"""
    r = cr.plan(g.offspring(), status, lab, group)
    assert r["balanced"], what
    before = g.get_state()
    info = g.apply_resample()
    src, dst = g.copy_plan()
    assert info == r["info"] and info["n_free"] == info["n_copies"] == src.size, (what, info, r["info"])
    assert np.array_equal(src, r["src"]) and np.array_equal(dst, r["dst"]), what
    after = g.get_state()
    assert u64(after.lay[..., dst]).tobytes() == u64(before.lay[..., src]).tobytes(), what
    assert u64(after.scal[:DT2M, dst]).tobytes() == u64(before.scal[:DT2M, src]).tobytes(), what
    assert np.array_equal(after.n_active[dst], before.n_active[src]), what
    others = np.setdiff1d(np.arange(g.ncol), dst)
    assert u64(after.lay[..., others]).tobytes() == u64(before.lay[..., others]).tobytes(), what
    assert u64(after.scal[:, others]).tobytes() == u64(before.scal[:, others]).tobytes(), what
    assert u64(after.scal[DT2M:]).tobytes() == u64(before.scal[DT2M:]).tobytes(), what
    assert np.array_equal(after.n_active[others], before.n_active[others]) and np.array_equal(g.get_status()[0], status), what
    # windows of the stored plan
    if src.size > 10:
        s2, d2 = g.copy_plan(3, 5)
        assert np.array_equal(s2, src[3:8]) and np.array_equal(d2, dst[3:8])
    return r, before, after


@pytest.mark.parametrize("group", [None, 3])
def test_the_plan_equals_the_rule_and_the_copies_their_sources(big, group):
    g, status = fresh(big)
    lab = big["lab"]
    pool = cr.pool_of(status, lab, group)
    m = int(pool.sum())
    assert m == (NCOL - 3 if group is None else m) and (group is None or 6000 < m < 8000)
    g.set_weights(R_RAND, "direct")
    for kind, u0, seed in (("systematic", 0.73, 0), ("stratified", 0.0, 20261021)):
        what = f"group {group}, {kind}"
        info = g.resample(m, kind, u0, seed, group)
        assert info["m_drawn"] == m and info["max_offspring"] >= 3
        r, before, after = check_apply(g, status, lab, group, what)
        assert r["info"]["n_copies"] > m // 5 and pool[r["dst"]].all() and pool[r["src"]].all()
        # the columns outside the group are untouched, as sources and as destinations
        outside = np.flatnonzero(~pool)
        assert u64(after.lay[..., outside]).tobytes() == u64(before.lay[..., outside]).tobytes()
        # member c is now held N_c times: the identity row says who sits where
        N = g.offspring().astype(np.int64)
        held = after.sc(R_ID)[pool].astype(np.int64)
        was = before.sc(R_ID).astype(np.int64)
        assert np.array_equal(np.bincount(held, minlength=NCOL), np.bincount(was, weights=N, minlength=NCOL).astype(np.int64)), what
        g.set_weights(R_RAND, "direct")                                   # the next draw weighs the members where they sit now


def test_one_member_takes_every_draw(big):
    g, status = fresh(big)
    m = NCOL - 3
    g.set_weights(R_DEG, "gauss", 1e-9)
    info = g.resample(m, "systematic", 0.37)
    assert info["n_survivors"] == 1 and info["max_offspring"] == m and info["argmax_offspring"] == BEST
    r, before, after = check_apply(g, status, big["lab"], None, "degenerate")
    assert r["info"] == dict(n_pool=m, n_free=m - 1, n_copies=m - 1, n_sources=1) and (r["src"] == BEST).all()
    running = np.flatnonzero(status == 0)
    assert (after.sc(R_ID)[running] == BEST).all() and (after.arr("flush_h")[:, running] == BEST).all()
    assert after.sc(R_ID)[list(STOPPED)].tolist() == list(STOPPED)


def test_unit_weights_copy_nothing(big):
    g, status = fresh(big)
    g.set_weights(R_ONE, "direct")
    g.resample(NCOL - 3, "stratified", seed=5)
    before = state_bytes(g)
    info = g.apply_resample()
    assert info == dict(n_pool=NCOL - 3, n_free=0, n_copies=0, n_sources=0)
    src, dst = g.copy_plan()
    assert src.size == 0 and dst.size == 0
    same(state_bytes(g), before, "unit weights")
    with pytest.raises(SamsimError) as e:                                 # and the rows count as applied
        g.apply_resample()
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_leave_the_ensemble_and_the_stored_plan(big):
    g, status = fresh(big)
    lab = big["lab"]
    m = NCOL - 3

    def refused(code, call):
        with pytest.raises(SamsimError) as e:
            call()
        assert e.value.code == code, (e.value.code, code)

    # before any apply of a handle there is no plan; without resample rows there is nothing to apply
    cfg, st = tcs.testcase1(8)
    small = samsim_amd.hip_solver(cfg, 8)
    small.set_state(st)
    buf = np.zeros(4, dtype=np.int64)
    assert small._f("get_copy_plan")(small._h, 0, 0, buf.ctypes.data, buf.ctypes.data) == -1
    refused(-1, small.apply_resample)
    small.close()
    # a plan in force
    g.set_weights(R_RAND, "direct")
    g.resample(m, "systematic", 0.25)
    g.apply_resample()
    plan = g.copy_plan()
    n_plan = plan[0].size
    before = state_bytes(g)
    info = ApplyInfo(-7, -7, -7, -7)

    def unchanged(what):
        same(state_bytes(g), before, what)
        src, dst = g.copy_plan(0, n_plan)
        assert np.array_equal(src, plan[0]) and np.array_equal(dst, plan[1]), what
        assert (info.n_pool, info.n_free, info.n_copies, info.n_sources) == (-7, -7, -7, -7), what

    refused(-1, lambda: g.apply_resample_raw(0, info))                    # a second apply
    unchanged("second apply")
    g.set_weights(R_RAND, "direct")
    for m_bad in (m - 1, m + 1, 3 * m):                                   # a draw of another size than the pool
        g.resample(m_bad, "systematic", 0.25)
        refused(-2, lambda: g.apply_resample_raw(0, info))
    unchanged("m != n_pool")
    g.resample(m, "systematic", 0.25, group=3)                            # a draw over a group with the size of the whole pool
    refused(-2, lambda: g.apply_resample_raw(0, info))
    unchanged("m of another pool")
    for what in (8, -1, 16 + 1):                                          # unknown bits, then rows the handle does not have
        refused(-1, lambda: g.apply_resample_raw(what, info))
    refused(-1, lambda: g.apply_resample_raw(capi.COPY_TRACKS, info))
    refused(-1, lambda: g.apply_resample_raw(capi.COPY_SCORES, info))
    unchanged("what")
    # a survivor that stopped between the draw and the apply
    g.resample(m, "systematic", 0.25)
    N = g.offspring()
    c = int(np.flatnonzero(N >= 1)[7])
    g.set_status(np.array([9], dtype=np.int32), col0=c)
    mid = state_bytes(g)
    refused(-2, lambda: g.apply_resample_raw(0, info))
    same(state_bytes(g), mid, "stopped survivor")
    g.set_status(np.array([0], dtype=np.int32), np.array([0], dtype=np.int64), np.array([0], dtype=np.int32), col0=c)
    unchanged("stopped survivor")
    # the refusals of copy_columns, in the documented order
    ok_src, ok_dst = np.array([1, 1, 2], dtype=np.int64), np.array([10, 11, 12], dtype=np.int64)
    raw = g.copy_columns_raw
    refused(-1, lambda: raw(3, None, ok_dst, 0))
    refused(-1, lambda: raw(3, ok_src, None, 0))
    for n in (0, -1, NCOL + 1):
        refused(-1, lambda: raw(n, ok_src, ok_dst, 0))
    for what in (8, -1, 32):
        refused(-1, lambda: raw(3, ok_src, ok_dst, what))
    refused(-1, lambda: raw(3, ok_src, ok_dst, capi.COPY_TRACKS))
    refused(-1, lambda: raw(3, ok_src, ok_dst, capi.COPY_SCORES))
    for bad in (-1, NCOL, 1 << 40):
        refused(-1, lambda: raw(3, np.array([1, bad, 2], dtype=np.int64), ok_dst, 0))
        refused(-1, lambda: raw(3, ok_src, np.array([10, 11, bad], dtype=np.int64), 0))
    refused(-1, lambda: raw(3, ok_src, np.array([10, 11, 10], dtype=np.int64), 0))        # a dst listed twice
    refused(-1, lambda: raw(3, ok_src, np.array([10, 2, 12], dtype=np.int64), 0))         # a dst that is a src
    refused(-1, lambda: raw(3, np.array([1, 12, 2], dtype=np.int64), ok_dst, 0))          # a src that is a later dst
    unchanged("copy_columns")
    # a good copy_columns does not change the stored plan either, and a new draw can be applied after the refusals
    g.copy_columns(ok_src, ok_dst)
    src, dst = g.copy_plan(0, n_plan)
    assert np.array_equal(src, plan[0]) and np.array_equal(dst, plan[1])
    for k0, nk in ((-1, 2), (0, -1), (n_plan, 1), (n_plan + 1, 0), (0, n_plan + 1)):
        assert g._f("get_copy_plan")(g._h, k0, nk, buf.ctypes.data, buf.ctypes.data) == -1, (k0, nk)
    assert g._f("get_copy_plan")(g._h, n_plan, 0, buf.ctypes.data, buf.ctypes.data) == 0
    status = g.get_status()[0]
    g.set_weights(R_RAND, "direct")
    g.resample(m, "stratified", seed=3)
    check_apply(g, status, lab, None, "after the refusals")
    g.clear_resample()                                                    # no rows: refused, and the plan stays
    refused(-1, g.apply_resample)
    assert g.copy_plan()[0].size == g.n_plan


# ------------------------------------------------------------------------------------------------------------- 7: tracers
def test_the_tracer_amounts_go_with_the_copy_and_the_water_below_stays():
    ncol = 4
    cfg, st = tcs.testcase1(ncol)
    bottom, total, q = tcs.tracers(cfg, st)
    handles = []
    for _ in range(2):
        g = samsim_amd.hip_solver(cfg, ncol)
        g.set_tracers(bottom, total)
        g.set_state(st)
        g.set_tracer_state(q * (1.0 + 0.25 * np.arange(ncol))[None, None, :])
        g.set_tracer_bottom(np.asarray(bottom)[:, None] * (1.0 + 0.5 * np.arange(ncol))[None, :])
        g.set_clock()
        g.step(40)
        handles.append(g)
    a, b = handles
    src, dst = np.array([1, 1], dtype=np.int64), np.array([3, 0], dtype=np.int64)
    qa, ba = a.get_tracer_state()
    assert u64(qa[..., 1]).tobytes() != u64(qa[..., 3]).tobytes() and len({ba[0, c] for c in range(ncol)}) == ncol
    a.copy_columns(src, dst)
    cr.host_route(b, src, dst)
    (q1, b1), (q2, b2) = a.get_tracer_state(), b.get_tracer_state()
    assert u64(q1[..., dst]).tobytes() == u64(qa[..., src]).tobytes() and u64(q1[..., [1, 2]]).tobytes() == u64(qa[..., [1, 2]]).tobytes()
    assert u64(b1).tobytes() == u64(ba).tobytes()                         # the concentration below stays with the slot
    assert u64(q1).tobytes() == u64(q2).tobytes() and u64(b1).tobytes() == u64(b2).tobytes()
    same(state_bytes(a), state_bytes(b), "after the copy")
    for g in (a, b):
        g.step(5)
    (q1, b1), (q2, b2) = a.get_tracer_state(), b.get_tracer_state()
    assert u64(q1).tobytes() == u64(q2).tobytes() and u64(b1).tobytes() == u64(b2).tobytes()
    same(state_bytes(a), state_bytes(b), "five steps later")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------- 8: the closed loop
def tempered(g, status, scale, lo, hi):
    """the GAUSS row of the accumulated misfit tempered -- the scale raised by a quarter at a time, which takes about a fifth off the
    copies -- until a systematic draw of the pool's size leaves between lo and hi copies to make; returns (scale, resample info)"""
    m = int((status == 0).sum())
    for _ in range(300):
        g.set_weights(J_SUM, "gauss", scale)
        info = g.resample(m, "systematic", 0.37)
        copies = m - info["n_survivors"]
        if copies <= hi:
            assert info["m_drawn"] == m and copies >= lo, (scale, copies)
            return scale, info
        scale *= 1.25
    raise AssertionError("no scale leaves so few copies")


def test_the_closed_loop_of_a_particle_filter():
    """set weights, resample, apply, reset the scores, step: no column stops, and the result is the one of a second handle whose
    copies went through the host (get_columns of the plan's sources -- the surplus entries of resampled_columns -- and set_state at
    the same slots).  Beside the background runs of the whole suite an upload of one column through the host took a tenth of a
    second, and the draw at the median's scale makes 1 355 copies: the cycle that is compared is tempered until at most 24 copies
    are left, and the cycle after it, with the median member at exp(-1) and a third of the pool replaced, runs on the first handle
    alone and is checked against the rule and the sources' own bytes."""
    ncol = 4197
    lab = (np.arange(ncol) % 3).astype(np.int32)
    lab[::7] = -1
    (a, status), (b, _) = (scored_ensemble(ncol, (5, 3000), lab, 3, 77) for _ in range(2))
    m = int((status == 0).sum())
    J = a.scores()["J_SUM"]
    median = float(np.median(J[(status == 0) & (J > 0.0)])) / 2.0
    scale, info = tempered(a, status, 64.0 * median, 4, 24)
    b.set_weights(J_SUM, "gauss", scale)
    assert b.resample(m, "systematic", 0.37) == info and m == ncol - 2
    print("closed loop: scale", scale / median, "x the median's, survivors", info["n_survivors"], "largest family", info["max_offspring"])
    r = cr.plan(b.offspring(), status, None, None)
    ainfo = a.apply_resample()
    assert ainfo == r["info"] and ainfo["n_copies"] == m - info["n_survivors"]
    src, dst = a.copy_plan()
    assert np.array_equal(src, r["src"]) and np.array_equal(dst, r["dst"])
    # the plan's sources are the ancestor list without the first entry of every family
    anc = b.ancestors()
    assert np.array_equal(src, anc[1:][anc[1:] == anc[:-1]])
    cr.host_route(b, src, dst)
    for g in (a, b):
        g.reset_scores()
    same(cr.everything(a, True, True), cr.everything(b, True, True), "after the apply")
    for g in (a, b):
        g.step(5)
    ea = cr.everything(a, True, True)
    same(ea, cr.everything(b, True, True), "five steps later")
    assert np.flatnonzero(ea["status"]).tolist() == [5, 3000]
    b.close()
    # the next cycle, a third of the pool replaced: scored again against the same member, weighted, drawn, applied, stepped
    a.score(a.sensor_values([77])[:, 0])
    a.set_weights(J_SUM, "gauss", median)
    info = a.resample(m, "systematic", 0.37)
    assert 100 < info["n_survivors"] < m - 500
    r = cr.plan(a.offspring(), status, None, None)
    want = a.get_columns(r["src"])
    assert a.apply_resample() == r["info"] and r["info"]["n_copies"] == m - info["n_survivors"]
    got = a.get_columns(r["dst"])
    assert got.lay.tobytes() == want.lay.tobytes() and got.scal[:DT2M].tobytes() == want.scal[:DT2M].tobytes()
    assert got.n_active.tobytes() == want.n_active.tobytes()
    a.reset_scores()
    a.step(5)
    assert np.flatnonzero(a.get_status()[0]).tolist() == [5, 3000]
    a.close()
