"""Sensors and the per-column misfit on the GPU (samsim_set_sensors, samsim_get_sensor_values, samsim_score, SAMSIM_SCORE_SLOT): the
model's equivalent of each sensor per column, and the weighted squared differences against an observation vector accumulated in
nine rows that every reduction reads as a slot.  The oracle is the numpy restatement of the header (tests/sensor_reference.py) on
the State that was uploaded or that get_state() returns; values and rows are compared as uint64, bit for bit.

samsim_set_state refuses n_active < 1, so Na == 0 cannot be put on the device: the crafted states let Na run over 1 .. nlayer, and
Na == 0 is covered on the reference alone (tests/test_sensors_host.py)."""
import functools

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi
from samsim_amd.capi import A, NSF, S, SCORE_FIELDS, STAT_DTYPE, FunctionalSpec, SensorSpec, State, TrackSpec, func_slot, score_slot
from tests import hist_reference as hr
from tests import sens_reference as cr
from tests import sensor_reference as sr
from tests.test_gpu_functionals import NCOL, STOPPED, consumers, crafted, crafted_handle, growth_handle, stats_of
from tests.test_gpu_profile_stats import check
from tests.test_gpu_sens import check_cov, check_pairs

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
mk = SensorSpec.make
DEPTHS = [0.1 * i for i in range(16)]        # 0, 0.1, ..., 1.5 m

# all three kinds, both origins, both interpolations; T, S_bu, S_abs, psi_l and ray: five rows, so more than one walk.  The first 16
# are a thermistor string, LINEAR from the top
SENSORS = ([mk("profile", "T", z, interp="linear", missing=-1.0) for z in DEPTHS]
           + [mk("profile", "S_bu", z, "bottom", "linear", missing=NAN) for z in (0.0, 0.3, 0.6, 0.9)]
           + [mk("profile", "S_abs", z, missing=-1.0) for z in (0.1, 0.4, 0.7)]
           + [mk("profile", "S_abs", z, "bottom", "linear", missing=-1.0) for z in (0.2, 0.5)]
           + [mk("profile", "psi_l", z, "bottom", missing=-2.0) for z in (0.0, 0.5, 1.0)]
           + [mk("profile", "ray", 1.5, "bottom", missing=-2.0)]
           + [mk("scalar", "thick_snow"), mk("ice_thickness"), mk("scalar", "T_top")])
assert len(SENSORS) == capi.MAX_SENSORS
NPROFILE = 29
# what a buoy carries: a 16-sensor temperature string from the top, two salinity sections, the ice thickness and the snow depth
BUOY = ([mk("profile", "T", 0.05 * i, interp="linear", missing=NAN) for i in range(16)]
        + [mk("profile", "S_bu", z, "bottom", missing=NAN) for z in (0.02, 0.1)] + [mk("ice_thickness"), mk("scalar", "thick_snow")])


def assert_same(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (what, bad[:8].tolist(), [got[tuple(b)] for b in bad[:8]], [want[tuple(b)] for b in bad[:8]])


def assert_rows(got, want, what):
    assert list(got) == SCORE_FIELDS == list(want)
    for f in SCORE_FIELDS:
        assert_same(got[f], want[f], (what, f))


def with_scalars(st, seed=3):
    """the crafted state with column scalars that differ per column"""
    st.scal[:] = np.random.default_rng(seed).uniform(-2.0, 2.0, st.scal.shape)
    return st


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("ncol", [NCOL, 1, 64])
def test_values_without_a_step(ncol):
    stopped = tuple(c for c in STOPPED if c < ncol)
    st = with_scalars(crafted(ncol))
    g, status = crafted_handle(ncol, st, stopped)
    g.set_sensors(SENSORS)
    rng = np.random.default_rng(5)
    cols = np.concatenate([rng.permutation(ncol), rng.integers(0, ncol, 40)])      # every column, shuffled, with duplicates
    got = g.sensor_values(cols)
    want, in_ice = sr.evaluate_all(SENSORS, st, status, uploaded=True, stepped=False)
    assert_same(got, want[:, cols], "crafted state")
    assert_same(got, sr.evaluate_all(SENSORS, g.get_state(), status, uploaded=True, stepped=False)[0][:, cols], "crafted state, get_state")
    assert_same(g.sensor_values(cols), got, "second evaluation")
    if ncol == NCOL:
        # no branch is silently empty: on the reference, not on the device
        frac = in_ice[:NPROFILE].mean()
        extra = zero = 0
        for spec in SENSORS[:NPROFILE]:
            info = {}
            sr.evaluate(spec, st, status, uploaded=True, stepped=False, info=info)
            extra, zero = extra + int(info["extrapolated"].sum()), zero + int(info["zero_neighbour"].sum())
        print("in the ice", frac, "| extrapolated", extra, "| zero-thickness neighbours", zero)
        assert 0.25 <= frac <= 0.75 and extra >= 100 and zero >= 50
        assert in_ice[NPROFILE:].all() and np.isnan(want).any()
        # a list longer than one piece of the device scratch (4 096 positions), and one column alone
        long = rng.integers(0, ncol, 4096 + 4096 + 37)
        assert_same(g.sensor_values(long), want[:, long], "three pieces")
        assert_same(g.sensor_values([196]), want[:, [196]], "one column")
        # fewer sensors: a smaller tile, one walk
        g.set_sensors(SENSORS[14:18])
        assert_same(g.sensor_values(cols), want[14:18][:, cols], "four sensors")
    g.close()


# ------------------------------------------------------------------------------------------------------------ 2
LABELS = ((np.arange(NCOL, dtype=np.int64) * 7919) % 4).astype(np.int32)
LABELS[::11] = -1


def observations(y, in_ice, ok):
    """three observation vectors near the ensemble's own values: the median over the running columns that have the sensor in the
    ice, shifted; the second with gaps, the third for the group call"""
    med = np.zeros(y.shape[0])
    for i in range(y.shape[0]):
        v = y[i][ok & in_ice[i]]
        v = v[~np.isnan(v)]
        med[i] = np.median(v) if v.size else 0.0
    obs1 = med + 0.125
    obs2 = med - 0.25
    obs2[[1, 5, 17, 30]] = NAN
    obs3 = med * 1.5
    weights = 1.0 / (0.1 + 0.05 * np.arange(y.shape[0])) ** 2
    return obs1, obs2, obs3, weights


def snapshot(g):
    s, (status, step, layer), k, o = g.get_state(), g.get_status(), g.get_clock(), g.get_output()
    return dict(lay=s.lay.tobytes(), scal=s.scal.tobytes(), n_active=s.n_active.tobytes(), status=status.tobytes(),
                err_step=step.tobytes(), err_layer=layer.tobytes(), clock=(k.time, k.step, k.n_time_out, k.time_counter, k.n_outputs),
                work=g.get_work(), out_lay=o.lay.tobytes(), out_scal=o.scal.tobytes(), out_n_active=o.n_active.tobytes(),
                out_when=(o.time, o.step), tracks=[{f: r.tobytes() for f, r in g.tracks(t).items()} for t in range(2)],
                functionals=[g.functionals(i).tobytes() for i in range(2)])


def make_scored(steps=(40,), split=None):
    """the growth wave after 40 steps with three stopped columns, SENSORS in force, scored three times: plain, with gaps and
    weights, and restricted to group 1"""
    g = growth_handle(corrupt=STOPPED, output_in=21)
    if split is not None:
        g.set_launch_split(*split)
    g.set_tracks([TrackSpec.make("ice_thickness"), TrackSpec.make("layer", "S_bu", layer=-1)], 5)
    g.set_functionals([FunctionalSpec.make("integral", "psi_l"), FunctionalSpec.make("mean", "S_bu", z_hi=0.1, missing=-1.0)])
    g.set_sensors(SENSORS)
    g.set_groups(LABELS, ngroups=4)
    for n in steps:
        g.step(n)
    y_dev = g.sensor_values(np.arange(NCOL))          # before any get_state: the clamp and the quotient are the kernel's own
    st, status = g.get_state(), g.get_status()[0]
    assert np.flatnonzero(status).tolist() == list(STOPPED)
    before = snapshot(g)
    ok = status == 0
    y, in_ice = sr.evaluate_all(SENSORS, st, status)
    obs1, obs2, obs3, w = observations(y, in_ice, ok)
    stages = [g.scores()]
    g.score(obs1)
    stages.append(g.scores())
    g.score(obs2, w)
    stages.append(g.scores())
    g.score(obs3, group=1)
    stages.append(g.scores())
    after = snapshot(g)
    for a in (st.lay, st.scal, st.n_active, status, y_dev, y, in_ice, *[r for s in stages for r in s.values()]):
        a.setflags(write=False)
    return dict(g=g, st=st, status=status, y_dev=y_dev, y=y, in_ice=in_ice, obs=(obs1, obs2, obs3, w), stages=stages, before=before,
                after=after)


@functools.lru_cache(maxsize=None)
def scored():
    """make_scored(), computed once and shared: whoever changes the sensors, the rows or the labels puts them back, nobody steps it"""
    return make_scored()


def test_scores_after_steps():
    d = scored()
    st, status, y, in_ice, stages = d["st"], d["status"], d["y"], d["in_ice"], d["stages"]
    obs1, obs2, obs3, w = d["obs"]
    ok = status == 0
    assert_same(d["y_dev"], y, "values after 40 steps")
    assert 0.05 < in_ice[:NPROFILE][:, ok].mean() < 0.95
    want = [sr.zero_rows(NCOL)]
    want.append(sr.score_update(want[-1], y, in_ice, obs1, None, ok))
    want.append(sr.score_update(want[-1], y, in_ice, obs2, w, ok))
    want.append(sr.score_update(want[-1], y, in_ice, obs3, None, ok & (LABELS == 1)))
    for n, (a, b) in enumerate(zip(stages, want)):
        assert_rows(a, b, f"after {n} calls")
    last = stages[3]
    assert (last["CALLS"][ok & (LABELS == 1)] == 3.0).all() and (last["CALLS"][ok & (LABELS != 1)] == 2.0).all()
    assert (last["J_SUM"][ok] > 0.0).all() and len(set(last["J_SUM"][ok].tolist())) > 5
    assert (stages[2]["N_LAST"][ok] < stages[1]["N_LAST"][ok]).any()          # the gaps count
    # stopped columns and columns outside the group: not a byte changes
    for f in SCORE_FIELDS:
        assert (last[f][list(STOPPED)].view(np.uint64) == 0).all(), f
        out = ~(ok & (LABELS == 1))
        assert last[f][out].tobytes() == stages[2][f][out].tobytes(), f
    # the calls wrote nothing to the ensemble
    assert sorted(k for k in d["before"] if d["before"][k] != d["after"][k]) == []
    assert d["after"]["out_when"][1] > 0


# ------------------------------------------------------------------------------------------------------------ 3
def test_twin_experiment():
    d = scored()
    g, st, status, y, in_ice = d["g"], d["st"], d["status"], d["y"], d["in_ice"]
    ok = status == 0
    keep = g.scores()
    m = 77
    assert ok[m]
    try:
        obs = g.sensor_values([m])[:, 0]
        assert_same(obs, y[:, m], "member's values")
        assert not np.isnan(obs[in_ice[:, m]]).any()
        g.score(obs)
        r = g.scores()
        assert r["J_LAST"][m] == 0.0 and r["B_LAST"][m] == 0.0 and r["N_LAST"][m] == in_ice[:, m].sum() > 3
        idx, n = g.select([(score_slot("J_LAST"), -INF, np.finfo(np.float64).tiny)])
        assert m in idx.tolist() and n < ok.sum()
        other = ok & (st.sc("dT2m") != st.sc("dT2m")[m])
        assert other.sum() > 100 and (r["J_LAST"][other] > 0.0).all()
    finally:
        g.set_score_state(keep)
    assert_rows(g.scores(), keep, "put back")


# ------------------------------------------------------------------------------------------------------------ 4
def test_rows_as_slots():
    d = scored()
    g, st, status = d["g"], d["st"], d["status"]
    ok = status == 0
    rows = g.scores()
    names = [score_slot("J_SUM"), score_slot("N_LAST")]
    row_of = {names[0]: rows["J_SUM"], names[1]: rows["N_LAST"]}
    q = g.ensemble_stats(names)
    q = {n: np.array([(x.count, x.mean, x.min, x.max, x.std)], dtype=STAT_DTYPE) for n, x in q.items()}
    check(q, {n: stats_of(row_of[n], ok) for n in names}, "ensemble_stats of score rows", exact_extremes=True)
    assert q[names[0]]["count"][0] == NCOL - 3
    check(g.group_stats(names), {n: np.concatenate([stats_of(row_of[n], ok & (LABELS == k)) for k in range(4)]) for n in names},
          "group_stats of score rows", exact_extremes=True)
    for n, (nv, v0, dv) in ((names[0], (12, 0.0, float(rows["J_SUM"][ok].max()) / 11.0)), (names[1], (capi.MAX_SENSORS, 0.5, 1.0))):
        want = hr.scalar_histogram_reference(row_of[n], status, nv, v0, dv)
        assert np.array_equal(g.histogram(n, nv, v0, dv), want), n
        assert np.array_equal(g.histogram(n, nv, v0, dv, by_group=True),
                              hr.scalar_histogram_reference(row_of[n], status, nv, v0, dv, LABELS, 4)), n
        assert (want > 0).sum() >= 2, (n, want.tolist())
    # the covariance with dT2m: the gradient a calibration follows
    for group in (None, 2):
        cnt = cr.counting(status, LABELS, group)
        got = g.covariance([names[0], "dT2m", names[1]], group=group)
        check_cov(got, cr.covariance_matrix([rows["J_SUM"][cnt], st.sc("dT2m")[cnt], rows["N_LAST"][cnt]]), f"covariance, group {group}")
        assert got[2][0, 1] != 0.0
    # the predictor of a profile regression: the reference reads its predictor from the State, so the row stands in for a scalar
    for n in names:
        st2 = State(st.lay.copy(), st.scal.copy(), st.n_active.copy())
        st2.scal[S["melt_err"]] = row_of[n]
        want = cr.profile_regression_reference(st2, status, ["T", "S_bu"], "melt_err", axis="layer", origin="top", nbins=3)
        check_pairs(g.profile_regression(["T", "S_bu"], n, axis="layer", origin="top", nbins=3), want, f"regression on {n:#x}")
    # selection on the rows
    lo, hi = np.quantile(rows["J_SUM"][ok], [0.25, 0.75])
    inside = (rows["J_SUM"] >= lo) & (rows["J_SUM"] < hi)
    idx, n = g.select([(names[0], float(lo), float(hi))])
    assert np.array_equal(idx, np.nonzero(ok & inside)[0]) and 0 < n < ok.sum()
    idx, n = g.select([(names[0], float(lo), float(hi)), (names[1], 5.0, INF)], group=1, status="any")
    assert np.array_equal(idx, np.nonzero(inside & (rows["N_LAST"] >= 5.0) & (LABELS == 1))[0])
    idx, n = g.select([(score_slot("CALLS"), 0.0, 0.5)], status="stopped")
    assert idx.tolist() == list(STOPPED)


def test_which_slots_are_good():
    g, status = crafted_handle(NCOL)
    g.set_groups(np.zeros(NCOL, dtype=np.int32), ngroups=1)
    every = [score_slot(f) for f in range(NSF)]
    for s in every:
        assert consumers(g, s) == [-1] * 6, hex(s)                 # no sensors set
    g.set_sensors(BUOY)
    for s in every:
        assert consumers(g, s) == [0] * 6, hex(s)
    bad = (score_slot(NSF), score_slot(0) - 1, score_slot(31), func_slot(0), func_slot(8), func_slot(0) - 1, capi.NSCAL, -2)
    for s in bad:
        assert consumers(g, s) == [-1] * 6, hex(s)
    g.set_functionals([FunctionalSpec.make("integral", "T")])
    assert consumers(g, func_slot(0)) == [0] * 6 and consumers(g, func_slot(1)) == [-1] * 6
    g.set_sensors(None)
    for s in every + list(bad[:3]):
        assert consumers(g, s) == [-1] * 6, hex(s)                 # after removal
    assert consumers(g, func_slot(0)) == [0] * 6 and consumers(g, S["thickness"]) == [0] * 6
    g.close()


# ------------------------------------------------------------------------------------------------------------ 5
def test_the_rows_do_not_depend_on_how_the_run_was_cut():
    base = scored()["stages"]
    for kw in (dict(steps=(13, 27)), dict(split=(2, 4))):          # two calls; every step as two concurrent launches
        d = make_scored(**kw)
        for n, (a, b) in enumerate(zip(d["stages"], base)):
            assert_rows(a, b, (kw, n))
        d["g"].close()


def test_a_column_does_not_depend_on_its_wave_mates():
    st = with_scalars(crafted(NCOL))
    places = (3, 64 + 17, 128 + 63, 192 + 4)         # three blocks and the tail
    src = 11                                         # 18 active layers
    for c in places:
        st.lay[:, :, c], st.scal[:, c], st.n_active[c] = st.lay[:, :, src], st.scal[:, src], st.n_active[src]
    assert st.n_active[src] > 10
    g, status = crafted_handle(NCOL, st)
    g.set_sensors(SENSORS)
    y, in_ice = sr.evaluate_all(SENSORS, st, status, uploaded=True, stepped=False)
    obs = y[:, 40] + 0.5
    w = np.linspace(0.5, 2.0, len(SENSORS))
    g.score(obs, w)
    g.score(y[:, 41])
    rows = g.scores()
    assert rows["N_LAST"][src] > 8
    for f, r in rows.items():
        assert len({r[c:c + 1].tobytes() for c in places + (src,)}) == 1, f
    # the same column in another handle, among other columns
    other = with_scalars(crafted(70, seed=9), seed=10)
    other.lay[:, :, 5], other.scal[:, 5], other.n_active[5] = st.lay[:, :, src], st.scal[:, src], st.n_active[src]
    g2, _ = crafted_handle(70, other)
    g2.set_sensors(SENSORS)
    g2.score(obs, w)
    g2.score(y[:, 41])
    for f, r in g2.scores().items():
        assert r[5:6].tobytes() == rows[f][src:src + 1].tobytes(), f
    # and the order of the sensors, hence the plan of the walks, does not change a value
    order = np.random.default_rng(2).permutation(len(SENSORS))
    cols = np.arange(NCOL)
    g.set_sensors([SENSORS[i] for i in order])
    assert_same(g.sensor_values(cols), y[order], "another order")
    g.close()
    g2.close()


# ------------------------------------------------------------------------------------------------------------ 6
def test_arguments():
    ncol = NCOL
    st = with_scalars(crafted(ncol))
    g, status = crafted_handle(ncol, st)
    sets, vals, score = g._f("set_sensors"), g._f("get_sensor_values"), g._f("score")
    gets, puts, reset = g._f("get_scores"), g._f("set_score_state"), g._f("reset_scores")
    cols = np.arange(8, dtype=np.int64)
    buf = np.full((capi.MAX_SENSORS, ncol + 8), -77.0)
    obs4 = np.array([0.5, 1.0, 0.0, 0.25])
    # nothing set yet: every call but the removal is refused
    assert vals(g._h, 8, cols.ctypes.data, buf.ctypes.data) == -1 and score(g._h, obs4.ctypes.data, None, -1) == -1
    assert gets(g._h, 0, 4, buf.ctypes.data) == -1 and puts(g._h, 0, 4, buf.ctypes.data) == -1 and reset(g._h) == -1
    assert (buf == -77.0).all()
    assert sets(g._h, 0, None) == 0
    good = [SENSORS[3], SENSORS[17], SENSORS[29], SENSORS[30]]
    g.set_sensors(good)
    g.score(obs4)
    rows = g.scores()
    y = g.sensor_values(np.arange(ncol))
    assert (rows["CALLS"] == 1.0).all() and (rows["J_SUM"] > 0.0).any()

    def untouched(what):
        assert_rows(g.scores(), rows, what)
        assert_same(g.sensor_values(np.arange(ncol)), y, what)
        assert (buf == -77.0).all(), what

    def refused(n, specs, code):
        arr = None if specs is None else (SensorSpec * max(1, len(specs)))(*specs)
        assert sets(g._h, n, arr) == code, (n, code)
        untouched(("set_sensors", n, code))

    def spec(**kw):
        s = mk("profile", "T", 0.25, "bottom", "linear", -1.0)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    refused(-1, good, -1)
    refused(33, good * 9, -1)
    refused(2, None, -1)
    refused(0, good, -1)
    refused(1, [spec(struct_size=48)], -6)
    refused(1, [spec(struct_size=48, kind=99, reserved=1)], -6)     # the struct size comes first
    refused(2, [spec(), spec(struct_size=0)], -6)
    refused(2, [spec(kind=-1), spec(struct_size=0)], -1)            # spec by spec
    sc, th = capi.SK["scalar"], capi.SK["ice_thickness"]
    for kw in (dict(kind=-1), dict(kind=3), dict(id=-1), dict(id=capi.NARR), dict(kind=sc, id=capi.NSCAL, origin=0, interp=0, z=0.0),
               dict(kind=sc, id=-1, origin=0, interp=0, z=0.0), dict(kind=th, id=1, origin=0, interp=0, z=0.0), dict(origin=2),
               dict(origin=-1), dict(interp=2), dict(interp=-1), dict(kind=sc, id=0, origin=1, interp=0, z=0.0),
               dict(kind=sc, id=0, origin=0, interp=1, z=0.0), dict(kind=sc, id=0, origin=0, interp=0, z=0.5),
               dict(kind=th, id=0, origin=0, interp=0, z=0.5), dict(kind=th, id=0, origin=1, interp=0, z=0.0), dict(z=NAN), dict(z=INF),
               dict(z=-0.1), dict(reserved=1)):
        refused(1, [spec(**kw)], -1)
        refused(2, [spec(), spec(**kw)], -1)
    # samsim_score: obs NULL; a bad weight where there is an observation (and none where there is not); then the group
    w = np.array([1.0, 2.0, 0.5, 4.0])
    assert score(g._h, None, w.ctypes.data, -1) == -1
    for bad in (0.0, -1.0, NAN, INF):
        wb = w.copy()
        wb[2] = bad
        assert score(g._h, obs4.ctypes.data, wb.ctypes.data, -1) == -1, bad
        assert score(g._h, obs4.ctypes.data, wb.ctypes.data, 7) == -1, bad
    for group in (0, -2, 7):                                          # no labels
        assert score(g._h, obs4.ctypes.data, w.ctypes.data, group) == -1, group
    g.set_groups(np.zeros(ncol, dtype=np.int32), ngroups=2)
    for group in (2, -2):
        assert score(g._h, obs4.ctypes.data, None, group) == -1, group
    untouched("score")
    gap = obs4.copy()
    gap[2] = NAN
    wb = w.copy()
    wb[2] = NAN
    assert score(g._h, gap.ctypes.data, wb.ctypes.data, 1) == 0      # nobody carries label 1: accepted, and nothing changes
    untouched("score of an empty group")
    # the list and the windows
    assert vals(g._h, 8, None, buf.ctypes.data) == -1 and vals(g._h, 8, cols.ctypes.data, None) == -1
    for n in (0, -1, capi.SELECT_MAX_OUT + 1):
        assert vals(g._h, n, cols.ctypes.data, buf.ctypes.data) == -1, n
    for badcol in (-1, ncol):
        c = cols.copy()
        c[5] = badcol
        assert vals(g._h, 8, c.ctypes.data, buf.ctypes.data) == -1, badcol
    for f in (gets, puts):
        assert f(g._h, 0, 4, None) == -1
        for args in ((-1, 4), (0, -1), (0, ncol + 1), (ncol, 1), (ncol + 1, 0)):
            assert f(g._h, *args, buf.ctypes.data) == -1, args
    untouched("lists and windows")
    # removal, twice in a row
    for _ in range(2):
        assert sets(g._h, 0, None) == 0
        assert gets(g._h, 0, 4, buf.ctypes.data) == -1 and score(g._h, obs4.ctypes.data, None, -1) == -1 and reset(g._h) == -1
    assert (buf == -77.0).all()
    g.close()


# ------------------------------------------------------------------------------------------------------------ 7
def test_restart():
    d = scored()
    g, y, in_ice, status = d["g"], d["y"], d["in_ice"], d["status"]
    whole = g.scores()
    for col0, n in ((3, 10), (60, 10), (0, 64), (63, 130), (192, 5), (196, 1), (197, 0)):
        part = g.scores(col0, n)
        for f in SCORE_FIELDS:
            assert part[f].tobytes() == whole[f][col0:col0 + n].tobytes(), (f, col0, n)
    # the rows after two calls go into a fresh handle window by window; its third call gives the uninterrupted handle's bytes
    two = d["stages"][2]
    g2 = growth_handle(corrupt=STOPPED, output_in=21)
    g2.step(40)
    g2.set_sensors(SENSORS)
    g2.set_groups(LABELS, ngroups=4)
    for col0, n in ((0, 63), (63, 130), (193, 4)):
        g2.set_score_state({f: r[col0:col0 + n] for f, r in two.items()}, col0)
    assert_rows(g2.scores(), two, "put back")
    g2.score(d["obs"][2], group=1)
    assert_rows(g2.scores(), d["stages"][3], "restarted")
    g2.reset_scores()
    assert_rows(g2.scores(), sr.zero_rows(NCOL), "reset")
    g2.score(d["obs"][0])
    assert_rows(g2.scores(), d["stages"][1], "after a reset")
    g2.close()
    assert_rows(g.scores(), whole, "the shared handle")
