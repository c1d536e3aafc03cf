"""Column functionals on the GPU (samsim_set_functionals, samsim_get_functionals, SAMSIM_FUNC_SLOT): per-column integrals, means,
extrema, crossing depths and conditional thicknesses of the layer profiles, evaluated on the device into rows that every reduction
reads as a slot.  The oracle is the numpy restatement of the header (tests/functional_reference.py) on the State that was uploaded
or that get_state() returns; every row is compared as uint64, bit for bit.

samsim_set_state refuses n_active < 1, so Na == 0 cannot be put on the device: the crafted states let Na run over 1 .. nlayer, and
Na == 0 is covered on the reference alone (tests/test_functionals_host.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bench
import samsim_amd
from samsim_amd import capi
from samsim_amd import testcases as tcs
from samsim_amd.capi import A, FN, STAT_DTYPE, FunctionalSpec, State, TrackSpec, func_slot
from tests import functional_reference as fr
from tests import hist_reference as hr
from tests.helpers import ROOT, golden
from tests.test_gpu_fortran_host import run_host
from tests.test_gpu_profile_stats import check

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "host", "samsim_host.x")
NCOL, NLAYER = 197, 20          # three full blocks and a tail of five columns
NAN, INF = float("nan"), float("inf")
STOPPED = (5, 100, 196)
mk = FunctionalSpec.make

# every kind, both origins, both senses, S_bu and S_abs, a finite window, a window [z, inf), a window entirely below the ice (H < 4 m),
# a NaN `missing`; five distinct arrays, so more than one walk
SPECS8 = [mk("integral", "S_abs"),
          mk("mean", "S_bu", z_lo=0.1, z_hi=0.5, missing=NAN),
          mk("min", "T", "bottom", z_lo=0.2, missing=-1.0),
          mk("max", "psi_l", missing=-1.0),
          mk("depth_of_min", "S_bu", "bottom", z_hi=0.6, missing=NAN),
          mk("depth_of_max", "ray", z_lo=50.0, z_hi=60.0, missing=-7.0),
          mk("crossing_depth", "psi_l", "bottom", z_lo=0.05, sense=-1, threshold=1.0, missing=-1.0),
          mk("thickness_where", "T", z_hi=1.0, sense=1, threshold=1.0)]
# what a user asks of sea ice: the permeable thickness, where the permeable ice begins, the -5 degC isotherm, the salinity of the upper
# 0.1 m, the brine volume, the largest Rayleigh number and where it sits (above the bottom), the coldest layer
SPECS_ICE = [mk("thickness_where", "psi_l", sense=1, threshold=0.05),
             mk("crossing_depth", "psi_l", sense=1, threshold=0.05, missing=-1.0),
             mk("crossing_depth", "T", sense=1, threshold=-5.0, missing=-1.0),
             mk("mean", "S_bu", z_hi=0.1, missing=-1.0),
             mk("integral", "psi_l"),
             mk("max", "ray", missing=-1.0),
             mk("depth_of_max", "ray", "bottom", missing=-1.0),
             mk("min", "S_abs", missing=-1.0)]


def crafted(ncol, nlayer=NLAYER, seed=7):
    """a hand-made state: Na over 1 .. nlayer across the columns, thick with zeros among them, values distinct per (array, layer,
    column), negative S_abs, one layer with m == 0, a few NaNs"""
    rng = np.random.default_rng(seed)
    st = State.empty(ncol, nlayer)
    st.lay[:] = rng.uniform(-1.0, 3.0, st.lay.shape)
    thick = rng.uniform(0.01, 0.2, (nlayer, ncol))
    thick[rng.random((nlayer, ncol)) < 0.1] = 0.0
    st.lay[A["thick"]] = thick
    st.lay[A["m"]] = rng.uniform(0.5, 2.0, (nlayer, ncol))
    st.lay[A["m"], 2 % nlayer, 10 % ncol] = 0.0
    for name, k, c in (("T", 3, 20), ("psi_l", 0, 70), ("S_abs", 1, 130), ("ray", 2, 3), ("S_bu", 0, 64)):
        st.lay[A[name], k % nlayer, c % ncol] = NAN
    st.n_active[:] = 1 + (np.arange(ncol) * 7) % nlayer
    assert ncol < nlayer or set(st.n_active.tolist()) == set(range(1, nlayer + 1))
    return st


def crafted_handle(ncol, st=None, stopped=()):
    cfg, _ = tcs.testcase4(1, nlayer=NLAYER, n_top=5, n_bottom=5)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(crafted(ncol) if st is None else st)
    status = np.zeros(ncol, dtype=np.int32)
    status[list(stopped)] = 99
    if stopped:
        g.set_status(status)
    return g, status


def rows_of(g, n):
    return [g.functionals(i) for i in range(n)]


def assert_rows(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        bad = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))
        assert bad.size == 0, (what, i, bad[:8].tolist(), a[bad[:8]].tolist(), b[bad[:8]].tolist())


def growth_handle(ncol=NCOL, corrupt=(), output_in=None):
    """the 17 columns of the committed growth wave (2 .. 12 active layers of 12) tiled over ncol columns, with the project's
    perturbation of the forcing; not stepped yet.  output_in: the step of the run that is an output point"""
    z = golden("growth_wave_12.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    st = State(bench.tile(np.ascontiguousarray(z["lay"]), ncol), bench.tile(np.ascontiguousarray(z["scal"]), ncol),
               bench.tile(np.ascontiguousarray(z["n_active"]), ncol).astype(np.int32))
    for c in corrupt:
        st.arr("H_abs")[0, c] = -1.0e15              # getT cannot converge: the column stops in its first step
    c75 = golden("sheba_ensemble_80_day75.npz")
    clock = dict(time=float(c75["time"]), step=int(c75["step"]), n_time_out=int(c75["n_time_out"]),
                 time_counter=int(c75["time_counter"]), n_outputs=int(c75["n_outputs"]))
    if output_in is not None:
        clock["n_time_out"] = cfg.i_time_out - output_in + 1
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*bench.sheba_forcing(), *tcs.ensemble_perturbation(ncol))
    g.set_state(st)
    g.set_clock(**clock)
    return g


def make_stepped():
    """the growth wave after 40 steps with SPECS_ICE in force and three stopped columns"""
    g = growth_handle(corrupt=STOPPED)
    g.step(40)
    g.set_functionals(SPECS_ICE)
    rows = rows_of(g, 8)                             # before any get_state: the clamp and the quotient are the kernel's own
    st, status = g.get_state(), g.get_status()[0]
    assert np.flatnonzero(status).tolist() == list(STOPPED)
    for a in (st.lay, st.scal, st.n_active, status, *rows):
        a.setflags(write=False)
    return g, st, status, rows


@functools.lru_cache(maxsize=None)
def stepped():
    """make_stepped(), computed once and shared: whoever changes the functionals or the labels puts them back, nobody steps it"""
    return make_stepped()


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("ncol", [NCOL, 1, 64])
def test_hand_made_state_without_a_step(ncol):
    stopped = tuple(c for c in STOPPED if c < ncol)
    st = crafted(ncol)
    g, status = crafted_handle(ncol, st, stopped)
    g.set_functionals(SPECS8)
    rows = rows_of(g, 8)
    want = fr.evaluate_all(SPECS8, st, status, uploaded=True, stepped=False)
    assert_rows(rows, want, "crafted state")
    assert_rows(rows, fr.evaluate_all(SPECS8, g.get_state(), status, uploaded=True, stepped=False), "crafted state, get_state")
    if ncol == NCOL:
        # the cases the specs are there for do occur
        assert (want[5] == -7.0).all() and np.isnan(want[1]).any() and not np.isnan(want[1]).all()
        assert (want[6] == -1.0).any() and (want[6] >= 0.05).any() and (want[7] > 0.0).any() and (want[7] == 0.0).any()
        assert np.isnan(want[0]).any() and len(set(want[3].tolist())) > 100
        # windows inside a block and across blocks are slices of the whole row
        for i in (0, 4):
            for col0, n in ((3, 10), (60, 10), (0, 64), (63, 130), (192, 5), (196, 1), (197, 0)):
                assert g.functionals(i, col0, n).tobytes() == rows[i][col0:col0 + n].tobytes(), (i, col0, n)
    g.close()


# ------------------------------------------------------------------------------------------------------------ 2
def test_after_steps_the_rows_follow_the_state():
    g, st, status, rows = make_stepped()
    assert_rows(rows, fr.evaluate_all(SPECS_ICE, st, status), "after 40 steps")
    ok = status == 0
    assert (rows[0][ok] > 0.0).all() and len(set(rows[0][ok].tolist())) > 5        # the permeable thickness is there and differs
    # lazy refresh: steps without any call in between, then a read
    g.step(3)
    rows3 = rows_of(g, 8)
    s1 = g.get_state()
    assert_rows(rows3, fr.evaluate_all(SPECS_ICE, s1, status), "after 43 steps")
    assert any(a.tobytes() != b.tobytes() for a, b in zip(rows, rows3))
    # an evaluation writes nothing to the ensemble
    g.set_functionals(SPECS_ICE)
    again = rows_of(g, 8)
    s2 = g.get_state()
    assert_rows(again, rows3, "second evaluation")
    assert s1.lay.tobytes() == s2.lay.tobytes() and s1.scal.tobytes() == s2.scal.tobytes() and s1.n_active.tobytes() == s2.n_active.tobytes()
    # set_state of other columns, across a block boundary, then a read: in an uploaded column of a handle that has stepped the
    # quotient S_abs / m is formed, the clamp is not
    w = crafted(10, nlayer=g.nlayer, seed=11)
    g.set_state(w, 60)
    up = np.zeros(g.ncol, dtype=bool)
    up[60:70] = True
    rows_up = rows_of(g, 8)
    full = State(s2.lay.copy(), s2.scal.copy(), s2.n_active.copy())
    full.lay[:, :, 60:70], full.n_active[60:70] = w.lay, w.n_active
    assert_rows(rows_up, fr.evaluate_all(SPECS_ICE, full, status, uploaded=up), "after set_state, from the upload")
    assert_rows(rows_up, fr.evaluate_all(SPECS_ICE, g.get_state(), status, uploaded=up), "after set_state, from get_state")
    assert rows_up[7][60:70].min() < 0.0             # min S_abs: not clamped there
    g.close()


# ------------------------------------------------------------------------------------------------------------ 3
def stats_of(row, ok):
    out = np.zeros(1, dtype=STAT_DTYPE)
    v = row[ok]
    out[0] = (v.size, v.mean(), v.min(), v.max(), v.std()) if v.size else (0, 0.0, 0.0, 0.0, 0.0)
    return out


def test_rows_as_slots():
    g, st, status, rows = stepped()
    ok = status == 0
    ncol = g.ncol
    labels = ((np.arange(ncol, dtype=np.int64) * 7919) % 4).astype(np.int32)
    labels[::11] = -1
    g.set_groups(labels, ngroups=4)
    names = [func_slot(i) for i in (0, 2, 3, 5)]
    row_of = {func_slot(i): rows[i] for i in range(8)}
    q = g.ensemble_stats(names)
    q = {n: np.array([(x.count, x.mean, x.min, x.max, x.std)], dtype=STAT_DTYPE) for n, x in q.items()}
    check(q, {n: stats_of(row_of[n], ok) for n in names}, "ensemble_stats of functional rows", exact_extremes=True)
    assert q[names[0]]["count"][0] == ncol - 3
    qg = g.group_stats(names)
    check(qg, {n: np.concatenate([stats_of(row_of[n], ok & (labels == k)) for k in range(4)]) for n in names},
          "group_stats of functional rows", exact_extremes=True)
    # histograms: the isotherm depth with missing = -1 and v0 = 0 (entry 0: the columns without one), and the permeable thickness
    for i, (nv, v0, dv) in ((2, (12, 0.0, 0.02)), (0, (10, 0.0, float(rows[0][ok].max()) / 9.0))):
        want = hr.scalar_histogram_reference(rows[i], status, nv, v0, dv)
        assert np.array_equal(g.histogram(func_slot(i), nv, v0, dv), want), i
        assert np.array_equal(g.histogram(func_slot(i), nv, v0, dv, by_group=True),
                              hr.scalar_histogram_reference(rows[i], status, nv, v0, dv, labels, 4)), i
        assert i == 2 or (want > 0).sum() >= 2, (i, want.tolist())
    # selection on a slot, every status mode reading the row
    lo, hi = np.quantile(rows[0][ok], [0.25, 0.75])
    term = (func_slot(0), float(lo), float(hi))
    inside = (rows[0] >= lo) & (rows[0] < hi)
    idx, n = g.select([term])
    assert np.array_equal(idx, np.nonzero(ok & inside)[0]) and 0 < n < ok.sum()
    idx, n = g.select([term], status="any")
    assert np.array_equal(idx, np.nonzero(inside)[0])
    idx, n = g.select([(func_slot(4), -INF, INF)], status="stopped")
    assert idx.tolist() == list(STOPPED)
    idx, n = g.select([term, (func_slot(2), 0.0, INF)], group=1)
    assert np.array_equal(idx, np.nonzero(ok & inside & (rows[2] >= 0.0) & (labels == 1))[0])
    # covariance with the slot listed twice: identical rows and columns
    count, mean, cov = g.covariance([func_slot(0), func_slot(0), "dT2m", func_slot(4)])
    assert count == ncol - 3 and mean[0].tobytes() == mean[1].tobytes()
    assert cov[0].tobytes() == cov[1].tobytes() and cov[:, 0].tobytes() == cov[:, 1].tobytes() and cov[0, 0] > 0.0
    assert abs(mean[0] - rows[0][ok].mean()) <= 1e-12 * max(1.0, abs(rows[0][ok].mean()))
    want_cov = np.mean((rows[0][ok] - rows[0][ok].mean()) * (rows[4][ok] - rows[4][ok].mean()))
    assert abs(cov[0, 3] - want_cov) <= 1e-10 * max(1e-3, abs(want_cov))
    # the predictor of a profile regression
    reg = g.profile_regression(["T"], func_slot(0), axis="layer", origin="top", nbins=2)["T"]
    assert reg["count"][0] == ncol - 3 and abs(reg["mean_x"][0] - rows[0][ok].mean()) <= 1e-12 * max(1.0, abs(rows[0][ok].mean()))
    g.set_groups(None)


# ------------------------------------------------------------------------------------------------------------ 4
def test_old_against_new():
    """MEAN of T from the top over [0, 0.5) is the one-bin depth profile of samsim_get_profile_stats: same overlaps, same sums, same
    division"""
    g, st, status, _ = stepped()
    g.set_functionals([mk("mean", "T", z_hi=0.5, missing=NAN)])
    try:
        q = g.ensemble_stats([func_slot(0)])[func_slot(0)]
        p = g.profile_stats(["T"], axis="depth", origin="top", nbins=1, z0=0.0, dz=0.5)["T"][0]
        assert q.count == p["count"] == g.ncol - 3
        assert np.float64(q.min).tobytes() == p["min"].tobytes() and np.float64(q.max).tobytes() == p["max"].tobytes()
        assert q.min < q.max
        nv, v0 = 16, float(q.min)
        dv = (float(q.max) - v0) / 15.0
        h = g.histogram(func_slot(0), nv, v0, dv)
        assert np.array_equal(h, g.profile_histogram("T", nv, v0, dv, axis="depth", origin="top", nbins=1, z0=0.0, dz=0.5)[0])
        assert h.sum() == q.count and (h > 0).sum() >= 3
    finally:
        g.set_functionals(SPECS_ICE)


# ------------------------------------------------------------------------------------------------------------ 5
def test_a_column_does_not_depend_on_its_wave_mates():
    st = crafted(NCOL)
    places = (3, 64 + 17, 128 + 63, 192 + 4)         # three blocks and the tail
    src = 11                                         # 18 active layers
    for c in places:
        st.lay[:, :, c], st.scal[:, c], st.n_active[c] = st.lay[:, :, src], st.scal[:, src], st.n_active[src]
    assert st.n_active[places[0]] > 10
    g, status = crafted_handle(NCOL, st)
    g.set_functionals(SPECS8)
    rows = rows_of(g, 8)
    for i, r in enumerate(rows):
        assert len({r[c:c + 1].tobytes() for c in places}) == 1, i
    g.set_functionals(SPECS8)
    assert_rows(rows_of(g, 8), rows, "second evaluation")
    # and the order of the functionals, hence the plan of the walks, does not change a value
    order = [7, 3, 1, 5, 0, 6, 2, 4]
    g.set_functionals([SPECS8[i] for i in order])
    assert_rows(rows_of(g, 8), [rows[i] for i in order], "another order")
    g.close()
    # a list on which the packing matters, on the stepped growth wave: three one-row functionals, then S_bu (S_abs and m: a second
    # walk), then a fifth array, which joins the first walk by first-fit and would join the second by next-fit
    g, st, status, _ = stepped()
    specs = [mk("integral", "T"), mk("max", "psi_l", missing=-1.0), mk("depth_of_max", "ray", "bottom", missing=-1.0),
             mk("mean", "S_bu", z_hi=0.1, missing=-1.0), mk("min", "H_abs", missing=-1.0)]
    g.set_functionals(specs)
    try:
        assert_rows(rows_of(g, 5), fr.evaluate_all(specs, st, status), "first-fit")
    finally:
        g.set_functionals(SPECS_ICE)


# ------------------------------------------------------------------------------------------------------------ 6
def consumers(g, slot):
    """the return code of each of the six consumers of a slot"""
    def code(call):
        try:
            call()
            return 0
        except samsim_amd.SamsimError as e:
            return e.code
    return [code(lambda: g.ensemble_stats([slot])), code(lambda: g.group_stats([slot])), code(lambda: g.histogram(slot, 4, 0.0, 1.0)),
            code(lambda: g.covariance([slot])), code(lambda: g.profile_regression(["T"], slot)), code(lambda: g.select([(slot, 0.0, 1.0)]))]


def test_refusals():
    g, status = crafted_handle(NCOL)
    g.set_groups(np.zeros(NCOL, dtype=np.int32), ngroups=1)
    assert consumers(g, func_slot(0)) == [-1] * 6                    # none set
    good = [SPECS8[0], SPECS8[6]]
    g.set_functionals(good)
    rows = rows_of(g, 2)
    assert consumers(g, func_slot(0)) == [0] * 6 and consumers(g, func_slot(1)) == [0] * 6
    for bad in (func_slot(2), func_slot(8), func_slot(0) - 1):
        assert consumers(g, bad) == [-1] * 6, bad
    setf = g._f("set_functionals")

    def refused(n, specs, code):
        arr = None if specs is None else (FunctionalSpec * max(1, len(specs)))(*specs)
        assert setf(g._h, n, arr) == code, (n, code)
        assert_rows(rows_of(g, 2), rows, "after a refused call")     # the previous functionals are in force

    def spec(**kw):
        s = mk("crossing_depth", "T", sense=1, threshold=0.5, missing=-1.0)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    refused(-1, good, -1)
    refused(9, good * 5, -1)
    refused(2, None, -1)
    refused(0, good, -1)
    refused(1, [spec(struct_size=48)], -6)
    refused(1, [spec(struct_size=48, kind=99, reserved=1)], -6)      # the struct size comes first
    refused(2, [spec(), spec(struct_size=0)], -6)
    refused(2, [spec(kind=-1), spec(struct_size=0)], -1)             # spec by spec
    for kw in (dict(kind=-1), dict(kind=len(FN)), dict(array=-1), dict(array=capi.NARR), dict(origin=2), dict(origin=-1),
               dict(sense=0), dict(sense=2), dict(kind=FN["thickness_where"], sense=0), dict(kind=FN["integral"], sense=1),
               dict(kind=FN["min"], sense=-1), dict(threshold=NAN), dict(threshold=INF), dict(z_lo=NAN), dict(z_lo=INF),
               dict(z_lo=-0.1), dict(z_hi=NAN), dict(z_lo=0.5, z_hi=0.5), dict(z_lo=0.5, z_hi=0.25), dict(z_hi=-INF), dict(reserved=1)):
        refused(1, [spec(**kw)], -1)
        refused(2, [spec(), spec(**kw)], -1)
    # a threshold that is not finite is fine where there is no condition
    g.set_functionals([mk("min", "T", threshold=NAN)] + good)
    assert_rows(rows_of(g, 3)[1:], rows, "shifted by one")
    g.set_functionals(good)
    # samsim_get_functionals
    getf = g._f("get_functionals")
    out = np.full(NCOL + 8, -77.0)
    for args in ((-1, 0, 4), (2, 0, 4), (0, -1, 4), (0, 0, -1), (0, 0, NCOL + 1), (0, NCOL, 1), (0, NCOL + 1, 0)):
        assert getf(g._h, *args, out.ctypes.data) == -1, args
    assert getf(g._h, 0, 0, 4, None) == -1
    assert (out == -77.0).all()
    assert getf(g._h, 1, 190, 7, out.ctypes.data) == 0 and out[:7].tobytes() == rows[1][190:].tobytes() and (out[7:] == -77.0).all()
    # removal, twice in a row; then the slot is bad again
    for _ in range(2):
        assert setf(g._h, 0, None) == 0
        assert consumers(g, func_slot(0)) == [-1] * 6
        assert getf(g._h, 0, 0, 4, out.ctypes.data) == -1
    assert consumers(g, capi.S["thickness"]) == [0] * 6
    g.close()


# ------------------------------------------------------------------------------------------------------------ 7
def test_the_run_is_untouched():
    """with functionals set, read in the middle of the run and through a slot, a 40-step run leaves state, status, clock, work
    counters, output snapshot and track rows as they are without them"""
    def run(with_functionals):
        g = growth_handle(corrupt=(STOPPED[0],), output_in=21)
        g.set_tracks([TrackSpec.make("ice_thickness"), TrackSpec.make("layer", "S_bu", layer=-1)], 5)
        if with_functionals:
            g.set_functionals(SPECS_ICE)
        g.step(17)
        if with_functionals:
            g.functionals(3)
        g.step(23)
        if with_functionals:
            g.ensemble_stats([func_slot(0)])
        s, (status, step, layer), k, o = g.get_state(), g.get_status(), g.get_clock(), g.get_output()
        got = dict(lay=s.lay.tobytes(), scal=s.scal.tobytes(), n_active=s.n_active.tobytes(), status=status.tobytes(),
                   err_step=step.tobytes(), err_layer=layer.tobytes(), clock=(k.time, k.step, k.n_time_out, k.time_counter, k.n_outputs),
                   work=g.get_work(), out_lay=o.lay.tobytes(), out_scal=o.scal.tobytes(), out_n_active=o.n_active.tobytes(),
                   out_when=(o.time, o.step),
                   tracks=[{f: r.tobytes() for f, r in g.tracks(t).items()} for t in range(2)])
        g.close()
        return got
    a, b = run(True), run(False)
    assert sorted(k for k in a if a[k] != b[k]) == []
    assert a["out_when"][1] > 0


# ------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran host not built (no flang)")
def test_fortran_host_permeable_file(tmp_path):
    """permeable_psi_l in &samsim_run: one row of dat_ens_permeable.dat per output point -- the time, then count, mean, min, max, std
    of the permeable thickness and of the depth at which the permeable ice begins --, printed with 17 digits; count, min and max are
    those of the Python path at the same output points (two of them: steps 1 and 3602)"""
    ncol = 64
    cfg, st = tcs.testcase1(ncol)
    total = 1 + cfg.i_time_out + 1
    run_host(tmp_path, f"&samsim_run testcase=1, ncol={ncol}, max_steps={total}, permeable_psi_l=0.05 /\n")
    f = np.loadtxt(tmp_path / "output" / "dat_ens_permeable.dat", ndmin=2)
    assert f.shape == (2, 11)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    g.set_functionals([mk("thickness_where", "psi_l", sense=1, threshold=0.05, missing=0.0),
                       mk("crossing_depth", "psi_l", sense=1, threshold=0.05, missing=-1.0)])
    for row in f:
        g.step(g.steps_to_output())
        q = g.ensemble_stats([func_slot(0), func_slot(1)])
        for j in range(2):
            x = q[func_slot(j)]
            print(row[0], j, x.count, x.mean, x.min, x.max, x.std, row[1 + 5 * j:6 + 5 * j].tolist())
            assert row[1 + 5 * j] == x.count == ncol and row[3 + 5 * j] == x.min and row[4 + 5 * j] == x.max, (row.tolist(), j)
    assert g.get_clock().step == total and f[1, 1 + 2] > 0.0
    g.close()
