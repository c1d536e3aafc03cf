"""Time-domain diagnostics on the GPU (samsim_set_tracks, samsim_get_tracks, SAMSIM_TRACK_SLOT): per-column tracks sampled on the
device between launches.  The reference is always the numpy restatement of the header's update rule (tests/track_reference.py)
applied to get_state() and get_status() of a handle that is stepped by hand to each sample point; the tracked handle is a second
handle with the same inputs.  Every field is compared byte for byte: the header promises a fixed sequence of IEEE operations on the
column's own data.  The waves are the committed melt-onset waves (70 columns: one full block and one of 6, 24 steps);
tests/test_tracks_host.py pins, on the CPU oracle, that the conditions used here come to hold in them."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi, testcases as tcs
from samsim_amd.capi import A, NSCAL, NTF, S, STAT_DTYPE, TRACK_FIELDS, TRACK_INITIAL, ProfileRequest, TrackSpec, track_slot
from tests import hist_reference as hr
from tests import melt_onset_seeds as mo
from tests import sens_reference as sr
from tests import track_reference as tr
from tests.helpers import golden, ROOT
from tests.test_gpu_melt_onset import assert_same_bits
from tests.test_gpu_profile_stats import check, close, ensemble
from tests.test_gpu_sens import check_against_statistics, check_cov

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "host", "samsim_host.x")
NCOL, NSTEPS = mo.NCOL, mo.NSTEPS

# every kind of observable, both senses of a condition and none, a layer from the top and one from the bottom
SPECS8 = [TrackSpec.make("scalar", "T_top", sense=+1, threshold=0.0), TrackSpec.make("scalar", "T_snow", sense=-1, threshold=-0.5),
          TrackSpec.make("scalar", "thick_snow"), TrackSpec.make("n_active"), TrackSpec.make("ice_thickness"),
          TrackSpec.make("bulk_salinity"), TrackSpec.make("layer", "T", layer=1), TrackSpec.make("layer", "S_bu", layer=-1)]


@functools.lru_cache(maxsize=None)
def wave(which):
    cfg, st, clock, dT, ps, _ = mo.load_wave(which)
    for a in (st.lay, st.scal, st.n_active, dT, ps):
        a.setflags(write=False)
    return cfg, st, clock, dT, ps


def handle(which, split=False, corrupt=None, n_time_out=None):
    cfg, st, clock, dT, ps = wave(which)
    clock = clock if n_time_out is None else dict(clock, n_time_out=n_time_out)
    if corrupt is not None:
        st = st.copy()
        st.arr("H_abs")[0, corrupt] = -1.0e15                # the column stops in its first step, as ensemble(..., corrupt=) does it
    g = samsim_amd.hip_solver(cfg, st.ncol)
    mo.prepare(g, cfg, st, clock, dT, ps)
    if split:
        g.set_launch_split(1, 4)                             # two blocks, one on each stream
    return g


def by_hand(g, nsteps, after=None):
    """[(clock.step, get_state(), status), ...] after each of nsteps single steps; after(g, i) runs once step i (1-based) has been
    recorded"""
    samples = []
    for i in range(1, nsteps + 1):
        g.step(1)
        samples.append((int(g.get_clock().step), g.get_state(), g.get_status()[0]))
        if after:
            after(g, i)
    return samples


@functools.lru_cache(maxsize=None)
def trajectory(which):
    """the reference's samples of a wave: computed once, shared, never modified"""
    g = handle(which)
    samples = by_hand(g, NSTEPS)
    g.close()
    assert [s for s, _, _ in samples] == list(range(wave(which)[2]["step"] + 1, wave(which)[2]["step"] + NSTEPS + 1))
    return samples


def all_tracks(g, n):
    return [g.tracks(t) for t in range(n)]


def everything(g):
    """what tracking must not change: the state, the status, the clock, the work counters and the output snapshot, as bytes"""
    s, (status, step, layer), k, o = g.get_state(), g.get_status(), g.get_clock(), g.get_output()
    return dict(lay=s.lay.tobytes(), scal=s.scal.tobytes(), n_active=s.n_active.tobytes(), status=status.tobytes(),
                err_step=step.tobytes(), err_layer=layer.tobytes(), clock=(k.time, k.step, k.n_time_out, k.time_counter, k.n_outputs),
                work=g.get_work(), out_lay=o.lay.tobytes(), out_scal=o.scal.tobytes(), out_n_active=o.n_active.tobytes(),
                out_when=(o.time, o.step)), s


@functools.lru_cache(maxsize=None)
def run_of_test_1():
    g = handle("spread")
    g.set_tracks(SPECS8, 1)
    g.step(NSTEPS)
    rows = all_tracks(g, 8)
    g.close()
    return rows


def test_every_step_every_kind():
    rows = run_of_test_1()
    samples = trajectory("spread")
    want = tr.apply(SPECS8, samples)
    step0 = samples[0][0] - 1
    # the reference is not idle: the condition comes to hold at many different steps, extremes move, every track was sampled 24 times
    assert len(set(want[0]["STEP_FIRST"].tolist())) >= 12 and (want[0]["STEP_FIRST"] > step0 + 1).all()
    assert all((w["N"] == NSTEPS).all() for w in want) and (want[0]["MIN"] < want[0]["MAX"]).all() and (want[6]["M2"] > 0.0).any()
    assert len(set(want[7]["LAST"].tolist())) >= 10
    assert tr.same_bytes(rows, want) == []


@pytest.mark.parametrize("every", [3, 5, 7])
def test_cadence_and_cuts(every):
    """3 and 5, and 7: the wave's clock is a multiple of 3, of neither 5 nor 7, and 24 is a multiple of neither 5 nor 7 (phase and
    tail); one launch of 24, 24 launches of 1 and launches of 7, each with the default launch and with the two blocks on two streams"""
    samples = trajectory("spread")
    due = [x for x in samples if x[0] % every == 0]
    assert 3 <= len(due) <= 8 and (every == 3 or (samples[0][0] % every != 1 and samples[-1][0] % every != 0))
    want = tr.apply(SPECS8, due)
    got = {}
    for plan, cuts in (("24", [24]), ("1", [1] * 24), ("7", [7, 7, 7, 3])):
        for split in (False, True):
            g = handle("spread", split)
            g.set_tracks(SPECS8, every)
            for n in cuts:
                g.step(n)
            got[plan, split] = all_tracks(g, 8)
            g.close()
    for key, rows in got.items():
        assert tr.same_bytes(rows, got["24", False]) == [], key
    assert (want[0]["N"] == len(due)).all()
    assert tr.same_bytes(got["24", False], want) == []


def test_the_run_is_untouched():
    """the run of test 1 -- with the wave's clock moved so that its tenth step is an output point and there is a snapshot to compare
    -- against handles that never had tracks: one cut where the tracked run is cut (every step), byte for byte in everything a
    handle returns; and one launch of 24, in the measure of the launch-cut tests"""
    nto = wave("spread")[0].i_time_out - 9
    g = handle("spread", n_time_out=nto)
    assert g.steps_to_output() == 10
    g.set_tracks(SPECS8, 1)
    g.step(NSTEPS)
    assert (g.tracks(0)["N"] == NSTEPS).all()
    tracked, state = everything(g)
    g.close()
    assert tracked["out_when"][1] == wave("spread")[2]["step"] + 10
    g = handle("spread", n_time_out=nto)
    for _ in range(NSTEPS):
        g.step(1)
    plain, _ = everything(g)
    g.close()
    assert sorted(k for k in tracked if tracked[k] != plain[k]) == []
    g = handle("spread", n_time_out=nto)
    g.step(NSTEPS)
    one, state1 = everything(g)
    g.close()
    assert_same_bits(state, state1, "tracked run against one launch of 24 without tracks")
    for k in ("scal", "n_active", "status", "err_step", "err_layer", "clock", "work", "out_when", "out_n_active"):
        assert tracked[k] == one[k], k


def test_stopped_columns():
    dead, frozen, half = 3, 67, NSTEPS // 2
    specs = SPECS8[:1] + SPECS8[4:]

    def freeze(g, i):
        if i == half:
            status, step, layer = g.get_status()
            assert status[frozen] == 0
            status[frozen], step[frozen], layer[frozen] = 99, g.get_clock().step, 1
            g.set_status(status, step, layer)
    ref = handle("spread", corrupt=dead)
    samples = by_hand(ref, NSTEPS, after=freeze)
    ref.close()
    # (the corrupted column stops in the first step -- in this wave with 431, the energy balance, ahead of getT's 99)
    assert samples[0][2][dead] != 0 and np.flatnonzero(samples[-1][2]).tolist() == [dead, frozen]
    want, at_half = tr.apply(specs, samples), tr.apply(specs, samples[:half])
    g = handle("spread", corrupt=dead)
    g.set_tracks(specs, 1)
    g.step(half)
    freeze(g, half)
    g.step(NSTEPS - half)
    rows = all_tracks(g, len(specs))
    g.close()
    for r, h in zip(rows, at_half):
        for f in TRACK_FIELDS:
            assert r[f][dead] == TRACK_INITIAL[f], f                       # stopped in the first step: never sampled
            assert r[f][frozen].tobytes() == h[f][frozen].tobytes(), f     # frozen after 12 steps: the step-12 values
        assert r["N"][frozen] == half and r["N"][dead] == 0
        assert (np.delete(r["N"], [dead, frozen]) == NSTEPS).all()
    assert tr.same_bytes(rows, want) == []


def test_ice_that_melts():
    samples = trajectory("melt")
    thickness = TrackSpec.make("ice_thickness")
    H0 = float(np.median(tr.observable(thickness, samples[NSTEPS // 2 - 1][1])[0]))
    specs = [TrackSpec.make("ice_thickness", sense=-1, threshold=H0), TrackSpec.make("bulk_salinity"),
             TrackSpec.make("scalar", "T_top", sense=+1, threshold=0.0)]
    want = tr.apply(specs, samples)
    below, moves = int((want[0]["STEP_FIRST"] >= 0).sum()), int((want[0]["MIN"] != want[0]["MAX"]).sum())
    print("thickness below the median of step 12 in", below, "columns; thickness moves in", moves, "; T_top >= 0 in",
          int((want[2]["N_HOLD"] > 0).sum()))
    assert 1 <= below <= NCOL - 1 and 1 <= moves <= NCOL - 1
    g = handle("melt")
    g.set_tracks(specs, 1)
    g.step(NSTEPS)
    rows = all_tracks(g, 3)
    g.close()
    for f in ("MIN", "STEP_MIN", "MAX", "STEP_MAX", "N_HOLD", "STEP_FIRST", "STEP_LAST"):
        for t in range(3):
            assert rows[t][f].tobytes() == want[t][f].tobytes(), (t, f)
    assert tr.same_bytes(rows, want) == []


def stats_of(row, ok):
    out = np.zeros(1, dtype=STAT_DTYPE)
    v = row[ok]
    out[0] = (v.size, v.mean(), v.min(), v.max(), v.std())
    return out


def test_many_blocks_ragged_tail_and_slots():
    """8 261 columns: 129 blocks and 5 columns, both parts of a split launch with many blocks; then the track rows as slots of
    the five reductions, each against numpy on the rows samsim_get_tracks returns"""
    ncol, every, nsteps, corrupt = 8261, 2, 6, (5, 4000, 8260)
    assert ncol == 129 * 64 + 5
    labels = ((np.arange(ncol, dtype=np.int64) * 7919) % 9).astype(np.int32)
    labels[::11] = -1
    ref = ensemble("sheba_ensemble_80.npz", ncol, 0, corrupt=corrupt)
    samples = by_hand(ref, nsteps)
    ref.close()
    status = samples[-1][2]
    assert np.flatnonzero(status).tolist() == list(corrupt) and np.flatnonzero(samples[0][2]).tolist() == list(corrupt)
    ok = status == 0
    median = float(np.median(samples[-1][1].sc("T_top")[ok]))
    specs = [TrackSpec.make("ice_thickness"), TrackSpec.make("bulk_salinity"), TrackSpec.make("scalar", "T_top", sense=+1, threshold=median)]
    due = [x for x in samples if x[0] % every == 0]
    assert len(due) == 3
    want = tr.apply(specs, due)
    g = ensemble("sheba_ensemble_80.npz", ncol, 0, corrupt=corrupt)
    g.set_launch_split(1, 4)
    g.set_groups(labels, ngroups=9)
    g.set_tracks(specs, every)
    g.step(nsteps)
    rows = all_tracks(g, 3)
    assert tr.same_bytes(rows, want) == []
    assert np.array_equal(g.get_status()[0], status)
    hold = want[2]["N_HOLD"]
    assert len(set(hold[ok].tolist())) >= 2 and (want[0]["N"][ok] == 3).all() and (want[0]["N"][~ok] == 0).all()
    # ---- the rows as slots
    slots = {(t, f): track_slot(t, f) for t in range(3) for f in ("LAST", "MEAN", "N_HOLD")}
    names = [slots[0, "LAST"], slots[0, "MEAN"], slots[1, "LAST"], slots[1, "MEAN"], slots[2, "LAST"], slots[2, "MEAN"]]
    row_of = {slots[t, f]: want[t][f] for (t, f) in slots}
    q = g.ensemble_stats(names)
    q = {n: np.array([(x.count, x.mean, x.min, x.max, x.std)], dtype=STAT_DTYPE) for n, x in q.items()}
    check(q, {n: stats_of(row_of[n], ok) for n in names}, "ensemble_stats of track rows", exact_extremes=True)
    assert q[names[0]]["count"][0] == ncol - 3 and q[names[0]]["mean"][0] > 0.1 and q[names[0]]["mean"][0] != q[names[2]]["mean"][0]
    qg = g.group_stats(names)
    rg = {n: np.concatenate([stats_of(row_of[n], ok & (labels == k)) for k in range(9)]) for n in names}
    check(qg, rg, "group_stats of track rows", exact_extremes=True)
    # histogram of N_HOLD: integer counts, exactly numpy's
    nv, v0, dv = 4, -0.5, 1.0
    assert np.array_equal(g.histogram(slots[2, "N_HOLD"], nv, v0, dv), hr.scalar_histogram_reference(hold, status, nv, v0, dv))
    assert np.array_equal(g.histogram(slots[2, "N_HOLD"], nv, v0, dv, by_group=True),
                          hr.scalar_histogram_reference(hold, status, nv, v0, dv, labels, 9))
    assert (hr.scalar_histogram_reference(hold, status, nv, v0, dv) > 0).sum() >= 2
    # covariance of the perturbations with two track rows
    state = samples[-1][1]
    cov_names = ["dT2m", "precip_scale", slots[0, "LAST"], slots[2, "N_HOLD"]]
    cov_rows = [state.sc("dT2m")[ok], state.sc("precip_scale")[ok], want[0]["LAST"][ok], hold[ok]]
    check_cov(g.covariance(cov_names), sr.covariance_matrix(cov_rows), "covariance with track rows")
    check_cov(g.covariance(cov_names, group=4), sr.covariance_matrix([r[labels[ok] == 4] for r in cov_rows]), "covariance with track rows, group 4")
    # regression of today's temperature profile on the current thickness: y is folded as the statistics fold it
    reg = g.profile_regression(["T"], slots[0, "LAST"], axis="layer", origin="top")
    check_against_statistics(reg, g.profile_stats(["T"], axis="layer", origin="top"), "profile_regression on a track row")
    full = reg["T"]["count"] == ncol - 3
    assert full.any() and close(reg["T"]["mean_x"][full], float(np.asarray(want[0]["LAST"][ok], dtype=np.longdouble).mean()), 1e-12).all()
    g.close()


def test_columns_of_different_depth():
    """in the waves every column holds all 80 layers; here 19 to 22 of them are active: the walk ends at different layers in the
    lanes of a wave, a layer counted from the bottom lies in different rows, and a layer that some columns lack is not sampled there"""
    ncol, nsteps = 300, 4
    specs = [TrackSpec.make("ice_thickness"), TrackSpec.make("bulk_salinity"), TrackSpec.make("layer", "T", layer=-1),
             TrackSpec.make("layer", "S_bu", layer=-3), TrackSpec.make("layer", "T", layer=21, sense=-1, threshold=-1.0),
             TrackSpec.make("layer", "psi_l", layer=-22), TrackSpec.make("layer", "S_abs", layer=1), TrackSpec.make("n_active")]
    ref = ensemble("sheba_ensemble_80_day75.npz", ncol, 0)
    samples = by_hand(ref, nsteps)
    ref.close()
    assert not samples[-1][2].any()
    want = tr.apply(specs, samples)
    na = samples[-1][1].n_active
    assert len(set(na.tolist())) >= 3 and na.max() < 80
    for t in (4, 5):                                            # sampled where the layer exists, untouched elsewhere
        assert (want[t]["N"] == 0).any() and (want[t]["N"] == nsteps).any()
    assert (want[2]["N"] == nsteps).all() and (want[0]["MIN"] > 0.0).all()
    g = ensemble("sheba_ensemble_80_day75.npz", ncol, 0)
    g.set_tracks(specs, 1)
    g.step(nsteps)
    rows = all_tracks(g, len(specs))
    g.close()
    assert tr.same_bytes(rows, want) == []


def test_restart():
    rows = run_of_test_1()
    half = NSTEPS // 2
    g = handle("spread")
    g.set_tracks(SPECS8, 1)
    g.step(half)
    kept, state, (status, step, layer), k = all_tracks(g, 8), g.get_state(), g.get_status(), g.get_clock()
    g.close()
    cfg, _, _, dT, ps = wave("spread")
    r = samsim_amd.hip_solver(cfg, NCOL)
    clock = dict(time=k.time, step=k.step, n_time_out=k.n_time_out, time_counter=k.time_counter, n_outputs=k.n_outputs)
    mo.prepare(r, cfg, state, clock, dT, ps)
    r.set_status(status, step, layer)
    r.set_tracks(SPECS8, 1)                                    # the tracks first, then their rows
    for t in range(8):
        r.set_track_state(t, kept[t])
    assert tr.same_bytes(all_tracks(r, 8), kept) == []
    assert {f: v.tobytes() for f, v in r.tracks(3, 5, 4).items()} == {f: v[5:9].tobytes() for f, v in kept[3].items()}   # a window
    r.step(NSTEPS - half)
    assert tr.same_bytes(all_tracks(r, 8), rows) == []         # byte for byte the uninterrupted run's
    r.reset_tracks()
    assert tr.same_bytes(all_tracks(r, 8), [tr.initial(NCOL)] * 8) == []
    r.set_tracks(SPECS8[:3], 1)                                # fewer tracks: no slot of the dropped ones stays valid
    assert r.ensemble_stats([track_slot(2, "N")])[track_slot(2, "N")].count == NCOL
    for t in range(3, 8):
        with pytest.raises(samsim_amd.SamsimError) as e:
            r.ensemble_stats([track_slot(t, "N")])
        assert e.value.code == -1
        with pytest.raises(samsim_amd.SamsimError) as e:
            r.tracks(t)
        assert e.value.code == -1
    r.close()


def test_determinism_and_errors():
    first = run_of_test_1()
    g = handle("spread")
    g.set_tracks(SPECS8, 1)
    g.step(NSTEPS)
    assert tr.same_bytes(all_tracks(g, 8), first) == []        # two identical runs, identical bytes
    g.close()

    g = handle("spread")
    g.set_groups((np.arange(NCOL) % 3).astype(np.int32))
    f = g._f("set_tracks")
    rq = ProfileRequest()
    rq.struct_size, rq.axis, rq.origin, rq.nbins, rq.narrays = C.sizeof(ProfileRequest), 0, 0, 8, 1
    rq.arrays[0] = A["T"]

    def reductions(slot):
        """the return codes of the five reductions for a slot"""
        out = np.zeros(64, dtype=STAT_DTYPE)
        one = (C.c_int32 * 1)(slot)
        codes = [g._f("get_ensemble_stats")(g._h, 1, one, out.ctypes.data_as(C.POINTER(capi.Stat))),
                 g._f("get_group_stats")(g._h, 1, one, out.ctypes.data)]
        for call, args in ((g.histogram_raw, (slot, capi.hist_bins(4, 0.0, 1.0))), (g.covariance_raw, ([0, slot],)),
                           (g.profile_regression_raw, (rq, slot))):
            try:
                call(*args)
                codes.append(0)
            except samsim_amd.SamsimError as e:
                codes.append(e.code)
        return codes
    # no tracks set: the track slots are bad slots, as NSCAL and -2 are; removing what is not there is accepted
    assert reductions(track_slot(0, "N")) == [-1] * 5 and reductions(NSCAL) == [-1] * 5 and reductions(-2) == [-1] * 5
    assert reductions(S["T_top"]) == [0] * 5 and reductions(-1) == [0] * 5
    assert f(g._h, 0, None, 0) == 0
    buf = np.zeros((NTF, NCOL))
    assert g._f("reset_tracks")(g._h) == -1 and g._f("get_tracks")(g._h, 0, 0, NCOL, buf.ctypes.data) == -1
    assert g._f("set_track_state")(g._h, 0, 0, NCOL, buf.ctypes.data) == -1

    def spec(**kw):
        s = TrackSpec.make("scalar", "T_top", sense=+1, threshold=0.0)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(specs, ntracks=None, every=1, h=True):
        arr = (TrackSpec * max(1, len(specs)))(*specs) if specs is not None else None
        return f(g._h if h else None, len(specs) if ntracks is None else ntracks, arr, every)
    good = [spec(), TrackSpec.make("ice_thickness")]
    assert call(good) == 0
    g.step(2)
    before = all_tracks(g, 2)
    assert (before[0]["N"] == 2).all()
    size = C.sizeof(TrackSpec)
    nl = g.nlayer
    layer = dict(kind=4, id=A["T"], layer=1)
    refused = [
        (-1, dict(specs=good, h=False)), (-1, dict(specs=good, ntracks=-1)), (-1, dict(specs=good * 4 + [spec()], ntracks=9)),
        (-1, dict(specs=None, ntracks=2)), (-1, dict(specs=good, every=0)), (-1, dict(specs=good, every=-3)),
        (-6, dict(specs=[spec(struct_size=size - 8)])), (-6, dict(specs=[spec(), spec(struct_size=size + 8)])),
        (-1, dict(specs=[spec(kind=5)])), (-1, dict(specs=[spec(kind=-1)])), (-1, dict(specs=[spec(id=NSCAL)])), (-1, dict(specs=[spec(id=-1)])),
        (-1, dict(specs=[spec(**dict(layer, id=capi.NARR))])), (-1, dict(specs=[spec(**dict(layer, layer=0))])),
        (-1, dict(specs=[spec(**dict(layer, layer=nl + 1))])), (-1, dict(specs=[spec(**dict(layer, layer=-nl - 1))])),
        (-1, dict(specs=[spec(layer=1)])), (-1, dict(specs=[spec(kind=2, id=1)])), (-1, dict(specs=[spec(kind=1, id=0, layer=-1)])),
        (-1, dict(specs=[spec(sense=2)])), (-1, dict(specs=[spec(sense=-2)])),
        (-1, dict(specs=[spec(threshold=float("nan"))])), (-1, dict(specs=[spec(threshold=float("inf"))])), (-1, dict(specs=[spec(reserved=1)])),
        # the order: the arguments before the specs, the specs in order, within a spec struct_size first (-6 tells them apart)
        (-1, dict(specs=[spec(struct_size=size - 8)], every=0)), (-1, dict(specs=[spec(struct_size=size - 8)] * 9, ntracks=9)),
        (-1, dict(specs=[spec(reserved=1), spec(struct_size=size - 8)])), (-6, dict(specs=[spec(struct_size=size - 8), spec(reserved=1)])),
        (-6, dict(specs=[spec(struct_size=size - 8, kind=9, sense=5, reserved=1)])),
    ]
    for code, kw in refused:
        assert call(**kw) == code, kw
    assert call([spec(**dict(layer, layer=nl)), spec(**dict(layer, layer=-nl)), spec(sense=0, threshold=float("nan"))]) == 0
    assert call(good) == 0                                      # (accepted calls start the rows afresh)
    g.step(2)
    for code, kw in refused[:8]:
        assert call(**kw) == code, kw
    # a refused call leaves the old tracks in force and sampling
    g.step(1)
    rows = all_tracks(g, 2)
    assert (rows[0]["N"] == 3).all() and (rows[0]["STEP_MAX"] >= g.get_clock().step - 2).all()
    # the other three calls
    fg, fs, fr = g._f("get_tracks"), g._f("set_track_state"), g._f("reset_tracks")
    assert fr(None) == -1
    whole = np.ascontiguousarray(np.stack([rows[0][x] for x in TRACK_FIELDS]))
    last = np.ascontiguousarray(np.stack([rows[1][x][NCOL - 1:] for x in TRACK_FIELDS]))
    for fn in (fg, fs):                                         # (the setter puts back what the getter returned)
        assert fn(g._h, 0, 0, NCOL, whole.ctypes.data) == 0 and fn(g._h, 1, NCOL - 1, 1, last.ctypes.data) == 0
        assert fn(None, 0, 0, NCOL, buf.ctypes.data) == -1 and fn(g._h, 0, 0, NCOL, None) == -1
        assert fn(g._h, 2, 0, NCOL, buf.ctypes.data) == -1 and fn(g._h, -1, 0, NCOL, buf.ctypes.data) == -1
        assert fn(g._h, 0, -1, 4, buf.ctypes.data) == -1 and fn(g._h, 0, 1, NCOL, buf.ctypes.data) == -1
        assert fn(g._h, 0, 0, NCOL + 1, buf.ctypes.data) == -1 and fn(g._h, 0, NCOL, 1, buf.ctypes.data) == -1
    assert tr.same_bytes(all_tracks(g, 2), rows) == []
    # track slots: good within the tracks in force, bad beyond
    assert reductions(track_slot(1, "STEP_LAST")) == [0] * 5 and reductions(track_slot(0, 0)) == [0] * 5
    for bad in (track_slot(2, 0), track_slot(0, NTF), track_slot(0, 31), track_slot(8, 0), track_slot(0, 0) - 1, NSCAL, -2):
        assert reductions(bad) == [-1] * 5, bad
    assert f(g._h, 0, None, 0) == 0 and reductions(track_slot(0, 0)) == [-1] * 5 and f(g._h, 0, None, 0) == 0
    g.close()


@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran host not built (no flang)")
def test_fortran_host_track_file(tmp_path):
    """track_every in &samsim_run: dat_ens_track.dat holds, for the thickness track and the T_top >= 0 track, the ensemble statistics
    of MEAN, MAX, STEP_MAX, N_HOLD and STEP_FIRST, equal at the printed precision (ES16.8) to what the Python mirror gets from an
    identically set up handle; without the key no new file appears"""
    sheba = golden("sheba_forcing.npz")
    keys = (("fl_sw", "flux_sw"), ("fl_lw", "flux_lw"), ("T2m", "T2m"), ("precip", "precip"))
    ncol, total, every = 96, 600, 50

    def run(d, extra):
        (d / "output").mkdir(parents=True)
        for key, name in keys:
            np.savetxt(d / f"{name}.txt.input", sheba[key], fmt="%.17e")
        (d / "samsim.nml").write_text(f"&samsim_run testcase=4, ncol={ncol}, perturb=.true., max_steps={total}{extra} /\n")
        r = subprocess.run([HOST], cwd=d, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return d / "output"
    tracked = run(tmp_path / "tracked", f", track_every={every}")
    plain = run(tmp_path / "plain", "")
    assert sorted(set(os.listdir(tracked)) - set(os.listdir(plain))) == ["dat_ens_track.dat"]
    assert (plain / "dat_ensemble.dat").read_bytes() == (tracked / "dat_ensemble.dat").read_bytes()
    cfg, st = tcs.testcase4(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*[sheba[k] for k, _ in keys], *tcs.ensemble_perturbation(ncol))
    g.set_state(st)
    g.set_clock()
    g.set_tracks([TrackSpec.make("ice_thickness"), TrackSpec.make("scalar", "T_top", sense=+1, threshold=0.0)], every)
    g.step(total)
    fields = ["MEAN", "MAX", "STEP_MAX", "N_HOLD", "STEP_FIRST"]
    slots = [track_slot(t, f) for t in range(2) for f in fields]
    q = g.ensemble_stats(slots)
    assert (g.tracks(0)["N"] == total // every).all()
    g.close()
    f = np.loadtxt(tracked / "dat_ens_track.dat")
    assert f.shape == (10, 7)
    assert f[:, 0].tolist() == [0] * 5 + [1] * 5 and f[:, 1].tolist() == [capi.TF[x] for x in fields] * 2

    def printed(got, want):
        """ES16.8 prints nine digits: half a unit of the ninth"""
        tol = 0.5e-8 * 10.0 ** math.floor(math.log10(abs(want))) * (1.0 + 1e-6) if want != 0.0 else 0.0
        return abs(got - want) <= tol
    for i, s in enumerate(slots):
        x = q[s]
        assert f[i, 2] == x.count == ncol, i
        assert all(printed(a, b) for a, b in zip(f[i, 3:], (x.mean, x.min, x.max, x.std))), (i, f[i], (x.mean, x.min, x.max, x.std))
    assert q[slots[0]].mean > 0.0 and q[slots[2]].min >= every
