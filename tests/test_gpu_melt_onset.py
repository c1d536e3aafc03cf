"""Melt onset on the device: the steps in which the fused down sweep's stored-row decision changes its answer.

sweep_down_fused (samsim_sweeps_fused.h) stores psi_s / psi_l / psi_g of layers >= 3 only where it predicts, from the finished top
layer, that func_freeboard or flush3 will read them later in the step, or where the step is the last of its launch or precedes an
output point.  Where the prediction is wrong nothing stops: refill_psi_rows (samsim_sweeps_unfused.h) rebuilds the rows from the
second sweep's temperature, which is not the reference's arithmetic.  Two waves of 70 columns x 80 layers, each under one clock
(tests/golden/make_melt_onset_fixtures.py): in `spread` (melt_onset_wave_80.npz) the columns are 2..17 steps before the late-reader
condition of tests/melt_onset_seeds.py goes from off to on, so they disagree about the decision in 15 of the 24 steps; in `melt`
(melt_onset_wave_80_melt.npz) the forcing takes all columns through their onset in one step and 64 of them have melt water in that
very step, which flush3 takes through the rows -- but under 0.04 mm of snow, below thick_min, where the sweep stores the rows
whatever the other terms say.  `melt_bare` is that wave with the snow taken away (tests/melt_onset_seeds.py): the T_top term alone
decides there, and a missing row becomes a wrong S_abs, m and thick.

Checked: every single step against the CPU oracle at RTOL (integers exactly), the volume fractions over all active layers
included; that the result does not depend on how the 24 steps are cut into launches (last_step), on the wave-mates, or on an output
point next to the onset (next_out, the step after an output, the unfused order of an output step), whose snapshot equals the
oracle's; the per-column-ocean and the tracer instantiation; crafted leaders of single terms of the condition with their twins.

With a counter build of the library (-DSAMSIM_STAMPS=2, selected with SAMSIM_HIP_LIB) the launch-cut test also asserts that no lane
called refill_psi_rows and that func_freeboard and flush3 did run (in launches of one step every row is stored anyway: the count
means something over the longer launches only)."""
import ctypes as C
import functools

import numpy as np
import pytest

import samsim_amd
from samsim_amd.capi import State
from tests import melt_onset_seeds as mo
from tests.helpers import RTOL, assert_state_close, rel_err

pytestmark = pytest.mark.gpu

NCOL, NSTEPS, WAVE = mo.NCOL, mo.NSTEPS, 64
ARRAYS = ["H_abs", "S_abs", "m", "thick", "T", "phi", "psi_s", "psi_l", "psi_g", "S_bu"]
CT_L_FLUSH3, CT_L_FREEBOARD, CT_REFILL = 29, 31, 32     # slots of samsim_debug_stamps (samsim_probe.h)


WHICH = list(mo.WAVES)


@functools.lru_cache(maxsize=None)
def wave(which):
    cfg, st, clock, dT, ps, onset = mo.load_wave(which)
    for a in (st.lay, st.scal, st.n_active, dT, ps, onset):
        a.setflags(write=False)
    return cfg, st, clock, dT, ps, onset


@functools.lru_cache(maxsize=None)
def oracle(which, variant="plain", n_time_out=None):
    """the oracle's states after each of the 24 steps, and its output snapshot -- computed once per set-up, never modified"""
    cfg, st, clock, dT, ps, _ = wave(which)
    clock = dict(clock) if n_time_out is None else dict(clock, n_time_out=n_time_out)
    traj, status, out = mo.oracle_trajectory(cfg, st, clock, dT, ps, NSTEPS, variant, want_output=True)
    assert not status.any()
    return traj, out


def gpu(which, variant="plain", n_time_out=None, repeat=1):
    cfg0, st, clock, dT, ps, _ = wave(which)
    cfg = mo.variant_config(cfg0, variant)
    clock = dict(clock) if n_time_out is None else dict(clock, n_time_out=n_time_out)
    if repeat > 1:
        st = State(np.ascontiguousarray(np.repeat(st.lay, repeat, axis=2)), np.ascontiguousarray(np.repeat(st.scal, repeat, axis=1)),
                   np.ascontiguousarray(np.repeat(st.n_active, repeat)))
        dT, ps = np.repeat(dT, repeat), np.repeat(ps, repeat)
    g = samsim_amd.hip_solver(cfg, st.ncol)
    mo.prepare(g, cfg, st, clock, dT, ps, variant)
    return g


def assert_same_bits(a, b, what):
    assert np.array_equal(a.n_active, b.n_active), what
    bad = np.nonzero((a.scal != b.scal).any(1))[0]
    assert bad.size == 0, f"{what}: scalars {[samsim_amd.capi.SCALARS[i] for i in bad]}"
    act = np.arange(a.nlayer)[:, None] < a.n_active[None, :]
    for n in ARRAYS:
        assert np.array_equal(np.where(act, a.arr(n), 0.0), np.where(act, b.arr(n), 0.0)), f"{what}: {n}"


def counters():
    """the counter build's read-out function, or None with the product library"""
    lib = samsim_amd.load()
    try:
        f = lib.samsim_debug_stamps
    except AttributeError:
        return None
    buf = (C.c_ulonglong * 48)()

    def read(reset):
        assert f(buf, reset) == 0
        return list(buf)
    return read


@pytest.mark.parametrize("which", WHICH)
def test_wave_follows_the_oracle_step_by_step(which):
    """24 launches of one step; after each, samsim_get_state against the oracle at RTOL, N_active and status exactly.  Every step
    is the last of its launch, so every row is stored: this holds last_step and, through melt_out*, S_abs, m and thick after
    flush3, the readers inside the step"""
    traj, _ = oracle(which)
    g = gpu(which)
    for i in range(NSTEPS):
        g.step(1)
        got = g.get_state()
        assert not g.get_status()[0].any()
        assert_state_close(got, traj[i], RTOL, what=f"step {i + 1}")
    g.close()


def cuts_of(total, chunk):
    return [min(chunk, total - d) for d in range(0, total, chunk)]


def cut_columns(which):
    """three columns with different onset steps where the wave has them, melt water in the onset step first"""
    _, _, _, _, _, onset = wave(which)
    grew = mo.golden(mo.WAVES[which])["grew"]
    order = sorted(range(NCOL), key=lambda c: (not grew[c], c))
    cols = []
    for c in order:
        if (which != "spread" or onset[c] not in [onset[d] for d in cols]) and 3 <= onset[c] <= 16:
            cols.append(c)
        if len(cols) == (3 if which == "spread" else 1):      # (in `melt` all onsets are in one step: one column stands for all)
            break
    return cols


@pytest.mark.parametrize("which", WHICH)
def test_launch_cuts_do_not_change_a_bit(which):
    """one launch of 24, launches of 1, launches of 7, and for three columns the onset step as the first, the only and the last step
    of its launch: same bits, and the oracle's final state at RTOL.  In a launch's last step every row is stored; in every other
    step the sweep decides -- a wrong decision shows as a difference between the cuts"""
    _, _, _, _, _, onset = wave(which)
    traj, _ = oracle(which)
    plans = {"24": [NSTEPS], "1": cuts_of(NSTEPS, 1), "7": cuts_of(NSTEPS, 7)}
    cols = cut_columns(which)
    assert len(cols) == (3 if which == "spread" else 1)
    for c in cols:
        k = int(onset[c])
        plans[f"col {c}: onset step {k} first of its launch"] = [k - 1, NSTEPS - k + 1]
        plans[f"col {c}: onset step {k} alone"] = [k - 1, 1, NSTEPS - k]
        plans[f"col {c}: onset step {k} last of its launch"] = [k, NSTEPS - k]
    states = {}
    read = counters()
    if read:
        read(1)
    for name, cuts in plans.items():
        assert sum(cuts) == NSTEPS and min(cuts) >= 1
        g = gpu(which)
        for n in cuts:
            g.step(n)
        assert not g.get_status()[0].any()
        states[name] = g.get_state()
        g.close()
        assert_state_close(states[name], traj[-1], RTOL, what=f"launches {name} against the oracle")
    for name, s in states.items():
        assert_same_bits(s, states["24"], f"launches {name} against one launch of 24")
    if read:        # a counter build: over all these launches no lane met a reader without its rows, and the readers did run
        v = read(0)
        print(f"counter build, {which}: refill_psi_rows lanes {v[CT_REFILL]}, func_freeboard lanes {v[CT_L_FREEBOARD]}, flush3 lanes {v[CT_L_FLUSH3]}")
        assert v[CT_REFILL] == 0 and v[CT_L_FREEBOARD] != 0
        assert which == "spread" or v[CT_L_FLUSH3] != 0       # (no melt water in `spread`: tests/test_melt_onset_host.py)


@pytest.mark.parametrize("which", WHICH)
def test_a_column_does_not_depend_on_its_wave_mates(which):
    """each column in a wave of 64 copies of itself (a 70 x 64 column handle) against the mixed wave, bit for bit: in the mixed wave
    the lanes disagree about the stored rows, in a wave of copies they never do"""
    g = gpu(which)
    g.step(NSTEPS)
    mixed = g.get_state()
    g.close()
    g = gpu(which, repeat=WAVE)
    g.step(NSTEPS)
    solo, status = g.get_state(), g.get_status()[0]
    g.close()
    assert not status.any()
    rep = State(np.repeat(mixed.lay, WAVE, axis=2), np.repeat(mixed.scal, WAVE, axis=1), np.repeat(mixed.n_active, WAVE))
    assert_same_bits(solo, rep, "wave of copies against the mixed wave")


@pytest.mark.parametrize("which,nth", [("spread", 0), ("spread", 1), ("melt_bare", 0)])
@pytest.mark.parametrize("offset", [-1, 0, 1, 2], ids=["onset-1", "onset", "onset+1", "onset+2"])
def test_output_point_next_to_an_onset(which, nth, offset):
    """n_time_out is set so that the output step is the step before a column's onset (next_out stores the rows in the step before
    that), the onset step itself (the unfused order), and the first and the second step after it: the snapshot equals the oracle's,
    and so does the state after the 24 steps"""
    cfg, st, clock, dT, ps, onset = wave(which)
    col = cut_columns(which)[nth]
    k = int(onset[col]) + offset
    assert 1 <= k <= NSTEPS
    nto = cfg.i_time_out - (k - 1)          # output_point fires in relative step k
    traj, oout = oracle(which, n_time_out=nto)
    o_onset, _, _ = mo.onsets(st, traj)
    assert np.array_equal(o_onset, onset), "moving the output point moved an onset"
    g = gpu(which, n_time_out=nto)
    assert g.steps_to_output() == k
    g.step(NSTEPS)
    gout, state = g.get_output(), g.get_state()
    assert not g.get_status()[0].any()
    g.close()
    assert gout.step == oout.step == clock["step"] + k
    assert np.array_equal(gout.n_active, oout.n_active)
    act = np.arange(cfg.nlayer)[:, None] < oout.n_active[None, :]
    for n in ["T", "psi_s", "psi_l", "psi_g", "S_bu", "thick", "H_abs", "S_abs", "m"]:
        e = rel_err(gout.arr(n)[act], oout.arr(n)[act], 1e-3 if n == "H_abs" else 1e-7)
        assert e <= RTOL, f"{n}: {e:.3e}"
    act1 = np.arange(cfg.nlayer)[:, None] < oout.n_active[None, :] - 1
    assert rel_err(gout.arr("ray")[act1], oout.arr("ray")[act1], 1e-6) <= RTOL, "ray"
    for n in ["freeboard", "thick_snow", "T_snow", "thickness", "bulk_salin", "energy_stored", "freshwater", "total_resist", "T_top",
              "grav_drain"]:
        e = rel_err(gout.sc(n), oout.sc(n), {"grav_drain": 1e-8}.get(n, 1e-7))
        assert e <= RTOL, f"{n}: {e:.3e}"
    assert_state_close(state, traj[-1], RTOL, what=f"after {NSTEPS} steps, output in step {k}")


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("variant", ["sites", "bgc"])
def test_other_instantiations_of_the_kernel(variant, which):
    """per-column ocean (zero offsets: KShebaSites decides as KSheba does) and one passive tracer (always the unfused order, every
    row stored), in launches of 7, against the oracle given the same set-up after each launch"""
    traj, _ = oracle(which, variant)
    g = gpu(which, variant)
    done = 0
    for n in cuts_of(NSTEPS, 7):
        g.step(n)
        done += n
        assert not g.get_status()[0].any()
        assert_state_close(g.get_state(), traj[done - 1], RTOL, what=f"{variant}, step {done}")
    g.close()


@functools.lru_cache(maxsize=None)
def seed_oracle(name):
    cfg, st, clock, dT, ps, roles = mo.build_seed_wave(mo.SEEDS[name])
    traj, status = mo.oracle_trajectory(cfg, st, clock, dT, ps, NSTEPS)
    assert not status.any()
    return traj


@pytest.mark.parametrize("name", list(mo.SEEDS))
def test_crafted_leaders_and_twins(name):
    """leaders in columns 0 and 69, their twin in lane 63, among winter columns in which no reader fires (psi_s_top) or among the
    columns of the melt wave (T_top_bare): every single step against the oracle, then one launch of 24 against the single steps, bit
    for bit"""
    cfg, st, clock, dT, ps, roles = mo.build_seed_wave(mo.SEEDS[name])
    traj = seed_oracle(name)
    onset, leaders, _ = mo.onsets(st, traj)
    assert all(onset[c] >= mo.MIN_LEAD for c, r in roles.items() if r == "leader") and not onset[[c for c, r in roles.items() if r != "leader"]].any()

    def handle():
        g = samsim_amd.hip_solver(cfg, st.ncol)
        mo.prepare(g, cfg, st, clock, dT, ps)
        return g
    g = handle()
    for i in range(NSTEPS):
        g.step(1)
        assert_state_close(g.get_state(), traj[i], RTOL, what=f"{name}, step {i + 1}")
    single = g.get_state()
    g.close()
    g = handle()
    g.step(NSTEPS)
    assert_same_bits(g.get_state(), single, f"{name}: one launch of {NSTEPS} against launches of 1")
    g.close()
