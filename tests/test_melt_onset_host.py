"""The melt-onset wave and the crafted leaders still do in the CPU oracle what tests/melt_onset_seeds.py and the fixture claim: the
onset steps, which term leads, melt water in the onset step of at least a quarter of the columns, the robustness condition, the rules
of a mutation.  Run with -s to see the table.  (No GPU: tests/test_gpu_melt_onset.py takes the same columns to the device.)"""
import functools

import numpy as np
import pytest

from tests import melt_onset_seeds as mo
from tests.helpers import golden


@functools.lru_cache(maxsize=None)
def wave_run(which):
    cfg, st, clock, dT, ps, onset = mo.load_wave(which)
    traj, status = mo.oracle_trajectory(cfg, st, clock, dT, ps)
    return cfg, st, clock, dT, ps, onset, traj, status


@pytest.mark.parametrize("which", list(mo.WAVES))
def test_wave_is_what_the_generator_recorded(which):
    cfg, st, clock, dT, ps, onset, traj, status = wave_run(which)
    z = golden(mo.WAVES[which])
    assert st.ncol == mo.NCOL and cfg.nlayer == 80 and (cfg.n_top, cfg.n_middle, cfg.n_bottom) == (20, 40, 20)
    assert st.lay.shape[0] == 4 and np.isfinite(st.lay).all() and np.isfinite(st.scal).all()
    assert not status.any()
    assert all((s.n_active >= 3).all() for s in traj) and (st.n_active >= 3).all()
    got, leaders, grew = mo.onsets(st, traj)
    print(f"\n{mo.WAVES[which]}: stages {sorted(set(z['source'].tolist()))}, clock step {clock['step']}")
    print("col member snapshot natural onset leaders                                   melt water  N_active thick_snow")
    for c in range(mo.NCOL):
        names = "+".join(n for n, b in zip(mo.TERMS, leaders[:, c]) if b)
        print(f"{c:3d} {int(z['member'][c]):6d} {int(z['snapshot_step'][c]):8d} {int(z['natural_step'][c]):7d} {got[c]:5d} {names:42s} "
              f"{'yes' if grew[c] else 'no':10s} {int(st.n_active[c]):8d} {st.sc('thick_snow')[c]:.4f}")
    assert np.array_equal(got, onset), "the onset steps moved"
    assert onset.min() >= mo.MIN_LEAD and onset.max() <= mo.MAX_LEAD
    assert np.array_equal(grew, z["grew"])
    # the columns of the wave disagree about the late readers in most of the 24 steps
    on = np.stack([mo.late_reader_terms(s).any(0) for s in traj])
    mixed = int(((on.sum(1) > 0) & (on.sum(1) < mo.NCOL)).sum())
    print(f"steps in which some columns are past their onset and some are not: {mixed} of {mo.NSTEPS}; leaders "
          f"{dict(zip(mo.TERMS, leaders.sum(1).tolist()))}; melt water in the onset step: {int(grew.sum())}")
    assert len(np.unique(z["member"])) >= mo.NCOL // 2
    if which == "spread":
        assert onset.min() <= 3 and onset.max() >= 16 and len(np.unique(onset)) >= 12, "the onsets do not spread over steps 2..17"
        assert 2 * mixed > mo.NSTEPS


def test_melt_water_in_the_onset_step_of_a_quarter_of_the_columns():
    """over the two waves; only there does a missing row reach flush3 in the onset step and become a wrong number"""
    grew = np.concatenate([mo.onsets(wave_run(w)[1], wave_run(w)[6])[2] for w in ("spread", "melt")])
    print(f"melt water in the onset step: {int(grew.sum())} of {grew.size} columns")
    assert 4 * int(grew.sum()) >= grew.size


@pytest.mark.parametrize("which", list(mo.WAVES))
def test_wave_is_robust(which):
    """H_abs * (1 +- 1e-13) and * (1 + 3e-13): same on/off pattern in every step, and within 1e-7 of the unscaled run after 24 steps"""
    cfg, st, clock, dT, ps, onset, traj, status = wave_run(which)
    ok = mo.robust(cfg, st, clock, dT, ps, traj)
    assert ok.all(), f"columns {np.nonzero(~ok)[0]} are decided by round-off"


def _mutation_rules(base, st, col):
    assert np.isfinite(st.lay).all() and np.isfinite(st.scal).all()
    assert np.array_equal(st.n_active, base.n_active)
    na = int(base.n_active[col])
    assert np.array_equal(st.lay[:, na:, col], base.lay[:, na:, col]), "a mutation touched an inactive layer"
    allowed = [mo.S[n] for n in mo.SNOW]
    other = np.delete(np.arange(st.scal.shape[0]), allowed)
    assert np.array_equal(st.scal[other, col], base.scal[other, col]), "a mutation touched a scalar that is not a snow scalar"


def test_crafted_leaders_and_twins():
    """every term of the condition has a leader (that term alone in the onset step, onset not before step 2) with a twin in which no
    reader fires, or a stated reason; the mutations keep to the rules; the winter wave-mates stay off"""
    single = {s.terms[0] for s in mo.SEEDS.values() if len(s.terms) == 1}
    assert single | set(mo.NO_LEADER) | set(mo.NATURAL_LEADER) == set(mo.TERMS) and single
    for term, why in list(mo.NO_LEADER.items()) + list(mo.NATURAL_LEADER.items()):
        assert len(why) > 80, f"{term}: no reason given"
        print(f"\n{term}: {why}")
    for term in mo.NATURAL_LEADER:          # ... and it does lead alone there
        cfg, st, clock, dT, ps, onset, traj, status = wave_run("spread")
        leaders = mo.onsets(st, traj)[1]
        assert np.array_equal(leaders, np.array([t == term for t in mo.TERMS])[:, None].repeat(mo.NCOL, 1))
    print()
    for name, seed in mo.SEEDS.items():
        cfg, st, clock, dT, ps, roles = mo.build_seed_wave(seed)
        base = mo.build_seed_wave(seed, mutated=False)[1]
        assert st.ncol == mo.NCOL and set(roles) == {0, 63, 69}
        traj, status = mo.oracle_trajectory(cfg, st, clock, dT, ps)
        assert not status.any()
        onset, leaders, grew = mo.onsets(st, traj)
        want = np.array([t in seed.terms for t in mo.TERMS])
        for c, role in roles.items():
            _mutation_rules(base, st, c)
            names = "+".join(n for n, b in zip(mo.TERMS, leaders[:, c]) if b) or "-"
            print(f"{name:14s} column {c:2d} {role:6s}: onset {onset[c]:2d}  {names}  melt water {'yes' if grew[c] else 'no'}")
            if role == "leader":
                assert mo.MIN_LEAD <= onset[c] <= mo.MAX_LEAD and np.array_equal(leaders[:, c], want), f"{name}: column {c}"
            else:
                assert not np.any([mo.late_reader_terms(t)[:, c].any() for t in traj]), f"{name}: a reader fires in the twin"
        mates = np.delete(np.arange(mo.NCOL), list(roles))
        assert not seed.quiet_mates or not onset[mates].any(), f"{name}: a reader fires in a wave-mate"
        assert np.array_equal(st.lay[:, :, mates], base.lay[:, :, mates]) and np.array_equal(st.scal[:, mates], base.scal[:, mates])
        ok = mo.robust(cfg, st, clock, dT, ps, traj)
        assert ok[list(roles)].all(), f"{name}: decided by round-off"
