#!/usr/bin/env python3
"""TEST INFRASTRUCTURE / fixture generator: two waves of columns that are a few steps away from a melt onset.

    tests/golden/melt_onset_wave_80.npz        `spread`: onsets spread over steps 2..17, no melt water in the onset step
    tests/golden/melt_onset_wave_80_melt.npz   `melt`: all onsets in one step, melt water in that step in 64 columns

    each: lay[4, 80, 70], scal[NSCAL, 70], n_active[70], dT2m[70], precip_scale[70], one clock, onset[70] (the step, counted from the
    clock, in which the late-reader condition of tests/melt_onset_seeds.py goes from off to on), grew[70] (melt_out1 + melt_out2 grew
    in that step), and where a column comes from: source[70], clock_set_back_days[70], member[70], snapshot_step[70], natural_step[70]

The CPU oracle alone does all of it (the reference tree is not read).

WHICH SOURCE.  Not sheba_ensemble_80_day300.npz: free-run, that stage meets its first onsets after 2.8 model days, but they are warm
spells of the winter (T_top >= T_freeze under 0.15-0.28 m of snow, 45 onsets a day, no melt water), and the melt season is 40 model
days = 13 minutes of oracle time away, which was the generator's whole budget.  Not tc4_melt_state.npz either: 64 perturbed replicas
of it, single-stepped for 31 days, gave 322 onsets, none with melt water in the onset step after a restart, and it has 100 layers, not
the headline 80.  Used: the later stages of the same ensemble, sheba_ensemble_80_day345.npz and sheba_ensemble_80_day360.npz (20+40+20,
256 members under their own perturbations), see SCANS.

 1. Each scan single-steps all 256 members of a stage: day 345 under its own clock for one day, day 345 with its clock SET BACK BY
    FIVE DAYS for five days (the melt-season columns meet the last cold nights again and go through their onsets once more), day 360
    for one day.  Every step in which the condition goes from off to on in a member with N_active >= 3 (after 17 steps off; day 360:
    after one) is an EVENT; the member's prognostic state 2..17 steps before it goes into a pool with the clock it was taken at.
    Printed by the run that wrote the committed files: 173, 1071 and 88 events.
 2. One wave shares one clock, and the natural onsets of the members do not give both a spread of onset steps and melt water in any
    window of 16 steps: the forcing tables have kinks at which a hundred members start in the same step, and between them no onset
    comes with melt water.  So the members are SHIFTED IN WALL TIME: the clocks 1..4 steps before the 12 densest windows of natural
    onsets are tried as the common one, the whole pool is run for 24 steps under each, and a pool state is a CANDIDATE under a clock
    if the oracle restarted from it has an onset in step 2..17 (N_active >= 3, status 0).  What is recorded is the onset the oracle
    gives under the common clock.  No column of the committed waves sits at its natural clock (snapshot_step differs from the
    clock's step in all 140): every onset in them is one under shifted forcing, and the re-onsets of day 360 did not survive a restart.
 3. No clock gives both properties, so two waves are written: `spread` under the clock with the most candidates on the most onset
    steps (step 2943783: 218 candidates, 16 onset steps, none with melt water), `melt` under the one with the most melt-water onsets
    (step 2977593: 273 candidates, all with their onset in step 11, 64 with melt water).
 4. Robustness filter: a candidate is kept if H_abs * (1 +- 1e-13) and H_abs * (1 + 3e-13) give the same on/off pattern in all 24
    steps and end within 1e-7 of the unscaled run in the measure of helpers.assert_state_close.  More than a quarter dropped is an
    error.  Dropped in the committed run: 0 of 218 and 0 of 273.
 5. 70 of the kept ones per wave, round-robin over the onset steps (in `melt`: the melt-water columns first).

What the `melt` wave does NOT give: its melt-water columns all carry 0.04 mm of snow, below thick_min, under which the down sweep
stores the psi rows unconditionally.  tests/melt_onset_seeds.py derives `melt_bare` from it (snow scalars zeroed), where it decides.

Run in the build container:  python tests/golden/make_melt_onset_fixtures.py [--cache PREFIX]   (about 8 minutes on 8 cores;
--cache keeps the pool of each scan in PREFIX.<n>.npz and reuses it)
"""
import argparse
import collections
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from samsim_amd.capi import State  # noqa: E402
from tests import melt_onset_seeds as mo  # noqa: E402
from tests.helpers import golden, sheba_forcing  # noqa: E402
from tests.oracle_lib import oracle_solver  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DAY = 8640
# (stage of the ensemble, days its clock is set back by, days of single steps, steps the condition must have been off before an event)
SCANS = (("sheba_ensemble_80_day345.npz", 0, 1, 17), ("sheba_ensemble_80_day345.npz", 5, 5, 17), ("sheba_ensemble_80_day360.npz", 0, 1, 1))
WINDOWS = 12                # densest windows of natural onsets whose clocks are tried as the common one
THREADS = min(8, len(os.sched_getaffinity(0)))
CLOCK_KEYS = ("time", "step", "n_time_out", "time_counter", "n_outputs")


def clock_of(o):
    k = o.get_clock()
    return {n: getattr(k, n) for n in CLOCK_KEYS}


def stage_config():
    return mo.config(golden(SCANS[0][0]))


def build_pool(source, back, days, min_off):
    """the events of `days` days of single steps from a stage, its clock set back by `back` days"""
    SCAN_STEPS = days * DAY
    z = golden(source)
    cfg = mo.config(z)
    n = int(z["lay"].shape[2])
    dT, ps = np.ascontiguousarray(z["dT2m"]), np.ascontiguousarray(z["precip_scale"])
    st = State(np.ascontiguousarray(z["lay"]), np.ascontiguousarray(z["scal"]), np.ascontiguousarray(z["n_active"]))
    clock = {k: (float(z[k]) if k == "time" else int(z[k])) for k in CLOCK_KEYS}
    clock["time"] -= back * DAY * cfg.dt
    clock["step"] -= back * DAY
    clock["time_counter"] -= back * 8          # 3-hourly forcing tables
    clock["n_outputs"] -= back
    o = oracle_solver(cfg, n)
    o.set_threads(THREADS)
    o.set_forcing(*sheba_forcing(), dT, ps)
    o.set_state(st)
    o.set_clock(**clock)
    t0 = time.time()
    ring = collections.deque(maxlen=mo.MAX_LEAD + 1)
    off_run = np.zeros(n, dtype=np.int64)
    pool = []
    for i in range(SCAN_STEPS):
        o.step(1)
        s, k = o.get_state(), clock_of(o)
        ring.append((s, k))
        on = mo.late_reader_terms(s).any(0)
        for c in np.nonzero(on & (off_run >= min_off) & (i > mo.MAX_LEAD) & (s.n_active >= 3))[0]:
            lead = mo.MIN_LEAD + len(pool) % (mo.MAX_LEAD - mo.MIN_LEAD + 1)
            zs, zk = ring[-1 - lead]
            pool.append(dict(lay=zs.lay[:4, :, c].copy(), scal=zs.scal[:, c].copy(), n_active=int(zs.n_active[c]), member=int(c),
                             natural_step=int(k["step"]), clock=zk))
        off_run = np.where(on, 0, off_run + 1)
    assert not o.get_status()[0].any()
    o.close()
    print(f"{source}, clock set back by {back} days: {len(pool)} events of {len({p['member'] for p in pool})} members in {SCAN_STEPS} single steps ({time.time() - t0:.0f} s)", flush=True)
    members = [p["member"] for p in pool]
    return dict(lay=np.stack([p["lay"] for p in pool], axis=2), scal=np.stack([p["scal"] for p in pool], axis=1),
                n_active=np.array([p["n_active"] for p in pool], dtype=np.int32), member=np.array(members),
                natural_step=np.array([p["natural_step"] for p in pool]), dT2m=dT[members], precip_scale=ps[members],
                clocks=np.array([[p["clock"][k] for k in CLOCK_KEYS] for p in pool], dtype=np.float64))


def build_pools(cache):
    pools = []
    for i, scan in enumerate(SCANS):
        f = f"{cache}.{i}.npz" if cache else None
        if f and os.path.exists(f):
            pools.append(dict(np.load(f)))
        else:
            pools.append(build_pool(*scan))
            if f:
                np.savez_compressed(f, **pools[-1])
    for i, p in enumerate(pools):
        p["scan"] = np.full(len(p["member"]), i)
    return {k: np.concatenate([p[k] for p in pools], axis=-1 if k in ("lay", "scal") else 0) for k in pools[0]}


def candidates(cfg, st, P, clock):
    traj, status = mo.oracle_trajectory(cfg, st, clock, P["dT2m"], P["precip_scale"], threads=THREADS)
    onset, leaders, grew = mo.onsets(st, traj)
    na_ok = np.all([s.n_active >= 3 for s in traj], axis=0)
    ok = (onset >= mo.MIN_LEAD) & (onset <= mo.MAX_LEAD) & na_ok & (status == 0)
    return ok, onset, leaders, grew, traj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None)
    a = ap.parse_args()
    P = build_pools(a.cache)
    cfg = stage_config()
    st = State(np.ascontiguousarray(P["lay"]), np.ascontiguousarray(P["scal"]), np.ascontiguousarray(P["n_active"]))
    # 3. the common clock: the pool clocks from which one of the densest 16-step windows of natural onsets is 2..17 steps away
    ns = P["natural_step"]
    dense = np.convolve(np.bincount(ns - ns.min()), np.ones(16, dtype=np.int64))      # [i]: onsets in steps i-15..i (from ns.min())
    starts = []
    for i in np.argsort(dense)[::-1]:
        if all(abs(int(i) - j) > 40 for j in starts):
            starts.append(int(i))
        if len(starts) == WINDOWS:
            break
    starts = np.array(starts) - 15 + ns.min()
    clocks = np.unique(P["clocks"], axis=0)
    clocks = clocks[[bool(((w - r[1] >= mo.MIN_LEAD - 1) & (w - r[1] <= mo.MIN_LEAD + 2)).any()) for r in clocks for w in [starts]]]
    best = {}
    t0 = time.time()
    for row in clocks:
        clock = {k: (float(v) if k == "time" else int(v)) for k, v in zip(CLOCK_KEYS, row)}
        ok, onset, leaders, grew, _ = candidates(cfg, st, P, clock)
        nsteps, ngrew = len(np.unique(onset[ok])), int((ok & grew).sum())
        print(f"clock step {clock['step']}: {int(ok.sum())} candidates on {nsteps} onset steps, {ngrew} with melt water in the onset step "
              f"({time.time() - t0:.0f} s)", flush=True)
        # no clock gives both (see the docstring): one wave for the spread of the onset steps, one for the melt water
        for which, score in (("spread", min(int(ok.sum()), 8 * nsteps)), ("melt", ngrew)):
            if which not in best or score > best[which][0]:
                best[which] = (score, clock)
    for which in ("spread", "melt"):
        write_wave(cfg, st, P, best[which][1], which)


def write_wave(cfg, st, P, clock, which):
    ok, onset, leaders, grew, traj = candidates(cfg, st, P, clock)
    idx = np.nonzero(ok)[0]
    natural = int((P["clocks"][idx, 1] == clock["step"]).sum())
    print(f"{which}: common clock step {clock['step']}, {len(idx)} candidates ({natural} of them taken at that very clock)")
    # 4. robustness
    cst = mo.columns(st, idx)
    ctraj = [mo.columns(s, idx) for s in traj]
    keep = mo.robust(cfg, cst, clock, P["dT2m"][idx], P["precip_scale"][idx], ctraj, threads=THREADS)
    print(f"{which}: robustness filter: {int((~keep).sum())} of {len(idx)} candidates dropped")
    assert 4 * int((~keep).sum()) <= len(idx), "the filter dropped more than a quarter of the candidates"
    idx = idx[keep]
    # 5. 70 columns: round-robin over the onset steps; in the melt wave the columns with melt water in the onset step first
    rng = np.random.default_rng(20)
    buckets = {k: list(rng.permutation(idx[onset[idx] == k])) for k in range(mo.MIN_LEAD, mo.MAX_LEAD + 1)}
    if which == "melt":
        buckets = {k: sorted(b, key=lambda j: not grew[j]) for k, b in buckets.items()}
    chosen = []
    while len(chosen) < mo.NCOL and any(buckets.values()):
        for k in range(mo.MIN_LEAD, mo.MAX_LEAD + 1):
            if buckets[k] and len(chosen) < mo.NCOL:
                chosen.append(int(buckets[k].pop(0)))
    assert len(chosen) == mo.NCOL, f"only {len(chosen)} columns"
    chosen = np.array(chosen)[rng.permutation(mo.NCOL)]      # no order of onsets along the lanes
    out = os.path.join(GOLDEN, mo.WAVES[which])
    np.savez_compressed(out, lay=np.ascontiguousarray(P["lay"][:, :, chosen]), scal=np.ascontiguousarray(P["scal"][:, chosen]),
                        n_active=np.ascontiguousarray(P["n_active"][chosen]), dT2m=P["dT2m"][chosen], precip_scale=P["precip_scale"][chosen],
                        onset=onset[chosen], grew=grew[chosen], member=P["member"][chosen], natural_step=P["natural_step"][chosen],
                        snapshot_step=P["clocks"][chosen, 1].astype(np.int64), source=np.array([SCANS[i][0] for i in P["scan"][chosen]]),
                        clock_set_back_days=np.array([SCANS[i][1] for i in P["scan"][chosen]]), nlayer=cfg.nlayer, n_top=cfg.n_top,
                        n_bottom=cfg.n_bottom, **clock)
    on_per_step = [int(((onset[chosen] <= s)).sum()) for s in range(1, mo.NSTEPS + 1)]
    print(f"{out}: {os.path.getsize(out) // 1024} KB; onset steps {np.bincount(onset[chosen], minlength=mo.MAX_LEAD + 1)[mo.MIN_LEAD:].tolist()}; "
          f"melt water in the onset step in {int(grew[chosen].sum())}; leaders {dict(zip(mo.TERMS, leaders[:, chosen].sum(1).tolist()))}; "
          f"members {len(set(P['member'][chosen].tolist()))}; columns past their onset after each step {on_per_step}")


if __name__ == "__main__":
    main()
