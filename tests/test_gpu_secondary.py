"""Parity of the HIP path on the secondary parametrisations: testcases 3, 5 and 7 of the
reference -- Notz climatological fluxes (atmoflux_flag 1), fixed fluxes (3), constant snow fall with precip_flag 0,
fl_grav_drain_simple (grav_flag 3), melt-water removal (flush_flag 4), flood_simple (flood_flag 3), albedo_flag 1.
Same bar as tests/test_gpu_parity.py: 1e-6 relative against the CPU oracle, integers exact; the oracle itself is
pinned bit for bit against the flang-built reference on these testcases (tests/test_oracle_golden.py)."""
import os

import numpy as np
import pytest

import samsim_amd
from samsim_amd import testcases as tcs
from tests.helpers import RTOL, assert_state_close, golden, rel_err, sheba_forcing
from tests.oracle_lib import oracle_solver
from tests.test_oracle_golden import _restore_midstep

pytestmark = pytest.mark.gpu

NTHREADS = min(16, len(os.sched_getaffinity(0)))


def _pair(cfg, ncol, st, forcing=None):
    g = samsim_amd.hip_solver(cfg, ncol)
    o = oracle_solver(cfg, ncol)
    o.set_threads(NTHREADS)
    for s in (g, o):
        if forcing is not None:
            s.set_forcing(*forcing, *tcs.ensemble_perturbation(ncol))
        s.set_state(st)
        s.set_clock()
    return g, o


def _check(g, o, what, rtol=RTOL):
    assert np.array_equal(g.get_status()[0], o.get_status()[0]), f"{what}: STOP codes differ"
    sg, so = g.get_state(), o.get_state()
    assert_state_close(sg, so, rtol, what=what)
    return sg, so


def _teacher_forced(g, o, total_steps, every, window, what, rtol=RTOL):
    """advance the oracle to `total_steps`; every `every` steps restart the HIP path from the oracle's state and require
    agreement `window` steps later (the melt seasons amplify round-off in a free run)"""
    seen, snow = set(), []
    while o.get_clock().step + every <= total_steps:
        k = o.get_clock()
        g.set_state(o.get_state())
        g.set_clock(time=k.time, step=k.step, n_time_out=k.n_time_out, time_counter=k.time_counter, n_outputs=k.n_outputs)
        g.step(window)
        o.step(window)
        _, so = _check(g, o, f"{what}: window at step {k.step}", rtol)
        seen.update(int(v) for v in so.n_active)
        snow.append(float(so.sc("thick_snow").max()))
        o.step(every - window)
    return seen, snow


def test_tc3_notz_fluxes_and_constant_snowfall():
    """testcase 3: free run from open water through the first 140 days against the oracle and against the reference's
    own output records, then teacher-forced windows through both melt seasons of the 756-day run"""
    ncol = 16
    cfg, st = tcs.testcase3(ncol)
    g, o = _pair(cfg, ncol, st)
    ref = golden("tc3_ref_fullprec.npz")
    g.set_output_window(0, 1)
    for i in range(40):
        out = g.run_to_output()
        assert out.step == ref["step"][i] and out.n_active[0] == ref["N_active"][i], f"output {i}"
        na = int(out.n_active[0])
        for n in ["T", "psi_s", "psi_l", "S_bu", "thick"]:
            assert rel_err(out.arr(n)[:na, 0], ref["a_" + n][i, :na], 1e-7) <= RTOL, f"output {i}: {n} vs reference"
        for n, floor in (("thick_snow", 1e-7), ("T_snow", 1e-2), ("T_top", 1e-2), ("freeboard", 1e-7), ("thickness", 1e-7)):
            assert rel_err(out.sc(n)[0], ref["s_" + n][i], floor) <= RTOL, f"output {i}: {n} vs reference"
    o.step(g.get_clock().step)
    sg, so = _check(g, o, "tc3 day 140")
    assert so.sc("thick_snow").min() > 0.01 and int(so.n_active[0]) > 5
    assert sg.sc("fl_rest")[0] == so.sc("fl_rest")[0] > 179.0          # sub_notzflux ran on both sides
    seen, snow = _teacher_forced(g, o, tcs.i_time(cfg), every=30240, window=3000, what="tc3")
    assert min(snow) < 1e-3 and max(snow) > 0.1, (seen, snow)     # windows in snow-covered winter and bare-ice summer


def test_tc5_fixed_fluxes_flushing_of_a_slab():
    """testcase 5: every layer active from the start, salinity reset at step 2, constant fluxes, flushing (flush3) melts the
    1 m slab down to a few layers; free run over the first 20 000 steps, then teacher-forced windows to the end"""
    ncol = 16
    cfg, st = tcs.testcase5(ncol)
    g, o = _pair(cfg, ncol, st)
    done = 0
    for upto in (1, 2, 3, 1080, 1081, 20000):
        g.step(upto - done)
        o.step(upto - done)
        done = upto
        sg, so = _check(g, o, f"tc5 step {upto}")
        if upto == 2:
            assert np.allclose(sg.arr("S_abs"), 5.0 * sg.arr("m"), rtol=1e-12, atol=0)    # mo_grotz.f90:543-544
    seen, _ = _teacher_forced(g, o, tcs.i_time(cfg), every=10800, window=1500, what="tc5", rtol=1e-6)
    assert min(seen) < 30 and max(seen) == 100, seen


def test_tc7_simple_parametrisations_free_run_and_reference_windows():
    """testcase 7: perturbed ensemble through open water, freeze-up and the first days of growth (grav_flag 3 acting), then
    12-hour windows restarted from the REFERENCE's own mid-step states (fixture) through growth, the melt season with
    flush_flag 4, and refreeze: HIP vs oracle at the parity bar, and HIP vs the reference's next record."""
    ncol = 16
    cfg, st = tcs.testcase7(ncol)
    g, o = _pair(cfg, ncol, st, forcing=sheba_forcing())
    for n in (1, 560000, 30000):
        g.step(n)
        o.step(n)
        sg, so = _check(g, o, f"tc7 free run to step {o.get_clock().step}")
    assert so.n_active.max() > 5

    ref = golden("tc7_ref_fullprec.npz")
    cfg1, _ = tcs.testcase7(1)
    g = samsim_amd.hip_solver(cfg1, 1)
    o = oracle_solver(cfg1, 1)
    for s in (g, o):
        s.set_forcing(*sheba_forcing())
    g.set_output_window(0, 1)
    for p, idx in enumerate(ref["tf_index"]):
        _restore_midstep(o, ref, 2 * p, cfg1)
        o.step_part_b()                                   # finish the reference's step: now at a step boundary
        k = o.get_clock()
        g.set_state(o.get_state())
        g.set_clock(time=k.time, step=k.step, n_time_out=k.n_time_out, time_counter=k.time_counter, n_outputs=k.n_outputs)
        og, oo = g.run_to_output(), o.run_to_output()
        j = 2 * p + 1
        assert og.step == oo.step == ref["tf_step"][j] and og.n_active[0] == ref["tf_N_active"][j], f"window {idx}"
        na = int(og.n_active[0])
        for n in ["T", "psi_s", "psi_l", "S_bu", "thick", "H_abs", "S_abs", "m"]:
            floor = 1e-3 if n == "H_abs" else 1e-7
            assert rel_err(og.arr(n)[:na, 0], ref["tf_a_" + n][j, :na], floor) <= RTOL, f"window {idx}: {n} vs reference"
        for n, floor in (("m_snow", 1e-5), ("thick_snow", 1e-7), ("T_snow", 1e-2), ("T_top", 1e-2), ("freeboard", 1e-7),
                         ("thickness", 1e-7)):
            assert rel_err(og.sc(n)[0], ref["tf_s_" + n][j], floor) <= RTOL, f"window {idx}: {n} vs reference"
        _check(g, o, f"tc7 window {idx}")


@pytest.mark.parametrize("tc,nout", [(2, 120), (9, 72), (6, 60), (33, 70), (34, 1417)])
def test_tank_experiments(tc, nout):
    """testcases 2, 6, 9, 33, 34 (boundflux_flag 3, tank_flag 2, T2m schedules): the HIP path's output snapshots against the
    reference's own records and, at the end, the full state against the oracle; the water below the ice gets saltier.
    At the parity bar: these runs amplify nothing (the checker and its FMA build stay within 3.3e-13 of each other over the whole
    free runs), and the HIP path stays within 3.1e-12 of the checker and 1.2e-13 of these records at every output of every run
    (profiles/r25_event_windows.json, "tank"; the 2e-6 asserted here until then was never needed).  Testcase 6 stays at its first
    60 of 156 outputs: the whole run is 280 800 steps of a single wave, 22 s on its own; all 156 were compared once, in that profile.
    tests/test_gpu_event_windows.py::test_tank_budget_in_ten_step_windows tiles the worst interval of three of the runs."""
    ncol = 8
    cfg, st = getattr(tcs, f"testcase{tc}")(ncol)
    g, o = _pair(cfg, ncol, st)
    ref = golden(f"tc{tc}_ref_fullprec.npz")
    rows = {int(x): j for j, x in enumerate(ref["index"])}
    g.set_output_window(3, 1)
    for i in range(nout):
        out = g.run_to_output()
        assert out.step == ref["all_step"][i] and out.n_active[0] == ref["all_N_active"][i], f"tc{tc} output {i}"
        for n, floor in (("S_bu_bottom", 1e-7), ("thickness", 1e-6), ("bulk_salin", 1e-5), ("T_top", 1e-2), ("freeboard", 1e-6)):
            assert rel_err(out.sc(n)[0], ref["all_s_" + n][i], floor) <= RTOL, f"tc{tc} output {i}: {n} vs reference"
        if i in rows:
            na = int(out.n_active[0])
            for n in ["T", "psi_s", "psi_l", "S_bu", "thick"]:
                assert rel_err(out.arr(n)[:na, 0], ref["a_" + n][rows[i], :na], 1e-6) <= RTOL, f"tc{tc} output {i}: {n}"
    o.step(g.get_clock().step)
    sg, so = _check(g, o, f"tc{tc} end of run")
    assert so.sc("S_bu_bottom")[0] > cfg.S_bu_bottom and (sg.lay == sg.lay[:, :, :1]).all()


def test_flood_simple_under_heavy_snow():
    """flood_flag 3 never fires in the reference's own testcase-7 run (the freeboard stays above -5 cm), so it is driven
    here: a winter state of that run is loaded with 1.3 m of cold snow, which pushes the freeboard below neg_free and
    makes flood_simple convert snow to slush every step until the column floats again"""
    ref = golden("tc7_ref_fullprec.npz")
    p = int(np.where(ref["tf_index"] == 400)[0][0])
    cfg, _ = tcs.testcase7(1)
    o = oracle_solver(cfg, 1)
    o.set_forcing(*sheba_forcing())
    _restore_midstep(o, ref, 2 * p, cfg)
    o.step_part_b()
    st, k = o.get_state(), o.get_clock()
    st.sc("thick_snow")[:] = 1.3
    st.sc("m_snow")[:] = 1.3 * tcs.RHO_SNOW
    st.sc("H_abs_snow")[:] = -st.sc("m_snow") * (tcs.LATENT_HEAT + 2020.0 * 15.0)
    st.sc("psi_s_snow")[:] = tcs.RHO_SNOW / 920.0
    st.sc("psi_g_snow")[:] = 1.0 - tcs.RHO_SNOW / 920.0
    st.sc("T_snow")[:] = -15.0
    ncol = 8
    g = samsim_amd.hip_solver(cfg, ncol)
    o = oracle_solver(cfg, ncol)
    for s in (g, o):
        s.set_forcing(*sheba_forcing(), *tcs.ensemble_perturbation(ncol))
        s.set_state(st.replicate(ncol))
        s.set_clock(time=k.time, step=k.step, n_time_out=k.n_time_out, time_counter=k.time_counter, n_outputs=k.n_outputs)
    snow0 = float(st.sc("thick_snow")[0])
    for n in (1, 1, 10, 500):
        g.step(n)
        o.step(n)
        sg, so = _check(g, o, f"flood_simple +{n}")
    assert so.sc("thick_snow").max() < snow0 - 0.05, "flood_simple did not fire"


def test_grid_of_columns_on_all_nine_forcing_sites():
    """samsim_set_forcing_sites: 72 perturbed columns spread over the nine ERA-interim sites of the reference
    (SHEBA, North Pole, Barrow, 70N00W, 75N180E, 80N00E, 75N00W, 85N180E, 80N90E); free run from open water through freeze-up
    against the oracle (every column reads its own tables), and the snapshots of an unperturbed North Pole column against the
    reference's own run on those tables"""
    sites = ["NorthPole", "barrow", "70N00W"]
    more = ["75N180E", "80N00E", "75N00W", "85N180E", "80N90E"]
    z, zm = golden("era_sites_forcing.npz"), golden("era_sites_forcing_more.npz")
    sheba = sheba_forcing()
    tables = [np.stack([sheba[i]] + [z[f"{s}_{n}"] for s in sites] + [zm[f"{s}_{n}"] for s in more])
              for i, n in enumerate(("fl_sw", "fl_lw", "T2m", "precip"))]
    nsite = 1 + len(sites) + len(more)
    ncol = 8 * nsite
    site = (np.arange(ncol) % nsite).astype(np.int32)
    dT, ps = tcs.ensemble_perturbation(ncol)
    dT[1], ps[1] = 0.0, 1.0                               # column 1 = the North Pole member as the reference runs it
    cfg, st = tcs.testcase4(ncol)
    g, o = samsim_amd.hip_solver(cfg, ncol), oracle_solver(cfg, ncol)
    o.set_threads(NTHREADS)
    for s in (g, o):
        s.set_forcing_sites(*tables, site, dT, ps)
        s.set_state(st)
        s.set_clock()
    g.set_output_window(1, 1)
    ref = golden("tc4_northpole_ref.npz")
    for i in range(6):
        out = g.run_to_output()
        assert out.step == ref["all_step"][i] and out.n_active[0] == ref["all_N_active"][i]
        for n, floor in (("T2m", 1e-2), ("T_top", 1e-2), ("thickness", 1e-7), ("thick_snow", 1e-7), ("bulk_salin", 1e-5)):
            assert rel_err(out.sc(n)[0], ref["all_s_" + n][i], floor) <= RTOL, f"north pole output {i}: {n}"
    o.step(g.get_clock().step)
    sg, so = _check(g, o, "nine sites, day 5")
    g.step(30000)
    o.step(30000)
    sg, so = _check(g, o, "nine sites, +30000")
    T2m = so.sc("T2m")
    assert len({round(float(T2m[site == k].mean()), 3) for k in range(nsite)}) == nsite      # the sites really differ


def test_the_five_later_era_sites_free_run_against_the_reference_records():
    """SURVEY.md 8 f.4 against the reference itself: testcase 4 on the tables of 75N180E, 80N00E, 75N00W, 85N180E and 80N90E
    (input/ERA-interim/<site>-p2/), one unperturbed column per site in ONE handle (samsim_set_forcing_sites: the KShebaSites
    instantiation), free from open water; every output day of the 150 the reference was run for against its own record of that day
    (tests/golden/tc4_sites_ref.npz: scalars of all days, layer arrays on the days the fixture holds them).
    80N90E meets a freeze-up event that amplifies round-off on output day 61 (ice of 8-9 layers melting back to 6): the checker
    and its own -ffp-contract=fast build part by 4e-4 there, the other four sites stay below 2e-12 for all 150 days
    (profiles/r3_site_sensitivity.json, CPU only).  So 80N90E is held to the parity bar up to day 60 and to the size of that event
    afterwards (1e-3: a small factor over the 4e-4 to 6e-4 of that record), the other sites to the parity bar throughout.  The parity
    bar THROUGH the event (days 59 to 63 in windows of 100 steps, N_active and every layer array) and after it (one-day windows from
    the checker's state at days 70, 100 and 130) is held by tests/test_gpu_event_windows.py, which is where a thin-snow-coupling or
    regrid regression below the event's size would show."""
    from tests import background_runs
    more = background_runs.SITES
    run = background_runs.get("sites_free_run")       # started with the session's first GPU test: it has been running beside the others
    outputs = run.result()
    assert len(outputs) == 150
    z = golden("tc4_sites_ref.npz")
    rows = {s: {int(x): j for j, x in enumerate(z[f"{s}_index"])} for s in more}
    scalars = (("thickness", 1e-7), ("bulk_salin", 1e-7), ("freeboard", 1e-7), ("m_snow", 1e-5), ("thick_snow", 1e-7), ("T_snow", 1e-2),
               ("T_top", 1e-2), ("T2m", 1e-2), ("energy_stored", 1e-3), ("total_resist", 1e-7), ("grav_salt", 1e-9))
    worst = {s: 0.0 for s in more}
    worst_event = 0.0
    layer_days = 0
    for i, out in enumerate(outputs):
        for c, s in enumerate(more):
            event = s == "80N90E" and i >= 60
            tol = 1e-3 if event else RTOL
            assert out.step == z[f"{s}_all_step"][i]
            if not event:
                assert out.n_active[c] == z[f"{s}_all_N_active"][i], f"{s} output {i}: N_active {out.n_active[c]} vs {z[f'{s}_all_N_active'][i]}"
            for n, floor in scalars:
                e = rel_err(out.sc(n)[c], z[f"{s}_all_s_{n}"][i], floor)
                if not event:
                    worst[s] = max(worst[s], e)
                else:
                    worst_event = max(worst_event, e)
                assert e <= tol, f"{s} output day {i}: {n} = {out.sc(n)[c]!r} vs the reference's {z[f'{s}_all_s_{n}'][i]!r} ({e:.2e})"
            if i in rows[s] and not event:
                j, na = rows[s][i], int(out.n_active[c])
                layer_days += 1
                for n in ["T", "psi_s", "psi_l", "S_bu", "thick", "H_abs", "S_abs", "m"]:
                    floor = 1e-3 if n == "H_abs" else 1e-9
                    e = rel_err(out.arr(n)[:na, c], z[f"{s}_a_{n}"][j, :na], floor)
                    worst[s] = max(worst[s], e)
                    assert e <= RTOL, f"{s} output day {i}: layers of {n} rel err {e:.2e} vs the reference record"
    assert not run.status.any()
    assert layer_days >= 12 and out.n_active.max() >= 90
    print("five sites, free run of 150 output days: worst relative deviation from the reference's records", {k: f"{v:.1e}" for k, v in worst.items()},
          f"; 80N90E from output day 60 on: {worst_event:.1e}")
    assert max(worst.values()) <= 1e-8


VARIANTS = {"prescribe": dict(flush_flag=4, grav_flag=1, flood_flag=1, prescribe_flag=2), "flush6": dict(flush_flag=6)}


@pytest.mark.parametrize("tc,variant,nout", [(5, "prescribe", 36), (5, "flush6", 36), (7, "prescribe", 150)])
def test_flag_variants_against_reference_records(tc, variant, nout):
    """the flag sets init(5) / init(7) keep commented out (mo_init.f90:1068-1071, 1386-1390): prescribed salinity profile
    (prescribe_flag 2 with flush_flag 4, grav_flag 1, flood_flag 1) and flush4 (flush_flag 6).  Free run of one column against
    the reference's own output records (fixture) -- testcase 5 through the first quarter / third of the run (the 1 m slab melting from the top), testcase 7 from
    open water through freeze-up and the 0.15 m lower branch of the profile -- then against the oracle's state."""
    cfg, st = getattr(tcs, f"testcase{tc}")(1)
    for k, v in VARIANTS[variant].items():
        setattr(cfg, k, v)
    g = samsim_amd.hip_solver(cfg, 1)
    o = oracle_solver(cfg, 1)
    for s in (g, o):
        if tc == 7:
            s.set_forcing(*sheba_forcing())
        s.set_state(st)
        s.set_clock()
    g.set_output_window(0, 1)
    ref = golden(f"tc{tc}_{variant}_ref.npz")
    rows = {int(x): j for j, x in enumerate(ref["index"])}
    rtol = 1e-6
    for i in range(nout):
        out = g.run_to_output()
        assert out.step == ref["all_step"][i] and out.n_active[0] == ref["all_N_active"][i], f"output {i}"
        for n, floor in (("m_snow", 1e-5), ("thick_snow", 1e-7), ("T_snow", 1e-2), ("T_top", 1e-2), ("freeboard", 1e-7),
                         ("thickness", 1e-7), ("bulk_salin", 1e-5)):
            assert rel_err(out.sc(n)[0], ref["all_s_" + n][i], floor) <= rtol, f"output {i}: {n} vs reference"
        if i in rows:
            na, j = int(out.n_active[0]), rows[i]
            for n in ["T", "psi_s", "psi_l", "S_bu", "thick"]:
                assert rel_err(out.arr(n)[:na, 0], ref["a_" + n][j, :na], 1e-7) <= rtol, f"output {i}: {n} vs reference"
    assert not g.get_status()[0].any()
    o.step(g.get_clock().step)
    _check(g, o, f"tc{tc} {variant} after {nout} outputs", rtol)
    if variant == "flush6":
        assert ref["a_S_bu"][rows[max(i for i in rows if i < nout)], 1] < 1e-3           # flush4 is rinsing the upper layers
    if tc == 7:
        assert ref["all_N_active"][nout - 1] > 15     # past the 0.15 m the lower branch of the profile spans


NOUT_TC50 = 2   # step 1 and day 30 (testcase 50 is outside SURVEY.md section 8: kept short; the oracle test runs six records)


def test_tc50_default_flags_against_reference_records():
    """init(50): the reference's default flag set on 70 layers from 5 mm of sea water; the HIP path's first output points
    (step 1 and day 30: open water) against the reference's own records, then the state
    against the oracle"""
    cfg, st = tcs.testcase50(1)
    g = samsim_amd.hip_solver(cfg, 1)
    o = oracle_solver(cfg, 1)
    for s in (g, o):
        s.set_state(st)
        s.set_clock()
    g.set_output_window(0, 1)
    ref = golden("tc50_ref_fullprec.npz")
    for i in range(NOUT_TC50):
        out = g.run_to_output()
        assert out.step == ref["step"][i] and out.n_active[0] == ref["N_active"][i], f"output {i}"
        na = int(out.n_active[0])
        for n in ["T", "psi_s", "psi_l", "S_bu", "thick"]:
            assert rel_err(out.arr(n)[:na, 0], ref["a_" + n][i, :na], 1e-7) <= RTOL, f"output {i}: {n} vs reference"
        for n, floor in (("T_top", 1e-2), ("freeboard", 1e-7), ("thickness", 1e-7)):
            assert rel_err(out.sc(n)[0], ref["s_" + n][i], floor) <= RTOL, f"output {i}: {n} vs reference"
    assert not g.get_status()[0].any()
    o.step(g.get_clock().step)
    _check(g, o, "tc50 day 30")
