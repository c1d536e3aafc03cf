"""HIP path against the REFERENCE's own records, without the oracle's trajectory in between (BASELINE cfg2 / cfg3 as
SURVEY.md section 8d specifies them).

cfg3 -- SHEBA / testcase 4: the flang-built reference dumps its full state inside `output` at every output day.  For days
sampled through open water, freeze-up, the growth season (tests/golden/tc4_tf_growth_ref.npz) and the melt seasons
(tf_* block of tc4_ref_fullprec.npz) the HIP path is started from the reference's day-D state and must reproduce the
reference's day-D+1 record (8641 steps later) at the parity bar.  The dump is taken in mid-step (mo_grotz.f90:363): the
checker finishes that one step (step_part_b), everything after it runs on the GPU.

cfg2 -- testcase 1 on 65 536 identical columns, the full 259 200-step run from the one-layer initial state: every column
bitwise equal to column 0, column 0 within 1e-6 of all 72 reference records."""
import numpy as np
import pytest

import samsim_amd
from samsim_amd import testcases as tcs
from tests.helpers import RTOL, golden, rel_err, sheba_forcing
from tests.oracle_lib import oracle_solver
from tests.test_oracle_golden import _restore_midstep

pytestmark = pytest.mark.gpu


def _windows():
    out = []
    for name in ("tc4_tf_growth_ref.npz", "tc4_ref_fullprec.npz"):
        try:
            ref = golden(name)
        except FileNotFoundError:
            continue
        out += [(name, p, int(day)) for p, day in enumerate(ref["tf_days"])]
    return out


def test_sheba_windows_started_from_the_reference_records():
    cfg, _ = tcs.testcase4(1)
    o = oracle_solver(cfg, 1)
    g = samsim_amd.hip_solver(cfg, 1)
    for s in (o, g):
        s.set_forcing(*sheba_forcing())
    g.set_output_window(0, 1)
    windows = _windows()
    assert len(windows) >= 12 and min(d for _, _, d in windows) <= 5 and max(d for _, _, d in windows) >= 700
    worst = 0.0
    for name, p, day in windows:
        ref = golden(name)
        _restore_midstep(o, ref, 2 * p, cfg)
        o.step_part_b()                                    # the rest of the step the reference was dumped in
        k = o.get_clock()
        g.set_state(o.get_state())
        g.set_clock(time=k.time, step=k.step, n_time_out=k.n_time_out, time_counter=k.time_counter, n_outputs=k.n_outputs)
        out = g.run_to_output()                            # 8640 more steps on the GPU, then the output point of day D+1
        j = 2 * p + 1
        assert not g.get_status()[0].any(), f"day {day}: STOP code {g.get_status()[0]}"
        assert out.step == ref["tf_step"][j], (day, out.step, ref["tf_step"][j])
        assert out.n_active[0] == ref["tf_N_active"][j], f"day {day}: N_active {out.n_active[0]} vs {ref['tf_N_active'][j]}"
        na = int(out.n_active[0])
        # Day 347 is the day a threshold event flips in the reference itself: its own -O2 build and its FMA build part ways there
        # by more than 1e-6 within one output interval (measured).  Round-off level differences (observed
        # elsewhere: <= 1e-11) decide which side of the threshold a step lands on, so that one window is held to the size of
        # the event, every other window to the parity bar.  The same 8 641 steps at the parity bar, in ten-step windows restarted from
        # the checker: tests/test_gpu_event_windows.py::test_reference_day_347_record_to_its_day_348_record_in_ten_step_windows (and
        # the 16 perturbed columns through days 346 to 349 beside it).
        tol = 2e-2 if day == 347 else RTOL
        for n in ["T", "psi_s", "psi_l", "S_bu", "thick", "H_abs", "S_abs", "m"]:
            floor = 1e-3 if n == "H_abs" else 1e-7
            e = rel_err(out.arr(n)[:na, 0], ref["tf_a_" + n][j, :na], floor)
            if day != 347:
                worst = max(worst, e)
            assert e <= tol, f"day {day}->{day + 1}: {n} rel err {e:.2e} vs the reference record"
        for n, floor in (("m_snow", 1e-5), ("thick_snow", 1e-7), ("T_snow", 1e-2), ("T_top", 1e-2), ("freeboard", 1e-7),
                         ("thickness", 1e-7), ("bulk_salin", 1e-7)):
            e = rel_err(out.sc(n)[0], ref["tf_s_" + n][j], floor)
            assert e <= tol, f"day {day}->{day + 1}: {n} rel err {e:.2e} vs the reference record"
    print(f"worst relative deviation from the reference records over {len(windows) - 1} windows: {worst:.2e}")
    assert worst <= 1e-9   # observed <= 1e-11: far inside the bar


def test_sheba_free_run_from_open_water_against_the_reference_records():
    """cfg3 as SURVEY.md section 8(d) words it: the unperturbed SHEBA column FREE from open water -- no restart from anybody's state
    in between -- through freeze-up, first snow and the growth season to day 300 (2.6 million steps), every output day against the
    flang-built reference's own record of that day: the scalars of all 300 days (tc4_ref_fullprec.npz all_s_*), the layer arrays on
    the days the fixture holds them (day_index).  The reference's -O2 and FMA builds stay within 2e-12 of each other over this
    span; the first melt season (day 347 on) is where free runs part, and is covered by the windows above."""
    from tests import background_runs
    ref = golden("tc4_ref_fullprec.npz")
    run = background_runs.get("sheba_free_run")       # started with the session's first GPU test: it has been running beside the others
    outputs = run.result()
    layer_days = {int(d): j for j, d in enumerate(ref["day_index"])}      # output number (1-based) -> row of the a_* block
    last, worst, worst_at = 301, 0.0, None
    scalars = (("thickness", 1e-7), ("bulk_salin", 1e-7), ("freeboard", 1e-7), ("energy_stored", 1e-3), ("freshwater", 1e-7),
               ("total_resist", 1e-7), ("m_snow", 1e-5), ("thick_snow", 1e-7), ("H_abs_snow", 1.0), ("T_snow", 1e-2), ("T_top", 1e-2),
               ("T2m", 1e-2), ("fl_q_bottom", 1e-7), ("albedo", 1e-7), ("fl_sw", 1e-7), ("fl_lw", 1e-7), ("grav_drain", 1e-12),
               ("grav_salt", 1e-9), ("grav_temp", 1e-6), ("melt_out1", 1e-9), ("melt_out2", 1e-9), ("melt_out3", 1e-9))
    seen_layers = 0
    assert len(outputs) == last
    for i, out in enumerate(outputs):                                      # output i is the reference's output day i (0-based)
        assert out.step == ref["all_step"][i], (i, out.step, ref["all_step"][i])
        assert out.n_active[0] == ref["all_N_active"][i], f"output {i}: N_active {out.n_active[0]} vs {ref['all_N_active'][i]}"
        for n, floor in scalars:
            e = rel_err(out.sc(n)[0], ref["all_s_" + n][i], floor)
            if e > worst:
                worst, worst_at = e, (i, n)
            assert e <= RTOL, f"free run, output day {i}: {n} = {out.sc(n)[0]!r} vs the reference's {ref['all_s_' + n][i]!r} ({e:.2e})"
        if i + 1 in layer_days:
            j, na = layer_days[i + 1], int(out.n_active[0])
            seen_layers += 1
            for n in ["T", "psi_s", "psi_l", "psi_g", "S_bu", "thick", "H_abs", "S_abs", "m", "ray"]:
                floor = {"H_abs": 1e-3, "psi_g": 1e-6, "ray": 1e-6}.get(n, 1e-9)
                hi = na - 1 if n == "ray" else na
                e = rel_err(out.arr(n)[:hi, 0], ref["a_" + n][j, :hi], floor)
                if e > worst:
                    worst, worst_at = e, (i, n)
                assert e <= RTOL, f"free run, output day {i}: layers of {n} rel err {e:.2e} vs the reference record"
    assert not run.status.any()
    assert seen_layers >= 15 and out.n_active[0] == 100                    # layer records through freeze-up and growth were compared
    print(f"free run to output day {last - 1}: worst relative deviation from the reference's records {worst:.2e} at {worst_at}")
    assert worst <= 1e-8   # (the bar is 1e-6; a free run that stays this close did not meet an amplifying event)


def test_cfg2_full_run_65536_columns_against_all_72_reference_records():
    ref = golden("tc1_ref_fullprec.npz")
    ncol = 65536
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    g.set_output_window(0, 1)
    total = tcs.i_time(cfg)
    assert total == 259200
    done, i = 0, 0
    while done < total:
        n = min(g.steps_to_output(), total - done)
        g.step(n)
        done += n
        if g.steps_to_output() == cfg.i_time_out + 1 or done == 1:      # an output point was just passed
            out = g.get_output()
            assert out.step == ref["step"][i] and out.n_active[0] == ref["N_active"][i], f"output {i}"
            na = int(out.n_active[0])
            for n in ["T", "psi_s", "psi_l", "S_bu", "thick", "H_abs", "S_abs", "m"]:
                floor = 1e-3 if n == "H_abs" else 1e-9
                e = rel_err(out.arr(n)[:na, 0], ref["a_" + n][i, :na], floor)
                assert e <= RTOL, f"output {i}: {n} rel err {e:.2e} vs the reference record"
            for n in ["freeboard", "thickness", "bulk_salin", "energy_stored", "grav_drain", "grav_salt"]:
                assert rel_err(out.sc(n)[0], ref["s_" + n][i], 1e-9) <= RTOL, f"output {i}: scalar {n}"
            i += 1
    assert i == 72
    assert not g.get_status()[0].any()
    s = g.get_state()
    assert s.n_active.min() == s.n_active.max()
    for a in range(9):   # prognostic arrays, T, phi, psi_s, psi_l, psi_g: every column equals column 0 bit for bit
        assert (s.lay[a] == s.lay[a][:, :1]).all(), f"array {a}: replicated columns diverged"
    assert (s.scal[:20] == s.scal[:20, :1]).all()


@pytest.mark.parametrize("name", ["harmonic1", "freeboard_snow1", "snow_flush0", "bottom2"])
def test_unshipped_flag_values_from_the_reference_records(name):
    """harmonic_flag 1, freeboard_snow_flag 1, snow_flush_flag 0, bottom_flag 2 (run-time-flag instantiation of the kernel): from
    the reference's day-D state of a testcase-4 run with that flag overridden to its day-D+1 record, days through growth and
    the first melt season (the oracle is bitwise on the same fixtures, tests/test_oracle_golden.py)"""
    from tests.test_oracle_golden import FLAG_VARIANTS
    ref = golden(f"tc4_flag_{name}_ref.npz")
    cfg, _ = tcs.testcase4(1)
    for k, v in FLAG_VARIANTS[name].items():
        setattr(cfg, k, v)
    o = oracle_solver(cfg, 1)
    g = samsim_amd.hip_solver(cfg, 1)
    for s in (o, g):
        s.set_forcing(*sheba_forcing())
    g.set_output_window(0, 1)
    for p, day in enumerate(ref["tf_days"]):
        if p % 2:            # every other pair (days 66, 120, 345, 358, 380): the checker covers all ten on the CPU
            continue
        _restore_midstep(o, ref, 2 * p, cfg)
        o.step_part_b()
        k = o.get_clock()
        g.set_state(o.get_state())
        g.set_clock(time=k.time, step=k.step, n_time_out=k.n_time_out, time_counter=k.time_counter, n_outputs=k.n_outputs)
        out = g.run_to_output()
        j = 2 * p + 1
        assert not g.get_status()[0].any(), f"{name} day {day}: STOP code {g.get_status()[0]}"
        assert out.step == ref["tf_step"][j] and out.n_active[0] == ref["tf_N_active"][j], f"{name} day {day}"
        na = int(out.n_active[0])
        for n in ["T", "psi_s", "psi_l", "S_bu", "thick", "H_abs", "S_abs", "m"]:
            floor = 1e-3 if n == "H_abs" else 1e-7
            e = rel_err(out.arr(n)[:na, 0], ref["tf_a_" + n][j, :na], floor)
            assert e <= RTOL, f"{name} day {day}->{day + 1}: {n} rel err {e:.2e} vs the reference record"
        for n, floor in (("m_snow", 1e-5), ("thick_snow", 1e-7), ("T_snow", 1e-2), ("T_top", 1e-2), ("freeboard", 1e-7),
                         ("thickness", 1e-7)):
            e = rel_err(out.sc(n)[0], ref["tf_s_" + n][j], floor)
            assert e <= RTOL, f"{name} day {day}->{day + 1}: {n} rel err {e:.2e} vs the reference record"
