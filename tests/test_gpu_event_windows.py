"""The HIP path at the parity bar THROUGH the events that amplify round-off (tests/event_windows.py): windows of ten steps, each
restarted from the checker's state, laid end to end over

  * the ocean grid's day 67 (first snow growing through thick_min on young ice; sites / ocean instantiation of the kernel),
  * the SHEBA melt onset, days 346 to 349 (16 perturbed columns), and the reference's own day-347 state to its day-348 record,
  * the melting back of 80N90E's young ice, days 59 to 63 of the five later ERA-interim sites (windows of 100 steps), and one-day
    windows of those sites at days 70, 100 and 130,

which the older tests hold to the size of the event (test_per_column_ocean_grid_of_columns: 4e-3 at day 67;
test_sheba_windows_started_from_the_reference_records: 2e-2 at day 347; the 80N90E free run: 1e-3 and no N_active from day 60 on).
Every assert of `tile` is at RTOL = 1e-6 with STOP codes and N_active exact.  The start states are committed checker states
(tests/golden/event_*.npz; tests/test_event_fixtures_host.py replays them on the CPU).

SECONDARY BOUND.  On top of the bar each span asserts 1 000 times what the checker's own -ffp-contract=fast build deviates by in the
same windows (tools/event_window_sensitivity.py, CPU only; profiles/r25_event_windows.json): the HIP path re-associates more than
FMA contraction does (shared reciprocals, Horner forms), three decades of margin cover that, and a drift that has eaten them is
still two to five decades inside the bar when it fails here.  None of these bounds is derived from the HIP path's own output.
The one span without it is the five sites' days 59 to 63: its windows are 100 steps long, long enough for 80N90E's event to amplify
(the ocean grid's 100-step windows reach 2e-4 between the two CPU builds), the FMA build's perturbation happens not to be picked
up there (4.5e-14) and the HIP path's is, in one window of 346 (1.1e-9, steps 518 919 to 519 019; every other window below 1e-11):
1 000 x 4.5e-14 is no envelope of that event, so the span is held to the bar alone, as measured in profiles/r25_event_windows.json.

TANK EXPERIMENTS.  test_gpu_secondary.py::test_tank_experiments asserted 2e-6 from the first round on.  Measured over the whole free
runs of testcases 2, 6 (all 156 outputs), 9, 33 and 34 the HIP path stays within 3.1e-12 of the checker in every compared quantity
at every output and within 1.2e-13 of the reference's records in the scalars (profiles/r25_event_windows.json, "tank"): nothing ever
needed the factor two.  The ten-step windows below hold the tank path (boundflux_flag 3, tank_flag 2, the S_bu_bottom budget) to the
bar over the output interval in which each run deviates most."""
import numpy as np
import pytest

from samsim_amd import testcases as tcs
from tests.oracle_lib import oracle_solver
from tests import event_windows as ew
from tests.helpers import RTOL, golden, load_checkpoint, rel_err
from tests.test_oracle_golden import _restore_midstep

pytestmark = pytest.mark.gpu

# checker vs its FMA build, worst window of the span (CPU)            x 1 000
FMA = {"ocean": 6.9e-13, 346: 4.3e-14, 347: 9.6e-14, 348: 5.4e-12, "sites": 4.5e-14, "sites_late": 1.2e-13,
       "tank": 1.5e-15}   # tank: the same three intervals in the same windows: 1.0e-15, 1.5e-15, 1.4e-16
SECONDARY = {"ocean": 1e-9, 346: 1e-10, 347: 1e-10, 348: 1e-8, "sites": None, "sites_late": 1.2e-10, "tank": 1.5e-12}


def _report(what, worst, key):
    w = np.array(worst)
    bound = SECONDARY[key]
    print(f"{what}: {len(w)} windows, worst {w.max():.2e} (window {int(w.argmax())}), checker vs FMA {FMA[key]:.1e}, secondary bound {bound}")
    assert w.max() <= RTOL
    if bound is not None:
        assert w.max() <= bound, f"{what}: worst window {w.max():.2e} above 1 000 x the checker-vs-FMA figure ({bound:.1e})"


def test_ocean_grid_day_67_first_snow_through_thick_min():
    """8 640 steps from step 578 947 in 864 windows of ten steps, 64 columns over 64 oceans.  What the span holds (the generator's CPU
    run): 47 columns start with a snow cover below thick_min, 45 of them end above it; N_active 5..8 at the start, 9..12 at the end."""
    cfg, _, o = ew.ocean_solver(ew.make_oracle)
    _, _, g = ew.ocean_solver(ew.make_hip)
    st, clock = load_checkpoint(ew.FIXTURES["ocean"])
    ew.load(o, st, clock)
    seen = set()
    worst = ew.tile(g, o, ew.OCEAN_STEPS, 10, "ocean grid, day 67", seen=seen)
    assert len(worst) == 864 and o.get_clock().step == 587587
    end = o.get_state()
    assert ew.same_bytes(end, ew.later_state(golden(ew.FIXTURES["ocean"]), "end")[0])      # the checker walked the committed trajectory
    thin = (st.sc("thick_snow") > 0) & (st.sc("thick_snow") < cfg.thick_min)
    assert thin.any() and (end.sc("thick_snow")[thin] > cfg.thick_min).any()                # the event is inside the span
    assert (end.n_active != st.n_active).any() and len(seen) >= 6                            # and N_active changes
    _report("ocean grid, day 67", worst, "ocean")


@pytest.mark.parametrize("day", ew.SHEBA_DAYS)
def test_sheba_melt_onset_one_day_in_ten_step_windows(day):
    """one output interval (8 641 steps: 864 windows of ten steps and one of a single step) of 16 perturbed SHEBA columns.  What the
    days hold (the generator's CPU run): N_active is 100 in every column throughout -- the top melt regrids of these days thin the
    middle layers and leave the count alone -- T_top sits at 0 degC at every day boundary, and the snow goes and comes back: all 16
    columns carry snow at day 346 (up to 17.7 mm), one at days 347 and 348 (35 and 27 micrometres), seven at day 349 (up to 1.5 mm)."""
    _, o = ew.sheba_solver(ew.make_oracle)
    _, g = ew.sheba_solver(ew.make_hip)
    name = ew.FIXTURES[f"sheba{day}"]
    st, clock = load_checkpoint(name)
    ew.load(o, st, clock)
    seen = set()
    worst = ew.tile(g, o, ew.DAY, 10, f"SHEBA, day {day}", seen=seen)
    assert len(worst) == 865 and o.get_clock().step == (day + 1) * ew.DAY
    end = o.get_state()
    assert ew.same_bytes(end, ew.later_state(golden(name), "end")[0])
    assert seen == {100}
    snow = {346: (16, 1), 347: (1, 1), 348: (1, 7)}[day]
    assert (int((st.sc("thick_snow") > 0).sum()), int((end.sc("thick_snow") > 0).sum())) == snow
    assert st.sc("thick_snow").max() < 0.02 and np.all(st.sc("T_top") == 0.0) and np.all(end.sc("T_top") == 0.0)
    _report(f"SHEBA, day {day}", worst, day)


def test_reference_day_347_record_to_its_day_348_record_in_ten_step_windows():
    """the window test_sheba_windows_started_from_the_reference_records holds to 2e-2: the reference's own mid-step state of day 347,
    its step finished by the checker, then 8 641 steps to the output point of day 348 in 865 windows at the bar (the reference counts
    its output days from 1: this is step 2 989 787 to 2 998 428, the span of the day-346 case above on the unperturbed column).  At the end the
    CHECKER's snapshot against the reference's record at 2e-2: the size of the event between two builds of the reference, which says
    that the tiled trajectory is the reference's, and nothing about the HIP path."""
    ref = golden("tc4_ref_fullprec.npz")
    p = int(np.where(ref["tf_days"] == 347)[0][0])
    cfg, o = ew.sheba_solver(ew.make_oracle, 1)
    _, g = ew.sheba_solver(ew.make_hip, 1)
    o.set_output_window(0, 1)
    _restore_midstep(o, ref, 2 * p, cfg)
    o.step_part_b()
    nsteps = o.steps_to_output()
    assert nsteps == 8641
    worst = ew.tile(g, o, nsteps, 10, "reference day 347 -> 348")
    assert len(worst) == 865
    out, j = o.get_output(), 2 * p + 1
    assert out.step == ref["tf_step"][j] and out.n_active[0] == ref["tf_N_active"][j]
    na = int(out.n_active[0])
    for n in ["T", "psi_s", "psi_l", "S_bu", "thick", "H_abs", "S_abs", "m"]:
        floor = 1e-3 if n == "H_abs" else 1e-7
        assert rel_err(out.arr(n)[:na, 0], ref["tf_a_" + n][j, :na], floor) <= 2e-2, f"checker vs the reference's day-348 record: {n}"
    for n, floor in (("m_snow", 1e-5), ("thick_snow", 1e-7), ("T_snow", 1e-2), ("T_top", 1e-2), ("freeboard", 1e-7), ("thickness", 1e-7),
                     ("bulk_salin", 1e-7)):
        assert rel_err(out.sc(n)[0], ref["tf_s_" + n][j], floor) <= 2e-2, f"checker vs the reference's day-348 record: {n}"
    _report("reference day 347 -> 348", worst, 346)


def test_five_sites_days_59_to_63_in_hundred_step_windows():
    """steps 509 819 to 544 383 of the five later ERA-interim sites in one handle: 346 windows (345 of 100 steps, one of 64), N_active
    and every array at the bar.  The span holds 80N90E's event: its ice of 10 layers melts back to 6 (column 4)."""
    _, _, o = ew.sites_solver(ew.make_oracle)
    _, _, g = ew.sites_solver(ew.make_hip)
    name = ew.FIXTURES["sites"]
    st, clock = load_checkpoint(name)
    ew.load(o, st, clock)
    seen = set()
    worst = ew.tile(g, o, ew.SITES_STEPS, 100, "five sites, days 59 to 63", seen=seen)
    assert len(worst) == 346 and o.get_clock().step == 544383
    end = o.get_state()
    assert ew.same_bytes(end, ew.later_state(golden(name), "end")[0])
    assert st.n_active[4] == 10 and end.n_active[4] == 6 and len(seen) >= 10
    _report("five sites, days 59 to 63", worst, "sites")


@pytest.mark.parametrize("day", ew.SITES_LATE_DAYS)
def test_five_sites_one_day_windows_after_the_event(day):
    """80N90E after its event (and the other four sites beside it): one output interval from the checker's state at days 70, 100
    and 130 in ONE window, N_active and every array at the bar.  The checker's FMA build stays within 1.2e-13 of it over these
    one-day windows (7.5e-14, 1.2e-13, 1.0e-13), so they need no shortening."""
    _, _, o = ew.sites_solver(ew.make_oracle)
    _, _, g = ew.sites_solver(ew.make_hip)
    z = golden(ew.FIXTURES["sites"])
    ew.load(o, *ew.later_state(z, f"day{day}"))
    worst = ew.tile(g, o, ew.DAY, ew.DAY, f"five sites, day {day}")
    assert len(worst) == 1 and ew.same_bytes(o.get_state(), ew.later_state(z, f"day{day + 1}")[0])
    _report(f"five sites, day {day}", worst, "sites_late")


@pytest.mark.parametrize("tc,output", [(2, 99), (9, 54), (33, 31)])
def test_tank_budget_in_ten_step_windows(tc, output):
    """boundflux_flag 3 / tank_flag 2: the output interval that ends in the output at which the HIP path's free run deviates most from
    the checker (testcase 2: psi_s at output 99, 3.0e-12; testcase 9: output 54, 2.7e-13; testcase 33: output 31, 9.4e-13), from the
    checker's state at the output before it, in ten-step windows: every array and scalar of the state, S_bu_bottom among them, at
    the bar, then the two output snapshots.  The checker gets to the start on the CPU (a second or less)."""
    cfg, st = getattr(tcs, f"testcase{tc}")(1)
    ref = golden(f"tc{tc}_ref_fullprec.npz")
    o, g = oracle_solver(cfg, 1), ew.make_hip(cfg, 1)
    for s in (o, g):
        s.set_output_window(0, 1)
    ew.load(o, st, dict(time=0.0, step=0, n_time_out=0, time_counter=1, n_outputs=0))
    for _ in range(output):
        o.run_to_output()
    assert o.get_clock().step == ref["all_step"][output - 1]
    nsteps = int(ref["all_step"][output] - ref["all_step"][output - 1])
    salt0 = float(o.get_state().sc("S_bu_bottom")[0])
    worst = ew.tile(g, o, nsteps, 10, f"tc{tc}, interval to output {output}")
    og, oo = g.get_output(), o.get_output()
    assert og.step == oo.step == ref["all_step"][output] and og.n_active[0] == oo.n_active[0] == ref["all_N_active"][output]
    for n, floor in (("S_bu_bottom", 1e-7), ("thickness", 1e-6), ("bulk_salin", 1e-5), ("T_top", 1e-2), ("freeboard", 1e-6)):
        assert rel_err(og.sc(n)[0], oo.sc(n)[0], floor) <= RTOL, f"tc{tc} output {output}: {n}"
    assert salt0 > cfg.S_bu_bottom and oo.n_active[0] > 1            # ice over a tank that has grown saltier
    _report(f"tc{tc}, interval to output {output}", worst, "tank")
