"""The crafted wave of tests/newton_seeds.py on the CPU: in the first step every class of getT's loop occurs among the lanes of the
wave in ONE layer (so that the GPU test cannot pass on a wave whose lanes all agree), the evaluation counts inside the wave span at
least 1 to 6, and the CPU oracle runs the 50 steps without a STOP in any column.  The seed of the jumps' sizes is chosen here: a seed
the oracle stops on is replaced (newton_seeds.SEEDS_TRIED), not excused.  The melt-season wave of the WARM instance is not crafted;
what is checked of it is that a column flushes within the 50 steps, which is what sends its wave through getT_chain<true> in the
lite up sweep."""
import numpy as np

from tests import newton_seeds as ns
from tests.helpers import sheba_forcing
from tests.oracle_lib import oracle_solver


def test_every_class_of_the_loop_meets_in_one_layer(capsys):
    cfg, st, _ = ns.crafted_wave()
    assert st.n_active.min() == 2 and st.n_active.max() == ns.NLAYER
    evals, flags = ns.sweep(cfg, st)
    k = ns.FEATURE_LAYERS[0] - 1
    lanes = {c: [i for i in range(ns.WAVE) if ns.lane_class(i) == c and evals[k, i] >= 0] for c in ns.CLASSES}
    row = [(i, ns.lane_class(i), int(evals[k, i]), sorted(flags[k][i])) for i in range(ns.WAVE)]
    with capsys.disabled():
        print("\nlayer %d of the first sweep: (lane, class, evaluations, flags)" % (k + 1))
        for r in row:
            print("  %2d %-5s %3d %s" % r)
    # the first evaluation already holds
    assert any(evals[k, i] == 1 and not flags[k][i] for i in lanes["iso"])
    # many evaluations
    assert any(evals[k, i] >= 6 for i in lanes["jump"])
    # odd from the start: fresh ice, pure brine
    assert any("fresh" in flags[k][i] for i in lanes["odd"]) and any("brine" in flags[k][i] for i in lanes["odd"])
    # the iterate leaves (-200, 0)
    assert any("leave" in flags[k][i] for i in lanes["leave"])
    # the guess has a liquidus salinity under 1e-4
    assert any("tiny" in flags[k][i] for i in lanes["tiny"])
    # lanes that sit the layer out
    assert (evals[k] == -1).any()
    mushy = evals[k][evals[k] > 0]
    assert mushy.min() == 1 and mushy.max() >= 6, "the evaluation counts inside the wave span at least 1 to 6"
    assert not any("stop99" in f for r in flags for f in r)
    # every feature layer of a column long enough holds its feature
    for k0 in ns.FEATURE_LAYERS:
        assert {"fresh", "brine", "leave", "tiny"} <= set().union(*flags[k0 - 1]), k0


def test_the_oracle_runs_the_crafted_wave_without_a_stop():
    cfg, st, clock = ns.crafted_wave()
    o = oracle_solver(cfg, ns.WAVE)
    o.set_threads(1)
    o.set_forcing(*sheba_forcing(), None, None)
    o.set_state(st)
    o.set_clock(**clock)
    o.set_output_window(0, 0)
    o.step(ns.NSTEPS)
    status = o.get_status()[0]
    end = o.get_state()
    o.close()
    assert not status.any(), f"STOP codes {np.unique(status)} in columns {np.nonzero(status)[0]}"
    # the lanes still disagree at the end: the later steps (the fused up sweep) meet the classes too
    evals, flags = ns.sweep(cfg, end)
    seen = set().union(*[f for r in flags for f in r])
    assert {"fresh", "brine", "leave"} <= seen and evals.max() >= 6, (seen, evals.max())


def flushed(st):
    """the condition under which the step that left `st` behind ran flush3 (flush_flag 5, mo_grotz.f90:715-724), read off the state"""
    return (st.sc("melt_thick") > 1.0e-12) & (st.sc("freeboard") > 0.001) & (st.n_active > 2)


def test_a_column_of_the_melt_wave_flushes():
    cfg, st, clock, dT2m, precip_scale = ns.warm_wave()
    assert cfg.flush_flag == 5
    o = oracle_solver(cfg, ns.WAVE)
    o.set_threads(1)
    o.set_forcing(*sheba_forcing(), dT2m, precip_scale)
    o.set_state(st)
    o.set_clock(**clock)
    o.set_output_window(0, 0)
    any_flush = np.zeros(ns.WAVE, dtype=bool)
    for _ in range(ns.NSTEPS - 1):      # a flush in the last step changes no sweep of the run
        o.step(1)
        any_flush |= flushed(o.get_state())
    o.step(1)
    status = o.get_status()[0]
    o.close()
    assert not status.any()
    assert any_flush.any(), "no column of the wave flushes within the 50 steps"
