"""The start states of the tiled event windows (tests/golden/event_*.npz, written by tests/golden/make_event_fixtures.py) are the
checker's own: restarted from the first state of a file, today's checker arrives at the later states the file holds, byte for byte.
No GPU; a few seconds of CPU time.  A change of the checker, of the forcing fixtures or of the set-up in tests/event_windows.py that
moves these trajectories fails here, before the GPU tests tile windows from states nobody can regenerate."""
import pytest

from tests import event_windows as ew
from tests.helpers import golden, load_checkpoint


def _replay(o, name, pairs):
    """pairs: (label of the state to start from or None for the file's checkpoint, label to arrive at)"""
    z = golden(name)
    for a, b in pairs:
        st, clock = load_checkpoint(name) if a is None else ew.later_state(z, a)
        want, kwant = ew.later_state(z, b)
        ew.load(o, st, clock)
        o.step(kwant["step"] - clock["step"])
        assert not o.get_status()[0].any()
        assert ew.clock_of(o) == kwant, f"{name}: clock at {b}"
        assert ew.same_bytes(o.get_state(), want), f"{name}: the checker's state at {b} is not the stored one"


def test_ocean_grid_day_67_replays_to_the_same_bytes():
    cfg, _, o = ew.ocean_solver(ew.make_oracle)
    st, clock = load_checkpoint(ew.FIXTURES["ocean"])
    assert clock["step"] == ew.OCEAN_STEP0 == 578947 and st.ncol == 64
    _replay(o, ew.FIXTURES["ocean"], [(None, "end")])
    end, kend = ew.later_state(golden(ew.FIXTURES["ocean"]), "end")
    assert kend["step"] == 587587
    # the span holds the event: first snow below thick_min at the start, above it at the end
    thin = (st.sc("thick_snow") > 0) & (st.sc("thick_snow") < cfg.thick_min)
    assert thin.sum() == 47 and (end.sc("thick_snow")[thin] > cfg.thick_min).sum() == 45
    assert end.n_active.min() > st.n_active.max()


@pytest.mark.parametrize("day", ew.SHEBA_DAYS)
def test_sheba_melt_onset_days_replay_to_the_same_bytes(day):
    _, o = ew.sheba_solver(ew.make_oracle)
    name = ew.FIXTURES[f"sheba{day}"]
    st, clock = load_checkpoint(name)
    assert clock["step"] == day * ew.DAY and st.ncol == 16 and (day != 346 or clock["step"] == 2989786)
    _replay(o, name, [(None, "end")])
    if day + 1 in ew.SHEBA_DAYS:     # the files chain: this one's end is the next one's start
        nxt, knxt = load_checkpoint(ew.FIXTURES[f"sheba{day + 1}"])
        end, kend = ew.later_state(golden(name), "end")
        assert ew.same_bytes(end, nxt) and kend == knxt


def test_five_sites_day_59_replays_to_the_same_bytes():
    _, _, o = ew.sites_solver(ew.make_oracle)
    name = ew.FIXTURES["sites"]
    st, clock = load_checkpoint(name)
    assert clock["step"] == ew.SITES_STEP0 == 509819 and st.ncol == 5
    _replay(o, name, [(None, "end")] + [(f"day{d}", f"day{d + 1}") for d in ew.SITES_LATE_DAYS])
    end, kend = ew.later_state(golden(name), "end")
    assert kend["step"] == 544383
    assert st.n_active[4] == 10 and end.n_active[4] == 6          # 80N90E's event: its young ice melts back inside the span
