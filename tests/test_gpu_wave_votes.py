"""The fused up sweep decides two things for a whole wave without the arithmetic behind them (tests/wave_votes.py): whether a row of the
Rayleigh-number array is stored (a division-free bound instead of the number) and whether getT's pure-brine test can fail in any
lane (two compares instead of the liquidus cubic).  What a column gets must not depend on either: not on the lanes beside it, not on
where a launch ends (the last step of a launch stores every row and takes no bound).

Handles of 64 and 70 columns x 80 layers (and one of 64 x 64 copies), at most 50 steps:
  bench     the first 64 members of the bench ensemble (day 200): rows on both sides of ray_crit, 3.6 % of the lane-rows within 1 %
            of it (tests/test_wave_votes_host.py prints the shares)
  crafted   tests/newton_seeds.py: fresh ice, pure brine and the other odd lanes of getT's loop in one layer, N_active 2..80
each against the CPU oracle at the project's bar (1e-6 relative), each column bitwise against a wave of 64 copies of itself, the
70-column handle (six lanes of the last wave active) bitwise against the 64-column one, and 24 steps bitwise as launches of 24,
7 + 17 and 24 x 1.
  edge      the bench wave with ONE lane changed in one layer to stand on either side of the shortcut's two limits (S_bu 39.9 / 40.1,
            H/c_l -2.9 / -3.1; and pure brine of S_bu 55 at -3.1), its neighbours mushy: against the oracle, and the other 63 columns bitwise against the wave without
            that lane."""
import functools
import os

import numpy as np
import pytest

import samsim_amd
from samsim_amd import testcases as tcs
from samsim_amd.capi import State
from tests import newton_seeds as ns
from tests.helpers import RTOL, assert_state_close, golden, sheba_forcing
from tests.oracle_lib import oracle_solver

pytestmark = pytest.mark.gpu

NTHREADS = min(16, len(os.sched_getaffinity(0)))
WHICH = ["bench", "crafted"]
BITWISE = ["H_abs", "S_abs", "m", "thick", "T", "phi", "psi_s", "psi_l", "psi_g", "S_bu"]
NSTEPS, NCUT = 50, 24
EDGE_LANE, EDGE_LAYER = 17, 30                       # 0-based lane, 1-based layer
# (S_bu, H / c_l): the first alone takes the shortcut; the last is pure brine colder than -3 C (S_br(-3.1) = 53.1 < 55), which a
# shortcut with a laxer salinity limit would call mushy
EDGES = [(39.9, -3.1), (40.1, -3.1), (39.9, -2.9), (40.1, -2.9), (55.0, -3.1)]


@functools.lru_cache(maxsize=None)
def wave(which):
    """(cfg, State, clock, dT2m, precip_scale)"""
    if which == "crafted":
        return ns.crafted_wave() + (None, None)
    z = golden("sheba_ensemble_80.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    st = State(np.ascontiguousarray(z["lay"][:4, :, :ns.WAVE]), np.ascontiguousarray(z["scal"][:, :ns.WAVE]),
               np.ascontiguousarray(z["n_active"][:ns.WAVE]))
    clock = dict(time=float(z["time"]), step=int(z["step"]), n_time_out=int(z["n_time_out"]),
                 time_counter=int(z["time_counter"]), n_outputs=int(z["n_outputs"]))
    return cfg, st, clock, np.ascontiguousarray(z["dT2m"][:ns.WAVE]), np.ascontiguousarray(z["precip_scale"][:ns.WAVE])


def edge_wave():
    """four copies of the bench wave in one handle, lane EDGE_LANE of copy v with layer EDGE_LAYER set to EDGES[v]: (State, dT2m,
    precip_scale)"""
    cfg, st, clock, dT2m, precip_scale = wave("bench")
    assert st.n_active[EDGE_LANE] >= EDGE_LAYER + 5
    lay = np.tile(st.lay, (1, 1, len(EDGES)))
    for v, (S_bu, Tl) in enumerate(EDGES):
        c, k = v * ns.WAVE + EDGE_LANE, EDGE_LAYER - 1
        m = lay[2, k, c]
        lay[0, k, c], lay[1, k, c] = tcs.C_L * Tl * m, S_bu * m
    return (State(np.ascontiguousarray(lay), np.ascontiguousarray(np.tile(st.scal, (1, len(EDGES)))), np.tile(st.n_active, len(EDGES))),
            np.tile(dT2m, len(EDGES)), np.tile(precip_scale, len(EDGES)))


def advance(solver, st, clock, dT2m, precip_scale, launches=(NSTEPS,)):
    solver.set_forcing(*sheba_forcing(), dT2m, precip_scale)
    solver.set_state(st)
    solver.set_clock(**clock)
    solver.set_output_window(0, 0)
    for n in launches:
        solver.step(n)
    return solver.get_state(), solver.get_status()[0]


@functools.lru_cache(maxsize=None)
def on_the_gpu(which, launches=(NSTEPS,)):
    """the wave's 64 columns in a handle of their own: (State, status), shared by the checks and left unchanged"""
    cfg, st, clock, dT2m, precip_scale = wave(which)
    g = samsim_amd.hip_solver(cfg, ns.WAVE)
    out = advance(g, st, clock, dT2m, precip_scale, launches)
    g.close()
    return out


def assert_same_bits(got, want, what):
    assert np.array_equal(got.n_active, want.n_active), f"{what}: N_active"
    assert np.array_equal(got.scal, want.scal), f"{what}: scalars"
    act = np.arange(want.nlayer)[:, None] < want.n_active[None, :]
    for name in BITWISE:
        assert np.array_equal(np.where(act, got.arr(name), 0.0), np.where(act, want.arr(name), 0.0)), f"{what}: {name}"


@pytest.mark.parametrize("which", WHICH)
def test_the_wave_matches_the_oracle(which):
    cfg, st, clock, dT2m, precip_scale = wave(which)
    got, status = on_the_gpu(which)
    assert not status.any(), f"STOP codes {np.unique(status)}"
    o = oracle_solver(cfg, ns.WAVE)
    o.set_threads(NTHREADS)
    want, ostatus = advance(o, st, clock, dT2m, precip_scale)
    o.close()
    assert np.array_equal(status, ostatus)
    assert_state_close(got, want, RTOL, what=f"{which} wave vs oracle")


@pytest.mark.parametrize("which", WHICH)
def test_a_column_does_not_depend_on_its_wave_mates(which):
    """wave b of the second handle = 64 copies of column b: every row vote and every shortcut is that column's alone"""
    cfg, st, clock, dT2m, precip_scale = wave(which)
    mixed, _ = on_the_gpu(which)
    g = samsim_amd.hip_solver(cfg, ns.WAVE * ns.WAVE)
    solo, sstatus = advance(g, ns.repeated(st, ns.WAVE), clock, None if dT2m is None else np.repeat(dT2m, ns.WAVE),
                            None if precip_scale is None else np.repeat(precip_scale, ns.WAVE))
    g.close()
    assert not sstatus.any()
    assert_same_bits(solo, ns.repeated(mixed, ns.WAVE), f"{which}: a column depends on its wave-mates")


@pytest.mark.parametrize("which", WHICH)
def test_the_last_wave_under_partial_exec(which):
    cfg, st, clock, dT2m, precip_scale = wave(which)
    whole, _ = on_the_gpu(which)
    st70, idx = ns.with_first_columns_again(st, 6)
    g = samsim_amd.hip_solver(cfg, st70.ncol)
    got, status = advance(g, st70, clock, None if dT2m is None else np.ascontiguousarray(dT2m[idx]),
                          None if precip_scale is None else np.ascontiguousarray(precip_scale[idx]))
    g.close()
    assert not status.any()
    assert_same_bits(got, ns.columns(whole, idx), f"{which}: 70 columns against 64")


@pytest.mark.parametrize("cuts", [(7, 17), (1,) * NCUT], ids=["7+17", "24x1"])
@pytest.mark.parametrize("which", WHICH)
def test_where_a_launch_ends_changes_no_bit(which, cuts):
    """the last step of a launch stores every row of the Rayleigh-number array and takes no bound: a cut puts that step's full path
    beside the bound's verdict on the same rows"""
    assert sum(cuts) == NCUT
    one, status = on_the_gpu(which, (NCUT,))
    cut, cstatus = on_the_gpu(which, cuts)
    assert np.array_equal(status, cstatus)
    assert_same_bits(cut, one, f"{which}: launches of {cuts} against one of {NCUT}")


def test_one_lane_on_either_side_of_the_shortcut():
    cfg, st, clock, dT2m, precip_scale = wave("bench")
    est, edT, eps = edge_wave()
    g = samsim_amd.hip_solver(cfg, est.ncol)
    got, status = advance(g, est, clock, edT, eps)
    g.close()
    o = oracle_solver(cfg, est.ncol)
    o.set_threads(NTHREADS)
    want, ostatus = advance(o, est, clock, edT, eps)
    o.close()
    assert np.array_equal(status, ostatus) and not status.any(), f"STOP codes {np.unique(status)} / {np.unique(ostatus)}"
    assert_state_close(got, want, RTOL, what="edge waves vs oracle")
    # the same wave without that lane: 63 columns in a handle of their own
    keep = np.array([i for i in range(ns.WAVE) if i != EDGE_LANE])
    g = samsim_amd.hip_solver(cfg, len(keep))
    without, wstatus = advance(g, ns.columns(st, keep), clock, np.ascontiguousarray(dT2m[keep]), np.ascontiguousarray(precip_scale[keep]))
    g.close()
    assert not wstatus.any()
    for v, edge in enumerate(EDGES):
        assert_same_bits(ns.columns(got, v * ns.WAVE + keep), without, f"edge {edge}: the other 63 columns")
    # ... and the changed lane took a different course in each wave: the four are four cases
    T = got.arr("T")[EDGE_LAYER - 1, EDGE_LANE::ns.WAVE]
    assert len(np.unique(T)) == len(EDGES), T
