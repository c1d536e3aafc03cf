"""getT_chain keeps each lane's part in the wave's Newton loop -- wants another evaluation, goes to the general routine -- as one bit
of two 64-bit lane masks (samsim_amd/csrc/samsim_thermo.h).  What a column gets must not depend on that: not on the lanes beside it,
not on how many lanes of the wave are active.

Two waves of 64 columns, 50 steps each:
  crafted   tests/newton_seeds.py: the lanes fall into every class of the loop in the same layer (first evaluation holds, many
            evaluations, fresh ice and pure brine, an iterate that leaves (-200, 0), a guess with S_br < 1e-4), N_active 2..80;
            the winter instance of the loop (the fused up sweep) and the full first sweep
  warm      64 members of the day-360 SHEBA ensemble, not crafted: a flushing wave runs getT_chain<true> in the full first sweep and
            in the lite up sweep (tests/test_newton_seeds_host.py: a column flushes within the 50 steps)
and for each of them
  * the wave against the CPU oracle at the project's bar (1e-6 relative, integers exact);
  * the wave bitwise against each of its columns in a wave of 64 copies of itself (the arrays tests/test_gpu_up_sweep_trips.py
    compares): a lane's masks hold only its own bit;
  * a handle of 70 columns (the wave and its first six columns again) bitwise against the 64-column handle on the shared columns:
    the last wave runs under partial exec, six lanes of 64."""
import functools
import os

import numpy as np
import pytest

import samsim_amd
from tests import newton_seeds as ns
from tests.helpers import RTOL, assert_state_close, sheba_forcing
from tests.oracle_lib import oracle_solver

pytestmark = pytest.mark.gpu

NTHREADS = min(16, len(os.sched_getaffinity(0)))
WHICH = ["crafted", "warm"]
BITWISE = ["H_abs", "S_abs", "m", "thick", "T", "phi", "psi_s", "psi_l", "psi_g", "S_bu"]


@functools.lru_cache(maxsize=None)
def wave(which):
    """(cfg, State, clock, dT2m, precip_scale)"""
    if which == "crafted":
        return ns.crafted_wave() + (None, None)
    return ns.warm_wave()


def advance(solver, st, clock, dT2m, precip_scale):
    solver.set_forcing(*sheba_forcing(), dT2m, precip_scale)
    solver.set_state(st)
    solver.set_clock(**clock)
    solver.set_output_window(0, 0)
    solver.step(ns.NSTEPS)
    return solver.get_state(), solver.get_status()[0]


@functools.lru_cache(maxsize=None)
def on_the_gpu(which):
    """the wave's 64 columns in a handle of their own: (State, status), shared by the three checks and left unchanged"""
    cfg, st, clock, dT2m, precip_scale = wave(which)
    g = samsim_amd.hip_solver(cfg, ns.WAVE)
    out = advance(g, st, clock, dT2m, precip_scale)
    g.close()
    return out


def assert_same_bits(got, want, what):
    """got against want over the active layers, in the arrays and scalars test_gpu_up_sweep_trips.py compares"""
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
def test_a_lane_holds_only_its_own_bit(which):
    """wave b of the second handle = 64 copies of column b"""
    cfg, st, clock, dT2m, precip_scale = wave(which)
    mixed, _ = on_the_gpu(which)
    rep = ns.repeated(st, ns.WAVE)
    g = samsim_amd.hip_solver(cfg, ns.WAVE * ns.WAVE)
    solo, sstatus = advance(g, rep, clock, None if dT2m is None else np.repeat(dT2m, ns.WAVE),
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
