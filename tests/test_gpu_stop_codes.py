"""STOP codes on the device: same code, step and layer as the CPU oracle on every route of the step.

Every seed of tests/stop_seeds.py that may go to the GPU is run in an ensemble of 70 columns (one full 64-column block and a partial
block of 6) in which one column -- lane 0, lane 63 or column 69 -- holds the seed's mutation and the others are healthy replicas
under the project's ensemble perturbation.  Checked: the status triple of all 70 columns against the oracle, exactly; the healthy
columns against the oracle (RTOL) and, bit for bit, against a second GPU run without the mutation; that a stopped column is frozen;
that the triple does not depend on how the steps are cut into launches, nor on whether the stop step is an output step (unfused
order) or follows one (fused order); the instantiations of the kernel (per-column ocean, one tracer, run-time flags).

Where the late stops land (the dynamics choose; the CPU test prints the table): late_99_cold_snow_x40 stops in step 25 in layer 10,
late_99_dense_cold_snow in step 18 in layer 7, both detected by the second getT chain of the fused up sweep (layers of the top
block, k mod 3 = 1 in both; neither is one of k = 1, 2, N_active - 1, N_active).  Layer 1 is hit by the coupling seeds and by the
double fault, layer 2 by first_sweep_99_short_column, all in the first step.  No late stop of the fused DOWN sweep exists: no late
1337 or 21234 seed was found (tests/stop_seeds.py, SITES)."""
import functools

import numpy as np
import pytest

import samsim_amd
from samsim_amd.capi import State
from tests import stop_seeds as ss
from tests.helpers import RTOL, assert_state_close, rel_err

pytestmark = pytest.mark.gpu

NCOL = ss.NCOL
ARRAYS = ["H_abs", "S_abs", "m", "thick", "T", "phi", "psi_s", "psi_l", "psi_g", "S_bu"]
CASES = [pytest.param(s, c, id=f"{s.name}-col{c}") for s in ss.GPU_SEEDS for c in ss.COLUMNS]


@functools.lru_cache(maxsize=None)
def oracle(name, col, mutated=True, variant="plain", nsteps=ss.MAX_STEPS, n_time_out=None):
    """the oracle's (status triple, state, relative stop step, output snapshot or None) -- computed once per case, never modified"""
    seed = ss.BY_NAME[name]
    o, cfg, st, clock = ss.run_oracle(seed, col, mutated, variant, nsteps, None if n_time_out is None else dict(n_time_out=n_time_out))
    triple = o.get_status()
    state = o.get_state()
    try:
        out = o.get_output()
    except samsim_amd.SamsimError:
        out = None
    o.close()
    rel = int(triple[1][col]) - clock["step"] if mutated else 0
    for a in triple:
        a.setflags(write=False)
    return triple, state, rel, out


def gpu(seed, col, mutated=True, variant="plain", n_time_out=None):
    cfg, st, clock = ss.build(seed, col, mutated, NCOL, variant)
    if n_time_out is not None:
        clock["n_time_out"] = n_time_out
    g = samsim_amd.hip_solver(cfg, NCOL)
    ss.prepare(g, cfg, st, clock, variant)
    return g, cfg, clock


def launch(g, cuts):
    for n in cuts:
        g.step(n)


def columns(st, idx):
    return State(np.ascontiguousarray(st.lay[:, :, idx]), np.ascontiguousarray(st.scal[:, idx]), np.ascontiguousarray(st.n_active[idx]))


def assert_triple(got, want, what):
    for name, a, b in zip(("status", "step", "layer"), got, want):
        assert np.array_equal(a, b), f"{what}: {name} differs in columns {np.nonzero(a != b)[0]}: {a[a != b]} (oracle {b[a != b]})"


def assert_same_bits(a, b, idx, what):
    """prognostic and diagnostic arrays over the active layers, the scalars, N_active: as test_a_column_does_not_depend_on_its_wave_mates"""
    assert np.array_equal(a.n_active[idx], b.n_active[idx]), what
    assert np.array_equal(a.scal[:, idx], b.scal[:, idx]), f"{what}: scalars"
    act = (np.arange(a.nlayer)[:, None] < a.n_active[None, :])[:, idx]
    for n in ARRAYS:
        assert np.array_equal(np.where(act, a.arr(n)[:, idx], 0.0), np.where(act, b.arr(n)[:, idx], 0.0)), f"{what}: {n}"


def cuts_of(total, chunk):
    return [min(chunk, total - d) for d in range(0, total, chunk)]


@pytest.mark.parametrize("seed,col", CASES)
def test_status_triple_and_wave_mates(seed, col):
    """status, step and layer of all 70 columns equal the oracle's; the healthy columns follow the oracle and are bit-identical to
    the run in which nobody stops"""
    want, ostate, rel, _ = oracle(seed.name, col)
    assert want[0][col] == seed.code and seed.min_step <= rel <= ss.MAX_STEPS     # (the CPU test's condition: no vacuous pass)
    g, cfg, clock = gpu(seed, col)
    g.step(ss.MAX_STEPS)
    got, state = g.get_status(), g.get_state()
    g.close()
    print(f"{seed.name} col {col}: gpu ({got[0][col]}, {got[1][col] - clock['step']}, {got[2][col]})  oracle ({want[0][col]}, {rel}, {want[2][col]})")
    assert_triple(got, want, seed.name)
    healthy = np.delete(np.arange(NCOL), col)
    assert_state_close(columns(state, healthy), columns(ostate, healthy), RTOL, what=f"{seed.name}: wave-mates against the oracle")
    c, _, _ = gpu(seed, col, mutated=False)
    c.step(ss.MAX_STEPS)
    clean, cstatus = c.get_state(), c.get_status()[0]
    c.close()
    assert not cstatus.any()
    assert_same_bits(state, clean, healthy, f"{seed.name}: wave-mates against the clean run")


@pytest.mark.parametrize("seed", ss.GPU_SEEDS, ids=lambda s: s.name)
def test_a_stopped_column_is_frozen(seed):
    col = 63
    want, _, rel, _ = oracle(seed.name, col)
    g, cfg, clock = gpu(seed, col)
    g.step(rel)
    triple, before = g.get_status(), g.get_state()
    assert_triple(triple, want, f"{seed.name} after its stop step")
    cells0 = g.get_work()[0]
    # single steps: the work counter grows by the N_active of the running columns, formed on the host from the state before the step
    state = before
    for _ in range(3):
        running = g.get_status()[0] == 0
        g.step(1)
        cells = g.get_work()[0]
        assert cells - cells0 == int(state.n_active[running].sum())
        cells0, state = cells, g.get_state()
    launch(g, (24, 23))          # 50 more steps in all
    after, triple2 = g.get_state(), g.get_status()
    stats = g.ensemble_stats(["N_active", "thick_snow"])
    g.close()
    assert_triple(triple2, triple, f"{seed.name} 50 steps later")
    assert np.array_equal(after.lay[:, :, col], before.lay[:, :, col]), "layer arrays of the stopped column changed"
    assert np.array_equal(after.scal[:, col], before.scal[:, col]), "scalars of the stopped column changed"
    assert after.n_active[col] == before.n_active[col]
    nstopped = int((triple2[0] != 0).sum())
    assert nstopped == 1
    assert stats["N_active"].count == NCOL - nstopped and stats["thick_snow"].count == NCOL - nstopped
    # and the others went on
    others = np.delete(np.arange(NCOL), col)
    assert not np.array_equal(after.arr("H_abs")[:, others], before.arr("H_abs")[:, others])


@pytest.mark.parametrize("seed", ss.GPU_SEEDS, ids=lambda s: s.name)
def test_launch_granularity(seed):
    """the stop step as the only step of its launch, a middle or the last one (launches of 1), inside launches of 7, inside one
    launch of all steps: same triple; on the late seeds the healthy columns keep their bits"""
    col = 69
    want, _, rel, _ = oracle(seed.name, col)
    total = ss.MAX_STEPS if seed.min_step >= 10 else 15
    states = []
    plans = [cuts_of(total, 1), cuts_of(total, 7), [total]]
    if rel > 1:
        plans.append([rel - 1, 1, total - rel])      # the only step of its launch
        plans.append([rel, total - rel])             # the last step of its launch
    for cuts in plans:
        g, cfg, clock = gpu(seed, col)
        launch(g, [n for n in cuts if n > 0])
        assert_triple(g.get_status(), want, f"{seed.name}, launches {cuts[:3]}...")
        states.append(g.get_state())
        g.close()
    healthy = np.delete(np.arange(NCOL), col)
    for st in states[1:]:
        assert_same_bits(st, states[0], healthy, f"{seed.name}: launch granularity")
        # the stopped column: what it holds is what its stop step left, whichever launch that step was part of.  Compared over the
        # prognostic arrays and the scalars: the diagnostic and work arrays (ray rows, S_br, perm, the volume fractions) are stored in full only by
        # the last step of a launch, so for a column that stopped in mid-step they depend on where the launch ended
        for n in ss.PROGNOSTIC:
            assert np.array_equal(st.arr(n)[:, col], states[0].arr(n)[:, col]), f"{seed.name}: {n} of the stopped column depends on the launches"
        assert st.n_active[col] == states[0].n_active[col] and np.array_equal(st.scal[:, col], states[0].scal[:, col])


OUTPUT_CASES = [("first_sweep_99_winter", 0), ("late_99_dense_cold_snow", 0), ("late_99_dense_cold_snow", 1)]


@pytest.mark.parametrize("name,lead", OUTPUT_CASES, ids=["first_sweep-stop_step_is_output_step", "late-stop_step_is_output_step",
                                                         "late-stop_step_follows_output_step"])
def test_stop_in_and_after_an_output_step(name, lead):
    """n_time_out is set so that the stop step is an output step (it takes the unfused order) or the step after one (the fused order
    again, with the Rayleigh numbers kept for the snapshot): the triple equals the oracle's in both, and the output snapshot of the
    healthy columns matches the oracle's"""
    seed, col = ss.BY_NAME[name], 63
    _, _, rel, _ = oracle(name, col)
    assert rel - lead >= 1
    cfg0 = ss.CONFIGS[seed.config]()
    nto = cfg0.i_time_out - (rel - lead - 1)      # output_point fires in relative step rel - lead
    want, _, rel2, oout = oracle(name, col, n_time_out=nto)
    assert rel2 == rel and want[0][col] == seed.code, "moving the output point moved the stop"
    g, cfg, clock = gpu(seed, col, n_time_out=nto)
    assert g.steps_to_output() == rel - lead
    g.step(ss.MAX_STEPS)
    got, gout = g.get_status(), g.get_output()
    g.close()
    assert_triple(got, want, f"{name}, output in step {rel - lead}")
    assert gout.step == oout.step == clock["step"] + rel - lead
    healthy = np.delete(np.arange(NCOL), col)
    assert np.array_equal(gout.n_active[healthy], oout.n_active[healthy])
    act = (np.arange(cfg.nlayer)[:, None] < oout.n_active[None, :])[:, healthy]
    for n in ["T", "psi_s", "psi_l", "psi_g", "S_bu", "thick", "H_abs", "S_abs", "m"]:
        assert rel_err(gout.arr(n)[:, healthy][act], oout.arr(n)[:, healthy][act], 1e-3 if n == "H_abs" else 1e-7) <= RTOL, n
    act1 = (np.arange(cfg.nlayer)[:, None] < oout.n_active[None, :] - 1)[:, healthy]
    assert rel_err(gout.arr("ray")[:, healthy][act1], oout.arr("ray")[:, healthy][act1], 1e-6) <= RTOL, "ray"
    for n in ["freeboard", "thick_snow", "T_snow", "thickness", "bulk_salin", "energy_stored", "freshwater", "total_resist", "T_top",
              "grav_drain"]:
        floor = {"grav_drain": 1e-8}.get(n, 1e-7)
        assert rel_err(gout.sc(n)[healthy], oout.sc(n)[healthy], floor) <= RTOL, n


VARIANT_CASES = [pytest.param(s, v, id=f"{s.name}-{v}") for s in ss.GPU_SEEDS for v in s.variants if v != "plain"]


@pytest.mark.parametrize("seed,variant", VARIANT_CASES)
def test_other_instantiations_of_the_kernel(seed, variant):
    """the late 99, the 431 and the 1337 seed under the per-column ocean (zero offsets, cfg.S_bu_bottom), with one passive tracer, and
    with harmonic_flag 1 (the kernel that reads its flags at run time); the oracle gets the same configuration"""
    col = 63
    want, ostate, rel, _ = oracle(seed.name, col, variant=variant)
    assert want[0][col] == seed.code and seed.min_step <= rel <= ss.MAX_STEPS
    g, cfg, clock = gpu(seed, col, variant=variant)
    g.step(ss.MAX_STEPS)
    got, state = g.get_status(), g.get_state()
    g.close()
    assert_triple(got, want, f"{seed.name} / {variant}")
    healthy = np.delete(np.arange(NCOL), col)
    assert_state_close(columns(state, healthy), columns(ostate, healthy), RTOL, what=f"{seed.name} / {variant}: wave-mates against the oracle")
