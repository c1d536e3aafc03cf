"""The rejuvenation of the resampled ensemble on the GPU (samsim_jitter, samsim_get_ocean, SAMSIM_OCEAN_SLOT, Solver.rejuvenate and
Solver.assimilate).  The reference is tests/jitter_reference.apply: the deviate of samsim_amd/csrc/samsim_jitter.h compiled for the
host and the value rule in numpy, applied to the rows, status and labels downloaded from the same handle; every comparison of a row
is bit for bit, through view(np.uint64).

The handles are the neighbours': the day-200 ensemble tiled over 300 columns (four full blocks and a ragged one of 44), three steps
on, and the 70 001 x 12 handle of tests/test_gpu_resample.py that is never stepped (1 094 blocks, a ragged last block, three stopped
columns, the last column among them).  Both are testcase 4, so both ocean rows can be set."""
import ctypes as C

import numpy as np
import pytest

import bench
import samsim_amd
from samsim_amd import capi, testcases as tcs
from samsim_amd.capi import JT, S, JitterInfo, JitterSpec, JitterTerm, SamsimError, ocean_slot
from tests import copy_reference as cr
from tests import hist_reference as hr
from tests import jitter_reference as jr
from tests.test_gpu_group_stats import labels_of_test_1
from tests.test_gpu_profile_stats import ensemble
from tests.test_gpu_weights import BUOY, J_SUM

pytestmark = pytest.mark.gpu
NCOL = 70001
STOPPED = (5, 40000, 70000)
GROUP = 3
DT2M, PSCALE = S["dT2m"], S["precip_scale"]
INF = np.inf
FIXTURE = "sheba_ensemble_80.npz"
MEMBER = 13


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def labels(ncol):
    """labels_of_test_1 at any size: nine groups and -1s (group 9, one column, exists from 12 346 columns on)"""
    c = np.arange(ncol, dtype=np.int64)
    lab = ((c * 7919) % 9).astype(np.int32)
    lab[::11] = -1
    if ncol > 12345:
        lab[12345] = 9
    return lab


def ocean_rows(ncol, seed=7):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, ncol), 34.0 + rng.uniform(-0.5, 0.5, ncol)


def small(ncol=300, nsteps=3, sensors=False):
    """the day-200 ensemble tiled over ncol columns, nsteps steps on, with labels and both ocean rows"""
    g = ensemble(FIXTURE, ncol, 0)
    g.set_ocean(*ocean_rows(ncol))
    g.set_groups(labels(ncol), ngroups=11)
    if nsteps:
        g.step(nsteps)
    assert not g.get_status()[0].any()
    if sensors:
        g.set_sensors(BUOY)
        g.score(g.sensor_values([77])[:, 0])
    return g


@pytest.fixture(scope="module")
def big():
    """70 001 columns of 12 layers, never stepped: the perturbation rows and the ocean rows set, labels, three columns stopped"""
    assert cr.grid_rule(NCOL) == (1094, 2, 547) and NCOL % 64 != 0 and STOPPED[-1] == NCOL - 1
    assert np.array_equal(labels(NCOL), labels_of_test_1(NCOL))
    rng = np.random.default_rng(23)
    cfg, st = tcs.testcase4(NCOL, nlayer=12, n_top=4, n_bottom=4)
    g = samsim_amd.hip_solver(cfg, NCOL)
    g.set_forcing(*bench.sheba_forcing(), rng.normal(0.0, 1.5, NCOL), 1.0 + rng.uniform(-0.3, 0.3, NCOL))
    g.set_ocean(*ocean_rows(NCOL))
    g.set_state(st)
    g.set_groups(labels(NCOL), ngroups=11)
    g.set_clock()
    for c in STOPPED:
        g.set_status(np.array([7], dtype=np.int32), col0=c)
    assert sorted(np.flatnonzero(g.get_status()[0])) == list(STOPPED)
    yield g
    g.close()


def rows_of(g, state=None):
    """{target: float64 [ncol]}: the four parameter rows as the getters return them"""
    s = g.get_state() if state is None else state
    dq, sb = g.get_ocean()
    return {0: s.sc("dT2m").copy(), 1: s.sc("precip_scale").copy(), 2: dq, 3: sb}


def everything(g):
    """copy_reference.everything with the two ocean rows"""
    e = cr.everything(g)
    dq, sb = g.get_ocean()
    e["ocean0"], e["ocean1"] = u64(dq).copy(), u64(sb).copy()
    return e


def only_the_named_rows_moved(before, after, targets, w, what):
    """two everything(): equal but for the rows of `targets` at the columns w (a mask)"""
    keep = ~w
    for k in before:
        if k == "scal":
            other = np.setdiff1d(np.arange(before[k].shape[0]), [r for t, r in ((0, DT2M), (1, PSCALE)) if t in targets])
            assert np.array_equal(before[k][other], after[k][other]), (what, k)
            assert np.array_equal(before[k][:, keep], after[k][:, keep]), (what, k, "columns not written")
        elif k in ("ocean0", "ocean1"):
            if int(k[-1]) + 2 in targets:
                assert np.array_equal(before[k][keep], after[k][keep]), (what, k, "columns not written")
            else:
                assert np.array_equal(before[k], after[k]), (what, k)
        else:
            assert np.array_equal(before[k], after[k]), (what, k)


def same_rows(got, want, what):
    for t in want:
        assert u64(got[t]).tobytes() == u64(want[t]).tobytes(), (what, capi.JITTER_TARGETS[t], np.flatnonzero(u64(got[t]) != u64(want[t]))[:8])


def four_terms(rows, run):
    """Liu and West at delta 0.9 on all four rows, with wide bounds"""
    a, h = capi.liu_west(0.9)
    out = []
    for t in range(4):
        v = rows[t][run]
        out.append(JitterTerm.make(t, float(v.mean()), a, h * float(v.std()), 0.0 if t == JT["S_bu_bottom"] else -INF, INF))
    return out


def refused(code, call):
    with pytest.raises(SamsimError) as e:
        call()
    assert e.value.code == code, (e.value.code, code)


# ---------------------------------------------------------------------------------------------------------- 1: bit for bit
def check_pool(g, lab, group, seed, what):
    status = g.get_status()[0]
    rows = rows_of(g)
    w = jr.written("pool", g.ncol, status, lab, group)
    terms = four_terms(rows, w)
    want, want_info = jr.apply(terms, rows, seed, "pool", status, lab, group)
    info = g.jitter(terms, "pool", seed, group)
    assert info == want_info and info["n_written"] == int(w.sum()) > 0, (what, info, want_info)
    got = rows_of(g)
    same_rows(got, want, what)
    for t in range(4):
        assert (u64(got[t])[w] != u64(rows[t])[w]).mean() > 0.99, (what, t)
    return rows, got, w


@pytest.mark.parametrize("group", [None, GROUP])
def test_pool_equals_the_reference_bit_for_bit_on_the_small_handle(group):
    g = small()
    _, _, w = check_pool(g, labels(300), group, 20261021, ("small", group))
    assert w.sum() == (300 if group is None else (labels(300) == GROUP).sum())
    g.close()


@pytest.mark.parametrize("group", [None, GROUP])
def test_pool_equals_the_reference_bit_for_bit_on_the_large_handle(big, group):
    rows, got, w = check_pool(big, labels(NCOL), group, (1 << 64) - 5, ("large", group))
    assert not w[list(STOPPED)].any() and w.sum() == (NCOL - 3 if group is None else w.sum()) and (group is None or 6000 < w.sum() < 8000)
    for t in range(4):                                                    # the stopped columns and those outside the group keep their bytes
        assert np.array_equal(u64(got[t])[~w], u64(rows[t])[~w])


# ---------------------------------------------------------------------------------------------------- 2: nothing else moves
def test_nothing_but_the_named_rows_of_the_written_columns_moves():
    a, b = small(), small()
    lab = labels(300)
    a.set_status(np.array([7], dtype=np.int32), col0=130)
    b.set_status(np.array([7], dtype=np.int32), col0=130)
    status = a.get_status()[0]
    e0 = everything(a)
    assert not cr.differing(e0, everything(b))
    calls = [([JitterTerm.make("dT2m", 0.0, 0.9, 0.5), JitterTerm.make("S_bu_bottom", 34.0, 0.9, 0.3, 0.0, INF)], None, 11),
             ([JitterTerm.make("dfl_q_bottom", 0.0, 0.5, 0.2)], GROUP, 12),
             ([JitterTerm.make("precip_scale", 1.0, 0.9, 0.05, 0.5, 2.0), JitterTerm.make("dT2m", 0.0, 1.0, 0.1)], 0, 11)]
    for terms, group, seed in calls:
        w = jr.written("pool", 300, status, lab, group)
        assert not w[130] and 0 < w.sum() < 300
        info = a.jitter(terms, "pool", seed, group)
        assert info == b.jitter(terms, "pool", seed, group) and info["n_written"] == w.sum()
        e1 = everything(a)
        only_the_named_rows_moved(e0, e1, [t.target for t in terms], w, (group, seed))
        assert cr.differing(e0, e1)
        assert not cr.differing(e1, everything(b))                        # two handles given the same calls hold the same bytes
        e0 = e1
    # the clock, the labels and the weight-free handle's refusals are as before: nothing was created on the way
    assert a.get_clock().step == b.get_clock().step == 3 + bench.load_ensemble(FIXTURE)[2]["step"]
    refused(-1, a.weights)
    refused(-1, a.offspring)
    # and the run goes on
    for g in (a, b):
        g.step(5)
    ea = everything(a)
    assert not cr.differing(ea, everything(b)) and np.flatnonzero(ea["status"]).tolist() == [130]
    a.close()
    b.close()


# ------------------------------------------------------------------------------------- 3: the deviate belongs to the column
def test_the_deviate_belongs_to_the_column(big):
    seed = 4242
    targets = ("dT2m", "precip_scale", "dfl_q_bottom")                    # (the salinity below cannot take an infinite lower bound)
    terms = [JitterTerm.make(t, 0.0, 0.37, 1.0) for t in targets]
    a, b = small(nsteps=0), small(nsteps=0)
    for g in (a, b, big):
        g.set_forcing(*bench.sheba_forcing(), np.zeros(g.ncol), np.zeros(g.ncol))
        g.set_ocean(np.zeros(g.ncol), ocean_rows(g.ncol)[1])
    info = a.jitter(terms, "pool", seed)
    assert info == {"n_written": 300, "n_lo": [0, 0, 0], "n_hi": [0, 0, 0]}
    ra = rows_of(a)
    for t in range(3):                                                    # the row becomes the reference's deviate exactly
        eps, att = jr.deviate(seed, np.arange(300), t)
        assert u64(ra[t]).tobytes() == u64(eps).tobytes() and att.max() <= 20, t
    # column c of the large handle receives the same deviate, whatever the group and the grid
    big.jitter(terms, "pool", seed, GROUP)
    rb = rows_of(big)
    w = jr.written("pool", NCOL, big.get_status()[0], labels(NCOL), GROUP)
    for t in range(3):
        eps, _ = jr.deviate(seed, np.arange(NCOL), t)
        assert u64(rb[t]).tobytes() == u64(np.where(w, eps, 0.0)).tobytes(), t
        assert np.array_equal(u64(rb[t])[:300][w[:300]], u64(ra[t])[w[:300]])
    # a two-term spec and two one-term specs, in the other order, give the same rows
    b.jitter(terms[2:], "pool", seed)
    b.jitter(terms[1:2], "pool", seed)
    b.jitter(terms[:1], "pool", seed)
    same_rows(rows_of(b), ra, "term by term")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------- 4, 5: the copies
def applied():
    """a scored 300-column handle, weighted so that the median member keeps exp(-1), drawn at the pool's size and applied with the
    forcing: (handle, src, dst)"""
    g = small(sensors=True)
    J = g.scores()["J_SUM"]
    g.set_weights(J_SUM, "gauss", float(np.median(J[J > 0.0])) / 2.0)
    r = g.resample(300, "systematic", 0.37)
    p = g.apply_resample(forcing=True)
    src, dst = g.copy_plan()
    assert p["n_copies"] == dst.size == 300 - r["n_survivors"] and 10 <= dst.size < 300
    return g, src, dst


COPY_TERMS = [JitterTerm.make("dT2m", 0.0, 0.95, 0.5), JitterTerm.make("precip_scale", 1.0, 0.95, 0.05, 0.1, 3.0),
              JitterTerm.make("dfl_q_bottom", 0.0, 0.95, 0.3), JitterTerm.make("S_bu_bottom", 34.0, 0.95, 0.2, 0.0, INF)]


def test_copies_writes_the_destinations_of_the_plan_and_nothing_else():
    (a, src, dst), (b, _, dst_b), (c, _, dst_c) = applied(), applied(), applied()
    assert np.array_equal(dst, dst_b) and np.array_equal(dst, dst_c)
    e0 = everything(a)
    r0 = rows_of(a)
    for t in range(4):                                                    # the copies are their sources, byte for byte
        assert np.array_equal(u64(r0[t])[dst], u64(r0[t])[src])
    info = a.jitter(COPY_TERMS, "copies", 99)
    assert info["n_written"] == dst.size
    assert b.jitter(COPY_TERMS, "pool", 99)["n_written"] == 300
    ra, rb = rows_of(a), rows_of(b)
    w = np.zeros(300, dtype=bool)
    w[dst] = True
    for t in range(4):
        assert np.array_equal(u64(ra[t])[dst], u64(rb[t])[dst]), t         # what POOL with the same spec gives them on a twin
        assert (u64(ra[t])[dst] != u64(r0[t])[dst]).all(), t
    only_the_named_rows_moved(e0, everything(a), [0, 1, 2, 3], w, "copies")   # every other column, the sources included
    want, want_info = jr.apply(COPY_TERMS, r0, 99, "copies", a.get_status()[0], plan_dst=dst)
    same_rows(ra, want, "copies against the reference")
    assert info == want_info
    # a destination stopped after the apply is skipped
    k = int(dst[dst.size // 2])
    c.set_status(np.array([9], dtype=np.int32), col0=k)
    info_c = c.jitter(COPY_TERMS, "copies", 99)
    assert info_c["n_written"] == dst.size - 1
    rc = rows_of(c)
    rest = dst[dst != k]
    for t in range(4):
        assert u64(rc[t])[k] == u64(r0[t])[k] and np.array_equal(u64(rc[t])[rest], u64(ra[t])[rest]), t
    assert a.copy_plan()[1].tobytes() == dst.tobytes()                     # the stored plan is not written
    for g in (a, b, c):
        g.close()


def test_duplicates_part_and_sources_do_not():
    """T_top is the weakest witness the state has: under snow it is the twice-iterated radiative balance started from T_snow, whose
    result depends on its start only in fourth order (the members' T_snow differ by 0.3 K, their T_top by 4e-8 K), and dT2m reaches
    T_snow only through the enthalpy of the falling snow (1.4e-8 m/s at day 200: 1e-6 K per step and kelvin of dT2m).  So a kelvin of
    dT2m moves T_top by some 1e-12 K in five steps, a few hundred ulp, and the jitter is wide here (5 K, no shrinkage) for the
    smallest of the ~150 deviates (~1e-2) still to show."""
    (a, src, dst), (d, _, _) = applied(), applied()
    a.jitter([JitterTerm.make("dT2m", 0.0, 1.0, 5.0)], "copies", 99)
    for g in (a, d):
        g.reset_scores()
        g.step(5)
    sa, sd = a.get_state(), d.get_state()
    assert not a.get_status()[0].any()
    T = sa.sc("T_top")
    gap = np.abs(T[dst] - T[src])
    print("duplicates:", dst.size, "copies,", int((gap == 0.0).sum()), "still at their source's T_top; |dT_top| min", float(gap.min()),
          "median", float(np.median(gap)), "| |d dT2m| min", float(np.abs(sa.sc("dT2m")[dst] - sa.sc("dT2m")[src]).min()),
          "| T_snow gap min", float(np.abs(sa.sc("T_snow")[dst] - sa.sc("T_snow")[src]).min()))
    assert (T[dst] != T[src]).all()                                       # each copy has left its source
    assert (sd.sc("T_top")[dst] == sd.sc("T_top")[src]).all()             # which, without the jitter, it never does
    others = np.setdiff1d(np.arange(300), dst)
    ea, ed = cr.everything(a), cr.everything(d)
    for k in ea:                                                          # sources and survivors: the bytes of the twin that did not jitter
        assert np.array_equal(ea[k][..., others], ed[k][..., others]) if ea[k].shape[-1] == 300 else np.array_equal(ea[k], ed[k]), k
    a.close()
    d.close()


# ------------------------------------------------------------------------------------------------------------- 6: clamps
def test_the_clamps_cut_both_tails_and_the_run_goes_on():
    g = small()
    rows, status = rows_of(g), g.get_status()[0]
    terms = [JitterTerm.make("dT2m", 0.0, 0.9, 0.5, -0.4, 0.4), JitterTerm.make("precip_scale", 1.0, 0.9, 0.1, 0.95, 1.05),
             JitterTerm.make("dfl_q_bottom", 0.0, 0.9, 1.0, -0.5, 0.5), JitterTerm.make("S_bu_bottom", 34.0, 0.9, 1.0, 33.5, 34.5)]
    want, want_info = jr.apply(terms, rows, 31337, "pool", status)
    info = g.jitter(terms, "pool", 31337)
    print("clamps:", info)
    assert info == want_info and info["n_written"] == 300
    assert min(info["n_lo"]) > 0 and min(info["n_hi"]) > 0                # else the test proves nothing
    got = rows_of(g)
    same_rows(got, want, "clamps")
    for i, t in enumerate(terms):
        v = got[t.target]
        assert (v >= t.lo).all() and (v <= t.hi).all() and (v == t.lo).sum() >= info["n_lo"][i] and (v == t.hi).sum() >= info["n_hi"][i]
    assert (got[3] >= 0.0).all()
    g.step(5)
    assert not g.get_status()[0].any()
    g.close()


# --------------------------------------------------------------------------------------------------------- 7: ocean rows
def test_the_ocean_rows_are_readable_and_are_slots(big):
    g = big
    dq, sb = ocean_rows(NCOL, 5)
    g.set_ocean(dq, sb)
    gq, gs = g.get_ocean()
    assert u64(gq).tobytes() == u64(dq).tobytes() and u64(gs).tobytes() == u64(sb).tobytes()
    wq, ws = g.get_ocean(69990, 11)
    assert u64(wq).tobytes() == u64(dq[69990:]).tobytes() and u64(ws).tobytes() == u64(sb[69990:]).tobytes()
    assert g.get_ocean(5, 3, S_bu_bottom=False)[1] is None and g.get_ocean(NCOL, 0)[0].size == 0
    for col0, n in ((-1, 2), (0, NCOL + 1), (NCOL, 1), (NCOL + 1, 0), (0, -1)):
        refused(-1, lambda: g.get_ocean(col0, n))
    status = g.get_status()[0]
    ok = status == 0
    q = g.ensemble_stats([ocean_slot(0), ocean_slot("S_bu_bottom")])
    for slot, v in ((ocean_slot(0), dq[ok]), (ocean_slot(1), sb[ok])):
        # the bars of tests/test_gpu_ensemble_io.py
        assert q[slot].count == NCOL - 3 and q[slot].min == v.min() and q[slot].max == v.max()
        assert abs(q[slot].mean - v.mean()) <= 1e-12 * max(1.0, abs(v.mean()))
        assert abs(q[slot].std - v.std()) <= 1e-10 * max(1e-3, v.std())
    assert np.array_equal(g.histogram(ocean_slot(0), 40, -1.0, 0.05), hr.scalar_histogram_reference(dq, status, 40, -1.0, 0.05))
    assert np.array_equal(g.histogram(ocean_slot(1), 25, 33.4, 0.05), hr.scalar_histogram_reference(sb, status, 25, 33.4, 0.05))
    count, mean, cov = g.covariance([ocean_slot(1), "dT2m"], group=GROUP)
    in_group = ok & (labels(NCOL) == GROUP)
    assert count == in_group.sum() and abs(mean[0] - sb[in_group].mean()) <= 1e-12 * 34.0
    # (a variance of 0.08 around a mean of 34: sums of n squares of size 34^2 carry n * 2^-53 * 34^2 / 0.08 ~ 1e-8 of it at the worst)
    assert abs(cov[0, 0] - sb[in_group].var()) <= 1e-8 * sb[in_group].var()
    # the slot is refused without its row, and so is the getter
    g.set_ocean(dq, None)
    assert g.ensemble_stats([ocean_slot(0)])[ocean_slot(0)].count == NCOL - 3
    refused(-1, lambda: g.ensemble_stats([ocean_slot(1)]))
    refused(-1, lambda: g.histogram(ocean_slot(1), 25, 33.4, 0.05))
    refused(-1, lambda: g.get_ocean())
    assert g.get_ocean(S_bu_bottom=False)[0].size == NCOL
    refused(-1, lambda: g.jitter([JitterTerm.make("S_bu_bottom", 34.0, 0.9, 0.1, 0.0, INF)]))
    g.set_ocean(None, None)
    refused(-1, lambda: g.ensemble_stats([ocean_slot(0)]))
    refused(-1, lambda: g.ensemble_stats([ocean_slot(2)]))
    g.set_ocean(dq, sb)


# ----------------------------------------------------------------------------------------------------------- 8: the cycle
def test_the_assimilation_cycle_keeps_the_members_distinct():
    ncol, rounds, seed = 4096, 4, 2026
    truth = ensemble(FIXTURE, 64, 0)
    truth.set_sensors(BUOY)
    truth_dT2m = float(truth.get_state().sc("dT2m")[MEMBER])
    a, b = ensemble(FIXTURE, ncol, 0), ensemble(FIXTURE, ncol, 0)
    # the fixture's 256 members are tiled over the columns: every column gets a dT2m of its own, so that the twin run starts from as
    # many distinct members as the run with rejuvenation and the loss of members is the resampling's doing, not the tiling's
    pert = bench.load_ensemble(FIXTURE)[3]
    dT2m = bench.tile(pert[0], ncol) + np.random.default_rng(8).normal(0.0, 0.1, ncol)
    assert np.unique(dT2m).size == ncol
    for g in (a, b):
        g.set_forcing(*bench.sheba_forcing(), dT2m, bench.tile(pert[1], ncol))
        assert np.unique(g.get_state().sc("dT2m")).size == ncol
        g.set_sensors(BUOY)
    scale, last_survivors = None, None
    for r in range(rounds):
        for g in (truth, a, b):
            g.step(8)
        obs = truth.sensor_values([MEMBER])[:, 0]
        # the twin: the same calls without the rejuvenation
        b.score(obs)
        if scale is None:                                                 # tempered once, from the first round's misfits: the median member keeps exp(-1)
            J = b.scores()["J_SUM"]
            scale = float(np.median(J[J > 0.0])) / 2.0
        wb = b.set_weights(J_SUM, "gauss", scale)
        step = int(b.get_clock().step)
        rb = b.resample(wb["n_in"], "systematic", u0=capi.rs_offset(seed, 2 * step))
        b.apply_resample(forcing=True)
        b.reset_scores()
        out = a.assimilate(obs, scale=scale, ess_frac=1.0, seed=seed, targets=("dT2m",), delta=0.98)
        assert out["resampled"] and out["n_in"] == ncol and out["jitter"]["n_written"] == ncol and out["jitter"]["count"] == ncol
        assert out["n_copies"] == ncol - out["n_survivors"]
        da, db = a.get_state().sc("dT2m"), b.get_state().sc("dT2m")
        if r == 0:                                                        # until the first jitter the two runs are one
            assert out["ess"] == wb["ess"] and out["n_survivors"] == rb["n_survivors"]
        print("round", r, "ESS", out["ess"], "survivors", out["n_survivors"], "| dT2m posterior mean", float(da.mean()), "spread", float(da.std()),
              "truth", truth_dT2m, "| without rejuvenation: survivors", rb["n_survivors"], "distinct", np.unique(db).size)
        assert np.unique(da).size == ncol                                 # with rejuvenation every member is its own
        assert np.unique(db).size <= rb["n_survivors"] < ncol             # without, the members only ever become fewer
        assert last_survivors is None or np.unique(db).size <= last_survivors
        last_survivors = rb["n_survivors"]
        # Liu and West keep the first two moments of the pool: the jitter's own moments against the rows it left
        m, v = out["jitter"]["mean"][0], out["jitter"]["var"][0]
        assert abs(da.mean() - m) < 5.0 * np.sqrt(v / ncol) + 1e-12 and abs(da.var() - v) < 5.0 * v * np.sqrt(2.0 / ncol) * 2.0 + 1e-12
    assert not a.get_status()[0].any() and not b.get_status()[0].any()
    for g in (truth, a, b):
        g.close()


# ----------------------------------------------------------------------------------------------------------- 9: refusals
def test_refusals_in_the_documented_order_leave_everything():
    g = small()
    before = everything(g)
    info = JitterInfo(-7)
    good = [JitterTerm.make("dT2m", 0.1, 0.9, 0.2, -3.0, 3.0), JitterTerm.make("S_bu_bottom", 34.0, 0.5, 1.0, 0.0, 40.0)]

    def no(code, spec):
        refused(code, lambda: g.jitter_raw(spec, info))
        assert info.n_written == -7 and list(info.n_lo) == [0, 0, 0, 0]

    def spec_with(i=0, which="pool", group=None, **kw):
        terms = [JitterTerm.make(t.target, t.centre, t.shrink, t.sigma, t.lo, t.hi) for t in good]
        for k, v in kw.items():
            setattr(terms[i], k, v)
        return JitterSpec.make(terms, which, 5, group)

    assert g._f("jitter")(None, C.byref(spec_with()), None) == -1
    no(-1, None)
    s = spec_with(which=5)                                                # the struct size before everything a spec holds
    s.struct_size += 4
    no(-6, s)
    no(-1, spec_with(which=2))
    for n in (0, 5, -1):
        s = spec_with()
        s.nterms = n
        no(-1, s)
    nan = float("nan")
    for i in (0, 1):
        for f in (dict(target=4), dict(target=-1), dict(reserved=2), dict(centre=nan), dict(shrink=INF), dict(sigma=nan), dict(shrink=1.5),
                  dict(shrink=-0.1), dict(sigma=-1.0), dict(lo=nan), dict(hi=nan), dict(lo=1.0, hi=0.5)):
            no(-1, spec_with(i, **f))
    no(-1, spec_with(1, target=JT["dT2m"]))                               # listed twice
    no(-1, spec_with(1, lo=-1.0))                                         # a negative salinity below
    no(-1, spec_with(group=11))                                           # the group checks of get_covariance
    no(-1, spec_with(group=-2))
    no(-1, spec_with(which="copies", group=GROUP))
    no(-1, spec_with(which="copies"))                                     # no plan applied yet
    assert not cr.differing(before, everything(g))
    # a target whose row is not set, and a group without labels
    cfg, st = tcs.testcase4(8, nlayer=12, n_top=4, n_bottom=4)
    tiny = samsim_amd.hip_solver(cfg, 8)
    tiny.set_state(st)
    refused(-1, lambda: tiny.jitter(good))
    refused(-1, lambda: tiny.jitter(good[:1], group=0))
    refused(-1, lambda: tiny.get_ocean())
    refused(-1, lambda: tiny.ensemble_stats([ocean_slot(0)]))
    assert tiny.jitter(good[:1])["n_written"] == 8
    tiny.close()
    # a plan without copies: nothing to do, and that is not an error
    g.set_weights("thickness", "gauss", 1e300)
    assert (g.weights() == 1.0).all()
    g.resample(300, "systematic", 0.5)
    assert g.apply_resample(forcing=True)["n_copies"] == 0
    mid = everything(g)
    assert g.jitter(good, "copies", 5) == {"n_written": 0, "n_lo": [0, 0], "n_hi": [0, 0]}
    no(-1, spec_with(which="copies", group=GROUP))
    assert not cr.differing(mid, everything(g)) and not cr.differing(before, mid)
    # and a good call still goes through
    assert g.jitter(good, "pool", 5, GROUP)["n_written"] == (labels(300) == GROUP).sum()
    g.close()
