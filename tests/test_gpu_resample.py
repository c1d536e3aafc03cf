"""The posterior draw on the GPU (samsim_resample, samsim_get_offspring, samsim_get_ancestors, SAMSIM_OFFSPRING_SLOT): the ensemble
resampled by its weight row, indices only.  The oracle is tests/resample_reference.py applied to the downloaded weight row, the
status and the labels of the same handle; every comparison with it is bit for bit, sum_w included -- the header fixes the bracketing
of the cumulative weight, so there is nothing to tolerate.

Independent of the oracle: the sum of the offspring is m, the ancestors ascend and their bincount is the offspring row, no column
without a positive weight, with a STOP code or with a foreign label is drawn, |N_c - m w_c / W| <= 1 + 1e-6 (systematic: the exact
bound is 1, and the rounding of C over 70 001 columns moves a t_c by at most 70 001 x 2^-53 x 210 004 = 1.6e-6 of a draw point's
spacing, which can only matter to a point that close to a boundary) and < 2 + 1e-6 (stratified); integer weights against exact
rational arithmetic.

The large handle (70 001 columns: 1 094 blocks, per = 2, 547 ranges, a ragged last block, three stopped columns, the last column
among them) has 12 layers and is never stepped: its weight rows are DIRECT and GAUSS rows of per-column scalars uploaded with the
state.  The small one (4 197 columns, labels) is the scored twin experiment of tests/test_gpu_weights.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import bench
import samsim_amd
from samsim_amd import capi, testcases as tcs
from samsim_amd.capi import S, ResampleInfo, ResampleSpec, SamsimError, offspring_slot, weight_slot
from tests import resample_reference as rr
from tests.test_gpu_group_stats import labels_of_test_1
from tests.test_gpu_profile_stats import ensemble
from tests.test_gpu_weights import J_SUM, scored_ensemble, snapshot

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
U0_LAST = 1.0 - 2.0 ** -53
NCOL = 70001
STOPPED = (5, 40000, 70000)
ONLY = 12345                                   # the one column of group 9 (labels_of_test_1); group 10 is empty
BEST = 45678                                   # the best member of the degenerate posterior
FIRST_OF_RANGE, LAST_OF_BLOCK = 128 * 300, 64 * 501 + 63
# the per-column scalars of the large handle that serve as weight sources (diagnostics an upload carries; the two perturbation
# slots belong to the forcing)
R_RAND, R_INT, R_ONE, R_DEG, R_TWO = "energy_stored", "total_resist", "fl_rest", "melt_err", "freshwater"
DRAWS = [("systematic", 0.0, 0), ("systematic", 0.73, 0), ("systematic", U0_LAST, 0), ("stratified", 0.0, 20261021)]


@pytest.fixture(scope="module")
def big():
    assert rr.grid_rule(NCOL) == (1094, 2, 547) and NCOL % 64 != 0 and STOPPED[-1] == NCOL - 1
    rng = np.random.default_rng(22)
    cfg, st = tcs.testcase4(NCOL, nlayer=12, n_top=4, n_bottom=4)
    rows = {}
    rows[R_RAND] = np.where(rng.uniform(size=NCOL) < 0.2, np.where(rng.uniform(size=NCOL) < 0.5, 0.0, -1.0), rng.exponential(1.0, NCOL))
    rows[R_RAND][ONLY] = 0.7
    rows[R_INT] = rng.integers(0, 6, NCOL).astype(np.float64)
    rows[R_ONE] = np.ones(NCOL)
    rows[R_DEG] = 1.0 + rng.uniform(0.001, 5.0, NCOL)
    rows[R_DEG][BEST] = 0.5
    two = np.zeros(NCOL)
    two[FIRST_OF_RANGE], two[LAST_OF_BLOCK] = 1.0, 0.5
    two[[FIRST_OF_RANGE - 1, FIRST_OF_RANGE + 1, LAST_OF_BLOCK - 1, LAST_OF_BLOCK + 1, 3, NCOL - 2]] = 1.0e-4
    rows[R_TWO] = two
    for name, r in rows.items():
        st.sc(name)[:] = r
    g = samsim_amd.hip_solver(cfg, NCOL)
    g.set_state(st)
    g.set_clock()
    for c in STOPPED:
        g.set_status(np.array([7], dtype=np.int32), col0=c)
    lab = labels_of_test_1(NCOL)
    g.set_groups(lab, ngroups=11)
    status = g.get_status()[0]
    assert sorted(np.flatnonzero(status)) == list(STOPPED) and lab[ONLY] == 9 and (lab == 10).sum() == 0
    for a in (status, lab, *rows.values()):
        a.setflags(write=False)
    return dict(g=g, status=status, lab=lab, rows=rows)


@pytest.fixture(scope="module")
def small():
    """4 197 columns (65 blocks + 37 columns: 66 ranges of one block), two stopped, labels 0..2 with -1s, scored against member 77"""
    ncol = 4197
    lab = (np.arange(ncol) % 3).astype(np.int32)
    lab[::7] = -1
    g, status = scored_ensemble(ncol, (5, 3000), lab, 3, 77)
    J = g.scores()["J_SUM"]
    scale = float(np.median(J[(status == 0) & (J > 0.0)])) / 2.0
    for a in (status, lab):
        a.setflags(write=False)
    return dict(g=g, status=status, lab=lab, scale=scale)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def draw(g, m, kind="systematic", u0=0.0, seed=0, group=None):
    info = g.resample(m, kind, u0, seed, group)
    return info, g.offspring(), g.ancestors()


def check_reference(g, w, status, lab, m, kind, u0, seed, group, what):
    """offspring row, ancestor list and info against the reference, bit for bit; returns the reference"""
    info, N, anc = draw(g, m, kind, u0, seed, group)
    r = rr.resample(w, status, lab, group, m, kind, u0, seed)
    assert bits([info["sum_w"]])[0] == bits([r["info"]["sum_w"]])[0], (what, info["sum_w"], r["info"]["sum_w"])
    assert info == r["info"], (what, info, r["info"])
    assert bits(N).tolist() == bits(r["offspring"]).tolist(), what
    assert anc.size == info["m_drawn"] and np.array_equal(anc, r["ancestors"]), what
    return r


def check_invariants(info, N, anc, w, counts_, m, kind, what):
    """what a resampler owes whatever the reference says: counts_ = the columns that count"""
    assert info["m_drawn"] == m == anc.size and N.sum() == m and (N >= 0).all() and (N == np.round(N)).all(), what
    assert (np.diff(anc) >= 0).all() and anc[0] >= 0 and anc[-1] < N.size, what
    assert np.array_equal(np.bincount(anc, minlength=N.size), N.astype(np.int64)), what
    assert not N[~counts_].any() and counts_[anc].all(), what
    assert info["n_pos"] == counts_.sum() and info["n_survivors"] == (N >= 1).sum() == np.unique(anc).size, what
    assert info["max_offspring"] == N.max() and info["argmax_offspring"] == np.argmax(N), what
    W = float(np.sum(w[counts_].astype(np.longdouble)))
    dev = float(np.abs(N[counts_] - m * w[counts_] / W).max())
    print(what, "max |N - m w / W| =", dev)
    assert dev <= 1.0 + 1e-6 if kind == "systematic" else dev < 2.0 + 1e-6, (what, dev)


# ------------------------------------------------------------------------------------------- 1: the reference, bit for bit
@pytest.mark.parametrize("group", [None, 3, 9, 10])
def test_the_reference_bit_for_bit_on_the_large_handle(big, group):
    g, status, lab = big["g"], big["status"], big["lab"]
    g.set_weights(R_RAND, "direct")
    w = g.weights()
    assert bits(w).tolist() == bits(np.where((status == 0) & (big["rows"][R_RAND] > 0.0), big["rows"][R_RAND], 0.0)).tolist()
    counts_ = rr.terms_of(w, status, lab, group)[1]
    n_in = int((rr.terms_of(np.ones(NCOL), status, lab, group)[1]).sum())
    assert n_in == {None: NCOL - 3, 9: 1, 10: 0}.get(group, n_in) and (group != 3 or 6000 < n_in < 8000)
    for m in (1, 63, 64, 65, max(n_in, 1), 3 * NCOL + 1):
        for kind, u0, seed in DRAWS:
            what = f"group {group}, m {m}, {kind}, u0 {u0}"
            r = check_reference(g, w, status, lab, m, kind, u0, seed, group, what)
            if group == 10:
                assert r["info"] == dict(n_pos=0, m_drawn=0, n_survivors=0, max_offspring=0, argmax_offspring=0, sum_w=0.0), what
                assert g.ancestors().size == 0 and not g.offspring().any()
            else:
                assert (np.diff(r["C"]) >= 0.0).all()
                check_invariants(r["info"], r["offspring"], r["ancestors"], w, counts_, m, kind, what)
            if group == 9:
                assert (r["ancestors"] == ONLY).all() and r["info"]["max_offspring"] == m and r["info"]["argmax_offspring"] == ONLY


def test_the_reference_bit_for_bit_on_the_scored_ensemble(small):
    g, status, lab = small["g"], small["status"], small["lab"]
    g.set_weights(J_SUM, "gauss", small["scale"])
    w = g.weights()
    assert (w > 0.0).sum() > 1000 and np.unique(w).size > 50
    for group in (None, 1):
        counts_ = rr.terms_of(w, status, lab, group)[1]
        for m in (1, 64, int(counts_.sum()), 3 * g.ncol + 1):
            for kind, u0, seed in DRAWS:
                what = f"small, group {group}, m {m}, {kind}, u0 {u0}"
                r = check_reference(g, w, status, lab, m, kind, u0, seed, group, what)
                check_invariants(r["info"], r["offspring"], r["ancestors"], w, counts_, m, kind, what)


# ---------------------------------------------------------------------------------------- 2: independent of the reference
def test_integer_weights_against_exact_rational_arithmetic(big):
    """DIRECT on a row of small integers: every C_c is an exact integer, so t_c = C_c m / W is known as a fraction and K(t_c) =
    clip(ceil(t_c - u0), 0, m) follows without a rounding -- provided no draw point lies within 1e-6 of a boundary t_c, which the
    test asserts about its own input first"""
    g, status = big["g"], big["status"]
    info_w = g.set_weights(R_INT, "direct")
    w = g.weights()
    assert (w == np.round(w)).all() and w.max() == 5.0 and (w == 0.0).sum() > 10000 and info_w["sum_w"] == w.sum()
    Wi = int(w.sum())
    Ci = np.cumsum(w.astype(np.int64))
    for m, u0 in ((NCOL, 0.73), (3 * NCOL + 1, 0.3)):
        u = Fraction(u0)                                                  # the double's exact value
        x = [Fraction(int(c) * m, Wi) - u for c in Ci]
        gap = min(abs(v - round(v)) for v in x)
        assert gap > Fraction(1, 10 ** 6), (m, u0, float(gap))
        K = np.array([min(max(-((-v.numerator) // v.denominator), 0), m) for v in x], dtype=np.int64)
        K[Ci == Wi] = m
        want = np.diff(K, prepend=np.int64(0))
        info, N, anc = draw(g, m, "systematic", u0)
        assert np.array_equal(N.astype(np.int64), want), (m, u0)
        assert np.array_equal(anc, np.repeat(np.arange(NCOL), want)) and info["sum_w"] == float(Wi) and info["m_drawn"] == m


@pytest.mark.parametrize("which", ["large", "identical"])
def test_unit_weights_draw_every_counting_column_once(big, which):
    if which == "large":
        g, status = big["g"], big["status"]
        g.set_weights(R_ONE, "direct")
    else:
        cfg, st = tcs.testcase1(256)
        g = samsim_amd.hip_solver(cfg, 256)
        g.set_state(st)
        g.set_clock()
        g.step(10)
        status = g.get_status()[0]
        g.set_weights("precip_scale", "direct")
    running = np.flatnonzero(status == 0)
    assert (g.weights()[running] == 1.0).all()
    for kind, u0, seed in (("systematic", 0.5, 0), ("stratified", 0.0, 99)):
        info, N, anc = draw(g, running.size, kind, u0, seed)
        assert np.array_equal(anc, running) and (N[running] == 1.0).all() and N.sum() == running.size, (which, kind)
        assert info["n_survivors"] == running.size == info["n_pos"] and info["max_offspring"] == 1 and info["argmax_offspring"] == running[0]
        assert info["sum_w"] == float(running.size)


# ---------------------------------------------------------------------------------------- 3: the degenerate posterior
def test_one_member_takes_every_draw(big):
    g = big["g"]
    info_w = g.set_weights(R_DEG, "gauss", 1e-9)
    w = g.weights()
    assert w[BEST] == 1.0 and w.sum() == 1.0 and info_w["n_pos"] == 1 and info_w["x_min"] == 0.5
    for m in (100_000, capi.RESAMPLE_MAX_DRAWS):
        for kind, u0, seed in (("systematic", 0.73, 0), ("stratified", 0.0, 3)):
            info, N, anc = draw(g, m, kind, u0, seed)
            assert anc.size == m and (anc == BEST).all(), (m, kind)
            assert info == dict(n_pos=1, m_drawn=m, n_survivors=1, max_offspring=m, argmax_offspring=BEST, sum_w=1.0)
            assert N[BEST] == m and N.sum() == m


def test_heavy_columns_beside_light_ones(big):
    """two members at 1.0 and 0.5 -- one the first lane of a range, one the last lane of a block -- with six at 1e-4 around them: the
    wave's cooperative fill next to the lanes' own"""
    g, status, lab = big["g"], big["status"], big["lab"]
    g.set_weights(R_TWO, "direct")
    w = g.weights()
    assert FIRST_OF_RANGE % (2 * 64) == 0 and LAST_OF_BLOCK % 64 == 63 and (w > 0.0).sum() == 8 and w[NCOL - 2] == 1e-4
    counts_ = w > 0.0
    for m in (100_000, 400_003, 64 * 3 + 5):
        for kind, u0, seed in DRAWS[1:]:
            what = f"two heavy, m {m}, {kind}"
            r = check_reference(g, w, status, lab, m, kind, u0, seed, None, what)
            check_invariants(r["info"], r["offspring"], r["ancestors"], w, counts_, m, kind, what)
            N = r["offspring"]
            if m >= 100_000:
                assert N[FIRST_OF_RANGE] >= 64 and N[LAST_OF_BLOCK] >= 64 and 1 <= N[FIRST_OF_RANGE + 1] < 64 and 1 <= N[LAST_OF_BLOCK - 1] < 64
            assert r["info"]["argmax_offspring"] == FIRST_OF_RANGE


# ------------------------------------------------------------------------------------------------ 4: the offspring slot
def test_the_offspring_row_as_a_slot(small):
    g, status, lab = small["g"], small["status"], small["lab"]
    g.set_weights(J_SUM, "gauss", small["scale"])
    m = 2 * g.ncol
    info, N, anc = draw(g, m, "systematic", 0.37)
    ok = status == 0
    slot = offspring_slot()
    nv = int(N.max()) + 2
    edges = np.concatenate([[-np.inf], -0.5 + np.arange(nv + 1), [np.inf]])
    want = np.histogram(N[ok], bins=edges)[0]
    got = g.histogram(slot, nv, -0.5, 1.0)
    assert np.array_equal(got, want) and got[0] == 0 and got[-1] == 0 and (got[1:-1] > 0).sum() >= 3
    by = g.histogram(slot, nv, -0.5, 1.0, by_group=True)
    assert all(np.array_equal(by[k], np.histogram(N[ok & (lab == k)], bins=edges)[0]) for k in range(3))
    idx, n = g.select([(slot, 1.0, INF)])
    assert np.array_equal(idx, np.unique(anc)) and n == info["n_survivors"] and 0 < n < ok.sum()
    st = g.ensemble_stats([slot])[slot]
    assert st.count == ok.sum() and st.min == 0.0 and st.max == info["max_offspring"] and abs(st.mean * st.count - m) <= 1e-9 * m
    per_site = g.group_stats([slot])[slot]
    assert [int(round(per_site["mean"][k] * per_site["count"][k])) for k in range(3)] == [int(N[ok & (lab == k)].sum()) for k in range(3)]
    # the offspring as weights of the next statistics, and the weight row still what it was
    assert g.weighted_stats([slot])[slot]["count"] == (g.weights() > 0.0).sum()
    g.clear_resample()
    for call in (lambda: g.histogram(slot, 4, 0.0, 1.0), lambda: g.select([(slot, 1.0, INF)]), lambda: g.ensemble_stats([slot]),
                 lambda: g.offspring(), lambda: g.ancestors(0, 0)):
        with pytest.raises(SamsimError) as e:
            call()
        assert e.value.code == -1
    g.clear_resample()                                                    # also when there are no rows


# ------------------------------------------------------------------------------------------------ 5: closing the loop
def test_the_resampled_columns_step_as_their_ancestors():
    ncol, m = 300, 500
    g = ensemble("sheba_ensemble_80.npz", ncol, 3)
    assert not g.get_status()[0].any()
    g.set_weights("thickness", "gauss", 0.05)
    info, N, anc = draw(g, m, "stratified", seed=11)
    assert 10 < info["n_survivors"] < ncol and info["max_offspring"] >= 2
    k0, nk = 100, 300
    window = anc[k0:k0 + nk]
    got = g.resampled_columns(k0, nk)
    full = g.get_state()
    assert got.lay.tobytes() == np.ascontiguousarray(full.lay[..., window]).tobytes()
    assert got.scal.tobytes() == np.ascontiguousarray(full.scal[..., window]).tobytes()
    assert got.n_active.tobytes() == np.ascontiguousarray(full.n_active[window]).tobytes()
    # a second handle continues from the copies: same forcing perturbations, same clock
    _, _, _, pert = bench.load_ensemble("sheba_ensemble_80.npz")
    h = samsim_amd.hip_solver(g.cfg, nk)
    h.set_forcing(*bench.sheba_forcing(), bench.tile(pert[0], ncol)[window], bench.tile(pert[1], ncol)[window])
    h.set_state(got)
    k = g.get_clock()
    h.set_clock(time=k.time, step=k.step, n_time_out=k.n_time_out, time_counter=k.time_counter, n_outputs=k.n_outputs)
    h.set_output_window(0, 0)
    g.step(5)
    h.step(5)
    a, b = g.get_state(), h.get_state()
    assert not h.get_status()[0].any()
    # (the prognostic arrays, the scalars and N_active: what a restart from a full state continues bit for bit, as
    # tests/test_gpu_ensemble_io.py has it for checkpoints)
    assert b.lay[:capi.NPROG].view(np.uint64).tobytes() == np.ascontiguousarray(a.lay[:capi.NPROG, :, window]).view(np.uint64).tobytes()
    assert b.scal.view(np.uint64).tobytes() == np.ascontiguousarray(a.scal[..., window]).view(np.uint64).tobytes()
    assert np.array_equal(b.n_active, a.n_active[window])
    # the rows outlive the steps, an upload and a new weight row: they describe the weights as they were at the call
    g.set_state(g.get_state(0, 10), 0)
    g.set_weights("N_active", "direct")
    assert g.offspring().tobytes() == N.tobytes() and g.ancestors().tobytes() == anc.tobytes()
    h.close()
    g.close()


# ------------------------------------------------------------------------------------- 6: read-only and deterministic
def test_the_calls_are_deterministic_and_write_nothing_else(small):
    g, status, lab = small["g"], small["status"], small["lab"]
    g.set_weights(J_SUM, "gauss", small["scale"])
    g.clear_resample()
    w = g.weights()
    before = snapshot(g)

    def everything(group):
        out = []
        for m in (3 * g.ncol + 1, 1000):
            for kind, u0, seed in DRAWS[1:]:
                info, N, anc = draw(g, m, kind, u0, seed, group)
                out.append((tuple(sorted(info.items())), N.tobytes(), anc.tobytes()))
        return out
    first = {group: everything(group) for group in (None, 1)}
    assert snapshot(g) == before and g.weights().tobytes() == w.tobytes()
    assert {group: everything(group) for group in (None, 1)} == first
    # relabelling the columns outside group 1 changes nothing of group 1's draw
    other = lab.copy()
    other[lab != 1] = np.where(lab[lab != 1] == 0, 2, -1)
    try:
        g.set_groups(other, ngroups=3)
        assert everything(1) == first[1]
    finally:
        g.set_groups(lab, ngroups=3)
    # a smaller m after a larger one: what lies behind m_drawn is out of the window
    draw(g, 5000)
    info, N, anc = draw(g, 100)
    assert anc.size == 100 and g.m_drawn == 100
    buf = np.full(5000, -77, dtype=np.int64)
    raw = g._f("get_ancestors")
    for k0, nk in ((0, 101), (0, 5000), (100, 1), (101, 0), (-1, 2), (0, -1), (50, 51)):
        assert raw(g._h, k0, nk, buf.ctypes.data) == -1, (k0, nk)
    assert (buf == -77).all()
    assert raw(g._h, 100, 0, buf.ctypes.data) == 0 and raw(g._h, 40, 60, buf.ctypes.data) == 0
    assert np.array_equal(buf[:60], anc[40:]) and (buf[60:] == -77).all()
    assert snapshot(g) == before and g.weights().tobytes() == w.tobytes()


# ------------------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_in_the_documented_order(small):
    g, status, lab = small["g"], small["status"], small["lab"]
    g.set_weights(J_SUM, "gauss", small["scale"])
    _, row, anc = draw(g, 777, "systematic", 0.25, group=1)

    def refused(code, call):
        with pytest.raises(SamsimError) as e:
            call()
        assert e.value.code == code, (e.value.code, code)
        assert g.offspring().tobytes() == row.tobytes() and g.ancestors(0, 777).tobytes() == anc.tobytes()   # the rows in force

    def spec(kind="systematic", **kw):
        sp = ResampleSpec.make(500, kind, 0.5 if kind == "systematic" else 0.0, 0 if kind == "systematic" else 9, 1)
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp
    info = ResampleInfo(-7, -7, -7, -7, -7, -77.0)
    refused(-1, lambda: g.resample_raw(None, info))                       # NULL spec asks for removal: no info then
    refused(-6, lambda: g.resample_raw(spec(struct_size=36, kind=5), info))   # the size comes before the kind
    refused(-6, lambda: g.resample_raw(spec(struct_size=48), info))
    for kind in (2, -1):
        refused(-1, lambda: g.resample_raw(spec(kind=kind), info))
    for group in (3, -2, 99):
        refused(-1, lambda: g.resample_raw(spec(group=group), info))
    for m in (0, -1, capi.RESAMPLE_MAX_DRAWS + 1, 1 << 40):
        refused(-1, lambda: g.resample_raw(spec(m=m), info))
    for u0 in (1.0, -0.25, -U0_LAST, 2.0, INF, NAN):
        refused(-1, lambda: g.resample_raw(spec(u0=u0), info))
    refused(-1, lambda: g.resample_raw(spec(seed=1), info))               # SYSTEMATIC takes no seed
    for u0 in (0.5, U0_LAST, NAN):
        refused(-1, lambda: g.resample_raw(spec("stratified", u0=u0), info))   # STRATIFIED takes no offset
    for kind in ("systematic", "stratified"):
        refused(-1, lambda: g.resample_raw(spec(kind, reserved=1), info))
    assert (info.n_pos, info.m_drawn, info.n_survivors, info.max_offspring, info.argmax_offspring, info.sum_w) == (-7, -7, -7, -7, -7, -77.0)
    # without a weight row: refused, and the rows of the last draw stay
    g.clear_weights()
    try:
        refused(-1, lambda: g.resample_raw(spec(), info))
        refused(-6, lambda: g.resample_raw(spec(struct_size=0), info))    # the size still comes first
        assert np.array_equal(g.select([(offspring_slot(), 1.0, INF)])[0], np.unique(anc))
    finally:
        g.set_weights(J_SUM, "gauss", small["scale"])
    # without labels a group is refused, -1 is not
    g.set_groups(None)
    try:
        refused(-1, lambda: g.resample(500, group=0))
    finally:
        g.set_groups(lab, ngroups=3)
    # the getters
    out, idx = np.full(8, -77.0), np.full(8, -77, dtype=np.int64)
    raw = g._f("get_offspring")
    assert raw(g._h, 0, 8, None) == -1
    for col0, n in ((-1, 4), (0, -1), (g.ncol - 3, 4), (g.ncol + 1, 0), (0, g.ncol + 1)):
        assert raw(g._h, col0, n, out.ctypes.data) == -1, (col0, n)
    raw = g._f("get_ancestors")
    assert raw(g._h, 0, 8, None) == -1
    for k0, nk in ((-1, 4), (0, -1), (775, 4), (778, 0), (0, 778)):
        assert raw(g._h, k0, nk, idx.ctypes.data) == -1, (k0, nk)
    assert (out == -77.0).all() and (idx == -77).all()
    # the specs themselves are good; info may be NULL
    g.resample_raw(spec(), None)
    g.resample_raw(spec("stratified"), None)
    assert g.offspring().sum() == 500 and g.ancestors(0, 500).size == 500 and (lab[g.ancestors(0, 500)] == 1).all()
    assert weight_slot() != offspring_slot() and S["thickness"] >= 0 and C.sizeof(ResampleSpec) == 40
