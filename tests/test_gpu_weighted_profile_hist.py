"""The weighted joint histogram of the layer profiles on the GPU (samsim_get_weighted_profile_histogram): per depth bin x value
entry the sum of the weights of samsim_set_weights, from which the posterior median and band of a profile follow.  The oracle is
tests/weighted_profile_hist_reference.py applied to get_state(), get_status(), the labels and the downloaded weight row of the same
handle.

The bar, derived and not measured: |got - want| <= 1e-12 want against math.fsum, and got == +0.0 exactly where want == 0.  An
entry's sum passes through at most 64 ceil(1 094 / G) additions in a wave, ceil(G / 64) in a lane of the merge and 64 across its
lanes, all of positive terms: at most 1 217 for any grid G in [64, 1 024], 1 217 x 2^-53 = 1.4e-13 relative.  The value edges come
from the reference's own bin values (their 5 % and 95 % quantiles), so both outer entries and several interior ones hold weight;
the tests assert that on the reference."""
import ctypes as C

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi, testcases as tcs
from samsim_amd.capi import S, SamsimError, SensorSpec, State, score_slot
from tests import hist_reference as hr
from tests import weighted_profile_hist_reference as whr
from tests import weighted_profile_reference as wpr
from tests import weights_reference as wr
from tests.profile_reference import column_thickness
from tests.test_gpu_group_stats import labels_of_test_1
from tests.test_gpu_profile_stats import ensemble, pick_dz
from tests.test_gpu_weights import BUOY, CORRUPT, J_SUM, MEMBER, bits, scored_ensemble, snapshot

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
NV64 = 59                                      # the most value bins at which a pass still serves 64 depth bins
NVBINS = (1, NV64, capi.HIST_MAX_VBINS)
assert capi.wphist_chunk(NV64) == 64 and capi.wphist_chunk(NV64 + 1) < 64 and capi.wphist_chunk(254) == 25


@pytest.fixture(scope="module")
def big():
    """70 001 columns x 80 layers: 1 094 blocks of 64, more than any grid the reduction may run, so every wave takes several trips
    and a lane of the merge several waves, and a ragged tail of 49; three columns stopped; eleven labels with -1s, one group of one
    column, one empty; GAUSS weights on the accumulated misfit of a twin experiment, tempered so that the median member keeps
    exp(-1) of the best member's weight.  The tests read reductions; a test that sets another weight row puts this one back."""
    ncol = 70001
    assert (ncol + 63) // 64 == 1094 and ncol % 64 == 49
    lab = labels_of_test_1(ncol)
    g, status = scored_ensemble(ncol, CORRUPT, lab, 11, MEMBER)
    s = g.get_state()
    J = g.scores()["J_SUM"]
    ok = status == 0
    scale = float(np.median(J[ok & (J > 0.0)])) / 2.0
    assert np.isfinite(scale) and scale > 0.0
    info = g.set_weights(J_SUM, "gauss", scale)
    w = g.weights()
    assert info["n_in"] == ncol - 3 and info["ess"] >= info["n_in"] / 10.0 and len(set(w[ok].tolist())) > 100
    H = column_thickness(s)
    for a in (s.lay, s.scal, s.n_active, status, lab, w, H):
        a.setflags(write=False)
    return dict(g=g, s=s, status=status, lab=lab, w=w, scale=scale, H=H, cache={}, groups=(None, int(lab[MEMBER + 256]), 9, 10))


@pytest.fixture(scope="module")
def small():
    """4 197 columns (65 blocks + 37 columns), two of them stopped, labels 0..2 with -1s; one running column's misfit is a NaN, so
    its weight is 0"""
    ncol = 4197
    lab = (np.arange(ncol) % 3).astype(np.int32)
    lab[::7] = -1
    g = ensemble("sheba_ensemble_80.npz", ncol, 0, corrupt=(5, 3000))
    g.set_output_window(0, 8)
    g.set_tracks([capi.TrackSpec.make("ice_thickness")], 1)
    g.step(3)
    g.set_functionals([capi.FunctionalSpec.make("thickness_where", "psi_l", sense=1, threshold=0.05)])
    g.set_groups(lab, ngroups=3)
    status = g.get_status()[0]
    assert sorted(np.flatnonzero(status)) == [5, 3000]
    c_nan = 1000
    one = g.get_state(c_nan, 1)
    one.scal[S["melt_err"]] = NAN
    g.set_state(one, c_nan)
    g.set_sensors(BUOY + [SensorSpec.make("scalar", "melt_err")])
    g.score(g.sensor_values([77])[:, 0])
    s, J = g.get_state(), g.scores()["J_SUM"]
    assert np.isnan(J[c_nan]) and np.isnan(J).sum() == 1
    finite = J[(status == 0) & ~np.isnan(J)]
    scale = float(np.median(finite[finite > 0.0])) / 2.0
    info = g.set_weights(J_SUM, "gauss", scale)
    w = g.weights()
    assert w[c_nan] == 0.0 and status[c_nan] == 0 and info["n_pos"] >= 100
    H = column_thickness(s)
    for a in (s.lay, s.scal, s.n_active, status, lab, w, H):
        a.setflags(write=False)
    return dict(g=g, s=s, status=status, lab=lab, w=w, scale=scale, H=H, c_nan=c_nan, cache={}, groups=(None, int(lab[c_nan]), 2))


@pytest.fixture(scope="module")
def same():
    """256 copies of one column (testcase 1), with weights that differ: the columns with label 1 are scored twice, the others
    once, and DIRECT on CALLS makes the row 2.0 and 1.0"""
    ncol = 256
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    g.step(4000)
    assert not g.get_status()[0].any()
    lab = (np.arange(ncol) % 5 == 1).astype(np.int32)
    g.set_groups(lab, ngroups=2)
    g.set_sensors([SensorSpec.make("ice_thickness")])
    obs = g.sensor_values([0])[:, 0]
    g.score(obs)
    g.score(obs, group=1)
    g.set_weights(score_slot("CALLS"), "direct")
    w = g.weights()
    assert bits(w).tolist() == bits(np.where(lab == 1, 2.0, 1.0)).tolist()
    return g, g.get_state(), lab, w


def depth_request(H_ok, nbins):
    """nbins depth bins of which the last four lie below (above) every column: nbins - 4 bins reach the thickest one"""
    base = float(H_ok.max()) / (nbins - 4)
    dz = pick_dz(H_ok, (base, 1.01 * base, 0.99 * base, 1.02 * base), nbins, (0.0,))
    assert dz is not None and nbins * dz > H_ok.max()
    return dict(axis="depth", nbins=nbins, z0=0.0, dz=dz)


def key_of(name, kw):
    return (name,) + tuple(sorted(kw.items()))


def reference_values(f, name, kw):
    """(v, has) of hist_reference.profile_values, computed once per fixture, array and request and left unchanged"""
    key = key_of(name, kw)
    if key not in f["cache"]:
        v, has = hr.profile_values(f["s"], f["status"], name, **kw)
        v.setflags(write=False)
        has.setflags(write=False)
        f["cache"][key] = (v, has)
    return f["cache"][key]


def edges_from(v, has, ok, nvbins):
    """(v0, dv): the value bins span the 5 % .. 95 % quantiles of the counting columns' bin values"""
    lo, hi = np.quantile(v[has & ok[None, :]], [0.05, 0.95])
    assert np.isfinite(lo) and hi > lo
    return float(lo), float((hi - lo) / nvbins)


def edges_of_request(f, name, kw, nvbins):
    """edges_from over the running columns of the fixture, for the tests that only need value bins that spread the data"""
    v, has = reference_values(f, name, kw)
    v0, dv = edges_from(v, has, f["status"] == 0, nvbins)
    print(name, kw["axis"], kw["origin"], "| value bins from", v0, "by", dv, "x", nvbins)
    return v0, dv


def check_table(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64
    zero = want == 0.0
    assert (bits(got[zero]) == 0).all(), what                                   # +0.0, not a rounding and not -0.0
    assert (got[~zero] > 0.0).all(), what
    ratio = np.abs(got[~zero] - want[~zero]) / (1e-12 * want[~zero])
    print(what, "| entries with weight", int((~zero).sum()), "| worst error / bar", float(ratio.max(initial=0.0)))
    assert (ratio <= 1.0).all(), what


def against_reference(f, name, kw):
    g, status, lab, w = f["g"], f["status"], f["lab"], f["w"]
    v, has = reference_values(f, name, kw)
    every = wpr.counting(status, w)
    if kw["axis"] == "depth":                  # bins that are empty, bins with a strict subset of the counting columns, bins with all
        cnt = (has & every[None, :]).sum(1)
        assert (cnt == 0).any() and ((cnt > 0) & (cnt < every.sum())).any() and cnt.max() == every.sum(), (name, kw)
    for nvbins in NVBINS:
        assert -(-kw["nbins"] // capi.wphist_chunk(nvbins)) >= (2 if kw["nbins"] > 64 else 1)
        v0, dv = edges_from(v, has, every, nvbins)
        en = whr.entries_of_bins(v, has, nvbins, v0, dv)
        for group in f["groups"]:
            ok = wpr.counting(status, w, lab, group)
            want = whr.table_from_entries(en, w, ok, nvbins)
            if group is None:                  # both outer entries and several interior ones of some row hold weight
                assert (want[:, 0] > 0.0).any() and (want[:, -1] > 0.0).any(), (name, kw, nvbins)
                assert (want[:, 1:-1] > 0.0).sum(1).max() >= min(3, nvbins), (name, kw, nvbins)
            elif not ok.any():
                assert not want.any()
            got = g.weighted_profile_histogram(name, nvbins, v0, dv, group=group, **kw)
            check_table(got, want, f"{name}/{kw['axis']}/{kw['origin']}/{kw['nbins']}/nvbins {nvbins}/group {group}")


# ------------------------------------------------------------------------------------------------- 1: against the reference
@pytest.mark.parametrize("name", ["T", "S_bu"])
@pytest.mark.parametrize("origin", ["top", "bottom"])
def test_by_layer_against_the_reference(big, name, origin):
    """80 layer bins are two passes at 1 and 59 value bins (64 + 16) and four at 254 (25 + 25 + 25 + 5); 1 094 blocks are more than
    the grid's waves"""
    assert big["w"][MEMBER] == 1.0 and (big["lab"] == 9).sum() == 1 and (big["lab"] == 10).sum() == 0
    against_reference(big, name, dict(axis="layer", origin=origin, nbins=80))


@pytest.mark.parametrize("name,origin", [("S_bu", "top"), ("T", "bottom")])
def test_by_depth_against_the_reference(big, name, origin):
    """the depth axis on the large ensemble, 16 bins (the reference forms a [bins, columns] table per layer)"""
    dq = depth_request(big["H"][big["status"] == 0], 16)
    against_reference(big, name, dict(origin=origin, **dq))


@pytest.mark.parametrize("name", ["T", "S_bu"])
@pytest.mark.parametrize("origin", ["top", "bottom"])
def test_more_depth_bins_than_a_pass_serves_with_a_nan_misfit(small, name, origin):
    """70 depth bins: two passes at 1 and 59 value bins, three at 254, from either origin all but one with `lead`"""
    dq = depth_request(small["H"][small["status"] == 0], 70)
    against_reference(small, name, dict(origin=origin, **dq))


# ------------------------------------------------------------------------------------------------- 2: the properties of the header
def test_unit_weights_are_the_counts_bit_for_bit(big):
    g, status, lab, scale = big["g"], big["status"], big["lab"], big["scale"]
    dq = depth_request(big["H"][status == 0], 70)
    k = big["groups"][1]
    try:
        for row_group in (None, k):
            g.set_weights(score_slot("CALLS"), "direct", group=row_group)       # scored once: a row of 0.0 and 1.0
            w = g.weights()
            member = (status == 0) & ((lab == row_group) if row_group is not None else True)
            assert bits(w).tolist() == bits(member.astype(np.float64)).tolist()
            for name, kw, nvbins, v0, dv in (("T", dict(axis="layer", origin="bottom", nbins=80), 254, -12.0, 0.05),
                                              ("S_bu", dict(origin="top", **dq), 40, 0.5, 0.3),
                                              ("psi_l", dict(origin="bottom", **dq), 254, 0.0, 0.002)):
                got = g.weighted_profile_histogram(name, nvbins, v0, dv, **kw)  # group -1: the row alone restricts the columns
                counts = g.profile_histogram(name, nvbins, v0, dv, group=row_group, **kw)
                assert counts.sum() > member.sum() and (counts[:, 1:-1] > 0).sum() > 20
                assert got.tobytes() == counts.astype(np.float64).tobytes(), (name, kw, row_group)
                if row_group is None:          # with labels on top of unit weights: the group call's counts
                    got = g.weighted_profile_histogram(name, nvbins, v0, dv, group=k, **kw)
                    counts = g.profile_histogram(name, nvbins, v0, dv, group=k, **kw)
                    assert got.tobytes() == counts.astype(np.float64).tobytes() and counts.sum() > 0, (name, kw)
    finally:
        g.set_weights(J_SUM, "gauss", scale)
    assert g.weights().tobytes() == big["w"].tobytes()


def test_integer_weights_give_exact_sums(small):
    """DIRECT on N_active (here the same 80 in every running column) and on the score row N_SUM (the sensors that had a value, which
    differ from column to column): every weight is an integer, so every sum of them is exact in any order"""
    g, status, lab = small["g"], small["status"], small["lab"]
    dq = depth_request(small["H"][status == 0], 70)
    try:
        for slot in ("N_active", score_slot("N_SUM")):
            g.set_weights(slot, "direct")
            w = g.weights()
            wi = w.astype(np.int64)
            assert bits(w).tolist() == bits(wi.astype(np.float64)).tolist() and (wi[status == 0] > 0).sum() >= 100
            if slot == "N_active":
                assert np.array_equal(wi, np.where(status == 0, small["s"].n_active, 0))
            print("integer weights from", slot, "| distinct values", sorted(set(wi.tolist())))
            for name, kw in (("T", dict(origin="top", **dq)), ("S_bu", dict(axis="layer", origin="bottom", nbins=80))):
                v, has = reference_values(small, name, kw)
                for nvbins in (NV64, 254):
                    v0, dv = edges_from(v, has, status == 0, nvbins)
                    en = whr.entries_of_bins(v, has, nvbins, v0, dv)
                    for group in (None, 1):
                        ok = wpr.counting(status, w, lab, group)
                        want = np.zeros((kw["nbins"], nvbins + 2), dtype=np.int64)
                        for b in range(kw["nbins"]):
                            use = (en[b] >= 0) & ok
                            np.add.at(want[b], en[b, use], wi[use])                 # integer sums
                        got = g.weighted_profile_histogram(name, nvbins, v0, dv, group=group, **kw)
                        assert want.sum() > 0 and got.tobytes() == want.astype(np.float64).tobytes(), (slot, name, kw, nvbins, group)
    finally:
        g.set_weights(J_SUM, "gauss", small["scale"])
    assert g.weights().tobytes() == small["w"].tobytes()


def test_two_calls_return_the_same_bytes(big):
    g = big["g"]
    dq = depth_request(big["H"][big["status"] == 0], 70)
    for name, kw in (("T", dict(origin="top", **dq)), ("S_bu", dict(axis="layer", origin="bottom", nbins=80))):
        v0, dv = edges_of_request(big, name, kw, 254)
        for group in (None, big["groups"][1]):
            a = g.weighted_profile_histogram(name, 254, v0, dv, group=group, **kw)
            b = g.weighted_profile_histogram(name, 254, v0, dv, group=group, **kw)
            assert (a > 0.0).sum() > 100 and a.tobytes() == b.tobytes(), (name, group)


def test_columns_outside_the_group_change_nothing(small):
    g, status, lab, w = small["g"], small["status"], small["lab"], small["w"]
    dq = depth_request(small["H"][status == 0], 70)
    before = snapshot(g)

    requests = [(name, nvbins, kw) + edges_of_request(small, name, kw, nvbins)
                for name, nvbins, kw in (("T", 254, dict(origin="top", **dq)), ("S_bu", NV64, dict(axis="layer", origin="bottom", nbins=80)))]

    def everything(group):
        tables = [g.weighted_profile_histogram(name, nvbins, v0, dv, group=group, **kw) for name, nvbins, kw, v0, dv in requests]
        assert all((t[:, 1:-1] > 0.0).sum() > 100 for t in tables)
        return tuple(t.tobytes() for t in tables)
    first = everything(1)
    assert everything(1) == first
    # relabelling the columns outside group 1
    other = lab.copy()
    other[lab != 1] = np.where(lab[lab != 1] == 0, 2, -1)
    try:
        g.set_groups(other, ngroups=3)
        assert everything(1) == first
    finally:
        g.set_groups(lab, ngroups=3)
    # re-weighting them: DIRECT on the thickness gives group 1 the same weights with and without the restriction of the row to the
    # group, and the other columns 0.0 or their thickness
    try:
        g.set_weights("thickness", "direct", group=1)
        only = g.weights()
        a = everything(1)
        g.set_weights("thickness", "direct")
        every = g.weights()
        assert bits(every[lab == 1]).tolist() == bits(only[lab == 1]).tolist() and (only[lab != 1] == 0.0).all() and (every[lab != 1] > 0.0).any()
        assert everything(1) == a and a != first
    finally:
        g.set_weights(J_SUM, "gauss", small["scale"])
    assert g.weights().tobytes() == w.tobytes() and snapshot(g) == before and everything(1) == first


def test_a_row_does_not_depend_on_the_number_of_bins(small):
    g = small["g"]
    chunk = capi.wphist_chunk(254)
    dq = depth_request(small["H"][small["status"] == 0], 70)
    for name, kw in (("T", dict(origin="top", **dq)), ("S_bu", dict(axis="layer", origin="top", nbins=80))):
        v0, dv = edges_of_request(small, name, kw, 254)
        whole = g.weighted_profile_histogram(name, 254, v0, dv, **kw)
        for k in (chunk - 1, chunk, chunk + 1):
            part = g.weighted_profile_histogram(name, 254, v0, dv, **dict(kw, nbins=k))
            assert part.shape == (k, 256) and part.tobytes() == whole[:k].tobytes(), (name, k)
            assert (part[:, 1:-1] > 0.0).sum() > 4 * k, (name, k)


def test_row_sums_and_extremes_agree_with_the_weighted_profile_statistics(big):
    g, status = big["g"], big["status"]
    dq = depth_request(big["H"][status == 0], 16)
    k = big["groups"][1]
    for name, kw in (("T", dict(origin="top", **dq)), ("S_bu", dict(axis="layer", origin="bottom", nbins=80))):
        v, has = reference_values(big, name, kw)
        nvbins = 254
        v0, dv = edges_from(v, has, status == 0, nvbins)
        for group in (None, k, 9):
            got = g.weighted_profile_histogram(name, nvbins, v0, dv, group=group, **kw)
            st = g.weighted_profile_stats([name], group=group, **kw)[name]
            full = st["count"] > 0
            assert full.any() and np.array_equal(got.sum(1) > 0.0, full)
            worst = float(np.max(np.abs(got.sum(1) - st["sum_w"])[full] / st["sum_w"][full]))
            print(name, kw["axis"], "group", group, "| row sums against sum_w, worst relative difference", worst)
            assert worst <= 1e-12
            for b in np.flatnonzero(full):
                pos = np.flatnonzero(got[b] > 0.0)
                lo, hi = hr.entries(np.array([st["min"][b], st["max"][b]]), nvbins, v0, dv)
                assert (lo, hi) == (pos[0], pos[-1]), (name, group, b)


# ------------------------------------------------------------------------------------------------- 3: identical columns
def test_identical_columns_put_all_weight_into_one_entry(same):
    g, s, lab, w = same
    H = float(column_thickness(s)[0])
    T = s.arr("T")[:int(s.n_active[0]), 0]
    v0, dv = float(T.min()) - 0.013, float(T.max() - T.min() + 0.03) / 200
    for kw in (dict(axis="layer", origin="top"), dict(axis="layer", origin="bottom"),
               dict(axis="depth", origin="top", nbins=70, z0=0.0, dz=H / 66.3), dict(axis="depth", origin="bottom", nbins=70, z0=0.0, dz=H / 66.3)):
        cnt = g.profile_histogram("T", 200, v0, dv, **kw)
        for group in (None, 1):
            got = g.weighted_profile_histogram("T", 200, v0, dv, group=group, **kw)
            total = float(w.sum()) if group is None else 2.0 * int((lab == 1).sum())
            full = cnt.sum(1) > 0
            assert full.any() and ((~full).any() or kw["axis"] == "layer")
            assert ((got > 0.0).sum(1) == full).all() and np.array_equal(got > 0.0, cnt > 0), (kw, group)
            assert (got[got > 0.0] == total).all() and (bits(got[got == 0.0]) == 0).all(), (kw, group)
            assert (got[full, 1:-1] > 0.0).any()


# ------------------------------------------------------------------------------------------------- 4: the posterior band
@pytest.mark.parametrize("which,nbins", [("big", 16), ("small", 70)])
def test_the_posterior_band_brackets_the_weighted_quantiles(request, which, nbins):
    """the median and the 5-95 % band of T(z) read off the device's table contain the reference's weighted quantiles of every depth
    bin's values.  Where the reference's cumulative weight sits within 1e-12 (relative) of an entry's end the target may fall
    either way; those bins are counted from the reference alone and may be 2 % of the bins at most."""
    f = request.getfixturevalue(which)
    g, status, w = f["g"], f["status"], f["w"]
    kw = dict(origin="top", **depth_request(f["H"][status == 0], nbins))
    v, has = reference_values(f, "T", kw)
    ok = wpr.counting(status, w)
    nvbins = 254
    v0, dv = edges_from(v, has, ok, nvbins)
    want = whr.weighted_joint_histogram(v, has, w, ok, nvbins, v0, dv)
    qs = (0.05, 0.5, 0.95)
    lo, hi = capi.weighted_profile_quantiles(g.weighted_profile_histogram("T", nvbins, v0, dv, **kw), v0, dv, qs)
    held = near = 0
    with_weight = np.flatnonzero(want.sum(1) > 0.0)
    for b in with_weight:
        cum = np.cumsum(want[b].astype(np.longdouble))
        for i, q in enumerate(qs):
            if (np.abs(cum[:-1] - np.longdouble(q) * cum[-1]) <= 1e-12 * cum[-1]).any():
                near += 1
                continue
            ref = wr.weighted_quantile(v[b], w, ok & has[b], q)
            assert lo[i, b] <= ref < hi[i, b], (b, q, lo[i, b], ref, hi[i, b])
            held += 1
        assert lo[0, b] <= lo[1, b] <= lo[2, b] and hi[0, b] <= hi[1, b] <= hi[2, b]
    empty = np.setdiff1d(np.arange(nbins), with_weight)
    assert empty.size >= 4 and np.isnan(lo[:, empty]).all() and np.isnan(hi[:, empty]).all()
    print(which, "bins with weight", with_weight.size, "| brackets held", held, "| targets within 1e-12 of an entry's end", near)
    assert near <= 0.02 * with_weight.size and held >= 3 * with_weight.size - near
    # (the value bins span the 5 % .. 95 % quantiles of all depths: the coldest and the warmest depth bins have a median outside them)
    assert (np.isfinite(lo[1, with_weight]) & np.isfinite(hi[1, with_weight])).sum() >= with_weight.size // 2


# ------------------------------------------------------------------------------------------------- 5: purity
def test_the_call_writes_nothing(small):
    g, status, lab, w = small["g"], small["status"], small["lab"], small["w"]
    dq = depth_request(small["H"][status == 0], 70)
    before = snapshot(g)
    by_label = g.histogram("N_active", 8, 0.0, 12.0, by_group=True).tobytes()  # what the labels say
    for name, kw in (("T", dict(origin="bottom", **dq)), ("S_bu", dict(axis="layer", origin="top", nbins=80))):
        v0, dv = edges_of_request(small, name, kw, 254)
        for group in (None, 2):
            assert (g.weighted_profile_histogram(name, 254, v0, dv, group=group, **kw)[:, 1:-1] > 0.0).sum() > 100
    assert snapshot(g) == before and g.weights().tobytes() == w.tobytes()
    assert g.histogram("N_active", 8, 0.0, 12.0, by_group=True).tobytes() == by_label
    assert g.get_status()[0].tobytes() == status.tobytes()


# ------------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_in_the_documented_order(small):
    g, lab, w = small["g"], small["lab"], small["w"]
    PAT = -77.0
    call = g._f("get_weighted_profile_histogram")
    out = np.full(9 * 256, PAT)

    def request(**kw):
        rq = g._profile_request(["T"], "depth", "top", 8, 0.0, 0.1)
        for k, v in kw.items():
            setattr(rq, k, v)
        return rq

    def bins(nvbins=16, v0=-8.0, dv=0.5, **kw):
        vb = capi.hist_bins(nvbins, v0, dv)
        for k, v in kw.items():
            setattr(vb, k, v)
        return vb

    def refused(code, rq, vb, group=-1):
        assert call(g._h, None if rq is None else C.byref(rq), None if vb is None else C.byref(vb), group, out.ctypes.data) == code, (code, group)
        assert (out == PAT).all()
    # -- NULLs
    refused(-1, None, bins())
    refused(-1, request(), None)
    assert call(g._h, C.byref(request()), C.byref(bins()), -1, None) == -1
    assert call(None, C.byref(request()), C.byref(bins()), -1, out.ctypes.data) == -1 and (out == PAT).all()
    # -- every check of samsim_get_profile_stats in its order: the size first, then axis, origin, nbins, the arrays, the depth bins
    refused(-6, request(struct_size=8, axis=7, nbins=0), bins(struct_size=4), 99)
    refused(-1, request(axis=2, origin=5), bins(struct_size=4))
    refused(-1, request(origin=2, nbins=0), bins(struct_size=4))
    for nbins in (0, -1, capi.PROFILE_MAX_BINS + 1):
        refused(-1, request(nbins=nbins), bins(struct_size=4))
    refused(-1, request(axis=0, nbins=g.nlayer + 1), bins(struct_size=4))
    for narrays in (0, capi.PROFILE_MAX_ARRAYS + 1):
        refused(-1, request(narrays=narrays), bins(struct_size=4))
    bad = request()
    bad.arrays[0] = capi.NARR
    refused(-1, bad, bins(struct_size=4))
    for z0, dz in ((NAN, 0.1), (0.0, INF), (-0.1, 0.1), (0.0, 0.0), (0.0, -1.0)):
        refused(-1, request(z0=z0, dz=dz), bins(struct_size=4), 99)
    # -- one array per call, before the value bins are looked at
    two = g._profile_request(["T", "S_bu"], "depth", "top", 8, 0.0, 0.1)
    refused(-1, two, bins(struct_size=4))
    # -- the value bins: the size, nvbins, the edges
    refused(-6, request(), bins(struct_size=4, nvbins=0), 99)
    for nvbins in (0, 255, -3):
        refused(-1, request(), bins(nvbins=nvbins), 99)
    for v0, dv in ((NAN, 0.5), (0.0, INF), (-INF, 0.5), (0.0, 0.0), (0.0, -0.5), (1e308, 1e307), (1e16, 0.5)):
        refused(-1, request(), bins(v0=v0, dv=dv), 99)
    # -- the group: below -1, beyond the labels
    for group in (-2, 3, 99):
        refused(-1, request(), bins(), group)
    # -- a good call writes exactly its share
    assert call(g._h, C.byref(request()), C.byref(bins()), 2, out.ctypes.data) == 0
    assert (out[:8 * 18] >= 0.0).all() and (out[:8 * 18] > 0.0).any() and (out[8 * 18:] == PAT).all()
    out[:] = PAT
    # -- without a weight row: refused after the value bins' checks
    try:
        g.clear_weights()
        refused(-1, request(), bins())
        refused(-6, request(), bins(struct_size=4))
        refused(-6, request(struct_size=8), bins())
        with pytest.raises(SamsimError) as e:
            g.weighted_profile_histogram("T", 16, -8.0, 0.5)
        assert e.value.code == -1
        assert g.profile_histogram("T", 16, -8.0, 0.5).sum() > 0                 # the unweighted call does not need the row
    finally:
        g.set_weights(J_SUM, "gauss", small["scale"])
    assert g.weights().tobytes() == w.tobytes()
    # -- without labels a group is refused, -1 is not
    g.set_groups(None)
    try:
        refused(-1, request(), bins(), 0)
        assert (g.weighted_profile_histogram("T", 16, -8.0, 0.5) > 0.0).any()
    finally:
        g.set_groups(lab, ngroups=3)
