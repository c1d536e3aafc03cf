"""samsim_get_histogram / samsim_get_profile_histogram on the GPU: fixed-edge histograms of the column scalars and joint histograms
of the layer profiles, reduced on the device.  The counts are integers: everything is checked by equality against the numpy
restatement of the header (tests/hist_reference.py) applied to get_state() of the same handle."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import bench
import samsim_amd
from samsim_amd import testcases as tcs
from samsim_amd.capi import A, ProfileRequest, State, hist_bins, quantile_bracket
from tests import hist_reference as hr
from tests.helpers import ROOT
from tests.profile_reference import column_thickness
from tests.test_gpu_profile_stats import ensemble, pick_dz

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "host", "samsim_host.x")
SCALARS = ("thick_snow", "T_top", "m_snow", "N_active")


def lds_threshold():
    text = open(os.path.join(ROOT, "samsim_amd", "csrc", "samsim_hist.h")).read()
    return int(re.search(r"^#define DEV_HIST_LDS_COUNTS\s+(\d+)", text, re.M).group(1))


def quantile_edges(v, nvbins):
    """(v0, dv, spread): edges from the 10 % to the 90 % quantile of the values.  A slot whose two quantiles coincide (every
    column of the melting ensemble has T_top = 0 and N_active = nlayer) has no such edges -- dv would be 0, which the library
    refuses --; it gets edges of width 2 centred on the value, which then lies exactly on an edge or next to one."""
    q10, q90 = np.quantile(v, [0.1, 0.9])
    if q90 > q10:
        return float(q10), float((q90 - q10) / nvbins), True
    return float(q10) - 1.0, 2.0 / nvbins, False


def scalar_values(s, name):
    return s.n_active.astype(np.float64) if name == "N_active" else s.sc(name)


@functools.lru_cache(maxsize=None)
def melting():
    """the ensemble of the two scalar tests, its state and its status: computed once, left unchanged"""
    g = ensemble("sheba_ensemble_80_day345.npz", 70001, 200, corrupt=(5, 40000, 70000))
    status = g.get_status()[0]
    assert (status != 0).sum() == 3
    return g, g.get_state(), status


def test_scalars_ungrouped():
    """70 001 columns: more blocks than the grid, a ragged last block, three stopped columns.  Where a slot is spread over the
    ensemble (asserted for thick_snow and m_snow) both outer entries and at least min(3, nvbins) inner ones must be occupied --
    one value bin has one inner entry --, else the comparison proves nothing."""
    g, s, status = melting()
    ok = status == 0
    stats = g.ensemble_stats(SCALARS)
    for name in SCALARS:
        v = scalar_values(s, name)
        for nvbins in (1, 30, 254):
            v0, dv, spread = quantile_edges(v[ok], nvbins)
            want = hr.scalar_histogram_reference(v, status, nvbins, v0, dv)
            inner = int((want[1:-1] > 0).sum())
            print(name, nvbins, "v0", v0, "dv", dv, "spread", spread, "outer", int(want[0]), int(want[-1]), "inner occupied", inner)
            if name in ("thick_snow", "m_snow"):
                assert spread and want[0] > 0 and want[-1] > 0 and inner >= min(3, nvbins), (name, nvbins)
            got = g.histogram(name, nvbins, v0, dv)
            assert got.dtype == np.int64 and got.shape == (nvbins + 2,)
            assert np.array_equal(got, want), (name, nvbins)
            assert got.sum() == stats[name].count == ok.sum(), (name, nvbins)
            occ = np.nonzero(got)[0]
            assert hr.entries([stats[name].min], nvbins, v0, dv)[0] == occ[0], (name, nvbins)
            assert hr.entries([stats[name].max], nvbins, v0, dv)[0] == occ[-1], (name, nvbins)
    # the median of the snow mass from the counts: the bracket holds the exact order statistic
    v = s.sc("m_snow")
    v0, dv, _ = quantile_edges(v[ok], 254)
    lo, hi = quantile_bracket(g.histogram("m_snow", 254, v0, dv), v0, dv, 0.5)
    assert lo <= np.sort(v[ok])[max(1, int(np.ceil(0.5 * ok.sum()))) - 1] < hi and hi - lo < 1.001 * dv


def test_scalars_per_group():
    g, s, status = melting()
    ok = status == 0
    c = np.arange(g.ncol)
    thr = lds_threshold()
    lab9 = (c % 9).astype(np.int32)
    lab9[::11] = -1
    lab1024 = (c % 1024).astype(np.int32)
    assert 9 * (30 + 2) <= thr < 1024 * (254 + 2)          # the two cases take the two paths of samsim_hist.h
    try:
        for lab, ng, nvbins in ((lab9, 9, 30), (lab1024, 1024, 254)):
            g.set_groups(lab, ngroups=ng)
            gstats = g.group_stats(SCALARS)
            for name in SCALARS:
                v = scalar_values(s, name)
                v0, dv, _ = quantile_edges(v[ok], nvbins)
                want = hr.scalar_histogram_reference(v, status, nvbins, v0, dv, lab, ng)
                got = g.histogram(name, nvbins, v0, dv, by_group=True)
                assert got.shape == (ng, nvbins + 2) and np.array_equal(got, want), (name, ng)
                assert np.array_equal(got.sum(1), gstats[name]["count"]), (name, ng)
        # relabelling the columns outside group 3 leaves group 3's row alone
        g.set_groups(lab9, ngroups=9)
        v0, dv, _ = quantile_edges(s.sc("m_snow")[ok], 30)
        before = g.histogram("m_snow", 30, v0, dv, by_group=True)
        lab2 = (lab9 + 5) % 9
        lab2[lab2 == 3] = 4
        lab2[c % 7 == 0] = -1
        lab2 = np.where(lab9 == 3, 3, lab2).astype(np.int32)
        assert np.array_equal(lab2 == 3, lab9 == 3) and (lab2 != lab9).sum() > g.ncol // 2
        g.set_groups(lab2, ngroups=9)
        after = g.histogram("m_snow", 30, v0, dv, by_group=True)
        assert before[3].sum() > 0 and before[3].tobytes() == after[3].tobytes() and not np.array_equal(before, after)
        # one group of every column is the ungrouped histogram
        g.set_groups(np.zeros(g.ncol, dtype=np.int32), ngroups=1)
        for name in SCALARS:
            v0, dv, _ = quantile_edges(scalar_values(s, name)[ok], 30)
            one = g.histogram(name, 30, v0, dv, by_group=True)
            assert one.shape == (1, 32) and one[0].tobytes() == g.histogram(name, 30, v0, dv).tobytes(), name
    finally:
        g.set_groups(None)


def test_profiles_by_layer_both_origins():
    ncol, nvbins = 70001, 40
    g = ensemble("sheba_ensemble_80_day75.npz", ncol, 300, corrupt=(5, 40000, 70000))
    status = g.get_status()[0]
    assert (status != 0).sum() == 3
    s = g.get_state()
    na_max = int(s.n_active[status == 0].max())
    assert na_max < g.nlayer
    for origin in ("top", "bottom"):
        for name in ("T", "S_bu", "psi_l"):
            v, has = hr.profile_values(s, status, name, axis="layer", origin=origin)
            v0, dv, spread = quantile_edges(v[has], nvbins)
            assert spread, name
            want = hr.joint_histogram(v, has, nvbins, v0, dv)
            got = g.profile_histogram(name, nvbins, v0, dv, axis="layer", origin=origin)
            assert got.shape == (g.nlayer, nvbins + 2) and got.dtype == np.int64
            print("layer", origin, name, "entries occupied", int((want > 0).sum()), "outer", int(want[:, 0].sum()), int(want[:, -1].sum()))
            assert want[:, 0].sum() > 0 and want[:, -1].sum() > 0 and (want[:, 1:-1].sum(0) > 0).sum() >= 3
            assert np.array_equal(got, want), (origin, name)
            assert np.array_equal(got.sum(1), g.profile_stats([name], axis="layer", origin=origin)[name]["count"]), (origin, name)
            assert (got[na_max:] == 0).all() and got[na_max - 1].sum() > 0


def full_members(fixture):
    """the members of a stage fixture as a State of every array.  The fixture holds the prognostic arrays only, and no step is
    taken, so the T row carries a stand-in computed here: the specific enthalpy H_abs / m over c_s = 2112 J/(kg K), a
    temperature-like number that varies over layers and members.  The histogram reads the row as stored."""
    z, st, clock, pert = bench.load_ensemble(fixture)
    m = State.empty(st.ncol, st.nlayer)
    m.lay[:4] = st.lay
    m.scal[:] = st.scal
    m.n_active[:] = st.n_active
    mass = m.arr("m")
    m.arr("T")[:] = np.where(mass != 0.0, m.arr("H_abs") / np.where(mass != 0.0, mass, 1.0), 0.0) / 2112.0
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    return cfg, m


def upload(cfg, members, ncol, chunk=32768):
    g = samsim_amd.hip_solver(cfg, ncol)
    for c0 in range(0, ncol, chunk):
        n = min(chunk, ncol - c0)
        g.set_state(State(bench.tile(members.lay, n, c0), bench.tile(members.scal, n, c0), bench.tile(members.n_active, n, c0).astype(np.int32)), c0)
    return g


def pick_dv(values, nvbins, lo, hi):
    """(v0, dv): the first of a short list of bin widths for which no reference value lies within 1e-9 max(1, |v|) of a value
    edge: which entry a value falls into is then beyond the rounding of W / L (a condition on the data, not a tolerance)"""
    base = (hi - lo) / nvbins
    for f in (1.0, 1.01, 0.99, 1.03, 0.97, 1.05):
        dv = base * f
        v0 = lo - dv / 3.0
        E = hr.edges(nvbins, v0, dv)
        if (np.abs(values[:, None] - E[None, :]) > 1e-9 * np.maximum(1.0, np.abs(values))[:, None]).all():
            return v0, dv
    return None


def test_profiles_by_depth():
    """the melting ensemble as loaded, no steps: the state is the upload, so the reference is formed for the 256 members and
    tiled.  70 001 columns with 32 depth bins; 5 003 columns with 100 depth bins (two passes); 254 value bins (the smaller depth
    chunk, three passes)."""
    cfg, members = full_members("sheba_ensemble_80_day345.npz")
    mstatus = np.zeros(members.ncol, dtype=np.int32)
    H = column_thickness(members)
    chunk_of = lambda nv: min(64, (65536 - 512) // (520 + 4 * ((nv + 2) | 1)))      # noqa: E731  (the rule of samsim.h)
    assert chunk_of(40) == 64 and chunk_of(254) < 64
    for ncol, nbins, nvbins, cand in ((70001, 32, 40, (0.07, 0.05, 0.09, 0.11)), (5003, 100, 40, (0.02, 0.021, 0.019, 0.022)),
                                      (5003, 100, 254, (0.02, 0.021, 0.019, 0.022))):
        g = upload(cfg, members, ncol)
        idx = np.arange(ncol) % members.ncol
        s = g.get_state()
        assert np.array_equal(s.lay[:5], members.lay[:5][:, :, idx]) and np.array_equal(s.n_active, members.n_active[idx])
        assert not g.get_status()[0].any()
        dz = pick_dz(H, cand, nbins, (0.0, 0.035))
        assert dz is not None
        lab = (np.arange(ncol) % 9).astype(np.int32)
        for origin, z0 in (("top", 0.0), ("bottom", 0.0), ("top", 0.035), ("bottom", 0.035)):
            for name in ("T", "S_bu"):
                v, has = hr.profile_values(members, mstatus, name, axis="depth", origin=origin, nbins=nbins, z0=z0, dz=dz)
                q10, q90 = np.quantile(v[has], [0.1, 0.9])
                picked = pick_dv(v[has], nvbins, q10, q90)
                assert picked is not None, (name, origin, z0)
                v0, dv = picked
                vt, ht = v[:, idx], has[:, idx]
                want = hr.joint_histogram(vt, ht, nvbins, v0, dv)
                assert want[:, 0].sum() > 0 and want[:, -1].sum() > 0 and (want[:, 1:-1].sum(0) > 0).sum() >= 3
                assert (want.sum(1) == 0).any() and (want.sum(1) == ncol).any()                       # bins in the water, bins every column fills
                if nbins > chunk_of(nvbins):
                    c = chunk_of(nvbins)
                    assert want[:c].sum() > 0 and want[c:].sum() > 0                                # more than one pass holds ice
                got = g.profile_histogram(name, nvbins, v0, dv, axis="depth", origin=origin, nbins=nbins, z0=z0, dz=dz)
                assert np.array_equal(got, want), (ncol, nbins, nvbins, origin, z0, name)
                cnt = g.profile_stats([name], axis="depth", origin=origin, nbins=nbins, z0=z0, dz=dz)[name]["count"]
                assert np.array_equal(got.sum(1), cnt)
                if name == "T" and z0 == 0.0:                                                        # the nine groups add up to the whole
                    g.set_groups(lab, ngroups=9)
                    parts = [g.profile_histogram(name, nvbins, v0, dv, axis="depth", origin=origin, nbins=nbins, z0=z0, dz=dz, group=k)
                             for k in range(9)]
                    assert np.array_equal(parts[4], hr.joint_histogram(vt, ht, nvbins, v0, dv, select=lab == 4))
                    assert np.array_equal(sum(parts), got) and all(p.sum() > 0 for p in parts)
                    g.set_groups(None)
        g.close()


def test_identical_columns():
    ncol = 256
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    g.set_clock()
    g.step(2000)
    assert not g.get_status()[0].any()
    for kw in (dict(axis="layer", origin="top"), dict(axis="layer", origin="bottom"),
               dict(axis="depth", origin="top", nbins=40, dz=0.0015), dict(axis="depth", origin="bottom", nbins=40, z0=0.001, dz=0.0015)):
        for name, v0, dv in (("T", -20.0, 0.25), ("S_bu", 0.0, 0.5), ("psi_l", 0.0, 0.01)):
            q = g.profile_histogram(name, 100, v0, dv, **kw)
            cnt = g.profile_stats([name], **kw)[name]["count"]
            occ = cnt > 0
            assert occ.any() and (cnt[occ] == ncol).all()
            assert ((q > 0).sum(1) == occ).all() and np.array_equal(q.max(1), cnt), (kw, name)
    one = g.histogram("thickness", 50, 0.0, 0.01)
    assert (one > 0).sum() == 1 and one.max() == ncol


def test_deterministic_and_leaves_the_run_alone():
    ncol = 1000

    def fresh():
        g = ensemble("sheba_ensemble_80_day75.npz", ncol, 0)
        g.set_launch_split(min_blocks=2)
        return g
    a, b = fresh(), fresh()
    a.step(500)
    s0, c0, st0 = a.get_state(), a.get_clock(), a.get_status()
    a.set_groups((np.arange(ncol) % 5).astype(np.int32))

    def calls():
        return [a.histogram("thickness", 30, 0.1, 0.005), a.histogram("T_top", 254, -3.0, 0.01, by_group=True),
                a.profile_histogram("T", 64, -3.0, 0.05, axis="layer", origin="bottom"),
                a.profile_histogram("S_bu", 254, 0.0, 0.1, axis="depth", origin="top", nbins=64, dz=0.005),
                a.profile_histogram("psi_l", 20, 0.0, 0.05, axis="depth", origin="bottom", nbins=30, dz=0.01, group=2)]
    q1, q2 = calls(), calls()
    for x, y in zip(q1, q2):
        assert x.tobytes() == y.tobytes() and x.sum() > 0
    assert q1[0].sum() == ncol and (q1[0] > 0).sum() > 3
    s1, c1, st1 = a.get_state(), a.get_clock(), a.get_status()
    assert np.array_equal(s0.lay, s1.lay) and np.array_equal(s0.scal, s1.scal) and np.array_equal(s0.n_active, s1.n_active)
    assert bytes(c0) == bytes(c1) and all(np.array_equal(x, y) for x, y in zip(st0, st1))
    a.step(500)
    b.step(1000)
    sa, sb = a.get_state(), b.get_state()
    assert np.array_equal(sa.n_active, sb.n_active)
    assert np.array_equal(sa.lay[:4], sb.lay[:4]) and np.array_equal(sa.scal, sb.scal)


def test_ensemble_beyond_32_bit_offsets():
    """419 840 columns of 80 layers: the layer block is just over 4 GiB.  Not stepped, members repeating with period 256: every
    count is the 256-member count times 1 640."""
    ncol, nbins, nvbins = 419840, 64, 40
    cfg, members = full_members("sheba_ensemble_80.npz")
    assert members.ncol == 256 and ncol % 256 == 0 and ncol // 64 * 80 * 16 * 64 * 8 > 1 << 32
    g = upload(cfg, members, ncol)
    mstatus = np.zeros(members.ncol, dtype=np.int32)
    dz = pick_dz(column_thickness(members), (0.03, 0.029, 0.031, 0.033), nbins, (0.0,))
    assert dz is not None
    for kw in (dict(axis="layer", origin="top"), dict(axis="layer", origin="bottom"),
               dict(axis="depth", origin="top", nbins=nbins, dz=dz), dict(axis="depth", origin="bottom", nbins=nbins, dz=dz)):
        v, has = hr.profile_values(members, mstatus, "T", **kw)
        q10, q90 = np.quantile(v[has], [0.1, 0.9])
        v0, dv = pick_dv(v[has], nvbins, q10, q90)
        want = hr.joint_histogram(v, has, nvbins, v0, dv) * (ncol // 256)
        assert want.sum() > 0 and (want[:, 1:-1].sum(0) > 0).sum() >= 3
        assert np.array_equal(g.profile_histogram("T", nvbins, v0, dv, **kw), want), kw


def test_argument_errors():
    ncol = 64
    cfg, st = tcs.testcase1(ncol)
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_state(st)
    size = C.sizeof(hist_bins(1, 0.0, 1.0))

    def bins(**kw):
        vb = hist_bins(8, 0.0, 0.5)
        for k, v in kw.items():
            setattr(vb, k, v)
        return vb

    def request(**kw):
        rq = ProfileRequest()
        rq.struct_size, rq.axis, rq.origin, rq.nbins, rq.narrays = C.sizeof(ProfileRequest), 1, 0, 8, 1
        rq.arrays[0] = A["T"]
        rq.z0, rq.dz = 0.0, 0.01
        for k, v in kw.items():
            if k == "array0":
                rq.arrays[0] = v
            else:
                setattr(rq, k, v)
        return rq

    def refused(code, f, *args):
        with pytest.raises(samsim_amd.SamsimError) as e:
            f(*args)
        assert e.value.code == code, args

    good = g.histogram_raw(0, bins())
    good_p = g.profile_histogram_raw(request(), bins())
    assert good.shape == (10,) and good.sum() == ncol and good_p.shape == (8, 10)
    bad_bins = [(dict(struct_size=size - 8), -6), (dict(nvbins=0), -1), (dict(nvbins=255), -1), (dict(v0=float("nan")), -1),
                (dict(v0=float("inf")), -1), (dict(dv=float("inf")), -1), (dict(dv=float("nan")), -1), (dict(dv=0.0), -1),
                (dict(dv=-0.5), -1), (dict(v0=1.0e300, dv=1.0e307, nvbins=254), -1),     # the last edges overflow
                (dict(v0=1.0, dv=1.0e-17), -1)]                                            # v0 + j dv == v0: not increasing
    for kw, code in bad_bins:
        refused(code, g.histogram_raw, 0, bins(**kw))
        refused(code, g.profile_histogram_raw, request(), bins(**kw))
    refused(-1, g.histogram_raw, 38, bins())
    refused(-1, g.histogram_raw, -2, bins())
    refused(-1, g.histogram_raw, 0, bins(), 2)
    refused(-1, g.histogram_raw, 0, bins(), -1)
    refused(-1, g.histogram_raw, 0, bins(), 1)                    # by_group without labels
    f, h = g._f("get_histogram"), g._h
    out = np.zeros(16, dtype=np.int64)
    assert f(h, 0, None, 0, out.ctypes.data) == -1 and f(h, 0, C.byref(bins()), 0, None) == -1 and f(None, 0, C.byref(bins()), 0, out.ctypes.data) == -1
    fp = g._f("get_profile_histogram")
    outp = np.zeros(8 * 16, dtype=np.int64)
    assert fp(h, None, C.byref(bins()), -1, outp.ctypes.data) == -1 and fp(h, C.byref(request()), None, -1, outp.ctypes.data) == -1
    assert fp(h, C.byref(request()), C.byref(bins()), -1, None) == -1 and fp(None, C.byref(request()), C.byref(bins()), -1, outp.ctypes.data) == -1
    # the profile call: the checks of the request first and in their order, then narrays, then the value bins, then the group
    for kw, code in [(dict(struct_size=C.sizeof(ProfileRequest) - 8), -6), (dict(nbins=0), -1), (dict(nbins=1025), -1), (dict(narrays=9), -1),
                     (dict(array0=15), -1), (dict(array0=-1), -1), (dict(dz=0.0), -1), (dict(dz=float("nan")), -1), (dict(z0=-0.01), -1),
                     (dict(z0=float("inf")), -1), (dict(axis=2), -1), (dict(origin=2), -1), (dict(axis=0, nbins=cfg.nlayer + 1), -1),
                     (dict(narrays=2), -1), (dict(narrays=0), -1)]:
        refused(code, g.profile_histogram_raw, request(**kw), bins())
    refused(-1, g.profile_histogram_raw, request(axis=2), bins(struct_size=size - 8))           # the request is looked at first
    refused(-6, g.profile_histogram_raw, request(struct_size=4), bins(nvbins=0))
    refused(-1, g.profile_histogram_raw, request(narrays=2), bins(struct_size=size - 8))        # narrays before the value bins
    refused(-6, g.profile_histogram_raw, request(), bins(struct_size=size - 8), -2)             # the value bins before the group
    refused(-1, g.profile_histogram_raw, request(), bins(), -2)
    refused(-1, g.profile_histogram_raw, request(), bins(), 0)                                  # a group without labels
    g.set_groups((np.arange(ncol) % 3).astype(np.int32))
    refused(-1, g.profile_histogram_raw, request(), bins(), 3)
    assert g.profile_histogram_raw(request(), bins(), 2).sum() < good_p.sum()
    assert g.histogram_raw(0, bins(), 1).shape == (3, 10)
    g.set_groups(None)
    # refused calls left nothing behind
    assert g.histogram_raw(0, bins()).tobytes() == good.tobytes() and g.profile_histogram_raw(request(), bins()).tobytes() == good_p.tobytes()
    assert g.profile_histogram_raw(request(axis=0, nbins=cfg.nlayer, dz=0.0), bins()).shape == (cfg.nlayer, 10)


@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran host not built (no flang)")
def test_fortran_host_histogram_file(tmp_path):
    """hist_bins / hist_max in &samsim_run: one row per output point in dat_ens_hist_thickness.dat; 100 identical columns fill
    one entry, the one whose bracket holds the mean thickness of dat_ensemble.dat; without the keys no such file appears and the
    other files do not change"""
    def run(d, nml):
        d.mkdir()
        (d / "output").mkdir()
        (d / "samsim.nml").write_text(nml)
        r = subprocess.run([HOST], cwd=d, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    ncol, nv, vmax, total = 100, 20, 1.0, 7300
    run(tmp_path / "hist", f"&samsim_run testcase=1, ncol={ncol}, max_steps={total}, hist_bins={nv}, hist_max={vmax} /\n")
    run(tmp_path / "plain", f"&samsim_run testcase=1, ncol={ncol}, max_steps={total} /\n")
    with_hist, plain = sorted(os.listdir(tmp_path / "hist" / "output")), sorted(os.listdir(tmp_path / "plain" / "output"))
    assert [f for f in with_hist if "hist" in f] == ["dat_ens_hist_thickness.dat"] and not [f for f in plain if "hist" in f]
    assert [f for f in with_hist if "hist" not in f] == plain and len(plain) > 5
    for f in plain:
        assert (tmp_path / "hist" / "output" / f).read_bytes() == (tmp_path / "plain" / "output" / f).read_bytes(), f
    ens = np.loadtxt(tmp_path / "hist" / "output" / "dat_ensemble.dat")
    rows = np.loadtxt(tmp_path / "hist" / "output" / "dat_ens_hist_thickness.dat")
    assert rows.shape == (3, 1 + nv + 2) and ens.shape[0] == 3                       # outputs at steps 1, 3602, 7203
    assert np.array_equal(rows[:, 0], ens[:, 0])
    for row, e in zip(rows, ens):
        counts = row[1:].astype(np.int64)
        assert (counts > 0).sum() == 1 and counts.max() == int(e[1]) == ncol
        lo, hi = quantile_bracket(counts, 0.0, vmax / nv, 0.5)
        assert lo <= e[2] < hi, (lo, e[2], hi)
    # the host refuses more value bins than the library takes, and a range that is not positive, where it reads the namelist
    for bad in ("hist_bins=255, hist_max=1.0", "hist_bins=20, hist_max=0.0", "hist_bins=20"):
        (tmp_path / "plain" / "samsim.nml").write_text(f"&samsim_run testcase=1, ncol={ncol}, max_steps=1, {bad} /\n")
        r = subprocess.run([HOST], cwd=tmp_path / "plain", capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "hist_bins" in r.stdout + r.stderr and "on HIP device" not in r.stdout, bad
