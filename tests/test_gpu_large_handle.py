"""One handle of exactly SAMSIM_MAX_NCOL columns (14 128 181 x 80 layers), the largest samsim_create admits.

The limit comes from the [SAMSIM_NSCAL][ncol] scalar block, which the kernel reaches with a scalar base and a 32-bit unsigned byte
offset (GSI / SPEC in samsim_kernels.hip): at this size rows 19-37 of nearly every column lie between 2^31 and 2^32 bytes into the
block, where a sign extension, a wrap or an `int` in the address path would corrupt the upper half of the handle without an error.
The same size reaches the partial last block (ncol = 220 752 * 64 + 53), the second launch of a split step with a large block0, the
2D copies of set_state / get_state with a 113 MB pitch, the device reduction of samsim_get_ensemble_stats over rows that start
beyond 2^31 bytes, and the bounded staging of set_state / get_state.

Footprint on the device: layer block 220 753 * 80 * 8 KiB = 144.7 GB, scalar block 38 * ncol * 8 = 4.29 GB, hand-over block
13 * ncol * 8 = 1.47 GB, the per-column integers 0.45 GB, and the staging buffer, at most SAMSIM_STAGE_MAX_BYTES (256 MiB):
about 151 GB of the MI355X's 288 GB.  On the host every array is a window (at most 2^20 columns); nothing holds the whole handle.

State: the 80-layer day-345 melt-season ensemble (256 members with their T2m / precipitation perturbations: snow cover, thin snow,
bare ice, flushing, freeboard), where most scalar rows are written, tiled over the columns (member = column mod 256).  It is stepped
through one output point and 40 steps beyond (386 steps), so the vital signs and the snapshot are written too.  Over that span the
day-345 members are not chaotic: a one-ulp perturbation of the oracle's initial state moves its layer arrays by at most 5e-10
relative and its compared scalars by less than RTOL, so the oracle holds at RTOL.

References: the project holds that a column's bits depend neither on its handle, its wave-mates nor the launch split (headline,
wave-mates, two-stream and sharding tests), so every copy in the large handle must equal its member in a 256-column handle of the
members BIT FOR BIT, and the members must agree with the oracle at RTOL.  Three blocks of the large handle do not hold the member
handle's wave-mates (the two blocks with a planted STOP code on either side of the launch split, and the partial last block): for
them the step-internal arrays (S_br, ray, perm, flush_v, flush_h, which the kernel stores per wave) are held against a "mirror" handle
that repeats those blocks lane for lane, planted codes included, and the state against the member handle."""
import math
import os
import re
import time

import numpy as np
import pytest

import bench
import samsim_amd
from samsim_amd import testcases as tcs
from samsim_amd.capi import ARRAYS, NPROG, NSCAL, SCALARS, S, State
from tests.helpers import ROOT, assert_state_close
from tests.oracle_lib import oracle_solver

pytestmark = pytest.mark.gpu

NTHREADS = min(16, len(os.sched_getaffinity(0)))
FIXTURE = "sheba_ensemble_80_day345.npz"
CHUNK = 1 << 20          # columns per upload call, and the width of the staging-cap window
EXTRA_STEPS = 40         # steps past the output point
LAUNCH_STEPS = 100       # steps per samsim_step of the large handle (launch granularity does not change a bit)
STATE_ARRAYS = ARRAYS[:10]   # H_abs .. S_bu; S_br, ray, perm, flush_v, flush_h are step-internal (stored per wave)


def header_define(name):
    """value of `#define name <integer expression>` in include/samsim.h"""
    text = open(os.path.join(ROOT, "include", "samsim.h")).read()
    expr = re.search(rf"^#define {name} (.+)$", text, re.M).group(1)
    expr = re.sub(r"\(int64_t\)", "", expr)
    expr = re.sub(r"\b(\d+)ull\b", r"\1", expr).replace("/", "//").replace("SAMSIM_NSCAL", str(NSCAL))
    assert re.fullmatch(r"[\d\s()+\-*/<>]+", expr), expr
    return int(eval(expr, {"__builtins__": {}}))   # noqa: S307  (digits and operators only, checked above)


def device_free_bytes():
    """hipMemGetInfo of the HIP runtime the product library is linked against (its own dependency, resolved through its handle)"""
    import ctypes as C
    lib = samsim_amd.load()
    free, total = C.c_size_t(), C.c_size_t()
    assert lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value, total.value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same_bits(got, want, arrays, what):
    """bitwise: n_active, every scalar, and the listed layer arrays over the active layers (the states are State objects)"""
    assert np.array_equal(got.n_active, want.n_active), f"{what}: N_active differs"
    assert np.array_equal(bits(got.scal), bits(want.scal)), \
        f"{what}: scalars differ in rows {sorted({SCALARS[i] for i in np.nonzero((bits(got.scal) != bits(want.scal)).any(1))[0]})}"
    act = np.arange(got.nlayer)[:, None] < want.n_active[None, :]
    for name in arrays:
        a = ARRAYS.index(name)
        g, w = np.where(act, got.lay[a], 0.0), np.where(act, want.lay[a], 0.0)
        assert np.array_equal(bits(g), bits(w)), f"{what}: array {name} differs in {int((bits(g) != bits(w)).any(0).sum())} columns"


def columns(st, idx):
    return State(np.ascontiguousarray(st.lay[..., idx]), np.ascontiguousarray(st.scal[..., idx]),
                 np.ascontiguousarray(st.n_active[idx]).astype(np.int32))


def small_handle(cfg, st, pert, forcing, clock, members, out_window, plants, nsteps):
    """a HIP handle whose column j is member members[j], with the planted STOP codes at local columns `plants`, stepped nsteps"""
    h = samsim_amd.hip_solver(cfg, len(members))
    h.set_forcing(*forcing, np.ascontiguousarray(pert[0][members]), np.ascontiguousarray(pert[1][members]))
    h.set_state(columns(st, members))
    h.set_clock(**clock)
    h.set_output_window(*out_window)
    for j, (code, step, layer) in plants.items():
        h.set_status([code], [step], [layer], col0=j)
    h.step(nsteps)
    return h


def test_handle_at_max_ncol_against_member_handle_and_oracle():
    t_start = time.time()
    ncol = header_define("SAMSIM_MAX_NCOL")
    cap = header_define("SAMSIM_STAGE_MAX_BYTES")
    assert NSCAL * ncol * 8 < 1 << 32 <= NSCAL * (ncol + 1) * 8   # the largest handle whose scalar block fits 32-bit offsets
    z, st, clock, pert = bench.load_ensemble(FIXTURE)
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    forcing = bench.sheba_forcing()
    nmem, N = st.ncol, int(cfg.nlayer)
    assert nmem == 256 and N == 80
    # geometry: the partial last block, and the launch split at the library's defaults (8 192 blocks, the first part 4/8 of them)
    nblk = (ncol + 63) // 64
    pb0 = (ncol // 64) * 64
    assert 0 < ncol - pb0 < 64 and nblk >= 8192
    split = (nblk * 4 + 7) // 8 * 64
    assert 19 * ncol * 8 + 16 * 8 < 1 << 31 <= 19 * ncol * 8 + 17 * 8   # row 19 crosses 2^31 bytes at column 17
    plants = {ncol - 1: (16, 2980801, 80), pb0 + 22: (1337, 2980803, 1), split - 1: (7889, 2980805, 40), split: (99, 2980807, 2)}
    planted = np.array(sorted(plants))
    # the blocks the mirror handle repeats lane for lane: both sides of the split, the last full block and the partial block
    mirror = np.concatenate([np.arange(split - 64, split + 64), np.arange(pb0 - 64, ncol)])
    odd = np.concatenate([np.arange(split - 64, split + 64), np.arange(pb0, ncol)])   # wave-mates differ from the member handle's
    out0 = pb0 - 64                                       # output window: the last full block and the partial block (117 columns)

    free0, total = device_free_bytes()
    g = samsim_amd.hip_solver(cfg, ncol)
    m = r = None
    try:
        g.set_launch_split(8192, 4)     # the defaults of samsim.h, set here so that `split` is where the second launch starts
        g.set_forcing(*forcing, bench.tile(pert[0], ncol), bench.tile(pert[1], ncol))
        g.ensemble_stats(["N_active"])  # (allocates the reduction's partials: all the handle holds but the staging buffer)
        free_h = device_free_bytes()[0]
        bench.upload_tiled(g, st, ncol, 0, chunk=CHUNK)
        stage_up = free_h - device_free_bytes()[0]
        g.set_clock(**clock)
        g.set_output_window(out0, ncol - out0)
        for c, (code, step, layer) in plants.items():
            g.set_status([code], [step], [layer], col0=c)
        before = {c: g.get_state(c, 1) for c in planted}
        nsteps = g.steps_to_output() + EXTRA_STEPS
        t_up = time.time()
        for s0 in range(0, nsteps, LAUNCH_STEPS):    # launches of ~10 s each rather than one of half a minute
            g.step(min(LAUNCH_STEPS, nsteps - s0))
        g.synchronize()
        t_step = time.time()
        peak = total - device_free_bytes()[0]

        m = small_handle(cfg, st, pert, forcing, clock, np.arange(nmem), (0, nmem), {}, nsteps)
        loc = {int(np.searchsorted(mirror, c)): v for c, v in plants.items()}
        r = small_handle(cfg, st, pert, forcing, clock, mirror % nmem, (int(np.searchsorted(mirror, out0)), ncol - out0), loc, nsteps)
        ms, rs = m.get_state(), r.get_state()
        assert not m.get_status()[0].any()
        # the mirror's columns hold their members' state: wave-mates do not change a column's bits
        keep_r = ~np.isin(mirror, planted)
        assert_same_bits(columns(rs, np.nonzero(keep_r)[0]), columns(ms, mirror[keep_r] % nmem), STATE_ARRAYS, "mirror vs members")

        # 1. status: the planted codes, steps and layers, zero everywhere else; the planted columns untouched
        status, err_step, err_layer = g.get_status()
        for arr, k in ((status, 0), (err_step, 1), (err_layer, 2)):
            nz = np.flatnonzero(arr)
            assert np.array_equal(nz, planted), f"status field {k}: non-zero at {nz[:8]}"
            assert [int(arr[c]) for c in planted] == [plants[c][k] for c in planted]
        del status, err_step, err_layer
        for c in planted:
            after = g.get_state(int(c), 1)
            assert np.array_equal(bits(after.lay), bits(before[c].lay)) and np.array_equal(bits(after.scal), bits(before[c].scal)), c
            assert np.array_equal(after.n_active, before[c].n_active), c

        # 2. whole handle, reduced on the device: count, min, max exact; mean against the copy-weighted mean of the members.
        # The device sums in a fixed tree: ~108 terms per thread (512 x 256 threads stride over the row), a 256-wide block tree and
        # 512 partials on the host, so its rounding error is at most about (108 + 8 + 9) * 2^-53 * sum|v| = 1.4e-14 * sum|v|.  The
        # bound 1e-12 is taken relative to the mean of |v| (a quantity of either sign can have a mean near zero): a factor 70 of margin.
        names = list(SCALARS) + ["N_active"]
        stats = g.ensemble_stats(names)
        copies = np.bincount(np.arange(ncol) % nmem, minlength=nmem) - np.bincount(planted % nmem, minlength=nmem)
        n = ncol - len(planted)
        assert copies.sum() == n and copies.min() > 0
        for name in names:
            v = ms.n_active.astype(np.float64) if name == "N_active" else ms.scal[S[name]]
            s = stats[name]
            assert s.count == n, name
            assert s.min == v.min() and s.max == v.max(), (name, s.min, v.min(), s.max, v.max())
            mean = math.fsum(copies * v) / n
            scale = math.fsum(copies * np.abs(v)) / n
            assert abs(s.mean - mean) <= 1e-12 * scale, (name, s.mean, mean)

        # 3. sampled windows, bitwise: block 0 (row 19 of column 17 is past 2^31 bytes), both sides of the split, the last full and
        # the partial block, and 64 windows from a seeded generator; every column against its member (all arrays where the
        # wave-mates are the member handle's, the state in the three blocks where they are not) and the mirror's columns against
        # the mirror (all arrays).  The planted columns were compared in 1.
        rng = np.random.default_rng(2026)
        starts = [0, split - 64, split, pb0 - 64, pb0] + [int(x) for x in rng.integers(0, ncol - 64, 64)]
        wins = [g.get_state(c0, min(64, ncol - c0)) for c0 in starts]
        cols = np.concatenate([np.arange(c0, c0 + w.ncol) for c0, w in zip(starts, wins)])
        got = State(np.concatenate([w.lay for w in wins], axis=2), np.concatenate([w.scal for w in wins], axis=1),
                    np.concatenate([w.n_active for w in wins]))
        live = ~np.isin(cols, planted)
        plain = live & ~np.isin(cols, odd)
        assert plain.sum() >= 64 * 64
        assert_same_bits(columns(got, np.nonzero(plain)[0]), columns(ms, cols[plain] % nmem), ARRAYS, "windows vs members")
        sel = live & np.isin(cols, odd)
        assert_same_bits(columns(got, np.nonzero(sel)[0]), columns(ms, cols[sel] % nmem), STATE_ARRAYS, "odd blocks vs members")
        sel = live & np.isin(cols, mirror)
        assert len(np.unique(cols[sel])) == len(mirror) - len(planted)
        assert_same_bits(columns(got, np.nonzero(sel)[0]), columns(rs, np.searchsorted(mirror, cols[sel])), ARRAYS, "windows vs mirror")

        # 4. the snapshot of the last 117 columns: the mirror's, bit for bit; the members' for the columns that ran
        og, orr, om = g.get_output(), r.get_output(), m.get_output()
        assert (og.time, og.step) == (orr.time, orr.step) == (om.time, om.step)
        assert np.array_equal(bits(og.lay), bits(orr.lay)) and np.array_equal(bits(og.scal), bits(orr.scal))
        assert np.array_equal(og.n_active, orr.n_active)
        oc = np.arange(out0, ncol)
        run = ~np.isin(oc, planted)
        for sel, arrays in ((run & ~np.isin(oc, odd), ARRAYS), (run & np.isin(oc, odd), STATE_ARRAYS)):
            idx = np.nonzero(sel)[0]
            assert_same_bits(columns(og, idx), columns(om, oc[idx] % nmem), arrays, "snapshot vs members")

        # 5. parity: the members against the oracle at RTOL
        o = oracle_solver(cfg, nmem)
        o.set_threads(NTHREADS)
        o.set_forcing(*forcing, pert[0], pert[1])
        o.set_state(columns(st, np.arange(nmem)))
        o.set_clock(**clock)
        o.step(nsteps)
        assert not o.get_status()[0].any()
        assert_state_close(ms, o.get_state(), what=f"{FIXTURE}, {nsteps} steps, members 0..255")

        # 6. staging cap (last: set_state clears the status of the columns it writes).  A 2^20-column window across the split
        # comes back as the members' stepped state, is written back and read again unchanged, and the device's free memory ends
        # within SAMSIM_STAGE_MAX_BYTES of where it was before these calls.  The upload of 2^20-column windows of 4 arrays (2.7 GB
        # each) left no more than the cap allocated either; the 64 MiB beyond the cap there are room for the runtime's own small
        # allocations, not for staging.  (Not measured across the steps: the runtime allocates the kernel's scratch memory then.)
        assert stage_up <= cap + (64 << 20), f"the upload left {stage_up / 2**20:.0f} MiB allocated"
        c0 = split - CHUNK // 2
        free_a = device_free_bytes()[0]
        s1 = g.get_state(c0, CHUNK, narr=NPROG)
        want = State(bench.tile(ms.lay[:NPROG], CHUNK, c0), bench.tile(ms.scal, CHUNK, c0), bench.tile(ms.n_active, CHUNK, c0))
        inside = planted[(planted >= c0) & (planted < c0 + CHUNK)] - c0
        assert len(inside) == 2
        for j in inside:     # the planted columns (compared in 1.) as read
            want.lay[..., j], want.scal[:, j], want.n_active[j] = s1.lay[..., j], s1.scal[:, j], s1.n_active[j]
        assert_same_bits(s1, want, ARRAYS[:NPROG], "2^20-column window vs members")
        del want
        g.set_state(s1, c0)
        s2 = g.get_state(c0, CHUNK, narr=NPROG)
        assert np.array_equal(bits(s2.lay), bits(s1.lay)) and np.array_equal(bits(s2.scal), bits(s1.scal))
        assert np.array_equal(s2.n_active, s1.n_active)
        free_b = device_free_bytes()[0]
        assert free_a - free_b <= cap, f"staging grew by {(free_a - free_b) / 2**20:.0f} MiB > {cap / 2**20:.0f} MiB"
        status = g.get_status()[0]
        assert not status[c0:c0 + CHUNK].any()
        assert np.array_equal(np.flatnonzero(status), planted[(planted < c0) | (planted >= c0 + CHUNK)])
        print(f"\nlarge handle: {ncol} columns x {N} layers, {nsteps} steps; device memory in use at the peak {peak / 1e9:.1f} GB "
              f"(free before {free0 / 1e9:.1f} of {total / 1e9:.1f} GB); set-up {t_up - t_start:.1f} s, steps {t_step - t_up:.1f} s, "
              f"checks {time.time() - t_step:.1f} s")
    finally:
        for h in (g, m, r):
            if h is not None:
                h.close()
