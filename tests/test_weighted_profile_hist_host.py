"""The weighted joint histogram of the layer profiles (samsim_get_weighted_profile_histogram) without a device: the symbol, the
refusals that need no handle, the chunk rule of samsim_pass_plan.h against its Python mirror and the bounds it has to keep, and
capi.weighted_profile_quantiles against the reference's weighted quantile."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi
from tests import weights_reference as wr
from tests.helpers import ROOT


def test_the_library_exports_the_symbol():
    lib = samsim_amd.load()
    assert hasattr(lib, "samsim_get_weighted_profile_histogram")


def test_null_pointers_are_refused_before_any_device_call():
    """without a handle there is nothing to launch on: every combination with h NULL comes back as SAMSIM_ERR_ARG (-1), with or
    without a GPU, and the buffer keeps its pattern"""
    lib = samsim_amd.load()
    f = lib.samsim_get_weighted_profile_histogram
    f.argtypes = [C.c_void_p, C.POINTER(capi.ProfileRequest), C.POINTER(capi.HistBins), C.c_int32, C.c_void_p]
    f.restype = C.c_int
    rq = capi.ProfileRequest()
    rq.struct_size, rq.nbins, rq.narrays = C.sizeof(capi.ProfileRequest), 4, 1
    rq.arrays[0] = capi.A["T"]
    vb = capi.hist_bins(8, -2.0, 0.25)
    buf = np.full(4 * 10, -77.0)
    assert f(None, C.byref(rq), C.byref(vb), -1, buf.ctypes.data) == -1
    assert f(None, None, C.byref(vb), -1, buf.ctypes.data) == -1
    assert f(None, C.byref(rq), None, -1, buf.ctypes.data) == -1
    assert f(None, C.byref(rq), C.byref(vb), -1, None) == -1
    assert f(None, None, None, 5, None) == -1
    assert (buf == -77.0).all()


CHUNK_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "samsim_pass_plan.h"

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s (nvbins %d, nbins %d, origin %d)\n", __LINE__, #c, g_nv, g_nbins, g_origin); std::exit(1); } } while (0)
static int g_nv, g_nbins, g_origin;

int main() {
  std::printf("grid %d lds %d scratch %llu max_bins %d max_vbins %d\n", (int)DEV_WPHIST_GRID, (int)DEV_WPHIST_LDS_BYTES,
              (unsigned long long)SAMSIM_WPHIST_SCRATCH_BYTES, (int)SAMSIM_PROFILE_MAX_BINS, (int)SAMSIM_HIST_MAX_VBINS);
  for (g_nv = 1; g_nv <= SAMSIM_HIST_MAX_VBINS; ++g_nv) {
    const int chunk = dev_wphist_chunk(g_nv);
    std::printf("%d %d %lld %lld\n", g_nv, chunk, dev_wphist_lds(g_nv), dev_wphist_wave_doubles(g_nv));
    const int NBINS[5] = {1, chunk - 1, chunk, chunk + 1, 1024};
    const int origins[2] = {SAMSIM_PROFILE_FROM_TOP, SAMSIM_PROFILE_FROM_BOTTOM};
    for (int in = 0; in < 5; ++in)
      for (int io = 0; io < 2; ++io) {
        g_nbins = NBINS[in]; g_origin = origins[io];
        if (g_nbins < 1) continue;   // chunk - 1 of a chunk of one bin
        int next = 0, passes = 0;
        const int rc = pass_plan(1, g_nbins, chunk, g_origin, [&](const PassSpan &s) {
          CHECK(s.array == 0 && s.b0 == next && s.nb >= 1 && s.nb <= chunk && s.b0 + s.nb <= g_nbins);
          const bool first = s.b0 == 0, last = s.b0 + s.nb == g_nbins;
          CHECK(s.lead == (g_origin == SAMSIM_PROFILE_FROM_TOP ? !first : !last));
          next = s.b0 + s.nb;
          ++passes;
          return 0;
        });
        CHECK(rc == 0 && next == g_nbins && passes == (g_nbins + chunk - 1) / chunk);
      }
  }
  std::printf("ok\n");
  return 0;
}
'''


def test_the_chunk_keeps_its_bounds_for_every_number_of_value_bins(tmp_path):
    """samsim_pass_plan.h compiled alone by g++.  For every nvbins in 1 .. 254: 1 <= chunk <= 64; the LDS of a pass -- the tile
    [chunk][65], the masks, the weights, the table [chunk][(nvbins + 2) | 1] of doubles, formed here on its own -- is what the header
    says and at most the launcher's limit; one more depth bin would not fit (below 64); the waves' tables of a pass and the largest
    result fit SAMSIM_WPHIST_SCRATCH_BYTES; capi.wphist_chunk is the header's chunk; and pass_plan with that chunk tiles [0, nbins)
    once in ascending b0 for nbins in {1, chunk - 1, chunk, chunk + 1, 1024} from both origins, with lead where the header says."""
    src = tmp_path / "wphist_chunk.cpp"
    src.write_text(CHUNK_PROGRAM)
    exe = tmp_path / "wphist_chunk"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "samsim_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout[-400:]
    head = lines[0].split()
    grid, lds_limit, scratch, max_bins, max_vbins = (int(head[i]) for i in (1, 3, 5, 7, 9))
    assert (grid, lds_limit, scratch) == (capi.WPHIST_GRID, capi.WPHIST_LDS_BYTES, capi.WPHIST_SCRATCH_BYTES)
    assert lds_limit <= 64 << 10 and max_vbins == capi.HIST_MAX_VBINS == 254 and max_bins == capi.PROFILE_MAX_BINS
    result = max_bins * (max_vbins + 2) * 8
    rows = [tuple(int(x) for x in ln.split()) for ln in lines[1:-1]]
    assert [r[0] for r in rows] == list(range(1, 255))
    for nv, chunk, lds, wave_doubles in rows:
        stride = (nv + 2) | 1
        assert 1 <= chunk <= 64, nv
        assert chunk == capi.wphist_chunk(nv), nv
        assert lds == chunk * 65 * 8 + 64 * 8 + 64 * 8 + chunk * stride * 8 <= lds_limit, nv
        assert chunk == 64 or (chunk + 1) * (65 + stride) * 8 + 1024 > lds_limit, nv          # the largest that fits
        assert wave_doubles == chunk * (nv + 2)
        assert grid * chunk * (nv + 2) * 8 + result <= scratch, nv
    chunks = {nv: c for nv, c, _, _ in rows}
    assert chunks[1] == chunks[59] == 64 and chunks[60] == 63 and chunks[254] == 25
    text = open(os.path.join(ROOT, "include", "samsim.h")).read()
    assert f"#define SAMSIM_WPHIST_SCRATCH_BYTES ({scratch >> 20}ull << 20)" in text


def test_profile_quantiles_against_the_weighted_quantile_of_the_reference():
    """a seeded random table of values and weights per depth bin: the bracket of every row and q contains the reference's weighted
    quantile of the row's values; a row without weight is NaN in both; all weight in an outer entry gives an infinite end; a
    negative sum is refused"""
    rng = np.random.default_rng(20211)
    nvbins, v0, dv, nbins, n = 24, -3.0, 0.25, 9, 400
    E = capi.hist_edges(nvbins, v0, dv)
    qs = (0.0, 0.05, 0.5, 0.95, 1.0)
    values = rng.normal(0.0, 2.0, (nbins, n))
    values[3] = -50.0 - rng.random(n)                                          # everything below the first edge
    values[4] = 50.0 + rng.random(n)                                           # everything at or above the last edge
    w = rng.gamma(0.5, 1.0, (nbins, n)) * rng.integers(1, 1 << 10, (nbins, n))  # positive, spread over decades
    w[6] = 0.0                                                                 # a row without weight
    assert (w[:6] > 0.0).all()
    table = np.zeros((nbins, nvbins + 2))
    for b in range(nbins):
        en = (E[None, :] <= values[b][:, None]).sum(1)
        for i in range(nvbins + 2):
            table[b, i] = w[b][en == i].sum()
    lo, hi = capi.weighted_profile_quantiles(table, v0, dv, qs)
    assert lo.shape == hi.shape == (len(qs), nbins)
    assert np.isnan(lo[:, 6]).all() and np.isnan(hi[:, 6]).all()
    assert (lo[:, 3] == -np.inf).all() and (hi[:, 3] == E[0]).all() and (lo[:, 4] == E[-1]).all() and (hi[:, 4] == np.inf).all()
    checked = 0
    for b in range(nbins):
        if b == 6:
            continue
        ok = np.ones(n, dtype=bool)
        for k, q in enumerate(qs):
            ref = wr.weighted_quantile(values[b], w[b], ok, q)
            # the table's sums and the reference's cumulative weights round differently: a target within 1e-12 of an entry's end
            # may fall either way, and the seed has none
            cum = np.cumsum(table[b])
            assert not (np.abs(cum[:-1] - q * cum[-1]) <= 1e-12 * cum[-1]).any() or q in (0.0, 1.0)
            assert lo[k, b] <= ref < hi[k, b], (b, q, lo[k, b], ref, hi[k, b])
            assert (lo[k, b], hi[k, b]) == capi.weighted_quantile_bracket(table[b], v0, dv, q)
            checked += 1
    assert checked == (nbins - 1) * len(qs)
    assert np.isfinite(lo[2, [0, 1, 2, 5, 7, 8]]).all() and np.isfinite(hi[2, [0, 1, 2, 5, 7, 8]]).all()    # the medians lie inside
    bad = table.copy()
    bad[1, 5] = -1.0
    with pytest.raises(ValueError):
        capi.weighted_profile_quantiles(bad, v0, dv, qs)
    with pytest.raises(ValueError):
        capi.weighted_profile_quantiles(table, v0, dv, (0.5, 1.5))
    with pytest.raises(ValueError):
        capi.weighted_profile_quantiles(table[0], v0, dv, qs)
