"""Host-side mirror of mo_init (samsim_amd/testcases.py) and ensemble helpers; CPU only."""
import re

import numpy as np
import pytest

from samsim_amd import testcases as tcs
from samsim_amd.capi import State, NARR, NSCAL
from tests.helpers import golden
from tests.oracle_lib import oracle_solver


def test_testcase1_settings_match_reference_dat_settings():
    """dat_settings.dat of Reference_testcase1_with_Version_2 (the reference's echo of init, mo_output.f90:41-106)"""
    text = str(golden("tc1_reference_dat.npz")["settings_text"])
    kv = dict(re.findall(r"^(\w+)\s*=?\s+(-?[\d.]+)\s*$", text, flags=re.M))
    cfg, st = tcs.testcase1(1)
    assert float(kv["dt"]) == cfg.dt and float(kv["thick_0"]) == cfg.thick_0
    assert float(kv["time_out"]) == cfg.time_out and float(kv["time_total"]) == cfg.time_total
    assert float(kv["T_bottom"]) == cfg.T_bottom and float(kv["S_bu_bottom"]) == cfg.S_bu_bottom
    assert int(kv["N_top"]) == cfg.n_top and int(kv["N_middle"]) == cfg.n_middle and int(kv["N_bottom"]) == cfg.n_bottom
    assert int(kv["Nlayer"]) == cfg.nlayer
    for flag in ["boundflux_flag", "atmoflux_flag", "albedo_flag", "grav_flag", "flush_flag", "flood_flag",
                 "grav_heat_flag", "flush_heat_flag", "harmonic_flag", "prescribe_flag", "salt_flag", "turb_flag",
                 "bottom_flag", "tank_flag"]:
        assert int(kv[flag]) == getattr(cfg, flag), flag
    assert cfg.precip_flag == 0 and re.search(r"^precip_flag\s*$", text, flags=re.M)  # I9.0 prints a zero as blanks
    assert cfg.i_time_out == 3600 and tcs.i_time(cfg) == 259200 and cfg.thick_min == 0.001


def test_testcase4_settings():
    cfg, st = tcs.testcase4(3)
    assert (cfg.nlayer, cfg.n_top, cfg.n_middle, cfg.n_bottom) == (100, 20, 60, 20)
    assert (cfg.boundflux_flag, cfg.atmoflux_flag, cfg.precip_flag, cfg.flush_flag, cfg.flush_heat_flag) == (2, 2, 1, 5, 2)
    assert cfg.i_time_out == 8640 and tcs.i_time(cfg) == 14191200
    assert st.lay.shape == (NARR, 100, 3) and st.scal.shape == (NSCAL, 3)
    assert (st.arr("thick")[0] == 0.01).all() and (st.arr("thick")[1:] == 0).all()
    assert (st.arr("S_abs")[0] == 34.0 * (0.01 * 1028.0)).all() and (st.arr("H_abs") == 0).all()


def test_ensemble_perturbation_is_counter_based():
    dT, ps = tcs.ensemble_perturbation(1000)
    assert dT[0] == 0.0 and ps[0] == 1.0
    assert (np.abs(dT) <= 2.0).all() and (np.abs(ps - 1.0) <= 0.3).all()
    assert np.std(dT) > 1.0 and np.std(ps) > 0.15
    # a shard regenerates exactly its slice of the global sequence
    dT2, ps2 = tcs.ensemble_perturbation(100, col0=500)
    assert np.array_equal(dT2, dT[500:600]) and np.array_equal(ps2, ps[500:600])


def test_state_replicate_and_window():
    cfg, st = tcs.testcase1(1)
    r = st.replicate(5)
    assert r.lay.shape[2] == 5 and (r.lay == st.lay[:, :, :1]).all()
    w = r.window(2, 2)
    assert w.ncol == 2 and w.lay.flags.c_contiguous


def test_checkpoint_file_roundtrip_and_bitwise_continuation(tmp_path):
    """samsim_amd.checkpoint driven through the checker library: a run interrupted by save -> new handle
    -> load continues bit for bit, in column chunks that do not divide the ensemble"""
    from samsim_amd import checkpoint
    from tests.helpers import sheba_forcing
    ncol = 10
    cfg, st = tcs.testcase4(ncol)
    dT, ps = tcs.ensemble_perturbation(ncol)

    def fresh():
        o = oracle_solver(cfg, ncol)
        o.set_forcing(*sheba_forcing(), dT, ps)
        return o
    a = fresh()
    a.set_state(st)
    a.set_clock()
    a.step(9000)                       # past the first output point and the first ice layers
    path = str(tmp_path / "restart.chk")
    checkpoint.save(a, path, chunk=4)
    h = checkpoint.read_header(path)
    assert (h["ncol"], h["nlayer"], h["step"], h["testcase"]) == (ncol, cfg.nlayer, 9000, 4)
    b = fresh()
    checkpoint.load(b, path)
    a.step(3000)
    b.step(3000)
    sa, sb = a.get_state(), b.get_state()
    assert np.array_equal(sa.lay, sb.lay) and np.array_equal(sa.scal, sb.scal) and np.array_equal(sa.n_active, sb.n_active)
    ka, kb = a.get_clock(), b.get_clock()
    assert (ka.time, ka.step, ka.n_time_out, ka.time_counter) == (kb.time, kb.step, kb.n_time_out, kb.time_counter)
    with pytest.raises(ValueError):
        checkpoint.load(oracle_solver(cfg, ncol + 1), path)


def test_checkpoint_with_tracers_continues_bitwise(tmp_path):
    """a tank experiment with its tracer (init(6): bgc_flag 2, tank_flag 2, so that the concentration of the water below is
    per-column state): save -> new handle -> set_tracers -> load continues bit for bit; a handle without tracers refuses"""
    from samsim_amd import checkpoint
    ncol = 3
    cfg, st = tcs.testcase6(ncol)
    bottom, total, q = tcs.tracers(cfg, st)

    def fresh():
        o = oracle_solver(cfg, ncol)
        o.set_tracers(bottom, total)
        return o
    a = fresh()
    a.set_state(st)
    a.set_tracer_state(q)
    a.set_clock()
    a.step(20000)
    assert a.get_state().n_active.min() > 3
    path = str(tmp_path / "restart_bgc.chk")
    checkpoint.save(a, path, chunk=2)
    assert checkpoint.read_header(path)["n_bgc"] == 1
    b = fresh()
    checkpoint.load(b, path)
    a.step(5000)
    b.step(5000)
    sa, sb = a.get_state(), b.get_state()
    assert np.array_equal(sa.lay, sb.lay) and np.array_equal(sa.scal, sb.scal) and np.array_equal(sa.n_active, sb.n_active)
    (qa, ba), (qb, bb) = a.get_tracer_state(), b.get_tracer_state()
    assert np.array_equal(qa, qb) and np.array_equal(ba, bb)
    assert ba.min() > bottom[0] and qa[0, 2].min() > 0.0        # the tank got richer, the ice holds tracer
    cfg0, _ = tcs.testcase6(ncol)
    with pytest.raises(ValueError):
        checkpoint.load(oracle_solver(cfg0, ncol), path)


def test_ensemble_statistics_of_the_checker():
    """samsim_get_ensemble_stats semantics (count / mean / min / max / population std over the columns without a STOP
    code) on the checker library against numpy"""
    from tests.helpers import sheba_forcing
    ncol = 24
    cfg, st = tcs.testcase4(ncol)
    o = oracle_solver(cfg, ncol)
    o.set_forcing(*sheba_forcing(), *tcs.ensemble_perturbation(ncol))
    o.set_state(st)
    o.set_clock()
    o.run_to_output()
    o.step(8641)                       # second output point: vital signs of an ice-covered ensemble
    s = o.get_state()
    stats = o.ensemble_stats(["thickness", "thick_snow", "T2m", "N_active"])
    for n in ("thickness", "thick_snow", "T2m"):
        v = s.sc(n)
        q = stats[n]
        assert q.count == ncol and q.min == v.min() and q.max == v.max()
        assert abs(q.mean - v.mean()) <= 1e-13 * max(1.0, abs(v.mean())) and abs(q.std - v.std()) <= 1e-12 * max(1.0, v.std())
    assert stats["N_active"].max == s.n_active.max() and stats["N_active"].mean == pytest.approx(s.n_active.mean())
    assert stats["T2m"].std > 0.5


def test_device_layout_index_is_a_bijection(tmp_path):
    """samsim_device.h: the layer block is stored per 64-column block, [block][layer][array][lane].  DEV_LAY_INDEX must map every
    (array, layer, column) of a handle to its own double inside DEV_LAY_DOUBLES, keep a wave's 64 columns of one (array, layer)
    contiguous, and keep the sixteen arrays of a layer row within 8 KiB of each other (the kernel addresses them with the
    signed 13-bit immediate of one row address) -- checked on the host with the header compiled by g++."""
    import os
    import subprocess
    from tests.helpers import ROOT
    src = tmp_path / "layout.cpp"
    src.write_text(r'''
#include <cstdio>
#include <vector>
#include "samsim_device.h"
int main() {
  const int N = 7; const size_t ncol = 200;   // not a multiple of 64: the last block is ragged
  const size_t total = DEV_LAY_DOUBLES(N, ncol);
  std::vector<char> seen(total, 0);
  for (int a = 0; a < DEV_NARR; ++a) for (int k = 0; k < N; ++k) for (size_t c = 0; c < ncol; ++c) {
    const size_t i = DEV_LAY_INDEX(a, k, c, N, ncol);
    if (i >= total || seen[i]) { std::printf("clash a=%d k=%d c=%zu\n", a, k, c); return 1; }
    seen[i] = 1;
  }
  // lanes contiguous, arrays of a row 512 B apart, rows DEV_ROWB apart
  if (DEV_LAY_INDEX(3, 2, 65, N, ncol) != DEV_LAY_INDEX(3, 2, 64, N, ncol) + 1) return 2;
  if ((DEV_LAY_INDEX(4, 2, 64, N, ncol) - DEV_LAY_INDEX(3, 2, 64, N, ncol)) * 8 != 512) return 3;
  if ((DEV_LAY_INDEX(0, 3, 64, N, ncol) - DEV_LAY_INDEX(0, 2, 64, N, ncol)) * 8 != DEV_ROWB) return 4;
  if (DEV_ROWB != 8192 || DEV_NARR != 16) return 5;
  std::printf("ok %zu\n", total);
  return 0;
}
''')
    exe = tmp_path / "layout"
    inc = os.path.join(ROOT, "samsim_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", inc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout


def test_checkpoint_layout_without_the_status_block_is_refused(tmp_path):
    """the chunk layout changed when checkpoints began to carry the STOP codes: files of the older layout carry another magic
    ("SAMCHK01") and are refused, not mis-read"""
    import struct
    from samsim_amd import checkpoint
    p = tmp_path / "old.chk"
    p.write_bytes(struct.pack("<6q d 4q 5q", int.from_bytes(b"SAMCHK01", "little"), 4, 90, 15, 38, 1, 0.0, 0, 0, 1, 0, 0, 0, 0, 0, 0))
    with pytest.raises(ValueError, match="SAMCHK01"):
        checkpoint.read_header(str(p))
    p.write_bytes(struct.pack("<6q d 4q 5q", checkpoint.MAGIC, 4, 90, 15, 38, 1, 0.0, 7, 0, 1, 0, 0, 1, 0, 0, 0))
    assert checkpoint.read_header(str(p))["step"] == 7


def test_plain_form_of_the_permeability_power_against_the_exact_power(tmp_path):
    """samsim_pow.h compiled for the host: x**3.1 as x*x*x * exp(0.1 * log x) (the form the kernel keeps for liquid fractions below
    1e-33, and the reference of its tenth-root form on the GPU, tools/div_probe) against powl(x, 3 + 0.1) over the range of the
    permeability law, 1e-9 .. 3000: within 1e-15 relative"""
    import os
    import subprocess
    src = tmp_path / "powtest.c"
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "samsim_amd", "csrc", "samsim_pow.h")
    src.write_text('''#include <stdio.h>
#include <math.h>
#include "%s"
int main(void) {
  double mx = 0.0;
  const long double e = (long double)3.0 + (long double)0.1;   /* the exponent the form evaluates: 3 + the double 0.1 */
  for (int i = 0; i < 4000000; i++) {
    const double u = (i + 0.5) / 4000000.0, x = exp(log(1e-9) + u * (log(3000.0) - log(1e-9)));
    const double r = (double)powl((long double)x, e), err = fabs(sp_pow_3p1_plain(x) - r) / r;
    if (err > mx) mx = err;
  }
  printf("%%.3e\\n", mx);
  return 0;
}
''' % hdr)
    exe = tmp_path / "powtest"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", str(src), "-o", str(exe), "-lm"])
    worst = float(subprocess.check_output([str(exe)]).decode())
    assert worst <= 1e-15, worst


def test_short_forms_of_the_scalar_powers_against_the_exact_powers(tmp_path):
    """samsim_pow.h compiled for the host: x*sqrt(x) for x**1.5 (bulk salinities 1e-3 .. 300 g/kg) and (x*x)*(x*x) for x**4
    (surface temperatures 150 .. 400 K) against powl: within 2 ulp (observed 2.2e-16 and 4.4e-16 relative)"""
    import os
    import subprocess
    src = tmp_path / "powtest2.c"
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "samsim_amd", "csrc", "samsim_pow.h")
    src.write_text('''#include <stdio.h>
#include <math.h>
#include "%s"
int main(void) {
  double m15 = 0.0, m4 = 0.0;
  for (int i = 0; i < 4000000; i++) {
    const double u = (i + 0.5) / 4000000.0, x = exp(log(1e-3) + u * (log(300.0) - log(1e-3))), t = 150.0 + 250.0 * u;
    const double r = (double)powl((long double)x, 1.5L), e = fabs(sp_pow_1p5(x) - r) / r;
    const double r4 = (double)powl((long double)t, 4.0L), e4 = fabs(sp_pow_4(t) - r4) / r4;
    if (e > m15) m15 = e;
    if (e4 > m4) m4 = e4;
  }
  printf("%%.3e %%.3e\\n", m15, m4);
  return 0;
}
''' % hdr)
    exe = tmp_path / "powtest2"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", str(src), "-o", str(exe), "-lm"])
    w15, w4 = (float(v) for v in subprocess.check_output([str(exe)]).decode().split())
    assert w15 <= 3.4e-16 and w4 <= 4.5e-16, (w15, w4)


ROW_PLAN_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "samsim.h"
#include "samsim_row_plan.h"

struct Item { int a, b; };   // b < 0: one array
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s (list %d, item %d)\n", __LINE__, #c, g_list, g_item); std::exit(1); } } while (0)
static int g_list = -1, g_item = -1;

template <int MAXG> int has(const RowPlan<MAXG> &p, int g, int x) {
  for (int j = 0; j < p.gn[g]; ++j) if (p.grow[g][j] == x) return 1;
  return 0;
}
template <int MAXG> bool room(const RowPlan<MAXG> &p, int g, Item it) {
  return p.gn[g] + !has(p, g, it.a) + (it.b >= 0 && !has(p, g, it.b)) <= ROW_PLAN_ROWS;
}

// plans the list and checks every property of the plan; at[i] = the place of item i
template <int MAXG> void plan(const Item *it, int n, RowPlan<MAXG> &p, RowPlace *at) {
  p = RowPlan<MAXG>{};
  for (int i = 0; i < n; ++i) {
    g_item = i;
    const RowPlan<MAXG> before = p;
    const RowPlace r = at[i] = row_plan_place(p, it[i].a, it[i].b);
    CHECK(r.group >= 0 && r.group <= before.ngroups && r.group < MAXG);
    for (int g = 0; g < r.group; ++g) CHECK(!room(before, g, it[i]));   // first-fit: no earlier walk had room for it
    if (r.group < before.ngroups) CHECK(room(before, r.group, it[i]) && p.ngroups == before.ngroups);
    else CHECK(p.ngroups == before.ngroups + 1);
    for (int g = 0; g < before.ngroups; ++g) {   // the rows the earlier items were given stay where they are
      CHECK(p.gn[g] >= before.gn[g] && (g == r.group || p.gn[g] == before.gn[g]));
      for (int j = 0; j < before.gn[g]; ++j) CHECK(p.grow[g][j] == before.grow[g][j]);
    }
  }
  g_item = -1;
  CHECK(p.ngroups >= (n > 0) && p.ngroups <= n);
  int items[MAXG] = {};
  for (int i = 0; i < n; ++i) {   // every needed array of an item is among its walk's rows, at ia / ib
    const RowPlace r = at[i];
    CHECK(r.group >= 0 && r.group < p.ngroups);
    ++items[r.group];
    CHECK(r.ia >= 0 && r.ia < p.gn[r.group] && p.grow[r.group][r.ia] == it[i].a);
    if (it[i].b >= 0) CHECK(r.ib >= 0 && r.ib < p.gn[r.group] && p.grow[r.group][r.ib] == it[i].b);
  }
  for (int g = 0; g < p.ngroups; ++g) {   // no walk is empty, holds a row twice or more than ROW_PLAN_ROWS rows
    CHECK(items[g] > 0 && p.gn[g] >= 1 && p.gn[g] <= ROW_PLAN_ROWS);
    for (int j = 0; j < p.gn[g]; ++j) {
      CHECK(p.grow[g][j] >= 0 && p.grow[g][j] < SAMSIM_NARR);
      for (int l = 0; l < j; ++l) CHECK(p.grow[g][l] != p.grow[g][j]);
    }
  }
}

static unsigned long long g_seed = 20240917ull;
static int rnd(int n) {   // a 64-bit LCG (Knuth's MMIX constants), the same lists wherever the program runs
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (int)((g_seed >> 33) % (unsigned long long)n);
}

int main() {
  const int S_BU_ROWS[2] = {SAMSIM_A_S_ABS, SAMSIM_A_M};
  int walks = 0, two = 0;
  for (g_list = 0; g_list < 300; ++g_list) {
    Item it[32];
    const int n = 1 + rnd(32);
    const int narr = g_list % 3 == 0 ? SAMSIM_NARR : 3 + rnd(SAMSIM_NARR - 2);   // few arrays: shared rows; many: full walks
    for (int i = 0; i < n; ++i) {
      it[i].a = rnd(narr);
      it[i].b = -1;
      if (rnd(3) == 0) { do it[i].b = rnd(narr); while (it[i].b == it[i].a); ++two; }
    }
    RowPlan<32> p;
    RowPlace at[32];
    plan(it, n, p, at);
    walks += p.ngroups;
  }
  CHECK(two > 1000 && walks > 600);   // the lists are not trivial
  g_list = -1;

  // SPECS_ICE of tests/test_gpu_functionals.py on a handle that has stepped (S_bu reads S_abs and m): five distinct rows, two walks;
  // the last functional, on S_abs, joins the first walk, where next-fit put it into the second
  {
    const Item ice[8] = {{SAMSIM_A_PSI_L, -1}, {SAMSIM_A_PSI_L, -1}, {SAMSIM_A_T, -1}, {S_BU_ROWS[0], S_BU_ROWS[1]},
                         {SAMSIM_A_PSI_L, -1}, {SAMSIM_A_RAY, -1}, {SAMSIM_A_RAY, -1}, {SAMSIM_A_S_ABS, -1}};
    const int want[8][3] = {{0, 0, 0}, {0, 0, 0}, {0, 1, 0}, {0, 2, 3}, {0, 0, 0}, {1, 0, 0}, {1, 0, 0}, {0, 2, 0}};
    RowPlan<8> p;
    RowPlace at[8];
    plan(ice, 8, p, at);
    CHECK(p.ngroups == 2 && p.gn[0] == 4 && p.gn[1] == 1);
    CHECK(p.grow[0][0] == SAMSIM_A_PSI_L && p.grow[0][1] == SAMSIM_A_T && p.grow[0][2] == SAMSIM_A_S_ABS && p.grow[0][3] == SAMSIM_A_M);
    CHECK(p.grow[1][0] == SAMSIM_A_RAY);
    for (g_item = 0; g_item < 8; ++g_item)
      CHECK(at[g_item].group == want[g_item][0] && at[g_item].ia == want[g_item][1] && at[g_item].ib == want[g_item][2]);
  }
  // three one-row items, then S_bu, then a fifth array: the fifth joins the first walk (next-fit: the second, at position 2)
  {
    const Item five[5] = {{SAMSIM_A_T, -1}, {SAMSIM_A_PSI_L, -1}, {SAMSIM_A_RAY, -1}, {S_BU_ROWS[0], S_BU_ROWS[1]}, {SAMSIM_A_H_ABS, -1}};
    RowPlan<8> p;
    RowPlace at[5];
    plan(five, 5, p, at);
    CHECK(p.ngroups == 2 && p.gn[0] == 4 && p.gn[1] == 2);
    CHECK(at[3].group == 1 && at[3].ia == 0 && at[3].ib == 1);
    CHECK(at[4].group == 0 && at[4].ia == 3 && p.grow[0][3] == SAMSIM_A_H_ABS);
  }
  std::printf("ok %d walks\n", walks);
  return 0;
}
'''


def test_row_plan_places_every_item_by_first_fit(tmp_path):
    """samsim_row_plan.h compiled alone by g++: 300 seeded random lists of up to 32 items that need one or two of the SAMSIM_NARR
    arrays.  In every plan each needed array of an item is among its walk's rows at ia / ib, no walk holds a row twice, more than
    four rows or no item, an item is never in a later walk when an earlier one had room (first-fit), and placing an item moves no
    row of the items before it.  Pinned: the plan of SPECS_ICE on a stepped handle (five distinct rows: two walks) and a list on
    which first-fit and next-fit differ."""
    import os
    import subprocess
    from tests.helpers import ROOT
    src = tmp_path / "row_plan.cpp"
    src.write_text(ROW_PLAN_PROGRAM)
    exe = tmp_path / "row_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "samsim_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout


PASS_PLAN_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "samsim_pass_plan.h"

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s (nbins %d, chunk %d, origin %d, narrays %d, pass %d)\n", __LINE__, #c, g_nbins, g_chunk, g_origin, g_narrays, g_pass); std::exit(1); } } while (0)
static int g_nbins, g_chunk, g_origin, g_narrays, g_pass;

int main() {
  const int NBINS[7] = {1, 63, 64, 65, 128, 129, 1024};
  const int chunks[3] = {dev_hist_chunk(40), dev_hist_chunk(254), dev_hist_chunk(1022)};   // the launcher's own rule
  CHECK(chunks[0] == 64 && chunks[1] == 42 && chunks[2] == 14);   // 64 and the two smaller chunks
  const int origins[2] = {SAMSIM_PROFILE_FROM_TOP, SAMSIM_PROFILE_FROM_BOTTOM};
  int passes = 0;
  for (int in = 0; in < 7; ++in)
    for (int ic = 0; ic < 3; ++ic)
      for (int io = 0; io < 2; ++io)
        for (int ia = 0; ia < 2; ++ia) {
          g_nbins = NBINS[in]; g_chunk = chunks[ic]; g_origin = origins[io]; g_narrays = ia ? 8 : 1;
          g_pass = 0;
          int array = 0, next = 0;   // the array being tiled and the bin its next pass must begin at
          const int rc = pass_plan(g_narrays, g_nbins, g_chunk, g_origin, [&](const PassSpan &s) {
            if (next == g_nbins) { ++array; next = 0; }   // the previous array is complete: the next one begins
            CHECK(s.array == array && array < g_narrays);
            CHECK(s.b0 == next && s.nb >= 1 && s.nb <= g_chunk && s.b0 + s.nb <= g_nbins);
            const bool first = s.b0 == 0, last = s.b0 + s.nb == g_nbins;
            CHECK(s.lead == (g_origin == SAMSIM_PROFILE_FROM_TOP ? !first : !last));
            next = s.b0 + s.nb;
            ++g_pass;
            return 0;
          });
          CHECK(rc == 0 && array == g_narrays - 1 && next == g_nbins);   // every array tiled to its end, none left out
          CHECK(g_pass == g_narrays * ((g_nbins + g_chunk - 1) / g_chunk));
          passes += g_pass;
        }
  // the first value that is not 0 ends the enumeration and comes back
  g_pass = 0;
  CHECK(pass_plan(8, 129, 64, SAMSIM_PROFILE_FROM_TOP, [&](const PassSpan &) { return ++g_pass == 4 ? -3 : 0; }) == -3 && g_pass == 4);
  std::printf("ok %d passes\n", passes);
  return 0;
}
'''


def test_pass_plan_tiles_every_array_once_and_marks_the_leading_passes(tmp_path):
    """samsim_pass_plan.h compiled alone by g++: nbins in {1, 63, 64, 65, 128, 129, 1024} x chunk in {64, 42, 14} (what a pass of the
    statistics serves and what dev_hist_chunk gives at 40, 254 and 1022 value bins) x both origins x 1 and 8 arrays.  The passes
    tile [0, nbins) exactly once per array, the arrays in order and b0 ascending, every nb <= chunk, and lead is set exactly for the
    passes that do not begin where the walk begins: from the top every pass but the first, from the bottom every pass but the last."""
    import os
    import subprocess
    from tests.helpers import ROOT
    src = tmp_path / "pass_plan.cpp"
    src.write_text(PASS_PLAN_PROGRAM)
    exe = tmp_path / "pass_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "samsim_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout


SLOT_WALK_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include "samsim_slot_walk.h"

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s (ns %d, p %d)\n", __LINE__, #c, g_ns, g_p); std::exit(1); } } while (0)
static int g_ns, g_p;

int main() {
  using namespace slot_walk;
  int pairs = 0;
  for (g_ns = 1; g_ns <= 8; ++g_ns) {
    // the lane update's own loop: p advances with (i, j) over the upper triangle, row by row
    g_p = 0;
    for (int i = 0; i < g_ns; ++i)
      for (int j = i; j < g_ns; ++j, ++g_p) {
        int pi = -1, pj = -1;
        pair_of(g_p, g_ns, pi, pj);
        CHECK(pi == i && pj == j);
      }
    CHECK(g_p == g_ns * (g_ns + 1) / 2);   // exactly the upper triangle, no pair left out and none twice
    pairs += g_p;
  }
  for (g_ns = 0; g_ns <= 9; ++g_ns) {
    int reached = 0, calls = 0;
    const bool known = dispatch_nslots(g_ns, [&](auto ns) { reached = decltype(ns)::value; ++calls; });
    if (g_ns >= 1 && g_ns <= 8) CHECK(known && calls == 1 && reached == g_ns);
    else CHECK(!known && calls == 0);
  }
  CHECK(slot_grid(1, 1024) == 1 && slot_grid(64, 1024) == 1 && slot_grid(65, 1024) == 2 && slot_grid(70001, 1024) == 1024);
  std::printf("ok %d pairs\n", pairs);
  return 0;
}
'''


def test_slot_walk_pairs_and_dispatch(tmp_path):
    """The plain-C++ part of samsim_slot_walk.h compiled alone by g++, once as it is and once under the address and undefined
    behaviour sanitizers: for 1 to 8 slots pair_of(p, ns) enumerates exactly the upper triangle, row by row, in the order in which
    the lane update's `for i, for j = i` loop advances p; dispatch_nslots reaches the instantiation NS == nslots for 1 to 8 and
    refuses 0 and 9 without a call."""
    import os
    import subprocess
    from tests.helpers import ROOT
    src = tmp_path / "slot_walk.cpp"
    src.write_text(SLOT_WALK_PROGRAM)
    for flags in ([], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]):
        exe = tmp_path / ("slot_walk_san" if flags else "slot_walk")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "samsim_amd", "csrc"),
                               str(src), "-o", str(exe)])
        out = subprocess.run([str(exe)], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok 120 pairs"), out.stdout + out.stderr
