// samsim_kernels.hip -- hand-written CDNA4 (gfx950) kernel for the per-timestep 1-D sea-ice column update.
//
// What it computes: the body of the reference time loop, pgriewank/SAMSIM mo_grotz.f90:182-835, for `ncol`
// independent columns, `nsteps` steps per launch.  One lane owns one column for the whole launch (columns
// never communicate), state lives in HBM per 64-column block as [block][layer][array][lane] float64 so that every
// per-layer access of a wave is one contiguous 512-byte line and a layer row's arrays sit within one row address's
// immediate range, and a column's layers are walked sequentially inside the lane with the neighbour values
// (k-1, k, k+1) carried in registers.  No MFMA (there is no contraction in this path); LDS holds the per-column
// scalars that must survive the two layer loops of a step (19 slots per lane, own words only: no barrier); no
// cross-lane traffic except wave-uniform votes.
//
// The sequential structure inside a column is dictated by the reference: getT's Newton iteration is seeded
// with the temperature of the layer below (mo_grotz.f90:298-303) and stops at |f| <= 1 J/kg, so the result
// depends on the guess (hard part 1) and the bottom->top chain has to be reproduced.
//
// Sweeps of a step (direction, what is fused, where it is; reference lines at the functions):
//   first sweep  up    S_bu, H -> getT chain -> S_br -> Expulsion; permeability + suffix scans -> Rayleigh number.  The previous step's
//                      up sweep has done it for layers N_active..2, so a step runs it for layer 1 only (prologue_top_layer,
//                      samsim_sweeps_fused.h); the full one (sweep_thermo_expulsion, samsim_sweeps_unfused.h) runs after
//                      samsim_set_state and after flushing or a regrid changed the column below layer 1
//   fused down   down  sweep_down_fused (samsim_sweeps_fused.h): expulsion_flux + mass_transfer + S_bu refresh, gravity drainage with
//                      its return flow, the conductive update of layers >= 2; thin-snow coupling, surface balance and Beer law inside
//   fused up     up    sweep_up_fused (samsim_sweeps_fused.h): the second getT chain and, from the same registers, the NEXT step's
//                      first sweep for layers N_active..2
//   unfused      down  down_unfused (samsim_sweeps_unfused.h): the reference's order sweep by sweep -- sweep_expulsion_transfer,
//                      sweep_grav_drain, sweep_heat_down -- for a wave with something between expulsion and drainage (an output
//                      point, a flooding the fused order cannot take) or without Rayleigh-number drainage; then the same up sweep
//   melt season: func_freeboard (2 down), flush3 (1 up + 1 down), flush4, flood (samsim_melt.h), snow (samsim_surface.h),
//                layer_dynamics (samsim_regrid.h); tracers: bgc_advection (samsim_tracers.h)
// The reference's O(N^2) loops (harmonic-mean permeability, freeboard search) are O(N) scans here; sums are
// therefore associated differently (1e-16 relative), everything else follows the reference's operation order.
//
// One translation unit in parts.  Every device function that takes the column struct or the context by reference has to be inlined
// into the kernel (see RARE, samsim_step_types.h), so the parts are headers included here in order, not separate objects.  They are
// not stand-alone headers: each relies on the ones before it and on the conventions of samsim_step_types.h -- `c` is the lane's Col,
// `x` the Ctx, `g` the run-time configuration; CL() an LDS scalar, GS() a word of the scalar block, LAY() / LAYU() an element of the
// layer block, CFG() a flag of the instantiation K.  This file keeps the output block, one time step (column_step), the kernel and
// its launch.
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

#include "samsim_device.h"
#include "samsim_probe.h"
#include "samsim_step_types.h"
#include "samsim_thermo.h"
#include "samsim_surface.h"
#include "samsim_sweeps_fused.h"
#include "samsim_melt.h"
#include "samsim_sweeps_unfused.h"
#include "samsim_regrid.h"
#include "samsim_tracers.h"

namespace {

// ---------------------------------------------------------------- vital signs, mo_grotz.f90:192-223 (output only)
template <class K>
__device__ RARE void vital_signs(Col &c, const Ctx &x) {
  const samsim_config &g = x.p->cfg;
  const int Na = c.Na;
  // (evaluated at the top of the loop with the PREVIOUS step's volume fractions, as in the reference: the psi arrays
  // are rewritten by this step's down sweep only later)
  double sH = 0.0, sm = 0.0, sS = 0.0, resist = 0.0, sth = 0.0, sS1 = 0.0, sm1 = 0.0;
  for (int k = 1; k <= Na; ++k) {
    const double H_abs = LAY(SAMSIM_A_H_ABS, k), m = LAY(SAMSIM_A_M, k), S_abs = LAY(SAMSIM_A_S_ABS, k);
    sH += H_abs; sm += m; sS += S_abs;
    if (k <= Na - 1) {
      const double thick = LAY(SAMSIM_A_THICK, k);
      resist = resist + thick / (LAY(SAMSIM_A_PSI_L, k) * k_l + LAY(SAMSIM_A_PSI_S, k) * k_s);
      sth += thick; sS1 += S_abs; sm1 += m;
    }
  }
  const double thN = LAY(SAMSIM_A_THICK, Na), psN = LAY(SAMSIM_A_PSI_S, Na);
  c.energy_stored = CL(H_abs_snow) + sH - g.T_bottom * sm * c_l;
  c.freshwater = sm / rho_l;
  c.freshwater = c.freshwater * (1.0 - sS / sm / ref_salinity);
  c.freshwater = c.freshwater + CL(m_snow) / rho_l;
  resist = resist + thN * psN / psi_s_min * (psi_s_min * k_s + 1.0 - psi_s_min * k_l);
  if (CL(thick_snow) > g.thick_min / 110.0) resist = resist + quot(CL(thick_snow), func_k_snow(CL(m_snow), CL(thick_snow)));
  c.total_resist = resist;
  c.thickness = ((Na > 1) ? sth : 0.0) + thN * psN / psi_s_min;
  if (Na > 1) {
    const double SN = LAY(SAMSIM_A_S_ABS, Na), mN = LAY(SAMSIM_A_M, Na);
    c.bulk_salin = (sS1 + SN * psN / psi_s_min) / (sm1 + mN * psN / psi_s_min);
  } else {
    c.bulk_salin = LAY(SAMSIM_A_S_ABS, 1) / LAY(SAMSIM_A_M, 1);
  }
}

// ---------------------------------------------------------------- output snapshot, mo_grotz.f90:340-398
template <class K>
__device__ RARE void output_point(Col &c, const Ctx &x, long long col, double time) {
  const samsim_config &g = x.p->cfg;
  if (c.Na > 1) GS(FREEBOARD) = func_freeboard<K>(c, x); else GS(FREEBOARD) = 0.0;
  if (CFG(grav_flag) == 2) {
    if (CL(grav_drain) == 0.0) CL(grav_temp) = 0.0; else CL(grav_temp) = CL(grav_temp) / CL(grav_drain);
    CL(grav_salt) = CL(grav_salt) / g.time_out;
    CL(grav_drain) = CL(grav_drain) / g.time_out;
  }
  {  // the vital signs are not carried in registers between output points: their slots of the scalar block are written here
    gdouble *sc = x.scal + c.col;
    const size_t nc = c.ncol;
    sc[(size_t)SAMSIM_S_ENERGY_STORED * nc] = c.energy_stored; sc[(size_t)SAMSIM_S_FRESHWATER * nc] = c.freshwater;
    sc[(size_t)SAMSIM_S_TOTAL_RESIST * nc] = c.total_resist; sc[(size_t)SAMSIM_S_THICKNESS * nc] = c.thickness;
    sc[(size_t)SAMSIM_S_BULK_SALIN * nc] = c.bulk_salin;
  }
  if (col >= x.out_col0 && col < x.out_col0 + x.out_ncols) {
    const size_t oc = (size_t)(col - x.out_col0), on = (size_t)x.out_ncols;
    for (int a = 0; a < SAMSIM_NARR; ++a) {
      if (a == SAMSIM_A_RAY) continue;  // captured before it was overwritten (see sweep_up_fused / column_step)
      for (int k = 1; k <= c.N; ++k) {
        double v = LAY(a, k);
        if (a == SAMSIM_A_S_BU && k <= c.Na) v = LAY(SAMSIM_A_S_ABS, k) / LAY(SAMSIM_A_M, k);  // refresh of mo_grotz.f90:333-335
        x.out_lay[((size_t)a * c.N + (k - 1)) * on + oc] = v;
      }
    }
    gdouble *o = x.out_scal + oc;
#define OUT(idx, v) o[(size_t)(idx) * on] = (v)
    OUT(SAMSIM_S_M_SNOW, CL(m_snow)); OUT(SAMSIM_S_H_ABS_SNOW, CL(H_abs_snow)); OUT(SAMSIM_S_S_ABS_SNOW, GS(S_ABS_SNOW));
    OUT(SAMSIM_S_THICK_SNOW, CL(thick_snow)); OUT(SAMSIM_S_PSI_S_SNOW, CL(psi_s_snow)); OUT(SAMSIM_S_PSI_L_SNOW, GS(PSI_L_SNOW));
    OUT(SAMSIM_S_PSI_G_SNOW, GS(PSI_G_SNOW)); OUT(SAMSIM_S_T_SNOW, CL(T_snow)); OUT(SAMSIM_S_PHI_S, GS(PHI_S));
    OUT(SAMSIM_S_T_TOP, CL(T_top)); OUT(SAMSIM_S_MELT_THICK, CL(melt_thick)); OUT(SAMSIM_S_T2M, CL(T2m));
    OUT(SAMSIM_S_LIQUID_PRECIP, CL(liquid_precip)); OUT(SAMSIM_S_SOLID_PRECIP, CL(solid_precip)); OUT(SAMSIM_S_FL_Q_BOTTOM, c.fl_q_bottom);
    OUT(SAMSIM_S_GRAV_DRAIN, CL(grav_drain)); OUT(SAMSIM_S_GRAV_SALT, CL(grav_salt)); OUT(SAMSIM_S_GRAV_TEMP, CL(grav_temp));
    OUT(SAMSIM_S_MELT_OUT1, GS(MELT_OUT1)); OUT(SAMSIM_S_MELT_OUT2, GS(MELT_OUT2)); OUT(SAMSIM_S_MELT_OUT3, GS(MELT_OUT3));
    OUT(SAMSIM_S_MELT_ERR, GS(MELT_ERR)); OUT(SAMSIM_S_FREEBOARD, GS(FREEBOARD)); OUT(SAMSIM_S_T_FREEZE, GS(T_FREEZE));
    OUT(SAMSIM_S_ALBEDO, CL(albedo)); OUT(SAMSIM_S_FL_SW, CL(fl_sw)); OUT(SAMSIM_S_FL_LW, CL(fl_lw));
    OUT(SAMSIM_S_MELT_THICK_SNOW, CL(melt_thick_snow)); OUT(SAMSIM_S_FL_Q_SNOW, CL(fl_Q_snow));
    OUT(SAMSIM_S_ENERGY_STORED, c.energy_stored); OUT(SAMSIM_S_FRESHWATER, c.freshwater); OUT(SAMSIM_S_TOTAL_RESIST, c.total_resist);
    OUT(SAMSIM_S_THICKNESS, c.thickness); OUT(SAMSIM_S_BULK_SALIN, c.bulk_salin);
    OUT(SAMSIM_S_FL_REST, (CFG(boundflux_flag) == 2 && (!K::general || CFG(atmoflux_flag) == 2)) ? CL(fl_lw) + 0.0 + 0.0
                                                                        : GSI(SAMSIM_S_FL_REST));
    OUT(SAMSIM_S_S_BU_BOTTOM, x.S_bu_bottom);
    OUT(SAMSIM_S_DT2M, GSI(SAMSIM_S_DT2M));
    OUT(SAMSIM_S_PRECIP_SCALE, GSI(SAMSIM_S_PRECIP_SCALE));
#undef OUT
    x.out_n_active[oc] = c.Na;
    if (HAS_BGC) {
      for (int t = 0; t < x.n_bgc; ++t) {
        for (int k = 1; k <= c.N; ++k) x.out_bgc[((size_t)t * c.N + (k - 1)) * on + oc] = BGC(t, k);
        x.out_bgc_bot[(size_t)t * on + oc] = BGC_BOT(t);
      }
    }
  }
  CL(grav_drain) = 0.0; CL(grav_salt) = 0.0; CL(grav_temp) = 0.0;
  GS(MELT_OUT1) = 0.0; GS(MELT_OUT2) = 0.0; GS(MELT_OUT3) = 0.0;
  (void)time;
}

// testcase specifics that only touch scalars, mo_grotz.f90:503-565
template <class K>
__device__ __forceinline__ void testcase_scalars(Col &c, const Ctx &x, const samsim_config &g, double time) {
  if (CFG(testcase) == 1) {  // sub_test1, mo_testcase_specifics.f90:42-89
    for (int n = 1; n <= 20; ++n) {
      if (fabs(time - (double)((float)(12 * n) * 3600.0f)) < (double)0.01f) { CL(T_top) = (n & 1) ? -10.0 : -5.0; break; }
    }
  } else if (K::general && CFG(testcase) == 3) {  // sub_test3, :172-187
    CL(liquid_precip) = 0.0;
    CL(solid_precip) = 0.15 / 86400.0 / 356.0;
  } else if (CFG(testcase) == 4 || CFG(testcase) == 7) {  // sub_test4, :197-202
    c.fl_q_bottom = -7.0 * sin(time * (2.0 * pi_f) / (86400.0 * 365.0)) + 7.0;
    if (K::sites) c.fl_q_bottom = c.fl_q_bottom + x.dflq;   // samsim_set_ocean: this column's offset (0 unless given)
  } else if (K::general && CFG(testcase) == 2) {  // sub_test2, :99-111
    if (time > 86400.0 * 25.0) CL(T2m) = 15.0;
    else if (time > 86400.0 * 15.0) CL(T2m) = 1.0;
  } else if (K::general && CFG(testcase) == 9) {  // sub_test9, :121-136
    if (time < 19.75 * 3600.0) CL(T2m) = 0.0;
    else if (time < 86400.0 * 3.0 + 2.25 * 3600.0) CL(T2m) = -15.0;
    else CL(T2m) = 1.0;
  } else if (K::general && CFG(testcase) == 34) {  // sub_test34, :146-162
    if (time < 2.0 * 3600.0) CL(T2m) = 0.0;
    else if (time < 86400.0 * 5.0) CL(T2m) = -15.0;
    else if (time < 86400.0 * 7.0) CL(T2m) = -5.0;
    else CL(T2m) = 1.0;
  } else if (K::general && CFG(testcase) == 6) {  // sub_test6, :211-232
    const double t[8] = {1714.0, 1676.0, 1525.0, 1483.0, 1385.0, 1349.0, 1160.0, 1100.0};
    for (int i = 0; i < 8; ++i) {
      if (time > t[i] * 60.0) { CL(T2m) = (i == 0) ? -19.0 : ((i & 1) ? -5.0 : -18.0); break; }
    }
  }
}

// ---------------------------------------------------------------- one time step, mo_grotz.f90:182-835
template <class K>
__device__ __forceinline__ void column_step(Col &c, Ctx &x, long long col, double time, int tc, bool out_step, bool next_out,
                                            bool last_step) {
  const samsim_config &g = x.p->cfg;
  const int N = c.N;

  if (out_step) {
    vital_signs<K>(c, x);  // mo_grotz.f90:192-223; only ever read by `output`
    // `output` prints the Rayleigh numbers of the PREVIOUS step's fl_grav_drain.  Normally the previous up sweep has
    // saved them before overwriting; on the first step after set_state the array itself still holds them.
    if ((c.flags & COLF_RESTART) && col >= x.out_col0 && col < x.out_col0 + x.out_ncols) {
      const size_t oc = (size_t)(col - x.out_col0), on = (size_t)x.out_ncols;
      for (int k = 1; k <= N; ++k) x.out_lay[((size_t)SAMSIM_A_RAY * N + (k - 1)) * on + oc] = LAY(SAMSIM_A_RAY, k);
    }
  }

  // forcing, mo_grotz.f90:229-241 (+ ensemble perturbation)
  if (CFG(atmoflux_flag) == 2) {
    if (time == time_input(tc)) {
      CL(T2m) = x.f_T2m[x.soff + tc - 1];
      CL(liquid_precip) = x.f_precip[x.soff + tc - 1];
    } else {
      const double temp = (time - time_input(tc - 1)) / (time_input(tc) - time_input(tc - 1));
      CL(T2m) = (1.0 - temp) * x.f_T2m[x.soff + tc - 2] + temp * x.f_T2m[x.soff + tc - 1];
      CL(liquid_precip) = (1.0 - temp) * x.f_precip[x.soff + tc - 2] + temp * x.f_precip[x.soff + tc - 1];
    }
    // the column's perturbation (samsim_set_forcing): two words of the scalar block, read where they are used
    CL(T2m) = CL(T2m) + GSI(SAMSIM_S_DT2M);
    CL(liquid_precip) = CL(liquid_precip) * GSI(SAMSIM_S_PRECIP_SCALE);
  }

  c.bgc_flood = 0.0; c.bgc_grav = false;
  snow_fall<K>(c, x);                  // mo_grotz.f90:251-265
  snow_block<K>(c, x);                 // mo_grotz.f90:273-292
  if (c.status) return;

  // first thermodynamic sweep, mo_grotz.f90:297-307 (+ Rayleigh numbers): only layer 1 is left to do unless the
  // column changed below layer 1 since the last up sweep
  c.ray_all = (c.flags & COLF_DIRTY) != 0;
  // (sparse Rayleigh rows need wave-uniform layer indices and every column of the wave in the sweep)
  const bool whole_wave = !wave_any(!c.ray_all);
  if (c.ray_all) { ST_COUNT(CT_DIRTY, 1); ST_COUNT(CT_L_DIRTY, (unsigned long long)__popcll(__ballot(1))); sweep_thermo_expulsion<K>(c, x, out_step, whole_wave); }
  else prologue_top_layer<K>(c, x);
  c.flags &= (COLF_REGULAR | COLF_FLUSHED);
  if (c.status) return;

  int Na = c.Na;
  const bool do_grav = (CFG(grav_flag) == 2 && Na > 1), do_beer = (CFG(boundflux_flag) == 2);
  // The fused down sweep covers the common step.  The reference's order is kept by the unfused path whenever something
  // sits between expulsion and gravity drainage: the output block, thin-snow coupling, a possible flooding event
  // (decided from SUM(psi_g*thick) AFTER expulsion_flux: m_snow above the solid-only buoyancy is treated as possible).
  const bool coupling = (CL(m_snow) > 0.0 && CL(thick_snow) < g.thick_min);
  const bool flood_possible = (CFG(flood_flag) > 1 && CL(m_snow) > 0.0 && CFG(freeboard_snow_flag) == 0 &&
                               CL(m_snow) > c.buoy_s * (rho_l - rho_s));
  // (a thin snow cover no longer needs the unfused order: the fused down sweep couples it to the top layer in place)
  // (a possible flooding no longer needs it either where flood_flag is 2 and no thin snow is coupled in the same step: see below)
  [[maybe_unused]] const bool fused_col = do_grav && !out_step && (c.step + 1 != 1) && (!flood_possible || (CFG(flood_flag) == 2 && !coupling)) &&
                     !(K::general && CFG(testcase) == 5 && c.step + 1 == 2) && !HAS_BGC &&
                     !(K::general && CFG(prescribe_flag) == 2)
                     && (c.flags & COLF_REGULAR) != 0   // the fused down sweep takes the thicknesses from the grid rule only
      ;
  // SAMSIM_PATH_MODE 2 (default): one path per wave.  A wave whose columns disagree runs both paths one after the other, each
  // with part of its lanes idle -- the normal state of a melt season, when some column of almost every wave has thin snow or a
  // flooded surface.  The unfused path is the general one (the reference's order, literally) and gives a column the same bits as
  // the fused one (tools/path_equiv.py compares the two on the GPU), so a wave in which any column needs it takes it for all.
  // SAMSIM_PATH_MODE 1 = always unfused (the build tools/path_equiv.py compares the product with).
#if SAMSIM_PATH_MODE == 1
  const bool fused = false;
#else
  const bool fused = !wave_any(!fused_col);
#endif

  ST_MARK(ST_PRO);
  ST_COUNT(CT_WAVESTEPS, 1);
  ST_COUNT(CT_LANES, (unsigned long long)__popcll(__ballot(1)));
  ST_COUNT(CT_L_COUPLING, (unsigned long long)__popcll(__ballot(coupling)));
  ST_COUNT(CT_L_FLOODP, (unsigned long long)__popcll(__ballot(flood_possible)));
  ST_COUNT(CT_L_IRREG, (unsigned long long)__popcll(__ballot((c.flags & COLF_REGULAR) == 0)));
  ST_COUNT(CT_L_UNFUSED, (unsigned long long)__popcll(__ballot(!fused_col)));
  bool surface_done = false;   // the fused down sweep has evaluated the surface balance already
  if (fused) {
    ST_COUNT(CT_FUSED, 1);
    // Flooding (mo_grotz.f90:428-445) sits between the brine expulsion and the gravity drainage.  Whether a column floods is
    // decided from the gas volume expulsion_flux leaves (freeboard) and what it moves depends on the top and bottom layers after the
    // expulsion -- both known only once the expulsion has gone through the whole column, while the fused sweep drains layer 1 long
    // before.  So a column whose snow load makes flooding possible first takes a DRY RUN of the expulsion (four loads per layer, no
    // store), floods its top and bottom layers and snow in registers exactly as flood() does on the arrays, and hands the fused sweep
    // the flooded top layer; the Rayleigh number of layer 1 is redone with the flooded thickness from the first sweep's scan.  One
    // read-only pass instead of the unfused order's three extra sweeps (and flood / refresh_ray_top no longer walk the column at
    // all): BASELINE cfg5, where every column floods in every step.
    if (flood_possible) {
      ExpelledEnds en;
      sweep_expulsion_transfer<K, true>(c, x, &en);
      THICK_RULE_INIT(tr);
      if (en.psi_gN > 0.0) {   // bottom-layer gas -> ocean water (mo_grotz.f90:405-410) precedes the flooding block
        const double temp2 = en.psi_gN * THICK_AT(tr, Na) * rho_l;
        en.mN = en.mN + temp2;
        en.SN = en.SN + temp2 * x.S_bu_bottom;
        en.HN = en.HN + temp2 * c_l * g.T_bottom;
      }
      const double buoy = c.buoy_s * (rho_l - rho_s) + en.buoy_g * rho_l;
      if (CL(m_snow) > buoy) {
        GS(FREEBOARD) = (buoy - CL(m_snow)) / rho_l;
        if (GS(FREEBOARD) < 0.0) {
          FloodEnds e;
          e.S1 = en.S1; e.H1 = en.H1; e.m1 = en.m1; e.th1 = LAY(SAMSIM_A_THICK, 1);
          e.SN = en.SN; e.HN = en.HN; e.mN = en.mN; e.TN = en.TN;
          const double th1_before = e.th1;
          flood_core<K>(c, x, SPEC(SP_FL_HP), SPEC(SP_FL_SALL), e);
          LAY(SAMSIM_A_THICK, 1) = e.th1;
          refresh_ray_top<K>(c, x, e.th1, en.psi_l1, en.S_br1);
          // (the scan rows have served: they carry the flooded top layer to the down sweep, see samsim_device.h)
          c.flags |= COLF_FLOODED;
          SPEC(SP_FLD_S1) = e.S1; SPEC(SP_FLD_H1) = e.H1; SPEC(SP_FLD_M1) = e.m1; SPEC(SP_FLD_TH1_BEFORE) = th1_before;
          if (e.deep) { c.flags |= COLF_FLOOD_DEEP; SPEC(SP_FL_HP) = e.incS; SPEC(SP_FL_SALL) = e.incH; }
        }
      }
    }
    // testcase specifics (mo_grotz.f90:503-565) and the radiation header only read time, snow scalars and psi_l(1),
    // none of which the down sweep changes, so they can run first
    testcase_scalars<K>(c, x, g, time);
    // with a thin snow cover somewhere in the wave the radiation header waits for the coupling inside the sweep (it reads T_snow)
    const bool late_rad = wave_any(coupling);
    double beer0 = 0.0;
    if (!late_rad) {
      beer0 = radiation_header<K>(c, x, time, tc);
      c.frad = 0.0;
    }
    // The volume fractions of layers >= 3 are only stored where something reads them (see sweep_down_fused): always through the
    // run-time-flag instantiation; with melt-water flushing (flush_flag 5 on the radiative surface) the sweep decides from the
    // finished top layer; without it (flush_flag 1) only the vital signs at the next output point and a get_state after the
    // launch read them
    bool store_default = true, decide_psi = false;
    if (K::fixed && K::boundflux_flag == 2 && K::flush_flag == 5) { store_default = next_out || last_step; decide_psi = true; }
    if (K::fixed && K::flush_flag == 1) store_default = next_out || last_step;
    // fl_rad(N_active) enters the conductive update of every layer (mo_heat_fluxes.f90:282-285), which the down sweep applies as
    // it goes: the Beer-law product over the layer thicknesses (a pass over one array) comes first
    if (do_beer && !late_rad) sweep_beer<K>(c, x, beer0);
    sweep_down_fused<K>(c, x, store_default, decide_psi, surface_done, coupling, late_rad, time, tc, do_beer);
    ST_MARK(ST_DFUSED);
    if (c.status) return;
  } else {
    ST_COUNT(CT_UNFUSED, 1);
    c.psi_full = true;
    down_unfused<K>(c, x, col, time, tc, out_step, coupling, do_grav, do_beer);
    ST_MARK(ST_DUNFUSED);
    if (c.status) return;
  }

  // tank: the water below holds what salt the ice does not, mo_grotz.f90:573-575
  if (K::general && CFG(tank_flag) == 2) {
    double sS = 0.0, sm = 0.0;
    for (int k = 1; k <= c.Na; ++k) { sS += LAY(SAMSIM_A_S_ABS, k); sm += LAY(SAMSIM_A_M, k); }
    x.S_bu_bottom = (g.S_total - sS) / (g.m_total - sm);
    if (HAS_BGC) {  // :575-577 (sic: the budget of tracer 1 sets the concentration of every tracer)
      double sb = 0.0;
      for (int k = 1; k <= c.Na; ++k) sb += BGC(0, k);
      const double v = (x.bgc_total0 - sb) / (g.m_total - sm);
      for (int t = 0; t < x.n_bgc; ++t) BGC_BOT(t) = v;
    }
  }

  // heat fluxes + second thermodynamic sweep (mo_grotz.f90:584-598) + first sweep of the next step for layers >= 2
  if (!surface_done) surface_flux<K>(c, x);
  ST_MARK(ST_SURF);
  sweep_up_fused<K>(c, x, col, next_out, next_out || last_step);
  ST_MARK(ST_UP);
  if (c.status) return;

  // snow thermodynamics again, mo_grotz.f90:603-625
  const double melt_thick_snow_old = CL(melt_thick_snow);
  snow_block<K>(c, x);
  if (c.status) return;
  CL(melt_thick_snow) = melt_thick_snow_old + CL(melt_thick_snow);

  // flushing preparations, mo_grotz.f90:632-664
  bool fb_valid = false;
  if (Na > 1 && CFG(flush_flag) > 2 && (CFG(boundflux_flag) == 2 || (K::general && CFG(boundflux_flag) == 3))) {
    // boundflux_flag 3 (:649-663) runs the same block on the air temperature instead of the surface temperature
    const bool lab = K::general && CFG(boundflux_flag) == 3;
    const double T_surf = lab ? CL(T2m) : CL(T_top);
    const double T_freeze = func_T_freeze(quot(LAY(SAMSIM_A_S_ABS, 1), LAY(SAMSIM_A_M, 1)), CFG(salt_flag), x.tf_c3);
    GS(T_FREEZE) = T_freeze;
    CL(melt_thick) = 0.0;
    const double psi_s1 = LAY(SAMSIM_A_PSI_S, 1);
    // the reference evaluates func_freeboard first (:636); its value is only read under the melt condition (:637)
    if (psi_s1 < psi_s_top_min || T_surf >= T_freeze) {
      if (!c.psi_full) refill_psi_rows<K>(c, x);
      ST_COUNT(CT_L_FREEBOARD, (unsigned long long)__popcll(__ballot(1)));
      GS(FREEBOARD) = func_freeboard<K>(c, x);
      fb_valid = true;
      if (GS(FREEBOARD) > 0.0000000000001) {
        double thick1 = LAY(SAMSIM_A_THICK, 1);
        const double thick1_in = thick1;
        double melt_thick = 0.0;
        sub_melt_thick(LAY(SAMSIM_A_PSI_L, 1), psi_s1, LAY(SAMSIM_A_PSI_G, 1), LAY(SAMSIM_A_T, 1), T_freeze, T_surf, CL(fl_Q1),
                       CL(thick_snow), g.dt, melt_thick, thick1, g.thick_min);
        CL(melt_thick) = melt_thick;
        if (lab) CL(melt_thick) = dmax(CL(melt_thick), 0.0);
        if (CL(thick_snow) >= g.thick_min / 100.0 && CL(melt_thick) > 0.00000000001 && CL(melt_thick_snow) == 0.0) {
          // sub_melt_snow, mo_functions.f90:443-474
          double H_abs = LAY(SAMSIM_A_H_ABS, 1), m = LAY(SAMSIM_A_M, 1);
          const double shift = 1.0 / dmax(GS(PSI_G_SNOW), 0.01) * CL(melt_thick);
          if (shift >= CL(thick_snow)) {
            CL(melt_thick) = CL(melt_thick) - CL(thick_snow) * GS(PSI_G_SNOW);
            H_abs = H_abs + CL(H_abs_snow);
            m = m + CL(m_snow);
            thick1 = thick1 + (1.0 - GS(PSI_G_SNOW)) * CL(thick_snow);
            CL(thick_snow) = 0.0; CL(m_snow) = 0.0; CL(H_abs_snow) = 0.0;
          } else {
            H_abs = H_abs + shift / CL(thick_snow) * CL(H_abs_snow);
            CL(H_abs_snow) = CL(H_abs_snow) - shift / CL(thick_snow) * CL(H_abs_snow);
            m = m + shift / CL(thick_snow) * CL(m_snow);
            CL(m_snow) = CL(m_snow) - shift / CL(thick_snow) * CL(m_snow);
            thick1 = thick1 + shift - CL(melt_thick);
            CL(thick_snow) = CL(thick_snow) - shift;
            CL(melt_thick) = 0.0;
          }
          LAY(SAMSIM_A_H_ABS, 1) = H_abs;
          LAY(SAMSIM_A_M, 1) = m;
          fb_valid = false;
        }
        if (thick1 != thick1_in) { LAY(SAMSIM_A_THICK, 1) = thick1; fb_valid = false; }
      }
    }
  }

  // flushing, mo_grotz.f90:670-737
  c.flags &= ~COLF_FLUSHED;
  // freeboard (:670) is only read when flush_flag 4 / flush3 can run (:704-716): N_active > 2 and melt water present
  const bool flush_possible = ((CFG(flush_flag) == 5 || (K::general && (CFG(flush_flag) == 4 || CFG(flush_flag) == 6))) && Na > 2 &&
                               CL(melt_thick) + CL(melt_thick_snow) > 0.000000000001);
  if (flush_possible && !c.psi_full) refill_psi_rows<K>(c, x);
  if (flush_possible && !fb_valid) GS(FREEBOARD) = func_freeboard<K>(c, x);
  // (the accumulators sit in the scalar block: x + 0 is x, so nothing is read or written while nothing melts)
  if (CL(melt_thick) != 0.0) GS(MELT_OUT1) = GS(MELT_OUT1) + CL(melt_thick);
  if (CL(melt_thick_snow) != 0.0) GS(MELT_OUT2) = GS(MELT_OUT2) + CL(melt_thick_snow);
  CL(melt_thick) = CL(melt_thick) + CL(melt_thick_snow);
  if (CL(melt_thick_snow) > 0.0) {
    const double mts = CL(melt_thick_snow);
    double H1 = LAY(SAMSIM_A_H_ABS, 1), S1 = LAY(SAMSIM_A_S_ABS, 1), m1 = LAY(SAMSIM_A_M, 1);
    H1 = H1 + mts * rho_l * c_l * CL(T_snow);
    S1 = S1 + mts * rho_l * S_br_clamped(x.salt, CL(T_snow), GS(S_ABS_SNOW) / CL(m_snow));
    m1 = m1 + mts * rho_l;
    LAY(SAMSIM_A_H_ABS, 1) = H1; LAY(SAMSIM_A_S_ABS, 1) = S1; LAY(SAMSIM_A_M, 1) = m1;
    LAY(SAMSIM_A_THICK, 1) = LAY(SAMSIM_A_THICK, 1) + mts;
    LAY(SAMSIM_A_S_BU, 1) = S1 / m1;
  }
  if (flush_possible && GS(FREEBOARD) > 0.001) {
    if (CL(melt_thick) > 0.000000000001) {
      if (K::general && CFG(flush_flag) == 4) {  // melt water simply leaves the top layer, mo_grotz.f90:704-713
        const double T1 = LAY(SAMSIM_A_T, 1), m1 = LAY(SAMSIM_A_M, 1);
        LAY(SAMSIM_A_H_ABS, 1) = LAY(SAMSIM_A_H_ABS, 1) - CL(melt_thick) * rho_l * c_l * T1;
        LAY(SAMSIM_A_S_ABS, 1) = LAY(SAMSIM_A_S_ABS, 1) * (1.0 - (CL(melt_thick) * rho_l) / m1);
        LAY(SAMSIM_A_THICK, 1) = LAY(SAMSIM_A_THICK, 1) - CL(melt_thick);
        LAY(SAMSIM_A_M, 1) = m1 - CL(melt_thick) * rho_l;
      } else if (K::general && CFG(flush_flag) == 6) {  // :729-733
        if (CL(thick_snow) < g.thick_0) {
          flush4<K>(c, x);
          c.flags |= COLF_DIRTY;
          if (c.status) return;
        }
      } else {
        if (CL(melt_thick_snow) > 0.0) GS(FREEBOARD) = func_freeboard<K>(c, x);  // layer 1 changed since the last evaluation (:717)
        ST_COUNT(CT_L_FLUSH3, (unsigned long long)__popcll(__ballot(1)));
        flush3<K>(c, x);
        c.flags |= COLF_DIRTY | COLF_FLUSHED;
        if (c.status) return;
      }
    }
  }

  // tracer advection with this step's brine fluxes, mo_grotz.f90:742-747
  if (HAS_BGC) bgc_advection<K>(c, x);

  // layer dynamics, mo_grotz.f90:755-795
  if (Na > 1) {
    const double th1 = LAY(SAMSIM_A_THICK, 1);
    if (LAY(SAMSIM_A_PHI, Na) > psi_s_min || LAY(SAMSIM_A_PHI, Na - 1) <= psi_s_min / 2.0 || th1 / g.thick_0 > 1.5 ||
        th1 / g.thick_0 < 0.5) {
      ST_COUNT(CT_L_REGRID, (unsigned long long)__popcll(__ballot(1)));
      layer_dynamics<K>(c, x);
      c.flags |= COLF_DIRTY | COLF_REGRID;
      if (c.status) return;
    }
    Na = c.Na;
    const int kn = (Na + 1 < N) ? Na + 1 : N;
    if (Na < N && LAY(SAMSIM_A_THICK, kn) == 0.0) {  // scrub, :772-783
      LAY(SAMSIM_A_T, Na + 1) = g.T_bottom;
      LAY(SAMSIM_A_S_BU, Na + 1) = x.S_bu_bottom;
      LAY(SAMSIM_A_PSI_L, Na + 1) = 1.0;
      LAY(SAMSIM_A_PSI_S, Na + 1) = 0.0;
      if (HAS_BGC) for (int t = 0; t < x.n_bgc; ++t) BGC(t, Na + 1) = 0.0;
    }
  } else {
    if (LAY(SAMSIM_A_PHI, 1) > psi_s_min) {
      layer_dynamics<K>(c, x);
      c.flags |= COLF_DIRTY | COLF_REGRID;
      if (c.status) return;
    }
  }

  ST_MARK(ST_POST);
  // health check, mo_grotz.f90:808-819 (negative S_abs is clamped element-wise at the next sweep)
  if (c.neg_psi) STOPC(1337, 0);
  if (c.Na == 1) {
    const double v = LAY(SAMSIM_A_S_ABS, 1);
    if (v < 0.0) LAY(SAMSIM_A_S_ABS, 1) = 0.0;
  }
}

#ifndef SAMSIM_WAVES
#define SAMSIM_WAVES 1
#endif
template <class K>
__global__ void __launch_bounds__(SAMSIM_BLOCK, SAMSIM_WAVES) samsim_step_kernel(const DevParams *__restrict__ pp, double *__restrict__ lay, double *__restrict__ scal,
                                                                        double *__restrict__ spec, int32_t *__restrict__ n_active,
                                                                        int32_t *__restrict__ status, int32_t *__restrict__ err_layer,
                                                                        long long *__restrict__ err_step, long long *__restrict__ work,
                                                                        int32_t *__restrict__ flags, const double *__restrict__ f_sw,
                                                                        const double *__restrict__ f_lw, const double *__restrict__ f_T2m,
                                                                        const double *__restrict__ f_precip, double *__restrict__ out_lay,
                                                                        double *__restrict__ out_scal, int32_t *__restrict__ out_n_active,
                                                                        double *__restrict__ bgc, double *__restrict__ bgc_bot,
                                                                        double *__restrict__ bfl, double *__restrict__ out_bgc,
                                                                        double *__restrict__ out_bgc_bot, const int32_t *__restrict__ site) {
  const DevParams &p = *pp;
  const long long blk = (long long)blockIdx.x + p.block0;
  const long long col = blk * blockDim.x + threadIdx.x;
  if (col >= p.ncol) return;
  Ctx x;
  x.p = pp;
  x.f_sw = (gcdouble *)f_sw; x.f_lw = (gcdouble *)f_lw; x.f_T2m = (gcdouble *)f_T2m; x.f_precip = (gcdouble *)f_precip;
  x.out_lay = (gdouble *)out_lay; x.out_scal = (gdouble *)out_scal; x.out_n_active = (gint32 *)out_n_active;
  x.scal = (gdouble *)scal;
  x.err_layer = (gint32 *)err_layer; x.err_step = (__attribute__((address_space(1))) long long *)err_step;
  x.bgc = (gdouble *)bgc; x.bgc_bot = (gdouble *)bgc_bot; x.bfl = (gdouble *)bfl;
  x.out_bgc = (gdouble *)out_bgc; x.out_bgc_bot = (gdouble *)out_bgc_bot;
  x.n_bgc = K::bgc ? p.n_bgc : 0; x.bgc_total0 = p.bgc_total0;
  x.soff = (K::sites && p.nsites > 1) ? site[col] * p.flen : 0;
  x.dflq = (K::sites && p.ocean_dflq) ? p.ocean_dflq[col] : 0.0;
  x.ocean_sbu = K::sites && p.ocean_sbu != nullptr;
  x.out_col0 = p.out_col0; x.out_ncols = p.out_ncols;
  x.p17 = p.p17; x.p14 = p.p14; x.tf_c3 = p.tf_c3;
  x.S_bu_bottom = (K::general && (K::fixed ? K::tank_flag : p.cfg.tank_flag) == 2) ? scal[(size_t)SAMSIM_S_S_BU_BOTTOM * (size_t)p.ncol + (size_t)col] : p.cfg.S_bu_bottom;
  if (K::sites && p.ocean_sbu && (K::fixed ? K::tank_flag : p.cfg.tank_flag) != 2) x.S_bu_bottom = p.ocean_sbu[col];
  x.rho_bottom = func_density(p.cfg.T_bottom, p.cfg.S_bu_bottom);
  if ((K::fixed ? K::salt_flag : p.cfg.salt_flag) == 1) x.salt = Salt{-18.7, -0.519, -0.00535, -21.4, -0.886, -0.0170};
  else x.salt = Salt{-17.6, -0.389, -0.00362, -17.6, -0.389, -0.00362};

#if SAMSIM_STAMPS
  __shared__ unsigned long long st_lds[48];
  if (threadIdx.x < 48) st_lds[threadIdx.x] = 0;
  __syncthreads();
  x.st.acc = st_lds;
  x.st.t0 = __builtin_amdgcn_s_memtime();
#endif
  Col c;
  c.lay = (gdouble *)((gchar *)lay + (size_t)blk * ((size_t)p.cfg.nlayer * DEV_ROWB) + 4096);
  c.col = (unsigned)col;
  c.coff = (unsigned)col * 8u;
  c.lcoff = threadIdx.x * 8u;
  c.rstride = (unsigned)p.ncol * 8u;
  c.astride = (size_t)p.cfg.nlayer * (size_t)p.ncol * 8u;
  c.ncol = (size_t)p.ncol;
  c.N = p.cfg.nlayer;
  c.Na = n_active[col];
  c.status = status[col];
  c.frad = 0.0; c.neg_psi = false; c.buoy_s = 0.0; c.buoy_g = 0.0; c.psi_l_top = 1.0;
  c.flags = flags[col];
  c.spec = (gdouble *)spec;
  const size_t nc = (size_t)p.ncol;
  double *sc = scal + col;
#define SLOAD(field, idx) c.field = sc[(size_t)(idx) * nc]
  SLOAD(fl_q_bottom, SAMSIM_S_FL_Q_BOTTOM);
#undef SLOAD
  // row flags of the Rayleigh-number array (Ctx::rflag): at the start of a launch every row is valid (the last up sweep of a
  // launch stores all rows, as does samsim_set_state's full first sweep)
  __shared__ unsigned long long lds_rflag[SAMSIM_MAX_NLAYER / 64];
  x.rflag = (volatile lu64 *)lds_rflag;
  for (int w = 0; w < SAMSIM_MAX_NLAYER / 64; ++w) x.rflag[w] = ~0ull;
  // the LDS-resident scalars (each lane reads and writes only its own words: no barrier needed)
  __shared__ double lds_scal[LD_NSLOT * SAMSIM_BLOCK];
  c.ld = (ldouble *)lds_scal + threadIdx.x;
#define LLOAD(field, idx) CL(field) = sc[(size_t)(idx) * nc]
  LLOAD(grav_drain, SAMSIM_S_GRAV_DRAIN); LLOAD(grav_salt, SAMSIM_S_GRAV_SALT); LLOAD(grav_temp, SAMSIM_S_GRAV_TEMP);
  LLOAD(T_top, SAMSIM_S_T_TOP); LLOAD(fl_Q_snow, SAMSIM_S_FL_Q_SNOW); LLOAD(melt_thick, SAMSIM_S_MELT_THICK);
  CL(fl_Q1) = 0.0;
  LLOAD(albedo, SAMSIM_S_ALBEDO); LLOAD(fl_sw, SAMSIM_S_FL_SW); LLOAD(fl_lw, SAMSIM_S_FL_LW);
  LLOAD(T2m, SAMSIM_S_T2M); LLOAD(liquid_precip, SAMSIM_S_LIQUID_PRECIP); LLOAD(solid_precip, SAMSIM_S_SOLID_PRECIP);
  LLOAD(m_snow, SAMSIM_S_M_SNOW); LLOAD(H_abs_snow, SAMSIM_S_H_ABS_SNOW); LLOAD(thick_snow, SAMSIM_S_THICK_SNOW);
  LLOAD(T_snow, SAMSIM_S_T_SNOW); LLOAD(psi_s_snow, SAMSIM_S_PSI_S_SNOW); LLOAD(melt_thick_snow, SAMSIM_S_MELT_THICK_SNOW);
#undef LLOAD

  // uniform clock (mo_data: time, i, n_time_out, time_counter) evolves identically in every lane
  double time = p.time0;
  long long step = p.step0;
  int n_time_out = p.n_time_out0, tc = p.time_counter0;
  long long work_done = 0;
  for (long long s = 0; s < p.nsteps; ++s) {
    if ((K::fixed ? K::atmoflux_flag : p.cfg.atmoflux_flag) == 2) {
      if (time > time_input(tc)) tc = tc + 1;
      if (tc > p.flen) tc = p.flen;
    }
    const bool out_step = (n_time_out == p.cfg.i_time_out) || (step + 1 == 1);
    if (out_step) n_time_out = 0; else n_time_out = n_time_out + 1;
    const bool next_out = (n_time_out == p.cfg.i_time_out);
    // `output` prints the Rayleigh numbers the step BEFORE the output step drained with (mo_grotz.f90:340-398 runs before
    // fl_grav_drain), i.e. those this step's up sweep writes when the step after next is an output step: then, before an
    // output step and at the end of a launch the up sweep stores every row
    const bool next2_out = ((next_out ? 0 : n_time_out + 1) == p.cfg.i_time_out);
    x.ray_rows_all = next_out || next2_out || (s + 1 == p.nsteps);
    ST_MARK(ST_HEAD);
    if (!c.status) {
      c.step = step;
      work_done += c.Na;
      // The lane's column index is the same in every step, so every address formed from it -- some forty scalar-block, hand-over
      // and top-layer words per step -- is invariant in this loop: left alone the optimiser computes all of them once, as 64-bit
      // per-lane addresses, keeps them for the whole launch and, having no registers for them, spills them at the start and
      // reloads one from scratch memory (= HBM) at every use.  Passing the index through an empty asm makes them values of the
      // step: each is formed where it is used (two or three vector instructions) and nothing is carried.
      // (Round 2 passed the stored index through an empty asm; the allocator then kept it in scratch memory and reloaded it at every
      // step.  Now the lane number is read off the hardware -- two instructions, no memory -- and the index rebuilt from it.)
      unsigned lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      asm volatile("" : "+v"(lane));
      c.lcoff = lane * 8u;
      c.col = (unsigned)(blk * SAMSIM_BLOCK) + lane;
      c.coff = c.col * 8u;
      const long long col_step = blk * SAMSIM_BLOCK + (long long)lane;
      column_step<K>(c, x, col_step, time, tc, out_step, next_out, s + 1 == p.nsteps);
    }
    time = time + p.cfg.dt;
    step = step + 1;
  }

  // (the column index and the scalar block's address are rebuilt from the lane number rather than carried through the time loop)
  unsigned lane_end = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  asm volatile("" : "+v"(lane_end));
  const long long col_end = blk * SAMSIM_BLOCK + (long long)lane_end;
  n_active[col_end] = c.Na;
  flags[col_end] = c.flags;
  status[col_end] = c.status;
  work[col_end] += work_done;
  sc = scal + col_end;
#define SSTORE(field, idx) sc[(size_t)(idx) * nc] = c.field
  SSTORE(fl_q_bottom, SAMSIM_S_FL_Q_BOTTOM);
#undef SSTORE
#define LSTORE(field, idx) sc[(size_t)(idx) * nc] = CL(field)
  LSTORE(grav_drain, SAMSIM_S_GRAV_DRAIN); LSTORE(grav_salt, SAMSIM_S_GRAV_SALT); LSTORE(grav_temp, SAMSIM_S_GRAV_TEMP);
  LSTORE(albedo, SAMSIM_S_ALBEDO); LSTORE(fl_sw, SAMSIM_S_FL_SW); LSTORE(fl_lw, SAMSIM_S_FL_LW);
  LSTORE(T2m, SAMSIM_S_T2M); LSTORE(liquid_precip, SAMSIM_S_LIQUID_PRECIP); LSTORE(solid_precip, SAMSIM_S_SOLID_PRECIP);
  LSTORE(T_top, SAMSIM_S_T_TOP); LSTORE(fl_Q_snow, SAMSIM_S_FL_Q_SNOW); LSTORE(melt_thick, SAMSIM_S_MELT_THICK);
  LSTORE(m_snow, SAMSIM_S_M_SNOW); LSTORE(H_abs_snow, SAMSIM_S_H_ABS_SNOW); LSTORE(thick_snow, SAMSIM_S_THICK_SNOW);
  LSTORE(T_snow, SAMSIM_S_T_SNOW); LSTORE(psi_s_snow, SAMSIM_S_PSI_S_SNOW); LSTORE(melt_thick_snow, SAMSIM_S_MELT_THICK_SNOW);
#undef LSTORE
  sc[(size_t)SAMSIM_S_S_BU_BOTTOM * nc] = x.S_bu_bottom;
  // fl_rest = fl_lw + sensible + latent (both zero) with the forcing tables, mo_heat_fluxes.f90:112
  if ((K::fixed ? K::boundflux_flag : p.cfg.boundflux_flag) == 2 && (!K::general || (K::fixed ? K::atmoflux_flag : p.cfg.atmoflux_flag) == 2)) sc[(size_t)SAMSIM_S_FL_REST * nc] = CL(fl_lw) + 0.0 + 0.0;
#if SAMSIM_STAMPS
  ST_MARK(ST_TAIL);
  __syncthreads();
  if (threadIdx.x < 48 && st_lds[threadIdx.x]) atomicAdd(&g_stamps[threadIdx.x], st_lds[threadIdx.x]);
#endif
}

}  // namespace

// d_params: device copy of the parameter block `hp` (host copy, used here for the direct pointer arguments)
extern "C" hipError_t samsim_launch_step(const DevParams *d_params, const DevParams *hp, long long grid, hipStream_t stream) {
  const int block = SAMSIM_BLOCK;
  const samsim_config &g = hp->cfg;
  // one instantiation per flag set; tracers (bgc_flag 2) and several forcing sets / oceans select their own
  const bool tracers = g.bgc_flag == 2, sites = hp->nsites > 1 || hp->ocean_dflq || hp->ocean_sbu;
  auto kernel = samsim_step_kernel<KGeneric>;
  if (!sites && flags_match<KSheba>(g)) kernel = tracers ? samsim_step_kernel<KShebaBgc> : samsim_step_kernel<KSheba>;
  else if (!tracers && sites && flags_match<KSheba>(g)) kernel = samsim_step_kernel<KShebaSites>;
  else if (!sites && flags_match<KPlate>(g)) kernel = tracers ? samsim_step_kernel<KPlateBgc> : samsim_step_kernel<KPlate>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), 0, stream, d_params, hp->lay, hp->scal, hp->spec,
                     hp->n_active, hp->status, hp->err_layer, hp->err_step, hp->work, hp->flags, hp->f_sw, hp->f_lw, hp->f_T2m,
                     hp->f_precip, hp->out_lay, hp->out_scal, hp->out_n_active, hp->bgc, hp->bgc_bot, hp->bfl, hp->out_bgc,
                     hp->out_bgc_bot, hp->site);
  return hipGetLastError();
}
