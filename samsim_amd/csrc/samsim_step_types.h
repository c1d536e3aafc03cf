// samsim_step_types.h -- what every part of the step kernel shares: the physical constants, the flag sets K the kernel is instantiated
// for, the column struct Col and the context Ctx, and the access macros (CL, GS / GSI, LAY / LAYU / LAYU_LD, SPEC, STOPC, BGC*,
// THICK_AT) with the wave votes.  The macros expect `c` = the lane's Col, `x` = the Ctx and, for CFG(), `g` = the run-time
// configuration in scope.  Part of the translation unit samsim_kernels.hip: expects samsim_device.h and samsim_probe.h.
#ifndef SAMSIM_STEP_TYPES_H
#define SAMSIM_STEP_TYPES_H

namespace {

// ---------------------------------------------------------------- constants, mo_parameters.f90:38-112
// `pi` and `grav` are default REAL (float32) in the reference (mo_parameters.f90:38-39)
constexpr double pi_f = (double)3.1415f;
constexpr double grav_f = (double)9.8061f;
constexpr double k_s = 2.2, k_l = 0.523;
constexpr double c_s = 2020.0, c_s_beta = 7.6973, c_l = 3400.0;
constexpr double rho_s = 920.0, rho_l = 1028.0, latent_heat = 333500.0, zeroK = 273.15;
// `0.8_wp*1e-3`: float32 literal factor (mo_parameters.f90:56,57,59)
constexpr double bbeta = 0.8 * (double)1e-3f;
constexpr double mu = 2.55 * (double)1e-3f;
constexpr double kappa_l = k_l / rho_l / c_l;
constexpr double sigma = 5.6704 * (double)1e-8f;
constexpr double psi_s_min = 0.05, neg_free = -0.05;
constexpr double x_grav = 0.000584, ray_crit = 4.89;
constexpr double para_flush_horiz = 1.0, para_flush_gamma = 0.9;
constexpr double psi_s_top_min = 0.40, ratio_flood = 1.50, ref_salinity = 34.0;
constexpr double rho_snow = 330.0, gas_snow_ice2 = 0.20;
constexpr double emissivity_ice = 0.95, emissivity_snow = 1.00, penetr = 0.30, extinc = 2.00;
constexpr double Turb_A = 0.1 * 0.05 * rho_l / 86400.0;
constexpr double Turb_B = 0.05;

// Every device function that takes the column struct or the context by reference is force-inlined: if one of them stayed
// out of line the struct would escape, its fields would live in scratch memory, the data pointers in it would lose their
// address space and the (uniform) config reads would become vector loads.  Measured: out-of-line rare paths by reference
// 101 ms, by value (struct copied in and out) 209 ms, everything inline 90 ms per launch of the default bench.
#define RARE __forceinline__

// ---------------------------------------------------------------- kernel instantiations
// The step kernel is instantiated per flag set K.  KGeneric reads every flag of samsim_config at run time and contains
// all supported parametrisations.  A fixed set (KSheba = testcase 4 as shipped = BASELINE cfg3 / cfg5, KPlate = testcase 1 =
// cfg1 / cfg2) turns the flags into compile-time constants: the branches of the other parametrisations, their registers
// and the flag loads disappear from the hot sweeps.  samsim_launch_step picks the instantiation whose flags equal the
// handle's configuration, KGeneric otherwise; the code paths taken are the same either way.
#define SAMSIM_FLAG_LIST(X)                                                                                               \
  X(atmoflux_flag) X(grav_flag) X(prescribe_flag) X(grav_heat_flag) X(flush_heat_flag) X(turb_flag) X(salt_flag)         \
  X(boundflux_flag) X(flush_flag) X(flood_flag) X(bottom_flag) X(precip_flag) X(harmonic_flag) X(tank_flag) X(albedo_flag) \
  X(lab_snow_flag) X(freeboard_snow_flag) X(snow_flush_flag) X(snow_precip_flag) X(testcase)
struct KGeneric {
  static constexpr bool fixed = false, general = true, sites = true, bgc = true;
#define X(f) [[maybe_unused]] static constexpr int f = 0;
  SAMSIM_FLAG_LIST(X)
#undef X
};
struct KSheba {  // init(4), mo_init.f90:1127-1207 on the defaults of :83-109
  static constexpr bool fixed = true, general = false, sites = false, bgc = false;
  static constexpr int atmoflux_flag = 2, grav_flag = 2, prescribe_flag = 1, grav_heat_flag = 1, flush_heat_flag = 2, turb_flag = 2,
                       salt_flag = 1, boundflux_flag = 2, flush_flag = 5, flood_flag = 2, bottom_flag = 1, precip_flag = 1,
                       harmonic_flag = 2, tank_flag = 1, albedo_flag = 2, lab_snow_flag = 0, freeboard_snow_flag = 0,
                       snow_flush_flag = 1, snow_precip_flag = 1, testcase = 4;
};
struct KShebaSites : KSheba {  // the same on several forcing sets (samsim_set_forcing_sites): a grid of columns
  static constexpr bool sites = true;
};
struct KPlate {  // init(1), mo_init.f90:865-945 (bgc off)
  static constexpr bool fixed = true, general = false, sites = false, bgc = false;
  static constexpr int atmoflux_flag = 1, grav_flag = 2, prescribe_flag = 1, grav_heat_flag = 1, flush_heat_flag = 1, turb_flag = 1,
                       salt_flag = 2, boundflux_flag = 1, flush_flag = 1, flood_flag = 2, bottom_flag = 1, precip_flag = 0,
                       harmonic_flag = 2, tank_flag = 1, albedo_flag = 2, lab_snow_flag = 0, freeboard_snow_flag = 0,
                       snow_flush_flag = 1, snow_precip_flag = 1, testcase = 1;
};
// the same flag sets carrying passive tracers (bgc_flag 2: testcase 1 as init ships it; a SHEBA ensemble with tracers)
struct KPlateBgc : KPlate {
  static constexpr bool bgc = true;
};
struct KShebaBgc : KSheba {
  static constexpr bool bgc = true;
};
template <class K>
bool flags_match(const samsim_config &g) {
#define X(f) if (g.f != K::f) return false;
  SAMSIM_FLAG_LIST(X)
#undef X
  return true;
}
// flag read inside a function template over K with `g` = the run-time configuration in scope
#define CFG(f) (K::fixed ? K::f : g.f)

// Device data pointers carry the global address space in their type: an access through them is a global_load / global_store
// even where the pointer itself has been through memory (a struct passed to a non-inlined function), where the compiler
// would otherwise have to assume a generic (flat) address.
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) const double gcdouble;
typedef __attribute__((address_space(1))) int32_t gint32;
typedef __attribute__((address_space(1))) char gchar;
typedef __attribute__((address_space(3))) double ldouble;
typedef __attribute__((address_space(3))) unsigned long long lu64;
// LDS-resident per-column scalars: slot s of lane l is word s*SAMSIM_BLOCK + l of the block's array
enum lds_slot {
  LD_grav_drain = 0, LD_grav_salt, LD_grav_temp,
  LD_albedo, LD_fl_sw, LD_fl_lw, LD_T2m, LD_liquid_precip, LD_solid_precip,
  LD_T_top, LD_fl_Q_snow, LD_melt_thick,   // state that only the code between the sweeps touches
  LD_fl_Q1,                                // fl_Q(1) of this step (surface balance -> top-layer block, melt film): not a slot of the scalar block
  // the snow cover: read and written before, between and after the two sweeps of every step, never inside them
  LD_m_snow, LD_H_abs_snow, LD_thick_snow, LD_T_snow, LD_psi_s_snow, LD_melt_thick_snow,
  LD_NSLOT
};
#define CL(f) c.ld[LD_##f * SAMSIM_BLOCK]
// Per-column scalars that the common step does not touch (melt-water accumulators, freeboard, T_freeze, the snow's salt and the
// volume fractions only snow_thermo itself reads) are read and written IN PLACE in the scalar block: GS(FREEBOARD) = slot
// SAMSIM_S_FREEBOARD of this lane's column.  19 LDS slots are what 16 one-wave workgroups per CU leave room for.
// (scalar base + 32-bit byte offset, like LAY: slot * bytes-per-row + this lane's column; 38 slots of at most 4 GiB / nlayer)
#define GSI(idx) (*(gdouble *)((gchar *)x.scal + (size_t)(unsigned)((unsigned)(idx) * c.rstride + c.coff)))
#define GS(IDX) GSI(SAMSIM_S_##IDX)

struct Salt {  // liquidus polynomial (func_S_br) and its derivative (func_ddT_S_br), mo_thermo_functions.f90:308-414
  double c2, c3, c4, d2, d3, d4;
};

struct Col {
  gdouble *lay;  // UNIFORM: 4096 bytes into the wave's 64-column block of the layer arrays 
  unsigned col; // this lane's column
  unsigned coff;     // col * 8: byte offset of the column inside a row of the scalar / hand-over blocks
  unsigned lcoff;    // lane * 8: byte offset of the column inside a row of its 64-column block
  unsigned rstride;  // UNIFORM ncol * 8: bytes per row
  size_t astride;    // UNIFORM nlayer * ncol * 8: bytes per layer array.  Nothing reads it; it stays because the built kernel is not the
                     // same bytes without it (docs/HISTORY.md, Source split)
  size_t ncol;
  int N;
  int Na;       // N_active
  int flags;          // COLF_*
  gdouble *spec;       // UNIFORM base of the [DEV_NSPEC][ncol] hand-over block
  int status;      // 0 or the reference's STOP code; where and when it stopped goes straight to the err_layer / err_step arrays
  long long step;  // completed steps; i = step + 1
  // per-column scalars (enum samsim_scalar)
  double fl_q_bottom;
  // The per-column scalars that every step touches live in LDS for the whole launch (CL(name), enum lds_slot: one 8-byte word per
  // lane and slot, no bank conflicts): the gravity-drainage accumulators (grav_*), the forcing of the step (T2m, precipitation,
  // albedo, short- and long-wave flux), the surface state between the sweeps (T_top, fl_Q_snow, melt_thick, fl_Q(1)) and the snow
  // cover.  Kept in registers they would be live across both layer loops of every step, where the allocator has no room for them:
  // they were spilled to scratch memory, i.e. to HBM, around every sweep.  What the common step does not touch -- melt_out*,
  // melt_err, freeboard, T_freeze, the ensemble perturbation -- stays in the scalar block (GS() above).
  ldouble *ld;
  double energy_stored, freshwater, total_resist, thickness, bulk_salin;  // vital signs: live at output points only
  // per-step temporaries that cross sweeps
  double frad;       // fl_rad(N_active)
  double flq2;       // fl_Q(2), handed from the down sweep (which applies the conductive update of layers >= 2) to the top-layer block
  double esum;       // SUM(H_abs before - H_abs after the conductive update) over layers >= 2 (energy assert, mo_heat_fluxes.f90:265-310)
  bool neg_psi;      // MINVAL(psi_s(1:N_active)) of this step's Expulsion is negative (health check at the end of the step)
  double buoy_s;     // SUM(psi_s*thick) over the active layers (from S1)
  double buoy_g;     // SUM(psi_g*thick) after expulsion_flux (from P2)
  double psi_l_top;  // psi_l(1) of this step's Expulsion (the albedo reads it before the down sweep stores the psi arrays)
  double bgc_flood;  // flood_brine of this step (fl_brine_bgc(N_active,1), mo_flood.f90:140-143)
  bool bgc_grav;     // fl_grav_drain ran this step (its fl_brine_bgc assignment, mo_grav_drain.f90:179)
  bool psi_full;     // this step's down sweep stored psi_s / psi_l / psi_g for every layer (not only for layer 1)
  bool ray_all;      // this step's first sweep was the full one (sweep_thermo_expulsion): every Rayleigh number of this column is in the array
};

// RARE_CHUNK: the sweeps of the melt season (flushing, freeboard, the unfused order of a step with thin snow or possible flooding)
// walk a column with a per-lane trip count and little arithmetic per layer; with a row requested where it is used every
// iteration waits a full memory latency (2 us under load against 0.1-0.5 us of work).  They request RARE_CHUNK rows at a time
// -- unconditionally, from a clamped row beyond the column's last layer -- and then work through them in order.
#ifndef RARE_CHUNK
#define RARE_CHUNK 8
#endif
// SAMSIM_PATH_MODE 2 (the product): one order of the step per wave, see column_step; 1 = always the unfused order (the checker
// build of tools/path_equiv.py, which shows on the GPU that the two orders give a column the same bits)
#ifndef SAMSIM_PATH_MODE
#define SAMSIM_PATH_MODE 2
#endif

static_assert(SAMSIM_BLOCK == 64, "the blocked layer layout, launch() and DEV_LAY_INDEX are written for one 64-lane wave per column block");
// Row (a, k) of the layer block starts at a wave-uniform address whenever k is uniform (all top-down loops, and the
// bottom-up loops that run from the wave maximum of N_active); the lane only adds its 32-bit column offset, which lets
// the compiler use scalar-base addressing (global_load ... v_off, s[base]) instead of a 64-bit VGPR address per array.
// Address of element (a, k): one 32-bit offset register per row serves all arrays of the row (a 64-bit per-lane address for every
// array costs two registers each and 64-bit vector arithmetic per access).
// Blocked layout (samsim_device.h): c.lay points 4096 bytes into the wave's own column block, so that array a of layer row k is at
// c.lay + (k-1)*DEV_ROWB + (a*512 - 4096) + lane*8: sixteen arrays within the signed 13-bit immediate of one row address.
// LAY takes any k (one 32-bit offset register per row, the lane's part included); LAYU is for a wave-uniform k: the row address is
// scalar arithmetic and the vector offset is the lane's constant c.lcoff.
#define LAY(a, k) (*(gdouble *)((gchar *)c.lay + (size_t)(unsigned)(((unsigned)(k) - 1u) * (unsigned)DEV_ROWB + c.lcoff) + (ptrdiff_t)((int)(a) * 512 - 4096)))
#define LAYU(a, k) (*(gdouble *)((gchar *)c.lay + (size_t)(((unsigned)(k) - 1u) * (unsigned)DEV_ROWB) + (size_t)c.lcoff + (ptrdiff_t)((int)(a) * 512 - 4096)))
// The row loads of the two fused sweeps are streaming accesses: a row is read once per sweep and not again before gigabytes of
// other rows have passed.  With the non-temporal hint (`global_load ... nt`) they do not displace what IS read again soon -- the
// per-column words of a step, the wave's scratch lines, the rows the down sweep has just written near the column's bottom -- from
// the L2: 760 -> 736 ms per 500 steps.  (The same hint on the sweeps' stores costs half of that again: 749 ms.)
#define LAYU_LD(a, k) __builtin_nontemporal_load(&LAYU(a, k))
// hand-over block [DEV_NSPEC][ncol]: scalar base + 32-bit byte offset, like GSI (samsim_create bounds ncol for both)
#define SPEC(i) (*(gdouble *)((gchar *)c.spec + (size_t)(unsigned)((unsigned)(i) * c.rstride + c.coff)))
#define STOPC(code, layer)            \
  do {                                \
    if (!c.status) {                  \
      c.status = (code);              \
      x.err_step[c.col] = c.step + 1; \
      x.err_layer[c.col] = (layer);   \
    }                                 \
    return;                           \
  } while (0)

// Wave-uniform maximum of a per-lane integer over the lanes that are EXECUTING the call (the sweeps are called under
// divergent conditions -- fused / unfused path, frozen columns -- so a shuffle butterfly would read stale registers of
// inactive lanes).  Layer loops run k over 1..wave_max (or wave_max..1) with the body predicated on k <= N_active: k then
// lives in an SGPR and every row address (array, k) is scalar arithmetic; a lane with fewer layers idles exactly as long
// as it would have waited for its wave.
__device__ __forceinline__ int wave_max(int v) {
  unsigned long long mask = __ballot(1);
  int m = 0;
  while (mask) {
    const int lane = __ffsll((long long)mask) - 1;
    const int val = __builtin_amdgcn_readlane(v, lane);
    m = val > m ? val : m;
    mask &= mask - 1;
  }
  return m;
}

// does any active lane of the wave hold the predicate?  (the ballot of a comparison result IS its lane mask: one scalar compare,
// where __ballot() first turns the predicate into an integer per lane and compares that again)
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }

struct Ctx {
  const DevParams *p;
  // The data pointers are taken from DIRECT kernel arguments, not from the parameter block: only then does the compiler
  // know they are global-memory pointers (global_load/global_store with scalar base) instead of generic flat ones.
  gcdouble *f_sw, *f_lw, *f_T2m, *f_precip;
  gdouble *out_lay, *out_scal;
  gdouble *scal;  // [SAMSIM_NSCAL][ncol] scalar block: slots that are not carried in registers (fl_rest) are read / written in place
  gint32 *out_n_active;
  gint32 *err_layer;                                   // [ncol] layer and step of a column's STOP (written once, when it stops)
  __attribute__((address_space(1))) long long *err_step;
  long long out_col0, out_ncols;
  Salt salt;
  double p17, p14, tf_c3;
  // salinity of the water below the ice: cfg.S_bu_bottom (uniform), or the column's tank budget with tank_flag 2 (mo_grotz.f90:573)
  double S_bu_bottom;
  double rho_bottom;   // func_density(T_bottom, S_bu_bottom) of sub_turb_flux, evaluated once per launch where the water below is uniform
  // passive tracers (bgc_flag 2, KGeneric only): amounts [n_bgc][N][ncol], concentration below the ice [n_bgc][ncol], this
  // step's brine fluxes [BFL_NROW][N][ncol], snapshot of the output window
  int soff;   // start of this column's forcing set in the tables (0 unless samsim_set_forcing_sites gave several)
  // the water below a grid of columns (samsim_set_ocean, K::sites instantiations): offset added to the oceanic heat flux the
  // testcase sets every step (sub_test4), and whether S_bu_bottom above is this column's own value
  double dflq;
  bool ocean_sbu;
  gdouble *bgc, *bgc_bot, *bfl, *out_bgc, *out_bgc_bot;
  int n_bgc;
  double bgc_total0;
  // Which rows of the Rayleigh-number array the last up sweep wrote (bit k-1 of word (k-1)/64 = row k), per wave, in LDS.
  // Gravity drainage only reads ray(k) where it exceeds ray_crit (mo_grav_drain.f90:144), which in winter holds in two or three
  // of 80 layers: the up sweep stores a row only when some column of the wave is above the threshold in that layer (or when the
  // whole array is wanted: output, end of a launch), the down sweeps load only those rows and take 0 elsewhere.
  // The words pass data between the lanes of the wave (the wave's first lane ORs a bit in, every lane reads it in the next step's
  // down sweep): volatile, so that every access is an LDS instruction in program order -- one wave issues its LDS instructions
  // in order and the LDS serves them in order -- and a wave barrier where the phases change (zeroing -> setting -> reading).
  volatile lu64 *rflag;
  bool ray_rows_all;   // this up sweep stores every row

#if SAMSIM_STAMPS
  mutable Stamps st;
#endif
};
#define BGC(t, k) (x.bgc + ((size_t)(t) * (size_t)c.N + (size_t)((k) - 1)) * c.ncol)[c.col]
#define BGC_BOT(t) (x.bgc_bot + (size_t)(t) * c.ncol)[c.col]
#define BFL(r, k) (x.bfl + ((size_t)(r) * (size_t)c.N + (size_t)((k) - 1)) * c.ncol)[c.col]
// tracers exist only in the run-time-flag instantiation; in the fixed ones the test folds to false
#define HAS_BGC (K::bgc && x.n_bgc > 0)

// thick(k), k >= 2, of a column that follows the grid rule; th_mid = thick(N_top+1)
__device__ __forceinline__ double thick_by_rule(int k, int n_top, int n_middle, double th_mid, double thick_0) {
  return (k > n_top && k <= n_top + n_middle) ? th_mid : thick_0;
}

// The thickness of layer kk for the sweeps of the melt season: from the grid rule where the column follows it, else from the array
struct ThickRule { bool reg; int n_top, n_middle; double th_mid, thick_0; };
#define THICK_RULE_INIT(tr)                                                                                   \
  ThickRule tr;                                                                                               \
  tr.reg = (c.flags & COLF_REGULAR) != 0; tr.n_top = x.p->cfg.n_top; tr.n_middle = x.p->cfg.n_middle; \
  tr.thick_0 = x.p->cfg.thick_0; tr.th_mid = LAY(SAMSIM_A_THICK, tr.n_top + 1)
#define THICK_AT(tr, kk) ((tr.reg && (kk) >= 2) ? thick_by_rule(kk, tr.n_top, tr.n_middle, tr.th_mid, tr.thick_0) : LAY(SAMSIM_A_THICK, kk))

// Does row k of the Rayleigh-number array hold this column's current value?  Row 1 is written by the first sweep of every step
// (prologue_top_layer / sweep_thermo_expulsion), the other rows by the last up sweep where flagged (Ctx::rflag), and all of them by
// this step's full first sweep.  A row that was not written held no value above ray_crit in any column of the wave.
__device__ __forceinline__ bool ray_row_valid(const Col &c, const Ctx &x, int k) {
  return k == 1 || c.ray_all || ((x.rflag[(k - 1) >> 6] >> ((k - 1) & 63)) & 1ull) != 0ull;
}

}  // namespace

#endif
