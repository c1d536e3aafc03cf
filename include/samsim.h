/*
 * samsim.h -- C-ABI of the MI355X-native batched sea-ice column solver (libsamsim_hip.so).
 *
 * Drop-in boundary for ONE path of pgriewank/SAMSIM V2.0: the body of the time loop
 * mo_grotz.f90:182-835 (the per-timestep 1-D thermodynamic + brine-transport + regrid update of a
 * column), evaluated for `ncol` independent columns at once.  The reference has no FFI: its physics
 * are Fortran module procedures called from `grotz` on the `mo_data` module globals.  Each entry point
 * below cites the reference interface it replaces; INTEGRATION.md shows the iso_c_binding stub a
 * maintainer adds on the Fortran side.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a HOST pointer; the library owns device memory.
 *   - layer arrays are struct-of-arrays, column fastest:  a[(k-1)*ncol + c], k = 1..nlayer (Fortran
 *     layer index), c = 0..ncol-1.  Scalars: s[idx*ncol + c].
 *   - all arithmetic is IEEE float64 (`wp = SELECTED_REAL_KIND(12,307)`, mo_parameters.f90:33).
 *   - return value: 0 = ok, negative = API error (samsim_strerror).  Physics failures (the reference's
 *     `STOP n`) never abort the process: they are recorded per column in
 *     status[] and the column is frozen.
 *   - flags and time are uniform over columns (they are scalars of mo_data in the reference), so time,
 *     step index and the forcing-table cursor live in the handle, not per column.
 */
#ifndef SAMSIM_H
#define SAMSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAMSIM_ABI_VERSION 6
#define SAMSIM_MAX_NLAYER 1024

/* -------- configuration: every flag of mo_data.f90:136-155 plus the scalars mo_init sets -------- */
typedef struct samsim_config {
  int32_t struct_size;          /* = sizeof(samsim_config); ABI check                                */
  int32_t testcase;             /* selects the time-dependent forcing of mo_grotz.f90:503-565:
                                   1 sub_test1 (T_top toggles), 2/6/9/34 sub_test2/6/9/34 (T2m schedule of the
                                   tank experiments), 3 sub_test3 (snow fall), 4/7 sub_test4 (fl_q_bottom),
                                   5 (S_abs reset at step 2); 8, 44, 45, 99, 101-105, 111 (lab tables, imposed
                                   snow) are refused; any other value (0, 33, 50): none               */
  int32_t nlayer, n_top, n_middle, n_bottom;          /* mo_data.f90:62-65                           */
  int32_t atmoflux_flag;        /* 1 Notz climatology, 2 forcing tables, 3 fixed fl_sw / fl_rest     */
  int32_t grav_flag;            /* 1 none, 2 Rayleigh-number gravity drainage, 3 simple              */
  int32_t prescribe_flag;       /* 1 none, 2 prescribed salinity profile (mo_grotz.f90:482-497)      */
  int32_t grav_heat_flag;       /* 1, 2                                                              */
  int32_t flush_heat_flag;      /* 1, 2                                                              */
  int32_t turb_flag;            /* 1, 2                                                              */
  int32_t salt_flag;            /* 1 sea salt, 2 NaCl                                                */
  int32_t boundflux_flag;       /* 1 cooling plate, 2 radiative balance, 3 lab air temperature T2m   */
  int32_t flush_flag;           /* 1 none, 4 melt water removed, 5 flush3, 6 flush4                  */
  int32_t flood_flag;           /* 1 none, 2 flood, 3 flood_simple                                   */
  int32_t bottom_flag;          /* 1, 2                                                              */
  int32_t debug_flag;           /* 1 (ignored)                                                       */
  int32_t precip_flag;          /* 0, 1                                                              */
  int32_t harmonic_flag;        /* 1, 2                                                              */
  int32_t tank_flag;            /* 1 ocean of fixed salinity, 2 tank: S_bu_bottom from the salt budget */
  int32_t albedo_flag;          /* 1, 2                                                              */
  int32_t lab_snow_flag;        /* 0 (1, snow in the lab with boundflux_flag 3, not supported)       */
  int32_t freeboard_snow_flag;  /* 0, 1                                                              */
  int32_t snow_flush_flag;      /* 0, 1                                                              */
  int32_t snow_precip_flag;     /* (echo only)                                                       */
  int32_t bgc_flag;             /* 1 none, 2 passive tracers advected with the brine (samsim_set_tracers)  */
  int32_t i_time_out;           /* INT(time_out/dt), mo_init.f90:2001                                */
  double  dt, thick_0, thick_min;            /* thick_min = thick_0/2, mo_init.f90:1994              */
  double  T_bottom, S_bu_bottom;
  double  k_snow_flush, max_flux_plate;      /* mo_parameters.f90:107,110                            */
  double  time_out, time_total;              /* echo / grav_* normalisation mo_grotz.f90:355-356     */
  double  alpha_flux_instable, alpha_flux_stable;   /* boundflux_flag 3, mo_heat_fluxes.f90:208-214   */
  double  m_total, S_total;                  /* tank_flag 2: water and salt in the tank, mo_init.f90:996-997 */
} samsim_config;

/* -------- per-column scalar slots (state + accumulators + output-only), s[idx*ncol + c] -------- */
enum samsim_scalar {
  SAMSIM_S_M_SNOW = 0, SAMSIM_S_H_ABS_SNOW, SAMSIM_S_S_ABS_SNOW, SAMSIM_S_THICK_SNOW,
  SAMSIM_S_PSI_S_SNOW, SAMSIM_S_PSI_L_SNOW, SAMSIM_S_PSI_G_SNOW, SAMSIM_S_T_SNOW, SAMSIM_S_PHI_S,
  SAMSIM_S_T_TOP, SAMSIM_S_MELT_THICK, SAMSIM_S_T2M, SAMSIM_S_LIQUID_PRECIP, SAMSIM_S_SOLID_PRECIP,
  SAMSIM_S_FL_Q_BOTTOM,
  SAMSIM_S_GRAV_DRAIN, SAMSIM_S_GRAV_SALT, SAMSIM_S_GRAV_TEMP,            /* accumulators            */
  SAMSIM_S_MELT_OUT1, SAMSIM_S_MELT_OUT2, SAMSIM_S_MELT_OUT3, SAMSIM_S_MELT_ERR,
  SAMSIM_S_FREEBOARD, SAMSIM_S_T_FREEZE, SAMSIM_S_ALBEDO, SAMSIM_S_FL_SW, SAMSIM_S_FL_LW,
  SAMSIM_S_MELT_THICK_SNOW, SAMSIM_S_FL_Q_SNOW,
  SAMSIM_S_ENERGY_STORED, SAMSIM_S_FRESHWATER, SAMSIM_S_TOTAL_RESIST,     /* vital signs             */
  SAMSIM_S_THICKNESS, SAMSIM_S_BULK_SALIN,
  SAMSIM_S_FL_REST,             /* bundled long-wave + turbulent flux (constant for atmoflux_flag 3) */
  SAMSIM_S_S_BU_BOTTOM,         /* salinity of the water below: evolves with tank_flag 2 (mo_grotz.f90:573-575);
                                   with tank_flag 1 an echo of cfg.S_bu_bottom that set_state ignores      */
  SAMSIM_S_DT2M, SAMSIM_S_PRECIP_SCALE,                                   /* ensemble perturbation   */
  SAMSIM_NSCAL
};

/* -------- per-column layer arrays, a[idx][k][c] -------- */
enum samsim_layer_array {
  SAMSIM_A_H_ABS = 0, SAMSIM_A_S_ABS, SAMSIM_A_M, SAMSIM_A_THICK,         /* prognostic (mo_data.f90:34-45) */
  SAMSIM_A_T, SAMSIM_A_PHI, SAMSIM_A_PSI_S, SAMSIM_A_PSI_L, SAMSIM_A_PSI_G,
  SAMSIM_A_S_BU, SAMSIM_A_S_BR, SAMSIM_A_RAY, SAMSIM_A_PERM,
  SAMSIM_A_FLUSH_V, SAMSIM_A_FLUSH_H,
  SAMSIM_NARR
};
#define SAMSIM_NPROG 4

/* Whole-column state as SoA blocks; used for initialisation, checkpoint/restart and parity tests.
 * (mo_data.f90:34-133; the reference keeps it in module globals allocated by sub_allocate,
 * mo_init.f90:2040-2090.) */
typedef struct samsim_state_soa {
  int64_t  ncol;
  int32_t  nlayer;
  int32_t  narr;      /* number of layer arrays present in `lay`: SAMSIM_NPROG (prognostic only; the carried
                         diagnostics are then initialised as mo_init.f90:1982-1990 does) or SAMSIM_NARR */
  double  *lay;       /* [narr][nlayer][ncol]                                                        */
  double  *scal;      /* [SAMSIM_NSCAL][ncol]                                                        */
  int32_t *n_active;  /* [ncol]                                                                      */
} samsim_state_soa;

/* uniform clock of the ensemble (mo_data: time, i, n_time_out, time_counter) */
typedef struct samsim_clock {
  double  time;          /* model time [s]                                                           */
  int64_t step;          /* number of completed time steps (= i-1 of mo_grotz.f90:182)               */
  int32_t n_time_out;    /* mo_grotz.f90:340,395-398                                                 */
  int32_t time_counter;  /* 1-based cursor into the 3-hourly tables, mo_grotz.f90:229-241            */
  int64_t n_outputs;     /* number of output points passed so far                                    */
} samsim_clock;

/* Snapshot taken at the reference's output point (mo_grotz.f90:340-398) for the column window
 * [col0, col0+ncols) chosen with samsim_set_output_window: exactly what mo_output.f90:129-144 writes. */
typedef struct samsim_output_soa {
  int64_t  ncols;
  int32_t  nlayer;
  int32_t  reserved;
  double  *lay;       /* [SAMSIM_NARR][nlayer][ncols]  (T, psi_s, psi_l, psi_g, S_bu, thick, ray, perm, flush_v, flush_h ...) */
  double  *scal;      /* [SAMSIM_NSCAL][ncols]         (freeboard, snow, vital signs, grav_*, T2m, T_top, melt_out) */
  int32_t *n_active;  /* [ncols]                                                                     */
  double   time;      /* model time of the snapshot                                                  */
  int64_t  step;      /* step index i (1-based) of the snapshot                                      */
} samsim_output_soa;

typedef struct samsim_handle samsim_handle;

/* sub_allocate (mo_init.f90:2040-2090) + the flag/scalar part of init (mo_init.f90:83-132, 1981-2031).
 * device: HIP device ordinal.  ncol columns of nlayer layers are allocated on it.  One handle holds at most
 * SAMSIM_MAX_NCOL columns (its [SAMSIM_NSCAL][ncol] scalar block is addressed with 32-bit byte offsets: SAMSIM_ERR_ARG
 * beyond), whatever nlayer is; larger ensembles take several handles (column ranges), which is also how they are spread
 * over GPUs. */
#define SAMSIM_MAX_NCOL ((int64_t)(((1ull << 32) - 1) / (8ull * SAMSIM_NSCAL)))
int samsim_create(const samsim_config *cfg, int64_t ncol, int32_t device, samsim_handle **h);

/* sub_input (mo_functions.f90:304-327): 3-hourly tables, time_input(k) = (k-1)*10800 s.
 * dT2m_col / precip_scale_col ([ncol] or NULL) perturb the ensemble: T2m_c = T2m + dT2m_c,
 * precip_c = precip * precip_scale_c (SURVEY.md section 8 d, cfg3). */
int samsim_set_forcing(samsim_handle *h, int32_t len, const double *fl_sw, const double *fl_lw,
                       const double *T2m, const double *precip,
                       const double *dT2m_col, const double *precip_scale_col);
/* Forcing for a grid of columns: nsites sets of the four tables (e.g. the nine ERA-interim sites
 * under input/ERA-interim of the reference), each array holding set s at [s*len, (s+1)*len); site_of_column[c] in
 * [0, nsites) selects the set column c reads.  samsim_set_forcing is the one-site case. */
int samsim_set_forcing_sites(samsim_handle *h, int32_t nsites, int32_t len, const double *fl_sw, const double *fl_lw,
                             const double *T2m, const double *precip, const int32_t *site_of_column,
                             const double *dT2m_col, const double *precip_scale_col);

/* The water below a grid of columns (the reference has one column and sets both as scalars of mo_data):
 * dfl_q_bottom_col[c] ([ncol] or NULL) is added to the oceanic heat flux sub_test4 assigns every step (testcases 4 and 7,
 * mo_testcase_specifics.f90:197-202: fl_q_bottom_c = -7 sin(2 pi t / year) + 7 + dfl_q_bottom_c); S_bu_bottom_col[c] ([ncol] or
 * NULL) replaces cfg.S_bu_bottom for column c wherever the reference reads S_bu_bottom (mass_transfer's ghost cell, flooding,
 * bottom turbulence, bottom growth; tank_flag 1 -- with tank_flag 2 the tank budget owns it, mo_grotz.f90:573-575).  A column
 * with offset 0 and cfg.S_bu_bottom is the reference's column.  NULL, NULL switches both off. */
int samsim_set_ocean(samsim_handle *h, const double *dfl_q_bottom_col, const double *S_bu_bottom_col);

/* initial state of init(testcase) (mo_init.f90:141-1978) or a checkpoint; col0 and s->ncol select a window.
 * The two perturbation slots SAMSIM_S_DT2M / SAMSIM_S_PRECIP_SCALE are owned by samsim_set_forcing: set_state
 * ignores them, get_state returns them.
 * The health check at the end of a step clamps S_abs >= 0 over the active layers (mo_grotz.f90:812-818).  The state samsim_get_state
 * returns after a step is the clamped one, as the reference holds it between two steps; a state that samsim_set_state uploads is
 * taken as it is, as the reference takes its initial state: a negative S_abs in it enters the first step (where the expelled brine's
 * mass_transfer may absorb it, or gravity drainage's MINVAL(S_abs) test stops the column with 1337). */
/* Both move the layer arrays of the window through a device staging buffer in pieces of at most SAMSIM_STAGE_MAX_BYTES: the
 * buffer never holds more, whatever the window. */
#define SAMSIM_STAGE_MAX_BYTES (256ull << 20)
int samsim_set_state(samsim_handle *h, const samsim_state_soa *s, int64_t col0);
int samsim_get_state(samsim_handle *h, samsim_state_soa *s, int64_t col0);
int samsim_set_clock(samsim_handle *h, const samsim_clock *c);
int samsim_get_clock(samsim_handle *h, samsim_clock *c);

/* The time loop body, mo_grotz.f90:182-835, nsteps times for every column.  Asynchronous on the
 * handle's HIP stream; every getter synchronises. */
int samsim_step(samsim_handle *h, int64_t nsteps);
/* same, and returns the device time of the launch(es) measured with HIP events on the handle's stream */
int samsim_step_timed(samsim_handle *h, int64_t nsteps, double *kernel_ms);
/* nlaunches launches of nsteps steps each, enqueued back to back (no wait in between: the tail of one launch is filled by the
 * head of the next), and the device time of the whole sequence, measured with HIP events on the handle's streams (ABI 4) */
int samsim_steps_timed(samsim_handle *h, int64_t nsteps, int32_t nlaunches, double *device_ms);
int samsim_synchronize(samsim_handle *h);
/* which GPU the handle lives on: the ordinal passed to samsim_create and the PCI bus id HIP reports for it (pci_bus_id: buffer
 * of len >= 16 bytes, or NULL).  A multi-process run records it per rank so that a scaling record shows no GPU was shared.  ABI 5. */
int samsim_get_device(samsim_handle *h, int32_t *device, char *pci_bus_id, int32_t len);
/* How a step of a large ensemble is launched (no reference counterpart; results do not depend on it, bit for bit).  From
 * min_blocks 64-column blocks up (default 8 192 = 524 288 columns; 0 = never) a step runs as two concurrent launches on the
 * handle's two HIP streams, the first taking first_part_eighths/8 of the blocks (default 4): the workgroups of one launch finish
 * raggedly and a second launch in flight tops the chip up.  Every other entry point waits for both.  ABI 5. */
int samsim_set_launch_split(samsim_handle *h, int64_t min_blocks, int32_t first_part_eighths);

/* number of steps until (and including) the next output point of mo_grotz.f90:340 */
int64_t samsim_steps_to_output(samsim_handle *h);
int samsim_set_output_window(samsim_handle *h, int64_t col0, int64_t ncols);
/* output (mo_output.f90:116-146): latest snapshot; returns SAMSIM_ERR_NO_OUTPUT if none was taken */
int samsim_get_output(samsim_handle *h, samsim_output_soa *o);

/* the reference's STOP codes: status[c] = 0 or code; step/layer of first failure.  Every code is one of the
 * reference's own (16, 99, 345, 431, 1337, 7889, 9876, 21234, ...): the library stops no column the reference would not.
 *
 * step[c] is the 1-based index i of the time step in which the column stopped (clock.step + 1 of that step).  A stopped column is
 * frozen: no later step changes its state, its status or its share of samsim_get_work, and the ensemble statistics leave it out.
 *
 * layer[c] is the library's own notion (the reference prints none).  It is the layer k where the reference's test sits inside a
 * layer loop or names a layer, and 0 where the reference tests a quantity of the whole column or of the snow:
 *
 *   code   site of the reference                                              layer
 *   99     getT of a layer, first or second sweep (mo_grotz.f90:297-307, 592-598)   k; several failing layers in one sweep: the
 *                                                                              LARGEST k -- the sweeps run from N_active up to 1,
 *                                                                              and that is where the reference aborts
 *   99     getT of layer 1 at the head of a step whose other layers were swept by the step before     1
 *   99     either getT of the thin-snow coupling, snow_coupling (mo_snow.f90:61-104), of the snow or of layer 1:      1
 *   16     the exchange loop of the thin-snow coupling does not converge        1
 *   99     getT of the snow in snow_thermo / snow_thermo_meltwater (mo_snow.f90:212-454)   0
 *   345    snow_thermo: psi_s_snow + psi_l_snow                                  0
 *   9876   snow_thermo: psi_g_snow < 0                                           0
 *   21234  gravity drainage: S_abs(k) < 0 after the loss of layer k (mo_grav_drain.f90:144-170)    k; several: the SMALLEST k (that
 *                                                                              loop runs from layer 1 to N_active - 1)
 *   1337   gravity drainage: MINVAL(S_abs) < 0 (mo_grav_drain.f90:197)           0
 *   431    energy balance of sub_heat_fluxes (mo_heat_fluxes.f90:265-310)        0
 *   9876   flush3: m(1) flushed away (mo_flush.f90)                              1
 *   9876   flush4: MINVAL(S_abs) < 0 (mo_flush.f90:253-296)                      0
 *   7889   top_melt: SUM(thick) (mo_layer_dynamics.f90:191-327)                  0
 *   1337   health check at the end of the step: MINVAL(psi_s) < 0 (mo_grotz.f90:808-819)   0
 *
 * A column that meets two tests in one step reports the one the reference reaches first; within sub_heat_fluxes and after it
 * the order is: thin-snow coupling (99, 16), energy balance (431), second getT sweep (99).
 * The coupling reports layer 1 for both of its getT calls because it runs them as one pair and keeps one return code.
 * STOP 431 fires only through round-off (an enthalpy whose ulp exceeds 1e-5 W * dt): the reference compares two column sums, the
 * library sums per-layer differences, so on such a column the two may stop in different steps (tests/stop_seeds.py). */
int samsim_get_status(samsim_handle *h, int32_t *status, int64_t *step, int32_t *layer);
/* restart only: puts back what samsim_get_status returned for the columns [col0, col0+ncols) (samsim_set_state clears the
 * status of the columns it uploads), so that a column frozen by a STOP code stays frozen -- and reported -- after a
 * checkpoint / restart.  step and layer may be NULL. */
int samsim_set_status(samsim_handle *h, const int32_t *status, const int64_t *step, const int32_t *layer, int64_t col0,
                      int64_t ncols);
/* sum over columns of N_active accumulated over all steps taken (layer-cell updates) */
int samsim_get_work(samsim_handle *h, int64_t *layer_cell_updates, int64_t *column_steps);

/* Passive biogeochemical tracers (bgc_flag 2; mo_data.f90:181-193, bgc_advection mo_mass.f90:150-209): n_bgc tracers,
 * bgc_abs[t][k][c] = amount of tracer t in layer k of column c.  samsim_set_tracers fixes their number, the concentration
 * of the water below the ice (bgc_bottom, mo_init.f90:934-935) and -- tank_flag 2 only, else NULL -- the totals in the tank
 * (bgc_total, mo_init.f90:1013); it must be called before the first step.  The tracer state is zero until set
 * (init: bgc_abs(1,:) = bgc_bottom(:)*m(1), mo_init.f90:940).  samsim_get_tracer_output returns the snapshot taken at the
 * reference's output point for the output window: bgc_abs[n_bgc][nlayer][ncols], bgc_bottom[n_bgc][ncols]. */
#define SAMSIM_MAX_NBGC 8
int samsim_set_tracers(samsim_handle *h, int32_t n_bgc, const double *bgc_bottom, const double *bgc_total);
int samsim_set_tracer_state(samsim_handle *h, const double *bgc_abs, int64_t col0, int64_t ncols);
int samsim_get_tracer_state(samsim_handle *h, double *bgc_abs, double *bgc_bottom, int64_t col0, int64_t ncols);
/* restart only: the per-column concentration of the water below, bgc_bottom[n_bgc][ncols], as samsim_get_tracer_state
 * returned it (it evolves with the tank budget, mo_grotz.f90:575-577; samsim_set_tracers sets one value for all columns) */
int samsim_set_tracer_bottom(samsim_handle *h, const double *bgc_bottom, int64_t col0, int64_t ncols);
int samsim_get_tracer_output(samsim_handle *h, double *bgc_abs, double *bgc_bottom);

/* Ensemble statistics (what replaces "one column per .dat row", mo_output.f90:129-144, when the
 * run holds 10^5..10^6 columns): for each requested per-column scalar (enum samsim_scalar, or SAMSIM_STAT_N_ACTIVE) the
 * number of columns that have not failed, their mean, minimum, maximum and population standard deviation, reduced on the
 * device.  The vital signs and the freeboard hold the values of the last output point (mo_grotz.f90:192-223, 340-347). */
#define SAMSIM_STAT_N_ACTIVE (-1)
typedef struct samsim_stat {
  int64_t count;
  double  mean, min, max, std;
} samsim_stat;
int samsim_get_ensemble_stats(samsim_handle *h, int32_t nslots, const int32_t *slots, samsim_stat *out);

/* Ensemble statistics of the layer profiles, by layer and by depth (ABI 6): the same five numbers as above for the layer arrays --
 * the reference's main products dat_T, dat_S_bu, dat_psi_l, dat_thick ..., which its plot scripts read as step functions of
 * depth -- per bin, reduced on the device; only per-bin results come back.  out[narrays][nbins].  A request is served in passes
 * of one array and at most 64 bins; a pass walks the layers of every column once and reads only the rows it needs (the array --
 * S_abs and m for S_bu --, and thick on the depth axis, which is therefore read once per array and chunk, twice from the bottom), so
 * the cost grows with narrays * ceil(nbins / 64).
 *
 *   Columns.  Only columns with status == 0 count.  Na = n_active[c].
 *   Layer value.  a_k is the stored value of the array in layer k, 1 <= k <= Na; for SAMSIM_A_S_BU it is S_abs(k)/m(k) where
 *     m(k) != 0 (the stored value elsewhere): what samsim_get_state returns.  After any launch every row is current (the last
 *     step of a launch stores everything), so the statistics describe the state samsim_get_state would return now.
 *   Depth coordinate.  Z_0 = 0, Z_k = Z_{k-1} + thick(k) by sequential double additions, k ascending; H = Z_Na.  Snow is not
 *     part of the coordinate; the lowest active layer counts with its full thick.
 *   SAMSIM_PROFILE_BY_LAYER.  Bin b (0-based) receives, FROM_TOP, a_{b+1} of the columns with b+1 <= Na; FROM_BOTTOM, a_{Na-b}
 *     of the columns with Na-b >= 1.
 *   SAMSIM_PROFILE_BY_DEPTH.  Edges e_b = z0 + b*dz (the product is rounded, then the sum; no fused multiply-add).  Layer k
 *     covers [lo_k, hi_k): FROM_TOP [Z_{k-1}, Z_k), FROM_BOTTOM [H - Z_k, H - Z_{k-1}).  o_kb = max(0, min(hi_k, e_{b+1}) -
 *     max(lo_k, e_b)); L_b = sum_k o_kb and W_b = sum_k o_kb*a_k, both over ascending k.  A column contributes to bin b if and
 *     only if L_b > 0, with the value v = W_b / L_b (IEEE division): the step-function profile averaged over the bin.
 *   Statistics.  Per (array, bin) over the contributing columns: count, mean, min, max and the population standard deviation
 *     sqrt(sum (v-mean)^2 / count) (formed from deviations, never from sum v^2 - n mean^2); with count == 0 the other four are 0.0.
 *     Fixed grid, fixed order of combination, no floating-point atomics: two calls on the same state return the same bytes.
 *   Errors, all found before any device work.  SAMSIM_ERR_ABI: wrong struct_size.  SAMSIM_ERR_ARG: axis, origin, nbins (also
 *     > nlayer with BY_LAYER), narrays or an array id out of range; with BY_DEPTH a non-finite z0 or dz, z0 < 0 or dz <= 0.
 *   Like every getter the call waits for the handle's streams; it changes neither the state, the clock nor the output snapshot.
 *   Device scratch: at most SAMSIM_PROFILE_SCRATCH_BYTES whatever ncol and the request are (every pass reuses it); allocated on first use, kept in the handle, freed by samsim_destroy. */
#define SAMSIM_PROFILE_MAX_BINS   1024   /* = SAMSIM_MAX_NLAYER */
#define SAMSIM_PROFILE_MAX_ARRAYS 8
#define SAMSIM_PROFILE_SCRATCH_BYTES (3ull << 20)
enum samsim_profile_axis   { SAMSIM_PROFILE_BY_LAYER = 0, SAMSIM_PROFILE_BY_DEPTH = 1 };
enum samsim_profile_origin { SAMSIM_PROFILE_FROM_TOP = 0, SAMSIM_PROFILE_FROM_BOTTOM = 1 };
typedef struct samsim_profile_request {
  int32_t struct_size;   /* = sizeof(samsim_profile_request) */
  int32_t axis, origin;
  int32_t nbins;         /* 1..SAMSIM_PROFILE_MAX_BINS; BY_LAYER: also <= nlayer */
  int32_t narrays;       /* 1..SAMSIM_PROFILE_MAX_ARRAYS */
  int32_t arrays[SAMSIM_PROFILE_MAX_ARRAYS];   /* enum samsim_layer_array */
  double  z0, dz;        /* BY_DEPTH only: z0 >= 0, dz > 0, finite; metres */
} samsim_profile_request;
int samsim_get_profile_stats(samsim_handle *h, const samsim_profile_request *rq, samsim_stat *out);

/* Ensemble statistics per group of columns -- per forcing site, per class of the perturbation, per ocean regime -- reduced on the
 * device.  The three entry points below were added without a change of SAMSIM_ABI_VERSION (it stays 6): they are new symbols only,
 * no existing struct or signature changed, and a caller that wants them finds them by symbol (dlsym; a library built before them
 * does not export them).
 *
 * samsim_set_groups attaches a label to every column: group_of_column[c] in [-1, ngroups), -1 = the column is in no group;
 *   ngroups in 1..SAMSIM_MAX_GROUPS.  ngroups == 0 with NULL removes the labels.  Every label is checked on the host before any
 *   device work: SAMSIM_ERR_ARG for a bad ngroups, a bad label or NULL with ngroups > 0, and a call that is refused leaves the
 *   previous labels in force.  The labels live on the device as int32[ncol] and belong to the caller, as the forcing does:
 *   samsim_set_state, samsim_set_status and stepping leave them alone, they are not part of a checkpoint (a restart sets them
 *   again, as it sets the forcing again), samsim_destroy frees them.
 * samsim_get_group_stats: out[nslots][ngroups], the slots of samsim_get_ensemble_stats (SAMSIM_STAT_N_ACTIVE included).  Group g
 *   covers the columns with status == 0 and label g; per (slot, group) count, mean, min, max and the population standard
 *   deviation, with count == 0 the other four are 0.0.  All groups of a slot are reduced in one walk over the row.
 *   SAMSIM_ERR_ARG when no labels are set or a slot is out of range, found before any device work.
 * samsim_get_group_profile_stats: samsim_get_profile_stats restricted to the columns with label `group` (a column with another
 *   label or -1 behaves like a stopped one); all of that function's argument checks, in the same order, then SAMSIM_ERR_ARG when
 *   no labels are set or group lies outside [0, ngroups).  One group per call: a request for G groups is G calls.
 *
 *   Statistics.  count, min and max are exact.  mean and std are formed from deviations (running and pairwise (n, mean, M2)), never
 *     from sum v^2 - n mean^2.  No floating-point atomics, a grid fixed by ncol and ngroups, a fixed order of combination: two calls
 *     on the same state and labels return the same bytes.
 *   Invariance.  The order in which the values of group g are combined depends only on the positions of g's columns: relabelling
 *     columns outside g (in other groups, or with label -1) leaves g's results unchanged, byte for byte.
 *   A group whose columns hold identical values gives mean == min == max and std == 0.0 exactly.
 *   With ngroups == 1 and every label 0, samsim_get_group_profile_stats(h, rq, 0, out) returns the bytes of
 *     samsim_get_profile_stats(h, rq, out).
 *   Like every getter the calls wait for the handle's streams; they change neither the state, the clock nor the output snapshot.
 *   Device scratch of samsim_get_group_stats: at most SAMSIM_GROUP_SCRATCH_BYTES whatever ncol, nslots and ngroups are (every slot
 *     reuses it); allocated on first use, kept in the handle, freed by samsim_destroy.  Only results come back to the host. */
#define SAMSIM_MAX_GROUPS 1024
#define SAMSIM_GROUP_SCRATCH_BYTES (16ull << 20)
int samsim_set_groups(samsim_handle *h, int32_t ngroups, const int32_t *group_of_column);
int samsim_get_group_stats(samsim_handle *h, int32_t nslots, const int32_t *slots, samsim_stat *out);
int samsim_get_group_profile_stats(samsim_handle *h, const samsim_profile_request *rq, int32_t group, samsim_stat *out);

/* Fixed-edge histograms of the ensemble, reduced on the device: how the columns are DISTRIBUTED, where the statistics above give
 * four moments -- the ice-thickness distribution of a perturbed ensemble, the share of columns above a threshold, the median and
 * the 5-95 % band of a profile (from the counts on the host: quantile brackets).  The two entry points below were added without a
 * change of SAMSIM_ABI_VERSION (it stays 6): new symbols only, found by symbol as the group functions are.  The output has a fixed
 * size and the counts are integers; this is not exact selection.
 *
 *   Edges.  E_j = v0 + j*dv, j = 0..nvbins (the product is rounded, then the sum; no fused multiply-add).
 *   Entries.  A row of counts has nvbins + 2 entries.  The entry of a value v is idx(v) = the number of edges E_j, j = 0..nvbins,
 *     with E_j <= v: entry 0 holds v < E_0, entry j+1 holds E_j <= v < E_{j+1}, entry nvbins+1 holds v >= E_nvbins.  A NaN compares
 *     false with every edge and lands in entry 0.  The definition holds exactly, against the rounded edges, not to within a rounding:
 *     the device may guess j from (v - v0)/dv, and then corrects the guess against the edges themselves.
 *   samsim_get_histogram.  slot is an enum samsim_scalar or SAMSIM_STAT_N_ACTIVE (the value is then (double)n_active).
 *     by_group == 0: counts[nvbins+2] over the columns with status == 0.  by_group == 1: counts[ngroups][nvbins+2]; group g covers the
 *     columns with status == 0 and label g (samsim_set_groups), and all groups are reduced in one walk over the row.
 *   samsim_get_profile_histogram.  rq is a request of samsim_get_profile_stats with narrays == 1; counts[rq->nbins][nvbins+2], a joint
 *     histogram over depth bin x value bin.  The value of column c in bin b is exactly the v of samsim_get_profile_stats -- BY_LAYER
 *     the layer value a_k, BY_DEPTH W_b / L_b from the same sums in the same order --, and a column contributes to bin b under exactly
 *     the same condition (BY_LAYER: the layer exists; BY_DEPTH: L_b > 0).  group == -1: every column with status == 0, no labels
 *     needed.  group >= 0: only the columns with that label, one group per call as with samsim_get_group_profile_stats.
 *     A request is served in passes of `chunk` depth bins, each a walk over the layers of every column as in the profile statistics:
 *     passes = ceil(nbins / chunk), chunk = 64 up to 121 value bins, falling to 42 at SAMSIM_HIST_MAX_VBINS (the walk's tile and
 *     the count table share the 64 KiB of LDS of a workgroup: chunk = min(64, 65 024 / (520 + 4 * ((nvbins + 2) | 1)))).
 *   Invariants.  The entries of a row sum to the `count` that the matching statistics call returns (samsim_get_ensemble_stats,
 *     samsim_get_group_stats, samsim_get_profile_stats, samsim_get_group_profile_stats).  Integer counts, no floating-point
 *     atomics: two calls on the same state return the same bytes.  Relabelling columns outside g leaves g's row unchanged.
 *     Like every getter the calls wait for the handle's streams; they change neither the state, the clock nor the output snapshot.
 *   Errors, all found before any device work.  SAMSIM_ERR_ARG: h, vb, rq or counts NULL.  SAMSIM_ERR_ABI: wrong struct_size of either
 *     struct.  SAMSIM_ERR_ARG: nvbins out of range; a non-finite v0 or dv; dv <= 0; edges that are not all finite and strictly
 *     increasing (checked on the host over all nvbins+1 edges); a bad slot; by_group other than 0 or 1; by_group == 1 without labels.
 *     samsim_get_profile_histogram checks in this order: every check of samsim_get_profile_stats, in its order; narrays != 1; the
 *     vb checks as above; group < -1, or group >= 0 without labels, or group >= ngroups.
 *   Device scratch: at most SAMSIM_HIST_SCRATCH_BYTES whatever ncol and the request are (the 64-bit counts of one request);
 *     allocated on first use, kept in the handle, freed by samsim_destroy.  Only counts come back to the host. */
#define SAMSIM_HIST_MAX_VBINS 254          /* value bins; a row of counts has nvbins + 2 entries */
#define SAMSIM_HIST_SCRATCH_BYTES (2ull << 20)   /* 1 024 rows (groups, or depth bins) of 256 int64 counts */
typedef struct samsim_hist_bins {
  int32_t struct_size;   /* = sizeof(samsim_hist_bins) */
  int32_t nvbins;        /* 1..SAMSIM_HIST_MAX_VBINS   */
  double  v0, dv;        /* edges E_j = v0 + j*dv, j = 0..nvbins */
} samsim_hist_bins;
int samsim_get_histogram(samsim_handle *h, int32_t slot, const samsim_hist_bins *vb, int32_t by_group, int64_t *counts);
int samsim_get_profile_histogram(samsim_handle *h, const samsim_profile_request *rq, const samsim_hist_bins *vb,
                                 int32_t group, int64_t *counts);

/* Ensemble sensitivities, reduced on the device: how two quantities of the same column vary TOGETHER over the ensemble, where
 * everything above gives marginal results -- the covariance matrix of up to SAMSIM_SENS_MAX_SLOTS per-column scalars, and per depth
 * bin the joint second moments of a layer profile and one per-column predictor, from which the host forms regression slopes
 * (cov / var_x) and correlations (cov / sqrt(var_x var_y)): the response of the ice to the perturbation of samsim_set_forcing.  The
 * two entry points below were added without a change of SAMSIM_ABI_VERSION (it stays 6): new symbols only, found by symbol as the
 * group and histogram functions are.
 *
 *   Columns (both).  A column counts if its status is 0 and, with group >= 0, its label (samsim_set_groups) equals group.
 *     group == -1: every column with status 0, no labels needed.  One group per call, as with samsim_get_group_profile_stats.
 *   Slots (both).  A slot is an enum samsim_scalar or SAMSIM_STAT_N_ACTIVE (the value is then (double)n_active).  A slot may appear
 *     twice in slots.  The perturbation slots SAMSIM_S_DT2M and SAMSIM_S_PRECIP_SCALE are the intended predictors.
 *   samsim_get_covariance.  count = the number of columns that count; mean[i] = the mean of slot i over them; cov[i][j] = the
 *     population covariance sum (x_i - mean_i)(x_j - mean_j) / count of slots i and j over them, the diagonal the variance.  One
 *     triangle is computed and mirrored: cov[i][j] and cov[j][i] are the same bytes.  With count == 0 every output is 0.0.
 *   samsim_get_profile_regression.  rq is a request of samsim_get_profile_stats with any narrays; out[narrays][nbins].  y is exactly
 *     the v of that function for (array, bin), and a column contributes to a bin under exactly that function's condition (BY_LAYER:
 *     the layer exists; BY_DEPTH: L_b > 0); x is the column's value of predictor_slot.  Per (array, bin), over the contributing
 *     columns: count, mean_x, mean_y, var_x, var_y and cov, population moments (sums of products of deviations / count).  The set of
 *     contributing columns differs from bin to bin, so mean_x and var_x are per-bin results.  With count == 0 the five doubles are
 *     0.0.  Slope and correlation are not part of the ABI: the host forms them.  A request is served in passes of one array and at
 *     most 64 bins, as samsim_get_profile_stats is.
 *   Arithmetic.  Everything is formed from deviations -- Welford's update of means and co-moments per lane, Chan's pairwise
 *     combination of (n, mean, co-moment) triples across lanes and waves --, never from sum xy - n mean_x mean_y.  No floating-point
 *     atomics, a grid fixed by ncol alone, a fixed order of combination: two calls on the same state return the same bytes, and
 *     relabelling columns outside `group` leaves the result unchanged, byte for byte.  Columns that hold identical values give means
 *     equal to the value and variances and covariances of 0.0, exactly.  A slot listed twice gives identical rows and columns:
 *     cov[i][j] == cov[i][i] == cov[j][j] bitwise.  samsim_get_profile_regression folds y with the fold and merge of the profile
 *     statistics: count and mean_y are the count and mean bytes of samsim_get_profile_stats for the same request
 *     (samsim_get_group_profile_stats with a group), and sqrt(var_y) is its std bytes.
 *   Errors, all found before any device work, in this order.  samsim_get_covariance: SAMSIM_ERR_ARG for h, slots, count, mean or cov
 *     NULL; nslots outside 1..SAMSIM_SENS_MAX_SLOTS; a bad slot; group < -1, group >= 0 without labels, or group >= ngroups.
 *     samsim_get_profile_regression: SAMSIM_ERR_ARG for h, rq or out NULL; every check of samsim_get_profile_stats, in its order; a bad
 *     predictor_slot; the group checks as above.
 *   Like every getter the calls wait for the handle's streams; they change neither the state, the clock, the output snapshot nor the
 *     labels.  Device scratch: at most SAMSIM_SENS_SCRATCH_BYTES whatever ncol and the request are (the waves' partials of one pass,
 *     then the results); allocated on first use, kept in the handle, freed by samsim_destroy.  Only results come back to the host;
 *     nothing is merged there.  A host that holds several handles or ranks can combine their results itself: (count, mean, count *
 *     cov) are (n, mean, co-moment) triples, merged by the same Chan update. */
#define SAMSIM_SENS_MAX_SLOTS 8
#define SAMSIM_SENS_SCRATCH_BYTES (4ull << 20)
typedef struct samsim_pair_stat {      /* 48 bytes */
  int64_t count;
  double  mean_x, mean_y, var_x, var_y, cov;   /* population moments: sums of products of deviations / count */
} samsim_pair_stat;
int samsim_get_covariance(samsim_handle *h, int32_t nslots, const int32_t *slots, int32_t group,
                          int64_t *count, double *mean /*[nslots]*/, double *cov /*[nslots][nslots]*/);
int samsim_get_profile_regression(samsim_handle *h, const samsim_profile_request *rq, int32_t predictor_slot,
                                  int32_t group, samsim_pair_stat *out /*[narrays][nbins]*/);

/* Time-domain diagnostics: per-column tracks sampled on the device.  Everything above describes the ensemble at one moment; a track
 * follows one observable of every column THROUGH the run and keeps eleven numbers per column -- the annual maximum of the ice
 * thickness and when it is reached, the first and last step at which a condition held (melt onset, freeze-up), for how many samples
 * it held (the length of the melt season), the mean and variance over time -- without a samsim_get_state per look.  The entry points
 * below were added without a change of SAMSIM_ABI_VERSION (it stays 6): new symbols only, found by symbol as the group, histogram and
 * sensitivity functions are.
 *
 *   Observable x of a column at a sample, computed from the state samsim_get_state would return at that moment.
 *     SAMSIM_OBS_SCALAR: the stored slot `id` (enum samsim_scalar).  SAMSIM_OBS_N_ACTIVE: (double)n_active.
 *     SAMSIM_OBS_ICE_THICKNESS: Z_Na of the profile statistics, Z_0 = 0, Z_k = Z_{k-1} + thick(k) by sequential double additions, k
 *     ascending.  SAMSIM_OBS_BULK_SALINITY: (sum_k S_abs(k)) / (sum_k m(k)), both sums sequential over k = 1..Na, then one IEEE
 *     division; with a zero mass sum the quotient is whatever IEEE gives.  SAMSIM_OBS_LAYER: the value of array `id` (enum
 *     samsim_layer_array) in the addressed layer, exactly as samsim_get_state returns it (for SAMSIM_A_S_BU S_abs/m where m != 0):
 *     layer k >= 1 counts from the top (layer k), k <= -1 from the bottom (layer Na + 1 + k).  A LAYER track whose layer does not
 *     exist in a column (k > Na or Na + 1 + k < 1) is not sampled for that column at that moment: none of its fields change.
 *   When samples are taken.  After the step that brings clock.step to s, whenever s % every == 0: sampling is tied to the absolute
 *     step count, not to the steps since samsim_set_tracks.  Every column with status == 0 at that moment is sampled with sample time
 *     s; stopped columns are never sampled, nor is the state before the first step.  How the caller cuts its samsim_step calls and how
 *     samsim_set_launch_split is set do not change a byte of any track (a call is cut into launches at the sample points inside it,
 *     and the run is bit-for-bit independent of where launches are cut); tracking does not change a byte of the state, the status,
 *     the clock, the work counters or the output snapshot.  samsim_steps_timed times the samples with the steps.
 *   Fields.  One double[ncol] row per track and field (enum samsim_track_field).  Initial values: N = 0, LAST = 0, MEAN = 0, M2 = 0,
 *     MIN = +inf, STEP_MIN = -1, MAX = -inf, STEP_MAX = -1, N_HOLD = 0, STEP_FIRST = -1, STEP_LAST = -1.  Update at a sample with value x
 *     and time s, in this order:
 *       N += 1;  LAST = x;  d = x - MEAN;  MEAN = MEAN + d / N (an IEEE division);  M2 = M2 + d * (x - MEAN) (the new MEAN; the
 *       product is rounded, then the sum; no fused multiply-add);
 *       if x < MIN: MIN = x, STEP_MIN = s;   if x > MAX: MAX = x, STEP_MAX = s;
 *       if the condition holds (sense +1: x >= threshold; sense -1: x < threshold; sense 0: never): N_HOLD += 1; if STEP_FIRST < 0:
 *       STEP_FIRST = s; STEP_LAST = s.
 *     The first attainment of an extreme is kept.  A NaN never becomes an extreme and never satisfies a condition.  Step numbers are
 *     stored as doubles, exact below 2^53.  The update of a column is a fixed sequence of IEEE operations on that column's own data, no
 *     cross-lane arithmetic: every field is reproducible to the bit by a host that applies the same sequence to samsim_get_state at
 *     the same moments.  The time variance is M2 / N, dates are STEP_* * dt: the host forms both.
 *   samsim_set_tracks.  ntracks in 1..SAMSIM_MAX_TRACKS, every >= 1: allocates [ntracks][SAMSIM_NTF][ncol] doubles on the device and
 *     sets them to the initial values.  ntracks == 0 with NULL removes tracking and frees the rows (also when none was set).  A call
 *     that is refused leaves the previous tracks in force.  samsim_reset_tracks sets the initial values again.  samsim_set_state,
 *     samsim_set_status and samsim_set_clock leave the rows alone; samsim_destroy frees them.  The rows are not part of a checkpoint:
 *     for a restart samsim_get_tracks and samsim_set_track_state move the window [col0, col0 + ncols) of one track, [SAMSIM_NTF][ncols];
 *     a restart sets the tracks first and then puts the rows back.
 *   Track rows as slots.  Wherever a slot is accepted -- samsim_get_ensemble_stats, samsim_get_group_stats, samsim_get_histogram, the
 *     slots of samsim_get_covariance, predictor_slot of samsim_get_profile_regression -- SAMSIM_TRACK_SLOT(track, field) is accepted
 *     too, with track < ntracks and field < SAMSIM_NTF of the tracks in force, and resolves to that row; without tracks, or out of
 *     range, it is the SAMSIM_ERR_ARG of any bad slot.  So the distribution of the onset date over the ensemble is a histogram of
 *     STEP_FIRST (with v0 = 0, entry 0 holds the columns in which it never happened), its statistics per site a samsim_get_group_stats,
 *     its covariance with dT2m a samsim_get_covariance; and a track of ICE_THICKNESS with `every` equal to the launch length gives
 *     the reductions a current thickness through LAST, where SAMSIM_S_THICKNESS holds the last output point's.
 *   Errors, all found before any device work, in this order.  samsim_set_tracks: SAMSIM_ERR_ARG for h NULL; ntracks out of range;
 *     specs NULL with ntracks > 0; every < 1 with ntracks > 0; then per spec in order: SAMSIM_ERR_ABI for a wrong struct_size;
 *     SAMSIM_ERR_ARG for a bad kind or a bad id for the kind; layer == 0 or |layer| > nlayer with LAYER; a non-zero layer or id where
 *     the kind takes none; sense outside {-1, 0, 1}; a non-finite threshold with sense != 0; reserved != 0.  SAMSIM_ERR_NOMEM if the rows
 *     cannot be allocated (the previous tracks stay).  The other three: SAMSIM_ERR_ARG for NULL pointers, no tracks set, a track
 *     outside [0, ntracks), a window outside [0, ncol). */
#define SAMSIM_MAX_TRACKS 8
enum samsim_observable_kind { SAMSIM_OBS_SCALAR = 0, SAMSIM_OBS_N_ACTIVE, SAMSIM_OBS_ICE_THICKNESS, SAMSIM_OBS_BULK_SALINITY, SAMSIM_OBS_LAYER };
enum samsim_track_field { SAMSIM_TF_N = 0, SAMSIM_TF_LAST, SAMSIM_TF_MEAN, SAMSIM_TF_M2, SAMSIM_TF_MIN, SAMSIM_TF_STEP_MIN,
                          SAMSIM_TF_MAX, SAMSIM_TF_STEP_MAX, SAMSIM_TF_N_HOLD, SAMSIM_TF_STEP_FIRST, SAMSIM_TF_STEP_LAST, SAMSIM_NTF };
typedef struct samsim_track_spec {
  int32_t struct_size; /* = sizeof(samsim_track_spec) */
  int32_t kind;        /* enum samsim_observable_kind */
  int32_t id;          /* SCALAR: enum samsim_scalar; LAYER: enum samsim_layer_array; else 0 */
  int32_t layer;       /* LAYER: k >= 1 counts from the top (layer k), k <= -1 from the bottom (layer Na + 1 + k); else 0 */
  int32_t sense;       /* 0 no condition, +1 holds when x >= threshold, -1 holds when x < threshold */
  int32_t reserved;    /* 0 */
  double  threshold;   /* finite when sense != 0 */
} samsim_track_spec;
int samsim_set_tracks(samsim_handle *h, int32_t ntracks, const samsim_track_spec *specs, int64_t every);
int samsim_reset_tracks(samsim_handle *h);
int samsim_get_tracks(samsim_handle *h, int32_t track, int64_t col0, int64_t ncols, double *out /*[SAMSIM_NTF][ncols]*/);
int samsim_set_track_state(samsim_handle *h, int32_t track, int64_t col0, int64_t ncols, const double *in /*[SAMSIM_NTF][ncols]*/);
#define SAMSIM_TRACK_SLOT(track, field) (0x10000 + (track) * 32 + (field))

/* Which columns, and what they look like.  Every reduction above answers a question about the ensemble as a whole; a histogram that
 * says 412 members are thinner than 0.3 m, or a status that says three columns stopped, ends in "show me those columns".  The two
 * entry points below return the indices of the columns a predicate holds for, evaluated on the device, and the full state of an
 * arbitrary list of columns -- without a download of the whole state and without one samsim_get_state per column.  They return
 * indices and the state of existing columns and write nothing to the ensemble: this is neither exact selection of quantiles nor a copy
 * of columns.  They were added without a change of SAMSIM_ABI_VERSION (it stays 6): new symbols only, found by symbol as the group,
 * histogram, sensitivity and track functions are.
 *
 *   samsim_select_columns.  A column matches when its status passes status_mode, its label passes group and every term holds.
 *     Slots.  A slot is an enum samsim_scalar, SAMSIM_STAT_N_ACTIVE (x is then (double)n_active) or SAMSIM_TRACK_SLOT(track, field) of
 *       the tracks in force: what every reduction above accepts.
 *     Terms.  A term holds when lo <= x && x < hi, two IEEE comparisons: a NaN x satisfies no term; lo = -inf and hi = +inf are
 *       allowed; lo >= hi is allowed and gives an empty selection.  The terms are ANDed; nterms == 0 puts no condition on values.
 *     Status.  SAMSIM_SELECT_RUNNING: status == 0, the columns the statistics count.  SAMSIM_SELECT_STOPPED: status != 0.
 *       SAMSIM_SELECT_CODE: status == code.  SAMSIM_SELECT_ANY: every column.  A stopped column is tested on the values it froze with.
 *     Group.  -1: any column, no labels needed.  >= 0: only the columns with that label (samsim_set_groups).
 *     Result.  *n_match is the exact number of matching columns, whatever max_out is.  cols_out receives the first
 *       min(*n_match, max_out) matching column indices in ascending order; entries beyond them are left alone.  max_out == 0 with
 *       cols_out == NULL only counts.  With the status mode RUNNING the matches of the term [E_j, E_{j+1}) are entry j+1 of
 *       samsim_get_histogram, and with no terms *n_match is the count of samsim_get_ensemble_stats (samsim_get_group_stats with a group).
 *     Invariants.  The order is fixed and the counts are integers; no atomics, no hand-off between workgroups: two calls on the same
 *       state return the same bytes.  Relabelling columns outside `group` does not change the result.  Like every getter the call waits
 *       for the handle's streams; it changes neither the state, the status, the clock, the labels, the tracks nor the output snapshot.
 *     Errors, all found before any device work, in this order.  SAMSIM_ERR_ARG: h, sel or n_match NULL.  SAMSIM_ERR_ABI: wrong
 *       struct_size.  SAMSIM_ERR_ARG: nterms out of range; per term in order a bad slot, reserved != 0, a NaN lo or hi; group < -1,
 *       group >= 0 without labels, or group >= ngroups; a status_mode outside the enum, or a non-zero code where the mode takes none;
 *       reserved != 0; max_out < 0, max_out > SAMSIM_SELECT_MAX_OUT, or max_out > 0 with cols_out NULL.
 *   samsim_get_columns.  The state of the columns cols[0 .. ncols), in the boundary's layout.
 *     Request.  s->ncol == ncols in 1..SAMSIM_SELECT_MAX_OUT, s->nlayer the handle's, s->narr SAMSIM_NPROG or SAMSIM_NARR.  Every cols[j]
 *       lies in [0, ncol); the whole list is checked on the host before any device work.  Any order is allowed, and so are duplicates.
 *     Result.  Position j of lay [narr][nlayer][ncols], scal [SAMSIM_NSCAL][ncols] and n_active [ncols] holds column cols[j]: exactly the
 *       bytes samsim_get_state returns for a one-column window at cols[j], the clamp S_abs >= 0 and the refreshed S_bu = S_abs/m
 *       included, under that function's conditions (after a step; status 0; the active layers; the clamp not in a column uploaded
 *       since the last step; the quotient where m != 0).  status, step and layer are [ncols] each or NULL and receive the entries
 *       samsim_get_status returns for those columns.
 *     No writes to the ensemble.  Clamp and quotient are formed in registers, as the track sampler forms them, so a column listed
 *       twice races with nothing; a later samsim_get_state still returns the same bytes, because it applies the same clamp.
 *     Staging.  The layer arrays pass through the staging buffer of samsim_get_state, in pieces of at most SAMSIM_STAGE_MAX_BYTES cut
 *       by the same rule (whole multiples of 64 list positions): at 1 024 layers SAMSIM_SELECT_MAX_OUT columns are far more than one piece.
 *     Errors, all found before any device work.  SAMSIM_ERR_ARG: h, cols or s NULL; the shape checks of samsim_get_state (a NULL array,
 *       a wrong nlayer or narr); ncols out of range or s->ncol != ncols; an index out of range.  Nothing is written to the caller's
 *       buffers when a call is refused.
 *     Tracers.  The tracer state is not part of this call: it stays with samsim_get_tracer_state.
 *   Device scratch of both calls: at most SAMSIM_SELECT_SCRATCH_BYTES whatever ncol and the request are (the waves' counts and
 *     offsets, and the index list); allocated on first use, kept in the handle, freed by samsim_destroy. */
#define SAMSIM_SELECT_MAX_TERMS 4
#define SAMSIM_SELECT_MAX_OUT   262144            /* indices per call, and columns per samsim_get_columns */
#define SAMSIM_SELECT_SCRATCH_BYTES (4ull << 20)  /* device scratch of both calls, whatever ncol and the request are */
enum samsim_select_status { SAMSIM_SELECT_RUNNING = 0,   /* status == 0: the columns the statistics count */
                            SAMSIM_SELECT_STOPPED,       /* status != 0 */
                            SAMSIM_SELECT_CODE,          /* status == code */
                            SAMSIM_SELECT_ANY };
typedef struct samsim_select_term { int32_t slot, reserved; double lo, hi; } samsim_select_term;   /* holds when lo <= x && x < hi */
typedef struct samsim_selection {
  int32_t struct_size;      /* = sizeof(samsim_selection) */
  int32_t nterms;           /* 0..SAMSIM_SELECT_MAX_TERMS; the terms are ANDed; 0 = no condition on values */
  int32_t group;            /* -1: any column; >= 0: only columns with that label (samsim_set_groups) */
  int32_t status_mode;      /* enum samsim_select_status */
  int32_t code;             /* SAMSIM_SELECT_CODE only, else 0 */
  int32_t reserved;         /* 0 */
  samsim_select_term terms[SAMSIM_SELECT_MAX_TERMS];
} samsim_selection;
int samsim_select_columns(samsim_handle *h, const samsim_selection *sel, int64_t max_out, int64_t *cols_out, int64_t *n_match);
int samsim_get_columns(samsim_handle *h, int64_t ncols, const int64_t *cols, samsim_state_soa *s,
                       int32_t *status, int64_t *step, int32_t *layer);

/* Column functionals: vertical integrals, extrema and crossing depths as slots.  Every reduction above consumes a slot, one
 * double[ncol] row; what a sea-ice user asks of a column is mostly a functional of its layer profile -- how thick the permeable part
 * of the ice is (psi_l >= 0.05), how deep the -5 degC isotherm lies, the mean salinity of the upper 0.5 m, the depth-integrated brine
 * volume, the largest Rayleigh number and where it sits.  samsim_set_functionals names up to SAMSIM_MAX_FUNCTIONALS of them; the
 * device evaluates each into a row of its own, and SAMSIM_FUNC_SLOT(i) is that row wherever a slot is accepted.  The entry points
 * below were added without a change of SAMSIM_ABI_VERSION (it stays 6): new symbols only, found by symbol as the group, histogram,
 * sensitivity, track and select functions are.  They read the state and write only their own rows.
 *
 *   Columns.  Every column c < ncol is evaluated, whatever its status, from the bytes samsim_get_state would return for it now:
 *     S_abs with the health check's clamp S_abs >= 0, and S_bu = S_abs/m where m != 0, under exactly that function's conditions (after a
 *     step; status 0; the clamp not in a column uploaded since the last step; the stored values elsewhere).  Clamp and quotient are
 *     formed in registers, as the track sampler forms them: nothing is written to the ensemble.  Na = n_active[c] clamped to
 *     [0, nlayer].  The consumers decide by status which columns count, as they do for every slot; a stopped column carries the value
 *     of the state it froze with (SAMSIM_SELECT_STOPPED / ANY read it).
 *   Depth.  Z_0 = 0, Z_k = Z_{k-1} + thick(k) by sequential double additions, k ascending; H = Z_Na.  origin is an enum
 *     samsim_profile_origin.  Layer k, 1 <= k <= Na, covers [lo_k, hi_k): FROM_TOP [Z_{k-1}, Z_k), FROM_BOTTOM [H - Z_k, H - Z_{k-1}).
 *     Window [z_lo, z_hi): z_lo >= 0 finite, z_hi > z_lo, z_hi = +inf allowed (the whole column).  With mn(x, y) = x < y ? x : y and
 *     mx(x, y) = x > y ? x : y:  e0_k = mx(lo_k, z_lo), e1_k = mn(hi_k, z_hi), o_k = e1_k - e0_k.  Layer k is IN THE WINDOW if and only
 *     if o_k > 0 (a layer of zero thickness never is, nor one whose edge only touches the window).  Snow is not part of the coordinate.
 *   Layer value.  a_k is the value of `array` (enum samsim_layer_array) in layer k as above.
 *   Condition (CROSSING_DEPTH and THICKNESS_WHERE only).  sense +1: a_k >= threshold.  sense -1: a_k < threshold.  A NaN satisfies
 *     neither.
 *   Kinds.  All sums run over the in-window layers in ascending k, from 0.0; products are rounded, then added; no fused multiply-add.
 *     SAMSIM_FN_INTEGRAL: W = sum o_k*a_k; 0.0 with no layer in the window.
 *     SAMSIM_FN_MEAN: W / L with L = sum o_k, one IEEE division.
 *     SAMSIM_FN_MIN / SAMSIM_FN_MAX: the extreme of a_k.  The first in-window a_k that is not a NaN begins it; a later a_k replaces it when
 *       a_k < min (a_k > max).  So the first attainment in ascending k is kept and a NaN never becomes an extreme.
 *     SAMSIM_FN_DEPTH_OF_MIN / SAMSIM_FN_DEPTH_OF_MAX: 0.5 * (lo_k + hi_k) of that layer: the sum is rounded, then halved; the layer's
 *       bounds are unclipped.
 *     SAMSIM_FN_CROSSING_DEPTH: e0_k = mx(lo_k, z_lo) of the first in-window layer, counted from the origin, in which the condition
 *       holds: the smallest such k FROM_TOP, the largest FROM_BOTTOM.
 *     SAMSIM_FN_THICKNESS_WHERE: sum o_k over the in-window layers in which the condition holds; 0.0 if there are none.
 *     missing: any double, NaN included: the value where MEAN, MIN, MAX, DEPTH_OF_* or CROSSING_DEPTH have no layer to speak of -- an
 *       empty window, Na == 0, only NaNs for the extremes, the condition never met.  With missing = -1 and v0 = 0, entry 0 of a
 *       histogram holds the columns in which it never happened, as with STEP_FIRST of the tracks.
 *     Every value is a fixed sequence of IEEE operations on the column's own data: a host reproduces it to the bit from samsim_get_state.
 *   When.  The rows are always current: they describe the state samsim_get_state would return now.  The library keeps a dirty flag,
 *     set by stepping, samsim_set_state, samsim_set_status and samsim_set_functionals; every entry point that resolves a
 *     SAMSIM_FUNC_SLOT, and samsim_get_functionals, evaluates first when the flag is set: one kernel on the handle's first stream,
 *     after the wait every getter makes.  Calls that use no functional slot launch nothing new.
 *   samsim_set_functionals.  n in 1..SAMSIM_MAX_FUNCTIONALS allocates [n][ncol] doubles on the device (64-bit offsets).  n == 0 with
 *     NULL removes them and frees the rows (also when none was set).  A call that is refused leaves the previous ones in force.  The
 *     specs belong to the caller, as the labels do: they are not part of a checkpoint; samsim_destroy frees the rows.
 *   samsim_get_functionals.  out[ncols] = the window [col0, col0 + ncols) of the row of functional `index`.
 *   Slots.  SAMSIM_FUNC_SLOT(i) with i < n of the functionals in force is accepted wherever a slot is -- samsim_get_ensemble_stats,
 *     samsim_get_group_stats, samsim_get_histogram, the slots of samsim_get_covariance, predictor_slot of
 *     samsim_get_profile_regression, the terms of samsim_select_columns -- and resolves to that row; without functionals, or out of
 *     range, it is the SAMSIM_ERR_ARG of any bad slot.  So the histogram of the permeable thickness per site is a
 *     samsim_get_histogram by group, the covariance of the isotherm depth with dT2m a samsim_get_covariance, and the members with no
 *     permeable layer at all a samsim_select_columns.
 *   Not in scope.  The tracks do not take a functional as an observable (enum samsim_observable_kind is closed), and the tracer state
 *     is not an array of this call.
 *   Errors, all found before any device work, in this order.  samsim_set_functionals: SAMSIM_ERR_ARG for h NULL; n outside
 *     0..SAMSIM_MAX_FUNCTIONALS; specs NULL with n > 0 (or not NULL with n == 0); then per spec in order: SAMSIM_ERR_ABI for a wrong
 *     struct_size; SAMSIM_ERR_ARG for a bad kind, array or origin; sense not +1 or -1 for the two kinds with a condition, or not 0 for
 *     the other kinds; a non-finite threshold with sense != 0; a non-finite or negative z_lo; a NaN z_hi or z_hi <= z_lo;
 *     reserved != 0.  SAMSIM_ERR_NOMEM if the rows cannot be allocated (the previous functionals stay).  samsim_get_functionals:
 *     SAMSIM_ERR_ARG for NULL pointers, no functionals set, index outside [0, n), a window outside [0, ncol); nothing is written to out
 *     when a call is refused. */
#define SAMSIM_MAX_FUNCTIONALS 8
#define SAMSIM_FUNC_SLOT(i) (0x20000 + (i))
enum samsim_functional_kind {
  SAMSIM_FN_INTEGRAL = 0, SAMSIM_FN_MEAN, SAMSIM_FN_MIN, SAMSIM_FN_MAX,
  SAMSIM_FN_DEPTH_OF_MIN, SAMSIM_FN_DEPTH_OF_MAX,
  SAMSIM_FN_CROSSING_DEPTH, SAMSIM_FN_THICKNESS_WHERE, SAMSIM_NFN };
typedef struct samsim_functional_spec {   /* 56 bytes */
  int32_t struct_size, kind, array, origin, sense, reserved;
  double  z_lo, z_hi, threshold, missing;
} samsim_functional_spec;
int samsim_set_functionals(samsim_handle *h, int32_t n, const samsim_functional_spec *specs);
int samsim_get_functionals(samsim_handle *h, int32_t index, int64_t col0, int64_t ncols, double *out /*[ncols]*/);

/* Sensors and the per-column misfit: the ensemble scored against observations.  Everything above describes the ensemble; a perturbed
 * ensemble is run to be held against data -- a thermistor string's temperatures, the bulk salinity of a core's sections, the ice
 * thickness and snow depth of a mass-balance buoy.  samsim_set_sensors names up to SAMSIM_MAX_SENSORS sensors; the device forms the
 * model's equivalent y_i of each per column (the observation operator), samsim_get_sensor_values returns it for a list of columns,
 * and samsim_score adds one weighted sum of squared differences per column against an observation vector to nine rows kept on the
 * device, over as many observation times as the run has.  SAMSIM_SCORE_SLOT(field) is such a row wherever a slot is accepted: the
 * histogram of the misfit, its statistics per site, its covariance with dT2m (the gradient a calibration follows), and
 * samsim_select_columns for the members under a misfit bound.  The entry points below were added without a change of
 * SAMSIM_ABI_VERSION (it stays 6): new symbols only, found by symbol as the functional functions are.  They read the state and write
 * only their own rows.
 *
 *   Columns.  Every column is evaluated, whatever its status, from the bytes samsim_get_state would return for it now: S_abs with
 *     the health check's clamp S_abs >= 0, and S_bu = S_abs/m where m != 0, under exactly that function's conditions (after a step;
 *     status 0; the clamp not in a column uploaded since the last step; the stored values elsewhere).  Clamp and quotient are formed in
 *     registers, as the functionals form them: nothing is written to the ensemble.  Na = n_active[c] clamped to [0, nlayer].
 *   Depth.  Z_0 = 0, Z_k = Z_{k-1} + thick(k) by sequential double additions, k ascending; H = Z_Na.  origin is an enum
 *     samsim_profile_origin.  Layer k, 1 <= k <= Na, covers [lo_k, hi_k): FROM_TOP [Z_{k-1}, Z_k), FROM_BOTTOM [H - Z_k, H - Z_{k-1}).
 *     Snow is not part of the coordinate.
 *   Layer value.  a_k is the value of array `id` (enum samsim_layer_array) in layer k as above.
 *   Kinds.
 *     SAMSIM_SENSOR_SCALAR: the stored slot `id` (enum samsim_scalar), e.g. the snow depth.  origin, interp and z must be 0.
 *     SAMSIM_SENSOR_ICE_THICKNESS: H (SAMSIM_S_THICKNESS holds the last output point's).  id, origin, interp and z must be 0.
 *     SAMSIM_SENSOR_PROFILE: array `id` at depth z >= 0, finite, measured from `origin`.  The containing layer is the smallest k in
 *       1..Na with lo_k <= z && z < hi_k (a layer of zero thickness never contains a sensor).  Without one -- the sensor lies below the
 *       ice, or Na == 0 -- y = missing and the sensor is NOT IN THE ICE for this column; SCALAR and ICE_THICKNESS sensors always are.
 *       SAMSIM_SENSOR_STEP: y = a_k.
 *       SAMSIM_SENSOR_LINEAR: between the midpoints c_k = 0.5 * (lo_k + hi_k) (the sum is rounded, then halved) of layer k and of its
 *         neighbour j on the side of z: where z >= c_k the adjacent layer with the next larger coordinate (k + 1 FROM_TOP, k - 1
 *         FROM_BOTTOM), else the one on the other side.  j outside 1..Na: y = a_k (constant in the outer half-layers).  Otherwise
 *         (c_a, a_a) is that of the two layers with the smaller coordinate -- FROM_TOP the one with the smaller index, FROM_BOTTOM the one
 *         with the larger -- and (c_b, a_b) the other; t = (z - c_a) / (c_b - c_a), one IEEE division; y = a_a + t * (a_b - a_a), the
 *         product rounded, then added, no fused multiply-add.  A neighbour of zero thickness takes part with its own midpoint; a zero
 *         denominator gives what IEEE gives.
 *     missing: any double, NaN included.
 *     Every value is a fixed sequence of IEEE operations on the column's own data: a host reproduces it to the bit from samsim_get_state.
 *   samsim_set_sensors.  n in 1..SAMSIM_MAX_SENSORS stores the specs and allocates the score rows [SAMSIM_NSF][ncol] as doubles on the
 *     device (64-bit offsets), all 0.0.  n == 0 with NULL removes sensors and rows (also when none was set).  A call that is refused
 *     leaves the previous sensors and rows in force.  Sensors and rows belong to the caller, as labels and tracks do: they are not
 *     part of a checkpoint; samsim_set_state, samsim_set_status, samsim_set_clock and stepping leave them alone; samsim_destroy frees
 *     them.
 *   samsim_get_sensor_values.  y[i][j] = the value of sensor i for column cols[j], y being [n][ncols].  The list rules are those of
 *     samsim_get_columns: ncols in 1..SAMSIM_SELECT_MAX_OUT, every index checked on the host first, any order, duplicates allowed.
 *     It writes nothing to the ensemble or to the rows.
 *   samsim_score.  A column is SCORED if its status is 0 and, with group >= 0, its label (samsim_set_groups) equals group; group == -1
 *     needs no labels.  For every other column no byte of any score row changes.  Sensor i is VALID for a scored column if and only if
 *     obs[i] is not a NaN and the sensor is in the ice; a NaN y_i of a valid sensor is not filtered (it makes J a NaN, which is
 *     information).  w_i = weight[i], or 1.0 when weight is NULL.  From N = J = B = W = 0.0, over the valid sensors in ascending i:
 *       d = y_i - obs[i];  N = N + 1;  J = J + w_i * (d * d) (d * d rounded, then the product with w_i rounded, then added);
 *       B = B + w_i * d;  W = W + w_i.
 *     Then, in this order: N_LAST, J_LAST, B_LAST, W_LAST = N, J, B, W; and if N > 0: N_SUM += N, J_SUM += J, B_SUM += B, W_SUM += W,
 *     CALLS += 1.  The RMS misfit sqrt(J_SUM / W_SUM) and the bias B_SUM / W_SUM are formed on the host.  No cross-lane arithmetic, no
 *     atomics: two calls on equal states give equal bytes, and a column's bytes do not depend on its neighbours.  One observation
 *     vector per call; a multi-site ensemble is scored site by site through `group`.
 *   samsim_get_scores / samsim_set_score_state.  The window [col0, col0 + ncols) of the nine rows, [SAMSIM_NSF][ncols], out of the
 *     handle and back into one (a restart, as samsim_get_tracks / samsim_set_track_state).  samsim_reset_scores sets every row to 0.0.
 *   Slots.  SAMSIM_SCORE_SLOT(field), field an enum samsim_score_field, is accepted wherever a slot is while sensors are set --
 *     samsim_get_ensemble_stats, samsim_get_group_stats, samsim_get_histogram, the slots of samsim_get_covariance, predictor_slot of
 *     samsim_get_profile_regression, the terms of samsim_select_columns -- and resolves to that row; without sensors, or with
 *     field >= SAMSIM_NSF, it is the SAMSIM_ERR_ARG of any bad slot.  There is no dirty flag: the rows change only in samsim_score,
 *     samsim_set_score_state and samsim_reset_scores.
 *   Not in scope.  The tracks do not take a sensor or a score as an observable (enum samsim_observable_kind is closed); sensors in the
 *     snow, the air or the ocean are simply not in the ice; tracers are not arrays of this call; one observation vector per call.
 *   Errors, all found before any device work, in this order; a call that is refused writes nothing to the caller's buffers or to the
 *     rows.  samsim_set_sensors: SAMSIM_ERR_ARG for h NULL; n outside 0..SAMSIM_MAX_SENSORS; specs NULL with n > 0 (or not NULL with
 *     n == 0); then per spec in order: SAMSIM_ERR_ABI for a wrong struct_size; SAMSIM_ERR_ARG for a bad kind; a bad id for the kind; a
 *     bad origin or interp; a non-zero id, origin, interp or z where the kind takes none; a non-finite or negative z; reserved != 0.
 *     SAMSIM_ERR_NOMEM if the rows cannot be allocated (the previous ones stay).  samsim_score: SAMSIM_ERR_ARG for h or obs NULL; no
 *     sensors set; a weight that is not finite or not > 0 in a position where obs is not a NaN; the group checks of
 *     samsim_get_covariance.  The others: SAMSIM_ERR_ARG for NULL pointers; no sensors set; a window outside [0, ncol); the list checks
 *     of samsim_get_columns. */
#define SAMSIM_MAX_SENSORS 32
#define SAMSIM_SCORE_SLOT(field) (0x30000 + (field))
enum samsim_sensor_kind { SAMSIM_SENSOR_PROFILE = 0, SAMSIM_SENSOR_SCALAR, SAMSIM_SENSOR_ICE_THICKNESS, SAMSIM_NSENSOR_KINDS };
enum samsim_sensor_interp { SAMSIM_SENSOR_STEP = 0, SAMSIM_SENSOR_LINEAR = 1 };
enum samsim_score_field {
  SAMSIM_SF_N_LAST = 0, SAMSIM_SF_J_LAST, SAMSIM_SF_B_LAST, SAMSIM_SF_W_LAST,
  SAMSIM_SF_N_SUM, SAMSIM_SF_J_SUM, SAMSIM_SF_B_SUM, SAMSIM_SF_W_SUM, SAMSIM_SF_CALLS, SAMSIM_NSF };
typedef struct samsim_sensor_spec {   /* 40 bytes */
  int32_t struct_size, kind, id, origin, interp, reserved;
  double  z, missing;
} samsim_sensor_spec;
int samsim_set_sensors(samsim_handle *h, int32_t n, const samsim_sensor_spec *specs);
int samsim_get_sensor_values(samsim_handle *h, int64_t ncols, const int64_t *cols, double *y /*[n][ncols]*/);
int samsim_score(samsim_handle *h, const double *obs /*[n]*/, const double *weight /*[n] or NULL*/, int32_t group);
int samsim_get_scores(samsim_handle *h, int64_t col0, int64_t ncols, double *out /*[SAMSIM_NSF][ncols]*/);
int samsim_set_score_state(samsim_handle *h, int64_t col0, int64_t ncols, const double *in /*[SAMSIM_NSF][ncols]*/);
int samsim_reset_scores(samsim_handle *h);

/* Posterior statistics: the ensemble weighted by its misfit, on the device.  A perturbed ensemble is scored to get the posterior --
 * the thickness, an isotherm depth, the melt-onset date GIVEN the buoy's data --, which is every diagnostic above taken with weights
 * w_c ~ exp(-J_c / 2).  samsim_set_weights forms one row w[ncol] of weights on the device from any slot; the two weighted reductions
 * read it, and SAMSIM_WEIGHT_SLOT is that row wherever a slot is accepted: the histogram of the weights, the members with w >= 0.01
 * through samsim_select_columns, the weight as the predictor of samsim_get_profile_regression (which gives the posterior mean of a
 * depth bin: sum w y / sum w = mean_y + cov / mean_x over the bin's contributing columns).  Nothing here writes to the ensemble:
 * the calls read slots, status and labels and write the weight row and their own scratch, as samsim_score writes only its rows.  The
 * entry points below were added without a change of SAMSIM_ABI_VERSION (it stays 6): new symbols only.
 *
 *   samsim_set_weights.  spec->slot is any slot the reductions accept (a scalar, SAMSIM_STAT_N_ACTIVE, a track row, a functional
 *     row -- refreshed first, as everywhere --, a score row) but not SAMSIM_WEIGHT_SLOT itself; x is the column's value of it.  A
 *     column is IN if its status is 0 and, with spec->group >= 0, its label (samsim_set_groups) equals group; group == -1 needs no
 *     labels.  Every column of the handle is written; a column that is not IN gets w = 0.0.
 *       SAMSIM_WEIGHT_DIRECT: w = x if x > 0 && x < +inf, else 0.0.  scale must be 0.
 *       SAMSIM_WEIGHT_GAUSS: x_min = the exact minimum of x over the IN columns whose x is not a NaN, reduced on the device;
 *         c = 0.5 / scale, one IEEE division on the host; t = (x - x_min) * c, the difference rounded, then the product (no fused
 *         multiply-add); w = t < 690.0 ? e(-t) : 0.0, where e is the library's fixed sequence of IEEE operations for the exponential
 *         (within 1 ulp of exp on [-690, 0], e(-0.0) == 1.0 exactly; a host that compiles the same sequence reproduces the row to the
 *         bit).  A NaN x or a NaN t gives 0.0.  scale = 1 with slot = SAMSIM_SCORE_SLOT(SAMSIM_SF_J_SUM) is the Gaussian likelihood of
 *         the accumulated misfit relative to the best member; scale > 1 tempers it.  A member with x == x_min has weight exactly 1.0.
 *         With no IN column that has a non-NaN x, x_min is reported as 0.0 and every weight is 0.0.  x_min of DIRECT is 0.0.
 *     info (or NULL): n_in = the number of IN columns, n_pos = the number with w > 0, sum_w and sum_w2 the sums of w and w * w over
 *     them in a fixed order; the effective sample size sum_w * sum_w / sum_w2 is formed on the host.
 *     Lifetime.  The row is allocated by the first successful call (doubles, 64-bit offsets); a later call replaces its contents;
 *     samsim_set_weights(h, NULL, NULL) frees it (also when none was set); a call that is refused leaves the previous row in force.
 *     There is no dirty flag: the row changes only in this call, as the score rows change only in samsim_score.  Stepping,
 *     samsim_set_state, samsim_set_status and samsim_set_clock leave it alone; it is not part of a checkpoint; samsim_destroy frees it.
 *   samsim_get_weights.  The window [col0, col0 + ncols) of the row.
 *   Slots.  While the row exists SAMSIM_WEIGHT_SLOT is accepted wherever a slot is; without it, it is the SAMSIM_ERR_ARG of any bad
 *     slot.
 *   samsim_get_weighted_stats.  nslots in 1..SAMSIM_SENS_MAX_SLOTS.  A column COUNTS if its status is 0, its label passes `group` as
 *     above, and w > 0.  Per slot: count, sum_w = sum of w and sum_w2 = sum of w * w over the counting columns, mean = sum w x / sum w,
 *     var = sum w (x - mean)^2 / sum w (the reliability-weighted population variance), min and max exact over the counting columns.
 *     Mean and var are formed from deviations, never as sum w x^2 - ...: in a lane West's update W += w; d = x - mean;
 *     mean += d * (w / W); M2 += w * d * (x - mean); across lanes and waves the weighted pairwise merge with the cross term
 *     delta^2 W_a W_b / W, in a fixed order.  count == 0: every double is 0.0.  Columns with identical x give mean == x and
 *     var == 0.0 exactly.  Two calls on the same state return the same bytes; relabelling columns outside `group` changes nothing.
 *   samsim_get_weighted_histogram.  Edges and the entry of a value are exactly those of samsim_get_histogram (a NaN lands in entry 0,
 *     the guessed bin is corrected against the rounded edges); wsum[i] is the sum of w over the counting columns that land in entry
 *     i, wsum being [nvbins + 2].  One group per call.  The order of summation is fixed: within a wave in ascending column order,
 *     then the waves' tables in wave order.
 *   Scratch: at most SAMSIM_WEIGHT_SCRATCH_BYTES of device memory for the three calls whatever ncol is, allocated on first use and
 *     freed by samsim_destroy.
 *   Not in scope.  Resampling or any write to the ensemble; all groups in one call; weights in checkpoint files.  (Weighted profile
 *     statistics and weighted covariances are the two entry points of the next block.)
 *   Errors, all found before any device work, in this order; a call that is refused writes nothing to the caller's buffers.
 *     samsim_set_weights: SAMSIM_ERR_ARG for h NULL; with spec NULL: info not NULL is SAMSIM_ERR_ARG, else the row is removed;
 *     SAMSIM_ERR_ABI for a wrong struct_size; SAMSIM_ERR_ARG for a bad kind; a bad slot or SAMSIM_WEIGHT_SLOT; the group checks of
 *     samsim_get_covariance; DIRECT with scale != 0; GAUSS with a scale that is not finite or not > 0; reserved != 0.
 *     SAMSIM_ERR_NOMEM if the row cannot be allocated.  samsim_get_weights: SAMSIM_ERR_ARG for NULL pointers; no row; a window
 *     outside [0, ncol).  samsim_get_weighted_stats: SAMSIM_ERR_ARG for NULL pointers; nslots outside 1..SAMSIM_SENS_MAX_SLOTS; a bad
 *     slot; no row; the group checks.  samsim_get_weighted_histogram: the checks of samsim_get_histogram in its order, without
 *     by_group; no row; the group checks. */
#define SAMSIM_WEIGHT_SLOT 0x40000
#define SAMSIM_WEIGHT_SCRATCH_BYTES (4ull << 20)   /* of which 2 MiB are the 1 024 waves' tables of 256 doubles */
enum samsim_weight_kind { SAMSIM_WEIGHT_DIRECT = 0, SAMSIM_WEIGHT_GAUSS = 1 };
typedef struct samsim_weight_spec {   /* 32 bytes */
  int32_t struct_size, kind, slot, group;
  double  scale, reserved;
} samsim_weight_spec;
typedef struct samsim_weight_info {   /* 40 bytes */
  int64_t n_in, n_pos;
  double  x_min, sum_w, sum_w2;
} samsim_weight_info;
typedef struct samsim_wstat {         /* 56 bytes */
  int64_t count;
  double  sum_w, sum_w2, mean, var, min, max;
} samsim_wstat;
int samsim_set_weights(samsim_handle *h, const samsim_weight_spec *spec, samsim_weight_info *info /* or NULL */);
int samsim_get_weights(samsim_handle *h, int64_t col0, int64_t ncols, double *out /*[ncols]*/);
int samsim_get_weighted_stats(samsim_handle *h, int32_t nslots, const int32_t *slots, int32_t group, samsim_wstat *out /*[nslots]*/);
int samsim_get_weighted_histogram(samsim_handle *h, int32_t slot, const samsim_hist_bins *vb, int32_t group,
                                  double *wsum /*[nvbins + 2]*/);

/* Posterior profiles and posterior sensitivities: the weight row applied to the layer profiles and to the joint moments of the
 * column scalars.  samsim_get_weighted_profile_stats is samsim_get_profile_stats with weights -- per depth bin the posterior mean of
 * T(z), S_bu(z) or psi_l(z) with its variance, its extremes and the sums from which the effective sample size of the bin follows --,
 * samsim_get_weighted_covariance is samsim_get_covariance with weights: how the thickness co-varies with dT2m GIVEN the buoy's data.
 * Both are read-only reductions: they read slots, status, labels, the layer block and the weight row and write only their own
 * scratch.  The entry points below were added without a change of SAMSIM_ABI_VERSION (it stays 6): new symbols only.
 *
 *   Columns (both).  A column COUNTS as in samsim_get_weighted_stats: its status is 0, its label passes `group` (-1: every label, no
 *     labels needed; >= 0: only that label of samsim_set_groups), and its weight w > 0.  One group per call.
 *   samsim_get_weighted_profile_stats.  rq is a request of samsim_get_profile_stats with any narrays; out[narrays][nbins].  The bins,
 *     the layer value a_k and the per-column bin value v are exactly those of that function, and a counting column contributes to a
 *     bin under exactly that function's condition (BY_LAYER: the layer exists; BY_DEPTH: L_b > 0); a column that does not count
 *     behaves like a stopped one.  Per (array, bin), over the counting columns that contribute: count, sum_w = sum of w,
 *     sum_w2 = sum of w * w, mean = sum w v / sum w, var = sum w (v - mean)^2 / sum w, min and max exact.  The contributing columns
 *     differ from bin to bin, so sum_w and sum_w2 are per-bin results; the effective sample size of a bin, sum_w^2 / sum_w2, is
 *     formed on the host.  With count == 0 every double is 0.0.  A request is served in passes of one array and at most 64 bins, as
 *     samsim_get_profile_stats is.
 *     Arithmetic.  The walk, the grid, the chunks and the wave order are those of samsim_get_profile_stats.  A wave folds the bin's
 *     values of one 64-column block in column order: mean_b = ref + (sum w_i (v_i - ref)) / (sum w_i) around the first counting value
 *     ref, then M2_b = sum w_i * (d_i * d_i), d_i = v_i - mean_b, in a second walk; blocks and then waves are merged in a fixed
 *     order by Chan's update with the total weight W in the place of the count: fb = W_b / W, mean += delta * fb,
 *     M2 += M2_b + delta * delta * (W_a * fb); var = M2 / W.  No fused multiply-add, no atomics, a grid fixed by ncol alone.
 *     Properties.  Two calls on the same state return the same bytes; relabelling or re-weighting columns outside `group` changes
 *     nothing.  Columns that hold identical v in a bin give mean == v == min == max and var == 0.0 exactly, whatever the weights.
 *     When every counting column has w == 1.0, count, mean, min and max are the bytes of samsim_get_profile_stats for the same
 *     request (samsim_get_group_profile_stats with a group), sqrt(var) is its std bytes, and sum_w == sum_w2 == (double)count:
 *     every product with w is then exact and every W an exactly represented integer.
 *   samsim_get_weighted_covariance.  nslots in 1..SAMSIM_SENS_MAX_SLOTS; the slots are those samsim_get_weighted_stats accepts
 *     (functional rows are refreshed first; SAMSIM_WEIGHT_SLOT itself is allowed; a slot may appear twice).  count, sum_w and sum_w2
 *     over the counting columns; mean[i] = sum w x_i / sum w; cov[i][j] = sum w (x_i - mean_i)(x_j - mean_j) / sum w, the diagonal
 *     the weighted variance.  One triangle is computed and mirrored: cov[i][j] and cov[j][i] are the same bytes.  With count == 0
 *     every output is 0.0.
 *     Arithmetic.  One walk serves all slots.  In a lane West's update of samsim_get_weighted_stats for the means and
 *     C_ij += w * d_i * (x_j - mean_j), d_i = x_i - mean_i before the update and mean_j after it; across lanes and waves the weighted
 *     pairwise merge with the cross term delta_i delta_j W_a W_b / W, in the order of samsim_get_weighted_stats.  No atomics.
 *     Properties.  Two calls return the same bytes; relabelling columns outside `group` changes nothing.  A slot listed twice gives
 *     cov[i][j] == cov[i][i] == cov[j][j] bitwise.  Identical columns give covariances of exactly 0.0.  mean[i] and cov[i][i] are
 *     the mean and var bytes of samsim_get_weighted_stats for the same slots and group, and count, sum_w and sum_w2 are its bytes
 *     too; a slot has the bytes it would have alone.  The correlations are formed on the host (cov / sqrt(var_i var_j)).
 *   Like every getter the calls wait for the handle's streams; they change neither the state, the status, the clock, the output
 *     snapshot, the labels, the tracks, the scores nor the weight row.
 *   Scratch.  samsim_get_weighted_covariance stays within SAMSIM_WEIGHT_SCRATCH_BYTES (its partials lie where those of the weighted
 *     moments do).  samsim_get_weighted_profile_stats: at most SAMSIM_WPROFILE_SCRATCH_BYTES of device memory whatever ncol and the
 *     request are (the waves' partials of one pass, then the results); allocated on first use, freed by samsim_destroy.
 *   Not in scope.  All groups in one call; resampling or any write to the ensemble; weights in checkpoint files.  (The weighted
 *     joint histogram of a profile is the entry point of the next block.)
 *   Errors, all found before any device work, in this order; a call that is refused writes nothing to the caller's buffers.
 *     samsim_get_weighted_profile_stats: SAMSIM_ERR_ARG for h, rq or out NULL; every check of samsim_get_profile_stats, in its order;
 *     no weight row; the group checks of samsim_get_covariance.  samsim_get_weighted_covariance: SAMSIM_ERR_ARG for any NULL pointer;
 *     nslots outside 1..SAMSIM_SENS_MAX_SLOTS; a bad slot; no weight row; the group checks. */
#define SAMSIM_WPROFILE_SCRATCH_BYTES (4ull << 20)   /* 3.5 MiB of partials (1 024 waves x 64 bins x 56 bytes), then the results */
int samsim_get_weighted_profile_stats(samsim_handle *h, const samsim_profile_request *rq, int32_t group,
                                      samsim_wstat *out /*[narrays][nbins]*/);
int samsim_get_weighted_covariance(samsim_handle *h, int32_t nslots, const int32_t *slots, int32_t group,
                                   int64_t *count, double *sum_w, double *sum_w2,
                                   double *mean /*[nslots]*/, double *cov /*[nslots][nslots]*/);

/* Posterior bands: the weight row applied to the joint histogram of a layer profile.  samsim_get_weighted_profile_histogram is
 * samsim_get_profile_histogram with weights -- per depth bin and value entry the sum of the weights of the columns that land there
 * --, from which the posterior median and the 5-95 % band of T(z), S_bu(z) or psi_l(z) follow on the host as quantile brackets per
 * depth bin: the summary of a skewed, bounded posterior that mean and variance are not.  A read-only reduction: it reads status,
 * labels, the layer block and the weight row and writes only its own scratch.  The entry point was added without a change of
 * SAMSIM_ABI_VERSION (it stays 6): a new symbol only.
 *
 *   Request.  rq is a request of samsim_get_profile_stats with narrays == 1; wsum[rq->nbins][nvbins+2].  The bins, the layer value
 *     a_k (the layer value of samsim_get_state with clamp = false and adjust = true, see "Layer value"), the per-column bin value v
 *     and the condition under which a column contributes to a bin are exactly those of samsim_get_profile_histogram for the same rq;
 *     the edges and the entry of a value are exactly those of samsim_get_histogram (a NaN lands in entry 0, the guessed bin is
 *     corrected against the rounded edges).
 *   Columns.  A column COUNTS as in samsim_get_weighted_profile_stats: its status is 0, its label passes `group` (-1: every column,
 *     no labels needed; >= 0: only that label of samsim_set_groups; one group per call), and its weight w > 0.  A column that does
 *     not count behaves like a stopped one.
 *   Result.  wsum[b][i] is the sum of w over the counting columns that contribute to bin b and whose bin value lands in entry i.
 *   Passes.  A request is served in passes of `chunk` depth bins, each a walk over the layers of every column as in the profile
 *     statistics: passes = ceil(nbins / chunk), chunk = min(64, 64 512 / (8 * (65 + ((nvbins + 2) | 1)))) -- the walk's tile
 *     [chunk][65], the lanes' masks, the block's 64 weights and the wave's table [chunk][(nvbins + 2) | 1] of doubles share the
 *     64 KiB of LDS of a workgroup --: 64 up to 59 value bins, 30 at 200, 25 at SAMSIM_HIST_MAX_VBINS.
 *   Order of summation, fixed.  A pass runs G = min(ceil(ncol / 64), 512) one-wave workgroups; wave g owns the 64-column blocks
 *     g, g + G, ...  In a block lane j owns depth bin j of the pass and walks row j of the tile over the 64 columns, so within a wave
 *     the weights of an entry are added in ascending column order.  Then the waves' tables are added per (bin, entry) in wave
 *     order with one bracket: lane l of the merge takes the waves [l * per, (l + 1) * per), per = ceil(G / 64), ascending, then
 *     the 64 lanes ascending.  No atomics of any kind; a plain sum, so no fused multiply-add either; the grid and the chunk are fixed
 *     by ncol and nvbins alone.
 *   Properties.  (1) Two calls on the same state return the same bytes.  (2) Relabelling or re-weighting columns outside `group`
 *     changes nothing.  (3) When every counting column has w == 1.0, wsum is (double)counts of samsim_get_profile_histogram for the
 *     same request and group, bit for bit; with integer-valued weights every entry is exact.  (4) wsum[b][i] > 0 exactly where at
 *     least one counting column lands in (b, i) -- the weights are positive, so no sum of them is 0 --; every other entry is +0.0.
 *     (5) A row's bytes do not depend on how many bins the request has: rows [0, k) of a from-top request with nbins = k are the
 *     first k rows of the same request with a larger nbins.  (6) The entries of row b sum to sum_w of bin b of
 *     samsim_get_weighted_profile_stats to within the rounding of the two orders of summation, and the lowest and the highest entry
 *     of positive weight contain that call's min and max.
 *   Like every getter the call waits for the handle's streams; it changes neither the state, the status, the clock, the output
 *     snapshot, the labels, the tracks, the scores nor the weight row.
 *   Scratch: at most SAMSIM_WPHIST_SCRATCH_BYTES of device memory whatever ncol and the request are -- the waves' tables of one pass,
 *     G x chunk x (nvbins + 2) doubles (every pass reuses them), then the result, at most 1 024 x 256 doubles --; allocated on first
 *     use, kept in the handle, freed by samsim_destroy.
 *   Not in scope.  All groups in one call; more than one array per call; exact quantiles; resampling or any write to the ensemble;
 *     weights in checkpoint files; the Fortran host's namelist.
 *   Errors, all found before any device work, in this order; a call that is refused writes nothing to wsum.  SAMSIM_ERR_ARG for h,
 *     rq, vb or wsum NULL; every check of samsim_get_profile_histogram in its order, through the vb checks (every check of
 *     samsim_get_profile_stats; narrays != 1; the vb checks); no weight row; the group checks of samsim_get_covariance. */
#define SAMSIM_WPHIST_SCRATCH_BYTES (32ull << 20)   /* 25 MiB of tables (512 waves x 25 bins x 256 doubles), then 2 MiB of result */
int samsim_get_weighted_profile_histogram(samsim_handle *h, const samsim_profile_request *rq, const samsim_hist_bins *vb,
                                          int32_t group, double *wsum /*[rq->nbins][vb->nvbins + 2]*/);

/* Posterior draws: the ensemble resampled by its weights, indices only.  A scored ensemble run as a particle filter drops the members
 * the data rule out and continues from copies of the ones they support; samsim_resample says which members to continue from and how
 * many copies of each, without a download of the weight row.  It is a read-only reduction like its predecessors: it reads the weight
 * row, status and the labels and writes two rows of its own -- per column the number of offspring, per draw the ancestor's column
 * index -- and its scratch.  Moving state stays with samsim_get_columns (which takes the ancestor list, duplicates allowed) and
 * samsim_set_state.  The entry points were added without a change of SAMSIM_ABI_VERSION (it stays 6): new symbols only.
 *
 *   Columns.  A column COUNTS as in samsim_get_weighted_stats: its status is 0, its label passes `group` (-1: every column, no
 *     labels needed; >= 0: only that label of samsim_set_groups; one group per call), and its weight w > 0.  Its term is w; the
 *     term of a column that does not count is +0.0.
 *   The cumulative weight C_c: the inclusive prefix sum of the terms in ascending column order, in one bracketing.  The nblk =
 *     ceil(ncol / 64) 64-column blocks are cut into G = ceil(nblk / per) contiguous ranges of per = ceil(nblk / 1024) blocks (the
 *     grid rule of samsim_select_columns: range order is column order).  Inside range g the local sum L_c runs sequentially, column
 *     after column, from 0.0; T_g is the range's last L; B_0 = 0.0 and B_{g+1} = B_g + T_g, sequentially; C_c = B_g + L_c; W = B_G,
 *     which is the last column's C by construction.  With this bracketing C does not decrease in c in floating point (a tree-shaped
 *     scan inside a block would not guarantee that).  No fused multiply-add anywhere.
 *   The draw coordinate: t_c = (C_c / W) * m, one IEEE division, then one product; t_{-1} = 0.  The last counting column has
 *     t == m exactly.
 *   The point count K(t), the number of draw points below t: K(t) = m if t >= m; else
 *       SAMSIM_RESAMPLE_SYSTEMATIC (points u0 + k): K(t) = min(max(ceil(t - u0), 0), m), the difference rounded;
 *       SAMSIM_RESAMPLE_STRATIFIED (points k + u(k)): f = floor(t), K(t) = f + (u(f) < t - f), with u(k) = (mix(seed, k) >> 11) * 2^-53
 *         and mix the splitmix64 finaliser of seed + (k + 1) * 0x9E3779B97F4A7C15: z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 *         z *= 0x94D049BB133111EB, z ^= z >> 31, in wrapping 64-bit arithmetic.
 *     Both K do not decrease in t.
 *   Offspring and ancestors.  N_c = K(t_c) - K(t_{c-1}) is the column's number of offspring, stored as a double in the offspring row
 *     [ncol]; its copies are ancestors[K(t_{c-1}) .. K(t_c)).  The ancestor list is ascending and has exactly m entries; a column
 *     that does not count never appears in it.  m may be below, equal to or above the number of columns.
 *   No draw.  W == 0 or W not finite: every offspring is 0, m_drawn = 0, sum_w reports W, and the call returns 0.
 *   info (may be NULL).  n_pos the counting columns, sum_w = W, m_drawn the entries of the ancestor list (m, or 0), n_survivors the
 *     columns with N_c >= 1, max_offspring the largest N_c and argmax_offspring the lowest column index that has it (0 without a
 *     draw).  All integer reductions; no atomics of any kind.
 *   Lifetime.  The offspring row (doubles, ncol) and the ancestor list (int64, grown to the largest m asked for) are allocated by the
 *     first successful call; a later call replaces their contents; samsim_resample(h, NULL, NULL) or samsim_destroy frees them.
 *     Stepping, uploads and samsim_set_weights leave the rows alone, and there is no dirty flag: the rows describe the weights as
 *     they were at the call.  They are not part of a checkpoint.  A call that is refused leaves the previous rows in force and writes
 *     nothing to the caller's buffers.
 *   samsim_get_offspring takes windows inside [0, ncol), samsim_get_ancestors windows inside [0, m_drawn) of the last call.
 *   Slot.  While the offspring row exists SAMSIM_OFFSPRING_SLOT is accepted wherever a slot is -- the survivors through
 *     samsim_select_columns on offspring >= 1, the histogram of the family sizes, the survivors per site through the group
 *     statistics --; without it, it is the SAMSIM_ERR_ARG of any bad slot.
 *   Properties.  Two calls return the same bytes; the sum of the offspring row is m_drawn; relabelling columns outside `group`
 *     changes nothing; |N_c - m w_c / W| is at most 1 (SYSTEMATIC) and below 2 (STRATIFIED) up to the rounding of C.
 *   Scratch: SAMSIM_RESAMPLE_SCRATCH_BYTES of device memory whatever ncol and m are -- the ranges' sums, bases and integer partials,
 *     then the result --, allocated on first use and freed by samsim_destroy; the two rows are not counted in it.
 *   Not in scope.  Any write to the ensemble: putting the copies where the dropped members were is samsim_apply_resample, below;
 *     multinomial or residual resampling; a draw across the handles of several ranks (each rank resamples its own shard; a global
 *     draw needs the ranks' W, which info returns); the Fortran host's namelist.
 *   Errors, all found before any device work, in this order.  samsim_resample: SAMSIM_ERR_ARG for h NULL; with spec NULL: info not
 *     NULL is SAMSIM_ERR_ARG, else the rows are removed (also when there are none); SAMSIM_ERR_ABI for a wrong struct_size;
 *     SAMSIM_ERR_ARG for a bad kind; no weight row; the group checks of samsim_get_covariance; m outside
 *     1..SAMSIM_RESAMPLE_MAX_DRAWS; SYSTEMATIC with u0 outside [0, 1) or a NaN, or with seed != 0; STRATIFIED with u0 != 0;
 *     reserved != 0; SAMSIM_ERR_NOMEM if a row cannot be allocated.  samsim_get_offspring, samsim_get_ancestors: SAMSIM_ERR_ARG for
 *     NULL pointers; no rows; a window outside the range. */
#define SAMSIM_OFFSPRING_SLOT 0x50000
#define SAMSIM_RESAMPLE_MAX_DRAWS 4194304
#define SAMSIM_RESAMPLE_SCRATCH_BYTES (64ull << 10)   /* partials only; a constant whatever ncol and m are */
enum samsim_resample_kind { SAMSIM_RESAMPLE_SYSTEMATIC = 0, SAMSIM_RESAMPLE_STRATIFIED = 1 };
typedef struct samsim_resample_spec {   /* 40 bytes */
  int32_t struct_size, kind, group, reserved;
  int64_t m;          /* draws, 1..SAMSIM_RESAMPLE_MAX_DRAWS */
  double  u0;         /* SYSTEMATIC: the offset, 0 <= u0 < 1; STRATIFIED: must be 0 */
  uint64_t seed;      /* STRATIFIED: the seed of the per-draw offsets; SYSTEMATIC: must be 0 */
} samsim_resample_spec;
typedef struct samsim_resample_info {   /* 48 bytes */
  int64_t n_pos, m_drawn, n_survivors, max_offspring, argmax_offspring;
  double  sum_w;
} samsim_resample_info;
int samsim_resample(samsim_handle *h, const samsim_resample_spec *spec, samsim_resample_info *info /* or NULL */);
int samsim_get_offspring(samsim_handle *h, int64_t col0, int64_t ncols, double *out /*[ncols]*/);
int samsim_get_ancestors(samsim_handle *h, int64_t k0, int64_t nk, int64_t *out /*[nk]*/);

/* Applying a resample on the device: whole columns copied in place.  The step that makes the scored, weighted and resampled ensemble
 * a particle filter: the copies of the members the data support go where the members they rule out were.  Through the host that is
 * samsim_get_columns of the ancestors followed by samsim_set_state, both bound by a copy through pageable host memory and the first
 * by SAMSIM_SELECT_MAX_OUT columns a call; here the data never leave the device.  The step kernel is not touched, nothing is written
 * but what the call names, and every result is defined as the bytes of a route that already exists.  The entry points were added
 * without a change of SAMSIM_ABI_VERSION (it stays 6): new symbols only.
 *
 *   samsim_copy_columns: entry k overwrites column dst[k] with column src[k], 1 <= n <= ncol.  Afterwards every getter returns for
 *     dst[k] what it would return after this route through the host, on the same handle:
 *       1. samsim_get_columns(src) with narr = SAMSIM_NARR, then samsim_set_state at dst[k];
 *       2. samsim_set_status with the status, step and layer samsim_get_columns reported for the source: a copy of a stopped column
 *          is a stopped column;
 *       3. with tracers: samsim_get_tracer_state(src), then samsim_set_tracer_state(dst); the concentration below stays with the slot;
 *       4. with SAMSIM_COPY_TRACKS: samsim_get_tracks, then samsim_set_track_state, for every track; with SAMSIM_COPY_SCORES:
 *          samsim_get_scores, then samsim_set_score_state.
 *     So of the destination: every layer of the fifteen public arrays becomes the layer value samsim_get_columns forms for the source
 *     (S_abs with the clamp and S_bu as the quotient over the active layers of a running source once the kernel has run, the stored
 *     element otherwise); the scalars below SAMSIM_S_DT2M, N_active, status, step and layer are the source's; the next step of the
 *     column runs the full first sweep, exactly as after samsim_set_state (the hand-over block of the up sweep is not copied, as
 *     samsim_set_state does not write it); the functionals are evaluated again before their next use.  Not written: the work
 *     counters, the labels, the weight row, the offspring row, the ancestor list, the output window, and every column that is not a
 *     destination.  Sources are only read.  Without SAMSIM_COPY_FORCING the scalars from SAMSIM_S_DT2M on, the forcing set of
 *     samsim_set_forcing_sites and the two rows of samsim_set_ocean stay with the slot, as with samsim_set_state; with it they are
 *     copied where they exist, so that a parameter ensemble keeps each particle's parameters.
 *     Duplicate sources are allowed: one source feeding many destinations is the normal case.
 *   samsim_apply_resample: the pair list from the offspring row N of the last samsim_resample, on the device, then the copy.
 *       The POOL is the columns with status 0 now whose label passes the group of that samsim_resample call.
 *       free   = the pool columns with N_c == 0, ascending;
 *       copies = for each column in ascending order, N_c - 1 entries of that column's index where N_c >= 2;
 *       entry k of the plan is (src = copies[k], dst = free[k]).
 *     Survivors keep their slot, no source is a destination, and the copy is in place: there is no second buffer.  dst ascends
 *     strictly and src does not descend.  The plan BALANCES when n_free == n_copies -- which needs m_drawn == n_pool: a resample
 *     with m other than the pool size cannot be applied in place -- and no column with N_c >= 1 has left the pool since the draw.
 *     A plan that does not balance is refused with SAMSIM_ERR_UNSUPPORTED by its counting pass, before any column is written:
 *     nothing of the ensemble changes, the stored plan stays and info is not written.  n_copies == 0 (unit weights) returns 0 and
 *     writes nothing of the ensemble.  A successful call marks the rows as applied: a second call without a samsim_resample in
 *     between is refused, because after steps it would silently copy again.
 *     info (may be NULL): n_pool the pool, n_free and n_copies the two lists' lengths (equal), n_sources the columns with N_c >= 2.
 *   samsim_get_copy_plan: windows inside [0, n_copies) of the plan of the last successful samsim_apply_resample; it is refused
 *     before the first.  samsim_copy_columns does not change the stored plan, and neither does a call that is refused.
 *   Properties.  Two handles given the same calls hold the same bytes; no atomics and no hand-off between workgroups; the plan is
 *     an ordered compaction like samsim_select_columns (count, one-wave scan, write), the totals come back in one small copy.
 *   Device memory, allocated on first use and freed by samsim_destroy: SAMSIM_COPY_SCRATCH_BYTES for the plan's counts, two int64
 *     rows of ncol for the lists of samsim_copy_columns and two more for the stored plan.
 *   Not in scope.  Jitter of the copies' state (their parameters: samsim_jitter, below); a copy across the handles of several ranks; the plan and the applied mark
 *     in checkpoint files; copying the hand-over block or the raw flags (the copy enters through the restart path on purpose).
 *   Errors, all found before any device work, in this order; a call that is refused writes nothing.  samsim_copy_columns, each
 *     SAMSIM_ERR_ARG: h, src or dst NULL; n outside 1..ncol; `what` with unknown bits; SAMSIM_COPY_TRACKS without tracks, then
 *     SAMSIM_COPY_SCORES without sensors; an index outside [0, ncol); a dst listed twice; a column that is both a dst and a src.
 *     samsim_apply_resample, each SAMSIM_ERR_ARG: h NULL; the checks of `what` as above; no resample rows; rows already applied; the
 *     labels of the draw's group removed since.
 *     samsim_get_copy_plan, each SAMSIM_ERR_ARG: h, src or dst NULL; no plan applied yet; a window outside [0, n_copies).
 *     SAMSIM_ERR_NOMEM if a list cannot be allocated. */
#define SAMSIM_COPY_FORCING 1   /* the perturbation slots >= SAMSIM_S_DT2M, the site index, the two ocean rows */
#define SAMSIM_COPY_TRACKS  2   /* all SAMSIM_NTF rows of every track set                                        */
#define SAMSIM_COPY_SCORES  4   /* all SAMSIM_NSF score rows                                                     */
#define SAMSIM_COPY_SCRATCH_BYTES (64ull << 10)   /* the plan's partials only; a constant whatever ncol is */
typedef struct samsim_apply_info {   /* 32 bytes */
  int64_t n_pool, n_free, n_copies, n_sources;
} samsim_apply_info;
int samsim_copy_columns(samsim_handle *h, int64_t n, const int64_t *src /*[n]*/, const int64_t *dst /*[n]*/, int32_t what);
int samsim_apply_resample(samsim_handle *h, int32_t what, samsim_apply_info *info /* or NULL */);
int samsim_get_copy_plan(samsim_handle *h, int64_t k0, int64_t nk, int64_t *src /*[nk]*/, int64_t *dst /*[nk]*/);

/* Rejuvenation: the per-column parameters jittered on the device.  The model is deterministic: what tells member c from member c' is
 * its perturbation -- the slots SAMSIM_S_DT2M and SAMSIM_S_PRECIP_SCALE and the two rows of samsim_set_ocean.  After
 * samsim_apply_resample with SAMSIM_COPY_FORCING a member drawn five times is five identical columns that stay identical, so every
 * resample cycle lowers the number of distinct members and nothing raises it again.  samsim_jitter is the kernel-shrinkage step of
 * Liu and West (2001) on those rows: each value is pulled towards a centre and moved by a normal deviate that belongs to the column.
 * Through the host that is samsim_get_state of the scalar rows, noise drawn there and samsim_set_forcing_sites with the tables again;
 * here the rows never leave the device.  The step kernel is not touched; the new parameters take effect at the next step (the kernel
 * reads the two slots every step and the ocean rows at the head of every launch).  New symbols only: SAMSIM_ABI_VERSION stays 6.
 *
 *   Rows.  SAMSIM_JT_DT2M and SAMSIM_JT_PRECIP_SCALE are the scalar rows of those names, SAMSIM_JT_DFL_Q_BOTTOM and
 *     SAMSIM_JT_S_BU_BOTTOM the first and the second row of samsim_set_ocean; a target whose row does not exist is refused.
 *   Which columns are written.  The POOL is the columns with status 0 now whose label passes `group` (-1: every column, no labels
 *     needed).  SAMSIM_JITTER_POOL writes every pool column.  SAMSIM_JITTER_COPIES writes, of the destination list of the last
 *     successful samsim_apply_resample (the stored plan), the columns whose status is 0 now; group must be -1, the plan carries the
 *     group of its draw.  Sources and survivors keep their values: only the duplicates move.  Every other column keeps its bytes.
 *   The normal deviate eps of (seed, column c, target t), Marsaglia's polar method on a counter-based stream: for attempt
 *     a = 0, 1, ... < SAMSIM_JITTER_MAX_ATTEMPTS, k = (c << 8) | (t << 6) | (a << 1), x = 2 * ((mix(seed, k) >> 11) * 2^-53) - 1 and y
 *     the same from k | 1 (both exact), s = x*x + y*y (two rounded products, the rounded sum); mix is the splitmix64 finaliser of
 *     seed + (k + 1) * 0x9E3779B97F4A7C15, the mixer of SAMSIM_RESAMPLE_STRATIFIED.  The first attempt with 0 < s < 1 is taken and
 *     eps = x * sqrt((-2.0 * log(s)) / s): the library's own logarithm (a fixed sequence of fused multiply-adds and one IEEE
 *     quotient, ~1e-16 absolute), one rounded product, one IEEE division, the correctly rounded square root, one product.  Without an
 *     accepted attempt (probability (1 - pi/4)^32 ~ 4e-22) eps = 0.  The key is the target, not the position of the term, and the
 *     column, not the thread: the deviate of a column does not depend on `which`, `group`, ncol, the other terms or the grid.
 *   The new value of term i for theta = row[c]: v = centre + shrink * (theta - centre) (the difference is rounded, then the product,
 *     then the sum); v = v + sigma * eps (the product is rounded, then the sum); if v < lo then v = lo and the column counts in
 *     n_lo[i], else if v > hi then v = hi and the column counts in n_hi[i].  A NaN compares false twice and is written as a NaN.
 *     Nothing is fused.  For Liu and West's step with the discount delta: a = (3 delta - 1) / (2 delta), centre the mean of the row
 *     over the pool, shrink = a, sigma = sqrt(1 - a * a) * the row's standard deviation (samsim_get_covariance gives both).
 *   info (may be NULL): n_written the columns written, the same for every term; n_lo and n_hi per term.  Integer reductions in the
 *     style of the copy plan: the workgroups' counts from wave ballots, a one-wave merge, one small copy; no atomics.
 *   Not written: anything but the named rows -- not the state, status, clock, work counters, output snapshot, labels, tracks,
 *     scores, weight row, offspring row or the stored plan; the functionals are not marked stale (none reads a parameter).
 *   Properties.  Two handles given the same calls hold the same bytes.  The call is enqueued on the handle's first stream and
 *     returns when the totals have arrived.
 *   Device memory, allocated on first use and freed by samsim_destroy: SAMSIM_JITTER_SCRATCH_BYTES for the counts.
 *   Not in scope.  Jitter of the state itself (enthalpy, salt and mass have to stay consistent); per-column physical parameters
 *     beyond the four rows; the jittered rows in checkpoint files (samsim_get_state and samsim_get_ocean return all four).
 *   Errors, all found before any device work, in this order; a call that is refused writes nothing.  SAMSIM_ERR_ARG for h or spec
 *     NULL; SAMSIM_ERR_ABI for a wrong struct_size; SAMSIM_ERR_ARG for a bad `which`, then nterms outside 1..4; then per term, in
 *     order, each SAMSIM_ERR_ARG: a bad target; a target listed twice; reserved != 0; a non-finite centre, shrink or sigma; shrink
 *     outside [0, 1]; sigma < 0; a NaN bound or lo > hi (infinite bounds are allowed); lo < 0 for SAMSIM_JT_S_BU_BOTTOM
 *     (samsim_set_ocean refuses a negative salinity).  Then SAMSIM_ERR_ARG for a target whose ocean row is not set; with POOL the
 *     group checks of samsim_get_covariance; with COPIES SAMSIM_ERR_ARG for group != -1, then for no plan applied yet; a plan with
 *     n_copies == 0 returns 0 with n_written == 0.
 *
 *   samsim_get_ocean: the window [col0, col0 + ncols) of the rows of samsim_set_ocean (either pointer may be NULL).
 *     SAMSIM_ERR_ARG for h NULL, a requested row that is not set, or a window outside [0, ncol).
 *   SAMSIM_OCEAN_SLOT(i), i = 0 the flux offset and i = 1 the salinity below, is accepted wherever a slot is while that row exists:
 *     the posterior of an ocean parameter comes from the reductions that exist. */
#define SAMSIM_JITTER_MAX_TERMS 4
#define SAMSIM_JITTER_MAX_ATTEMPTS 32
#define SAMSIM_JITTER_SCRATCH_BYTES (320ull << 10)   /* the ranges' counts only; a constant whatever ncol is */
#define SAMSIM_OCEAN_SLOT(i) (0x60000 + (i))
enum samsim_jitter_target { SAMSIM_JT_DT2M = 0, SAMSIM_JT_PRECIP_SCALE, SAMSIM_JT_DFL_Q_BOTTOM, SAMSIM_JT_S_BU_BOTTOM };
enum samsim_jitter_which  { SAMSIM_JITTER_POOL = 0, SAMSIM_JITTER_COPIES = 1 };
typedef struct samsim_jitter_term {   /* 48 bytes */
  int32_t target, reserved;
  double centre, shrink, sigma, lo, hi;
} samsim_jitter_term;
typedef struct samsim_jitter_spec {   /* 216 bytes */
  int32_t struct_size, which, group, nterms;
  uint64_t seed;
  samsim_jitter_term term[SAMSIM_JITTER_MAX_TERMS];
} samsim_jitter_spec;
typedef struct samsim_jitter_info {   /* 72 bytes */
  int64_t n_written, n_lo[SAMSIM_JITTER_MAX_TERMS], n_hi[SAMSIM_JITTER_MAX_TERMS];
} samsim_jitter_info;
int samsim_jitter(samsim_handle *h, const samsim_jitter_spec *spec, samsim_jitter_info *info /* or NULL */);
int samsim_get_ocean(samsim_handle *h, int64_t col0, int64_t ncols, double *dfl_q_bottom /*[ncols] or NULL*/,
                     double *S_bu_bottom /*[ncols] or NULL*/);

void samsim_destroy(samsim_handle *h);
const char *samsim_strerror(int code);
int samsim_abi_version(void);
int samsim_device_count(void);

enum samsim_error {
  SAMSIM_OK = 0,
  SAMSIM_ERR_ARG = -1, SAMSIM_ERR_UNSUPPORTED = -2, SAMSIM_ERR_HIP = -3, SAMSIM_ERR_NO_DEVICE = -4,
  SAMSIM_ERR_NO_OUTPUT = -5, SAMSIM_ERR_ABI = -6, SAMSIM_ERR_NOMEM = -7
};

#ifdef __cplusplus
}
#endif
#endif /* SAMSIM_H */
