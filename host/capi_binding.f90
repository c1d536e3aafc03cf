!> iso_c_binding view of the C-ABI in include/samsim.h (libsamsim_hip.so).
!! This is the stub a maintainer of the reference adds on the Fortran side (see INTEGRATION.md): the derived types
!! mirror `samsim_config`, `samsim_state_soa`, `samsim_clock`, `samsim_output_soa` field by field.
MODULE mo_samsim_capi
  USE, INTRINSIC :: iso_c_binding
  IMPLICIT NONE
  PUBLIC

  ! enum samsim_layer_array (0-based in C, used 1-based here: index = value + 1)
  INTEGER, PARAMETER :: A_H_ABS = 1, A_S_ABS = 2, A_M = 3, A_THICK = 4, A_T = 5, A_PHI = 6, A_PSI_S = 7, A_PSI_L = 8, &
                        A_PSI_G = 9, A_S_BU = 10, A_S_BR = 11, A_RAY = 12, A_PERM = 13, A_FLUSH_V = 14, A_FLUSH_H = 15, &
                        SAMSIM_NARR = 15, SAMSIM_NPROG = 4
  ! enum samsim_scalar (index = value + 1)
  INTEGER, PARAMETER :: S_M_SNOW = 1, S_H_ABS_SNOW = 2, S_S_ABS_SNOW = 3, S_THICK_SNOW = 4, S_PSI_S_SNOW = 5, &
                        S_PSI_L_SNOW = 6, S_PSI_G_SNOW = 7, S_T_SNOW = 8, S_PHI_S = 9, S_T_TOP = 10, S_MELT_THICK = 11, &
                        S_T2M = 12, S_LIQUID_PRECIP = 13, S_SOLID_PRECIP = 14, S_FL_Q_BOTTOM = 15, S_GRAV_DRAIN = 16, &
                        S_GRAV_SALT = 17, S_GRAV_TEMP = 18, S_MELT_OUT1 = 19, S_MELT_OUT2 = 20, S_MELT_OUT3 = 21, &
                        S_MELT_ERR = 22, S_FREEBOARD = 23, S_T_FREEZE = 24, S_ALBEDO = 25, S_FL_SW = 26, S_FL_LW = 27, &
                        S_MELT_THICK_SNOW = 28, S_FL_Q_SNOW = 29, S_ENERGY_STORED = 30, S_FRESHWATER = 31, &
                        S_TOTAL_RESIST = 32, S_THICKNESS = 33, S_BULK_SALIN = 34, S_FL_REST = 35, S_S_BU_BOTTOM = 36, S_DT2M = 37, &
                        S_PRECIP_SCALE = 38, &
                        SAMSIM_NSCAL = 38

  TYPE, BIND(C) :: samsim_config
     INTEGER(c_int32_t) :: struct_size, testcase, nlayer, n_top, n_middle, n_bottom
     INTEGER(c_int32_t) :: atmoflux_flag, grav_flag, prescribe_flag, grav_heat_flag, flush_heat_flag, turb_flag, salt_flag, &
                           boundflux_flag, flush_flag, flood_flag, bottom_flag, debug_flag, precip_flag, harmonic_flag, &
                           tank_flag, albedo_flag, lab_snow_flag, freeboard_snow_flag, snow_flush_flag, snow_precip_flag, &
                           bgc_flag, i_time_out
     REAL(c_double)     :: dt, thick_0, thick_min, T_bottom, S_bu_bottom, k_snow_flush, max_flux_plate, time_out, time_total
     REAL(c_double)     :: alpha_flux_instable, alpha_flux_stable, m_total, S_total
  END TYPE samsim_config

  TYPE, BIND(C) :: samsim_state_soa
     INTEGER(c_int64_t) :: ncol
     INTEGER(c_int32_t) :: nlayer, narr
     TYPE(c_ptr)        :: lay, scal, n_active
  END TYPE samsim_state_soa

  TYPE, BIND(C) :: samsim_clock
     REAL(c_double)     :: time
     INTEGER(c_int64_t) :: step
     INTEGER(c_int32_t) :: n_time_out, time_counter
     INTEGER(c_int64_t) :: n_outputs
  END TYPE samsim_clock

  TYPE, BIND(C) :: samsim_output_soa
     INTEGER(c_int64_t) :: ncols
     INTEGER(c_int32_t) :: nlayer, reserved
     TYPE(c_ptr)        :: lay, scal, n_active
     REAL(c_double)     :: time
     INTEGER(c_int64_t) :: step
  END TYPE samsim_output_soa

  TYPE, BIND(C) :: samsim_stat               ! samsim_stat: ensemble statistics of one per-column scalar
     INTEGER(c_int64_t) :: count
     REAL(c_double)     :: mean, min, max, std
  END TYPE

  ! samsim_get_profile_stats (ABI 6): enum samsim_profile_axis / samsim_profile_origin and the request
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_PROFILE_BY_LAYER = 0, SAMSIM_PROFILE_BY_DEPTH = 1, &
                                   SAMSIM_PROFILE_FROM_TOP = 0, SAMSIM_PROFILE_FROM_BOTTOM = 1
  INTEGER, PARAMETER :: SAMSIM_PROFILE_MAX_BINS = 1024, SAMSIM_PROFILE_MAX_ARRAYS = 8
  TYPE, BIND(C) :: samsim_profile_request
     INTEGER(c_int32_t) :: struct_size, axis, origin, nbins, narrays
     INTEGER(c_int32_t) :: arrays(SAMSIM_PROFILE_MAX_ARRAYS)     ! enum samsim_layer_array values (0-based)
     REAL(c_double)     :: z0, dz                                ! depth axis only, metres
  END TYPE samsim_profile_request

  ! samsim_get_histogram / samsim_get_profile_histogram: the value bins, edges E_j = v0 + j*dv, j = 0..nvbins; a row of counts has nvbins + 2 entries
  INTEGER, PARAMETER :: SAMSIM_HIST_MAX_VBINS = 254
  TYPE, BIND(C) :: samsim_hist_bins
     INTEGER(c_int32_t) :: struct_size, nvbins
     REAL(c_double)     :: v0, dv
  END TYPE samsim_hist_bins

  ! samsim_get_covariance / samsim_get_profile_regression: joint population moments of a predictor x and a value y
  INTEGER, PARAMETER :: SAMSIM_SENS_MAX_SLOTS = 8
  TYPE, BIND(C) :: samsim_pair_stat
     INTEGER(c_int64_t) :: count
     REAL(c_double)     :: mean_x, mean_y, var_x, var_y, cov
  END TYPE samsim_pair_stat

  ! samsim_set_tracks: enum samsim_observable_kind, enum samsim_track_field (0-based rows of a track) and the description of one track
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_OBS_SCALAR = 0, SAMSIM_OBS_N_ACTIVE = 1, SAMSIM_OBS_ICE_THICKNESS = 2, &
                                   SAMSIM_OBS_BULK_SALINITY = 3, SAMSIM_OBS_LAYER = 4
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_TF_N = 0, SAMSIM_TF_LAST = 1, SAMSIM_TF_MEAN = 2, SAMSIM_TF_M2 = 3, SAMSIM_TF_MIN = 4, &
                                   SAMSIM_TF_STEP_MIN = 5, SAMSIM_TF_MAX = 6, SAMSIM_TF_STEP_MAX = 7, SAMSIM_TF_N_HOLD = 8, &
                                   SAMSIM_TF_STEP_FIRST = 9, SAMSIM_TF_STEP_LAST = 10, SAMSIM_NTF = 11
  INTEGER, PARAMETER :: SAMSIM_MAX_TRACKS = 8
  TYPE, BIND(C) :: samsim_track_spec
     INTEGER(c_int32_t) :: struct_size, kind, id, layer, sense, reserved
     REAL(c_double)     :: threshold
  END TYPE samsim_track_spec

  ! samsim_select_columns / samsim_get_columns: enum samsim_select_status, one term (holds when lo <= x < hi) and the selection
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_SELECT_RUNNING = 0, SAMSIM_SELECT_STOPPED = 1, SAMSIM_SELECT_CODE = 2, SAMSIM_SELECT_ANY = 3
  INTEGER, PARAMETER :: SAMSIM_SELECT_MAX_TERMS = 4, SAMSIM_SELECT_MAX_OUT = 262144
  TYPE, BIND(C) :: samsim_select_term
     INTEGER(c_int32_t) :: slot, reserved                        ! slot 0-based, -1 = N_active, or samsim_track_slot
     REAL(c_double)     :: lo, hi
  END TYPE samsim_select_term
  TYPE, BIND(C) :: samsim_selection
     INTEGER(c_int32_t) :: struct_size, nterms, group, status_mode, code, reserved
     TYPE(samsim_select_term) :: terms(SAMSIM_SELECT_MAX_TERMS)
  END TYPE samsim_selection

  ! samsim_set_functionals: enum samsim_functional_kind and the description of one functional of a column's layer profile
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_FN_INTEGRAL = 0, SAMSIM_FN_MEAN = 1, SAMSIM_FN_MIN = 2, SAMSIM_FN_MAX = 3, &
                                   SAMSIM_FN_DEPTH_OF_MIN = 4, SAMSIM_FN_DEPTH_OF_MAX = 5, SAMSIM_FN_CROSSING_DEPTH = 6, &
                                   SAMSIM_FN_THICKNESS_WHERE = 7
  INTEGER, PARAMETER :: SAMSIM_MAX_FUNCTIONALS = 8
  TYPE, BIND(C) :: samsim_functional_spec
     INTEGER(c_int32_t) :: struct_size, kind, array, origin, sense, reserved   ! array: enum samsim_layer_array (0-based)
     REAL(c_double)     :: z_lo, z_hi, threshold, missing
  END TYPE samsim_functional_spec

  ! samsim_set_sensors: enum samsim_sensor_kind, enum samsim_sensor_interp, the description of one sensor, and enum
  ! samsim_score_field, the rows of the per-column misfit
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_SENSOR_PROFILE = 0, SAMSIM_SENSOR_SCALAR = 1, SAMSIM_SENSOR_ICE_THICKNESS = 2
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_SENSOR_STEP = 0, SAMSIM_SENSOR_LINEAR = 1
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_SF_N_LAST = 0, SAMSIM_SF_J_LAST = 1, SAMSIM_SF_B_LAST = 2, SAMSIM_SF_W_LAST = 3, &
                                   SAMSIM_SF_N_SUM = 4, SAMSIM_SF_J_SUM = 5, SAMSIM_SF_B_SUM = 6, SAMSIM_SF_W_SUM = 7, &
                                   SAMSIM_SF_CALLS = 8
  INTEGER, PARAMETER :: SAMSIM_MAX_SENSORS = 32, SAMSIM_NSF = 9
  TYPE, BIND(C) :: samsim_sensor_spec
     INTEGER(c_int32_t) :: struct_size, kind, id, origin, interp, reserved   ! id: enum samsim_layer_array or samsim_scalar (0-based)
     REAL(c_double)     :: z, missing
  END TYPE samsim_sensor_spec

  ! samsim_set_weights: the weight row as a slot, enum samsim_weight_kind, how the row is formed and what the call reports of it;
  ! samsim_get_weighted_stats: the weighted moments of one slot
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_WEIGHT_SLOT = 262144_c_int32_t
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_WEIGHT_DIRECT = 0, SAMSIM_WEIGHT_GAUSS = 1
  TYPE, BIND(C) :: samsim_weight_spec
     INTEGER(c_int32_t) :: struct_size, kind, slot, group          ! slot 0-based, -1 = N_active, or samsim_*_slot; group -1 = any
     REAL(c_double)     :: scale, reserved
  END TYPE samsim_weight_spec
  TYPE, BIND(C) :: samsim_weight_info
     INTEGER(c_int64_t) :: n_in, n_pos
     REAL(c_double)     :: x_min, sum_w, sum_w2
  END TYPE samsim_weight_info
  TYPE, BIND(C) :: samsim_wstat
     INTEGER(c_int64_t) :: count
     REAL(c_double)     :: sum_w, sum_w2, mean, var, min, max
  END TYPE samsim_wstat

  ! samsim_resample: the offspring row as a slot, enum samsim_resample_kind, the draw and what the call reports of it (Fortran has
  ! no unsigned kind: seed carries the bits of the uint64_t)
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_OFFSPRING_SLOT = 327680_c_int32_t
  INTEGER(c_int64_t), PARAMETER :: SAMSIM_RESAMPLE_MAX_DRAWS = 4194304_c_int64_t
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_RESAMPLE_SYSTEMATIC = 0, SAMSIM_RESAMPLE_STRATIFIED = 1
  TYPE, BIND(C) :: samsim_resample_spec
     INTEGER(c_int32_t) :: struct_size, kind, group, reserved      ! group -1 = any
     INTEGER(c_int64_t) :: m
     REAL(c_double)     :: u0
     INTEGER(c_int64_t) :: seed
  END TYPE samsim_resample_spec
  TYPE, BIND(C) :: samsim_resample_info
     INTEGER(c_int64_t) :: n_pos, m_drawn, n_survivors, max_offspring, argmax_offspring
     REAL(c_double)     :: sum_w
  END TYPE samsim_resample_info

  ! samsim_copy_columns / samsim_apply_resample: what is copied beside the state, and what the plan reports
  INTEGER(c_int32_t), PARAMETER :: SAMSIM_COPY_FORCING = 1, SAMSIM_COPY_TRACKS = 2, SAMSIM_COPY_SCORES = 4
  TYPE, BIND(C) :: samsim_apply_info
     INTEGER(c_int64_t) :: n_pool, n_free, n_copies, n_sources
  END TYPE samsim_apply_info

  INTERFACE
     INTEGER(c_int) FUNCTION samsim_create(cfg, ncol, device, h) BIND(C, name='samsim_create')
       IMPORT
       TYPE(samsim_config), INTENT(in) :: cfg
       INTEGER(c_int64_t), VALUE :: ncol
       INTEGER(c_int32_t), VALUE :: device
       TYPE(c_ptr), INTENT(out) :: h
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_set_forcing(h, len, fl_sw, fl_lw, T2m, precip, dT2m_col, precip_scale_col) &
          BIND(C, name='samsim_set_forcing')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: len
       REAL(c_double), INTENT(in) :: fl_sw(*), fl_lw(*), T2m(*), precip(*)
       TYPE(c_ptr), VALUE :: dT2m_col, precip_scale_col
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_set_forcing_sites(h, nsites, len, fl_sw, fl_lw, T2m, precip, site_of_column, dT2m_col, &
          precip_scale_col) BIND(C, name='samsim_set_forcing_sites')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: nsites, len
       REAL(c_double), INTENT(in) :: fl_sw(*), fl_lw(*), T2m(*), precip(*)      ! (len, nsites)
       INTEGER(c_int32_t), INTENT(in) :: site_of_column(*)                      ! 0-based
       TYPE(c_ptr), VALUE :: dT2m_col, precip_scale_col
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_set_state(h, s, col0) BIND(C, name='samsim_set_state')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_state_soa), INTENT(in) :: s
       INTEGER(c_int64_t), VALUE :: col0
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_get_state(h, s, col0) BIND(C, name='samsim_get_state')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_state_soa), INTENT(inout) :: s
       INTEGER(c_int64_t), VALUE :: col0
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_set_clock(h, c) BIND(C, name='samsim_set_clock')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_clock), INTENT(in) :: c
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_get_clock(h, c) BIND(C, name='samsim_get_clock')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_clock), INTENT(out) :: c
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_step(h, nsteps) BIND(C, name='samsim_step')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: nsteps
     END FUNCTION
     INTEGER(c_int64_t) FUNCTION samsim_steps_to_output(h) BIND(C, name='samsim_steps_to_output')
       IMPORT
       TYPE(c_ptr), VALUE :: h
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_set_output_window(h, col0, ncols) BIND(C, name='samsim_set_output_window')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: col0, ncols
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_get_output(h, o) BIND(C, name='samsim_get_output')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_output_soa), INTENT(inout) :: o
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_get_status(h, status, step, layer) BIND(C, name='samsim_get_status')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), INTENT(out) :: status(*)
       INTEGER(c_int64_t), INTENT(out) :: step(*)
       INTEGER(c_int32_t), INTENT(out) :: layer(*)
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_set_ocean(h, dfl_q_bottom_col, S_bu_bottom_col) BIND(C, name='samsim_set_ocean')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(c_ptr), VALUE :: dfl_q_bottom_col, S_bu_bottom_col   ! [ncol] each, or c_null_ptr
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_set_status(h, status, step, layer, col0, ncols) BIND(C, name='samsim_set_status')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), INTENT(in) :: status(*)
       INTEGER(c_int64_t), INTENT(in) :: step(*)
       INTEGER(c_int32_t), INTENT(in) :: layer(*)
       INTEGER(c_int64_t), VALUE :: col0, ncols
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_set_tracers(h, n_bgc, bgc_bottom, bgc_total) BIND(C, name='samsim_set_tracers')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: n_bgc
       REAL(c_double), INTENT(in) :: bgc_bottom(*)
       TYPE(c_ptr), VALUE :: bgc_total                    ! [n_bgc] with tank_flag 2, else c_null_ptr
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_set_tracer_state(h, bgc_abs, col0, ncols) BIND(C, name='samsim_set_tracer_state')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       REAL(c_double), INTENT(in) :: bgc_abs(*)           ! (ncols, nlayer, n_bgc), column fastest
       INTEGER(c_int64_t), VALUE :: col0, ncols
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_set_tracer_bottom(h, bgc_bottom, col0, ncols) BIND(C, name='samsim_set_tracer_bottom')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       REAL(c_double), INTENT(in) :: bgc_bottom(*)        ! (ncols, n_bgc), column fastest
       INTEGER(c_int64_t), VALUE :: col0, ncols
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_get_tracer_state(h, bgc_abs, bgc_bottom, col0, ncols) BIND(C, name='samsim_get_tracer_state')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       REAL(c_double), INTENT(out) :: bgc_abs(*), bgc_bottom(*)
       INTEGER(c_int64_t), VALUE :: col0, ncols
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_get_tracer_output(h, bgc_abs, bgc_bottom) BIND(C, name='samsim_get_tracer_output')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       REAL(c_double), INTENT(out) :: bgc_abs(*), bgc_bottom(*)
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_get_ensemble_stats(h, nslots, slots, out) BIND(C, name='samsim_get_ensemble_stats')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: nslots
       INTEGER(c_int32_t), INTENT(in) :: slots(*)        ! enum samsim_scalar values (0-based), -1 = N_active
       TYPE(samsim_stat), INTENT(out) :: out(*)
     END FUNCTION
     !> statistics of the layer profiles per layer or per depth bin; out(nbins, narrays), bin fastest (ABI 6)
     INTEGER(c_int) FUNCTION samsim_get_profile_stats(h, rq, out) BIND(C, name='samsim_get_profile_stats')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_profile_request), INTENT(in) :: rq
       TYPE(samsim_stat), INTENT(out) :: out(*)
     END FUNCTION
     !> a group label per column, -1 = in no group (0-based labels below ngroups); ngroups = 0 with c_null_ptr removes the labels
     INTEGER(c_int) FUNCTION samsim_set_groups(h, ngroups, group_of_column) BIND(C, name='samsim_set_groups')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: ngroups
       TYPE(c_ptr), VALUE :: group_of_column             ! int32 [ncol], or c_null_ptr
     END FUNCTION
     !> the statistics of samsim_get_ensemble_stats per group; out(ngroups, nslots), group fastest
     INTEGER(c_int) FUNCTION samsim_get_group_stats(h, nslots, slots, out) BIND(C, name='samsim_get_group_stats')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: nslots
       INTEGER(c_int32_t), INTENT(in) :: slots(*)        ! enum samsim_scalar values (0-based), -1 = N_active
       TYPE(samsim_stat), INTENT(out) :: out(*)
     END FUNCTION
     !> samsim_get_profile_stats over the columns with label group (0-based); out(nbins, narrays)
     INTEGER(c_int) FUNCTION samsim_get_group_profile_stats(h, rq, group, out) BIND(C, name='samsim_get_group_profile_stats')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_profile_request), INTENT(in) :: rq
       INTEGER(c_int32_t), VALUE :: group
       TYPE(samsim_stat), INTENT(out) :: out(*)
     END FUNCTION
     !> fixed-edge histogram of a per-column scalar (slot 0-based, -1 = N_active); counts(nvbins+2), with by_group = 1 counts(nvbins+2, ngroups)
     INTEGER(c_int) FUNCTION samsim_get_histogram(h, slot, vb, by_group, counts) BIND(C, name='samsim_get_histogram')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: slot
       TYPE(samsim_hist_bins), INTENT(in) :: vb
       INTEGER(c_int32_t), VALUE :: by_group
       INTEGER(c_int64_t), INTENT(out) :: counts(*)
     END FUNCTION
     !> joint histogram over depth bin x value bin of one layer array (rq%narrays = 1); group -1 = every column; counts(nvbins+2, nbins)
     INTEGER(c_int) FUNCTION samsim_get_profile_histogram(h, rq, vb, group, counts) BIND(C, name='samsim_get_profile_histogram')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_profile_request), INTENT(in) :: rq
       TYPE(samsim_hist_bins), INTENT(in) :: vb
       INTEGER(c_int32_t), VALUE :: group
       INTEGER(c_int64_t), INTENT(out) :: counts(*)
     END FUNCTION
     !> count, means and population covariance matrix of up to SAMSIM_SENS_MAX_SLOTS per-column scalars (slots 0-based, -1 = N_active)
     !! over the columns with status 0 (group -1) or with that 0-based label as well; mean(nslots), cov(nslots, nslots) (symmetric)
     INTEGER(c_int) FUNCTION samsim_get_covariance(h, nslots, slots, group, count, mean, cov) BIND(C, name='samsim_get_covariance')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: nslots
       INTEGER(c_int32_t), INTENT(in) :: slots(*)
       INTEGER(c_int32_t), VALUE :: group
       INTEGER(c_int64_t), INTENT(out) :: count
       REAL(c_double), INTENT(out) :: mean(*), cov(*)
     END FUNCTION
     !> per bin of a profile request the joint moments of the bin value and the scalar predictor_slot (0-based, -1 = N_active);
     !! group -1 = every column; out(nbins, narrays), bin fastest
     INTEGER(c_int) FUNCTION samsim_get_profile_regression(h, rq, predictor_slot, group, out) BIND(C, name='samsim_get_profile_regression')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_profile_request), INTENT(in) :: rq
       INTEGER(c_int32_t), VALUE :: predictor_slot, group
       TYPE(samsim_pair_stat), INTENT(out) :: out(*)
     END FUNCTION
     !> follow ntracks observables of every column through the run, sampled after each step that brings the step count to a multiple
     !! of every; ntracks = 0 with c_null_ptr removes tracking
     INTEGER(c_int) FUNCTION samsim_set_tracks(h, ntracks, specs, every) BIND(C, name='samsim_set_tracks')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: ntracks
       TYPE(c_ptr), VALUE :: specs                       ! samsim_track_spec [ntracks] (c_loc of a TARGET array), or c_null_ptr
       INTEGER(c_int64_t), VALUE :: every
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_reset_tracks(h) BIND(C, name='samsim_reset_tracks')
       IMPORT
       TYPE(c_ptr), VALUE :: h
     END FUNCTION
     !> the rows of one track (0-based) for the columns [col0, col0+ncols): out(ncols, SAMSIM_NTF), column fastest
     INTEGER(c_int) FUNCTION samsim_get_tracks(h, track, col0, ncols, out) BIND(C, name='samsim_get_tracks')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: track
       INTEGER(c_int64_t), VALUE :: col0, ncols
       REAL(c_double), INTENT(out) :: out(*)
     END FUNCTION
     !> restart: puts back what samsim_get_tracks returned (after samsim_set_tracks)
     INTEGER(c_int) FUNCTION samsim_set_track_state(h, track, col0, ncols, in) BIND(C, name='samsim_set_track_state')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: track
       INTEGER(c_int64_t), VALUE :: col0, ncols
       REAL(c_double), INTENT(in) :: in(*)
     END FUNCTION
     !> the 0-based indices of the columns a selection holds for, ascending: cols_out(max_out) receives the first min(n_match, max_out),
     !! n_match the exact number of matches
     INTEGER(c_int) FUNCTION samsim_select_columns(h, sel, max_out, cols_out, n_match) BIND(C, name='samsim_select_columns')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_selection), INTENT(in) :: sel
       INTEGER(c_int64_t), VALUE :: max_out
       INTEGER(c_int64_t), INTENT(out) :: cols_out(*)
       INTEGER(c_int64_t), INTENT(out) :: n_match
     END FUNCTION
     !> the state of the columns cols(1:ncols) (0-based indices, any order), position j holding column cols(j); s%ncol = ncols;
     !! status, step, layer: c_loc of arrays of ncols entries, or c_null_ptr
     INTEGER(c_int) FUNCTION samsim_get_columns(h, ncols, cols, s, status, step, layer) BIND(C, name='samsim_get_columns')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: ncols
       INTEGER(c_int64_t), INTENT(in) :: cols(*)
       TYPE(samsim_state_soa), INTENT(inout) :: s
       TYPE(c_ptr), VALUE :: status, step, layer
     END FUNCTION
     !> evaluate n functionals of every column's layer profile on the device: samsim_func_slot(i) is then a slot of the ensemble
     !! reductions, always current; n = 0 with c_null_ptr removes them
     INTEGER(c_int) FUNCTION samsim_set_functionals(h, n, specs) BIND(C, name='samsim_set_functionals')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: n
       TYPE(c_ptr), VALUE :: specs                       ! samsim_functional_spec [n] (c_loc of a TARGET array), or c_null_ptr
     END FUNCTION
     !> the value of functional index (0-based) in the columns [col0, col0+ncols)
     INTEGER(c_int) FUNCTION samsim_get_functionals(h, index, col0, ncols, out) BIND(C, name='samsim_get_functionals')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: index
       INTEGER(c_int64_t), VALUE :: col0, ncols
       REAL(c_double), INTENT(out) :: out(*)
     END FUNCTION
     !> name n sensors and allocate the score rows [SAMSIM_NSF][ncol], all zero: samsim_score_slot(field) is then a slot of the
     !! ensemble reductions; n = 0 with c_null_ptr removes sensors and rows
     INTEGER(c_int) FUNCTION samsim_set_sensors(h, n, specs) BIND(C, name='samsim_set_sensors')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: n
       TYPE(c_ptr), VALUE :: specs                       ! samsim_sensor_spec [n] (c_loc of a TARGET array), or c_null_ptr
     END FUNCTION
     !> y [n][ncols] (C order): the value of every sensor for the columns cols (0-based, any order, duplicates allowed)
     INTEGER(c_int) FUNCTION samsim_get_sensor_values(h, ncols, cols, y) BIND(C, name='samsim_get_sensor_values')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: ncols
       INTEGER(c_int64_t), INTENT(in) :: cols(*)
       REAL(c_double), INTENT(out) :: y(*)
     END FUNCTION
     !> add the weighted squared differences against obs [n] (NaN: no observation) to the score rows of the running columns --
     !! group >= 0: of those with that label --; weight [n] (c_loc) or c_null_ptr for 1.0
     INTEGER(c_int) FUNCTION samsim_score(h, obs, weight, group) BIND(C, name='samsim_score')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       REAL(c_double), INTENT(in) :: obs(*)
       TYPE(c_ptr), VALUE :: weight
       INTEGER(c_int32_t), VALUE :: group
     END FUNCTION
     !> the window [col0, col0 + ncols) of the score rows, out [SAMSIM_NSF][ncols] (C order)
     INTEGER(c_int) FUNCTION samsim_get_scores(h, col0, ncols, out) BIND(C, name='samsim_get_scores')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: col0, ncols
       REAL(c_double), INTENT(out) :: out(*)
     END FUNCTION
     !> restart: put back what samsim_get_scores returned for that window
     INTEGER(c_int) FUNCTION samsim_set_score_state(h, col0, ncols, rows) BIND(C, name='samsim_set_score_state')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: col0, ncols
       REAL(c_double), INTENT(in) :: rows(*)
     END FUNCTION
     !> every score row back to 0.0
     INTEGER(c_int) FUNCTION samsim_reset_scores(h) BIND(C, name='samsim_reset_scores')
       IMPORT
       TYPE(c_ptr), VALUE :: h
     END FUNCTION
     !> form the weight row from a slot (DIRECT w = x, GAUSS w = exp(-(x - x_min) / (2 scale))): SAMSIM_WEIGHT_SLOT is then a slot of
     !! the ensemble reductions; spec = c_null_ptr (with info = c_null_ptr) removes the row
     INTEGER(c_int) FUNCTION samsim_set_weights(h, spec, info) BIND(C, name='samsim_set_weights')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(c_ptr), VALUE :: spec                        ! samsim_weight_spec (c_loc of a TARGET), or c_null_ptr
       TYPE(c_ptr), VALUE :: info                        ! samsim_weight_info (c_loc of a TARGET), or c_null_ptr
     END FUNCTION
     !> the window [col0, col0 + ncols) of the weight row
     INTEGER(c_int) FUNCTION samsim_get_weights(h, col0, ncols, out) BIND(C, name='samsim_get_weights')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: col0, ncols
       REAL(c_double), INTENT(out) :: out(*)
     END FUNCTION
     !> the weighted moments of nslots slots over the running columns with a positive weight -- group >= 0: of those with that label
     INTEGER(c_int) FUNCTION samsim_get_weighted_stats(h, nslots, slots, group, out) BIND(C, name='samsim_get_weighted_stats')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: nslots, group
       INTEGER(c_int32_t), INTENT(in) :: slots(*)
       TYPE(samsim_wstat), INTENT(out) :: out(*)
     END FUNCTION
     !> wsum [nvbins + 2]: the sum of the weights per entry of samsim_get_histogram over the same columns
     INTEGER(c_int) FUNCTION samsim_get_weighted_histogram(h, slot, vb, group, wsum) BIND(C, name='samsim_get_weighted_histogram')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: slot, group
       TYPE(samsim_hist_bins), INTENT(in) :: vb
       REAL(c_double), INTENT(out) :: wsum(*)
     END FUNCTION
     !> per bin of a profile request the weighted moments of the bin value over the running columns with a positive weight that
     !! contribute to the bin -- group >= 0: of those with that label, -1 = any --; out(nbins, narrays), bin fastest
     INTEGER(c_int) FUNCTION samsim_get_weighted_profile_stats(h, rq, group, out) BIND(C, name='samsim_get_weighted_profile_stats')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_profile_request), INTENT(in) :: rq
       INTEGER(c_int32_t), VALUE :: group
       TYPE(samsim_wstat), INTENT(out) :: out(*)
     END FUNCTION
     !> the weighted means and the weighted population covariances of nslots slots over the same columns; cov(nslots, nslots) is
     !! symmetric, its diagonal the var of samsim_get_weighted_stats
     INTEGER(c_int) FUNCTION samsim_get_weighted_covariance(h, nslots, slots, group, count, sum_w, sum_w2, mean, cov) &
          BIND(C, name='samsim_get_weighted_covariance')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: nslots
       INTEGER(c_int32_t), INTENT(in) :: slots(*)
       INTEGER(c_int32_t), VALUE :: group
       INTEGER(c_int64_t), INTENT(out) :: count
       REAL(c_double), INTENT(out) :: sum_w, sum_w2
       REAL(c_double), INTENT(out) :: mean(*), cov(*)
     END FUNCTION
     !> the weighted joint histogram of one layer array: wsum(nvbins + 2, nbins), entry fastest, the sum of the weights of the
     !! columns per depth bin and value entry of samsim_get_profile_histogram (rq%narrays must be 1; group as there)
     INTEGER(c_int) FUNCTION samsim_get_weighted_profile_histogram(h, rq, vb, group, wsum) &
          BIND(C, name='samsim_get_weighted_profile_histogram')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(samsim_profile_request), INTENT(in) :: rq
       TYPE(samsim_hist_bins), INTENT(in) :: vb
       INTEGER(c_int32_t), VALUE :: group
       REAL(c_double), INTENT(out) :: wsum(*)
     END FUNCTION
     !> draw spec%m members by the weight row: the offspring row (SAMSIM_OFFSPRING_SLOT is then a slot of the ensemble reductions) and
     !! the ascending ancestor list; nothing of the ensemble is written; spec = c_null_ptr (with info = c_null_ptr) removes the rows
     INTEGER(c_int) FUNCTION samsim_resample(h, spec, info) BIND(C, name='samsim_resample')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       TYPE(c_ptr), VALUE :: spec                        ! samsim_resample_spec (c_loc of a TARGET), or c_null_ptr
       TYPE(c_ptr), VALUE :: info                        ! samsim_resample_info (c_loc of a TARGET), or c_null_ptr
     END FUNCTION
     !> the window [col0, col0 + ncols) of the offspring row
     INTEGER(c_int) FUNCTION samsim_get_offspring(h, col0, ncols, out) BIND(C, name='samsim_get_offspring')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: col0, ncols
       REAL(c_double), INTENT(out) :: out(*)
     END FUNCTION
     !> the 0-based column indices of the ancestors of the draws [k0, k0 + nk), ascending
     INTEGER(c_int) FUNCTION samsim_get_ancestors(h, k0, nk, out) BIND(C, name='samsim_get_ancestors')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: k0, nk
       INTEGER(c_int64_t), INTENT(out) :: out(*)
     END FUNCTION
     !> overwrite column dst(k) with column src(k) on the device (0-based indices): the bytes of samsim_get_columns -> samsim_set_state
     !! -> samsim_set_status; what = a sum of SAMSIM_COPY_FORCING, SAMSIM_COPY_TRACKS, SAMSIM_COPY_SCORES
     INTEGER(c_int) FUNCTION samsim_copy_columns(h, n, src, dst, what) BIND(C, name='samsim_copy_columns')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: n
       INTEGER(c_int64_t), INTENT(in) :: src(*), dst(*)
       INTEGER(c_int32_t), VALUE :: what
     END FUNCTION
     !> put the copies of the last samsim_resample where the dropped members were; SAMSIM_ERR_UNSUPPORTED, and nothing written, unless
     !! the draw had as many members as the pool and every drawn column still runs
     INTEGER(c_int) FUNCTION samsim_apply_resample(h, what, info) BIND(C, name='samsim_apply_resample')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), VALUE :: what
       TYPE(c_ptr), VALUE :: info                        ! samsim_apply_info (c_loc of a TARGET), or c_null_ptr
     END FUNCTION
     !> the entries [k0, k0 + nk) of the plan of the last samsim_apply_resample, 0-based column indices
     INTEGER(c_int) FUNCTION samsim_get_copy_plan(h, k0, nk, src, dst) BIND(C, name='samsim_get_copy_plan')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: k0, nk
       INTEGER(c_int64_t), INTENT(out) :: src(*), dst(*)
     END FUNCTION
     !> the HIP device ordinal of the handle and its PCI bus id (pci_bus_id: at least 16 characters) (ABI 5)
     INTEGER(c_int) FUNCTION samsim_get_device(h, device, pci_bus_id, len) BIND(C, name='samsim_get_device')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int32_t), INTENT(out) :: device
       CHARACTER(kind=c_char), INTENT(out) :: pci_bus_id(*)
       INTEGER(c_int32_t), VALUE :: len
     END FUNCTION
     !> from how many 64-column blocks a step runs as two concurrent launches (0 = never) and the first part's share (ABI 5)
     INTEGER(c_int) FUNCTION samsim_set_launch_split(h, min_blocks, first_part_eighths) BIND(C, name='samsim_set_launch_split')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: min_blocks
       INTEGER(c_int32_t), VALUE :: first_part_eighths
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_get_work(h, cells, colsteps) BIND(C, name='samsim_get_work')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), INTENT(out) :: cells, colsteps
     END FUNCTION
     INTEGER(c_int) FUNCTION samsim_synchronize(h) BIND(C, name='samsim_synchronize')
       IMPORT
       TYPE(c_ptr), VALUE :: h
     END FUNCTION
     !> nlaunches launches of nsteps steps, enqueued back to back, and the device time of the sequence [ms] (ABI 4)
     INTEGER(c_int) FUNCTION samsim_steps_timed(h, nsteps, nlaunches, device_ms) BIND(C, name='samsim_steps_timed')
       IMPORT
       TYPE(c_ptr), VALUE :: h
       INTEGER(c_int64_t), VALUE :: nsteps
       INTEGER(c_int32_t), VALUE :: nlaunches
       REAL(c_double), INTENT(out) :: device_ms
     END FUNCTION
     SUBROUTINE samsim_destroy(h) BIND(C, name='samsim_destroy')
       IMPORT
       TYPE(c_ptr), VALUE :: h
     END SUBROUTINE
     TYPE(c_ptr) FUNCTION samsim_strerror(code) BIND(C, name='samsim_strerror')
       IMPORT
       INTEGER(c_int), VALUE :: code
     END FUNCTION
  END INTERFACE

CONTAINS

  !> aborts with the library's message when a C-ABI call fails (the reference aborts with STOP as well)
  SUBROUTINE samsim_check(rc, what)
    INTEGER(c_int), INTENT(in)   :: rc
    CHARACTER(len=*), INTENT(in) :: what
    CHARACTER(kind=c_char), POINTER :: msg(:)
    INTEGER :: n
    IF (rc == 0) RETURN
    CALL c_f_pointer(samsim_strerror(rc), msg, (/ 200 /))
    n = 1
    DO WHILE (n < 200 .AND. msg(n) /= c_null_char)
       n = n + 1
    END DO
    PRINT *, 'samsim C-ABI error in ', what, ': code', rc, ' ', msg(1:n-1)
    STOP 3
  END SUBROUTINE samsim_check

  !> SAMSIM_TRACK_SLOT(track, field): the row of a track (both 0-based) as a slot of the ensemble reductions
  PURE FUNCTION samsim_track_slot(track, field) RESULT(slot)
    INTEGER(c_int32_t), INTENT(in) :: track, field
    INTEGER(c_int32_t) :: slot
    slot = 65536_c_int32_t + track*32_c_int32_t + field
  END FUNCTION samsim_track_slot

  !> SAMSIM_FUNC_SLOT(i): the row of functional i (0-based) as a slot of the ensemble reductions
  PURE FUNCTION samsim_func_slot(i) RESULT(slot)
    INTEGER(c_int32_t), INTENT(in) :: i
    INTEGER(c_int32_t) :: slot
    slot = 131072_c_int32_t + i
  END FUNCTION samsim_func_slot

  !> SAMSIM_SCORE_SLOT(field): a row of the per-column misfit (SAMSIM_SF_*) as a slot of the ensemble reductions
  PURE FUNCTION samsim_score_slot(field) RESULT(slot)
    INTEGER(c_int32_t), INTENT(in) :: field
    INTEGER(c_int32_t) :: slot
    slot = 196608_c_int32_t + field
  END FUNCTION samsim_score_slot

END MODULE mo_samsim_capi
