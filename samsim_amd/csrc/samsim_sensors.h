// samsim_sensors.h -- what samsim_sensors.hip and the C-ABI host code share about the sensors and the per-column misfit
// (samsim_set_sensors, samsim_get_sensor_values, samsim_score, SAMSIM_SCORE_SLOT, include/samsim.h).  The step kernel does not
// include this header.
#ifndef SAMSIM_SENSORS_H
#define SAMSIM_SENSORS_H

#include <hip/hip_runtime.h>

#include "samsim_column_read.h"
#include "samsim_row_plan.h"

// A walk over the layers serves one group of profile sensors: those whose arrays need at most ROW_PLAN_ROWS distinct rows of the
// layer block beside thick.  The host forms the groups by first-fit (samsim_row_plan.h; sensor_plan, samsim_capi.cpp).  A
// thermistor string and a salinity core take one walk; in the worst case every sensor has a walk of its own.

// one sensor as the kernel sees it: samsim_sensor_spec, checked by samsim_set_sensors, and its place in the plan
struct SensorDev {
  int32_t kind;     // enum samsim_sensor_kind
  int32_t id;       // SCALAR: enum samsim_scalar
  int32_t origin;   // enum samsim_profile_origin
  int32_t interp;   // enum samsim_sensor_interp
  int32_t mode;     // enum column_read::layer_mode
  int32_t group;    // the walk that serves it (PROFILE), -1 for the other kinds
  int32_t ia, ib;   // positions among the group's rows; ib only with LAYER_S_BU
  double z, missing;
};

// One evaluation: every sensor of the handle, one wave per 64 columns (score) or per 64 list positions (values).  Passed by value as
// the kernel's argument.
struct SensorParams {
  const double *lay;          // layer block, DEV_LAY_INDEX
  const double *scal;         // [SAMSIM_NSCAL][ncol]
  const int32_t *n_active, *status, *flags;
  const int32_t *labels;      // score: the group labels when group >= 0, else null
  const long long *cols;      // values: the list of columns, one per position; null for a score
  double *out;                // score: the rows [SAMSIM_NSF][ncol]; values: y [ns][npos]
  long long ncol;
  long long npos;             // values: positions of this launch
  int32_t N;                  // nlayer
  int32_t ns;                 // sensors
  int32_t stepped;            // the kernel has run: samsim_get_state clamps S_abs and refreshes S_bu in the running columns
  int32_t need_H;             // an ICE_THICKNESS sensor, or a profile sensor that counts from the bottom: a thick-only pre-pass forms H
  int32_t group;              // score: the label a scored column carries, or -1
  uint32_t obs_mask;          // score: bit i set where obs[i] is not a NaN
  RowPlan<SAMSIM_MAX_SENSORS> plan;   // the walks: at most one per profile sensor
  double obs[SAMSIM_MAX_SENSORS], weight[SAMSIM_MAX_SENSORS];
  SensorDev s[SAMSIM_MAX_SENSORS];
};
static_assert(SAMSIM_MAX_SENSORS == 32, "one bit per sensor in a 32-bit lane mask");
static_assert(sizeof(SensorDev) == 48 && sizeof(SensorParams) == 2416, "the evaluation's parameters travel as a kernel argument");

// positions whose values one launch of the list variant leaves in the scratch: [SAMSIM_MAX_SENSORS][DEV_SENSOR_PIECE] doubles, 1 MiB
#define DEV_SENSOR_PIECE 4096

// samsim_sensors.hip: enqueue one score update of every block of the handle, or the values of p->npos list positions, on `stream`
extern "C" hipError_t samsim_launch_score(const SensorParams *p, hipStream_t stream);
extern "C" hipError_t samsim_launch_sensor_values(const SensorParams *p, hipStream_t stream);

#endif
