// samsim_select.h -- what samsim_select.hip and the C-ABI host code share about the selection of columns and the gather of scattered
// columns (samsim_select_columns, samsim_get_columns, include/samsim.h).  The step kernel does not include this header.
#ifndef SAMSIM_SELECT_H
#define SAMSIM_SELECT_H

#include <hip/hip_runtime.h>

#include "samsim_device.h"

// The select scratch of a handle, SAMSIM_SELECT_SCRATCH_BYTES at most:
//   [0, DEV_SEL_OFFSETS_AT)                 the waves' counts, int64 [DEV_SEL_GRID]
//   [DEV_SEL_OFFSETS_AT, DEV_SEL_LIST_AT)   their exclusive offsets, int64 [DEV_SEL_GRID], then the total
//   [DEV_SEL_LIST_AT, DEV_SEL_BYTES)        the index list, int64 [SAMSIM_SELECT_MAX_OUT]: the result of samsim_select_columns, or the
//                                           request of samsim_get_columns
#define DEV_SEL_GRID DEV_PROF_GRID   // one-wave workgroups of the count and the write kernel, at most
#define DEV_SEL_OFFSETS_AT ((size_t)DEV_SEL_GRID * 8)
#define DEV_SEL_LIST_AT (DEV_SEL_OFFSETS_AT + ((size_t)DEV_SEL_GRID + 8) * 8)
#define DEV_SEL_BYTES (DEV_SEL_LIST_AT + (size_t)SAMSIM_SELECT_MAX_OUT * 8)
static_assert(DEV_SEL_BYTES <= SAMSIM_SELECT_SCRATCH_BYTES, "select scratch bound of samsim.h");
static_assert(DEV_SEL_GRID % 64 == 0, "the scan gives every lane the same number of waves");

// one term as the kernels see it: the [ncol] row of its slot (null: the value is (double)n_active) and the two bounds
struct SelTerm {
  const double *row;
  double lo, hi;
};

// One selection, passed by value as the kernels' argument.  Wave w of nwaves owns the 64-column blocks [w * per, (w + 1) * per), so
// that wave order is column order.
struct SelParams {
  SelTerm t[SAMSIM_SELECT_MAX_TERMS];
  const int32_t *n_active;
  const int32_t *status;    // null with SAMSIM_SELECT_ANY: the row is not read
  const int32_t *labels;    // null with group == -1: the row is not read
  long long ncol;
  long long per;            // blocks per wave
  long long max_out;
  int32_t nwaves;
  int32_t nterms;
  int32_t group;
  int32_t status_mode;      // enum samsim_select_status
  int32_t code;
};

// what the gather of the per-column rows leaves in the staging buffer for w columns, in this order (8-byte rows first)
//   double scal[SAMSIM_NSCAL][w]; int64 err_step[w]; int32 n_active[w], status[w], err_layer[w]
#define DEV_SEL_COLUMN_BYTES ((size_t)SAMSIM_NSCAL * 8 + 8 + 3 * 4)

// samsim_select.hip.  All three enqueue on `stream` and return at once.
// the counts of every wave, their offsets and the total into `scratch`; with max_out > 0 also the first max_out indices
extern "C" hipError_t samsim_launch_select(const SelParams *p, void *scratch, hipStream_t stream);
// stage[(a * N + k) * w + j] = array a, 0-based layer k of column cols[j], as samsim_get_state returns it (`stepped`: the clamp of
// S_abs and the quotient S_bu apply), for a < narr, k < N, j < w
extern "C" hipError_t samsim_launch_gather_layers(const double *lay, const long long *cols, const int32_t *n_active, const int32_t *status,
                                                  const int32_t *flags, double *stage, int narr, int N, long long ncol, long long w,
                                                  int stepped, hipStream_t stream);
// the per-column rows of the columns cols[0 .. w) into `stage`, laid out as above
extern "C" hipError_t samsim_launch_gather_columns(const double *scal, const int32_t *n_active, const int32_t *status,
                                                   const long long *err_step, const int32_t *err_layer, const long long *cols, void *stage,
                                                   long long ncol, long long w, hipStream_t stream);

#endif
