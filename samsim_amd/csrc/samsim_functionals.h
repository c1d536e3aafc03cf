// samsim_functionals.h -- what samsim_functionals.hip and the C-ABI host code share about the column functionals
// (samsim_set_functionals, samsim_get_functionals, SAMSIM_FUNC_SLOT, include/samsim.h).  The step kernel does not include this header.
#ifndef SAMSIM_FUNCTIONALS_H
#define SAMSIM_FUNCTIONALS_H

#include <hip/hip_runtime.h>

#include "samsim_column_read.h"
#include "samsim_row_plan.h"

// A walk over the layers serves one group of functionals: those whose arrays need at most ROW_PLAN_ROWS distinct rows of the layer
// block beside thick.  The host forms the groups by first-fit (samsim_row_plan.h; func_plan, samsim_capi.cpp); with up to four rows
// per walk the eight functionals of a handle take one walk in the common case and three at the most.

// one functional as the kernel sees it: samsim_functional_spec, checked by samsim_set_functionals, and its place in the plan
struct FuncDev {
  int32_t kind;     // enum samsim_functional_kind
  int32_t origin;   // enum samsim_profile_origin
  int32_t sense;    // +1 (a_k >= threshold), -1 (a_k < threshold), 0
  int32_t mode;     // enum column_read::layer_mode
  int32_t group;    // the walk that serves it
  int32_t ia, ib;   // positions among the group's rows; ib only with LAYER_S_BU
  int32_t pad;
  double z_lo, z_hi, threshold, missing;
};

// One evaluation: every functional of the handle for every 64-column block, one wave per block.  Passed by value as the kernel's
// argument.
struct FuncParams {
  const double *lay;          // layer block, DEV_LAY_INDEX
  const int32_t *n_active, *status, *flags;
  double *rows;               // [nf][ncol]
  long long ncol;
  int32_t N;                  // nlayer
  int32_t nf;
  int32_t stepped;            // the kernel has run: samsim_get_state clamps S_abs and refreshes S_bu in the running columns
  int32_t need_H;             // some functional counts from the bottom: a thick-only pre-pass forms H
  RowPlan<SAMSIM_MAX_FUNCTIONALS> plan;   // the walks: at most one per functional
  FuncDev f[SAMSIM_MAX_FUNCTIONALS];
};
static_assert(sizeof(FuncDev) == 64 && sizeof(FuncParams) == 648, "the evaluation's parameters travel as a kernel argument");

// samsim_functionals.hip: enqueues one evaluation of every block of the handle on `stream`
extern "C" hipError_t samsim_launch_functionals(const FuncParams *p, hipStream_t stream);

#endif
