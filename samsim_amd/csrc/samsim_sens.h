// samsim_sens.h -- what samsim_sens.hip and the C-ABI host code share about the ensemble sensitivities (samsim_get_covariance,
// samsim_get_profile_regression, include/samsim.h).  The step kernel does not include this header.
#ifndef SAMSIM_SENS_H
#define SAMSIM_SENS_H

#include <hip/hip_runtime.h>

#include "samsim_profile.h"
#include "samsim_slot_walk.h"

// Both reductions run a fixed grid of at most DEV_SENS_GRID one-wave workgroups (a wave per 64-column block at a time), fixed by
// ncol alone; every wave leaves one partial, merged in wave order.
#define DEV_SENS_GRID 1024
#define DEV_SENS_PAIRS (SAMSIM_SENS_MAX_SLOTS * (SAMSIM_SENS_MAX_SLOTS + 1) / 2)   // the upper triangle, diagonal included

// Covariances.  A wave's partial is DEV_COV_PART doubles whatever nslots is: n (a count below 2^53 is exact in a double), the
// means of the slots, the co-moments of the pairs (i, j), i <= j, row by row of the upper triangle of nslots slots.
#define DEV_COV_MEAN0 1
#define DEV_COV_C0 (1 + SAMSIM_SENS_MAX_SLOTS)
#define DEV_COV_PART (1 + SAMSIM_SENS_MAX_SLOTS + DEV_SENS_PAIRS)
// the result on the device: count, mean[SAMSIM_SENS_MAX_SLOTS], cov[nslots][nslots]
struct CovResult {
  long long count;
  double mean[SAMSIM_SENS_MAX_SLOTS];
  double cov[SAMSIM_SENS_MAX_SLOTS * SAMSIM_SENS_MAX_SLOTS];
};
// the [ncol] rows of the slots; a null row is n_active
struct SensRows { const double *row[SAMSIM_SENS_MAX_SLOTS]; };

// Profile regressions.  One pass serves one array and at most DEV_PROF_BINS bins, as a pass of the profile statistics does; a
// wave's partial per bin is the statistics' (n, mean, M2) of the bin value with the predictor's riding along.
struct SensProfPartial { double mean_y, m2_y, mean_x, m2_x, cxy; long long n; };

// device scratch of both: the waves' partials of one pass, then the results of the largest request
#define DEV_SENS_PART_BYTES (sizeof(SensProfPartial) * DEV_SENS_GRID * DEV_PROF_BINS)
static_assert(sizeof(double) * DEV_COV_PART * DEV_SENS_GRID <= DEV_SENS_PART_BYTES, "the covariance partials fit where the regression's do");
#define DEV_SENS_RESULT_BYTES (sizeof(samsim_pair_stat) * SAMSIM_PROFILE_MAX_ARRAYS * SAMSIM_PROFILE_MAX_BINS)
static_assert(sizeof(CovResult) <= DEV_SENS_RESULT_BYTES, "the covariance result fits where the regression's do");

// LDS of a regression workgroup: the walk's tile, the lanes' masks and the block's 64 predictor values
#define DEV_SENS_PROFILE_LDS (sizeof(double) * DEV_PROF_BINS * (DEV_PROF_BINS + 1) + 512 + 512)
static_assert(4 * DEV_SENS_PROFILE_LDS <= (160u << 10), "four regression workgroups per CU, as the statistics kernels get");

// samsim_sens.hip.  cs: the columns that count (samsim_slot_walk.h).  part and out lie in the handle's scratch; the calls only
// enqueue.
extern "C" hipError_t samsim_launch_covariance(slot_walk::ColSet cs, SensRows rows, int nslots, double *part, CovResult *out,
                                               hipStream_t stream);
// one pass (samsim_profile.h), results to out[0 .. nb); x: the predictor's [ncol] row, or null for n_active
extern "C" hipError_t samsim_launch_profile_regression(ProfPass p, const double *x, SensProfPartial *part, samsim_pair_stat *out,
                                                       hipStream_t stream);

#endif
