// samsim_weights.h -- what samsim_weights.hip and the C-ABI host code share about the weight row and the weighted reductions
// (samsim_set_weights, samsim_get_weighted_stats, samsim_get_weighted_histogram, samsim_get_weighted_covariance, include/samsim.h).
// The step kernel does not include this header.
#ifndef SAMSIM_WEIGHTS_H
#define SAMSIM_WEIGHTS_H

#include <hip/hip_runtime.h>

#include "samsim_hist.h"
#include "samsim_sens.h"

// Every kernel runs a fixed grid of at most DEV_WEIGHT_GRID one-wave workgroups (a wave per 64-column block at a time), fixed by
// ncol alone; every wave leaves one partial, merged in wave order.
#define DEV_WEIGHT_GRID 1024
#define DEV_WEIGHT_ENTRIES (SAMSIM_HIST_MAX_VBINS + 2)   // a wave's table of the weighted histogram

// what a wave knows of the columns it saw.  samsim_set_weights: the minimum of x over the IN columns with a non-NaN x and how many
// there were (n_pos), then n_in, n_pos, sum_w, sum_w2 of the row it wrote
struct WeightPartial { double x_min, sum_w, sum_w2; long long n_in, n_pos; };
// samsim_get_weighted_stats: n columns of total weight W (and sum of squared weights W2) with weighted mean `mean` and weighted sum
// of squared deviations m2
struct WStatPartial { double W, W2, mean, m2, mn, mx; long long n; };

// device scratch of the three calls: the waves' histogram tables, the waves' partials (every pass reuses them), then the results
#define DEV_WEIGHT_TABLES_AT 0
#define DEV_WEIGHT_TABLES_BYTES (sizeof(double) * DEV_WEIGHT_GRID * DEV_WEIGHT_ENTRIES)
#define DEV_WEIGHT_PART_AT (DEV_WEIGHT_TABLES_AT + DEV_WEIGHT_TABLES_BYTES)
#define DEV_WEIGHT_PART_BYTES (sizeof(WStatPartial) * DEV_WEIGHT_GRID * SAMSIM_SENS_MAX_SLOTS)   // [wave][slot]
static_assert(sizeof(WeightPartial) <= sizeof(WStatPartial), "the partials of samsim_set_weights fit where the statistics' do");
#define DEV_WEIGHT_RESULT_AT (DEV_WEIGHT_PART_AT + DEV_WEIGHT_PART_BYTES)
#define DEV_WEIGHT_RESULT_BYTES (sizeof(double) * DEV_WEIGHT_ENTRIES)
static_assert(sizeof(samsim_wstat) * SAMSIM_SENS_MAX_SLOTS <= DEV_WEIGHT_RESULT_BYTES && sizeof(WeightPartial) <= DEV_WEIGHT_RESULT_BYTES,
              "the results of the other two calls fit where a histogram row does");
#define DEV_WEIGHT_BYTES (DEV_WEIGHT_RESULT_AT + DEV_WEIGHT_RESULT_BYTES)
static_assert(DEV_WEIGHT_BYTES <= SAMSIM_WEIGHT_SCRATCH_BYTES, "weight scratch bound of samsim.h");

// samsim_get_weighted_covariance.  A wave's partial is DEV_WCOV_PART doubles whatever nslots is: n (a count below 2^53 is exact in a
// double), W, W2, the weighted means of the slots, the weighted co-moments of the pairs (i, j), i <= j, row by row of the upper
// triangle of nslots slots.  The partials lie where those of the weighted moments do, the result where theirs does.
#define DEV_WCOV_MEAN0 3
#define DEV_WCOV_C0 (3 + SAMSIM_SENS_MAX_SLOTS)
#define DEV_WCOV_PART (3 + SAMSIM_SENS_MAX_SLOTS + DEV_SENS_PAIRS)
struct WCovResult {
  long long count;
  double sum_w, sum_w2;
  double mean[SAMSIM_SENS_MAX_SLOTS];
  double cov[SAMSIM_SENS_MAX_SLOTS * SAMSIM_SENS_MAX_SLOTS];
};
static_assert(sizeof(double) * DEV_WCOV_PART * DEV_WEIGHT_GRID <= DEV_WEIGHT_PART_BYTES, "the covariance partials fit where the moments' do");
static_assert(sizeof(WCovResult) <= DEV_WEIGHT_RESULT_BYTES, "the covariance result fits where a histogram row does");

// samsim_weights.hip.  cs: the columns that are IN (samsim_slot_walk.h).  x: the [ncol] row of the source slot, or null for
// n_active.  part and out lie in the handle's scratch; the calls only enqueue.
// The weight row w[ncol] of `kind` (enum samsim_weight_kind) with c = 0.5 / scale; out: x_min, sum_w, sum_w2, n_in, n_pos.
extern "C" hipError_t samsim_launch_set_weights(slot_walk::ColSet cs, const double *x, int kind, double c, double *w, WeightPartial *part,
                                                WeightPartial *out, hipStream_t stream);
// the weighted moments of the nslots rows (SensRows of samsim_sens.h: a null row is n_active) over the columns that are IN and have
// w > 0, in one walk, to out[0 .. nslots)
extern "C" hipError_t samsim_launch_weighted_stats(slot_walk::ColSet cs, SensRows rows, int nslots, const double *w, WStatPartial *part,
                                                   samsim_wstat *out, hipStream_t stream);
// the sum of w per entry of the histogram of one row over the same columns: tables [grid][DEV_WEIGHT_ENTRIES], out [nvbins + 2]
extern "C" hipError_t samsim_launch_weighted_hist(slot_walk::ColSet cs, const double *x, const double *w, HistEdges e, double *tables,
                                                  double *out, hipStream_t stream);
// the weighted means and covariances of the nslots rows over the same columns, in one walk: part [grid][DEV_WCOV_PART]
extern "C" hipError_t samsim_launch_weighted_covariance(slot_walk::ColSet cs, SensRows rows, int nslots, const double *w, double *part,
                                                        WCovResult *out, hipStream_t stream);

#endif
