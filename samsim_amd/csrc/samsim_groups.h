// samsim_groups.h -- what samsim_groups.hip and the C-ABI host code share about the per-group ensemble statistics
// (samsim_set_groups / samsim_get_group_stats, include/samsim.h).  The step kernel does not include this header.
#ifndef SAMSIM_GROUPS_H
#define SAMSIM_GROUPS_H

#include <hip/hip_runtime.h>

#include "../../include/samsim.h"
#include "samsim_slot_walk.h"

// One pass reduces one [ncol] row with a fixed grid of one-wave workgroups; every wave leaves one partial per group, merged in
// wave order.  The grid is the largest that keeps the waves' partials within DEV_GROUP_PART_ENTRIES, at most DEV_GROUP_GRID
// waves: 1 024 waves up to 256 groups, 256 waves at SAMSIM_MAX_GROUPS.  It depends on ncol and ngroups alone.
#define DEV_GROUP_GRID 1024
#define DEV_GROUP_PART_ENTRIES (256 * SAMSIM_MAX_GROUPS)
struct GroupPartial { double mean, m2, mn, mx; long long n; };

static inline int dev_group_waves(long long ncol, int ngroups) {
  const long long w = DEV_GROUP_PART_ENTRIES / ngroups;
  return slot_walk::slot_grid(ncol, w < DEV_GROUP_GRID ? w : DEV_GROUP_GRID);
}

// samsim_groups.hip: the statistics of one row (row, or n_active where row is null) per group of cs.labels,
// results to out[0 .. ngroups).  part holds dev_group_waves(ncol, ngroups) * ngroups partials and is reused by the next pass on the
// same stream.
extern "C" hipError_t samsim_launch_group_stats(slot_walk::LabelSet cs, const double *row, int ngroups, GroupPartial *part, samsim_stat *out,
                                                hipStream_t stream);

#endif
