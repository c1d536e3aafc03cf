// samsim_wphist.h -- what samsim_wphist.hip and the C-ABI host code share about the weighted joint histogram of the layer profiles
// (samsim_get_weighted_profile_histogram, include/samsim.h).  The step kernel does not include this header.
#ifndef SAMSIM_WPHIST_H
#define SAMSIM_WPHIST_H

#include <hip/hip_runtime.h>

#include "samsim_hist.h"

// A pass serves `chunk` depth bins of the one array (dev_wphist_chunk, samsim_pass_plan.h): the LDS of a one-wave workgroup holds
// the walk's tile [chunk][64 + 1] doubles, the lanes' bin masks (512 B), the block's 64 weights (512 B) and the wave's table
// [chunk][W | 1] of doubles, W = nvbins + 2 (the odd row stride spreads the 64 lanes' rows over the banks); together at most the
// 64 KiB a workgroup gets without an opt-in:
//   chunk = min(64, 64 512 / (8 * (65 + ((nvbins + 2) | 1)))),
// 64 up to 59 value bins, 25 at SAMSIM_HIST_MAX_VBINS.  A pass runs at most DEV_WPHIST_GRID one-wave workgroups, fixed by ncol
// alone; every wave stores its table [chunk][W] to device memory and a merge kernel adds the waves' tables in wave order.
//
// device scratch: the waves' tables of one pass (every pass reuses them), then the result of the largest request
constexpr long long dev_wphist_max_wave_doubles() {
  long long m = 0;
  for (int nv = 1; nv <= SAMSIM_HIST_MAX_VBINS; ++nv) m = dev_wphist_wave_doubles(nv) > m ? dev_wphist_wave_doubles(nv) : m;
  return m;
}
#define DEV_WPHIST_PART_BYTES (sizeof(double) * (size_t)DEV_WPHIST_GRID * (size_t)dev_wphist_max_wave_doubles())
#define DEV_WPHIST_RESULT_BYTES (sizeof(double) * (size_t)SAMSIM_PROFILE_MAX_BINS * (SAMSIM_HIST_MAX_VBINS + 2))
#define DEV_WPHIST_BYTES (DEV_WPHIST_PART_BYTES + DEV_WPHIST_RESULT_BYTES)
static_assert(DEV_WPHIST_BYTES <= SAMSIM_WPHIST_SCRATCH_BYTES, "weighted profile histogram scratch bound of samsim.h");
static_assert(dev_wphist_lds(1) <= DEV_WPHIST_LDS_BYTES && dev_wphist_lds(SAMSIM_HIST_MAX_VBINS) <= DEV_WPHIST_LDS_BYTES &&
                  dev_wphist_chunk(SAMSIM_HIST_MAX_VBINS) >= 1,
              "a pass fits the LDS of a workgroup");

// the merge kernel adds DEV_WPHIST_MERGE_ENTRIES consecutive entries of the pass's rows [nb][W] per workgroup: a lane reads them
// as one 64-byte piece of a wave's table
#define DEV_WPHIST_MERGE_ENTRIES 8

// samsim_wphist.hip.  One pass (samsim_profile.h) with nb <= dev_wphist_chunk(nvbins): rows b0 .. b0+nb-1 of result[nbins][W].
// w: the [ncol] weight row; a column counts if its status is 0, its label passes and w > 0.  tables: DEV_WPHIST_PART_BYTES.
// tables and result lie in the handle's scratch; the call only enqueues.
extern "C" hipError_t samsim_launch_weighted_profile_hist(ProfPass p, const double *w, HistEdges e, double *tables, double *result,
                                                          hipStream_t stream);

#endif
