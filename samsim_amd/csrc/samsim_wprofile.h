// samsim_wprofile.h -- what samsim_wprofile.hip and the C-ABI host code share about the weighted profile statistics
// (samsim_get_weighted_profile_stats, include/samsim.h).  The step kernel does not include this header.
#ifndef SAMSIM_WPROFILE_H
#define SAMSIM_WPROFILE_H

#include <hip/hip_runtime.h>

#include "samsim_profile.h"

// One pass serves one array and at most DEV_PROF_BINS bins with the grid of samsim_launch_profile -- at most DEV_PROF_GRID one-wave
// workgroups, fixed by ncol alone --, as a pass of the profile statistics does; a wave's partial per bin is the statistics'
// (n, mean, M2, min, max) of the bin value with the total weight W in the place of n, and the sum of squared weights beside it.
struct WProfPartial { double W, W2, mean, m2, mn, mx; long long n; };

// device scratch: the waves' partials of one pass (every pass reuses them), then the results of the largest request
#define DEV_WPROF_PART_BYTES (sizeof(WProfPartial) * DEV_PROF_GRID * DEV_PROF_BINS)
#define DEV_WPROF_RESULT_BYTES (sizeof(samsim_wstat) * SAMSIM_PROFILE_MAX_ARRAYS * SAMSIM_PROFILE_MAX_BINS)
#define DEV_WPROF_BYTES (DEV_WPROF_PART_BYTES + DEV_WPROF_RESULT_BYTES)
static_assert(DEV_WPROF_BYTES <= SAMSIM_WPROFILE_SCRATCH_BYTES, "weighted profile scratch bound of samsim.h");

// LDS of a workgroup: the walk's tile, the lanes' masks and the block's 64 weights
#define DEV_WPROF_LDS (sizeof(double) * DEV_PROF_BINS * (DEV_PROF_BINS + 1) + 512 + 512)
static_assert(4 * DEV_WPROF_LDS <= (160u << 10), "four workgroups per CU, as the statistics kernels get");

// samsim_wprofile.hip.  One pass (samsim_profile.h), results to out[0 .. nb).  w: the [ncol] weight row; a column counts if its
// status is 0, its label passes and w > 0.  part and out lie in the handle's scratch; the call only enqueues.
extern "C" hipError_t samsim_launch_weighted_profile(ProfPass p, const double *w, WProfPartial *part, samsim_wstat *out,
                                                     hipStream_t stream);

#endif
