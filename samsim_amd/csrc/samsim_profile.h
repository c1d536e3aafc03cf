// samsim_profile.h -- what the four reductions of the layer profiles share with each other and with the C-ABI host code: the
// statistics (samsim_profile.hip), the joint histograms (samsim_hist.hip), the regressions (samsim_sens.hip) and the weighted
// statistics (samsim_wprofile.hip).  The step kernel does not include this header.
//
// One pass serves one requested array and one chunk of bins.  One wave owns one 64-column block at a time (lane = column) and
// strides over the blocks with a fixed grid; the walk of a block is samsim_profile_walk.h, what a family does with the finished bin
// values is its own.  The grid depends on ncol alone and the waves' results are combined in wave order, so a result depends on
// nothing but the state and the request.
#ifndef SAMSIM_PROFILE_H
#define SAMSIM_PROFILE_H

#include <hip/hip_runtime.h>

#include "samsim_device.h"

// What every pass of every family needs, formed in one place (for_each_pass, samsim_capi.cpp).  Every launcher takes it; the
// kernels of the statistics and of the weighted statistics take it by value, the others get its fields.
struct ProfPass {
  const double *lay;                          // the layer block [block][layer][array][64]
  const int32_t *n_active, *status, *labels;  // [ncol] rows; labels null: every column counts, else only those with label `group`
  long long ncol;
  double z0, dz;                              // the depth bins [z0 + b dz, z0 + (b+1) dz); 0 and 1 on the layer axis
  int group, N;
  int axis;                                   // picks the kernel in the launcher; no kernel reads it
  int origin, array;                          // enum samsim_profile_origin, enum samsim_layer_array
  int b0, nb;                                 // bins [b0, b0 + nb) of the request
  int lead;                                   // samsim_pass_plan.h
};

// a wave's partial of one bin of the statistics
struct ProfPartial { double mean, m2, mn, mx; long long n; };

// The grid of a pass, the one rule of the four launchers: one-wave workgroups, one per 64-column block and at most grid_max (the
// number of waves decides the merge order and so the bytes); 0 for a pass whose nb is not within [1, nb_max].
inline int pass_grid(const ProfPass &p, int grid_max, int nb_max) {
  if (p.nb < 1 || p.nb > nb_max) return 0;
  const long long nblk = (p.ncol + 63) / 64;
  return (int)(nblk < grid_max ? nblk : grid_max);
}

// A pass of a family whose kernel is one template over the axis (instantiated twice: the two walks keep their own register
// budgets) and folds the LDS tile: at most DEV_PROF_BINS bins, kernel(pass, extra..., part) leaves the waves' partials, then
// `merge` combines them in wave order and writes out[0 .. nb).  part is reused by the next pass on the same stream.
template <class K, class M, class P, class O, class... X>
inline hipError_t launch_tile_pass(K layer, K depth, M merge, int grid_max, const ProfPass &p, hipStream_t stream, P *part, O *out,
                                   X... extra) {
  const int grid = pass_grid(p, grid_max, DEV_PROF_BINS);
  if (!grid) return hipErrorInvalidValue;
  const K kernel = p.axis == SAMSIM_PROFILE_BY_LAYER ? layer : depth;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, stream, p, extra..., part);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(merge, dim3(1), dim3(64), 0, stream, part, grid, p.nb, out);
  return hipGetLastError();
}

// samsim_profile.hip.  One pass of samsim_get_profile_stats: results to out[0 .. nb); part holds DEV_PROF_GRID * DEV_PROF_BINS
// partials.  Both lie in the handle's scratch; the call only enqueues.
extern "C" hipError_t samsim_launch_profile(ProfPass p, ProfPartial *part, samsim_stat *out, hipStream_t stream);

#endif
