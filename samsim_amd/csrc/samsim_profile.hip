// samsim_profile.hip -- device-side ensemble statistics of the layer profiles (samsim_get_profile_stats, include/samsim.h).
//
// One pass of the reduction serves one requested array and one chunk of at most DEV_PROF_BINS bins.  One wave owns one 64-column
// block at a time (lane = column) and strides over the blocks with a fixed grid.  The wave walks the layers k of its block with
// 512-byte row loads from the device layout [block][layer][array][64]; only the rows the request needs are touched (the array
// itself -- S_abs and m for S_bu -- and thick for the depth axis).  Every lane moves through the bins of its own column
// monotonically and drops each finished bin value v into an LDS tile [bin][lane] (the walk: samsim_profile_walk.h, shared with
// the joint histograms of samsim_hist.hip).  After the block, lane j folds row j of the
// tile in lane order into its own running (n, mean, M2, min, max) of bin j: a transposition through LDS, no cross-lane
// reduction, no atomics.  At the end every wave stores its 64 partials; profile_merge_kernel combines the waves' partials in
// wave order (Chan's pairwise update), so the result depends on nothing but the state and the request.
#include <hip/hip_runtime.h>

#include "samsim_device.h"
#include "samsim_profile_fold.h"
#include "samsim_profile_walk.h"

namespace {

using namespace profile_walk;   // the block walk the reductions share (samsim_profile_walk.h)
using namespace profile_fold;   // Run, merge and fold_tile, shared with the regressions of samsim_sens.hip (samsim_profile_fold.h)

__device__ __forceinline__ void store_partials(ProfPartial *part, int lane, const Run &run) {
  ProfPartial p;
  p.mean = run.mean; p.m2 = run.m2; p.mn = run.mn; p.mx = run.mx; p.n = run.n;
  part[(size_t)blockIdx.x * DEV_PROF_BINS + lane] = p;
}

// ---- layer axis (profile_walk::layer_block): bins [b0, b0+nb)
__global__ void __launch_bounds__(64) profile_layer_kernel(const double *__restrict__ lay, const int32_t *__restrict__ n_active,
                                                           const int32_t *__restrict__ status, const int32_t *__restrict__ labels,
                                                           int group, long long ncol, int N, int origin, int array, int b0, int nb,
                                                           ProfPartial *__restrict__ part) {
  __shared__ double tile[DEV_PROF_BINS * kTileStride];
  __shared__ unsigned long long smask[64];
  const int lane = threadIdx.x;
  const long long nblk = (ncol + 63) / 64;
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  Co none{0.0, 0.0, 0.0};   // no predictor rides along
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(n_active, status, labels, group, ncol, blk, lane, N);
    TileSink sink{tile, lane, 0};
    layer_block(lay, ncol, N, blk, lane, na, origin, array, b0, nb, sink);
    fold_tile<false>(tile, nullptr, smask, sink.mask, lane, run, none);
  }
  store_partials(part, lane, run);
}

// ---- depth axis (profile_walk::depth_block): bins [b0, b0+nb)
__global__ void __launch_bounds__(64) profile_depth_kernel(const double *__restrict__ lay, const int32_t *__restrict__ n_active,
                                                           const int32_t *__restrict__ status, const int32_t *__restrict__ labels,
                                                           int group, long long ncol, int N, int origin, int array, int b0, int nb,
                                                           int lead, double z0, double dz, ProfPartial *__restrict__ part) {
  __shared__ double tile[DEV_PROF_BINS * kTileStride];
  __shared__ unsigned long long smask[64];
  const int lane = threadIdx.x;
  const long long nblk = (ncol + 63) / 64;
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  Co none{0.0, 0.0, 0.0};   // no predictor rides along
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(n_active, status, labels, group, ncol, blk, lane, N);
    TileSink sink{tile, lane, 0};
    depth_block(lay, ncol, N, blk, lane, na, origin, array, b0, nb, lead, z0, dz, sink);
    fold_tile<false>(tile, nullptr, smask, sink.mask, lane, run, none);
  }
  store_partials(part, lane, run);
}

// the waves' partials of one pass, combined in wave order; thread j writes bin b0 + j of the pass's array
__global__ void __launch_bounds__(64) profile_merge_kernel(const ProfPartial *__restrict__ part, int nwaves, int nb,
                                                           samsim_stat *__restrict__ out) {
  const int j = threadIdx.x;
  if (j >= nb) return;
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  for (int w = 0; w < nwaves; ++w) {
    const ProfPartial p = part[(size_t)w * DEV_PROF_BINS + j];
    if (p.n > 0) merge(run, p.n, p.mean, p.m2, p.mn, p.mx);
  }
  samsim_stat st;
  st.count = run.n;
  if (run.n > 0) {
    st.mean = run.mean; st.min = run.mn; st.max = run.mx;
    st.std = sqrt(run.m2 / (double)run.n);
  } else {
    st.mean = st.min = st.max = st.std = 0.0;
  }
  out[j] = st;
}

}  // namespace

// One pass: array `array`, bins [b0, b0 + nb) of the request's nbins with nb <= DEV_PROF_BINS, results to out[0 .. nb).  part holds DEV_PROF_GRID *
// DEV_PROF_BINS partials and is reused by the next pass on the same stream.  labels: null (every column counts), or the [ncol] label row
// of samsim_set_groups, of which only the columns with label `group` count.
extern "C" hipError_t samsim_launch_profile(const double *lay, const int32_t *n_active, const int32_t *status, const int32_t *labels,
                                            int group, long long ncol, int N, int axis, int origin, int array, int b0, int nb, int nbins,
                                            double z0, double dz, ProfPartial *part, samsim_stat *out, hipStream_t stream) {
  const long long nblk = (ncol + 63) / 64;
  const int grid = (int)(nblk < DEV_PROF_GRID ? nblk : DEV_PROF_GRID);
  if (axis == SAMSIM_PROFILE_BY_LAYER)
    hipLaunchKernelGGL(profile_layer_kernel, dim3(grid), dim3(64), 0, stream, lay, n_active, status, labels, group, ncol, N, origin, array, b0,
                       nb, part);
  else
    hipLaunchKernelGGL(profile_depth_kernel, dim3(grid), dim3(64), 0, stream, lay, n_active, status, labels, group, ncol, N, origin, array,
                       b0, nb, origin == SAMSIM_PROFILE_FROM_TOP ? b0 > 0 : b0 + nb < nbins, z0, dz, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(profile_merge_kernel, dim3(1), dim3(64), 0, stream, part, grid, nb, out);
  return hipGetLastError();
}
