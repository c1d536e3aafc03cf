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
#include "samsim_profile_walk.h"

namespace {

using namespace profile_walk;   // the block walk both reductions share (samsim_profile_walk.h)

// running statistics of one bin in one lane: n values with mean `mean` and sum of squared deviations `m2`
struct Run {
  long long n;
  double mean, m2, mn, mx;
};

// Chan et al.: (n, mean, M2) of the union of two sets from those of the sets; b is not empty
__device__ __forceinline__ void merge(Run &a, long long nb, double mean_b, double m2_b, double mn_b, double mx_b) {
  if (a.n == 0) {
    a.n = nb; a.mean = mean_b; a.m2 = m2_b; a.mn = mn_b; a.mx = mx_b;
    return;
  }
  const long long n = a.n + nb;
  const double delta = mean_b - a.mean;
  const double fb = (double)nb / (double)n;
  a.mean = a.mean + delta * fb;
  a.m2 = a.m2 + m2_b + delta * delta * ((double)a.n * fb);
  a.n = n;
  a.mn = mn_b < a.mn ? mn_b : a.mn;
  a.mx = mx_b > a.mx ? mx_b : a.mx;
}

// Lane j folds row j of the tile: the values of bin j of the columns whose bit j is set in their lane's mask, in lane order.
// The block's mean is formed around the first value (identical columns give it back exactly), the squared deviations in a
// second walk over the row.
__device__ __forceinline__ void fold_tile(const double *tile, unsigned long long *smask, unsigned long long mask, int lane, Run &run) {
  smask[lane] = mask;
  __syncthreads();
  long long n = 0;
  double ref = 0.0, s = 0.0, mn = 1.0e300, mx = -1.0e300;
  const double *row = tile + lane * kTileStride;
#pragma unroll 8
  for (int i = 0; i < 64; ++i) {
    const bool ok = (smask[i] >> lane) & 1ull;
    const double v = row[i];
    ref = (ok && n == 0) ? v : ref;
    s += ok ? v - ref : 0.0;
    mn = (ok && v < mn) ? v : mn;
    mx = (ok && v > mx) ? v : mx;
    n += ok ? 1 : 0;
  }
  if (n > 0) {
    const double mean = ref + s / (double)n;
    double m2 = 0.0;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const bool ok = (smask[i] >> lane) & 1ull;
      const double d = row[i] - mean;
      m2 += ok ? d * d : 0.0;
    }
    merge(run, n, mean, m2, mn, mx);
  }
  __syncthreads();
}

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
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(n_active, status, labels, group, ncol, blk, lane, N);
    TileSink sink{tile, lane, 0};
    layer_block(lay, ncol, N, blk, lane, na, origin, array, b0, nb, sink);
    fold_tile(tile, smask, sink.mask, lane, run);
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
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(n_active, status, labels, group, ncol, blk, lane, N);
    TileSink sink{tile, lane, 0};
    depth_block(lay, ncol, N, blk, lane, na, origin, array, b0, nb, lead, z0, dz, sink);
    fold_tile(tile, smask, sink.mask, lane, run);
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
