// samsim_profile.hip -- device-side ensemble statistics of the layer profiles (samsim_get_profile_stats, include/samsim.h).
//
// The pass, its grid and its launch are those of samsim_profile.h, the walk that fills the LDS tile [bin][lane] that of
// samsim_profile_walk.h.  After the block, lane j folds row j of the tile in lane order into its own running
// (n, mean, M2, min, max) of bin j (samsim_profile_fold.h): a transposition through LDS, no cross-lane reduction, no atomics.  At the
// end every wave stores its 64 partials; profile_merge_kernel combines the waves' partials in wave order (Chan's pairwise update).
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

template <int AXIS>
__global__ void __launch_bounds__(64) profile_kernel(ProfPass p, ProfPartial *__restrict__ part) {
  __shared__ double tile[DEV_PROF_BINS * kTileStride];
  __shared__ unsigned long long smask[64];
  const int lane = threadIdx.x;
  const long long nblk = (p.ncol + 63) / 64;
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  Co none{0.0, 0.0, 0.0};   // no predictor rides along
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(p, blk, lane);
    TileSink sink{tile, lane, 0};
    walk_block<AXIS>(p, blk, lane, na, sink);
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

extern "C" hipError_t samsim_launch_profile(ProfPass p, ProfPartial *part, samsim_stat *out, hipStream_t stream) {
  return launch_tile_pass(profile_kernel<SAMSIM_PROFILE_BY_LAYER>, profile_kernel<SAMSIM_PROFILE_BY_DEPTH>, profile_merge_kernel,
                          DEV_PROF_GRID, p, stream, part, out);
}
