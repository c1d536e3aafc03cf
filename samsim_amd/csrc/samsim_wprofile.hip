// samsim_wprofile.hip -- device-side weighted statistics of the layer profiles (samsim_get_weighted_profile_stats, include/samsim.h):
// the posterior mean, variance, extremes and effective sample size of every depth bin, with the weight row of samsim_set_weights.
//
// A pass is that of the profile statistics (samsim_profile.h), with their grid and their walk (samsim_profile_walk.h), which drops
// every finished bin value into the LDS tile [bin][lane].  A column whose weight is not positive enters the walk with no active layers, as a stopped one does.  The
// block's 64 weights lie beside the tile, as the predictor of the regressions does (samsim_sens.hip), and lane j folds row j with
// fold_tile_weighted below: the fold of samsim_profile_fold.h with every term multiplied by its weight and the total weight W in the
// place of the count.  At the end every wave stores its 64 partials; wprofile_merge_kernel combines them in wave order, as
// profile_merge_kernel does.  With unit weights every product with w is exact and every W is the count as a double, so the
// operations are those of the unweighted call, value for value: count, mean, min and max are its bytes and sqrt(var) its std.
//
// No atomics of any kind, no floating-point sum whose order depends on scheduling: two calls return the same bytes.  The kernels
// read the layer block, n_active, status, the labels and the weight row and write the handle's scratch, nothing else.
#include <hip/hip_runtime.h>

#include "samsim_profile_walk.h"
#include "samsim_wprofile.h"

namespace {

using namespace profile_walk;   // the block walk the reductions share (samsim_profile_walk.h)

// running weighted statistics of one bin in one lane: n values of total weight W (sum of squared weights W2) with weighted mean
// `mean` and weighted sum of squared deviations `m2`
struct WRun {
  long long n;
  double W, W2, mean, m2, mn, mx;
};

// Chan et al. with the weights in the place of the counts (profile_fold::merge with W for n): b is not empty
__device__ __forceinline__ void merge(WRun &a, long long nb, double W_b, double W2_b, double mean_b, double m2_b, double mn_b, double mx_b) {
  if (a.n == 0) {
    a.n = nb; a.W = W_b; a.W2 = W2_b; a.mean = mean_b; a.m2 = m2_b; a.mn = mn_b; a.mx = mx_b;
    return;
  }
  const double W = a.W + W_b;
  const double delta = mean_b - a.mean;
  const double fb = W_b / W;
  a.mean = a.mean + delta * fb;
  a.m2 = a.m2 + m2_b + delta * delta * (a.W * fb);
  a.W = W;
  a.W2 = a.W2 + W2_b;
  a.n += nb;
  a.mn = mn_b < a.mn ? mn_b : a.mn;
  a.mx = mx_b > a.mx ? mx_b : a.mx;
}

// Lane j folds row j of the tile: the values of bin j of the columns whose bit j is set in their lane's mask, in lane order, each
// with its column's weight ws[i] (LDS; positive wherever a bit is set).  The block's mean is formed around the first value --
// ref + sum w (v - ref) / sum w, so identical columns give it back exactly whatever the weights --, the weighted squared deviations
// sum w d^2 in a second walk over the row.
__device__ __forceinline__ void fold_tile_weighted(const double *tile, const double *ws, unsigned long long *smask, unsigned long long mask,
                                                   int lane, WRun &run) {
  smask[lane] = mask;
  __syncthreads();
  long long n = 0;
  double ref = 0.0, s = 0.0, W = 0.0, W2 = 0.0, mn = 1.0e300, mx = -1.0e300;
  const double *row = tile + lane * kTileStride;
#pragma unroll 8
  for (int i = 0; i < 64; ++i) {
    const bool ok = (smask[i] >> lane) & 1ull;
    const double v = row[i], w = ws[i];
    ref = (ok && n == 0) ? v : ref;
    s += ok ? w * (v - ref) : 0.0;
    W += ok ? w : 0.0;
    W2 += ok ? w * w : 0.0;
    mn = (ok && v < mn) ? v : mn;
    mx = (ok && v > mx) ? v : mx;
    n += ok ? 1 : 0;
  }
  if (n > 0) {
    const double mean = ref + s / W;
    double m2 = 0.0;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const bool ok = (smask[i] >> lane) & 1ull;
      const double d = row[i] - mean;
      m2 += ok ? ws[i] * (d * d) : 0.0;
    }
    merge(run, n, W, W2, mean, m2, mn, mx);
  }
  __syncthreads();
}

// the lane's column of block blk: its weight (0.0 beyond ncol) and its number of active layers, 0 for a column that does not count
__device__ __forceinline__ int counting_layers(const ProfPass &p, const double *w, long long blk, int lane, double &wv) {
  const long long col = blk * 64 + lane;
  wv = col < p.ncol ? w[col] : 0.0;
  const int na = active_layers(p, blk, lane);
  return wv > 0.0 ? na : 0;
}

__device__ __forceinline__ void store_partials(WProfPartial *part, int lane, const WRun &run) {
  WProfPartial p;
  p.W = run.W; p.W2 = run.W2; p.mean = run.mean; p.m2 = run.m2; p.mn = run.mn; p.mx = run.mx; p.n = run.n;
  part[(size_t)blockIdx.x * DEV_PROF_BINS + lane] = p;
}

template <int AXIS>
__global__ void __launch_bounds__(64) wprofile_kernel(ProfPass p, const double *__restrict__ w, WProfPartial *__restrict__ part) {
  __shared__ double tile[DEV_PROF_BINS * kTileStride];
  __shared__ unsigned long long smask[64];
  __shared__ double ws[64];   // the block's weights, lane by lane
  const int lane = threadIdx.x;
  const long long nblk = (p.ncol + 63) / 64;
  WRun run{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    double wv;
    const int na = counting_layers(p, w, blk, lane, wv);
    TileSink sink{tile, lane, 0};
    walk_block<AXIS>(p, blk, lane, na, sink);
    ws[lane] = wv;
    fold_tile_weighted(tile, ws, smask, sink.mask, lane, run);
  }
  store_partials(part, lane, run);
}

// the waves' partials of one pass, combined in wave order; thread j writes bin b0 + j of the pass's array
__global__ void __launch_bounds__(64) wprofile_merge_kernel(const WProfPartial *__restrict__ part, int nwaves, int nb,
                                                            samsim_wstat *__restrict__ out) {
  const int j = threadIdx.x;
  if (j >= nb) return;
  WRun run{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int wv = 0; wv < nwaves; ++wv) {
    const WProfPartial p = part[(size_t)wv * DEV_PROF_BINS + j];
    if (p.n > 0) merge(run, p.n, p.W, p.W2, p.mean, p.m2, p.mn, p.mx);
  }
  samsim_wstat st;
  st.count = run.n;
  if (run.n > 0) {
    st.sum_w = run.W; st.sum_w2 = run.W2; st.mean = run.mean; st.var = run.m2 / run.W; st.min = run.mn; st.max = run.mx;
  } else {
    st.sum_w = st.sum_w2 = st.mean = st.var = st.min = st.max = 0.0;
  }
  out[j] = st;
}

}  // namespace

extern "C" hipError_t samsim_launch_weighted_profile(ProfPass p, const double *w, WProfPartial *part, samsim_wstat *out,
                                                     hipStream_t stream) {
  return launch_tile_pass(wprofile_kernel<SAMSIM_PROFILE_BY_LAYER>, wprofile_kernel<SAMSIM_PROFILE_BY_DEPTH>, wprofile_merge_kernel,
                          DEV_PROF_GRID, p, stream, part, out, w);
}
