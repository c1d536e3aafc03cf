// samsim_profile_fold.h -- the running moments of one bin in one lane, Chan's pairwise update, and the fold of the LDS tile the
// block walk fills (samsim_profile_walk.h): shared by the profile statistics (samsim_profile.hip) and the profile regressions
// (samsim_sens.hip).  The regression is the statistics with a second variable riding along -- the column's predictor x beside the
// bin value v --, so both go through the same fold_tile and the same merge: count, mean and M2 of v are formed by the same
// operations in the same order with or without x, which is why samsim_get_profile_regression returns the count and mean bytes of
// samsim_get_profile_stats and the square of its std.  The step kernel does not include this header.
#ifndef SAMSIM_PROFILE_FOLD_H
#define SAMSIM_PROFILE_FOLD_H

#include <hip/hip_runtime.h>

#include "samsim_profile_walk.h"

namespace profile_fold {

using profile_walk::kTileStride;

// running statistics of one bin in one lane: n values with mean `mean` and sum of squared deviations `m2`
struct Run {
  long long n;
  double mean, m2, mn, mx;
};

// what rides along in a regression: the predictor's mean and sum of squared deviations over the same n columns, and the sum of
// products of the deviations of x and v
struct Co {
  double mean_x, m2_x, cxy;
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

// the same update with x riding along: the cross term of the co-moment is dx * dv * n_a * n_b / n.  v goes through merge() itself.
__device__ __forceinline__ void merge(Run &a, Co &ax, long long nb, double mean_b, double m2_b, double mn_b, double mx_b, const Co &bx) {
  if (a.n == 0) {
    ax = bx;
  } else {
    const long long n = a.n + nb;
    const double dx = bx.mean_x - ax.mean_x, dv = mean_b - a.mean;
    const double fb = (double)nb / (double)n;
    const double w = (double)a.n * fb;
    ax.mean_x = ax.mean_x + dx * fb;
    ax.m2_x = ax.m2_x + bx.m2_x + dx * dx * w;
    ax.cxy = ax.cxy + bx.cxy + dx * dv * w;
  }
  merge(a, nb, mean_b, m2_b, mn_b, mx_b);
}

// Lane j folds row j of the tile: the values of bin j of the columns whose bit j is set in their lane's mask, in lane order.
// The block's mean is formed around the first value (identical columns give it back exactly), the squared deviations in a
// second walk over the row.  PAIR: xs[i] is the predictor of the block's column i (LDS); its mean is formed the same way, and the
// second walk also sums dx * dx and dx * dv.
template <bool PAIR>
__device__ __forceinline__ void fold_tile(const double *tile, const double *xs, unsigned long long *smask, unsigned long long mask, int lane,
                                          Run &run, Co &co) {
  smask[lane] = mask;
  __syncthreads();
  long long n = 0;
  double ref = 0.0, s = 0.0, mn = 1.0e300, mx = -1.0e300;
  double refx = 0.0, sx = 0.0;
  const double *row = tile + lane * kTileStride;
#pragma unroll 8
  for (int i = 0; i < 64; ++i) {
    const bool ok = (smask[i] >> lane) & 1ull;
    const double v = row[i];
    if (PAIR) {
      const double x = xs[i];
      refx = (ok && n == 0) ? x : refx;
      sx += ok ? x - refx : 0.0;
    }
    ref = (ok && n == 0) ? v : ref;
    s += ok ? v - ref : 0.0;
    mn = (ok && v < mn) ? v : mn;
    mx = (ok && v > mx) ? v : mx;
    n += ok ? 1 : 0;
  }
  if (n > 0) {
    const double mean = ref + s / (double)n;
    const double mean_x = PAIR ? refx + sx / (double)n : 0.0;
    double m2 = 0.0, m2x = 0.0, cxy = 0.0;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const bool ok = (smask[i] >> lane) & 1ull;
      const double d = row[i] - mean;
      m2 += ok ? d * d : 0.0;
      if (PAIR) {
        const double dx = xs[i] - mean_x;
        m2x += ok ? dx * dx : 0.0;
        cxy += ok ? dx * d : 0.0;
      }
    }
    if (PAIR) merge(run, co, n, mean, m2, mn, mx, Co{mean_x, m2x, cxy});
    else merge(run, n, mean, m2, mn, mx);
  }
  __syncthreads();
}

}  // namespace profile_fold

#endif
