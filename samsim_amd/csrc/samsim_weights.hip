// samsim_weights.hip -- the weight row of the ensemble and the reductions that take it (samsim_set_weights,
// samsim_get_weighted_stats, samsim_get_weighted_histogram, samsim_get_weighted_covariance, include/samsim.h): posterior statistics
// with w ~ exp(-J / 2) formed and applied on the device.
//
// Every kernel is the walk and the bracket of samsim_slot_walk.h (the weighted moments spell theirs out, see there).  A lane
// keeps its own running sums (West's weighted update for the moments, every slot of the request in one walk: a template on nslots);
// at the end the 64 lanes are combined in lane order through LDS and the wave's partial is stored; a merge kernel combines the waves' partials.
// The weighted histogram adds a block's weights to the wave's LDS table in lane order -- ascending column order --, the lane that
// owns an entry (entry mod 64) doing the addition, and a second kernel adds the waves' tables.
// The weighted covariances are the weighted moments with the co-moments of every pair of slots riding along: the same lane update,
// the same lane-to-wave order and the same merge, so their diagonal is samsim_get_weighted_stats byte for byte.
//
// No atomics of any kind, no floating-point sum whose order depends on scheduling: two calls return the same bytes.  The kernels
// read slots, status and labels and write the weight row and the handle's weight scratch, nothing else.
#include <hip/hip_runtime.h>

#include <cmath>

#include "samsim_pow.h"
#include "samsim_weights.h"

namespace {

using namespace slot_walk;

// ------------------------------------------------------------------------------------------------------------- the weight row

// a minimum and how many values it is of
struct MinAcc {
  double mn;
  long long n;
  __device__ __forceinline__ void absorb(const MinAcc &b) {
    mn = b.mn < mn ? b.mn : mn;
    n += b.n;
  }
};
// n_in, n_pos, sum_w and sum_w2 of a stretch of the weight row
struct SumAcc {
  double sw, sw2;
  long long n_in, n_pos;
  __device__ __forceinline__ void absorb(const SumAcc &b) {
    sw = sw + b.sw; sw2 = sw2 + b.sw2;
    n_in += b.n_in; n_pos += b.n_pos;
  }
};

// x_min of SAMSIM_WEIGHT_GAUSS: the minimum over the IN columns whose x is not a NaN, and how many there are
__global__ void __launch_bounds__(64) weight_min_kernel(const double *__restrict__ x, ColSet cs, WeightPartial *__restrict__ part) {
  __shared__ MinAcc s_acc[64];
  const int lane = threadIdx.x;
  MinAcc acc{INFINITY, 0};
  walk_blocks<Cols<1>>(
      cs.ncol, lane, [&](long long blk, int ln, Cols<1> &col) { load_cols(cs, x, nullptr, blk, ln, col); },
      [&](long long, const Cols<1> &col) {
        if (col.ok && col.v[0] == col.v[0]) acc.absorb(MinAcc{col.v[0], 1});
      });
  if (!fold_lanes(acc, s_acc, lane)) return;
  part[blockIdx.x].x_min = acc.mn;
  part[blockIdx.x].n_pos = acc.n;
}

__global__ void __launch_bounds__(64) weight_min_merge_kernel(const WeightPartial *__restrict__ part, int nwaves,
                                                              WeightPartial *__restrict__ out) {
  __shared__ MinAcc s_acc[64];
  MinAcc acc{INFINITY, 0};
  if (!merge_waves(nwaves, acc, s_acc, threadIdx.x, [&](int w) { return MinAcc{part[w].x_min, part[w].n_pos}; })) return;
  out->x_min = acc.n > 0 ? acc.mn : 0.0;   // no IN column with a value: every t below is a NaN, every weight 0.0
}

// the weight of one IN column.  GAUSS: t is a difference and a product, each rounded (no fused multiply-add); a NaN x or t compares
// false and gives 0.0.  DIRECT: x where it is positive and finite.
template <int KIND>
__device__ __forceinline__ double weight_of(double x, double x_min, double c) {
  if (KIND == SAMSIM_WEIGHT_DIRECT) return (x > 0.0 && x < INFINITY) ? x : 0.0;
  const double t = (x - x_min) * c;
  return t < 690.0 ? sp_exp(-t) : 0.0;
}

// every column of the handle gets its weight (0.0 where it is not IN); the wave's n_in, n_pos, sum_w and sum_w2
template <int KIND>
__global__ void __launch_bounds__(64) weight_fill_kernel(const double *__restrict__ x, ColSet cs, const WeightPartial *__restrict__ xmin_at,
                                                         double c, double *__restrict__ w, WeightPartial *__restrict__ part) {
  __shared__ SumAcc s_acc[64];
  const int lane = threadIdx.x;
  const double x_min = xmin_at->x_min;
  SumAcc acc{0.0, 0.0, 0, 0};
  walk_blocks<Cols<1>>(
      cs.ncol, lane, [&](long long blk, int ln, Cols<1> &col) { load_cols(cs, x, nullptr, blk, ln, col); },
      [&](long long blk, const Cols<1> &col) {
        const long long at = blk * 64 + lane;
        const double wv = col.ok ? weight_of<KIND>(col.v[0], x_min, c) : 0.0;
        if (at < cs.ncol) w[at] = wv;
        if (col.ok) acc.n_in += 1;
        if (wv > 0.0) {
          acc.n_pos += 1;
          acc.sw = acc.sw + wv;
          acc.sw2 = acc.sw2 + wv * wv;
        }
      });
  if (!fold_lanes(acc, s_acc, lane)) return;
  WeightPartial p;
  p.x_min = x_min; p.sum_w = acc.sw; p.sum_w2 = acc.sw2; p.n_in = acc.n_in; p.n_pos = acc.n_pos;
  part[blockIdx.x] = p;
}

__global__ void __launch_bounds__(64) weight_sum_merge_kernel(const WeightPartial *__restrict__ part, int nwaves,
                                                              WeightPartial *__restrict__ out) {
  __shared__ SumAcc s_acc[64];
  SumAcc acc{0.0, 0.0, 0, 0};
  const bool last = merge_waves(nwaves, acc, s_acc, threadIdx.x, [&](int w) {
    return SumAcc{part[w].sum_w, part[w].sum_w2, part[w].n_in, part[w].n_pos};
  });
  if (!last) return;
  out->sum_w = acc.sw; out->sum_w2 = acc.sw2; out->n_in = acc.n_in; out->n_pos = acc.n_pos;   // x_min stays what weight_min_merge_kernel left
}

// ---------------------------------------------------------------------------------------------------------- weighted moments

// This family keeps the kernels it had before samsim_slot_walk.h: wstat_kernel over walk_blocks and load_cols with wstat_merge_kernel
// over merge_waves measured 7 to 9 % slower than they (tools/weighted_profile_bench.py, weighted_stats of one slot and of eight:
// 0.0756 -> 0.0823 ms and 0.0975 -> 0.1045 ms at a run-to-run spread of 0.004 ms; profiles/r21_refactor_ab_first_form.json,
// docs/HISTORY.md).  The loader, the loop and the bracket below are those of the header, written out; the bytes are the same.

// Running weighted moments: n columns of total weight W, the weighted mean and the weighted sum of squared deviations
struct WRun {
  long long n;
  double W, W2, mean, m2, mn, mx;
  // West: the first value of a lane is its mean exactly (w / W == 1), equal values leave the mean and M2 alone (d is 0)
  __device__ __forceinline__ void push(double x, double w) {
    n += 1;
    W = W + w;
    W2 = W2 + w * w;
    const double d = x - mean;
    mean = mean + d * (w / W);
    m2 = m2 + w * d * (x - mean);
    mn = x < mn ? x : mn;
    mx = x > mx ? x : mx;
  }
  // Chan et al. with weights in the place of counts: the cross term is delta^2 W_a W_b / W; b is not empty
  __device__ __forceinline__ void merge(const WStatPartial &b) {
    if (n == 0) {
      n = b.n; W = b.W; W2 = b.W2; mean = b.mean; m2 = b.m2; mn = b.mn; mx = b.mx;
      return;
    }
    const double Wn = W + b.W;
    const double delta = b.mean - mean;
    const double fb = b.W / Wn;
    mean = mean + delta * fb;
    m2 = m2 + b.m2 + delta * delta * (W * fb);
    W = Wn;
    W2 = W2 + b.W2;
    n += b.n;
    mn = b.mn < mn ? b.mn : mn;
    mx = b.mx > mx ? b.mx : mx;
  }
  __device__ __forceinline__ WStatPartial partial() const {
    WStatPartial p;
    p.W = W; p.W2 = W2; p.mean = mean; p.m2 = m2; p.mn = mn; p.mx = mx; p.n = n;
    return p;
  }
};
__device__ __forceinline__ WRun empty_run() { return WRun{0, 0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY}; }

// the lane's column of block blk: whether it counts (IN and w > 0), its weight and its values of the NS slots
template <int NS>
__device__ __forceinline__ void load_slots(const SensRows &rows, const double *w, const int32_t *n_active, const int32_t *status,
                                           const int32_t *labels, int group, long long ncol, long long blk, int lane, bool &ok, double &wv,
                                           double (&v)[NS]) {
  const long long col = blk * 64 + lane;
  ok = false; wv = 0.0;
#pragma unroll
  for (int i = 0; i < NS; ++i) v[i] = 0.0;
  if (col < ncol) {
    wv = w[col];
    ok = status[col] == 0 && (!labels || labels[col] == group) && wv > 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i] = rows.row[i] ? rows.row[i][col] : (double)n_active[col];
  }
}

// One walk serves every slot of the request (a template on nslots: every index is a compile-time one, as in cov_kernel).  The
// operations on a slot do not depend on the others, so a slot has the bytes it would have alone.
template <int NS>
__global__ void __launch_bounds__(64) wstat_kernel(SensRows rows, const double *__restrict__ w, const int32_t *__restrict__ n_active,
                                                   const int32_t *__restrict__ status, const int32_t *__restrict__ labels, int group,
                                                   long long ncol, WStatPartial *__restrict__ part) {
  __shared__ WStatPartial s_run[NS * 64];   // [slot][lane]
  const int lane = threadIdx.x;
  const long long nblk = (ncol + 63) / 64;
  WRun run[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) run[i] = empty_run();
  bool ok, ok_next = false;
  double wv, wv_next = 0.0, v[NS], v_next[NS];
  load_slots<NS>(rows, w, n_active, status, labels, group, ncol, blockIdx.x, lane, ok, wv, v);
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    // the next block's loads are under way while this block is consumed
    if (blk + gridDim.x < nblk) load_slots<NS>(rows, w, n_active, status, labels, group, ncol, blk + gridDim.x, lane, ok_next, wv_next, v_next);
    if (ok) {
#pragma unroll
      for (int i = 0; i < NS; ++i) run[i].push(v[i], wv);
    }
    ok = ok_next; wv = wv_next;
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i] = v_next[i];
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) s_run[i * 64 + lane] = run[i].partial();
  __syncthreads();
  if (lane >= NS) return;
  // the 64 lanes in lane order, one thread per slot
  WRun all = empty_run();
  for (int l = 0; l < 64; ++l)
    if (s_run[lane * 64 + l].n > 0) all.merge(s_run[lane * 64 + l]);
  part[(size_t)blockIdx.x * SAMSIM_SENS_MAX_SLOTS + lane] = all.partial();
}

// one workgroup per slot: the waves' partials in wave order
__global__ void __launch_bounds__(64) wstat_merge_kernel(const WStatPartial *__restrict__ part, int nwaves, samsim_wstat *__restrict__ out) {
  __shared__ WStatPartial s_run[64];
  const int lane = threadIdx.x, slot = blockIdx.x, per = (nwaves + 63) / 64;
  WRun run = empty_run();
  for (int w = lane * per; w < (lane + 1) * per && w < nwaves; ++w) {
    const WStatPartial p = part[(size_t)w * SAMSIM_SENS_MAX_SLOTS + slot];
    if (p.n > 0) run.merge(p);
  }
  s_run[lane] = run.partial();
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < 64; ++l)
    if (s_run[l].n > 0) run.merge(s_run[l]);
  samsim_wstat st;
  st.count = run.n;
  if (run.n > 0) {
    st.sum_w = run.W; st.sum_w2 = run.W2; st.mean = run.mean; st.var = run.m2 / run.W; st.min = run.mn; st.max = run.mx;
  } else {
    st.sum_w = st.sum_w2 = st.mean = st.var = st.min = st.max = 0.0;
  }
  out[slot] = st;
}

// ------------------------------------------------------------------------------------------------------ weighted covariances

// Running weighted moments of one pair of slots (i, j): n columns of total weight W, the two weighted means, the weighted sum of
// products of deviations.  WRun::merge with a second variable: for i == j every operation is that of WRun::merge on m2, and every
// update is symmetric in i and j down to the bits, so a slot listed twice gives the bytes of its variance.
struct WPairAcc {
  long long n;
  double W, W2, mi, mj, c;
  // the cross term is delta_i delta_j W_a W_b / W; b is not empty
  __device__ __forceinline__ void add(long long nb, double W_b, double W2_b, double mi_b, double mj_b, double c_b) {
    if (n == 0) {
      n = nb; W = W_b; W2 = W2_b; mi = mi_b; mj = mj_b; c = c_b;
      return;
    }
    const double Wn = W + W_b;
    const double di = mi_b - mi, dj = mj_b - mj;
    const double fb = W_b / Wn;
    mi = mi + di * fb;
    mj = mj + dj * fb;
    c = c + c_b + di * dj * (W * fb);
    W = Wn;
    W2 = W2 + W2_b;
    n += nb;
  }
  __device__ __forceinline__ void absorb(const WPairAcc &b) {
    if (b.n > 0) add(b.n, b.W, b.W2, b.mi, b.mj, b.c);
  }
};

// One walk serves every slot and every pair of the request (a template on nslots: every index is a compile-time one).  A lane
// applies WRun::push to the means -- West's update -- and C_ij += w * d_i * (x_j - mean_j) with mean_j already updated, which for
// i == j is the m2 of WRun::push, operation for operation; then the 64 lanes in lane order through LDS, one thread per pair.
// (Not cov_kernel's lane update with a weight: d_i * d_j * (n - 1) / n rounds differently.)
template <int NS>
__global__ void __launch_bounds__(64) wcov_kernel(SensRows rows, const double *__restrict__ w, ColSet cs, double *__restrict__ part) {
  constexpr int NP = NS * (NS + 1) / 2;
  __shared__ double s[(3 + NS + NP) * kLaneStride];   // [n, W, W2, means, co-moments][lane]
  const int lane = threadIdx.x;
  long long n = 0;
  double W = 0.0, W2 = 0.0, mean[NS], C[NP];
#pragma unroll
  for (int i = 0; i < NS; ++i) mean[i] = 0.0;
#pragma unroll
  for (int p = 0; p < NP; ++p) C[p] = 0.0;
  walk_blocks<Cols<NS>>(
      cs.ncol, lane, [&](long long blk, int ln, Cols<NS> &c) { load_cols<NS>(cs, rows.row, w, blk, ln, c); },
      [&](long long, const Cols<NS> &c) {
        if (!c.ok) return;
        n += 1;
        W = W + c.w;
        W2 = W2 + c.w * c.w;
        double wd[NS], e[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const double d = c.v[i] - mean[i];
          mean[i] = mean[i] + d * (c.w / W);
          wd[i] = c.w * d;
          e[i] = c.v[i] - mean[i];
        }
        int p = 0;
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
          for (int j = i; j < NS; ++j, ++p) C[p] = C[p] + wd[i] * e[j];
      });
  s[lane] = (double)n; s[kLaneStride + lane] = W; s[2 * kLaneStride + lane] = W2;
#pragma unroll
  for (int i = 0; i < NS; ++i) s[(3 + i) * kLaneStride + lane] = mean[i];
#pragma unroll
  for (int p = 0; p < NP; ++p) s[(3 + NS + p) * kLaneStride + lane] = C[p];
  __syncthreads();
  if (lane >= NP) return;
  // the 64 lanes in lane order, one thread per pair of slots
  int i, j;
  pair_of(lane, NS, i, j);
  WPairAcc acc{0, 0.0, 0.0, 0.0, 0.0, 0.0};
  absorb_lanes(acc, [&](int l) {
    return WPairAcc{(long long)s[l],
                    s[kLaneStride + l],
                    s[2 * kLaneStride + l],
                    s[(3 + i) * kLaneStride + l],
                    s[(3 + j) * kLaneStride + l],
                    s[(3 + NS + lane) * kLaneStride + l]};
  });
  double *mine = part + (size_t)blockIdx.x * DEV_WCOV_PART;
  mine[DEV_WCOV_C0 + lane] = acc.c;
  if (i == j) mine[DEV_WCOV_MEAN0 + i] = acc.mi;
  if (lane == 0) { mine[0] = (double)acc.n; mine[1] = acc.W; mine[2] = acc.W2; }
}

// One workgroup per pair of slots: the waves' partials in wave order.  The pair (i, j) goes to cov[i][j] and cov[j][i]: one
// value, stored twice.
__global__ void __launch_bounds__(64) wcov_merge_kernel(const double *__restrict__ part, int nwaves, int ns, WCovResult *__restrict__ out) {
  __shared__ WPairAcc s_acc[64];
  const int p = blockIdx.x;
  int i, j;
  pair_of(p, ns, i, j);
  WPairAcc acc{0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const bool last = merge_waves(nwaves, acc, s_acc, threadIdx.x, [&](int wv) {
    const double *q = part + (size_t)wv * DEV_WCOV_PART;
    return WPairAcc{(long long)q[0], q[1], q[2], q[DEV_WCOV_MEAN0 + i], q[DEV_WCOV_MEAN0 + j], q[DEV_WCOV_C0 + p]};
  });
  if (!last) return;
  const double cov = acc.n > 0 ? acc.c / acc.W : 0.0;
  out->cov[i * ns + j] = cov;
  out->cov[j * ns + i] = cov;
  if (i == j) out->mean[i] = acc.n > 0 ? acc.mi : 0.0;
  if (p == 0) {
    out->count = acc.n;
    out->sum_w = acc.n > 0 ? acc.W : 0.0;
    out->sum_w2 = acc.n > 0 ? acc.W2 : 0.0;
  }
}

// -------------------------------------------------------------------------------------------------------- weighted histogram

__global__ void __launch_bounds__(64) whist_kernel(const double *__restrict__ x, const double *__restrict__ w, ColSet cs, HistEdges e,
                                                   double *__restrict__ tables) {
  __shared__ double table[DEV_WEIGHT_ENTRIES];
  const int lane = threadIdx.x, W = e.nvbins + 2;
  for (int i = lane; i < W; i += 64) table[i] = 0.0;
  __syncthreads();
  walk_blocks<Cols<1>>(
      cs.ncol, lane, [&](long long blk, int ln, Cols<1> &c) { load_cols(cs, x, w, blk, ln, c); },
      [&](long long, const Cols<1> &c) {
        const int entry = c.ok ? hist_entry(c.v[0], e) : 0;
        unsigned long long todo = __ballot(c.ok);
        while (todo) {   // the lanes whose column counts, in lane order; only the owner of an entry ever touches it
          const int i = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const int en = __builtin_amdgcn_readlane(entry, i);
          const double wi = lane_value(c.w, i);
          if (lane == (en & 63)) table[en] = table[en] + wi;
        }
      });
  __syncthreads();
  for (int i = lane; i < W; i += 64) tables[(size_t)blockIdx.x * DEV_WEIGHT_ENTRIES + i] = table[i];
}

// a plain sum: every partial is added, in order
struct SumOf {
  double s;
  __device__ __forceinline__ void absorb(const SumOf &b) { s = s + b.s; }
};

// one workgroup per entry: the waves' tables in wave order
__global__ void __launch_bounds__(64) whist_merge_kernel(const double *__restrict__ tables, int nwaves, double *__restrict__ out) {
  __shared__ SumOf s_sum[64];
  const int entry = blockIdx.x;
  SumOf sum{0.0};
  if (merge_waves(nwaves, sum, s_sum, threadIdx.x, [&](int w) { return SumOf{tables[(size_t)w * DEV_WEIGHT_ENTRIES + entry]}; }))
    out[entry] = sum.s;
}

}  // namespace

extern "C" hipError_t samsim_launch_set_weights(ColSet cs, const double *x, int kind, double c, double *w, WeightPartial *part,
                                                WeightPartial *out, hipStream_t stream) {
  const int grid = slot_grid(cs.ncol, DEV_WEIGHT_GRID);
  hipError_t e = hipMemsetAsync(out, 0, sizeof(WeightPartial), stream);   // x_min of DIRECT is 0.0
  if (e != hipSuccess) return e;
  if (kind == SAMSIM_WEIGHT_GAUSS) {
    hipLaunchKernelGGL(weight_min_kernel, dim3(grid), dim3(64), 0, stream, x, cs, part);
    hipLaunchKernelGGL(weight_min_merge_kernel, dim3(1), dim3(64), 0, stream, part, grid, out);
    hipLaunchKernelGGL(weight_fill_kernel<SAMSIM_WEIGHT_GAUSS>, dim3(grid), dim3(64), 0, stream, x, cs, out, c, w, part);
  } else if (kind == SAMSIM_WEIGHT_DIRECT) {
    hipLaunchKernelGGL(weight_fill_kernel<SAMSIM_WEIGHT_DIRECT>, dim3(grid), dim3(64), 0, stream, x, cs, out, c, w, part);
  } else {
    return hipErrorInvalidValue;
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(weight_sum_merge_kernel, dim3(1), dim3(64), 0, stream, part, grid, out);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_weighted_stats(ColSet cs, SensRows rows, int nslots, const double *w, WStatPartial *part,
                                                   samsim_wstat *out, hipStream_t stream) {
  const int grid = slot_grid(cs.ncol, DEV_WEIGHT_GRID);
  const bool known = dispatch_nslots(nslots, [&](auto ns) {
    hipLaunchKernelGGL(wstat_kernel<decltype(ns)::value>, dim3(grid), dim3(64), 0, stream, rows, w, cs.n_active, cs.status, cs.labels,
                       cs.group, cs.ncol, part);
  });
  if (!known) return hipErrorInvalidValue;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wstat_merge_kernel, dim3(nslots), dim3(64), 0, stream, part, grid, out);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_weighted_hist(ColSet cs, const double *x, const double *w, HistEdges e, double *tables, double *out,
                                                  hipStream_t stream) {
  const int grid = slot_grid(cs.ncol, DEV_WEIGHT_GRID);
  if (e.nvbins < 1 || e.nvbins + 2 > DEV_WEIGHT_ENTRIES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(whist_kernel, dim3(grid), dim3(64), 0, stream, x, w, cs, e, tables);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(whist_merge_kernel, dim3(e.nvbins + 2), dim3(64), 0, stream, tables, grid, out);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_weighted_covariance(ColSet cs, SensRows rows, int nslots, const double *w, double *part,
                                                        WCovResult *out, hipStream_t stream) {
  const int grid = slot_grid(cs.ncol, DEV_WEIGHT_GRID);
  const bool known = dispatch_nslots(nslots, [&](auto ns) {
    hipLaunchKernelGGL(wcov_kernel<decltype(ns)::value>, dim3(grid), dim3(64), 0, stream, rows, w, cs, part);
  });
  if (!known) return hipErrorInvalidValue;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wcov_merge_kernel, dim3(nslots * (nslots + 1) / 2), dim3(64), 0, stream, part, grid, nslots, out);
  return hipGetLastError();
}
