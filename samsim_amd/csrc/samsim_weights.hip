// samsim_weights.hip -- the weight row of the ensemble and the reductions that take it (samsim_set_weights,
// samsim_get_weighted_stats, samsim_get_weighted_histogram, samsim_get_weighted_covariance, include/samsim.h): posterior statistics
// with w ~ exp(-J / 2) formed and applied on the device.
//
// Every kernel follows the unweighted reductions: one wave owns one 64-column block at a time (lane = column) and strides over the
// blocks with a fixed grid; its loads of the rows, of status and of the labels are coalesced and the next block's are under way
// while this block is consumed.  A lane keeps its own running sums (West's weighted update for the moments, every slot of the
// request in one walk: a template on nslots, as cov_kernel is); at the end the 64 lanes are combined in lane order through LDS and
// the wave's partial is stored; a merge kernel combines the waves' partials in wave order, bracketed as group_merge_kernel brackets
// them (lane l the waves [l * per, (l + 1) * per), then the lanes in order).
// The weighted histogram adds a block's weights to the wave's LDS table in lane order -- ascending column order --, the lane that
// owns an entry (entry mod 64) doing the addition, and a second kernel adds the waves' tables in the same bracketing.
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

// the lane's column of block blk: whether it is IN (status 0, within ncol, the right label) and its value of the source row
__device__ __forceinline__ void load_x(const double *x, const int32_t *n_active, const int32_t *status, const int32_t *labels, int group,
                                       long long ncol, long long blk, int lane, bool &in, double &v) {
  const long long col = blk * 64 + lane;
  in = false; v = 0.0;
  if (col < ncol) {
    in = status[col] == 0 && (!labels || labels[col] == group);
    v = x ? x[col] : (double)n_active[col];
  }
}
// the same with the column's weight: the column counts if it is IN and w > 0
__device__ __forceinline__ void load_xw(const double *x, const double *w, const int32_t *n_active, const int32_t *status,
                                        const int32_t *labels, int group, long long ncol, long long blk, int lane, bool &ok, double &v,
                                        double &wv) {
  load_x(x, n_active, status, labels, group, ncol, blk, lane, ok, v);
  wv = blk * 64 + lane < ncol ? w[blk * 64 + lane] : 0.0;
  ok = ok && wv > 0.0;
}

// the waves [l * per, (l + 1) * per) of lane l: the bracketing of every merge below
__device__ __forceinline__ int waves_per_lane(int nwaves) { return (nwaves + 63) / 64; }

// ------------------------------------------------------------------------------------------------------------- the weight row

// x_min of SAMSIM_WEIGHT_GAUSS: the minimum over the IN columns whose x is not a NaN, and how many there are
__global__ void __launch_bounds__(64) weight_min_kernel(const double *__restrict__ x, const int32_t *__restrict__ n_active,
                                                        const int32_t *__restrict__ status, const int32_t *__restrict__ labels, int group,
                                                        long long ncol, WeightPartial *__restrict__ part) {
  __shared__ double s_mn[64];
  __shared__ long long s_n[64];
  const int lane = threadIdx.x;
  const long long nblk = (ncol + 63) / 64;
  double mn = INFINITY;
  long long n = 0;
  bool in, in_next = false;
  double v, v_next = 0.0;
  load_x(x, n_active, status, labels, group, ncol, blockIdx.x, lane, in, v);
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    // the next block's loads are under way while this block is consumed
    if (blk + gridDim.x < nblk) load_x(x, n_active, status, labels, group, ncol, blk + gridDim.x, lane, in_next, v_next);
    if (in && v == v) {
      mn = v < mn ? v : mn;
      n += 1;
    }
    in = in_next; v = v_next;
  }
  s_mn[lane] = mn; s_n[lane] = n;
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < 64; ++l) {
    mn = s_mn[l] < mn ? s_mn[l] : mn;
    n += s_n[l];
  }
  part[blockIdx.x].x_min = mn;
  part[blockIdx.x].n_pos = n;
}

__global__ void __launch_bounds__(64) weight_min_merge_kernel(const WeightPartial *__restrict__ part, int nwaves,
                                                              WeightPartial *__restrict__ out) {
  __shared__ double s_mn[64];
  __shared__ long long s_n[64];
  const int lane = threadIdx.x, per = waves_per_lane(nwaves);
  double mn = INFINITY;
  long long n = 0;
  for (int w = lane * per; w < (lane + 1) * per && w < nwaves; ++w) {
    mn = part[w].x_min < mn ? part[w].x_min : mn;
    n += part[w].n_pos;
  }
  s_mn[lane] = mn; s_n[lane] = n;
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < 64; ++l) {
    mn = s_mn[l] < mn ? s_mn[l] : mn;
    n += s_n[l];
  }
  out->x_min = n > 0 ? mn : 0.0;   // no IN column with a value: every t below is a NaN, every weight 0.0
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
__global__ void __launch_bounds__(64) weight_fill_kernel(const double *__restrict__ x, const int32_t *__restrict__ n_active,
                                                         const int32_t *__restrict__ status, const int32_t *__restrict__ labels, int group,
                                                         long long ncol, const WeightPartial *__restrict__ xmin_at, double c,
                                                         double *__restrict__ w, WeightPartial *__restrict__ part) {
  __shared__ double s_w[64], s_w2[64];
  __shared__ long long s_in[64], s_pos[64];
  const int lane = threadIdx.x;
  const long long nblk = (ncol + 63) / 64;
  const double x_min = xmin_at->x_min;
  double sw = 0.0, sw2 = 0.0;
  long long n_in = 0, n_pos = 0;
  bool in, in_next = false;
  double v, v_next = 0.0;
  load_x(x, n_active, status, labels, group, ncol, blockIdx.x, lane, in, v);
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    if (blk + gridDim.x < nblk) load_x(x, n_active, status, labels, group, ncol, blk + gridDim.x, lane, in_next, v_next);
    const long long col = blk * 64 + lane;
    const double wv = in ? weight_of<KIND>(v, x_min, c) : 0.0;
    if (col < ncol) w[col] = wv;
    if (in) n_in += 1;
    if (wv > 0.0) {
      n_pos += 1;
      sw = sw + wv;
      sw2 = sw2 + wv * wv;
    }
    in = in_next; v = v_next;
  }
  s_w[lane] = sw; s_w2[lane] = sw2; s_in[lane] = n_in; s_pos[lane] = n_pos;
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < 64; ++l) {
    sw = sw + s_w[l]; sw2 = sw2 + s_w2[l];
    n_in += s_in[l]; n_pos += s_pos[l];
  }
  WeightPartial p;
  p.x_min = x_min; p.sum_w = sw; p.sum_w2 = sw2; p.n_in = n_in; p.n_pos = n_pos;
  part[blockIdx.x] = p;
}

__global__ void __launch_bounds__(64) weight_sum_merge_kernel(const WeightPartial *__restrict__ part, int nwaves,
                                                              WeightPartial *__restrict__ out) {
  __shared__ double s_w[64], s_w2[64];
  __shared__ long long s_in[64], s_pos[64];
  const int lane = threadIdx.x, per = waves_per_lane(nwaves);
  double sw = 0.0, sw2 = 0.0;
  long long n_in = 0, n_pos = 0;
  for (int w = lane * per; w < (lane + 1) * per && w < nwaves; ++w) {
    sw = sw + part[w].sum_w; sw2 = sw2 + part[w].sum_w2;
    n_in += part[w].n_in; n_pos += part[w].n_pos;
  }
  s_w[lane] = sw; s_w2[lane] = sw2; s_in[lane] = n_in; s_pos[lane] = n_pos;
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < 64; ++l) {
    sw = sw + s_w[l]; sw2 = sw2 + s_w2[l];
    n_in += s_in[l]; n_pos += s_pos[l];
  }
  out->sum_w = sw; out->sum_w2 = sw2; out->n_in = n_in; out->n_pos = n_pos;   // x_min stays what weight_min_merge_kernel left
}

// ---------------------------------------------------------------------------------------------------------- weighted moments

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
  const int lane = threadIdx.x, slot = blockIdx.x, per = waves_per_lane(nwaves);
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

template <int NS>
void launch_wstat(SensRows rows, const double *w, const int32_t *n_active, const int32_t *status, const int32_t *labels, int group,
                  long long ncol, int grid, WStatPartial *part, hipStream_t stream) {
  hipLaunchKernelGGL(wstat_kernel<NS>, dim3(grid), dim3(64), 0, stream, rows, w, n_active, status, labels, group, ncol, part);
}

// ------------------------------------------------------------------------------------------------------ weighted covariances

constexpr int kLaneStride = 65;   // doubles from one quantity's 64 lane values to the next in LDS

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
};

// pair p of the upper triangle of ns slots, row by row: (0,0), (0,1), .. (0,ns-1), (1,1), ..
__device__ __forceinline__ void pair_of(int p, int ns, int &i, int &j) {
  i = 0;
  while (p >= ns - i) { p -= ns - i; ++i; }
  j = i + p;
}

// One walk serves every slot and every pair of the request (a template on nslots: every index is a compile-time one).  A lane
// applies WRun::push to the means -- West's update -- and C_ij += w * d_i * (x_j - mean_j) with mean_j already updated, which for
// i == j is the m2 of WRun::push, operation for operation; then the 64 lanes in lane order through LDS, one thread per pair.
template <int NS>
__global__ void __launch_bounds__(64) wcov_kernel(SensRows rows, const double *__restrict__ w, const int32_t *__restrict__ n_active,
                                                  const int32_t *__restrict__ status, const int32_t *__restrict__ labels, int group,
                                                  long long ncol, double *__restrict__ part) {
  constexpr int NP = NS * (NS + 1) / 2;
  __shared__ double s[(3 + NS + NP) * kLaneStride];   // [n, W, W2, means, co-moments][lane]
  const int lane = threadIdx.x;
  const long long nblk = (ncol + 63) / 64;
  long long n = 0;
  double W = 0.0, W2 = 0.0, mean[NS], C[NP];
#pragma unroll
  for (int i = 0; i < NS; ++i) mean[i] = 0.0;
#pragma unroll
  for (int p = 0; p < NP; ++p) C[p] = 0.0;
  bool ok, ok_next = false;
  double wv, wv_next = 0.0, v[NS], v_next[NS];
  load_slots<NS>(rows, w, n_active, status, labels, group, ncol, blockIdx.x, lane, ok, wv, v);
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    // the next block's loads are under way while this block is consumed
    if (blk + gridDim.x < nblk) load_slots<NS>(rows, w, n_active, status, labels, group, ncol, blk + gridDim.x, lane, ok_next, wv_next, v_next);
    if (ok) {
      n += 1;
      W = W + wv;
      W2 = W2 + wv * wv;
      double wd[NS], e[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const double d = v[i] - mean[i];
        mean[i] = mean[i] + d * (wv / W);
        wd[i] = wv * d;
        e[i] = v[i] - mean[i];
      }
      int p = 0;
#pragma unroll
      for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = i; j < NS; ++j, ++p) C[p] = C[p] + wd[i] * e[j];
    }
    ok = ok_next; wv = wv_next;
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i] = v_next[i];
  }
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
  for (int l = 0; l < 64; ++l) {
    const long long nb = (long long)s[l];
    if (nb > 0)
      acc.add(nb, s[kLaneStride + l], s[2 * kLaneStride + l], s[(3 + i) * kLaneStride + l], s[(3 + j) * kLaneStride + l],
              s[(3 + NS + lane) * kLaneStride + l]);
  }
  double *mine = part + (size_t)blockIdx.x * DEV_WCOV_PART;
  mine[DEV_WCOV_C0 + lane] = acc.c;
  if (i == j) mine[DEV_WCOV_MEAN0 + i] = acc.mi;
  if (lane == 0) { mine[0] = (double)acc.n; mine[1] = acc.W; mine[2] = acc.W2; }
}

// One workgroup per pair of slots: the waves' partials in wave order, bracketed as wstat_merge_kernel brackets them.  The pair
// (i, j) goes to cov[i][j] and cov[j][i]: one value, stored twice.
__global__ void __launch_bounds__(64) wcov_merge_kernel(const double *__restrict__ part, int nwaves, int ns, WCovResult *__restrict__ out) {
  __shared__ double s_n[64], s_W[64], s_W2[64], s_mi[64], s_mj[64], s_c[64];
  const int lane = threadIdx.x, p = blockIdx.x, per = waves_per_lane(nwaves);
  int i, j;
  pair_of(p, ns, i, j);
  WPairAcc acc{0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int wv = lane * per; wv < (lane + 1) * per && wv < nwaves; ++wv) {
    const double *q = part + (size_t)wv * DEV_WCOV_PART;
    const long long nb = (long long)q[0];
    if (nb > 0) acc.add(nb, q[1], q[2], q[DEV_WCOV_MEAN0 + i], q[DEV_WCOV_MEAN0 + j], q[DEV_WCOV_C0 + p]);
  }
  s_n[lane] = (double)acc.n; s_W[lane] = acc.W; s_W2[lane] = acc.W2; s_mi[lane] = acc.mi; s_mj[lane] = acc.mj; s_c[lane] = acc.c;
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < 64; ++l) {
    const long long nb = (long long)s_n[l];
    if (nb > 0) acc.add(nb, s_W[l], s_W2[l], s_mi[l], s_mj[l], s_c[l]);
  }
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

template <int NS>
void launch_wcov(SensRows rows, const double *w, const int32_t *n_active, const int32_t *status, const int32_t *labels, int group,
                 long long ncol, int grid, double *part, hipStream_t stream) {
  hipLaunchKernelGGL(wcov_kernel<NS>, dim3(grid), dim3(64), 0, stream, rows, w, n_active, status, labels, group, ncol, part);
}

// -------------------------------------------------------------------------------------------------------- weighted histogram

// lane i's value in every lane (i is the same in every lane)
__device__ __forceinline__ double lane_value(double v, int i) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), i), hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
  return __hiloint2double(hi, lo);
}

__global__ void __launch_bounds__(64) whist_kernel(const double *__restrict__ x, const double *__restrict__ w,
                                                   const int32_t *__restrict__ n_active, const int32_t *__restrict__ status,
                                                   const int32_t *__restrict__ labels, int group, long long ncol, HistEdges e,
                                                   double *__restrict__ tables) {
  __shared__ double table[DEV_WEIGHT_ENTRIES];
  const int lane = threadIdx.x, W = e.nvbins + 2;
  for (int i = lane; i < W; i += 64) table[i] = 0.0;
  __syncthreads();
  const long long nblk = (ncol + 63) / 64;
  bool ok, ok_next = false;
  double v, wv, v_next = 0.0, wv_next = 0.0;
  load_xw(x, w, n_active, status, labels, group, ncol, blockIdx.x, lane, ok, v, wv);
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    // the next block's loads are under way while this block is added
    if (blk + gridDim.x < nblk) load_xw(x, w, n_active, status, labels, group, ncol, blk + gridDim.x, lane, ok_next, v_next, wv_next);
    const int entry = ok ? hist_entry(v, e) : 0;
    unsigned long long todo = __ballot(ok);
    while (todo) {   // the lanes whose column counts, in lane order; only the owner of an entry ever touches it
      const int i = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int en = __builtin_amdgcn_readlane(entry, i);
      const double wi = lane_value(wv, i);
      if (lane == (en & 63)) table[en] = table[en] + wi;
    }
    ok = ok_next; v = v_next; wv = wv_next;
  }
  __syncthreads();
  for (int i = lane; i < W; i += 64) tables[(size_t)blockIdx.x * DEV_WEIGHT_ENTRIES + i] = table[i];
}

// one workgroup per entry: the waves' tables in wave order
__global__ void __launch_bounds__(64) whist_merge_kernel(const double *__restrict__ tables, int nwaves, double *__restrict__ out) {
  __shared__ double s_sum[64];
  const int lane = threadIdx.x, entry = blockIdx.x, per = waves_per_lane(nwaves);
  double sum = 0.0;
  for (int w = lane * per; w < (lane + 1) * per && w < nwaves; ++w) sum = sum + tables[(size_t)w * DEV_WEIGHT_ENTRIES + entry];
  s_sum[lane] = sum;
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < 64; ++l) sum = sum + s_sum[l];
  out[entry] = sum;
}

int grid_of(long long ncol) {
  const long long nblk = (ncol + 63) / 64;
  return (int)(nblk < DEV_WEIGHT_GRID ? nblk : DEV_WEIGHT_GRID);
}

}  // namespace

extern "C" hipError_t samsim_launch_set_weights(const double *x, const int32_t *n_active, const int32_t *status, const int32_t *labels,
                                                int group, long long ncol, int kind, double c, double *w, WeightPartial *part,
                                                WeightPartial *out, hipStream_t stream) {
  const int grid = grid_of(ncol);
  hipError_t e = hipMemsetAsync(out, 0, sizeof(WeightPartial), stream);   // x_min of DIRECT is 0.0
  if (e != hipSuccess) return e;
  if (kind == SAMSIM_WEIGHT_GAUSS) {
    hipLaunchKernelGGL(weight_min_kernel, dim3(grid), dim3(64), 0, stream, x, n_active, status, labels, group, ncol, part);
    hipLaunchKernelGGL(weight_min_merge_kernel, dim3(1), dim3(64), 0, stream, part, grid, out);
    hipLaunchKernelGGL(weight_fill_kernel<SAMSIM_WEIGHT_GAUSS>, dim3(grid), dim3(64), 0, stream, x, n_active, status, labels, group, ncol,
                       out, c, w, part);
  } else if (kind == SAMSIM_WEIGHT_DIRECT) {
    hipLaunchKernelGGL(weight_fill_kernel<SAMSIM_WEIGHT_DIRECT>, dim3(grid), dim3(64), 0, stream, x, n_active, status, labels, group, ncol,
                       out, c, w, part);
  } else {
    return hipErrorInvalidValue;
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(weight_sum_merge_kernel, dim3(1), dim3(64), 0, stream, part, grid, out);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_weighted_stats(SensRows rows, int nslots, const double *w, const int32_t *n_active,
                                                   const int32_t *status, const int32_t *labels, int group, long long ncol,
                                                   WStatPartial *part, samsim_wstat *out, hipStream_t stream) {
  const int grid = grid_of(ncol);
  switch (nslots) {
    case 1: launch_wstat<1>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 2: launch_wstat<2>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 3: launch_wstat<3>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 4: launch_wstat<4>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 5: launch_wstat<5>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 6: launch_wstat<6>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 7: launch_wstat<7>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 8: launch_wstat<8>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    default: return hipErrorInvalidValue;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wstat_merge_kernel, dim3(nslots), dim3(64), 0, stream, part, grid, out);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_weighted_hist(const double *x, const double *w, const int32_t *n_active, const int32_t *status,
                                                  const int32_t *labels, int group, long long ncol, HistEdges e, double *tables, double *out,
                                                  hipStream_t stream) {
  const int grid = grid_of(ncol);
  if (e.nvbins < 1 || e.nvbins + 2 > DEV_WEIGHT_ENTRIES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(whist_kernel, dim3(grid), dim3(64), 0, stream, x, w, n_active, status, labels, group, ncol, e, tables);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(whist_merge_kernel, dim3(e.nvbins + 2), dim3(64), 0, stream, tables, grid, out);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_weighted_covariance(SensRows rows, int nslots, const double *w, const int32_t *n_active,
                                                        const int32_t *status, const int32_t *labels, int group, long long ncol,
                                                        double *part, WCovResult *out, hipStream_t stream) {
  const int grid = grid_of(ncol);
  switch (nslots) {
    case 1: launch_wcov<1>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 2: launch_wcov<2>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 3: launch_wcov<3>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 4: launch_wcov<4>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 5: launch_wcov<5>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 6: launch_wcov<6>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 7: launch_wcov<7>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    case 8: launch_wcov<8>(rows, w, n_active, status, labels, group, ncol, grid, part, stream); break;
    default: return hipErrorInvalidValue;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wcov_merge_kernel, dim3(nslots * (nslots + 1) / 2), dim3(64), 0, stream, part, grid, nslots, out);
  return hipGetLastError();
}
