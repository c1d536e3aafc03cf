// samsim_resample.hip -- the posterior draw (samsim_resample, include/samsim.h): the ensemble resampled by its weight row, indices
// only.  A read-only reduction like the weighted ones: the kernels read the weight row, status and the labels and write the offspring
// row, the ancestor list and the handle's resample scratch, nothing else.
//
// Four launches on the handle's stream in the pattern of samsim_select.hip -- one-wave workgroups, range g owning the contiguous
// 64-column blocks [g * per, (g + 1) * per), so range order is column order --, no hand-off between workgroups, no atomics:
//   rs_sum_kernel    each range forms T_g: the lanes' terms of a block in lane order (lane_value, as whist_kernel takes them), one
//                    dependent addition per counting column; the next block's loads are under way meanwhile.  A column that does not
//                    count has the term +0.0, which changes no sum that is not negative: it is left out.
//   rs_scan_kernel   one wave forms B_g sequentially, from registers, and W; both stay in the scratch: no host round trip.
//   rs_draw_kernel   each range forms L_c again -- the same additions, so the same bits --, then C_c = B_g + L_c, t_c, K(t_c), the
//                    predecessor's K from the lane below (lane 0: the running value, which starts as K of B_g), N_c and the column's
//                    first position K(t_{c-1}).  A lane writes its own copies while they are fewer than 64; a column with 64 or more
//                    is written by the whole wave, 512 contiguous bytes per store: the member that takes nearly all the draws of a
//                    degenerate posterior does not serialise on its lane.
//   rs_merge_kernel  the ranges' integer partials in the bracket of merge_waves.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "samsim_resample.h"

#pragma clang fp contract(off)

namespace {

using namespace slot_walk;

// the lane's column of a block: whether it counts, and its term
struct RsCol {
  double w;
  bool ok;
};
__device__ __forceinline__ void rs_load(const RsParams &p, long long blk, int lane, RsCol &c) {
  const long long col = blk * 64 + lane;
  c.w = 0.0; c.ok = false;
  if (col < p.cs.ncol) {
    const double wv = p.w[col];
    c.ok = p.cs.in(col) && wv > 0.0;
    c.w = c.ok ? wv : 0.0;
  }
}

// the blocks of range g
__device__ __forceinline__ void rs_range(const RsParams &p, long long &b0, long long &b1) {
  const long long nblk = col_blocks(p.cs.ncol);
  b0 = (long long)blockIdx.x * p.per;
  b1 = b0 + p.per < nblk ? b0 + p.per : nblk;
}

// The terms of the block's counting columns added to L in lane order; `mine` leaves with the lane's inclusive local sum L_c (that
// of the last counting column at or below the lane, or what it held).  L is the same in every lane.
__device__ __forceinline__ void rs_add_block(const RsCol &c, int lane, double &L, double &mine) {
  unsigned long long todo = __ballot(c.ok);
  while (todo) {
    const int i = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    L = L + lane_value(c.w, i);
    if (lane >= i) mine = L;
  }
}

__global__ void __launch_bounds__(64) rs_sum_kernel(const RsParams p, double *__restrict__ sums) {
  const int lane = threadIdx.x;
  long long b0, b1;
  rs_range(p, b0, b1);
  RsCol v{}, v_next{};
  if (b0 < b1) rs_load(p, b0, lane, v);
  double L = 0.0, mine = 0.0;
  for (long long blk = b0; blk < b1; ++blk) {
    if (blk + 1 < b1) rs_load(p, blk + 1, lane, v_next);   // the next block's loads are under way while this block is added
    rs_add_block(v, lane, L, mine);
    v = v_next;
  }
  if (lane == 0) sums[blockIdx.x] = L;
}

// One wave: lane l holds the sums of the ranges [l * each, (l + 1) * each) in registers; B runs over the lanes in lane order and
// over a lane's ranges in range order -- one chain of additions, B_{g+1} = B_g + T_g -- and lane l keeps B as it stood before
// its own ranges, from which it forms their bases again with the same additions.
__global__ void __launch_bounds__(64) rs_scan_kernel(const double *__restrict__ sums, int ranges, double *__restrict__ bases,
                                                     double *__restrict__ total) {
  constexpr int each = DEV_RS_GRID / 64;
  const int lane = threadIdx.x;
  double t[each];
#pragma unroll
  for (int i = 0; i < each; ++i) t[i] = lane * each + i < ranges ? sums[lane * each + i] : 0.0;
  double B = 0.0, before = 0.0;
  for (int l = 0; l < 64; ++l) {
    if (lane == l) before = B;
#pragma unroll
    for (int i = 0; i < each; ++i) B = B + lane_value(t[i], l);
  }
  double b = before;
#pragma unroll
  for (int i = 0; i < each; ++i) {
    if (lane * each + i < ranges) bases[lane * each + i] = b;
    b = b + t[i];
  }
  if (lane == 0) *total = B;
}

// the integer side of a range: counting columns, survivors, offspring, the largest family and the lowest column that has it
struct RsAcc {
  long long n_pos, n_surv, sum_n, max_n, argmax;
  __device__ __forceinline__ void absorb(const RsAcc &b) {
    n_pos += b.n_pos; n_surv += b.n_surv; sum_n += b.sum_n;
    if (b.max_n > max_n || (b.max_n == max_n && b.argmax < argmax)) { max_n = b.max_n; argmax = b.argmax; }
  }
};
__device__ __forceinline__ RsAcc rs_empty() { return RsAcc{0, 0, 0, -1, LLONG_MAX}; }

template <int KIND>
__global__ void __launch_bounds__(64) rs_draw_kernel(const RsParams p, const double *__restrict__ bases, const double *__restrict__ total,
                                                     double *__restrict__ offspring, long long *__restrict__ ancestors,
                                                     RsPartial *__restrict__ part) {
  __shared__ RsAcc s_acc[64];
  const int lane = threadIdx.x;
  long long b0, b1;
  rs_range(p, b0, b1);
  const double W = *total, B = bases[blockIdx.x];
  const bool draw = W > 0.0 && W < INFINITY;
  // K(t) of a cumulative weight: one division, one product, then the kind's count
  auto count = [&](double C) -> long long {
    if (!draw) return 0;
    const double t = (C / W) * (double)p.m;
    return KIND == SAMSIM_RESAMPLE_SYSTEMATIC ? rs_count_systematic(t, p.m, p.u0) : rs_count_stratified(t, p.m, p.seed);
  };
  long long k_run = count(B);   // K of the column before the range: its C is B_g, by the scan's own addition
  RsAcc acc = rs_empty();
  RsCol v{}, v_next{};
  if (b0 < b1) rs_load(p, b0, lane, v);
  double L = 0.0;
  for (long long blk = b0; blk < b1; ++blk) {
    if (blk + 1 < b1) rs_load(p, blk + 1, lane, v_next);
    double mine = L;
    rs_add_block(v, lane, L, mine);
    const long long k = count(B + mine);
    long long k_below = __shfl_up(k, 1);
    if (lane == 0) k_below = k_run;
    k_run = __shfl(k, 63);
    const long long n = k - k_below, col = blk * 64 + lane;
    if (col < p.cs.ncol) {
      offspring[col] = (double)n;
      acc.absorb(RsAcc{v.ok ? 1 : 0, n >= 1 ? 1 : 0, n, n, col});
    }
    // the copies: [k_below, k) lies within [0, m) -- K is within [0, m] and does not decrease
    if (n > 0 && n < 64)
      for (long long j = 0; j < n; ++j) ancestors[k_below + j] = col;
    unsigned long long heavy = __ballot(n >= 64);
    while (heavy) {
      const int i = __ffsll((long long)heavy) - 1;
      heavy &= heavy - 1;
      const long long at = __shfl(k_below, i), cnt = __shfl(n, i), c = blk * 64 + i;
      for (long long j = lane; j < cnt; j += 64) ancestors[at + j] = c;
    }
    v = v_next;
  }
  if (!fold_lanes(acc, s_acc, lane)) return;
  part[blockIdx.x] = RsPartial{acc.n_pos, acc.n_surv, acc.sum_n, acc.max_n, acc.argmax};
}

__global__ void __launch_bounds__(64) rs_merge_kernel(const RsPartial *__restrict__ part, int ranges, const double *__restrict__ total,
                                                      RsResult *__restrict__ out) {
  __shared__ RsAcc s_acc[64];
  RsAcc acc = rs_empty();
  const bool last = merge_waves(ranges, acc, s_acc, threadIdx.x, [&](int g) {
    return RsAcc{part[g].n_pos, part[g].n_surv, part[g].sum_n, part[g].max_n, part[g].argmax};
  });
  if (!last) return;
  *out = RsResult{acc.n_pos, acc.sum_n, acc.n_surv, acc.max_n, acc.argmax, *total};
}

}  // namespace

extern "C" hipError_t samsim_launch_resample(const RsParams *p, void *scratch, double *offspring, long long *ancestors, hipStream_t stream) {
  double *sums = (double *)((char *)scratch + DEV_RS_SUMS_AT);
  double *bases = (double *)((char *)scratch + DEV_RS_BASES_AT);
  double *total = (double *)((char *)scratch + DEV_RS_TOTAL_AT);
  RsPartial *part = (RsPartial *)((char *)scratch + DEV_RS_PART_AT);
  RsResult *out = (RsResult *)((char *)scratch + DEV_RS_RESULT_AT);
  if (p->ranges < 1 || p->ranges > DEV_RS_GRID) return hipErrorInvalidValue;
  const dim3 grid((unsigned)p->ranges), wave(64);
  hipLaunchKernelGGL(rs_sum_kernel, grid, wave, 0, stream, *p, sums);
  hipLaunchKernelGGL(rs_scan_kernel, dim3(1), wave, 0, stream, sums, (int)p->ranges, bases, total);
  if (p->kind == SAMSIM_RESAMPLE_SYSTEMATIC)
    hipLaunchKernelGGL(rs_draw_kernel<SAMSIM_RESAMPLE_SYSTEMATIC>, grid, wave, 0, stream, *p, bases, total, offspring, ancestors, part);
  else if (p->kind == SAMSIM_RESAMPLE_STRATIFIED)
    hipLaunchKernelGGL(rs_draw_kernel<SAMSIM_RESAMPLE_STRATIFIED>, grid, wave, 0, stream, *p, bases, total, offspring, ancestors, part);
  else
    return hipErrorInvalidValue;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rs_merge_kernel, dim3(1), wave, 0, stream, part, (int)p->ranges, total, out);
  return hipGetLastError();
}
