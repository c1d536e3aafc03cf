// samsim_jitter.hip -- the rejuvenation of a resampled ensemble on the device (samsim_jitter, include/samsim.h): the per-column
// parameters -- the two perturbation slots of the forcing and the two ocean rows -- shrunk towards a centre and jittered by a normal
// deviate that belongs to the column, so that the copies samsim_apply_resample made part again.  Nothing leaves HBM.
//
//   jt_map_kernel    one-wave workgroups, one entry per lane, range g owning the contiguous 64-entry blocks [g * per, (g + 1) * per).
//                    An entry is a column (POOL) or a destination of the stored plan (COPIES; the list ascends, so the accesses are
//                    ordered, though scattered).  Status and label are read once, then every term of the column in one pass: its row
//                    is read once and written once, coalesced with POOL.  The deviate's attempt loop is per lane and bounded
//                    (SAMSIM_JITTER_MAX_ATTEMPTS); the logarithm, the quotient and the root follow it once.  The counts are wave
//                    ballots kept in scalar registers: no LDS, no atomics.
//   jt_merge_kernel  one wave sums the ranges' counts: the totals the host fetches in one small copy.
//
// Every value is a function of (seed, column, target, the term, the row's value) alone (samsim_jitter.h): nothing depends on the grid,
// on `which`, on the group or on the other terms.
#include <hip/hip_runtime.h>

#include "samsim_jitter.h"

#pragma clang fp contract(off)

namespace {

// the sum of v over the wave, in every lane
__device__ __forceinline__ long long wave_sum(long long v) {
  for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w);
  return v;
}

__global__ void __launch_bounds__(64) jt_map_kernel(const JtParams p, JtCounts *__restrict__ part) {
  const int lane = threadIdx.x;
  const long long nblk = (p.n + 63) / 64;
  const long long b0 = (long long)blockIdx.x * p.per;
  const long long b1 = b0 + p.per < nblk ? b0 + p.per : nblk;
  JtCounts q{};
  for (long long blk = b0; blk < b1; ++blk) {
    const long long e = blk * 64 + lane;
    long long col = e;
    bool w = e < p.n;
    if (w && p.dst) col = p.dst[e];
    w = w && col >= 0 && col < p.ncol;   // never false for a list the plan has written
    if (w) w = p.status[col] == 0 && (!p.labels || p.labels[col] == p.group);
    q.n_written += __popcll(__ballot(w));
    // (unrolled, so that row[i], term[i] and the counts are named statically; all four terms and rows of the by-value argument are
    // then live in scalar registers across the loop, and the compiler parks 39 of them in lanes of a vector register -- no memory
    // traffic, accepted: the call is 0.1 ms at 1 048 576 columns)
#pragma unroll
    for (int i = 0; i < SAMSIM_JITTER_MAX_TERMS; ++i) {
      if (i >= p.nterms) break;   // uniform over the grid
      bool lo = false, hi = false;
      if (w) {
        int attempts;
        const double eps = jt_deviate(p.seed, (uint64_t)col, p.term[i].target, &attempts);
        const JtValue r = jt_value(p.term[i], p.row[i][col], eps);
        p.row[i][col] = r.v;
        lo = r.lo; hi = r.hi;
      }
      q.n_lo[i] += __popcll(__ballot(lo));
      q.n_hi[i] += __popcll(__ballot(hi));
    }
  }
  if (lane == 0) part[blockIdx.x] = q;
}

// One wave: lane l sums the counts of the ranges [l * each, (l + 1) * each), the 64 sums are added across the lanes.  Integers: the
// order does not matter to the result.
__global__ void __launch_bounds__(64) jt_merge_kernel(const JtCounts *__restrict__ part, int ranges, JtCounts *__restrict__ out) {
  const int lane = threadIdx.x;
  const int each = (ranges + 63) / 64;
  const int g0 = lane * each;
  JtCounts q{};
  for (int i = 0; i < each; ++i)
    if (g0 + i < ranges) {
      const JtCounts r = part[g0 + i];
      q.n_written += r.n_written;
      for (int t = 0; t < SAMSIM_JITTER_MAX_TERMS; ++t) { q.n_lo[t] += r.n_lo[t]; q.n_hi[t] += r.n_hi[t]; }
    }
  q.n_written = wave_sum(q.n_written);
  for (int t = 0; t < SAMSIM_JITTER_MAX_TERMS; ++t) { q.n_lo[t] = wave_sum(q.n_lo[t]); q.n_hi[t] = wave_sum(q.n_hi[t]); }
  if (lane == 0) *out = q;
}

}  // namespace

extern "C" hipError_t samsim_launch_jitter(const JtParams *p, void *scratch, hipStream_t stream) {
  JtCounts *part = (JtCounts *)((char *)scratch + DEV_JT_PART_AT);
  JtCounts *out = (JtCounts *)((char *)scratch + DEV_JT_RESULT_AT);
  if (p->ranges < 1 || p->ranges > DEV_JT_GRID || p->nterms < 1 || p->nterms > SAMSIM_JITTER_MAX_TERMS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(jt_map_kernel, dim3((unsigned)p->ranges), dim3(64), 0, stream, *p, part);
  hipLaunchKernelGGL(jt_merge_kernel, dim3(1), dim3(64), 0, stream, part, (int)p->ranges, out);
  return hipGetLastError();
}
