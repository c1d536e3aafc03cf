// samsim_resample.h -- what samsim_resample.hip and the C-ABI host code share about the posterior draw (samsim_resample,
// samsim_get_offspring, samsim_get_ancestors, include/samsim.h): the ensemble resampled by its weights, indices only.  The step kernel
// does not include this header.
//
// The first part is plain C++ (tests/test_resample_host.py compiles it alone with g++): the grid rule, the mixer of the stratified
// offsets, the two point counts K(t) and the scratch layout.  They are the very functions the kernels call.  The second needs hipcc.
#ifndef SAMSIM_RESAMPLE_H
#define SAMSIM_RESAMPLE_H

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "samsim_device.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

#define DEV_RS_GRID 1024   // one-wave workgroups of the sum and the draw kernel, at most (the grid rule of samsim_select_columns)
static_assert(DEV_RS_GRID % 64 == 0, "the scan gives every lane the same number of ranges");

// The grid: the nblk 64-column blocks cut into `ranges` contiguous ranges of `per` blocks (the last may be shorter); range g owns
// the blocks [g * per, min((g + 1) * per, nblk)), so range order is column order.
struct RsGrid { long long nblk, per; int ranges; };
inline RsGrid rs_grid(long long ncol) {
  RsGrid g;
  g.nblk = (ncol + 63) / 64;
  g.per = (g.nblk + DEV_RS_GRID - 1) / DEV_RS_GRID;
  g.ranges = (int)((g.nblk + g.per - 1) / g.per);
  return g;
}

// the splitmix64 finaliser of seed + (k + 1) * 0x9E3779B97F4A7C15, in wrapping 64-bit arithmetic
RS_HD inline uint64_t rs_mix(uint64_t seed, uint64_t k) {
  uint64_t z = seed + (k + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the offset of draw point k of SAMSIM_RESAMPLE_STRATIFIED, in [0, 1): the upper 53 bits of the mix
RS_HD inline double rs_offset(uint64_t seed, uint64_t k) { return (double)(rs_mix(seed, k) >> 11) * 0x1.0p-53; }

// K(t): how many of the m draw points lie below t, 0 <= t <= m.  SYSTEMATIC: the points are u0 + k, k = 0 .. m - 1; the difference
// t - u0 is rounded, then ceil.  STRATIFIED: point k is k + u(k).  Both are non-decreasing in t, and K(t) = m from t >= m on.
RS_HD inline long long rs_count_systematic(double t, long long m, double u0) {
  if (t >= (double)m) return m;
  const double k = std::ceil(t - u0);
  return k <= 0.0 ? 0 : (k >= (double)m ? m : (long long)k);
}
RS_HD inline long long rs_count_stratified(double t, long long m, uint64_t seed) {
  if (t >= (double)m) return m;
  const double f = std::floor(t);
  return (long long)f + (rs_offset(seed, (uint64_t)f) < t - f ? 1 : 0);
}

// what a range knows of the columns it drew for: all integers, so their merge does not depend on the order
struct RsPartial { long long n_pos, n_surv, sum_n, max_n, argmax; };
// what the merge leaves for the host: samsim_resample_info, field for field
struct RsResult { long long n_pos, m_drawn, n_surv, max_n, argmax; double sum_w; };

// The resample scratch of a handle, SAMSIM_RESAMPLE_SCRATCH_BYTES whatever ncol and m are:
//   [DEV_RS_SUMS_AT, DEV_RS_BASES_AT)   the ranges' sums T_g, double [DEV_RS_GRID] (0.0 behind the last range)
//   [DEV_RS_BASES_AT, DEV_RS_PART_AT)   their bases B_g, double [DEV_RS_GRID], then W = B_G
//   [DEV_RS_PART_AT, DEV_RS_RESULT_AT)  the ranges' integer partials, RsPartial [DEV_RS_GRID]
//   [DEV_RS_RESULT_AT, DEV_RS_BYTES)    the result
#define DEV_RS_SUMS_AT ((size_t)0)
#define DEV_RS_BASES_AT (DEV_RS_SUMS_AT + (size_t)DEV_RS_GRID * 8)
#define DEV_RS_TOTAL_AT (DEV_RS_BASES_AT + (size_t)DEV_RS_GRID * 8)
#define DEV_RS_PART_AT (DEV_RS_TOTAL_AT + 64)
#define DEV_RS_RESULT_AT (DEV_RS_PART_AT + (size_t)DEV_RS_GRID * sizeof(RsPartial))
#define DEV_RS_BYTES (DEV_RS_RESULT_AT + 64)
static_assert(sizeof(RsResult) <= 64 && sizeof(RsResult) == sizeof(samsim_resample_info), "the result is samsim_resample_info");
static_assert(DEV_RS_BYTES <= SAMSIM_RESAMPLE_SCRATCH_BYTES, "resample scratch bound of samsim.h");
inline size_t rs_scratch_bytes() { return DEV_RS_BYTES; }

#ifdef __HIPCC__

#include "samsim_slot_walk.h"

// One draw, passed by value as the kernels' argument.
struct RsParams {
  slot_walk::ColSet cs;     // the columns that are IN; a column counts when it is IN and w > 0
  const double *w;          // the weight row [ncol]
  long long per;            // blocks per range
  long long m;              // draws
  double u0;                // SYSTEMATIC
  uint64_t seed;            // STRATIFIED
  int32_t ranges;
  int32_t kind;             // enum samsim_resample_kind
};

// samsim_resample.hip.  Enqueues the four kernels on `stream` and returns at once: the offspring row [ncol], the first m_drawn
// entries of the ancestor list (room for m) and the result at DEV_RS_RESULT_AT of `scratch`.
extern "C" hipError_t samsim_launch_resample(const RsParams *p, void *scratch, double *offspring, long long *ancestors, hipStream_t stream);

#endif   // __HIPCC__

#endif
