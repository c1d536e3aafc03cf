// samsim_jitter.h -- what samsim_jitter.hip and the C-ABI host code share about the rejuvenation of a resampled ensemble (samsim_jitter,
// include/samsim.h): the kernel-shrinkage step of Liu and West on the per-column parameters, so that the copies of a member part
// again.  The step kernel does not include this header.
//
// The first part is plain C++ (tests/jitter_reference.py compiles it alone with g++): the checks of a spec, the key of a deviate, the
// deviate, the rule for the new value, the grid rule and the scratch layout.  They are the very functions the kernel calls.  The
// second needs hipcc.
#ifndef SAMSIM_JITTER_H
#define SAMSIM_JITTER_H

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "samsim_device.h"
#include "samsim_pow.h"        // sp_log: a fixed sequence of explicit FMAs and one IEEE quotient, the same on the host and the device
#include "samsim_resample.h"   // rs_mix, rs_offset: the mixer of the stratified offsets, not restated here

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define JT_HD __host__ __device__
#define JT_D __device__            // what calls sp_log: samsim_pow.h is device code under hipcc
#define JT_SQRT(x) __builtin_sqrt(x)
#else
#define JT_HD
#define JT_D
#define JT_SQRT(x) std::sqrt(x)
#endif

#define DEV_JT_GRID 4096   // one-wave workgroups of the map, at most: four waves a SIMD on 256 compute units
static_assert(DEV_JT_GRID % 64 == 0, "the merge gives every lane the same number of ranges");

// The grid: the nblk 64-entry blocks of the n entries walked (columns with POOL, entries of the plan with COPIES) cut into `ranges`
// contiguous ranges of `per` blocks, as cp_grid cuts the columns.
struct JtGrid { long long nblk, per; int ranges; };
inline JtGrid jt_grid(long long n) {
  JtGrid g;
  g.nblk = (n + 63) / 64;
  g.per = (g.nblk + DEV_JT_GRID - 1) / DEV_JT_GRID;
  g.ranges = g.per > 0 ? (int)((g.nblk + g.per - 1) / g.per) : 0;
  return g;
}

// ---- the checks of a spec, in the order samsim.h gives; everything samsim_jitter refuses before it touches the device.  What the
// handle knows comes as arguments, so the order is tested without one: whether the two ocean rows exist, whether spec->group passes
// the group checks of samsim_get_covariance, and the length of the stored plan (-1: none applied yet).
inline bool jt_good_target(int32_t t) { return t >= SAMSIM_JT_DT2M && t <= SAMSIM_JT_S_BU_BOTTOM; }
inline int jt_check_term(const samsim_jitter_spec *spec, int i) {
  const samsim_jitter_term &t = spec->term[i];
  if (!jt_good_target(t.target)) return SAMSIM_ERR_ARG;
  for (int j = 0; j < i; ++j)
    if (spec->term[j].target == t.target) return SAMSIM_ERR_ARG;
  if (t.reserved != 0) return SAMSIM_ERR_ARG;
  if (!std::isfinite(t.centre) || !std::isfinite(t.shrink) || !std::isfinite(t.sigma)) return SAMSIM_ERR_ARG;
  if (!(t.shrink >= 0.0 && t.shrink <= 1.0)) return SAMSIM_ERR_ARG;
  if (t.sigma < 0.0) return SAMSIM_ERR_ARG;
  if (std::isnan(t.lo) || std::isnan(t.hi) || t.lo > t.hi) return SAMSIM_ERR_ARG;
  if (t.target == SAMSIM_JT_S_BU_BOTTOM && t.lo < 0.0) return SAMSIM_ERR_ARG;
  return SAMSIM_OK;
}
inline int jt_check(const samsim_jitter_spec *spec, bool have_dfl_q, bool have_S_bu, bool group_ok, long long plan_n) {
  if (!spec) return SAMSIM_ERR_ARG;
  if (spec->struct_size != (int32_t)sizeof(samsim_jitter_spec)) return SAMSIM_ERR_ABI;
  if (spec->which != SAMSIM_JITTER_POOL && spec->which != SAMSIM_JITTER_COPIES) return SAMSIM_ERR_ARG;
  if (spec->nterms < 1 || spec->nterms > SAMSIM_JITTER_MAX_TERMS) return SAMSIM_ERR_ARG;
  for (int i = 0; i < spec->nterms; ++i) {
    const int rc = jt_check_term(spec, i);
    if (rc) return rc;
  }
  for (int i = 0; i < spec->nterms; ++i) {
    if (spec->term[i].target == SAMSIM_JT_DFL_Q_BOTTOM && !have_dfl_q) return SAMSIM_ERR_ARG;
    if (spec->term[i].target == SAMSIM_JT_S_BU_BOTTOM && !have_S_bu) return SAMSIM_ERR_ARG;
  }
  if (spec->which == SAMSIM_JITTER_POOL) return group_ok ? SAMSIM_OK : SAMSIM_ERR_ARG;
  if (spec->group != -1) return SAMSIM_ERR_ARG;
  if (plan_n < 0) return SAMSIM_ERR_ARG;
  return SAMSIM_OK;
}

// ---- the normal deviate of (seed, column c, target t): Marsaglia's polar method on a counter-based stream.  Attempt a draws the
// point (x, y) of the square [-1, 1)^2 from the keys k and k | 1, k = (c << 8) | (t << 6) | (a << 1): c < SAMSIM_MAX_NCOL < 2^27, so
// the shift stays far inside 64 bits, t < 4 takes two bits and a < 32 five.  x and y are exact: a multiple of 2^-52 below 1 in size.
JT_HD inline uint64_t jt_key(uint64_t c, int t, int a) { return (c << 8) | ((uint64_t)t << 6) | ((uint64_t)a << 1); }
JT_HD inline double jt_uniform(uint64_t seed, uint64_t k) { return 2.0 * rs_offset(seed, k) - 1.0; }
static_assert(SAMSIM_JITTER_MAX_ATTEMPTS <= 32 && SAMSIM_JT_S_BU_BOTTOM < 4, "the key has five bits for the attempt and two for the target");
// The first attempt with 0 < s = x*x + y*y < 1 is taken (two rounded products, the rounded sum), and the deviate is
// x * sqrt((-2 log s) / s): sp_log, one rounded product, one IEEE division, the correctly rounded square root, one product.  Without
// an accepted attempt -- probability (1 - pi/4)^32 ~ 4e-22 -- the deviate is 0.  *attempts: the attempts made.
JT_D inline double jt_deviate(uint64_t seed, uint64_t c, int t, int *attempts) {
  double x = 0.0, s = 0.0;
  bool found = false;
  int a = 0;
  while (a < SAMSIM_JITTER_MAX_ATTEMPTS && !found) {
    const uint64_t k = jt_key(c, t, a);
    x = jt_uniform(seed, k);
    const double y = jt_uniform(seed, k | 1);
    const double xx = x * x, yy = y * y;
    s = xx + yy;
    found = s > 0.0 && s < 1.0;
    ++a;
  }
  *attempts = a;
  if (!found) return 0.0;
  // (the logarithm is taken once, behind the loop: on the device the lanes of a wave leave the loop at different attempts)
  const double l = -2.0 * sp_log(s);
  const double q = l / s;
  return x * JT_SQRT(q);
}

// ---- the new value of a term for theta = row[c] and the column's deviate: v = centre + shrink * (theta - centre) -- the difference
// rounded, then the product, then the sum --, v = v + sigma * eps -- the product rounded, then the sum --, then the two bounds.  A
// NaN compares false twice and is written as it is.
struct JtValue { double v; bool lo, hi; };
JT_HD inline JtValue jt_value(const samsim_jitter_term &t, double theta, double eps) {
  const double d = theta - t.centre;
  const double p = t.shrink * d;
  double v = t.centre + p;
  const double e = t.sigma * eps;
  v = v + e;
  JtValue r{v, false, false};
  if (v < t.lo) { r.v = t.lo; r.lo = true; }
  else if (v > t.hi) { r.v = t.hi; r.hi = true; }
  return r;
}

// what a range knows of the columns it wrote, and what the merge leaves for the host: samsim_jitter_info, field for field.  All
// integers, so the merge does not depend on the order.
struct JtCounts { long long n_written, n_lo[SAMSIM_JITTER_MAX_TERMS], n_hi[SAMSIM_JITTER_MAX_TERMS]; };
static_assert(sizeof(JtCounts) == sizeof(samsim_jitter_info) && sizeof(JtCounts) == 72, "the counts are samsim_jitter_info");

// The jitter scratch of a handle, within SAMSIM_JITTER_SCRATCH_BYTES whatever ncol is:
//   [DEV_JT_PART_AT, DEV_JT_RESULT_AT)  the ranges' counts, JtCounts [DEV_JT_GRID]
//   [DEV_JT_RESULT_AT, DEV_JT_BYTES)    the totals
#define DEV_JT_PART_AT ((size_t)0)
#define DEV_JT_RESULT_AT (DEV_JT_PART_AT + (size_t)DEV_JT_GRID * sizeof(JtCounts))
#define DEV_JT_BYTES (DEV_JT_RESULT_AT + 128)
static_assert(DEV_JT_BYTES <= SAMSIM_JITTER_SCRATCH_BYTES, "jitter scratch bound of samsim.h");
inline size_t jt_scratch_bytes() { return DEV_JT_BYTES; }

#ifdef __HIPCC__

// One call, passed by value as the kernel's argument.
struct JtParams {
  double *row[SAMSIM_JITTER_MAX_TERMS];   // the [ncol] row of each term's target
  samsim_jitter_term term[SAMSIM_JITTER_MAX_TERMS];
  const int32_t *status;      // [ncol]
  const int32_t *labels;      // [ncol], or null: every running column is in the pool
  const long long *dst;       // COPIES: the destination list of the stored plan, n entries, ascending; null with POOL
  long long ncol;
  long long n;                // entries walked: ncol with POOL, the plan's length with COPIES
  long long per;              // blocks per range
  uint64_t seed;
  int32_t ranges, group, nterms;
};

// samsim_jitter.hip.  Enqueues the map and the one-wave merge on `stream` and returns at once: the rows rewritten, the totals at
// DEV_JT_RESULT_AT of `scratch`.
extern "C" hipError_t samsim_launch_jitter(const JtParams *p, void *scratch, hipStream_t stream);

#endif   // __HIPCC__

#endif
