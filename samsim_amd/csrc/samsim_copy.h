// samsim_copy.h -- what samsim_copy.hip and the C-ABI host code share about the device-side copy of whole columns (samsim_copy_columns,
// samsim_apply_resample, samsim_get_copy_plan, include/samsim.h): the step that puts the copies of a posterior draw where the dropped
// members were.  The step kernel does not include this header.
//
// The first part is plain C++ (tests/test_copy_host.py compiles it alone with g++): the plan's rule for one column, the grid rule and
// the scratch layout.  They are the very functions the kernels call.  The second needs hipcc.
#ifndef SAMSIM_COPY_H
#define SAMSIM_COPY_H

#include <cstddef>
#include <cstdint>

#include "samsim_device.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define CP_HD __host__ __device__
#else
#define CP_HD
#endif

#define DEV_CP_GRID 1024   // one-wave workgroups of the count and the write kernel, at most (the grid rule of samsim_select_columns)
static_assert(DEV_CP_GRID % 64 == 0, "the scan gives every lane the same number of ranges");

// The grid: the nblk 64-column blocks cut into `ranges` contiguous ranges of `per` blocks (the last may be shorter); range g owns
// the blocks [g * per, min((g + 1) * per, nblk)), so range order is column order.
struct CpGrid { long long nblk, per; int ranges; };
inline CpGrid cp_grid(long long ncol) {
  CpGrid g;
  g.nblk = (ncol + 63) / 64;
  g.per = (g.nblk + DEV_CP_GRID - 1) / DEV_CP_GRID;
  g.ranges = (int)((g.nblk + g.per - 1) / g.per);
  return g;
}

// What the plan takes from one column: `pool` says whether the column runs and carries the label of the draw, n is its offspring.
//   free     the column is in the pool and nobody drew it: a copy goes here
//   surplus  the copies of the column beyond the one that keeps its slot
//   source   the column is copied at least once
//   bad      the column was drawn but is no longer in the pool: the plan cannot be applied
struct CpColumn { long long surplus; bool free, source, bad; };
CP_HD inline CpColumn cp_column(bool pool, double offspring) {
  const long long n = offspring >= 1.0 ? (long long)offspring : 0;
  CpColumn c;
  c.free = pool && n == 0;
  c.surplus = pool && n >= 2 ? n - 1 : 0;
  c.source = c.surplus > 0;
  c.bad = !pool && n >= 1;
  return c;
}

// what a range knows of its columns: all integers, so their merge does not depend on the order
struct CpPartial { long long n_pool, n_free, n_copies, n_sources, n_bad; };
// what the scan leaves for the host: samsim_apply_info, field for field, then the columns that were drawn and left the pool
struct CpResult { long long n_pool, n_free, n_copies, n_sources, n_bad; };
// the plan balances: as many free slots as copies, and every drawn column still in the pool
CP_HD inline bool cp_balanced(const CpResult &r) { return r.n_free == r.n_copies && r.n_bad == 0; }

// The copy scratch of a handle, SAMSIM_COPY_SCRATCH_BYTES whatever ncol is:
//   [DEV_CP_PART_AT, DEV_CP_FREE_AT)      the ranges' partials, CpPartial [DEV_CP_GRID]
//   [DEV_CP_FREE_AT, DEV_CP_COPIES_AT)    the ranges' first free slot in the plan, int64 [DEV_CP_GRID]
//   [DEV_CP_COPIES_AT, DEV_CP_RESULT_AT)  the ranges' first copy in the plan, int64 [DEV_CP_GRID]
//   [DEV_CP_RESULT_AT, DEV_CP_BYTES)      the result
#define DEV_CP_PART_AT ((size_t)0)
#define DEV_CP_FREE_AT (DEV_CP_PART_AT + (size_t)DEV_CP_GRID * sizeof(CpPartial))
#define DEV_CP_COPIES_AT (DEV_CP_FREE_AT + (size_t)DEV_CP_GRID * 8)
#define DEV_CP_RESULT_AT (DEV_CP_COPIES_AT + (size_t)DEV_CP_GRID * 8)
#define DEV_CP_BYTES (DEV_CP_RESULT_AT + 64)
static_assert(sizeof(CpResult) <= 64 && sizeof(CpResult) == sizeof(samsim_apply_info) + 8, "the result is samsim_apply_info and n_bad");
static_assert(DEV_CP_BYTES <= SAMSIM_COPY_SCRATCH_BYTES, "copy scratch bound of samsim.h");
inline size_t cp_scratch_bytes() { return DEV_CP_BYTES; }

// The layer kernel takes the pair list in pieces: one thread per (array, layer, entry) of a piece, at most this many threads a launch
#define DEV_CP_PIECE_THREADS ((size_t)1 << 30)
inline size_t cp_piece_entries(size_t nlayer) { return DEV_CP_PIECE_THREADS / ((size_t)SAMSIM_NARR * nlayer); }

#ifdef __HIPCC__

// One plan, passed by value as the kernels' argument.
struct CpParams {
  const double *offspring;    // the offspring row [ncol] of the last samsim_resample
  const int32_t *status;      // [ncol]
  const int32_t *labels;      // [ncol], or null: every running column is in the pool
  long long ncol;
  long long per;              // blocks per range
  int32_t ranges;
  int32_t group;
};

// samsim_copy.hip.  All of them enqueue on `stream` and return at once.
// the count and the scan: the result at DEV_CP_RESULT_AT of `scratch`, the ranges' offsets before it
extern "C" hipError_t samsim_launch_copy_plan_count(const CpParams *p, void *scratch, hipStream_t stream);
// the pair list of a plan that balances: src[k], dst[k] for k < n_copies, rows with room for `cap` entries each
extern "C" hipError_t samsim_launch_copy_plan_write(const CpParams *p, void *scratch, long long *src, long long *dst, long long cap,
                                                    hipStream_t stream);
// the fifteen public layer arrays of the n pairs: element (a, k, dst[j]) of the layer block becomes the layer value of (a, k, src[j])
extern "C" hipError_t samsim_launch_copy_layers(double *lay, const long long *src, const long long *dst, const int32_t *n_active,
                                                const int32_t *status, const int32_t *flags, int N, long long ncol, long long n, int stepped,
                                                hipStream_t stream);
// rows [nrows][ncol] of 8-byte or 4-byte words: word dst[j] of every row becomes word src[j]
extern "C" hipError_t samsim_launch_copy_rows8(void *rows, long long nrows, long long ncol, const long long *src, const long long *dst,
                                               long long n, hipStream_t stream);
extern "C" hipError_t samsim_launch_copy_rows4(void *rows, long long nrows, long long ncol, const long long *src, const long long *dst,
                                               long long n, hipStream_t stream);
// row[dst[j]] = value
extern "C" hipError_t samsim_launch_copy_fill4(int32_t *row, long long ncol, const long long *dst, long long n, int32_t value, hipStream_t stream);

#endif   // __HIPCC__

#endif
