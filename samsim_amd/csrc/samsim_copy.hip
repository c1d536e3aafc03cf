// samsim_copy.hip -- whole columns copied in place on the device (samsim_copy_columns, samsim_apply_resample, include/samsim.h): the
// step that makes a scored, weighted and resampled ensemble a particle filter.  Nothing leaves HBM.
//
// The plan (samsim_apply_resample) is an ordered compaction in the pattern of samsim_select.hip -- one-wave workgroups, range g owning
// the contiguous 64-column blocks [g * per, (g + 1) * per), so range order is column order --, no hand-off between workgroups, no
// atomics:
//   cp_count_kernel  each range counts its pool columns, its free slots (pool, no offspring), its surplus copies (offspring - 1 where
//                    that is positive), its sources and the drawn columns that left the pool.
//   cp_scan_kernel   one wave turns the ranges' two counts into exclusive offsets and forms the totals: the result the host fetches
//                    in one small copy and decides on -- a plan that does not balance writes nothing.
//   cp_write_kernel  each range evaluates its columns again; a free lane stores its column at offset + (free lanes below it), a
//                    source stores its column surplus times from offset + (surplus of the lanes below it); a column with 64 or more
//                    surplus copies is written by the whole wave, as rs_draw_kernel writes its ancestors.
//
// The copy: the pair list is read-only to every kernel, sources are only read and destinations only written, and no column is both
// (the host has checked that, or the plan's rule guarantees it), so no launch races with itself or with another.
//   copy_layers_kernel  gather_layers_kernel of samsim_select.hip with a store into the layer block in place of the staging buffer:
//                    one thread per (array, layer, entry), the entry fastest.  The plan's list ascends in dst and does not descend in
//                    src, so neighbouring threads store to neighbouring lanes of one 512-byte row and the entries of one family load
//                    one element.  The layer value samsim_get_state returns (samsim_column_read.h) is formed in registers; the
//                    scratch row D_V_EX is not among the arrays.
//   copy_rows_kernel the per-column rows [rows][ncol], 8-byte or 4-byte words, the entry fastest.
//   copy_fill_kernel one value into the destinations' entries of an int32 row (the restart flags).
#include <hip/hip_runtime.h>

#include "samsim_column_read.h"
#include "samsim_copy.h"

#pragma clang fp contract(off)

namespace {

// the lane's column of a block
struct CpLoad {
  double n;
  int32_t st, lab;
  bool in;
};
__device__ __forceinline__ void cp_load(const CpParams &p, long long blk, int lane, CpLoad &v) {
  const long long col = blk * 64 + lane;
  v.in = col < p.ncol;
  v.n = 0.0; v.st = 0; v.lab = 0;
  if (!v.in) return;
  v.n = p.offspring[col];
  v.st = p.status[col];
  if (p.labels) v.lab = p.labels[col];
}
__device__ __forceinline__ CpColumn cp_rule(const CpParams &p, const CpLoad &v) {
  if (!v.in) return CpColumn{0, false, false, false};
  return cp_column(v.st == 0 && (!p.labels || v.lab == p.group), v.n);
}
__device__ __forceinline__ bool cp_in_pool(const CpParams &p, const CpLoad &v) {
  return v.in && v.st == 0 && (!p.labels || v.lab == p.group);
}

__device__ __forceinline__ void cp_range(const CpParams &p, long long &b0, long long &b1) {
  const long long nblk = (p.ncol + 63) / 64;
  b0 = (long long)blockIdx.x * p.per;
  b1 = b0 + p.per < nblk ? b0 + p.per : nblk;
}

// the sum of v over the wave, in every lane
__device__ __forceinline__ long long wave_sum(long long v) {
  for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w);
  return v;
}

__global__ void __launch_bounds__(64) cp_count_kernel(const CpParams p, CpPartial *__restrict__ part) {
  const int lane = threadIdx.x;
  long long b0, b1;
  cp_range(p, b0, b1);
  CpLoad v{}, v_next{};
  if (b0 < b1) cp_load(p, b0, lane, v);
  long long n_pool = 0, n_free = 0, n_copies = 0, n_sources = 0, n_bad = 0;
  for (long long blk = b0; blk < b1; ++blk) {
    if (blk + 1 < b1) cp_load(p, blk + 1, lane, v_next);   // the next block's loads are under way while this block is counted
    const CpColumn c = cp_rule(p, v);
    n_pool += cp_in_pool(p, v) ? 1 : 0;
    n_free += c.free ? 1 : 0;
    n_copies += c.surplus;
    n_sources += c.source ? 1 : 0;
    n_bad += c.bad ? 1 : 0;
    v = v_next;
  }
  n_pool = wave_sum(n_pool); n_free = wave_sum(n_free); n_copies = wave_sum(n_copies);
  n_sources = wave_sum(n_sources); n_bad = wave_sum(n_bad);
  if (lane == 0) part[blockIdx.x] = CpPartial{n_pool, n_free, n_copies, n_sources, n_bad};
}

// One wave: lane l sums the counts of the ranges [l * each, (l + 1) * each) in range order, the 64 sums are scanned across the lanes,
// and lane l writes the exclusive offsets of its ranges.  Integers: the order does not matter to the result.
__device__ __forceinline__ long long wave_inclusive(long long mine, int lane) {
  long long incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  return incl;
}
__global__ void __launch_bounds__(64) cp_scan_kernel(const CpPartial *__restrict__ part, int ranges, long long *__restrict__ at_free,
                                                     long long *__restrict__ at_copies, CpResult *__restrict__ out) {
  const int lane = threadIdx.x;
  const int each = (ranges + 63) / 64;
  const int g0 = lane * each;
  long long f = 0, c = 0, pool = 0, sources = 0, bad = 0;
  for (int i = 0; i < each; ++i)
    if (g0 + i < ranges) {
      const CpPartial q = part[g0 + i];
      f += q.n_free; c += q.n_copies; pool += q.n_pool; sources += q.n_sources; bad += q.n_bad;
    }
  const long long f_incl = wave_inclusive(f, lane), c_incl = wave_inclusive(c, lane);
  long long f_run = f_incl - f, c_run = c_incl - c;
  for (int i = 0; i < each; ++i)
    if (g0 + i < ranges) {
      at_free[g0 + i] = f_run; at_copies[g0 + i] = c_run;
      f_run += part[g0 + i].n_free; c_run += part[g0 + i].n_copies;
    }
  pool = wave_sum(pool); sources = wave_sum(sources); bad = wave_sum(bad);
  if (lane == 63) *out = CpResult{pool, f_incl, c_incl, sources, bad};
}

__global__ void __launch_bounds__(64) cp_write_kernel(const CpParams p, const long long *__restrict__ at_free,
                                                      const long long *__restrict__ at_copies, long long *__restrict__ src,
                                                      long long *__restrict__ dst, long long cap) {
  const int lane = threadIdx.x;
  long long b0, b1;
  cp_range(p, b0, b1);
  long long f_at = at_free[blockIdx.x], c_at = at_copies[blockIdx.x];
  const unsigned long long below = (1ull << lane) - 1ull;
  CpLoad v{}, v_next{};
  if (b0 < b1) cp_load(p, b0, lane, v);
  for (long long blk = b0; blk < b1; ++blk) {
    if (blk + 1 < b1) cp_load(p, blk + 1, lane, v_next);
    const CpColumn c = cp_rule(p, v);
    const long long col = blk * 64 + lane;
    // the free slots, ascending
    const unsigned long long vote = __ballot(c.free);
    const long long rank = f_at + __popcll(vote & below);
    if (c.free && rank < cap) dst[rank] = col;
    f_at += __popcll(vote);
    // the copies: the lane's entries lie at [first, first + surplus), within [0, cap) for a plan that balances
    const long long incl = wave_inclusive(c.surplus, lane);
    const long long first = c_at + incl - c.surplus;
    if (c.surplus > 0 && c.surplus < 64)
      for (long long j = 0; j < c.surplus; ++j)
        if (first + j < cap) src[first + j] = col;
    unsigned long long heavy = __ballot(c.surplus >= 64);
    while (heavy) {
      const int i = __ffsll((long long)heavy) - 1;
      heavy &= heavy - 1;
      const long long at = __shfl(first, i), cnt = __shfl(c.surplus, i), from = blk * 64 + i;
      for (long long j = lane; j < cnt; j += 64)
        if (at + j < cap) src[at + j] = from;
    }
    c_at += __shfl(incl, 63);
    v = v_next;
  }
}

__global__ void __launch_bounds__(256) copy_layers_kernel(double *lay, const long long *__restrict__ src, const long long *__restrict__ dst,
                                                          const int32_t *__restrict__ n_active, const int32_t *__restrict__ status,
                                                          const int32_t *__restrict__ flags, int N, size_t ncol, size_t w, int stepped) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)SAMSIM_NARR * N * w) return;
  const size_t j = i % w, ak = i / w;
  const int k = (int)(ak % (size_t)N), a = (int)(ak / (size_t)N);
  const size_t c = (size_t)src[j], d = (size_t)dst[j];
  if (c >= ncol || d >= ncol) return;   // never true for a list the host has checked or the plan has written
  double v = lay[DEV_LAY_INDEX(a, k, c, N, ncol)];
  // the layer value samsim_get_columns forms for the source (gather_layers_kernel of samsim_select.hip): the layers below the active
  // ones keep what they hold
  if (a == SAMSIM_A_S_ABS || a == SAMSIM_A_S_BU) {
    const column_read::Column q = column_read::column(n_active, status, flags, c, N, stepped != 0);
    if (q.adjust && k < q.na) {
      if (a == SAMSIM_A_S_ABS) {
        v = column_read::s_abs_value(v, q.clamp);
      } else {
        const double s = lay[DEV_LAY_INDEX(SAMSIM_A_S_ABS, k, c, N, ncol)], m = lay[DEV_LAY_INDEX(SAMSIM_A_M, k, c, N, ncol)];
        v = column_read::s_bu_value(s, m, q.adjust, q.clamp, [&] { return v; });
      }
    }
  }
  lay[DEV_LAY_INDEX(a, k, d, N, ncol)] = v;
}

template <class T>
__global__ void __launch_bounds__(256) copy_rows_kernel(T *rows, size_t nrows, size_t ncol, const long long *__restrict__ src,
                                                        const long long *__restrict__ dst, size_t w) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows * w) return;
  const size_t j = i % w, r = i / w;
  const size_t c = (size_t)src[j], d = (size_t)dst[j];
  if (c >= ncol || d >= ncol) return;
  rows[r * ncol + d] = rows[r * ncol + c];
}

__global__ void __launch_bounds__(256) copy_fill_kernel(int32_t *row, size_t ncol, const long long *__restrict__ dst, size_t w, int32_t value) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= w) return;
  const size_t d = (size_t)dst[j];
  if (d < ncol) row[d] = value;
}

template <class T>
hipError_t copy_rows(void *rows, long long nrows, long long ncol, const long long *src, const long long *dst, long long n, hipStream_t stream) {
  if (nrows <= 0 || n <= 0) return hipSuccess;
  // pieces of rows, so that a launch stays within DEV_CP_PIECE_THREADS threads
  const size_t pr = DEV_CP_PIECE_THREADS / (size_t)n > 0 ? DEV_CP_PIECE_THREADS / (size_t)n : 1;
  for (size_t r0 = 0; r0 < (size_t)nrows; r0 += pr) {
    const size_t nr = (size_t)nrows - r0 < pr ? (size_t)nrows - r0 : pr, t = nr * (size_t)n;
    hipLaunchKernelGGL(copy_rows_kernel<T>, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, stream, (T *)rows + r0 * (size_t)ncol, nr,
                       (size_t)ncol, src, dst, (size_t)n);
  }
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t samsim_launch_copy_plan_count(const CpParams *p, void *scratch, hipStream_t stream) {
  CpPartial *part = (CpPartial *)((char *)scratch + DEV_CP_PART_AT);
  long long *at_free = (long long *)((char *)scratch + DEV_CP_FREE_AT);
  long long *at_copies = (long long *)((char *)scratch + DEV_CP_COPIES_AT);
  CpResult *out = (CpResult *)((char *)scratch + DEV_CP_RESULT_AT);
  if (p->ranges < 1 || p->ranges > DEV_CP_GRID) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cp_count_kernel, dim3((unsigned)p->ranges), dim3(64), 0, stream, *p, part);
  hipLaunchKernelGGL(cp_scan_kernel, dim3(1), dim3(64), 0, stream, part, (int)p->ranges, at_free, at_copies, out);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_copy_plan_write(const CpParams *p, void *scratch, long long *src, long long *dst, long long cap,
                                                    hipStream_t stream) {
  const long long *at_free = (const long long *)((char *)scratch + DEV_CP_FREE_AT);
  const long long *at_copies = (const long long *)((char *)scratch + DEV_CP_COPIES_AT);
  if (p->ranges < 1 || p->ranges > DEV_CP_GRID) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cp_write_kernel, dim3((unsigned)p->ranges), dim3(64), 0, stream, *p, at_free, at_copies, src, dst, cap);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_copy_layers(double *lay, const long long *src, const long long *dst, const int32_t *n_active,
                                                const int32_t *status, const int32_t *flags, int N, long long ncol, long long n, int stepped,
                                                hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const size_t pc = cp_piece_entries((size_t)N);
  for (size_t p0 = 0; p0 < (size_t)n; p0 += pc) {
    const size_t pw = (size_t)n - p0 < pc ? (size_t)n - p0 : pc, t = (size_t)SAMSIM_NARR * (size_t)N * pw;
    hipLaunchKernelGGL(copy_layers_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, stream, lay, src + p0, dst + p0, n_active, status,
                       flags, N, (size_t)ncol, pw, stepped);
  }
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_copy_rows8(void *rows, long long nrows, long long ncol, const long long *src, const long long *dst,
                                               long long n, hipStream_t stream) {
  return copy_rows<unsigned long long>(rows, nrows, ncol, src, dst, n, stream);
}

extern "C" hipError_t samsim_launch_copy_rows4(void *rows, long long nrows, long long ncol, const long long *src, const long long *dst,
                                               long long n, hipStream_t stream) {
  return copy_rows<uint32_t>(rows, nrows, ncol, src, dst, n, stream);
}

extern "C" hipError_t samsim_launch_copy_fill4(int32_t *row, long long ncol, const long long *dst, long long n, int32_t value, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(copy_fill_kernel, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, stream, row, (size_t)ncol, dst, (size_t)n, value);
  return hipGetLastError();
}
