// samsim_select.hip -- which columns, and what they look like (samsim_select_columns, samsim_get_columns, include/samsim.h).
//
// Selection: an ordered compaction in three launches on the handle's stream, no hand-off between workgroups and no atomics of any
// kind.  select_kernel<NT, false> counts: one-wave workgroups, wave w owning the contiguous 64-column blocks [w * per, (w + 1) * per)
// -- wave order is column order --, lane = column, the predicate's rows coalesced and the next block's loads under way while this
// block is voted on (__ballot / __popcll).  select_scan_kernel, one wave, turns the at most DEV_SEL_GRID counts into exclusive
// offsets and the total.  select_kernel<NT, true> evaluates the predicate again and every matching lane stores its column index at
// offset + (matches in lower lanes) while that rank is below max_out; a wave whose offset has reached max_out returns at once, and
// one that reaches it on the way stops there.  The predicate reads the rows its terms name, and status and the labels only where
// the request needs them; the kernels are templates on the number of terms, so a one-term selection holds one value per lane.
//
// Gather: gather_layers_kernel is lay_window<true> of samsim_capi.cpp with a list in place of a window -- one thread per (array,
// layer, j), j fastest, so the stores into the staging buffer coalesce; the loads are 8 bytes each, 512 B apart within a column
// block.  The layer value samsim_get_state returns (samsim_column_read.h) is formed in registers here, over the active layers as
// samsim_get_state adjusts them: nothing is written to the ensemble, so a column listed twice is read twice
// and races with nothing.  gather_columns_kernel takes the per-column rows the same way.
#include <hip/hip_runtime.h>

#include "samsim_column_read.h"
#include "samsim_select.h"

#pragma clang fp contract(off)

namespace {

// what a lane holds of its column before the vote
template <int NT>
struct SelLoad {
  double x[NT > 0 ? NT : 1];
  int32_t st, lab;
  bool in;
};

template <int NT>
__device__ __forceinline__ void sel_load(const SelParams &p, long long blk, int lane, SelLoad<NT> &v) {
  const long long col = blk * 64 + lane;
  v.in = col < p.ncol;
  v.st = 0; v.lab = 0;
#pragma unroll
  for (int i = 0; i < NT; ++i) v.x[i] = 0.0;
  if (!v.in) return;
  if (p.status) v.st = p.status[col];
  if (p.labels) v.lab = p.labels[col];
#pragma unroll
  for (int i = 0; i < NT; ++i) v.x[i] = p.t[i].row ? p.t[i].row[col] : (double)p.n_active[col];
}

// the predicate of samsim.h: two IEEE comparisons per term (a NaN satisfies none), the status mode, the label
template <int NT>
__device__ __forceinline__ bool sel_holds(const SelParams &p, const SelLoad<NT> &v) {
  bool ok = v.in;
  if (p.status_mode == SAMSIM_SELECT_RUNNING) ok = ok && v.st == 0;
  else if (p.status_mode == SAMSIM_SELECT_STOPPED) ok = ok && v.st != 0;
  else if (p.status_mode == SAMSIM_SELECT_CODE) ok = ok && v.st == p.code;
  if (p.labels) ok = ok && v.lab == p.group;
#pragma unroll
  for (int i = 0; i < NT; ++i) ok = ok && p.t[i].lo <= v.x[i] && v.x[i] < p.t[i].hi;
  return ok;
}

template <int NT, bool WRITE>
__global__ void __launch_bounds__(64) select_kernel(const SelParams p, long long *__restrict__ counts, const long long *__restrict__ offsets,
                                                    long long *__restrict__ list) {
  const int lane = threadIdx.x;
  const long long nblk = (p.ncol + 63) / 64;
  const long long b0 = (long long)blockIdx.x * p.per;
  long long b1 = b0 + p.per;
  if (b1 > nblk) b1 = nblk;
  long long at = 0;   // WRITE: the rank of the wave's next match; else the wave's matches so far
  if (WRITE) {
    at = offsets[blockIdx.x];
    if (at >= p.max_out) return;
  }
  SelLoad<NT> v{}, v_next{};
  if (b0 < b1) sel_load<NT>(p, b0, lane, v);
  for (long long blk = b0; blk < b1; ++blk) {
    if (blk + 1 < b1) sel_load<NT>(p, blk + 1, lane, v_next);   // the next block's loads are under way while this block is voted on
    const bool ok = sel_holds<NT>(p, v);
    const unsigned long long vote = __ballot(ok);
    if (WRITE) {
      const long long rank = at + __popcll(vote & ((1ull << lane) - 1ull));
      if (ok && rank < p.max_out) list[rank] = blk * 64 + lane;
    }
    at += __popcll(vote);
    if (WRITE && at >= p.max_out) return;
    v = v_next;
  }
  if (!WRITE && lane == 0) counts[blockIdx.x] = at;
}

// One wave: lane l sums the counts of the waves [l * each, (l + 1) * each) in wave order, the 64 sums are scanned across the lanes,
// and lane l writes the exclusive offsets of its waves; lane 63 holds the total.  Integers: the order does not matter to the result.
__global__ void __launch_bounds__(64) select_scan_kernel(const long long *__restrict__ counts, int nwaves, long long *__restrict__ offsets) {
  const int lane = threadIdx.x;
  const int each = (nwaves + 63) / 64;
  const int w0 = lane * each;
  long long mine = 0;
  for (int i = 0; i < each; ++i)
    if (w0 + i < nwaves) mine += counts[w0 + i];
  long long incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  long long run = incl - mine;
  for (int i = 0; i < each; ++i)
    if (w0 + i < nwaves) { offsets[w0 + i] = run; run += counts[w0 + i]; }
  if (lane == 63) offsets[DEV_SEL_GRID] = incl;
}

template <int NT>
hipError_t select_launch(const SelParams &p, long long *counts, long long *offsets, long long *list, hipStream_t stream) {
  hipLaunchKernelGGL((select_kernel<NT, false>), dim3((unsigned)p.nwaves), dim3(64), 0, stream, p, counts, offsets, list);
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(64), 0, stream, counts, (int)p.nwaves, offsets);
  if (p.max_out > 0) hipLaunchKernelGGL((select_kernel<NT, true>), dim3((unsigned)p.nwaves), dim3(64), 0, stream, p, counts, offsets, list);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256) gather_layers_kernel(const double *__restrict__ lay, const long long *__restrict__ cols,
                                                            const int32_t *__restrict__ n_active, const int32_t *__restrict__ status,
                                                            const int32_t *__restrict__ flags, double *__restrict__ stage, int narr, int N,
                                                            size_t ncol, size_t w, int stepped) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)narr * N * w) return;
  const size_t j = i % w, ak = i / w;
  const int k = (int)(ak % (size_t)N), a = (int)(ak / (size_t)N);
  const size_t c = (size_t)cols[j];
  double v = lay[DEV_LAY_INDEX(a, k, c, N, ncol)];
  // what samsim_get_state does to the device copy before it reads it (clamp_s_abs and refresh_s_bu of samsim_capi.cpp): the layers
  // below the active ones keep what they hold
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
  stage[i] = v;
}

__global__ void __launch_bounds__(256) gather_columns_kernel(const double *__restrict__ scal, const int32_t *__restrict__ n_active,
                                                             const int32_t *__restrict__ status, const long long *__restrict__ err_step,
                                                             const int32_t *__restrict__ err_layer, const long long *__restrict__ cols,
                                                             double *__restrict__ o_scal, long long *__restrict__ o_step,
                                                             int32_t *__restrict__ o_na, int32_t *__restrict__ o_status,
                                                             int32_t *__restrict__ o_layer, size_t ncol, size_t w) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= w) return;
  const size_t c = (size_t)cols[j];
#pragma unroll 2
  for (int r = 0; r < SAMSIM_NSCAL; ++r) o_scal[(size_t)r * w + j] = scal[(size_t)r * ncol + c];
  o_step[j] = err_step[c];
  o_na[j] = n_active[c];
  o_status[j] = status[c];
  o_layer[j] = err_layer[c];
}

}  // namespace

extern "C" hipError_t samsim_launch_select(const SelParams *p, void *scratch, hipStream_t stream) {
  long long *counts = (long long *)scratch;
  long long *offsets = (long long *)((char *)scratch + DEV_SEL_OFFSETS_AT);
  long long *list = (long long *)((char *)scratch + DEV_SEL_LIST_AT);
  switch (p->nterms) {
    case 0: return select_launch<0>(*p, counts, offsets, list, stream);
    case 1: return select_launch<1>(*p, counts, offsets, list, stream);
    case 2: return select_launch<2>(*p, counts, offsets, list, stream);
    case 3: return select_launch<3>(*p, counts, offsets, list, stream);
    case 4: return select_launch<4>(*p, counts, offsets, list, stream);
  }
  return hipErrorInvalidValue;
}

extern "C" hipError_t samsim_launch_gather_layers(const double *lay, const long long *cols, const int32_t *n_active, const int32_t *status,
                                                  const int32_t *flags, double *stage, int narr, int N, long long ncol, long long w,
                                                  int stepped, hipStream_t stream) {
  const size_t n = (size_t)narr * (size_t)N * (size_t)w;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_layers_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, lay, cols, n_active, status, flags, stage,
                     narr, N, (size_t)ncol, (size_t)w, stepped);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_gather_columns(const double *scal, const int32_t *n_active, const int32_t *status,
                                                   const long long *err_step, const int32_t *err_layer, const long long *cols, void *stage,
                                                   long long ncol, long long w, hipStream_t stream) {
  if (w <= 0) return hipSuccess;
  const size_t n = (size_t)w;
  double *o_scal = (double *)stage;
  long long *o_step = (long long *)(o_scal + (size_t)SAMSIM_NSCAL * n);
  int32_t *o_na = (int32_t *)(o_step + n);
  hipLaunchKernelGGL(gather_columns_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, scal, n_active, status, err_step, err_layer,
                     cols, o_scal, o_step, o_na, o_na + n, o_na + 2 * n, (size_t)ncol, n);
  return hipGetLastError();
}
