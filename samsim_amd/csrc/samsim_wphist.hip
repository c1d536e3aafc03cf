// samsim_wphist.hip -- device-side weighted joint histogram of the layer profiles (samsim_get_weighted_profile_histogram,
// include/samsim.h): per depth bin x value entry the sum of the weights of samsim_set_weights over the columns that land there, from
// which the posterior median and the 5-95 % band of T(z), S_bu(z) or psi_l(z) follow as quantile brackets.
//
// A pass is that of the joint histogram (samsim_hist.hip): the walk of samsim_profile_walk.h fills the LDS tile [bin][lane], then
// lane j walks row j of the tile over the 64 columns and adds each column's weight to its own row of the wave's table -- a table
// of doubles where the counts have 32-bit entries, the block's 64 weights beside the tile as the weighted statistics keep them
// (samsim_wprofile.hip).  Only the owner lane of a row ever touches it, so a wave adds in ascending column order.  A column whose
// weight is not positive enters the walk with no active layers, as a stopped one does.  At the end every wave stores its rows;
// wphist_merge_kernel adds the waves' tables per (bin, entry) in wave order with the bracket of merge_waves (samsim_slot_walk.h).
//
// No atomics of any kind, no floating-point sum whose order depends on scheduling: two calls return the same bytes.  The kernels
// read the layer block, n_active, status, the labels and the weight row and write the handle's scratch, nothing else.
#include <hip/hip_runtime.h>

#include "samsim_profile_walk.h"
#include "samsim_wphist.h"

namespace {

using namespace profile_walk;
using namespace slot_walk;

// The lane's column of block blk: its weight (0.0 beyond ncol) and its number of active layers, 0 for a column that does not
// count.  The column rule of the weighted profile statistics (counting_layers, samsim_wprofile.hip), line for line.
__device__ __forceinline__ int counting_layers(const ProfPass &p, const double *w, long long blk, int lane, double &wv) {
  const long long col = blk * 64 + lane;
  wv = col < p.ncol ? w[col] : 0.0;
  const int na = active_layers(p, blk, lane);
  return wv > 0.0 ? na : 0;
}

// Lane j adds row j of the tile: the weights of the columns whose bit j is set in their lane's mask, in lane order, each to the
// entry of the column's value of bin j.  count_tile of samsim_hist.hip with ws[i] in the place of the 1.
__device__ __forceinline__ void add_tile(const double *tile, const double *ws, unsigned long long *smask, unsigned long long mask, int lane,
                                         int nb, const HistEdges &e, double *my_row) {
  smask[lane] = mask;
  __syncthreads();
  if (lane < nb) {
    const double *row = tile + lane * kTileStride;
    for (int i = 0; i < 64; ++i)
      if ((smask[i] >> lane) & 1ull) {
        const int en = hist_entry(row[i], e);
        my_row[en] = my_row[en] + ws[i];
      }
  }
  __syncthreads();
}

// LDS: tile [chunk][kTileStride] doubles, the lanes' masks, the block's weights, the wave's table [chunk][stride] (samsim_wphist.h)
template <int AXIS>
__global__ void __launch_bounds__(64) wphist_kernel(ProfPass p, const double *__restrict__ w, HistEdges e, int chunk,
                                                    double *__restrict__ tables) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x, W = e.nvbins + 2, stride = W | 1;
  double *tile = (double *)lds;
  unsigned long long *smask = (unsigned long long *)(tile + (size_t)chunk * kTileStride);
  double *ws = (double *)(smask + 64);
  double *table = ws + 64;
  for (int i = lane; i < chunk * stride; i += 64) table[i] = 0.0;
  __syncthreads();
  const long long nblk = col_blocks(p.ncol);
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    double wv;
    const int na = counting_layers(p, w, blk, lane, wv);
    TileSink sink{tile, lane, 0};
    walk_block<AXIS>(p, blk, lane, na, sink);
    ws[lane] = wv;
    add_tile(tile, ws, smask, sink.mask, lane, p.nb, e, table + lane * stride);
  }
  // the wave's nb rows, dense, to its table [chunk][W] in device memory
  double *mine = tables + (size_t)blockIdx.x * (size_t)chunk * (size_t)W;
  for (int r = 0; r < p.nb; ++r)
    for (int i = lane; i < W; i += 64) mine[(size_t)r * W + i] = table[r * stride + i];
}

// plain sums of DEV_WPHIST_MERGE_ENTRIES neighbouring entries: every partial is added, in order, entry by entry
struct SumsOf {
  double s[DEV_WPHIST_MERGE_ENTRIES];
  __device__ __forceinline__ void absorb(const SumsOf &b) {
#pragma unroll
    for (int k = 0; k < DEV_WPHIST_MERGE_ENTRIES; ++k) s[k] = s[k] + b.s[k];
  }
};

// One workgroup per DEV_WPHIST_MERGE_ENTRIES entries of the pass's rows, taken as one row of total = nb * W entries: the waves'
// tables in wave order.  An entry's sum is that of whist_merge_kernel (samsim_weights.hip) whatever its neighbours hold.
__global__ void __launch_bounds__(64) wphist_merge_kernel(const double *__restrict__ tables, int nwaves, size_t wave_doubles, int total,
                                                          double *__restrict__ out) {
  __shared__ SumsOf s_sum[64];
  const int at = blockIdx.x * DEV_WPHIST_MERGE_ENTRIES;
  SumsOf sum;
#pragma unroll
  for (int k = 0; k < DEV_WPHIST_MERGE_ENTRIES; ++k) sum.s[k] = 0.0;
  const bool last = merge_waves(nwaves, sum, s_sum, threadIdx.x, [&](int wv) {
    const double *t = tables + (size_t)wv * wave_doubles + at;
    SumsOf b;
#pragma unroll
    for (int k = 0; k < DEV_WPHIST_MERGE_ENTRIES; ++k) b.s[k] = at + k < total ? t[k] : 0.0;
    return b;
  });
  if (!last) return;
#pragma unroll
  for (int k = 0; k < DEV_WPHIST_MERGE_ENTRIES; ++k)
    if (at + k < total) out[at + k] = sum.s[k];
}

}  // namespace

extern "C" hipError_t samsim_launch_weighted_profile_hist(ProfPass p, const double *w, HistEdges e, double *tables, double *result,
                                                          hipStream_t stream) {
  if (e.nvbins < 1 || e.nvbins > SAMSIM_HIST_MAX_VBINS) return hipErrorInvalidValue;
  const int chunk = dev_wphist_chunk(e.nvbins), W = e.nvbins + 2;
  const size_t lds = (size_t)dev_wphist_lds(e.nvbins);
  const int grid = pass_grid(p, DEV_WPHIST_GRID, chunk);
  if (!grid || lds > DEV_WPHIST_LDS_BYTES) return hipErrorInvalidValue;
  if (p.axis == SAMSIM_PROFILE_BY_LAYER)
    hipLaunchKernelGGL(wphist_kernel<SAMSIM_PROFILE_BY_LAYER>, dim3(grid), dim3(64), lds, stream, p, w, e, chunk, tables);
  else
    hipLaunchKernelGGL(wphist_kernel<SAMSIM_PROFILE_BY_DEPTH>, dim3(grid), dim3(64), lds, stream, p, w, e, chunk, tables);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int total = p.nb * W;
  hipLaunchKernelGGL(wphist_merge_kernel, dim3((total + DEV_WPHIST_MERGE_ENTRIES - 1) / DEV_WPHIST_MERGE_ENTRIES), dim3(64), 0, stream,
                     tables, grid, (size_t)chunk * (size_t)W, total, result + (size_t)p.b0 * W);
  return hipGetLastError();
}
