// samsim_hist.hip -- device-side fixed-edge histograms of the ensemble (samsim_get_histogram, samsim_get_profile_histogram,
// include/samsim.h): of a per-column scalar over all columns or per group, and of the layer profiles as a joint histogram over
// depth bin x value bin.
//
// Scalars: the walk of samsim_slot_walk.h, every column counted where its label and its value say.
// Profiles: a pass of samsim_profile.h, whose walk (samsim_profile_walk.h) fills the LDS tile [bin][lane]; then lane j walks
// row j of the tile and increments its own row of the count table -- no atomics in the loop.  Either way a wave counts in
// 32-bit LDS entries and adds its table to the 64-bit result with integer atomics at the end (samsim_hist.h); there is no
// floating-point atomic and no floating-point sum at all, so two calls return the same bytes.
#include <hip/hip_runtime.h>

#include "samsim_hist.h"
#include "samsim_profile_walk.h"

namespace {

using namespace profile_walk;
using namespace slot_walk;

// what a wave counted, added to the 64-bit result
__device__ __forceinline__ void flush_table(const uint32_t *table, int n, int lane, unsigned long long *out) {
  for (int i = lane; i < n; i += 64) {
    const uint32_t c = table[i];
    if (c) atomicAdd(out + i, (unsigned long long)c);
  }
}

// LDS: the wave's table [ngroups][W] of 32-bit counts in LDS (dev_hist_in_lds); else every lane adds into the result itself
template <bool LDS>
__global__ void __launch_bounds__(64) hist_kernel(const double *__restrict__ row, LabelSet cs, int ngroups, HistEdges e,
                                                  unsigned long long *__restrict__ counts) {
  extern __shared__ uint32_t table[];   // [ngroups][W]
  const int lane = threadIdx.x, W = e.nvbins + 2;
  if (LDS) {
    for (int i = lane; i < ngroups * W; i += 64) table[i] = 0;
    __syncthreads();
  }
  walk_blocks<LabelCol>(
      cs.ncol, lane, [&](long long blk, int ln, LabelCol &c) { load_label_col(cs, row, ngroups, blk, ln, c); },
      [&](long long, const LabelCol &c) {
        if (c.lab >= 0) {
          const int i = c.lab * W + hist_entry(c.v, e);
          if (LDS) atomicAdd(table + i, 1u);
          else atomicAdd(counts + i, 1ull);
        }
      });
  if (LDS) {
    __syncthreads();
    flush_table(table, ngroups * W, lane, counts);
  }
}

// Lane j counts row j of the tile: the values of bin j of the columns whose bit j is set in their lane's mask.
__device__ __forceinline__ void count_tile(const double *tile, unsigned long long *smask, unsigned long long mask, int lane, int nb,
                                           const HistEdges &e, uint32_t *my_row) {
  smask[lane] = mask;
  __syncthreads();
  if (lane < nb) {
    const double *row = tile + lane * kTileStride;
    for (int i = 0; i < 64; ++i)
      if ((smask[i] >> lane) & 1ull) my_row[hist_entry(row[i], e)] += 1;
  }
  __syncthreads();
}

// LDS of the two profile kernels: tile [chunk][kTileStride] doubles, the lanes' masks, the count table [chunk][stride] (samsim_hist.h)
struct ProfLds {
  double *tile;
  unsigned long long *smask;
  uint32_t *table;
};
__device__ __forceinline__ ProfLds carve(unsigned char *lds, int chunk, int stride, int lane) {
  ProfLds p;
  p.tile = (double *)lds;
  p.smask = (unsigned long long *)(p.tile + (size_t)chunk * kTileStride);
  p.table = (uint32_t *)(p.smask + 64);
  for (int i = lane; i < chunk * stride; i += 64) p.table[i] = 0;
  __syncthreads();
  return p;
}
// the wave's rows of the table added to rows b0 .. b0+nb-1 of the result [nbins][W]
__device__ __forceinline__ void flush_rows(const uint32_t *table, int stride, int nb, int W, int lane, unsigned long long *out) {
  __syncthreads();
  for (int r = 0; r < nb; ++r) flush_table(table + r * stride, W, lane, out + (size_t)r * W);
}

// The layer / depth pair as it was before the pass descriptor: hist_profile_kernel<AXIS>(ProfPass, ...) measured 0.7 % slower at
// 254 value bins (docs/HISTORY.md, "Profile reductions: one pass descriptor"), so this family keeps its two kernels.
__global__ void __launch_bounds__(64) hist_layer_kernel(const double *__restrict__ lay, const int32_t *__restrict__ n_active,
                                                        const int32_t *__restrict__ status, const int32_t *__restrict__ labels, int group,
                                                        long long ncol, int N, int origin, int array, int b0, int nb, int chunk,
                                                        HistEdges e, unsigned long long *__restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x, stride = (e.nvbins + 2) | 1;
  const ProfLds p = carve(lds, chunk, stride, lane);
  const long long nblk = col_blocks(ncol);
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(n_active, status, labels, group, ncol, blk, lane, N);
    TileSink sink{p.tile, lane, 0};
    layer_block(lay, ncol, N, blk, lane, na, origin, array, b0, nb, sink);
    count_tile(p.tile, p.smask, sink.mask, lane, nb, e, p.table + lane * stride);
  }
  flush_rows(p.table, stride, nb, e.nvbins + 2, lane, counts + (size_t)b0 * (e.nvbins + 2));
}

__global__ void __launch_bounds__(64) hist_depth_kernel(const double *__restrict__ lay, const int32_t *__restrict__ n_active,
                                                        const int32_t *__restrict__ status, const int32_t *__restrict__ labels, int group,
                                                        long long ncol, int N, int origin, int array, int b0, int nb, int chunk, int lead,
                                                        double z0, double dz, HistEdges e, unsigned long long *__restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x, stride = (e.nvbins + 2) | 1;
  const ProfLds p = carve(lds, chunk, stride, lane);
  const long long nblk = col_blocks(ncol);
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(n_active, status, labels, group, ncol, blk, lane, N);
    TileSink sink{p.tile, lane, 0};
    depth_block(lay, ncol, N, blk, lane, na, origin, array, b0, nb, lead, z0, dz, sink);
    count_tile(p.tile, p.smask, sink.mask, lane, nb, e, p.table + lane * stride);
  }
  flush_rows(p.table, stride, nb, e.nvbins + 2, lane, counts + (size_t)b0 * (e.nvbins + 2));
}

}  // namespace

extern "C" hipError_t samsim_launch_hist(LabelSet cs, const double *row, int ngroups, HistEdges e, unsigned long long *counts,
                                         hipStream_t stream) {
  const int grid = slot_grid(cs.ncol, DEV_HIST_GRID);
  if (dev_hist_in_lds(ngroups, e.nvbins))
    hipLaunchKernelGGL(hist_kernel<true>, dim3(grid), dim3(64), sizeof(uint32_t) * (size_t)ngroups * (e.nvbins + 2), stream, row, cs,
                       ngroups, e, counts);
  else
    hipLaunchKernelGGL(hist_kernel<false>, dim3(grid), dim3(64), 0, stream, row, cs, ngroups, e, counts);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_profile_hist(ProfPass p, HistEdges e, unsigned long long *counts, hipStream_t stream) {
  const int chunk = dev_hist_chunk(e.nvbins);
  const size_t lds = dev_hist_profile_lds(e.nvbins);
  const int grid = pass_grid(p, DEV_HIST_GRID, chunk);
  if (!grid || lds > DEV_HIST_LDS_BYTES) return hipErrorInvalidValue;
  if (p.axis == SAMSIM_PROFILE_BY_LAYER)
    hipLaunchKernelGGL(hist_layer_kernel, dim3(grid), dim3(64), lds, stream, p.lay, p.n_active, p.status, p.labels, p.group, p.ncol, p.N,
                       p.origin, p.array, p.b0, p.nb, chunk, e, counts);
  else
    hipLaunchKernelGGL(hist_depth_kernel, dim3(grid), dim3(64), lds, stream, p.lay, p.n_active, p.status, p.labels, p.group, p.ncol, p.N,
                       p.origin, p.array, p.b0, p.nb, chunk, p.lead, p.z0, p.dz, e, counts);
  return hipGetLastError();
}
