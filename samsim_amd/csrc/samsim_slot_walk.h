// samsim_slot_walk.h -- what the reductions of the per-column scalars ("slots") share: the per-group statistics
// (samsim_groups.hip), the scalar histograms (samsim_hist.hip), the covariances (samsim_sens.hip) and the weight row with its
// weighted reductions (samsim_weights.hip).  The step kernel does not include this header.
//
// One wave owns one 64-column block at a time (lane = column) and strides over the blocks with a fixed grid that depends on ncol
// alone.  ColSet says which columns count and what their value is, the loaders read the lane's column of a block with coalesced
// loads, walk_blocks has the next block's loads under way while this block is consumed.  A wave leaves one partial; merge_waves
// combines the waves' partials in wave order with one bracketing whatever the data: lane l takes the waves [l * per, (l + 1) * per)
// ascending, then lane 0 takes the 64 lanes ascending through LDS.  The byte-for-byte promises of include/samsim.h (two calls
// return the same bytes; a slot alone has the bytes it has among eight) rest on every family going through these functions.
//
// The first part is plain C++ (tests/test_host_logic.py compiles it alone), the second needs hipcc.
#ifndef SAMSIM_SLOT_WALK_H
#define SAMSIM_SLOT_WALK_H

#include <cstdint>
#include <type_traits>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SLOT_HD __host__ __device__
#else
#define SLOT_HD
#endif

namespace slot_walk {

constexpr int kLaneStride = 65;   // doubles from one quantity's 64 lane values to the next in LDS

// the 64-column blocks of ncol columns
SLOT_HD constexpr long long col_blocks(long long ncol) { return (ncol + 63) / 64; }

// the grid of a reduction: one-wave workgroups, one per block and at most cap (the number of waves decides the merge order)
inline int slot_grid(long long ncol, long long cap) {
  const long long nblk = col_blocks(ncol);
  return (int)(nblk < cap ? nblk : cap);
}

// pair p of the upper triangle of ns slots, row by row: (0,0), (0,1), .. (0,ns-1), (1,1), ..
SLOT_HD constexpr void pair_of(int p, int ns, int &i, int &j) {
  i = 0;
  while (p >= ns - i) { p -= ns - i; ++i; }
  j = i + p;
}

// f(std::integral_constant<int, NS>) for NS == nslots; false, and no call, outside 1 .. 8 (SAMSIM_SENS_MAX_SLOTS)
template <class F>
inline bool dispatch_nslots(int nslots, F f) {
  switch (nslots) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 3: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 5: f(std::integral_constant<int, 5>{}); return true;
    case 6: f(std::integral_constant<int, 6>{}); return true;
    case 7: f(std::integral_constant<int, 7>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
    default: return false;
  }
}

#ifdef __HIPCC__

// Which columns a reduction ranges over.  The fields of either set stand in the order the kernels took them as single arguments,
// so a kernel that takes the set by value in their place keeps its kernarg offsets.
struct ColRows {
  const int32_t *n_active, *status, *labels;   // [ncol] rows; labels null: every column with status 0 counts
  // a null row is n_active
  __device__ __forceinline__ double value(const double *row, long long col) const { return row ? row[col] : (double)n_active[col]; }
};
// one group: with labels, only the columns with label `group` count
struct ColSet : ColRows {
  int group;
  long long ncol;
  __device__ __forceinline__ bool in(long long col) const { return status[col] == 0 && (!labels || labels[col] == group); }
};
// the per-label flavour of the group statistics and the histograms: every group at once
struct LabelSet : ColRows {
  long long ncol;
  // the column's group, -1 where it does not count; without labels every column is of group 0
  __device__ __forceinline__ int label(long long col, int ngroups) const {
    const int l = labels ? labels[col] : 0;
    return (status[col] == 0 && l < ngroups) ? l : -1;
  }
};

// the lane's column of a block: whether it counts, its weight and its values of NS rows
template <int NS>
struct Cols {
  bool ok;
  double w, v[NS];
};
// ok: in the set, within ncol, and w > 0; a null w is a weight of one everywhere
template <int NS>
__device__ __forceinline__ void load_cols(const ColSet &cs, const double *const *rows, const double *w, long long blk, int lane,
                                          Cols<NS> &c) {
  const long long col = blk * 64 + lane;
  c.ok = false; c.w = 0.0;
#pragma unroll
  for (int i = 0; i < NS; ++i) c.v[i] = 0.0;
  if (col < cs.ncol) {
    c.w = w ? w[col] : 1.0;
    c.ok = cs.in(col) && c.w > 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) c.v[i] = cs.value(rows[i], col);
  }
}

// one row
__device__ __forceinline__ void load_cols(const ColSet &cs, const double *row, const double *w, long long blk, int lane, Cols<1> &c) {
  load_cols<1>(cs, &row, w, blk, lane, c);
}

// the per-label flavour: the column's group (-1: stopped, unlabelled or beyond ncol) and its value
struct LabelCol {
  int lab;
  double v;
};
__device__ __forceinline__ void load_label_col(const LabelSet &cs, const double *row, int ngroups, long long blk, int lane, LabelCol &c) {
  const long long col = blk * 64 + lane;
  c.lab = -1; c.v = 0.0;
  if (col < cs.ncol) {
    c.lab = cs.label(col, ngroups);
    c.v = cs.value(row, col);
  }
}

// The wave's blocks blockIdx.x, blockIdx.x + gridDim.x, ..: load(blk, lane, V &) reads the lane's column, use(blk, const V &)
// consumes it; the next block's loads are under way while this block is consumed.
template <class V, class Load, class Use>
__device__ __forceinline__ void walk_blocks(long long ncol, int lane, Load load, Use use) {
  const long long nblk = col_blocks(ncol);
  V cur, next = V();
  load(blockIdx.x, lane, cur);
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    if (blk + gridDim.x < nblk) load(blk + gridDim.x, lane, next);
    use(blk, cur);
    cur = next;
  }
}

// lane i's value in every lane (i is the same in every lane)
__device__ __forceinline__ double lane_value(double v, int i) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), i), hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
  return __hiloint2double(hi, lo);
}

// An accumulator Acc has absorb(const Acc &b): b combined into *this, after whatever is in *this; a family with a count leaves an
// empty b (n == 0) out there, a plain sum adds every b.
// at(l) for l = 0 .. 63 ascending, absorbed into acc (empty on entry, so the first absorbed value is copied): the lanes' values in
// lane order, as the thread of a walk kernel that owns a slot or a pair combines them
template <class Acc, class At>
__device__ __forceinline__ void absorb_lanes(Acc &acc, At at) {
  for (int l = 0; l < 64; ++l) acc.absorb(at(l));
}
// The 64 lanes' accumulators in lane order through s[64] (LDS), into lane 0's own; true in lane 0, which has the result.
template <class Acc>
__device__ __forceinline__ bool fold_lanes(Acc &acc, Acc *s, int lane) {
  s[lane] = acc;
  __syncthreads();
  if (lane != 0) return false;
#pragma unroll 8   // unrolled whole, the 63 reads of a plain sum are issued at once and take 250 VGPRs
  for (int l = 1; l < 64; ++l) acc.absorb(s[l]);
  return true;
}
// The bracket of every merge kernel (one 64-lane workgroup): lane l absorbs partial(w) of the waves [l * per, (l + 1) * per)
// ascending into acc (empty on entry), then fold_lanes.
template <class Acc, class Partial>
__device__ __forceinline__ bool merge_waves(int nwaves, Acc &acc, Acc *s, int lane, Partial partial) {
  const int per = (nwaves + 63) / 64;
  for (int w = lane * per; w < (lane + 1) * per && w < nwaves; ++w) acc.absorb(partial(w));
  return fold_lanes(acc, s, lane);
}

#endif   // __HIPCC__

}  // namespace slot_walk

#endif
