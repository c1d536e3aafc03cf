// samsim_profile_walk.h -- how one wave walks the layers of one 64-column block and finds every column's value in every bin of a
// profile request (include/samsim.h, samsim_get_profile_stats): shared by the four reductions of samsim_profile.h, which differ only
// in what they do with the finished values.  The step kernel does not include this header.
//
// A walk serves one pass (ProfPass): one requested array and the bins [b0, b0 + nb) of the request, nb <= 64, for one block
// (lane = column), through walk_block<AXIS>.  It reads
// 512-byte rows from the device layout [block][layer][array][64]; only the rows the request needs are touched (the array itself --
// S_abs and m for S_bu -- and thick for the depth axis), and the rows of kAhead layers are requested before the first is waited
// for.  Every lane moves through the bins of its own column monotonically and hands each finished bin value to the sink:
//   sink.put(r, v)   -- the lane's column has the value v in bin b0 + r, 0 <= r < nb; at most once per (lane, r) and block.
#ifndef SAMSIM_PROFILE_WALK_H
#define SAMSIM_PROFILE_WALK_H

#include <hip/hip_runtime.h>

#include "samsim_column_read.h"
#include "samsim_profile.h"

namespace profile_walk {

using namespace column_read;   // kRow, wave_max, wave_min, ld

constexpr int kAhead = 8;                        // layers whose rows a wave requests before it waits for the first
constexpr int kTileStride = DEV_PROF_BINS + 1;   // row stride of the LDS tile in doubles: lane j reads row j without a bank pile-up

// The sink both reductions use: an LDS tile [bin][lane] of the block's values and, per lane, the mask of the bins its column
// reached.  After the block lane j walks row j of the tile (a transposition through LDS).
struct TileSink {
  double *tile;
  int lane;
  unsigned long long mask;
  __device__ __forceinline__ void put(int r, double v) {
    tile[r * kTileStride + lane] = v;
    mask |= 1ull << r;
  }
};

// The value of the requested array in one layer row (`row` = the lane's element of array 0 of that layer) in two halves, so that a
// wave can request the rows of several layers before it waits for the first: row_request loads the stored value -- for the bulk
// salinity S_abs and m --, requested_value forms a_k from them.  The profile requests read the layer value of
// samsim_column_read.h with clamp = false and adjust = true, whatever the column: S_abs as stored and S_bu always as the quotient
// where m != 0 (a stopped column takes no part).  That is their documented definition ("Layer value" of samsim_get_profile_stats,
// include/samsim.h), kept as it is.
__device__ __forceinline__ void row_request(const double *row, int array, double &x, double &y) {
  const bool sbu = array == SAMSIM_A_S_BU;
  x = ld(row + (sbu ? (int)SAMSIM_A_S_ABS : array) * 64);
  y = sbu ? ld(row + SAMSIM_A_M * 64) : 1.0;
}
__device__ __forceinline__ double requested_value(const double *row, int array, double x, double y) {
  if (array != SAMSIM_A_S_BU) return x;
  return s_bu_value(x, y, /*adjust=*/true, /*clamp=*/false, [&] { return ld(row + SAMSIM_A_S_BU * 64); });
}

// the lane's column of block blk: its number of active layers, 0 for a column that stopped, lies beyond ncol or -- with a label row
// (samsim_get_group_profile_stats) -- carries another label than `group`: such a column behaves like a stopped one
__device__ __forceinline__ int active_layers(const int32_t *n_active, const int32_t *status, const int32_t *labels, int group, long long ncol,
                                             long long blk, int lane, int N) {
  const long long col = blk * 64 + lane;
  if (col >= ncol || status[col] != 0) return 0;
  if (labels && labels[col] != group) return 0;
  return layers_within(n_active[col], N);
}
__device__ __forceinline__ int active_layers(const ProfPass &p, long long blk, int lane) {
  return active_layers(p.n_active, p.status, p.labels, p.group, p.ncol, blk, lane, p.N);
}

// ---- layer axis: bin b holds layer b+1 (from the top) or layer N_active-b (from the bottom); bins [b0, b0+nb) of block blk,
// na = active_layers() of the lane's column
template <class Sink>
__device__ __forceinline__ void layer_block(const double *__restrict__ lay, long long ncol, int N, long long blk, int lane, int na, int origin,
                                            int array, int b0, int nb, Sink &sink) {
  const int kmax = wave_max(na);
  const double *base = lay + DEV_LAY_INDEX(0, 0, blk * 64 + lane, N, ncol);   // the lane's element of array 0, layer 1
  int klo, khi;
  if (origin == SAMSIM_PROFILE_FROM_TOP) {
    klo = b0 + 1;
    khi = b0 + nb < kmax ? b0 + nb : kmax;
  } else {
    const int kmin = wave_min(na > 0 ? na : N + 1);   // fewest active layers among the columns that count
    klo = kmin - b0 - nb + 1;
    klo = klo < 1 ? 1 : klo;
    khi = kmax - b0;
  }
  for (int k0 = klo; k0 <= khi; k0 += kAhead) {   // the rows of kAhead layers requested together
    double x[kAhead], y[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      x[u] = y[u] = 0.0;
      if (k0 + u <= khi) row_request(base + (size_t)(k0 + u - 1) * kRow, array, x[u], y[u]);
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const int k = k0 + u;
      const int r = origin == SAMSIM_PROFILE_FROM_TOP ? k - 1 - b0 : na - k - b0;
      if (k <= khi && k <= na && r >= 0 && r < nb) sink.put(r, requested_value(base + (size_t)(k - 1) * kRow, array, x[u], y[u]));
    }
  }
}

// ---- depth axis: bin b is [z0 + b dz, z0 + (b+1) dz) below the ice surface (from the top) or above the ice bottom; a column's
// value in a bin is the overlap-weighted mean of its layers there (samsim.h); bins [b0, b0+nb) of block blk.  lead: the chunk does
// not begin where the walk begins (from the top: b0 > 0; from the bottom: not the last chunk).
template <class Sink>
__device__ __forceinline__ void depth_block(const double *__restrict__ lay, long long ncol, int N, long long blk, int lane, int na, int origin,
                                            int array, int b0, int nb, int lead, double z0, double dz, Sink &sink) {
  const bool top = origin == SAMSIM_PROFILE_FROM_TOP;
  const int kmax = wave_max(na);
  const double *base = lay + DEV_LAY_INDEX(0, 0, blk * 64 + lane, N, ncol);   // the lane's element of array 0, layer 1
  const double H = top ? 0.0 : ice_thickness(base, na, kmax);
  int cur = top ? b0 : b0 + nb - 1;   // the bin the lane's column is filling
  const int step = top ? 1 : -1;
  double Z = 0.0, W = 0.0, L = 0.0;
  for (int k0 = 1; k0 <= kmax; k0 += kAhead) {   // the rows of kAhead layers requested together, then the lanes' bin walks
    // the rows only while some column of the wave still has bins of this chunk to fill
    if (!__any(k0 <= na && cur >= b0 && cur < b0 + nb)) break;
    double tk[kAhead], x[kAhead], y[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      tk[u] = 0.0;
      if (k0 + u <= kmax) tk[u] = ld(base + (size_t)(k0 + u - 1) * kRow + SAMSIM_A_THICK * 64);
    }
    if (lead) {
      // A chunk that does not begin where the walk begins: while no column of the wave has reached the chunk the layers overlap
      // none of its bins, so only Z moves on -- by the same additions -- and the array rows are not requested.
      double Ze = Z;
#pragma unroll
      for (int u = 0; u < kAhead; ++u) Ze = k0 + u <= na ? Ze + tk[u] : Ze;
      const bool reached = top ? Ze > z0 + (double)b0 * dz : H - Ze < z0 + (double)(b0 + nb) * dz;
      if (!__any(reached && k0 <= na)) {
        Z = Ze;
        continue;
      }
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      x[u] = y[u] = 0.0;
      if (k0 + u <= kmax) row_request(base + (size_t)(k0 + u - 1) * kRow, array, x[u], y[u]);
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const int k = k0 + u;
      if (k <= na) {
        const double a = requested_value(base + (size_t)(k - 1) * kRow, array, x[u], y[u]);
        const double Zn = Z + tk[u];
        const double lo = top ? Z : H - Zn, hi = top ? Zn : H - Z;
        while (cur >= b0 && cur < b0 + nb) {
          const double e0 = z0 + (double)cur * dz, e1 = z0 + (double)(cur + 1) * dz;
          const double xo = (hi < e1 ? hi : e1) - (lo > e0 ? lo : e0);
          const double o = xo > 0.0 ? xo : 0.0;
          L += o;
          W += o * a;
          if (!(top ? hi > e1 : lo < e0)) break;   // the layer ends inside this bin
          if (L > 0.0) sink.put(cur - b0, W / L);
          W = 0.0; L = 0.0;
          cur += step;
        }
        Z = Zn;
      }
    }
  }
  if (cur >= b0 && cur < b0 + nb && L > 0.0) sink.put(cur - b0, W / L);   // the bin in which the column ends
}

// the walk of the pass's axis, chosen at compile time: a family's kernel is one template over AXIS
template <int AXIS, class Sink>
__device__ __forceinline__ void walk_block(const ProfPass &p, long long blk, int lane, int na, Sink &sink) {
  if (AXIS == SAMSIM_PROFILE_BY_LAYER) layer_block(p.lay, p.ncol, p.N, blk, lane, na, p.origin, p.array, p.b0, p.nb, sink);
  else depth_block(p.lay, p.ncol, p.N, blk, lane, na, p.origin, p.array, p.b0, p.nb, p.lead, p.z0, p.dz, sink);
}

}  // namespace profile_walk

#endif
