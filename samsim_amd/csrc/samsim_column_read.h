// samsim_column_read.h -- how a diagnostic reads a column: the one definition of the layer value samsim_get_state returns, and the
// pieces every walk over the layer rows of a 64-column block shares.  Device code only, no kernel; the step kernel does not include
// this header.
//
// The layer value ("The layer value"): after a step, in a column with status 0, S_abs carries the health check's clamp
// S_abs >= 0 -- but not in a column uploaded since the last step (COLF_RESTART) -- and S_bu is S_abs / m where m != 0; everywhere
// else, and for every other array, the value is the stored one.  Column says which of the two adjustments a column takes, s_abs_value
// and s_bu_value are the arithmetic on values the caller has loaded (the loads, their kind and their lead stay the caller's), and
// row_value applies them to one of four loaded rows by a layer_mode.
#ifndef SAMSIM_COLUMN_READ_H
#define SAMSIM_COLUMN_READ_H

#include <hip/hip_runtime.h>

#include "samsim_device.h"

namespace column_read {

constexpr size_t kRow = DEV_ROWB / sizeof(double);   // doubles from one layer row of a 64-column block to the next (samsim_device.h)

__device__ __forceinline__ int wave_max(int v) {
  for (int w = 32; w > 0; w >>= 1) { const int o = __shfl_xor(v, w); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
  for (int w = 32; w > 0; w >>= 1) { const int o = __shfl_xor(v, w); v = o < v ? o : v; }
  return v;
}

__device__ __forceinline__ double ld(const double *p) { return __builtin_nontemporal_load(p); }

// what a walk knows of its column before it reads a layer
struct Column {
  int na_raw;    // n_active as stored
  int na;        // the same within [0, N]: the layers a walk visits
  bool adjust;   // the column runs and the kernel has run: S_bu is the quotient
  bool clamp;    // and the column was not uploaded since the last step: S_abs carries the clamp
};
__device__ __forceinline__ int layers_within(int na_raw, int N) { return na_raw < 0 ? 0 : (na_raw > N ? N : na_raw); }
__device__ __forceinline__ Column column(const int32_t *n_active, const int32_t *status, const int32_t *flags, size_t c, int N, bool stepped) {
  Column q;
  q.na_raw = n_active[c];
  q.na = layers_within(q.na_raw, N);
  q.adjust = stepped && status[c] == 0;
  q.clamp = q.adjust && (flags[c] & COLF_RESTART) == 0;
  return q;
}

__device__ __forceinline__ double s_abs_value(double x, bool clamp) { return (clamp && x < 0.0) ? 0.0 : x; }
// stored() fetches the stored S_bu of the layer, and is called only in a column that is not adjusted or in the rare lane with m = 0
template <class Stored>
__device__ __forceinline__ double s_bu_value(double s_abs, double m, bool adjust, bool clamp, Stored stored) {
  if (adjust && m != 0.0) return s_abs_value(s_abs, clamp) / m;
  return stored();
}

// how the layer value a_k is formed from the loaded rows of a walk (the host's row plan sets it, samsim_capi.cpp)
enum layer_mode {
  LAYER_PLAIN = 0,   // the stored value of row ia
  LAYER_S_ABS,       // row ia is S_abs
  LAYER_S_BU         // row ia is S_abs, row ib is m
};
// a_k from the loaded rows x0..x3 of a walk; row = the lane's element of array 0 of that layer
__device__ __forceinline__ double row_value(int mode, int ia, int ib, double x0, double x1, double x2, double x3, const double *row,
                                            bool adjust, bool clamp) {
  const double xa = ia == 0 ? x0 : (ia == 1 ? x1 : (ia == 2 ? x2 : x3));
  if (mode == LAYER_S_ABS) return s_abs_value(xa, clamp);
  if (mode == LAYER_S_BU) {
    const double m = ib == 0 ? x0 : (ib == 1 ? x1 : (ib == 2 ? x2 : x3));
    return s_bu_value(xa, m, adjust, clamp, [&] { return ld(row + SAMSIM_A_S_BU * 64); });
  }
  return xa;
}

// the ice thickness of the lane's column, a thick-only pass before the walk: Z_k = Z_{k-1} + thick(k), k ascending; base = the lane's
// element of array 0, layer 1, kmax = wave_max(na)
__device__ __forceinline__ double ice_thickness(const double *base, int na, int kmax) {
  double H = 0.0;
#pragma unroll 4
  for (int k = 1; k <= kmax; ++k) {
    const double t = ld(base + (size_t)(k - 1) * kRow + SAMSIM_A_THICK * 64);
    H = k <= na ? H + t : H;
  }
  return H;
}

}  // namespace column_read

#endif
