// samsim_profile.hip -- device-side ensemble statistics of the layer profiles (samsim_get_profile_stats, include/samsim.h).
//
// One pass of the reduction serves one requested array and one chunk of at most DEV_PROF_BINS bins.  One wave owns one 64-column
// block at a time (lane = column) and strides over the blocks with a fixed grid.  The wave walks the layers k of its block with
// 512-byte row loads from the device layout [block][layer][array][64]; only the rows the request needs are touched (the array
// itself -- S_abs and m for S_bu -- and thick for the depth axis).  Every lane moves through the bins of its own column
// monotonically and drops each finished bin value v into an LDS tile [bin][lane].  After the block, lane j folds row j of the
// tile in lane order into its own running (n, mean, M2, min, max) of bin j: a transposition through LDS, no cross-lane
// reduction, no atomics.  At the end every wave stores its 64 partials; profile_merge_kernel combines the waves' partials in
// wave order (Chan's pairwise update), so the result depends on nothing but the state and the request.
#include <hip/hip_runtime.h>

#include "samsim_device.h"

namespace {

constexpr int kAhead = 8;                        // layers whose rows a wave requests before it waits for the first
constexpr size_t kRow = DEV_ROWB / sizeof(double);   // doubles from one layer row of a 64-column block to the next (samsim_device.h)
constexpr int kTileStride = DEV_PROF_BINS + 1;   // row stride of the LDS tile in doubles: lane j reads row j without a bank pile-up

// running statistics of one bin in one lane: n values with mean `mean` and sum of squared deviations `m2`
struct Run {
  long long n;
  double mean, m2, mn, mx;
};

// Chan et al.: (n, mean, M2) of the union of two sets from those of the sets; b is not empty
__device__ __forceinline__ void merge(Run &a, long long nb, double mean_b, double m2_b, double mn_b, double mx_b) {
  if (a.n == 0) {
    a.n = nb; a.mean = mean_b; a.m2 = m2_b; a.mn = mn_b; a.mx = mx_b;
    return;
  }
  const long long n = a.n + nb;
  const double delta = mean_b - a.mean;
  const double fb = (double)nb / (double)n;
  a.mean = a.mean + delta * fb;
  a.m2 = a.m2 + m2_b + delta * delta * ((double)a.n * fb);
  a.n = n;
  a.mn = mn_b < a.mn ? mn_b : a.mn;
  a.mx = mx_b > a.mx ? mx_b : a.mx;
}

// Lane j folds row j of the tile: the values of bin j of the columns whose bit j is set in their lane's mask, in lane order.
// The block's mean is formed around the first value (identical columns give it back exactly), the squared deviations in a
// second walk over the row.
__device__ __forceinline__ void fold_tile(const double *tile, unsigned long long *smask, unsigned long long mask, int lane, Run &run) {
  smask[lane] = mask;
  __syncthreads();
  long long n = 0;
  double ref = 0.0, s = 0.0, mn = 1.0e300, mx = -1.0e300;
  const double *row = tile + lane * kTileStride;
#pragma unroll 8
  for (int i = 0; i < 64; ++i) {
    const bool ok = (smask[i] >> lane) & 1ull;
    const double v = row[i];
    ref = (ok && n == 0) ? v : ref;
    s += ok ? v - ref : 0.0;
    mn = (ok && v < mn) ? v : mn;
    mx = (ok && v > mx) ? v : mx;
    n += ok ? 1 : 0;
  }
  if (n > 0) {
    const double mean = ref + s / (double)n;
    double m2 = 0.0;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const bool ok = (smask[i] >> lane) & 1ull;
      const double d = row[i] - mean;
      m2 += ok ? d * d : 0.0;
    }
    merge(run, n, mean, m2, mn, mx);
  }
  __syncthreads();
}

__device__ __forceinline__ int wave_max(int v) {
  for (int w = 32; w > 0; w >>= 1) { const int o = __shfl_xor(v, w); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
  for (int w = 32; w > 0; w >>= 1) { const int o = __shfl_xor(v, w); v = o < v ? o : v; }
  return v;
}

__device__ __forceinline__ double ld(const double *p) { return __builtin_nontemporal_load(p); }

// The value of the requested array in one layer row (`row` = the lane's element of array 0 of that layer) in two halves, so that a
// wave can request the rows of several layers before it waits for the first: row_request loads the stored value -- for the bulk
// salinity S_abs and m --, row_value forms a_k from them: S_abs / m where m is not zero (what samsim_get_state returns after a
// step), the stored S_bu in the rare lane with m = 0.
__device__ __forceinline__ void row_request(const double *row, int array, double &x, double &y) {
  const bool sbu = array == SAMSIM_A_S_BU;
  x = ld(row + (sbu ? (int)SAMSIM_A_S_ABS : array) * 64);
  y = sbu ? ld(row + SAMSIM_A_M * 64) : 1.0;
}
__device__ __forceinline__ double row_value(const double *row, int array, double x, double y) {
  if (array != SAMSIM_A_S_BU) return x;
  if (y != 0.0) return x / y;
  return ld(row + SAMSIM_A_S_BU * 64);
}

__device__ __forceinline__ void store_partials(ProfPartial *part, int lane, const Run &run) {
  ProfPartial p;
  p.mean = run.mean; p.m2 = run.m2; p.mn = run.mn; p.mx = run.mx; p.n = run.n;
  part[(size_t)blockIdx.x * DEV_PROF_BINS + lane] = p;
}

// the lane's column of block blk: its number of active layers, 0 for a column that stopped, lies beyond ncol or -- with a label row
// (samsim_get_group_profile_stats) -- carries another label than `group`: such a column behaves like a stopped one
__device__ __forceinline__ int active_layers(const int32_t *n_active, const int32_t *status, const int32_t *labels, int group, long long ncol,
                                             long long blk, int lane, int N) {
  const long long col = blk * 64 + lane;
  if (col >= ncol || status[col] != 0) return 0;
  if (labels && labels[col] != group) return 0;
  const int na = n_active[col];
  return na < 0 ? 0 : (na > N ? N : na);
}

// ---- layer axis: bin b holds layer b+1 (from the top) or layer N_active-b (from the bottom); bins [b0, b0+nb)
__global__ void __launch_bounds__(64) profile_layer_kernel(const double *__restrict__ lay, const int32_t *__restrict__ n_active,
                                                           const int32_t *__restrict__ status, const int32_t *__restrict__ labels,
                                                           int group, long long ncol, int N, int origin, int array, int b0, int nb,
                                                           ProfPartial *__restrict__ part) {
  __shared__ double tile[DEV_PROF_BINS * kTileStride];
  __shared__ unsigned long long smask[64];
  const int lane = threadIdx.x;
  const long long nblk = (ncol + 63) / 64;
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(n_active, status, labels, group, ncol, blk, lane, N);
    const int kmax = wave_max(na);
    const double *base = lay + DEV_LAY_INDEX(0, 0, blk * 64 + lane, N, ncol);   // the lane's element of array 0, layer 1
    unsigned long long mask = 0;
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
        if (k <= khi && k <= na && r >= 0 && r < nb) {
          tile[r * kTileStride + lane] = row_value(base + (size_t)(k - 1) * kRow, array, x[u], y[u]);
          mask |= 1ull << r;
        }
      }
    }
    fold_tile(tile, smask, mask, lane, run);
  }
  store_partials(part, lane, run);
}

// ---- depth axis: bin b is [z0 + b dz, z0 + (b+1) dz) below the ice surface (from the top) or above the ice bottom; a column's
// value in a bin is the overlap-weighted mean of its layers there (samsim.h); bins [b0, b0+nb)
__global__ void __launch_bounds__(64) profile_depth_kernel(const double *__restrict__ lay, const int32_t *__restrict__ n_active,
                                                           const int32_t *__restrict__ status, const int32_t *__restrict__ labels,
                                                           int group, long long ncol, int N, int origin, int array, int b0, int nb,
                                                           int lead, double z0, double dz, ProfPartial *__restrict__ part) {
  __shared__ double tile[DEV_PROF_BINS * kTileStride];
  __shared__ unsigned long long smask[64];
  const int lane = threadIdx.x;
  const long long nblk = (ncol + 63) / 64;
  const bool top = origin == SAMSIM_PROFILE_FROM_TOP;
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(n_active, status, labels, group, ncol, blk, lane, N);
    const int kmax = wave_max(na);
    const double *base = lay + DEV_LAY_INDEX(0, 0, blk * 64 + lane, N, ncol);   // the lane's element of array 0, layer 1
    double H = 0.0;
    if (!top) {   // the ice thickness first: Z_k = Z_{k-1} + thick(k), k ascending
#pragma unroll 4
      for (int k = 1; k <= kmax; ++k) {
        const double t = ld(base + (size_t)(k - 1) * kRow + SAMSIM_A_THICK * 64);
        H = k <= na ? H + t : H;
      }
    }
    unsigned long long mask = 0;
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
        // A chunk that does not begin where the walk begins (from the top: b0 > 0; from the bottom: not the last chunk): while no
        // column of the wave has reached the chunk the layers overlap none of its bins, so only Z moves on -- by the same
        // additions -- and the array rows are not requested.
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
          const double a = row_value(base + (size_t)(k - 1) * kRow, array, x[u], y[u]);
          const double Zn = Z + tk[u];
          const double lo = top ? Z : H - Zn, hi = top ? Zn : H - Z;
          while (cur >= b0 && cur < b0 + nb) {
            const double e0 = z0 + (double)cur * dz, e1 = z0 + (double)(cur + 1) * dz;
            const double xo = (hi < e1 ? hi : e1) - (lo > e0 ? lo : e0);
            const double o = xo > 0.0 ? xo : 0.0;
            L += o;
            W += o * a;
            if (!(top ? hi > e1 : lo < e0)) break;   // the layer ends inside this bin
            if (L > 0.0) {
              tile[(cur - b0) * kTileStride + lane] = W / L;
              mask |= 1ull << (cur - b0);
            }
            W = 0.0; L = 0.0;
            cur += step;
          }
          Z = Zn;
        }
      }
    }
    if (cur >= b0 && cur < b0 + nb && L > 0.0) {   // the bin in which the column ends
      tile[(cur - b0) * kTileStride + lane] = W / L;
      mask |= 1ull << (cur - b0);
    }
    fold_tile(tile, smask, mask, lane, run);
  }
  store_partials(part, lane, run);
}

// the waves' partials of one pass, combined in wave order; thread j writes bin b0 + j of the pass's array
__global__ void __launch_bounds__(64) profile_merge_kernel(const ProfPartial *__restrict__ part, int nwaves, int nb,
                                                           samsim_stat *__restrict__ out) {
  const int j = threadIdx.x;
  if (j >= nb) return;
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  for (int w = 0; w < nwaves; ++w) {
    const ProfPartial p = part[(size_t)w * DEV_PROF_BINS + j];
    if (p.n > 0) merge(run, p.n, p.mean, p.m2, p.mn, p.mx);
  }
  samsim_stat st;
  st.count = run.n;
  if (run.n > 0) {
    st.mean = run.mean; st.min = run.mn; st.max = run.mx;
    st.std = sqrt(run.m2 / (double)run.n);
  } else {
    st.mean = st.min = st.max = st.std = 0.0;
  }
  out[j] = st;
}

}  // namespace

// One pass: array `array`, bins [b0, b0 + nb) of the request's nbins with nb <= DEV_PROF_BINS, results to out[0 .. nb).  part holds DEV_PROF_GRID *
// DEV_PROF_BINS partials and is reused by the next pass on the same stream.  labels: null (every column counts), or the [ncol] label row
// of samsim_set_groups, of which only the columns with label `group` count.
extern "C" hipError_t samsim_launch_profile(const double *lay, const int32_t *n_active, const int32_t *status, const int32_t *labels,
                                            int group, long long ncol, int N, int axis, int origin, int array, int b0, int nb, int nbins,
                                            double z0, double dz, ProfPartial *part, samsim_stat *out, hipStream_t stream) {
  const long long nblk = (ncol + 63) / 64;
  const int grid = (int)(nblk < DEV_PROF_GRID ? nblk : DEV_PROF_GRID);
  if (axis == SAMSIM_PROFILE_BY_LAYER)
    hipLaunchKernelGGL(profile_layer_kernel, dim3(grid), dim3(64), 0, stream, lay, n_active, status, labels, group, ncol, N, origin, array, b0,
                       nb, part);
  else
    hipLaunchKernelGGL(profile_depth_kernel, dim3(grid), dim3(64), 0, stream, lay, n_active, status, labels, group, ncol, N, origin, array,
                       b0, nb, origin == SAMSIM_PROFILE_FROM_TOP ? b0 > 0 : b0 + nb < nbins, z0, dz, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(profile_merge_kernel, dim3(1), dim3(64), 0, stream, part, grid, nb, out);
  return hipGetLastError();
}
