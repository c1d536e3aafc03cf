// samsim_tracks.hip -- the sampling kernel of the time-domain diagnostics (samsim_set_tracks, include/samsim.h).
//
// launch() of samsim_capi.cpp enqueues one sample directly behind the step launch that brings clock.step to a multiple of `every`,
// on that launch's stream and for its block range.  One wave owns one 64-column block (lane = column) and serves every track of
// the handle: the column's status, n_active and flags are read once, the scalars of the SCALAR tracks once, and the layers are
// walked at most once -- up to the wave's largest n_active, 512-byte rows of the device layout [block][layer][array][64] -- and only
// when a track needs a column sum: thick for ICE_THICKNESS, S_abs and m for BULK_SALINITY.  A LAYER track costs one load per lane
// after the walk, from the lane's own layer (the wave's row for a layer counted from the top; for one counted from the bottom the
// lanes' rows differ where their n_active do).  Then every lane applies the update rule of samsim.h to its own eleven fields per
// track: a fixed sequence of IEEE operations on the column's own data, no cross-lane arithmetic, no atomics, plain division, and
// no contraction of d * (x - MEAN) + M2 into a fused multiply-add (the Makefile's -ffp-contract=off, and the pragma below for a
// build that drops it).  A column that stopped, or a LAYER track whose layer the column does not have, is left alone.
//
// The observable is formed from what samsim_get_state would return (samsim_column_read.h); the sampler only runs behind a step, so
// it reads its columns as stepped.
// Every offset into the track rows is 64-bit: ntracks * SAMSIM_NTF * ncol * 8 bytes pass 4 GiB from 6.1 million columns on.
#include <hip/hip_runtime.h>

#include "samsim_column_read.h"
#include "samsim_tracks.h"

#pragma clang fp contract(off)

namespace {

using namespace column_read;

constexpr int kAhead = 8;                            // layers whose rows a wave requests before it waits for the first

// the value of array `a` in the layer row `row` (the lane's element of array 0 of that layer) of a column that runs, with plain loads
__device__ __forceinline__ double layer_value(const double *row, int a, bool clamp) {
  if (a == SAMSIM_A_S_BU)
    return s_bu_value(row[SAMSIM_A_S_ABS * 64], row[SAMSIM_A_M * 64], true, clamp, [&] { return row[SAMSIM_A_S_BU * 64]; });
  const double v = row[a * 64];
  return a == SAMSIM_A_S_ABS ? s_abs_value(v, clamp) : v;
}

__global__ void __launch_bounds__(64) track_sample_kernel(const TrackParams p) {
  const int lane = threadIdx.x;
  const long long blk = p.block0 + (long long)blockIdx.x;
  const long long col = blk * 64 + lane;
  const bool live = col < p.ncol && p.status[col] == 0;
  if (!__any(live)) return;
  const size_t nc = (size_t)p.ncol, c = (size_t)col;
  Column cl{};
  if (live) cl = column(p.n_active, p.status, p.flags, c, p.N, true);   // stepped: the sample follows a step launch
  const int na_raw = cl.na_raw, na = cl.na;
  const bool clamp = cl.clamp;
  const double *base = p.lay + DEV_LAY_INDEX(0, 0, (size_t)blk * 64 + lane, p.N, nc);   // the lane's element of array 0, layer 1

  // ---- the column sums: one walk over the layers, only the rows a track needs
  double Z = 0.0, ssum = 0.0, msum = 0.0;
  if (p.need_thick || p.need_salt) {
    const int kmax = wave_max(na);
    for (int k0 = 1; k0 <= kmax; k0 += kAhead) {   // the rows of kAhead layers requested together
      double tk[kAhead], sa[kAhead], mm[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        tk[u] = sa[u] = mm[u] = 0.0;
        if (k0 + u <= kmax) {
          const double *row = base + (size_t)(k0 + u - 1) * kRow;
          if (p.need_thick) tk[u] = row[SAMSIM_A_THICK * 64];
          if (p.need_salt) { sa[u] = row[SAMSIM_A_S_ABS * 64]; mm[u] = row[SAMSIM_A_M * 64]; }
        }
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        if (k0 + u <= na) {   // sequential double additions, k ascending
          Z = Z + tk[u];
          ssum = ssum + s_abs_value(sa[u], clamp);
          msum = msum + mm[u];
        }
      }
    }
  }

  // ---- per track: the observable, then the update of the lane's own eleven fields
#pragma unroll
  for (int t = 0; t < SAMSIM_MAX_TRACKS; ++t) {
    if (t >= p.ntracks) break;
    const TrackDev &tr = p.t[t];
    bool has = live;
    double x = 0.0;
    switch (tr.kind) {
      case SAMSIM_OBS_SCALAR: if (has) x = p.scal[(size_t)tr.id * nc + c]; break;
      case SAMSIM_OBS_N_ACTIVE: x = (double)na_raw; break;
      case SAMSIM_OBS_ICE_THICKNESS: x = Z; break;
      case SAMSIM_OBS_BULK_SALINITY: x = ssum / msum; break;
      default: {   // SAMSIM_OBS_LAYER
        const int k = tr.layer > 0 ? tr.layer : na + 1 + tr.layer;
        has = has && k >= 1 && k <= na;   // a layer the column does not have: not sampled
        if (has) x = layer_value(base + (size_t)(k - 1) * kRow, tr.id, clamp);
      }
    }
    if (!has) continue;
    double *f = p.rows + (size_t)t * SAMSIM_NTF * nc + c;   // field i of the lane's column: f[i * nc]
    const double n = f[SAMSIM_TF_N * nc] + 1.0;
    const double mean0 = f[SAMSIM_TF_MEAN * nc], m20 = f[SAMSIM_TF_M2 * nc];
    const double mn = f[SAMSIM_TF_MIN * nc], mx = f[SAMSIM_TF_MAX * nc];
    const double d = x - mean0;
    const double q = d / n;
    const double mean = mean0 + q;
    const double e = x - mean;
    const double prod = d * e;
    f[SAMSIM_TF_N * nc] = n;
    f[SAMSIM_TF_LAST * nc] = x;
    f[SAMSIM_TF_MEAN * nc] = mean;
    f[SAMSIM_TF_M2 * nc] = m20 + prod;
    if (x < mn) { f[SAMSIM_TF_MIN * nc] = x; f[SAMSIM_TF_STEP_MIN * nc] = p.step; }
    if (x > mx) { f[SAMSIM_TF_MAX * nc] = x; f[SAMSIM_TF_STEP_MAX * nc] = p.step; }
    const bool hold = tr.sense > 0 ? x >= tr.threshold : (tr.sense < 0 ? x < tr.threshold : false);
    if (hold) {
      f[SAMSIM_TF_N_HOLD * nc] = f[SAMSIM_TF_N_HOLD * nc] + 1.0;
      if (f[SAMSIM_TF_STEP_FIRST * nc] < 0.0) f[SAMSIM_TF_STEP_FIRST * nc] = p.step;
      f[SAMSIM_TF_STEP_LAST * nc] = p.step;
    }
  }
}

}  // namespace

extern "C" hipError_t samsim_launch_track_sample(const TrackParams *p, long long nblocks, hipStream_t stream) {
  if (nblocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(track_sample_kernel, dim3((unsigned)nblocks), dim3(64), 0, stream, *p);
  return hipGetLastError();
}
