// samsim_sensors.hip -- the observation operator and the per-column misfit (samsim_set_sensors, samsim_get_sensor_values,
// samsim_score, include/samsim.h): per column the model's equivalent of each sensor of a thermistor string, a salinity core or a
// mass-balance buoy, and one weighted sum of squared differences against an observation vector, accumulated over the calls in nine
// double[ncol] rows that every reduction reads as a slot (SAMSIM_SCORE_SLOT).
//
// One wave owns 64 columns (lane = column; for samsim_get_sensor_values lane = list position, each lane at its own column's rows)
// and serves every sensor of the handle.  Status, flags and n_active are read once.  The layers are walked once per group of profile
// sensors (samsim_sensors.h; one group for a string and a core), up to the wave's largest n_active or until no lane has a sensor of
// the group left, over 512-byte rows of the device layout [block][layer][array][64]: thick and the group's distinct rows only, the
// rows of kAhead layers requested with non-temporal loads before the first is waited for.  A thick-only pre-pass forms H when a
// sensor needs it.  Inside a chunk of kAhead layers the sensors are a wave-uniform loop over the parameters, each sensor taking the
// chunk's layers in ascending k with its parameters read once (the sensors do not depend on each other); a lane resolves a sensor
// in the layer that contains it, or, for a LINEAR sensor whose neighbour is the following layer, one layer later -- the boundaries
// and row values of the layer before the chunk stay in registers, and two 32-bit lane masks say which sensors are in the ice and
// which are pending.
//
// Where the values live: 32 doubles per lane do not fit in registers beside the walk's 4 x 5 requested values and the previous
// layer's, and resolving the sensors in register chunks of eight would walk the layers four times for a 32-sensor string.  They are
// kept in an LDS tile [sensor][lane], 512 bytes per sensor in force and 16 KiB per wave at the most: each lane touches only its own
// column of the tile, so no barrier is needed, and a row of the tile is 64 consecutive doubles, which ds_read_b64 / ds_write_b64
// serve without a bank conflict.  A full tile leaves ten waves per CU, an 18-sensor one the sixteen that the kernel's 108
// VGPRs allow; there is no scratch.
//
// Every value is a fixed sequence of IEEE operations on the column's own data: no cross-lane arithmetic beyond the wave maximum of
// n_active and the votes that skip work, no atomics, plain division, products rounded before they are added (the Makefile's
// -ffp-contract=off, and the pragma below for a build that drops it).  The layer value is what samsim_get_state would return
// (samsim_column_read.h), formed in registers.  Every offset into the rows is 64-bit.
#include <hip/hip_runtime.h>

#include "samsim_sensors.h"

#pragma clang fp contract(off)

namespace {

using namespace column_read;

constexpr int kAhead = 4;                            // layers whose rows a wave requests before it waits for the first
constexpr int kRows = ROW_PLAN_ROWS;

// between the midpoints of two adjacent layers, (cl, al) of the one with the smaller k and (cu, au) of the other: from the top the
// smaller k has the smaller coordinate, from the bottom the larger
__device__ __forceinline__ double between(bool top, double z, double cl, double al, double cu, double au) {
  const double ca = top ? cl : cu, aa = top ? al : au, cb = top ? cu : cl, ab = top ? au : al;
  const double t = (z - ca) / (cb - ca);
  const double prod = t * (ab - aa);
  return aa + prod;
}

template <bool LIST>
__global__ void __launch_bounds__(64) sensors_kernel(const SensorParams p) {
  extern __shared__ double y_tile[];                 // the lane's sensor values, [sensor][lane]: 512 bytes per sensor in force
  double *y = y_tile + threadIdx.x;
  const int lane = threadIdx.x;
  const long long pos = (long long)blockIdx.x * 64 + lane;
  const bool in = pos < (LIST ? p.npos : p.ncol);
  // a lane beyond the list reads column 0; a lane beyond ncol its own (zero) rows, as the block is allocated whole
  const long long col = LIST ? (in ? p.cols[pos] : 0) : pos;
  const size_t nc = (size_t)p.ncol, c = (size_t)col;
  Column cl{};
  bool scored = false;
  if (in) {
    cl = column(p.n_active, p.status, p.flags, c, p.N, p.stepped != 0);
    if (!LIST) {   // a column that is not scored takes no part in the walk and writes nothing
      scored = p.status[c] == 0 && (p.labels == nullptr || p.labels[c] == p.group);
      if (!scored) cl.na = 0;
    }
  }
  const int na = cl.na;
  const bool adjust = cl.adjust, clamp = cl.clamp;
  const int kmax = wave_max(na);
  const double *base = p.lay + DEV_LAY_INDEX(0, 0, c, p.N, nc);   // the lane's element of array 0, layer 1

  const double H = p.need_H ? ice_thickness(base, na, kmax) : 0.0;

  // bit i of `found`: sensor i is in the ice; of `pend`: its value waits for the following layer
  uint32_t found = 0, pend = 0;
  for (int i = 0; i < p.ns; ++i) {
    const SensorDev &q = p.s[i];
    double v = q.missing;
    if (q.kind != SAMSIM_SENSOR_PROFILE) {
      found |= 1u << i;
      v = q.kind == SAMSIM_SENSOR_ICE_THICKNESS ? H : (in ? p.scal[(size_t)q.id * nc + c] : 0.0);
    }
    y[i * 64] = v;
  }

  for (int g = 0; g < p.plan.ngroups; ++g) {
    const int gn = p.plan.gn[g];
    const int o0 = p.plan.grow[g][0] * 64, o1 = p.plan.grow[g][1] * 64, o2 = p.plan.grow[g][2] * 64, o3 = p.plan.grow[g][3] * 64;
    uint32_t gmask = 0;   // the sensors of this walk (wave-uniform)
    for (int i = 0; i < p.ns; ++i)
      if (p.s[i].group == g) gmask |= 1u << i;
    // the layer boundaries around the chunk and the rows of the layer before it: e[j] = Z_{k0 - 2 + j} for the top origin, H - that for
    // the bottom; xx[r][j] the group's row r in layer k0 - 1 + j
    double Zm = 0.0, Z = 0.0;
    double px0 = 0.0, px1 = 0.0, px2 = 0.0, px3 = 0.0;
    for (int k0 = 1; k0 <= kmax; k0 += kAhead) {   // the rows of kAhead layers requested together
      if (!__any(k0 <= na && ((~found | pend) & gmask) != 0)) break;   // no lane has a sensor of the group left
      double tk[kAhead], xx[kRows][kAhead + 1];
      xx[0][0] = px0; xx[1][0] = px1; xx[2][0] = px2; xx[3][0] = px3;
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        tk[u] = xx[0][u + 1] = xx[1][u + 1] = xx[2][u + 1] = xx[3][u + 1] = 0.0;
        if (k0 + u <= kmax) {
          const double *row = base + (size_t)(k0 + u - 1) * kRow;
          tk[u] = ld(row + SAMSIM_A_THICK * 64);
          if (gn > 0) xx[0][u + 1] = ld(row + o0);
          if (gn > 1) xx[1][u + 1] = ld(row + o1);
          if (gn > 2) xx[2][u + 1] = ld(row + o2);
          if (gn > 3) xx[3][u + 1] = ld(row + o3);
        }
      }
      double et[kAhead + 2], eb[kAhead + 2];
      et[0] = Zm; et[1] = Z;
#pragma unroll
      for (int u = 0; u < kAhead; ++u) et[u + 2] = k0 + u <= na ? et[u + 1] + tk[u] : et[u + 1];   // sequential double additions, k ascending
#pragma unroll
      for (int j = 0; j < kAhead + 2; ++j) eb[j] = H - et[j];
      const double *row0 = base + (size_t)(k0 - 1) * kRow;
      // the sensors are independent of each other: each takes the chunk's layers in ascending k with its parameters loaded once
      for (int i = 0; i < p.ns; ++i) {
        const uint32_t bit = 1u << i;
        if (!(gmask & bit)) continue;
        if (!__any(k0 <= na && ((pend | ~found) & bit) != 0)) continue;
        const SensorDev &q = p.s[i];
        const bool top = q.origin == SAMSIM_PROFILE_FROM_TOP;
        const double z = q.z;
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          const int k = k0 + u;
          if (k > na || ((pend | ~found) & bit) == 0) continue;
          // layer k covers [lo, hi), layer k - 1 [plo, phi)
          const double lo = top ? et[u + 1] : eb[u + 2], hi = top ? et[u + 2] : eb[u + 1];
          const double *row = row0 + (size_t)u * kRow;
          if (pend & bit) {   // found in layer k - 1, the neighbour is this one
            const double plo = top ? et[u] : eb[u + 1], phi = top ? et[u + 1] : eb[u];
            const double al = row_value(q.mode, q.ia, q.ib, xx[0][u], xx[1][u], xx[2][u], xx[3][u], row - kRow, adjust, clamp);
            const double au = row_value(q.mode, q.ia, q.ib, xx[0][u + 1], xx[1][u + 1], xx[2][u + 1], xx[3][u + 1], row, adjust, clamp);
            y[i * 64] = between(top, z, 0.5 * (plo + phi), al, 0.5 * (lo + hi), au);
            pend &= ~bit;
          } else if (lo <= z && z < hi) {   // not found yet, and this is the smallest such k: a sensor is resolved once
            found |= bit;
            const double ak = row_value(q.mode, q.ia, q.ib, xx[0][u + 1], xx[1][u + 1], xx[2][u + 1], xx[3][u + 1], row, adjust, clamp);
            double v = ak;
            if (q.interp == SAMSIM_SENSOR_LINEAR) {
              const double ck = 0.5 * (lo + hi);
              const bool next = top ? z >= ck : !(z >= ck);   // the neighbour on the side of z is layer k + 1
              if (next) {
                if (k < na) pend |= bit;
              } else if (k > 1) {
                const double plo = top ? et[u] : eb[u + 1], phi = top ? et[u + 1] : eb[u];
                const double al = row_value(q.mode, q.ia, q.ib, xx[0][u], xx[1][u], xx[2][u], xx[3][u], row - kRow, adjust, clamp);
                v = between(top, z, 0.5 * (plo + phi), al, ck, ak);
              }
            }
            y[i * 64] = v;
          }
        }
      }
      Zm = et[kAhead]; Z = et[kAhead + 1];
      px0 = xx[0][kAhead]; px1 = xx[1][kAhead]; px2 = xx[2][kAhead]; px3 = xx[3][kAhead];
    }
  }

  if (LIST) {
    if (!in) return;
    for (int i = 0; i < p.ns; ++i) p.out[(size_t)i * (size_t)p.npos + (size_t)pos] = y[i * 64];
    return;
  }
  if (!scored) return;
  double n = 0.0, j = 0.0, b = 0.0, w = 0.0;
  for (int i = 0; i < p.ns; ++i) {   // the valid sensors in ascending i
    if (!((p.obs_mask & found) >> i & 1u)) continue;
    const double d = y[i * 64] - p.obs[i];
    const double wi = p.weight[i];
    const double dd = d * d;
    const double wdd = wi * dd, wd = wi * d;
    n = n + 1.0;
    j = j + wdd;
    b = b + wd;
    w = w + wi;
  }
  double *r = p.out + c;
  r[(size_t)SAMSIM_SF_N_LAST * nc] = n;
  r[(size_t)SAMSIM_SF_J_LAST * nc] = j;
  r[(size_t)SAMSIM_SF_B_LAST * nc] = b;
  r[(size_t)SAMSIM_SF_W_LAST * nc] = w;
  if (n > 0.0) {
    r[(size_t)SAMSIM_SF_N_SUM * nc] = r[(size_t)SAMSIM_SF_N_SUM * nc] + n;
    r[(size_t)SAMSIM_SF_J_SUM * nc] = r[(size_t)SAMSIM_SF_J_SUM * nc] + j;
    r[(size_t)SAMSIM_SF_B_SUM * nc] = r[(size_t)SAMSIM_SF_B_SUM * nc] + b;
    r[(size_t)SAMSIM_SF_W_SUM * nc] = r[(size_t)SAMSIM_SF_W_SUM * nc] + w;
    r[(size_t)SAMSIM_SF_CALLS * nc] = r[(size_t)SAMSIM_SF_CALLS * nc] + 1.0;
  }
}

}  // namespace

extern "C" hipError_t samsim_launch_score(const SensorParams *p, hipStream_t stream) {
  const long long nblk = (p->ncol + 63) / 64;
  if (nblk <= 0 || p->ns <= 0) return hipSuccess;
  hipLaunchKernelGGL(sensors_kernel<false>, dim3((unsigned)nblk), dim3(64), (size_t)p->ns * 512, stream, *p);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_sensor_values(const SensorParams *p, hipStream_t stream) {
  const long long nblk = (p->npos + 63) / 64;
  if (nblk <= 0 || p->ns <= 0) return hipSuccess;
  hipLaunchKernelGGL(sensors_kernel<true>, dim3((unsigned)nblk), dim3(64), (size_t)p->ns * 512, stream, *p);
  return hipGetLastError();
}
