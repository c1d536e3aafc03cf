// samsim_functionals.hip -- the evaluation kernel of the column functionals (samsim_set_functionals, include/samsim.h): per column
// a vertical integral, a mean, an extreme and its depth, the depth of the first layer that meets a condition, or the thickness of
// the layers that meet it, each over a depth window, written to one double[ncol] row per functional that every reduction reads as
// a slot (SAMSIM_FUNC_SLOT).
//
// One wave owns one 64-column block (lane = column) and serves every functional of the handle.  The column's status, n_active and
// flags are read once.  The layers are walked once per group of functionals (samsim_functionals.h; one group in the common case),
// up to the wave's largest n_active, over 512-byte rows of the device layout [block][layer][array][64]: thick and the group's
// distinct rows only, the rows of kAhead layers requested with non-temporal loads before the first is waited for.  A thick-only
// pre-pass forms H when some functional counts from the bottom.  Every lane then applies the definition of samsim.h to its own
// column: a fixed sequence of IEEE operations on the column's own data in ascending k, no LDS, no cross-lane arithmetic beyond the
// wave maximum of n_active, no atomics, plain division, products rounded before they are added (the Makefile's -ffp-contract=off,
// and the pragma below for a build that drops it).  Each lane ends with one 8-byte store per functional; nothing else is written.
//
// The layer value is what samsim_get_state would return (samsim_column_read.h), formed in registers.  Every offset into the rows is
// 64-bit.
#include <hip/hip_runtime.h>

#include "samsim_functionals.h"

#pragma clang fp contract(off)

namespace {

using namespace column_read;

constexpr int kAhead = 4;                            // layers whose rows a wave requests before it waits for the first
constexpr int kRows = ROW_PLAN_ROWS;

// the running result of one functional in one lane
struct Acc {
  double r0 = 0.0;   // W, the extreme, or the thickness
  double r1 = 0.0;   // L, or the depth
  bool found = false;
};

// layer k of the lane's column, [Z, Zn) below the surface, against functional q; x0..x3 the loaded rows of q's group, row = the
// lane's element of array 0 of that layer
__device__ __forceinline__ void update(const FuncDev &q, Acc &s, double Z, double Zn, double H, double x0, double x1, double x2, double x3,
                                       const double *row, bool adjust, bool clamp) {
  const bool top = q.origin == SAMSIM_PROFILE_FROM_TOP;
  const double lo = top ? Z : H - Zn, hi = top ? Zn : H - Z;
  const double e1 = hi < q.z_hi ? hi : q.z_hi, e0 = lo > q.z_lo ? lo : q.z_lo;
  const double xo = e1 - e0;
  if (!(xo > 0.0)) return;   // the layer is not in the window
  const double o = xo;
  const double a = row_value(q.mode, q.ia, q.ib, x0, x1, x2, x3, row, adjust, clamp);
  const bool cond = q.sense > 0 ? a >= q.threshold : (q.sense < 0 ? a < q.threshold : false);
  switch (q.kind) {
    case SAMSIM_FN_INTEGRAL: case SAMSIM_FN_MEAN: {
      const double prod = o * a;
      s.r0 = s.r0 + prod;
      s.r1 = s.r1 + o;
      s.found = true;
      break;
    }
    case SAMSIM_FN_MIN: case SAMSIM_FN_DEPTH_OF_MIN:
      if (s.found ? a < s.r0 : a == a) { s.r0 = a; s.r1 = 0.5 * (lo + hi); s.found = true; }
      break;
    case SAMSIM_FN_MAX: case SAMSIM_FN_DEPTH_OF_MAX:
      if (s.found ? a > s.r0 : a == a) { s.r0 = a; s.r1 = 0.5 * (lo + hi); s.found = true; }
      break;
    case SAMSIM_FN_CROSSING_DEPTH:
      // the first such layer counted from the origin: the smallest k from the top (kept), the largest from the bottom (overwritten)
      if (cond && !(top && s.found)) { s.r1 = e0; s.found = true; }
      break;
    default:   // SAMSIM_FN_THICKNESS_WHERE
      if (cond) s.r0 = s.r0 + o;
  }
}

__device__ __forceinline__ double result(const FuncDev &q, const Acc &s) {
  switch (q.kind) {
    case SAMSIM_FN_INTEGRAL: case SAMSIM_FN_THICKNESS_WHERE: return s.r0;
    case SAMSIM_FN_MEAN: return s.found ? s.r0 / s.r1 : q.missing;
    case SAMSIM_FN_MIN: case SAMSIM_FN_MAX: return s.found ? s.r0 : q.missing;
    default: return s.found ? s.r1 : q.missing;   // DEPTH_OF_MIN, DEPTH_OF_MAX, CROSSING_DEPTH
  }
}

__global__ void __launch_bounds__(64) functionals_kernel(const FuncParams p) {
  const int lane = threadIdx.x;
  const long long blk = (long long)blockIdx.x;
  const long long col = blk * 64 + lane;
  const bool in = col < p.ncol;
  const size_t nc = (size_t)p.ncol, c = (size_t)col;
  Column cl{};
  if (in) cl = column(p.n_active, p.status, p.flags, c, p.N, p.stepped != 0);
  const int na = cl.na;
  const bool adjust = cl.adjust, clamp = cl.clamp;
  const int kmax = wave_max(na);
  // the lane's element of array 0, layer 1; the block is allocated whole, so the lanes beyond ncol read their own (zero) rows
  const double *base = p.lay + DEV_LAY_INDEX(0, 0, (size_t)blk * 64 + lane, p.N, nc);

  const double H = p.need_H ? ice_thickness(base, na, kmax) : 0.0;

  Acc acc[SAMSIM_MAX_FUNCTIONALS];
  for (int g = 0; g < p.plan.ngroups; ++g) {
    const int gn = p.plan.gn[g];
    const int o0 = p.plan.grow[g][0] * 64, o1 = p.plan.grow[g][1] * 64, o2 = p.plan.grow[g][2] * 64, o3 = p.plan.grow[g][3] * 64;
    double Z = 0.0;
    for (int k0 = 1; k0 <= kmax; k0 += kAhead) {   // the rows of kAhead layers requested together
      double tk[kAhead], x[kRows][kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        tk[u] = x[0][u] = x[1][u] = x[2][u] = x[3][u] = 0.0;
        if (k0 + u <= kmax) {
          const double *row = base + (size_t)(k0 + u - 1) * kRow;
          tk[u] = ld(row + SAMSIM_A_THICK * 64);
          if (gn > 0) x[0][u] = ld(row + o0);
          if (gn > 1) x[1][u] = ld(row + o1);
          if (gn > 2) x[2][u] = ld(row + o2);
          if (gn > 3) x[3][u] = ld(row + o3);
        }
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        if (k0 + u <= na) {   // sequential double additions, k ascending
          const double Zn = Z + tk[u];
          const double *row = base + (size_t)(k0 + u - 1) * kRow;
#pragma unroll
          for (int f = 0; f < SAMSIM_MAX_FUNCTIONALS; ++f)
            if (f < p.nf && p.f[f].group == g) update(p.f[f], acc[f], Z, Zn, H, x[0][u], x[1][u], x[2][u], x[3][u], row, adjust, clamp);
          Z = Zn;
        }
      }
    }
  }

  if (!in) return;
#pragma unroll
  for (int f = 0; f < SAMSIM_MAX_FUNCTIONALS; ++f)
    if (f < p.nf) p.rows[(size_t)f * nc + c] = result(p.f[f], acc[f]);
}

}  // namespace

extern "C" hipError_t samsim_launch_functionals(const FuncParams *p, hipStream_t stream) {
  const long long nblk = (p->ncol + 63) / 64;
  if (nblk <= 0 || p->nf <= 0) return hipSuccess;
  hipLaunchKernelGGL(functionals_kernel, dim3((unsigned)nblk), dim3(64), 0, stream, *p);
  return hipGetLastError();
}
