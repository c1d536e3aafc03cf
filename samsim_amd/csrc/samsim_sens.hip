// samsim_sens.hip -- device-side ensemble sensitivities (samsim_get_covariance, samsim_get_profile_regression, include/samsim.h):
// joint second moments of the per-column scalars, and per depth bin the joint moments of a layer profile and one per-column
// predictor.
//
// Scalars: the walk and the bracket of samsim_slot_walk.h.  Every lane applies Welford's update to its own running moments of the
// nslots rows (a template on nslots); the lanes and then the waves are combined with Chan's pairwise update.
//
// Profiles: a pass of samsim_profile.h, whose walk (samsim_profile_walk.h) fills the LDS tile [bin][lane]; the block's 64
// predictor values lie beside it, and lane j folds row j with the statistics' own fold and merge (samsim_profile_fold.h) with the
// predictor riding along.
//
// No atomics of any kind, no floating-point sum whose order depends on scheduling: two calls return the same bytes.
#include <hip/hip_runtime.h>

#include "samsim_profile_fold.h"
#include "samsim_profile_walk.h"
#include "samsim_sens.h"

namespace {

using namespace profile_walk;
using namespace profile_fold;
using namespace slot_walk;

// ---------------------------------------------------------------------------------------------------------------- scalars

// Running moments of one pair of slots (i, j): n columns, the two means, the sum of products of deviations.  Every update is
// symmetric in i and j down to the bits (dx * dy == dy * dx), so a slot listed twice gives the bytes of its variance.
struct PairAcc {
  long long n;
  double mi, mj, c;
  // Chan et al. for a co-moment; b is not empty
  __device__ __forceinline__ void add(long long nb, double mi_b, double mj_b, double c_b) {
    if (n == 0) {
      n = nb; mi = mi_b; mj = mj_b; c = c_b;
      return;
    }
    const long long nn = n + nb;
    const double di = mi_b - mi, dj = mj_b - mj;
    const double fb = (double)nb / (double)nn;
    const double w = (double)n * fb;
    mi = mi + di * fb;
    mj = mj + dj * fb;
    c = c + c_b + di * dj * w;
    n = nn;
  }
  __device__ __forceinline__ void absorb(const PairAcc &b) {
    if (b.n > 0) add(b.n, b.mi, b.mj, b.c);
  }
};

// Every lane keeps its own running n, NS means and NS (NS + 1) / 2 co-moments in registers (every index is a compile-time one);
// at the end the 64 lanes in lane order through LDS, one thread per pair of slots, and the wave's partial is stored.
template <int NS>
__global__ void __launch_bounds__(64) cov_kernel(SensRows rows, ColSet cs, double *__restrict__ part) {
  constexpr int NP = NS * (NS + 1) / 2;
  __shared__ double s[(1 + NS + NP) * kLaneStride];   // [n, means, co-moments][lane]
  const int lane = threadIdx.x;
  long long n = 0;
  double mean[NS], C[NP];
#pragma unroll
  for (int i = 0; i < NS; ++i) mean[i] = 0.0;
#pragma unroll
  for (int p = 0; p < NP; ++p) C[p] = 0.0;
  walk_blocks<Cols<NS>>(
      cs.ncol, lane, [&](long long blk, int ln, Cols<NS> &c) { load_cols<NS>(cs, rows.row, nullptr, blk, ln, c); },
      [&](long long, const Cols<NS> &c) {
        if (!c.ok) return;
        // Welford: the first value of a lane is its mean exactly (0 + v / 1), equal values leave the means and the co-moments
        // alone (every d is 0).  The co-moment takes d_i * d_j * (n - 1) / n, the form of the update that is symmetric in i and j.
        n += 1;
        const double dn = (double)n, f = (double)(n - 1) / dn;
        double d[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          d[i] = c.v[i] - mean[i];
          mean[i] = mean[i] + d[i] / dn;
        }
        int p = 0;
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
          for (int j = i; j < NS; ++j, ++p) C[p] = C[p] + d[i] * d[j] * f;
      });
  s[lane] = (double)n;
#pragma unroll
  for (int i = 0; i < NS; ++i) s[(1 + i) * kLaneStride + lane] = mean[i];
#pragma unroll
  for (int p = 0; p < NP; ++p) s[(1 + NS + p) * kLaneStride + lane] = C[p];
  __syncthreads();
  if (lane >= NP) return;
  int i, j;
  pair_of(lane, NS, i, j);
  PairAcc acc{0, 0.0, 0.0, 0.0};
  absorb_lanes(acc, [&](int l) {
    return PairAcc{(long long)s[l], s[(1 + i) * kLaneStride + l], s[(1 + j) * kLaneStride + l], s[(1 + NS + lane) * kLaneStride + l]};
  });
  double *mine = part + (size_t)blockIdx.x * DEV_COV_PART;
  mine[DEV_COV_C0 + lane] = acc.c;
  if (i == j) mine[DEV_COV_MEAN0 + i] = acc.mi;
  if (lane == 0) mine[0] = (double)acc.n;
}

// One workgroup per pair of slots: the waves' partials in wave order.  The pair (i, j) goes to cov[i][j] and cov[j][i]: one
// value, stored twice.
__global__ void __launch_bounds__(64) cov_merge_kernel(const double *__restrict__ part, int nwaves, int ns, CovResult *__restrict__ out) {
  __shared__ PairAcc s_acc[64];
  const int p = blockIdx.x;
  int i, j;
  pair_of(p, ns, i, j);
  PairAcc acc{0, 0.0, 0.0, 0.0};
  const bool last = merge_waves(nwaves, acc, s_acc, threadIdx.x, [&](int w) {
    const double *q = part + (size_t)w * DEV_COV_PART;
    return PairAcc{(long long)q[0], q[DEV_COV_MEAN0 + i], q[DEV_COV_MEAN0 + j], q[DEV_COV_C0 + p]};
  });
  if (!last) return;
  const double cov = acc.n > 0 ? acc.c / (double)acc.n : 0.0;
  out->cov[i * ns + j] = cov;
  out->cov[j * ns + i] = cov;
  if (i == j) out->mean[i] = acc.n > 0 ? acc.mi : 0.0;
  if (p == 0) out->count = acc.n;
}

// --------------------------------------------------------------------------------------------------------------- profiles

// the lane's predictor value of block blk (0.0 beyond ncol: such a lane's mask is empty)
__device__ __forceinline__ double predictor(const double *x, const int32_t *n_active, long long ncol, long long blk, int lane) {
  const long long col = blk * 64 + lane;
  if (col >= ncol) return 0.0;
  return x ? x[col] : (double)n_active[col];
}

__device__ __forceinline__ void store_partials(SensProfPartial *part, int lane, const Run &run, const Co &co) {
  SensProfPartial p;
  p.mean_y = run.mean; p.m2_y = run.m2; p.mean_x = co.mean_x; p.m2_x = co.m2_x; p.cxy = co.cxy; p.n = run.n;
  part[(size_t)blockIdx.x * DEV_PROF_BINS + lane] = p;
}

// The layer / depth pair as it was before the pass descriptor: sens_profile_kernel<AXIS>(ProfPass, ...) measured 2.3 % slower on
// the depth axis (docs/HISTORY.md, "Profile reductions: one pass descriptor"), so this family keeps its two kernels.
// ---- layer axis (profile_walk::layer_block): bins [b0, b0+nb)
__global__ void __launch_bounds__(64) sens_layer_kernel(const double *__restrict__ lay, const double *__restrict__ x,
                                                        const int32_t *__restrict__ n_active, const int32_t *__restrict__ status,
                                                        const int32_t *__restrict__ labels, int group, long long ncol, int N, int origin,
                                                        int array, int b0, int nb, SensProfPartial *__restrict__ part) {
  __shared__ double tile[DEV_PROF_BINS * kTileStride];
  __shared__ unsigned long long smask[64];
  __shared__ double xs[64];   // the block's predictor values, lane by lane
  const int lane = threadIdx.x;
  const long long nblk = col_blocks(ncol);
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  Co co{0.0, 0.0, 0.0};
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(n_active, status, labels, group, ncol, blk, lane, N);
    const double xv = predictor(x, n_active, ncol, blk, lane);   // requested before the walk, needed after it
    TileSink sink{tile, lane, 0};
    layer_block(lay, ncol, N, blk, lane, na, origin, array, b0, nb, sink);
    xs[lane] = xv;
    fold_tile<true>(tile, xs, smask, sink.mask, lane, run, co);
  }
  store_partials(part, lane, run, co);
}

// ---- depth axis (profile_walk::depth_block): bins [b0, b0+nb)
__global__ void __launch_bounds__(64) sens_depth_kernel(const double *__restrict__ lay, const double *__restrict__ x,
                                                        const int32_t *__restrict__ n_active, const int32_t *__restrict__ status,
                                                        const int32_t *__restrict__ labels, int group, long long ncol, int N, int origin,
                                                        int array, int b0, int nb, int lead, double z0, double dz,
                                                        SensProfPartial *__restrict__ part) {
  __shared__ double tile[DEV_PROF_BINS * kTileStride];
  __shared__ unsigned long long smask[64];
  __shared__ double xs[64];
  const int lane = threadIdx.x;
  const long long nblk = col_blocks(ncol);
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  Co co{0.0, 0.0, 0.0};
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int na = active_layers(n_active, status, labels, group, ncol, blk, lane, N);
    const double xv = predictor(x, n_active, ncol, blk, lane);
    TileSink sink{tile, lane, 0};
    depth_block(lay, ncol, N, blk, lane, na, origin, array, b0, nb, lead, z0, dz, sink);
    xs[lane] = xv;
    fold_tile<true>(tile, xs, smask, sink.mask, lane, run, co);
  }
  store_partials(part, lane, run, co);
}

// the waves' partials of one pass, combined in wave order; thread j writes bin b0 + j of the pass's array
__global__ void __launch_bounds__(64) sens_profile_merge_kernel(const SensProfPartial *__restrict__ part, int nwaves, int nb,
                                                                samsim_pair_stat *__restrict__ out) {
  const int j = threadIdx.x;
  if (j >= nb) return;
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  Co co{0.0, 0.0, 0.0};
  for (int w = 0; w < nwaves; ++w) {
    const SensProfPartial p = part[(size_t)w * DEV_PROF_BINS + j];
    if (p.n > 0) merge(run, co, p.n, p.mean_y, p.m2_y, 0.0, 0.0, Co{p.mean_x, p.m2_x, p.cxy});
  }
  samsim_pair_stat st;
  st.count = run.n;
  if (run.n > 0) {
    const double dn = (double)run.n;
    st.mean_x = co.mean_x; st.mean_y = run.mean;
    st.var_x = co.m2_x / dn; st.var_y = run.m2 / dn; st.cov = co.cxy / dn;
  } else {
    st.mean_x = st.mean_y = st.var_x = st.var_y = st.cov = 0.0;
  }
  out[j] = st;
}

}  // namespace

extern "C" hipError_t samsim_launch_covariance(ColSet cs, SensRows rows, int nslots, double *part, CovResult *out, hipStream_t stream) {
  const int grid = slot_grid(cs.ncol, DEV_SENS_GRID);
  const bool known = dispatch_nslots(nslots, [&](auto ns) {
    hipLaunchKernelGGL(cov_kernel<decltype(ns)::value>, dim3(grid), dim3(64), 0, stream, rows, cs, part);
  });
  if (!known) return hipErrorInvalidValue;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cov_merge_kernel, dim3(nslots * (nslots + 1) / 2), dim3(64), 0, stream, part, grid, nslots, out);
  return hipGetLastError();
}

extern "C" hipError_t samsim_launch_profile_regression(ProfPass p, const double *x, SensProfPartial *part, samsim_pair_stat *out,
                                                       hipStream_t stream) {
  const int grid = pass_grid(p, DEV_SENS_GRID, DEV_PROF_BINS);
  if (!grid) return hipErrorInvalidValue;
  if (p.axis == SAMSIM_PROFILE_BY_LAYER)
    hipLaunchKernelGGL(sens_layer_kernel, dim3(grid), dim3(64), 0, stream, p.lay, x, p.n_active, p.status, p.labels, p.group, p.ncol, p.N,
                       p.origin, p.array, p.b0, p.nb, part);
  else
    hipLaunchKernelGGL(sens_depth_kernel, dim3(grid), dim3(64), 0, stream, p.lay, x, p.n_active, p.status, p.labels, p.group, p.ncol, p.N,
                       p.origin, p.array, p.b0, p.nb, p.lead, p.z0, p.dz, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sens_profile_merge_kernel, dim3(1), dim3(64), 0, stream, part, grid, p.nb, out);
  return hipGetLastError();
}
