// samsim_groups.hip -- device-side ensemble statistics of the per-column scalars per group of columns (samsim_get_group_stats,
// include/samsim.h).
//
// One pass serves one [ncol] row (a scalar slot, or n_active) and every group at once.  One wave owns one 64-column block at a time
// (lane = column) and strides over the blocks with a fixed grid; its loads of the row, of status and of the labels are coalesced.
// The wave keeps a table of running (n, mean, M2, min, max) per group in LDS, sized by the handle's ngroups (40 B per group).  The
// values of a block are folded into the table in lane order: the wave walks the lanes whose column counts, broadcasts that lane's
// label and value, and the lane that owns the table entry (label mod 64) applies Welford's update.  No atomics, no [ngroups][ncol]
// intermediate.  At the end every wave stores its table; group_merge_kernel combines the waves' partials of a group in wave order
// (Chan's pairwise update), so a group's result depends on nothing but the values and the positions of its own columns.
#include <hip/hip_runtime.h>

#include "samsim_groups.h"

namespace {

// running statistics: n values with mean `mean` and sum of squared deviations `m2`
struct Run {
  long long n;
  double mean, m2, mn, mx;
};

// Chan et al.: (n, mean, M2) of the union of two sets from those of the sets; b is not empty (as merge of samsim_profile.hip)
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

// lane i's value in every lane (i is the same in every lane)
__device__ __forceinline__ double lane_value(double v, int i) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), i), hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
  return __hiloint2double(hi, lo);
}

// the lane's column of block blk: its group (-1: stopped, unlabelled or beyond ncol) and its value
__device__ __forceinline__ void load_column(const double *row, const int32_t *n_active, const int32_t *status, const int32_t *labels,
                                            long long ncol, int ngroups, long long blk, int lane, int &lab, double &v) {
  const long long col = blk * 64 + lane;
  lab = -1; v = 0.0;
  if (col < ncol) {
    const int l = labels[col];
    lab = (status[col] == 0 && l < ngroups) ? l : -1;
    v = row ? row[col] : (double)n_active[col];
  }
}

__global__ void __launch_bounds__(64) group_stats_kernel(const double *__restrict__ row, const int32_t *__restrict__ n_active,
                                                         const int32_t *__restrict__ status, const int32_t *__restrict__ labels,
                                                         long long ncol, int ngroups, GroupPartial *__restrict__ part) {
  extern __shared__ double table[];   // [5][ngroups]: mean, m2, min, max, n
  double *t_mean = table, *t_m2 = table + ngroups, *t_mn = table + 2 * (size_t)ngroups, *t_mx = table + 3 * (size_t)ngroups;
  long long *t_n = (long long *)(table + 4 * (size_t)ngroups);
  const int lane = threadIdx.x;
  for (int g = lane; g < ngroups; g += 64) {
    t_mean[g] = 0.0; t_m2[g] = 0.0; t_mn[g] = 1.0e300; t_mx[g] = -1.0e300; t_n[g] = 0;
  }
  __syncthreads();
  const long long nblk = (ncol + 63) / 64;
  int lab, lab_next = -1;
  double v, v_next = 0.0;
  load_column(row, n_active, status, labels, ncol, ngroups, blockIdx.x, lane, lab, v);
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    // the next block's loads are under way while this block is folded
    if (blk + gridDim.x < nblk) load_column(row, n_active, status, labels, ncol, ngroups, blk + gridDim.x, lane, lab_next, v_next);
    unsigned long long todo = __ballot(lab >= 0);
    while (todo) {   // the lanes whose column counts, in lane order
      const int i = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int g = __builtin_amdgcn_readlane(lab, i);
      const double x = lane_value(v, i);
      if (lane == (g & 63)) {   // Welford: the first value of a group is its mean exactly, equal values leave mean and M2 alone
        const long long n = t_n[g] + 1;
        const double mean = t_mean[g], delta = x - mean;
        const double mean1 = mean + delta / (double)n;
        t_n[g] = n;
        t_mean[g] = mean1;
        t_m2[g] = t_m2[g] + delta * (x - mean1);
        t_mn[g] = x < t_mn[g] ? x : t_mn[g];
        t_mx[g] = x > t_mx[g] ? x : t_mx[g];
      }
    }
    lab = lab_next; v = v_next;
  }
  __syncthreads();
  for (int g = lane; g < ngroups; g += 64) {
    GroupPartial p;
    p.mean = t_mean[g]; p.m2 = t_m2[g]; p.mn = t_mn[g]; p.mx = t_mx[g]; p.n = t_n[g];
    part[(size_t)blockIdx.x * ngroups + g] = p;
  }
}

// One workgroup per group: lane l combines the partials of the waves [l * per, (l + 1) * per) in wave order, then lane 0 combines
// the 64 lanes' results in lane order -- the waves' partials in wave order, bracketed the same way whatever the data.
__global__ void __launch_bounds__(64) group_merge_kernel(const GroupPartial *__restrict__ part, int nwaves, int ngroups,
                                                         samsim_stat *__restrict__ out) {
  __shared__ GroupPartial s_run[64];
  const int lane = threadIdx.x, g = blockIdx.x;
  const int per = (nwaves + 63) / 64;
  Run run{0, 0.0, 0.0, 0.0, 0.0};
  for (int w = lane * per; w < (lane + 1) * per && w < nwaves; ++w) {
    const GroupPartial p = part[(size_t)w * ngroups + g];
    if (p.n > 0) merge(run, p.n, p.mean, p.m2, p.mn, p.mx);
  }
  GroupPartial mine;
  mine.mean = run.mean; mine.m2 = run.m2; mine.mn = run.mn; mine.mx = run.mx; mine.n = run.n;
  s_run[lane] = mine;
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < 64; ++l) {
    const GroupPartial p = s_run[l];
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
  out[g] = st;
}

}  // namespace

extern "C" hipError_t samsim_launch_group_stats(const double *row, const int32_t *n_active, const int32_t *status, const int32_t *labels,
                                                long long ncol, int ngroups, GroupPartial *part, samsim_stat *out, hipStream_t stream) {
  const int grid = dev_group_waves(ncol, ngroups);
  hipLaunchKernelGGL(group_stats_kernel, dim3(grid), dim3(64), sizeof(GroupPartial) * (size_t)ngroups, stream, row, n_active, status,
                     labels, ncol, ngroups, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(group_merge_kernel, dim3(ngroups), dim3(64), 0, stream, part, grid, ngroups, out);
  return hipGetLastError();
}
