// samsim_groups.hip -- device-side ensemble statistics of the per-column scalars per group of columns (samsim_get_group_stats,
// include/samsim.h).
//
// One pass serves one [ncol] row (a scalar slot, or n_active) and every group at once, with the walk and the bracket of
// samsim_slot_walk.h.  The wave keeps a table of running (n, mean, M2, min, max) per group in LDS, sized by the handle's ngroups
// (40 B per group).  The values of a block are folded into the table in lane order: the wave walks the lanes whose column counts,
// broadcasts that lane's label and value, and the lane that owns the table entry (label mod 64) applies Welford's update.  No
// atomics, no [ngroups][ncol] intermediate.  At the end every wave stores its table; group_merge_kernel combines the waves'
// partials of a group (Chan's pairwise update, samsim_profile_fold.h), so a group's result depends on nothing but the values and
// the positions of its own columns.
#include <hip/hip_runtime.h>

#include "samsim_groups.h"
#include "samsim_profile_fold.h"

namespace {

using namespace slot_walk;

// the running statistics of the profile families, as the bracket takes them
struct GroupAcc : profile_fold::Run {
  __device__ __forceinline__ void absorb(const GroupAcc &b) {
    if (b.n > 0) profile_fold::merge(*this, b.n, b.mean, b.m2, b.mn, b.mx);
  }
};

__global__ void __launch_bounds__(64) group_stats_kernel(const double *__restrict__ row, LabelSet cs, int ngroups,
                                                         GroupPartial *__restrict__ part) {
  extern __shared__ double table[];   // [5][ngroups]: mean, m2, min, max, n
  double *t_mean = table, *t_m2 = table + ngroups, *t_mn = table + 2 * (size_t)ngroups, *t_mx = table + 3 * (size_t)ngroups;
  long long *t_n = (long long *)(table + 4 * (size_t)ngroups);
  const int lane = threadIdx.x;
  for (int g = lane; g < ngroups; g += 64) {
    t_mean[g] = 0.0; t_m2[g] = 0.0; t_mn[g] = 1.0e300; t_mx[g] = -1.0e300; t_n[g] = 0;
  }
  __syncthreads();
  walk_blocks<LabelCol>(
      cs.ncol, lane, [&](long long blk, int ln, LabelCol &c) { load_label_col(cs, row, ngroups, blk, ln, c); },
      [&](long long, const LabelCol &c) {
        unsigned long long todo = __ballot(c.lab >= 0);
        while (todo) {   // the lanes whose column counts, in lane order
          const int i = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const int g = __builtin_amdgcn_readlane(c.lab, i);
          const double x = lane_value(c.v, i);
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
      });
  __syncthreads();
  for (int g = lane; g < ngroups; g += 64) {
    GroupPartial p;
    p.mean = t_mean[g]; p.m2 = t_m2[g]; p.mn = t_mn[g]; p.mx = t_mx[g]; p.n = t_n[g];
    part[(size_t)blockIdx.x * ngroups + g] = p;
  }
}

// one workgroup per group: the waves' partials of the group in wave order
__global__ void __launch_bounds__(64) group_merge_kernel(const GroupPartial *__restrict__ part, int nwaves, int ngroups,
                                                         samsim_stat *__restrict__ out) {
  __shared__ GroupAcc s_run[64];
  const int g = blockIdx.x;
  GroupAcc run{{0, 0.0, 0.0, 0.0, 0.0}};
  const bool last = merge_waves(nwaves, run, s_run, threadIdx.x, [&](int w) {
    const GroupPartial p = part[(size_t)w * ngroups + g];
    return GroupAcc{{p.n, p.mean, p.m2, p.mn, p.mx}};
  });
  if (!last) return;
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

extern "C" hipError_t samsim_launch_group_stats(LabelSet cs, const double *row, int ngroups, GroupPartial *part, samsim_stat *out,
                                                hipStream_t stream) {
  const int grid = dev_group_waves(cs.ncol, ngroups);
  hipLaunchKernelGGL(group_stats_kernel, dim3(grid), dim3(64), sizeof(GroupPartial) * (size_t)ngroups, stream, row, cs, ngroups, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(group_merge_kernel, dim3(ngroups), dim3(64), 0, stream, part, grid, ngroups, out);
  return hipGetLastError();
}
