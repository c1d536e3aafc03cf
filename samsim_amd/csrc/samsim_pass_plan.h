// samsim_pass_plan.h -- the passes of a profile request (include/samsim.h, samsim_get_profile_stats): one per requested array and
// chunk of at most `chunk` bins, the arrays in the order of the request and the chunks of an array in ascending b0.  Plain C++, as
// samsim_row_plan.h is: the host loop of samsim_capi.cpp is this function, and tests/test_host_logic.py runs it without a device.
#ifndef SAMSIM_PASS_PLAN_H
#define SAMSIM_PASS_PLAN_H

#include "samsim_device.h"

// One pass: entry `array` of the request's list, bins [b0, b0 + nb).  lead: the pass does not begin where the walk of a column
// begins -- from the top every pass but the first, from the bottom every pass but the last (the depth walk skips the layers before
// such a chunk, samsim_profile_walk.h; the layer walk indexes its layers and does not ask).
struct PassSpan { int array, b0, nb, lead; };

// f(span) for every pass in order; the first value of f that is not 0 ends the enumeration and is returned
template <class F>
inline int pass_plan(int narrays, int nbins, int chunk, int origin, F f) {
  for (int i = 0; i < narrays; ++i)
    for (int b0 = 0; b0 < nbins; b0 += chunk) {
      const int nb = nbins - b0 < chunk ? nbins - b0 : chunk;
      const int lead = origin == SAMSIM_PROFILE_FROM_TOP ? b0 > 0 : b0 + nb < nbins;
      if (const int rc = f(PassSpan{i, b0, nb, lead})) return rc;
    }
  return 0;
}

// The chunk of a pass of the joint histograms (samsim_hist.h): the depth bins whose tile rows and count rows fit the LDS of a
// one-wave workgroup beside the lanes' masks, at most the DEV_PROF_BINS of a statistics pass.
#define DEV_HIST_LDS_BYTES (64 << 10)
static inline int dev_hist_row_stride(int nvbins) { return (nvbins + 2) | 1; }
static inline int dev_hist_chunk(int nvbins) {
  const int per_bin = (DEV_PROF_BINS + 1) * (int)sizeof(double) + dev_hist_row_stride(nvbins) * (int)sizeof(uint32_t);
  const int c = (DEV_HIST_LDS_BYTES - 64 * (int)sizeof(unsigned long long)) / per_bin;
  return c < DEV_PROF_BINS ? c : DEV_PROF_BINS;
}

// The chunk of a pass of the weighted joint histogram (samsim_wphist.h): the same rule with a table of doubles -- the depth bins
// whose tile rows and table rows [(nvbins + 2) | 1] fit the LDS of a one-wave workgroup beside the lanes' masks and the block's 64
// weights.  64 up to 59 value bins, 25 at SAMSIM_HIST_MAX_VBINS.  A request runs at most DEV_WPHIST_GRID waves, whatever ncol is:
// the number of waves decides the merge order and so the bytes, and with the chunk it bounds the waves' tables of a pass.
#define DEV_WPHIST_LDS_BYTES (64 << 10)
#ifndef DEV_WPHIST_GRID   // (a measuring build of the library may set another; the product is this line)
#define DEV_WPHIST_GRID 512
#endif
constexpr int dev_wphist_row_stride(int nvbins) { return (nvbins + 2) | 1; }
constexpr int dev_wphist_chunk(int nvbins) {
  const int per_bin = (DEV_PROF_BINS + 1 + dev_wphist_row_stride(nvbins)) * (int)sizeof(double);
  const int c = (DEV_WPHIST_LDS_BYTES - 64 * (int)sizeof(unsigned long long) - 64 * (int)sizeof(double)) / per_bin;
  return c < DEV_PROF_BINS ? c : DEV_PROF_BINS;
}
// LDS bytes of a pass, and the doubles of one wave's table in device memory [chunk][nvbins + 2]
constexpr long long dev_wphist_lds(int nvbins) {
  return (long long)dev_wphist_chunk(nvbins) * (DEV_PROF_BINS + 1 + dev_wphist_row_stride(nvbins)) * (long long)sizeof(double) + 1024;
}
constexpr long long dev_wphist_wave_doubles(int nvbins) { return (long long)dev_wphist_chunk(nvbins) * (nvbins + 2); }

#endif
