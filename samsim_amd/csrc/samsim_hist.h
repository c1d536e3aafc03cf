// samsim_hist.h -- what samsim_hist.hip and the C-ABI host code share about the fixed-edge ensemble histograms
// (samsim_get_histogram / samsim_get_profile_histogram, include/samsim.h).  The step kernel does not include this header.
#ifndef SAMSIM_HIST_H
#define SAMSIM_HIST_H

#include <hip/hip_runtime.h>

#include "samsim_pass_plan.h"
#include "samsim_profile.h"
#include "samsim_slot_walk.h"

// A row of counts has W = nvbins + 2 entries.  Both reductions run a fixed grid of at most DEV_HIST_GRID one-wave workgroups; a
// wave counts in 32-bit entries of an LDS table and adds what it found to the 64-bit result table in device memory with integer
// atomics when it is done: integer adds are exact in any order, so the result depends on nothing but the state and the request.
#define DEV_HIST_GRID 1024

// ---- scalars.  A wave's table holds ngroups * W counts (ngroups = 1 without groups).  Up to DEV_HIST_LDS_COUNTS counts (32 KiB
// of LDS: two waves per CU's 64 KiB share and more) the table lives in LDS; beyond, every lane adds straight into the 64-bit
// result table.  Nine sites x 32 entries take the LDS path, 1 024 groups x 256 entries the global one.
#define DEV_HIST_LDS_COUNTS 8192
static inline bool dev_hist_in_lds(int ngroups, int nvbins) { return (long long)ngroups * (nvbins + 2) <= DEV_HIST_LDS_COUNTS; }

// ---- layer profiles.  A pass serves `chunk` depth bins: the LDS of a one-wave workgroup holds the walk's tile [chunk][64 + 1]
// doubles, the lanes' bin masks (512 B) and the count table [chunk][W | 1] of 32-bit entries (the odd row stride spreads the 64
// lanes' rows over the banks); together at most the 64 KiB a workgroup gets without an opt-in.  Up to 121 value bins a pass
// serves 64 depth bins as the statistics do, at SAMSIM_HIST_MAX_VBINS (254) 42.  Cost: passes = ceil(nbins / chunk), each a walk over
// the layers of every column as in samsim_get_profile_stats.
// (DEV_HIST_LDS_BYTES, dev_hist_row_stride and dev_hist_chunk: samsim_pass_plan.h, where the host test of the passes reaches them)
static inline size_t dev_hist_profile_lds(int nvbins) {
  const size_t c = (size_t)dev_hist_chunk(nvbins);
  return c * (DEV_PROF_BINS + 1) * sizeof(double) + 64 * sizeof(unsigned long long) + c * dev_hist_row_stride(nvbins) * sizeof(uint32_t);
}

// the edges of a request: E_j = v0 + j*dv (product rounded, then the sum); rdv = 1/dv only serves the device's first guess
struct HistEdges { double v0, dv, rdv; int nvbins; };

// The entry of a value, the one rule the histograms of samsim_hist.hip and the weighted one of samsim_weights.hip count by: the
// number of edges E_j = v0 + j*dv, j = 0..nvbins, with E_j <= v.  The quotient only guesses j; the guess is then moved until E_j <= v < E_{j+1} holds for the rounded edges themselves (the host has checked that they increase strictly).
// A NaN compares false and lands in entry 0.
__device__ __forceinline__ int hist_entry(double v, const HistEdges &e) {
  if (!(v >= e.v0)) return 0;   // below E_0 = v0 + 0*dv = v0, or NaN
  const double t = (v - e.v0) * e.rdv;
  int j = t >= (double)e.nvbins ? e.nvbins : (t > 0.0 ? (int)t : 0);   // the largest j with E_j <= v, if the guess is right
  while (j < e.nvbins && e.v0 + (double)(j + 1) * e.dv <= v) ++j;
  while (j > 0 && e.v0 + (double)j * e.dv > v) --j;
  return j + 1;
}

// samsim_hist.hip.  counts: the 64-bit result table in device memory, zero before the first pass of a request.
// Scalars: the histogram of one row (row, or n_active where row is null) per group of cs.labels -- null: one group of every column
// with status 0 --, counts[ngroups][W].
extern "C" hipError_t samsim_launch_hist(slot_walk::LabelSet cs, const double *row, int ngroups, HistEdges e, unsigned long long *counts,
                                         hipStream_t stream);
// Profiles, one pass (samsim_profile.h) with nb <= dev_hist_chunk(nvbins): rows b0 .. b0+nb-1 of counts[nbins][W].
extern "C" hipError_t samsim_launch_profile_hist(ProfPass p, HistEdges e, unsigned long long *counts, hipStream_t stream);

#endif
