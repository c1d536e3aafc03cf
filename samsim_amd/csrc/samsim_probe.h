// samsim_probe.h -- instrumentation of the step kernel for the profiling builds: SAMSIM_STAMPS (clock stamps / event counters) and
// SAMSIM_ISA_MARKS (marks in the assembly listing).  In the product library all of it compiles to nothing.
// Part of the translation unit samsim_kernels.hip: expects <hip/hip_runtime.h>; ST_MARK / ST_COUNT expect the context `x` in scope.
#ifndef SAMSIM_PROBE_H
#define SAMSIM_PROBE_H

// SAMSIM_STAMPS (profiling builds only, never the product library): 1 = s_memtime stamps around the regions of a time step,
// summed per wave in LDS and added to g_stamps at the end of the launch; 2 = event counters (Newton evaluations, loop trips).
// tools/stamps.py reads g_stamps through samsim_debug_stamps.
#ifndef SAMSIM_STAMPS
#define SAMSIM_STAMPS 0
#endif
// SAMSIM_ISA_MARKS: comment lines in the assembly listing at the boundaries of the hot loops (tools/isa_loops.py --marks)
#ifdef SAMSIM_ISA_MARKS
#define ISA_MARK(name) asm volatile("; ISA_MARK " name)
#else
#define ISA_MARK(name) ((void)0)
#endif
// (g_stamps and its reader have external linkage -- the host side finds them by name; the rest sits in the anonymous namespace)
#if SAMSIM_STAMPS
__device__ unsigned long long g_stamps[48];
extern "C" int samsim_debug_stamps(unsigned long long *out, int reset) {
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 48) != hipSuccess) return -1;
  if (reset) { unsigned long long z[48] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z)) != hipSuccess) return -1; }
  return 0;
}
#endif

namespace {

#if SAMSIM_STAMPS
enum { ST_PRO = 0, ST_DFUSED, ST_DUNFUSED, ST_SURF, ST_UP, ST_POST, ST_HEAD, ST_TAIL,
       CT_WAVESTEPS = 8, CT_FUSED, CT_UNFUSED, CT_UP_TRIPS, CT_NEWTON_WAVE, CT_NEWTON_LANE, CT_LANES, CT_DOWN_TRIPS, CT_DRAIN_WAVE,
       CT_DRAIN_LANE, CT_DIRTY, CT_L_COUPLING, ST_U_HEAD = 20, ST_U_GETT, ST_U_TAIL, ST_D_A, ST_D_B,
       CT_L_FLOODP = 25, CT_L_IRREG, CT_L_DIRTY, CT_L_UNFUSED, CT_L_FLUSH3, CT_L_REGRID, CT_L_FREEBOARD,
       CT_REFILL = 32, CT_ROWS, CT_ROWS_STILL, CT_ODD_LANES, CT_ODD_WAVES, CT_ODD_EVALS_WAVE, CT_LITE,
       CT_RAY_ROWS = 39, CT_RAY_ROWS_BOUND, CT_ABOVE_ROWS, CT_ABOVE_FAST, ST_NSLOT = 48 };
struct Stamps {
  unsigned long long *acc;   // [48] in LDS, one block = one wave
  unsigned long long t0;
};
__device__ __forceinline__ bool st_leader() { return (int)__lane_id() == __ffsll((long long)__ballot(1)) - 1; }
__device__ __forceinline__ void st_mark(Stamps &st, int region) {
#if SAMSIM_STAMPS == 1
  const unsigned long long t = __builtin_amdgcn_s_memtime();
  if (st_leader()) st.acc[region] += t - st.t0;
  st.t0 = t;
#endif
}
__device__ __forceinline__ void st_count(Stamps &st, int counter, unsigned long long n = 1) {
#if SAMSIM_STAMPS == 2
  if (st_leader()) st.acc[counter] += n;
#endif
}
#define ST_MARK(r) st_mark(x.st, r)
#define ST_COUNT(cn, n) st_count(x.st, cn, n)
#else
#define ST_MARK(r) ((void)0)
#define ST_COUNT(cn, n) ((void)0)
#endif

}  // namespace

#endif
