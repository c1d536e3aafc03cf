// samsim_capi.cpp -- host side of the C-ABI declared in include/samsim.h.
//
// Owns the HBM allocations of a handle (layout: samsim_device.h), mirrors the uniform clock of the ensemble on
// the host (time, step, output counter, forcing-table cursor are the same for every column, so nothing has to
// be read back to know them) and launches the step kernel on the handle's HIP stream.  There is no CPU
// implementation of the physics here or anywhere else in the product: without a HIP device every entry point
// that would compute returns SAMSIM_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "samsim_copy.h"
#include "samsim_device.h"
#include "samsim_functionals.h"
#include "samsim_groups.h"
#include "samsim_hist.h"
#include "samsim_jitter.h"
#include "samsim_pass_plan.h"
#include "samsim_resample.h"
#include "samsim_select.h"
#include "samsim_sensors.h"
#include "samsim_sens.h"
#include "samsim_tracks.h"
#include "samsim_weights.h"
#include "samsim_wphist.h"
#include "samsim_wprofile.h"

extern "C" hipError_t samsim_launch_step(const DevParams *d_params, const DevParams *hp, long long grid, hipStream_t stream);

namespace {

constexpr int kRing = 16;

thread_local char g_last_hip_error[256] = "";

bool hip_ok(hipError_t e, const char *what) {
  if (e == hipSuccess) return true;
  std::snprintf(g_last_hip_error, sizeof(g_last_hip_error), "%s: %s", what, hipGetErrorString(e));
  return false;
}
#define HIPCHK(call)                                  \
  do {                                                \
    if (!hip_ok((call), #call)) return SAMSIM_ERR_HIP; \
  } while (0)

}  // namespace

struct samsim_handle {
  samsim_config cfg{};
  long long ncol = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  // A step of a large ensemble is two launches: the first half of the 64-column blocks on `stream`, the rest on `stream2`.  Columns
  // never meet, so each part only follows its own previous launch; the workgroups of a launch finish raggedly (the last of the
  // four rounds of a 16 384-block launch leaves the chip partly idle for 15 % of a workgroup's run time), and with two launches
  // in flight per step, and the next step's enqueued behind them, a draining launch is topped up by the others.  Every other entry point waits for both.
  hipStream_t stream2 = nullptr;
  hipEvent_t fork = nullptr;      // recorded on `stream` when other work was enqueued there since the last launch: stream2 waits for it
  bool other_work = true;
  int split_eighths = 4;          // share of the first part in eighths (samsim_set_launch_split; 4, 5, 6, 7 eighths measured 962, 973,
                                  // 968, 992 ms per 500-step step of 1 048 576 columns, one launch 1 009 ms; three and four parts 1 015, 969-986)
  long long split_blocks = 8192;  // a launch of at least this many 64-column blocks is split (samsim_set_launch_split; 0 = never)
  hipEvent_t ev0b = nullptr, ev1b = nullptr;
  // device memory
  double *lay = nullptr, *scal = nullptr;
  int32_t *n_active = nullptr, *status = nullptr, *err_layer = nullptr;
  long long *err_step = nullptr, *work = nullptr;
  double *spec = nullptr;      // hand-over block of the up sweep, [DEV_NSPEC][ncol]
  int32_t *flags = nullptr;    // COLF_* per column
  void *d_stat = nullptr;      // block partials of samsim_get_ensemble_stats
  void *d_prof = nullptr;      // samsim_get_profile_stats: the waves' partials of one pass, then the results (kProfScratch bytes)
  int32_t *groups = nullptr;   // [ncol] group label of each column (samsim_set_groups), owned by the caller as the forcing is
  int32_t ngroups = 0;         // 0: no labels
  void *d_group = nullptr;     // samsim_get_group_stats: the waves' partials of one slot, then its results (kGroupScratch bytes)
  void *d_hist = nullptr;      // samsim_get_histogram / samsim_get_profile_histogram: the 64-bit counts of one request (kHistScratch bytes)
  void *d_sens = nullptr;      // samsim_get_covariance / samsim_get_profile_regression: the waves' partials of one pass, then the results (kSensScratch bytes)
  void *d_select = nullptr;    // samsim_select_columns / samsim_get_columns: the waves' counts and offsets, and the index list (kSelectScratch bytes)
  double *tracks = nullptr;    // [ntracks][SAMSIM_NTF][ncol] rows of the time-domain diagnostics (samsim_set_tracks), sampled by launch()
  int32_t ntracks = 0;         // 0: no tracking
  long long track_every = 0;   // a sample follows the step that brings clk.step to a multiple of it
  TrackDev track[SAMSIM_MAX_TRACKS]{};
  double *func_rows = nullptr; // [nfunc][ncol] rows of the column functionals (samsim_set_functionals), evaluated by func_refresh()
  int32_t nfunc = 0;           // 0: no functionals
  bool func_dirty = true;      // the state changed since the rows were evaluated (stepping, set_state, set_status, set_functionals)
  samsim_functional_spec func[SAMSIM_MAX_FUNCTIONALS]{};
  double *score_rows = nullptr; // [SAMSIM_NSF][ncol] rows of the per-column misfit (samsim_set_sensors), updated by samsim_score
  int32_t nsensors = 0;        // 0: no sensors
  samsim_sensor_spec sensor[SAMSIM_MAX_SENSORS]{};
  double *weight_row = nullptr; // [ncol] weights of the columns (samsim_set_weights), changed by that call alone
  void *d_weight = nullptr;    // samsim_set_weights and the weighted reductions: the waves' tables and partials, then the results (kWeightScratch bytes)
  void *d_wprof = nullptr;     // samsim_get_weighted_profile_stats: the waves' partials of one pass, then the results (kWProfScratch bytes)
  void *d_wphist = nullptr;    // samsim_get_weighted_profile_histogram: the waves' tables of one pass, then the result (kWPHistScratch bytes)
  double *offspring_row = nullptr;   // [ncol] offspring of the columns (samsim_resample), changed by that call alone
  long long *ancestors = nullptr;    // [ancestors_cap] the ancestor of every draw, the first m_drawn entries valid
  long long ancestors_cap = 0, m_drawn = 0;
  void *d_resample = nullptr;  // samsim_resample: the ranges' sums, bases and partials, then the result (kResampleScratch bytes)
  int32_t rs_group = -1;       // the group of the last samsim_resample: the pool of samsim_apply_resample
  bool rs_applied = false;     // samsim_apply_resample has applied the rows of the last samsim_resample
  long long *copy_src = nullptr, *copy_dst = nullptr;   // [ncol] each: the lists of samsim_copy_columns on the device
  long long *plan_src = nullptr, *plan_dst = nullptr;   // [ncol] each: the plan of the last samsim_apply_resample, plan_n entries
  long long plan_n = -1;       // -1: no plan applied yet
  void *d_copy = nullptr;      // samsim_apply_resample: the ranges' partials and offsets, then the result (kCopyScratch bytes)
  void *d_jitter = nullptr;    // samsim_jitter: the ranges' counts, then the totals (kJitterScratch bytes)
  double *stage = nullptr;     // staging buffer of samsim_set_state / samsim_get_state (boundary layout), grown on demand up to
  size_t stage_n = 0;          // kStageBytes and kept: no hipMalloc / hipFree -- both wait for the whole device -- per call
  // passive tracers (bgc_flag 2)
  double *bgc = nullptr, *bgc_bot = nullptr, *bfl = nullptr, *out_bgc = nullptr, *out_bgc_bot = nullptr;
  int32_t n_bgc = 0;
  double bgc_total0 = 0.0;
  double *f_sw = nullptr, *f_lw = nullptr, *f_T2m = nullptr, *f_precip = nullptr;
  int32_t flen = 0, nsites = 1;
  int32_t *site = nullptr;     // [ncol] forcing set of each column (nsites > 1)
  double *ocean_dflq = nullptr, *ocean_sbu = nullptr;   // samsim_set_ocean: per-column oceanic heat-flux offset / salinity below
  double *out_lay = nullptr, *out_scal = nullptr;
  int32_t *out_n_active = nullptr;
  long long out_col0 = 0, out_ncols = 0;
  // parameter ring (pinned host + device), one event per slot
  DevParams *h_params = nullptr, *d_params = nullptr;
  hipEvent_t slot_done[kRing]{};
  int slot = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // uniform clock, mirrored on the host
  samsim_clock clk{};
  bool stepped = false;        // the kernel has run since the last samsim_set_state: S_bu is refreshed from S_abs / m on get_state
  bool snap_valid = false;
  double snap_time = 0.0;
  long long snap_step = 0;
  double p17 = 0, p14 = 0, tf_c3 = 0;
};

namespace {

// Upper bound of the staging buffer (SAMSIM_STAGE_MAX_BYTES, 256 MiB): samsim_set_state / samsim_get_state move a window through
// it in pieces of at most this many bytes, so the buffer never holds more, whatever the window.  Unbounded, one full-handle
// get_state at SAMSIM_MAX_NCOL x 80 layers would need 136 GB of staging beside the 151 GB handle.  256 MiB is 0.2 % of such a
// handle, yet a piece is still ~10 ms of copying over the host link against some tens of microseconds of fixed cost (one scatter /
// gather launch and one synchronisation), so pieces cost no throughput.  It also bounds the scatter / gather grid (32 Mi threads
// per launch; a whole window of 15 arrays of 80 layers would pass the 2^32 work-items of one dispatch from 3.6 M columns on).
constexpr size_t kStageBytes = (size_t)SAMSIM_STAGE_MAX_BYTES;

// columns of one staging piece for narr arrays of N layers: a multiple of 64 (whole column blocks) within kStageBytes
static_assert(kStageBytes / ((size_t)SAMSIM_NARR * SAMSIM_MAX_NLAYER * sizeof(double)) >= 64, "a staging piece holds a column block");
size_t stage_cols(int narr, size_t N) { return (kStageBytes / ((size_t)narr * N * sizeof(double))) & ~(size_t)63; }

// rows x cols doubles between two row-major blocks of row lengths dpitch / spitch (in doubles): one plain copy when both are
// contiguous (a window that fits one piece), else one 2D copy
hipError_t copy_rows(double *dst, size_t dpitch, const double *src, size_t spitch, size_t cols, size_t rows, hipMemcpyKind kind,
                     hipStream_t s) {
  if (dpitch == cols && spitch == cols) return hipMemcpyAsync(dst, src, rows * cols * sizeof(double), kind, s);
  return hipMemcpy2DAsync(dst, dpitch * sizeof(double), src, spitch * sizeof(double), cols * sizeof(double), rows, kind, s);
}

// the handle's staging buffer with room for n doubles
hipError_t stage_for(samsim_handle *h, size_t n) {
  if (n <= h->stage_n) return hipSuccess;
  (void)hipFree(h->stage);
  h->stage = nullptr; h->stage_n = 0;
  hipError_t e = hipMalloc((void **)&h->stage, n * sizeof(double));
  if (e == hipSuccess) h->stage_n = n;
  return e;
}

int validate(const samsim_config &c) {
  if (c.struct_size != (int32_t)sizeof(samsim_config)) return SAMSIM_ERR_ABI;
  if (c.nlayer < 3 || c.nlayer > SAMSIM_MAX_NLAYER) return SAMSIM_ERR_ARG;
  if (c.n_top < 3 || c.n_bottom < 1 || c.n_middle < 1 || c.n_top + c.n_middle + c.n_bottom != c.nlayer) return SAMSIM_ERR_ARG;
  if (!(c.dt > 0.0) || !(c.thick_0 > 0.0) || c.i_time_out < 0) return SAMSIM_ERR_ARG;
  auto in = [](int v, std::initializer_list<int> ok) { for (int o : ok) if (v == o) return true; return false; };
  // testcases whose per-step specifics (mo_grotz.f90:505-565) read the lab's forcing tables or re-impose a snow cover: refused
  // rather than run without them
  if (in(c.testcase, {8, 44, 45, 99, 101, 102, 103, 104, 105, 111})) return SAMSIM_ERR_UNSUPPORTED;
  if (!in(c.boundflux_flag, {1, 2, 3}) || (c.boundflux_flag == 3 && c.lab_snow_flag != 0)) return SAMSIM_ERR_UNSUPPORTED;
  if (!in(c.atmoflux_flag, {1, 2, 3})) return SAMSIM_ERR_UNSUPPORTED;
  if (c.tank_flag == 2 && !(c.m_total > 0.0)) return SAMSIM_ERR_ARG;
  if (!in(c.grav_flag, {1, 2, 3}) || !in(c.prescribe_flag, {1, 2}) || !in(c.grav_heat_flag, {1, 2}) || !in(c.flush_heat_flag, {1, 2}))
    return SAMSIM_ERR_UNSUPPORTED;
  if (!in(c.turb_flag, {1, 2}) || !in(c.salt_flag, {1, 2}) || !in(c.flush_flag, {1, 4, 5, 6}) || !in(c.flood_flag, {1, 2, 3}))
    return SAMSIM_ERR_UNSUPPORTED;
  if (!in(c.bottom_flag, {1, 2}) || !in(c.precip_flag, {0, 1}) || !in(c.harmonic_flag, {1, 2}) || !in(c.tank_flag, {1, 2}))
    return SAMSIM_ERR_UNSUPPORTED;
  if (!in(c.albedo_flag, {1, 2}) || !in(c.freeboard_snow_flag, {0, 1}) || !in(c.snow_flush_flag, {0, 1}) || !in(c.bgc_flag, {1, 2}))
    return SAMSIM_ERR_UNSUPPORTED;
  return SAMSIM_OK;
}

template <typename T>
hipError_t dalloc(T **p, size_t n) { return hipMalloc((void **)p, n * sizeof(T)); }

bool launch_needs_forcing(const samsim_config &c) { return c.atmoflux_flag == 2; }

// ---- ensemble statistics: two passes (mean / min / max, then the squared deviations) over one [ncol] row, columns with a
// STOP code skipped; fixed grid + tree reduction, so the result does not depend on scheduling
constexpr int kStatBlock = 256, kStatGrid = 512;
struct StatPartial { double sum, mn, mx, ssq; long long n; };

template <bool PASS2>
__global__ void __launch_bounds__(kStatBlock) stat_kernel(const double *__restrict__ row, const int32_t *__restrict__ irow,
                                                          const int32_t *__restrict__ status, long long n, double mean,
                                                          StatPartial *__restrict__ part) {
  __shared__ double s_sum[kStatBlock], s_mn[kStatBlock], s_mx[kStatBlock];
  __shared__ long long s_n[kStatBlock];
  double sum = 0.0, mn = 1.0e300, mx = -1.0e300;
  long long cnt = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (status[i]) continue;
    const double v = row ? row[i] : (double)irow[i];
    if (PASS2) {
      sum += (v - mean) * (v - mean);
    } else {
      sum += v; mn = v < mn ? v : mn; mx = v > mx ? v : mx; ++cnt;
    }
  }
  const int t = threadIdx.x;
  s_sum[t] = sum; s_mn[t] = mn; s_mx[t] = mx; s_n[t] = cnt;
  __syncthreads();
  for (int w = kStatBlock / 2; w > 0; w >>= 1) {
    if (t < w) {
      s_sum[t] += s_sum[t + w];
      s_mn[t] = s_mn[t + w] < s_mn[t] ? s_mn[t + w] : s_mn[t];
      s_mx[t] = s_mx[t + w] > s_mx[t] ? s_mx[t + w] : s_mx[t];
      s_n[t] += s_n[t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    if (PASS2) part[blockIdx.x].ssq = s_sum[0];
    else { part[blockIdx.x].sum = s_sum[0]; part[blockIdx.x].mn = s_mn[0]; part[blockIdx.x].mx = s_mx[0]; part[blockIdx.x].n = s_n[0]; }
  }
}

// device scratch of samsim_get_profile_stats: the partials of one pass (every pass reuses them), then the results of the largest request
constexpr size_t kProfPartBytes = sizeof(ProfPartial) * DEV_PROF_GRID * DEV_PROF_BINS;
constexpr size_t kProfScratch = kProfPartBytes + sizeof(samsim_stat) * SAMSIM_PROFILE_MAX_ARRAYS * SAMSIM_PROFILE_MAX_BINS;
static_assert(kProfScratch <= SAMSIM_PROFILE_SCRATCH_BYTES && SAMSIM_PROFILE_SCRATCH_BYTES <= (64ull << 20), "profile scratch bound of samsim.h");
static_assert(SAMSIM_PROFILE_MAX_BINS == SAMSIM_MAX_NLAYER, "a layer-axis request may ask for every layer");

// device scratch of samsim_get_group_stats: the partials of one slot (every slot reuses them), then the results of one slot
constexpr size_t kGroupPartBytes = sizeof(GroupPartial) * DEV_GROUP_PART_ENTRIES;
constexpr size_t kGroupScratch = kGroupPartBytes + sizeof(samsim_stat) * SAMSIM_MAX_GROUPS;
static_assert(kGroupScratch <= SAMSIM_GROUP_SCRATCH_BYTES, "group scratch bound of samsim.h");
static_assert(DEV_GROUP_PART_ENTRIES >= SAMSIM_MAX_GROUPS, "at least one wave at the largest number of groups");
static_assert(sizeof(GroupPartial) * SAMSIM_MAX_GROUPS <= (64u << 10), "a wave's table of every group fits the LDS of a workgroup");

// device scratch of the histograms: the counts of the largest request, [ngroups][nvbins + 2] or [nbins][nvbins + 2]
constexpr size_t kHistScratch = sizeof(int64_t) * (SAMSIM_HIST_MAX_VBINS + 2) *
                                (SAMSIM_MAX_GROUPS > SAMSIM_PROFILE_MAX_BINS ? SAMSIM_MAX_GROUPS : SAMSIM_PROFILE_MAX_BINS);
static_assert(kHistScratch <= SAMSIM_HIST_SCRATCH_BYTES && SAMSIM_HIST_SCRATCH_BYTES <= (16ull << 20), "histogram scratch bound of samsim.h");
static_assert(sizeof(uint32_t) * DEV_HIST_LDS_COUNTS <= DEV_HIST_LDS_BYTES, "a wave's table of the scalar histogram fits the LDS of a workgroup");

// device scratch of the sensitivities: the partials of one pass (every pass reuses them), then the results of the largest request
constexpr size_t kSensScratch = DEV_SENS_PART_BYTES + DEV_SENS_RESULT_BYTES;
static_assert(kSensScratch <= SAMSIM_SENS_SCRATCH_BYTES && SAMSIM_SENS_SCRATCH_BYTES <= (16ull << 20), "sensitivity scratch bound of samsim.h");
static_assert(sizeof(samsim_pair_stat) == 48, "samsim_pair_stat of samsim.h");

// device scratch of the selection and of the gather of scattered columns: the waves' counts and offsets, and the index list
constexpr size_t kSelectScratch = DEV_SEL_BYTES;
static_assert(kSelectScratch <= SAMSIM_SELECT_SCRATCH_BYTES && SAMSIM_SELECT_SCRATCH_BYTES <= (16ull << 20), "select scratch bound of samsim.h");
static_assert(sizeof(samsim_select_term) == 24 && sizeof(samsim_selection) == 24 + 24 * SAMSIM_SELECT_MAX_TERMS, "samsim_selection of samsim.h");
static_assert((size_t)SAMSIM_SELECT_MAX_OUT * DEV_SEL_COLUMN_BYTES <= kStageBytes, "the per-column rows of the largest request are one piece");

// device scratch of the weight row and the weighted reductions: the waves' histogram tables, their partials, then the results
constexpr size_t kWeightScratch = DEV_WEIGHT_BYTES;
static_assert(kWeightScratch <= SAMSIM_WEIGHT_SCRATCH_BYTES && SAMSIM_WEIGHT_SCRATCH_BYTES <= (16ull << 20), "weight scratch bound of samsim.h");
static_assert(sizeof(samsim_weight_spec) == 32 && sizeof(samsim_weight_info) == 40 && sizeof(samsim_wstat) == 56, "the weight structs of samsim.h");

// device scratch of the weighted profile statistics: the waves' partials of one pass, then the results of the largest request
constexpr size_t kWProfScratch = DEV_WPROF_BYTES;
static_assert(kWProfScratch <= SAMSIM_WPROFILE_SCRATCH_BYTES && SAMSIM_WPROFILE_SCRATCH_BYTES <= (16ull << 20), "weighted profile scratch bound of samsim.h");

// device scratch of the weighted joint histogram: the waves' tables of one pass, then the result of the largest request
constexpr size_t kWPHistScratch = DEV_WPHIST_BYTES;
static_assert(kWPHistScratch <= SAMSIM_WPHIST_SCRATCH_BYTES && SAMSIM_WPHIST_SCRATCH_BYTES <= (64ull << 20), "weighted profile histogram scratch bound of samsim.h");
// samsim_resample: the ranges' sums, bases and integer partials, then the result (samsim_resample.h); the two rows are the handle's own
constexpr size_t kResampleScratch = DEV_RS_BYTES;
constexpr size_t kCopyScratch = DEV_CP_BYTES;
static_assert(kCopyScratch <= SAMSIM_COPY_SCRATCH_BYTES, "copy scratch bound of samsim.h");
constexpr size_t kJitterScratch = DEV_JT_BYTES;
static_assert(kJitterScratch <= SAMSIM_JITTER_SCRATCH_BYTES, "jitter scratch bound of samsim.h");
static_assert(sizeof(samsim_jitter_term) == 48 && sizeof(samsim_jitter_spec) == 216 && sizeof(samsim_jitter_info) == 72, "the jitter structs of samsim.h");
static_assert(kResampleScratch <= SAMSIM_RESAMPLE_SCRATCH_BYTES, "resample scratch bound of samsim.h");

// fill a [rows][ncol] device block with one value per row-set
__global__ void fill_rows(double *dst, size_t n, double v) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = v;
}
__global__ void fill_i32(int32_t *dst, size_t n, int32_t v) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = v;
}

// S_bu(k) = S_abs(k)/m(k) for the active layers: the kernel keeps the bulk salinity in registers only (every reader
// derives it from S_abs and m), so the array is brought up to date when the host asks for the state
__global__ void refresh_s_bu(double *lay, const int32_t *n_active, const int32_t *status, const int32_t *flags, size_t ncol, int N, size_t col0,
                             size_t w) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w) return;
  const size_t c = col0 + i;
  const column_read::Column q = column_read::column(n_active, status, flags, c, N, true);
  if (!q.adjust) return;   // a column that stopped keeps what it held (its masses may be zero)
  for (int k = 0; k < q.na; ++k) {
    const double m = lay[DEV_LAY_INDEX(SAMSIM_A_M, k, c, N, ncol)];
    if (m != 0.0) lay[DEV_LAY_INDEX(SAMSIM_A_S_BU, k, c, N, ncol)] = lay[DEV_LAY_INDEX(SAMSIM_A_S_ABS, k, c, N, ncol)] / m;
  }
}

// The health check at the end of a step clamps S_abs >= 0 over the active layers (mo_grotz.f90:812-818); the step kernel applies it
// in the first sweep of the NEXT step.  samsim_get_state applies it to what it returns (and to the device copy, which the next first
// sweep would clamp to the same values), so the state at a step boundary is the reference's and a checkpoint holds nothing that still
// waits for the clamp.  Columns that stopped, and columns uploaded since the last step (COLF_RESTART), keep what they hold
// (column_read::Column; both kernels are launched only once the step kernel has run).
__global__ void clamp_s_abs(double *lay, const int32_t *n_active, const int32_t *status, const int32_t *flags, size_t ncol, int N, size_t col0,
                            size_t w) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w) return;
  const size_t c = col0 + i;
  const column_read::Column q = column_read::column(n_active, status, flags, c, N, true);
  if (!q.clamp) return;
  for (int k = 0; k < q.na; ++k) {
    const size_t j = DEV_LAY_INDEX(SAMSIM_A_S_ABS, k, c, N, ncol);
    if (lay[j] < 0.0) lay[j] = 0.0;
  }
}

// The boundary keeps [array][layer][column] (samsim_state_soa); the device layout is DEV_LAY_INDEX.  A window of columns passes
// through a staging buffer in the boundary's layout: scatter = staging -> device layout, gather = the reverse.
template <bool GATHER>
__global__ void lay_window(double *lay, double *stage, int narr, int N, size_t ncol, size_t col0, size_t w) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)narr * N * w) return;
  const size_t cw = i % w, ak = i / w;
  const int k = (int)(ak % (size_t)N), a = (int)(ak / (size_t)N);
  const size_t j = DEV_LAY_INDEX(a, k, col0 + cw, N, ncol);
  if (GATHER) stage[i] = lay[j]; else lay[j] = stage[i];
}
// one value into every layer of one array
__global__ void lay_fill_array(double *lay, int a, int N, size_t ncol, double v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)N * ncol) return;
  lay[DEV_LAY_INDEX(a, (int)(i / ncol), i % ncol, N, ncol)] = v;
}

hipError_t fill(double *dst, size_t n, double v, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(fill_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, n, v);
  return hipGetLastError();
}

void advance_clock(samsim_handle *h, long long nsteps) {
  samsim_clock &k = h->clk;
  const samsim_config &c = h->cfg;
  for (long long s = 0; s < nsteps; ++s) {
    if (c.atmoflux_flag == 2) {
      const double ti = ((double)(float)k.time_counter - 1.0) * 3600.0 * 3.0;
      if (k.time > ti) k.time_counter += 1;
      if (k.time_counter > h->flen) k.time_counter = h->flen;
    }
    const bool out = (k.n_time_out == c.i_time_out) || (k.step + 1 == 1);
    if (out) {
      k.n_time_out = 0;
      k.n_outputs += 1;
      h->snap_valid = h->out_ncols > 0;
      h->snap_time = k.time;
      h->snap_step = k.step + 1;
    } else {
      k.n_time_out += 1;
    }
    k.time = k.time + c.dt;
    k.step += 1;
  }
}

// one launch of nsteps steps (two from split_blocks blocks up); with `sample` each part's launch is followed, on its own stream, by
// the sampling kernel of the tracks for that part's blocks
int launch_cut(samsim_handle *h, long long nsteps, bool sample) {
  if (nsteps <= 0) return SAMSIM_OK;
  // the forcing tables are read whenever atmoflux_flag is 2 (T2m / precipitation in every step, the radiative fluxes with
  // boundflux_flag 2): no launch without them, whatever the other flags say
  if (launch_needs_forcing(h->cfg) && (!h->f_sw || !h->f_lw || !h->f_T2m || !h->f_precip || h->flen < 2)) return SAMSIM_ERR_ARG;
  if (h->cfg.bgc_flag == 2 && h->n_bgc < 1) return SAMSIM_ERR_ARG;   // samsim_set_tracers first
  const long long nblk = (h->ncol + 63) / 64;
  // two parts from 8 192 blocks up (two rounds of the chip's 4 096 wave slots): below that a launch has no rounds to speak of
  const bool split = h->stream2 && h->split_blocks > 0 && nblk >= h->split_blocks && nblk >= 2;
  const int nparts = split ? 2 : 1;
  auto stream_of = [&](int part) { return part == 0 ? h->stream : h->stream2; };
  // part boundaries: the first part takes split_eighths/8 of the blocks
  auto bound = [&](int part) -> long long {
    if (part <= 0) return 0;
    if (part >= nparts) return nblk;
    return (nblk * h->split_eighths + 7) / 8;
  };
  if (split && h->other_work) {
    HIPCHK(hipEventRecord(h->fork, h->stream));
    HIPCHK(hipStreamWaitEvent(h->stream2, h->fork, 0));
  }
  h->other_work = false;
  for (int part = 0; part < nparts; ++part) {
    const long long b0 = bound(part), nb = bound(part + 1) - b0;
    if (nb <= 0) continue;
    hipStream_t st = stream_of(part);
    const int s = h->slot;
    h->slot = (h->slot + 1) % kRing;
    HIPCHK(hipEventSynchronize(h->slot_done[s]));
    DevParams &p = h->h_params[s];
    p.cfg = h->cfg;
    p.lay = h->lay; p.scal = h->scal; p.n_active = h->n_active; p.status = h->status; p.err_layer = h->err_layer;
    p.err_step = h->err_step; p.work = h->work;
    p.spec = h->spec; p.flags = h->flags;
    p.f_sw = h->f_sw; p.f_lw = h->f_lw; p.f_T2m = h->f_T2m; p.f_precip = h->f_precip; p.flen = h->flen;
    p.nsites = h->nsites; p.site = h->site;
    p.ocean_dflq = h->ocean_dflq; p.ocean_sbu = h->ocean_sbu;
    p.ncol = h->ncol;
    p.block0 = b0;
    p.time0 = h->clk.time; p.step0 = h->clk.step; p.n_time_out0 = h->clk.n_time_out; p.time_counter0 = h->clk.time_counter;
    p.nsteps = nsteps;
    p.out_lay = h->out_lay; p.out_scal = h->out_scal; p.out_n_active = h->out_n_active;
    p.out_col0 = h->out_col0; p.out_ncols = h->out_ncols;
    p.p17 = h->p17; p.p14 = h->p14; p.tf_c3 = h->tf_c3;
    p.bgc = h->bgc; p.bgc_bot = h->bgc_bot; p.bfl = h->bfl; p.out_bgc = h->out_bgc; p.out_bgc_bot = h->out_bgc_bot;
    p.n_bgc = h->n_bgc; p.bgc_total0 = h->bgc_total0;
    HIPCHK(hipMemcpyAsync(&h->d_params[s], &p, sizeof(DevParams), hipMemcpyHostToDevice, st));
    HIPCHK(samsim_launch_step(&h->d_params[s], &p, nb, st));
    HIPCHK(hipEventRecord(h->slot_done[s], st));
    if (sample) {
      // directly behind the step launch of the same blocks on the same stream: the columns of a part are independent of the other
      // part's, so the sample waits for nothing else
      TrackParams tp{};
      tp.lay = h->lay; tp.scal = h->scal; tp.n_active = h->n_active; tp.status = h->status; tp.flags = h->flags;
      tp.rows = h->tracks;
      tp.ncol = h->ncol; tp.block0 = b0;
      tp.step = (double)(h->clk.step + nsteps);
      tp.N = h->cfg.nlayer; tp.ntracks = h->ntracks;
      for (int t = 0; t < h->ntracks; ++t) {
        tp.t[t] = h->track[t];
        if (h->track[t].kind == SAMSIM_OBS_ICE_THICKNESS) tp.need_thick = 1;
        if (h->track[t].kind == SAMSIM_OBS_BULK_SALINITY) tp.need_salt = 1;
      }
      HIPCHK(samsim_launch_track_sample(&tp, nb, st));
    }
  }
  h->stepped = true;
  h->func_dirty = true;
  advance_clock(h, nsteps);
  return SAMSIM_OK;
}

// nsteps steps.  With tracks in force the call is cut at the sample points inside it (the steps that bring clk.step to a multiple
// of track_every): each cut ends a launch -- whose last step stores everything, so the sample reads current rows -- and is followed
// by the sample.  The run does not depend on where launches are cut, bit for bit.  Without tracks, or with no sample point inside
// the call, this is one launch_cut and the sequence of device calls is what it was before there were tracks.
int launch(samsim_handle *h, long long nsteps) {
  if (h->ntracks < 1) return launch_cut(h, nsteps, false);
  while (nsteps > 0) {
    const long long to_sample = h->track_every - h->clk.step % h->track_every;
    const long long n = nsteps < to_sample ? nsteps : to_sample;
    const int rc = launch_cut(h, n, n == to_sample);
    if (rc) return rc;
    nsteps -= n;
  }
  return SAMSIM_OK;
}

// a slot of the statistics: an enum samsim_scalar, SAMSIM_STAT_N_ACTIVE, SAMSIM_TRACK_SLOT(track, field) of the tracks in force, or
// SAMSIM_FUNC_SLOT(i) of the functionals in force, or SAMSIM_SCORE_SLOT(field) while sensors are set, or SAMSIM_WEIGHT_SLOT while the
// weight row exists, or SAMSIM_OFFSPRING_SLOT while the offspring row does, or SAMSIM_OCEAN_SLOT(i) while that row of samsim_set_ocean does
bool func_slot(int32_t slot) { return slot >= SAMSIM_FUNC_SLOT(0) && slot < SAMSIM_FUNC_SLOT(SAMSIM_MAX_FUNCTIONALS); }
bool score_slot(int32_t slot) { return slot >= SAMSIM_SCORE_SLOT(0) && slot < SAMSIM_SCORE_SLOT(SAMSIM_NSF); }
bool good_slot(const samsim_handle *h, int32_t slot) {
  if (slot == SAMSIM_STAT_N_ACTIVE || (slot >= 0 && slot < SAMSIM_NSCAL)) return true;
  if (func_slot(slot)) return h->func_rows && slot - SAMSIM_FUNC_SLOT(0) < h->nfunc;
  if (score_slot(slot)) return h->score_rows != nullptr;
  if (slot == SAMSIM_WEIGHT_SLOT) return h->weight_row != nullptr;
  if (slot == SAMSIM_OFFSPRING_SLOT) return h->offspring_row != nullptr;
  if (slot == SAMSIM_OCEAN_SLOT(0)) return h->ocean_dflq != nullptr;
  if (slot == SAMSIM_OCEAN_SLOT(1)) return h->ocean_sbu != nullptr;
  const int32_t o = slot - SAMSIM_TRACK_SLOT(0, 0);
  return h->tracks && o >= 0 && o / 32 < h->ntracks && o % 32 < SAMSIM_NTF;
}
// the [ncol] row of a good slot; null for SAMSIM_STAT_N_ACTIVE (the reductions then read n_active)
const double *slot_row(const samsim_handle *h, int32_t slot) {
  if (slot == SAMSIM_STAT_N_ACTIVE) return nullptr;
  if (slot < SAMSIM_NSCAL) return h->scal + (size_t)slot * (size_t)h->ncol;
  if (func_slot(slot)) return h->func_rows + (size_t)(slot - SAMSIM_FUNC_SLOT(0)) * (size_t)h->ncol;
  if (score_slot(slot)) return h->score_rows + (size_t)(slot - SAMSIM_SCORE_SLOT(0)) * (size_t)h->ncol;
  if (slot == SAMSIM_WEIGHT_SLOT) return h->weight_row;
  if (slot == SAMSIM_OFFSPRING_SLOT) return h->offspring_row;
  if (slot == SAMSIM_OCEAN_SLOT(0)) return h->ocean_dflq;
  if (slot == SAMSIM_OCEAN_SLOT(1)) return h->ocean_sbu;
  const int32_t o = slot - SAMSIM_TRACK_SLOT(0, 0);
  return h->tracks + ((size_t)(o / 32) * SAMSIM_NTF + (size_t)(o % 32)) * (size_t)h->ncol;
}

// every entry point but the stepping ones waits for the second stream and makes the next launch's second part wait for whatever
// it leaves on the first
int use(samsim_handle *h, bool stepping = false) {
  if (!h) return SAMSIM_ERR_ARG;
  HIPCHK(hipSetDevice(h->device));
  if (!stepping) {
    if (h->stream2) HIPCHK(hipStreamSynchronize(h->stream2));
    h->other_work = true;
  }
  return SAMSIM_OK;
}

// The rows an item on `array` needs and how its layer value is formed from them (column_read::layer_mode): its array; S_abs and m for
// S_bu once the kernel has run, as samsim_get_state then forms the quotient.  row_plan_place (samsim_row_plan.h) puts it into a walk.
template <int MAXG>
RowPlace plan_item(RowPlan<MAXG> &plan, int array, bool stepped, int32_t *mode) {
  *mode = array == SAMSIM_A_S_ABS ? column_read::LAYER_S_ABS : column_read::LAYER_PLAIN;
  if (array != SAMSIM_A_S_BU || !stepped) return row_plan_place(plan, array, -1);
  *mode = column_read::LAYER_S_BU;
  return row_plan_place(plan, SAMSIM_A_S_ABS, SAMSIM_A_M);
}

// func_plan and sensor_plan fill a Params struct that arrives zeroed (`FuncParams p{}`, `SensorParams p{}`): the plan starts from no
// group, and it has room for one group per item (nfunc <= SAMSIM_MAX_FUNCTIONALS, nsensors <= SAMSIM_MAX_SENSORS).
void func_plan(const samsim_handle *h, FuncParams *p) {
  for (int i = 0; i < h->nfunc; ++i) {
    const samsim_functional_spec &s = h->func[i];
    FuncDev &d = p->f[i];
    d = FuncDev{s.kind, s.origin, s.sense, 0, 0, 0, 0, 0, s.z_lo, s.z_hi, s.threshold, s.missing};
    const RowPlace at = plan_item(p->plan, s.array, h->stepped, &d.mode);
    d.group = at.group; d.ia = at.ia; d.ib = at.ib;
    if (s.origin == SAMSIM_PROFILE_FROM_BOTTOM) p->need_H = 1;
  }
}

void sensor_plan(const samsim_handle *h, SensorParams *p) {
  for (int i = 0; i < h->nsensors; ++i) {
    const samsim_sensor_spec &s = h->sensor[i];
    SensorDev &d = p->s[i];
    d = SensorDev{s.kind, s.id, s.origin, s.interp, 0, -1, 0, 0, s.z, s.missing};
    if (s.kind == SAMSIM_SENSOR_ICE_THICKNESS) p->need_H = 1;
    if (s.kind != SAMSIM_SENSOR_PROFILE) continue;
    if (s.origin == SAMSIM_PROFILE_FROM_BOTTOM) p->need_H = 1;
    const RowPlace at = plan_item(p->plan, s.id, h->stepped, &d.mode);
    d.group = at.group; d.ia = at.ia; d.ib = at.ib;
  }
}

// the rows of the functionals brought up to date, on the handle's first stream: one kernel, and only when the state changed since the
// last evaluation.  Called behind use() by samsim_get_functionals and by every consumer that was handed a SAMSIM_FUNC_SLOT.
int func_refresh(samsim_handle *h) {
  if (!h->func_rows || !h->func_dirty) return SAMSIM_OK;
  FuncParams p{};
  p.lay = h->lay; p.n_active = h->n_active; p.status = h->status; p.flags = h->flags;
  p.rows = h->func_rows;
  p.ncol = h->ncol; p.N = h->cfg.nlayer; p.nf = h->nfunc; p.stepped = h->stepped ? 1 : 0;
  func_plan(h, &p);
  HIPCHK(samsim_launch_functionals(&p, h->stream));
  h->func_dirty = false;
  return SAMSIM_OK;
}
int func_refresh_for(samsim_handle *h, int32_t nslots, const int32_t *slots) {
  for (int i = 0; i < nslots; ++i)
    if (func_slot(slots[i])) return func_refresh(h);
  return SAMSIM_OK;
}

// one group per call: -1 every column, else a label of samsim_set_groups
bool good_group(const samsim_handle *h, int32_t group) { return group == -1 || (group >= 0 && h->groups && group < h->ngroups); }
// the label row a reduction over `group` reads: none where every column counts
const int32_t *labels_for(const samsim_handle *h, int32_t group) { return group >= 0 ? h->groups : nullptr; }
// the columns a slot reduction over `group` ranges over (samsim_slot_walk.h)
slot_walk::ColSet col_set(const samsim_handle *h, int32_t group) {
  return slot_walk::ColSet{{h->n_active, h->status, labels_for(h, group)}, group, h->ncol};
}
// the columns a per-label reduction ranges over: every group of samsim_set_groups at once, or without labels one group of all
slot_walk::LabelSet label_set(const samsim_handle *h, bool by_group) {
  return slot_walk::LabelSet{{h->n_active, h->status, by_group ? h->groups : nullptr}, h->ncol};
}
// count, mean[nslots] and cov[nslots][nslots] of a covariance result (CovResult, WCovResult), copied from the device to the caller
template <class R>
int fetch_cov(samsim_handle *h, const R *d_out, int32_t nslots, R *res, int64_t *count, double *mean, double *cov) {
  HIPCHK(hipMemcpyAsync(res, d_out, sizeof(R), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *count = res->count;
  std::memcpy(mean, res->mean, sizeof(double) * (size_t)nslots);
  std::memcpy(cov, res->cov, sizeof(double) * (size_t)nslots * (size_t)nslots);
  return SAMSIM_OK;
}

// a scratch buffer of the handle: allocated by the first call that needs it and kept
hipError_t scratch(void **buf, size_t bytes) { return *buf ? hipSuccess : hipMalloc(buf, bytes); }

// What the reductions over a list of slots do between their null checks and their launch, in the order samsim.h gives: the checks
// of the list, of the weight row (weighted) and of the group -- nothing touches the device before the request is known to be
// good --, then use(), the functionals the list names brought up to date, and the rows of the slots.
int slot_rows(samsim_handle *h, int32_t nslots, const int32_t *slots, bool weighted, int32_t group, SensRows *rows) {
  if (nslots < 1 || nslots > SAMSIM_SENS_MAX_SLOTS) return SAMSIM_ERR_ARG;
  for (int i = 0; i < nslots; ++i)
    if (!good_slot(h, slots[i])) return SAMSIM_ERR_ARG;
  if (weighted && !h->weight_row) return SAMSIM_ERR_ARG;
  if (!good_group(h, group)) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  rc = func_refresh_for(h, nslots, slots);
  if (rc) return rc;
  for (int i = 0; i < nslots; ++i) rows->row[i] = slot_row(h, slots[i]);
  return SAMSIM_OK;
}

// The passes of a profile request, enqueued in order on the handle's stream: one per requested array and chunk of `chunk` bins
// (samsim_pass_plan.h), so a pass's merge has read the partials before the next pass writes them.  launch(pass, at) enqueues the
// family's pass; at = the place of the pass's first bin among the results [narrays][nbins] of the request.
template <class Launch>
int for_each_pass(const samsim_handle *h, const samsim_profile_request *rq, int32_t group, int chunk, Launch launch) {
  const bool depth = rq->axis == SAMSIM_PROFILE_BY_DEPTH;
  return pass_plan(rq->narrays, rq->nbins, chunk, rq->origin, [&](const PassSpan &s) -> int {
    ProfPass p;
    p.lay = h->lay; p.n_active = h->n_active; p.status = h->status; p.labels = labels_for(h, group);
    p.ncol = h->ncol; p.z0 = depth ? rq->z0 : 0.0; p.dz = depth ? rq->dz : 1.0;
    p.group = group; p.N = h->cfg.nlayer; p.axis = rq->axis; p.origin = rq->origin; p.array = rq->arrays[s.array];
    p.b0 = s.b0; p.nb = s.nb; p.lead = s.lead;
    HIPCHK(launch(p, (size_t)s.array * (size_t)rq->nbins + (size_t)s.b0));
    return SAMSIM_OK;
  });
}

}  // namespace

extern "C" {

int samsim_abi_version(void) { return SAMSIM_ABI_VERSION; }

int samsim_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *samsim_strerror(int code) {
  switch (code) {
    case SAMSIM_OK: return "ok";
    case SAMSIM_ERR_ARG: return "bad argument";
    case SAMSIM_ERR_UNSUPPORTED: return "flag value not supported by the HIP path";
    case SAMSIM_ERR_HIP: return g_last_hip_error[0] ? g_last_hip_error : "HIP error";
    case SAMSIM_ERR_NO_DEVICE: return "no HIP device";
    case SAMSIM_ERR_NO_OUTPUT: return "no output snapshot has been taken";
    case SAMSIM_ERR_ABI: return "samsim_config.struct_size does not match this library";
    case SAMSIM_ERR_NOMEM: return "out of memory";
  }
  return "unknown error";
}

int samsim_create(const samsim_config *cfg, int64_t ncol, int32_t device, samsim_handle **out) {
  if (!cfg || !out || ncol <= 0) return SAMSIM_ERR_ARG;
  int rc = validate(*cfg);
  if (rc) return rc;
  // The kernel reaches the [slot][ncol] blocks (per-column scalars, hand-over block of the up sweep) with a scalar base and a 32-bit
  // byte offset slot * ncol * 8 + col * 8 (GSI / SPEC in samsim_kernels.hip): the widest of them must stay below 4 GiB.  The layer
  // block has no such bound: it is stored per 64-column block, whose base is 64-bit arithmetic and whose rows (nlayer * 8 KiB) lie
  // within a 32-bit offset for any nlayer samsim_config admits.
  constexpr unsigned long long kRows = (int)SAMSIM_NSCAL > (int)DEV_NSPEC ? (int)SAMSIM_NSCAL : (int)DEV_NSPEC;
  if (kRows * (unsigned long long)ncol * 8ull >= (1ull << 32)) return SAMSIM_ERR_ARG;
  if (device < 0 || device >= samsim_device_count()) return SAMSIM_ERR_NO_DEVICE;
  HIPCHK(hipSetDevice(device));
  samsim_handle *h = new (std::nothrow) samsim_handle();
  if (!h) return SAMSIM_ERR_NOMEM;
  h->cfg = *cfg; h->ncol = ncol; h->device = device;
  h->clk = samsim_clock{0.0, 0, 0, 1, 0};
  h->p17 = std::pow(10.0, -17.0);
  h->p14 = std::pow(10.0, -14.0);
  h->tf_c3 = (double)(5.33f * std::pow(10.0f, -7.0f));
  const size_t N = (size_t)cfg->nlayer, nc = (size_t)ncol;
  bool ok = hip_ok(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking), "hipStreamCreate");
  ok = ok && hip_ok(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking), "hipStreamCreate");
  ok = ok && hip_ok(hipEventCreateWithFlags(&h->fork, hipEventDisableTiming), "hipEventCreate");
  ok = ok && hip_ok(hipEventCreate(&h->ev0b), "hipEventCreate") && hip_ok(hipEventCreate(&h->ev1b), "hipEventCreate");
  ok = ok && hip_ok(dalloc(&h->lay, DEV_LAY_DOUBLES(N, nc)), "hipMalloc lay");
  ok = ok && hip_ok(dalloc(&h->scal, (size_t)SAMSIM_NSCAL * nc), "hipMalloc scal");
  ok = ok && hip_ok(dalloc(&h->n_active, nc), "hipMalloc n_active");
  ok = ok && hip_ok(dalloc(&h->status, nc), "hipMalloc status");
  ok = ok && hip_ok(dalloc(&h->err_layer, nc), "hipMalloc err_layer");
  ok = ok && hip_ok(dalloc(&h->err_step, nc), "hipMalloc err_step");
  ok = ok && hip_ok(dalloc(&h->work, nc), "hipMalloc work");
  ok = ok && hip_ok(dalloc(&h->spec, (size_t)DEV_NSPEC * nc), "hipMalloc spec");
  ok = ok && hip_ok(dalloc(&h->flags, nc), "hipMalloc flags");
  ok = ok && hip_ok(dalloc(&h->d_params, (size_t)kRing), "hipMalloc params");
  ok = ok && hip_ok(hipHostMalloc((void **)&h->h_params, sizeof(DevParams) * kRing, hipHostMallocDefault), "hipHostMalloc params");
  for (int i = 0; ok && i < kRing; ++i) ok = hip_ok(hipEventCreateWithFlags(&h->slot_done[i], hipEventDisableTiming), "hipEventCreate");
  ok = ok && hip_ok(hipEventCreate(&h->ev0), "hipEventCreate") && hip_ok(hipEventCreate(&h->ev1), "hipEventCreate");
  if (ok) {
    // sub_allocate zeros (mo_init.f90:2081-2087) and the defaults of mo_init.f90:1982-1990
    ok = hip_ok(hipMemsetAsync(h->lay, 0, sizeof(double) * DEV_LAY_DOUBLES(N, nc), h->stream), "memset lay");
    ok = ok && hip_ok(hipMemsetAsync(h->scal, 0, sizeof(double) * SAMSIM_NSCAL * nc, h->stream), "memset scal");
    ok = ok && hip_ok(hipMemsetAsync(h->status, 0, sizeof(int32_t) * nc, h->stream), "memset");
    ok = ok && hip_ok(hipMemsetAsync(h->err_layer, 0, sizeof(int32_t) * nc, h->stream), "memset");
    ok = ok && hip_ok(hipMemsetAsync(h->err_step, 0, sizeof(long long) * nc, h->stream), "memset");
    ok = ok && hip_ok(hipMemsetAsync(h->work, 0, sizeof(long long) * nc, h->stream), "memset");
    ok = ok && hip_ok(hipMemsetAsync(h->spec, 0, sizeof(double) * DEV_NSPEC * nc, h->stream), "memset");
    if (ok) {
      const unsigned fg = (unsigned)((N * nc + 255) / 256);
      hipLaunchKernelGGL(lay_fill_array, dim3(fg), dim3(256), 0, h->stream, h->lay, (int)SAMSIM_A_T, (int)N, nc, cfg->T_bottom);
      hipLaunchKernelGGL(lay_fill_array, dim3(fg), dim3(256), 0, h->stream, h->lay, (int)SAMSIM_A_S_BU, (int)N, nc, cfg->S_bu_bottom);
      hipLaunchKernelGGL(lay_fill_array, dim3(fg), dim3(256), 0, h->stream, h->lay, (int)SAMSIM_A_PSI_L, (int)N, nc, 1.0);
      ok = hip_ok(hipGetLastError(), "fill layer arrays");
    }
    ok = ok && hip_ok(fill(h->scal + (size_t)SAMSIM_S_PRECIP_SCALE * nc, nc, 1.0, h->stream), "fill precip_scale");
    ok = ok && hip_ok(fill(h->scal + (size_t)SAMSIM_S_S_BU_BOTTOM * nc, nc, cfg->S_bu_bottom, h->stream), "fill S_bu_bottom");
    if (ok) {
      hipLaunchKernelGGL(fill_i32, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, h->stream, h->n_active, nc, 1);
      hipLaunchKernelGGL(fill_i32, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, h->stream, h->flags, nc,
                         COLF_DIRTY | COLF_RESTART);
      ok = hip_ok(hipGetLastError(), "fill n_active/flags");
    }
    ok = ok && hip_ok(hipStreamSynchronize(h->stream), "sync");
  }
  if (!ok) { samsim_destroy(h); return SAMSIM_ERR_HIP; }
  rc = samsim_set_output_window(h, 0, 1);
  if (rc) { samsim_destroy(h); return rc; }
  *out = h;
  return SAMSIM_OK;
}

void samsim_destroy(samsim_handle *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream2) (void)hipStreamSynchronize(h->stream2);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  (void)hipFree(h->lay); (void)hipFree(h->scal); (void)hipFree(h->n_active); (void)hipFree(h->status);
  (void)hipFree(h->err_layer); (void)hipFree(h->err_step); (void)hipFree(h->work);
  (void)hipFree(h->spec); (void)hipFree(h->flags); (void)hipFree(h->d_stat); (void)hipFree(h->d_prof); (void)hipFree(h->stage);
  (void)hipFree(h->groups); (void)hipFree(h->d_group); (void)hipFree(h->d_hist); (void)hipFree(h->d_sens); (void)hipFree(h->tracks);
  (void)hipFree(h->func_rows);
  (void)hipFree(h->score_rows);
  (void)hipFree(h->weight_row); (void)hipFree(h->d_weight); (void)hipFree(h->d_wprof); (void)hipFree(h->d_wphist);
  (void)hipFree(h->offspring_row); (void)hipFree(h->ancestors); (void)hipFree(h->d_resample);
  (void)hipFree(h->copy_src); (void)hipFree(h->copy_dst); (void)hipFree(h->plan_src); (void)hipFree(h->plan_dst); (void)hipFree(h->d_copy);
  (void)hipFree(h->d_jitter);
  (void)hipFree(h->d_select);
  (void)hipFree(h->bgc); (void)hipFree(h->bgc_bot); (void)hipFree(h->bfl); (void)hipFree(h->out_bgc); (void)hipFree(h->out_bgc_bot);
  (void)hipFree(h->f_sw); (void)hipFree(h->f_lw); (void)hipFree(h->f_T2m); (void)hipFree(h->f_precip); (void)hipFree(h->site);
  (void)hipFree(h->ocean_dflq); (void)hipFree(h->ocean_sbu);
  (void)hipFree(h->out_lay); (void)hipFree(h->out_scal); (void)hipFree(h->out_n_active);
  (void)hipFree(h->d_params);
  if (h->h_params) (void)hipHostFree(h->h_params);
  for (int i = 0; i < kRing; ++i) if (h->slot_done[i]) (void)hipEventDestroy(h->slot_done[i]);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->fork) (void)hipEventDestroy(h->fork);
  if (h->ev0b) (void)hipEventDestroy(h->ev0b);
  if (h->ev1b) (void)hipEventDestroy(h->ev1b);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int samsim_set_forcing(samsim_handle *h, int32_t len, const double *fl_sw, const double *fl_lw, const double *T2m,
                       const double *precip, const double *dT2m_col, const double *precip_scale_col) {
  return samsim_set_forcing_sites(h, 1, len, fl_sw, fl_lw, T2m, precip, nullptr, dT2m_col, precip_scale_col);
}

int samsim_set_forcing_sites(samsim_handle *h, int32_t nsites, int32_t len, const double *fl_sw, const double *fl_lw,
                             const double *T2m, const double *precip, const int32_t *site_of_column,
                             const double *dT2m_col, const double *precip_scale_col) {
  int rc = use(h);
  if (rc) return rc;
  if (len < 2 || nsites < 1 || !fl_sw || !fl_lw || !T2m || !precip || (nsites > 1 && !site_of_column)) return SAMSIM_ERR_ARG;
  for (long long c = 0; nsites > 1 && c < h->ncol; ++c)
    if (site_of_column[c] < 0 || site_of_column[c] >= nsites) return SAMSIM_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->stream));
  (void)hipFree(h->f_sw); (void)hipFree(h->f_lw); (void)hipFree(h->f_T2m); (void)hipFree(h->f_precip); (void)hipFree(h->site);
  h->f_sw = h->f_lw = h->f_T2m = h->f_precip = nullptr; h->site = nullptr;
  const size_t bytes = sizeof(double) * (size_t)len * (size_t)nsites;
  HIPCHK(dalloc(&h->f_sw, (size_t)len * nsites)); HIPCHK(dalloc(&h->f_lw, (size_t)len * nsites));
  HIPCHK(dalloc(&h->f_T2m, (size_t)len * nsites)); HIPCHK(dalloc(&h->f_precip, (size_t)len * nsites));
  h->nsites = nsites;
  if (nsites > 1) {
    HIPCHK(dalloc(&h->site, (size_t)h->ncol));
    HIPCHK(hipMemcpy(h->site, site_of_column, sizeof(int32_t) * (size_t)h->ncol, hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemcpy(h->f_sw, fl_sw, bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->f_lw, fl_lw, bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->f_T2m, T2m, bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->f_precip, precip, bytes, hipMemcpyHostToDevice));
  h->flen = len;
  const size_t nc = (size_t)h->ncol;
  if (dT2m_col) HIPCHK(hipMemcpy(h->scal + (size_t)SAMSIM_S_DT2M * nc, dT2m_col, sizeof(double) * nc, hipMemcpyHostToDevice));
  else HIPCHK(hipMemset(h->scal + (size_t)SAMSIM_S_DT2M * nc, 0, sizeof(double) * nc));
  if (precip_scale_col) {
    HIPCHK(hipMemcpy(h->scal + (size_t)SAMSIM_S_PRECIP_SCALE * nc, precip_scale_col, sizeof(double) * nc, hipMemcpyHostToDevice));
  } else {
    HIPCHK(fill(h->scal + (size_t)SAMSIM_S_PRECIP_SCALE * nc, nc, 1.0, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return SAMSIM_OK;
}

int samsim_set_ocean(samsim_handle *h, const double *dfl_q_bottom_col, const double *S_bu_bottom_col) {
  int rc = use(h);
  if (rc) return rc;
  // the offset rides on the flux sub_test4 sets every step; the salinity replaces cfg.S_bu_bottom, which the tank budget owns with tank_flag 2
  if (dfl_q_bottom_col && h->cfg.testcase != 4 && h->cfg.testcase != 7) return SAMSIM_ERR_UNSUPPORTED;
  if (S_bu_bottom_col && h->cfg.tank_flag == 2) return SAMSIM_ERR_UNSUPPORTED;
  const size_t nc = (size_t)h->ncol;
  for (size_t i = 0; S_bu_bottom_col && i < nc; ++i) if (!(S_bu_bottom_col[i] >= 0.0)) return SAMSIM_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->stream));
  // the new arrays are complete on the device before the handle sees them: a call that fails leaves the handle as it was
  double *dq = nullptr, *sb = nullptr;
  bool ok = true;
  if (dfl_q_bottom_col)
    ok = hip_ok(dalloc(&dq, nc), "hipMalloc ocean_dflq") &&
         hip_ok(hipMemcpy(dq, dfl_q_bottom_col, sizeof(double) * nc, hipMemcpyHostToDevice), "hipMemcpy ocean_dflq");
  if (ok && S_bu_bottom_col)
    ok = hip_ok(dalloc(&sb, nc), "hipMalloc ocean_sbu") &&
         hip_ok(hipMemcpy(sb, S_bu_bottom_col, sizeof(double) * nc, hipMemcpyHostToDevice), "hipMemcpy ocean_sbu");
  if (!ok) { (void)hipFree(dq); (void)hipFree(sb); return SAMSIM_ERR_HIP; }
  (void)hipFree(h->ocean_dflq); (void)hipFree(h->ocean_sbu);
  h->ocean_dflq = dq; h->ocean_sbu = sb;
  return SAMSIM_OK;
}

static int check_soa(samsim_handle *h, const samsim_state_soa *s, int64_t col0) {
  if (!s || !s->lay || !s->scal || !s->n_active) return SAMSIM_ERR_ARG;
  if (s->nlayer != h->cfg.nlayer || s->ncol <= 0 || col0 < 0 || col0 + s->ncol > h->ncol) return SAMSIM_ERR_ARG;
  if (s->narr != SAMSIM_NPROG && s->narr != SAMSIM_NARR) return SAMSIM_ERR_ARG;
  return SAMSIM_OK;
}

int samsim_set_state(samsim_handle *h, const samsim_state_soa *s, int64_t col0) {
  int rc = use(h);
  if (rc) return rc;
  rc = check_soa(h, s, col0);
  if (rc) return rc;
  const size_t N = (size_t)s->nlayer, nc = (size_t)h->ncol, w = (size_t)s->ncol;
  for (size_t i = 0; i < w; ++i) if (s->n_active[i] < 1 || s->n_active[i] > (int)N) return SAMSIM_ERR_ARG;
  h->func_dirty = true;
  HIPCHK(hipStreamSynchronize(h->stream));
  // the window in pieces of at most stage_cols columns: rows [narr][N] of the piece's columns are gathered from the caller's
  // [narr][N][w] into the staging buffer by one 2D copy, then scattered into the device layout
  const size_t pc = stage_cols(s->narr, N), rows = (size_t)s->narr * N;
  HIPCHK(stage_for(h, rows * (w < pc ? w : pc)));
  for (size_t p0 = 0; p0 < w; p0 += pc) {
    const size_t pw = w - p0 < pc ? w - p0 : pc, n = rows * pw;
    HIPCHK(copy_rows(h->stage, pw, s->lay + p0, w, pw, rows, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(lay_window<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->lay, h->stage, (int)s->narr, (int)N, nc,
                       (size_t)col0 + p0, pw);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  // the perturbation slots (>= SAMSIM_S_DT2M) belong to the forcing: set_state leaves them alone
  HIPCHK(hipMemcpy2D(h->scal + col0, nc * sizeof(double), s->scal, w * sizeof(double), w * sizeof(double), (size_t)SAMSIM_S_DT2M,
                     hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->n_active + col0, s->n_active, w * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(h->status + col0, 0, w * sizeof(int32_t)));
  // the next step of these columns runs the full first sweep and treats RAY as the previous step's Rayleigh numbers
  hipLaunchKernelGGL(fill_i32, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, h->stream, h->flags + col0, w,
                     COLF_DIRTY | COLF_RESTART);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_get_state(samsim_handle *h, samsim_state_soa *s, int64_t col0) {
  int rc = use(h);
  if (rc) return rc;
  rc = check_soa(h, s, col0);
  if (rc) return rc;
  const size_t N = (size_t)s->nlayer, nc = (size_t)h->ncol, w = (size_t)s->ncol;
  if (h->stepped) {
    hipLaunchKernelGGL(clamp_s_abs, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, h->stream, h->lay, h->n_active, h->status, h->flags,
                       nc, (int)N, (size_t)col0, w);
    HIPCHK(hipGetLastError());
  }
  if (s->narr == SAMSIM_NARR && h->stepped) {
    hipLaunchKernelGGL(refresh_s_bu, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, h->stream, h->lay, h->n_active, h->status, h->flags,
                       nc, (int)N, (size_t)col0, w);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t pc = stage_cols(s->narr, N), rows = (size_t)s->narr * N;   // pieces as in samsim_set_state
  HIPCHK(stage_for(h, rows * (w < pc ? w : pc)));
  for (size_t p0 = 0; p0 < w; p0 += pc) {
    const size_t pw = w - p0 < pc ? w - p0 : pc, n = rows * pw;
    hipLaunchKernelGGL(lay_window<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->lay, h->stage, (int)s->narr, (int)N, nc,
                       (size_t)col0 + p0, pw);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_rows(s->lay + p0, w, h->stage, pw, pw, rows, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  HIPCHK(hipMemcpy2D(s->scal, w * sizeof(double), h->scal + col0, nc * sizeof(double), w * sizeof(double), (size_t)SAMSIM_NSCAL,
                     hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(s->n_active, h->n_active + col0, w * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

int samsim_set_clock(samsim_handle *h, const samsim_clock *c) {
  if (!h || !c || c->time_counter < 1 || c->step < 0) return SAMSIM_ERR_ARG;
  h->clk = *c;
  return SAMSIM_OK;
}

int samsim_get_clock(samsim_handle *h, samsim_clock *c) {
  if (!h || !c) return SAMSIM_ERR_ARG;
  *c = h->clk;
  return SAMSIM_OK;
}

int samsim_step(samsim_handle *h, int64_t nsteps) {
  int rc = use(h, true);
  if (rc) return rc;
  if (nsteps < 0) return SAMSIM_ERR_ARG;
  return launch(h, nsteps);
}

int samsim_steps_timed(samsim_handle *h, int64_t nsteps, int32_t nlaunches, double *device_ms) {
  int rc = use(h);   // (waits for the second stream: the timed region starts with both streams idle or ordered behind ev0)
  if (rc) return rc;
  if (nsteps < 0 || nlaunches < 1 || !device_ms) return SAMSIM_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  for (int32_t i = 0; i < nlaunches; ++i) {
    rc = launch(h, nsteps);
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(hipEventRecord(h->ev1b, h->stream2));
  HIPCHK(hipEventSynchronize(h->ev1));
  HIPCHK(hipEventSynchronize(h->ev1b));
  float ms = 0.f, msb = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  HIPCHK(hipEventElapsedTime(&msb, h->ev0, h->ev1b));   // (the other streams' first launches are ordered behind ev0 by the fork event)
  if (msb > ms) ms = msb;
  *device_ms = (double)ms;
  return SAMSIM_OK;
}

int samsim_step_timed(samsim_handle *h, int64_t nsteps, double *kernel_ms) { return samsim_steps_timed(h, nsteps, 1, kernel_ms); }

int samsim_get_device(samsim_handle *h, int32_t *device, char *pci_bus_id, int32_t len) {
  if (!h) return SAMSIM_ERR_ARG;
  if (device) *device = h->device;
  if (pci_bus_id && len > 0) HIPCHK(hipDeviceGetPCIBusId(pci_bus_id, len, h->device));
  return SAMSIM_OK;
}

int samsim_set_launch_split(samsim_handle *h, int64_t min_blocks, int32_t first_part_eighths) {
  int rc = use(h);
  if (rc) return rc;
  if (min_blocks < 0 || first_part_eighths < 1 || first_part_eighths > 7) return SAMSIM_ERR_ARG;
  h->split_blocks = min_blocks;
  h->split_eighths = first_part_eighths;
  return SAMSIM_OK;
}

int samsim_synchronize(samsim_handle *h) {
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int64_t samsim_steps_to_output(samsim_handle *h) {
  if (!h) return 0;
  if (h->clk.step == 0) return 1;
  return (int64_t)(h->cfg.i_time_out - h->clk.n_time_out) + 1;
}

int samsim_set_output_window(samsim_handle *h, int64_t col0, int64_t ncols) {
  int rc = use(h);
  if (rc) return rc;
  if (col0 < 0 || ncols < 0 || col0 + ncols > h->ncol) return SAMSIM_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->stream));
  (void)hipFree(h->out_lay); (void)hipFree(h->out_scal); (void)hipFree(h->out_n_active);
  h->out_lay = h->out_scal = nullptr; h->out_n_active = nullptr;
  h->out_col0 = col0; h->out_ncols = ncols; h->snap_valid = false;
  if (ncols > 0) {
    const size_t N = (size_t)h->cfg.nlayer, w = (size_t)ncols;
    HIPCHK(dalloc(&h->out_lay, (size_t)SAMSIM_NARR * N * w));
    HIPCHK(dalloc(&h->out_scal, (size_t)SAMSIM_NSCAL * w));
    HIPCHK(dalloc(&h->out_n_active, w));
    HIPCHK(hipMemset(h->out_lay, 0, sizeof(double) * SAMSIM_NARR * N * w));
    HIPCHK(hipMemset(h->out_scal, 0, sizeof(double) * SAMSIM_NSCAL * w));
    HIPCHK(hipMemset(h->out_n_active, 0, sizeof(int32_t) * w));
  }
  if (h->n_bgc > 0) {  // tracer snapshot follows the window
    (void)hipFree(h->out_bgc); (void)hipFree(h->out_bgc_bot);
    h->out_bgc = h->out_bgc_bot = nullptr;
    const size_t N = (size_t)h->cfg.nlayer, w = (size_t)(ncols > 0 ? ncols : 1);
    HIPCHK(dalloc(&h->out_bgc, (size_t)h->n_bgc * N * w));
    HIPCHK(dalloc(&h->out_bgc_bot, (size_t)h->n_bgc * w));
    HIPCHK(hipMemset(h->out_bgc, 0, sizeof(double) * (size_t)h->n_bgc * N * w));
    HIPCHK(hipMemset(h->out_bgc_bot, 0, sizeof(double) * (size_t)h->n_bgc * w));
  }
  return SAMSIM_OK;
}

int samsim_get_output(samsim_handle *h, samsim_output_soa *o) {
  int rc = use(h);
  if (rc) return rc;
  if (!o || !o->lay || !o->scal || !o->n_active || o->ncols != h->out_ncols || o->nlayer != h->cfg.nlayer) return SAMSIM_ERR_ARG;
  if (!h->snap_valid || h->out_ncols == 0) return SAMSIM_ERR_NO_OUTPUT;
  const size_t N = (size_t)o->nlayer, w = (size_t)o->ncols;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(o->lay, h->out_lay, sizeof(double) * SAMSIM_NARR * N * w, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(o->scal, h->out_scal, sizeof(double) * SAMSIM_NSCAL * w, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(o->n_active, h->out_n_active, sizeof(int32_t) * w, hipMemcpyDeviceToHost));
  o->time = h->snap_time;
  o->step = h->snap_step;
  return SAMSIM_OK;
}

int samsim_get_status(samsim_handle *h, int32_t *status, int64_t *step, int32_t *layer) {
  int rc = use(h);
  if (rc) return rc;
  const size_t nc = (size_t)h->ncol;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (status) HIPCHK(hipMemcpy(status, h->status, sizeof(int32_t) * nc, hipMemcpyDeviceToHost));
  if (step) HIPCHK(hipMemcpy(step, h->err_step, sizeof(long long) * nc, hipMemcpyDeviceToHost));
  if (layer) HIPCHK(hipMemcpy(layer, h->err_layer, sizeof(int32_t) * nc, hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

int samsim_set_status(samsim_handle *h, const int32_t *status, const int64_t *step, const int32_t *layer, int64_t col0, int64_t ncols) {
  int rc = use(h);
  if (rc) return rc;
  if (!status || col0 < 0 || ncols < 0 || col0 + ncols > h->ncol) return SAMSIM_ERR_ARG;
  h->func_dirty = true;
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t w = (size_t)ncols;
  HIPCHK(hipMemcpy(h->status + col0, status, sizeof(int32_t) * w, hipMemcpyHostToDevice));
  if (step) HIPCHK(hipMemcpy(h->err_step + col0, step, sizeof(long long) * w, hipMemcpyHostToDevice));
  if (layer) HIPCHK(hipMemcpy(h->err_layer + col0, layer, sizeof(int32_t) * w, hipMemcpyHostToDevice));
  return SAMSIM_OK;
}

int samsim_get_work(samsim_handle *h, int64_t *layer_cell_updates, int64_t *column_steps) {
  int rc = use(h);
  if (rc) return rc;
  const size_t nc = (size_t)h->ncol;
  HIPCHK(hipStreamSynchronize(h->stream));
  std::vector<long long> w;
  try { w.resize(nc); } catch (const std::bad_alloc &) { return SAMSIM_ERR_NOMEM; }
  HIPCHK(hipMemcpy(w.data(), h->work, sizeof(long long) * nc, hipMemcpyDeviceToHost));
  long long tot = 0;
  for (size_t i = 0; i < nc; ++i) tot += w[i];
  if (layer_cell_updates) *layer_cell_updates = tot;
  if (column_steps) *column_steps = (int64_t)h->clk.step * (int64_t)h->ncol;
  return SAMSIM_OK;
}

// ---- passive tracers
int samsim_set_tracers(samsim_handle *h, int32_t n_bgc, const double *bgc_bottom, const double *bgc_total) {
  int rc = use(h);
  if (rc) return rc;
  if (h->cfg.bgc_flag != 2 || n_bgc < 1 || n_bgc > SAMSIM_MAX_NBGC || !bgc_bottom) return SAMSIM_ERR_ARG;
  if (h->cfg.tank_flag == 2 && !bgc_total) return SAMSIM_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t N = (size_t)h->cfg.nlayer, nc = (size_t)h->ncol, w = (size_t)(h->out_ncols > 0 ? h->out_ncols : 1);
  if (n_bgc != h->n_bgc) {
    (void)hipFree(h->bgc); (void)hipFree(h->bgc_bot); (void)hipFree(h->bfl); (void)hipFree(h->out_bgc); (void)hipFree(h->out_bgc_bot);
    h->bgc = h->bgc_bot = h->bfl = h->out_bgc = h->out_bgc_bot = nullptr;
    HIPCHK(dalloc(&h->bgc, (size_t)n_bgc * N * nc));
    HIPCHK(dalloc(&h->bgc_bot, (size_t)n_bgc * nc));
    HIPCHK(dalloc(&h->bfl, (size_t)BFL_NROW * N * nc));
    HIPCHK(dalloc(&h->out_bgc, (size_t)n_bgc * N * w));
    HIPCHK(dalloc(&h->out_bgc_bot, (size_t)n_bgc * w));
    HIPCHK(hipMemsetAsync(h->bgc, 0, sizeof(double) * (size_t)n_bgc * N * nc, h->stream));
    HIPCHK(hipMemsetAsync(h->out_bgc, 0, sizeof(double) * (size_t)n_bgc * N * w, h->stream));
    HIPCHK(hipMemsetAsync(h->out_bgc_bot, 0, sizeof(double) * (size_t)n_bgc * w, h->stream));
    h->n_bgc = n_bgc;
  }
  HIPCHK(hipMemsetAsync(h->bfl, 0, sizeof(double) * (size_t)BFL_NROW * N * nc, h->stream));
  for (int t = 0; t < n_bgc; ++t) HIPCHK(fill(h->bgc_bot + (size_t)t * nc, nc, bgc_bottom[t], h->stream));
  h->bgc_total0 = bgc_total ? bgc_total[0] : 0.0;
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_set_tracer_state(samsim_handle *h, const double *bgc_abs, int64_t col0, int64_t ncols) {
  int rc = use(h);
  if (rc) return rc;
  if (!bgc_abs || h->n_bgc < 1 || col0 < 0 || ncols < 0 || col0 + ncols > h->ncol) return SAMSIM_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t N = (size_t)h->cfg.nlayer, nc = (size_t)h->ncol, w = (size_t)ncols;
  HIPCHK(hipMemcpy2D(h->bgc + col0, nc * sizeof(double), bgc_abs, w * sizeof(double), w * sizeof(double), (size_t)h->n_bgc * N,
                     hipMemcpyHostToDevice));
  return SAMSIM_OK;
}

int samsim_set_tracer_bottom(samsim_handle *h, const double *bgc_bottom, int64_t col0, int64_t ncols) {
  int rc = use(h);
  if (rc) return rc;
  if (!bgc_bottom || h->n_bgc < 1 || col0 < 0 || ncols < 0 || col0 + ncols > h->ncol) return SAMSIM_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t nc = (size_t)h->ncol, w = (size_t)ncols;
  HIPCHK(hipMemcpy2D(h->bgc_bot + col0, nc * sizeof(double), bgc_bottom, w * sizeof(double), w * sizeof(double), (size_t)h->n_bgc,
                     hipMemcpyHostToDevice));
  return SAMSIM_OK;
}

int samsim_get_tracer_state(samsim_handle *h, double *bgc_abs, double *bgc_bottom, int64_t col0, int64_t ncols) {
  int rc = use(h);
  if (rc) return rc;
  if (!bgc_abs || h->n_bgc < 1 || col0 < 0 || ncols < 0 || col0 + ncols > h->ncol) return SAMSIM_ERR_ARG;
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t N = (size_t)h->cfg.nlayer, nc = (size_t)h->ncol, w = (size_t)ncols;
  HIPCHK(hipMemcpy2D(bgc_abs, w * sizeof(double), h->bgc + col0, nc * sizeof(double), w * sizeof(double), (size_t)h->n_bgc * N,
                     hipMemcpyDeviceToHost));
  if (bgc_bottom)
    HIPCHK(hipMemcpy2D(bgc_bottom, w * sizeof(double), h->bgc_bot + col0, nc * sizeof(double), w * sizeof(double), (size_t)h->n_bgc,
                       hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

int samsim_get_tracer_output(samsim_handle *h, double *bgc_abs, double *bgc_bottom) {
  int rc = use(h);
  if (rc) return rc;
  if (!bgc_abs || h->n_bgc < 1) return SAMSIM_ERR_ARG;
  if (!h->snap_valid) return SAMSIM_ERR_NO_OUTPUT;
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t N = (size_t)h->cfg.nlayer, w = (size_t)h->out_ncols;
  HIPCHK(hipMemcpy(bgc_abs, h->out_bgc, sizeof(double) * (size_t)h->n_bgc * N * w, hipMemcpyDeviceToHost));
  if (bgc_bottom) HIPCHK(hipMemcpy(bgc_bottom, h->out_bgc_bot, sizeof(double) * (size_t)h->n_bgc * w, hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

int samsim_get_ensemble_stats(samsim_handle *h, int32_t nslots, const int32_t *slots, samsim_stat *out) {
  int rc = use(h);
  if (rc) return rc;
  if (nslots < 0 || (nslots > 0 && (!slots || !out))) return SAMSIM_ERR_ARG;
  for (int i = 0; i < nslots; ++i)
    if (!good_slot(h, slots[i])) return SAMSIM_ERR_ARG;
  rc = func_refresh_for(h, nslots, slots);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_stat, sizeof(StatPartial) * kStatGrid));
  StatPartial *d_part = (StatPartial *)h->d_stat;
  std::vector<StatPartial> part(kStatGrid);
  const long long nc = h->ncol;
  for (int i = 0; i < nslots; ++i) {
    const double *row = slot_row(h, slots[i]);
    hipLaunchKernelGGL(stat_kernel<false>, dim3(kStatGrid), dim3(kStatBlock), 0, h->stream, row, h->n_active, h->status, nc, 0.0,
                       d_part);
    HIPCHK(hipMemcpyAsync(part.data(), d_part, sizeof(StatPartial) * kStatGrid, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    samsim_stat st{0, 0.0, 1.0e300, -1.0e300, 0.0};
    double sum = 0.0;
    for (const StatPartial &q : part) {
      st.count += q.n; sum += q.sum;
      st.min = q.mn < st.min ? q.mn : st.min;
      st.max = q.mx > st.max ? q.mx : st.max;
    }
    if (st.count > 0) {
      st.mean = sum / (double)st.count;
      hipLaunchKernelGGL(stat_kernel<true>, dim3(kStatGrid), dim3(kStatBlock), 0, h->stream, row, h->n_active, h->status, nc,
                         st.mean, d_part);
      HIPCHK(hipMemcpyAsync(part.data(), d_part, sizeof(StatPartial) * kStatGrid, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      double ssq = 0.0;
      for (const StatPartial &q : part) ssq += q.ssq;
      st.std = sqrt(ssq / (double)st.count);
    } else {
      st.min = st.max = 0.0;
    }
    out[i] = st;
  }
  return SAMSIM_OK;
}

// the checks of a profile request, in the order samsim.h gives (h and rq are not null)
static int check_profile_request(const samsim_handle *h, const samsim_profile_request *rq) {
  if (rq->struct_size != (int32_t)sizeof(samsim_profile_request)) return SAMSIM_ERR_ABI;
  const bool depth = rq->axis == SAMSIM_PROFILE_BY_DEPTH;
  if (!depth && rq->axis != SAMSIM_PROFILE_BY_LAYER) return SAMSIM_ERR_ARG;
  if (rq->origin != SAMSIM_PROFILE_FROM_TOP && rq->origin != SAMSIM_PROFILE_FROM_BOTTOM) return SAMSIM_ERR_ARG;
  if (rq->nbins < 1 || rq->nbins > SAMSIM_PROFILE_MAX_BINS || (!depth && rq->nbins > h->cfg.nlayer)) return SAMSIM_ERR_ARG;
  if (rq->narrays < 1 || rq->narrays > SAMSIM_PROFILE_MAX_ARRAYS) return SAMSIM_ERR_ARG;
  for (int i = 0; i < rq->narrays; ++i)
    if (rq->arrays[i] < 0 || rq->arrays[i] >= SAMSIM_NARR) return SAMSIM_ERR_ARG;
  if (depth && (!std::isfinite(rq->z0) || !std::isfinite(rq->dz) || rq->z0 < 0.0 || !(rq->dz > 0.0))) return SAMSIM_ERR_ARG;
  return SAMSIM_OK;
}

// samsim_get_profile_stats over every column (labels null) or over the columns with label `group` (samsim_get_group_profile_stats)
static int profile_stats(samsim_handle *h, const samsim_profile_request *rq, bool grouped, int32_t group, samsim_stat *out) {
  // every check of the request first: nothing below touches the device before the request is known to be good
  if (!h || !rq || !out) return SAMSIM_ERR_ARG;
  int rc = check_profile_request(h, rq);
  if (rc) return rc;
  if (grouped && (!h->groups || group < 0 || group >= h->ngroups)) return SAMSIM_ERR_ARG;
  rc = use(h);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_prof, kProfScratch));
  ProfPartial *d_part = (ProfPartial *)h->d_prof;
  samsim_stat *d_out = (samsim_stat *)((char *)h->d_prof + kProfPartBytes);
  rc = for_each_pass(h, rq, grouped ? group : -1, DEV_PROF_BINS,
                     [&](const ProfPass &p, size_t at) { return samsim_launch_profile(p, d_part, d_out + at, h->stream); });
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(out, d_out, sizeof(samsim_stat) * (size_t)rq->narrays * (size_t)rq->nbins, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_get_profile_stats(samsim_handle *h, const samsim_profile_request *rq, samsim_stat *out) {
  return profile_stats(h, rq, false, 0, out);
}

int samsim_get_group_profile_stats(samsim_handle *h, const samsim_profile_request *rq, int32_t group, samsim_stat *out) {
  return profile_stats(h, rq, true, group, out);
}

int samsim_set_groups(samsim_handle *h, int32_t ngroups, const int32_t *group_of_column) {
  // every check first: a call that is refused leaves the previous labels in force
  if (!h) return SAMSIM_ERR_ARG;
  const bool clear = ngroups == 0 && !group_of_column;
  if (!clear) {
    if (ngroups < 1 || ngroups > SAMSIM_MAX_GROUPS || !group_of_column) return SAMSIM_ERR_ARG;
    for (long long c = 0; c < h->ncol; ++c)
      if (group_of_column[c] < -1 || group_of_column[c] >= ngroups) return SAMSIM_ERR_ARG;
  }
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  // the new labels are complete on the device before the handle sees them
  int32_t *g = nullptr;
  if (!clear) {
    const bool ok = hip_ok(dalloc(&g, (size_t)h->ncol), "hipMalloc groups") &&
                    hip_ok(hipMemcpy(g, group_of_column, sizeof(int32_t) * (size_t)h->ncol, hipMemcpyHostToDevice), "hipMemcpy groups");
    if (!ok) { (void)hipFree(g); return SAMSIM_ERR_HIP; }
  }
  (void)hipFree(h->groups);
  h->groups = g;
  h->ngroups = clear ? 0 : ngroups;
  return SAMSIM_OK;
}

int samsim_get_group_stats(samsim_handle *h, int32_t nslots, const int32_t *slots, samsim_stat *out) {
  if (!h || nslots < 0 || (nslots > 0 && (!slots || !out))) return SAMSIM_ERR_ARG;
  if (!h->groups) return SAMSIM_ERR_ARG;
  for (int i = 0; i < nslots; ++i)
    if (!good_slot(h, slots[i])) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  rc = func_refresh_for(h, nslots, slots);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_group, kGroupScratch));
  GroupPartial *d_part = (GroupPartial *)h->d_group;
  samsim_stat *d_out = (samsim_stat *)((char *)h->d_group + kGroupPartBytes);
  const size_t ng = (size_t)h->ngroups;
  // one pass per slot, all on the handle's stream: a slot's results have left the scratch before the next slot's merge writes them
  for (int i = 0; i < nslots; ++i) {
    const double *row = slot_row(h, slots[i]);
    HIPCHK(samsim_launch_group_stats(label_set(h, true), row, h->ngroups, d_part, d_out, h->stream));
    HIPCHK(hipMemcpyAsync(out + (size_t)i * ng, d_out, sizeof(samsim_stat) * ng, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

// the checks of the value bins of a histogram request, in the order samsim.h gives (vb is not null); fills the device's view
static int check_hist_bins(const samsim_hist_bins *vb, HistEdges *e) {
  if (vb->struct_size != (int32_t)sizeof(samsim_hist_bins)) return SAMSIM_ERR_ABI;
  if (vb->nvbins < 1 || vb->nvbins > SAMSIM_HIST_MAX_VBINS) return SAMSIM_ERR_ARG;
  if (!std::isfinite(vb->v0) || !std::isfinite(vb->dv)) return SAMSIM_ERR_ARG;
  if (!(vb->dv > 0.0)) return SAMSIM_ERR_ARG;
  double prev = 0.0;
  for (int j = 0; j <= vb->nvbins; ++j) {   // E_j = v0 + j*dv as the device forms it: product rounded, then the sum
    const double p = (double)j * vb->dv;
    const double ej = vb->v0 + p;
    if (!std::isfinite(ej) || (j > 0 && !(ej > prev))) return SAMSIM_ERR_ARG;
    prev = ej;
  }
  e->v0 = vb->v0; e->dv = vb->dv; e->rdv = 1.0 / vb->dv; e->nvbins = vb->nvbins;
  return SAMSIM_OK;
}

int samsim_get_histogram(samsim_handle *h, int32_t slot, const samsim_hist_bins *vb, int32_t by_group, int64_t *counts) {
  // every check first: nothing below touches the device before the request is known to be good
  if (!h || !vb || !counts) return SAMSIM_ERR_ARG;
  HistEdges e;
  int rc = check_hist_bins(vb, &e);
  if (rc) return rc;
  if (!good_slot(h, slot)) return SAMSIM_ERR_ARG;
  if (by_group != 0 && by_group != 1) return SAMSIM_ERR_ARG;
  if (by_group && !h->groups) return SAMSIM_ERR_ARG;
  rc = use(h);
  if (rc) return rc;
  rc = func_refresh_for(h, 1, &slot);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_hist, kHistScratch));
  const int ng = by_group ? h->ngroups : 1;
  const size_t bytes = sizeof(int64_t) * (size_t)ng * (size_t)(e.nvbins + 2);
  const double *row = slot_row(h, slot);
  HIPCHK(hipMemsetAsync(h->d_hist, 0, bytes, h->stream));
  HIPCHK(samsim_launch_hist(label_set(h, by_group != 0), row, ng, e, (unsigned long long *)h->d_hist, h->stream));
  HIPCHK(hipMemcpyAsync(counts, h->d_hist, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_get_profile_histogram(samsim_handle *h, const samsim_profile_request *rq, const samsim_hist_bins *vb, int32_t group,
                                 int64_t *counts) {
  // every check first: nothing below touches the device before the request is known to be good
  if (!h || !rq || !vb || !counts) return SAMSIM_ERR_ARG;
  int rc = check_profile_request(h, rq);
  if (rc) return rc;
  if (rq->narrays != 1) return SAMSIM_ERR_ARG;
  HistEdges e;
  rc = check_hist_bins(vb, &e);
  if (rc) return rc;
  if (group < -1 || (group >= 0 && (!h->groups || group >= h->ngroups))) return SAMSIM_ERR_ARG;
  rc = use(h);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_hist, kHistScratch));
  const size_t bytes = sizeof(int64_t) * (size_t)rq->nbins * (size_t)(e.nvbins + 2);
  HIPCHK(hipMemsetAsync(h->d_hist, 0, bytes, h->stream));
  // the passes add into disjoint rows of the counts
  rc = for_each_pass(h, rq, group, dev_hist_chunk(e.nvbins), [&](const ProfPass &p, size_t) {
    return samsim_launch_profile_hist(p, e, (unsigned long long *)h->d_hist, h->stream);
  });
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(counts, h->d_hist, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_get_covariance(samsim_handle *h, int32_t nslots, const int32_t *slots, int32_t group, int64_t *count, double *mean, double *cov) {
  // every check first: nothing below touches the device before the request is known to be good
  if (!h || !slots || !count || !mean || !cov) return SAMSIM_ERR_ARG;
  SensRows rows{};
  const int rc = slot_rows(h, nslots, slots, false, group, &rows);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_sens, kSensScratch));
  double *d_part = (double *)h->d_sens;
  CovResult *d_out = (CovResult *)((char *)h->d_sens + DEV_SENS_PART_BYTES);
  HIPCHK(samsim_launch_covariance(col_set(h, group), rows, nslots, d_part, d_out, h->stream));
  CovResult res;
  return fetch_cov(h, d_out, nslots, &res, count, mean, cov);
}

int samsim_get_profile_regression(samsim_handle *h, const samsim_profile_request *rq, int32_t predictor_slot, int32_t group,
                                  samsim_pair_stat *out) {
  // every check first: nothing below touches the device before the request is known to be good
  if (!h || !rq || !out) return SAMSIM_ERR_ARG;
  int rc = check_profile_request(h, rq);
  if (rc) return rc;
  if (!good_slot(h, predictor_slot)) return SAMSIM_ERR_ARG;
  if (!good_group(h, group)) return SAMSIM_ERR_ARG;
  rc = use(h);
  if (rc) return rc;
  rc = func_refresh_for(h, 1, &predictor_slot);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_sens, kSensScratch));
  SensProfPartial *d_part = (SensProfPartial *)h->d_sens;
  samsim_pair_stat *d_out = (samsim_pair_stat *)((char *)h->d_sens + DEV_SENS_PART_BYTES);
  const double *x = slot_row(h, predictor_slot);
  rc = for_each_pass(h, rq, group, DEV_PROF_BINS, [&](const ProfPass &p, size_t at) {
    return samsim_launch_profile_regression(p, x, d_part, d_out + at, h->stream);
  });
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(out, d_out, sizeof(samsim_pair_stat) * (size_t)rq->narrays * (size_t)rq->nbins, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

// the checks of one track, in the order samsim.h gives
static int check_track_spec(const samsim_handle *h, const samsim_track_spec &s) {
  if (s.struct_size != (int32_t)sizeof(samsim_track_spec)) return SAMSIM_ERR_ABI;
  switch (s.kind) {
    case SAMSIM_OBS_SCALAR: if (s.id < 0 || s.id >= SAMSIM_NSCAL) return SAMSIM_ERR_ARG; break;
    case SAMSIM_OBS_LAYER: if (s.id < 0 || s.id >= SAMSIM_NARR) return SAMSIM_ERR_ARG; break;
    case SAMSIM_OBS_N_ACTIVE: case SAMSIM_OBS_ICE_THICKNESS: case SAMSIM_OBS_BULK_SALINITY: break;
    default: return SAMSIM_ERR_ARG;
  }
  if (s.kind == SAMSIM_OBS_LAYER) {
    if (s.layer == 0 || s.layer > h->cfg.nlayer || s.layer < -h->cfg.nlayer) return SAMSIM_ERR_ARG;
  } else if (s.layer != 0 || (s.kind != SAMSIM_OBS_SCALAR && s.id != 0)) {
    return SAMSIM_ERR_ARG;
  }
  if (s.sense < -1 || s.sense > 1) return SAMSIM_ERR_ARG;
  if (s.sense != 0 && !std::isfinite(s.threshold)) return SAMSIM_ERR_ARG;
  if (s.reserved != 0) return SAMSIM_ERR_ARG;
  return SAMSIM_OK;
}

// the initial values into the rows of nt tracks, enqueued on the handle's stream
static hipError_t init_tracks(samsim_handle *h, double *rows, int nt) {
  const size_t nc = (size_t)h->ncol;
  for (int t = 0; t < nt; ++t)
    for (int f = 0; f < SAMSIM_NTF; ++f) {
      const hipError_t e = fill(rows + ((size_t)t * SAMSIM_NTF + (size_t)f) * nc, nc, dev_track_initial(f), h->stream);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

int samsim_set_tracks(samsim_handle *h, int32_t ntracks, const samsim_track_spec *specs, int64_t every) {
  // every check first: a call that is refused leaves the previous tracks in force
  if (!h) return SAMSIM_ERR_ARG;
  if (ntracks < 0 || ntracks > SAMSIM_MAX_TRACKS) return SAMSIM_ERR_ARG;
  if (ntracks == 0 && specs) return SAMSIM_ERR_ARG;
  if (ntracks > 0 && !specs) return SAMSIM_ERR_ARG;
  if (ntracks > 0 && every < 1) return SAMSIM_ERR_ARG;
  for (int t = 0; t < ntracks; ++t) {
    const int rc = check_track_spec(h, specs[t]);
    if (rc) return rc;
  }
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  // the new rows hold their initial values on the device before the handle sees them
  double *rows = nullptr;
  if (ntracks > 0) {
    if (dalloc(&rows, (size_t)ntracks * SAMSIM_NTF * (size_t)h->ncol) != hipSuccess) {
      (void)hipGetLastError();
      return SAMSIM_ERR_NOMEM;
    }
    if (!hip_ok(init_tracks(h, rows, ntracks), "fill tracks") || !hip_ok(hipStreamSynchronize(h->stream), "sync")) {
      (void)hipFree(rows);
      return SAMSIM_ERR_HIP;
    }
  }
  (void)hipFree(h->tracks);
  h->tracks = rows;
  h->ntracks = ntracks;
  h->track_every = ntracks > 0 ? every : 0;
  for (int t = 0; t < ntracks; ++t) h->track[t] = TrackDev{specs[t].kind, specs[t].id, specs[t].layer, specs[t].sense, specs[t].threshold};
  return SAMSIM_OK;
}

int samsim_reset_tracks(samsim_handle *h) {
  if (!h || !h->tracks) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(init_tracks(h, h->tracks, h->ntracks));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

// a window [col0, col0 + ncols) of the handle's columns, which may be empty and may begin at ncol
static int check_window(const samsim_handle *h, int64_t col0, int64_t ncols) {
  return (col0 < 0 || ncols < 0 || col0 > h->ncol || ncols > h->ncol - col0) ? SAMSIM_ERR_ARG : SAMSIM_OK;
}

// the checks samsim_get_tracks and samsim_set_track_state share, in the order samsim.h gives
static int check_track_window(const samsim_handle *h, const void *buf, int32_t track, int64_t col0, int64_t ncols) {
  if (!h || !buf) return SAMSIM_ERR_ARG;
  if (!h->tracks) return SAMSIM_ERR_ARG;
  if (track < 0 || track >= h->ntracks) return SAMSIM_ERR_ARG;
  return check_window(h, col0, ncols);
}

int samsim_get_tracks(samsim_handle *h, int32_t track, int64_t col0, int64_t ncols, double *out) {
  int rc = check_track_window(h, out, track, col0, ncols);
  if (rc) return rc;
  rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (ncols == 0) return SAMSIM_OK;
  const size_t nc = (size_t)h->ncol, w = (size_t)ncols;
  HIPCHK(hipMemcpy2D(out, w * sizeof(double), h->tracks + (size_t)track * SAMSIM_NTF * nc + (size_t)col0, nc * sizeof(double),
                     w * sizeof(double), (size_t)SAMSIM_NTF, hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

int samsim_set_track_state(samsim_handle *h, int32_t track, int64_t col0, int64_t ncols, const double *in) {
  int rc = check_track_window(h, in, track, col0, ncols);
  if (rc) return rc;
  rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (ncols == 0) return SAMSIM_OK;
  const size_t nc = (size_t)h->ncol, w = (size_t)ncols;
  HIPCHK(hipMemcpy2D(h->tracks + (size_t)track * SAMSIM_NTF * nc + (size_t)col0, nc * sizeof(double), in, w * sizeof(double),
                     w * sizeof(double), (size_t)SAMSIM_NTF, hipMemcpyHostToDevice));
  return SAMSIM_OK;
}

int samsim_select_columns(samsim_handle *h, const samsim_selection *sel, int64_t max_out, int64_t *cols_out, int64_t *n_match) {
  // every check first, in the order samsim.h gives: nothing below touches the device before the request is known to be good
  if (!h || !sel || !n_match) return SAMSIM_ERR_ARG;
  if (sel->struct_size != (int32_t)sizeof(samsim_selection)) return SAMSIM_ERR_ABI;
  if (sel->nterms < 0 || sel->nterms > SAMSIM_SELECT_MAX_TERMS) return SAMSIM_ERR_ARG;
  for (int i = 0; i < sel->nterms; ++i) {
    const samsim_select_term &t = sel->terms[i];
    if (!good_slot(h, t.slot)) return SAMSIM_ERR_ARG;
    if (t.reserved != 0) return SAMSIM_ERR_ARG;
    if (std::isnan(t.lo) || std::isnan(t.hi)) return SAMSIM_ERR_ARG;
  }
  if (!good_group(h, sel->group)) return SAMSIM_ERR_ARG;
  if (sel->status_mode < SAMSIM_SELECT_RUNNING || sel->status_mode > SAMSIM_SELECT_ANY) return SAMSIM_ERR_ARG;
  if (sel->status_mode != SAMSIM_SELECT_CODE && sel->code != 0) return SAMSIM_ERR_ARG;
  if (sel->reserved != 0) return SAMSIM_ERR_ARG;
  if (max_out < 0 || max_out > SAMSIM_SELECT_MAX_OUT || (max_out > 0 && !cols_out)) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  for (int i = 0; i < sel->nterms && !rc; ++i) rc = func_refresh_for(h, 1, &sel->terms[i].slot);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_select, kSelectScratch));
  SelParams p{};
  for (int i = 0; i < sel->nterms; ++i) p.t[i] = SelTerm{slot_row(h, sel->terms[i].slot), sel->terms[i].lo, sel->terms[i].hi};
  p.n_active = h->n_active;
  p.status = sel->status_mode == SAMSIM_SELECT_ANY ? nullptr : h->status;
  p.labels = labels_for(h, sel->group);
  p.ncol = h->ncol;
  // wave w owns the blocks [w * per, (w + 1) * per): as many waves as that leaves with a block, DEV_SEL_GRID at most
  const long long nblk = (h->ncol + 63) / 64;
  p.per = (nblk + DEV_SEL_GRID - 1) / DEV_SEL_GRID;
  p.nwaves = (int32_t)((nblk + p.per - 1) / p.per);
  p.max_out = max_out;
  p.nterms = sel->nterms; p.group = sel->group; p.status_mode = sel->status_mode; p.code = sel->code;
  HIPCHK(samsim_launch_select(&p, h->d_select, h->stream));
  long long total = 0;
  HIPCHK(hipMemcpyAsync(&total, (const char *)h->d_select + DEV_SEL_OFFSETS_AT + (size_t)DEV_SEL_GRID * 8, sizeof(long long),
                        hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const long long nout = total < max_out ? total : max_out;
  if (nout > 0)
    HIPCHK(hipMemcpy(cols_out, (const char *)h->d_select + DEV_SEL_LIST_AT, sizeof(int64_t) * (size_t)nout, hipMemcpyDeviceToHost));
  *n_match = total;
  return SAMSIM_OK;
}

// A host list of column indices, checked against the handle and -- behind use() -- on its way into the index list of the select
// scratch, on the handle's stream: *d_cols is the device copy.  A list that is refused touches nothing.
static int stage_list(samsim_handle *h, int64_t ncols, const int64_t *cols, long long **d_cols) {
  for (int64_t j = 0; j < ncols; ++j)
    if (cols[j] < 0 || cols[j] >= h->ncol) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_select, kSelectScratch));
  *d_cols = (long long *)((char *)h->d_select + DEV_SEL_LIST_AT);
  HIPCHK(hipMemcpyAsync(*d_cols, cols, sizeof(int64_t) * (size_t)ncols, hipMemcpyHostToDevice, h->stream));
  return SAMSIM_OK;
}

int samsim_get_columns(samsim_handle *h, int64_t ncols, const int64_t *cols, samsim_state_soa *s, int32_t *status, int64_t *step,
                       int32_t *layer) {
  // every check first: a call that is refused writes nothing to the caller's buffers
  if (!h || !cols || !s) return SAMSIM_ERR_ARG;
  // the shape checks of check_soa, without its window: a list may be longer than the handle (duplicates)
  if (!s->lay || !s->scal || !s->n_active || s->nlayer != h->cfg.nlayer) return SAMSIM_ERR_ARG;
  if (s->narr != SAMSIM_NPROG && s->narr != SAMSIM_NARR) return SAMSIM_ERR_ARG;
  if (ncols < 1 || ncols > SAMSIM_SELECT_MAX_OUT || s->ncol != ncols) return SAMSIM_ERR_ARG;
  long long *d_cols = nullptr;
  int rc = stage_list(h, ncols, cols, &d_cols);
  if (rc) return rc;
  const size_t N = (size_t)s->nlayer, w = (size_t)ncols;
  // the list's positions in pieces as samsim_get_state cuts a window; the staging buffer also takes the per-column rows, one piece
  const size_t pc = stage_cols(s->narr, N), rows = (size_t)s->narr * N;
  const size_t lay_n = rows * (w < pc ? w : pc), col_n = (w * DEV_SEL_COLUMN_BYTES + 7) / 8;
  HIPCHK(stage_for(h, lay_n > col_n ? lay_n : col_n));
  HIPCHK(samsim_launch_gather_columns(h->scal, h->n_active, h->status, h->err_step, h->err_layer, d_cols, h->stage, h->ncol, (long long)w,
                                      h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  {
    const double *g_scal = h->stage;
    const long long *g_step = (const long long *)(g_scal + (size_t)SAMSIM_NSCAL * w);
    const int32_t *g_na = (const int32_t *)(g_step + w);
    HIPCHK(hipMemcpy(s->scal, g_scal, sizeof(double) * SAMSIM_NSCAL * w, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(s->n_active, g_na, sizeof(int32_t) * w, hipMemcpyDeviceToHost));
    if (step) HIPCHK(hipMemcpy(step, g_step, sizeof(int64_t) * w, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, g_na + w, sizeof(int32_t) * w, hipMemcpyDeviceToHost));
    if (layer) HIPCHK(hipMemcpy(layer, g_na + 2 * w, sizeof(int32_t) * w, hipMemcpyDeviceToHost));
  }
  for (size_t p0 = 0; p0 < w; p0 += pc) {
    const size_t pw = w - p0 < pc ? w - p0 : pc;
    HIPCHK(samsim_launch_gather_layers(h->lay, d_cols + p0, h->n_active, h->status, h->flags, h->stage, (int)s->narr, (int)N, h->ncol,
                                       (long long)pw, h->stepped ? 1 : 0, h->stream));
    HIPCHK(copy_rows(s->lay + p0, w, h->stage, pw, pw, rows, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return SAMSIM_OK;
}

// the checks of one functional, in the order samsim.h gives
static int check_functional_spec(const samsim_functional_spec &s) {
  if (s.struct_size != (int32_t)sizeof(samsim_functional_spec)) return SAMSIM_ERR_ABI;
  if (s.kind < 0 || s.kind >= SAMSIM_NFN) return SAMSIM_ERR_ARG;
  if (s.array < 0 || s.array >= SAMSIM_NARR) return SAMSIM_ERR_ARG;
  if (s.origin != SAMSIM_PROFILE_FROM_TOP && s.origin != SAMSIM_PROFILE_FROM_BOTTOM) return SAMSIM_ERR_ARG;
  const bool cond = s.kind == SAMSIM_FN_CROSSING_DEPTH || s.kind == SAMSIM_FN_THICKNESS_WHERE;
  if (cond ? (s.sense != 1 && s.sense != -1) : s.sense != 0) return SAMSIM_ERR_ARG;
  if (s.sense != 0 && !std::isfinite(s.threshold)) return SAMSIM_ERR_ARG;
  if (!std::isfinite(s.z_lo) || s.z_lo < 0.0) return SAMSIM_ERR_ARG;
  if (std::isnan(s.z_hi) || !(s.z_hi > s.z_lo)) return SAMSIM_ERR_ARG;
  if (s.reserved != 0) return SAMSIM_ERR_ARG;
  return SAMSIM_OK;
}

int samsim_set_functionals(samsim_handle *h, int32_t n, const samsim_functional_spec *specs) {
  // every check first: a call that is refused leaves the previous functionals in force
  if (!h) return SAMSIM_ERR_ARG;
  if (n < 0 || n > SAMSIM_MAX_FUNCTIONALS) return SAMSIM_ERR_ARG;
  if ((n > 0 && !specs) || (n == 0 && specs)) return SAMSIM_ERR_ARG;
  for (int i = 0; i < n; ++i) {
    const int rc = check_functional_spec(specs[i]);
    if (rc) return rc;
  }
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  double *rows = nullptr;
  if (n > 0 && dalloc(&rows, (size_t)n * (size_t)h->ncol) != hipSuccess) {
    (void)hipGetLastError();
    return SAMSIM_ERR_NOMEM;
  }
  (void)hipFree(h->func_rows);
  h->func_rows = rows;
  h->nfunc = n;
  h->func_dirty = true;
  static_assert(sizeof(samsim_functional_spec) == 56, "samsim_functional_spec of samsim.h");
  for (int i = 0; i < n; ++i) h->func[i] = specs[i];
  return SAMSIM_OK;
}

int samsim_get_functionals(samsim_handle *h, int32_t index, int64_t col0, int64_t ncols, double *out) {
  if (!h || !out) return SAMSIM_ERR_ARG;
  if (!h->func_rows) return SAMSIM_ERR_ARG;
  if (index < 0 || index >= h->nfunc) return SAMSIM_ERR_ARG;
  int rc = check_window(h, col0, ncols);
  if (rc) return rc;
  rc = use(h);
  if (rc) return rc;
  rc = func_refresh(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (ncols == 0) return SAMSIM_OK;
  HIPCHK(hipMemcpy(out, h->func_rows + (size_t)index * (size_t)h->ncol + (size_t)col0, sizeof(double) * (size_t)ncols, hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

// the checks of one sensor, in the order samsim.h gives
static int check_sensor_spec(const samsim_sensor_spec &s) {
  if (s.struct_size != (int32_t)sizeof(samsim_sensor_spec)) return SAMSIM_ERR_ABI;
  switch (s.kind) {
    case SAMSIM_SENSOR_PROFILE: if (s.id < 0 || s.id >= SAMSIM_NARR) return SAMSIM_ERR_ARG; break;
    case SAMSIM_SENSOR_SCALAR: if (s.id < 0 || s.id >= SAMSIM_NSCAL) return SAMSIM_ERR_ARG; break;
    case SAMSIM_SENSOR_ICE_THICKNESS: if (s.id != 0) return SAMSIM_ERR_ARG; break;
    default: return SAMSIM_ERR_ARG;
  }
  if (s.origin != SAMSIM_PROFILE_FROM_TOP && s.origin != SAMSIM_PROFILE_FROM_BOTTOM) return SAMSIM_ERR_ARG;
  if (s.interp != SAMSIM_SENSOR_STEP && s.interp != SAMSIM_SENSOR_LINEAR) return SAMSIM_ERR_ARG;
  if (s.kind != SAMSIM_SENSOR_PROFILE && (s.origin != 0 || s.interp != 0 || !(s.z == 0.0))) return SAMSIM_ERR_ARG;
  if (!std::isfinite(s.z) || s.z < 0.0) return SAMSIM_ERR_ARG;
  if (s.reserved != 0) return SAMSIM_ERR_ARG;
  return SAMSIM_OK;
}

// what a score and the values of a list share
static void sensor_params(const samsim_handle *h, SensorParams *p) {
  p->lay = h->lay; p->scal = h->scal; p->n_active = h->n_active; p->status = h->status; p->flags = h->flags;
  p->ncol = h->ncol; p->N = h->cfg.nlayer; p->ns = h->nsensors; p->stepped = h->stepped ? 1 : 0;
  p->group = -1;
  sensor_plan(h, p);
}

static hipError_t zero_scores(samsim_handle *h, double *rows) {
  return fill(rows, (size_t)SAMSIM_NSF * (size_t)h->ncol, 0.0, h->stream);
}

int samsim_set_sensors(samsim_handle *h, int32_t n, const samsim_sensor_spec *specs) {
  // every check first: a call that is refused leaves the previous sensors and rows in force
  if (!h) return SAMSIM_ERR_ARG;
  if (n < 0 || n > SAMSIM_MAX_SENSORS) return SAMSIM_ERR_ARG;
  if ((n > 0 && !specs) || (n == 0 && specs)) return SAMSIM_ERR_ARG;
  for (int i = 0; i < n; ++i) {
    const int rc = check_sensor_spec(specs[i]);
    if (rc) return rc;
  }
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  // the new rows hold their zeros on the device before the handle sees them
  double *rows = nullptr;
  if (n > 0) {
    if (dalloc(&rows, (size_t)SAMSIM_NSF * (size_t)h->ncol) != hipSuccess) {
      (void)hipGetLastError();
      return SAMSIM_ERR_NOMEM;
    }
    if (!hip_ok(zero_scores(h, rows), "fill scores") || !hip_ok(hipStreamSynchronize(h->stream), "sync")) {
      (void)hipFree(rows);
      return SAMSIM_ERR_HIP;
    }
  }
  (void)hipFree(h->score_rows);
  h->score_rows = rows;
  h->nsensors = n;
  static_assert(sizeof(samsim_sensor_spec) == 40, "samsim_sensor_spec of samsim.h");
  for (int i = 0; i < n; ++i) h->sensor[i] = specs[i];
  return SAMSIM_OK;
}

int samsim_get_sensor_values(samsim_handle *h, int64_t ncols, const int64_t *cols, double *y) {
  // every check first: a call that is refused writes nothing to the caller's buffer
  if (!h || !cols || !y) return SAMSIM_ERR_ARG;
  if (!h->score_rows) return SAMSIM_ERR_ARG;
  if (ncols < 1 || ncols > SAMSIM_SELECT_MAX_OUT) return SAMSIM_ERR_ARG;
  long long *d_cols = nullptr;
  int rc = stage_list(h, ncols, cols, &d_cols);
  if (rc) return rc;
  const size_t w = (size_t)ncols, ns = (size_t)h->nsensors;
  HIPCHK(stage_for(h, ns * (w < DEV_SENSOR_PIECE ? w : (size_t)DEV_SENSOR_PIECE)));
  SensorParams p{};
  sensor_params(h, &p);
  p.out = h->stage;
  // the list's positions in pieces of DEV_SENSOR_PIECE: the scratch holds [n][piece] values, whatever the list
  for (size_t p0 = 0; p0 < w; p0 += DEV_SENSOR_PIECE) {
    const size_t pw = w - p0 < DEV_SENSOR_PIECE ? w - p0 : (size_t)DEV_SENSOR_PIECE;
    p.cols = d_cols + p0;
    p.npos = (long long)pw;
    HIPCHK(samsim_launch_sensor_values(&p, h->stream));
    HIPCHK(copy_rows(y + p0, w, h->stage, pw, pw, ns, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return SAMSIM_OK;
}

int samsim_score(samsim_handle *h, const double *obs, const double *weight, int32_t group) {
  if (!h || !obs) return SAMSIM_ERR_ARG;
  if (!h->score_rows) return SAMSIM_ERR_ARG;
  for (int i = 0; i < h->nsensors; ++i)
    if (weight && !std::isnan(obs[i]) && !(std::isfinite(weight[i]) && weight[i] > 0.0)) return SAMSIM_ERR_ARG;
  if (!good_group(h, group)) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  SensorParams p{};
  sensor_params(h, &p);
  p.out = h->score_rows;
  p.labels = labels_for(h, group);
  p.group = group;
  for (int i = 0; i < h->nsensors; ++i) {
    const bool have = !std::isnan(obs[i]);
    if (have) p.obs_mask |= 1u << i;
    p.obs[i] = have ? obs[i] : 0.0;
    p.weight[i] = (weight && have) ? weight[i] : 1.0;
  }
  HIPCHK(samsim_launch_score(&p, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

// the checks samsim_get_scores and samsim_set_score_state share, in the order samsim.h gives
static int check_score_window(const samsim_handle *h, const void *buf, int64_t col0, int64_t ncols) {
  if (!h || !buf) return SAMSIM_ERR_ARG;
  if (!h->score_rows) return SAMSIM_ERR_ARG;
  return check_window(h, col0, ncols);
}

int samsim_get_scores(samsim_handle *h, int64_t col0, int64_t ncols, double *out) {
  int rc = check_score_window(h, out, col0, ncols);
  if (rc) return rc;
  rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (ncols == 0) return SAMSIM_OK;
  const size_t nc = (size_t)h->ncol, w = (size_t)ncols;
  HIPCHK(hipMemcpy2D(out, w * sizeof(double), h->score_rows + (size_t)col0, nc * sizeof(double), w * sizeof(double), (size_t)SAMSIM_NSF,
                     hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

int samsim_set_score_state(samsim_handle *h, int64_t col0, int64_t ncols, const double *in) {
  int rc = check_score_window(h, in, col0, ncols);
  if (rc) return rc;
  rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (ncols == 0) return SAMSIM_OK;
  const size_t nc = (size_t)h->ncol, w = (size_t)ncols;
  HIPCHK(hipMemcpy2D(h->score_rows + (size_t)col0, nc * sizeof(double), in, w * sizeof(double), w * sizeof(double), (size_t)SAMSIM_NSF,
                     hipMemcpyHostToDevice));
  return SAMSIM_OK;
}

int samsim_reset_scores(samsim_handle *h) {
  if (!h || !h->score_rows) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(zero_scores(h, h->score_rows));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_set_weights(samsim_handle *h, const samsim_weight_spec *spec, samsim_weight_info *info) {
  // every check first, in the order samsim.h gives: a call that is refused leaves the previous row in force
  if (!h) return SAMSIM_ERR_ARG;
  if (!spec) {
    if (info) return SAMSIM_ERR_ARG;
    int rc = use(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    (void)hipFree(h->weight_row);
    h->weight_row = nullptr;
    return SAMSIM_OK;
  }
  if (spec->struct_size != (int32_t)sizeof(samsim_weight_spec)) return SAMSIM_ERR_ABI;
  if (spec->kind != SAMSIM_WEIGHT_DIRECT && spec->kind != SAMSIM_WEIGHT_GAUSS) return SAMSIM_ERR_ARG;
  if (spec->slot == SAMSIM_WEIGHT_SLOT || !good_slot(h, spec->slot)) return SAMSIM_ERR_ARG;
  if (!good_group(h, spec->group)) return SAMSIM_ERR_ARG;
  if (spec->kind == SAMSIM_WEIGHT_DIRECT && spec->scale != 0.0) return SAMSIM_ERR_ARG;
  if (spec->kind == SAMSIM_WEIGHT_GAUSS && !(std::isfinite(spec->scale) && spec->scale > 0.0)) return SAMSIM_ERR_ARG;
  if (spec->reserved != 0.0) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  // the row of the first call, kept and rewritten by the later ones (the source is never the row itself)
  double *row = h->weight_row;
  if (!row && dalloc(&row, (size_t)h->ncol) != hipSuccess) {
    (void)hipGetLastError();
    return SAMSIM_ERR_NOMEM;
  }
  const bool fresh = !h->weight_row;
  rc = func_refresh_for(h, 1, &spec->slot);
  if (!rc && !hip_ok(scratch(&h->d_weight, kWeightScratch), "hipMalloc weight scratch")) rc = SAMSIM_ERR_HIP;
  if (rc) {
    if (fresh) (void)hipFree(row);
    return rc;
  }
  h->weight_row = row;
  WeightPartial *d_part = (WeightPartial *)((char *)h->d_weight + DEV_WEIGHT_PART_AT);
  WeightPartial *d_out = (WeightPartial *)((char *)h->d_weight + DEV_WEIGHT_RESULT_AT);
  const double c = spec->kind == SAMSIM_WEIGHT_GAUSS ? 0.5 / spec->scale : 0.0;
  HIPCHK(samsim_launch_set_weights(col_set(h, spec->group), slot_row(h, spec->slot), spec->kind, c, row, d_part, d_out, h->stream));
  WeightPartial res;
  HIPCHK(hipMemcpyAsync(&res, d_out, sizeof(WeightPartial), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (info) *info = samsim_weight_info{res.n_in, res.n_pos, res.x_min, res.sum_w, res.sum_w2};
  return SAMSIM_OK;
}

int samsim_get_weights(samsim_handle *h, int64_t col0, int64_t ncols, double *out) {
  if (!h || !out) return SAMSIM_ERR_ARG;
  if (!h->weight_row) return SAMSIM_ERR_ARG;
  int rc = check_window(h, col0, ncols);
  if (rc) return rc;
  rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (ncols == 0) return SAMSIM_OK;
  HIPCHK(hipMemcpy(out, h->weight_row + (size_t)col0, sizeof(double) * (size_t)ncols, hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

int samsim_get_weighted_stats(samsim_handle *h, int32_t nslots, const int32_t *slots, int32_t group, samsim_wstat *out) {
  // every check first: nothing below touches the device before the request is known to be good
  if (!h || !slots || !out) return SAMSIM_ERR_ARG;
  SensRows rows{};
  const int rc = slot_rows(h, nslots, slots, true, group, &rows);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_weight, kWeightScratch));
  WStatPartial *d_part = (WStatPartial *)((char *)h->d_weight + DEV_WEIGHT_PART_AT);
  samsim_wstat *d_out = (samsim_wstat *)((char *)h->d_weight + DEV_WEIGHT_RESULT_AT);
  HIPCHK(samsim_launch_weighted_stats(col_set(h, group), rows, nslots, h->weight_row, d_part, d_out, h->stream));
  HIPCHK(hipMemcpyAsync(out, d_out, sizeof(samsim_wstat) * (size_t)nslots, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_get_weighted_histogram(samsim_handle *h, int32_t slot, const samsim_hist_bins *vb, int32_t group, double *wsum) {
  // every check first: nothing below touches the device before the request is known to be good
  if (!h || !vb || !wsum) return SAMSIM_ERR_ARG;
  HistEdges e;
  int rc = check_hist_bins(vb, &e);
  if (rc) return rc;
  if (!good_slot(h, slot)) return SAMSIM_ERR_ARG;
  if (!h->weight_row) return SAMSIM_ERR_ARG;
  if (!good_group(h, group)) return SAMSIM_ERR_ARG;
  rc = use(h);
  if (rc) return rc;
  rc = func_refresh_for(h, 1, &slot);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_weight, kWeightScratch));
  double *d_tables = (double *)((char *)h->d_weight + DEV_WEIGHT_TABLES_AT);
  double *d_out = (double *)((char *)h->d_weight + DEV_WEIGHT_RESULT_AT);
  HIPCHK(samsim_launch_weighted_hist(col_set(h, group), slot_row(h, slot), h->weight_row, e, d_tables, d_out, h->stream));
  HIPCHK(hipMemcpyAsync(wsum, d_out, sizeof(double) * (size_t)(e.nvbins + 2), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_get_weighted_profile_stats(samsim_handle *h, const samsim_profile_request *rq, int32_t group, samsim_wstat *out) {
  // every check first: nothing below touches the device before the request is known to be good
  if (!h || !rq || !out) return SAMSIM_ERR_ARG;
  int rc = check_profile_request(h, rq);
  if (rc) return rc;
  if (!h->weight_row) return SAMSIM_ERR_ARG;
  if (!good_group(h, group)) return SAMSIM_ERR_ARG;
  rc = use(h);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_wprof, kWProfScratch));
  WProfPartial *d_part = (WProfPartial *)h->d_wprof;
  samsim_wstat *d_out = (samsim_wstat *)((char *)h->d_wprof + DEV_WPROF_PART_BYTES);
  rc = for_each_pass(h, rq, group, DEV_PROF_BINS, [&](const ProfPass &p, size_t at) {
    return samsim_launch_weighted_profile(p, h->weight_row, d_part, d_out + at, h->stream);
  });
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(out, d_out, sizeof(samsim_wstat) * (size_t)rq->narrays * (size_t)rq->nbins, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_get_weighted_profile_histogram(samsim_handle *h, const samsim_profile_request *rq, const samsim_hist_bins *vb, int32_t group,
                                          double *wsum) {
  // every check first: nothing below touches the device before the request is known to be good
  if (!h || !rq || !vb || !wsum) return SAMSIM_ERR_ARG;
  int rc = check_profile_request(h, rq);
  if (rc) return rc;
  if (rq->narrays != 1) return SAMSIM_ERR_ARG;
  HistEdges e;
  rc = check_hist_bins(vb, &e);
  if (rc) return rc;
  if (!h->weight_row) return SAMSIM_ERR_ARG;
  if (!good_group(h, group)) return SAMSIM_ERR_ARG;
  rc = use(h);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_wphist, kWPHistScratch));
  double *d_tables = (double *)h->d_wphist;
  double *d_out = (double *)((char *)h->d_wphist + DEV_WPHIST_PART_BYTES);
  // a pass's merge writes its own rows of the result, every entry of them
  rc = for_each_pass(h, rq, group, dev_wphist_chunk(e.nvbins), [&](const ProfPass &p, size_t) {
    return samsim_launch_weighted_profile_hist(p, h->weight_row, e, d_tables, d_out, h->stream);
  });
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(wsum, d_out, sizeof(double) * (size_t)rq->nbins * (size_t)(e.nvbins + 2), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_get_weighted_covariance(samsim_handle *h, int32_t nslots, const int32_t *slots, int32_t group, int64_t *count, double *sum_w,
                                   double *sum_w2, double *mean, double *cov) {
  // every check first: nothing below touches the device before the request is known to be good
  if (!h || !slots || !count || !sum_w || !sum_w2 || !mean || !cov) return SAMSIM_ERR_ARG;
  SensRows rows{};
  int rc = slot_rows(h, nslots, slots, true, group, &rows);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_weight, kWeightScratch));
  double *d_part = (double *)((char *)h->d_weight + DEV_WEIGHT_PART_AT);
  WCovResult *d_out = (WCovResult *)((char *)h->d_weight + DEV_WEIGHT_RESULT_AT);
  HIPCHK(samsim_launch_weighted_covariance(col_set(h, group), rows, nslots, h->weight_row, d_part, d_out, h->stream));
  WCovResult res;
  rc = fetch_cov(h, d_out, nslots, &res, count, mean, cov);
  if (rc) return rc;
  *sum_w = res.sum_w;
  *sum_w2 = res.sum_w2;
  return SAMSIM_OK;
}

int samsim_resample(samsim_handle *h, const samsim_resample_spec *spec, samsim_resample_info *info) {
  // every check first, in the order samsim.h gives: a call that is refused leaves the previous rows in force
  if (!h) return SAMSIM_ERR_ARG;
  if (!spec) {
    if (info) return SAMSIM_ERR_ARG;
    int rc = use(h);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    (void)hipFree(h->offspring_row); (void)hipFree(h->ancestors);
    h->offspring_row = nullptr; h->ancestors = nullptr;
    h->ancestors_cap = 0; h->m_drawn = 0;
    h->rs_applied = false;
    return SAMSIM_OK;
  }
  if (spec->struct_size != (int32_t)sizeof(samsim_resample_spec)) return SAMSIM_ERR_ABI;
  if (spec->kind != SAMSIM_RESAMPLE_SYSTEMATIC && spec->kind != SAMSIM_RESAMPLE_STRATIFIED) return SAMSIM_ERR_ARG;
  if (!h->weight_row) return SAMSIM_ERR_ARG;
  if (!good_group(h, spec->group)) return SAMSIM_ERR_ARG;
  if (spec->m < 1 || spec->m > SAMSIM_RESAMPLE_MAX_DRAWS) return SAMSIM_ERR_ARG;
  if (spec->kind == SAMSIM_RESAMPLE_SYSTEMATIC && (!(spec->u0 >= 0.0 && spec->u0 < 1.0) || spec->seed != 0)) return SAMSIM_ERR_ARG;
  if (spec->kind == SAMSIM_RESAMPLE_STRATIFIED && spec->u0 != 0.0) return SAMSIM_ERR_ARG;
  if (spec->reserved != 0) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  // the rows of the first call, kept and rewritten by the later ones; the list grows to the largest m asked for, and the one in
  // force goes only once its successor stands
  double *row = h->offspring_row;
  long long *list = h->ancestors;
  if (!row && dalloc(&row, (size_t)h->ncol) != hipSuccess) {
    (void)hipGetLastError();
    return SAMSIM_ERR_NOMEM;
  }
  if (spec->m > h->ancestors_cap && dalloc(&list, (size_t)spec->m) != hipSuccess) {
    (void)hipGetLastError();
    if (!h->offspring_row) (void)hipFree(row);
    return SAMSIM_ERR_NOMEM;
  }
  if (!hip_ok(scratch(&h->d_resample, kResampleScratch), "hipMalloc resample scratch")) {
    if (!h->offspring_row) (void)hipFree(row);
    if (list != h->ancestors) (void)hipFree(list);
    return SAMSIM_ERR_HIP;
  }
  h->offspring_row = row;
  if (list != h->ancestors) {
    HIPCHK(hipStreamSynchronize(h->stream));
    (void)hipFree(h->ancestors);
    h->ancestors = list;
    h->ancestors_cap = spec->m;
  }
  h->m_drawn = 0;   // until the draw below stands
  const RsGrid grid = rs_grid(h->ncol);
  RsParams p{};
  p.cs = col_set(h, spec->group);
  p.w = h->weight_row;
  p.per = grid.per; p.ranges = grid.ranges;
  p.m = spec->m; p.u0 = spec->u0; p.seed = spec->seed; p.kind = spec->kind;
  HIPCHK(samsim_launch_resample(&p, h->d_resample, h->offspring_row, h->ancestors, h->stream));
  RsResult res;
  HIPCHK(hipMemcpyAsync(&res, (const char *)h->d_resample + DEV_RS_RESULT_AT, sizeof(RsResult), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->m_drawn = res.m_drawn;
  h->rs_group = spec->group; h->rs_applied = false;   // what samsim_apply_resample takes its pool from
  if (info) *info = samsim_resample_info{res.n_pos, res.m_drawn, res.n_surv, res.max_n, res.argmax, res.sum_w};
  return SAMSIM_OK;
}

int samsim_get_offspring(samsim_handle *h, int64_t col0, int64_t ncols, double *out) {
  if (!h || !out) return SAMSIM_ERR_ARG;
  if (!h->offspring_row) return SAMSIM_ERR_ARG;
  int rc = check_window(h, col0, ncols);
  if (rc) return rc;
  rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (ncols == 0) return SAMSIM_OK;
  HIPCHK(hipMemcpy(out, h->offspring_row + (size_t)col0, sizeof(double) * (size_t)ncols, hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

int samsim_get_ancestors(samsim_handle *h, int64_t k0, int64_t nk, int64_t *out) {
  if (!h || !out) return SAMSIM_ERR_ARG;
  if (!h->offspring_row) return SAMSIM_ERR_ARG;
  if (k0 < 0 || nk < 0 || k0 > h->m_drawn || nk > h->m_drawn - k0) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (nk == 0) return SAMSIM_OK;
  HIPCHK(hipMemcpy(out, h->ancestors + (size_t)k0, sizeof(int64_t) * (size_t)nk, hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

}  // extern "C"

// ---- whole columns copied in place (samsim_copy.hip)
namespace {

constexpr int32_t kCopyAll = SAMSIM_COPY_FORCING | SAMSIM_COPY_TRACKS | SAMSIM_COPY_SCORES;

// the checks of `what` samsim_copy_columns and samsim_apply_resample share, in the order samsim.h gives
int check_copy_what(const samsim_handle *h, int32_t what) {
  if (what & ~kCopyAll) return SAMSIM_ERR_ARG;
  if ((what & SAMSIM_COPY_TRACKS) && !h->tracks) return SAMSIM_ERR_ARG;
  if ((what & SAMSIM_COPY_SCORES) && !h->score_rows) return SAMSIM_ERR_ARG;
  return SAMSIM_OK;
}

// two int64 rows of ncol, allocated together on first use
int copy_lists(samsim_handle *h, long long **a, long long **b) {
  if (*a && *b) return SAMSIM_OK;
  long long *x = nullptr, *y = nullptr;
  if (dalloc(&x, (size_t)h->ncol) != hipSuccess || dalloc(&y, (size_t)h->ncol) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(x); (void)hipFree(y);
    return SAMSIM_ERR_NOMEM;
  }
  *a = x; *b = y;
  return SAMSIM_OK;
}

// The copy of the n pairs (src[j], dst[j]) of two device lists, enqueued on the handle's stream: what include/samsim.h says of
// samsim_copy_columns.  Sources are only read and destinations only written, so the launches do not depend on one another.
int copy_run(samsim_handle *h, long long n, const long long *src, const long long *dst, int32_t what) {
  const long long nc = h->ncol;
  const size_t N = (size_t)h->cfg.nlayer;
  h->func_dirty = true;
  HIPCHK(samsim_launch_copy_layers(h->lay, src, dst, h->n_active, h->status, h->flags, (int)N, nc, n, h->stepped ? 1 : 0, h->stream));
  // the perturbation slots (>= SAMSIM_S_DT2M) belong to the forcing: they stay with the slot unless the call asks for them
  const long long nscal = (what & SAMSIM_COPY_FORCING) ? (long long)SAMSIM_NSCAL : (long long)SAMSIM_S_DT2M;
  HIPCHK(samsim_launch_copy_rows8(h->scal, nscal, nc, src, dst, n, h->stream));
  HIPCHK(samsim_launch_copy_rows4(h->n_active, 1, nc, src, dst, n, h->stream));
  HIPCHK(samsim_launch_copy_rows4(h->status, 1, nc, src, dst, n, h->stream));
  HIPCHK(samsim_launch_copy_rows4(h->err_layer, 1, nc, src, dst, n, h->stream));
  HIPCHK(samsim_launch_copy_rows8(h->err_step, 1, nc, src, dst, n, h->stream));
  // the next step of the copies runs the full first sweep and treats RAY as the previous step's Rayleigh numbers, as after samsim_set_state
  HIPCHK(samsim_launch_copy_fill4(h->flags, nc, dst, n, COLF_DIRTY | COLF_RESTART, h->stream));
  if (h->n_bgc > 0) HIPCHK(samsim_launch_copy_rows8(h->bgc, (long long)h->n_bgc * (long long)N, nc, src, dst, n, h->stream));
  if (what & SAMSIM_COPY_TRACKS) HIPCHK(samsim_launch_copy_rows8(h->tracks, (long long)h->ntracks * SAMSIM_NTF, nc, src, dst, n, h->stream));
  if (what & SAMSIM_COPY_SCORES) HIPCHK(samsim_launch_copy_rows8(h->score_rows, (long long)SAMSIM_NSF, nc, src, dst, n, h->stream));
  if (what & SAMSIM_COPY_FORCING) {
    if (h->site) HIPCHK(samsim_launch_copy_rows4(h->site, 1, nc, src, dst, n, h->stream));
    if (h->ocean_dflq) HIPCHK(samsim_launch_copy_rows8(h->ocean_dflq, 1, nc, src, dst, n, h->stream));
    if (h->ocean_sbu) HIPCHK(samsim_launch_copy_rows8(h->ocean_sbu, 1, nc, src, dst, n, h->stream));
  }
  return SAMSIM_OK;
}

}  // namespace

extern "C" {

int samsim_copy_columns(samsim_handle *h, int64_t n, const int64_t *src, const int64_t *dst, int32_t what) {
  // every check first, in the order samsim.h gives: a call that is refused writes nothing
  if (!h || !src || !dst) return SAMSIM_ERR_ARG;
  if (n < 1 || n > h->ncol) return SAMSIM_ERR_ARG;
  int rc = check_copy_what(h, what);
  if (rc) return rc;
  for (int64_t j = 0; j < n; ++j)
    if (src[j] < 0 || src[j] >= h->ncol || dst[j] < 0 || dst[j] >= h->ncol) return SAMSIM_ERR_ARG;
  std::vector<unsigned char> is_dst;
  try { is_dst.assign((size_t)h->ncol, 0); } catch (const std::bad_alloc &) { return SAMSIM_ERR_NOMEM; }
  for (int64_t j = 0; j < n; ++j) {
    if (is_dst[(size_t)dst[j]]) return SAMSIM_ERR_ARG;
    is_dst[(size_t)dst[j]] = 1;
  }
  for (int64_t j = 0; j < n; ++j)
    if (is_dst[(size_t)src[j]]) return SAMSIM_ERR_ARG;
  rc = use(h);
  if (rc) return rc;
  rc = copy_lists(h, &h->copy_src, &h->copy_dst);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(h->copy_src, src, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->copy_dst, dst, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  rc = copy_run(h, n, h->copy_src, h->copy_dst, what);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return SAMSIM_OK;
}

int samsim_apply_resample(samsim_handle *h, int32_t what, samsim_apply_info *info) {
  if (!h) return SAMSIM_ERR_ARG;
  int rc = check_copy_what(h, what);
  if (rc) return rc;
  if (!h->offspring_row) return SAMSIM_ERR_ARG;
  if (h->rs_applied) return SAMSIM_ERR_ARG;
  // the labels may have been removed since the draw: the pool of a group cannot be formed without them
  if (!good_group(h, h->rs_group)) return SAMSIM_ERR_ARG;
  rc = use(h);
  if (rc) return rc;
  rc = copy_lists(h, &h->plan_src, &h->plan_dst);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_copy, kCopyScratch));
  const CpGrid grid = cp_grid(h->ncol);
  CpParams p{};
  p.offspring = h->offspring_row; p.status = h->status; p.labels = labels_for(h, h->rs_group);
  p.ncol = h->ncol; p.per = grid.per; p.ranges = grid.ranges; p.group = h->rs_group;
  HIPCHK(samsim_launch_copy_plan_count(&p, h->d_copy, h->stream));
  CpResult res;
  HIPCHK(hipMemcpyAsync(&res, (const char *)h->d_copy + DEV_CP_RESULT_AT, sizeof(CpResult), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  // the counting pass decides, before any column and before the stored plan is written
  if (!cp_balanced(res) || res.n_copies > h->ncol) return SAMSIM_ERR_UNSUPPORTED;
  if (res.n_copies > 0) {
    HIPCHK(samsim_launch_copy_plan_write(&p, h->d_copy, h->plan_src, h->plan_dst, h->ncol, h->stream));
    rc = copy_run(h, res.n_copies, h->plan_src, h->plan_dst, what);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  h->plan_n = res.n_copies;
  h->rs_applied = true;
  if (info) *info = samsim_apply_info{res.n_pool, res.n_free, res.n_copies, res.n_sources};
  return SAMSIM_OK;
}

int samsim_get_copy_plan(samsim_handle *h, int64_t k0, int64_t nk, int64_t *src, int64_t *dst) {
  if (!h || !src || !dst) return SAMSIM_ERR_ARG;
  if (h->plan_n < 0) return SAMSIM_ERR_ARG;
  if (k0 < 0 || nk < 0 || k0 > h->plan_n || nk > h->plan_n - k0) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (nk == 0) return SAMSIM_OK;
  HIPCHK(hipMemcpy(src, h->plan_src + (size_t)k0, sizeof(int64_t) * (size_t)nk, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(dst, h->plan_dst + (size_t)k0, sizeof(int64_t) * (size_t)nk, hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

// ---- the per-column parameters: read back, and jittered on the device (samsim_jitter.hip)
int samsim_get_ocean(samsim_handle *h, int64_t col0, int64_t ncols, double *dfl_q_bottom, double *S_bu_bottom) {
  if (!h) return SAMSIM_ERR_ARG;
  if ((dfl_q_bottom && !h->ocean_dflq) || (S_bu_bottom && !h->ocean_sbu)) return SAMSIM_ERR_ARG;
  if (col0 < 0 || ncols < 0 || col0 > h->ncol || ncols > h->ncol - col0) return SAMSIM_ERR_ARG;
  int rc = use(h);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (ncols == 0) return SAMSIM_OK;
  if (dfl_q_bottom) HIPCHK(hipMemcpy(dfl_q_bottom, h->ocean_dflq + (size_t)col0, sizeof(double) * (size_t)ncols, hipMemcpyDeviceToHost));
  if (S_bu_bottom) HIPCHK(hipMemcpy(S_bu_bottom, h->ocean_sbu + (size_t)col0, sizeof(double) * (size_t)ncols, hipMemcpyDeviceToHost));
  return SAMSIM_OK;
}

int samsim_jitter(samsim_handle *h, const samsim_jitter_spec *spec, samsim_jitter_info *info) {
  // every check first, in the order samsim.h gives (jt_check, samsim_jitter.h): a call that is refused writes nothing
  if (!h || !spec) return SAMSIM_ERR_ARG;
  int rc = jt_check(spec, h->ocean_dflq != nullptr, h->ocean_sbu != nullptr, good_group(h, spec->group), h->plan_n);
  if (rc) return rc;
  const bool copies = spec->which == SAMSIM_JITTER_COPIES;
  if (copies && h->plan_n == 0) {
    if (info) *info = samsim_jitter_info{};
    return SAMSIM_OK;
  }
  rc = use(h);
  if (rc) return rc;
  HIPCHK(scratch(&h->d_jitter, kJitterScratch));
  JtParams p{};
  for (int i = 0; i < spec->nterms; ++i) {
    p.term[i] = spec->term[i];
    switch (spec->term[i].target) {
      case SAMSIM_JT_DT2M: p.row[i] = h->scal + (size_t)SAMSIM_S_DT2M * (size_t)h->ncol; break;
      case SAMSIM_JT_PRECIP_SCALE: p.row[i] = h->scal + (size_t)SAMSIM_S_PRECIP_SCALE * (size_t)h->ncol; break;
      case SAMSIM_JT_DFL_Q_BOTTOM: p.row[i] = h->ocean_dflq; break;
      default: p.row[i] = h->ocean_sbu; break;
    }
  }
  p.status = h->status;
  p.labels = copies ? nullptr : labels_for(h, spec->group);
  p.dst = copies ? h->plan_dst : nullptr;
  p.ncol = h->ncol;
  p.n = copies ? h->plan_n : h->ncol;
  const JtGrid grid = jt_grid(p.n);
  p.per = grid.per; p.ranges = grid.ranges;
  p.seed = spec->seed; p.group = spec->group; p.nterms = spec->nterms;
  HIPCHK(samsim_launch_jitter(&p, h->d_jitter, h->stream));
  JtCounts res;
  HIPCHK(hipMemcpyAsync(&res, (const char *)h->d_jitter + DEV_JT_RESULT_AT, sizeof(JtCounts), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (info) std::memcpy(info, &res, sizeof(JtCounts));
  return SAMSIM_OK;
}

}  // extern "C"
