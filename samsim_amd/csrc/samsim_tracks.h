// samsim_tracks.h -- what samsim_tracks.hip and the C-ABI host code share about the time-domain diagnostics (samsim_set_tracks,
// samsim_get_tracks, include/samsim.h).  The step kernel does not include this header.
#ifndef SAMSIM_TRACKS_H
#define SAMSIM_TRACKS_H

#include <hip/hip_runtime.h>

#include "samsim_device.h"

// one track as the sampling kernel sees it: samsim_track_spec, checked by samsim_set_tracks
struct TrackDev {
  int32_t kind;     // enum samsim_observable_kind
  int32_t id;       // SCALAR: row of the scalar block; LAYER: array of the layer block
  int32_t layer;    // LAYER: k >= 1 from the top, k <= -1 from the bottom
  int32_t sense;    // 0, +1 (x >= threshold), -1 (x < threshold)
  double threshold;
};

// One sample: every track of the handle for the 64-column blocks [block0, block0 + nblocks), one wave per block.  Passed by value
// as the kernel's argument (no parameter ring: a sample may follow a launch on either stream).
struct TrackParams {
  const double *lay;          // layer block, DEV_LAY_INDEX
  const double *scal;         // [SAMSIM_NSCAL][ncol]
  const int32_t *n_active, *status, *flags;
  double *rows;               // [ntracks][SAMSIM_NTF][ncol]
  long long ncol;
  long long block0;
  double step;                // the sample time s = clock.step after the launch the sample follows, as the rows store it
  int32_t N;                  // nlayer
  int32_t ntracks;
  int32_t need_thick;         // some track is ICE_THICKNESS: the walk reads thick
  int32_t need_salt;          // some track is BULK_SALINITY: the walk reads S_abs and m
  TrackDev t[SAMSIM_MAX_TRACKS];
};
static_assert(sizeof(TrackParams) <= 512, "the sample's parameters travel as a kernel argument");

// the initial value of field f of a track (samsim.h)
static inline double dev_track_initial(int f) {
  switch (f) {
    case SAMSIM_TF_MIN: return __builtin_inf();
    case SAMSIM_TF_MAX: return -__builtin_inf();
    case SAMSIM_TF_STEP_MIN: case SAMSIM_TF_STEP_MAX: case SAMSIM_TF_STEP_FIRST: case SAMSIM_TF_STEP_LAST: return -1.0;
    default: return 0.0;
  }
}

// samsim_tracks.hip: enqueues one sample of nblocks blocks on `stream`
extern "C" hipError_t samsim_launch_track_sample(const TrackParams *p, long long nblocks, hipStream_t stream);

#endif
