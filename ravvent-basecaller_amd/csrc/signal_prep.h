// Signal preparation on the device (signal_prep.hip): what its kernels and the host (ravvent_hip.cpp) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int SP_THREADS = 256;
constexpr int SP_PER_THREAD = 8;
constexpr int SP_TILE = SP_THREADS * SP_PER_THREAD;     // samples one workgroup of the scan takes
constexpr int SP_MAX_SAMPLES = 1 << 22;                 // with |x| <= 32768 every running sum of x^2 stays below 2^53: exact in fp64
constexpr int SP_FIT = 12;                              // per read: event feature means [5], scales [5], raw mean, raw scale

struct SpParams {
  int w1, w2;
  double threshold1, threshold2, peak_height;
  int stride, max_raw_len, max_event_len;
};

// One read of a batch as the kernels see it.  off: its first element in the per-sample arrays of the batch, where it takes n + 1
// (prefix sums: entry 0 is the empty sum); tile0 / ntile: its tiles in the per-tile arrays.  The members below n_ev are set by the host
// between the peak pass and the event kernels, when the number of events is known
struct SpRead {
  long long off;
  int n, tile0, ntile, n_ev;
  int64_t *ev_start, *ev_len;
  double *ev_mean, *ev_stdv;
  float *raw_sc, *ev_sc;
  int32_t* win;
};

// The scratch of a batch (the handle's, reused and grown): per sample x, ps / pq (prefix sums of x and x^2), t1 / t2 (t-statistics of
// both windows), bounds (per event: the uint32 end index and the clock it was made at); per tile the sums of x, x^2 [2] and of the
// squared deviations; per read the counts and the fits
struct SpScratch {
  const int16_t* x;
  double *ps, *pq, *t1, *t2;
  uint2* bounds;
  long long* tile_sums;
  double* var_part;
  int *n_ev, *n_win;
  double* fit;
};

// Stages in launch order.  scan .. peaks run before the event counts are known (they set n_ev[r]); the host then fills the output
// addresses of `reads` and runs events .. windows (windows sets n_win[r], zeroed by the caller).  max_tiles / max_ev / max_win: the
// largest of the batch, which size the grids
void sp_launch_scan(const SpRead* reads, int n_reads, int max_tiles, const SpScratch& sc, hipStream_t s);
void sp_launch_tstat(const SpRead* reads, int n_reads, int max_tiles, const SpScratch& sc, const SpParams& p, hipStream_t s);
void sp_launch_peaks(const SpRead* reads, int n_reads, const SpScratch& sc, const SpParams& p, hipStream_t s);
void sp_launch_events(const SpRead* reads, int n_reads, int max_ev, const SpScratch& sc, const SpParams& p, hipStream_t s);
void sp_launch_fit(const SpRead* reads, int n_reads, const SpScratch& sc, hipStream_t s);
void sp_launch_raw_scale(const SpRead* reads, int n_reads, int max_tiles, const SpScratch& sc, hipStream_t s);
void sp_launch_windows(const SpRead* reads, int n_reads, int max_win, const SpScratch& sc, const SpParams& p, hipStream_t s);
