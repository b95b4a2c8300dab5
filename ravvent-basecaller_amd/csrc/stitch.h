// Stitching a read's chunk calls by signal position on the device (stitch.hip): what its kernels and the host
// (ravvent_hip.cpp) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int ST_THREADS = 256;                         // chunks one workgroup of the scan takes (its tile): one per thread
constexpr int ST_LANES = 64;                            // one wave per chunk, lane = column: a row holds at most this many letters

// A read as the kernels see it: its event starts and lengths [n_ev] (null in raw mode, which never reads them)
struct StRead {
  const int64_t *ev_start, *ev_len;
  int n_ev;
};

// A chunk: its window row (raw_start, raw_len, event_start, event_len), its read in the table of StRead, its place k in the read and
// the read's chunk count (k == 0: no cut below, k == n_k - 1: none above; the neighbours' rows are the chunks next to it)
struct StChunk {
  int32_t a, la, e, le;
  int32_t read, k, n_k;
};

// The call tables [n, stride] / [n] the kernels read, on the device
struct StIn {
  const uint8_t* bases;
  const float* probs;
  const int32_t* lengths;
  const float *raw_pos, *raw_mass, *event_pos, *event_mass;
  int n, stride, mode;                                  // mode: RV_MODE_*
};

// The seven per-base outputs (any may be null), on the device
struct StOut {
  uint8_t* bases;
  float* probs;
  double* positions;
  float *raw_mass, *event_mass;
  int32_t *source_chunk, *source_index;
};

// keep [n]: (first kept index, kept count) of every chunk.  off [n + 1]: the exclusive scan of the counts, entry n the total.
// tiles [n / ST_THREADS + 1]: the scan's tile sums (one more than ceil(n / ST_THREADS) when n is a multiple of the tile: entry n
// of `off` lies in a tile of its own then).  read_rows / read_off [n_reads + 1]: the first chunk of every read (ascending,
// entry n_reads = n) and, out of the same scan, the first base of every read
void st_launch_keep(const StIn& in, const StChunk* chunks, const StRead* reads, int2* keep, hipStream_t s);
void st_launch_scan(const int2* keep, int n, long long* tiles, long long* off, const int32_t* read_rows, int n_reads, long long* read_off,
                    hipStream_t s);
void st_launch_scatter(const StIn& in, const StChunk* chunks, const StRead* reads, const int2* keep, const long long* off, const StOut& out,
                       hipStream_t s);
