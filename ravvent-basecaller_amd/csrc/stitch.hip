// Stitching a read's chunk calls by signal position: every chunk owns the stretch of signal around its own
// centre, a called base belongs to the chunk that owns the sample it lies on, and the read is the kept bases of its chunks in order.
// Parallel over chunks: no alignment, no chain from chunk to chunk.  tests/stitch_reference.py states the rule in numpy.
//
// Exactness.  A position is basecaller.signal_positions in fp64, operation by operation: this file is compiled with -ffp-contract=off, so
// that `c_i + (e - i) * (c_j - c_i)` stays a product and a sum.  The centres m = a + la / 2 and the cuts (m' + m) / 2 of int32 window rows
// are exact quarter samples.  Nothing is summed over bases: the result does not depend on any order, and no atomics are used.
#include "stitch.h"
#include <math.h>

namespace {

constexpr int ST_MODE_RAW = 0, ST_MODE_EVENT = 1;      // RV_MODE_* of include/ravvent_hip.h (2: joint)
constexpr int ST_WAVES = ST_THREADS / ST_LANES;        // chunks one workgroup of the keep and scatter kernels takes

// signal_positions: the raw estimate a + raw_pos (+ the offset 0), the event estimate between the centres of neighbouring events, and
// in joint mode the raw one where raw_mass >= event_mass (a NaN mass compares false: the event estimate)
__device__ inline double st_position(int mode, const StChunk& ck, const StRead& rd, float rp, float rm, float ep, float em) {
  const double raw = (double)ck.a + (double)rp + 0.0;
  if (mode == ST_MODE_RAW) return raw;
  double ev = __longlong_as_double(0x7ff8000000000000ll);
  const double e = (double)ck.e + (double)ep;
  const int E = rd.n_ev;
  if (E > 0 && e == e) {
    double fe = floor(e);                               // clip(floor(e), 0, E - 1)
    fe = fe < 0. ? 0. : fe;
    fe = fe > (double)(E - 1) ? (double)(E - 1) : fe;
    const long long i = (long long)fe, j = i + 1 < E ? i + 1 : E - 1;
    const double ci = (double)rd.ev_start[i] + (double)rd.ev_len[i] / 2.0, cj = (double)rd.ev_start[j] + (double)rd.ev_len[j] / 2.0;
    ev = ci + (e - (double)i) * (cj - ci);
  }
  if (mode == ST_MODE_EVENT) return ev;
  return rm >= em ? raw : ev;
}

__device__ inline double st_centre(const StChunk& ck) { return (double)ck.a + 0.5 * (double)ck.la; }

// A chunk's letters: its length clamped into [0, stride] (and to the wave) before it indexes anything
__device__ inline int st_len(const StIn& in, int c) { return min(max(in.lengths[c], 0), min(in.stride, ST_LANES)); }

__device__ inline double st_position_at(const StIn& in, const StChunk& ck, const StRead* reads, size_t i) {
  return st_position(in.mode, ck, reads[ck.read], in.raw_pos[i], in.raw_mass[i], in.event_pos[i], in.event_mass[i]);
}

// ---- positions and keep ranges: one wave per chunk, lane = column.  inside = lo <= p < hi (a NaN is never inside); the first and the
// last inside lane bound what the chunk keeps (the hull), and their distance is its count
__global__ void __launch_bounds__(ST_THREADS) k_st_keep(StIn in, const StChunk* chunks, const StRead* reads, int2* keep) {
  const int c = blockIdx.x * ST_WAVES + (threadIdx.x / ST_LANES), lane = threadIdx.x % ST_LANES;
  if (c >= in.n) return;                                // (uniform over the wave)
  const StChunk ck = chunks[c];
  const double m = st_centre(ck);
  double lo = -INFINITY, hi = INFINITY;
  if (ck.k > 0 && c > 0) lo = 0.5 * (st_centre(chunks[c - 1]) + m);
  if (ck.k < ck.n_k - 1 && c + 1 < in.n) hi = 0.5 * (m + st_centre(chunks[c + 1]));
  bool inside = false;
  if (lane < st_len(in, c)) {
    const double p = st_position_at(in, ck, reads, (size_t)c * in.stride + lane);
    inside = lo <= p && p < hi;
  }
  const unsigned long long mask = __ballot(inside);
  if (lane == 0) {
    const int f = mask ? __ffsll((long long)mask) - 1 : 0, l = mask ? 63 - __clzll((long long)mask) : -1;
    keep[c] = make_int2(f, l - f + 1);
  }
}

// ---- exclusive scan of the counts over all chunks of the call (signal_prep.hip's pattern): tile sums, their exclusive scan by one
// workgroup, then the scan inside each tile.  Entry n of `off` is the total; tiles = n / ST_THREADS + 1 covers it
__device__ inline long long block_scan(long long v, long long* l) {      // inclusive, over the workgroup's threads
  const int t = threadIdx.x;
  l[t] = v;
  __syncthreads();
  for (int d = 1; d < ST_THREADS; d <<= 1) {
    const long long x = t >= d ? l[t - d] : 0;
    __syncthreads();
    l[t] += x;
    __syncthreads();
  }
  const long long r = l[t];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(ST_THREADS) k_st_scan_tiles(const int2* keep, int n, long long* tiles) {
  __shared__ long long l[ST_THREADS];
  const long long c = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  const long long s = block_scan(c < n ? (long long)keep[c].y : 0, l);
  if (threadIdx.x == ST_THREADS - 1) tiles[blockIdx.x] = s;
}

__global__ void __launch_bounds__(ST_THREADS) k_st_scan_carry(long long* tiles, int ntile) {
  __shared__ long long l[ST_THREADS];
  const int per = (ntile + ST_THREADS - 1) / ST_THREADS;
  const int a = min((int)threadIdx.x * per, ntile), b = min(a + per, ntile);
  long long s = 0;
  for (int i = a; i < b; ++i) s += tiles[i];
  long long e = block_scan(s, l) - s;
  for (int i = a; i < b; ++i) { const long long v = tiles[i]; tiles[i] = e; e += v; }
}

// off[c] for c = 0 .. n; and the per-read offsets out of the same values: the thread of entry c serves every read whose first chunk is c
// (read_rows ascends, so they stand together; an empty read shares its entry with the next one)
__global__ void __launch_bounds__(ST_THREADS) k_st_scan_offsets(const int2* keep, int n, const long long* tiles, long long* off,
                                                                const int32_t* read_rows, int n_reads, long long* read_off) {
  __shared__ long long l[ST_THREADS];
  const long long c = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
  const long long v = c < n ? (long long)keep[c].y : 0;
  const long long o = tiles[blockIdx.x] + block_scan(v, l) - v;
  if (c > n) return;
  off[c] = o;
  int lo = 0, hi = n_reads + 1;                         // the first entry of read_rows that is >= c
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (read_rows[mid] < c) lo = mid + 1; else hi = mid; }
  for (int r = lo; r <= n_reads && read_rows[r] == c; ++r) read_off[r] = o;
}

// ---- scatter: one wave per chunk; lane i of [f, f + count) writes its seven values at off + i - f.  Each output element is written once
__global__ void __launch_bounds__(ST_THREADS) k_st_scatter(StIn in, const StChunk* chunks, const StRead* reads, const int2* keep,
                                                           const long long* off, StOut out) {
  const int c = blockIdx.x * ST_WAVES + (threadIdx.x / ST_LANES), lane = threadIdx.x % ST_LANES;
  if (c >= in.n) return;
  const int2 kp = keep[c];
  const int len = st_len(in, c);
  if (lane < kp.x || lane >= kp.x + kp.y || lane >= len) return;
  const StChunk ck = chunks[c];
  const size_t i = (size_t)c * in.stride + lane;
  const long long o = off[c] + (lane - kp.x);
  if (out.bases) out.bases[o] = in.bases[i];
  if (out.probs) out.probs[o] = in.probs[i];
  if (out.positions) out.positions[o] = st_position_at(in, ck, reads, i);
  if (out.raw_mass) out.raw_mass[o] = in.raw_mass[i];
  if (out.event_mass) out.event_mass[o] = in.event_mass[i];
  if (out.source_chunk) out.source_chunk[o] = ck.k;
  if (out.source_index) out.source_index[o] = lane;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

}  // namespace

void st_launch_keep(const StIn& in, const StChunk* chunks, const StRead* reads, int2* keep, hipStream_t s) {
  if (in.n > 0) hipLaunchKernelGGL(k_st_keep, dim3(cdiv(in.n, ST_WAVES)), dim3(ST_THREADS), 0, s, in, chunks, reads, keep);
}
void st_launch_scan(const int2* keep, int n, long long* tiles, long long* off, const int32_t* read_rows, int n_reads, long long* read_off,
                    hipStream_t s) {
  const int ntile = n / ST_THREADS + 1;
  hipLaunchKernelGGL(k_st_scan_tiles, dim3(ntile), dim3(ST_THREADS), 0, s, keep, n, tiles);
  hipLaunchKernelGGL(k_st_scan_carry, dim3(1), dim3(ST_THREADS), 0, s, tiles, ntile);
  hipLaunchKernelGGL(k_st_scan_offsets, dim3(ntile), dim3(ST_THREADS), 0, s, keep, n, (const long long*)tiles, off, read_rows, n_reads, read_off);
}
void st_launch_scatter(const StIn& in, const StChunk* chunks, const StRead* reads, const int2* keep, const long long* off, const StOut& out,
                       hipStream_t s) {
  if (in.n > 0) hipLaunchKernelGGL(k_st_scatter, dim3(cdiv(in.n, ST_WAVES)), dim3(ST_THREADS), 0, s, in, chunks, reads, keep, off, out);
}
