// Signal preparation on the device: from a batch of reads as int16 ADC samples to each read's events, its two
// scaled tables and its window table -- what data_loader.prepare_windows makes on the host for an unlabelled read.
//
// Exactness.  The samples are integers, |x| <= 32768, n <= 2^22: every running sum of x and of x^2 is an integer below 2^53, exact in
// fp64 in any summation order.  So the multi-block scan below (in int64) yields the very values the host detector's ring of running
// sums holds, and every later operation of the detector is event_core.h's -- the same IEEE fp64 operation on the same operands.  This
// file is compiled with -ffp-contract=off: `sumsq / len - m * m` must not become an fma.
//
// The ring.  The host keeps the sums in a ring of buf_len = 1 + 2 w2 slots; slot j holds the sums of the latest clock t' <= tw with
// t' = j (mod buf_len), tw = the last clock written, or 0 while no such clock has been (slot 0: the empty sum, also 0).  ring() reads
// exactly that from the prefix array, so the start-up reads of wrapped uint32 indices (small t) come out as on the host.
#include "common.h"
#include "event_core.h"
#include "signal_prep.h"

namespace {

using namespace evcore;

__device__ inline double ring(const double* P, uint32_t slot, uint32_t tw, uint32_t buf_len) {
  return tw >= slot ? P[slot + buf_len * ((tw - slot) / buf_len)] : 0.;      // (the index is <= tw <= n: inside the read's n + 1 entries)
}

// Inclusive scan of (a, b) over the workgroup's threads
__device__ inline void block_scan2(long long& a, long long& b, long long* la, long long* lb) {
  const int t = threadIdx.x;
  la[t] = a; lb[t] = b;
  __syncthreads();
  for (int d = 1; d < SP_THREADS; d <<= 1) {
    const long long xa = t >= d ? la[t - d] : 0, xb = t >= d ? lb[t - d] : 0;
    __syncthreads();
    la[t] += xa; lb[t] += xb;
    __syncthreads();
  }
  a = la[t]; b = lb[t];
  __syncthreads();
}

// Sum over the workgroup's threads in one fixed tree order
template <class T>
__device__ inline T block_sum(T v, T* l) {
  const int t = threadIdx.x;
  l[t] = v;
  __syncthreads();
  for (int d = SP_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) l[t] += l[t + d];
    __syncthreads();
  }
  const T r = l[0];
  __syncthreads();
  return r;
}

// ---- prefix sums of x and x^2: tile sums, their exclusive scan per read, then the scan inside each tile
__global__ void __launch_bounds__(SP_THREADS) k_sp_tile_sums(const SpRead* reads, SpScratch sc) {
  __shared__ long long l[SP_THREADS];
  const SpRead rd = reads[blockIdx.y];
  const int tile = blockIdx.x;
  if (tile >= rd.ntile) return;
  const int16_t* x = sc.x + rd.off;
  long long s = 0, q = 0;
  const int k0 = tile * SP_TILE + threadIdx.x * SP_PER_THREAD;
  for (int j = 0; j < SP_PER_THREAD; ++j)
    if (k0 + j < rd.n) { const long long v = x[k0 + j]; s += v; q += v * v; }
  s = block_sum(s, l);
  q = block_sum(q, l);
  if (threadIdx.x == 0) { sc.tile_sums[2 * (size_t)(rd.tile0 + tile)] = s; sc.tile_sums[2 * (size_t)(rd.tile0 + tile) + 1] = q; }
}

// One workgroup per read: its tile sums become exclusive prefixes in place; the raw mean = (sum of x) / n, exact sum
__global__ void __launch_bounds__(SP_THREADS) k_sp_tile_scan(const SpRead* reads, SpScratch sc) {
  __shared__ long long la[SP_THREADS], lb[SP_THREADS];
  const SpRead rd = reads[blockIdx.x];
  long long* ts = sc.tile_sums + 2 * (size_t)rd.tile0;
  const int c = (rd.ntile + SP_THREADS - 1) / SP_THREADS;
  const int a = min(threadIdx.x * c, rd.ntile), b = min(a + c, rd.ntile);
  long long s = 0, q = 0;
  for (int i = a; i < b; ++i) { s += ts[2 * i]; q += ts[2 * i + 1]; }
  long long is = s, iq = q;
  block_scan2(is, iq, la, lb);
  long long es = is - s, eq = iq - q;
  for (int i = a; i < b; ++i) {
    const long long vs = ts[2 * i], vq = ts[2 * i + 1];
    ts[2 * i] = es; ts[2 * i + 1] = eq;
    es += vs; eq += vq;
  }
  if (threadIdx.x == SP_THREADS - 1) sc.fit[(size_t)blockIdx.x * SP_FIT + 10] = rd.n > 0 ? (double)is / (double)rd.n : 0.;
}

// ps[k + 1], pq[k + 1] = the sums of the first k + 1 samples; and the tile's sum of squared deviations from the raw mean
__global__ void __launch_bounds__(SP_THREADS) k_sp_prefix(const SpRead* reads, SpScratch sc) {
  __shared__ long long la[SP_THREADS], lb[SP_THREADS];
  __shared__ double ld[SP_THREADS];
  const SpRead rd = reads[blockIdx.y];
  const int tile = blockIdx.x;
  if (tile >= rd.ntile) return;
  const int16_t* x = sc.x + rd.off;
  double *ps = sc.ps + rd.off, *pq = sc.pq + rd.off;
  const double mean = sc.fit[(size_t)blockIdx.y * SP_FIT + 10];
  const int k0 = tile * SP_TILE + threadIdx.x * SP_PER_THREAD;
  long long v[SP_PER_THREAD];
  long long s = 0, q = 0;
  double dev = 0.;
  for (int j = 0; j < SP_PER_THREAD; ++j) {
    v[j] = k0 + j < rd.n ? (long long)x[k0 + j] : 0;
    s += v[j]; q += v[j] * v[j];
    if (k0 + j < rd.n) { const double d = (double)v[j] - mean; dev += d * d; }
  }
  long long is = s, iq = q;
  block_scan2(is, iq, la, lb);
  long long rs = sc.tile_sums[2 * (size_t)(rd.tile0 + tile)] + is - s, rq = sc.tile_sums[2 * (size_t)(rd.tile0 + tile) + 1] + iq - q;
  for (int j = 0; j < SP_PER_THREAD; ++j) {
    rs += v[j]; rq += v[j] * v[j];
    if (k0 + j < rd.n) { ps[k0 + j + 1] = (double)rs; pq[k0 + j + 1] = (double)rq; }
  }
  if (tile == 0 && threadIdx.x == 0) { ps[0] = 0.; pq[0] = 0.; }
  dev = block_sum(dev, ld);
  if (threadIdx.x == 0) sc.var_part[rd.tile0 + tile] = dev;
}

// ---- the t-statistics of both windows after every sample: independent per sample
__device__ inline double tstat_at(const double* ps, const double* pq, uint32_t t, uint32_t buf_mid, int w, int w2, int buf_len) {
  if (tstat_is_zero(t, w)) return 0.;
  const uint32_t tw = t - 1u;
  if (tw >= (uint32_t)(w2 + w)) {      // past the start-up: buf_mid - w >= 0, and all three clocks lie inside the ring's last buf_len
    return tstat(ps[buf_mid - w], pq[buf_mid - w], ps[buf_mid], pq[buf_mid], ps[buf_mid + w], pq[buf_mid + w], w);
  }
  const TstatSlots k = tstat_slots(buf_mid, w, buf_len);
  return tstat(ring(ps, k.st, tw, buf_len), ring(pq, k.st, tw, buf_len), ring(ps, k.i, tw, buf_len), ring(pq, k.i, tw, buf_len),
               ring(ps, k.en, tw, buf_len), ring(pq, k.en, tw, buf_len), w);
}

__global__ void __launch_bounds__(SP_THREADS) k_sp_tstat(const SpRead* reads, SpScratch sc, SpParams p) {
  const SpRead rd = reads[blockIdx.y];
  const int k = blockIdx.x * SP_THREADS + threadIdx.x;
  if (k >= rd.n) return;
  const int buf_len = 1 + 2 * p.w2;
  const uint32_t t = (uint32_t)k + 2u, buf_mid = buf_mid_of(t, buf_len);
  const double *ps = sc.ps + rd.off, *pq = sc.pq + rd.off;
  sc.t1[rd.off + k] = tstat_at(ps, pq, t, buf_mid, p.w1, p.w2, buf_len);
  sc.t2[rd.off + k] = tstat_at(ps, pq, t, buf_mid, p.w2, p.w2, buf_len);
}

// ---- the peak detector: a sequential state machine, run as it is written by one wave per read.  The lanes fetch the next 64 samples'
// t-statistics while the wave steps through the current 64; the state is uniform over the wave.  An event here is its end index and the
// clock it was made at (its sums are read from the prefix arrays afterwards, in parallel: k_sp_events)
__device__ inline double lane_value(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

__global__ void __launch_bounds__(64) k_sp_peaks(const SpRead* reads, SpScratch sc, SpParams p) {
  const SpRead rd = reads[blockIdx.x];
  const int lane = threadIdx.x, n = rd.n;
  const double *t1 = sc.t1 + rd.off, *t2 = sc.t2 + rd.off;
  uint2* bounds = sc.bounds + rd.off;
  const int buf_len = 1 + 2 * p.w2;
  const bool long_is_short = p.w1 == p.w2;
  Detector sd = make_detector(p.threshold1, p.w1), ld = make_detector(p.threshold2, p.w2);
  int64_t evt_st = 0;
  int cnt = 0;
  double a1 = lane < n ? t1[lane] : 0., a2 = lane < n ? t2[lane] : 0.;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const double c1 = a1, c2 = a2;
    const int nk = k0 + 64 + lane;
    a1 = nk < n ? t1[nk] : 0.; a2 = nk < n ? t2[nk] : 0.;
    const int m = min(64, n - k0);
    for (int j = 0; j < m; ++j) {
      const double u1 = lane_value(c1, j), u2 = lane_value(c2, j);
      const uint32_t t = (uint32_t)(k0 + j) + 2u, buf_mid = buf_mid_of(t, buf_len);
      const bool p1 = detect_peak(u1, sd, ld, true, buf_mid, p.peak_height);
      const bool p2 = detect_peak(u2, ld, ld, long_is_short, buf_mid, p.peak_height);
      if (p1 || p2) {
        const uint32_t evt_en = evt_en_of(buf_mid, p.w1);
        if (event_len(evt_en, evt_st) < kFltMin) continue;
        if (lane == 0) bounds[cnt] = make_uint2(evt_en, t - 1u);      // (at most one event per sample: cnt < n)
        ++cnt;
        evt_st = (int64_t)evt_en;
      }
    }
  }
  if (lane == 0) sc.n_ev[blockIdx.x] = cnt;
}

// ---- the events' four arrays, one thread per event (_create_event: the sums at its end, and those kept from the event before)
__global__ void __launch_bounds__(SP_THREADS) k_sp_events(const SpRead* reads, SpScratch sc, SpParams p) {
  const SpRead rd = reads[blockIdx.y];
  const int e = blockIdx.x * SP_THREADS + threadIdx.x;
  if (e >= rd.n_ev) return;
  const uint32_t buf_len = 1u + 2u * (uint32_t)p.w2;
  const double *ps = sc.ps + rd.off, *pq = sc.pq + rd.off;
  const uint2* bounds = sc.bounds + rd.off;
  const uint2 b = bounds[e];
  int64_t evt_st = 0;
  double s_st = 0., q_st = 0.;
  if (e > 0) {
    const uint2 a = bounds[e - 1];
    evt_st = (int64_t)a.x;
    s_st = ring(ps, a.x % buf_len, a.y, buf_len); q_st = ring(pq, a.x % buf_len, a.y, buf_len);
  }
  const double len = event_len(b.x, evt_st);
  double m, v;
  event_stats(ring(ps, b.x % buf_len, b.y, buf_len), ring(pq, b.x % buf_len, b.y, buf_len), s_st, q_st, len, &m, &v);
  rd.ev_start[e] = evt_st; rd.ev_len[e] = (int64_t)len; rd.ev_mean[e] = m; rd.ev_stdv[e] = v;
}

// ---- the two StandardScaler fits, one workgroup per read, every sum in one fixed order; then the scaled event table.  Features as
// prepare_windows forms them: (length, mean, stdv, mean^2, mean - the mean before, 0 for the first)
__device__ inline void event_features(const SpRead& rd, int e, double f[5]) {
  const double mu = rd.ev_mean[e];
  f[0] = (double)rd.ev_len[e]; f[1] = mu; f[2] = rd.ev_stdv[e]; f[3] = mu * mu; f[4] = e > 0 ? mu - rd.ev_mean[e - 1] : 0.;
}

__global__ void __launch_bounds__(SP_THREADS) k_sp_fit(const SpRead* reads, SpScratch sc) {
  __shared__ double l[SP_THREADS];
  const SpRead rd = reads[blockIdx.x];
  double* fit = sc.fit + (size_t)blockIdx.x * SP_FIT;
  const int E = rd.n_ev;
  double mean[5] = {0., 0., 0., 0., 0.}, scale[5] = {1., 1., 1., 1., 1.}, f[5];
  if (E > 0) {
    double s[5] = {0., 0., 0., 0., 0.};
    for (int e = threadIdx.x; e < E; e += SP_THREADS) {
      event_features(rd, e, f);
      for (int c = 0; c < 5; ++c) s[c] += f[c];
    }
    for (int c = 0; c < 5; ++c) mean[c] = block_sum(s[c], l) / (double)E;
    for (int c = 0; c < 5; ++c) s[c] = 0.;
    for (int e = threadIdx.x; e < E; e += SP_THREADS) {
      event_features(rd, e, f);
      for (int c = 0; c < 5; ++c) { const double d = f[c] - mean[c]; s[c] += d * d; }
    }
    for (int c = 0; c < 5; ++c) {
      const double sd = sqrt(block_sum(s[c], l) / (double)E);
      scale[c] = sd == 0. ? 1. : sd;
    }
    for (int e = threadIdx.x; e < E; e += SP_THREADS) {
      event_features(rd, e, f);
      for (int c = 0; c < 5; ++c) rd.ev_sc[(size_t)e * 5 + c] = (float)((f[c] - mean[c]) / scale[c]);
    }
  }
  double v = 0.;
  for (int i = threadIdx.x; i < rd.ntile; i += SP_THREADS) v += sc.var_part[rd.tile0 + i];
  v = block_sum(v, l);
  if (threadIdx.x == 0) {
    for (int c = 0; c < 5; ++c) { fit[c] = mean[c]; fit[5 + c] = scale[c]; }
    const double sd = rd.n > 0 ? sqrt(v / (double)rd.n) : 0.;
    fit[11] = sd == 0. ? 1. : sd;
  }
}

__global__ void __launch_bounds__(SP_THREADS) k_sp_raw_scale(const SpRead* reads, SpScratch sc) {
  const SpRead rd = reads[blockIdx.y];
  const int k = blockIdx.x * SP_THREADS + threadIdx.x;
  if (k >= rd.n) return;
  const double* fit = sc.fit + (size_t)blockIdx.y * SP_FIT;
  rd.raw_sc[k] = (float)(((double)sc.x[rd.off + k] - fit[10]) / fit[11]);
}

// ---- the window table in closed form, one thread per chunk.  C[j], the sum of the event lengths up to and including j, is event j's
// end: events are contiguous from sample 0 by construction (an event starts where the one before ended)
__global__ void __launch_bounds__(SP_THREADS) k_sp_windows(const SpRead* reads, SpScratch sc, SpParams p) {
  const SpRead rd = reads[blockIdx.y];
  const int k = blockIdx.x * SP_THREADS + threadIdx.x;
  const int E = rd.n_ev;
  const long long i = (long long)k * p.stride;
  if (i >= E) return;
  auto C = [&](int j) { return (long long)(rd.ev_start[j] + rd.ev_len[j]); };
  if (C(0) > p.max_raw_len) return;                     // an oversized first event: the loop stops at once, no windows at all
  const long long target = (i > 0 ? C((int)i - 1) : 0) + p.max_raw_len;
  int lo = 0, hi = E;                                   // end = the first j with C[j] > target
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (C(mid) > target) hi = mid; else lo = mid + 1; }
  if (lo >= E) return;                                  // the tail fits: the table ends before this chunk
  const int end = lo;                                   // (>= 1: C[0] <= max_raw_len <= target)
  const long long N = rd.n;
  const long long ra = min(max((long long)(int32_t)rd.ev_start[i], 0ll), N), rb = min(max((long long)(int32_t)rd.ev_start[end - 1], 0ll), N);
  int32_t* w = rd.win + (size_t)k * 4;
  w[0] = (int32_t)ra; w[1] = (int32_t)min(max(rb - ra, 0ll), (long long)p.max_raw_len);
  w[2] = (int32_t)i; w[3] = (int32_t)min(max((long long)end - i, 0ll), (long long)p.max_event_len);
  atomicMax(&sc.n_win[blockIdx.y], k + 1);              // (valid chunks are a prefix: base grows with k)
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

}  // namespace

void sp_launch_scan(const SpRead* reads, int n_reads, int max_tiles, const SpScratch& sc, hipStream_t s) {
  if (max_tiles > 0) hipLaunchKernelGGL(k_sp_tile_sums, dim3(max_tiles, n_reads), dim3(SP_THREADS), 0, s, reads, sc);
  hipLaunchKernelGGL(k_sp_tile_scan, dim3(n_reads), dim3(SP_THREADS), 0, s, reads, sc);
  if (max_tiles > 0) hipLaunchKernelGGL(k_sp_prefix, dim3(max_tiles, n_reads), dim3(SP_THREADS), 0, s, reads, sc);
}
void sp_launch_tstat(const SpRead* reads, int n_reads, int max_tiles, const SpScratch& sc, const SpParams& p, hipStream_t s) {
  if (max_tiles > 0) hipLaunchKernelGGL(k_sp_tstat, dim3(max_tiles * SP_PER_THREAD, n_reads), dim3(SP_THREADS), 0, s, reads, sc, p);
}
void sp_launch_peaks(const SpRead* reads, int n_reads, const SpScratch& sc, const SpParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_sp_peaks, dim3(n_reads), dim3(64), 0, s, reads, sc, p);
}
void sp_launch_events(const SpRead* reads, int n_reads, int max_ev, const SpScratch& sc, const SpParams& p, hipStream_t s) {
  if (max_ev > 0) hipLaunchKernelGGL(k_sp_events, dim3(cdiv(max_ev, SP_THREADS), n_reads), dim3(SP_THREADS), 0, s, reads, sc, p);
}
void sp_launch_fit(const SpRead* reads, int n_reads, const SpScratch& sc, hipStream_t s) {
  hipLaunchKernelGGL(k_sp_fit, dim3(n_reads), dim3(SP_THREADS), 0, s, reads, sc);
}
void sp_launch_raw_scale(const SpRead* reads, int n_reads, int max_tiles, const SpScratch& sc, hipStream_t s) {
  if (max_tiles > 0) hipLaunchKernelGGL(k_sp_raw_scale, dim3(max_tiles * SP_PER_THREAD, n_reads), dim3(SP_THREADS), 0, s, reads, sc);
}
void sp_launch_windows(const SpRead* reads, int n_reads, int max_win, const SpScratch& sc, const SpParams& p, hipStream_t s) {
  if (max_win > 0) hipLaunchKernelGGL(k_sp_windows, dim3(cdiv(max_win, SP_THREADS), n_reads), dim3(SP_THREADS), 0, s, reads, sc, p);
}
