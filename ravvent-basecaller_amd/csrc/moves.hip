// The moves of a call: where in the attention memory each token of each of the W hypotheses comes from.
//
// Every decode form leaves one record per (step, chunk, beam row) in DecState::step_moves (common.h): the raw and the event segment's
// attention mass and first moment, and the peak.  The row is the one the attention of that step ran on -- before the step's top-k
// reordered the rows -- so the token a hypothesis holds in slot p_t at column t was produced from row parent_ids[t][b][p_t] of step t
// (TFA's decoder step computes the alignments before its beam step reorders the rows: SURVEY.md A.5).  k_dec_finalize_moves runs the
// back-trace of k_dec_finalize_beams (beams.hip) -- the same S, So, Lb and slot chain -- and hands out that row's record per column.
// k_dec_finalize_calls_moves does the same for the best hypothesis of a call with fused post-processing and compacts the values like the
// letters (rv_beam_search_*calls_moves); k_forced_moves hands out the records of a forced decode, one beam row, no back-trace
// (rv_teacher_forced_moves*).  DESIGN.md section 18.
#include "common.h"

// One 64-thread workgroup per chunk.  LDS: the chunk's parents and the slots of the back-trace, [64 steps][RV_MAX_BEAM] ints each
// (4 KB); the records themselves are read from global memory where they are used.
__global__ __launch_bounds__(64) void k_dec_finalize_moves(DecState d, MovesOut o) {
  __shared__ int s_par[64 * RV_MAX_BEAM], s_row[64 * RV_MAX_BEAM];
  __shared__ int s_S;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int steps = d.L - 1, W = d.W;
  if (d.chunk_steps) {
    int m = 0;
    for (int i = tid; i < d.B; i += 64) m = max(m, d.chunk_steps[i]);
    for (int x = 32; x > 0; x >>= 1) m = max(m, __shfl_xor(m, x));
    if (tid == 0) s_S = m;
    __syncthreads();
  }
  // (S_dev is read only: k_dec_finalize_beams of the same part ran before this kernel and left it)
  const int S = min(max(d.chunk_steps ? s_S : d.S_dev[0], 0), steps);
  const int So = min(max(d.chunk_steps ? d.chunk_steps[b] : d.S_dev[1 + d.part], 0), S);
  for (int i = tid; i < So * W; i += 64) s_par[i] = d.parent_ids[((size_t)(i / W) * d.B + b) * W + i % W];
  const int len = tid < W ? d.lengths[(size_t)b * W + tid] : 0;
  int maxlen = len;
  for (int x = 32; x > 0; x >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, x));
  const int Lb = min(So, maxlen);
  __syncthreads();
  if (tid < W) {
    const int w = tid;
    int p = w;
    for (int t = Lb - 1; t >= 0; --t) {
      p = min(max(p, 0), W - 1);
      const int par = s_par[t * W + p];
      // the record's row: the parent of the slot, or -1 for a column the hypothesis does not own
      s_row[t * W + w] = t < len ? min(max(par, 0), W - 1) : -1;
      p = par;
    }
  }
  __syncthreads();
  const size_t row = (size_t)b * steps * W;
  for (int i = tid; i < steps * W; i += 64) {
    const int s = i / W;
    const int r = s < Lb ? s_row[i] : -1;
    float rp = -1.f, rm = 0.f, ep = -1.f, em = 0.f, pw = 0.f;
    int pk = -1;
    if (r >= 0) {
      const float* m = d.step_moves + (((size_t)s * d.B + b) * W + r) * RV_MOVE_COLS;
      rm = m[0]; em = m[2]; pw = m[4]; pk = (int)m[5];
      // mass == 0 ? -1 : m1 / mass, the IEEE division (correctly rounded; a NaN mass divides to NaN)
      rp = rm == 0.f ? -1.f : m[1] / rm;
      ep = em == 0.f ? -1.f : m[3] / em;
    }
    if (o.raw_pos) o.raw_pos[row + i] = rp;
    if (o.raw_mass) o.raw_mass[row + i] = rm;
    if (o.event_pos) o.event_pos[row + i] = ep;
    if (o.event_mass) o.event_mass[row + i] = em;
    if (o.peak) o.peak[row + i] = pk;
    if (o.peak_weight) o.peak_weight[row + i] = pw;
  }
}

void launch_dec_finalize_moves(const DecState& d, const MovesOut& o, hipStream_t s) {
  hipLaunchKernelGGL(k_dec_finalize_moves, dim3(d.B), dim3(64), 0, s, d, o);
}

// A record as the six values a caller sees; r < 0: a column nobody owns (positions -1, masses and peak weight 0, peak -1)
struct MoveVals { float rp, rm, ep, em, pw; int pk; };
__device__ __forceinline__ MoveVals move_vals(const float* m) {
  MoveVals v{-1.f, 0.f, -1.f, 0.f, 0.f, -1};
  if (m) {
    v.rm = m[0]; v.em = m[2]; v.pw = m[4]; v.pk = (int)m[5];
    // mass == 0 ? -1 : m1 / mass, the IEEE division (correctly rounded; a NaN mass divides to NaN): k_dec_finalize_moves' quotients
    v.rp = v.rm == 0.f ? -1.f : m[1] / v.rm;
    v.ep = v.em == 0.f ? -1.f : m[3] / v.em;
  }
  return v;
}
__device__ __forceinline__ void move_store(const MovesOut& o, size_t i, const MoveVals& v) {
  if (o.raw_pos) o.raw_pos[i] = v.rp;
  if (o.raw_mass) o.raw_mass[i] = v.rm;
  if (o.event_pos) o.event_pos[i] = v.ep;
  if (o.event_mass) o.event_mass[i] = v.em;
  if (o.peak) o.peak[i] = v.pk;
  if (o.peak_weight) o.peak_weight[i] = v.pw;
}

// The moves of a call with fused post-processing (rv_beam_search_calls_moves*): one value per LETTER of the chunk's string.  Runs
// behind k_dec_finalize (decode.hip) of the same part, which left the best hypothesis' tokens [B,L-1] in `tokens`, call_bases and S.
// One 64-thread workgroup per chunk: lane 0 back-traces hypothesis 0 exactly as k_dec_finalize_moves does for w = 0 (same S, So, Lb,
// parents clamped to [0, W-1], record row = the parent of the slot), then lane = step, and the six values of the steps whose token
// has a letter (lut[token] != 0: k_dec_finalize's rule for call_bases, same ballot and popcount) are compacted to the front through
// LDS.  Outputs [B,L-1]; elements at and beyond the chunk's letter count hold the fill values.
__global__ __launch_bounds__(64) void k_dec_finalize_calls_moves(DecState d, const int32_t* tokens, MovesOut o) {
  __shared__ int s_par[64 * RV_MAX_BEAM], s_row[64];
  __shared__ float s_f[5][64];
  __shared__ int s_pk[64];
  __shared__ int s_S;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int steps = min(d.L - 1, 64), W = d.W;
  if (d.chunk_steps) {
    int m = 0;
    for (int i = tid; i < d.B; i += 64) m = max(m, d.chunk_steps[i]);
    for (int x = 32; x > 0; x >>= 1) m = max(m, __shfl_xor(m, x));
    if (tid == 0) s_S = m;
    __syncthreads();
  }
  // (S_dev is read only: k_dec_finalize / k_dec_reduce_steps of the same part ran before this kernel and left it)
  const int S = min(max(d.chunk_steps ? s_S : d.S_dev[0], 0), steps);
  const int So = min(max(d.chunk_steps ? d.chunk_steps[b] : d.S_dev[1 + d.part], 0), S);
  for (int i = tid; i < So * W; i += 64) s_par[i] = d.parent_ids[((size_t)(i / W) * d.B + b) * W + i % W];
  const int len = tid < W ? d.lengths[(size_t)b * W + tid] : 0;
  const int len0 = __shfl(len, 0);
  int maxlen = len;
  for (int x = 32; x > 0; x >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, x));
  const int Lb = min(So, maxlen);
  __syncthreads();
  if (tid == 0) {
    int p = 0;
    for (int t = Lb - 1; t >= 0; --t) {
      p = min(max(p, 0), W - 1);
      const int par = s_par[t * W + p];
      s_row[t] = t < len0 ? min(max(par, 0), W - 1) : -1;
      p = par;
    }
  }
  __syncthreads();
  // one wave, lane = step (max_output_len <= 64)
  const int s = tid;
  const int r = s < Lb ? s_row[s] : -1;
  const MoveVals v = move_vals(r >= 0 ? d.step_moves + (((size_t)s * d.B + b) * W + r) * RV_MOVE_COLS : nullptr);
  const int tokv = s < S ? tokens[(size_t)b * steps + s] : d.pad_token;
  const uint8_t ch = (s < S && tokv >= 0 && tokv < RV_MAX_VOCAB) ? d.lut[tokv] : 0;
  const unsigned long long m = __ballot(ch != 0);
  const int pos = __popcll(m & ((1ull << s) - 1ull)), n = __popcll(m);
  if (ch) { s_f[0][pos] = v.rp; s_f[1][pos] = v.rm; s_f[2][pos] = v.ep; s_f[3][pos] = v.em; s_f[4][pos] = v.pw; s_pk[pos] = v.pk; }
  __syncthreads();
  if (s < steps) {
    MoveVals w{-1.f, 0.f, -1.f, 0.f, 0.f, -1};
    if (s < n) w = MoveVals{s_f[0][s], s_f[1][s], s_f[2][s], s_f[3][s], s_f[4][s], s_pk[s]};
    move_store(o, (size_t)b * steps + s, w);
  }
}

void launch_dec_finalize_calls_moves(const DecState& d, const int32_t* tokens, const MovesOut& o, hipStream_t s) {
  hipLaunchKernelGGL(k_dec_finalize_calls_moves, dim3(d.B), dim3(64), 0, s, d, tokens, o);
}

// The moves of a forced decode (rv_teacher_forced_moves*): one workgroup per chunk, lane = step.  Column t holds the record of step t
// (row 0 of its one beam row) -- the step that was fed targets[b, t] and scored targets[b, t + 1], so the column belongs to that label,
// as nll[b, t] does; the fill values where that label is pad_token.  Every chunk of a forced decode runs all L - 1 steps.
__global__ __launch_bounds__(64) void k_forced_moves(DecState d, MovesOut o) {
  const int b = blockIdx.x, s = threadIdx.x;
  const int steps = min(d.L - 1, 64);
  if (s >= steps) return;
  const bool pad = d.forced[(size_t)b * d.L + s + 1] == d.pad_token;
  move_store(o, (size_t)b * steps + s, move_vals(pad ? nullptr : d.step_moves + ((size_t)s * d.B + b) * d.W * RV_MOVE_COLS));
}

void launch_forced_moves(const DecState& d, const MovesOut& o, hipStream_t s) {
  hipLaunchKernelGGL(k_forced_moves, dim3(d.B), dim3(64), 0, s, d, o);
}
