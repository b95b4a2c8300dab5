// The moves of a call: where in the attention memory each token of each of the W hypotheses comes from.
//
// Every decode form leaves one record per (step, chunk, beam row) in DecState::step_moves (common.h): the raw and the event segment's
// attention mass and first moment, and the peak.  The row is the one the attention of that step ran on -- before the step's top-k
// reordered the rows -- so the token a hypothesis holds in slot p_t at column t was produced from row parent_ids[t][b][p_t] of step t
// (TFA's decoder step computes the alignments before its beam step reorders the rows: SURVEY.md A.5).  k_dec_finalize_moves runs the
// back-trace of k_dec_finalize_beams (beams.hip) -- the same S, So, Lb and slot chain -- and hands out that row's record per column.
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
