// The whole beam of a call: every one of the W hypotheses back-traced, with the scores that belong to it.
//
// k_dec_finalize (decode.hip) hands out predicted_ids[:, :, 0] and scores[:, :, 0], what Basecaller.beam_search_prediction
// returns (/root/reference/basecaller.py:313-315).  TFA's BeamSearchDecoder returns the FinalBeamSearchDecoderOutput [B,S,W] and the
// final state's log_probs and lengths as well; k_dec_finalize_beams is that finalize for a call that asks for them
// (rv_beam_search_all*).  It reads the records the decode leaves -- step_ids / parent_ids / step_scores of every slot of every step,
// lengths per beam, chunk_steps or S_dev -- and takes k_dec_finalize's place for such a call: nothing of the decode changes.
#include "common.h"

// One 64-thread workgroup per chunk, as in k_dec_finalize.  The chunk's [So,W] records are staged in LDS, lane w < W back-traces
// hypothesis w (TFA gather_tree), then the wave writes the chunk's [L-1,W] rows, beam innermost.
__global__ __launch_bounds__(64) void k_dec_finalize_beams(DecState d, BeamsOut o) {
  __shared__ int s_ids[64 * RV_MAX_BEAM], s_par[64 * RV_MAX_BEAM], s_tok[64 * RV_MAX_BEAM], s_slot[64 * RV_MAX_BEAM];
  __shared__ float s_sc[64 * RV_MAX_BEAM];
  __shared__ int s_S;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int steps = d.L - 1, W = d.W;
  // S: steps the reference loop runs for the whole slab; So: steps this chunk (persistent decode) / this sub-slab (per-step kernels)
  // ran -- both exactly as k_dec_finalize takes them
  if (d.chunk_steps) {
    int m = 0;
    for (int i = tid; i < d.B; i += 64) m = max(m, d.chunk_steps[i]);
    for (int x = 32; x > 0; x >>= 1) m = max(m, __shfl_xor(m, x));
    if (tid == 0) { s_S = m; if (b == 0) { d.S_host[0] = m; d.S_dev[0] = m; d.S_dev[1] = m; } }
    __syncthreads();
  }
  // (the clamps hold for every record the decode writes, L <= 64; they keep the LDS indices below in range whatever is read)
  const int S = min(max(d.chunk_steps ? s_S : d.S_dev[0], 0), steps);
  const int So = min(max(d.chunk_steps ? d.chunk_steps[b] : d.S_dev[1 + d.part], 0), S);
  for (int i = tid; i < So * W; i += 64) {
    const int s = i / W, w = i % W;
    const size_t g = ((size_t)s * d.B + b) * W + w;
    s_ids[i] = d.step_ids[g];
    s_par[i] = d.parent_ids[g];
    s_sc[i] = d.step_scores[g];
  }
  // TFA's max_sequence_lengths of the chunk
  int len = tid < W ? d.lengths[(size_t)b * W + tid] : 0;
  int maxlen = len;
  for (int x = 32; x > 0; x >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, x));
  const int Lb = min(So, maxlen);      // = min(S, maxlen): a beam's length never exceeds the steps its chunk ran
  __syncthreads();
  if (tid < W) {
    const int w = tid;
    int p = w;
    for (int t = Lb - 1; t >= 0; --t) {
      p = min(max(p, 0), W - 1);
      s_slot[t * W + w] = p;
      s_tok[t * W + w] = s_ids[t * W + p];
      p = s_par[t * W + p];
    }
    bool done = false;
    for (int t = 0; t < Lb; ++t) {
      if (done) s_tok[t * W + w] = d.end_token;
      else if (s_tok[t * W + w] == d.end_token) done = true;
    }
  }
  __syncthreads();
  // the chunk's rows, [steps][W] flat: consecutive lanes write consecutive addresses
  const size_t row = (size_t)b * steps * W;
  for (int i = tid; i < steps * W; i += 64) {
    const int s = i / W, w = i % W;
    int tokv = d.pad_token;
    float scv = 0.f, pv = 0.f;
    if (s < S) {
      tokv = s < Lb ? s_tok[i] : d.end_token;
      if (So > 0) scv = s_sc[min(s, So - 1) * W + w];
      if (Lb > 0) { const int t = min(s, Lb - 1); pv = s_sc[t * W + s_slot[t * W + w]]; }
    }
    o.tokens[row + i] = tokv;
    o.scores[row + i] = scv;
    if (o.path_scores) o.path_scores[row + i] = pv;
  }
  if (tid < W) {
    if (o.log_probs) o.log_probs[(size_t)b * W + tid] = So > 0 ? s_sc[(So - 1) * W + tid] : (tid == 0 ? 0.f : -INFINITY);
    if (o.lengths) o.lengths[(size_t)b * W + tid] = len;
  }
}

void launch_dec_finalize_beams(const DecState& d, const BeamsOut& o, hipStream_t s) {
  hipLaunchKernelGGL(k_dec_finalize_beams, dim3(d.B), dim3(64), 0, s, d, o);
}
