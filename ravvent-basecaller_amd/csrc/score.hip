// Scoring of label rows against logits: what every number of the reference's training and validation logs is made of.
//
// Basecaller.loss_function (/root/reference/basecaller.py:212-220) is the sparse cross-entropy of the logits at the label, zero where the
// label is the padding token, summed and divided by the number of labels that are not; utils.masked_accuracy (/root/reference/utils.py:15-24)
// is the share of labels outside an omit set that the argmax equals.  k_score_tokens leaves the per-position terms and the per-chunk sums
// of both; the caller forms the two quotients (sum(nll_sum) / sum(n_labels), sum(n_match) / sum(n_counted)), so there is no float atomic
// and a chunk's numbers never depend on the slab it is scored in.
#include "common.h"
#include <math.h>

// One 64-thread workgroup per chunk, lane = position (S <= 64).  The row's nll terms meet in LDS and lane 0 adds them in column order.
__global__ __launch_bounds__(64) void k_score_tokens(ScoreArgs a) {
  __shared__ float s_nll[64];
  const int b = blockIdx.x, s = threadIdx.x, V = a.V;
  const bool live = s < a.S;
  float nll = 0.f;
  int counted = 0, match = 0, labelled = 0;
  if (live) {
    const float* lg = a.logits + ((size_t)b * a.S + s) * V;
    const int label = a.labels[(size_t)b * a.label_stride + s];
    float l[RV_MAX_VOCAB];
#pragma unroll
    for (int v = 0; v < RV_MAX_VOCAB; ++v) l[v] = v < V ? lg[v] : -INFINITY;
    float m = l[0], at = 0.f;
    int arg = 0;
#pragma unroll
    for (int v = 1; v < RV_MAX_VOCAB; ++v)
      if (l[v] > m) { m = l[v]; arg = v; }      // strictly greater: the first maximum wins a tie
    float sum = 0.f;
#pragma unroll
    for (int v = 0; v < RV_MAX_VOCAB; ++v) {
      sum += v < V ? expf(l[v] - m) : 0.f;        // max-subtracted: every term <= 1, the largest exactly 1
      at = v == label ? l[v] : at;
    }
    labelled = label != a.pad_token;
    const bool in_vocab = (unsigned)label < (unsigned)V;      // an id never selects a logit unchecked
    if (labelled) nll = in_vocab ? (m - at) + logf(sum) : NAN;
    counted = !(label >= 0 && label < 32 && ((a.omit_mask >> label) & 1u));
    match = counted && label == arg;
    if (a.nll) a.nll[(size_t)b * a.S + s] = nll;
    if (a.pred) a.pred[(size_t)b * a.S + s] = arg;
  }
  s_nll[s] = nll;
  const int n_counted = __popcll(__ballot(counted != 0)), n_match = __popcll(__ballot(match != 0)), n_labels = __popcll(__ballot(labelled != 0));
  __syncthreads();
  if (s == 0) {
    float t = 0.f;
    for (int i = 0; i < a.S; ++i) t += s_nll[i];
    if (a.nll_sum) a.nll_sum[b] = t;
    if (a.n_labels) a.n_labels[b] = n_labels;
    if (a.n_match) a.n_match[b] = n_match;
    if (a.n_counted) a.n_counted[b] = n_counted;
  }
}

void launch_score_tokens(const ScoreArgs& a, hipStream_t s) {
  if (a.B <= 0 || a.S <= 0) return;
  hipLaunchKernelGGL(k_score_tokens, dim3(a.B), dim3(64), 0, s, a);
}
