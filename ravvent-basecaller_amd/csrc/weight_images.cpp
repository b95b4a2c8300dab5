// The weight images, built on the host (weight_images.h).  Every split-f16 image goes through rv_write_fragment and takes its scale
// from rv_column_scale (split_image.h); each builder's loops follow the layout comment common.h keeps beside the kernel that reads it.
#include "weight_images.h"
#include "split_image.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace wimg {

namespace {

constexpr int G = 4 * U;                    // an LSTM cell's gate columns (RV_G); also the width of the decoder images

// bf16 with round-to-nearest-even, and back (finite inputs: the weights)
inline uint16_t bf16_rne(float x) {
  uint32_t u; memcpy(&u, &x, 4);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_value(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float x; memcpy(&x, &u, 4);
  return x;
}

// The bound-based rule (a different one from rv_column_scale: a margin, in double): the power of two that brings bound x 1.0001
// into [2^13, 2^14)
float bound_scale(double bound) {
  int ex = 0;
  if (bound > 0.0 && std::isfinite(bound)) std::frexp(bound * 1.0001, &ex);
  return std::ldexp(1.0f, 14 - ex);
}

}  // namespace

BlobLayout::BlobLayout(const RvConfig& c, int rnn) : enc_depth(c.enc_depth) {
  const size_t u = c.enc_units, d = c.dec_units, V = c.vocab;
  const size_t g = gates(rnn), NB = rnn == RV_RNN_BIGRU ? 2 : 1;
  size_t p = 0;
  auto cell = [&](size_t F, size_t n) {
    CellOffsets w;
    w.W = p; p += F * g * n;
    w.U = p; p += n * g * n;
    w.b = p; p += NB * g * n;
    return w;
  };
  for (int e = 0; e < 2; ++e)
    for (int l = 0; l < c.enc_depth; ++l)
      for (int dr = 0; dr < 2; ++dr) enc[e].push_back(cell(l > 0 ? 2 * u : (e == 0 ? 1 : 5), u));
  for (int k = 0; k < c.dec_depth; ++k) dec.push_back(cell(k == 0 ? V + d : d, d));
  W_mem = p; p += 2 * u * d;
  W_q = p; p += d * d;
  v_att = p; p += d;
  W_att = p; p += (d + 2 * u) * d;
  W_fc = p; p += d * V;
  b_fc = p; p += V;
  total = p;
}

void round_blob_weights(const RvConfig& c, float* blob) {
  const BlobLayout lay(c, RV_RNN_BILSTM);
  const size_t u = c.enc_units, d = c.dec_units;
  for (int e = 0; e < 2; ++e)
    for (int l = 0; l < c.enc_depth; ++l)
      for (int dr = 0; dr < 2; ++dr) {
        const CellOffsets& w = lay.cell(e, l, dr);
        if (l > 0) for (size_t n = 0; n < 4 * u; ++n) rv_round_column(blob + w.W + n, 4 * u, (int)(2 * u));
        for (size_t n = 0; n < 4 * u; ++n) rv_round_column(blob + w.U + n, 4 * u, (int)u);
      }
  for (size_t n = 0; n < d; ++n) rv_round_column(blob + lay.W_mem + n, d, (int)(2 * u));
  for (size_t n = 0; n < d; ++n) rv_round_column(blob + lay.W_att + d * d + n, d, (int)(2 * u));      // A_c
}

ImageCounts image_counts(const RvConfig& c, int rnn) {
  const bool gru = rnn == RV_RNN_BIGRU;
  const size_t L1 = (size_t)2 * (c.enc_depth - 1);
  ImageCounts n;
#define X(T, name, count) n.name = (count);
  RV_WEIGHT_IMAGES(X)
#undef X
  return n;
}

// Recurrent kernel Uk [128][128 g] as MFMA A fragments of U^T for the matrix-pipe recurrences (k_lstm_rec_mx: g = 4, k_gru_rec_mx: g = 3):
// wave w, gate gg, k-step ks, part p, lane (m = lane % 16, kq = lane / 16) holds s_r U[32 ks + 8 kq + j][r], r = 128 gg + 16 w + m (s_r:
// the column's scale; s_r U is exact), then the 128 g factors 2^-14 / s_r
void pack_recurrent(const float* Uk, int g, uint16_t* img) {
  const int N = g * U;
  std::vector<float> cs(N);
  for (int r = 0; r < N; ++r) {
    cs[r] = rv_column_scale(Uk + r, N, U);
    rv_put_factor(&img[(size_t)2 * U * N + 2 * r], cs[r]);
  }
  for (int w = 0; w < 8; ++w)
    for (int gg = 0; gg < g; ++gg)
      for (int ks = 0; ks < 4; ++ks)
        rv_write_fragment(img + ((((size_t)w * g + gg) * 4 + ks) * 2) * 512, 512, [&](int k, int m) {
          const int r = gg * U + 16 * w + m;
          return Uk[(size_t)(32 * ks + k) * N + r] * cs[r];
        });
}

// Input kernel W [256][512] of an encoder layer >= 1 for the fused recurrence: tile nt, part p, k-step ks, lane (n, kq) holds
// s_c W[32 ks + 8 kq + j][c], c = 16 nt + n; the low part times 2048 (rv_write_fragment); then the 512 factors 2^-14 / s_c
void pack_wh(const float* W, uint16_t* img) {
  std::vector<float> cs(G);
  for (int n = 0; n < G; ++n) {
    cs[n] = rv_column_scale(W + n, G, E);
    rv_put_factor(&img[(size_t)2 * E * G + 2 * n], cs[n]);
  }
  for (int nt = 0; nt < 32; ++nt)
    for (int ks = 0; ks < 8; ++ks)
      rv_write_fragment(img + (((size_t)nt * 2) * 8 + ks) * 512, (size_t)8 * 512, [&](int k, int n) {
        const int c = 16 * nt + n;
        return W[(size_t)(32 * ks + k) * G + c] * cs[c];
      }, 2048.f);
}

// Bahdanau's query layer W_q [128][128] for the matrix pipe (DecState::Wq16): one scale for the tensor; wave wv, k-step ks, lane (n, kq)
// holds T W_q[32 ks + 8 kq + j][16 wv + n]
float pack_wq16(const float* Wq, uint16_t* img) {
  float mq = 0.f;
  for (size_t i = 0; i < (size_t)U * U; ++i) mq = std::max(mq, std::fabs(Wq[i]));
  const float T = rv_column_scale(mq);
  for (int wv = 0; wv < 8; ++wv)
    for (int ks = 0; ks < 4; ++ks)
      rv_write_fragment(img + (((size_t)wv * 4 + ks) * 2) * 512, 512, [&](int k, int n) { return Wq[(size_t)(32 * ks + k) * U + 16 * wv + n] * T; });
  return T;
}

namespace {

// A decoder kernel of KR rows for the matrix-pipe cell product, per wave in B-fragment order: wave wv, pair pr = (k-step, gate), part p,
// lane (n, kq) holds el(pr, k within the k-step, column 128 gate + 16 wv + n) -- scaled by the caller (Wc16: 4 gates of every k-step
// of [ctx' | h (| h_0)]; W1c16: the pairs of W_1, then those of U_1)
template <class El>
void pack_gate_pairs(int pairs, uint16_t* img, El el) {
  for (int wv = 0; wv < 8; ++wv)
    for (int pr = 0; pr < pairs; ++pr)
      rv_write_fragment(img + (((size_t)wv * pairs + pr) * 2) * 512, 512, [&](int k, int n) { return el(pr, k, U * (pr & 3) + 16 * wv + n); });
}

// The first parts alone of `frags` fragments kept as [2 parts][512] each (weight_parts 1: the second parts are zero)
void first_parts(const uint16_t* img, size_t frags, std::vector<uint16_t>& p1) {
  for (size_t fr = 0; fr < frags; ++fr) memcpy(&p1[fr * 512], &img[fr * 1024], 512 * sizeof(uint16_t));
}

// Recurrent kernel [128][512] -> [32 i][512 threads][4 slots] for the packed-FMA recurrence: thread = 4 j + kq holds k = 32 kq + i,
// slot r = gate (kq + r) & 3
void pack_up(const float* Uk, float* up) {
  for (int i = 0; i < 32; ++i)
    for (int tid = 0; tid < 512; ++tid) {
      const int j = tid >> 2, kq = tid & 3;
      for (int r = 0; r < 4; ++r) up[((size_t)i * 512 + tid) * 4 + r] = Uk[(size_t)(32 * kq + i) * G + ((kq + r) & 3) * U + j];
    }
}

// Input kernel W [256][512] of an encoder layer >= 1 -> [32 column tiles][16 k-groups][64 lanes][4]: lane (q = lane / 16, col = lane % 16)
// of tile nt finds W[16 g + 4 i + q][16 nt + col] for its 4 MFMAs i of k-group g in one float4 (lstm_rec.hip)
void pack_wp(const float* W, float* t) {
  for (int nt = 0; nt < 32; ++nt)
    for (int g = 0; g < 16; ++g)
      for (int ln = 0; ln < 64; ++ln)
        for (int i = 0; i < 4; ++i) t[(((size_t)nt * 16 + g) * 64 + ln) * 4 + i] = W[(size_t)(16 * g + 4 * i + (ln >> 4)) * G + 16 * nt + (ln & 15)];
}

// ... and as three bf16 parts: lane (kq = lane / 16, col = lane % 16) of tile nt, part, k-step ks holds W[32 ks + 8 kq + j][16 nt + col], j = 0..7
void pack_wsb(const float* W, uint16_t* sb) {
  for (int nt = 0; nt < 32; ++nt)
    for (int ks = 0; ks < 8; ++ks)
      for (int ln = 0; ln < 64; ++ln)
        for (int j = 0; j < 8; ++j) {
          float r = W[(size_t)(32 * ks + 8 * (ln >> 4) + j) * G + 16 * nt + (ln & 15)];
          for (int part = 0; part < 3; ++part) {
            const uint16_t b = bf16_rne(r);
            sb[((((size_t)nt * 3 + part) * 8 + ks) * 64 + ln) * 8 + j] = b;
            r -= bf16_value(b);                    // exact
          }
        }
}

// The encoders' images of either family (g gates): the recurrent fragments of every (encoder, layer, direction) into `ua`; for layers
// >= 1 both directions' input kernels [fwd | bwd] as the g column blocks of the split GEMM into `wx16` (rv_pack_split_image takes any
// block count) with their input biases -- the first bias row -- into `bias`
void build_encoder_images(const RvConfig& c, const BlobLayout& lay, const float* blob, int g, std::vector<uint16_t>& ua,
                          std::vector<uint16_t>& wx16, std::vector<float>& bias) {
  const int N = g * U;
  for (int e = 0; e < 2; ++e)
    for (int l = 0; l < c.enc_depth; ++l)
      for (int dr = 0; dr < 2; ++dr)
        pack_recurrent(blob + lay.cell(e, l, dr).U, g, ua.data() + ((size_t)(e * c.enc_depth + l) * 2 + dr) * ua_slot(g));
  for (int e = 0; e < 2; ++e)
    for (int l = 1; l < c.enc_depth; ++l) {
      const size_t slot = (size_t)(e * (c.enc_depth - 1) + (l - 1));
      const CellOffsets* dir = &lay.cell(e, l, 0);           // [fwd, bwd]
      for (int dr = 0; dr < 2; ++dr) memcpy(&bias[(slot * 2 + dr) * N], blob + dir[dr].b, N * sizeof(float));
      rv_pack_split_image(blob, N, g, [&](int cc) { return dir[cc / N].W + (size_t)(cc % N); }, wx16.data() + slot * wx16_slot(g));
    }
}

// The LSTM encoders' images for the packed-FMA and fused-projection kernels
void build_lstm_encoder_extras(const RvConfig& c, const BlobLayout& lay, const float* blob, HostImages& im) {
  for (int e = 0; e < 2; ++e)
    for (int l = 0; l < c.enc_depth; ++l)
      for (int dr = 0; dr < 2; ++dr) {
        const float* cell = blob + lay.cell(e, l, dr).U;
        pack_up(cell, im.Up.data() + ((size_t)(e * c.enc_depth + l) * 2 + dr) * U * G);
        if (l == 0) continue;
        const float* W = blob + lay.cell(e, l, dr).W;
        const size_t slot = (size_t)(e * (c.enc_depth - 1) + (l - 1)) * 2 + dr;
        pack_wp(W, im.Wp.data() + slot * E * G);
        pack_wsb(W, im.Wsb.data() + slot * 3 * E * G);
        pack_wh(W, im.Wh.data() + slot * WH_SLOT);
      }
}

// [W_mem | A_c] [256][256]: column block 0 = W_mem (keys), column block 1 = rows 128..383 of the attention layer (its context part), so
// that enc_out . Wmp = [keys | image of the values under the attention layer]; its split image; and the scales of both products
void build_memory_images(const BlobLayout& lay, const float* blob, std::vector<float>& wmp, std::vector<uint16_t>& wmp16,
                         std::vector<uint16_t>& wkp16, ImageScales& sc) {
  const float *Wmem = blob + lay.W_mem, *Ac = blob + lay.W_att + (size_t)U * U;
  for (int k = 0; k < E; ++k)
    for (int n = 0; n < U; ++n) {
      wmp[(size_t)k * E + n] = Wmem[(size_t)k * U + n];
      wmp[(size_t)k * E + U + n] = Ac[(size_t)k * U + n];
    }
  // |enc_out| <= 1, so |key_tu| <= sum_k |W_mem[k][u]| and |U'_tn| <= sum_k |A_c[k][n]|: the largest column sums bound both
  double bk = 0.0, bu = 0.0;
  for (int n = 0; n < E; ++n) {
    double cs = 0.0;
    for (int k = 0; k < E; ++k) cs += std::fabs((double)wmp[(size_t)k * E + n]);
    if (n < U) bk = std::max(bk, cs); else bu = std::max(bu, cs);
  }
  sc.kscale = bound_scale(bk); sc.uscale = bound_scale(bu);
  rv_pack_split_image(wmp.data(), E, 1, [](int cc) { return (size_t)cc; }, wmp16.data());
  // the same f16 parts of the W_mem half, for the decode's own projection (DecState::Wkp16): lane (i, kq) of key tile 2 ks + y takes
  // what lane (c % 16, kq) of column tile c / 16 holds, c = 32 ks + 8 (i / 4) + 4 y + i % 4 -- a permutation, no second rounding
  for (int st = 0; st < 8; ++st)
    for (int t8 = 0; t8 < 8; ++t8)
      for (int part = 0; part < 2; ++part)
        for (int ln = 0; ln < 64; ++ln) {
          const int i = ln & 15, q = ln >> 4, cc = 32 * (t8 >> 1) + 8 * (i >> 2) + 4 * (t8 & 1) + (i & 3);
          memcpy(&wkp16[((((size_t)st * 8 + t8) * 2 + part) * 64 + ln) * 8],
                 &wmp16[((((size_t)st * 16 + cc / 16) * 2 + part) * 64 + 16 * q + cc % 16) * 8], 8 * sizeof(uint16_t));
        }
}

// A_h W_fc [128][V] (products in double): the h half of the folded output layer
void fold_output_h(const float* Ah, const float* Wfc, int V, float* nh) {
  for (int i = 0; i < U; ++i)
    for (int v = 0; v < V; ++v) {
      double acc = 0.0;
      for (int j = 0; j < U; ++j) acc += (double)Ah[(size_t)i * U + j] * (double)Wfc[(size_t)j * V + v];
      nh[(size_t)i * V + v] = (float)acc;
    }
}

// The factor the f16 image of row k of [ctx' | h (| h_0)] carries: ctx' the scale of U', every h 2^14
inline float input_factor(int k, float uscale) { return k < U ? uscale : 16384.f; }

// The folded output layer [W_fc ; A_h W_fc] on the [ctx' | h] image (DecState::Wl16): rows divided by their input's factor (exact:
// powers of two), columns >= V zero, one power-of-two scale for the tensor, k-step ks, part p
struct OutputLayer {
  const float *fcw, *nh;                    // W_fc [128][V], A_h W_fc [128][V]
  int V;
  float uscale;
  float at(int k, int v) const { return v >= V ? 0.f : (k < U ? fcw[(size_t)k * V + v] : nh[(size_t)(k - U) * V + v]) / input_factor(k, uscale); }
  float scale() const {
    float ml = 0.f;
    for (int k = 0; k < E; ++k)
      for (int v = 0; v < V; ++v) ml = std::max(ml, std::fabs(at(k, v)));
    return rv_column_scale(ml);
  }
  void pack(float Tl, uint16_t* img) const {
    for (int ks = 0; ks < 8; ++ks) rv_write_fragment(img + ((size_t)ks * 2) * 512, 512, [&](int k, int n) { return at(32 * ks + k, n) * Tl; });
  }
};

// One or two decoder cells: attention = h . A_h + ctx' (h = the top cell's output); its h part is folded into what consumes the attention
// vector (products in double):
//   one cell : next cell input  [ctx' | h] . [W_a ; U + A_h W_a],                 logits  ctx' . W_fc + h . (A_h W_fc) + b
//   two cells: cell 0's input   [ctx' | h_1 | h_0] . [W_a ; A_h W_a ; U_0],       logits  ctx' . W_fc + h_1 . (A_h W_fc) + b
void build_folded_decoder(const RvConfig& c, const BlobLayout& lay, const ImageCounts& cnt, bool one_part, const float* blob, HostImages& im) {
  const int V = c.vocab;
  const bool two = c.dec_depth == 2;
  const int KR = two ? 3 * U : E;                           // rows of cell 0's folded kernel
  const float *Wa = blob + lay.dec[0].W + (size_t)V * G, *U0 = blob + lay.dec[0].U, *Ah = blob + lay.W_att, *Wfc = blob + lay.W_fc;
  ImageScales& sc = im.scales;
  std::vector<float> w2((size_t)KR * G), nh(cnt.Nh, 0.f);
  for (int i = 0; i < U; ++i)
    for (int n = 0; n < G; ++n) {
      w2[(size_t)i * G + n] = Wa[(size_t)i * G + n];
      double acc = two ? 0.0 : (double)U0[(size_t)i * G + n];
      for (int j = 0; j < U; ++j) acc += (double)Ah[(size_t)i * U + j] * (double)Wa[(size_t)j * G + n];
      w2[(size_t)(U + i) * G + n] = (float)acc;
      if (two) w2[(size_t)(2 * U + i) * G + n] = U0[(size_t)i * G + n];
    }
  fold_output_h(Ah, Wfc, V, nh.data());
  // the scales of the matrix-pipe images of both folded tensors (Wc16, Wl16): rows divided by the factor their input's f16 image
  // carries (exact: powers of two), then one power-of-two scale for the tensor
  auto xs = [&](int k) { return input_factor(k, sc.uscale); };
  float mx = 0.f;
  for (int k = 0; k < KR; ++k)
    for (int n = 0; n < G; ++n) mx = std::max(mx, std::fabs(w2[(size_t)k * G + n] / xs(k)));
  const float T = rv_column_scale(mx);
  std::vector<float> fcw(Wfc, Wfc + (size_t)U * V);      // W_fc, the output layer's upper half
  const OutputLayer out{fcw.data(), nh.data(), V, sc.uscale};
  const float Tl = out.scale();
  if (one_part) {   // weight_parts 1: both folded tensors rounded to the first f16 part of those images, under the scales just taken
                    // (kept for the packing below), so that their fp32 images (Wcat2, Nh) carry the same numbers
    for (int k = 0; k < KR; ++k)
      for (int n = 0; n < G; ++n) w2[(size_t)k * G + n] = rv_round_to_first_part(w2[(size_t)k * G + n] / xs(k), T) * xs(k);
    for (int k = 0; k < E; ++k)
      for (int v = 0; v < V; ++v) (k < U ? fcw[(size_t)k * V + v] : nh[(size_t)(k - U) * V + v]) = rv_round_to_first_part(out.at(k, v), Tl) * xs(k);
  }
  if (!two) im.Wcat2 = w2;                                  // (the packed-FMA form of one cell)
  im.Nh = nh;
  // the same kernel for the matrix-pipe cell product (DecState::Wc16): pair pr = 4 ks + gate over the KR / 32 k-steps (one cell: the 128
  // rows a second cell would add stay zero)
  sc.cdescale = 1.0f / T;
  const int NP = KR / 8;
  im.Wc16.assign(cnt.Wc16, 0);
  pack_gate_pairs(NP, im.Wc16.data(), [&](int pr, int k, int n) { const int row = 32 * (pr >> 2) + k; return (w2[(size_t)row * G + n] / xs(row)) * T; });
  if (one_part && !two) { im.Wc16p1.assign(cnt.Wc16p1, 0); first_parts(im.Wc16.data(), (size_t)8 * NP, im.Wc16p1); }      // (k_dec_persist_1p)
  if (two) {   // cell 1's kernels on h_0 (W_1: pairs 0..15) and on h_1 (U_1: pairs 16..31): DecState::W1c16, rows divided by the 2^14 their inputs' images carry
    const float *W1 = blob + lay.dec[1].W, *U1 = blob + lay.dec[1].U;
    float m1 = 0.f;
    for (size_t i = 0; i < (size_t)U * G; ++i) m1 = std::max(m1, std::max(std::fabs(W1[i]), std::fabs(U1[i])) / 16384.f);
    const float T1 = rv_column_scale(m1);
    sc.c1descale = 1.0f / T1;
    im.W1c16.assign(cnt.W1c16, 0);
    pack_gate_pairs(32, im.W1c16.data(), [&](int pr, int k, int n) { return ((pr < 16 ? W1 : U1)[(size_t)(32 * ((pr & 15) >> 2) + k) * G + n] / 16384.f) * T1; });
  }
  // the output layer on the same [ctx' | h] image: logits = ctx' . W_fc + h . (A_h W_fc) + b_fc, k-step ks, part p
  sc.ldescale = 1.0f / Tl;
  im.Wl16.assign(cnt.Wl16, 0);
  out.pack(Tl, im.Wl16.data());
  if (one_part) { im.Wl16p1.assign(cnt.Wl16p1, 0); first_parts(im.Wl16.data(), 8, im.Wl16p1); }
  if (!two) {
    im.Wq16.assign(cnt.Wq16, 0);
    sc.qdescale = std::ldexp(1.0f, -14) / pack_wq16(blob + lay.W_q, im.Wq16.data());
  }
}

}  // namespace

// One GRU decoder cell (Keras, reset_after) for the persistent decode.  As build_folded_decoder, attention = h . A_h + ctx' is folded
// into what consumes it, tile by tile: z and r take [ctx' | h] . [W_a ; U + A_h W_a]; the candidate's input half takes [ctx' | h] .
// [W_a,h ; A_h W_a,h] and its recurrent half [0 ; U_h] alone, so that the reset gate multiplies h . U_h + b[1]_h and nothing else
// (products in double).  The cell-independent images are build_memory_images' and the LSTM forms' output layer on the GRU blob.
GruPersistImages build_gru_persist_images(const RvConfig& c, const float* blob) {
  const BlobLayout lay(c, RV_RNN_BIGRU);
  const int V = c.vocab, N = 3 * U;
  GruPersistImages g;
#define X(T, name, count) g.name.assign((count), 0);
  RV_GRU_PERSIST_IMAGES(X)
#undef X
  ImageScales& sc = g.scales;
  build_memory_images(lay, blob, g.gWmp, g.gWmp16, g.gWkp16, sc);
  const float *W0 = blob + lay.dec[0].W, *Wa = W0 + (size_t)V * N, *Uk = blob + lay.dec[0].U, *b = blob + lay.dec[0].b;
  const float *Ah = blob + lay.W_att, *Wfc = blob + lay.W_fc;
  std::vector<float> w2((size_t)E * G, 0.f), nh((size_t)U * V, 0.f);
  for (int i = 0; i < U; ++i)
    for (int tile = 0; tile < 4; ++tile)
      for (int n = 0; n < U; ++n) {
        const int col = tile * U + n, src = std::min(tile, 2) * U + n;      // (the blob's gate columns: z, r, h)
        w2[(size_t)i * G + col] = tile < 3 ? Wa[(size_t)i * N + src] : 0.f;
        double acc = tile != 2 ? (double)Uk[(size_t)i * N + src] : 0.0;
        if (tile < 3)
          for (int j = 0; j < U; ++j) acc += (double)Ah[(size_t)i * U + j] * (double)Wa[(size_t)j * N + src];
        w2[(size_t)(U + i) * G + col] = (float)acc;
      }
  fold_output_h(Ah, Wfc, V, nh.data());
  // scales and fragments as build_folded_decoder takes them: rows divided by the factor their input's f16 image carries, one
  // power-of-two scale per tensor
  auto xs = [&](int k) { return input_factor(k, sc.uscale); };
  float mx = 0.f;
  for (int k = 0; k < E; ++k)
    for (int n = 0; n < G; ++n) mx = std::max(mx, std::fabs(w2[(size_t)k * G + n] / xs(k)));
  const float T = rv_column_scale(mx);
  sc.cdescale = 1.0f / T;
  pack_gate_pairs(E / 8, g.gWc16.data(), [&](int pr, int k, int n) { const int row = 32 * (pr >> 2) + k; return (w2[(size_t)row * G + n] / xs(row)) * T; });
  const OutputLayer out{Wfc, nh.data(), V, sc.uscale};
  const float Tl = out.scale();
  sc.ldescale = 1.0f / Tl;
  out.pack(Tl, g.gWl16.data());
  sc.qdescale = std::ldexp(1.0f, -14) / pack_wq16(blob + lay.W_q, g.gWq16.data());
  // the token table and the bias in the same four tiles: b[1]_h rides in the fourth tile's row, inside the reset product
  for (int v = 0; v < V; ++v)
    for (int n = 0; n < N; ++n) g.gWtok[(size_t)v * G + n] = W0[(size_t)v * N + n];
  for (int n = 0; n < U; ++n) {
    g.gbdec[n] = b[n] + b[N + n];
    g.gbdec[U + n] = b[U + n] + b[N + U + n];
    g.gbdec[2 * U + n] = b[2 * U + n];
    g.gbdec[3 * U + n] = b[N + 2 * U + n];
  }
  return g;
}

HostImages build_weight_images(const RvConfig& c, int rnn, int weight_parts, const float* blob) {
  const BlobLayout lay(c, rnn);
  const ImageCounts cnt = image_counts(c, rnn);
  const bool gru = rnn == RV_RNN_BIGRU;
  HostImages im;
  // what every load of the family builds (an image the configuration has none of has count 0 and stays empty); the folded decoder
  // tensors take their room in build_folded_decoder
#define TAKE(name) im.name.assign(cnt.name, 0)
  TAKE(WmemT);
  if (gru) { TAKE(gUa); TAKE(gWx16); TAKE(gbx); TAKE(gWcatT); }
  else { TAKE(Up); TAKE(Wp); TAKE(Wsb); TAKE(Wh); TAKE(Ua); TAKE(Wx16); TAKE(bx2); TAKE(WcatT); TAKE(Wmp); TAKE(Wmp16); TAKE(Wkp16); }
#undef TAKE
  for (int i = 0; i < E; ++i)                             // W_mem [256][128] -> [128][256]
    for (int j = 0; j < U; ++j) im.WmemT[(size_t)j * E + i] = blob[lay.W_mem + (size_t)i * U + j];
  build_encoder_images(c, lay, blob, gates(rnn), gru ? im.gUa : im.Ua, gru ? im.gWx16 : im.Wx16, gru ? im.gbx : im.bx2);
  if (gru) {
    // decoder cells for k_dec_cell_gru: ([W_in ; U])^T as four column tiles of 128 -- z, r, [W_h ; 0], [0 ; U_h] -- [512][256], so that
    // the candidate gate's input and recurrent parts leave the one product apart (W_in: the rows of W behind cell 0's one-hot rows)
    const int N = 3 * U;
    for (int k = 0; k < c.dec_depth; ++k) {
      float* t = im.gWcatT.data() + (size_t)k * G * E;
      const float *Win = blob + lay.dec[k].W + (k == 0 ? (size_t)c.vocab * N : 0), *Uk = blob + lay.dec[k].U;
      for (int tile = 0; tile < 4; ++tile)
        for (int n = 0; n < U; ++n)
          for (int kk = 0; kk < E; ++kk) {
            const int col = (tile < 2 ? tile : 2) * U + n;
            const bool in_half = kk < U;
            float v = in_half ? Win[(size_t)kk * N + col] : Uk[(size_t)(kk - U) * N + col];
            if ((tile == 2 && !in_half) || (tile == 3 && in_half)) v = 0.f;
            t[((size_t)tile * U + n) * E + kk] = v;
          }
    }
    return im;
  }
  // the decoder cell kernel: the input-kernel rows that multiply a dense input (rows V.. of W_0; all of W_k for k >= 1) followed by
  // U_k form a contiguous [256][512] matrix in the blob; the kernel wants it column-major ([512][256])
  for (int l = 0; l < c.dec_depth; ++l) {
    const float* W = blob + lay.dec[l].W + (l == 0 ? (size_t)c.vocab * G : 0);
    float* t = im.WcatT.data() + (size_t)l * G * E;
    for (int k = 0; k < E; ++k)
      for (int n = 0; n < G; ++n) t[(size_t)n * E + k] = W[(size_t)k * G + n];
  }
  build_lstm_encoder_extras(c, lay, blob, im);
  build_memory_images(lay, blob, im.Wmp, im.Wmp16, im.Wkp16, im.scales);
  if (c.dec_depth <= 2) build_folded_decoder(c, lay, cnt, weight_parts == 1, blob, im);
  return im;
}

}  // namespace wimg
