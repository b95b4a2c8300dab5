// The images of the weights that the kernels read, built on the host from the flat blob (weights.py: blob order).  Pure host code: no
// HIP, no handle.  rv_create_rnn allocates every image from image_counts(), rv_load_weights uploads what build_weight_images() returns;
// the layouts are the ones common.h documents beside the kernels that read them.
#pragma once
#include "../../include/ravvent_hip.h"

#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace wimg {

constexpr int U = 128, E = 256;             // units per direction / decoder units; encoder output width (common.h: RV_U, RV_E)
constexpr int MAX_VOCAB = 8;                // (RV_MAX_VOCAB)
constexpr size_t WH_SLOT = (size_t)2 * E * 4 * U + 2 * 4 * U;      // uint16 per (encoder, layer, direction) of Wh

inline int gates(int rnn) { return rnn == RV_RNN_BIGRU ? 3 : 4; }
// uint16 per slot of the recurrent image (RV_UA_SLOT, RV_GRU_UA_SLOT) and of the input-kernel image (RV_WX16_SLOT, RV_GRU_WX16_SLOT)
inline size_t ua_slot(int g) { return (size_t)2 * U * g * U + 2 * g * U; }
inline size_t wx16_slot(int g) { return (size_t)2 * E * 2 * g * U + 2 * 2 * g * U; }

// The one walk of the blob: float offsets of every tensor.  Per cell W[F, G u]  U[u, G u]  b[NB, G u] -- LSTM: G = 4 gates, one bias
// row; GRU: G = 3, input and recurrent bias rows
struct CellOffsets { size_t W, U, b; };
struct BlobLayout {
  int enc_depth = 0;
  std::vector<CellOffsets> enc[2];          // [enc][2 layer + dir]
  std::vector<CellOffsets> dec;             // stacked decoder cells
  size_t W_mem = 0, W_q = 0, v_att = 0, W_att = 0, W_fc = 0, b_fc = 0, total = 0;
  BlobLayout(const RvConfig& c, int rnn);
  const CellOffsets& cell(int e, int l, int dr) const { return enc[e][(size_t)2 * l + dr]; }
};

// Option weight_parts 1, the tensors that are a slice of an LSTM blob: each column rounded to what the first f16 part of its split image
// holds (rv_round_column) -- U of every encoder layer and direction over its 128 rows, W of encoder layers >= 1 over 256 rows, W_mem
// and A_c (rows u .. 3u - 1 of the attention layer) over 256 rows.  Everything else stays as it is; the folded tensors (cell kernel,
// output layer) are rounded after their fold by build_weight_images.
void round_blob_weights(const RvConfig& c, float* blob);

// Every image: element type, name, elements a handle of (c, gru) holds (0: it has no such image).  g = gates(rnn), L1 = encoder layers >= 1.
//   X(type, name, count)
#define RV_WEIGHT_IMAGES(X)                                                                                                             \
  X(float, WmemT, (size_t)U * E)                                  /* W_mem^T [128][256] */                                              \
  X(float, Up, gru ? 0 : (size_t)2 * c.enc_depth * 2 * U * 4 * U) /* recurrent kernels in the packed-FMA kernels' register order, [enc][layer][dir][65536] */ \
  X(float, Wp, gru ? 0 : L1 * 2 * E * 4 * U)                      /* input kernels of encoder layers >= 1 as MFMA B fragments, [enc][layer-1][dir][131072] */ \
  X(uint16_t, Wsb, gru ? 0 : L1 * 2 * 3 * E * 4 * U)              /* ... cut into three bf16 parts, [enc][layer-1][dir][32 tiles][3 parts][8 k-steps][64 lanes][8] */ \
  X(uint16_t, Wh, gru ? 0 : L1 * 2 * WH_SLOT)                     /* ... as two f16 parts of the column-scaled kernels + 512 column factors, [enc][layer-1][dir][WH_SLOT] */ \
  X(uint16_t, Ua, gru ? 0 : (size_t)2 * c.enc_depth * 2 * ua_slot(4))   /* recurrent kernels as MFMA A fragments (two f16 parts) + row factors, [enc][layer][dir][RV_UA_SLOT] */ \
  X(uint16_t, Wx16, gru ? 0 : L1 * wx16_slot(4))                  /* input kernels of encoder layers >= 1, both directions, as the split GEMM's B slabs, [enc][layer-1][RV_WX16_SLOT] */ \
  X(float, bx2, gru ? 0 : L1 * 2 * 4 * U)                         /* [b_fwd | b_bwd] of those layers, [enc][layer-1][1024] */                 \
  X(float, WcatT, gru ? 0 : (size_t)c.dec_depth * 4 * U * E)      /* ([W_dec[V:] ; U_dec])^T, [cell][512][256] */                             \
  X(float, Wmp, gru ? 0 : (size_t)E * E)                          /* [W_mem | A_c] [256][256] (A_c = W_att rows 128..383) */                   \
  X(uint16_t, Wmp16, gru ? 0 : (size_t)2 * E * E + 2 * E)         /* Wmp as two f16 parts in MFMA fragment order + column factors (RV_WMP16_SLOT) */ \
  X(uint16_t, Wkp16, gru ? 0 : (size_t)2 * E * U)                 /* the W_mem half of those parts, columns permuted into key-tile rows (RV_WKP16_SLOT) */ \
  X(float, Wcat2, gru ? 0 : (size_t)E * 4 * U)                    /* (one decoder cell): [W_a ; U + A_h W_a] [256][512] */                    \
  X(float, Nh, gru ? 0 : (size_t)U * MAX_VOCAB)                   /* (one or two decoder cells): A_h W_fc [128][V] */                          \
  X(uint16_t, Wc16, gru ? 0 : (size_t)2 * 3 * U * 4 * U)          /* (one or two cells): cell 0's folded kernel as two f16 parts in MFMA B-fragment order; room for two cells' 384 rows */ \
  X(uint16_t, Wc16p1, gru ? 0 : (size_t)E * 4 * U)                /* weight_parts 1: the first parts of Wc16 alone, [wave][pair][64 lanes][8 f16] */ \
  X(uint16_t, W1c16, gru || c.dec_depth != 2 ? 0 : (size_t)2 * E * 4 * U)   /* (two decoder cells): [W_1 | U_1] as MFMA B fragments */       \
  X(uint16_t, Wl16, gru ? 0 : (size_t)2 * E * 16)                 /* (one or two cells): [W_fc ; A_h W_fc] as MFMA B fragments */              \
  X(uint16_t, Wl16p1, gru ? 0 : (size_t)E * 16)                   /* weight_parts 1: its first parts alone, [8 k-steps][64 lanes][8 f16] */    \
  X(uint16_t, Wq16, gru ? 0 : (size_t)2 * U * U)                  /* (one decoder cell): Bahdanau's W_q as MFMA B fragments */                 \
  X(uint16_t, gUa, gru ? (size_t)2 * c.enc_depth * 2 * ua_slot(3) : 0)   /* GRU: recurrent kernels as MFMA A fragments + column factors, [enc][layer][dir][RV_GRU_UA_SLOT] */ \
  X(uint16_t, gWx16, gru ? L1 * wx16_slot(3) : 0)                 /* GRU: input kernels of encoder layers >= 1 as three B slabs of the split GEMM, [enc][layer-1][RV_GRU_WX16_SLOT] */ \
  X(float, gbx, gru ? L1 * 2 * 3 * U : 0)                         /* GRU: [b[0]_fwd | b[0]_bwd] of those layers, [enc][layer-1][768] */        \
  X(float, gWcatT, gru ? (size_t)c.dec_depth * 4 * U * E : 0)     /* GRU: decoder cells for k_dec_cell_gru, column tiles z, r, [W_h ; 0], [0 ; U_h], [cell][512][256] */

// Elements of every image a handle of (c, rnn) allocates
struct ImageCounts {
#define X(T, name, count) size_t name;
  RV_WEIGHT_IMAGES(X)
#undef X
};
ImageCounts image_counts(const RvConfig& c, int rnn);

// The weight-derived scalars that travel to the decode kernels by value (DecState::mx_*)
struct ImageScales {
  float kscale = 1.f, uscale = 1.f;         // powers of two from the bounds of [keys | U'] = enc_out . Wmp
  float cdescale = 1.f;                     // 1 / the power-of-two scale of the Wc16 image
  float ldescale = 1.f;                     // ... of the Wl16 image
  float qdescale = 1.f;                     // 2^-14 / the scale of the Wq16 image
  float c1descale = 1.f;                    // 1 / the scale of the W1c16 image
};

// What one rv_load_weights builds.  An image this load does not build (the configuration has none, or weight_parts says so) is empty;
// every other holds image_counts() elements.
struct HostImages {
#define X(T, name, count) std::vector<T> name;
  RV_WEIGHT_IMAGES(X)
#undef X
  ImageScales scales;
};

// blob: BlobLayout(c, rnn).total floats, already rounded (round_blob_weights) where weight_parts is 1
HostImages build_weight_images(const RvConfig& c, int rnn, int weight_parts, const float* blob);

// The images of the persistent decode of a GRU handle (option gru_persistent; decode.hip: k_dec_persist_gru), apart from the table
// above: a handle allocates and builds them only once that option is set.  One decoder cell.  The cell product's four column tiles of
// 128 are z, r and the candidate's input and recurrent halves; with W_a = rows V.. of the cell's W [V + u, 3 u], U its recurrent kernel
// and A_h, A_c the attention layer's h and context rows:
//   X(type, name, elements)
#define RV_GRU_PERSIST_IMAGES(X)                                                                                                        \
  X(float, gWmp, (size_t)E * E)                       /* [W_mem | A_c] [256][256], as Wmp */                                            \
  X(uint16_t, gWmp16, (size_t)2 * E * E + 2 * E)      /* ... as Wmp16 */                                                                \
  X(uint16_t, gWkp16, (size_t)2 * E * U)              /* ... as Wkp16 */                                                                \
  X(uint16_t, gWc16, (size_t)2 * E * 4 * U)           /* rows ctx': W_a,z | W_a,r | W_a,h | 0; rows h: U_z + A_h W_a,z | U_r + A_h W_a,r | A_h W_a,h | U_h; in Wc16's B-fragment order */ \
  X(uint16_t, gWl16, (size_t)2 * E * 16)              /* [W_fc ; A_h W_fc], as Wl16 */                                                  \
  X(uint16_t, gWq16, (size_t)2 * U * U)               /* Bahdanau's W_q, as Wq16 */                                                     \
  X(float, gWtok, (size_t)MAX_VOCAB * 4 * U)          /* the token's W row in tiles z, r, candidate-input; zeros in the fourth: [V][512] */ \
  X(float, gbdec, (size_t)4 * U)                      /* b[0] + b[1] for z and r, b[0]_h, b[1]_h: [512] */
struct GruPersistImages {
#define X(T, name, count) std::vector<T> name;
  RV_GRU_PERSIST_IMAGES(X)
#undef X
  ImageScales scales;                       // all but c1descale
};
// blob: BlobLayout(c, RV_RNN_BIGRU).total floats; c.dec_depth == 1
GruPersistImages build_gru_persist_images(const RvConfig& c, const float* blob);

// The builders of the image families that share the fragment writer of split_image.h, one slot each (tests/kernels/wimg_dump.cpp)
void pack_recurrent(const float* Uk, int g, uint16_t* img);        // Uk [128][128 g] -> [8 waves][g gates][4 k-steps][2 parts][64 lanes][8] + 128 g factors
void pack_wh(const float* W, uint16_t* img);                       // W [256][512] -> [32 tiles][2 parts][8 k-steps][64 lanes][8] (low part x 2048) + 512 factors
float pack_wq16(const float* Wq, uint16_t* img);                   // W_q [128][128] -> [8 waves][4 k-steps][2 parts][64 lanes][8]; returns its one scale

}  // namespace wimg
