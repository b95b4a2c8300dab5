// Shared declarations of the gfx950 kernels behind libravvent_hip.so.
// Units are fixed at u = d = 128 (every reference script uses 128:
// /root/reference/ravvent_performance_evaluator.py:92-93, ravvent.py:14-15); the recurrence
// kernel's register tiling is built around that number.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RV_U 128          // LSTM units per direction / decoder units
#define RV_G 512          // 4 gates x RV_U
#define RV_E 256          // encoder output width 2u
#define RV_MAX_BEAM 8
#define RV_MAX_VOCAB 8

// ---------------------------------------------------------------- kernel forms (rv_get_tensor "kernel_forms" / "kernel_form_list")
// A launcher given a FormLog notes the instantiation it launches, from the same walk of its form list that launches it: one row
// (kernel id, template parameters, zero-filled) per form, each row once.  Host code only.
enum {
  RV_K_DEC_PERSIST = 0,        // k_dec_persist<W, NIT, D, ATT>
  RV_K_DEC_ATTEND_FLASH = 1,   // k_dec_attend_flash<W, NT>
  RV_K_DEC_ATTEND = 2,         // k_dec_attend<W, TB, 4 TB>: (W, TB)
  RV_K_LSTM_REC = 3,           // k_lstm_rec<BT, F>
  RV_K_LSTM_REC_TW = 4,        // k_lstm_rec_tw<BT, F>
  RV_K_LSTM_REC_PROJ = 5,      // k_lstm_rec_proj<BT, SB>
  RV_K_LSTM_REC_MX = 6,        // k_lstm_rec_mx<F, CH>
  RV_K_INPROJ_SMALL = 7,       // k_inproj_small<F>
  RV_K_DEC_PERSIST_1P = 8,     // k_dec_persist_1p<W, NIT, ATT>: (W, NIT, 1, ATT); launched under option weight_parts 1 only
  RV_K_GRU_REC_MX = 9,         // k_gru_rec_mx<F, CH> (a GRU handle only: rv_create_rnn)
  RV_K_DEC_CELL_GRU = 10,      // k_dec_cell_gru: no parameters
  RV_K_DEC_PERSIST_GRU = 11,   // k_dec_persist_gru<W, NIT, ATT>: (W, NIT, 1, ATT); a GRU handle under option gru_persistent 1 only
  RV_K_LSTM_REC_MX_PROJ = 12,  // k_lstm_rec_mx_proj: (CH) = (16); launched under option fused_inproj only, a list of its own
};
#define RV_FORM_ROWS 512
struct FormLog {
  int n = 0;
  bool full = false;           // a row did not fit (rv_get_tensor then fails rather than answer with a short table)
  int row[RV_FORM_ROWS][5];
  void add(int k, int p1, int p2 = 0, int p3 = 0, int p4 = 0) {
    for (int i = 0; i < n; ++i)
      if (row[i][0] == k && row[i][1] == p1 && row[i][2] == p2 && row[i][3] == p3 && row[i][4] == p4) return;
    if (n == RV_FORM_ROWS) { full = true; return; }
    int* r = row[n++];
    r[0] = k; r[1] = p1; r[2] = p2; r[3] = p3; r[4] = p4;
  }
  void merge(const FormLog& o) {
    for (int i = 0; i < o.n; ++i) add(o.row[i][0], o.row[i][1], o.row[i][2], o.row[i][3], o.row[i][4]);
    full = full || o.full;
  }
};
// every instantiation the form lists hold, whatever a call would pick (the lists are walked; no kernel is named)
void list_rec_forms(FormLog& log);
void list_mx_forms(FormLog& log);
void list_mx_proj_forms(FormLog& log);     // the projecting matrix-pipe recurrence (option fused_inproj): a list of its own ("kernel_form_list_proj")
void list_decode_forms(FormLog& log);
void list_decode_forms_1p(FormLog& log);   // the one-part forms of the persistent decode: a list of their own ("kernel_form_list_1p")
void list_decode_forms_gru(FormLog& log);  // the persistent decode of a GRU cell: listed on a GRU handle's "kernel_form_list" only

// ---------------------------------------------------------------- K1: BiLSTM recurrence
// Members of a coalesced call whose inputs are read where their callers left them (matrix-pipe layer 0 only): chunk b of the group with
// row0[m] <= b < row0[m] + rows[m] is row b - row0[m] of x[m] [rows[m],T,F].  n = 0: every chunk is a row of RecArgs::x.
#define RV_MAX_MEMBERS 8
struct RecMembers { int n; int row0[RV_MAX_MEMBERS]; int rows[RV_MAX_MEMBERS]; const float* x[RV_MAX_MEMBERS]; };
// A chunk as windows of a read that lies on the device once (rv_beam_search_windows*): raw_len samples from `raw`,
// ev_len events of five features from `ev`.  The host resolves and bounds-checks every row against its read before anything is queued
// (0 <= len <= T, the window inside the read); positions len .. T - 1 of the chunk are the padding value.
struct RecWindow { const float* raw; const float* ev; int raw_len; int ev_len; };
struct RecArgs {
  const float* x;        // F>0: chunk input [B,T,F];  F==0: pre-projected xw [B,T,2,512] (bias folded)
  const float* W[2];     // F>0: input kernel [F,512] per direction
  const float* bias[2];  // F>0: [512] per direction
  const float* U[2];     // recurrent kernel [128,512] per direction (blob order)
  const float* Up[2];    // the same kernel in the recurrence's register order: [32 i][512 threads] float4 = (slot 0..3 of k = 32 kq + i), slot r = gate (kq + r) & 3 of unit j; thread = 4 j + kq
  const float* Wp[2];    // fused-projection kernel only: input kernel [256,512] as MFMA B fragments [32 tiles][16 k-groups][64 lanes][4]
  const uint16_t* Wsb[2];  // the same kernel as three bf16 parts for the split-bf16 projection, [32 tiles][3 parts][8 k-steps][64 lanes][8]; null = f32 MFMA
  const uint16_t* Wh[2];   // ... as two f16 parts of the column-scaled kernel, [32 tiles][2 parts][8 k-steps][64 lanes][8], then 512 floats 2^-14 / s_n; takes precedence over Wsb
  const uint16_t* Ua[2];   // matrix-pipe recurrence (lstm_mx.hip): U^T as MFMA A fragments, [8 waves][4 gates][4 k-steps][2 parts][64 lanes][8 f16]
                           // of the row-scaled kernel, then 512 floats 2^-14 / s_r (RV_UA_SLOT uint16 per direction)
  const float* h0[2];    // initial states [B,128] or nullptr (zeros)
  const float* c0[2];
  float* hT[2];          // final states [B,128]
  float* cT[2];
  float* out;            // [B,out_T,256]; direction d writes columns [128d,128d+128) at time out_t0+t
  int out_T, out_t0;
  int B, T;
  long long* dbg_ts;     // diagnostic builds (-DRV_REC_STAMPS, env RV_REC_STAMPS): [24] per-wave {busy, barrier-wait} cycle sums of workgroup (0,0)
  int tail_wave;         // layer 0 (F > 0), rows_per_block >= 2: the cell update runs on a ninth wave (k_lstm_rec_tw)
  int dbg_role;          // timing probe only (RV_DBG_ROLE): 1 = projection waves skip their math, 2 = recurrence waves skip theirs
  uint8_t* mask;         // matrix-pipe raw layer 0 only: also leaves utils.input_mask of its chunks at mask[b * mask_T + mask_t0 + t]
  int mask_T, mask_t0;   //   (the window is in LDS anyway; saves the slab a launch).  null = not asked for
  float pad;
  const void* const* ptab;   // matrix-pipe raw layer 0 only: non-null = read the chunk inputs' address from ptab[RV_PTAB_RAW] instead of `x`
  RecMembers members;        // matrix-pipe layer 0 only: n > 0 = the chunks' inputs are rows of the members' own tensors, not of `x`
  const RecWindow* windows;  // matrix-pipe layer 0 only: non-null = chunk b is the window windows[b] of a read (device table [B]), not a row of `x`
                             // (last: the argument offsets of every member above are those of the builds before it)
};
// Caller pointers of a slab call, read by the kernels through a small table in mapped pinned memory when the slab replays from a
// hipGraph whose kernel arguments are frozen (ravvent_hip.cpp, option "slab_graph": one graph per slab context and call shape): the
// only addresses that change from call to call.
enum { RV_PTAB_RAW = 0, RV_PTAB_EVENT = 1, RV_PTAB_TOKENS = 2, RV_PTAB_OUT2 = 3, RV_PTAB_N = 4 };
// F in {0,1,5}; rows_per_block in {1,2,4,8}
void launch_lstm_rec(const RecArgs& a, int F, int rows_per_block, hipStream_t s, FormLog* log = nullptr);
// layers >= 1 with x . W + b computed inside the kernel (MFMA waves beside the recurrence waves): a.x = [B,T,256] activations,
// a.Wp / a.bias per direction
void launch_lstm_rec_proj(const RecArgs& a, int rows_per_block, hipStream_t s, FormLog* log = nullptr);
// Matrix-pipe recurrence, RV_MX_ROWS chunks of one direction per workgroup (lstm_mx.hip).  F == 1: raw layer 0 (a.x = chunk inputs
// [B,T,1], a.W / a.bias per direction); F == 0: a.x = pre-projected inputs xw [B,T,2,512] (bias folded).  Needs a.Ua.
#define RV_MX_ROWS 16
#define RV_UA_SLOT ((size_t)2 * RV_U * RV_G + 2 * RV_G)
void launch_lstm_rec_mx(const RecArgs& a, int F, hipStream_t s, bool rows8 = false, FormLog* log = nullptr);   // rows8: eight chunks per workgroup (latency form)
// The projecting form for layers >= 1 (option fused_inproj; sixteen chunks per workgroup only): a.x = the previous layer's output
// act [B*T,256], a.Wh[0] = the split GEMM's image of the layer's input kernels (Wx16: both directions, RV_WX16_SLOT), a.bias[0] = their
// biases [b_fwd | b_bwd] (bx2).  No xw tensor: the results are those of launch_gemm_split_blocks + launch_lstm_rec_mx(F = 0), bit for bit.
void launch_lstm_rec_mx_proj(const RecArgs& a, hipStream_t s, FormLog* log = nullptr);
bool lstm_rec_mx_window_fits(int T, int F = 1);   // layer 0 with its input projection in the lane: do the input windows of a workgroup's chunks fit in LDS?
hipError_t configure_mx_kernels();
// The padded chunk tensors of a window table, written on the device (k_expand_windows): raw [B,T_r,1] from the rows' raw windows (null:
// not asked for), ev [B,T_e,5] from their event windows; positions beyond a window's length take `pad`.  For every path whose layer-0
// kernels read chunk tensors.
void launch_expand_windows(const RecWindow* windows, int B, float* raw, int T_r, float* ev, int T_e, float pad, hipStream_t s);
// xw [rows,2,512] = x [rows,F] . W_dir [F,512] + b_dir for a layer-0 encoder with F = 5 (or 1) input features, both directions
// mask != null: also writes utils.input_mask of the rows, mask[(r / T) * mask_T + mask_t0 + r % T] = all(x[r, :] != pad)
// xtab != null: x is read from xtab[RV_PTAB_EVENT] (F == 5) / xtab[RV_PTAB_RAW] (F == 1) on the device instead
void launch_inproj_small(const float* x, int rows, int F, const float* W0, const float* b0, const float* W1, const float* b1, float* xw,
                         uint8_t* mask, int T, int mask_T, int mask_t0, float pad, hipStream_t s, const void* const* xtab = nullptr,
                         FormLog* log = nullptr);
hipError_t configure_rec_kernels();   // dynamic-LDS opt-in of the recurrence kernels; first error or hipSuccess
// layer 0 stages its chunks' whole input windows in LDS: does a window of T steps x F features fit with that many rows per workgroup?
bool lstm_rec_window_fits(int F, int rows_per_block, int T);

// ---------------------------------------------------------------- K1g / D1g: the BiGRU family (gru_mx.hip)
#define RV_GG 384         // 3 gates (z, r, h) x RV_U
// Arguments of k_gru_rec_mx, a struct of its own: RecArgs travels by value into every LSTM recurrence kernel and stays as it is.
struct GruRecArgs {
  const float* x;          // F>0: chunk input [B,T,F];  F==0: pre-projected xw [B,T,2,384] = x . W + b[0]
  const float* W[2];       // F>0: input kernel [F,384] per direction
  const float* b[2];       // [2,384] per direction: row 0 the input bias (read by the F > 0 forms), row 1 the recurrent bias (every form)
  const uint16_t* Ua[2];   // U^T as MFMA A fragments, [8 waves][3 gates][4 k-steps][2 parts][64 lanes][8 f16] of the column-scaled kernel,
                           // then 384 floats 2^-14 / s_r (RV_GRU_UA_SLOT uint16 per direction)
  const float* h0[2];      // initial state [B,128] or nullptr (zeros); |h0| <= 1
  float* hT[2];            // final state [B,128]
  float* out;              // [B,out_T,256]; direction d writes columns [128d,128d+128) at time out_t0+t
  int out_T, out_t0;
  int B, T;
  uint8_t* mask;           // F>0: also leaves utils.input_mask of its chunks at mask[b * mask_T + mask_t0 + t]; null = not asked for
  int mask_T, mask_t0;
  float pad;
};
#define RV_GRU_UA_SLOT ((size_t)2 * RV_U * RV_GG + 2 * RV_GG)
// the split GEMM's image of a [256 x 768] input kernel (both directions, three column blocks of 256) and its 768 column factors
#define RV_GRU_WX16_SLOT ((size_t)2 * RV_E * 2 * RV_GG + 2 * 2 * RV_GG)
void list_gru_forms(FormLog& log);
hipError_t configure_gru_kernels();
bool gru_rec_mx_window_fits(int T, int F);     // layer 0: do the input windows of a workgroup's sixteen chunks fit in LDS?
void launch_gru_rec_mx(const GruRecArgs& a, int F, hipStream_t s, FormLog* log = nullptr);   // F in {0, 1, 5}
struct DecState;
// the GRU cell of the per-step decode, where launch_dec_cell launches k_dec_cell: WcatT [512,256] = column tiles z, r, [W_h ; 0],
// [0 ; U_h] of ([W_in ; U])^T, Wtok [V,384] (cell 0's one-hot rows, null for the cells above), bias [2,384]
void launch_dec_cell_gru(const DecState& d, int layer, const float* WcatT, const float* Wtok, const float* bias, int step, hipStream_t s,
                         FormLog* log = nullptr);

// ---------------------------------------------------------------- K0/K2: fp32 MFMA GEMM
struct GemmArgs {
  const float* A; int lda;     // [M,K]
  const float* Bm; int ldb;    // [K,N]
  float* C; int ldc;           // [M,N]
  int M, N, K;                 // K % 16 == 0, N % 64 == 0
  const float* bias;           // [N] or nullptr
  const uint8_t* row_mask;     // [M] or nullptr: masked-off rows are written as 0
  const int* gather_idx;       // [M] or nullptr: adds gather_tab[gather_idx[m]*ld_tab + n]
  const float* gather_tab; int ld_tab;
  // optional second problem sharing A (blockIdx.z == 1): the other LSTM direction of the same layer
  const float* Bm1; const float* bias1; float* C1;
  int xcd_remap;               // 1: 1-D grid, the workgroups sharing an A tile are dealt to ONE XCD (L2 reuse)
  const int* skip_flag; int skip_when;   // if skip_flag && *skip_flag >= skip_when: kernel exits
};
void launch_gemm_f32(const GemmArgs& a, bool small_tile, hipStream_t s);
// C[M,256] = A[M,256] . Wmp[256,256] on split-f16 MFMAs; img = [8 k-steps][16 tiles][2 parts][64 lanes][8 f16] of the column-scaled
// kernel, then 256 floats 2^-14 / s_n (RV_WMP16_SLOT uint16).  Precondition: |A| <= 1 (rows of an LSTM layer's output).
#define RV_WMP16_SLOT ((size_t)2 * RV_E * RV_E + 2 * RV_E)
void launch_gemm_mem_split(const float* A, int M, const uint16_t* img, float* C, hipStream_t s);
#define RV_WKP16_SLOT ((size_t)2 * RV_E * RV_U)      // DecState::Wkp16
// The same kernel over `ncb` column blocks of 256: C[M, ldc] (columns 256 cb ..) = A[M,256] . W_cb[256,256] (+ bias[256 cb ..]);
// img = [ncb][8 k-steps][16 tiles][2 parts][64 lanes][8 f16], then 256 ncb floats 2^-14 / s_n.  A workgroup takes the ncb blocks of a
// row tile one after the other, so A comes from HBM once.  The input projection of encoder layers >= 1 for the matrix-pipe
// recurrence: ncb = 4 (two directions x 512 gate columns), ldc = 1024, bias = [b_fwd | b_bwd]; of the BiGRU family: ncb = 3 (two
// directions x 384), ldc = 768 (RV_GRU_WX16_SLOT), on the weight-stationary form only.
#define RV_WX16_SLOT ((size_t)2 * RV_E * 2 * RV_G + 2 * 2 * RV_G)
hipError_t configure_gemm_kernels();   // dynamic-LDS opt-in of the weight-stationary split GEMM
void launch_gemm_split_blocks(const float* A, int M, const uint16_t* img, int ncb, const float* bias, float* C, int ldc, hipStream_t s);

// ---------------------------------------------------------------- small encoder-side kernels
void launch_input_mask(const float* raw, const float* ev, int B, int T_r, int T_e, float pad,
                       uint8_t* mask /*[B,T_r+T_e]*/, hipStream_t s);

// ---------------------------------------------------------------- decoder
struct DecState {
  // per-call shapes
  int B, W, Tm, V, L;
  int greedy, attention;
  int start_token, end_token, pad_token;
  // memory
  const float* keys;      // [B,Tm,128]
  const float* values;    // [B,Tm,256]  (= enc_output; masked positions never contribute)
  const uint8_t* mask;    // [B,Tm]
  // recurrent state, N = B*W rows
  // StackedRNNCells (basecaller.py:85-91): layer k's buffers sit at base + k * ls_* elements
  int depth;              // decoder_depth
  size_t ls_xh, ls_c;     // layer strides (elements) of xh and of c / c_new / h_new
  float* xh;              // [depth][N,256]: layer 0 = [attention | h_0], layer k>=1 = [h_{k-1} (new) | h_k]
  float* z;               // [N,512] gate pre-activations (unused by the fused cell kernel)
  float* c;               // [depth][N,128]
  float* c_new;           // [depth][N,128]
  float* h_new;           // [depth][N,128]
  int* tok;               // [N]
  float* log_probs;       // [N]
  uint8_t* finished;      // [N]
  int* lengths;           // [N]
  // weights
  const float* W_att;     // [384,128]
  const float* W_fc;      // [128,V]
  const float* b_fc;      // [V]
  const float* W_q;       // [128,128]
  const float* v_att;     // [128]
  // per-step records, time-major
  int* step_ids;          // [L-1,B,W]
  int* parent_ids;        // [L-1,B,W]
  float* step_scores;     // [L-1,B,W]
  float* step_logits;     // [L-1,B,W,V]   (greedy or debug) or nullptr
  float* step_align;      // [L-1,B,W,Tm]  (debug) or nullptr
  float* persist_align;   // [L-1,B,W,Tm]  alignments of the persistent decode (option persist_taps) or nullptr; unlike step_align
                          // it keeps the persistent decode, whose matrix-pipe forms record the f16 image the context product consumes
  int* nfin;              // [L] chunks-finished counter per step
  // optional fused post-processing of the best beam (basecaller.py:289-294 + utils.py:123-128)
  uint8_t* call_bases;    // [B,L-1] compacted base letters of tokens_to_nuc_sequences (or nullptr)
  float* call_probs;      // [B,L-1] exp(score_t - score_{t-1})
  int* call_len;          // [B] letters per chunk
  uint8_t lut[RV_MAX_VOCAB];   // token id -> upper-case letter, 0 for tokens the string form drops
  int* chunk_steps;       // persistent decode: [B] steps each chunk ran (nullptr on the per-step graph path)
  int* S_dev;             // [8]: [0] = S of the whole slab, [1+g] = S of sub-slab g
  int* S_host;            // device address of the host-mapped pinned words the call's S is left in (no copy launch for 4 bytes): [RV_MAX_MEMBERS],
                          // one per member of a coalesced call (DecMembers), word 0 for every other call
  // The form of the persistent decode this call runs (dec_persist_form: k_dec_persist's ATT), -1 on the per-step kernels.  Its
  // matrix-pipe forms take the scores (Luong) and the context as split-f16 MFMAs.  Scales: powers of two that bring the largest
  // value a key / a U' element can take (from the weights; |enc_out| <= 1) into [2^13, 2^14); descale = 2^-14 / scale (the query
  // and the alignments are scaled by 2^14)
  int persist_att; float mx_kscale, mx_kdescale, mx_uscale, mx_udescale;
  // Option fused_memory: the default form (Luong, one cell, ATT 3) projects its chunk's [keys | U'] itself (decode.hip,
  // persist_project_memory) when enc_rows is set: the encoder output [B,Tm,256] (`values` is not read then).  Wmp16 = the split GEMM's
  // image of [W_mem | A_c] with its column factors (RV_WMP16_SLOT; the A_c tiles feed the U' product as they are); Wkp16 = the W_mem
  // half of the same f16 parts with the columns permuted into the rows of the key tiles, [8 k-steps][8 tiles][2 parts][64 lanes][8 f16]:
  // lane (i, kq) of tile 2 ks + y holds column 32 ks + 8 (i / 4) + 4 y + i % 4 (RV_WKP16_SLOT uint16).  mem_tap (option persist_taps):
  // [B,Tm,256] that the workgroups also store their fp32 values to, or nullptr
  const float* enc_rows; const uint16_t* Wmp16; const uint16_t* Wkp16; float* mem_tap;
  // ... and the cell product [ctx' | h] . Wcat2 too (ATT 3, 4): Wc16 = Wcat2 as MFMA B fragments of two f16 parts,
  // [8 waves][32 (k-step, gate) pairs][2 parts][64 lanes][8 f16]; wave w owns units 16 w .. 16 w + 15 of all four gates; lane (n, kq)
  // of pair p = 4 ks + g holds T . Wcat2[k][128 g + 16 w + n] / xs[k], k = 32 ks + 8 kq + 0..7, with xs = mx_uscale for the ctx' rows
  // (k < 128) and 2^14 for the h rows -- the factors the inputs' f16 images carry -- and T the power of two that brings the largest
  // such element into [2^13, 2^14); mx_cdescale = 1 / T
  const uint16_t* Wc16; float mx_cdescale;
  // ... and the output layer of that decode: Wl16 = [W_fc ; A_h W_fc] [256][16 (V padded)] as B fragments of two f16 parts,
  // [8 k-steps][2 parts][64 lanes][8 f16] (16 KB), rows divided like Wc16's, one power-of-two scale; mx_ldescale = its inverse.
  // Wave 0 takes the logits of all beams as 24 MFMAs on the [ctx' | h] image while the other waves already stream the cell product
  const uint16_t* Wl16; float mx_ldescale;
  // Bahdanau on the matrix pipe (ATT 4): W_q [128][128] as B fragments of two f16 parts,
  // [8 waves][4 k-steps][2 parts][64 lanes][8 f16] (64 KB): wave w owns columns 16 w .. 16 w + 15, lane (n, kq) of k-step ks holds
  // T . W_q[32 ks + 8 kq + 0..7][16 w + n]; the A operand is the h half of the [ctx' | h] image (h 2^14): mx_qdescale = 2^-14 / T
  const uint16_t* Wq16; float mx_qdescale;
  // Two decoder cells on the matrix pipe (depth == 2, ATT 3).  Wc16 is then cell 0's product over [ctx' | h_1 | h_0]:
  // [W_a ; A_h W_a ; U_0] [384][512] as [8 waves][48 (k-step, gate) pairs][2 parts][64 lanes][8 f16] (768 KB; rows divided by mx_uscale /
  // 2^14 / 2^14, one power-of-two scale, mx_cdescale its inverse); W1c16 = cell 1's two products, [8 waves][32 pairs][2][64][8] (512 KB):
  // pairs 0..15 = W_1 (input product on h_0), pairs 16..31 = U_1 (recurrent product on h_1), rows divided by 2^14, one scale (mx_c1descale)
  const uint16_t* W1c16; float mx_c1descale;
  int attend_threads;     // 0: pick by slab size; 256 / 512: force that single-pass attend variant
  int part;               // sub-slab index (decode of one slab may run as up to 4 concurrent sub-slabs)
  long long* dbg_ts;      // diagnostic: [16] s_memtime stamps of block 0 at the phase boundaries of step 3
  int dbg_stop;           // diagnostic builds only: leave k_dec_attend after phase N (0 = run everything)
  // Forced decode (rv_teacher_forced*: Decoder.call with TrainingSampler, basecaller.py:142-152): label rows [B,L], row stride L, or
  // nullptr (every other call).  Set only with greedy and W == 1: step s feeds forced[b*L + s] instead of the previous argmax, step_ids
  // still records the argmax (sample_id), and every chunk runs exactly L - 1 steps -- nothing is added to nfin, chunk_steps[b] = L - 1.
  // An id outside [0, V) adds no input row (tf.one_hot gives zeros); the persistent decode takes such calls only with V < RV_MAX_VOCAB
  // (last: the kernel-argument offsets of the members above are those of every earlier build)
  const int* forced;
  // Moves (rv_beam_search_moves*): where in the memory each step's attention lay, one record per beam row as it
  // is when the attention of the step runs (before the step's top-k reorders the rows), reduced on chip from the alignments the
  // context product consumes.  step_moves [L-1,B,W,RV_MOVE_COLS]: raw_mass = sum_{t < Tr} a_t, raw_m1 = sum_{t < Tr} a_t t,
  // event_mass = sum_{Tr <= t < Tm} a_t, event_m1 = sum_{Tr <= t < Tm} a_t (t - Tr), peak_weight = max_t a_t, peak_t = the first t
  // holding it (as a float; -1 and NaN in the other five when the row's alignments are NaN: an all-padding chunk).  nullptr: every
  // other call -- the kernels test the pointer at run time.  Tr: the split index (T_m in raw mode, 0 in event mode).
  // moves_only (per-step kernels): this launch of k_dec_attend leaves after its softmax, having written the step's records alone
  // (appended like `forced`: the offsets above stay)
  float* step_moves; int Tr; int moves_only;
};
#define RV_MOVE_COLS 6
hipError_t configure_decode_kernels();   // per-device dynamic-LDS opt-in; call after hipSetDevice; first error or hipSuccess
void launch_dec_init(const DecState& d, hipStream_t s);
// layer: which stacked cell; Wtok (one-hot embedding rows) is non-null for layer 0 only
void launch_dec_cell(const DecState& d, int layer, const float* WcatT /*[512,256] = ([W_in;U])^T*/, const float* Wtok /*[V,512]*/,
                     const float* bias /*[512]*/, int step, hipStream_t s);
// flash: single-pass Luong attend over `values` only (WmemT = W_mem^T [128,256]); else the two-pass kernel
void launch_dec_attend(const DecState& d, const float* WmemT, bool flash, int step, hipStream_t s, FormLog* log = nullptr);
// Persistent decode (Luong beam search with W <= 8, W <= 5 with two stacked cells; greedy search; no taps): the whole loop in
// one launch, the chunk's attention memory resident in registers; also writes S_dev[0..1].  d.values must point at the
// PROJECTED memory [B,Tm,256] = enc_output . [W_mem | A_c] (keys | attention-layer image of the values).
// One cell: Wcat = [W_a ; U + A_h W_a] and Nh = A_h W_fc [128,V] (the attention layer's h part folded into the weights);
// two cells: Wcat = [W_a ; U_0], Wcat1 / bdec1 = second cell ([W_1;U_1], b_1), Nh unused.  Launches the form d.persist_att.
// dec_persist_form: the one place that picks that form from a call's options and shape -- k_dec_persist's ATT (PersistLds: Luong 0
// on packed FMAs, 2 with the scores and context on the matrix pipe (option matrix_attention, one cell), 3 with the cell product and
// the output layer there too (and matrix_cell); Bahdanau 1 on packed FMAs, 4 with all but the scores on the matrix pipe (both options,
// one cell)), or -1 when no instantiation serves the call or its LDS does not fit.  W: the effective beam (1 for greedy search).
int dec_persist_form(int attention, int depth, int W, int Tm, bool greedy, bool matrix_attention, bool matrix_cell);
void launch_dec_persist(const DecState& d, const float* Wcat /*[256,512]*/, const float* Wtok /*[V,512]*/,
                        const float* bdec /*[512]*/, const float* Wcat1, const float* bdec1, const float* Nh, hipStream_t s,
                        FormLog* log = nullptr, const uint16_t* Wc16p1 = nullptr, const uint16_t* Wl16p1 = nullptr);
// Wc16p1 / Wl16p1 (option weight_parts 1; both or neither): the first f16 parts of the Wc16 / Wl16 images on their own.  Where the
// one-part list holds a form for the call, k_dec_persist_1p runs on them in k_dec_persist's place; elsewhere k_dec_persist runs on
// d's two-part images, whose second parts are zero then -- the same results bit for bit, but for the sign of a zero
// The persistent decode of ONE Keras GRU cell (reset_after), k_dec_persist_gru: the same body and arguments with d.Wc16 / d.Wl16 /
// d.Wq16 naming the folded GRU images (weight_images.h: GruPersistImages), Wtok [V,512] / bdec [512] its token table and bias in the
// cell product's four tiles z, r, candidate-input, candidate-recurrent.  att: 3 Luong, 4 Bahdanau.  dec_persist_form_gru: att when the
// GRU list holds a form for (W, T_m) and its LDS fits, else -1
int dec_persist_form_gru(int attention, int W, int Tm, bool greedy);
void launch_dec_persist_gru(const DecState& d, const float* Wtok, const float* bdec, hipStream_t s, FormLog* log = nullptr);
// ptab != null: the two output addresses are read from ptab[RV_PTAB_TOKENS] / ptab[RV_PTAB_OUT2] on the device instead
// Members (persistent beam-search decode only): the slab is n slabs of the asynchronous calls decoded as one, back to back.  Member m
// owns rows row0[m] .. row0[m] + rows[m] - 1: its S is the maximum of chunk_steps over those rows alone, goes to S_host[m], and its rows
// are written through tokens[m] / out2[m] at the member's own row index.  n = 0: one member, the whole slab, the launcher's two pointers.
struct DecMembers { int n; int row0[RV_MAX_MEMBERS]; int rows[RV_MAX_MEMBERS]; int32_t* tokens[RV_MAX_MEMBERS]; float* out2[RV_MAX_MEMBERS]; };
void launch_dec_finalize(const DecState& d, int32_t* tokens /*[B,L-1]*/, float* scores_or_logits, hipStream_t s, const void* const* ptab = nullptr,
                         const DecMembers* members = nullptr);
struct DecParts { const int* nfin[4]; int B[4]; int n; int steps; int* S_dev; int* S_host; };
void launch_dec_reduce_steps(const DecParts& p, hipStream_t s);   // S_dev[0] = max_g S_g, S_dev[1+g] = S_g
// The whole beam of a call (beams.hip, rv_beam_search_all*): k_dec_finalize_beams takes k_dec_finalize's place for such a call, one
// launch per decode part.  Row stride (L-1) W, beam innermost; tokens / scores / path_scores [B,L-1,W], log_probs / lengths [B,W]
// (include/ravvent_hip.h: RvBeams).  path_scores, log_probs and lengths may be null: the kernel skips a null output.
struct BeamsOut { int32_t* tokens; float* scores; float* path_scores; float* log_probs; int32_t* lengths; };
void launch_dec_finalize_beams(const DecState& d, const BeamsOut& o, hipStream_t s);
// The moves of a call (moves.hip, rv_beam_search_moves*): k_dec_finalize_moves runs behind k_dec_finalize_beams, one launch per decode
// part, and back-traces the step_moves records like the tokens.  Six outputs [B,L-1,W], beam innermost (include/ravvent_hip.h:
// RvMoves); the kernel skips a null output.
struct MovesOut { float* raw_pos; float* raw_mass; float* event_pos; float* event_mass; int32_t* peak; float* peak_weight; };
void launch_dec_finalize_moves(const DecState& d, const MovesOut& o, hipStream_t s);
// The moves of a call with fused post-processing (rv_beam_search_calls_moves*): k_dec_finalize_calls_moves runs behind k_dec_finalize,
// one launch per decode part, back-traces the best hypothesis' records and compacts them like call_bases.  `tokens` [B,L-1]: what
// k_dec_finalize of that part wrote.  Six outputs [B,L-1] (include/ravvent_hip.h: RvCallMoves); the kernel skips a null output.
void launch_dec_finalize_calls_moves(const DecState& d, const int32_t* tokens, const MovesOut& o, hipStream_t s);
// The moves of a forced decode (rv_teacher_forced_moves*): k_forced_moves hands out step t's record in column t, [B,L-1]; needs
// d.forced and d.step_moves.
void launch_forced_moves(const DecState& d, const MovesOut& o, hipStream_t s);

// ---------------------------------------------------------------- scoring (score.hip)
// Masked sparse cross-entropy and masked token accuracy of label rows against logits (Basecaller.loss_function, basecaller.py:212-220;
// utils.masked_accuracy, utils.py:15-24), per position and per chunk; the caller forms the two scalar quotients.  One wave per chunk,
// lane = position: S <= 64, 2 <= V <= RV_MAX_VOCAB.  Every output may be null.
struct ScoreArgs {
  const float* logits;      // [B,S,V]
  const int* labels;        // row b at labels + b * label_stride, S ids
  int label_stride;
  int B, S, V;
  int pad_token;            // nll is 0 and n_labels does not count where label == pad_token (the mask of loss_function)
  uint32_t omit_mask;       // bit t set: label id t is left out of n_counted / n_match (masked_accuracy's omit_vals)
  float* nll;               // [B,S]  logsumexp(logits) - logits[label], max-subtracted; NaN for a non-pad label outside [0, V)
  int* pred;                // [B,S]  argmax, first maximum on ties
  float* nll_sum;           // [B]    nll summed over the row in column order by one lane
  int* n_labels;            // [B]    labels != pad_token
  int* n_match;             // [B]    counted labels that equal pred
  int* n_counted;           // [B]    labels outside the omit set
};
void launch_score_tokens(const ScoreArgs& a, hipStream_t s);

// ---------------------------------------------------------------- device math helpers
#ifdef __HIPCC__
#ifdef RV_ACT_IEEE
// A/B build only (make actvar): the library's activations as the IEEE functions -- the fp32 floor of the recurrences' error
__device__ __forceinline__ float rv_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float rv_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ float rv_tanh_abs(float x) { return tanhf(x); }
#else
__device__ __forceinline__ float rv_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
__device__ __forceinline__ float rv_tanh(float x) {
  // Relative accuracy at every magnitude (2 sigmoid(2x) - 1 has an ABSOLUTE error of ~1e-7: 9e-2 relative at 1e-6, zero below
  // 3e-8, and a large recurrent gain multiplies that step after step).  |x| < 0.25: the odd Taylor polynomial to x^11 (truncation
  // < 3e-10 relative); above: (1 - e) / (1 + e), e = exp(-2|x|) (1 - e is exact up to |x| = 0.35 and never loses more than a factor
  // 1.6 of e's accuracy); |x| >= 9: 1 exactly; then x's sign.  Exactly odd, +-0 -> +-0, +-inf -> +-1, NaN -> NaN.  Branch-free:
  // both forms, two selects.  (The x^9 polynomial without the |x| >= 9 select, as accurate, makes k_lstm_rec_mx<5, 16> spill.)
  const float a = fabsf(x);
  const float e = __expf(-2.0f * a);
  const float big = (1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e);
  const float a2 = a * a;
  float p = fmaf(a2, -1382.0f / 155925.0f, 62.0f / 2835.0f);
  p = fmaf(p, a2, -17.0f / 315.0f);
  p = fmaf(p, a2, 2.0f / 15.0f);
  p = fmaf(p, a2, -1.0f / 3.0f);
  const float small = fmaf(p * a2, a, a);
  return copysignf(a < 0.25f ? small : (a >= 9.0f ? 1.0f : big), x);
}
// 2 sigmoid(2x) - 1 (absolute error ~1e-7), kept for one site only: the g gate of the decode form with the Luong attention on the
// matrix pipe and the cell product on packed FMAs (decode.hip, dec_gate_tanh), where rv_tanh pushes k_dec_persist<5,11,1,2> over its
// scratch bound in tests/test_build.py
__device__ __forceinline__ float rv_tanh_abs(float x) {
  return fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * x)), -1.0f);
}
#endif
#endif
