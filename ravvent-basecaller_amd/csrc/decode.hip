// Decoder-side kernels: one AttentionWrapper step + output layer + beam expansion per launch
// pair, replacing the tf.while_loop body of tfa.seq2seq.BeamSearchDecoder / BasicDecoder that
// /root/reference/basecaller.py:306-313 and :322-329 drive (semantics: SURVEY.md A.3-A.6).
//
//   k_dec_gates   LSTM cell non-linearity on the pre-activations the D1 GEMM produced.
//   k_dec_attend  ONE workgroup per chunk handles all W beams of that chunk, so keys/values are
//                 read once per chunk instead of once per beam (the reference tiles them W times,
//                 tile_batch at basecaller.py:300-301): score (Luong q.k / Bahdanau v.tanh(k+Wq q)),
//                 -inf masking, softmax, context, attention layer, fc, log-softmax, finished-beam
//                 masking, top-W over W*V, and the parent-gather of every state tensor.
//   k_dec_finalize gather_tree for beam 0 + slicing of predicted_ids[:,:,0] / scores[:,:,0].
// Loop control: the reference stops when ALL rows are finished; here each chunk-workgroup counts
// itself into nfin[step] once all its beams are finished, and every kernel of step s exits early
// when nfin[s-1] == B (the launch sequence is fixed, so it can live in a hipGraph).
#include "common.h"
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <type_traits>

namespace {

__global__ void k_input_mask(const float* raw, const float* ev, int B, int T_r, int T_e, float pad,
                             uint8_t* mask) {
  const int Tm = T_r + T_e;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * Tm) return;
  const int b = idx / Tm, t = idx % Tm;
  bool ok;
  if (t < T_r) {
    ok = raw[(size_t)b * T_r + t] != pad;            // all(x != pad) over the 1 raw feature
  } else {
    const float* e = ev + ((size_t)b * T_e + (t - T_r)) * 5;
    ok = e[0] != pad && e[1] != pad && e[2] != pad && e[3] != pad && e[4] != pad;
  }
  mask[idx] = ok ? 1 : 0;
}

__global__ void k_dec_init(DecState d) {
  const int N = d.B * d.W;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < N) {
    d.tok[idx] = d.forced ? d.forced[(size_t)idx * d.L] : d.start_token;   // forced decode (W == 1): TrainingSampler feeds the label row's own first token
    d.log_probs[idx] = (idx % d.W) == 0 ? 0.f : -INFINITY;   // one_hot(0, W, on=0, off=-inf)
    d.finished[idx] = 0;
    d.lengths[idx] = 0;
  }
  if (idx < d.L) d.nfin[idx] = 0;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// D1 -- decoder LSTM cell, fused: pre-activations on v_mfma_f32_16x16x4_f32 + gate math.
// z = [attention | h] . [W_dec[V:] ; U_dec] + W_dec[token] + b  (cell input = concat(one_hot, attention),
// SURVEY.md A.4; the one-hot product is a row gather).
// Workgroup = 64 beam rows x 16 units x 4 gates, K = 256 in one shot: the 64 KB activation panel and
// the 64 KB weight panel (pre-transposed to [col][k] at load time, so both are coalesced 1 KB row
// copies) go to LDS with every load in flight -- the epilogue's token / bias / cell-state operands are
// fetched first so their round trips hide under the panels -- ONE barrier, then each of the 8 waves
// runs 2 x 64 MFMAs (16 rows x one gate's 16 units per tile, operands read as float4 along k) and the
// four gate tiles meet in LDS for the cell update.  (Measured alternatives: fragments straight from
// global to registers 14 us -- 64 cache lines per load instruction; 32-row tiles 12 us -- two
// rounds of workgroups; this form 8-10 us.)
constexpr int CELL_LD = 260;                       // padded row length of the LDS panels (floats)
constexpr int CELL_ROWS = 64;
constexpr int CELL_LDS_FLOATS = (CELL_ROWS + 64) * CELL_LD + 4 * CELL_ROWS * 17;
__global__ __launch_bounds__(512) void k_dec_cell(DecState d, int layer, const float* __restrict__ WcatT,
                                                  const float* __restrict__ Wtok, const float* __restrict__ bias,
                                                  int step) {
  if (step > 0 && d.nfin[step - 1] >= d.B) return;
  const float* xh_l = d.xh + layer * d.ls_xh;
  const float* c_l = d.c + layer * d.ls_c;
  float* cn_l = d.c_new + layer * d.ls_c;
  float* hn_l = d.h_new + layer * d.ls_c;
  float* xh_up = layer + 1 < d.depth ? d.xh + (layer + 1) * d.ls_xh : nullptr;   // next cell's input half
  extern __shared__ __align__(16) float csm[];
  float* As = csm;                                  // [64 rows][260]
  float* Bs = csm + CELL_ROWS * CELL_LD;            // [64 cols = 4 gates x 16 units][260]
  float* zs = csm + (CELL_ROWS + 64) * CELL_LD;     // [4 gates][64 rows][17]
  const int N = d.B * d.W;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r0 = blockIdx.y * CELL_ROWS, u0 = blockIdx.x * 16;
  // epilogue operands first (their round trips hide under the panel loads): thread = 2 x (row, unit)
  int en[2]; float ec[2], eb[4], ew[2][4];
  const int eun = tid & 15, ecol = u0 + eun;
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) eb[gg] = bias[gg * RV_U + ecol];
  int etok[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    en[p] = min(r0 + (tid >> 4) + 32 * p, N - 1);
    etok[p] = Wtok ? d.tok[en[p]] : 0;
    ec[p] = c_l[(size_t)en[p] * RV_U + ecol];
  }
  float4 ra[8], rb[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int idx = tid + 512 * p, row = idx >> 6, c4 = idx & 63;        // 64 float4 per 1 KB row
    const int n = min(r0 + row, N - 1);
    ra[p] = *reinterpret_cast<const float4*>(xh_l + (size_t)n * RV_E + 4 * c4);
    const int col = (row >> 4) * RV_U + u0 + (row & 15);                 // panel row = gate*16 + unit
    rb[p] = *reinterpret_cast<const float4*>(WcatT + (size_t)col * RV_E + 4 * c4);
  }
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int idx = tid + 512 * p, row = idx >> 6, c4 = idx & 63;
    *reinterpret_cast<float4*>(As + row * CELL_LD + 4 * c4) = ra[p];
    *reinterpret_cast<float4*>(Bs + row * CELL_LD + 4 * c4) = rb[p];
  }
#pragma unroll
  for (int p = 0; p < 2; ++p)       // one-hot row gather; lands while the MFMAs run
#pragma unroll
    for (int gg = 0; gg < 4; ++gg)      // (an id outside the vocabulary -- a forced decode's device labels -- adds no row: tf.one_hot gives zeros)
      ew[p][gg] = (Wtok && (unsigned)etok[p] < (unsigned)d.V) ? Wtok[(size_t)etok[p] * RV_G + gg * RV_U + ecol] : 0.f;
  __syncthreads();
  const int rq = wv & 3, gh = wv >> 2;            // wave = 16-row quarter x gate pair
  const int li = lane & 15, kq = lane >> 4;       // lane group kq supplies k in [64kq, 64kq+64)
  const float4* ap = reinterpret_cast<const float4*>(As + (16 * rq + li) * CELL_LD + 64 * kq);
#pragma unroll
  for (int gi = 0; gi < 2; ++gi) {
    const int g = 2 * gh + gi;
    const float4* bp = reinterpret_cast<const float4*>(Bs + (16 * g + li) * CELL_LD + 64 * kq);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 av = ap[i], bv = bp[i];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc1, 0, 0, 0);
    }
    // C/D map of the 16x16 tile: col = lane & 15, row = 4*(lane >> 4) + reg
#pragma unroll
    for (int r = 0; r < 4; ++r) zs[(g * CELL_ROWS + 16 * rq + 4 * kq + r) * 17 + li] = acc0[r] + acc1[r];
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int row = (tid >> 4) + 32 * p;
    if (r0 + row < N) {
      const float zi = zs[(0 * CELL_ROWS + row) * 17 + eun] + ew[p][0] + eb[0];
      const float zf = zs[(1 * CELL_ROWS + row) * 17 + eun] + ew[p][1] + eb[1];
      const float zg = zs[(2 * CELL_ROWS + row) * 17 + eun] + ew[p][2] + eb[2];
      const float zo = zs[(3 * CELL_ROWS + row) * 17 + eun] + ew[p][3] + eb[3];
      const float c2 = fmaf(rv_sigmoid(zf), ec[p], rv_sigmoid(zi) * rv_tanh(zg));
      const float hh = rv_sigmoid(zo) * rv_tanh(c2);
      cn_l[(size_t)en[p] * RV_U + ecol] = c2;
      hn_l[(size_t)en[p] * RV_U + ecol] = hh;
      if (xh_up) xh_up[(size_t)en[p] * RV_E + ecol] = hh;
    }
  }
}

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
// 8 floats -> two f16 fragments of v * scale: hi = f16(s), lo = f16(s - hi) (the residual is exact in f32)
__device__ __forceinline__ void split_f16x8(const float* v, float scale, float4& hi, float4& lo) {
  h8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float sv = v[j] * scale;
    a[j] = (_Float16)sv;
    b[j] = (_Float16)(sv - (float)a[j]);
  }
  hi = __builtin_bit_cast(float4, a); lo = __builtin_bit_cast(float4, b);
}

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
// sum over the 16 lanes of a DPP row; every lane ends with the total
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp<0x141>(v);   // row_half_mirror
  v += dpp<0x140>(v);   // row_mirror
  return v;
}
// value of lane n (0..7) of the caller's 16-lane row, in every lane of that row (DPP row_newbcast)
__device__ __forceinline__ float row_bcast(float v, int n) {
  switch (n) {
    case 0: return dpp<0x150>(v); case 1: return dpp<0x151>(v); case 2: return dpp<0x152>(v);
    case 3: return dpp<0x153>(v); case 4: return dpp<0x154>(v); case 5: return dpp<0x155>(v);
    case 6: return dpp<0x156>(v); default: return dpp<0x157>(v);
  }
}
// same, source lane n in 0..15
__device__ __forceinline__ float row_bcast16(float v, int n) {
  switch (n) {
    case 0: return dpp<0x150>(v); case 1: return dpp<0x151>(v); case 2: return dpp<0x152>(v); case 3: return dpp<0x153>(v);
    case 4: return dpp<0x154>(v); case 5: return dpp<0x155>(v); case 6: return dpp<0x156>(v); case 7: return dpp<0x157>(v);
    case 8: return dpp<0x158>(v); case 9: return dpp<0x159>(v); case 10: return dpp<0x15A>(v); case 11: return dpp<0x15B>(v);
    case 12: return dpp<0x15C>(v); case 13: return dpp<0x15D>(v); case 14: return dpp<0x15E>(v); default: return dpp<0x15F>(v);
  }
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// wave-uniform max via DPP inside the four 16-lane rows + readlane across them (no LDS round trips)
__device__ __forceinline__ float wave_max_fast(float v) {
  v = fmaxf(v, dpp<0xB1>(v));
  v = fmaxf(v, dpp<0x4E>(v));
  v = fmaxf(v, dpp<0x141>(v));
  v = fmaxf(v, dpp<0x140>(v));
  const int vi = __float_as_int(v);
  const float a = __int_as_float(__builtin_amdgcn_readlane(vi, 0)), b = __int_as_float(__builtin_amdgcn_readlane(vi, 16));
  const float c = __int_as_float(__builtin_amdgcn_readlane(vi, 32)), e = __int_as_float(__builtin_amdgcn_readlane(vi, 48));
  return fmaxf(fmaxf(a, b), fmaxf(c, e));
}

// wave-uniform sum, fixed order: DPP inside the 16-lane rows, then rows 0..3 left to right
__device__ __forceinline__ float wave_sum_fast(float v) {
  v = row16_sum(v);
  const int vi = __float_as_int(v);
  const float a = __int_as_float(__builtin_amdgcn_readlane(vi, 0)), b = __int_as_float(__builtin_amdgcn_readlane(vi, 16));
  const float c = __int_as_float(__builtin_amdgcn_readlane(vi, 32)), e = __int_as_float(__builtin_amdgcn_readlane(vi, 48));
  return ((a + b) + c) + e;
}

// ---- moves (DecState::step_moves): a beam row's record of one step, reduced from its alignments.  A lane adds its own steps in
// ascending t, partial records merge pairwise in an order fixed by the lane / wave numbers alone; sums commute, and of two equal
// peaks the smaller t stays, so both sides of a butterfly exchange end with the same bits.
struct MoveAcc { float rm, r1, em, e1, pk; int pt; };
__device__ __forceinline__ MoveAcc move_zero() { return MoveAcc{0.f, 0.f, 0.f, 0.f, -INFINITY, -1}; }
__device__ __forceinline__ void move_add(MoveAcc& a, float al, int t, int Tr) {
  // (selects, not a branch over the members: the compiler turns that into an indexed access of the record, in scratch.  Adding 0 and
  // fma(0, t, x) leave a sum's bits alone)
  const float ar = t < Tr ? al : 0.f, ae = t < Tr ? 0.f : al;
  a.rm += ar; a.r1 = fmaf(ar, (float)t, a.r1);
  a.em += ae; a.e1 = fmaf(ae, (float)(t - Tr), a.e1);
  if (al > a.pk) { a.pk = al; a.pt = t; }      // strict: the first maximum; a NaN never enters
}
__device__ __forceinline__ void move_merge(MoveAcc& a, const MoveAcc& o) {
  a.rm += o.rm; a.r1 += o.r1; a.em += o.em; a.e1 += o.e1;
  if (o.pk > a.pk || (o.pk == a.pk && (unsigned)o.pt < (unsigned)a.pt)) { a.pk = o.pk; a.pt = o.pt; }
}
__device__ __forceinline__ MoveAcc move_shfl_xor(const MoveAcc& a, int x) {
  return MoveAcc{__shfl_xor(a.rm, x), __shfl_xor(a.r1, x), __shfl_xor(a.em, x), __shfl_xor(a.e1, x), __shfl_xor(a.pk, x), __shfl_xor(a.pt, x)};
}
// No alignment was greater than -inf: the row is NaN (all-padding chunk) -- NaN in the five value columns whatever the segments hold.
// z = pk - pk is that NaN (-inf - -inf) and +0 for every other row, and v + 0 is v for these non-negative values: no select, and no
// NaN constant for the compiler to keep in a register through the persistent decode's step loop
__device__ __forceinline__ void move_store(float* rec, const MoveAcc& a) {
  const float z = a.pk - a.pk;
  rec[0] = a.rm + z; rec[1] = a.r1 + z; rec[2] = a.em + z; rec[3] = a.e1 + z; rec[4] = a.pk + z;
  rec[5] = (float)a.pt;
}
// one wave owns the row: lane `lane` holds the partial record of its steps
__device__ __forceinline__ void move_wave_store(float* rec, MoveAcc a, int lane) {
  for (int x = 32; x > 0; x >>= 1) { const MoveAcc o = move_shfl_xor(a, x); move_merge(a, o); }
  if (lane == 0) move_store(rec, a);
}

constexpr int WB = RV_MAX_BEAM;
constexpr int ATT_THREADS = 512;
#ifndef RV_STAMP_WAVE
#define RV_STAMP_WAVE 1      // which wave stamps its cell product (diagnostic builds may pick another: make decvar DECFLAGS=-DRV_STAMP_WAVE=4)
#endif
#define RV_STAMP_W1(d, step, i) do { if ((d).dbg_ts && blockIdx.x == 0 && threadIdx.x == 64 * RV_STAMP_WAVE && (step) == 3) (d).dbg_ts[i] = __builtin_readcyclecounter(); } while (0)
#define RV_STAMP(d, step, i) do { if ((d).dbg_ts && blockIdx.x == 0 && threadIdx.x == 0 && (step) == 3) (d).dbg_ts[i] = __builtin_readcyclecounter(); } while (0)
constexpr float LOG2E = 1.4426950408889634f;
// Matrix-pipe forms of the persistent decode: the A operand of every product (query, alignments, [ctx' | h]) has the beams as rows,
// at most 8 of an MFMA tile's 16.  Both f16 PARTS of a beam's value therefore ride in ONE tile -- beam w: high part in row
// 4 (w % 4) + 2 (w / 4), low part in the row after it -- so a product is TWO MFMAs per k-step (the tile against the high and against the
// low part of B) instead of three, and one LDS read per k-step instead of two: rows r, r + 1 of `. B_hi` and row r of `. B_lo` are the
// three exact part products (row r + 1 of `. B_lo` is the low x low term, below 2^-22 of the product: it is simply added too).
// C/D map of the 16x16 tile: lane (column l % 16, g = l / 16) holds rows 4 g + i, i = 0..3: registers 0 + 1 = beam g, 2 + 3 = beam g + 4.
__host__ __device__ constexpr int mx_row(int w) { return 4 * (w & 3) + 2 * (w >> 2); }

// Static LDS shared by both attend kernels: output layer, new cell states, beam bookkeeping.
struct AttShared {
  float wfc[RV_U * RV_MAX_VOCAB + RV_MAX_VOCAB];   // W_fc [128][V] then b_fc [V]
  float cnew[WB * RV_U];
  float lprob[WB];
  int fin[WB], len[WB], parent[WB];
};

// Dynamic LDS carve-up (floats), shared with the host-side size computation.
struct AttLds {
  int q, pq, sc, al, part, hcT, att, lg, fold, total;
  __host__ __device__ AttLds(int W, int TmP, bool flash, int NT = 512) {
    const int NW = NT / 64;                     // waves per workgroup
    int o = 0;
    q = o; o += W * RV_U;
    pq = o; o += flash ? W * RV_E : W * RV_U;   // Bahdanau processed query [W][128] / flash q' [W][256]
    sc = o; o += flash ? (NT / 16) * WB * 2 : W * TmP; // two-pass: scores [W][TmP]; flash: per-stream (max, sum) [NT/16][WB][2]
    al = o; o += flash ? 2 * WB : TmP * WB;     // two-pass: alignments [TmP][WB]; flash: merged (max, 1/sum)
    part = o; o += NW * W * RV_E;               // partial sums [NW][W][256] (also [2 NW][W][128])
    hcT = o; o += (RV_U + RV_E) * WB;           // [h ; context] k-major, beam-minor
    att = o; o += W * RV_U;
    lg = o; o += WB * RV_MAX_VOCAB;
    fold = o; o += flash ? NW * W * 4 * (NT == 512 ? 32 : 16) * 4 : 0;  // flash: wave-private fold slabs [NW][W*4][32|16] float4
    total = o;
  }
};

// ---- phase A: one round of small loads -> LDS: query = cell output h of every beam (also rows
// 0..127 of hcT), the new cell states, the beam bookkeeping and the output layer.
template <int W, int NT>
__device__ __forceinline__ void att_prologue(const DecState& d, AttShared& S, float* q, float* hcT, size_t row0, int tid) {
  constexpr int ATT_THREADS = NT;
  const int V = d.V;
  const float* hn_top = d.h_new + (d.depth - 1) * d.ls_c;
  const float* cn_top = d.c_new + (d.depth - 1) * d.ls_c;
  for (int i = tid; i < W * RV_U; i += ATT_THREADS) {
    const float v = hn_top[row0 * RV_U + i];
    q[i] = v;
    hcT[(i & 127) * WB + (i >> 7)] = v;
    S.cnew[i] = cn_top[row0 * RV_U + i];
  }
  for (int i = tid; i < RV_U * V; i += ATT_THREADS) S.wfc[i] = d.W_fc[i];
  if (tid < V) S.wfc[RV_U * V + tid] = d.b_fc[tid];
  if (tid < W) {
    S.fin[tid] = d.finished[row0 + tid];
    S.lprob[tid] = d.log_probs[row0 + tid];
    S.len[tid] = d.lengths[row0 + tid];
  }
}

// ---- phases E-H: attention layer, output layer, sampler / beam step, parent-gather of the state.
// Expects hcT = [h ; context] complete and a barrier behind it.
template <int W, int NT>
__device__ __forceinline__ void att_tail(const DecState& d, AttShared& S, const float* q, const float* hcT, float* part,
                                         float* att, float* lg, int b, int step, int tid, bool all_fin = false) {
  constexpr int ATT_THREADS = NT;
  constexpr int NKG = NT / 32;              // K-groups of the attention layer: 16 x 24 rows (NT=512) / 8 x 48 (NT=256)
  constexpr int KPG = 384 / NKG;
  const int V = d.V;
  const size_t row0 = (size_t)b * W;
  if (!all_fin) {     // a chunk whose beams are all finished needs no logits (see the caller)
  // E: attention = [h ; context] . W_att   (Dense, no bias, no activation)
  //    thread = (4 output columns, 1 of NKG K-groups of KPG rows); 24 float4 weight loads in flight
  {
    const int d4 = tid & 31, kg = tid >> 5;
    f2 acc[W][2];
#pragma unroll
    for (int w = 0; w < W; ++w) { acc[w][0] = f2{0.f, 0.f}; acc[w][1] = f2{0.f, 0.f}; }
#pragma unroll
    for (int k0 = 0; k0 < KPG; k0 += 24) {
      float4 wv[24];
      const float* wa = d.W_att + (size_t)(KPG * kg + k0) * RV_U + 4 * d4;
#pragma unroll
      for (int u = 0; u < 24; ++u) wv[u] = *reinterpret_cast<const float4*>(wa + (size_t)u * RV_U);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 24; ++u) {
        float hv[WB];
        *reinterpret_cast<float4*>(hv) = *reinterpret_cast<const float4*>(&hcT[(KPG * kg + k0 + u) * WB]);
        if (W > 4) *reinterpret_cast<float4*>(hv + 4) = *reinterpret_cast<const float4*>(&hcT[(KPG * kg + k0 + u) * WB + 4]);
#pragma unroll
        for (int w = 0; w < W; ++w) {
          acc[w][0] = __builtin_elementwise_fma(f2{hv[w], hv[w]}, f2{wv[u].x, wv[u].y}, acc[w][0]);
          acc[w][1] = __builtin_elementwise_fma(f2{hv[w], hv[w]}, f2{wv[u].z, wv[u].w}, acc[w][1]);
        }
      }
    }
#pragma unroll
    for (int w = 0; w < W; ++w)
      *reinterpret_cast<float4*>(&part[(kg * W + w) * RV_U + 4 * d4]) =
          make_float4(acc[w][0].x, acc[w][0].y, acc[w][1].x, acc[w][1].y);
  }
  __syncthreads();
  for (int i = tid; i < W * RV_U; i += ATT_THREADS) {      // fixed-order reduction of the partials
    const int w = i >> 7, col = i & 127;
    float s0 = 0.f;
#pragma unroll
    for (int g = 0; g < NKG; ++g) s0 += part[(g * W + w) * RV_U + col];
    att[i] = s0;
  }
  __syncthreads();
  RV_STAMP(d, step, 5);
  if (d.dbg_stop == 5) return;

  // F: logits = attention . W_fc + b_fc ; one 16-lane row per (beam, token)
  {
    const int sub = tid & 15, o = tid >> 4;         // 32 outputs per pass
    for (int ob = o; ob < W * V; ob += ATT_THREADS / 16) {
      const int w = ob / V, v = ob % V;
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) p = fmaf(att[w * RV_U + 8 * sub + i], S.wfc[(8 * sub + i) * V + v], p);
      p = row16_sum(p) + S.wfc[RV_U * V + v];
      if (sub == 0) {
        lg[w * RV_MAX_VOCAB + v] = p;
        if (d.step_logits) d.step_logits[(((size_t)step * d.B + b) * W + w) * V + v] = p;
      }
    }
  }
  __syncthreads();
  RV_STAMP(d, step, 6);
  if (d.dbg_stop == 6) return;
  }   // !all_fin

  // G: sampler / beam step, wave 0: lane = candidate (beam w, token v), W*V <= 64
  if (tid < 64) {
    const int lane = tid, w = lane / V, v = lane % V;
    const bool cand = lane < W * V;
    const size_t o = ((size_t)step * d.B + b) * W;
    const bool forced = W == 1 && d.forced;      // (a forced decode has one beam: the wider instantiations compile the test away)
    float val = -INFINITY;
    if (d.greedy) {
      if (cand) val = lg[v];
    } else if (cand) {
      float m = lg[w * RV_MAX_VOCAB];
      for (int x = 1; x < V; ++x) m = fmaxf(m, lg[w * RV_MAX_VOCAB + x]);
      float ssum = 0.f;
      for (int x = 0; x < V; ++x) ssum += __expf(lg[w * RV_MAX_VOCAB + x] - m);
      const float lse = __logf(ssum);
      const bool fin = S.fin[w] != 0;
      const float lp = fin ? (v == d.end_token ? 0.f : -FLT_MAX) : (lg[w * RV_MAX_VOCAB + v] - m) - lse;
      val = S.lprob[w] + lp;
    }
    // top-W by repeated wave max; ties -> lowest flat index (tf.math.top_k order)
    bool taken = !cand;
    int my_word = 0, my_par = 0; float my_val = 0.f;
    for (int k = 0; k < W; ++k) {
      const float mx = wave_max_fast(taken ? -INFINITY : val);
      const unsigned long long hit = __ballot(!taken && (val == mx || mx == -INFINITY));
      const int win = __ffsll((long long)hit) - 1;
      const float wval = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(val), win));
      if (lane == win) taken = true;
      if (lane == k) { my_word = win % V; my_par = win / V; my_val = wval; }
    }
    bool nf = false; int nl = 0;
    if (lane < W) {
      if (d.greedy) {
        nf = !forced && (S.fin[0] != 0 || my_word == d.end_token);      // forced decode: every chunk runs all L - 1 steps, nfin stays 0
      } else {
        const bool pf = S.fin[my_par] != 0;
        nf = pf || my_word == d.end_token;
        nl = S.len[my_par] + (pf ? 0 : 1);
      }
    }
    const unsigned long long fmask = __ballot(lane < W && nf);
    if (lane < W) {
      d.step_ids[o + lane] = my_word; d.parent_ids[o + lane] = my_par; d.step_scores[o + lane] = my_val;
      d.tok[row0 + lane] = forced ? d.forced[(size_t)b * d.L + step + 1] : my_word;   // forced: the next label, whatever the argmax was
      d.finished[row0 + lane] = nf;
      if (!d.greedy) { d.log_probs[row0 + lane] = my_val; d.lengths[row0 + lane] = nl; }
      S.parent[lane] = my_par;
    }
    if (lane == 0 && __popcll(fmask) == W) atomicAdd(&d.nfin[step], 1);
  }
  __syncthreads();
  RV_STAMP(d, step, 7);
  if (d.dbg_stop == 7) return;

  // H: next-step state of every stacked cell, gathered by parent beam: layer 0 input = [attention | h_0],
  //    layer k input's own half = h_k, cell states c_k.  The top layer's h / c are already in LDS.
  const int top = d.depth - 1;
  for (int i = tid; i < W * RV_U; i += ATT_THREADS) {
    const int w = i >> 7, e = i & 127, p = S.parent[w];
    d.xh[(row0 + w) * RV_E + e] = att[p * RV_U + e];
    (d.xh + top * d.ls_xh)[(row0 + w) * RV_E + RV_U + e] = q[p * RV_U + e];
    (d.c + top * d.ls_c)[(row0 + w) * RV_U + e] = S.cnew[p * RV_U + e];
    for (int k = 0; k < top; ++k) {
      (d.xh + k * d.ls_xh)[(row0 + w) * RV_E + RV_U + e] = (d.h_new + k * d.ls_c)[(row0 + p) * RV_U + e];
      (d.c + k * d.ls_c)[(row0 + w) * RV_U + e] = (d.c_new + k * d.ls_c)[(row0 + p) * RV_U + e];
    }
  }
}

// =====================================================================================
// Two-pass attend (exact reference dataflow: scores from keys, then context from values).
// Used for Bahdanau attention and whenever per-step alignments are tapped.
// TB / TD: compile-time trip counts of the score / context sweeps (T_m <= 32*TB and <= 8*TD), so every
// load of a sweep is issued before its first use.
template <int W, int TB, int TD>
__global__ __launch_bounds__(ATT_THREADS) void k_dec_attend(DecState d, int step) {
  extern __shared__ __align__(16) float dsm[];
  const int Tm = d.Tm;
  const int TmP = (Tm + 3) & ~3;
  const AttLds L(W, TmP, false);
  float* q = dsm + L.q;        // [W][128]
  float* pq = dsm + L.pq;      // [W][128]
  float* sc = dsm + L.sc;      // [W][TmP]
  float* al = dsm + L.al;      // [TmP][WB]
  float* part = dsm + L.part;
  float* hcT = dsm + L.hcT;    // [384][WB]
  float* att = dsm + L.att;    // [W][128]
  float* lg = dsm + L.lg;      // [WB][8]
  __shared__ AttShared S;

  const int b = blockIdx.x, tid = threadIdx.x;
  if (step > 0 && d.nfin[step - 1] >= d.B) {      // whole batch finished earlier: propagate
    if (tid == 0 && !d.moves_only) atomicAdd(&d.nfin[step], 1);      // (moves_only: the step's own attend, launched next, counts)
    return;
  }
  const size_t row0 = (size_t)b * W;
  att_prologue<W, 512>(d, S, q, hcT, row0, tid);
  __syncthreads();
  if (d.attention == 1) {   // Bahdanau: processed query = q . W_q ; thread = (column, K quarter)
    const int jj = tid & 127, kq = tid >> 7;
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0.f;
    for (int k = kq * 32; k < kq * 32 + 32; ++k) {
      const float wq = d.W_q[k * RV_U + jj];
#pragma unroll
      for (int w = 0; w < W; ++w) acc[w] = fmaf(q[w * RV_U + k], wq, acc[w]);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) part[(kq * W + w) * RV_U + jj] = acc[w];
    __syncthreads();
    if (tid < RV_U)
#pragma unroll
      for (int w = 0; w < W; ++w)
        pq[w * RV_U + tid] = (part[(0 * W + w) * RV_U + tid] + part[(1 * W + w) * RV_U + tid]) +
                             (part[(2 * W + w) * RV_U + tid] + part[(3 * W + w) * RV_U + tid]);
    __syncthreads();
  }

  // ---- B: scores.  A DPP row (16 lanes) shares one memory step; all key loads in flight first.
  {
    const int sub = tid & 15, grp = tid >> 4;
    float qr[W][8], vr[8];
    const float* qsrc = d.attention == 1 ? pq : q;
#pragma unroll
    for (int w = 0; w < W; ++w)
#pragma unroll
      for (int i = 0; i < 8; ++i) qr[w][i] = qsrc[w * RV_U + 8 * sub + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) vr[i] = d.attention == 1 ? d.v_att[8 * sub + i] : 0.f;
    const float* kbase = d.keys + (size_t)b * Tm * RV_U + 8 * sub;
    const uint8_t* mrow = d.mask + (size_t)b * Tm;
    float4 k0[TB], k1[TB];
    uint8_t mk[TB];
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      const int t = min(grp + 32 * u, Tm - 1);
      const float4* kp = reinterpret_cast<const float4*>(kbase + (size_t)t * RV_U);
      k0[u] = kp[0]; k1[u] = kp[1];
      mk[u] = mrow[t];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      const int t = grp + 32 * u;
      const float kk[8] = {k0[u].x, k0[u].y, k0[u].z, k0[u].w, k1[u].x, k1[u].y, k1[u].z, k1[u].w};
      float mine = 0.f;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        float p = 0.f;
        if (d.attention == 1) {
#pragma unroll
          for (int i = 0; i < 8; ++i) p = fmaf(vr[i], tanhf(kk[i] + qr[w][i]), p);
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) p = fmaf(kk[i], qr[w][i], p);
        }
        p = row16_sum(p);
        mine = sub == w ? p : mine;
      }
      if (t < Tm && sub < W) sc[sub * TmP + t] = mk[u] ? mine : -INFINITY;   // _maybe_mask_score
    }
  }

  // ---- D (loads): every value row this thread needs, issued before the softmax so the memory
  //         latency hides under phase C.  thread = (4 columns, 1 of 8 interleaved t-groups)
  const int cg = tid & 63, tg = tid >> 6;
  float4 vv[TD];
  {
    const float* vbase = d.values + (size_t)b * Tm * RV_E + 4 * cg;
#pragma unroll
    for (int u = 0; u < TD; ++u) {
      const int t = min(tg + 8 * u, Tm - 1);
      vv[u] = *reinterpret_cast<const float4*>(vbase + (size_t)t * RV_E);
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();

  // ---- C: softmax over T_m, one wave per beam
  {
    const int lane = tid & 63, wv = tid >> 6;
    if (wv < W) {
      const int w = wv;
      float m = -INFINITY;
      for (int t = lane; t < Tm; t += 64) m = fmaxf(m, sc[w * TmP + t]);
      m = wave_max(m);
      float sum = 0.f;
      for (int t = lane; t < Tm; t += 64) {
        const float e = expf(sc[w * TmP + t] - m);
        sc[w * TmP + t] = e;
        sum += e;
      }
      sum = wave_sum(sum);
      MoveAcc mv = move_zero();
      for (int t = lane; t < Tm; t += 64) {
        const float a = sc[w * TmP + t] / sum;
        al[t * WB + w] = a;
        if (d.step_align) d.step_align[(((size_t)step * d.B + b) * W + w) * Tm + t] = a;
        if (d.step_moves) move_add(mv, a, t, d.Tr);
      }
      if (d.step_moves) move_wave_store(d.step_moves + (((size_t)step * d.B + b) * W + w) * RV_MOVE_COLS, mv, lane);   // moves: this wave owns the beam
    }
  }
  if (d.moves_only) return;      // (uniform) a moves call beside the single-pass attend: the records were all this launch is for
  __syncthreads();

  // ---- D (math): context = sum_t alpha_t * values_t
  {
    f2 acc[W][2];
#pragma unroll
    for (int w = 0; w < W; ++w) { acc[w][0] = f2{0.f, 0.f}; acc[w][1] = f2{0.f, 0.f}; }
#pragma unroll
    for (int u = 0; u < TD; ++u) {
      const int t = tg + 8 * u;
      if (t < Tm) {
        float a[WB];
        *reinterpret_cast<float4*>(a) = *reinterpret_cast<const float4*>(&al[t * WB]);
        if (W > 4) *reinterpret_cast<float4*>(a + 4) = *reinterpret_cast<const float4*>(&al[t * WB + 4]);
#pragma unroll
        for (int w = 0; w < W; ++w) {
          acc[w][0] = __builtin_elementwise_fma(f2{a[w], a[w]}, f2{vv[u].x, vv[u].y}, acc[w][0]);
          acc[w][1] = __builtin_elementwise_fma(f2{a[w], a[w]}, f2{vv[u].z, vv[u].w}, acc[w][1]);
        }
      }
    }
#pragma unroll
    for (int w = 0; w < W; ++w)
      *reinterpret_cast<float4*>(&part[((tg * W + w) * RV_E) + 4 * cg]) =
          make_float4(acc[w][0].x, acc[w][0].y, acc[w][1].x, acc[w][1].y);
  }
  __syncthreads();
  for (int i = tid; i < W * RV_E; i += ATT_THREADS) {     // fixed-order reduction of the 8 partials
    const int w = i >> 8, col = i & 255;
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) s += part[(g * W + w) * RV_E + col];
    hcT[(RV_U + col) * WB + w] = s;
  }
  __syncthreads();
  att_tail<W, 512>(d, S, q, hcT, part, att, lg, b, step, tid);
}

// =====================================================================================
// Single-pass ("flash") attend for Luong attention -- the production path.
// The per-step attention is HBM-bound: keys [T_m,128] + values [T_m,256] per chunk are re-read every
// step (130 MB per step at B = 256).  Luong's score is linear in the keys, and keys = values . W_mem,
// so   score_t = q . (values_t . W_mem) = values_t . q'   with  q' = W_mem . q   (256-vector).
// One sweep over `values` then yields scores AND context (online softmax), and `keys` is never read:
// a third fewer bytes.  fp32 re-association only (|delta score| ~ 1e-6; tolerance 1e-4).
// 32 independent streams per chunk (a DPP row of 16 lanes each, 16 columns per lane) walk
// t = stream, stream+32, ... with a 3-deep register prefetch, keep their own running
// (max, sum, context[W][256]) and are merged once at the end in a fixed order.
// q' carries log2(e) so the exponentials are bare v_exp_f32.
// NT = 512: 32 streams, one workgroup per CU (slabs up to the CU count).  NT = 256: 16 streams, 71 KB of LDS
// and 196 VGPRs -> TWO workgroups per CU, so one chunk's latency-bound phases (cell-output fetch, q',
// attention layer, beam step) run under the other chunk's HBM-bound sweep (slabs larger than the CU count).
template <int W, int NT>
__global__ __launch_bounds__(NT) void k_dec_attend_flash(DecState d, const float* __restrict__ WmemT, int step) {
  constexpr int ATT_THREADS = NT, NW = NT / 64, NS = NT / 16;
  extern __shared__ __align__(16) float dsm[];
  const int Tm = d.Tm;
  const AttLds L(W, 0, true, NT);
  float* q = dsm + L.q;        // [W][128]
  float* qp = dsm + L.pq;      // [W][256]  q' * log2(e)
  float* ml = dsm + L.sc;      // [32][WB][2] per-stream (max, sum)
  float* mg = dsm + L.al;      // [WB][2] merged (max, 1/sum)
  float* part = dsm + L.part;  // [8][W][256]
  float* hcT = dsm + L.hcT;    // [384][WB]
  float* att = dsm + L.att;    // [W][128]
  float* lg = dsm + L.lg;      // [WB][8]
  float* fold = dsm + L.fold;
  __shared__ AttShared S;

  const int b = blockIdx.x, tid = threadIdx.x;
  if (step > 0 && d.nfin[step - 1] >= d.B) {
    if (tid == 0) atomicAdd(&d.nfin[step], 1);
    return;
  }
  const size_t row0 = (size_t)b * W;
  RV_STAMP(d, step, 0);
  const int lane = tid & 63, wv = tid >> 6, sub = lane & 15, sid = tid >> 4;   // sid: stream 0..NS-1
  constexpr int PD = 3;                                                       // prefetch depth (iterations)
  const float* vbase = d.values + (size_t)b * Tm * RV_E + 4 * sub;
  const uint8_t* mrow = d.mask + (size_t)b * Tm;
  const int nit = (Tm + NS - 1) / NS;
  float4 pv[PD][4];
  uint8_t pm[PD];
  auto issue = [&](int slot, int it) {
    const int t = min(sid + NS * it, Tm - 1);
    const float* p = vbase + (size_t)t * RV_E;
#pragma unroll
    for (int m = 0; m < 4; ++m) pv[slot][m] = *reinterpret_cast<const float4*>(p + 64 * m);
    pm[slot] = mrow[t];
  };
  // small loads first, INTO REGISTERS (vmcnt retires in issue order), then the stream, then the LDS
  // writes: the prologue waits one short round trip while the value rows are already in flight.
  constexpr int NC = (W * RV_U + ATT_THREADS - 1) / ATT_THREADS;
  constexpr int NWF = (RV_U * RV_MAX_VOCAB + ATT_THREADS - 1) / ATT_THREADS;   // W_fc staging slots per thread
  float hr[NC], cr[NC], wfr[NWF];
  int sm0 = 0, sm2 = 0; float sm1 = 0.f;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int idx = tid + ATT_THREADS * i;
    hr[i] = idx < W * RV_U ? (d.h_new + (d.depth - 1) * d.ls_c)[row0 * RV_U + idx] : 0.f;
    cr[i] = idx < W * RV_U ? (d.c_new + (d.depth - 1) * d.ls_c)[row0 * RV_U + idx] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < NWF; ++i) { const int idx = tid + ATT_THREADS * i; wfr[i] = idx < RV_U * d.V ? d.W_fc[idx] : 0.f; }
  const float bfr = tid < d.V ? d.b_fc[tid] : 0.f;
  if (tid < W) { sm0 = d.finished[row0 + tid]; sm1 = d.log_probs[row0 + tid]; sm2 = d.lengths[row0 + tid]; }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < PD; ++k) issue(k, k);            // the stream starts before any math
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int idx = tid + ATT_THREADS * i;
    if (idx < W * RV_U) { q[idx] = hr[i]; hcT[(idx & 127) * WB + (idx >> 7)] = hr[i]; S.cnew[idx] = cr[i]; }
  }
#pragma unroll
  for (int i = 0; i < NWF; ++i) { const int idx = tid + ATT_THREADS * i; if (idx < RV_U * d.V) S.wfc[idx] = wfr[i]; }
  if (tid < d.V) S.wfc[RV_U * d.V + tid] = bfr;
  if (tid < W) { S.fin[tid] = sm0; S.lprob[tid] = sm1; S.len[tid] = sm2; }
  __syncthreads();
  RV_STAMP(d, step, 1);
  // A chunk whose W beams are ALL finished contributes only (beam, end-token) candidates at unchanged
  // scores (finished rows are replaced by [min.., 0 at '^']): its logits are never read,
  // so the cell output, attention and output layer are skipped and only the beam bookkeeping runs.  The
  // states written for such a chunk are never used for an output again.  (Not under debug taps, which
  // record logits of finished beams, and not for greedy decoding, whose rows keep sampling.)
  bool all_fin = !d.greedy && !d.step_logits && !d.step_align;
  for (int w = 0; w < W; ++w) all_fin = all_fin && S.fin[w] != 0;
  if (all_fin) {
    att_tail<W, NT>(d, S, q, hcT, part, att, lg, b, step, tid, true);
    return;
  }
  // q' = W_mem . q (times log2 e): thread = (4 columns, 1 of NW j-groups), W_memT is [128][256]
  {
    constexpr int JPG = RV_U / NW;                      // rows of W_memT per j-group (16 or 32)
    const int c4 = tid & 63, jg = tid >> 6;
    f2 acc[W][2];
#pragma unroll
    for (int w = 0; w < W; ++w) { acc[w][0] = f2{0.f, 0.f}; acc[w][1] = f2{0.f, 0.f}; }
#pragma unroll
    for (int j0 = 0; j0 < JPG; j0 += 16) {
      float4 wm[16];
      const float* wp = WmemT + (size_t)(JPG * jg + j0) * RV_E + 4 * c4;
#pragma unroll
      for (int u = 0; u < 16; ++u) wm[u] = *reinterpret_cast<const float4*>(wp + (size_t)u * RV_E);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        float hv[WB];
        *reinterpret_cast<float4*>(hv) = *reinterpret_cast<const float4*>(&hcT[(JPG * jg + j0 + u) * WB]);
        if (W > 4) *reinterpret_cast<float4*>(hv + 4) = *reinterpret_cast<const float4*>(&hcT[(JPG * jg + j0 + u) * WB + 4]);
#pragma unroll
        for (int w = 0; w < W; ++w) {
          acc[w][0] = __builtin_elementwise_fma(f2{hv[w], hv[w]}, f2{wm[u].x, wm[u].y}, acc[w][0]);
          acc[w][1] = __builtin_elementwise_fma(f2{hv[w], hv[w]}, f2{wm[u].z, wm[u].w}, acc[w][1]);
        }
      }
    }
#pragma unroll
    for (int w = 0; w < W; ++w)
      *reinterpret_cast<float4*>(&part[(jg * W + w) * RV_E + 4 * c4]) =
          make_float4(acc[w][0].x, acc[w][0].y, acc[w][1].x, acc[w][1].y);
  }
  __syncthreads();
  for (int i = tid; i < W * RV_E; i += ATT_THREADS) {
    const int w = i >> 8, col = i & 255;
    float s0 = 0.f;
#pragma unroll
    for (int g = 0; g < NW; ++g) s0 += part[(g * W + w) * RV_E + col];
    qp[i] = s0 * LOG2E;
  }
  __syncthreads();

  RV_STAMP(d, step, 2);
  // ---- the sweep.  Lane (sub) owns columns {4 sub + 64 m + 0..3 : m = 0..3} of its stream's rows.
  // Beam w's running (max, sum) of a stream lives in lane sub == w of its row; the rescale factor and
  // the new weight reach the other lanes through DPP row_newbcast.
  float M = -INFINITY, l = 0.f;
  f2 acc[W][8];
#pragma unroll
  for (int w = 0; w < W; ++w)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[w][i] = f2{0.f, 0.f};
  for (int it0 = 0; it0 < nit; it0 += PD) {
#pragma unroll
    for (int k = 0; k < PD; ++k) {
      const int it = it0 + k;
      if (it < nit) {                                   // wave-uniform
        asm volatile("" ::: "memory");                  // keep the q' LDS reads inside the loop (LICM would
                                                        // pin 16*W registers and spill; spill traffic drains vmcnt)
        const int t = sid + NS * it;
        const bool live = t < Tm && pm[k] != 0;
        f2 v[8];
#pragma unroll
        for (int m = 0; m < 4; ++m) { v[2 * m] = f2{pv[k][m].x, pv[k][m].y}; v[2 * m + 1] = f2{pv[k][m].z, pv[k][m].w}; }
        if (it + PD < nit) issue(k, it + PD);           // refill this slot (registers already copied)
        float mys = -INFINITY;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          f2 pp = f2{0.f, 0.f};
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const float4 qv = *reinterpret_cast<const float4*>(&qp[w * RV_E + 4 * sub + 64 * m]);
            pp = __builtin_elementwise_fma(v[2 * m], f2{qv.x, qv.y}, pp);
            pp = __builtin_elementwise_fma(v[2 * m + 1], f2{qv.z, qv.w}, pp);
          }
          const float sw = row16_sum(pp.x + pp.y);      // log2-domain score, uniform across the row
          mys = sub == w ? sw : mys;
        }
        if (d.step_align && sub < W && t < Tm)          // tap: raw masked score (host normalises)
          d.step_align[(((size_t)step * d.B + b) * W + sub) * Tm + t] = live ? mys : -INFINITY;
        mys = live ? mys : -INFINITY;                   // _maybe_mask_score
        const float Mn = fmaxf(M, mys);
        const float mref = Mn == -INFINITY ? 0.f : Mn;
        const float scl = exp2f(M - mref), pe = exp2f(mys - mref);
        l = fmaf(l, scl, pe);
        M = Mn;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          const float sc_w = row_bcast(scl, w), pe_w = row_bcast(pe, w);
#pragma unroll
          for (int i = 0; i < 8; ++i)
            acc[w][i] = __builtin_elementwise_fma(acc[w][i], f2{sc_w, sc_w}, f2{pe_w, pe_w} * v[i]);
        }
      }
    }
  }
  RV_STAMP(d, step, 3);
  // ---- merge the NS streams: global max / sum per beam, then a fixed-order sum of rescaled contexts
  if (sub < W) { ml[(sid * WB + sub) * 2] = M; ml[(sid * WB + sub) * 2 + 1] = l; }
  __syncthreads();
  for (int w = wv; w < W; w += NW) {     // a wave merges beam w: lane = stream
    const float Ms = lane < NS ? ml[(lane * WB + w) * 2] : -INFINITY;
    const float ls = lane < NS ? ml[(lane * WB + w) * 2 + 1] : 0.f;
    const float Mg = wave_max_fast(Ms);
    const float lsum = wave_sum_fast(Ms == -INFINITY ? 0.f : ls * exp2f(Ms - Mg));
    if (lane == 0) {
      mg[w * 2] = Mg;
      mg[w * 2 + 1] = 1.0f / lsum;       // all-masked chunk: 1/0 -> inf, context NaN like the reference's softmax
    }
  }
  __syncthreads();
  {
    const float Mg = sub < W ? mg[sub * 2] : 0.f;
    const float fs = M == -INFINITY ? 0.f : exp2f(M - Mg);          // this stream's weight for beam `sub`
    // fold the wave's 4 streams (its 4 DPP rows hold the same columns) through a wave-private 16-lane LDS
    // slab: row 3 -> row 1, row 2 -> row 0, row 1 -> row 0.  Same-wave exchange: no workgroup barrier.
    constexpr int SL = NT == 512 ? 32 : 16;             // slab lanes: 2-step fold where LDS allows, else 3-step
    float4* slab = reinterpret_cast<float4*>(fold + (size_t)wv * (W * 4 * SL * 4));
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const float f = row_bcast(fs, w);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[w][i] = acc[w][i] * f2{f, f};
    }
    const int row = lane >> 4;
    // both schedules add (row0 + row2) + (row1 + row3): identical results
    constexpr int NSTEP = NT == 512 ? 2 : 3;
#pragma unroll
    for (int stepf = 0; stepf < NSTEP; ++stepf) {
      bool is_src, is_dst; int sl;
      if (NT == 512) {       // rows {2,3} -> {0,1}, then row 1 -> row 0
        is_src = stepf == 0 ? lane >= 32 : row == 1;
        is_dst = stepf == 0 ? lane < 32 : row == 0;
        sl = stepf == 0 ? (lane & 31) : sub;
      } else {               // row 3 -> 1, row 2 -> 0, row 1 -> 0
        const int src = stepf == 0 ? 3 : (stepf == 1 ? 2 : 1), dst = stepf == 0 ? 1 : 0;
        is_src = row == src; is_dst = row == dst; sl = sub;
      }
      if (is_src) {
#pragma unroll
        for (int w = 0; w < W; ++w)
#pragma unroll
          for (int m = 0; m < 4; ++m)
            slab[(w * 4 + m) * SL + sl] = make_float4(acc[w][2 * m].x, acc[w][2 * m].y, acc[w][2 * m + 1].x, acc[w][2 * m + 1].y);
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);               // lgkmcnt(0): the wave's LDS writes have landed
      if (is_dst) {
#pragma unroll
        for (int w = 0; w < W; ++w)
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const float4 o = slab[(w * 4 + m) * SL + sl];
            acc[w][2 * m] += f2{o.x, o.y}; acc[w][2 * m + 1] += f2{o.z, o.w};
          }
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);
    }
    if (row == 0) {
#pragma unroll
      for (int w = 0; w < W; ++w)
#pragma unroll
        for (int m = 0; m < 4; ++m)
          *reinterpret_cast<float4*>(&part[(wv * W + w) * RV_E + 4 * sub + 64 * m]) =
              make_float4(acc[w][2 * m].x, acc[w][2 * m].y, acc[w][2 * m + 1].x, acc[w][2 * m + 1].y);
    }
  }
  __syncthreads();
  for (int i = tid; i < W * RV_E; i += ATT_THREADS) {     // fixed-order reduction over the waves
    const int w = i >> 8, col = i & 255;
    float s0 = 0.f;
#pragma unroll
    for (int g = 0; g < NW; ++g) s0 += part[(g * W + w) * RV_E + col];
    hcT[(RV_U + col) * WB + w] = s0 * mg[w * 2 + 1];
  }
  __syncthreads();
  RV_STAMP(d, step, 4);
  att_tail<W, NT>(d, S, q, hcT, part, att, lg, b, step, tid);
  RV_STAMP(d, step, 8);
}

// =====================================================================================
// Persistent decode: the WHOLE beam-search loop of one chunk in one workgroup, with the chunk's
// attention memory resident ON CHIP.
// The per-step attention is HBM-bound when `values` [T_m,256] fp32 (338 KB per chunk at T_m = 330)
// is re-streamed every step (k_dec_attend_flash: 86.6 MB per step at B = 256).  A CU's register file
// is 512 KB: thread (stream sid = tid>>4, sub = tid&15) loads rows t = sid + 32 it, columns
// {4 sub + 64 m + 0..3} of its chunk ONCE into NIT*16 VGPRs and keeps them for all L-1 steps.
// Chunks never interact inside the decode loop (the reference's loop only shares its stop test,
// "until every row of the slab is finished"): each workgroup runs until ITS beams are finished and
// records that step; k_dec_finalize extends earlier finishers exactly as the shared loop would
// (end token, unchanged score -- SURVEY.md A.5).  No hipGraph, no per-step launches, no HBM stream:
// per step the CU pulls only the weights (cell 512 KB + W_mem 128 KB + W_att 192 KB) from L2.
// Luong attention; beam search with W <= 8 (W <= 5 with two stacked cells: LDS) and greedy search.
// one decoder cell and W <= 5 leave 48 KB of LDS: 24 of the 256 weight rows the cell product streams from L2 every step stay on chip
__host__ __device__ constexpr bool persist_weight_cache(int W, int D) { return D == 1 && W <= 5; }
constexpr int PERSIST_MAX_NIT = 11;      // resident row groups of 32 steps: T_m <= 352
// `part` also holds the matrix-pipe attention's alignment image (two f16 parts of [32 NIT steps][8 beam slots] = NIT * 256 floats):
// with one beam that image is larger than the partial sums, so the block is sized for the larger of the two
__host__ __device__ constexpr int part_floats(int W) { return 4 * W * RV_G > PERSIST_MAX_NIT * 256 ? 4 * W * RV_G : PERSIST_MAX_NIT * 256; }
// ATT == 3 (matrix-pipe cell product): gate pre-activations z~ [W][RV_G + 16] (one plane: the product is complete inside a wave; rows
// padded so that the four beams a wave stores at once fall into different banks).  Weight cache in LDS: ALL 32 (k-step, gate) pairs
// of wave 0 (64 KB) -- wave 0 takes the output layer and the beam step first (4.7 k cycles) and would stream its share alone afterwards --
// and the last mxc_nc(W) pairs of each of the other seven waves (2 KB per pair and wave); the output layer's fragments (Wl16, 16 KB) sit in
// LDS as well.  This form needs neither `qp` / `att` (fp32 copies of h and ctx') nor `attT` / `hcT` nor the fp32 output layer in static LDS
__host__ __device__ constexpr int mxc_nc(int W) { return W <= 5 ? 2 : 1; }
// static LDS (bytes, an upper bound) of a form: ~1 KB with the cell product on the matrix pipe (bias, beam bookkeeping), ~8.7 KB of output
// layer in the others.  A form runs only where its dynamic LDS fits beside it (dec_persist_form) and opts in to no more than that
constexpr int persist_static_lds(int ATT) { return ATT >= 3 ? 1024 : 10 * 1024; }
__host__ __device__ constexpr int mxc_cache_floats(int W) { return (32 + 7 * mxc_nc(W)) * 512; }
// One-part forms (k_dec_persist_1p, option weight_parts 1): a fragment is 1 KB, so wave 0's copy is 32 KB and the output layer 8 KB.  The
// 40 KB that frees goes to the other waves' on-chip fragments: mxc_nc1(W) per wave in the space the two-part form gives mxc_nc(W) pairs
// plus what was freed -- the form's dynamic LDS is never more than its two-part counterpart's
__host__ __device__ constexpr int mxc_nc1(int W) { return W <= 5 ? 8 : 6; }
__host__ __device__ constexpr int mxc_cache_floats_1p(int W) { return (32 + 7 * mxc_nc1(W)) * 256; }
// two decoder cells on the matrix pipe: per step and wave 48 pairs of cell 0's product ([ctx' | h_1 | h_0] . [W_a ; A_h W_a ; U_0], K = 384) and
// 16 of cell 1's recurrent product (h_1 . U_1) at the end of the step, 16 of cell 1's input product (h_0 . W_1) after cell 0's gates.  The
// LDS that is left (W <= 5) keeps the first MXC2_CACHE of wave 0's 64 end-of-step pairs: wave 0 joins that stream 4.7 k cycles late
constexpr int MXC2_CACHE = 32;
constexpr int MXC_ZS = RV_G + 16;
__host__ __device__ constexpr int part_floats_mxc(int W) { return W * MXC_ZS > PERSIST_MAX_NIT * 256 ? W * MXC_ZS : PERSIST_MAX_NIT * 256; }
struct PersistLds {
  int attT, zb, cS, qp, part, ctxp, hcT, att, ml, mg, lg, fold, h0T, cS1, b1s, pq, vat, xim, wl16, wcache, total;
  // ATT: 0 Luong on fp32 rows, 1 Bahdanau, 2 Luong on the matrix pipe, 3 = 2 + the cell product on the matrix pipe,
  // 4 = Bahdanau scores on the VALU (fp32 key rows) with context, cell product and output layer on the matrix pipe as in 3
  // P: f16 parts per weight of the cell kernel's and the output layer's fragments (1: k_dec_persist_1p, one cell on the matrix pipe)
  __host__ __device__ PersistLds(int W, int D = 1, int ATT = 0, int P = 2) {
    const bool mxc = ATT == 3 || ATT == 4;
    int o = 0;
    attT = o; if (!mxc) o += RV_U * WB;   // attention vectors k-major beam-minor (cell input rows 0..127); mxc: the f16 image `xim` instead
    zb = o; o += RV_MAX_VOCAB * RV_G;  // one-hot token rows of the cell kernel + bias: [V][512]
    cS = o; o += 2 * W * RV_U;         // cell states, double-buffered: the new state of beam w comes from its parent's
    qp = o; if (!mxc) o += W * RV_U;   // h * log2(e): the score query (fp32 rows) and the output layer's h part
    part = o; o += mxc ? part_floats_mxc(W) : part_floats(W);     // cell-product partial sums [4][W][512] (end of step -> gates), then the attention
                                       // layer's h-part partial sums [16][W][128] (after the gates -> merge)
    ctxp = part;                       // context partial sums of the 8 waves [8][W][128]: one cell -> inside `part` (idle between
    if (D > 1 && !mxc) { ctxp = o; o += 8 * W * RV_U; }   // the gates and the end of the step); two cells -> own space (`part` holds h . A_h then)
    if (D > 1 && mxc) { ctxp = o; o += W * MXC_ZS; }      // two cells on the matrix pipe: h_1 . U_1 of the beams, [W][RV_G + 16] (`partU`)
    fold = o; o += mxc ? 1024 : 8 * 4 * 2 * 16 * 4;   // (mxc: only the query image, 2 parts x 1024 f16)   wave-private fold slab: 4 streams x 2 float4 x 16 lanes.  ctxp + fold also hold the
                                       // second cell's recurrent partial sums [3][W][512] between the end of a step and its gates
    hcT = o; if (!mxc) o += RV_U * WB;  // h of the top cell, k-major beam-minor (cell input rows 128..255, attention-layer input)
    att = o; if (!mxc) o += W * RV_U;
    ml = o; o += 64 * WB;              // per-stream max [32][WB], per-stream sum [32][WB]
    mg = o; o += 2 * WB;               // merged max, 1/sum
    lg = o; o += WB * RV_MAX_VOCAB;
    h0T = o; cS1 = o; b1s = o;
    if (D > 1) {                       // StackedRNNCells, second cell (basecaller.py:85-91)
      h0T = o; if (!mxc) o += RV_U * WB;   // h of cell 0, k-major beam-minor (input of cell 1 and rows 128..255 of cell 0's product); mxc: in `xim`
      cS1 = o; o += 2 * W * RV_U;
      b1s = o; o += RV_G;
    }
    pq = o; vat = o;
    if (ATT == 1 || ATT == 4) {        // Bahdanau (basecaller.py:131-132): processed query (h . W_q) per beam, and attention_v
      pq = o; o += W * RV_U;
      vat = o; o += RV_U;
    }
    xim = o;
    if (mxc) o += D > 1 ? 3072 : 2048; // [ctx' | h] ([ctx' | h_1 | h_0] with two cells) of the beams as MFMA A fragments: [32 | 48 k-blocks][16 rows][8] f16
    wl16 = o;
    if (mxc) o += P == 1 ? 2048 : 4096;   // the output layer [W_fc ; A_h W_fc] as B fragments (DecState::Wl16, 16 KB): wave 0's logits
    wcache = o;
    if (mxc) o += D > 1 ? MXC2_CACHE * 512 : (P == 1 ? mxc_cache_floats_1p(W) : mxc_cache_floats(W));
    else if (persist_weight_cache(W, D)) o += 24 * RV_G;   // 24 rows of the cell kernel kept in LDS (48 KB): the last 8 rows of K groups 1-3
    total = o;
  }
};

// The decoder cells' tanh is rv_tanh, relatively accurate (a large recurrent gain multiplies an absolute error step after step).  One
// exception: the g gate of the non-default form with the Luong scores and context on the matrix pipe and the cell product on packed
// FMAs (ATT 2) keeps 2 sigmoid(2x) - 1 -- rv_tanh at both of that form's sites raises the scratch of k_dec_persist<5,11,1,2> from 20 to
// 36 B per lane, over its bound in tests/test_build.py; at either one alone it stays at 20.  The cell-state site is the one that
// holds an adversarial recurrent kernel closer to fp64, and that form is held to 1e-4 only (tests/test_bench_config_gpu.py, DESIGN.md
// section 5)
template <int ATT>
__device__ __forceinline__ float dec_gate_tanh(float x) {
  if constexpr (ATT == 2) return rv_tanh_abs(x);
  else return rv_tanh(x);
}

// Tap (option persist_taps) of a matrix-pipe form's alignments: what the context product consumes, (hi + lo) 2^-14 read back from its
// A image [k-block t / 8][row mx_row(beam) (+ 1: low part)][t % 8] in `part` (after the barrier that completes the image; a loop of its
// own, away from the resident fragments' registers).  d.persist_align [L-1][B][W][T_m], steps t < T_m only.
// The loop's shape is picked per form by what keeps each kernel within its scratch bound (tests/test_build.py): one flat loop over
// (beam, step) for Bahdanau (ATT 4), a rolled loop over the beams for the Luong forms (ATT 2, 3)
template <int W, bool FLAT>
__device__ __forceinline__ void tap_align_image(const DecState& d, const float* part, int b, int step, int tid) {
  const _Float16* aa = reinterpret_cast<const _Float16*>(part);
  float* out = d.persist_align + ((size_t)step * d.B + b) * W * d.Tm;
  int t0 = tid;
  asm volatile("" : "+v"(t0));     // nothing of this loop is hoisted out of the step loop (no registers held while taps are off)
  if constexpr (FLAT) {
    for (int i = t0; i < W * d.Tm; i += 512) {
      const int w = i / d.Tm, t = i - w * d.Tm;
      const _Float16* q = aa + ((t >> 3) * 16 + mx_row(w)) * 8 + (t & 7);
      out[i] = ((float)q[0] + (float)q[8]) * (1.0f / 16384.f);
    }
  } else {
#pragma unroll 1
    for (int w = 0; w < W; ++w)
      for (int t = t0; t < d.Tm; t += 512) {
        const _Float16* q = aa + ((t >> 3) * 16 + mx_row(w)) * 8 + (t & 7);
        out[(unsigned)(w * d.Tm + t)] = ((float)q[0] + (float)q[8]) * (1.0f / 16384.f);
      }
  }
}

// The moves arguments of the call as the step loop reads them: from the LDS words the prologue left (k_dec_persist: s_moves), brought
// into scalar registers for the length of the block that uses them
__device__ __forceinline__ float* persist_moves_arg(float* const& s_moves, const int& s_Tr, int& Tr) {
  const uint2 v = *reinterpret_cast<const uint2*>(&s_moves);
  Tr = __builtin_amdgcn_readfirstlane(s_Tr);
  const uint64_t a = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(v.y) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane(v.x);
  return reinterpret_cast<float*>(a);
}

// Moves (DecState::step_moves) of a matrix-pipe form: the same read-back of the A image as the tap above, reduced instead of stored.
// Wave w < W owns beam w and walks its T_m steps, lane l those with t % 64 == l; nothing but the six floats per beam leaves the chip.
// These kernels hold 255 of 256 VGPRs through the step loop, so the record is not kept in six accumulators: one rolled pass over the
// image per column -- the peak first (it says whether the row is NaN), then the four sums -- each with a handful of registers live
// The shape is picked per form by what the register allocator makes of it, like the tap's: the forms reduce across the wave by DPP and
// readlane (FAST), except Bahdanau (ATT 4) at beam 5, which by shuffles alone stays within its scratch bound (tests/test_build.py: 188 B
// against 200).  At its other beams the shuffles cost that form up to 96 B more scratch than it had and 3.5 % of a call without moves
// (beam 7); with FAST every instantiation but <3,8,1,4> (32 -> 56 B) spills no more than before the moves
template <int W, int NIT, bool FAST>
__device__ __forceinline__ void moves_from_image(const DecState& d, float* moves, int Tr, const float* part, int b, int step, int tid) {
  auto wmax = [](float v) { if constexpr (FAST) return wave_max_fast(v); else return wave_max(v); };
  auto wsum = [](float v) { if constexpr (FAST) return wave_sum_fast(v); else return wave_sum(v); };
  const _Float16* aa = reinterpret_cast<const _Float16*>(part);
  int t0 = tid;
  asm volatile("" : "+v"(t0));     // nothing of this is hoisted out of the step loop (no registers held while the pointer is null)
  const int lane = t0 & 63, w = __builtin_amdgcn_readfirstlane(t0 >> 6);      // (the wave's number, in a scalar register)
  if (w >= W) return;
  float* rec = moves + (((size_t)step * d.B + b) * W + w) * RV_MOVE_COLS;
  const _Float16* row = aa + mx_row(w) * 8;
  // The image holds 32 NIT steps: those from T_m on are padding and carry exactly 0 (NaN in a NaN row), so every pass walks the
  // whole image -- a trip count the wave shares, no lane leaves a loop early (an exec mask saved per loop is two scalar registers, and
  // the Bahdanau form spills those to memory)
  constexpr int TRIPS = (32 * NIT + 63) / 64;
  auto alpha = [&](int t) {
    const int tc = min(t, 32 * NIT - 1);
    const _Float16* q = row + (tc >> 3) * 128 + (tc & 7);
    return ((float)q[0] + (float)q[8]) * (1.0f / 16384.f);
  };
  // the row's maximum (fmaxf drops a NaN: -inf stays for a NaN row), then the first t that holds it (t < 2^24: exact as a float)
  float pk = -INFINITY;
#pragma unroll 1
  for (int i = 0; i < TRIPS; ++i) pk = fmaxf(pk, alpha(lane + 64 * i));
  const float pmax = wmax(pk);
  float nt = -INFINITY;            // minus the lane's first such t
#pragma unroll 1
  for (int i = 0; i < TRIPS; ++i) { const int t = lane + 64 * i; nt = fmaxf(nt, (alpha(t) == pmax && t < 32 * NIT) ? -(float)t : -INFINITY); }
  const float pfirst = pmax == -INFINITY ? -1.0f : -wmax(nt);
  const float z = pmax - pmax;     // NaN for a NaN row (no alignment was greater than -inf), +0 for every other: see move_store
  if (lane == 0) { rec[4] = pmax + z; rec[5] = pfirst; }
  auto segment = [&](int c, int lo, int hi, bool first_moment) {      // steps [lo, hi), weight 1 or t - lo
    float acc = 0.f;
#pragma unroll 1
    for (int i = 0; i < TRIPS; ++i) {
      const int t = lane + 64 * i;
      const float al = (t >= lo && t < hi) ? alpha(t) : 0.f;
      acc = fmaf(al, first_moment ? (float)(t - lo) : 1.0f, acc);
    }
    acc = wsum(acc);
    if (lane == 0) rec[c] = acc + z;
  };
  segment(0, 0, Tr, false); segment(1, 0, Tr, true); segment(2, Tr, d.Tm, false); segment(3, Tr, d.Tm, true);
}

// The default form's own memory projection (option fused_memory; DecState::enc_rows): the chunk's [keys | U'] = enc_out . [W_mem | A_c]
// computed by its decode workgroup straight into the resident fragments, instead of a GEMM launch that writes [B,T_m,256] floats
// which this prologue would read back.  Every element keeps the chain of k_gemm_mem_split3 (gemm_f32.hip): k in eight steps of 32,
// per step w_lo . a_hi, w_hi . a_lo, w_hi . a_hi into one f32 accumulator, a' = 2^14 a, w' from the same host-packed parts, then
// fma(acc, 2^-14 / s_n, +0) -- so the fp32 value that split_f16x8 cuts is the GEMM's, bit for bit.
// No transposition: an MFMA's C/D registers give lane (n, q) rows 4 q + i, both resident layouts give lane (n, kq) 8 consecutive
// indices; a tile's rows are free to choose, so each 32 indices are TWO tiles, X with row 4 q + i <-> index 8 q + i and Y with + 4,
// and a lane's X and Y accumulators are its fragment.
//   U' first.  Its fragments belong to the wave that owns the UNITS, over all of time, but a wave computes what it can feed from
//   its own rows of enc_out: (32-step block, X | Y) unit wv + 8 r against all 8 unit tiles of A_c (the A_c half of Wmp16, 128 KB, in
//   LDS).  The accumulators then cross to the owning waves through LDS, lane to the same lane, in two rounds of (NIT + 1) / 2 blocks
//   (96 KB at most, over the weights that are dead by then).  Every wave reads in both rounds: fragments defined under a per-wave
//   branch made k_dec_persist<5,11,1,3> spill one of them across the whole step loop.
//   Keys second: wave wv owns the 16-step tiles wv + 8 c as in the step loop; the permuted rows are weight columns, a second
//   host-packed image (Wkp16, 128 KB, in LDS).  All of a wave's tiles advance together, so each weight fragment is read once per wave;
//   the accumulators of both phases turn into the resident fragments in place (8 floats -> two f16 parts of 8).
// Rows t >= T_m are clamped to row T_m - 1 and livebits is built as in the GEMM-fed prologue.  d.mem_tap (option persist_taps): the
// fp32 values are also stored where the GEMM would have put them.  Uses the first 128 KB of the dynamic LDS, which the caller
// initialises only afterwards; ends with a barrier.
template <int NIT>
__device__ __forceinline__ void persist_project_memory(const DecState& d, int b, float* dsm, float4 (&kb)[(2 * NIT + 7) / 8][4][2],
                                                       float4 (&ub)[NIT][2], unsigned& livebits) {
  constexpr int NTT = (2 * NIT + 7) / 8;     // a wave's 16-step key tiles, and as many (block, X | Y) units of U'
  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, kq = lane >> 4, Tm = d.Tm;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);      // (uniform: what depends on the wave alone stays on the scalar side)
  const float* enc = d.enc_rows + (size_t)b * Tm * RV_E + 8 * kq;
  const float* css = reinterpret_cast<const float*>(d.Wmp16 + (size_t)2 * RV_E * RV_E);    // 2^-14 / s_n
  uint4* wls = reinterpret_cast<uint4*>(dsm);           // [8 k-steps][8 tiles][2 parts][64 lanes] uint4 (128 KB)
  f4v* xb = reinterpret_cast<f4v*>(dsm);                // exchange: [8 unit tiles][2 HB units of a round][64 lanes] float4
  float* tap = d.mem_tap ? d.mem_tap + (size_t)b * Tm * RV_E : nullptr;
  f4v acc[NTT][8];
  int trow[NTT];
  // one pass over a wave's NTT row tiles: SWAP = false: D = a . w (rows = steps: U'), true: D = w . a (rows = weight columns: keys)
  auto product = [&](auto swap) {
    constexpr bool SWAP = decltype(swap)::value;
#pragma unroll
    for (int r = 0; r < NTT; ++r)
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[r][u] = f4v{0.f, 0.f, 0.f, 0.f};
    float4 nx[NTT][2];
#pragma unroll
    for (int r = 0; r < NTT; ++r) {
      nx[r][0] = *reinterpret_cast<const float4*>(enc + (size_t)trow[r] * RV_E);
      nx[r][1] = *reinterpret_cast<const float4*>(enc + (size_t)trow[r] * RV_E + 4);
    }
#pragma unroll 1
    for (int ks = 0; ks < 8; ++ks) {
      h8 ah[NTT], al[NTT];
#pragma unroll
      for (int r = 0; r < NTT; ++r) {
        const float v[8] = {nx[r][0].x, nx[r][0].y, nx[r][0].z, nx[r][0].w, nx[r][1].x, nx[r][1].y, nx[r][1].z, nx[r][1].w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float sv = v[j] * 16384.f;
          ah[r][j] = (_Float16)sv;
          al[r][j] = (_Float16)(sv - (float)ah[r][j]);
        }
      }
      const int kn = min(ks + 1, 7);         // the next k-step's floats travel under this one's MFMAs (the last step re-reads its own)
#pragma unroll
      for (int r = 0; r < NTT; ++r) {
        nx[r][0] = *reinterpret_cast<const float4*>(enc + (size_t)trow[r] * RV_E + 32 * kn);
        nx[r][1] = *reinterpret_cast<const float4*>(enc + (size_t)trow[r] * RV_E + 32 * kn + 4);
      }
      const uint4* wp = wls + ks * 1024 + lane;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const h8 wh = __builtin_bit_cast(h8, wp[u * 128]), wl = __builtin_bit_cast(h8, wp[u * 128 + 64]);
#pragma unroll
        for (int r = 0; r < NTT; ++r) {
          if constexpr (SWAP) {
            acc[r][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, ah[r], acc[r][u], 0, 0, 0);
            acc[r][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, al[r], acc[r][u], 0, 0, 0);
            acc[r][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, ah[r], acc[r][u], 0, 0, 0);
          } else {
            acc[r][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[r], wl, acc[r][u], 0, 0, 0);
            acc[r][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[r], wh, acc[r][u], 0, 0, 0);
            acc[r][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[r], wh, acc[r][u], 0, 0, 0);
          }
        }
      }
    }
  };

  // ---- U': the A_c tiles (nt = 8..15) of every k-step of the GEMM's image -> LDS
  {
    const uint4* img = reinterpret_cast<const uint4*>(d.Wmp16);
#pragma unroll
    for (int i = 0; i < 16; ++i) { const int x = tid + 512 * i; wls[x] = img[(x >> 10) * 2048 + 1024 + (x & 1023)]; }
  }
#pragma unroll
  for (int r = 0; r < NTT; ++r) {            // unit wv + 8 r = (block, X | Y): tile row i <-> step 32 block + 8 (i / 4) + 4 (X | Y) + i % 4
    const int un = wv + 8 * r;
    trow[r] = min(32 * (un >> 1) + 8 * (l16 >> 2) + 4 * (un & 1) + (l16 & 3), Tm - 1);
  }
  __syncthreads();
  product(std::false_type{});
  __syncthreads();                           // the weights are dead: the accumulators cross over them
  constexpr int HB = (NIT + 1) / 2;          // blocks per round
  const int col = RV_U + 16 * wv + l16;      // lane (n = unit, kq) of wave wv: U'[32 ks + 8 kq + 0..7][16 wv + n]
  const float cf = css[col];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
    for (int r = 0; r < NTT; ++r) {
      const int un = wv + 8 * r - 2 * HB * hf;
      if (un >= 0 && un < 2 * HB && un + 2 * HB * hf < 2 * NIT)
#pragma unroll
        for (int u = 0; u < 8; ++u) xb[(u * 2 * HB + un) * 64 + lane] = acc[r][u];
    }
    __syncthreads();
#pragma unroll
    for (int kl = 0; kl < HB; ++kl) {
      const int ks = HB * hf + kl;
      if (ks < NIT) {
        const f4v x = xb[(wv * 2 * HB + 2 * kl) * 64 + lane], y = xb[(wv * 2 * HB + 2 * kl + 1) * 64 + lane];
        const float v[8] = {fmaf(x[0], cf, 0.f), fmaf(x[1], cf, 0.f), fmaf(x[2], cf, 0.f), fmaf(x[3], cf, 0.f),
                            fmaf(y[0], cf, 0.f), fmaf(y[1], cf, 0.f), fmaf(y[2], cf, 0.f), fmaf(y[3], cf, 0.f)};
        if (tap)
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (32 * ks + 8 * kq + j < Tm) tap[(size_t)(32 * ks + 8 * kq + j) * RV_E + col] = v[j];
        split_f16x8(v, d.mx_uscale, ub[ks][0], ub[ks][1]);
      }
    }
    __syncthreads();
  }

  // ---- keys: the permuted image of W_mem -> LDS
  {
    const uint4* img = reinterpret_cast<const uint4*>(d.Wkp16);
#pragma unroll
    for (int i = 0; i < 16; ++i) wls[tid + 512 * i] = img[tid + 512 * i];
  }
#pragma unroll
  for (int c = 0; c < NTT; ++c) trow[c] = min(16 * (wv + 8 * c) + l16, Tm - 1);
  __syncthreads();
  product(std::true_type{});
  const uint8_t* mrow = d.mask + (size_t)b * Tm;
#pragma unroll
  for (int c = 0; c < NTT; ++c) {            // lane (n = step, kq): key[t][32 ks + 8 kq + 0..7] = X and Y accumulators of tiles 2 ks, 2 ks + 1
    const int t = 16 * (wv + 8 * c) + l16;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const float4 f0 = *reinterpret_cast<const float4*>(css + 32 * ks + 8 * kq), f1 = *reinterpret_cast<const float4*>(css + 32 * ks + 8 * kq + 4);
      const f4v x = acc[c][2 * ks], y = acc[c][2 * ks + 1];
      const float v[8] = {fmaf(x[0], f0.x, 0.f), fmaf(x[1], f0.y, 0.f), fmaf(x[2], f0.z, 0.f), fmaf(x[3], f0.w, 0.f),
                          fmaf(y[0], f1.x, 0.f), fmaf(y[1], f1.y, 0.f), fmaf(y[2], f1.z, 0.f), fmaf(y[3], f1.w, 0.f)};
      if (tap && t < Tm) {
        *reinterpret_cast<float4*>(tap + (size_t)t * RV_E + 32 * ks + 8 * kq) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(tap + (size_t)t * RV_E + 32 * ks + 8 * kq + 4) = make_float4(v[4], v[5], v[6], v[7]);
      }
      split_f16x8(v, d.mx_kscale, kb[c][ks][0], kb[c][ks][1]);
    }
    if (t < Tm && mrow[trow[c]]) livebits |= 1u << c;      // _maybe_mask_score: padded steps never score
  }
  __syncthreads();
}

// Forced decode (DecState::forced): chunk b's input token of step s, as the row of the resident zb table it selects.  An id outside
// the vocabulary selects row V, which holds the bias alone -- no input row, as tf.one_hot gives zeros -- so an id never indexes LDS unchecked
__device__ __forceinline__ int persist_forced_tok(const DecState& d, int b, int s) {
  const int t = d.forced[(size_t)b * d.L + s];
  return (unsigned)t < (unsigned)d.V ? t : d.V;
}

// The compile-time facts of one form k_dec_persist<W, NIT, D, ATT>
template <int W_, int NIT_, int D_, int ATT_, int PARTS_ = 2, bool GRU_ = false>
struct PersistTraits {
  static constexpr int W = W_, NIT = NIT_, D = D_, ATT = ATT_;
  static constexpr bool GRU = GRU_;               // k_dec_persist_gru: the one cell is a Keras GRU (reset_after), its four gate tiles z, r, candidate-input, candidate-recurrent
  static_assert(!GRU || (PARTS_ == 2 && D == 1 && (ATT == 3 || ATT == 4)), "a GRU cell: one cell, two-part fragments, the cell product on the matrix pipe");
  static constexpr int PARTS = PARTS_;            // f16 parts per weight of the Wc16 / Wl16 fragments: 2, or 1 in k_dec_persist_1p (the beams' A image keeps both of its parts)
  static constexpr bool P1 = PARTS == 1;
  static constexpr int FR = P1 ? 64 : 128;        // uint4 per (k-step, gate) pair of a wave: 64 lanes x PARTS fragments
  static_assert(PARTS == 2 || (PARTS == 1 && D == 1 && (ATT == 3 || ATT == 4)), "one-part fragments: one cell with the cell product on the matrix pipe");
  static constexpr bool BAH = ATT == 1 || ATT == 4;   // Bahdanau scores on the VALU (fp32 key rows)
  static constexpr bool MX = ATT >= 2;            // the context on the matrix pipe (U' resident as f16 B fragments, alignments through an LDS image)
  static constexpr bool MXS = ATT == 2 || ATT == 3;   // ... and the Luong scores (keys resident as f16 B fragments, query through an LDS image)
  static constexpr bool MXC = ATT == 3 || ATT == 4;   // ... and the cell product [ctx' | h] . Wcat2 and the output layer (weights as B fragments: Wc16, Wl16)
  static constexpr bool MXC2 = MXC && D == 2;     // two decoder cells, every product on the matrix pipe
  static constexpr int ZS = MXC ? MXC_ZS : RV_G;  // row stride of the gate pre-activations in `part`
  static constexpr int NC = MXC2 ? 0 : (P1 ? mxc_nc1(W) : mxc_nc(W));
  static constexpr int NR = (ATT == 3 && D == 1 && NIT <= 8) ? (P1 ? 10 : 5) : 0;   // (one-part: the same ten registers hold ten pairs)   // T_m <= 256 leaves ~50 registers: waves 1-7 keep NR more (k-step, gate) pairs of their share there
  static constexpr int NP = (NIT + 1) / 2;        // fp32 key rows: pairs of rows per stream
  static constexpr int NTT = (2 * NIT + 7) / 8;   // matrix pipe: a wave's 16-step key tiles
  static constexpr int NI = W > 4 ? 2 : 1;        // C/D registers of a tile: pairs of part rows per lane (beams kq, kq + 4)
  static constexpr bool CACHE = MXC || persist_weight_cache(W, D);
  static constexpr bool FUSE = ATT == 3 && D == 1;   // the default form projects its chunk's memory itself when the call hands it enc_out (persist_project_memory)
  // output layer weights, transposed to [v][k] (rows padded to 132 floats: the 8-lane groups of two outputs then read different banks)
  static constexpr int FCW = RV_U + 4;
  static constexpr int BFC = MXC ? 0 : RV_MAX_VOCAB * FCW;      // offset of b_fc in s_wfc
  static_assert(!MX || D == 1 || ATT == 3, "two decoder cells run either on packed FMAs (ATT 0) or with everything on the matrix pipe (ATT 3)");
  static_assert(NIT <= PERSIST_MAX_NIT && NIT * 256 <= (MXC ? part_floats_mxc(W) : part_floats(W)), "the alignment image (2 f16 parts x 32 NIT steps x 8 slots) must fit `part`");
  static_assert(2 * 1024 * sizeof(_Float16) /* query image: 2 parts x [16 k-blocks][8 slots][8] f16 */ <= (8 * 4 * 2 * 16 * 4) * sizeof(float), "the query image must fit `fold`");
};

// ---- bodies the phases of the persistent decode share
// C/D registers of a 16-column tile: lane (column l16, kq) holds rows 4 kq + i: registers 0 + 1 = beam kq (its high- and low-part rows),
// 2 + 3 = beam kq + 4.  Beam kq + 4 i of a product taken against the high (a0) and the low part (a1) of its B operand
__device__ __forceinline__ float tile_pair_sum(const f4v& a0, const f4v& a1, int i) { return (a0[2 * i] + a0[2 * i + 1]) + (a1[2 * i] + a1[2 * i + 1]); }
// packed FMAs: one float4 weight row times the W beams' values xrow[0..W-1], into 4 columns per beam
template <int W>
__device__ __forceinline__ void beams_fma_row(f2 (&acc)[W][2], const float4& wr, const float* xrow) {
  float xv[WB];
  *reinterpret_cast<float4*>(xv) = *reinterpret_cast<const float4*>(xrow);
  if (W > 4) *reinterpret_cast<float4*>(xv + 4) = *reinterpret_cast<const float4*>(xrow + 4);
#pragma unroll
  for (int w = 0; w < W; ++w) {
    acc[w][0] = __builtin_elementwise_fma(f2{xv[w], xv[w]}, f2{wr.x, wr.y}, acc[w][0]);
    acc[w][1] = __builtin_elementwise_fma(f2{xv[w], xv[w]}, f2{wr.z, wr.w}, acc[w][1]);
  }
}
// h . M for a [128,128] matrix M -- W_q (Bahdanau's processed query) or A_h (two cells: the attention layer's h part) -- of which this
// thread holds 8 rows x 4 columns in pw: thread = (4 columns, 1 of 16 K groups of 8 rows), one batch; partial sums [16][W][128] -> `part`
template <int W>
__device__ __forceinline__ void persist_h_times_rows(float* part, const float* hcT, const float4 (&pw)[8], int tid) {
  const int d4 = tid & 31, kg = tid >> 5;
  f2 acc[W][2];
#pragma unroll
  for (int w = 0; w < W; ++w) { acc[w][0] = f2{0.f, 0.f}; acc[w][1] = f2{0.f, 0.f}; }
#pragma unroll
  for (int u = 0; u < 8; ++u) beams_fma_row<W>(acc, pw[u], &hcT[(8 * kg + u) * WB]);
#pragma unroll
  for (int w = 0; w < W; ++w)
    *reinterpret_cast<float4*>(&part[(kg * W + w) * RV_U + 4 * d4]) = make_float4(acc[w][0].x, acc[w][0].y, acc[w][1].x, acc[w][1].y);
}

// ================= the phases of the prologue that stand as functions, in the order the kernel calls them (the other phases stay
//   inline in the kernel).  Each takes the thread id and derives the coordinates it needs.

// ---- the keys of d.values = [keys | U'] as MFMA B fragments (v_mfma_f32_16x16x32_f16), two f16 parts of the scaled values each.  Scores (MXS): wave
//   wv owns the 16-step tiles wv + 8 c; lane (n = step l % 16 of the tile, kq = l / 16) holds key[t][32 ks + 8 kq + 0..7].
//   Context (MX, inline in the kernel): wave wv owns units 16 wv .. 16 wv + 15; lane (n = unit, kq) holds U'[32 ks + 8 kq + 0..7][unit].  The scales are
//   powers of two from the weights (|key| <= sum_k |W_mem[k][u]| because |enc_out| <= 1): nothing can overflow f16, and what
//   falls into its subnormals is below 2^-28 of the largest value the column can take.
template <typename T>
__device__ __forceinline__ void persist_load_keys_mx(const DecState& d, int b, int tid, float4 (&kb)[T::MXS ? T::NTT : 1][4][2], unsigned& livebits) {
  const int lane = tid & 63, l16 = lane & 15, kq = lane >> 4, wv0 = tid >> 6, Tm = d.Tm;
  const float* cbase = d.values + (size_t)b * Tm * RV_E;
  const uint8_t* mrow = d.mask + (size_t)b * Tm;
#pragma unroll
  for (int c = 0; c < T::NTT; ++c) {
    const int t = 16 * (wv0 + 8 * c) + l16, tc = min(t, Tm - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      float v[8];
      *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(cbase + (size_t)tc * RV_E + 32 * ks + 8 * kq);
      *reinterpret_cast<float4*>(v + 4) = *reinterpret_cast<const float4*>(cbase + (size_t)tc * RV_E + 32 * ks + 8 * kq + 4);
      split_f16x8(v, d.mx_kscale, kb[c][ks][0], kb[c][ks][1]);
    }
    if (t < Tm && mrow[tc]) livebits |= 1u << c;          // _maybe_mask_score: padded steps never score
  }
}

// ---- Bahdanau beside the matrix pipe: tanh(k + q) = 1 - 2 / (1 + 2^(k' + q')) with k' = 2 log2(e) k, and 2^(k' + q') = 2^k' . 2^q': the resident
//   rows hold E_k = 2^k' (ONE exponential per key element for the whole decode), a step's queries come as E_q = 2^q', and a score element
//   costs a multiply-add and ONE reciprocal instead of an exponential and a reciprocal -- the loop is bound by the transcendental rate
//   (16 lanes per clock and CU).  Exact for |k'| <= 64 and |q'| <= 60 (the product stays a normal f32: |k| <= 22, |h . W_q| <= 20);
//   a chunk with a larger key keeps k' and takes the two-transcendental form for all its steps, a step with a larger query takes
//   2^(log2(E_k) + q') -- both block-uniform choices, neither ever seen with weights of any plausible scale.
//   Two phases around the kernel's block-wide OR: does this thread hold a key out of range; k' -> E_k
template <typename T>
__device__ __forceinline__ bool persist_keys_out_of_range(const float4 (&kr)[T::MXS ? 1 : T::NP][4]) {
  bool big = false;
#pragma unroll
  for (int p = 0; p < T::NP; ++p)
#pragma unroll
    for (int m = 0; m < 4; ++m)
      big = big || !(fabsf(kr[p][m].x) <= 64.f && fabsf(kr[p][m].y) <= 64.f && fabsf(kr[p][m].z) <= 64.f && fabsf(kr[p][m].w) <= 64.f);
  return big;
}
template <typename T>
__device__ __forceinline__ void persist_keys_to_exp2(float4 (&kr)[T::MXS ? 1 : T::NP][4]) {
#pragma unroll
  for (int p = 0; p < T::NP; ++p)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      kr[p][m].x = __builtin_amdgcn_exp2f(kr[p][m].x); kr[p][m].y = __builtin_amdgcn_exp2f(kr[p][m].y);
      kr[p][m].z = __builtin_amdgcn_exp2f(kr[p][m].z); kr[p][m].w = __builtin_amdgcn_exp2f(kr[p][m].w);
    }
}

// ---- (T_m <= 256, default form) pairs 32 - NC - NR .. 32 - NC - 1 of this wave's share of the cell product, in registers for the whole decode
template <typename T>
__device__ __forceinline__ void persist_load_resident_pairs(const DecState& d, int tid, uint4 (&rbh)[T::NR > 0 ? T::NR : 1], uint4 (&rbl)[(T::NR > 0 && !T::P1) ? T::NR : 1]) {
  const uint4* wimg = reinterpret_cast<const uint4*>(d.Wc16) + (size_t)(tid >> 6) * (32 * T::FR) + (tid & 63);
#pragma unroll
  for (int r = 0; r < T::NR; ++r) {
    if constexpr (T::P1) rbh[r] = wimg[(32 - T::NC - T::NR + r) * 64];
    else { rbh[r] = wimg[(2 * (32 - T::NC - T::NR + r)) * 64]; rbl[r] = wimg[(2 * (32 - T::NC - T::NR + r) + 1) * 64]; }
  }
}

// ================= the phases of a step that stand as functions, in the order the kernel calls them.  None holds a barrier: every
//   __syncthreads of a step stands in the kernel body.  Each takes the thread id of this step (the opaque copy) and the pointers it uses.

// ---- Luong scores on the matrix pipe: rows = beams, columns = the 16 steps of a tile, K = 128 units, query image in `fold` -> sc
template <typename T>
__device__ __forceinline__ void persist_scores_mx(const DecState& d, int tid, unsigned livebits, const float4 (&kb)[T::MXS ? T::NTT : 1][4][2], float (&sc)[T::NTT][T::NI], const float* fold) {

  constexpr int W = T::W;
  const int lane = tid & 63, wv = tid >> 6, l16 = lane & 15, kq = lane >> 4;

  {
    const _Float16* qa = reinterpret_cast<const _Float16*>(fold) + (kq * 16 + l16) * 8;    // row l16 of k-block 4 ks + kq
    // the tiles in turns (against the low, then against the high part of the keys): an MFMA accumulates onto a result that is NTT
    // instructions old, not onto the one issued just before it
    f4v acc[T::NTT];
#pragma unroll
    for (int c = 0; c < T::NTT; ++c) acc[c] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {                    // one k-step of the query at a time: 4 registers of A fragments live
      const h8 a = *reinterpret_cast<const h8*>(qa + ks * 512);
#pragma unroll
      for (int c = 0; c < T::NTT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, kb[c][ks][1]), acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < T::NTT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, kb[c][ks][0]), acc[c], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int c = 0; c < T::NTT; ++c) {
      const bool live = (livebits >> c) & 1u;
#pragma unroll
      for (int i = 0; i < T::NI; ++i)
        sc[c][i] = (live && kq + 4 * i < W) ? (acc[c][2 * i] + acc[c][2 * i + 1]) * d.mx_kdescale : -INFINITY;
    }
  }
}

// ---- softmax on the matrix-pipe scores, first half: this wave's maximum (-> mrow_) and sum of every beam -> `ml`; sc <- exp2(sc - max)
template <typename T>
__device__ __forceinline__ void persist_softmax_wave_mx(int tid, float (&sc)[T::NTT][T::NI], float (&mrow_)[T::NI], float* ml) {

  const int lane = tid & 63, wv = tid >> 6, l16 = lane & 15, kq = lane >> 4;

#pragma unroll
  for (int i = 0; i < T::NI; ++i) {
    float m = sc[0][i];
#pragma unroll
    for (int c = 1; c < T::NTT; ++c) m = fmaxf(m, sc[c][i]);
    m = fmaxf(m, dpp<0xB1>(m)); m = fmaxf(m, dpp<0x4E>(m)); m = fmaxf(m, dpp<0x141>(m)); m = fmaxf(m, dpp<0x140>(m));
    const float ms = m == -INFINITY ? 0.f : m;           // a wave without live steps for this beam: every term exp2(-inf) = 0
    float lsum = 0.f;
#pragma unroll
    for (int c = 0; c < T::NTT; ++c) { sc[c][i] = __builtin_amdgcn_exp2f(sc[c][i] - ms); lsum += sc[c][i]; }
    lsum = row16_sum(lsum);
    mrow_[i] = m;
    if (l16 == 0) { ml[wv * WB + kq + 4 * i] = m; ml[(8 + wv) * WB + kq + 4 * i] = lsum; }
  }
}

// k_dec_persist and k_dec_persist_1p are two kernels over ONE body, decode_persist_body.inc: each names its compile-time facts (W, NIT,
// D, ATT and the traits T, which hold the part count of the weight fragments) and includes it.  Textual, not a function both call: the
// two-part kernels then compile to the instruction streams they had before the one-part forms existed
template <int W, int NIT, int D, int ATT = 0>
__global__ __launch_bounds__(512) void k_dec_persist(DecState d, const float* __restrict__ Wcat /*[256,512] = [W_in rows of the attention input ; U]*/,
                                                      const float* __restrict__ Wtok /*[V,512]*/, const float* __restrict__ bdec /*[512]*/,
                                                      const float* __restrict__ Wcat1 /*D == 2: [256,512] = [W_1 ; U_1]*/, const float* __restrict__ bdec1,
                                                      const float* __restrict__ Nh /*D == 1: A_h . W_fc [128,V]*/) {
  constexpr int NT = 512;
  using T = PersistTraits<W, NIT, D, ATT>;
#include "decode_persist_body.inc"
}
// Option weight_parts 1: d.Wc16 / d.Wl16 name the one-part images [wave][pair][64 lanes][8 f16] / [8 k-steps][64 lanes][8 f16] (one
// decoder cell; the second parts, all zero in that mode, are neither stored nor streamed nor multiplied)
template <int W, int NIT, int ATT>
__global__ __launch_bounds__(512) void k_dec_persist_1p(DecState d, const float* __restrict__ Wcat, const float* __restrict__ Wtok, const float* __restrict__ bdec,
                                                         const float* __restrict__ Wcat1, const float* __restrict__ bdec1, const float* __restrict__ Nh) {
  constexpr int NT = 512, D = 1;
  using T = PersistTraits<W, NIT, D, ATT, 1>;
#include "decode_persist_body.inc"
}

// One 64-thread workgroup per chunk: the chunk's [S,W] ids/parents are staged in LDS so the
// serial gather_tree back-trace runs on LDS latency, not on dependent global loads.
__global__ __launch_bounds__(64) void k_dec_finalize(DecState d, int32_t* tokens, float* out2, const void* const* ptab, DecMembers mem) {
  __shared__ int s_ids[64 * RV_MAX_BEAM], s_par[64 * RV_MAX_BEAM], s_tok[64];
  __shared__ int s_S;
  if (ptab) {      // graph replay: this call's output addresses (the kernel arguments are the capture's)
    tokens = static_cast<int32_t*>(const_cast<void*>(ptab[RV_PTAB_TOKENS]));
    out2 = static_cast<float*>(const_cast<void*>(ptab[RV_PTAB_OUT2]));
  }
  const int b = blockIdx.x, tid = threadIdx.x;
  const int steps = d.L - 1, W = d.W, V = d.V;
  // the member of a coalesced call this chunk belongs to: its rows, its outputs, its word for S (one member = the whole slab otherwise)
  int r0 = 0, nr = d.B, mi = 0;
#pragma unroll
  for (int m = 0; m < RV_MAX_MEMBERS; ++m)
    if (m < mem.n && b >= mem.row0[m] && b < mem.row0[m] + mem.rows[m]) { r0 = mem.row0[m]; nr = mem.rows[m]; mi = m; tokens = mem.tokens[m]; out2 = mem.out2[m]; }
  const int br = b - r0;      // the chunk's row in its member's outputs
  // S: steps the reference loop runs for the WHOLE slab (until every row is finished); So: steps this
  // sub-slab actually ran.  For s in [So, S) all of its beams are finished: the reference emits the
  // end token at an unchanged top-1 score there, which is what is written below.
  // persistent decode: S of the slab = the slowest chunk's step count, taken here by every workgroup (B <= a few thousand ints
  // from L2) instead of in a launch of its own; workgroup 0 leaves it in S_dev for the host
  if (d.chunk_steps) {
    int m = 0;
    for (int i = tid; i < nr; i += 64) m = max(m, d.chunk_steps[r0 + i]);
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if (tid == 0) { s_S = m; if (br == 0) { d.S_host[mi] = m; if (b == 0) { d.S_dev[0] = m; d.S_dev[1] = m; } } }
    __syncthreads();
  }
  const int S = d.chunk_steps ? s_S : d.S_dev[0], So = d.chunk_steps ? d.chunk_steps[b] : d.S_dev[1 + d.part];
  int32_t* tk = tokens + (size_t)br * steps;
  if (d.greedy) {
    for (int s = tid; s < steps; s += 64) {
      tk[s] = s < S ? d.step_ids[(size_t)s * d.B + b] : d.pad_token;
      for (int v = 0; v < V; ++v)
        out2[((size_t)br * steps + s) * V + v] = s < S ? d.step_logits[((size_t)s * d.B + b) * V + v] : 0.f;
    }
    return;
  }
  for (int i = tid; i < So * W; i += 64) {
    const int s = i / W, w = i % W;
    s_ids[i] = d.step_ids[((size_t)s * d.B + b) * W + w];
    s_par[i] = d.parent_ids[((size_t)s * d.B + b) * W + w];
  }
  __syncthreads();
  if (tid == 0) {
    int maxlen = 0;
    for (int w = 0; w < W; ++w) maxlen = max(maxlen, d.lengths[(size_t)b * W + w]);
    const int Lb = min(S, maxlen);
    for (int s = 0; s < S; ++s) s_tok[s] = d.end_token;
    if (Lb > 0) {
      s_tok[Lb - 1] = s_ids[(Lb - 1) * W];
      int p = s_par[(Lb - 1) * W];
      for (int t = Lb - 2; t >= 0; --t) {
        s_tok[t] = s_ids[t * W + p];
        p = s_par[t * W + p];
      }
      bool done = false;
      for (int t = 0; t < Lb; ++t) {
        if (done) s_tok[t] = d.end_token;
        else if (s_tok[t] == d.end_token) done = true;
      }
    }
  }
  __syncthreads();
  // one wave, lane = step (max_output_len <= 64)
  const int s = tid;
  const int tokv = s < S ? s_tok[s] : d.pad_token;
  const float scv = s < S ? d.step_scores[((size_t)min(s, So - 1) * d.B + b) * W] : 0.f;
  if (s < steps) { tk[s] = tokv; out2[(size_t)br * steps + s] = scv; }
  if (d.call_bases) {
    // fused tokens_to_nuc_sequences + calc_prob_logits_beam_search_scores for this chunk
    const float prev = __shfl_up(scv, 1);
    const uint8_t ch = (s < S && tokv >= 0 && tokv < RV_MAX_VOCAB) ? d.lut[tokv] : 0;
    const unsigned long long m = __ballot(ch != 0);
    const int pos = __popcll(m & ((1ull << s) - 1ull));
    if (s < steps) {
      d.call_probs[(size_t)b * steps + s] = s < S ? __expf(scv - (s == 0 ? 0.f : prev)) : 0.f;
      d.call_bases[(size_t)b * steps + s] = 0;
    }
    __syncthreads();
    if (ch) d.call_bases[(size_t)b * steps + pos] = ch;
    if (s == 0) d.call_len[b] = __popcll(m);
  }
}

// one wave: lane s looks at step s (max_output_len <= 64), ballot finds the first finished step
__global__ __launch_bounds__(64) void k_dec_reduce_steps(DecParts p) {
  const int lane = threadIdx.x;
  int S = 0;
  for (int g = 0; g < p.n; ++g) {
    const bool done = lane < p.steps && p.nfin[g][lane] >= p.B[g];
    const unsigned long long m = __ballot(done);
    const int Sg = m ? __ffsll((long long)m) : p.steps;      // first finished step index + 1
    if (lane == 0) p.S_dev[1 + g] = Sg;
    S = max(S, Sg);
  }
  if (lane == 0) { p.S_dev[0] = S; p.S_host[0] = S; }
}

// The instantiations of the decode kernels, each listed once: the dynamic-LDS opt-ins, the persistent decode's form check and the
// launches walk these lists, so adding or removing a form is a change to its list only.  A list calls fn with each form in turn until
// fn returns true, and says whether one did.  (Function templates rather than nested generic lambdas, whose instantiations the
// compiler emits in reverse: a list's order is the order the kernels are emitted in, and the compiler's code for some of the
// matrix-pipe persistent forms changes with that order)

// k_dec_persist<W, NIT, D, ATT>: one decoder cell in each attention form (PersistLds) for every beam width, two cells (Luong: every
// product on the matrix pipe, or packed FMAs) for W <= 5 (LDS).  NIT resident row groups serve T_m <= 32 NIT: the first form of
// the list that serves a call has the fewest
template <int W_, int NIT_, int D_, int ATT_> struct PersistForm { static constexpr int W = W_, NIT = NIT_, D = D_, ATT = ATT_; };
template <int W, int D, int ATT, typename Fn> bool persist_nit(Fn& fn) {
  return fn(PersistForm<W, 2, D, ATT>{}) || fn(PersistForm<W, 8, D, ATT>{}) || fn(PersistForm<W, 11, D, ATT>{});
}
template <int W, typename Fn> bool persist_w(Fn& fn) {
  if constexpr (W <= 5)
    if (persist_nit<W, 2, 3>(fn) || persist_nit<W, 2, 0>(fn)) return true;
  return persist_nit<W, 1, 4>(fn) || persist_nit<W, 1, 1>(fn) || persist_nit<W, 1, 3>(fn) || persist_nit<W, 1, 2>(fn) || persist_nit<W, 1, 0>(fn);
}
template <typename Fn> bool for_each_persist_form(Fn&& fn) {
  return persist_w<1>(fn) || persist_w<2>(fn) || persist_w<3>(fn) || persist_w<4>(fn) || persist_w<5>(fn) || persist_w<6>(fn) ||
         persist_w<7>(fn) || persist_w<8>(fn);
}
template <typename F> bool persist_serves(int W, int D, int ATT, int Tm) { return F::W == W && F::D == D && F::ATT == ATT && Tm <= 32 * F::NIT; }
// k_dec_persist_1p<W, NIT, ATT> (option weight_parts 1): Luong with the cell product on the matrix pipe, one cell, at the NIT bands of
// the two-part list, for the beam widths of greedy / forced decodes and of the flagship beam search.  A width without a form here runs
// k_dec_persist on the zero-lo images
template <typename Fn> bool for_each_persist_form_1p(Fn&& fn) { return persist_nit<1, 1, 3>(fn) || persist_nit<5, 1, 3>(fn); }

// The per-step attend kernels: k_dec_attend_flash<W, NT> runs NT threads; k_dec_attend<W, TB, TD = 4 TB> serves T_m <= 32 TB (the
// first of the list that serves a call has the shortest sweeps)
template <int W_, int NT_> struct FlashForm { static constexpr bool FLASH = true; static constexpr int W = W_, NT = NT_; };
template <int W_, int TB_> struct AttendForm { static constexpr bool FLASH = false; static constexpr int W = W_, TB = TB_, TD = 4 * TB_; };
template <int W, typename Fn> bool attend_w(Fn& fn) {
  return fn(FlashForm<W, 256>{}) || fn(FlashForm<W, 512>{}) || fn(AttendForm<W, 2>{}) || fn(AttendForm<W, 7>{}) || fn(AttendForm<W, 11>{});
}
template <typename Fn> bool for_each_attend_form(Fn&& fn) {
  return attend_w<1>(fn) || attend_w<2>(fn) || attend_w<3>(fn) || attend_w<4>(fn) || attend_w<5>(fn) || attend_w<6>(fn) ||
         attend_w<7>(fn) || attend_w<8>(fn);
}
// (the flash forms of W 6-8 are listed and opted in, but a call only takes the single-pass attend with an effective beam <= 5:
// ravvent_hip.cpp, record_slab, lflash)
template <typename F> bool attend_serves(int W, bool flash, int NT, int Tm) {
  if constexpr (F::FLASH) return F::W == W && flash && F::NT == NT;
  else return F::W == W && !flash && Tm <= 32 * F::TB;
}

}  // namespace

void list_decode_forms_1p(FormLog& log) {
  for_each_persist_form_1p([&](auto f) { using F = decltype(f); log.add(RV_K_DEC_PERSIST_1P, F::W, F::NIT, F::D, F::ATT); return false; });
}
void list_decode_forms(FormLog& log) {
  for_each_persist_form([&](auto f) { using F = decltype(f); log.add(RV_K_DEC_PERSIST, F::W, F::NIT, F::D, F::ATT); return false; });
  for_each_attend_form([&](auto f) {
    using F = decltype(f);
    if constexpr (F::FLASH) log.add(RV_K_DEC_ATTEND_FLASH, F::W, F::NT);
    else log.add(RV_K_DEC_ATTEND, F::W, F::TB);
    return false;
  });
}

int dec_persist_form(int attention, int depth, int W, int Tm, bool greedy, bool matrix_attention, bool matrix_cell) {
  const bool mxc = matrix_attention && matrix_cell;
  const int att = attention == 1 ? (mxc ? 4 : 1) : attention == 0 ? (mxc ? 3 : (matrix_attention && depth == 1 ? 2 : 0)) : -1;
  if (greedy && W != 1) return -1;            // (greedy search decodes one beam)
  if (!for_each_persist_form([&](auto f) { return persist_serves<decltype(f)>(W, depth, att, Tm); })) return -1;
  return sizeof(float) * PersistLds(W, depth, att).total + persist_static_lds(att) <= 160 * 1024 ? att : -1;
}
// (defined at the end of the file: the one-part kernels are emitted after every kernel that was there before them, whose code
// depends on the order of emission -- see the note above the form lists)
static bool launch_dec_persist_1p(const DecState& d, const float* Wcat, const float* Wtok, const float* bdec, const float* Wcat1, const float* bdec1,
                                  const float* Nh, hipStream_t s, FormLog* log, const uint16_t* Wc16p1, const uint16_t* Wl16p1);
void launch_dec_persist(const DecState& d, const float* Wcat, const float* Wtok, const float* bdec,
                        const float* Wcat1, const float* bdec1, const float* Nh, hipStream_t s, FormLog* log,
                        const uint16_t* Wc16p1, const uint16_t* Wl16p1) {
  if (Wc16p1 && Wl16p1 && launch_dec_persist_1p(d, Wcat, Wtok, bdec, Wcat1, bdec1, Nh, s, log, Wc16p1, Wl16p1)) return;
  for_each_persist_form([&](auto f) {
    using F = decltype(f);
    if (!persist_serves<F>(d.W, d.depth, d.persist_att, d.Tm)) return false;
    hipLaunchKernelGGL((k_dec_persist<F::W, F::NIT, F::D, F::ATT>), dim3(d.B), dim3(512), sizeof(float) * PersistLds(F::W, F::D, F::ATT).total, s,
                       d, Wcat, Wtok, bdec, Wcat1, bdec1, Nh);
    if (log) log->add(RV_K_DEC_PERSIST, F::W, F::NIT, F::D, F::ATT);
    return true;
  });
  // (S = max over chunk_steps is taken by k_dec_finalize)
}

void launch_dec_reduce_steps(const DecParts& p, hipStream_t s) {
  hipLaunchKernelGGL(k_dec_reduce_steps, dim3(1), dim3(64), 0, s, p);
}

void launch_input_mask(const float* raw, const float* ev, int B, int T_r, int T_e, float pad,
                       uint8_t* mask, hipStream_t s) {
  const int n = B * (T_r + T_e);
  hipLaunchKernelGGL(k_input_mask, dim3((n + 255) / 256), dim3(256), 0, s, raw, ev, B, T_r, T_e, pad, mask);
}
void launch_dec_init(const DecState& d, hipStream_t s) {
  const int n = max(d.B * d.W, d.L);
  hipLaunchKernelGGL(k_dec_init, dim3((n + 255) / 256), dim3(256), 0, s, d);
}
void launch_dec_cell(const DecState& d, int layer, const float* WcatT, const float* Wtok, const float* bias, int step,
                     hipStream_t s) {
  const int N = d.B * d.W;
  const size_t shm = sizeof(float) * CELL_LDS_FLOATS;
  hipLaunchKernelGGL(k_dec_cell, dim3(RV_U / 16, (N + CELL_ROWS - 1) / CELL_ROWS), dim3(512), shm, s, d, layer, WcatT, Wtok, bias, step);
}
void launch_dec_attend(const DecState& d, const float* WmemT, bool flash, int step, hipStream_t s, FormLog* log) {
  // flash: more chunks than CUs -> two 256-thread workgroups per CU overlap each other's phases
  const int NT = (d.attend_threads ? d.attend_threads == 256 : d.B > 320) ? 256 : 512;
  for_each_attend_form([&](auto f) {
    using F = decltype(f);
    if (!attend_serves<F>(d.W, flash, NT, d.Tm)) return false;
    if constexpr (F::FLASH) {
      hipLaunchKernelGGL((k_dec_attend_flash<F::W, F::NT>), dim3(d.B), dim3(F::NT), sizeof(float) * AttLds(F::W, 0, true, F::NT).total, s, d, WmemT, step);
      if (log) log->add(RV_K_DEC_ATTEND_FLASH, F::W, F::NT);
    } else {
      hipLaunchKernelGGL((k_dec_attend<F::W, F::TB, F::TD>), dim3(d.B), dim3(ATT_THREADS), sizeof(float) * AttLds(F::W, (d.Tm + 3) & ~3, false).total, s, d, step);
      if (log) log->add(RV_K_DEC_ATTEND, F::W, F::TB);
    }
    return true;
  });
}
// Kernels that use more than the default dynamic-LDS limit opt in once per device (called by rv_create after hipSetDevice): sized
// for the largest shapes the library accepts (T_m <= 352), up to what the kernel's static LDS leaves of the 160 KB (the attend
// kernels' static part, like k_dec_persist's with packed-FMA cells, is under 10 KB)
static hipError_t configure_dec_persist_gru();      // (the GRU forms: defined with their kernel at the end of the file)
hipError_t configure_decode_kernels() {
  hipError_t first = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dec_cell), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(sizeof(float) * CELL_LDS_FLOATS));
  auto opt = [&](const void* f, size_t bytes, int static_lds) {
    const size_t cap = 160 * 1024 - static_lds;
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes < cap ? bytes : cap));
    if (e != hipSuccess && first == hipSuccess) first = e;
    return false;
  };
  for_each_attend_form([&](auto f) {
    using F = decltype(f);
    if constexpr (F::FLASH)
      return opt(reinterpret_cast<const void*>(&k_dec_attend_flash<F::W, F::NT>), sizeof(float) * AttLds(F::W, 0, true, F::NT).total, 10 * 1024);
    else
      return opt(reinterpret_cast<const void*>(&k_dec_attend<F::W, F::TB, F::TD>), sizeof(float) * AttLds(F::W, 32 * F::TB, false).total, 10 * 1024);
  });
  for_each_persist_form([&](auto f) {
    using F = decltype(f);
    return opt(reinterpret_cast<const void*>(&k_dec_persist<F::W, F::NIT, F::D, F::ATT>), sizeof(float) * PersistLds(F::W, F::D, F::ATT).total,
               persist_static_lds(F::ATT));
  });
  for_each_persist_form_1p([&](auto f) {
    using F = decltype(f);
    return opt(reinterpret_cast<const void*>(&k_dec_persist_1p<F::W, F::NIT, F::ATT>), sizeof(float) * PersistLds(F::W, 1, F::ATT, 1).total,
               persist_static_lds(F::ATT));
  });
  const hipError_t eg = configure_dec_persist_gru();
  return first != hipSuccess ? first : eg;
}

void launch_dec_finalize(const DecState& d, int32_t* tokens, float* out2, hipStream_t s, const void* const* ptab, const DecMembers* members) {
  DecMembers mem{};
  if (members) mem = *members;
  hipLaunchKernelGGL(k_dec_finalize, dim3(d.B), dim3(64), 0, s, d, tokens, out2, ptab, mem);
}

// The one-part form that serves the call, if the one-part list holds one: k_dec_persist_1p on the one-part images
static bool launch_dec_persist_1p(const DecState& d, const float* Wcat, const float* Wtok, const float* bdec, const float* Wcat1, const float* bdec1,
                                  const float* Nh, hipStream_t s, FormLog* log, const uint16_t* Wc16p1, const uint16_t* Wl16p1) {
  return for_each_persist_form_1p([&](auto f) {
    using F = decltype(f);
    if (!persist_serves<F>(d.W, d.depth, d.persist_att, d.Tm)) return false;
    DecState d1 = d;
    d1.Wc16 = Wc16p1; d1.Wl16 = Wl16p1;
    hipLaunchKernelGGL((k_dec_persist_1p<F::W, F::NIT, F::ATT>), dim3(d.B), dim3(512), sizeof(float) * PersistLds(F::W, 1, F::ATT, 1).total, s,
                       d1, Wcat, Wtok, bdec, Wcat1, bdec1, Nh);
    if (log) log->add(RV_K_DEC_PERSIST_1P, F::W, F::NIT, F::D, F::ATT);
    return true;
  });
}

// ---- the persistent decode of a GRU cell (a GRU handle under option gru_persistent 1).  A third kernel over the body of k_dec_persist:
// one cell, two-part fragments, the cell product on the matrix pipe; T::GRU switches the gate phase, nothing else.  d.Wc16 / d.Wl16 /
// d.Wq16 name the folded GRU images, whose four column tiles are z, r and the candidate's input and recurrent halves; Wcat, Wcat1, bdec1
// and Nh are unused (the arguments stay those of the body).  Kernel, form list and launchers stand behind every kernel that was in this
// file before them: see the note above the form lists
namespace {
template <int W, int NIT, int ATT>
__global__ __launch_bounds__(512) void k_dec_persist_gru(DecState d, const float* __restrict__ Wcat, const float* __restrict__ Wtok, const float* __restrict__ bdec,
                                                          const float* __restrict__ Wcat1, const float* __restrict__ bdec1, const float* __restrict__ Nh) {
  constexpr int NT = 512, D = 1;
  using T = PersistTraits<W, NIT, D, ATT, 2, true>;
#include "decode_persist_body.inc"
}
// k_dec_persist_gru<W, NIT, ATT>: Luong (3) and Bahdanau (4) for every beam width at the NIT bands of the LSTM list
template <int W, typename Fn> bool persist_gru_w(Fn& fn) { return persist_nit<W, 1, 3>(fn) || persist_nit<W, 1, 4>(fn); }
template <typename Fn> bool for_each_persist_form_gru(Fn&& fn) {
  return persist_gru_w<1>(fn) || persist_gru_w<2>(fn) || persist_gru_w<3>(fn) || persist_gru_w<4>(fn) || persist_gru_w<5>(fn) ||
         persist_gru_w<6>(fn) || persist_gru_w<7>(fn) || persist_gru_w<8>(fn);
}
}  // namespace

void list_decode_forms_gru(FormLog& log) {
  for_each_persist_form_gru([&](auto f) { using F = decltype(f); log.add(RV_K_DEC_PERSIST_GRU, F::W, F::NIT, F::D, F::ATT); return false; });
}
int dec_persist_form_gru(int attention, int W, int Tm, bool greedy) {
  const int att = attention == 1 ? 4 : attention == 0 ? 3 : -1;
  if (greedy && W != 1) return -1;
  if (!for_each_persist_form_gru([&](auto f) { return persist_serves<decltype(f)>(W, 1, att, Tm); })) return -1;
  return sizeof(float) * PersistLds(W, 1, att).total + persist_static_lds(att) <= 160 * 1024 ? att : -1;
}
void launch_dec_persist_gru(const DecState& d, const float* Wtok, const float* bdec, hipStream_t s, FormLog* log) {
  for_each_persist_form_gru([&](auto f) {
    using F = decltype(f);
    if (!persist_serves<F>(d.W, d.depth, d.persist_att, d.Tm)) return false;
    hipLaunchKernelGGL((k_dec_persist_gru<F::W, F::NIT, F::ATT>), dim3(d.B), dim3(512), sizeof(float) * PersistLds(F::W, 1, F::ATT).total, s,
                       d, nullptr, Wtok, bdec, nullptr, nullptr, nullptr);
    if (log) log->add(RV_K_DEC_PERSIST_GRU, F::W, F::NIT, F::D, F::ATT);
    return true;
  });
}
static hipError_t configure_dec_persist_gru() {
  hipError_t first = hipSuccess;
  for_each_persist_form_gru([&](auto f) {
    using F = decltype(f);
    const size_t bytes = sizeof(float) * PersistLds(F::W, 1, F::ATT).total, cap = 160 * 1024 - persist_static_lds(F::ATT);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dec_persist_gru<F::W, F::NIT, F::ATT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes < cap ? bytes : cap));
    if (e != hipSuccess && first == hipSuccess) first = e;
    return false;
  });
  return first;
}
