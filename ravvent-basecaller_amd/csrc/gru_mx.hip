// The BiGRU family (rv_create_rnn, RV_RNN_BIGRU): the encoder recurrence on the 16-bit matrix pipe and the decoder
// cell of the per-step decode.  Cell math: Keras GRUCell with its defaults (reset_after = True, sigmoid / tanh, gate order z, r, h) --
// the cells /root/reference/basecaller.py:18-46, 85-89 build for rnn_type 'bigru':
//     xi = x . W + b[0]          hr = h . U + b[1]
//     z  = sigmoid(xi_z + hr_z)  r = sigmoid(xi_r + hr_r)
//     hh = tanh(xi_h + r * hr_h) h' = z * h + (1 - z) * hh
//
// K1g, k_gru_rec_mx<F, CH> -- modelled on rec_mx_body of lstm_mx.hip, sixteen chunks of ONE direction per workgroup of 512 threads.  With
// reset_after the recurrent product of a step is one h . U of 3u columns: z^T [384 gate columns x 16 chunks] = U^T [384 x 128] . h^T
// [128 x 16] on v_mfma_f32_16x16x32_f16 with split operands (two f16 parts per value, three exact part products, f32 accumulation):
//   * U^T stays resident as A fragments: wave w owns units 16 w .. 16 w + 15 of the three gates = 3 row tiles x 4 k-steps x 2 parts x
//     4 VGPRs = 96 VGPRs;
//   * h^T goes through the same double-buffered LDS image, [part][k-block of 8 units][chunk][8 f16], scaled by 2^14: |h| <= 1 holds for a
//     GRU started from zeros or from a chained final state (h' is a convex combination of h and a tanh);
//   * per gate column r a power-of-two scale s_r brings its largest element into [2^13, 2^14); hr = acc * (2^-14 / s_r) + b[1].  The
//     factors and b[1] are staged side by side in LDS;
//   * the C/D layout gives lane (chunk n = lane % 16, q = lane / 16) all three gate sums of units 16 w + 4 q + 0..3 of chunk n: the update
//     is local to the lane, with the previous h of those units in four registers.  hr_h stays apart from xi_h until r has multiplied it;
//   * one raw s_barrier per step.
// F = 1 / F = 5: layer 0 takes x . W + b[0] in the lane from LDS-staged input windows and leaves utils.input_mask of its chunks, as the LSTM
// forms do.  F = 0: pre-projected inputs xw [B,T,2,384] = x . W + b[0] (the split-f16 GEMM of gemm_f32.hip over three column blocks),
// requested two steps ahead through a ring of three register sets.  CH = 16 only; chunk tensors only (a window call runs behind
// k_expand_windows, the asynchronous calls of a GRU handle are never coalesced).
//
// D1g, k_dec_cell_gru -- modelled on k_dec_cell of decode.hip: 64 beam rows x 16 units per workgroup, K = 256 = [attention or the lower
// cell's h | h], fp32 MFMA.  The pre-transposed image holds FOUR column tiles per unit block: z, r, [W_h ; 0] and [0 ; U_h], so that the
// candidate gate's input part xi_h and recurrent part hr_h come out of the same product apart (the zero halves add exact zeros).
#include "common.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4v __attribute__((ext_vector_type(4)));

#define RV_GRU_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)

template <int F, int CH>
__global__ __launch_bounds__(512) void k_gru_rec_mx(GruRecArgs a) {
  static_assert(F == 0 || F == 1 || F == 5, "pre-projected inputs, or layer 0 on its F input features (raw samples: 1; events: 5)");
  static_assert(CH == 16, "sixteen chunks per workgroup");
  extern __shared__ __align__(16) char gsm[];
  char* hb = gsm;                                                // [2 buffers][2 parts][16 k-blocks][16 chunks][8 f16] = 16 KB
  float* dss = reinterpret_cast<float*>(gsm + 16384);            // [384] 2^-14 / s_r
  float* b1s = dss + RV_GG;                                      // [384] recurrent bias b[1]
  float* wxs = b1s + RV_GG;                                      // F > 0: [F][384] input kernel rows, [384] input bias b[0]
  float* xs = wxs + (F + 1) * RV_GG;                             // F > 0: [CH][T][F] input windows

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, q = lane >> 4;
  const int dir = blockIdx.y, b0 = blockIdx.x * CH, T = a.T;
  const int bc = min(b0 + n, a.B - 1);                           // rows beyond the slab compute on a copy of its last chunk, never stored
  const bool live = b0 + n < a.B;
  const int u0 = 16 * w + 4 * q;                                 // this lane's four units

  // ---- U^T -> registers (A fragments), once
  float4 ua[3][4][2];
  {
    const float4* src = reinterpret_cast<const float4*>(a.Ua[dir]) + (size_t)w * (3 * 4 * 2 * 64) + lane;
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int p = 0; p < 2; ++p) ua[g][ks][p] = src[((g * 4 + ks) * 2 + p) * 64];
  }
  {
    const float* dsg = reinterpret_cast<const float*>(a.Ua[dir] + (size_t)2 * RV_U * RV_GG);
    if (tid < RV_GG) {
      dss[tid] = dsg[tid];
      b1s[tid] = a.b[dir][RV_GG + tid];
      if (F > 0) {
#pragma unroll
        for (int f = 0; f < F; ++f) wxs[f * RV_GG + tid] = a.W[dir][f * RV_GG + tid];
        wxs[F * RV_GG + tid] = a.b[dir][tid];
      }
    }
    if (F > 0) {
      for (int r = 0; r < CH; ++r) {
        const int b = min(b0 + r, a.B - 1);
        const bool wm = a.mask && dir == 0 && b0 + r < a.B;     // utils.input_mask of this encoder's part (utils.py:26-32: all features != pad), once per chunk
        for (int i = tid; i < T; i += 512) {
          const float* v = a.x + ((size_t)b * T + i) * F;
          bool real = true;
#pragma unroll
          for (int f = 0; f < F; ++f) { const float xv = v[f]; xs[(r * T + i) * F + f] = xv; real = real && xv != a.pad; }
          if (wm) a.mask[(size_t)b * a.mask_T + a.mask_t0 + i] = real ? 1 : 0;
        }
      }
    }
  }
  // ---- initial state: h in registers and as the first B image.  A lane writes its four units of chunk n as f16 parts
  float hl[4];
  {
    float4 h0{0.f, 0.f, 0.f, 0.f};
    if (a.h0[dir]) h0 = *reinterpret_cast<const float4*>(a.h0[dir] + (size_t)bc * RV_U + u0);
    hl[0] = h0.x; hl[1] = h0.y; hl[2] = h0.z; hl[3] = h0.w;
    h4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float sv = hl[i] * 16384.f; hi[i] = (_Float16)sv; lo[i] = (_Float16)(sv - (float)hi[i]); }
    char* dst = hb + ((2 * w + (q >> 1)) * 16 + n) * 16 + (q & 1) * 8;
    *reinterpret_cast<h4*>(dst) = hi; *reinterpret_cast<h4*>(dst + 4096) = lo;
  }
  // pre-projected inputs: the loads of step s + 2 are issued in step s into a ring of three register sets; the step loop is unrolled by
  // three so that no set is ever copied (lstm_mx.hip)
  float4 xc[3], xn[3], xnn[3];
  const float* xrow = F == 0 ? a.x + ((size_t)bc * T * 2 + dir) * RV_GG + u0 : nullptr;    // + t * 768 + g * 128
  if (F == 0) {
    const int t0 = dir ? T - 1 : 0, t1 = dir ? max(T - 2, 0) : min(1, T - 1);
#pragma unroll
    for (int g = 0; g < 3; ++g) xc[g] = *reinterpret_cast<const float4*>(xrow + (size_t)t0 * (2 * RV_GG) + g * RV_U);
#pragma unroll
    for (int g = 0; g < 3; ++g) xn[g] = *reinterpret_cast<const float4*>(xrow + (size_t)t1 * (2 * RV_GG) + g * RV_U);
  }
  __syncthreads();

  int cur = 0;
  auto step = [&](int s, const float4 (&xu)[3], float4 (&xl)[3]) {
    const int t = dir ? T - 1 - s : s;
    if (F == 0) {                                                // the inputs of step s + 2: in flight across two barriers
      const int tn = dir ? max(t - 2, 0) : min(t + 2, T - 1);
#pragma unroll
      for (int g = 0; g < 3; ++g) xl[g] = *reinterpret_cast<const float4*>(xrow + (size_t)tn * (2 * RV_GG) + g * RV_U);
    }
    f4v acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f4v{0.f, 0.f, 0.f, 0.f};
    {
      const char* hp = hb + cur * 8192 + (q * 16 + n) * 16;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const h8 bh = *reinterpret_cast<const h8*>(hp + ks * 1024), bl = *reinterpret_cast<const h8*>(hp + 4096 + ks * 1024);
        // the three gates in turns for each part product: an MFMA accumulates onto a result that is three instructions old
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][0]), bl, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][1]), bh, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][0]), bh, acc[g], 0, 0, 0);
      }
    }
    // ---- the two halves of every gate's pre-activation for this lane's four units: xi = x . W + b[0], hr = h . U + b[1]
    float xi[3][4], hr[3][4];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const float4 ds = *reinterpret_cast<const float4*>(&dss[g * RV_U + u0]);
      const float4 bb = *reinterpret_cast<const float4*>(&b1s[g * RV_U + u0]);
      float4 xin;
      if (F == 0) xin = xu[g];
      else {                                                     // b[0] + sum_f x_f w_f, features in order
#pragma unroll
        for (int f = 0; f < F; ++f) {
          const float xv = xs[(n * T + t) * F + f];
          const float4 wv = *reinterpret_cast<const float4*>(&wxs[f * RV_GG + g * RV_U + u0]);
          if (f == 0) xin = *reinterpret_cast<const float4*>(&wxs[F * RV_GG + g * RV_U + u0]);
          xin.x = fmaf(xv, wv.x, xin.x); xin.y = fmaf(xv, wv.y, xin.y); xin.z = fmaf(xv, wv.z, xin.z); xin.w = fmaf(xv, wv.w, xin.w);
        }
      }
      xi[g][0] = xin.x; xi[g][1] = xin.y; xi[g][2] = xin.z; xi[g][3] = xin.w;
      hr[g][0] = fmaf(acc[g][0], ds.x, bb.x); hr[g][1] = fmaf(acc[g][1], ds.y, bb.y);
      hr[g][2] = fmaf(acc[g][2], ds.z, bb.z); hr[g][3] = fmaf(acc[g][3], ds.w, bb.w);
    }
    h4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float z = rv_sigmoid(xi[0][i] + hr[0][i]);
      const float r = rv_sigmoid(xi[1][i] + hr[1][i]);
      const float hh = rv_tanh(fmaf(r, hr[2][i], xi[2][i]));     // the reset gate multiplies the recurrent part alone (reset_after)
      const float hn = fmaf(z, hl[i] - hh, hh);                  // z h + (1 - z) hh
      hl[i] = hn;
      const float sv = hn * 16384.f;
      hi[i] = (_Float16)sv; lo[i] = (_Float16)(sv - (float)hi[i]);
    }
    {
      char* dst = hb + (cur ^ 1) * 8192 + ((2 * w + (q >> 1)) * 16 + n) * 16 + (q & 1) * 8;
      *reinterpret_cast<h4*>(dst) = hi; *reinterpret_cast<h4*>(dst + 4096) = lo;
    }
    if (live) *reinterpret_cast<float4*>(a.out + ((size_t)(b0 + n) * a.out_T + a.out_t0 + t) * RV_E + dir * RV_U + u0) = make_float4(hl[0], hl[1], hl[2], hl[3]);
    cur ^= 1;
    RV_GRU_BARRIER();
  };
  // whole triples in the loop, the one or two steps that are left after it (lstm_mx.hip: a conditional step inside the loop drains the
  // vector-memory counter at the loop header)
  int s = 0;
  for (; s + 2 < T; s += 3) {
    step(s, xc, xnn);
    step(s + 1, xn, xc);
    step(s + 2, xnn, xn);
  }
  if (s < T) {
    step(s, xc, xnn);
    if (s + 1 < T) step(s + 1, xn, xc);
  }
  if (live) *reinterpret_cast<float4*>(a.hT[dir] + (size_t)(b0 + n) * RV_U + u0) = make_float4(hl[0], hl[1], hl[2], hl[3]);
}

// the instantiations of k_gru_rec_mx, (F, CH): adding or removing a form is this one line
template <int F_, int CH_> struct GruForm { static constexpr int F = F_, CH = CH_; };
template <typename Fn> void for_each_gru_form(Fn&& fn) { fn(GruForm<0, 16>{}); fn(GruForm<1, 16>{}); fn(GruForm<5, 16>{}); }

constexpr size_t gru_lds_bytes(int F, int T) { return 16384 + sizeof(float) * ((size_t)2 * RV_GG + (F > 0 ? (size_t)(F + 1) * RV_GG + (size_t)RV_MX_ROWS * T * F : 0)); }

// D1g -- the decoder GRU cell of the per-step decode (see the head of this file).  Workgroup = 64 beam rows x 16 units x 4 column tiles,
// K = 256 in one shot; panels, barrier and MFMA loop are k_dec_cell's.  Reads h from the h half of its xh rows, writes h_new and the
// next cell's input half; the c buffers are not touched.
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int GCELL_LD = 260;                      // padded row length of the LDS panels (floats)
constexpr int GCELL_ROWS = 64;
constexpr int GCELL_LDS_FLOATS = (GCELL_ROWS + 64) * GCELL_LD + 4 * GCELL_ROWS * 17;
__global__ __launch_bounds__(512) void k_dec_cell_gru(DecState d, int layer, const float* __restrict__ WcatT /*[512,256]: tiles z, r, [W_h;0], [0;U_h]*/,
                                                      const float* __restrict__ Wtok /*[V,384]*/, const float* __restrict__ bias /*[2,384]*/,
                                                      int step) {
  if (step > 0 && d.nfin[step - 1] >= d.B) return;
  const float* xh_l = d.xh + layer * d.ls_xh;
  float* hn_l = d.h_new + layer * d.ls_c;
  float* xh_up = layer + 1 < d.depth ? d.xh + (layer + 1) * d.ls_xh : nullptr;   // next cell's input half
  extern __shared__ __align__(16) float gcsm[];
  float* As = gcsm;                                 // [64 rows][260]
  float* Bs = gcsm + GCELL_ROWS * GCELL_LD;         // [64 cols = 4 tiles x 16 units][260]
  float* zs = gcsm + (GCELL_ROWS + 64) * GCELL_LD;  // [4 tiles][64 rows][17]
  const int N = d.B * d.W;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r0 = blockIdx.y * GCELL_ROWS, u0 = blockIdx.x * 16;
  // epilogue operands first (their round trips hide under the panel loads): thread = 2 x (row, unit)
  int en[2]; float eh[2], ew[2][3];
  const int eun = tid & 15, ecol = u0 + eun;
  const float bz = bias[ecol] + bias[RV_GG + ecol], br = bias[RV_U + ecol] + bias[RV_GG + RV_U + ecol];
  const float bxh = bias[2 * RV_U + ecol], bhh = bias[RV_GG + 2 * RV_U + ecol];
  int etok[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    en[p] = min(r0 + (tid >> 4) + 32 * p, N - 1);
    etok[p] = Wtok ? d.tok[en[p]] : 0;
    eh[p] = xh_l[(size_t)en[p] * RV_E + RV_U + ecol];
  }
  float4 ra[8], rb[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int idx = tid + 512 * p, row = idx >> 6, c4 = idx & 63;        // 64 float4 per 1 KB row
    const int n = min(r0 + row, N - 1);
    ra[p] = *reinterpret_cast<const float4*>(xh_l + (size_t)n * RV_E + 4 * c4);
    const int col = (row >> 4) * RV_U + u0 + (row & 15);                 // panel row = tile*16 + unit
    rb[p] = *reinterpret_cast<const float4*>(WcatT + (size_t)col * RV_E + 4 * c4);
  }
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int idx = tid + 512 * p, row = idx >> 6, c4 = idx & 63;
    *reinterpret_cast<float4*>(As + row * GCELL_LD + 4 * c4) = ra[p];
    *reinterpret_cast<float4*>(Bs + row * GCELL_LD + 4 * c4) = rb[p];
  }
#pragma unroll
  for (int p = 0; p < 2; ++p)       // one-hot row gather into the input part (z, r, xi_h); an id outside the vocabulary adds no row
#pragma unroll
    for (int gg = 0; gg < 3; ++gg)
      ew[p][gg] = (Wtok && (unsigned)etok[p] < (unsigned)d.V) ? Wtok[(size_t)etok[p] * RV_GG + gg * RV_U + ecol] : 0.f;
  __syncthreads();
  const int rq = wv & 3, gh = wv >> 2;            // wave = 16-row quarter x tile pair
  const int li = lane & 15, kq = lane >> 4;       // lane group kq supplies k in [64kq, 64kq+64)
  const float4* ap = reinterpret_cast<const float4*>(As + (16 * rq + li) * GCELL_LD + 64 * kq);
#pragma unroll
  for (int gi = 0; gi < 2; ++gi) {
    const int g = 2 * gh + gi;
    const float4* bp = reinterpret_cast<const float4*>(Bs + (16 * g + li) * GCELL_LD + 64 * kq);
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
    for (int r = 0; r < 4; ++r) zs[(g * GCELL_ROWS + 16 * rq + 4 * kq + r) * 17 + li] = acc0[r] + acc1[r];
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int row = (tid >> 4) + 32 * p;
    if (r0 + row < N) {
      const float z = rv_sigmoid(zs[(0 * GCELL_ROWS + row) * 17 + eun] + ew[p][0] + bz);
      const float r = rv_sigmoid(zs[(1 * GCELL_ROWS + row) * 17 + eun] + ew[p][1] + br);
      const float xih = zs[(2 * GCELL_ROWS + row) * 17 + eun] + ew[p][2] + bxh;
      const float hrh = zs[(3 * GCELL_ROWS + row) * 17 + eun] + bhh;
      const float hh = rv_tanh(fmaf(r, hrh, xih));
      const float hn = fmaf(z, eh[p] - hh, hh);
      hn_l[(size_t)en[p] * RV_U + ecol] = hn;
      if (xh_up) xh_up[(size_t)en[p] * RV_E + ecol] = hn;
    }
  }
}

}  // namespace

void list_gru_forms(FormLog& log) {
  for_each_gru_form([&](auto form) { using M = decltype(form); log.add(RV_K_GRU_REC_MX, M::F, M::CH); });
  log.add(RV_K_DEC_CELL_GRU, 0);
}

bool gru_rec_mx_window_fits(int T, int F) { return gru_lds_bytes(F, T) <= 160 * 1024; }

hipError_t configure_gru_kernels() {
  hipError_t first = hipSuccess;
  for_each_gru_form([&](auto form) {
    using M = decltype(form);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gru_rec_mx<M::F, M::CH>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess && first == hipSuccess) first = e;
  });
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dec_cell_gru), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           GCELL_LDS_FLOATS * (int)sizeof(float));
  return first != hipSuccess ? first : e;
}

void launch_gru_rec_mx(const GruRecArgs& a, int F, hipStream_t s, FormLog* log) {
  for_each_gru_form([&](auto form) {
    using M = decltype(form);
    if (M::F == F) {
      const dim3 grid((a.B + M::CH - 1) / M::CH, 2);
      hipLaunchKernelGGL((k_gru_rec_mx<M::F, M::CH>), grid, dim3(512), gru_lds_bytes(M::F, a.T), s, a);
      if (log) log->add(RV_K_GRU_REC_MX, M::F, M::CH);
    }
  });
}

void launch_dec_cell_gru(const DecState& d, int layer, const float* WcatT, const float* Wtok, const float* bias, int step, hipStream_t s,
                         FormLog* log) {
  const int N = d.B * d.W;
  hipLaunchKernelGGL(k_dec_cell_gru, dim3(RV_U / 16, (N + GCELL_ROWS - 1) / GCELL_ROWS), dim3(512), GCELL_LDS_FLOATS * sizeof(float), s, d, layer,
                     WcatT, Wtok, bias, step);
  if (log) log->add(RV_K_DEC_CELL_GRU, 0);
}
