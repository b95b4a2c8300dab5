// K1m -- the BiLSTM recurrence on the 16-bit matrix pipe, SIXTEEN chunks per workgroup (replaces the tf.while_loop of LSTMCell
// steps that Encoder.call drives: /root/reference/basecaller.py:19-32,48-59; cell math SURVEY.md A.1/A.2).
//
// The packed-FMA kernels of lstm_rec.hip cost the same per chunk-row however many rows a workgroup holds (2,390 cycles per
// step for 2 rows, 8,400 for 8): they are bound by fp32 FMA issue.  Here the recurrent product of a step is ONE matrix
// product per workgroup, z^T [512 gate columns x 16 chunks] = U^T [512 x 128] . h^T [128 x 16], on v_mfma_f32_16x16x32_f16 with
// split operands (two f16 parts per value, three exact part products, f32 accumulation: DESIGN.md section 4) -- its cost does
// not depend on how many of the 16 columns are in use, so a workgroup takes 16 chunks of ONE direction:
//   * U^T stays resident as A fragments: wave w owns units 16 w .. 16 w + 15 of all four gates = 4 row tiles x 4 k-steps x
//     2 parts x 4 VGPRs = 128 VGPRs (the whole kernel, 256 KB, in the register file of the CU -- as the FMA kernels keep it);
//   * h^T goes through LDS as B fragments: [part][k-block of 8 units][chunk][8 f16], double-buffered, 1 KB per wave read;
//   * the C/D layout of the 16x16 tile gives lane (chunk n = lane % 16, q = lane / 16) the four gate sums of units
//     16 w + 4 q + 0..3 of chunk n: the cell update is local to the lane (no reduction, no gather, no tail waves), c stays in 4
//     registers, and the new h leaves as one float4 to the layer output and as 4 + 4 f16 to the LDS image;
//   * one raw s_barrier per step (LDS hand-off only: the next step's pre-projected inputs stay in flight across it).
// Scales: h' = 2^14 h (|h| <= 1), U' = s_r U with s_r the power of two that brings the largest element of gate column r into
// [2^13, 2^14); z = acc * (2^-14 / s_r) + (x . W + b).  Layer 0 with one input feature (raw samples) adds x_t W + b in the lane from
// an LDS-staged window; every other layer reads its pre-projected inputs xw [B,T,2,512] (event layer 0: k_inproj_small; layers
// >= 1: the split-f16 GEMM of gemm_f32.hip), one float4 per gate per lane, requested a step ahead.
// The reverse direction walks t = T-1..0 and, as in the reference (no mask is passed, basecaller.py:400,403), starts on the padding.
//
// CH = 8 (round 4; the per-call choice `wide_recurrence = -1` takes it for slabs that leave the chip idle): EIGHT chunks per workgroup for
// latency.  The product's 16 columns then hold both f16 PARTS of a chunk's h -- high part in column n, low part in column n + 8 -- so a
// (row tile, k-step) takes TWO MFMAs (U_hi . [h_hi | h_lo], U_lo . [h_hi | h_lo]: the three exact part products plus the low x low term,
// below 2^-22 of the product) instead of three, one LDS read instead of two; lanes n and n + 8 add their accumulators (DPP row_ror:8)
// and take two of the four units each: half the cell update per lane.  2.0 k cycles per step against 3.15 k, on twice the workgroups:
// more CU-time per chunk, which is why the streamed path keeps sixteen.  The sums associate differently: results agree with CH = 16 to
// fp32 rounding, not bit for bit.
//
// One body (rec_mx_body) serves all six forms, F in {0, 1, 5} x CH in {16, 8}.  Its sixteen-chunk code keeps round 3's wording, because
// the default path's <0, 16> and <1, 16> compile to round 3's instruction stream only with it: float4 state loads and stores, x_t w + b
// loaded in that order, the f16 parts of h split inside the cell update, the lane's chunk n as the one variable the step and the h image
// read, the mask test of the staged inputs inside its branch.  (Round 4 had kept a second, generic body for the other forms; it ran the
// default forms 1-3 % slower on the same box, same inputs -- 0.3945 -> 0.3990 ms for raw layer 0, 0.4035 -> 0.4155 for layer 1 -- the
// scheduling differed, not the work.)
#include <type_traits>

#include "common.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));

#define RV_MX_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)

template <int NU>                                                // NU floats as one vector: a single 8- / 16-byte store
__device__ __forceinline__ auto vec(const float (&v)[NU]) {
  if constexpr (NU == 2) return make_float2(v[0], v[1]);
  else return make_float4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ float ror8_add(float v) {           // v + (v of the lane 8 apart in this 16-lane row)
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, false));
}

// Where the staging prologue of a layer-0 form finds its chunks' inputs: rows of one chunk tensor, rows of the members' own tensors
// (a coalesced call, RecArgs::members), or windows of reads (RecArgs::windows)
enum { SRC_TENSOR = 0, SRC_MEMBERS = 1, SRC_WINDOWS = 2 };

template <int F, int CH, int SRC = SRC_TENSOR>
__device__ __forceinline__ void rec_mx_body(const RecArgs& a) {
  static_assert(F == 0 || F == 1 || F == 5, "pre-projected inputs, or layer 0 on its F input features (raw samples: 1; events: 5)");
  static_assert(CH == 16 || CH == 8, "sixteen chunks per workgroup, or eight with both parts of h in the product's columns");
  constexpr bool C8 = CH == 8;
  constexpr int NU = C8 ? 2 : 4;                                 // units per lane
  using fv = std::conditional_t<C8, float2, float4>;             // a lane's NU units: one 8- / 16-byte access
  typedef _Float16 hv __attribute__((ext_vector_type(NU)));      // the same NU units as f16: one part of the h image
  extern __shared__ __align__(16) char mxsm[];
  char* hb = mxsm;                                               // [2 buffers][2 parts][16 k-blocks][16 chunks][8 f16] = 16 KB  (CH = 8: [2][16 k-blocks][8 high | 8 low columns][8 f16])
  float* dss = reinterpret_cast<float*>(mxsm + 16384);           // [512] 2^-14 / s_r
  float* wxs = dss + RV_G;                                       // F > 0: [F][512] input kernel rows, [512] bias
  float* xs = wxs + (F + 1) * RV_G;                              // F > 0: [CH][T][F] input windows

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & (CH - 1), q = lane >> 4;
  const int hs = C8 ? (lane >> 3) & 1 : 0;                       // CH = 8: which half of the four units (and: high / low column)
  const int dir = blockIdx.y, b0 = blockIdx.x * CH, T = a.T;
  const int bc = min(b0 + n, a.B - 1);                           // rows beyond the slab compute on a copy of its last chunk, never stored
  const bool live = b0 + n < a.B;
  const int u0 = 16 * w + 4 * q + 2 * hs;                        // this lane's NU units

  // ---- U^T -> registers (A fragments), once
  float4 ua[4][4][2];
  {
    const float4* src = reinterpret_cast<const float4*>(a.Ua[dir]) + (size_t)w * (4 * 4 * 2 * 64) + lane;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int p = 0; p < 2; ++p) ua[g][ks][p] = src[((g * 4 + ks) * 2 + p) * 64];
  }
  {
    const float* dsg = reinterpret_cast<const float*>(a.Ua[dir] + (size_t)2 * RV_U * RV_G);
    dss[tid] = dsg[tid];
    if (F > 0) {
#pragma unroll
      for (int f = 0; f < F; ++f) wxs[f * RV_G + tid] = a.W[dir][f * RV_G + tid];
      wxs[F * RV_G + tid] = a.bias[dir][tid];
      const float* xg = a.ptab ? static_cast<const float*>(a.ptab[F == 1 ? RV_PTAB_RAW : RV_PTAB_EVENT]) : a.x;     // (graph replay: the caller's address of this call)
      for (int r = 0; r < CH; ++r) {
        const int b = min(b0 + r, a.B - 1);
        const bool wm = a.mask && dir == 0 && b0 + r < a.B;     // utils.input_mask of this encoder's part (utils.py:26-32: all features != pad), once per chunk
        const float* xb = xg;
        int br = b;
        if constexpr (SRC == SRC_WINDOWS) {    // chunk b is a window of a read: len real positions from the read's table, the padding value behind them.
                                // The host has checked the window against its read and len <= T (resolve_windows); scalar 4-byte loads: a
                                // window starts at any float offset.  The mask is the chunk tensor's: every feature != pad, so 0 beyond len
          const RecWindow wr = a.windows[b];
          const float* wp = F == 1 ? wr.raw : wr.ev;
          const int len = F == 1 ? wr.raw_len : wr.ev_len;
          for (int i = tid; i < T; i += 512) {
            float v[F];
#pragma unroll
            for (int f = 0; f < F; ++f) v[f] = i < len ? wp[(size_t)i * F + f] : a.pad;
#pragma unroll
            for (int f = 0; f < F; ++f) xs[(r * T + i) * F + f] = v[f];
            if (wm) {
              bool real = true;
#pragma unroll
              for (int f = 0; f < F; ++f) real = real && v[f] != a.pad;
              a.mask[(size_t)b * a.mask_T + a.mask_t0 + i] = real ? 1 : 0;
            }
          }
          continue;
        }
        if constexpr (SRC == SRC_MEMBERS) {    // chunk b is a row of its member's own tensor (a workgroup's chunks may straddle members, so per chunk; scalar
                                // 4-byte loads below: a member's tensor may sit at any float offset)
          for (int m = 0; m < a.members.n; ++m)
            if (b >= a.members.row0[m] && b < a.members.row0[m] + a.members.rows[m]) { xb = a.members.x[m]; br = b - a.members.row0[m]; }
        }
        for (int i = tid; i < T; i += 512) {
          const float* v = xb + ((size_t)br * T + i) * F;
#pragma unroll
          for (int f = 0; f < F; ++f) xs[(r * T + i) * F + f] = v[f];
          if (wm) {
            bool real = true;
#pragma unroll
            for (int f = 0; f < F; ++f) real = real && v[f] != a.pad;
            a.mask[(size_t)b * a.mask_T + a.mask_t0 + i] = real ? 1 : 0;
          }
        }
      }
    }
  }
  // ---- initial state: c in registers, h as the first B image.  A lane writes its NU units of chunk n as f16 parts; CH = 16: [part][k-block]
  // [chunk][8]; CH = 8: [k-block][column][8] with the high part in column n and the low part in column n + 8
  float c[NU];
  {
    fv h0{0.f}, c0{0.f};
    if (a.h0[dir]) { h0 = *reinterpret_cast<const fv*>(a.h0[dir] + (size_t)bc * RV_U + u0); c0 = *reinterpret_cast<const fv*>(a.c0[dir] + (size_t)bc * RV_U + u0); }
    hv hi, lo;
#pragma unroll
    for (int i = 0; i < NU; ++i) { c[i] = c0[i]; const float sv = h0[i] * 16384.f; hi[i] = (_Float16)sv; lo[i] = (_Float16)(sv - (float)hi[i]); }
    char* dst = hb + ((2 * w + (q >> 1)) * 16 + n) * 16 + (q & 1) * 8 + hs * 4;
    *reinterpret_cast<hv*>(dst) = hi; *reinterpret_cast<hv*>(dst + (C8 ? 8 * 16 : 4096)) = lo;
  }
  // pre-projected inputs: the loads of step s + 2 are issued in step s (one step, ~1.3 us, is less than an HBM round trip under
  // load) into a ring of three register sets; the step loop is unrolled by three so that no set is ever COPIED -- a register
  // move from a load's destination waits for the load, which is what made a "prefetch" into a staging set synchronous
  fv xc[4], xn[4], xnn[4];
  const float* xrow = F == 0 ? a.x + ((size_t)bc * T * 2 + dir) * RV_G + u0 : nullptr;    // + t * 1024 + g * 128
  if (F == 0) {
    const int t0 = dir ? T - 1 : 0, t1 = dir ? max(T - 2, 0) : min(1, T - 1);
#pragma unroll
    for (int g = 0; g < 4; ++g) xc[g] = *reinterpret_cast<const fv*>(xrow + (size_t)t0 * (2 * RV_G) + g * RV_U);
#pragma unroll
    for (int g = 0; g < 4; ++g) xn[g] = *reinterpret_cast<const fv*>(xrow + (size_t)t1 * (2 * RV_G) + g * RV_U);
  }
  __syncthreads();

  float hl[NU] = {};
  int cur = 0;
  // diagnostic (RV_REC_STAMPS, tools/rec_stamps.py): cycle sums of workgroup (0, 0), wave 0 over all steps: [0] top of step -> gate sums in
  // registers, [1] -> cell update done, [2] -> LDS image and output store issued, [3] -> behind the barrier
#ifdef RV_MX_STAMPS      // diagnostic builds only (make mxvar V=1 MXFLAGS=-DRV_MX_STAMPS; RAVVENT_HIP_LIB=...libravvent_hip_m1.so): four scalar branches per step otherwise
  const bool stamp = a.dbg_ts != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0;
#else
  constexpr bool stamp = false;
#endif
  long long st_sum[4] = {0, 0, 0, 0};
  auto step = [&](int s, const fv (&xu)[4], fv (&xl)[4]) {
    const int t = dir ? T - 1 - s : s;
    long long st0 = 0;
    if (stamp) st0 = __builtin_readcyclecounter();
    if (F == 0) {                                                // the inputs of step s + 2: in flight across two barriers
      const int tn = dir ? max(t - 2, 0) : min(t + 2, T - 1);
#pragma unroll
      for (int g = 0; g < 4; ++g) xl[g] = *reinterpret_cast<const fv*>(xrow + (size_t)tn * (2 * RV_G) + g * RV_U);
    }
    f4v acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f4v{0.f, 0.f, 0.f, 0.f};
    if constexpr (C8) {
      const char* hp = hb + cur * 4096 + (q * 16 + (lane & 15)) * 16;   // column lane % 16: chunk n, high (hs = 0) or low part
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const h8 bb = *reinterpret_cast<const h8*>(hp + ks * 1024);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][1]), bb, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][0]), bb, acc[g], 0, 0, 0);
      }
    } else {
      const char* hp = hb + cur * 8192 + (q * 16 + n) * 16;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const h8 bh = *reinterpret_cast<const h8*>(hp + ks * 1024), bl = *reinterpret_cast<const h8*>(hp + 4096 + ks * 1024);
        // the four gates in turns for each part product: an MFMA accumulates onto a result that is four instructions old, not onto the one
        // issued just before it (per accumulator the order of the additions is unchanged: identical results)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][0]), bl, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][1]), bh, acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][0]), bh, acc[g], 0, 0, 0);
      }
    }
    // ---- gate pre-activations of this lane's NU units, cell update (i, f, c~, o)
    float z[4][NU];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float sacc[NU];
      if constexpr (C8) {                                        // columns n and n + 8 = [U . h_hi] and [U . h_lo] of one chunk: add; this lane keeps units 2 hs, + 1
        const float s0 = ror8_add(acc[g][0]), s1 = ror8_add(acc[g][1]), s2 = ror8_add(acc[g][2]), s3 = ror8_add(acc[g][3]);
        sacc[0] = hs ? s2 : s0; sacc[1] = hs ? s3 : s1;
      } else {
#pragma unroll
        for (int i = 0; i < NU; ++i) sacc[i] = acc[g][i];
      }
      const fv ds = *reinterpret_cast<const fv*>(&dss[g * RV_U + u0]);
      fv xin;
      if (F == 0) xin = xu[g];
      else {                                                     // b + sum_f x_f w_f, features in order (the same additions as k_inproj_small: identical bits)
#pragma unroll
        for (int f = 0; f < F; ++f) {
          const float xv = xs[(n * T + t) * F + f];
          const fv wv = *reinterpret_cast<const fv*>(&wxs[f * RV_G + g * RV_U + u0]);
          if (f == 0) xin = *reinterpret_cast<const fv*>(&wxs[F * RV_G + g * RV_U + u0]);
#pragma unroll
          for (int i = 0; i < NU; ++i) xin[i] = fmaf(xv, wv[i], xin[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < NU; ++i) z[g][i] = fmaf(sacc[i], ds[i], xin[i]);
    }
    if (stamp) { asm volatile("" :: "v"(z[0][0]), "v"(z[3][NU - 1])); const long long tn = __builtin_readcyclecounter(); st_sum[0] += tn - st0; st0 = tn; }
    hv hi, lo;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      // (Round 4 tried this update on 7 transcendentals instead of 10 -- c' and h' each as ONE reciprocal of a product of (1 + 2^x) terms --
      //  parity-green and no faster: 0.394 / 0.424 ms per C3 layer either way.  The step is bound by the SIMD's issue with both of its waves
      //  in the same phase -- tools/mx_stamps.py: 1.24 k cycles of MFMA phase + 1.0 k of cell update + 0.26 k + 0.7 k at the barrier -- and a
      //  two-group form that interleaves one group's MFMAs with the other's cell update inside every wave did not overlap them either
      //  (DESIGN.md section 7).)
      const float cc = fmaf(rv_sigmoid(z[1][i]), c[i], rv_sigmoid(z[0][i]) * rv_tanh(z[2][i]));
      const float hh = rv_sigmoid(z[3][i]) * rv_tanh(cc);
      c[i] = cc; hl[i] = hh;
      const float sv = hh * 16384.f;
      hi[i] = (_Float16)sv; lo[i] = (_Float16)(sv - (float)hi[i]);
    }
    if (stamp) { asm volatile("" :: "v"(hl[0]), "v"(hl[NU - 1])); const long long tn = __builtin_readcyclecounter(); st_sum[1] += tn - st0; st0 = tn; }
    {
      char* dst = hb + (cur ^ 1) * (C8 ? 4096 : 8192) + ((2 * w + (q >> 1)) * 16 + n) * 16 + (q & 1) * 8 + hs * 4;
      *reinterpret_cast<hv*>(dst) = hi; *reinterpret_cast<hv*>(dst + (C8 ? 8 * 16 : 4096)) = lo;
    }
    if (live) *reinterpret_cast<fv*>(a.out + ((size_t)(b0 + n) * a.out_T + a.out_t0 + t) * RV_E + dir * RV_U + u0) = vec(hl);
    cur ^= 1;
    if (stamp) { const long long tn = __builtin_readcyclecounter(); st_sum[2] += tn - st0; st0 = tn; }
    RV_MX_BARRIER();
    if (stamp) { const long long tn = __builtin_readcyclecounter(); st_sum[3] += tn - st0; }
  };
  // whole triples in the loop, the one or two steps that are left after it: a conditional step INSIDE the loop makes the compiler merge
  // two histories of pending loads / stores at the loop header, and it then drains the vector-memory counter there (`s_waitcnt vmcnt(0)`
  // once per three steps: the wave waited for the previous step's output store and for inputs it had requested one step earlier)
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
  if (stamp) { for (int i = 0; i < 4; ++i) a.dbg_ts[i] = st_sum[i]; a.dbg_ts[4] = T; }
  if (live) {
    *reinterpret_cast<fv*>(a.hT[dir] + (size_t)(b0 + n) * RV_U + u0) = vec(hl);
    *reinterpret_cast<fv*>(a.cT[dir] + (size_t)(b0 + n) * RV_U + u0) = vec(c);
  }
}

template <int F, int CH>
__global__ __launch_bounds__(512) void k_lstm_rec_mx(RecArgs a) { rec_mx_body<F, CH>(a); }

// The layer-0 forms (F > 0) for a coalesced call whose members' inputs stay where their callers hold them (RecArgs::members): the same body,
// with the staging prologue resolving each chunk to its member's tensor.  Instantiations of their own, so that the step loops of the forms
// above keep their instruction stream (the head of this file); they are logged as the (F, CH) form they are.
template <int F, int CH>
__global__ __launch_bounds__(512) void k_lstm_rec_mx_members(RecArgs a) { rec_mx_body<F, CH, SRC_MEMBERS>(a); }

// ... and for a call whose chunks are windows of reads (RecArgs::windows; a coalesced group of such calls too: its table is its
// members' rows back to back, so no member lookup).  Logged as the (F, CH) form they are.
template <int F, int CH>
__global__ __launch_bounds__(512) void k_lstm_rec_mx_windows(RecArgs a) { rec_mx_body<F, CH, SRC_WINDOWS>(a); }

// ---------------------------------------------------------------------------------------------------------------------------------
// The PROJECTING form for layers >= 1 (option fused_inproj): the sixteen-chunk recurrence computes x_t . W + b itself, on its own MFMAs,
// from the previous layer's output act [B*T, 256] -- no k_gemm_ws launch and no xw [B,T,2,512] round trip through HBM (315 MB written and
// read back per C3 raw layer).  A body of its own, so that the six forms above keep their instruction streams.
//   * The split GEMM issues mfma(weight fragment, activation fragment): lane (chunk n, q) of its transposed tile ends with gate columns
//     16 nt + 4 q + 0..3 of row n -- with nt = w, column block cb = 2 dir + g / 2 and half hb = g & 1 that IS the recurrence's C/D map
//     (units 16 w + 4 q + 0..3 of gate g).  Wave w's projection of a timestep leaves in every lane the 16 floats the lane adds to its
//     gate sums: no LDS block, no exchange.  The (k-step, gate) fragment pair of wave w is 2 KB contiguous in the GEMM's own image Wx16,
//     at cb 262144 + ks 32768 + hb 16384 + (2 w + part) 1024 + lane 16; the column factors follow the image, the biases are bx2.
//   * TWO timesteps per pass (MXP_NT): in front of every pair of steps one pass projects the pair's two timesteps (in walking order) into
//     32 registers, where the form <0, 16> keeps its ring of pre-projected inputs; each streamed weight fragment meets two activation
//     fragments: 512 KB from L2 per pass and workgroup, 256 KB per step.  (Three per pass -- 48 accumulators, 171 KB per step -- do not fit
//     beside U's 128 registers without scratch: 36 to 212 B per lane in every schedule tried, profiles/fused_inproj.md.)
//   * The activations reach the pass as B fragments of two f16 parts (the GEMM's split: sv = 2^14 v, hi = f16(sv), lo = f16(sv - hi)) in
//     LDS, [2 buffers][2 timesteps][2 parts][32 k-blocks of 8][16 chunks][8 f16] = 2 x 32 KB, converted once per workgroup: thread
//     (chunk tid % 16, k-block tid / 16) moves eight floats per timestep.  Step s converts the row of walking position s + 2, requested
//     one step earlier (eight registers in flight, across the pass too), into the next pass's buffer and requests position s + 3: every
//     request has a whole step or more to come back from HBM, and a pass's two timesteps are in LDS behind the barrier of the step before it.
//   * Every xin element keeps k_gemm_ws's chain -- k in eight steps of 32, per step w_lo a_hi, w_hi a_lo, w_hi a_hi into one f32
//     accumulator, then fmaf(acc, column factor, bias) -- and the step is the one above: the results are those of the two launches bit
//     for bit (tests/test_fused_inproj_gpu.py), which is what lets a call choose the form.
// RecArgs: x = act [B*T, 256], Wh[0] = the layer's Wx16 image (both directions), bias[0] = its bx2 [1024]; Ua, h0 .. cT, out as above.
constexpr int MXP_NT = 2;                                         // timesteps per projection pass
constexpr int MXP_FRAG = MXP_NT * 2 * 32 * 16 * 16;               // one fragment buffer: 16 KB per timestep
constexpr int MXP_LDS = 16384 + 3 * RV_G * (int)sizeof(float) + 2 * MXP_FRAG;
constexpr int MXP_RING = 3;                                       // (k-step, gate) weight fragment pairs in flight per wave (four: 16 B of scratch)

__global__ __launch_bounds__(512) void k_lstm_rec_mx_proj(RecArgs a) {
  extern __shared__ __align__(16) char mxsm[];
  char* hb = mxsm;                                               // the h image, as above
  float* dss = reinterpret_cast<float*>(mxsm + 16384);           // [512] 2^-14 / s_r
  float* css = dss + RV_G;                                       // [512] the projection's column factors of this direction
  float* bss = css + RV_G;                                       // [512] ... and its biases
  char* frag = mxsm + 16384 + 3 * RV_G * sizeof(float);          // the two fragment buffers

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, q = lane >> 4;
  const int dir = blockIdx.y, b0 = blockIdx.x * 16, T = a.T;
  const int bc = min(b0 + n, a.B - 1);                           // rows beyond the slab compute on a copy of its last chunk, never stored
  const bool live = b0 + n < a.B;
  const int u0 = 16 * w + 4 * q;

  float4 ua[4][4][2];
  {
    const float4* src = reinterpret_cast<const float4*>(a.Ua[dir]) + (size_t)w * (4 * 4 * 2 * 64) + lane;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int p = 0; p < 2; ++p) ua[g][ks][p] = src[((g * 4 + ks) * 2 + p) * 64];
  }
  const char* img = reinterpret_cast<const char*>(a.Wh[0]);
  {
    const float* dsg = reinterpret_cast<const float*>(a.Ua[dir] + (size_t)2 * RV_U * RV_G);
    dss[tid] = dsg[tid];
    css[tid] = reinterpret_cast<const float*>(img + (size_t)4 * 262144)[dir * RV_G + tid];
    bss[tid] = a.bias[0][dir * RV_G + tid];
  }
  float c[4];
  {
    float4 h0{0.f, 0.f, 0.f, 0.f}, c0{0.f, 0.f, 0.f, 0.f};
    if (a.h0[dir]) { h0 = *reinterpret_cast<const float4*>(a.h0[dir] + (size_t)bc * RV_U + u0); c0 = *reinterpret_cast<const float4*>(a.c0[dir] + (size_t)bc * RV_U + u0); }
    const float hv0[4] = {h0.x, h0.y, h0.z, h0.w}, cv0[4] = {c0.x, c0.y, c0.z, c0.w};
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    h4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) { c[i] = cv0[i]; const float sv = hv0[i] * 16384.f; hi[i] = (_Float16)sv; lo[i] = (_Float16)(sv - (float)hi[i]); }
    char* dst = hb + ((2 * w + (q >> 1)) * 16 + n) * 16 + (q & 1) * 8;
    *reinterpret_cast<h4*>(dst) = hi; *reinterpret_cast<h4*>(dst + 4096) = lo;
  }
  // ---- the staging role of this thread: eight floats (one lane's share of a B fragment) of chunk tid % 16, k-block tid / 16
  // (addresses as a workgroup-uniform 64-bit base + a 32-bit lane offset: a register less each than a 64-bit lane pointer, which this kernel has not got)
  const float* abase = a.x + (size_t)b0 * T * RV_E;
  const unsigned aoff = (unsigned)(min(b0 + (tid & 15), a.B - 1) - b0) * (unsigned)T * RV_E + (tid >> 4) * 8;
  float* obase = a.out + ((size_t)b0 * a.out_T + a.out_t0) * RV_E + dir * RV_U;
  const unsigned ooff = (unsigned)n * (unsigned)a.out_T * RV_E + u0;
  auto trow = [&](int s) { s = min(s, T - 1); return dir ? T - 1 - s : s; };      // the timestep of walking position s (past the end: the last one again)
  auto split_store = [&](const float4& x0, const float4& x1, char* dst) {
    const float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float sv = v[j] * 16384.f; hi[j] = (_Float16)sv; lo[j] = (_Float16)(sv - (float)hi[j]); }
    *reinterpret_cast<h8*>(dst) = hi; *reinterpret_cast<h8*>(dst + 8192) = lo;
  };
#pragma unroll
  for (int j = 0; j < MXP_NT; ++j) {                             // the first pass: nothing was requested ahead
    const float* ap = abase + (size_t)trow(j) * RV_E + aoff;
    split_store(*reinterpret_cast<const float4*>(ap), *reinterpret_cast<const float4*>(ap + 4), frag + j * 16384 + tid * 16);
  }
  float4 pf[2];                                                  // the row in flight: walking position s + MXP_NT at the top of step s
  { const float* ap = abase + (size_t)trow(MXP_NT) * RV_E + aoff; pf[0] = *reinterpret_cast<const float4*>(ap); pf[1] = *reinterpret_cast<const float4*>(ap + 4); }
  __syncthreads();

  // ---- one projection pass: xa[j][g] = x_{t_j} . W + b of this lane's four units of gate g, for the MXP_NT timesteps of fragment buffer `buf`
  // (the wave's stream as a wave-uniform base + a 32-bit lane offset that the compiler must take as new in every pass: left to itself it
  //  forms the 64 fragment addresses once, in front of the step loop, and spills them)
  const char* wsrc = img + (size_t)dir * 524288 + __builtin_amdgcn_readfirstlane(w) * 2048;
  auto pass = [&](int buf, f4v (&xa)[MXP_NT][4]) {
    unsigned wo = lane * 16;
    asm volatile("" : "+v"(wo));
#pragma unroll
    for (int j = 0; j < MXP_NT; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) xa[j][g] = f4v{0.f, 0.f, 0.f, 0.f};
    const char* fb = frag + buf * MXP_FRAG + (q * 16 + n) * 16;
    h8 wr[MXP_RING][2];                                          // [slot][high part, low part]
    auto wload = [&](int p, int slot) {                          // pair p = 4 ks + g
      const char* src = wsrc + (wo + (unsigned)(((p & 3) >> 1) * 262144 + (p >> 2) * 32768 + (p & 1) * 16384));
      wr[slot][0] = *reinterpret_cast<const h8*>(src); wr[slot][1] = *reinterpret_cast<const h8*>(src + 1024);
    };
#pragma unroll
    for (int p = 0; p < MXP_RING; ++p) wload(p, p);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      h8 bh[MXP_NT], bl[MXP_NT];
#pragma unroll
      for (int j = 0; j < MXP_NT; ++j) { bh[j] = *reinterpret_cast<const h8*>(fb + j * 16384 + ks * 1024); bl[j] = *reinterpret_cast<const h8*>(fb + j * 16384 + 8192 + ks * 1024); }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int p = 4 * ks + g;
        const h8 wh = wr[p % MXP_RING][0], wl = wr[p % MXP_RING][1];
        // the MXP_NT timesteps in turns for each part product (per accumulator: w_lo a_hi, w_hi a_lo, w_hi a_hi -- k_gemm_ws's order)
#pragma unroll
        for (int j = 0; j < MXP_NT; ++j) xa[j][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, bh[j], xa[j][g], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < MXP_NT; ++j) xa[j][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, bl[j], xa[j][g], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < MXP_NT; ++j) xa[j][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, bh[j], xa[j][g], 0, 0, 0);
        if (p + MXP_RING < 32) wload(p + MXP_RING, p % MXP_RING);
        __builtin_amdgcn_sched_barrier(0);                       // (without the fences the scheduler hoists the k-step's fragment reads and the ring's loads, and spills)
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 f = *reinterpret_cast<const float4*>(&css[g * RV_U + u0]), bb = *reinterpret_cast<const float4*>(&bss[g * RV_U + u0]);
#pragma unroll
      for (int j = 0; j < MXP_NT; ++j)
        xa[j][g] = f4v{fmaf(xa[j][g][0], f.x, bb.x), fmaf(xa[j][g][1], f.y, bb.y), fmaf(xa[j][g][2], f.z, bb.z), fmaf(xa[j][g][3], f.w, bb.w)};
    }
  };

  float hl[4] = {};
  int cur = 0;
  // a step of the form <0, 16> on the pass's xin.  PF = 0, 1: the step's place in its pair -- it converts the row in flight into timestep
  // PF of the next pass's fragment buffer nbuf and requests the next row; MXP_NT: neither (the step behind the last whole pair)
  auto step = [&](int s, const f4v (&xin)[4], auto pfc, int nbuf) {
    constexpr int PF = decltype(pfc)::value;
    const int t = dir ? T - 1 - s : s;
    char* fdst = frag + nbuf * MXP_FRAG + tid * 16;
    if constexpr (PF < MXP_NT) {                                 // position s + MXP_NT is timestep PF of the next pass; position s + MXP_NT + 1 goes out
      split_store(pf[0], pf[1], fdst + PF * 16384);
      const float* ap = abase + (size_t)trow(s + MXP_NT + 1) * RV_E + aoff;
      pf[0] = *reinterpret_cast<const float4*>(ap); pf[1] = *reinterpret_cast<const float4*>(ap + 4);
    }
    f4v acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f4v{0.f, 0.f, 0.f, 0.f};
    const char* hp = hb + cur * 8192 + (q * 16 + n) * 16;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const h8 bh = *reinterpret_cast<const h8*>(hp + ks * 1024), bl = *reinterpret_cast<const h8*>(hp + 4096 + ks * 1024);
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][0]), bl, acc[g], 0, 0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][1]), bh, acc[g], 0, 0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ua[g][ks][0]), bh, acc[g], 0, 0, 0);
    }
    float z[4][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 ds = *reinterpret_cast<const float4*>(&dss[g * RV_U + u0]);
      const float dv[4] = {ds.x, ds.y, ds.z, ds.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) z[g][i] = fmaf(acc[g][i], dv[i], xin[g][i]);
    }
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    h4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float cc = fmaf(rv_sigmoid(z[1][i]), c[i], rv_sigmoid(z[0][i]) * rv_tanh(z[2][i]));
      const float hh = rv_sigmoid(z[3][i]) * rv_tanh(cc);
      c[i] = cc; hl[i] = hh;
      const float sv = hh * 16384.f;
      hi[i] = (_Float16)sv; lo[i] = (_Float16)(sv - (float)hi[i]);
    }
    {
      char* dst = hb + (cur ^ 1) * 8192 + ((2 * w + (q >> 1)) * 16 + n) * 16 + (q & 1) * 8;
      *reinterpret_cast<h4*>(dst) = hi; *reinterpret_cast<h4*>(dst + 4096) = lo;
    }
    if (live) *reinterpret_cast<float4*>(obase + (size_t)t * RV_E + ooff) = vec(hl);
    cur ^= 1;
    RV_MX_BARRIER();
  };
  // whole pairs in the loop (every one requests the rows of the next: past the end the last timestep again, which no step consumes),
  // the one step that may be left behind it -- as in rec_mx_body, no conditional step inside the loop
  f4v xa[MXP_NT][4];
  int s = 0, buf = 0;
  for (; s + 1 < T; s += 2) {
    pass(buf, xa);
    step(s, xa[0], std::integral_constant<int, 0>{}, buf ^ 1);
    step(s + 1, xa[1], std::integral_constant<int, 1>{}, buf ^ 1);
    buf ^= 1;
  }
  if (s < T) {
    pass(buf, xa);
    step(s, xa[0], std::integral_constant<int, MXP_NT>{}, 0);
  }
  if (live) {
    *reinterpret_cast<float4*>(a.hT[dir] + (size_t)(b0 + n) * RV_U + u0) = vec(hl);
    *reinterpret_cast<float4*>(a.cT[dir] + (size_t)(b0 + n) * RV_U + u0) = vec(c);
  }
}

// The padded chunk tensors of a window table for every path that reads chunk tensors (the packed-FMA recurrence, k_inproj_small, the
// tapped and profiled calls): workgroup (b, seg) writes chunk b's raw [T_r,1] (seg 0) or event [T_e,5] (seg 1) row.  The rows were
// checked on the host, like the windows kind of the recurrence; a null output is a segment the mode does not use.
__global__ __launch_bounds__(256) void k_expand_windows(const RecWindow* __restrict__ win, float* __restrict__ raw, int T_r,
                                                         float* __restrict__ ev, int T_e, float pad) {
  const int b = blockIdx.x, seg = blockIdx.y;
  const RecWindow w = win[b];
  float* out = seg ? ev : raw;
  if (!out) return;
  const int F = seg ? 5 : 1, T = seg ? T_e : T_r;
  const float* src = seg ? w.ev : w.raw;
  const int n = (seg ? w.ev_len : w.raw_len) * F;
  out += (size_t)b * T * F;
  for (int i = threadIdx.x; i < T * F; i += 256) out[i] = i < n ? src[i] : pad;
}

// x . W + b for a layer-0 encoder with a handful of input features (the event encoder: F = 5), both directions:
// xw [B*T, 2, 512].  One thread = 4 gate columns of one row; HBM-bound on its output (4 KB per chunk-timestep).
template <int F>
__global__ __launch_bounds__(256) void k_inproj_small(const float* __restrict__ x_arg, int rows, const float* __restrict__ W0, const float* __restrict__ b0,
                                                       const float* __restrict__ W1, const float* __restrict__ b1, float* __restrict__ xw,
                                                       uint8_t* __restrict__ mask, int T, int mask_T, int mask_t0, float pad, const void* const* xtab) {
  const float* __restrict__ x = xtab ? static_cast<const float*>(xtab[F == 1 ? RV_PTAB_RAW : RV_PTAB_EVENT]) : x_arg;
  const int c4 = threadIdx.x & 127, dir = threadIdx.x >> 7;
  const float* W = dir ? W1 : W0;
  const float* b = dir ? b1 : b0;
  float4 wr[F];
#pragma unroll
  for (int f = 0; f < F; ++f) wr[f] = *reinterpret_cast<const float4*>(W + (size_t)f * RV_G + 4 * c4);
  const float4 bv = *reinterpret_cast<const float4*>(b + 4 * c4);
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    float4 acc = bv;
    bool real = true;                                            // utils.input_mask (utils.py:26-32): all features != pad
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const float xv = x[(size_t)r * F + f];
      real = real && xv != pad;
      acc.x = fmaf(xv, wr[f].x, acc.x); acc.y = fmaf(xv, wr[f].y, acc.y); acc.z = fmaf(xv, wr[f].z, acc.z); acc.w = fmaf(xv, wr[f].w, acc.w);
    }
    *reinterpret_cast<float4*>(xw + ((size_t)r * 2 + dir) * RV_G + 4 * c4) = acc;
    if (mask && threadIdx.x == 0) mask[(size_t)(r / T) * mask_T + mask_t0 + r % T] = real ? 1 : 0;
  }
}

// the instantiations of k_lstm_rec_mx, (F, CH): adding or removing a form is this one line
template <int F_, int CH_> struct MxForm { static constexpr int F = F_, CH = CH_; };
template <typename Fn> void for_each_mx_form(Fn&& fn) { fn(MxForm<0, 16>{}); fn(MxForm<1, 16>{}); fn(MxForm<5, 16>{}); fn(MxForm<0, 8>{}); fn(MxForm<1, 8>{}); fn(MxForm<5, 8>{}); }
template <typename M> bool mx_serves(int F, int CH) { return M::F == F && M::CH == CH; }
// ... and of k_inproj_small<F>: fn with each form in turn until it returns true
template <int F_> struct InprojForm { static constexpr int F = F_; };
template <typename Fn> bool for_each_inproj_form(Fn&& fn) { return fn(InprojForm<5>{}) || fn(InprojForm<1>{}); }

constexpr size_t mx_lds_bytes(int F, int T) { return 16384 + sizeof(float) * ((size_t)RV_G + (F > 0 ? (size_t)(F + 1) * RV_G + (size_t)RV_MX_ROWS * T * F : 2 * RV_G)); }

}  // namespace

void list_mx_forms(FormLog& log) {
  for_each_mx_form([&](auto form) { using M = decltype(form); log.add(RV_K_LSTM_REC_MX, M::F, M::CH); });
  for_each_inproj_form([&](auto form) { log.add(RV_K_INPROJ_SMALL, decltype(form)::F); return false; });
}

void list_mx_proj_forms(FormLog& log) { log.add(RV_K_LSTM_REC_MX_PROJ, RV_MX_ROWS); }

bool lstm_rec_mx_window_fits(int T, int F) { return mx_lds_bytes(F, T) <= 160 * 1024; }

hipError_t configure_mx_kernels() {
  hipError_t first = hipSuccess;
  for_each_mx_form([&](auto form) {
    using M = decltype(form);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lstm_rec_mx<M::F, M::CH>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess && first == hipSuccess) first = e;
    if constexpr (M::F > 0) {
      const hipError_t em = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lstm_rec_mx_members<M::F, M::CH>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (em != hipSuccess && first == hipSuccess) first = em;
      const hipError_t ew = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lstm_rec_mx_windows<M::F, M::CH>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (ew != hipSuccess && first == hipSuccess) first = ew;
    }
  });
  const hipError_t ep = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lstm_rec_mx_proj), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (ep != hipSuccess && first == hipSuccess) first = ep;
  return first;
}

void launch_lstm_rec_mx_proj(const RecArgs& a, hipStream_t s, FormLog* log) {
  hipLaunchKernelGGL(k_lstm_rec_mx_proj, dim3((a.B + RV_MX_ROWS - 1) / RV_MX_ROWS, 2), dim3(512), MXP_LDS, s, a);      // (its LDS does not depend on T)
  if (log) log->add(RV_K_LSTM_REC_MX_PROJ, RV_MX_ROWS);
}

void launch_lstm_rec_mx(const RecArgs& a, int F, hipStream_t s, bool rows8, FormLog* log) {
  const int CH = rows8 ? 8 : RV_MX_ROWS;                         // eight chunks per workgroup: the latency form (see the head of this file)
  for_each_mx_form([&](auto form) {
    using M = decltype(form);
    if (mx_serves<M>(F, CH)) {
      const dim3 grid((a.B + CH - 1) / CH, 2);
      auto kernel = &k_lstm_rec_mx<M::F, M::CH>;
      if constexpr (M::F > 0) {
        if (a.windows) kernel = &k_lstm_rec_mx_windows<M::F, M::CH>;
        else if (a.members.n > 0) kernel = &k_lstm_rec_mx_members<M::F, M::CH>;
      }
      hipLaunchKernelGGL(kernel, grid, dim3(512), mx_lds_bytes(M::F, a.T), s, a);
      if (log) log->add(RV_K_LSTM_REC_MX, M::F, M::CH);
    }
  });
}

void launch_expand_windows(const RecWindow* windows, int B, float* raw, int T_r, float* ev, int T_e, float pad, hipStream_t s) {
  if (B <= 0 || (!raw && !ev)) return;
  hipLaunchKernelGGL(k_expand_windows, dim3(B, 2), dim3(256), 0, s, windows, raw, T_r, ev, T_e, pad);
}

void launch_inproj_small(const float* x, int rows, int F, const float* W0, const float* b0, const float* W1, const float* b1, float* xw,
                         uint8_t* mask, int T, int mask_T, int mask_t0, float pad, hipStream_t s, const void* const* xtab, FormLog* log) {
  const int grid = rows < 4096 ? rows : 4096;
  for_each_inproj_form([&](auto form) {
    using P = decltype(form);
    if (P::F != F) return false;
    hipLaunchKernelGGL((k_inproj_small<P::F>), dim3(grid), dim3(256), 0, s, x, rows, W0, b0, W1, b1, xw, mask, T, mask_T, mask_t0, pad, xtab);
    if (log) log->add(RV_K_INPROJ_SMALL, P::F);
    return true;
  });
}
