// K0 / K2 -- exact-fp32 MFMA GEMM  C[M,N] = A[M,K] . B[K,N] (+ bias, + gathered row, * row mask)
// on v_mfma_f32_32x32x2_f32 (f32 in / f32 accumulate: bit-for-bit a k-ordered fmaf chain).
//
// Used for the dense contractions of the path only:
//   K0  layer>=1 input projection  [B*T,256] x [256,512] per direction  (Keras LSTMCell x.W + b,
//       SURVEY.md A.1; the reference does it per timestep inside tf.while_loop)
//   K2  attention keys             [B*T_m,256] x [256,128], rows of padded steps zeroed
//       (setup_memory: values = memory*mask, keys = values.W_mem -- /root/reference/basecaller.py:303)
//   D1  decoder cell pre-activations [B*W,256] x [256,512] + W[one_hot(token)] + b
//       (cell input = concat(one_hot, attention) -- SURVEY.md A.4)
//
// Block = 4 waves (2x2), each wave TMxTN tiles of 32x32; K step 16, double-buffered LDS with the
// next tile's global loads held in registers across the MFMA phase.  A is stored k-major in LDS
// (row pad 2 -> conflict-free ds_write_b32 of the transposed float4s, conflict-free operand reads).
#include "common.h"
#include <cstdlib>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int TM, int TN, int BK>
__global__ __launch_bounds__(256) void k_gemm_f32(GemmArgs a) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int KV = BK / 4;                 // float4 per A row per K tile
  constexpr int LDA_S = BM + 2, LDB_S = BN + 4;
  __shared__ __align__(16) float As[2][BK * LDA_S];
  __shared__ __align__(16) float Bs[2][BK * LDB_S];

  if (a.skip_flag && *a.skip_flag >= a.skip_when) return;
  // Tile coordinates.  Plain: (x = N tile, y = M tile, z = problem).  XCD-aware: workgroups are dealt
  // round-robin to the 8 XCDs (private L2s), so ids {x, x+8, x+16, ...} share an XCD; the
  // ntn*nprob workgroups that read the same A tile are made consecutive on ONE XCD -- the A
  // panel is then fetched from HBM once instead of once per XCD (PMC: 8.4x -> ~1x the bytes).
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (a.xcd_remap) {
    const int ntn = a.N / BN, nprob = a.Bm1 ? 2 : 1, per = ntn * nprob;
    const int id = blockIdx.x, xcd = id & 7, j = id >> 3;
    const int combo = j % per;
    by = (j / per) * 8 + xcd;
    bx = combo % ntn; bz = combo / ntn;
    if (by * BM >= a.M) return;
  }
  if (bz == 1) { a.Bm = a.Bm1; a.bias = a.bias1; a.C = a.C1; }

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = by * BM, n0 = bx * BN;
  const int nk = a.K / BK;

  constexpr int NA = TM * KV / 4, NB = TN * KV / 4;   // float4 loads per thread per K tile
  float4 ra[NA], rb[NB];
  auto gload = [&](int kt) {
    const int k0 = kt * BK;
#pragma unroll
    for (int p = 0; p < NA; ++p) {
      const int idx = tid + 256 * p, row = idx / KV, kv = idx % KV;
      const int m = m0 + row;
      ra[p] = m < a.M ? *reinterpret_cast<const float4*>(a.A + (size_t)m * a.lda + k0 + 4 * kv)
                      : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int p = 0; p < NB; ++p) {
      const int idx = tid + 256 * p, kr = idx / (BN / 4), nv = idx % (BN / 4);
      rb[p] = *reinterpret_cast<const float4*>(a.Bm + (size_t)(k0 + kr) * a.ldb + n0 + 4 * nv);
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int p = 0; p < NA; ++p) {
      const int idx = tid + 256 * p, row = idx / KV, kv = idx % KV;
      float* d = &As[buf][(4 * kv) * LDA_S + row];
      d[0] = ra[p].x; d[LDA_S] = ra[p].y; d[2 * LDA_S] = ra[p].z; d[3 * LDA_S] = ra[p].w;
    }
#pragma unroll
    for (int p = 0; p < NB; ++p) {
      const int idx = tid + 256 * p, kr = idx / (BN / 4), nv = idx % (BN / 4);
      *reinterpret_cast<float4*>(&Bs[buf][kr * LDB_S + 4 * nv]) = rb[p];
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int jn = 0; jn < TN; ++jn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][jn][r] = 0.f;

  gload(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
    const float* as = &As[buf][(lane >> 5) * LDA_S + wm * 32 * TM + (lane & 31)];
    const float* bs = &Bs[buf][(lane >> 5) * LDB_S + wn * 32 * TN + (lane & 31)];
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = as[kk * LDA_S + 32 * i];
#pragma unroll
      for (int jn = 0; jn < TN; ++jn) bv[jn] = bs[kk * LDB_S + 32 * jn];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int jn = 0; jn < TN; ++jn)
          acc[i][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[jn], acc[i][jn], 0, 0, 0);
    }
    if (kt + 1 < nk) sstore(buf ^ 1);
    __syncthreads();
  }

  // epilogue: C/D map of the 32x32 tile: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 * TM + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m >= a.M) continue;
      const bool keep = a.row_mask ? a.row_mask[m] != 0 : true;
      const float* grow = a.gather_idx ? a.gather_tab + (size_t)a.gather_idx[m] * a.ld_tab : nullptr;
#pragma unroll
      for (int jn = 0; jn < TN; ++jn) {
        const int n = n0 + wn * 32 * TN + 32 * jn + (lane & 31);
        float v = acc[i][jn][r];
        if (grow) v += grow[n];
        if (a.bias) v += a.bias[n];
        a.C[(size_t)m * a.ldc + n] = keep ? v : 0.f;
      }
    }
  }
}

}  // namespace

void launch_gemm_f32(const GemmArgs& a, bool small_tile, hipStream_t s) {
  if (small_tile) {
    dim3 grid(a.N / 64, (a.M + 63) / 64);
    hipLaunchKernelGGL((k_gemm_f32<1, 1, 16>), grid, dim3(256), 0, s, a);
  } else {
    const int ntm = (a.M + 127) / 128, ntn = a.N / 128, nprob = a.Bm1 ? 2 : 1;
    dim3 grid(ntn, ntm, nprob);
    if (a.xcd_remap) grid = dim3(((ntm + 7) / 8) * 8 * ntn * nprob, 1, 1);
    hipLaunchKernelGGL((k_gemm_f32<2, 2, 16>), grid, dim3(256), 0, s, a);
  }
}

// ------------------------------------------------------------------------------------------------
// K2s -- the attention-memory projection  C[M,256] = A[M,256] . Wmp[256,256]  on v_mfma_f32_16x16x32_f16 with both
// operands cut into two f16 parts (the split of lstm_rec.hip's SB = 2, without the 2^11 on the low part: with the operands
// scaled up by 2^14 the low parts sit far above the f16 subnormals on their own).  a' = 2^14 a (|a| <= 1: rows of the
// encoder output), w' = s_n w (s_n: the power of two that brings column n's largest weight into [2^13, 2^14));
// a'.w' = ah.wh + ah.wl + al.wh (+ al.wl, below 2^-22 of the product, dropped), every f16 x f16 product exact in f32, one
// f32 accumulator.  3 MFMAs of 16 cycles per 16x16x32 block instead of 8 v_mfma_f32_32x32x2_f32 of 64: the f32 form is
// MFMA-bound at ~0.13 ms on the C3 slab, this one is bound by its HBM bytes (A once, C once).
//
// Workgroup = 4 waves, 128 rows x all 256 columns; a wave owns 32 rows (two 16-row tiles) x 16 column tiles = 128
// accumulator registers.  K runs in 8 steps of 32: the step's B slab (16 tiles x 2 parts x 1 KB, fragment order, built at
// load time) is staged through LDS, double-buffered, and shared by the four waves; A fragments go from global memory
// straight to registers (a lane reads the 8 consecutive floats of its row that its fragment holds) and are split there.
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));

// The kernel below is the third form of this product.  Measured on the way (C3 slab; both deleted from the tree after round 2, their
// numbers are in DESIGN.md section 4): (1) one role -- every wave loads its A rows AND stages the B slabs: 0.084 ms, a wave's
// vector-memory counter retires in issue order, so it waits for HBM at every slab hand-off; (2) six 16-row compute waves + two
// loader waves, 96-row tiles: 0.065 ms, twice the LDS reads per MFMA of (3).
// (3) The two memory streams live in different waves: 4 compute waves of 32 rows (two 16-row tiles per B fragment read, one compute
// wave per SIMD) touch global memory only for A; 2 loader waves only move the B slabs L2 -> LDS (LDS-DMA, three buffers), two
// k-steps ahead.  128-row tiles, persistent: workgroup w takes tiles w, w + gridDim.x, ...  The barriers are raw s_barrier +
// lgkmcnt(0) (LDS hand-off only): __syncthreads() would also drain the A loads in flight.  The (tile, k-step) pairs of a workgroup form one
// flat stream: the A floats of stream position it + 2 are requested while position it is multiplied, across tile boundaries too.
template <int NCB>
__global__ __launch_bounds__(384) void k_gemm_mem_split3(const float* __restrict__ A, int M, const uint16_t* __restrict__ img,
                                                         float* __restrict__ C, int ntiles, int dbg_arg, int ldc,
                                                         const float* __restrict__ bias) {
  constexpr int ncb = NCB;
  // dbg: timing probes (1 = no C stores, 2 = no A loads, 4 = no MFMAs; results invalid).  The launcher passes 0 unless the library
  // was built with -DRV_GEMM_DIAG (`make gemm_diag`, tools/gemm_probe.sh).  It stays a RUN-TIME value on purpose: the never-taken
  // branches keep the scheduler from hoisting a k-step's 32 fragment reads above its MFMAs (as a compile-time 0 the kernel goes
  // from 213 to 256 VGPRs and spills).
  const int dbg = dbg_arg;
  __shared__ __align__(16) char Bs[3][32768];
  __shared__ __align__(16) float css[4 * RV_E];            // column factors of up to 4 column blocks
  __shared__ __align__(16) float bss[4 * RV_E];            // ... and their biases (zeros without one): the epilogue must not load from global
                                                           // memory -- 32 dependent L2 round trips per pair cost more than the pair's MFMAs
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // a workgroup's stream: its row tiles (blockIdx.x, + gridDim.x, ...), and for each of them the ncb column blocks in turn
  const int nloc = ncb * ((ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x);     // (tile, column block) pairs (>= 1)
#define RV_LDS_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)
  if (wave >= 4) {                                         // ---------------- loader role
    // slab -> LDS by LDS-DMA (16 x 1 KB per wave, no staging registers, no ds_write): thread p moves bytes [16 p + 2048 i, +16);
    // a wave instruction lands 1 KB at its wave-uniform base + 16 lane.  Three buffers: slab it + 2 is requested at the start
    // of iteration it (its buffer was last read in it - 1), slab it + 1 must have landed at its end: vmcnt(16) = all but
    // the youngest batch.
    const int p = tid - 256;                               // 0..127
    const float* cs = reinterpret_cast<const float*>(reinterpret_cast<const char*>(img) + (size_t)ncb * 8 * 32768);
    for (int i = p; i < ncb * RV_E; i += 128) { css[i] = cs[i]; bss[i] = bias ? bias[i] : 0.f; }
    const int nslab = 8 * ncb;
    auto dma = [&](int slab) {
      const char* src = reinterpret_cast<const char*>(img) + (size_t)(slab % nslab) * 32768 + p * 16;
      char* dst = Bs[slab % 3] + (wave - 4) * 1024;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 2048 * i),
                                         (__attribute__((address_space(3))) void*)(dst + 2048 * i), 16, 0, 0);
    };
    dma(0); dma(1);
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    RV_LDS_BARRIER();
    for (int it = 0; it < 8 * nloc; ++it) {
      dma(it + 2);
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      RV_LDS_BARRIER();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return;
  }
  // ---------------- compute role
  const int l16 = lane & 15, q = lane >> 4;
  float4 a0[2][2], a1[2][2];                               // A floats of the even / odd stream positions in flight ([row tile][half])
#define RV_A_LOAD(tile_, ks_, dst_) do { \
    _Pragma("unroll") for (int m_ = 0; m_ < 2; ++m_) { \
      const float* ap_ = A + (size_t)min((tile_) * 128 + 32 * wave + 16 * m_ + l16, M - 1) * RV_E + 8 * q + 32 * (ks_); \
      dst_[m_][0] = *reinterpret_cast<const float4*>(ap_); dst_[m_][1] = *reinterpret_cast<const float4*>(ap_ + 4); } } while (0)
  RV_A_LOAD((int)blockIdx.x, 0, a0);
  RV_A_LOAD((int)blockIdx.x, 1, a1);
  RV_LDS_BARRIER();
  for (int n = 0; n < nloc; ++n) {
    const int tile = blockIdx.x + (n / ncb) * gridDim.x, cb = n % ncb;
    const int tnext = n + 1 < nloc ? (int)blockIdx.x + ((n + 1) / ncb) * (int)gridDim.x : tile;      // (the last pair re-reads two of its own k-steps: L2 hits, dropped)
    f4v acc[2][16];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nt = 0; nt < 16; ++nt) acc[m][nt] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      h8 ah[2], al[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const float4 x0 = (ks & 1) ? a1[m][0] : a0[m][0], x1 = (ks & 1) ? a1[m][1] : a0[m][1];
        const float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float sv = v[j] * 16384.f;
          ah[m][j] = (_Float16)sv;
          al[m][j] = (_Float16)(sv - (float)ah[m][j]);
        }
      }
#ifdef RV_GEMM_DIAG
      if (!(dbg & 2))
#endif
      {                                                    // stream position + 2, into the registers just consumed.  (Unconditional in
        // the product build: a run-time condition around these loads makes the compiler merge "requested" and "not requested" at the
        // next k-step and drain the vector-memory counter there -- the loads were then waited for one k-step after their request, not two)
        if (ks & 1) RV_A_LOAD(ks + 2 < 8 ? tile : tnext, (ks + 2) & 7, a1); else RV_A_LOAD(ks + 2 < 8 ? tile : tnext, (ks + 2) & 7, a0);
      }
      const char* bs = Bs[(8 * n + ks) % 3] + lane * 16;
      // B fragments of column tile nt + 1 are read from LDS while the six MFMAs of tile nt run (two fragment pairs live): without the
      // explicit pipeline every tile waits a full LDS round trip before its MFMAs, and with no fences the scheduler hoists all 32
      // reads of the k-step and spills
      h8 bh = *reinterpret_cast<const h8*>(bs), bl = *reinterpret_cast<const h8*>(bs + 1024);
#pragma unroll
      for (int nt = 0; nt < 16; ++nt) {
        h8 bhn = bh, bln = bl;
        if (nt + 1 < 16) { bhn = *reinterpret_cast<const h8*>(bs + (2 * nt + 2) * 1024); bln = *reinterpret_cast<const h8*>(bs + (2 * nt + 3) * 1024); }
        __builtin_amdgcn_sched_barrier(0);
        if (!(dbg & 4)) {
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            // operands swapped: the tile comes out TRANSPOSED (rows = 16 columns of C, columns = the 16 rows of this row tile), so a
            // lane ends up with 4 consecutive columns of one row of C: a 16-byte store instead of four 4-byte ones
            acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl, ah[m], acc[m][nt], 0, 0, 0);
            acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, al[m], acc[m][nt], 0, 0, 0);
            acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, ah[m], acc[m][nt], 0, 0, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        bh = bhn; bl = bln;
      }
      RV_LDS_BARRIER();
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int row = tile * 128 + 32 * wave + 16 * m + l16;      // C/D map of the transposed tile: column = lane % 16 = row of C,
      if (row < M && !(dbg & 1)) {                                //   rows 4 q + i = columns 16 nt + 4 q + i of C
        // (pairing the column tiles into whole-line stores, as k_gemm_ws does, measured no gain here: 0.052-0.054 ms either way)
#pragma unroll
        for (int nt = 0; nt < 16; ++nt) {
          const int col = cb * RV_E + 16 * nt + 4 * q;
          const float4 f = *reinterpret_cast<const float4*>(&css[col]);
          const float4 bb = *reinterpret_cast<const float4*>(&bss[col]);
          *reinterpret_cast<float4*>(&C[(size_t)row * ldc + col]) =
              make_float4(fmaf(acc[m][nt][0], f.x, bb.x), fmaf(acc[m][nt][1], f.y, bb.y), fmaf(acc[m][nt][2], f.z, bb.z), fmaf(acc[m][nt][3], f.w, bb.w));
        }
      }
    }
  }
#undef RV_LDS_BARRIER
#undef RV_A_LOAD
}

// ------------------------------------------------------------------------------------------------
// (4) WEIGHT-STATIONARY form (round 3; what launch_gemm_split_blocks runs).  Probes of form (3) on the encoder input projection
// (C3: M = 76,800, N = 1,024; tools/gemm_probe.sh) showed its parts ADD -- slab staging + barriers 0.054 ms, MFMAs + 0.098, C stores
// + 0.05: one workgroup per CU whose six waves meet at a barrier every k-step leaves nothing to overlap with.  Here a workgroup
// keeps ONE half column block (128 columns x K = 256, two f16 parts: 128 KB) in LDS for its whole life and its waves (three per
// SIMD) run free: a wave takes 32-row tiles of its workgroup's row group, loads its own A rows straight into registers (RING stream
// positions in flight: slot = k-step % RING at compile time, 8 k-steps per tile, across tile boundaries too), splits them, multiplies
// against the resident fragments (64 accumulator registers: 32 rows x 128 columns) and stores -- no barrier after the weight
// load, so one wave's loads, conversions and stores run under the other waves' MFMAs.  (The vector-memory counter retires in
// order and counts stores: a load issued after a tile's 16 stores cannot be waited for without draining them -- the other waves
// of the SIMD cover that wait.)
// Twelve waves (three per SIMD, 168 VGPRs) with two stream positions in flight each: measured 0.148 ms on the C3 input projection
// against 0.156-0.160 for eight waves with two or four positions (256 VGPRs): the third wave per SIMD hides more of the A-load and
// store latency than the deeper ring does.  (-DRV_WS_THREADS=512 -DRV_WS_RING=4 rebuilds the eight-wave form.)
#ifndef RV_WS_THREADS
#define RV_WS_THREADS 768
#endif
#ifndef RV_WS_RING
#define RV_WS_RING 2       // A stream positions in flight per wave (a divisor of 8)
#endif
// Workgroup id -> (row group, column half): the 2 ncb workgroups that share a row group have the same id % 8, i.e. sit on one
// XCD and run at the same time, so the row group's A rows come from HBM once and from that XCD's L2 otherwise.
__global__ __launch_bounds__(RV_WS_THREADS) void k_gemm_ws(const float* __restrict__ A, int M, const uint16_t* __restrict__ img, int ncb,
                                                 const float* __restrict__ bias, float* __restrict__ C, int ldc, int nrg) {
  extern __shared__ __align__(16) char wsm[];
  char* Bl = wsm;                                                    // [8 k-steps][8 column tiles][2 parts][64 lanes][8 f16] = 128 KB
  float* css = reinterpret_cast<float*>(wsm + 131072);               // [128] column factors, [128] biases
  float* bss = css + 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
  const int nch = 2 * ncb;                                           // half column blocks
  const int id = blockIdx.x;
  const int rg = (id & 7) + 8 * (id / (8 * nch)), ch = (id >> 3) % nch;
  const int cb = ch >> 1, hb = ch & 1, col0 = cb * RV_E + hb * 128;
  {
    const char* src = reinterpret_cast<const char*>(img) + (size_t)cb * 8 * 32768 + hb * 16384;
    for (int i = tid; i < 8 * 1024; i += RV_WS_THREADS)       // 8 k-steps x 16 KB, 16 bytes per thread and pass
      *reinterpret_cast<float4*>(Bl + i * 16) = *reinterpret_cast<const float4*>(src + (size_t)(i >> 10) * 32768 + (i & 1023) * 16);
    const float* cs = reinterpret_cast<const float*>(reinterpret_cast<const char*>(img) + (size_t)ncb * 8 * 32768);
    if (tid < 128) { css[tid] = cs[col0 + tid]; bss[tid] = bias ? bias[col0 + tid] : 0.f; }
  }
  __syncthreads();
  const int ntile = (M + 31) / 32;
  // this wave's tiles: t_j = rg + nrg * (wave + NW j)
  constexpr int NW = RV_WS_THREADS / 64;
  const int tstride = NW * nrg;
  int t = rg + nrg * wave;
  if (t >= ntile) return;
  constexpr int RING = RV_WS_RING;
  float4 ar[RING][2][2];                                             // [slot][row tile][half]
#define RV_WS_LOAD(tile_, ks_, slot_) do { \
    _Pragma("unroll") for (int m_ = 0; m_ < 2; ++m_) { \
      const float* ap_ = A + (size_t)min((tile_) * 32 + 16 * m_ + l16, M - 1) * RV_E + 8 * q + 32 * (ks_); \
      ar[slot_][m_][0] = *reinterpret_cast<const float4*>(ap_); ar[slot_][m_][1] = *reinterpret_cast<const float4*>(ap_ + 4); } } while (0)
#pragma unroll
  for (int p0 = 0; p0 < RING; ++p0) RV_WS_LOAD(t, p0, p0);
  for (; t < ntile; t += tstride) {
    const int tn = t + tstride < ntile ? t + tstride : t;            // (the last tile re-reads four of its own k-steps: L2 hits, dropped)
    f4v acc[2][8];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) acc[m][nt] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      h8 ah[2], al[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const float4 x0 = ar[ks % RING][m][0], x1 = ar[ks % RING][m][1];
#ifdef RV_WS_PRESPLIT   // (diagnostic builds, results invalid: what the k-loop costs when A arrives as f16 parts)
        __builtin_memcpy(&ah[m], &x0, 16); __builtin_memcpy(&al[m], &x1, 16);
#else
        const float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float sv = v[j] * 16384.f;
          ah[m][j] = (_Float16)sv;
          al[m][j] = (_Float16)(sv - (float)ah[m][j]);
        }
#endif
      }
#ifndef RV_WS_NOALOAD   // (diagnostic builds: results invalid)
      if (ks + RING < 8) RV_WS_LOAD(t, ks + RING, ks % RING); else RV_WS_LOAD(tn, ks + RING - 8, ks % RING);     // stream position + RING, into the slot just consumed
#endif
      const char* bs = Bl + ks * 16384 + lane * 16;
      // Two column tiles at a time: four accumulators (2 row tiles x 2 column tiles) take the three part products in turn, so that
      // every MFMA has three independent ones between it and the next one on its accumulator (back-to-back MFMAs on ONE accumulator
      // wait out the full pipeline latency: the first form of this loop, one column tile per group, ran at a third of the MFMA rate).
      // Operands swapped: a tile comes out TRANSPOSED (rows = 16 columns of C, columns = the 16 rows of the row tile), so a lane ends
      // up with 4 consecutive columns of one row of C: a 16-byte store instead of four 4-byte ones.
#ifdef RV_WS_NOMFMA   // (diagnostic builds: results invalid -- the memory side alone)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[m][ks][j & 3] += (float)ah[m][j] + (float)al[m][j];
      (void)bs;
#else
#pragma unroll
      for (int np = 0; np < 8; np += 2) {
        const h8 bh0 = *reinterpret_cast<const h8*>(bs + (2 * np) * 1024), bl0 = *reinterpret_cast<const h8*>(bs + (2 * np + 1) * 1024);
        const h8 bh1 = *reinterpret_cast<const h8*>(bs + (2 * np + 2) * 1024), bl1 = *reinterpret_cast<const h8*>(bs + (2 * np + 3) * 1024);
        __builtin_amdgcn_sched_barrier(0);
        acc[0][np] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl0, ah[0], acc[0][np], 0, 0, 0);
        acc[1][np] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl0, ah[1], acc[1][np], 0, 0, 0);
        acc[0][np + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl1, ah[0], acc[0][np + 1], 0, 0, 0);
        acc[1][np + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl1, ah[1], acc[1][np + 1], 0, 0, 0);
        acc[0][np] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh0, al[0], acc[0][np], 0, 0, 0);
        acc[1][np] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh0, al[1], acc[1][np], 0, 0, 0);
        acc[0][np + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh1, al[0], acc[0][np + 1], 0, 0, 0);
        acc[1][np + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh1, al[1], acc[1][np + 1], 0, 0, 0);
        acc[0][np] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh0, ah[0], acc[0][np], 0, 0, 0);
        acc[1][np] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh0, ah[1], acc[1][np], 0, 0, 0);
        acc[0][np + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh1, ah[0], acc[0][np + 1], 0, 0, 0);
        acc[1][np + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh1, ah[1], acc[1][np + 1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#endif
    }
    // Epilogue.  C/D map of the transposed tile: lane (l16 = row of C, q) holds columns 16 nt + 4 q + 0..3 -- a store instruction of one
    // column tile would write 64 bytes to each of 16 rows (half cache lines, rows 4 KB apart).  Two column tiles are paired instead:
    // lanes l16 and l16 ^ 8 swap one tile each (DPP row_ror:8), so that an instruction writes the 32 columns of the pair -- one whole 128-byte
    // line -- to each of 8 rows: half as many write requests, all of them full lines (round 4: 0.147 -> 0.135 ms on the C3 projection).
    // (Tried with it and dropped: whole-line A loads by the same exchange, the weight image in the matching k order -- parity-identical, but
    //  52 B of scratch at twelve waves, 0.165 ms; eight waves 0.154-0.163.  Ablations of this kernel, tools/gemm_ab.py: without the stores
    //  0.105 ms, without the A loads 0.097, without either 0.082, and with a quarter of the MFMAs and no LDS reads still 0.145: the launch is
    //  bound by its memory side -- 394 MB at 2.7-2.9 TB/s where a plain fill of the 315 MB output runs at 6.7 TB/s.
    //  Second pass of ablations, -DRV_WS_NOMFMA builds = the memory side alone: stores alone 0.056 ms, A loads alone 0.108, both 0.184; MFMAs
    //  + LDS reads alone 0.082.  Timed and dropped, each with the stores' `nt` hint: the output as [tile][column half][32][128] so that a wave's
    //  tile leaves as one contiguous 16 KB: 0.122 against 0.121; A in a blocked order so that every load instruction reads one contiguous KB
    //  (results invalid, timing only): loads alone 0.072, the whole kernel 0.122 -- the access pattern of neither stream is the bound; every
    //  workgroup touching 1 / 8 of the 64-byte sectors of the tile its waves take two tiles later, so that the stream positions come from L2:
    //  0.147; A arriving as f16 parts, no conversion in the loop (-DRV_WS_PRESPLIT, timing only): 0.115; MFMAs + LDS reads alone then 0.0815.)
    // Nontemporal stores (round 4): the 315 MB of xw are read again only after the whole launch, by another kernel -- written with the
    // `nt` hint they do not push the A rows that the other column blocks of the row group still need out of L2: 0.139 -> 0.121 ms.
    // (The same hint on k_gemm_mem_split3's half-line stores: 0.051 -> 0.057 ms; not there.)
#define RV_WS_ST(p_, v_) do { const float4 v__ = (v_); __builtin_nontemporal_store(v__.x, (p_)); __builtin_nontemporal_store(v__.y, (p_) + 1); \
    __builtin_nontemporal_store(v__.z, (p_) + 2); __builtin_nontemporal_store(v__.w, (p_) + 3); } while (0)      /* one global_store_dwordx4 ... nt */
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int up = l16 >> 3;                                       // this lane writes the pair's first (0) / second (1) column tile
      const int r1 = t * 32 + 16 * m + (l16 & 7), r2 = r1 + 8;
#pragma unroll
      for (int nt = 0; nt < 8; nt += 2) {
        f4v x, y;                                                    // x: the partner's second tile, y: the partner's first tile
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          x[i] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc[m][nt + 1][i]), 0x128, 0xF, 0xF, false));
          y[i] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc[m][nt][i]), 0x128, 0xF, 0xF, false));
        }
        const f4v v1 = up ? x : acc[m][nt], v2 = up ? acc[m][nt + 1] : y;     // rows l16 & 7 / 8 + (l16 & 7) of the row tile
        const int cl = 16 * (nt + up) + 4 * q;
        const float4 f = *reinterpret_cast<const float4*>(&css[cl]), bb = *reinterpret_cast<const float4*>(&bss[cl]);
#ifdef RV_WS_NOSTORE
        if (r1 < M && v1[0] == 12345.f)
#else
        if (r1 < M)
#endif
          RV_WS_ST(&C[(size_t)r1 * ldc + col0 + cl],
              make_float4(fmaf(v1[0], f.x, bb.x), fmaf(v1[1], f.y, bb.y), fmaf(v1[2], f.z, bb.z), fmaf(v1[3], f.w, bb.w)));
#ifdef RV_WS_NOSTORE
        if (r2 < M && v2[0] == 12345.f)
#else
        if (r2 < M)
#endif
          RV_WS_ST(&C[(size_t)r2 * ldc + col0 + cl],
              make_float4(fmaf(v2[0], f.x, bb.x), fmaf(v2[1], f.y, bb.y), fmaf(v2[2], f.z, bb.z), fmaf(v2[3], f.w, bb.w)));
      }
    }
  }
#undef RV_WS_LOAD
#undef RV_WS_ST
}
constexpr int GEMM_WS_LDS = 131072 + 1024;

hipError_t configure_gemm_kernels() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_ws), hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_WS_LDS);
}

void launch_gemm_split_blocks(const float* A, int M, const uint16_t* img, int ncb, const float* bias, float* C, int ldc, hipStream_t s) {
  const int nt128 = (M + 127) / 128;
  int dbg = 0;
#ifdef RV_GEMM_DIAG
  static const int dbg_env = getenv("RV_GEMM_DBG") ? atoi(getenv("RV_GEMM_DBG")) : 0;
  dbg = dbg_env;
#endif
  bool old_form = false;
#ifdef RV_GEMM_DIAG
  static const bool form3_env = getenv("RV_GEMM_FORM3") != nullptr;     // A/B timing of the slab-streaming form (diagnostic builds only)
  old_form = form3_env;
#endif
  // ncb == 1 (the attention-memory projection, N = 256) stays on form (3): with two column halves a workgroup would load its 128 KB of
  // weights for some twenty 32-row tiles, and the load shows (0.056 vs 0.052 ms at C3)
  // (ncb == 3, the BiGRU family's [256 x 768] input kernel, has this form alone: the diagnostic switches above do not apply to it)
  if ((!old_form && !dbg && ncb > 1) || ncb == 3) {
    // row groups: 8 k with 8 k x 2 ncb ~ 256 workgroups, but no more groups than there is work for their waves
    const int nch = 2 * ncb, ntile = (M + 31) / 32, nw = RV_WS_THREADS / 64;
    int k = 256 / (8 * nch);
    while (k > 1 && 8 * (k - 1) * nw >= ntile) --k;               // keep every wave of every workgroup busy with at least one tile where possible
    const int nrg = 8 * k;
    hipLaunchKernelGGL(k_gemm_ws, dim3(nrg * nch), dim3(RV_WS_THREADS), GEMM_WS_LDS, s, A, M, img, ncb, bias, C, ldc, nrg);
    return;
  }
  const dim3 grid(nt128 < 256 ? nt128 : 256), block(384);
  if (ncb == 1) hipLaunchKernelGGL(k_gemm_mem_split3<1>, grid, block, 0, s, A, M, img, C, nt128, dbg, ldc, bias);
  else if (ncb == 4) hipLaunchKernelGGL(k_gemm_mem_split3<4>, grid, block, 0, s, A, M, img, C, nt128, dbg, ldc, bias);
  else abort();   // (internal: 1 = attention memory, 4 = both directions of a BiLSTM layer; 3 = of a BiGRU layer never gets here)
}
void launch_gemm_mem_split(const float* A, int M, const uint16_t* img, float* C, hipStream_t s) {
  launch_gemm_split_blocks(A, M, img, 1, nullptr, C, RV_E, s);
}
