// Device probe of the projection GEMMs (csrc/gemm_f32.hip): k_gemm_f32<2,2,16> through launch_gemm_f32 with the three argument sets
// the library uses, and k_gemm_mem_split3<1> / k_gemm_ws through launch_gemm_split_blocks with ncb = 1 / 3 and 4, on chosen A, W, bias and M.
// Built by `make libravvent_gemmprobe.so` in csrc with the library's flags and linked with the library's gemm_f32.o and its weight-image
// packer (csrc/split_image.h); tests/test_gemm_probe_gpu.py loads it through ctypes and holds the kernels to numpy fp64.
//
// Host arrays in, host arrays out.  On the device A is followed by RV_PROBE_GUARD rows of NaN and C by as many guard rows; C, guard
// rows and guard columns (ldc > N) included, is prefilled with the 32-bit pattern `fill` and comes back whole: an element the kernel
// never wrote, or wrote outside [M, N], shows as (or in place of) that pattern.  Return value: a hipError_t (0 = success), -1 = bad arguments.
#include "common.h"
#include "split_image.h"
#include <vector>

#define RV_PROBE_GUARD 128

namespace {

struct Dev {                                   // frees what it holds on every return path
  void* p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int n = 0;
  hipError_t alloc(void** out, size_t bytes) {
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipSuccess) p[n++] = *out;
    return e;
  }
  hipError_t upload(void** out, const void* src, size_t bytes) {
    hipError_t e = alloc(out, bytes);
    return e == hipSuccess ? hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice) : e;
  }
  ~Dev() { for (int i = 0; i < n; ++i) (void)hipFree(p[i]); }
};

hipError_t configure_once() {
  static const hipError_t e = configure_gemm_kernels();
  return e;
}

// A [M][256] -> device, followed by the guard rows of NaN
hipError_t upload_a(Dev& d, float** dA, const float* A, int M) {
  const size_t rows = (size_t)M + RV_PROBE_GUARD;
  hipError_t e = d.alloc(reinterpret_cast<void**>(dA), rows * RV_E * sizeof(float));
  if (e != hipSuccess) return e;
  e = hipMemset(*dA + (size_t)M * RV_E, 0xFF, (size_t)RV_PROBE_GUARD * RV_E * sizeof(float));      // 0xFFFFFFFF: a NaN
  return e == hipSuccess ? hipMemcpy(*dA, A, (size_t)M * RV_E * sizeof(float), hipMemcpyHostToDevice) : e;
}

hipError_t alloc_c(Dev& d, float** dC, int M, int ldc, uint32_t fill) {
  const size_t n = ((size_t)M + RV_PROBE_GUARD) * ldc;
  hipError_t e = d.alloc(reinterpret_cast<void**>(dC), n * sizeof(float));
  return e == hipSuccess ? hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(*dC), (int)fill, n) : e;
}

hipError_t finish(float* C_out, const float* dC, int M, int ldc) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e == hipSuccess ? hipMemcpy(C_out, dC, ((size_t)M + RV_PROBE_GUARD) * ldc * sizeof(float), hipMemcpyDeviceToHost) : e;
}

}  // namespace

extern "C" int rv_gemm_probe_guard_rows() { return RV_PROBE_GUARD; }

// The weight image alone (host code; no device needed): W [256][ld] (ld >= 256 ncb) -> img, RV_WMP16_SLOT / RV_WX16_SLOT uint16
extern "C" int rv_gemm_probe_pack(const float* W, int ld, int ncb, uint16_t* img) {
  if ((ncb != 1 && ncb != 3 && ncb != 4) || ld < RV_E * ncb) return -1;
  rv_pack_split_image(W, (size_t)ld, ncb, [](int c) { return (size_t)c; }, img);
  return 0;
}

// launch_gemm_f32(g, false) as the library calls it.  K = 256, A [M][256].
//   set 0, keys:             N = 128, W0 [256][128], row_mask [M], plain grid;                              C_out [M + guard][128]
//   set 1, memory:           N = 256, W0 [256][256], xcd_remap;                                             C_out [M + guard][256]
//   set 2, input projection: N = 512, W0 / W1 [256][512] and b0 / b1 [512] (the two directions), xcd_remap; C_out [M + guard][1024]
extern "C" int rv_gemm_probe_f32(int set, const float* A, int M, const float* W0, const float* W1, const float* b0, const float* b1,
                                 const uint8_t* row_mask, uint32_t fill, float* C_out) {
  if (set < 0 || set > 2 || M <= 0 || !A || !W0 || !C_out) return -1;
  if (set == 0 && !row_mask) return -1;
  if (set == 2 && (!W1 || !b0 || !b1)) return -1;
  const int N = set == 0 ? RV_U : set == 1 ? RV_E : RV_G, ldc = set == 2 ? 2 * RV_G : N;
  Dev d;
  float *dA = nullptr, *dC = nullptr, *dW0 = nullptr, *dW1 = nullptr, *db0 = nullptr, *db1 = nullptr;
  uint8_t* dmask = nullptr;
  hipError_t e = upload_a(d, &dA, A, M);
  if (e == hipSuccess) e = alloc_c(d, &dC, M, ldc, fill);
  if (e == hipSuccess) e = d.upload(reinterpret_cast<void**>(&dW0), W0, (size_t)RV_E * N * sizeof(float));
  if (e == hipSuccess && set == 0) e = d.upload(reinterpret_cast<void**>(&dmask), row_mask, (size_t)M);
  if (e == hipSuccess && set == 2) {
    // one buffer for what remains: [W1 | b0 | b1]
    std::vector<float> rest((size_t)RV_E * N + 2 * N);
    memcpy(rest.data(), W1, (size_t)RV_E * N * sizeof(float));
    memcpy(rest.data() + (size_t)RV_E * N, b0, N * sizeof(float));
    memcpy(rest.data() + (size_t)RV_E * N + N, b1, N * sizeof(float));
    e = d.upload(reinterpret_cast<void**>(&dW1), rest.data(), rest.size() * sizeof(float));
    db0 = dW1 + (size_t)RV_E * N; db1 = db0 + N;
  }
  if (e != hipSuccess) return (int)e;
  GemmArgs g{};
  g.A = dA; g.lda = RV_E; g.Bm = dW0; g.ldb = N; g.C = dC; g.ldc = ldc;
  g.M = M; g.N = N; g.K = RV_E;
  if (set == 0) g.row_mask = dmask;
  if (set >= 1) g.xcd_remap = 1;
  if (set == 2) { g.bias = db0; g.Bm1 = dW1; g.bias1 = db1; g.C1 = dC + RV_G; }
  launch_gemm_f32(g, false, 0);
  return (int)finish(C_out, dC, M, ldc);
}

// launch_gemm_split_blocks: C [M][ldc] (columns 0 .. 256 ncb) = A [M][256] . W [256][256 ncb] (+ bias [256 ncb], may be null), with W
// packed by rv_pack_split_image first.  ncb = 1: k_gemm_mem_split3<1> (the attention-memory projection); ncb = 3: k_gemm_ws over six
// half column blocks (both directions of a BiGRU layer >= 1, N = 768); ncb = 4: k_gemm_ws over eight (of a BiLSTM layer >= 1, N = 1024).
// ldc >= 256 ncb, a multiple of 4.
// C_out [M + guard][ldc].
extern "C" int rv_gemm_probe_split(int ncb, const float* A, int M, const float* W, const float* bias, int ldc, uint32_t fill, float* C_out) {
  if ((ncb != 1 && ncb != 3 && ncb != 4) || M <= 0 || !A || !W || !C_out || ldc < RV_E * ncb || ldc % 4) return -1;
  hipError_t e = configure_once();
  if (e != hipSuccess) return (int)e;
  const int N = RV_E * ncb;
  std::vector<uint16_t> img((size_t)2 * RV_E * N + 2 * N);
  rv_pack_split_image(W, (size_t)N, ncb, [](int c) { return (size_t)c; }, img.data());
  Dev d;
  float *dA = nullptr, *dC = nullptr, *db = nullptr;
  uint16_t* dimg = nullptr;
  e = upload_a(d, &dA, A, M);
  if (e == hipSuccess) e = alloc_c(d, &dC, M, ldc, fill);
  if (e == hipSuccess) e = d.upload(reinterpret_cast<void**>(&dimg), img.data(), img.size() * sizeof(uint16_t));
  if (e == hipSuccess && bias) e = d.upload(reinterpret_cast<void**>(&db), bias, (size_t)N * sizeof(float));
  if (e != hipSuccess) return (int)e;
  launch_gemm_split_blocks(dA, M, dimg, ncb, db, dC, ldc, 0);
  return (int)finish(C_out, dC, M, ldc);
}
