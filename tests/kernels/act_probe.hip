// Device probe of the library's activation helpers (csrc/common.h): rv_tanh(x), rv_sigmoid(x) and rv_tanh_abs(x) of every element of
// a host array, computed on the GPU by the same inline functions the encoder and decoder cells call.  Built by `make libravvent_actprobe.so` in
// csrc with the library's flags; tests/test_activations_gpu.py loads it through ctypes and holds it against numpy fp64.
#include "common.h"

__global__ void k_act_probe(const float* __restrict__ x, float* __restrict__ t, float* __restrict__ s, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float v = x[i];
    t[i] = rv_tanh(v);
    s[i] = rv_sigmoid(v);
  }
}

// host arrays of n floats in, out; returns a hipError_t (0 = success)
extern "C" int rv_act_probe(const float* x, float* tanh_out, float* sigmoid_out, int n) {
  if (n <= 0) return 0;
  const size_t bytes = (size_t)n * sizeof(float);
  float* d = nullptr;
  hipError_t e = hipMalloc(&d, 3 * bytes);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpy(d, x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_act_probe, dim3((n + 255) / 256), dim3(256), 0, 0, d, d + n, d + 2 * (size_t)n, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(tanh_out, d + n, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(sigmoid_out, d + 2 * (size_t)n, bytes, hipMemcpyDeviceToHost);
  const hipError_t f = hipFree(d);
  return (int)(e != hipSuccess ? e : f);
}

__global__ void k_act_probe_tanh_abs(const float* __restrict__ x, float* __restrict__ t, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) t[i] = rv_tanh_abs(x[i]);
}

// rv_tanh_abs, the g gate of k_dec_persist<.., ATT = 2>: host arrays of n floats in, out; returns a hipError_t (0 = success)
extern "C" int rv_act_probe_tanh_abs(const float* x, float* tanh_abs_out, int n) {
  if (n <= 0) return 0;
  const size_t bytes = (size_t)n * sizeof(float);
  float* d = nullptr;
  hipError_t e = hipMalloc(&d, 2 * bytes);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpy(d, x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_act_probe_tanh_abs, dim3((n + 255) / 256), dim3(256), 0, 0, d, d + n, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(tanh_abs_out, d + n, bytes, hipMemcpyDeviceToHost);
  const hipError_t f = hipFree(d);
  return (int)(e != hipSuccess ? e : f);
}
