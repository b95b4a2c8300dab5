// The split-f16 B image of the split GEMMs (common.h: launch_gemm_mem_split / launch_gemm_split_blocks), built on the host.
// One function for every site that uploads such an image (rv_set_weights: the input projection of encoder layers >= 1 with
// ncb = 4, the attention-memory projection with ncb = 1) and for the kernels' probe (tests/kernels/gemm_probe.hip).  Host code only.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <cmath>

// Logical kernel W[256][256 ncb]: element (k, c) = w[col(c) + k * ld], where col(c) is the offset of column c's first element (a
// kernel kept as several arrays, e.g. one per direction, is addressed through it).
// img: [ncb][8 k-steps][16 tiles][2 parts][64 lanes][8 f16] of the column-scaled kernel, then 256 ncb floats 2^-14 / s_c -- exactly
// RV_WMP16_SLOT (ncb = 1) / RV_WX16_SLOT (ncb = 4) uint16.  Column c = 256 cb + 16 nt + n: lane (n, kq = lane / 16) of tile nt,
// k-step ks holds s_c W[32 ks + 8 kq + j][c], j = 0..7, part 0 = its f16 rounding, part 1 = the f16 rounding of what that left
// (s_c W is exact: s_c is the power of two that brings the column's largest |w| into [2^13, 2^14); 2^14 for a zero or non-finite one).
// The power of two s that brings a column's largest |w| (mx) into [2^13, 2^14); 2^14 for a zero or non-finite one: the scale of every
// per-column split-f16 image (below, and the Ua / Wh packers of rv_load_weights)
inline float rv_column_scale(float mx) {
  int ex = 0;
  if (mx > 0.f && std::isfinite(mx)) std::frexp(mx, &ex);    // mx = m 2^ex, m in [0.5, 1)
  return std::ldexp(1.0f, 14 - ex);
}
// Option weight_parts 1: one weight rounded to what the first f16 part of its image holds under the image's scale s (a power of two)
inline float rv_round_to_first_part(float w, float s) { return (float)(_Float16)(w * s) / s; }
// ... and a column of `rows` elements (stride ld) under its own scale
inline void rv_round_column(float* w, size_t ld, int rows) {
  float mx = 0.f;
  for (int k = 0; k < rows; ++k) mx = std::max(mx, std::fabs(w[(size_t)k * ld]));
  const float s = rv_column_scale(mx);
  for (int k = 0; k < rows; ++k) w[(size_t)k * ld] = rv_round_to_first_part(w[(size_t)k * ld], s);
}

template <class ColOffset>
inline void rv_pack_split_image(const float* w, size_t ld, int ncb, ColOffset col, uint16_t* img) {
  const size_t block = (size_t)2 * 256 * 256;               // uint16 per column block
  for (int c = 0; c < 256 * ncb; ++c) {
    const float* wc = w + col(c);
    float mx = 0.f;
    for (int k = 0; k < 256; ++k) mx = std::max(mx, std::fabs(wc[(size_t)k * ld]));
    int ex = 0;
    if (mx > 0.f && std::isfinite(mx)) std::frexp(mx, &ex);  // mx = m 2^ex, m in [0.5, 1)
    const float sc = std::ldexp(1.0f, 14 - ex);              // s_c; mx s_c in [2^13, 2^14)
    const float f = std::ldexp(1.0f, -14) / sc;
    memcpy(&img[(size_t)ncb * block + 2 * (size_t)c], &f, 4);
    const int cb = c / 256, nn = c % 256, nt = nn / 16;
    for (int k = 0; k < 256; ++k) {
      const float v = wc[(size_t)k * ld] * sc;
      const _Float16 hi = (_Float16)v;
      const _Float16 lo = (_Float16)(v - (float)hi);
      uint16_t hb, lb; memcpy(&hb, &hi, 2); memcpy(&lb, &lo, 2);
      const int ks = k / 32, ln = 16 * ((k % 32) / 8) + (nn % 16), j = k % 8;
      const size_t base = (size_t)cb * block + ((((size_t)ks * 16 + nt) * 2) * 64) * 8;
      img[base + (size_t)ln * 8 + j] = hb;
      img[base + 64 * 8 + (size_t)ln * 8 + j] = lb;
    }
  }
}
