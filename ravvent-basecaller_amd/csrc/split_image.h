// The split-f16 building blocks of the weight images, host code only: the one power-of-two scale rule, the one writer of an MFMA
// 16x16x32 fragment as two f16 parts, and on top of them the B image of the split GEMMs (common.h: launch_gemm_mem_split /
// launch_gemm_split_blocks).  Behind every such image weight_images.cpp builds, and behind the kernels' probe (tests/kernels/gemm_probe.hip).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <vector>

// The power of two s that brings a largest |w| (mx: of a column, or of a whole tensor) into [2^13, 2^14); 2^14 for a zero or non-finite
// one: the scale of every split-f16 image
inline float rv_column_scale(float mx) {
  int ex = 0;
  if (mx > 0.f && std::isfinite(mx)) std::frexp(mx, &ex);    // mx = m 2^ex, m in [0.5, 1)
  return std::ldexp(1.0f, 14 - ex);
}
// ... and of a column of `rows` elements (stride ld)
inline float rv_column_scale(const float* w, size_t ld, int rows) {
  float mx = 0.f;
  for (int k = 0; k < rows; ++k) mx = std::max(mx, std::fabs(w[(size_t)k * ld]));
  return rv_column_scale(mx);
}
// What an image carries beside its scaled columns: the factor 2^-14 / s that undoes scale s, as two uint16
inline void rv_put_factor(uint16_t* at, float s) {
  const float f = std::ldexp(1.0f, -14) / s;
  memcpy(at, &f, 4);
}
// Option weight_parts 1: one weight rounded to what the first f16 part of its image holds under the image's scale s (a power of two)
inline float rv_round_to_first_part(float w, float s) { return (float)(_Float16)(w * s) / s; }
// ... and a column of `rows` elements (stride ld) under its own scale
inline void rv_round_column(float* w, size_t ld, int rows) {
  const float s = rv_column_scale(w, ld, rows);
  for (int k = 0; k < rows; ++k) w[(size_t)k * ld] = rv_round_to_first_part(w[(size_t)k * ld], s);
}

// One MFMA 16x16x32 fragment of 32 k x 16 n scaled elements el(k, n) as two f16 parts of [64 lanes][8]: lane 16 (k / 8) + n holds
// k % 8 = 0..7.  Part 0, at p0, is the f16 rounding of el; part 1, at p0 + part_stride, the f16 rounding of lo_mul times what that
// left (lo_mul 2048 keeps the rest of a small element out of the f16 subnormals: the Wh image, whose kernel divides it out again)
template <class El>
inline void rv_write_fragment(uint16_t* p0, size_t part_stride, El el, float lo_mul = 1.f) {
  for (int ln = 0; ln < 64; ++ln)
    for (int j = 0; j < 8; ++j) {
      const float v = el(8 * (ln >> 4) + j, ln & 15);
      const _Float16 hi = (_Float16)v;
      const _Float16 lo = (_Float16)((v - (float)hi) * lo_mul);
      memcpy(&p0[(size_t)ln * 8 + j], &hi, 2);
      memcpy(&p0[part_stride + (size_t)ln * 8 + j], &lo, 2);
    }
}

// Logical kernel W[256][256 ncb]: element (k, c) = w[col(c) + k * ld], where col(c) is the offset of column c's first element (a
// kernel kept as several arrays, e.g. one per direction, is addressed through it).
// img: [ncb][8 k-steps][16 tiles][2 parts][64 lanes][8 f16] of the column-scaled kernel, then 256 ncb floats 2^-14 / s_c -- exactly
// RV_WMP16_SLOT (ncb = 1) / RV_GRU_WX16_SLOT (ncb = 3) / RV_WX16_SLOT (ncb = 4) uint16.  Column c = 256 cb + 16 nt + n: lane (n, kq)
// of tile nt, k-step ks holds s_c W[32 ks + 8 kq + j][c] (s_c W is exact: s_c = rv_column_scale of the column)
template <class ColOffset>
inline void rv_pack_split_image(const float* w, size_t ld, int ncb, ColOffset col, uint16_t* img) {
  const size_t block = (size_t)2 * 256 * 256;               // uint16 per column block
  std::vector<float> sc((size_t)256 * ncb);
  for (int c = 0; c < 256 * ncb; ++c) {
    sc[c] = rv_column_scale(w + col(c), ld, 256);
    rv_put_factor(&img[(size_t)ncb * block + 2 * (size_t)c], sc[c]);
  }
  for (int cb = 0; cb < ncb; ++cb)
    for (int ks = 0; ks < 8; ++ks)
      for (int nt = 0; nt < 16; ++nt)
        rv_write_fragment(img + (size_t)cb * block + (((size_t)ks * 16 + nt) * 2) * 512, 512, [&](int k, int n) {
          const int c = 256 * cb + 16 * nt + n;
          return w[col(c) + (size_t)(32 * ks + k) * ld] * sc[c];
        });
}
