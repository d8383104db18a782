// bf16_frag.h — what the bf16 matrix-core convolutions share (spconv_bf16.hip: plain bf16, inference;
// spconv_split.hip: split bf16 planes, training): the MFMA fragment types, the row decomposition of a workgroup, the
// rounding and the column-group rule.
#pragma once
#include "common.h"

namespace usc {
namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int kRowTiles = 2;            // 32-row tiles per wave
constexpr int kBlockRows = 4 * 32 * kRowTiles;

// round to nearest even; NaN stays a (quiet) NaN
__device__ inline uint16_t f32_to_bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// 32-column tiles per workgroup column group: the widest of 3, 2, 1 that divides cout / 32 (four tiles, 128 accumulator
// registers, leave one wave per SIMD)
inline int col_tiles(int cout) {
  const int T = cout / 32;
  return T % 3 == 0 ? 3 : T % 2 == 0 ? 2 : 1;
}

}  // namespace
}  // namespace usc
