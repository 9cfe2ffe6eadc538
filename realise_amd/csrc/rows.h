// What the row-kernel files share on the device, and nothing else: the bf16 16-byte chunk pack / unpack (layernorm.hip, loss.hip), the
// all-zero quad test (tokens.hip, glyph_rows.hip) and the row-width bound of the one-wave-per-row kernels (layernorm.hip, fusion.hip).
#pragma once
#include "common.h"

namespace rl {

constexpr int LN_MAXV = 4;   // up to 4 x (64 lanes x 4 elems) = 1024 columns per row

// a 16-byte chunk of eight bf16 columns <-> eight floats
__device__ __forceinline__ void unpack8(const uint4 u, float (&f)[8]) {
  f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
  f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
  f[4] = __uint_as_float(u.z << 16); f[5] = __uint_as_float(u.z & 0xffff0000u);
  f[6] = __uint_as_float(u.w << 16); f[7] = __uint_as_float(u.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  uint4 u;
  u.x = pack2bf(f[0], f[1]); u.y = pack2bf(f[2], f[3]); u.z = pack2bf(f[4], f[5]); u.w = pack2bf(f[6], f[7]);
  return u;
}

// an exact-zero column quad: a padded token's gradient (embed_bwd, segment_sum)
__device__ __forceinline__ bool quad_is_zero(floatx4 d) { return d[0] == 0.f && d[1] == 0.f && d[2] == 0.f && d[3] == 0.f; }

}  // namespace rl
