// Operand shadows (the "weight shadows" section of ops.h): compute-dtype copies of the fp32 master weights - the flat cast and its
// inverse, the cast + transpose of the Linear weights (one matrix, or all of them in one launch), the conv-weight forward / dgrad
// copies (one tensor, or the whole glyph ResNet in one launch) and the NHWC glyph table.
#include "ops.h"
#include "launch.h"

namespace rl {

// ---------------------------------------------------------------------------------------------
// Operand shadows
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void cast_copy_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = from_f<T>(src[i]);
}
template <typename T> int cast_copy(hipStream_t st, const float* src, T* dst, int64_t n) {
  if (n <= 0) return RL_OK;
  hipLaunchKernelGGL((cast_copy_kernel<T>), dim3(ew_blocks(n)), dim3(256), 0, st, src, dst, n);
  return RL_LAUNCH_CHECK();
}
template int cast_copy<bf16_t>(hipStream_t, const float*, bf16_t*, int64_t);
template int cast_copy<float>(hipStream_t, const float*, float*, int64_t);

// T -> fp32 (the reference returns fp32 logits, models.py:859; the bf16 engine widens them on request), 8 elements per lane
template <typename T>
__global__ void cast_to_f32_kernel(const T* __restrict__ src, float* __restrict__ dst, int64_t n) {
  const int64_t n8 = n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    floatx4 a, b;
    load8<T>(src + i * 8, a, b);
    *(floatx4*)(dst + i * 8) = a;
    *(floatx4*)(dst + i * 8 + 4) = b;
  }
  if (blockIdx.x == 0)
    for (int64_t i = (n8 << 3) + threadIdx.x; i < n; i += blockDim.x) dst[i] = to_f<T>(src[i]);
}
template <typename T> int cast_to_f32(hipStream_t st, const T* src, float* dst, int64_t n) {
  if (n <= 0) return RL_OK;
  if (((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return RL_ERR_ARG;
  hipLaunchKernelGGL((cast_to_f32_kernel<T>), dim3(ew_blocks(n / 8)), dim3(256), 0, st, src, dst, n);
  return RL_LAUNCH_CHECK();
}
template int cast_to_f32<bf16_t>(hipStream_t, const bf16_t*, float*, int64_t);
template int cast_to_f32<float>(hipStream_t, const float*, float*, int64_t);

template <typename T>
__global__ void __launch_bounds__(256)
cast_transpose_kernel(const float* __restrict__ src, int R, int C, T* __restrict__ dst, T* __restrict__ dstT) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + 8 * k, c = c0 + tx;
    float v = 0.f;
    if (r < R && c < C) {
      v = src[(int64_t)r * C + c];
      if (dst != nullptr) dst[(int64_t)r * C + c] = from_f<T>(v);
    }
    tile[ty + 8 * k][tx] = v;
  }
  __syncthreads();
  if (dstT != nullptr) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + ty + 8 * k, r = r0 + tx;
      if (r < R && c < C) dstT[(int64_t)c * R + r] = from_f<T>(tile[tx][ty + 8 * k]);
    }
  }
}
template <typename T> int cast_transpose(hipStream_t st, const float* src, int R, int C, T* dst, T* dstT) {
  hipLaunchKernelGGL((cast_transpose_kernel<T>), dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0, st, src, R, C, dst, dstT);
  return RL_LAUNCH_CHECK();
}
// 64 x 64 tiles, 16 B fp32 reads / 4-element writes; the transposed copy goes through a padded LDS tile so both outputs
// are written in 128-byte (bf16) row segments.
template <typename T>
__global__ void __launch_bounds__(256) cast_transpose_multi_kernel(const CastDesc* __restrict__ descs, int n) {
  __shared__ float tile[64][65];
  int lo = 0, hi = n - 1;                               // last descriptor with tile_begin <= blockIdx.x
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].tile_begin <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const CastDesc d = descs[lo];
  const int t = blockIdx.x - d.tile_begin;
  const int r0 = (t / d.tiles_c) * 64, c0 = (t % d.tiles_c) * 64;
  const int q = threadIdx.x & 15, y = threadIdx.x >> 4;     // 16 quads x 16 rows per pass
  T* dst = (T*)d.dst;
  T* dstT = (T*)d.dstT;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + y + 16 * k, c = c0 + 4 * q;
    floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
    if (r < d.R && c < d.C) {                           // C % 4 == 0
      v = *(const floatx4*)(d.src + (int64_t)r * d.C + c);
      if (dst != nullptr) store4<T>(dst + (int64_t)r * d.C + c, v);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[y + 16 * k][4 * q + j] = v[j];
  }
  __syncthreads();
  if (dstT == nullptr) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + y + 16 * k, r = r0 + 4 * q;
    if (c < d.C && r < d.R) {
      if (r + 3 < d.R && (d.R & 3) == 0) {
        floatx4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = tile[4 * q + j][y + 16 * k];
        store4<T>(dstT + (int64_t)c * d.ldT + r, v);
      } else {
        for (int j = 0; j < 4 && r + j < d.R; ++j) dstT[(int64_t)c * d.ldT + r + j] = from_f<T>(tile[4 * q + j][y + 16 * k]);
      }
    }
  }
}
template <typename T> int cast_transpose_multi(hipStream_t st, const CastDesc* descs, int n, int total_tiles) {
  if (n <= 0 || total_tiles <= 0) return RL_OK;
  hipLaunchKernelGGL((cast_transpose_multi_kernel<T>), dim3(total_tiles), dim3(256), 0, st, descs, n);
  return RL_LAUNCH_CHECK();
}
template int cast_transpose_multi<bf16_t>(hipStream_t, const CastDesc*, int, int);
template int cast_transpose_multi<float>(hipStream_t, const CastDesc*, int, int);
template int cast_transpose<bf16_t>(hipStream_t, const float*, int, int, bf16_t*, bf16_t*);
template int cast_transpose<float>(hipStream_t, const float*, int, int, float*, float*);

template <typename T>
__global__ void conv_weight_shadow_kernel(const float* __restrict__ w, int Co, int Ci, int KHW, int Cpad, int CiRows,
                                          T* __restrict__ fwd, T* __restrict__ dgrad, TapOrder order) {
  const int64_t nf = (int64_t)Co * KHW * Cpad, nd = (int64_t)CiRows * KHW * Co;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nf + nd; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < nf) {
      if (fwd == nullptr) continue;
      const int ci = (int)(i % Cpad);
      const int tap = (int)((i / Cpad) % KHW);
      const int co = (int)(i / ((int64_t)Cpad * KHW));
      fwd[i] = from_f<T>(ci < Ci ? w[((int64_t)co * Ci + ci) * KHW + tap] : 0.f);
    } else {
      if (dgrad == nullptr) continue;
      const int64_t k = i - nf;
      const int co = (int)(k % Co);
      const int tap = (int)((k / Co) % KHW);
      const int ci = (int)(k / ((int64_t)Co * KHW));
      const int src_tap = order.n ? order.t[tap] : tap;          // slot `tap` of the data-gradient copy holds original tap order.t[tap]
      dgrad[k] = from_f<T>(ci < Ci ? w[((int64_t)co * Ci + ci) * KHW + src_tap] : 0.f);
    }
  }
}
template <typename T>
int conv_weight_shadow(hipStream_t st, const float* w, int Co, int Ci, int KHW, int Cpad, int CiRows, T* fwd, T* dgrad, const TapOrder& order) {
  if (order.n != 0 && order.n != KHW) return RL_ERR_ARG;
  const int64_t n = (int64_t)Co * KHW * Cpad + (int64_t)CiRows * KHW * Co;
  hipLaunchKernelGGL((conv_weight_shadow_kernel<T>), dim3(ew_blocks(n)), dim3(256), 0, st, w, Co, Ci, KHW, Cpad, CiRows, fwd, dgrad, order);
  return RL_LAUNCH_CHECK();
}
template int conv_weight_shadow<bf16_t>(hipStream_t, const float*, int, int, int, int, int, bf16_t*, bf16_t*, const TapOrder&);
template int conv_weight_shadow<float>(hipStream_t, const float*, int, int, int, int, int, float*, float*, const TapOrder&);

// All conv-weight operand copies of the glyph ResNet in ONE launch (was 20 launches of ~13 us on the glyph stream).  A workgroup
// takes a [32 co][32 ci][KHW] block of one weight tensor: the source rows w[co][ci0 .. ci0 + 31][:] are contiguous runs of 32 * KHW
// floats (coalesced reads), the block goes through LDS, and both copies leave in 64-byte segments - fwd[co][tap][ci0 ..] and
// dgrad[ci][slot][co0 ..].  (The element-per-thread form gathered every source float with a 36-byte stride: 167 us for 14 M weights.)
// Padding entries (ci >= Ci of a Cpad-wide row, rows >= Ci of the dgrad copy) are never written: the shadow arena is zero-filled.
constexpr int CSH_T = 32;
// (KHW and, on full tiles, the tile edges are compile-time constants: the index arithmetic is shifts and multiply-shifts - with
// run-time divisors the kernel was bound by its integer divisions, 123 us)
template <typename T, int KHW, bool FULL>
__device__ __forceinline__ void conv_shadow_tile(const ConvShadowDesc& d, float (*tile)[CSH_T * 9 + 1], int co0, int ci0, int nco_, int nci_) {
  const int nco = FULL ? CSH_T : nco_, nci = FULL ? CSH_T : nci_, run = nci * KHW;
  const int Co = d.Co, Ci = d.Ci, Cpad = d.Cpad;
  T* fwd = (T*)d.fwd;
  T* dgrad = (T*)d.dgrad;
  for (int e = threadIdx.x; e < nco * run; e += 256) {                    // [co][ci][tap] block -> LDS, the same order
    const int c = e / run, r = e - c * run;
    tile[c][r] = d.w[((int64_t)(co0 + c) * Ci + ci0) * KHW + r];
  }
  __syncthreads();
  if (fwd != nullptr)
    for (int e = threadIdx.x; e < nco * KHW * nci; e += 256) {            // fwd[co][tap][ci]: ci fastest
      const int ci = e % nci, rest = e / nci, tap = rest % KHW, c = rest / KHW;
      fwd[((int64_t)(co0 + c) * KHW + tap) * Cpad + ci0 + ci] = from_f<T>(tile[c][ci * KHW + tap]);
    }
  if (dgrad != nullptr)
    for (int e = threadIdx.x; e < nci * KHW * nco; e += 256) {            // dgrad[ci][slot][co]: co fastest
      const int c = e % nco, rest = e / nco, slot = rest % KHW, ci = rest / KHW;
      const int src_tap = d.order.n ? d.order.t[slot] : slot;
      dgrad[((int64_t)(ci0 + ci) * KHW + slot) * Co + co0 + c] = from_f<T>(tile[c][ci * KHW + src_tap]);
    }
}
template <typename T>
__global__ void __launch_bounds__(256) conv_weight_shadow_multi_kernel(ConvShadowDescs ds) {
  __shared__ float tile[CSH_T][CSH_T * 9 + 1];
  int k = 0;
#pragma unroll 1
  for (int i = 1; i < ds.n; ++i) if ((int)blockIdx.x >= ds.d[i].block_begin) k = i;
  const ConvShadowDesc& d = ds.d[k];
  const int tiles_ci = (d.Ci + CSH_T - 1) / CSH_T;
  const int b = (int)blockIdx.x - d.block_begin;
  const int co0 = (b / tiles_ci) * CSH_T, ci0 = (b % tiles_ci) * CSH_T;
  const int nco = min(CSH_T, d.Co - co0), nci = min(CSH_T, d.Ci - ci0);
  const bool full = nco == CSH_T && nci == CSH_T;
  if (d.KHW == 9) { if (full) conv_shadow_tile<T, 9, true>(d, tile, co0, ci0, nco, nci); else conv_shadow_tile<T, 9, false>(d, tile, co0, ci0, nco, nci); }
  else if (d.KHW == 1) { if (full) conv_shadow_tile<T, 1, true>(d, tile, co0, ci0, nco, nci); else conv_shadow_tile<T, 1, false>(d, tile, co0, ci0, nco, nci); }
}
template <typename T> int conv_weight_shadow_multi(hipStream_t st, ConvShadowDescs& ds) {
  if (ds.n < 1 || ds.n > CONV_SHADOW_MAX) return RL_ERR_ARG;
  int blocks = 0;
  for (int k = 0; k < ds.n; ++k) {
    const ConvShadowDesc& d = ds.d[k];
    if ((d.order.n != 0 && d.order.n != d.KHW) || (d.KHW != 1 && d.KHW != 9) || d.Ci > d.Cpad || d.Ci > d.CiRows) return RL_ERR_ARG;
    ds.d[k].block_begin = blocks;
    blocks += ((d.Co + CSH_T - 1) / CSH_T) * ((d.Ci + CSH_T - 1) / CSH_T);
  }
  hipLaunchKernelGGL((conv_weight_shadow_multi_kernel<T>), dim3(blocks), dim3(256), 0, st, ds);
  return RL_LAUNCH_CHECK();
}
template int conv_weight_shadow_multi<bf16_t>(hipStream_t, ConvShadowDescs&);
template int conv_weight_shadow_multi<float>(hipStream_t, ConvShadowDescs&);

template <typename T>
__global__ void glyph_shadow_kernel(const float* __restrict__ tbl, int64_t V, int F, int HW, int Cpad, T* __restrict__ out) {
  const int64_t n = V * HW * Cpad;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(i % Cpad);
    const int64_t px = (i / Cpad) % HW;
    const int64_t v = i / ((int64_t)Cpad * HW);
    out[i] = from_f<T>(f < F ? tbl[(v * F + f) * HW + px] : 0.f);
  }
}
template <typename T> int glyph_shadow(hipStream_t st, const float* tbl, int V, int F, int HW, int Cpad, T* out) {
  hipLaunchKernelGGL((glyph_shadow_kernel<T>), dim3(4096), dim3(256), 0, st, tbl, (int64_t)V, F, HW, Cpad, out);
  return RL_LAUNCH_CHECK();
}
template int glyph_shadow<bf16_t>(hipStream_t, const float*, int, int, int, int, bf16_t*);
template int glyph_shadow<float>(hipStream_t, const float*, int, int, int, int, float*);

}  // namespace rl
