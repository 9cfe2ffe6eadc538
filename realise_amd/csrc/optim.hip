// Optimizer (K15, K16; the "optimizer" section of ops.h): the global gradient norm, the AdamW sweeps of
// transformers/optimization.py:110-169 (flat, grouped, chunk list, and the sweep fused with the operand copies of the Linear weights),
// the in-place half of clip_grad_norm_ (run.py:207), and the fills of the flat arenas.
#include "ops.h"
#include "launch.h"

namespace rl {

// ---- knob (ops.h: set_adamw_reg) ----
// realise_set_ln key 6: 1 = the register-transpose tile above, 0 (default) = the LDS tile (round 4).  Measured level (14.67 against 14.61-
// 14.83 ms/step, three pairs), and the pipelined sweep on it is level with the plain sweep too: what overlaps competes for HBM.
static int g_adamw_reg = 0;
void set_adamw_reg(int on) { g_adamw_reg = on; }

// ---------------------------------------------------------------------------------------------
// Optimizer: global grad norm + AdamW over flat arenas
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sumsq_kernel(const float* __restrict__ g, int64_t n, float* out) {
  __shared__ float sm[4];
  float s = 0.f;
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const floatx4 v = *(const floatx4*)(g + i * 4);
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t i = n4 * 4; i < n; ++i) s += g[i] * g[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, sm[0] + sm[1] + sm[2] + sm[3]);
}
int sumsq_accum(hipStream_t st, const float* g, int64_t n, float* out) {
  if (n <= 0) return RL_OK;
  hipLaunchKernelGGL(sumsq_kernel, dim3(ew_blocks(n / 4 + 1)), dim3(256), 0, st, g, n, out);
  return RL_LAUNCH_CHECK();
}

// One element of an AdamW step: the one statement of the arithmetic that every sweep kernel below shares (flat, grouped, chunk list,
// LDS tile, register tile).  Contraction is switched off inside it: left to the compiler, each kernel fused its own choice of the
// multiply-adds, and the register tile's p differed in the last bit from the LDS tile's (tests/test_optim_edges_gpu.py) although both
// were documented as the same bits.  Every product and sum now rounds on its own, in every kernel alike.
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float clip, float lr, float beta1, float beta2,
                                           float eps, float wd, float step_size) {
#pragma clang fp contract(off)
  const float gi = g * clip;
  const float mi = m * beta1 + (1.0f - beta1) * gi;
  const float vi = v * beta2 + (1.0f - beta2) * gi * gi;
  float pi = p - step_size * (mi / (sqrtf(vi) + eps));
  if (wd > 0.f) pi -= lr * wd * pi;                 // decoupled decay AFTER the update (optimization.py:162-167)
  m = mi; v = vi; p = pi;
}
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float clip, const AdamwGroup& h) {
  adamw_elem(p, g, m, v, clip, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.step_size);
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             int64_t n, float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2,
                             const float* __restrict__ norm_sq, float max_norm) {
  float clip = 1.0f;
  if (norm_sq != nullptr) {
    const float c = max_norm / (sqrtf(norm_sq[0]) + 1e-6f);
    clip = c < 1.0f ? c : 1.0f;
  }
  const float step_size = lr * sqrtf(bc2) / bc1;     // optimization.py:156-160
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_elem(pi, g[i], mi, vi, clip, lr, beta1, beta2, eps, wd, step_size);
    m[i] = mi; v[i] = vi; p[i] = pi;
  }
}
int adamw_flat(hipStream_t st, float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
               float eps, float weight_decay, float bias_c1, float bias_c2, const float* norm_sq, float max_norm) {
  if (n <= 0) return RL_OK;
  hipLaunchKernelGGL(adamw_kernel, dim3(ew_blocks(n)), dim3(256), 0, st, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay,
                     bias_c1, bias_c2, norm_sq, max_norm);
  return RL_LAUNCH_CHECK();
}

// AdamW with per-group hyper-parameters in ONE launch over the arena (the reference's decay / no-decay parameter groups,
// run.py:146-151, with a non-zero weight decay): group_of_block[i >> 6] names the group of elements [64 b, 64 b + 64) (every tensor
// of the arena starts on a 64-element boundary), 255 = not optimised.
__global__ void adamw_grouped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                     int64_t n, const uint8_t* __restrict__ group_of_block, AdamwGroups gs,
                                     const float* __restrict__ norm_sq, float max_norm, const uint8_t* __restrict__ skip_block) {
  float clip = 1.0f;
  if (norm_sq != nullptr) {
    const float c = max_norm / (sqrtf(norm_sq[0]) + 1e-6f);
    clip = c < 1.0f ? c : 1.0f;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int gid = group_of_block[i >> 6];
    if (gid >= gs.n) continue;
    if (skip_block != nullptr && skip_block[i >> 6]) continue;      // stepped by adamw_cast_multi_kernel (the Linear weights)
    const AdamwGroup h = gs.g[gid];
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_elem(pi, g[i], mi, vi, clip, h);
    m[i] = mi; v[i] = vi; p[i] = pi;
  }
}
int adamw_grouped(hipStream_t st, float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* group_of_block,
                  const AdamwGroups& gs, const float* norm_sq, float max_norm, const uint8_t* skip_block) {
  if (n <= 0) return RL_OK;
  if (gs.n < 1 || gs.n > ADAMW_MAX_GROUPS || group_of_block == nullptr) return RL_ERR_ARG;
  hipLaunchKernelGGL(adamw_grouped_kernel, dim3(ew_blocks(n)), dim3(256), 0, st, p, g, m, v, n, group_of_block, gs, norm_sq, max_norm, skip_block);
  return RL_LAUNCH_CHECK();
}

// the grouped sweep over a chunk list (block b steps chunk b: [off, off + len), len <= 64 Ki floats, 64-element aligned): what the
// tiled launches below do not own
__global__ void __launch_bounds__(256) adamw_chunks_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                           const FillChunk* __restrict__ chunks, const uint8_t* __restrict__ group_of_block, AdamwGroups gs,
                                                           const float* __restrict__ norm_sq, float max_norm) {
  float clip = 1.0f;
  if (norm_sq != nullptr) {
    const float c = max_norm / (sqrtf(norm_sq[0]) + 1e-6f);
    clip = c < 1.0f ? c : 1.0f;
  }
  const FillChunk ch = chunks[blockIdx.x];
  if (threadIdx.x == 0)
    for (int k = ch.len & ~3; k < ch.len; ++k) {          // a tensor whose length is not a multiple of 4 ends the arena
      const int64_t i = ch.off + k;
      const int gid = group_of_block[i >> 6];
      if (gid >= gs.n) continue;
      const AdamwGroup h = gs.g[gid];
      float pi = p[i], mi = m[i], vi = v[i];
      adamw_elem(pi, g[i], mi, vi, clip, h);
      m[i] = mi; v[i] = vi; p[i] = pi;
    }
  for (int k = threadIdx.x * 4; k + 3 < ch.len; k += 1024) {
    const int64_t i = ch.off + k;
    const int gid = group_of_block[i >> 6];
    if (gid >= gs.n) continue;
    const AdamwGroup h = gs.g[gid];
    floatx4 pv = *(const floatx4*)(p + i), mv = *(const floatx4*)(m + i), vv = *(const floatx4*)(v + i);
    const floatx4 gv = *(const floatx4*)(g + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pi = pv[j], mi = mv[j], vi = vv[j];
      adamw_elem(pi, gv[j], mi, vi, clip, h);
      pv[j] = pi; mv[j] = mi; vv[j] = vi;
    }
    *(floatx4*)(m + i) = mv; *(floatx4*)(v + i) = vv; *(floatx4*)(p + i) = pv;
  }
}
int adamw_chunks(hipStream_t st, float* p, const float* g, float* m, float* v, const FillChunk* chunks_dev, int n_chunks,
                 const uint8_t* group_of_block, const AdamwGroups& gs, const float* norm_sq, float max_norm) {
  if (n_chunks <= 0) return RL_OK;
  if (gs.n < 1 || gs.n > ADAMW_MAX_GROUPS || group_of_block == nullptr) return RL_ERR_ARG;
  hipLaunchKernelGGL(adamw_chunks_kernel, dim3(n_chunks), dim3(256), 0, st, p, g, m, v, chunks_dev, group_of_block, gs, norm_sq, max_norm);
  return RL_LAUNCH_CHECK();
}

// AdamW over the Linear weights in the 64 x 64 tiles of cast_transpose_multi: the pass that reads and writes every parameter anyway
// also emits the compute-dtype operand copies W and W^T the next forward / backward multiply with (the transposed copy through a
// padded LDS tile, 128-byte row segments on both sides) - the separate refresh (8 B / parameter of reads + writes, two launches)
// disappears from a FusedAdamW step.  Element (r, c) of descriptor d sits at arena offset (d.src - P0) + r * C + c in p / g / m / v.
template <typename T>
__global__ void __launch_bounds__(256) adamw_cast_multi_kernel(const CastDesc* __restrict__ descs, int n, float* __restrict__ P0,
                                                               const float* __restrict__ G0, float* __restrict__ M0, float* __restrict__ V0,
                                                               const uint8_t* __restrict__ group_of_block, AdamwGroups gs,
                                                               const float* __restrict__ norm_sq, float max_norm, int tile_base) {
  __shared__ float tile[64][65];
  // tile_base (round 6): the launch covers a SLICE of a descriptor group - descs points at the slice's first descriptor, whose
  // tile_begin (counted from the group's first) is tile_base
  const int bid = (int)blockIdx.x + tile_base;
  int lo = 0, hi = n - 1;                               // last descriptor with tile_begin <= bid
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].tile_begin <= bid) lo = mid; else hi = mid - 1;
  }
  const CastDesc d = descs[lo];
  const int t = bid - d.tile_begin;
  const int r0 = (t / d.tiles_c) * 64, c0 = (t % d.tiles_c) * 64;
  const int q = threadIdx.x & 15, y = threadIdx.x >> 4;     // 16 quads x 16 rows per pass
  T* dst = (T*)d.dst;
  T* dstT = (T*)d.dstT;
  const int64_t base = d.src - P0;
  float clip = 1.0f;
  if (norm_sq != nullptr) {
    const float c = max_norm / (sqrtf(norm_sq[0]) + 1e-6f);
    clip = c < 1.0f ? c : 1.0f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + y + 16 * k, c = c0 + 4 * q;
    floatx4 pv = floatx4{0.f, 0.f, 0.f, 0.f};
    if (r < d.R && c < d.C) {                           // C % 4 == 0
      const int64_t e = base + (int64_t)r * d.C + c;
      pv = *(const floatx4*)(P0 + e);
      const int gid = group_of_block[e >> 6];           // a quad never straddles a 64-element block (base % 64 == 0, C % 4 == 0)
      if (gid < gs.n) {
        const AdamwGroup h = gs.g[gid];
        const floatx4 gv = *(const floatx4*)(G0 + e);
        floatx4 mv = *(const floatx4*)(M0 + e), vv = *(const floatx4*)(V0 + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float pi = pv[j], mi = mv[j], vi = vv[j];
          adamw_elem(pi, gv[j], mi, vi, clip, h);
          pv[j] = pi; mv[j] = mi; vv[j] = vi;
        }
        *(floatx4*)(M0 + e) = mv; *(floatx4*)(V0 + e) = vv; *(floatx4*)(P0 + e) = pv;
      }
      if (dst != nullptr) store4<T>(dst + (int64_t)r * d.C + c, pv);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[y + 16 * k][4 * q + j] = pv[j];
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
// The same tile without LDS (round 6): a thread owns a 4 x 4 block - rows r0 + 4 y .. + 3, columns c0 + 4 q .. + 3 - so the transposed
// copy is an in-register transpose (four 8-byte stores of four consecutive W^T columns each), all sixteen 16-byte loads of the thread
// are in flight together, there is no barrier, and - the reason it was written - a workgroup that needs no LDS can share a CU with the
// two 80 KB GEMM workgroups of a running forward (the pipelined sweep, engine.hip adamw_step).  The same adamw_elem per element: the same
// bits (tests/test_optim_edges_gpu.py).
template <typename T>
__global__ void __launch_bounds__(256) adamw_cast_multi_reg_kernel(const CastDesc* __restrict__ descs, int n, float* __restrict__ P0,
                                                                   const float* __restrict__ G0, float* __restrict__ M0, float* __restrict__ V0,
                                                                   const uint8_t* __restrict__ group_of_block, AdamwGroups gs,
                                                                   const float* __restrict__ norm_sq, float max_norm, int tile_base) {
  const int bid = (int)blockIdx.x + tile_base;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].tile_begin <= bid) lo = mid; else hi = mid - 1;
  }
  const CastDesc d = descs[lo];
  const int t = bid - d.tile_begin;
  const int r0 = (t / d.tiles_c) * 64, c0 = (t % d.tiles_c) * 64;
  const int q = threadIdx.x & 15, y = threadIdx.x >> 4;
  T* dst = (T*)d.dst;
  T* dstT = (T*)d.dstT;
  const int64_t base = d.src - P0;
  float clip = 1.0f;
  if (norm_sq != nullptr) {
    const float c = max_norm / (sqrtf(norm_sq[0]) + 1e-6f);
    clip = c < 1.0f ? c : 1.0f;
  }
  const int c = c0 + 4 * q, rb = r0 + 4 * y;
  if (c >= d.C || rb >= d.R) return;
  floatx4 pv[4], gv[4], mv[4], vv[4];
  int gid[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = rb + k;
    pv[k] = floatx4{0.f, 0.f, 0.f, 0.f}; gid[k] = 255;
    if (r < d.R) {
      const int64_t e = base + (int64_t)r * d.C + c;
      pv[k] = *(const floatx4*)(P0 + e);
      gid[k] = group_of_block[e >> 6];
      if (gid[k] < gs.n) { gv[k] = *(const floatx4*)(G0 + e); mv[k] = *(const floatx4*)(M0 + e); vv[k] = *(const floatx4*)(V0 + e); }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = rb + k;
    if (r >= d.R) continue;
    const int64_t e = base + (int64_t)r * d.C + c;
    if (gid[k] < gs.n) {
      const AdamwGroup h = gs.g[gid[k]];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pi = pv[k][j], mi = mv[k][j], vi = vv[k][j];
        adamw_elem(pi, gv[k][j], mi, vi, clip, h);
        pv[k][j] = pi; mv[k][j] = mi; vv[k][j] = vi;
      }
      *(floatx4*)(M0 + e) = mv[k]; *(floatx4*)(V0 + e) = vv[k]; *(floatx4*)(P0 + e) = pv[k];
    }
    if (dst != nullptr) store4<T>(dst + (int64_t)r * d.C + c, pv[k]);
  }
  if (dstT == nullptr) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const floatx4 v = floatx4{pv[0][j], pv[1][j], pv[2][j], pv[3][j]};
    if (rb + 3 < d.R && (d.ldT & 3) == 0) store4<T>(dstT + (int64_t)(c + j) * d.ldT + rb, v);
    else for (int k = 0; k < 4 && rb + k < d.R; ++k) dstT[(int64_t)(c + j) * d.ldT + rb + k] = from_f<T>(v[k]);
  }
}

template <typename T>
int adamw_cast_multi(hipStream_t st, const CastDesc* descs, int n, int total_tiles, float* P0, const float* G0, float* M0, float* V0,
                     const uint8_t* group_of_block, const AdamwGroups& gs, const float* norm_sq, float max_norm, int tile_base) {
  if (n <= 0 || total_tiles <= 0) return RL_OK;
  if (gs.n < 1 || gs.n > ADAMW_MAX_GROUPS || group_of_block == nullptr) return RL_ERR_ARG;
  if (g_adamw_reg) hipLaunchKernelGGL((adamw_cast_multi_reg_kernel<T>), dim3(total_tiles), dim3(256), 0, st, descs, n, P0, G0, M0, V0, group_of_block, gs, norm_sq, max_norm, tile_base);
  else hipLaunchKernelGGL((adamw_cast_multi_kernel<T>), dim3(total_tiles), dim3(256), 0, st, descs, n, P0, G0, M0, V0, group_of_block, gs, norm_sq, max_norm, tile_base);
  return RL_LAUNCH_CHECK();
}
template int adamw_cast_multi<bf16_t>(hipStream_t, const CastDesc*, int, int, float*, const float*, float*, float*, const uint8_t*, const AdamwGroups&, const float*, float, int);
template int adamw_cast_multi<float>(hipStream_t, const CastDesc*, int, int, float*, const float*, float*, float*, const uint8_t*, const AdamwGroups&, const float*, float, int);

// g *= min(1, max_norm / (sqrt(*norm_sq) + 1e-6)) - the in-place half of clip_grad_norm_ (run.py:207) for callers that step with a
// stock optimizer (FusedAdamW applies the coefficient inside its own sweep instead)
__global__ void clip_scale_kernel(float* __restrict__ g, int64_t n, const float* __restrict__ norm_sq, float max_norm) {
  const float c = max_norm / (sqrtf(norm_sq[0]) + 1e-6f);
  if (c >= 1.0f) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) g[i] *= c;
}
int clip_scale(hipStream_t st, float* g, int64_t n, const float* norm_sq, float max_norm) {
  if (n <= 0) return RL_OK;
  hipLaunchKernelGGL(clip_scale_kernel, dim3(ew_blocks(n)), dim3(256), 0, st, g, n, norm_sq, max_norm);
  return RL_LAUNCH_CHECK();
}

// zero several ranges of one arena in ONE launch: block b clears chunk b = [off[b], off[b] + len[b]) (chunks <= 1 Mi floats)
__global__ void __launch_bounds__(256) zero_chunks_kernel(float* __restrict__ base, const FillChunk* __restrict__ chunks) {
  const FillChunk c = chunks[blockIdx.x];
  float* p = base + c.off;
  const int n4 = c.len >> 2;
  for (int i = threadIdx.x; i < n4; i += 256) ((floatx4*)p)[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += 256) p[i] = 0.f;
}
int zero_chunks(hipStream_t st, float* base, const FillChunk* chunks_dev, int n) {
  if (n <= 0) return RL_OK;
  hipLaunchKernelGGL(zero_chunks_kernel, dim3(n), dim3(256), 0, st, base, chunks_dev);
  return RL_LAUNCH_CHECK();
}

__global__ void fill_kernel(float* p, float v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}
int fill_f32(hipStream_t st, float* p, float v, int64_t n) {
  if (n <= 0) return RL_OK;
  hipLaunchKernelGGL(fill_kernel, dim3(ew_blocks(n)), dim3(256), 0, st, p, v, n);
  return RL_LAUNCH_CHECK();
}
__global__ void add_i64_kernel(int64_t* p, int64_t v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] += v;
}
int add_i64(hipStream_t st, int64_t* p, int64_t v, int n) {
  hipLaunchKernelGGL(add_i64_kernel, dim3((n + 63) / 64), dim3(64), 0, st, p, v, n);
  return RL_LAUNCH_CHECK();
}

}  // namespace rl
