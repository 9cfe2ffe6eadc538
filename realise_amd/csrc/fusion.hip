// Fusion of the three branches (K11; the "fusion" section of ops.h): the gate family - the masked mean, the forward per number of
// sources and activation (sigmoids / one softmax), the three backward kernels - and the plain sum fusion.  One wave per token row,
// rows up to LN_MAXV x 256 columns (rows.h).
#include "ops.h"
#include "launch.h"
#include "rows.h"

namespace rl {

// ---------------------------------------------------------------------------------------------
// Gate fusion (models.py:840-850).  The [T, 4H] concat is never materialised.
// ---------------------------------------------------------------------------------------------
// masked mean of the bert states of a sentence (models.py:842-843).  grid (H / 256, B), 256 threads = 64 column quads x 4 row lanes:
// a thread walks S / 4 rows, the four lanes meet in LDS (one thread per column quad walking all S rows serially took 53 us for
// 12.6 MB; this form ~10).  Row lane order and the final 4-way sum are fixed: deterministic.
template <typename T>
__global__ void __launch_bounds__(256) gate_mean_kernel(GateArgs<T> a) {
  __shared__ floatx4 part[4][64];
  __shared__ float mpart[4];
  const int q = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + q) * 4;
  const int b = blockIdx.y;
  floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
  float ms = 0.f;
  for (int s = rl; s < a.S; s += 4) {
    const float m = (float)a.masks[b * a.S + s];
    ms += m;
    // (select, not multiply: a masked row of a live-row step holds whatever an earlier step left there - 0 * NaN must not get in)
    if (c < a.H && m != 0.f) acc += load4<T>(a.bert + ((int64_t)b * a.S + s) * a.H + c) * m;
  }
  part[rl][q] = acc;
  if (q == 0) mpart[rl] = ms;
  __syncthreads();
  if (rl == 0) {
    const float msum = (mpart[0] + mpart[1]) + (mpart[2] + mpart[3]);
    if (c < a.H) *(floatx4*)(a.mean + (int64_t)b * a.H + c) = ((part[0][q] + part[1][q]) + (part[2][q] + part[3][q])) / msum;
    if (c == 0) a.msum[b] = msum;
  }
}

// The gate family is instantiated per number of sources NSRC (src/models_abla.py:239-275): bert, then pho and res where present.
// W rows are (NSRC + 1) H wide, [src 0 | ... | src NSRC-1 | mean]; g / dz rows keep a pitch of 4 (unused slots hold 0).  NSRC = 3 is
// SpellBertPho2ResArch3 and performs the same operations in the same order as the three-source kernels always did.
// SM (GateArgs::softmax) selects the activation over the NSRC pre-activations z: false = independent sigmoids (models.py:843-848),
// true = one softmax over them (SpellBertPho2ResArch4, models.py:1139-1150).  The sigmoid instantiations compile what they always did.
template <typename T, int NSRC> __device__ __forceinline__ void gate_sources(const GateArgs<T>& a, const T* (&x)[NSRC]) {
  x[0] = a.bert;
  if constexpr (NSRC == 3) { x[1] = a.pho; x[2] = a.res; }
  if constexpr (NSRC == 2) x[1] = a.pho != nullptr ? a.pho : a.res;
}
template <typename T, int NSRC> __device__ __forceinline__ void gate_grads(const GateArgs<T>& a, T* (&d)[NSRC]) {
  d[0] = a.dbert;
  if constexpr (NSRC == 3) { d[1] = a.dpho; d[2] = a.dres; }
  if constexpr (NSRC == 2) d[1] = a.pho != nullptr ? a.dpho : a.dres;
}

template <typename T, int NSRC, bool SM>
__global__ void __launch_bounds__(256) gate_fwd_kernel(GateArgs<T> a) {   // one wave per token
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= a.B * a.S) return;
  const int H = a.H, b = row / a.S;
  const T* src[NSRC];
  gate_sources<T, NSRC>(a, src);
  floatx4 xs[NSRC][LN_MAXV];
  float z[NSRC];
#pragma unroll
  for (int k = 0; k < NSRC; ++k) z[k] = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
#pragma unroll
      for (int d = 0; d < NSRC; ++d) xs[d][i] = load4<T>(src[d] + (int64_t)row * H + c);
      const floatx4 xm = *(const floatx4*)(a.mean + (int64_t)b * H + c);
#pragma unroll
      for (int k = 0; k < NSRC; ++k) {
        const float* w = a.W + (int64_t)k * (NSRC + 1) * H + c;
        floatx4 wd[NSRC + 1];
#pragma unroll
        for (int d = 0; d <= NSRC; ++d) wd[d] = *(const floatx4*)(w + d * H);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float t = wd[0][j] * xs[0][i][j];
#pragma unroll
          for (int d = 1; d < NSRC; ++d) t = t + wd[d][j] * xs[d][i][j];
          z[k] += t + wd[NSRC][j] * xm[j];
        }
      }
    }
  }
  float gk[NSRC];
#pragma unroll
  for (int k = 0; k < NSRC; ++k) {
    if constexpr (SM) gk[k] = wave_sum(z[k]) + a.bias[k];
    else gk[k] = sigmoidf_(wave_sum(z[k]) + a.bias[k]);
  }
  if constexpr (SM) {      // softmax over the NSRC pre-activations, row maximum subtracted (torch.softmax): every exponent is <= 0
    float zmax = gk[0], den = 0.f;
#pragma unroll
    for (int k = 1; k < NSRC; ++k) zmax = fmaxf(zmax, gk[k]);
#pragma unroll
    for (int k = 0; k < NSRC; ++k) { gk[k] = expf(gk[k] - zmax); den += gk[k]; }
#pragma unroll
    for (int k = 0; k < NSRC; ++k) gk[k] = gk[k] / den;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.g[row * 4 + k] = k < NSRC ? gk[k < NSRC ? k : 0] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      floatx4 f = xs[0][i] * gk[0];
#pragma unroll
      for (int d = 1; d < NSRC; ++d) f = f + xs[d][i] * gk[d];
      store4<T>(a.fused + (int64_t)row * H + c, f);
    }
  }
}
template <typename T> static bool gate_args_ok(const GateArgs<T>& a) {
  if ((a.H & 3) || a.H > LN_MAXV * 256 || a.nsrc < 1 || a.nsrc > 3) return false;
  if (a.nsrc == 3) return a.pho != nullptr && a.res != nullptr;
  if (a.nsrc == 2) return (a.pho != nullptr) != (a.res != nullptr);
  return true;
}
template <typename T> int gate_fwd(hipStream_t st, const GateArgs<T>& a) {
  if (!gate_args_ok(a)) return RL_ERR_ARG;
  hipLaunchKernelGGL((gate_mean_kernel<T>), dim3((a.H / 4 + 63) / 64, a.B), dim3(256), 0, st, a);
  const dim3 grid((a.B * a.S + 3) / 4);
  if (a.softmax) {
    switch (a.nsrc) {
      case 3: hipLaunchKernelGGL((gate_fwd_kernel<T, 3, true>), grid, dim3(256), 0, st, a); break;
      case 2: hipLaunchKernelGGL((gate_fwd_kernel<T, 2, true>), grid, dim3(256), 0, st, a); break;
      default: hipLaunchKernelGGL((gate_fwd_kernel<T, 1, true>), grid, dim3(256), 0, st, a); break;
    }
  } else {
    switch (a.nsrc) {
      case 3: hipLaunchKernelGGL((gate_fwd_kernel<T, 3, false>), grid, dim3(256), 0, st, a); break;
      case 2: hipLaunchKernelGGL((gate_fwd_kernel<T, 2, false>), grid, dim3(256), 0, st, a); break;
      default: hipLaunchKernelGGL((gate_fwd_kernel<T, 1, false>), grid, dim3(256), 0, st, a); break;
    }
  }
  return RL_LAUNCH_CHECK();
}
template int gate_fwd<bf16_t>(hipStream_t, const GateArgs<bf16_t>&);
template int gate_fwd<float>(hipStream_t, const GateArgs<float>&);

// backward, step 1 (per token): dz_k and the direct parts of the source gradients
template <typename T, int NSRC, bool SM>
__global__ void __launch_bounds__(256) gate_bwd_token_kernel(GateArgs<T> a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= a.B * a.S) return;
  const int H = a.H;
  T* dst[NSRC];
  gate_grads<T, NSRC>(a, dst);
  if (a.row_live != nullptr && a.row_live[row] == 0) {      // padding row: d fused is an exact zero, so is everything derived from it
    if (lane == 0) *(floatx4*)(a.dz + (int64_t)row * 4) = floatx4{0.f, 0.f, 0.f, 0.f};
    const floatx4 z4 = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
#pragma unroll
        for (int d = 0; d < NSRC; ++d) store4<T>(dst[d] + (int64_t)row * H + c, z4);
      }
    }
    return;
  }
  const T* src[NSRC];
  gate_sources<T, NSRC>(a, src);
  floatx4 df[LN_MAXV];
  float dg[NSRC];
#pragma unroll
  for (int d = 0; d < NSRC; ++d) dg[d] = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      df[i] = load4<T>(a.dfused + (int64_t)row * H + c);
      floatx4 x[NSRC];
#pragma unroll
      for (int d = 0; d < NSRC; ++d) x[d] = load4<T>(src[d] + (int64_t)row * H + c);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int d = 0; d < NSRC; ++d) dg[d] += df[i][j] * x[d][j];
    }
  }
  float gk[NSRC], dz[NSRC];
#pragma unroll
  for (int k = 0; k < NSRC; ++k) {
    gk[k] = a.g[row * 4 + k];
    if constexpr (SM) dz[k] = wave_sum(dg[k]);
    else dz[k] = wave_sum(dg[k]) * gk[k] * (1.0f - gk[k]);
  }
  if constexpr (SM) {      // softmax: dz_k = g_k (dg_k - sum_j g_j dg_j)
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < NSRC; ++k) dot += gk[k] * dz[k];
#pragma unroll
    for (int k = 0; k < NSRC; ++k) dz[k] = gk[k] * (dz[k] - dot);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.dz[row * 4 + k] = k < NSRC ? dz[k < NSRC ? k : 0] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      floatx4 o[NSRC];
#pragma unroll
      for (int d = 0; d < NSRC; ++d) o[d] = df[i] * gk[d];
#pragma unroll
      for (int k = 0; k < NSRC; ++k) {
        const float* w = a.W + (int64_t)k * (NSRC + 1) * H + c;
#pragma unroll
        for (int d = 0; d < NSRC; ++d) o[d] += *(const floatx4*)(w + d * H) * dz[k];
      }
#pragma unroll
      for (int d = 0; d < NSRC; ++d) store4<T>(dst[d] + (int64_t)row * H + c, o[d]);
    }
  }
}
// step 2 (per sentence): d(mean) -> spread over the masked tokens of dbert, and dW[:, NSRC H:(NSRC + 1) H] += sum_s dz * mean.
// grid (H / 256, B), 256 threads = 64 column quads x 4 row lanes (the row walk over S is split four ways).
template <typename T, int NSRC>
__global__ void __launch_bounds__(256) gate_bwd_mean_kernel(GateArgs<T> a) {
  __shared__ float zpart[4][4];
  const int q = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + q) * 4;
  const int b = blockIdx.y;
  const int H = a.H;
  constexpr int WP = NSRC + 1;                   // W row pitch in units of H
  if (q < NSRC) {                                // lane q of row lane rl: partial sum of dz_q over its rows
    float z = 0.f;
    for (int s = rl; s < a.S; s += 4) z += a.dz[((int64_t)b * a.S + s) * 4 + q];
    zpart[rl][q] = z;
  }
  __syncthreads();
  float zs[NSRC];
#pragma unroll
  for (int k = 0; k < NSRC; ++k) zs[k] = (zpart[0][k] + zpart[1][k]) + (zpart[2][k] + zpart[3][k]);
  if (c >= H) return;
  floatx4 dm = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < NSRC; ++k) dm += *(const floatx4*)(a.W + (int64_t)k * WP * H + NSRC * H + c) * zs[k];
  if (rl == 0) {
    const floatx4 mean = *(const floatx4*)(a.mean + (int64_t)b * H + c);
#pragma unroll
    for (int k = 0; k < NSRC; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(a.dW + (int64_t)k * WP * H + NSRC * H + c + j, zs[k] * mean[j]);
    if (c == 0)
#pragma unroll
      for (int k = 0; k < NSRC; ++k) atomicAdd(a.dbias + k, zs[k]);
  }
  dm = dm / a.msum[b];
  for (int s = rl; s < a.S; s += 4) {
    const int64_t m = a.masks[b * a.S + s];
    if (m != 0) {
      T* p = a.dbert + ((int64_t)b * a.S + s) * H + c;
      store4<T>(p, load4<T>(p) + dm * (float)m);
    }
  }
}
// step 3: dW[k, src H + c] += sum_t dz_k[t] * X_src(t, c) for every source and gate in ONE pass over the sources
// (was nine column reductions, each re-reading one source: 190 us of launches at the join of the three branches).
// grid (H / 128, row chunks), 256 threads = 32 column quads x 8 row lanes; NSRC x NSRC float4 accumulators per thread; atomics at the end.
template <typename T, int NSRC>
__global__ void __launch_bounds__(256) gate_dw_kernel(GateArgs<T> a, int rows_per_block) {
  __shared__ floatx4 red[8][32];
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int c = (blockIdx.x * 32 + cx) * 4;
  const int H = a.H, T_ = a.B * a.S;
  const int r0 = blockIdx.y * rows_per_block, r1 = min(T_, r0 + rows_per_block);
  const T* src[NSRC];
  gate_sources<T, NSRC>(a, src);
  floatx4 acc[NSRC][NSRC];
#pragma unroll
  for (int s = 0; s < NSRC; ++s)
#pragma unroll
    for (int k = 0; k < NSRC; ++k) acc[s][k] = floatx4{0.f, 0.f, 0.f, 0.f};
  if (c < H) {
    for (int r = r0 + ry; r < r1; r += 8) {
      const floatx4 dz = *(const floatx4*)(a.dz + (int64_t)r * 4);
      bool zero = true;
#pragma unroll
      for (int k = 0; k < NSRC; ++k) zero = zero && dz[k] == 0.f;
      if (zero) continue;      // padding rows (and any other all-zero row): nothing to add, nothing read
      floatx4 x[NSRC];
#pragma unroll
      for (int s = 0; s < NSRC; ++s) x[s] = load4<T>(src[s] + (int64_t)r * H + c);
#pragma unroll
      for (int s = 0; s < NSRC; ++s)
#pragma unroll
        for (int k = 0; k < NSRC; ++k) acc[s][k] += x[s] * dz[k];
    }
  }
#pragma unroll
  for (int s = 0; s < NSRC; ++s)
#pragma unroll
    for (int k = 0; k < NSRC; ++k) {
      __syncthreads();
      red[ry][cx] = acc[s][k];
      __syncthreads();
      if (ry == 0 && c < H) {
        floatx4 v = red[0][cx];
#pragma unroll
        for (int j = 1; j < 8; ++j) v += red[j][cx];
        float* o = a.dW + (int64_t)k * (NSRC + 1) * H + (int64_t)s * H + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(o + j, v[j]);
      }
    }
}
template <typename T, int NSRC> static void gate_bwd_launch(hipStream_t st, const GateArgs<T>& a) {
  const int T_ = a.B * a.S;
  if (a.softmax) hipLaunchKernelGGL((gate_bwd_token_kernel<T, NSRC, true>), dim3((T_ + 3) / 4), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((gate_bwd_token_kernel<T, NSRC, false>), dim3((T_ + 3) / 4), dim3(256), 0, st, a);
  hipLaunchKernelGGL((gate_bwd_mean_kernel<T, NSRC>), dim3((a.H / 4 + 63) / 64, a.B), dim3(256), 0, st, a);
  const int gx = (a.H + 127) / 128;
  int gy = 1024 / gx;
  if (gy > (T_ + 31) / 32) gy = (T_ + 31) / 32;
  if (gy < 1) gy = 1;
  const int rows_per_block = (T_ + gy - 1) / gy;
  hipLaunchKernelGGL((gate_dw_kernel<T, NSRC>), dim3(gx, gy), dim3(256), 0, st, a, rows_per_block);
}
template <typename T> int gate_bwd(hipStream_t st, const GateArgs<T>& a) {
  if (!gate_args_ok(a)) return RL_ERR_ARG;
  if (a.nsrc == 2 && (a.pho != nullptr ? a.dpho : a.dres) == nullptr) return RL_ERR_ARG;
  switch (a.nsrc) {
    case 3: gate_bwd_launch<T, 3>(st, a); break;
    case 2: gate_bwd_launch<T, 2>(st, a); break;
    default: gate_bwd_launch<T, 1>(st, a); break;
  }
  return RL_LAUNCH_CHECK();
}
template int gate_bwd<bf16_t>(hipStream_t, const GateArgs<bf16_t>&);
template int gate_bwd<float>(hipStream_t, const GateArgs<float>&);

// ---------------------------------------------------------------------------------------------
// Sum fusion (src/models_abla.py:278-279): hiddens = bert + pho + res, evaluated left to right in fp32 as torch does.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) sum_fuse_fwd_kernel(const T* bert, const T* pho, const T* res, T* fused, int rows, int H) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;      // one wave per token row
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  for (int c = lane * 4; c < H; c += 256) {
    const int64_t o = (int64_t)row * H + c;
    store4<T>(fused + o, (load4<T>(bert + o) + load4<T>(pho + o)) + load4<T>(res + o));
  }
}
// The backward hands the same d fused to every branch.  Not aliased: the bert and pinyin stacks' backwards overwrite their incoming
// gradient buffer in place (layers_backward: d output in, d input out) and run concurrently, so each branch gets its own copy.
// row_live (nullable): a padding row (0) gets exact zeros without its d fused row being read, as the gate backward does.
template <typename T>
__global__ void __launch_bounds__(256) sum_fuse_bwd_kernel(const T* dfused, T* dbert, T* dpho, T* dres, int rows, int H, const uint8_t* row_live) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const bool live = row_live == nullptr || row_live[row] != 0;
  for (int c = lane * 4; c < H; c += 256) {
    const int64_t o = (int64_t)row * H + c;
    const floatx4 d = live ? load4<T>(dfused + o) : floatx4{0.f, 0.f, 0.f, 0.f};
    store4<T>(dbert + o, d);
    store4<T>(dpho + o, d);
    store4<T>(dres + o, d);
  }
}
template <typename T> int sum_fuse_fwd(hipStream_t st, const T* bert, const T* pho, const T* res, T* fused, int rows, int H) {
  if (!bert || !pho || !res || !fused || rows < 1 || H < 4 || (H & 3)) return RL_ERR_ARG;
  hipLaunchKernelGGL((sum_fuse_fwd_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, st, bert, pho, res, fused, rows, H);
  return RL_LAUNCH_CHECK();
}
template <typename T> int sum_fuse_bwd(hipStream_t st, const T* dfused, T* dbert, T* dpho, T* dres, int rows, int H, const uint8_t* row_live) {
  if (!dfused || !dbert || !dpho || !dres || rows < 1 || H < 4 || (H & 3)) return RL_ERR_ARG;
  hipLaunchKernelGGL((sum_fuse_bwd_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, st, dfused, dbert, dpho, dres, rows, H, row_live);
  return RL_LAUNCH_CHECK();
}
template int sum_fuse_fwd<bf16_t>(hipStream_t, const bf16_t*, const bf16_t*, const bf16_t*, bf16_t*, int, int);
template int sum_fuse_fwd<float>(hipStream_t, const float*, const float*, const float*, float*, int, int);
template int sum_fuse_bwd<bf16_t>(hipStream_t, const bf16_t*, bf16_t*, bf16_t*, bf16_t*, int, int, const uint8_t*);
template int sum_fuse_bwd<float>(hipStream_t, const float*, float*, float*, float*, int, int, const uint8_t*);

}  // namespace rl
