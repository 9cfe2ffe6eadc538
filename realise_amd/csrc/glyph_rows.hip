// Rows of the glyph branch, which runs once per DISTINCT token id of the batch (the "glyph rows" section of ops.h): the dedup
// bookkeeping (glyph_unique), the segment sum back onto the distinct glyphs, the image gather, the per-token gather of glyph rows, and
// the three _chw4 operators that carry the NCHW flatten of a 2x2 top map (ln_fwd_chw4 among them: it needs only LnFwdArgs and wave_sum).
#include "ops.h"
#include "launch.h"
#include "rows.h"

namespace rl {

// ---- knob (ops.h: set_glyph_dedup) ----
static int g_glyph_dedup = 1;
void set_glyph_dedup(int on) { g_glyph_dedup = on; }

// ---------------------------------------------------------------------------------------------
// Glyph dedup: distinct token ids of the batch in order of first occurrence (deterministic).
// ---------------------------------------------------------------------------------------------
__global__ void gu_clear_kernel(int* first, int V, float* counts, int T_) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < V) first[i] = 0x7fffffff;
  if (i < T_) counts[i] = 0.f;
}
__global__ void gu_first_kernel(const int64_t* __restrict__ ids, int T_, int* first) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < T_) atomicMin(first + (int)ids[t], t);
}
// single workgroup: exclusive scan of is_first over t -> slot of every first occurrence
__global__ void __launch_bounds__(1024) gu_scan_kernel(const int64_t* __restrict__ ids, int T_, const int* __restrict__ first,
                                                       int* slot_of_t, int64_t* uniq_ids, int* bounds, HwList hw) {
  __shared__ int wsum[16];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int base = 0; base < T_; base += 1024) {
    const int t = base + threadIdx.x;
    const int flag = (t < T_ && first[(int)ids[t]] == t) ? 1 : 0;
    int v = flag;                                   // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int n = __shfl_up(v, o, 64); if (lane >= o) v += n; }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int off = carry;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    const int excl = off + v - flag;
    if (t < T_) {
      slot_of_t[t] = flag ? excl : -1;
      if (flag) uniq_ids[excl] = ids[t];
    }
    __syncthreads();
    if (threadIdx.x == 1023) carry = off + v;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int U = carry;
    bounds[0] = U;
    for (int k = 0; k < hw.n; ++k) bounds[1 + k] = U * hw.v[k];
  }
}
__global__ void gu_final_kernel(const int64_t* __restrict__ ids, int T_, const int* __restrict__ first, const int* __restrict__ slot_of_t,
                                int* inv, float* counts) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T_) return;
  const int s = slot_of_t[first[(int)ids[t]]];
  inv[t] = s;
  atomicAdd(counts + s, 1.0f);
}
__global__ void gu_identity_kernel(const int64_t* __restrict__ ids, int T_, int64_t* uniq_ids, float* counts, int* inv, int* bounds, HwList hw) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < T_) { uniq_ids[t] = ids[t]; counts[t] = 1.0f; inv[t] = t; }
  if (t == 0) { bounds[0] = T_; for (int k = 0; k < hw.n; ++k) bounds[1 + k] = T_ * hw.v[k]; }
}
int glyph_unique(hipStream_t st, const int64_t* ids, int T_, int V, int* first_scratch, int* flag_scratch, int64_t* uniq_ids,
                 float* counts, int* inv, int* bounds, HwList hw) {
  if (!g_glyph_dedup) {
    hipLaunchKernelGGL(gu_identity_kernel, dim3((T_ + 255) / 256), dim3(256), 0, st, ids, T_, uniq_ids, counts, inv, bounds, hw);
    return RL_LAUNCH_CHECK();
  }
  const int n = V > T_ ? V : T_;
  hipLaunchKernelGGL(gu_clear_kernel, dim3((n + 255) / 256), dim3(256), 0, st, first_scratch, V, counts, T_);
  hipLaunchKernelGGL(gu_first_kernel, dim3((T_ + 255) / 256), dim3(256), 0, st, ids, T_, first_scratch);
  hipLaunchKernelGGL(gu_scan_kernel, dim3(1), dim3(1024), 0, st, ids, T_, first_scratch, flag_scratch, uniq_ids, bounds, hw);
  hipLaunchKernelGGL(gu_final_kernel, dim3((T_ + 255) / 256), dim3(256), 0, st, ids, T_, first_scratch, flag_scratch, inv, counts);
  return RL_LAUNCH_CHECK();
}

template <typename T>
__global__ void segsum_scatter_kernel(const T* __restrict__ x, const int* __restrict__ inv, int T_, int C, float* acc) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int t = blockIdx.y;
  if (c >= C) return;
  const floatx4 v = load4<T>(x + (int64_t)t * C + c);
  if (quad_is_zero(v)) return;                       // padded tokens: exact zeros, all on the slot of token id 0
  float* o = acc + (int64_t)inv[t] * C + c;
#pragma unroll
  for (int j = 0; j < 4; ++j) atomicAdd(o + j, v[j]);
}
template <typename T>
__global__ void segsum_cast_kernel(const float* __restrict__ acc, T* __restrict__ out, int C, const int* __restrict__ nuniq) {
  const int64_t n = (int64_t)(*nuniq) * C;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * blockDim.x * 4)
    store4<T>(out + i, *(const floatx4*)(acc + i));
}
template <typename T> int segment_sum(hipStream_t st, const T* x, const int* inv, int T_, int C, float* acc, T* out, const int* nuniq_dev) {
  if (C & 3) return RL_ERR_ARG;
  (void)hipMemsetAsync(acc, 0, (size_t)T_ * C * sizeof(float), st);
  hipLaunchKernelGGL((segsum_scatter_kernel<T>), dim3((C / 4 + 63) / 64, T_), dim3(64), 0, st, x, inv, T_, C, acc);
  hipLaunchKernelGGL((segsum_cast_kernel<T>), dim3(1024), dim3(256), 0, st, acc, out, C, nuniq_dev);
  return RL_LAUNCH_CHECK();
}
template int segment_sum<bf16_t>(hipStream_t, const bf16_t*, const int*, int, int, float*, bf16_t*, const int*);
template int segment_sum<float>(hipStream_t, const float*, const int*, int, int, float*, float*, const int*);

// dense[u] = table[ids[u]] for the U distinct glyphs of the batch (one contiguous NHWC image each): the block-1 convolutions and
// their weight gradients then address images by slot, without the id indirection in their gather loops
template <typename T>
__global__ void __launch_bounds__(256) gather_images_kernel(const T* __restrict__ table, const int64_t* __restrict__ ids,
                                                            const int* __restrict__ nuniq, int64_t elems, T* __restrict__ dense) {
  const int u = blockIdx.x;
  if (u >= *nuniq) return;
  const uint4* s = (const uint4*)(table + ids[u] * elems);
  uint4* d = (uint4*)(dense + (int64_t)u * elems);
  const int n16 = (int)(elems * sizeof(T) / 16);
  for (int i = threadIdx.x; i < n16; i += 256) d[i] = s[i];
}
template <typename T> int gather_images(hipStream_t st, const T* table, const int64_t* ids, const int* nuniq, int max_images, int64_t elems, T* dense) {
  if ((elems * sizeof(T)) & 15) return RL_ERR_ARG;
  hipLaunchKernelGGL((gather_images_kernel<T>), dim3(max_images), dim3(256), 0, st, table, ids, nuniq, elems, dense);
  return RL_LAUNCH_CHECK();
}
template int gather_images<bf16_t>(hipStream_t, const bf16_t*, const int64_t*, const int*, int, int64_t, bf16_t*);
template int gather_images<float>(hipStream_t, const float*, const int64_t*, const int*, int, int64_t, float*);

// out[t, :] = x[inv[t], :]  (per-distinct-glyph rows back to per-token rows; the glyph-only entry point, BASELINE configs[3])
template <typename T>
__global__ void gather_rows_kernel(const T* __restrict__ x, const int* __restrict__ inv, int T_, int C, T* __restrict__ out) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int t = blockIdx.y;
  if (c >= C) return;
  store4<T>(out + (int64_t)t * C + c, load4<T>(x + (int64_t)inv[t] * C + c));
}
template <typename T> int gather_rows(hipStream_t st, const T* x, const int* inv, int T_, int C, T* out) {
  if (C & 3) return RL_ERR_ARG;
  hipLaunchKernelGGL((gather_rows_kernel<T>), dim3((C / 4 + 63) / 64, T_), dim3(64), 0, st, x, inv, T_, C, out);
  return RL_LAUNCH_CHECK();
}
template int gather_rows<bf16_t>(hipStream_t, const bf16_t*, const int*, int, int, bf16_t*);
template int gather_rows<float>(hipStream_t, const float*, const int*, int, int, float*);

// ---------------------------------------------------------------------------------------------
// The NCHW flatten of a 2x2 top map (CharResNet1, char_cnn.py:74 `h.view(h.shape[0], -1)` of [N, C, 2, 2]): the tower keeps its maps
// NHWC, a row of the top is [p][c] (p = 2y + x, storage index p * C + c) and its consumers need feature f = c * 4 + p.  The three
// kernels at that boundary carry the permutation themselves, so no launch exists only to permute: one 64-lane wave per row, lane l
// owns channels 4l .. 4l + 3 = the 16 consecutive features 16l .. 16l + 15.  It reads its channels as one 4-wide access per pixel
// (contiguous across the lanes), transposes the 4 x 4 block in registers and touches the feature-ordered side as 16 consecutive
// elements - both global sides stay contiguous, no strided scatter.  H = 4 C, C % 4 == 0, H <= 1024.
// ---------------------------------------------------------------------------------------------
static inline bool chw4_ok(int H) { return H >= 16 && (H & 15) == 0 && H <= 1024; }
// resnet_layernorm (models.py:838) over rows read in storage order (through row_index: the glyph dedup gather): the statistics do not
// depend on the order; gamma / beta are applied and y / xhat stored at the feature index, so the backward is the plain ln_bwd
template <typename T>
__global__ void __launch_bounds__(256) ln_fwd_chw4_kernel(LnFwdArgs<T> a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= a.rows) return;
  const int H = a.H, C = H >> 2, c0 = lane * 4;
  const bool on = c0 < C;
  const T* src = a.x + (int64_t)(a.row_index ? a.row_index[row] : row) * H;
  floatx4 q[4];
  float sum = 0.f;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    q[p] = on ? load4<T>(src + p * C + c0) : floatx4{0.f, 0.f, 0.f, 0.f};
    sum += q[p][0] + q[p][1] + q[p][2] + q[p][3];
  }
  const float mean = wave_sum(sum) / (float)H;
  float sq = 0.f;
  if (on) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = q[p][j] - mean; sq += d * d; }
  }
  const float var = wave_sum(sq) / (float)H;
  const float rstd = 1.0f / sqrtf(var + a.eps);
  if (lane == 0 && a.rstd != nullptr) a.rstd[row] = rstd;
  if (!on) return;
  const int64_t o = (int64_t)row * H + 4 * c0;          // channel c0 + j owns features 4 (c0 + j) + p
#pragma unroll
  for (int j = 0; j < 4; j += 2) {
    floatx4 xh[2], y[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const floatx4 gm = *(const floatx4*)(a.gamma + 4 * (c0 + j + h)), bt = *(const floatx4*)(a.beta + 4 * (c0 + j + h));
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        xh[h][p] = (q[p][j + h] - mean) * rstd;
        y[h][p] = xh[h][p] * gm[p] + bt[p];
      }
    }
    if (a.xhat != nullptr) store8<T>(a.xhat + o + 4 * j, xh[0], xh[1]);
    store8<T>(a.y + o + 4 * j, y[0], y[1]);
  }
}
template <typename T> int ln_fwd_chw4(hipStream_t st, const LnFwdArgs<T>& a) {
  if (a.rows <= 0) return RL_OK;
  if (!chw4_ok(a.H) || a.in_mode != 0 || a.drop.thresh != 0u || a.row_live != nullptr) return RL_ERR_ARG;
  hipLaunchKernelGGL((ln_fwd_chw4_kernel<T>), dim3((a.rows + 3) / 4), dim3(256), 0, st, a);
  return RL_LAUNCH_CHECK();
}
template int ln_fwd_chw4<bf16_t>(hipStream_t, const LnFwdArgs<bf16_t>&);
template int ln_fwd_chw4<float>(hipStream_t, const LnFwdArgs<float>&);

// out[t][c * 4 + p] = x[inv[t]][p * C + c]: gather_rows with the flatten (the glyph-only entry point)
template <typename T>
__global__ void __launch_bounds__(256) gather_rows_chw4_kernel(const T* __restrict__ x, const int* __restrict__ inv, int T_, int H, T* __restrict__ out) {
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), c0 = (threadIdx.x & 63) * 4, C = H >> 2;
  if (t >= T_ || c0 >= C) return;
  const T* src = x + (int64_t)inv[t] * H;
  floatx4 q[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) q[p] = load4<T>(src + p * C + c0);
  T* o = out + (int64_t)t * H + 4 * c0;
#pragma unroll
  for (int j = 0; j < 4; j += 2)
    store8<T>(o + 4 * j, floatx4{q[0][j], q[1][j], q[2][j], q[3][j]}, floatx4{q[0][j + 1], q[1][j + 1], q[2][j + 1], q[3][j + 1]});
}
template <typename T> int gather_rows_chw4(hipStream_t st, const T* x, const int* inv, int T_, int H, T* out) {
  if (!chw4_ok(H)) return RL_ERR_ARG;
  if (T_ <= 0) return RL_OK;
  hipLaunchKernelGGL((gather_rows_chw4_kernel<T>), dim3((T_ + 3) / 4), dim3(256), 0, st, x, inv, T_, H, out);
  return RL_LAUNCH_CHECK();
}
template int gather_rows_chw4<bf16_t>(hipStream_t, const bf16_t*, const int*, int, int, bf16_t*);
template int gather_rows_chw4<float>(hipStream_t, const float*, const int*, int, int, float*);

// segment_sum whose input rows are in feature order and whose output rows are in storage order: the scatter into the fp32
// accumulator is the plain one, the cast that follows it anyway stores out[u][p * C + c] = acc[u][c * 4 + p]
template <typename T>
__global__ void segsum_cast_chw4_kernel(const float* __restrict__ acc, T* __restrict__ out, int H, const int* __restrict__ nuniq) {
  const int C = H >> 2, per_row = H >> 4;
  const int64_t n = (int64_t)(*nuniq) * per_row;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = i / per_row;
    const int c0 = (int)(i - u * per_row) * 4;
    const float* a = acc + u * H + 4 * c0;
    const floatx4 v0 = *(const floatx4*)a, v1 = *(const floatx4*)(a + 4), v2 = *(const floatx4*)(a + 8), v3 = *(const floatx4*)(a + 12);
    T* o = out + u * H + c0;
#pragma unroll
    for (int p = 0; p < 4; ++p) store4<T>(o + p * C, floatx4{v0[p], v1[p], v2[p], v3[p]});
  }
}
template <typename T> int segment_sum_chw4(hipStream_t st, const T* x, const int* inv, int T_, int H, float* acc, T* out, const int* nuniq_dev) {
  if (!chw4_ok(H)) return RL_ERR_ARG;
  if (T_ <= 0) return RL_OK;
  (void)hipMemsetAsync(acc, 0, (size_t)T_ * H * sizeof(float), st);
  hipLaunchKernelGGL((segsum_scatter_kernel<T>), dim3((H / 4 + 63) / 64, T_), dim3(64), 0, st, x, inv, T_, H, acc);
  hipLaunchKernelGGL((segsum_cast_chw4_kernel<T>), dim3(1024), dim3(256), 0, st, acc, out, H, nuniq_dev);
  return RL_LAUNCH_CHECK();
}
template int segment_sum_chw4<bf16_t>(hipStream_t, const bf16_t*, const int*, int, int, float*, bf16_t*, const int*);
template int segment_sum_chw4<float>(hipStream_t, const float*, const int*, int, int, float*, float*, const int*);

}  // namespace rl
