// Per-token bookkeeping and the embedding-side row kernels (the "tokens" section of ops.h): the additive attention mask, the live-row
// bytes and block lists of a padded batch (row_liveness), the embedding backward, the token tables of evaluation (token_copy /
// token_scatter) and the stand-alone dropout map.
#include "ops.h"
#include "launch.h"
#include "rows.h"

namespace rl {

__global__ void mask_to_additive_kernel(const int64_t* __restrict__ m, float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (1.0f - (float)m[i]) * -10000.0f;       // modeling_bert.py:696-697
}
int mask_to_additive(hipStream_t st, const int64_t* masks, float* out, int n) {
  hipLaunchKernelGGL(mask_to_additive_kernel, dim3((n + 255) / 256), dim3(256), 0, st, masks, out, n);
  return RL_LAUNCH_CHECK();
}

// row_liveness (ops.h): one workgroup.  Phase 1: last flagged position of every sentence; phase 2: row bytes; phase 3: the 64-,
// 32- and 16-row block lists by ballot + prefix scan (ascending, deterministic).
__global__ void __launch_bounds__(1024) row_liveness_kernel(const int64_t* __restrict__ masks, const int64_t* __restrict__ loss_masks, int B, int S,
                                                             uint8_t* __restrict__ row_live, int* __restrict__ tiles64, int* __restrict__ tiles32,
                                                             int* __restrict__ tiles16, int* __restrict__ n_tiles, int* __restrict__ rlen, int* __restrict__ rows) {
  __shared__ int wsum[16];
  __shared__ int base_s;
  const int T = B * S, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // phases 1 + 2: a wave per sentence finds 1 + the last flagged position, then writes the sentence's row bytes
  for (int b = wave; b < B; b += 16) {
    int last = 0;
    for (int s0 = 0; s0 < S; s0 += 64) {
      const int s = s0 + lane;
      const bool f = s < S && (masks[(int64_t)b * S + s] == 1 || (loss_masks != nullptr && loss_masks[(int64_t)b * S + s] == 1));
      const unsigned long long bal = __ballot(f);
      if (bal != 0ull) last = s0 + 64 - __clzll(bal);
    }
    for (int s = lane; s < S; s += 64) row_live[(int64_t)b * S + s] = s < last ? 1 : 0;
    if (lane == 0 && rlen != nullptr) rlen[b] = last;
  }
  __syncthreads();
  // phase 3: block lists
  for (int pass = 0; pass < 4; ++pass) {          // (pass 3: the live ROWS themselves, n_tiles[3] of them - the row-granular GEMM list)
    const int bp = pass == 3 ? 1 : 64 >> pass;
    int* out = pass == 0 ? tiles64 : (pass == 1 ? tiles32 : (pass == 2 ? tiles16 : rows));
    if (out == nullptr) continue;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    const int nblk = T / bp;
    for (int k0 = 0; k0 < nblk; k0 += 1024) {
      const int k = k0 + threadIdx.x;
      bool live = false;
      if (k < nblk && bp == 1) live = row_live[k] != 0;
      else if (k < nblk)
        for (int r = 0; r < bp; r += 16) {                       // 16 row bytes at a time
          const uint4 v = *(const uint4*)(row_live + (int64_t)k * bp + r);
          live = live || (v.x | v.y | v.z | v.w) != 0u;
        }
      const unsigned long long bal = __ballot(live);
      const int before = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wsum[wave] = __popcll(bal);
      __syncthreads();
      int off = base_s;
      for (int w = 0; w < wave; ++w) off += wsum[w];
      if (live) out[off + before] = k;
      __syncthreads();
      if (threadIdx.x == 0) { int t = base_s; for (int w = 0; w < 16; ++w) t += wsum[w]; base_s = t; }
      __syncthreads();
    }
    if (threadIdx.x == 0) n_tiles[pass] = base_s;
    __syncthreads();
  }
}
int row_liveness(hipStream_t st, const int64_t* masks, const int64_t* loss_masks, int B, int S, uint8_t* row_live, int* tiles64, int* tiles32,
                 int* tiles16, int* n_tiles, int* rlen, int* rows) {
  if (B < 1 || S < 1 || ((int64_t)B * S) % 64 != 0 || masks == nullptr) return RL_ERR_ARG;
  hipLaunchKernelGGL(row_liveness_kernel, dim3(1), dim3(1024), 0, st, masks, loss_masks, B, S, row_live, tiles64, tiles32, tiles16, n_tiles, rlen, rows);
  return RL_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// Embedding backward: thread owns 4 columns of one sequence position s and walks the batch.
// ---------------------------------------------------------------------------------------------
// Padded positions receive an exactly-zero gradient (masked as attention keys, excluded from the loss and from the
// masked mean), and they all carry token id 0: skipping all-zero quads is exact and removes the thousands-way
// same-address atomic pile-up on that one embedding row.
template <typename T>
__global__ void embed_bwd_kernel(const T* __restrict__ de, const int64_t* __restrict__ ids, int B, int S, int H,
                                 float* word_grad, float* pos_grad, int pos_zero, float* type_grad) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int s = blockIdx.y;
  if (c >= H) return;
  const int bchunk = (B + gridDim.z - 1) / gridDim.z;
  const int b0 = blockIdx.z * bchunk, b1 = min(B, b0 + bchunk);
  floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int b = b0; b < b1; ++b) {
    const int64_t row = (int64_t)b * S + s;
    const floatx4 d = load4<T>(de + row * H + c);
    if (quad_is_zero(d)) continue;
    acc += d;
    if (word_grad != nullptr) {
      float* w = word_grad + ids[row] * H + c;
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(w + j, d[j]);
    }
  }
  if (quad_is_zero(acc)) return;
  // The token-type row (every token adds to it) and, with position_ids == 0, the single position row are plain column sums of de:
  // they come from a column reduction (embed_bwd below) - as per-block atomics they were a 1024-way pile-up on 768 addresses
  // (~80 of this kernel's 117 us).
  if (pos_zero) return;
  float* p = pos_grad + (int64_t)s * H + c;
#pragma unroll
  for (int j = 0; j < 4; ++j) atomicAdd(p + j, acc[j]);
}
template <typename T>
int embed_bwd(hipStream_t st, const T* de, const int64_t* ids, int B, int S, int H, float* word_grad, float* pos_grad,
              int pos_zero, float* type_grad) {
  if (H & 3) return RL_ERR_ARG;
  const int tx = 64;
  const int bz = B >= 32 ? 8 : (B >= 8 ? 4 : 1);
  if (word_grad != nullptr || !pos_zero)
    hipLaunchKernelGGL((embed_bwd_kernel<T>), dim3((H / 4 + tx - 1) / tx, S, bz), dim3(tx), 0, st, de, ids, B, S, H, word_grad,
                       pos_grad, pos_zero, type_grad);
  int rc = bias_grad<T>(st, de, H, B * S, H, type_grad, nullptr);
  if (rc == RL_OK && pos_zero) rc = bias_grad<T>(st, de, H, B * S, H, pos_grad, nullptr);
  return rc != RL_OK ? rc : RL_LAUNCH_CHECK();
}
template int embed_bwd<bf16_t>(hipStream_t, const bf16_t*, const int64_t*, int, int, int, float*, float*, int, float*);
template int embed_bwd<float>(hipStream_t, const float*, const int64_t*, int, int, int, float*, float*, int, float*);

// ---------------------------------------------------------------------------------------------
// Token tables: rows by token id, 16 bytes per lane and access, one wave per row and four rows per workgroup as ln_fwd_kernel
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) token_copy_kernel(const T* __restrict__ table, int64_t ld, const int64_t* __restrict__ ids, int rows, int H,
                                                         T* __restrict__ out, int64_t ldo) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;
  constexpr int E = 16 / (int)sizeof(T);                 // elements per 16-byte chunk
  const T* src = table + ids[row] * ld;
  T* dst = out + (int64_t)row * ldo;
  for (int c = lane * E; c < H; c += 64 * E) *(uint4*)(dst + c) = *(const uint4*)(src + c);
}
template <typename T> int token_copy(hipStream_t st, const T* table, int64_t ld, const int64_t* ids, int rows, int H, T* out, int64_t ldo) {
  if (!table || !ids || !out || H < 8 || (H & 7) || (ld & 7) || (ldo & 7) || ld < H || ldo < H) return RL_ERR_ARG;
  if (rows <= 0) return RL_OK;
  hipLaunchKernelGGL((token_copy_kernel<T>), dim3((rows + 3) / 4), dim3(256), 0, st, table, ld, ids, rows, H, out, ldo);
  return RL_LAUNCH_CHECK();
}
template int token_copy<bf16_t>(hipStream_t, const bf16_t*, int64_t, const int64_t*, int, int, bf16_t*, int64_t);
template int token_copy<float>(hipStream_t, const float*, int64_t, const int64_t*, int, int, float*, int64_t);

// blockIdx.y: 0 = the pinyin pair, 1 = the glyph pair (a missing pair returns at once)
template <typename T>
__global__ void __launch_bounds__(256) token_scatter_kernel(const int64_t* __restrict__ ids, int rows, int H, const T* __restrict__ rows0,
                                                            T* __restrict__ table0, const T* __restrict__ rows1, T* __restrict__ table1, int64_t ld) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  const T* src = blockIdx.y ? rows1 : rows0;
  T* table = blockIdx.y ? table1 : table0;
  if (row >= rows || src == nullptr || table == nullptr) return;
  constexpr int E = 16 / (int)sizeof(T);
  src += (int64_t)row * H;
  T* dst = table + ids[row] * ld;
  for (int c = lane * E; c < H; c += 64 * E) *(uint4*)(dst + c) = *(const uint4*)(src + c);
}
template <typename T> int token_scatter(hipStream_t st, const int64_t* ids, int rows, int H, const T* pho_rows, T* pho_table,
                                        const T* res_rows, T* res_table, int64_t ld) {
  const bool pho = pho_rows && pho_table, res = res_rows && res_table;
  if (!ids || (!pho && !res) || H < 8 || (H & 7) || (ld & 7) || ld < H) return RL_ERR_ARG;
  if (rows <= 0) return RL_OK;
  hipLaunchKernelGGL((token_scatter_kernel<T>), dim3((rows + 3) / 4, 2), dim3(256), 0, st, ids, rows, H, pho ? pho_rows : nullptr,
                     pho ? pho_table : nullptr, res ? res_rows : nullptr, res ? res_table : nullptr, ld);
  return RL_LAUNCH_CHECK();
}
template int token_scatter<bf16_t>(hipStream_t, const int64_t*, int, int, const bf16_t*, bf16_t*, const bf16_t*, bf16_t*, int64_t);
template int token_scatter<float>(hipStream_t, const int64_t*, int, int, const float*, float*, const float*, float*, int64_t);

// ---------------------------------------------------------------------------------------------
// Dropout as a stand-alone map (the one before the classifier, models.py:858)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n, DropParams d) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  floatx4 v = load4<T>(x + i);
  v *= drop_mult4(d.seed, d.thresh, d.scale, (uint32_t)i);
  store4<T>(y + i, v);
}
template <typename T> int dropout_apply(hipStream_t st, const T* x, T* y, int rows, int H, DropParams d) {
  const int64_t n = (int64_t)rows * H;
  if (n & 3) return RL_ERR_ARG;
  hipLaunchKernelGGL((dropout_kernel<T>), dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, x, y, n, d);
  return RL_LAUNCH_CHECK();
}
template int dropout_apply<bf16_t>(hipStream_t, const bf16_t*, bf16_t*, int, int, DropParams);
template int dropout_apply<float>(hipStream_t, const float*, float*, int, int, DropParams);

}  // namespace rl
