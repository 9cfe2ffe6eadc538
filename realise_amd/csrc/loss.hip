// Masked cross-entropy and what surrounds it in the head (K13; the "loss" section of ops.h): the count and the list of the rows that
// enter the loss, the two row kernels (generic, and bf16 with the row in registers) with their ranking instantiations, the ordered
// fold of the per-row terms, the movers of the compacted rows (gather by a device-side list, scatter back with dropout), and the
// evaluation side: arg-max under the same ranking rule, the decode merge and the decode loss.
#include "ops.h"
#include "launch.h"
#include "rows.h"

namespace rl {

// ---- knob (ops.h: set_ce_fast) ----
static int g_ce_fast = 1;                            // bf16 cross-entropy with the row in registers (realise_set_ln key 4)
void set_ce_fast(int on) { g_ce_fast = on; }

// ---------------------------------------------------------------------------------------------
// Masked cross-entropy (models.py:862-869): one 256-thread workgroup per token row.
// ---------------------------------------------------------------------------------------------
// rows that enter the loss: loss_mask == 1 (models.py:864) and label != -100 (CrossEntropyLoss's default ignore_index)
#define RL_CE_IGNORE_INDEX (-100)
__global__ void count_active_kernel(const int64_t* __restrict__ m, const int64_t* __restrict__ labels, int n, float* out) {
  float c = 0.f;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    c += (m[i] == 1 && labels[i] != RL_CE_IGNORE_INDEX) ? 1.f : 0.f;
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c != 0.f) atomicAdd(out, c);
}

// Rows that enter the loss, in order: act_idx[j] = token row of the j-th active row, inv[row] = j (or -1), *n_act and *count = how
// many, row_loss[row] = 0 for the others.  One workgroup of 1024 threads (rows <= 65536), ballot + wave-prefix scan: deterministic.
__global__ void __launch_bounds__(1024) active_rows_kernel(const int64_t* __restrict__ m, const int64_t* __restrict__ labels, int n,
                                                            int* __restrict__ act_idx, int* __restrict__ inv, int* __restrict__ n_act,
                                                            float* __restrict__ count, float* __restrict__ row_loss) {
  __shared__ int wsum[16];
  __shared__ int base_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  for (int r0 = 0; r0 < n; r0 += 1024) {
    const int r = r0 + threadIdx.x;
    const bool a = r < n && m[r] == 1 && labels[r] != RL_CE_IGNORE_INDEX;
    const unsigned long long b = __ballot(a);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (r < n) {
      if (a) { act_idx[off + before] = r; inv[r] = off + before; }
      else { inv[r] = -1; if (row_loss != nullptr) row_loss[r] = 0.f; }
    }
    __syncthreads();
    if (threadIdx.x == 0) { int t = base_s; for (int w = 0; w < 16; ++w) t += wsum[w]; base_s = t; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { *n_act = base_s; *count = (float)base_s; }
}

__device__ __forceinline__ float block_reduce(float v, float* sm, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[wave] = v;
  __syncthreads();
  float r = sm[0];
  for (int w = 1; w < 4; ++w) r = is_max ? fmaxf(r, sm[w]) : r + sm[w];
  return r;
}

// the project's ranking rule (argmax_rows, gemm_nt_decode, the ranking cross-entropy): a NaN beats a number, then the larger value,
// then the lower column (-0.0 == +0.0: the lower column)
__device__ __forceinline__ bool amax_better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}
// The ranking switch of the cross-entropy row kernels (ops.h: CePred).  Off, a kernel takes an empty struct in the place of the request
// and every ranking statement is discarded at compile time: the instantiation is the kernel as it was.  On, each thread looks among the
// elements it already holds for the lowest column equal to the row maximum - one compare and one select per element, in the loop that
// sums the exponentials -, the workgroup reduces to the minimum and thread 0 writes the row's prediction.
struct CeNoPred {};
template <bool RANK> struct CeRankArg { typedef CeNoPred type; };
template <> struct CeRankArg<true> { typedef CePred type; };
// Fast form (every row without a NaN): the row maximum mx is known from the pass's own reduction, so the prediction is the LOWEST
// column whose value equals mx (float equality: -0.0 == +0.0) - one compare and one select per element, then an integer minimum over the
// workgroup (ce_rank_min).  The comparator's other cases, uniform per workgroup and rare: a row whose sum of exponentials is NaN (it
// holds a NaN, or a +inf) is scanned once more for its lowest NaN column, which wins if there is one; a row whose every element is
// -inf matches nothing (the maximum is clamped at -3e38) and gets column 0, the lowest of its equal values.
__device__ __forceinline__ int ce_rank_min(int bi, int* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bi = min(bi, __shfl_xor(bi, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = bi;
  __syncthreads();
  return min(min(si[0], si[1]), min(si[2], si[3]));
}
__device__ __forceinline__ void ce_rank_write(int bi, const CePred& pr, int64_t j, int64_t lab64) {
  if (threadIdx.x == 0) {
    if (j >= 0 && (pr.capacity <= 0 || j < pr.capacity)) {
      if (pr.pred != nullptr) pr.pred[j] = bi;
      if (pr.labels_out != nullptr) pr.labels_out[j] = lab64;
    }
    if (pr.hits != nullptr && (int64_t)bi == lab64) atomicAdd(pr.hits, 1);
  }
}
// where an active row's prediction goes: compacted form - the workgroup's index; a given list - the row's entry; else the row
__device__ __forceinline__ int64_t ce_rank_slot(const CePred& pr, const int* act_idx, int row) {
  if (act_idx != nullptr) return (int64_t)blockIdx.x;
  return pr.inv != nullptr ? (int64_t)pr.inv[row] : (int64_t)row;
}
// a row outside the loss, dense form without a list: its prediction is -1
__device__ __forceinline__ void ce_rank_inactive(const CePred& pr, const int* act_idx, int row) {
  if (threadIdx.x == 0 && act_idx == nullptr && pr.inv == nullptr && pr.pred != nullptr && (pr.capacity <= 0 || row < pr.capacity)) pr.pred[row] = -1;
}

template <typename T, bool RANK = false>
__global__ void __launch_bounds__(256)
ce_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, const int64_t* __restrict__ loss_mask,
          int V, float* loss_out, const float* __restrict__ count, T* __restrict__ dlogits, float* __restrict__ row_loss, int64_t ld_dl,
          const int* __restrict__ act_idx, const int* __restrict__ n_act, int logits_compact, typename CeRankArg<RANK>::type pr) {
  __shared__ float sm[4];
  // compacted form (act_idx != nullptr): workgroup j works on the j-th ACTIVE row and writes gradient row j; the rows outside the loss
  // are not visited at all (their loss terms were zeroed by active_rows_kernel, their gradient rows do not exist)
  if (act_idx != nullptr && (int)blockIdx.x >= *n_act) return;
  const int row = act_idx != nullptr ? act_idx[blockIdx.x] : (int)blockIdx.x;
  const T* x = logits + (int64_t)(logits_compact ? (int)blockIdx.x : row) * ld;
  T* dx = dlogits ? dlogits + (int64_t)(act_idx != nullptr ? (int)blockIdx.x : row) * ld_dl : nullptr;
  // a padded gradient row (ld_dl > V: 128-byte aligned rows for the GEMMs that consume it) keeps exact zeros in its tail
  if (dx != nullptr)
    for (int c = V + threadIdx.x * 4; c < ld_dl; c += 1024) store4<T>(dx + c, floatx4{0.f, 0.f, 0.f, 0.f});
  const int64_t lab64 = labels[row];
  const bool active = loss_mask[row] == 1 && lab64 != RL_CE_IGNORE_INDEX;
  if (!active) {
    if (row_loss != nullptr && threadIdx.x == 0) row_loss[row] = 0.f;
    if (dx != nullptr)
      for (int c = threadIdx.x * 4; c < V; c += 1024) store4<T>(dx + c, floatx4{0.f, 0.f, 0.f, 0.f});
    if constexpr (RANK) ce_rank_inactive(pr, act_idx, row);
    return;
  }
  float mx = -3.0e38f;
  for (int c = threadIdx.x * 4; c < V; c += 1024) {
    const floatx4 v = load4<T>(x + c);
    mx = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  }
  mx = block_reduce(mx, sm, true);
  float s = 0.f;
  int bi = 0x7fffffff;
  for (int c = threadIdx.x * 4; c < V; c += 1024) {
    const floatx4 v = load4<T>(x + c);
    s += exp_t<T>(v[0] - mx) + exp_t<T>(v[1] - mx) + exp_t<T>(v[2] - mx) + exp_t<T>(v[3] - mx);
    if constexpr (RANK) {      // (columns ascend inside a thread: the first match is its lowest)
#pragma unroll
      for (int j = 3; j >= 0; --j) bi = v[j] == mx ? min(bi, c + j) : bi;
    }
  }
  s = block_reduce(s, sm, false);
  if constexpr (RANK) {      // (this kernel is never run in place: the logits are still there for the general walk)
    __shared__ int rk_i[4];
    bi = ce_rank_min(bi, rk_i);
    if (s != s) {
      int bn = 0x7fffffff;
      for (int c = threadIdx.x; c < V; c += 256) {
        const float v = to_f<T>(x[c]);
        bn = v != v ? min(bn, c) : bn;
      }
      bn = ce_rank_min(bn, rk_i);
      bi = bn != 0x7fffffff ? bn : bi;
    }
    bi = bi == 0x7fffffff ? 0 : bi;
    ce_rank_write(bi, pr, ce_rank_slot(pr, act_idx, row), lab64);
  }
  const float inv_n = 1.0f / count[0];
  // a label outside [0, V) is an error PyTorch raises on; here it poisons the loss (NaN) instead of reading out of bounds
  const bool lab_ok = lab64 >= 0 && lab64 < V;
  const int lab = lab_ok ? (int)lab64 : 0;
  const float lse = mx + logf(s);
  if (threadIdx.x == 0) {
    const float l = lab_ok ? (lse - to_f<T>(x[lab])) * inv_n : __builtin_nanf("");
    if (row_loss != nullptr) row_loss[row] = l;          // deterministic path: per-row terms, folded in a fixed order below
    else atomicAdd(loss_out, l);
  }
  if (dx != nullptr) {
    const float inv_s = 1.0f / s;
    for (int c = threadIdx.x * 4; c < V; c += 1024) {
      const floatx4 v = load4<T>(x + c);
      floatx4 d;
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = (exp_t<T>(v[j] - mx) * inv_s - ((c + j) == lab ? 1.0f : 0.0f)) * inv_n;
      store4<T>(dx + c, d);
    }
  }
}
// bf16 fast path of the masked cross-entropy (V % 8 == 0, V <= 256 * 8 * NCH, 16-byte aligned rows): the row - 21128 logits = 42 KB -
// is read ONCE into registers (NCH 16-byte chunks per thread, all loads in flight together) and the maximum, the sum of exponentials
// and the gradient row come from the registers; the generic kernel walks the row three times with 8-byte loads and, with thousands of
// rows in flight, every walk comes from HBM (PMC round 3: 659 MB read per launch for 207 MB of active rows).
// the lowest column of this thread's chunks whose value is a NaN, or INT_MAX - on the packed bf16 bits (a NaN: exponent all ones and a
// mantissa, (h & 0x7fff) > 0x7f80; element 2w of a chunk is the low half of word w).  Descending over the chunks and inside a chunk: a later
// match is a lower column and simply replaces the earlier one.  (The filler chunks beyond the row are -inf: no NaN.)
template <int NCH>
__device__ __forceinline__ int ce_row16_nan_scan(const uint4 (&r)[NCH]) {
  int bi = 0x7fffffff;
#pragma unroll
  for (int i = NCH - 1; i >= 0; --i) {
    const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
    int m = 8;
#pragma unroll
    for (int q = 3; q >= 0; --q) {
      m = ((w[q] >> 16) & 0x7fffu) > 0x7f80u ? 2 * q + 1 : m;
      m = (w[q] & 0x7fffu) > 0x7f80u ? 2 * q : m;
    }
    bi = m < 8 ? 8 * ((int)threadIdx.x + 256 * i) + m : bi;
  }
  return bi;
}
template <int NCH, bool RANK = false>
__global__ void __launch_bounds__(256)
ce_row16_kernel(const bf16_t* logits, int64_t ld, const int64_t* __restrict__ labels, const int64_t* __restrict__ loss_mask,
                int V, float* loss_out, const float* __restrict__ count, bf16_t* dlogits, float* __restrict__ row_loss, int64_t ld_dl,
                const int* __restrict__ act_idx, const int* __restrict__ n_act, int logits_compact, typename CeRankArg<RANK>::type pr) {
  __shared__ float sm[4];
  if (act_idx != nullptr && (int)blockIdx.x >= *n_act) return;
  const int row = act_idx != nullptr ? act_idx[blockIdx.x] : (int)blockIdx.x;
  // logits_compact (round 6, K13): the logits exist for the loss rows only, row j of `logits` = the j-th active row - possibly the SAME
  // buffer as dlogits: the row is read whole into registers before its gradient row is stored over it
  const bf16_t* x = logits + (int64_t)(logits_compact ? (int)blockIdx.x : row) * ld;
  bf16_t* dx = dlogits ? dlogits + (int64_t)(act_idx != nullptr ? (int)blockIdx.x : row) * ld_dl : nullptr;
  if (dx != nullptr)
    for (int c = V + threadIdx.x * 4; c < ld_dl; c += 1024) store4<bf16_t>(dx + c, floatx4{0.f, 0.f, 0.f, 0.f});
  const int64_t lab64 = labels[row];
  const bool active = loss_mask[row] == 1 && lab64 != RL_CE_IGNORE_INDEX;
  const int nch = V >> 3;
  if (!active) {
    if (row_loss != nullptr && threadIdx.x == 0) row_loss[row] = 0.f;
    if (dx != nullptr)
      for (int k = threadIdx.x; k < nch; k += 256) *(uint4*)(dx + 8 * k) = uint4{0u, 0u, 0u, 0u};
    if constexpr (RANK) ce_rank_inactive(pr, act_idx, row);
    return;
  }
  uint4 r[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int k = threadIdx.x + 256 * i;
    r[i] = k < nch ? *(const uint4*)(x + 8 * k) : uint4{0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u};      // -inf pairs: exp() = 0
  }
  // the label's logit is read here, with the row, and pinned behind its wait: in the in-place form (logits == dlogits) other waves
  // store gradient chunks over the row as soon as they are past the two reductions below
  const bool lab_ok0 = lab64 >= 0 && lab64 < V;
  float x_lab = to_f<bf16_t>(x[lab_ok0 ? (int)lab64 : 0]);
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x_lab));
#endif
  float mx = -3.0e38f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    float v[8];
    unpack8(r[i], v);
#pragma unroll
    for (int j = 0; j < 8; ++j) mx = fmaxf(mx, v[j]);
  }
  mx = block_reduce(mx, sm, true);
  float s = 0.f;
  int bi = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    float v[8];
    unpack8(r[i], v);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += exp_t<bf16_t>(v[j] - mx);
    if constexpr (RANK) {      // the chunk's lowest column equal to mx, on the values the sum just used (chunks ascend: the first match stays)
      int m = 8;
#pragma unroll
      for (int j = 7; j >= 0; --j) m = v[j] == mx ? j : m;
      bi = min(bi, m < 8 ? 8 * ((int)threadIdx.x + 256 * i) + m : 0x7fffffff);
    }
  }
  s = block_reduce(s, sm, false);
  if constexpr (RANK) {      // from the registers: the row as read, whatever other waves have stored over it since (in-place form)
    __shared__ int rk_i[4];
    bi = ce_rank_min(bi, rk_i);
    if (s != s) {      // a NaN (or +inf) in the row: the lowest NaN column wins, still from the registers
      const int bn = ce_rank_min(ce_row16_nan_scan<NCH>(r), rk_i);
      bi = bn != 0x7fffffff ? bn : bi;
    }
    bi = bi == 0x7fffffff ? 0 : bi;
    ce_rank_write(bi, pr, ce_rank_slot(pr, act_idx, row), lab64);
  }
  const float inv_n = 1.0f / count[0];
  const bool lab_ok = lab64 >= 0 && lab64 < V;
  const int lab = lab_ok ? (int)lab64 : 0;
  const float lse = mx + logf(s);
  if (threadIdx.x == 0) {
    const float l = lab_ok ? (lse - x_lab) * inv_n : __builtin_nanf("");
    if (row_loss != nullptr) row_loss[row] = l;
    else atomicAdd(loss_out, l);
  }
  if (dx != nullptr) {
    const float inv_s = 1.0f / s;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int k = threadIdx.x + 256 * i;
      if (k < nch) {
        float v[8], d[8];
        unpack8(r[i], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = (exp_t<bf16_t>(v[j] - mx) * inv_s - ((8 * k + j) == lab ? 1.0f : 0.0f)) * inv_n;
        *(uint4*)(dx + 8 * k) = pack8(d);
      }
    }
  }
}
template <typename T>
static bool ce_row16_launch(hipStream_t, const T*, int64_t, const int64_t*, const int64_t*, int, int, float*, float*, T*, float*, int64_t, const int*, const int*, int,
                            const CePred*) { return false; }
template <>
bool ce_row16_launch<bf16_t>(hipStream_t st, const bf16_t* logits, int64_t ld, const int64_t* labels, const int64_t* loss_mask, int rows, int V,
                             float* loss_out, float* count_buf, bf16_t* dlogits, float* row_loss, int64_t ld_dl, const int* act_idx, const int* n_act, int compact,
                             const CePred* pr) {
  constexpr int NCH = 11;          // 256 threads x 11 chunks x 8 = 22528 >= 21128
  if (!g_ce_fast || (V & 7) || (ld & 7) || (ld_dl & 7) || V > 256 * 8 * NCH || ((uintptr_t)logits & 15) || ((uintptr_t)dlogits & 15)) return false;
  if (pr != nullptr)
    hipLaunchKernelGGL((ce_row16_kernel<NCH, true>), dim3(rows), dim3(256), 0, st, logits, ld, labels, loss_mask, V, loss_out, count_buf, dlogits, row_loss,
                       ld_dl, act_idx, n_act, compact, *pr);
  else
    hipLaunchKernelGGL((ce_row16_kernel<NCH>), dim3(rows), dim3(256), 0, st, logits, ld, labels, loss_mask, V, loss_out, count_buf, dlogits, row_loss, ld_dl,
                       act_idx, n_act, compact, CeNoPred());
  return true;
}
// the generic row kernel, ranking or not
template <typename T>
static void ce_generic_launch(hipStream_t st, const T* logits, int64_t ld, const int64_t* labels, const int64_t* loss_mask, int rows, int V, float* loss_out,
                              float* count_buf, T* dlogits, float* row_loss, int64_t ld_dl, const int* act_idx, const int* n_act, int compact, const CePred* pr) {
  if (pr != nullptr)
    hipLaunchKernelGGL((ce_kernel<T, true>), dim3(rows), dim3(256), 0, st, logits, ld, labels, loss_mask, V, loss_out, count_buf, dlogits, row_loss, ld_dl,
                       act_idx, n_act, compact, *pr);
  else
    hipLaunchKernelGGL((ce_kernel<T>), dim3(rows), dim3(256), 0, st, logits, ld, labels, loss_mask, V, loss_out, count_buf, dlogits, row_loss, ld_dl,
                       act_idx, n_act, compact, CeNoPred());
}

// loss = sum of the per-row terms in a fixed order (256 strided partial sums, then a fixed tree): bitwise reproducible
__global__ void __launch_bounds__(256) ce_fold_kernel(const float* __restrict__ row_loss, int rows, float* loss_out) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) s += row_loss[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss_out = red[0];
}
template <typename T>
int ce_loss(hipStream_t st, const T* logits, int64_t ld, const int64_t* labels, const int64_t* loss_mask, int rows, int V,
            float* loss_out, float* count_buf, T* dlogits, float* row_loss, int64_t ld_dl, const CeCompact& cc, const CePred* pr) {
  if (ld_dl <= 0) ld_dl = ld;
  if ((V & 3) || (ld & 3) || (ld_dl & 3) || ld_dl < V) return RL_ERR_ARG;
  if (pr != nullptr && cc.phase != 1) {      // the ranking pass: the hit counter starts at zero, the active-row count is passed on
    if (pr->pred == nullptr) return RL_ERR_ARG;
    if (pr->hits != nullptr && hipMemsetAsync(pr->hits, 0, sizeof(int32_t), st) != hipSuccess) return RL_ERR_LAUNCH;
  }
  if (cc.act_idx != nullptr) {       // compacted gradient rows (needs the per-row loss terms: the ordered fold is the only sum)
    if (row_loss == nullptr || cc.inv == nullptr || cc.n_act == nullptr || rows > 65536) return RL_ERR_ARG;
    // phases: 1 = list the active rows, 2 = loss + gradient rows, 0 = both (cc.logits_compact needs the list before the logits exist:
    // the caller runs phase 1, the classifier over the listed rows, then phase 2)
    if (cc.phase != 2)
      hipLaunchKernelGGL(active_rows_kernel, dim3(1), dim3(1024), 0, st, loss_mask, labels, rows, cc.act_idx, cc.inv, cc.n_act, count_buf, row_loss);
    if (cc.phase == 1) return RL_LAUNCH_CHECK();
    if (pr != nullptr && pr->n_active != nullptr &&
        hipMemcpyAsync(pr->n_active, cc.n_act, sizeof(int32_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return RL_ERR_LAUNCH;
    const bool fast = ce_row16_launch<T>(st, logits, ld, labels, loss_mask, rows, V, loss_out, count_buf, dlogits, row_loss, ld_dl, (const int*)cc.act_idx,
                                         (const int*)cc.n_act, cc.logits_compact, pr);
    if (!fast) {
      if (cc.logits_compact && (const void*)logits == (const void*)dlogits) return RL_ERR_ARG;      // (the generic kernel walks a row three times: not in place)
      ce_generic_launch<T>(st, logits, ld, labels, loss_mask, rows, V, loss_out, count_buf, dlogits, row_loss, ld_dl, (const int*)cc.act_idx,
                           (const int*)cc.n_act, cc.logits_compact, pr);
    }
    hipLaunchKernelGGL(ce_fold_kernel, dim3(1), dim3(256), 0, st, row_loss, rows, loss_out);
    return RL_LAUNCH_CHECK();
  }
  if (pr != nullptr && pr->n_active != nullptr && pr->n_src != nullptr &&
      hipMemcpyAsync(pr->n_active, pr->n_src, sizeof(int32_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return RL_ERR_LAUNCH;
  (void)hipMemsetAsync(loss_out, 0, sizeof(float), st);
  (void)hipMemsetAsync(count_buf, 0, sizeof(float), st);
  hipLaunchKernelGGL(count_active_kernel, dim3(64), dim3(256), 0, st, loss_mask, labels, rows, count_buf);
  if (!ce_row16_launch<T>(st, logits, ld, labels, loss_mask, rows, V, loss_out, count_buf, dlogits, row_loss, ld_dl, nullptr, nullptr, 0, pr))
    ce_generic_launch<T>(st, logits, ld, labels, loss_mask, rows, V, loss_out, count_buf, dlogits, row_loss, ld_dl, nullptr, nullptr, 0, pr);
  if (row_loss != nullptr) hipLaunchKernelGGL(ce_fold_kernel, dim3(1), dim3(256), 0, st, row_loss, rows, loss_out);
  return RL_LAUNCH_CHECK();
}
template int ce_loss<bf16_t>(hipStream_t, const bf16_t*, int64_t, const int64_t*, const int64_t*, int, int, float*, float*, bf16_t*, float*, int64_t, const CeCompact&,
                             const CePred*);
template int ce_loss<float>(hipStream_t, const float*, int64_t, const int64_t*, const int64_t*, int, int, float*, float*, float*, float*, int64_t, const CeCompact&,
                            const CePred*);

// out[j] = in[idx[j]] for j < *n (rows of H elements, 16 bytes per lane)
template <typename T>
__global__ void gather_rows_kernel(const T* __restrict__ in, const int* __restrict__ idx, const int* __restrict__ n, int H, T* __restrict__ out) {
  const int j = blockIdx.x;
  if (j >= *n) return;
  const uint4* src = (const uint4*)(in + (int64_t)idx[j] * H);
  uint4* dst = (uint4*)(out + (int64_t)j * H);
  for (int c = threadIdx.x; c < H * (int)sizeof(T) / 16; c += blockDim.x) dst[c] = src[c];
}
template <typename T> int gather_listed_rows(hipStream_t st, const T* in, const int* idx, const int* n_dev, int max_rows, int H, T* out) {
  if ((H * (int)sizeof(T)) & 15) return RL_ERR_ARG;
  hipLaunchKernelGGL((gather_rows_kernel<T>), dim3(max_rows), dim3(96), 0, st, in, idx, n_dev, H, out);
  return RL_LAUNCH_CHECK();
}
template int gather_listed_rows<bf16_t>(hipStream_t, const bf16_t*, const int*, const int*, int, int, bf16_t*);
template int gather_listed_rows<float>(hipStream_t, const float*, const int*, const int*, int, int, float*);
// out[row] = inv[row] >= 0 ? in[inv[row]] * dropout(row, c) : 0   (the inverse of the gather, fused with the dropout map of the site)
template <typename T>
__global__ void scatter_rows_drop_kernel(const T* __restrict__ in, const int* __restrict__ inv, int H, T* __restrict__ out, DropParams d,
                                         const float* __restrict__ scale_dev) {
  const int row = blockIdx.x, j = inv[row];
  const float sc = scale_dev != nullptr ? *scale_dev : 1.0f;
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4) {
    floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
    if (j >= 0) v = load4<T>(in + (int64_t)j * H + c) * drop_mult4(d.seed, d.thresh, d.scale, (uint32_t)row * (uint32_t)H + (uint32_t)c) * sc;
    store4<T>(out + (int64_t)row * H + c, v);
  }
}
template <typename T> int scatter_rows_drop(hipStream_t st, const T* in, const int* inv, int rows, int H, T* out, DropParams d, const float* scale_dev) {
  if (H & 3) return RL_ERR_ARG;
  hipLaunchKernelGGL((scatter_rows_drop_kernel<T>), dim3(rows), dim3(192), 0, st, in, inv, H, out, d, scale_dev);
  return RL_LAUNCH_CHECK();
}
// the same scatter fed by the fp32 partial planes of a split-K GEMM: out[row] = inv[row] >= 0 ? (sum_s slab[s][inv[row]]) * dropout : 0,
// planes added in index order (bit-reproducible)
template <typename T>
__global__ void scatter_rows_drop_slab_kernel(const float* __restrict__ slab, int nsplit, int64_t stride, const int* __restrict__ inv, int H,
                                              T* __restrict__ out, DropParams d, const float* __restrict__ scale_dev) {
  const int row = blockIdx.x, j = inv[row];
  const float sc = scale_dev != nullptr ? *scale_dev : 1.0f;
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4) {
    floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
    if (j >= 0) {
      const float* p = slab + (int64_t)j * H + c;
      v = *(const floatx4*)p;
      for (int s = 1; s < nsplit; ++s) v += *(const floatx4*)(p + s * stride);
      v *= drop_mult4(d.seed, d.thresh, d.scale, (uint32_t)row * (uint32_t)H + (uint32_t)c) * sc;
    }
    store4<T>(out + (int64_t)row * H + c, v);
  }
}
template <typename T> int scatter_rows_drop_slab(hipStream_t st, const float* slab, int nsplit, int64_t stride, const int* inv, int rows, int H, T* out,
                                                 DropParams d, const float* scale_dev) {
  if ((H & 3) || nsplit < 1) return RL_ERR_ARG;
  hipLaunchKernelGGL((scatter_rows_drop_slab_kernel<T>), dim3(rows), dim3(192), 0, st, slab, nsplit, stride, inv, H, out, d, scale_dev);
  return RL_LAUNCH_CHECK();
}
template int scatter_rows_drop_slab<bf16_t>(hipStream_t, const float*, int, int64_t, const int*, int, int, bf16_t*, DropParams, const float*);
template int scatter_rows_drop_slab<float>(hipStream_t, const float*, int, int64_t, const int*, int, int, float*, DropParams, const float*);
template int scatter_rows_drop<bf16_t>(hipStream_t, const bf16_t*, const int*, int, int, bf16_t*, DropParams, const float*);
template int scatter_rows_drop<float>(hipStream_t, const float*, const int*, int, int, float*, DropParams, const float*);

// x *= *scale_dev (n % 4 == 0): the dense-classifier fallback of the incoming loss gradient (engine.hip stage_head)
template <typename T>
__global__ void __launch_bounds__(256) scale_dev_kernel(T* __restrict__ x, int64_t n4, const float* __restrict__ scale_dev) {
  const float sc = *scale_dev;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) store4<T>(x + 4 * i, load4<T>(x + 4 * i) * sc);
}
template <typename T> int scale_by_dev(hipStream_t st, T* x, int64_t n, const float* scale_dev) {
  if ((n & 3) || scale_dev == nullptr) return RL_ERR_ARG;
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL((scale_dev_kernel<T>), dim3((int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048)), dim3(256), 0, st, x, n4, scale_dev);
  return RL_LAUNCH_CHECK();
}
template int scale_by_dev<bf16_t>(hipStream_t, bf16_t*, int64_t, const float*);
template int scale_by_dev<float>(hipStream_t, float*, int64_t, const float*);

// ---------------------------------------------------------------------------------------------
// Row-wise argmax: one 256-thread workgroup per row, 16-byte loads, (value, index) pairs reduced with the
// first-occurrence tie rule.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) argmax_kernel(const T* __restrict__ logits, int64_t ld, int V, int64_t* __restrict__ ids) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const T* row = logits + (int64_t)blockIdx.x * ld;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  const int v8 = ((ld & 7) == 0) ? (V & ~7) : 0;          // 8-wide body when every row start is 16-byte aligned
  for (int c = threadIdx.x * 8; c < v8; c += 256 * 8) {
    floatx4 a, b;
    load8<T>(row + c, a, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) if (amax_better(a[j], c + j, bv, bi)) { bv = a[j]; bi = c + j; }
#pragma unroll
    for (int j = 0; j < 4; ++j) if (amax_better(b[j], c + 4 + j, bv, bi)) { bv = b[j]; bi = c + 4 + j; }
  }
  for (int c = v8 + threadIdx.x; c < V; c += 256) {
    const float v = to_f<T>(row[c]);
    if (amax_better(v, c, bv, bi)) { bv = v; bi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (amax_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) if (amax_better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
    ids[blockIdx.x] = bi;
  }
}
template <typename T> int argmax_rows(hipStream_t st, const T* logits, int64_t ld, int rows, int V, int64_t* ids) {
  if (rows <= 0) return RL_OK;
  if (V <= 0 || ld < V) return RL_ERR_ARG;
  hipLaunchKernelGGL((argmax_kernel<T>), dim3(rows), dim3(256), 0, st, logits, ld, V, ids);
  return RL_LAUNCH_CHECK();
}
template int argmax_rows<bf16_t>(hipStream_t, const bf16_t*, int64_t, int, int, int64_t*);
template int argmax_rows<float>(hipStream_t, const float*, int64_t, int, int, int64_t*);

// ---- decode GEMM: merge of the per-slab records (what np.argmax(preds, -1) of src/run.py:262-263 / src/test.py:143 read the [B, S, V]
// logits for).  One lane per row; records are [plane][slab][row] 16-byte words, so a wave reads 1 KiB lines.  Slabs are folded in
// ascending column order with the comparator of the epilogue (DecCand, gemm_dev.h): a function of the records alone.
template <int KC>
__global__ void __launch_bounds__(64) decode_merge_kernel(const uint4* __restrict__ rec, int nslab, int M, int k, int64_t* __restrict__ ids,
                                                          float* __restrict__ values, float* __restrict__ probs, float* __restrict__ lse) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= M) return;
  uint32_t key[KC]; int col[KC];
#pragma unroll
  for (int j = 0; j < KC; ++j) { key[j] = 0u; col[j] = 0x7FFFFFFF; }
  float m = -__builtin_huge_valf(), s = 0.f;
  auto beats = [](uint32_t ka, int ca, uint32_t kb, int cb) { return ka > kb || (ka == kb && ca < cb); };
  auto keyof = [](float x) {
    const float y = x + 0.0f;
    const uint32_t u = __float_as_uint(y);
    return (y != y) ? 0xFFFFFFFFu : (u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u));
  };
  for (int sl = 0; sl < nslab; ++sl) {
    uint32_t v[KC]; int c[KC]; float m2, s2;
    if constexpr (KC == 1) {
      const uint4 r = rec[(int64_t)sl * M + row];
      v[0] = r.x; c[0] = (int)r.y; m2 = __uint_as_float(r.z); s2 = __uint_as_float(r.w);
    } else {
      const uint4 r0 = rec[(int64_t)sl * M + row], r1 = rec[((int64_t)nslab + sl) * M + row], r2 = rec[((int64_t)2 * nslab + sl) * M + row];
      v[0] = r0.x; v[1] = r0.y; v[2] = r0.z; v[3] = r0.w;
      c[0] = (int)r1.x; c[1] = (int)r1.y; c[2] = (int)r1.z; c[3] = (int)r1.w;
      m2 = __uint_as_float(r2.x); s2 = __uint_as_float(r2.y);
    }
    if (c[0] == 0x7FFFFFFF) continue;                  // a slab that lies beyond N as a whole
#pragma unroll
    for (int e = 0; e < KC; ++e) {
      const int ce = c[e];
      const uint32_t ke = ce == 0x7FFFFFFF ? 0u : keyof(__uint_as_float(v[e]));
      bool b[KC];
#pragma unroll
      for (int j = 0; j < KC; ++j) b[j] = beats(ke, ce, key[j], col[j]);
#pragma unroll
      for (int j = KC - 1; j >= 0; --j) {
        const int jm = j > 0 ? j - 1 : 0;
        const bool up = j > 0 && b[jm];
        key[j] = b[j] ? (up ? key[jm] : ke) : key[j];
        col[j] = b[j] ? (up ? col[jm] : ce) : col[j];
      }
    }
    const float mm = fmaxf(m, m2);
    s = s * (m == mm ? 1.0f : expf(m - mm)) + s2 * (m2 == mm ? 1.0f : expf(m2 - mm));
    m = mm;
  }
  const float l = m + logf(s);
  lse[row] = l;
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    if (j < k) {
      const uint32_t kj = key[j];
      const float val = __uint_as_float(kj == 0xFFFFFFFFu ? 0x7FC00000u : ((kj & 0x80000000u) ? (kj ^ 0x80000000u) : ~kj));
      ids[(int64_t)row * k + j] = col[j];
      values[(int64_t)row * k + j] = val;
      probs[(int64_t)row * k + j] = expf(val - l);
    }
  }
}
int decode_merge(hipStream_t st, const float* rec, int kc, int nslab, int M, int k, int64_t* ids, float* values, float* probs, float* lse) {
  if (!rec || !ids || !values || !probs || !lse || M < 1 || nslab < 1 || k < 1 || k > kc || (kc != 1 && kc != 4)) return RL_ERR_ARG;
  const dim3 grid((M + 63) / 64);
  if (kc == 1) hipLaunchKernelGGL((decode_merge_kernel<1>), grid, dim3(64), 0, st, (const uint4*)rec, nslab, M, k, ids, values, probs, lse);
  else hipLaunchKernelGGL((decode_merge_kernel<4>), grid, dim3(64), 0, st, (const uint4*)rec, nslab, M, k, ids, values, probs, lse);
  return RL_LAUNCH_CHECK();
}

// the loss of models.py:862-869 from the decode outputs: mean over the active rows of lse - logit[label]
__global__ void __launch_bounds__(256) decode_loss_kernel(const float* __restrict__ lse, const float* __restrict__ label_logit,
                                                          const int64_t* __restrict__ labels, const int64_t* __restrict__ loss_mask, int rows,
                                                          float* __restrict__ loss_out) {
  __shared__ float sm[8];
  float a = 0.f, n = 0.f;
  for (int i = threadIdx.x; i < rows; i += 256) {
    if (loss_mask[i] == 1 && labels[i] != -100) { a += lse[i] - label_logit[i]; n += 1.f; }
  }
  a = wave_sum(a); n = wave_sum(n);
  if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = a; sm[4 + (threadIdx.x >> 6)] = n; }
  __syncthreads();
  if (threadIdx.x == 0) *loss_out = (sm[0] + sm[1] + sm[2] + sm[3]) / (sm[4] + sm[5] + sm[6] + sm[7]);
}
int decode_loss(hipStream_t st, const float* lse, const float* label_logit, const int64_t* labels, const int64_t* loss_mask, int rows, float* loss_out) {
  if (!lse || !label_logit || !labels || !loss_mask || !loss_out || rows < 1) return RL_ERR_ARG;
  hipLaunchKernelGGL(decode_loss_kernel, dim3(1), dim3(256), 0, st, lse, label_logit, labels, loss_mask, rows, loss_out);
  return RL_LAUNCH_CHECK();
}

}  // namespace rl
