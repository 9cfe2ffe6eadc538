// BatchNorm2d over NHWC activations [P][C] (K9, char_cnn.py:17-32; the "BatchNorm" section of ops.h) and the column reductions under
// it: the host plan of every launch (bn_plan and its parts), col_reduce / col_fold and what reduces through them (bias_grad, col_sum,
// col_sumsq_centered, the backward sums), the 16-byte and one-pass training statistics, the paired reduce of bn2 + shortcut BN, the
// two launch sequences bn_stats / bn_backward, then finalize, apply, backward apply and relu_bwd.  col_fold_kernel lives here with the
// reductions that launch it; other families reach it through the launchers of ops.h (bias_grad, col_sum).
#include "ops.h"
#include "launch.h"

namespace rl {

// ---- knobs (ops.h: set_bn_fast / set_bn_chunks) ----
static int g_bn_fast = 1, g_bn_chunks = 1024;       // bf16 16-byte BatchNorm / column-reduction kernels; row chunks (= workgroups) of the reductions
static int g_bn_onepass = 1;                        // bf16 training statistics in one pass about the running mean (bn_stats_train16)
void set_bn_fast(int on) { g_bn_fast = on & 1; g_bn_onepass = (on & 1) && !(on & 2); }
void set_bn_chunks(int n) { if (n >= 1 && n <= 4096) g_bn_chunks = n; }

// ---- the host plan of the BatchNorm launches (ops.h; realise_debug_bn_plan): every kernel choice below is made here and nowhere else ----
// the 16-byte kernels apply: bf16, C a power of two in [8, 2048], hw a power of two
static inline bool bn_fast_shape(int elem_bytes, int C, int hw) {
  const int cs = pow2_shift(C);
  return elem_bytes == 2 && g_bn_fast && cs >= 3 && cs <= 11 && pow2_shift(hw) >= 0;
}
// row chunks of a 16-byte reduction: the knob, at least four row passes per workgroup, the records inside the scratch
static inline int reduce16_chunks(int rows, int C, int stride) {
  const int rpp = 2048 / C;
  int g = g_bn_chunks;
  const int max_g = (rows + 4 * rpp - 1) / (4 * rpp);
  if (g > max_g) g = max_g;
  if ((int64_t)g * stride > COL_SLOT_FLOATS) g = COL_SLOT_FLOATS / stride;
  return g < 1 ? 1 : g;
}
BnPass col_reduce_plan(int elem_bytes, int rows, int C, int hw, bool slots_given, int nout, bool fast) {
  BnPass p;
  if (fast && slots_given && bn_fast_shape(elem_bytes, C, hw)) {       // (the 16-byte kernels write records only: they need the scratch)
    p.kernel = BN_16B; p.stride = nout * C; p.g = reduce16_chunks(rows, C, p.stride); p.fold_wgs = (p.stride + 31) / 32; p.overwrite = 1;
    return p;
  }
  p.tpr_shift = 5;
  while (p.tpr_shift > 2 && (1 << p.tpr_shift) * 4 > C) --p.tpr_shift;      // 32 threads x 4 columns unless the row is narrower
  const int tpr = 1 << p.tpr_shift;
  p.gx = (C + tpr * 4 - 1) / (tpr * 4);
  int gy = 1024 / p.gx;
  if (gy < 1) gy = 1;
  const int rpp = 256 / tpr;
  const int max_gy = (rows + 4 * rpp - 1) / (4 * rpp);                      // at least 4 passes per workgroup
  if (gy > max_gy) gy = max_gy;
  if (gy < 1) gy = 1;
  if (slots_given) {           // per-chunk partial records [C | C] + ordered fold: bitwise reproducible (gy * 2C <= COL_SLOT_FLOATS)
    p.stride = 2 * C;
    if ((int64_t)gy * p.stride > COL_SLOT_FLOATS) gy = COL_SLOT_FLOATS / p.stride;      // (0: refused)
    p.fold_wgs = ((nout > 1 ? 2 * C : C) + 31) / 32;
    p.overwrite = 1;
  }
  p.g = gy;
  return p;
}
BnPass bn_stats_plan(int elem_bytes, int P, int C, int hw, bool slots_given) {
  if (slots_given && g_bn_onepass && P > 0 && bn_fast_shape(elem_bytes, C, hw)) {
    BnPass p;
    p.kernel = BN_ONEPASS; p.stride = 2 * C; p.g = reduce16_chunks(P, C, p.stride); p.fold_wgs = (C + 31) / 32; p.overwrite = 1;
    return p;
  }
  return col_reduce_plan(elem_bytes, P, C, hw, slots_given, 1, true);
}
BnPass bn_map_plan(int elem_bytes, int P, int C, int hw) {
  BnPass p;
  p.overwrite = 1;
  if (bn_fast_shape(elem_bytes, C, hw) && (((int64_t)P * C) & 7) == 0) p.kernel = BN_16B;
  return p;
}
bool bn_pair_ok(int elem_bytes, int P, int C, int hw, bool slots_given) {
  return col_reduce_plan(elem_bytes, P, C, hw, slots_given, 4, true).kernel == BN_16B && bn_map_plan(elem_bytes, P, C, hw).kernel == BN_16B &&
         4 * C <= BN_PAIR_SUMS;
}
int bn_plan(int elem_bytes, int P, int C, int hw, bool slots_given, int branches, BnPlan& pl) {
  pl = BnPlan();
  if ((elem_bytes != 2 && elem_bytes != 4) || P < 1 || C < 4 || (C & 3) || hw < 1 || branches < 1 || branches > 2) return RL_ERR_ARG;
  pl.stats = bn_stats_plan(elem_bytes, P, C, hw, slots_given);
  pl.apply = bn_map_plan(elem_bytes, P, C, hw);
  const bool pair = branches == 2 && bn_pair_ok(elem_bytes, P, C, hw, slots_given);
  pl.bwd_reduce = col_reduce_plan(elem_bytes, P, C, hw, slots_given, pair ? 4 : 2, true);
  pl.bwd_apply = bn_map_plan(elem_bytes, P, C, hw);
  if (pair) pl.bwd_reduce.kernel = pl.bwd_apply.kernel = BN_PAIRED;
  return (pl.stats.g < 1 || pl.bwd_reduce.g < 1) ? RL_ERR_ARG : RL_OK;
}

// ---------------------------------------------------------------------------------------------
// Column reductions over a row-major [rows][C] matrix: 32 threads x 4 columns wide, 8 row lanes.
// ---------------------------------------------------------------------------------------------
template <typename F>
__global__ void __launch_bounds__(256) col_reduce_kernel(F f, int rows_max, int C, int tpr_shift, float* out0, float* out1, RowBound rb,
                                                          float* slots, int slot_stride) {
  // tpr = threads per row (each owns 4 consecutive columns); 256 / tpr rows are read per pass, so a wave always touches
  // whole contiguous rows (C = 64: 16 threads x 4 cols = one 128-byte bf16 row, 4 rows per wave-instruction).
  __shared__ floatx4 red[2][256];
  const int tpr = 1 << tpr_shift, rpp = 256 >> tpr_shift;
  const int cx = threadIdx.x & (tpr - 1), ry = threadIdx.x >> tpr_shift;
  const int col = (blockIdx.x * tpr + cx) * 4;
  const int rows = rb_rows(rb, rows_max);
  const int chunk = (rows + gridDim.y - 1) / gridDim.y;          // live rows are re-split evenly over the grid
  const int r0 = blockIdx.y * chunk;
  const int r1 = min(rows, r0 + chunk);
  floatx4 a0 = floatx4{0.f, 0.f, 0.f, 0.f}, a1 = floatx4{0.f, 0.f, 0.f, 0.f};
  if (col < C) {
    // four independent accumulator pairs: the loads of four row passes are in flight together (one pass at a time left a
    // 64-column reduction over 957k rows at 1.2 TB/s: a thread's 8-byte load, then its dependent add, then the next load)
    floatx4 b0 = a0, b1 = a0, c0 = a0, c1 = a0, d0 = a0, d1 = a0;
    int r = r0 + ry;
    for (; r + 3 * rpp < r1; r += 4 * rpp) {
      f(r, col, a0, a1);
      f(r + rpp, col, b0, b1);
      f(r + 2 * rpp, col, c0, c1);
      f(r + 3 * rpp, col, d0, d1);
    }
    for (; r < r1; r += rpp) f(r, col, a0, a1);
    a0 = (a0 + b0) + (c0 + d0);
    a1 = (a1 + b1) + (c1 + d1);
  }
  red[0][threadIdx.x] = a0;
  red[1][threadIdx.x] = a1;
  __syncthreads();
  if (ry == 0 && col < C) {
    for (int k = 1; k < rpp; ++k) { a0 += red[0][k * tpr + cx]; a1 += red[1][k * tpr + cx]; }
    if (slot_stride) {     // deterministic path: this row chunk's partial sums go to their own [C | C] record
      float* rec = slots + (int64_t)blockIdx.y * slot_stride;      // col_fold_kernel adds the records up in a fixed order
      *(floatx4*)(rec + col) = a0;
      if (out1 != nullptr) *(floatx4*)(rec + C + col) = a1;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        atomicAdd(out0 + col + j, a0[j]);
        if (out1 != nullptr) atomicAdd(out1 + col + j, a1[j]);
      }
    }
  }
}
// out[i] (+)= sum over the nrec partial records, in a fixed order: 32 record lanes per column quad (each adds records
// k, k + 32, ... in order), then a fixed pairwise tree over the 32 lane sums.  One workgroup per 32 columns.
// overwrite: out = sum (no zero-fill needed before the reduction); clean: the records are left zeroed (accumulator records that the
// next launch adds into with atomics need no memset).
__global__ void __launch_bounds__(256) col_fold_kernel(float* __restrict__ slots, int slot_stride, int nrec, int n, float* out0,
                                                        float* out1, int C, int overwrite, int clean, float alpha) {
  __shared__ floatx4 red[32][8];
  const int cq = threadIdx.x & 7, kl = threadIdx.x >> 3;
  const int i = (blockIdx.x * 8 + cq) * 4;                 // i in [0, n): n = C or 2C laid out [C | C], C % 4 == 0
  floatx4 s = floatx4{0.f, 0.f, 0.f, 0.f};
  if (i < n)
    for (int k = kl; k < nrec; k += 32) {
      floatx4* p = (floatx4*)(slots + (int64_t)k * slot_stride + i);
      s += *p;
      if (clean) *p = floatx4{0.f, 0.f, 0.f, 0.f};
    }
  red[kl][cq] = s;
  __syncthreads();
#pragma unroll
  for (int w = 16; w > 0; w >>= 1) {
    if (kl < w) red[kl][cq] += red[kl + w][cq];
    __syncthreads();
  }
  if (kl == 0 && i < n) {
    float* o = i < C ? out0 + i : out1 + (i - C);
    if (overwrite) *(floatx4*)o = red[0][cq] * alpha;
    else *(floatx4*)o += red[0][cq] * alpha;
  }
}
template <typename F>
static int launch_col_reduce(hipStream_t st, const F& f, int rows, int C, float* out0, float* out1, const BnPass& pl, RowBound rb = RowBound(),
                             float* slots = nullptr, float alpha = 1.0f) {
  if (rows <= 0 || C <= 0) return RL_OK;
  if (C & 3) return RL_ERR_ARG;
  if (pl.g < 1) return RL_ERR_ARG;
  if (slots != nullptr) {      // per-chunk partial records + ordered fold: bitwise reproducible (col_reduce_plan keeps g * 2C <= COL_SLOT_FLOATS)
    hipLaunchKernelGGL((col_reduce_kernel<F>), dim3(pl.gx, pl.g), dim3(256), 0, st, f, rows, C, pl.tpr_shift, out0, out1, rb, slots, pl.stride);
    const int n = out1 ? 2 * C : C;
    hipLaunchKernelGGL(col_fold_kernel, dim3(pl.fold_wgs), dim3(256), 0, st, slots, pl.stride, pl.g, n, out0, out1, C, 1, 0, alpha);     // OVERWRITES out0 / out1
  } else {
    if (alpha != 1.0f) return RL_ERR_ARG;        // the scaled form exists on the record + fold path only
    hipLaunchKernelGGL((col_reduce_kernel<F>), dim3(pl.gx, pl.g), dim3(256), 0, st, f, rows, C, pl.tpr_shift, out0, out1, rb, (float*)nullptr, 0);
  }
  return RL_LAUNCH_CHECK();
}

// ---- bf16 fast path of the column reductions: 16-byte loads, C a power of two in [8, 2048] ----------------------------------
// One workgroup spans all C columns (C / 8 threads per row, 2048 / C rows per pass) over a contiguous chunk of rows.  The four row
// passes of an iteration are LOADED before the first is added (4 x 16 B per input tensor in flight per thread, against 4 x 8 B and
// a 64-bit row * ld multiply per load in the generic kernel), row weights come from a shift, and the per-column constants (mean,
// rstd) sit in registers for the whole loop.  Partial sums go to the chunk's record and the same ordered fold as above: bitwise
// reproducible.  The 64-channel reductions over the 957k rows of block 1 went from 1.1-1.6 TB/s to the figures in
// profiles/round3_bn_probe.log.
struct RowW16 {                       // multiplicity of a row's glyph (dedup), hw a power of two
  const float* counts; int hw_shift;
  __device__ __forceinline__ float operator()(int r) const { return counts ? counts[r >> hw_shift] : 1.0f; }
};
template <int N> struct Acc16 { floatx4 lo[N], hi[N]; };

struct WSum16F {                      // sum_r w_r x[r][c]
  static constexpr int NACC = 1;
  const bf16_t* x; RowW16 w;
  struct Item { uint4 x; };
  struct Ctx {};
  __device__ __forceinline__ Ctx prep(int, int) const { return Ctx{}; }
  __device__ __forceinline__ Item load(int64_t e) const { return Item{*(const uint4*)(x + e)}; }
  __device__ __forceinline__ void add(Acc16<1>& a, const Item& it, const Ctx&, int r) const {
    floatx4 lo, hi; unpack8(it.x, lo, hi);
    const float ww = w(r);
    a.lo[0] += lo * ww; a.hi[0] += hi * ww;
  }
};
struct SumSqC16F {                    // sum_r w_r (x[r][c] - mean[c])^2
  static constexpr int NACC = 1;
  const bf16_t* x; const float* mean; RowW16 w;
  struct Item { uint4 x; };
  struct Ctx { floatx4 mlo, mhi; };
  __device__ __forceinline__ Ctx prep(int col, int) const { return Ctx{*(const floatx4*)(mean + col), *(const floatx4*)(mean + col + 4)}; }
  __device__ __forceinline__ Item load(int64_t e) const { return Item{*(const uint4*)(x + e)}; }
  __device__ __forceinline__ void add(Acc16<1>& a, const Item& it, const Ctx& c, int r) const {
    floatx4 lo, hi; unpack8(it.x, lo, hi);
    lo -= c.mlo; hi -= c.mhi;
    const float ww = w(r);
    a.lo[0] += lo * lo * ww; a.hi[0] += hi * hi * ww;
  }
};
// BatchNorm backward sums of NB normalisations that share the incoming gradient and ReLU mask (bn2 and the shortcut's BN both feed
// out = relu(bn2(c2) + bns(cs)), char_cnn.py:30-32): acc 0 = sum g, acc 1 + b = sum g * xhat_b, with dy and the mask read ONCE.
template <int NB> struct BnBwd16F {
  static constexpr int NACC = 1 + NB;
  const bf16_t* dy; const bf16_t* relu_src; const bf16_t* x[NB]; const float* mean[NB]; const float* rstd[NB];
  struct Item { uint4 g, o, x[NB]; };
  struct Ctx { floatx4 mlo[NB], mhi[NB], rlo[NB], rhi[NB]; };
  __device__ __forceinline__ Ctx prep(int col, int) const {
    Ctx c;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      c.mlo[b] = *(const floatx4*)(mean[b] + col); c.mhi[b] = *(const floatx4*)(mean[b] + col + 4);
      c.rlo[b] = *(const floatx4*)(rstd[b] + col); c.rhi[b] = *(const floatx4*)(rstd[b] + col + 4);
    }
    return c;
  }
  __device__ __forceinline__ Item load(int64_t e) const {
    Item it;
    it.g = *(const uint4*)(dy + e);
    it.o = relu_src ? *(const uint4*)(relu_src + e) : uint4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
#pragma unroll
    for (int b = 0; b < NB; ++b) it.x[b] = *(const uint4*)(x[b] + e);
    return it;
  }
  __device__ __forceinline__ void add(Acc16<NACC>& a, const Item& it, const Ctx& c, int) const {
    floatx4 glo, ghi, olo, ohi;
    unpack8(it.g, glo, ghi); unpack8(it.o, olo, ohi);
#pragma unroll
    for (int j = 0; j < 4; ++j) { glo[j] = olo[j] > 0.f ? glo[j] : 0.f; ghi[j] = ohi[j] > 0.f ? ghi[j] : 0.f; }
    a.lo[0] += glo; a.hi[0] += ghi;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      floatx4 xlo, xhi; unpack8(it.x[b], xlo, xhi);
      a.lo[1 + b] += glo * ((xlo - c.mlo[b]) * c.rlo[b]);
      a.hi[1 + b] += ghi * ((xhi - c.mhi[b]) * c.rhi[b]);
    }
  }
};

// One-pass BatchNorm training statistics: S1 = sum w (x - K), S2 = sum w (x - K)^2 about the per-channel pivot K = the first row of
// the batch itself (round 3 pivoted on the running mean: fresh or foreign running statistics far from the batch mean made the
// subtraction below cancel - ADVICE round 3).  mean = K + S1 / n, var = S2 / n - (S1 / n)^2: with fp32 sums the cancellation error
// is ~1e-7 (1 + (mean - K)^2 / var) relative, far inside bf16 activations' own rounding; the fp32 parity mode keeps the two-pass form.
struct Moments16F {
  static constexpr int NACC = 2;
  const bf16_t* x; RowW16 w;
  struct Item { uint4 x; };
  struct Ctx { floatx4 klo, khi; };
  // pivot K = the batch's own first row (a sample of the distribution being measured: |mean - K| is of the order of the standard
  // deviation whatever the running statistics hold - fresh buffers, buffers loaded from another domain)
  // (no live row under a device-side bound of 0: row 0 is not read, the pivot is 0 - bn_fold_train_kernel adds the same back)
  __device__ __forceinline__ Ctx prep(int col, int rows) const {
    Ctx c;
    if (rows > 0) unpack8(*(const uint4*)(x + col), c.klo, c.khi);
    else c.klo = c.khi = floatx4{0.f, 0.f, 0.f, 0.f};
    return c;
  }
  __device__ __forceinline__ Item load(int64_t e) const { return Item{*(const uint4*)(x + e)}; }
  __device__ __forceinline__ void add(Acc16<2>& a, const Item& it, const Ctx& c, int r) const {
    floatx4 lo, hi; unpack8(it.x, lo, hi);
    lo -= c.klo; hi -= c.khi;
    const float ww = w(r);
    const floatx4 wlo = lo * ww, whi = hi * ww;
    a.lo[0] += wlo; a.hi[0] += whi;
    a.lo[1] += wlo * lo; a.hi[1] += whi * hi;
  }
};
// Ordered fold of the [S1 | S2] records (same lane / tree order as col_fold_kernel) + everything bn_train_kernel does, one workgroup
// per 32 channels: mean, rstd, scale, shift, running statistics (unbiased variance, momentum), num_batches_tracked.
__global__ void __launch_bounds__(256) bn_fold_train_kernel(const float* __restrict__ slots, int slot_stride, int nrec, int C, float inv_n, float unbias,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum,
                                                             float* rmean, float* rvar, float* mean, float* rstd, float* scale, float* shift, int64_t* nbt,
                                                             const bf16_t* __restrict__ x0, const int* __restrict__ rows_dev) {
  __shared__ floatx4 red[2][32][8];
  const int cq = threadIdx.x & 7, kl = threadIdx.x >> 3;
  const int c = (blockIdx.x * 8 + cq) * 4;
  floatx4 s1 = floatx4{0.f, 0.f, 0.f, 0.f}, s2 = s1;
  if (c < C)
    for (int k = kl; k < nrec; k += 32) {
      const float* rec = slots + (int64_t)k * slot_stride;
      s1 += *(const floatx4*)(rec + c);
      s2 += *(const floatx4*)(rec + C + c);
    }
  red[0][kl][cq] = s1; red[1][kl][cq] = s2;
  __syncthreads();
#pragma unroll
  for (int w = 16; w > 0; w >>= 1) {
    if (kl < w) { red[0][kl][cq] += red[0][kl + w][cq]; red[1][kl][cq] += red[1][kl + w][cq]; }
    __syncthreads();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && nbt != nullptr) *nbt += 1;
  if (kl == 0 && c < C) {
    const bool pivot = rows_dev == nullptr || *rows_dev > 0;
    s1 = red[0][0][cq]; s2 = red[1][0][cq];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = s1[j] * inv_n, m = (pivot ? to_f<bf16_t>(x0[c + j]) : 0.f) + d;   // the pivot was the batch's first row (Moments16F::prep)
      const float var = fmaxf(s2[j] * inv_n - d * d, 0.f);
      const float rs = 1.0f / sqrtf(var + eps), g = gamma[c + j];
      mean[c + j] = m; rstd[c + j] = rs; scale[c + j] = g * rs; shift[c + j] = beta[c + j] - m * g * rs;
      rmean[c + j] = (1.0f - momentum) * rmean[c + j] + momentum * m;
      rvar[c + j] = (1.0f - momentum) * rvar[c + j] + momentum * (var * unbias);
    }
  }
}
template <typename F>
__global__ void __launch_bounds__(256) col_reduce16_kernel(F f, int rows_max, int c_shift, RowBound rb, float* __restrict__ slots, int slot_stride,
                                                            int dup0_at) {
  __shared__ floatx4 red[2][256];
  const int tshift = c_shift - 3, tpr = 1 << tshift, rpp = 256 >> tshift;
  const int cx = threadIdx.x & (tpr - 1), ry = threadIdx.x >> tshift, col = cx * 8;
  const int rows = rb_rows(rb, rows_max);
  const int chunk = (rows + gridDim.x - 1) / gridDim.x;
  const int r0 = blockIdx.x * chunk, r1 = min(rows, r0 + chunk);
  Acc16<F::NACC> acc;
#pragma unroll
  for (int k = 0; k < F::NACC; ++k) acc.lo[k] = acc.hi[k] = floatx4{0.f, 0.f, 0.f, 0.f};
  const typename F::Ctx ctx = f.prep(col, rows);
  int r = r0 + ry;
  const int64_t step = (int64_t)rpp << c_shift;
  int64_t e = ((int64_t)r << c_shift) + col;
  for (; r + 3 * rpp < r1; r += 4 * rpp, e += 4 * step) {
    const typename F::Item i0 = f.load(e), i1 = f.load(e + step), i2 = f.load(e + 2 * step), i3 = f.load(e + 3 * step);
    f.add(acc, i0, ctx, r); f.add(acc, i1, ctx, r + rpp); f.add(acc, i2, ctx, r + 2 * rpp); f.add(acc, i3, ctx, r + 3 * rpp);
  }
  for (; r < r1; r += rpp, e += step) { const typename F::Item i0 = f.load(e); f.add(acc, i0, ctx, r); }
  float* rec = slots + (int64_t)blockIdx.x * slot_stride;
  const int C = 1 << c_shift;
#pragma unroll
  for (int k = 0; k < F::NACC; ++k) {
    red[0][threadIdx.x] = acc.lo[k];
    red[1][threadIdx.x] = acc.hi[k];
    __syncthreads();
    if (ry == 0) {
      floatx4 lo = acc.lo[k], hi = acc.hi[k];
      for (int j = 1; j < rpp; ++j) { lo += red[0][j * tpr + cx]; hi += red[1][j * tpr + cx]; }
      // record layout: accumulator k at [k * C, (k + 1) * C); with dup0_at > 0 (two normalisations) accumulator 0 is stored again at
      // dup0_at * C and accumulators >= dup0_at move up one slot, so that the folded output reads [sum g | sum g xhat_0 | sum g | sum g xhat_1]
      const int slot = (dup0_at > 0 && k >= dup0_at) ? k + 1 : k;
      *(floatx4*)(rec + slot * C + col) = lo; *(floatx4*)(rec + slot * C + col + 4) = hi;
      if (k == 0 && dup0_at > 0) { *(floatx4*)(rec + dup0_at * C + col) = lo; *(floatx4*)(rec + dup0_at * C + col + 4) = hi; }
    }
    __syncthreads();
  }
}
// nout = folded outputs of C floats each, written contiguously to `out` (overwritten); alpha scales them; pl: a BN_16B plan of col_reduce_plan
template <typename F>
static int launch_col_reduce16(hipStream_t st, const F& f, int rows, int C, float* out, int dup0_at, const RowBound& rb, float alpha, const BnPass& pl) {
  if (rows <= 0) return RL_OK;
  hipLaunchKernelGGL((col_reduce16_kernel<F>), dim3(pl.g), dim3(256), 0, st, f, rows, pow2_shift(C), rb, rb.slots, pl.stride, dup0_at);
  hipLaunchKernelGGL(col_fold_kernel, dim3(pl.fold_wgs), dim3(256), 0, st, rb.slots, pl.stride, pl.g, pl.stride, out, out + C, C, 1, 0, alpha);
  return RL_LAUNCH_CHECK();
}

template <typename T> struct SumF {
  const T* x; int64_t ld;
  __device__ __forceinline__ void operator()(int r, int c, floatx4& a0, floatx4&) const { a0 += load4<T>(x + (int64_t)r * ld + c); }
};
template <typename T> int bias_grad(hipStream_t st, const T* dy, int64_t ld, int rows, int N, float* out, const int* rows_dev) {
  if (ld & 3) return RL_ERR_ARG;
  SumF<T> f{dy, ld};
  RowBound rb;
  rb.rows_dev = rows_dev;
  return launch_col_reduce(st, f, rows, N, out, nullptr, col_reduce_plan((int)sizeof(T), rows, N, 1, false, 1, false), rb);
}
template int bias_grad<bf16_t>(hipStream_t, const bf16_t*, int64_t, int, int, float*, const int*);
template int bias_grad<float>(hipStream_t, const float*, int64_t, int, int, float*, const int*);

template <typename T> struct WSumF {
  const T* x; int64_t ld; RowBound rb;
  __device__ __forceinline__ void operator()(int r, int c, floatx4& a0, floatx4&) const {
    a0 += load4<T>(x + (int64_t)r * ld + c) * rb_weight(rb, r);
  }
};
template <typename T> int col_sum(hipStream_t st, const T* x, int P, int C, float* out, RowBound rb, float scale) {
  const BnPass pl = col_reduce_plan((int)sizeof(T), P, C, rb.hw, rb.slots != nullptr, 1, true);
  if constexpr (sizeof(T) == 2) {
    if (pl.kernel == BN_16B) { WSum16F f{x, RowW16{rb.counts, pow2_shift(rb.hw)}}; return launch_col_reduce16(st, f, P, C, out, 0, rb, scale, pl); }
  }
  WSumF<T> f{x, (int64_t)C, rb};
  return launch_col_reduce(st, f, P, C, out, nullptr, pl, rb, rb.slots, scale);
}
template int col_sum<bf16_t>(hipStream_t, const bf16_t*, int, int, float*, RowBound, float);
template int col_sum<float>(hipStream_t, const float*, int, int, float*, RowBound, float);

template <typename T> struct SumSqCF {
  const T* x; int64_t ld; const float* mean; RowBound rb;
  __device__ __forceinline__ void operator()(int r, int c, floatx4& a0, floatx4&) const {
    const floatx4 d = load4<T>(x + (int64_t)r * ld + c) - *(const floatx4*)(mean + c);
    a0 += d * d * rb_weight(rb, r);
  }
};
template <typename T> int col_sumsq_centered(hipStream_t st, const T* x, int P, int C, const float* mean, float* out, RowBound rb) {
  const BnPass pl = col_reduce_plan((int)sizeof(T), P, C, rb.hw, rb.slots != nullptr, 1, true);
  if constexpr (sizeof(T) == 2) {
    if (pl.kernel == BN_16B) { SumSqC16F f{x, mean, RowW16{rb.counts, pow2_shift(rb.hw)}}; return launch_col_reduce16(st, f, P, C, out, 0, rb, 1.0f, pl); }
  }
  SumSqCF<T> f{x, (int64_t)C, mean, rb};
  return launch_col_reduce(st, f, P, C, out, nullptr, pl, rb, rb.slots);
}
template int col_sumsq_centered<bf16_t>(hipStream_t, const bf16_t*, int, int, const float*, float*, RowBound);
template int col_sumsq_centered<float>(hipStream_t, const float*, int, int, const float*, float*, RowBound);

template <typename T> struct BnBwdF {
  const T* dy; const T* relu_src; const T* x; const float* mean; const float* rstd; int64_t ld;
  __device__ __forceinline__ void operator()(int r, int c, floatx4& a0, floatx4& a1) const {
    floatx4 g = load4<T>(dy + (int64_t)r * ld + c);
    if (relu_src != nullptr) {
      const floatx4 o = load4<T>(relu_src + (int64_t)r * ld + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = o[j] > 0.f ? g[j] : 0.f;
    }
    const floatx4 xh = (load4<T>(x + (int64_t)r * ld + c) - *(const floatx4*)(mean + c)) * *(const floatx4*)(rstd + c);
    a0 += g;
    a1 += g * xh;
  }
};
template <typename T>
int bn_bwd_reduce(hipStream_t st, const T* dy, const T* relu_src, const T* x, const float* mean, const float* rstd, int P, int C,
                  float* sums, RowBound rb) {
  const BnPass pl = col_reduce_plan((int)sizeof(T), P, C, rb.hw, rb.slots != nullptr, 2, true);
  if constexpr (sizeof(T) == 2) {
    if (pl.kernel == BN_16B) { BnBwd16F<1> f{dy, relu_src, {x}, {mean}, {rstd}}; return launch_col_reduce16(st, f, P, C, sums, 0, rb, 1.0f, pl); }
  }
  BnBwdF<T> f{dy, relu_src, x, mean, rstd, (int64_t)C};
  return launch_col_reduce(st, f, P, C, sums, sums + C, pl, rb, rb.slots);
}
int bn_stats_train16(hipStream_t st, const bf16_t* x, int P, int C, int n_stat, const float* gamma, const float* beta, float eps, float momentum,
                     float* rmean, float* rvar, float* mean, float* rstd, float* scale, float* shift, int64_t* nbt, RowBound rb) {
  const BnPass pl = bn_stats_plan(2, P, C, rb.hw, rb.slots != nullptr);
  if (pl.kernel != BN_ONEPASS) return RL_ERR_ARG;
  Moments16F f{x, RowW16{rb.counts, pow2_shift(rb.hw)}};
  hipLaunchKernelGGL((col_reduce16_kernel<Moments16F>), dim3(pl.g), dim3(256), 0, st, f, P, pow2_shift(C), rb, rb.slots, pl.stride, 0);
  const int n = n_stat > 0 ? n_stat : P;
  hipLaunchKernelGGL(bn_fold_train_kernel, dim3(pl.fold_wgs), dim3(256), 0, st, rb.slots, pl.stride, pl.g, C, 1.0f / (float)n,
                     (float)n / (float)(n > 1 ? n - 1 : 1), gamma, beta, eps, momentum, rmean, rvar, mean, rstd, scale, shift, nbt, x, rb.rows_dev);
  return RL_LAUNCH_CHECK();
}
// Two normalisations sharing dy and the ReLU mask: sums = [sum g | sum g xhat_a | sum g | sum g xhat_b] (4C floats).  Returns
// RL_ERR_ARG when the fast path does not apply (the caller then runs the two single reductions).
int bn_bwd_reduce2(hipStream_t st, const bf16_t* dy, const bf16_t* relu_src, const bf16_t* xa, const float* mean_a, const float* rstd_a,
                   const bf16_t* xb, const float* mean_b, const float* rstd_b, int P, int C, float* sums, RowBound rb) {
  if (!bn_pair_ok(2, P, C, rb.hw, rb.slots != nullptr)) return RL_ERR_ARG;
  BnBwd16F<2> f{dy, relu_src, {xa, xb}, {mean_a, mean_b}, {rstd_a, rstd_b}};
  return launch_col_reduce16(st, f, P, C, sums, 2, rb, 1.0f, col_reduce_plan(2, P, C, rb.hw, true, 4, true));
}
template int bn_bwd_reduce<bf16_t>(hipStream_t, const bf16_t*, const bf16_t*, const bf16_t*, const float*, const float*, int, int, float*, RowBound);
template int bn_bwd_reduce<float>(hipStream_t, const float*, const float*, const float*, const float*, const float*, int, int, float*, RowBound);

// ---- the two BatchNorm launch sequences (ops.h): what the plan above decides, issued here and nowhere else ----
template <typename T>
int bn_stats(hipStream_t st, const T* x, int P, int C, int n_stat, int training, const float* gamma, const float* beta, float eps, float momentum,
             float* rmean, float* rvar, int64_t* nbt, float* mean, float* rstd, float* scale, float* shift, float* scratch, RowBound rb) {
  if (!training) return bn_finalize_eval(st, C, gamma, beta, eps, rmean, rvar, scale, shift);
  const int n = n_stat > 0 ? n_stat : P;
  if constexpr (sizeof(T) == 2) {
    if (bn_stats_train16(st, x, P, C, n, gamma, beta, eps, momentum, rmean, rvar, mean, rstd, scale, shift, nbt, rb) == RL_OK) return RL_OK;
  }
  if (rb.slots != nullptr) {
    RL_TRY(col_sum<T>(st, x, P, C, mean, rb, 1.0f / (float)n));          // the fold writes the mean directly
  } else {
    RL_TRY(fill_f32(st, scratch, 0.0f, 2 * C));
    RL_TRY(col_sum<T>(st, x, P, C, scratch, rb));
    RL_TRY(bn_finalize_mean(st, scratch, C, n, mean));
  }
  RL_TRY(col_sumsq_centered<T>(st, x, P, C, mean, scratch + C, rb));
  return bn_finalize_train(st, mean, scratch + C, C, n, gamma, beta, eps, momentum, rmean, rvar, rstd, scale, shift, nbt);
}
template int bn_stats<bf16_t>(hipStream_t, const bf16_t*, int, int, int, int, const float*, const float*, float, float, float*, float*, int64_t*, float*,
                              float*, float*, float*, float*, RowBound);
template int bn_stats<float>(hipStream_t, const float*, int, int, int, int, const float*, const float*, float, float, float*, float*, int64_t*, float*,
                             float*, float*, float*, float*, RowBound);
template <typename T>
int bn_backward(hipStream_t st, const T* dy, const T* relu_src, int P, int C, int n_stat, const BnBranch<T>& a, const BnBranch<T>& b, float* sums,
                RowBound rb) {
  if constexpr (sizeof(T) == 2) {
    // (paired while bn_pair_ok says so: the 16-byte kernels apply and 4 C floats fit the sums scratch)
    if (b.x != nullptr && bn_bwd_reduce2(st, dy, relu_src, a.x, a.mean, a.rstd, b.x, b.mean, b.rstd, P, C, sums, rb) == RL_OK)
      return bn_bwd_apply2(st, dy, relu_src, a.x, a.mean, a.rstd, a.gamma, a.dx, a.dgamma, a.dbeta, b.x, b.mean, b.rstd, b.gamma, b.dx, b.dgamma,
                           b.dbeta, sums, P, C, rb, n_stat);
  }
  for (const BnBranch<T>* br : {&a, &b}) {
    if (br->x == nullptr) continue;
    if (rb.slots == nullptr) RL_TRY(fill_f32(st, sums, 0.0f, 2 * C));      // (atomics; with records the reduction overwrites)
    RL_TRY(bn_bwd_reduce<T>(st, dy, relu_src, br->x, br->mean, br->rstd, P, C, sums, rb));
    RL_TRY(bn_bwd_apply<T>(st, dy, relu_src, br->x, br->mean, br->rstd, br->gamma, sums, P, C, br->dx, br->dgamma, br->dbeta, rb, n_stat));
  }
  return RL_OK;
}
template int bn_backward<bf16_t>(hipStream_t, const bf16_t*, const bf16_t*, int, int, int, const BnBranch<bf16_t>&, const BnBranch<bf16_t>&, float*, RowBound);
template int bn_backward<float>(hipStream_t, const float*, const float*, int, int, int, const BnBranch<float>&, const BnBranch<float>&, float*, RowBound);

// ---------------------------------------------------------------------------------------------
// BatchNorm2d over NHWC [P][C] (char_cnn.py:17-28): statistics come from col_sum /
// col_sumsq_centered (above); these kernels finalise and apply them.
// ---------------------------------------------------------------------------------------------
__global__ void bn_mean_kernel(const float* sum, int C, float inv_p, float* mean) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) mean[c] = sum[c] * inv_p;
}
int bn_finalize_mean(hipStream_t st, const float* sum, int C, int P, float* mean) {
  hipLaunchKernelGGL(bn_mean_kernel, dim3((C + 255) / 256), dim3(256), 0, st, sum, C, 1.0f / (float)P, mean);
  return RL_LAUNCH_CHECK();
}
__global__ void bn_train_kernel(const float* mean, const float* sqsum, int C, int P, const float* gamma, const float* beta,
                                float eps, float momentum, float* rmean, float* rvar, float* rstd, float* scale, float* shift, int64_t* nbt) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && nbt != nullptr) *nbt += 1;                               // num_batches_tracked
  if (c >= C) return;
  const float var = sqsum[c] / (float)P;                                 // biased: used to normalise
  const float unbiased = sqsum[c] / (float)(P > 1 ? P - 1 : 1);          // running_var update
  const float rs = 1.0f / sqrtf(var + eps);
  rstd[c] = rs;
  scale[c] = gamma[c] * rs;
  shift[c] = beta[c] - mean[c] * gamma[c] * rs;
  rmean[c] = (1.0f - momentum) * rmean[c] + momentum * mean[c];
  rvar[c] = (1.0f - momentum) * rvar[c] + momentum * unbiased;
}
int bn_finalize_train(hipStream_t st, const float* mean, const float* sqsum, int C, int P, const float* gamma, const float* beta,
                      float eps, float momentum, float* running_mean, float* running_var, float* rstd, float* scale, float* shift,
                      int64_t* num_batches_tracked) {
  hipLaunchKernelGGL(bn_train_kernel, dim3((C + 255) / 256), dim3(256), 0, st, mean, sqsum, C, P, gamma, beta, eps, momentum,
                     running_mean, running_var, rstd, scale, shift, num_batches_tracked);
  return RL_LAUNCH_CHECK();
}
__global__ void bn_eval_kernel(int C, const float* gamma, const float* beta, float eps, const float* rmean, const float* rvar,
                               float* scale, float* shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float rs = 1.0f / sqrtf(rvar[c] + eps);
  scale[c] = gamma[c] * rs;
  shift[c] = beta[c] - rmean[c] * gamma[c] * rs;
}
int bn_finalize_eval(hipStream_t st, int C, const float* gamma, const float* beta, float eps, const float* running_mean,
                     const float* running_var, float* scale, float* shift) {
  hipLaunchKernelGGL(bn_eval_kernel, dim3((C + 255) / 256), dim3(256), 0, st, C, gamma, beta, eps, running_mean, running_var,
                     scale, shift);
  return RL_LAUNCH_CHECK();
}

template <typename T>
__global__ void bn_apply_kernel(const T* __restrict__ x1, const float* __restrict__ sc1, const float* __restrict__ sh1,
                                const T* __restrict__ x2, const float* __restrict__ sc2, const float* __restrict__ sh2,
                                T* __restrict__ y, int P, int C, int relu, RowBound rb) {
  const int64_t n = (int64_t)rb_rows(rb, P) * C;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * blockDim.x * 4) {
    const int c = (int)(i % C);
    floatx4 v = load4<T>(x1 + i) * *(const floatx4*)(sc1 + c) + *(const floatx4*)(sh1 + c);
    if (x2 != nullptr) v += load4<T>(x2 + i) * *(const floatx4*)(sc2 + c) + *(const floatx4*)(sh2 + c);
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    }
    store4<T>(y + i, v);
  }
}
// ---- bf16 fast paths of the BatchNorm maps: 16-byte accesses, C and hw powers of two ------------------------------------------
// A thread owns 8 consecutive channels; the grid stride (workgroups x 2048 elements) is a multiple of C, so its channels never
// change and scale / shift / mean / rstd / gamma live in registers for the whole loop; rows and glyph multiplicities come from
// shifts (the generic kernels pay a 64-bit i % C and i / C per 4 elements); four items are loaded before the first is used.
struct F8 { floatx4 lo, hi; };
__device__ __forceinline__ F8 ld8f(const float* p) { return F8{*(const floatx4*)p, *(const floatx4*)(p + 4)}; }

template <int NX>
__global__ void __launch_bounds__(256) bn_apply16_kernel(const bf16_t* __restrict__ x1, const float* __restrict__ sc1, const float* __restrict__ sh1,
                                                          const bf16_t* __restrict__ x2, const float* __restrict__ sc2, const float* __restrict__ sh2,
                                                          bf16_t* __restrict__ y, int P, int c_shift, int relu, RowBound rb) {
  const int64_t n8 = ((int64_t)rb_rows(rb, P) << c_shift) >> 3;
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)((i << 3) & ((1 << c_shift) - 1));
  const F8 s1 = ld8f(sc1 + c), h1 = ld8f(sh1 + c);
  F8 s2 = s1, h2 = h1;
  if constexpr (NX == 2) { s2 = ld8f(sc2 + c); h2 = ld8f(sh2 + c); }
  auto one = [&](int64_t k, uint4 u1, uint4 u2) {
    floatx4 lo, hi; unpack8(u1, lo, hi);
    lo = lo * s1.lo + h1.lo; hi = hi * s1.hi + h1.hi;
    if constexpr (NX == 2) {
      floatx4 lo2, hi2; unpack8(u2, lo2, hi2);
      lo += lo2 * s2.lo + h2.lo; hi += hi2 * s2.hi + h2.hi;
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { lo[j] = fmaxf(lo[j], 0.f); hi[j] = fmaxf(hi[j], 0.f); }
    }
    store8<bf16_t>(y + (k << 3), lo, hi);
  };
  const uint4* p1 = (const uint4*)x1; const uint4* p2 = (const uint4*)x2;
  for (; i + 3 * stride < n8; i += 4 * stride) {
    const uint4 a0 = p1[i], a1 = p1[i + stride], a2 = p1[i + 2 * stride], a3 = p1[i + 3 * stride];
    uint4 b0 = a0, b1 = a1, b2 = a2, b3 = a3;
    if constexpr (NX == 2) { b0 = p2[i]; b1 = p2[i + stride]; b2 = p2[i + 2 * stride]; b3 = p2[i + 3 * stride]; }
    one(i, a0, b0); one(i + stride, a1, b1); one(i + 2 * stride, a2, b2); one(i + 3 * stride, a3, b3);
  }
  for (; i < n8; i += stride) { const uint4 a0 = p1[i]; uint4 b0 = a0; if constexpr (NX == 2) b0 = p2[i]; one(i, a0, b0); }
}

// dx_b = gamma_b rstd_b (g - w m1 - xhat_b w m2_b) for NB normalisations that share dy and the ReLU mask (bn2 + shortcut BN)
struct BnBwdBranch { const bf16_t* x; const float* mean; const float* rstd; const float* gamma; const float* sums; bf16_t* dx; float* dgamma; float* dbeta; };
template <int NB>
__global__ void __launch_bounds__(256) bn_bwd_apply16_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ relu_src, BnBwdBranch b0,
                                                              BnBwdBranch b1, int P, int c_shift, int hw_shift, float inv_p, RowBound rb) {
  const int C = 1 << c_shift;
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < C; c += 256) {
      if (b0.dgamma != nullptr) { b0.dbeta[c] += b0.sums[c]; b0.dgamma[c] += b0.sums[C + c]; }
      if (NB == 2 && b1.dgamma != nullptr) { b1.dbeta[c] += b1.sums[c]; b1.dgamma[c] += b1.sums[C + c]; }
    }
  }
  const int64_t n8 = ((int64_t)rb_rows(rb, P) << c_shift) >> 3;
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)((i << 3) & (C - 1));
  const BnBwdBranch br[2] = {b0, b1};
  F8 mean[NB], k0[NB], rs[NB], m2[NB];
  const F8 m1 = ld8f(b0.sums + c);                      // sum g is the same for both branches
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    mean[b] = ld8f(br[b].mean + c); rs[b] = ld8f(br[b].rstd + c); m2[b] = ld8f(br[b].sums + C + c);
    const F8 g = ld8f(br[b].gamma + c);
    k0[b].lo = g.lo * rs[b].lo; k0[b].hi = g.hi * rs[b].hi;
  }
  const int row_shift = c_shift - 3 + hw_shift;         // item index -> glyph index
  const uint4* pg = (const uint4*)dy; const uint4* po = (const uint4*)relu_src;
  auto one = [&](int64_t k, uint4 ug, uint4 uo, const uint4* ux) {
    floatx4 glo, ghi, olo, ohi;
    unpack8(ug, glo, ghi);
    if (relu_src != nullptr) {
      unpack8(uo, olo, ohi);
#pragma unroll
      for (int j = 0; j < 4; ++j) { glo[j] = olo[j] > 0.f ? glo[j] : 0.f; ghi[j] = ohi[j] > 0.f ? ghi[j] : 0.f; }
    }
    const float w = (rb.counts ? rb.counts[k >> row_shift] : 1.0f) * inv_p;
    const floatx4 a_lo = glo - m1.lo * w, a_hi = ghi - m1.hi * w;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      floatx4 xlo, xhi; unpack8(ux[b], xlo, xhi);
      xlo = (xlo - mean[b].lo) * rs[b].lo; xhi = (xhi - mean[b].hi) * rs[b].hi;
      store8<bf16_t>(br[b].dx + (k << 3), k0[b].lo * (a_lo - xlo * (m2[b].lo * w)), k0[b].hi * (a_hi - xhi * (m2[b].hi * w)));
    }
  };
  for (; i + stride < n8; i += 2 * stride) {
    const uint4 g0 = pg[i], g1 = pg[i + stride];
    uint4 o0 = g0, o1 = g1;
    if (relu_src != nullptr) { o0 = po[i]; o1 = po[i + stride]; }
    uint4 x0[NB], x1[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { x0[b] = ((const uint4*)br[b].x)[i]; x1[b] = ((const uint4*)br[b].x)[i + stride]; }
    one(i, g0, o0, x0); one(i + stride, g1, o1, x1);
  }
  for (; i < n8; i += stride) {
    const uint4 g0 = pg[i];
    uint4 o0 = g0;
    if (relu_src != nullptr) o0 = po[i];
    uint4 x0[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) x0[b] = ((const uint4*)br[b].x)[i];
    one(i, g0, o0, x0);
  }
}
// the two-branch backward map (bn2 + shortcut BN of a BasicBlock): RL_ERR_ARG when the fast path does not apply
int bn_bwd_apply2(hipStream_t st, const bf16_t* dy, const bf16_t* relu_src, const bf16_t* xa, const float* mean_a, const float* rstd_a,
                  const float* gamma_a, bf16_t* dxa, float* dgamma_a, float* dbeta_a, const bf16_t* xb, const float* mean_b, const float* rstd_b,
                  const float* gamma_b, bf16_t* dxb, float* dgamma_b, float* dbeta_b, const float* sums4, int P, int C, RowBound rb, int n_stat) {
  if (!bn_pair_ok(2, P, C, rb.hw, true)) return RL_ERR_ARG;
  const BnBwdBranch b0{xa, mean_a, rstd_a, gamma_a, sums4, dxa, dgamma_a, dbeta_a}, b1{xb, mean_b, rstd_b, gamma_b, sums4 + 2 * C, dxb, dgamma_b, dbeta_b};
  const int64_t n8 = (int64_t)P * C / 8;
  hipLaunchKernelGGL((bn_bwd_apply16_kernel<2>), dim3(ew16_blocks(n8)), dim3(256), 0, st, dy, relu_src, b0, b1, P, pow2_shift(C), pow2_shift(rb.hw),
                     1.0f / (float)(n_stat > 0 ? n_stat : P), rb);
  return RL_LAUNCH_CHECK();
}

template <typename T>
int bn_apply(hipStream_t st, const T* x1, const float* sc1, const float* sh1, const T* x2, const float* sc2, const float* sh2,
             T* y, int P, int C, int relu, RowBound rb) {
  if (C & 3) return RL_ERR_ARG;
  const int64_t n = (int64_t)P * C;
  if constexpr (sizeof(T) == 2) {
    if (bn_map_plan(2, P, C, rb.hw).kernel == BN_16B) {
      if (x2 != nullptr) hipLaunchKernelGGL((bn_apply16_kernel<2>), dim3(ew16_blocks(n / 8)), dim3(256), 0, st, x1, sc1, sh1, x2, sc2, sh2, y, P, pow2_shift(C), relu, rb);
      else hipLaunchKernelGGL((bn_apply16_kernel<1>), dim3(ew16_blocks(n / 8)), dim3(256), 0, st, x1, sc1, sh1, x2, sc2, sh2, y, P, pow2_shift(C), relu, rb);
      return RL_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL((bn_apply_kernel<T>), dim3(ew_blocks(n / 4)), dim3(256), 0, st, x1, sc1, sh1, x2, sc2, sh2, y, P, C, relu, rb);
  return RL_LAUNCH_CHECK();
}
template int bn_apply<bf16_t>(hipStream_t, const bf16_t*, const float*, const float*, const bf16_t*, const float*, const float*, bf16_t*, int, int, int, RowBound);
template int bn_apply<float>(hipStream_t, const float*, const float*, const float*, const float*, const float*, const float*, float*, int, int, int, RowBound);

template <typename T>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ relu_src, const T* __restrict__ x,
                                    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
                                    const float* __restrict__ sums, int P, int C, float inv_p, T* __restrict__ dx, RowBound rb,
                                    float* dgamma, float* dbeta) {
  if (blockIdx.x == 0 && dgamma != nullptr)            // parameter gradients ride along: dbeta += sum g, dgamma += sum g * xhat
    for (int c = threadIdx.x; c < C; c += blockDim.x) { dbeta[c] += sums[c]; dgamma[c] += sums[C + c]; }
  const int64_t n = (int64_t)rb_rows(rb, P) * C;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * blockDim.x * 4) {
    const int c = (int)(i % C);
    const float w = rb_weight(rb, (int)(i / C));
    floatx4 g = load4<T>(dy + i);
    if (relu_src != nullptr) {
      const floatx4 o = load4<T>(relu_src + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = o[j] > 0.f ? g[j] : 0.f;
    }
    const floatx4 rs = *(const floatx4*)(rstd + c);
    const floatx4 xh = (load4<T>(x + i) - *(const floatx4*)(mean + c)) * rs;
    const floatx4 m1 = *(const floatx4*)(sums + c) * (inv_p * w), m2 = *(const floatx4*)(sums + C + c) * (inv_p * w);
    store4<T>(dx + i, *(const floatx4*)(gamma + c) * rs * (g - m1 - xh * m2));
  }
}
__global__ void bn_param_grad_kernel(const float* sums, int C, float* dgamma, float* dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) { dbeta[c] += sums[c]; dgamma[c] += sums[C + c]; }
}
template <typename T>
int bn_bwd_apply(hipStream_t st, const T* dy, const T* relu_src, const T* x, const float* mean, const float* rstd,
                 const float* gamma, const float* sums, int P, int C, T* dx, float* dgamma, float* dbeta, RowBound rb, int n_stat) {
  if (C & 3) return RL_ERR_ARG;
  const int64_t n = (int64_t)P * C;
  if constexpr (sizeof(T) == 2) {
    if (bn_map_plan(2, P, C, rb.hw).kernel == BN_16B) {
      const BnBwdBranch b0{x, mean, rstd, gamma, sums, dx, dgamma, dbeta};
      hipLaunchKernelGGL((bn_bwd_apply16_kernel<1>), dim3(ew16_blocks(n / 8)), dim3(256), 0, st, dy, relu_src, b0, b0, P, pow2_shift(C), pow2_shift(rb.hw),
                         1.0f / (float)(n_stat > 0 ? n_stat : P), rb);
      return RL_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL((bn_bwd_apply_kernel<T>), dim3(ew_blocks(n / 4)), dim3(256), 0, st, dy, relu_src, x, mean, rstd, gamma,
                     sums, P, C, 1.0f / (float)(n_stat > 0 ? n_stat : P), dx, rb, dgamma, dbeta);
  return RL_LAUNCH_CHECK();
}
template int bn_bwd_apply<bf16_t>(hipStream_t, const bf16_t*, const bf16_t*, const bf16_t*, const float*, const float*, const float*, const float*, int, int, bf16_t*, float*, float*, RowBound, int);
template int bn_bwd_apply<float>(hipStream_t, const float*, const float*, const float*, const float*, const float*, const float*, const float*, int, int, float*, float*, float*, RowBound, int);

template <typename T>
__global__ void relu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ src, T* __restrict__ g, int64_t n) {
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * blockDim.x * 4) {
    floatx4 d = load4<T>(dy + i);
    const floatx4 o = load4<T>(src + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = o[j] > 0.f ? d[j] : 0.f;
    store4<T>(g + i, d);
  }
}
template <typename T> int relu_bwd(hipStream_t st, const T* dy, const T* relu_src, T* g, int64_t n) {
  if (n & 3) return RL_ERR_ARG;
  hipLaunchKernelGGL((relu_bwd_kernel<T>), dim3(ew_blocks(n / 4)), dim3(256), 0, st, dy, relu_src, g, n);
  return RL_LAUNCH_CHECK();
}
template int relu_bwd<bf16_t>(hipStream_t, const bf16_t*, const bf16_t*, bf16_t*, int64_t);
template int relu_bwd<float>(hipStream_t, const float*, const float*, float*, int64_t);

}  // namespace rl
