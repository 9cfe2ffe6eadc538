// LayerNorm (K1, K4 tail, K10; the "LayerNorm" section of ops.h): the forward with the embedding sum in front of it (one wave per row,
// and the bf16 half-wave-per-row fast path), the three backward kernels with the fold of their [dgamma | dbeta] records (ln_fold,
// ln_fold_multi), and the backward fused with the erf-GELU backward of the prediction head.  One 64-lane wave per row with 8-16 byte
// per-lane accesses (a 768-wide row = 3 coalesced 4-element vectors per lane); statistics are always fp32.  The _chw4 forward lives
// with the other flatten kernels in glyph_rows.hip.
#include "ops.h"
#include "launch.h"
#include "rows.h"

namespace rl {

// ---- knobs (ops.h: set_ln_fast / set_ln_v2 / set_ln_bwd_blocks) ----
static int g_ln_fast = 1, g_ln_bwd_blocks = 512;
// round 5 (realise_set_ln key 5): 1 = the row reductions of the bf16 LayerNorm kernels through DPP (wave_sum_dpp) and the backward on
// ln_bwd16v2_kernel (no barrier before the first row, four rows of a wave in flight, one-barrier epilogue); 0 = the round-4 kernels
static int g_ln_v2 = 1, g_ln_bwd_blocks_v2 = 256;
void set_ln_v2(int on) { g_ln_v2 = on; }
void set_ln_fast(int on) { g_ln_fast = on; }
void set_ln_bwd_blocks(int n) { if (g_ln_v2) g_ln_bwd_blocks_v2 = n > 0 ? n : 256; else g_ln_bwd_blocks = n > 0 ? n : 512; }      // (of the active variant)

// ---------------------------------------------------------------------------------------------
// LayerNorm forward (BertEmbeddings modeling_bert.py:183-193, BertSelfOutput/BertOutput :273-277,
// :339-343, resnet_layernorm models.py:838)
// ---------------------------------------------------------------------------------------------
// in_mode 3: columns c .. c + 3 of a token-table row with ONE 16-byte load per lane.  fp32: the four floats.  bf16: the 16-byte chunk of
// eight columns that holds them (two neighbouring lanes read the same chunk and keep a half each), so a lane ends up with exactly the
// columns - and the sums - of the 8-byte load of modes 0 / 2.
template <typename T> __device__ __forceinline__ floatx4 load4_of16(const T* row, int c);
template <> __device__ __forceinline__ floatx4 load4_of16<float>(const float* row, int c) { return *(const floatx4*)(row + c); }
template <> __device__ __forceinline__ floatx4 load4_of16<bf16_t>(const bf16_t* row, int c) {
  const uint4 u = *(const uint4*)(row + (c & ~7));
  const uint32_t lo = (c & 4) ? u.z : u.x, hi = (c & 4) ? u.w : u.y;
  floatx4 r;
  r[0] = __uint_as_float(lo << 16); r[1] = __uint_as_float(lo & 0xffff0000u);
  r[2] = __uint_as_float(hi << 16); r[3] = __uint_as_float(hi & 0xffff0000u);
  return r;
}

template <typename T>
__global__ void __launch_bounds__(256) ln_fwd_kernel(LnFwdArgs<T> a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= a.rows) return;
  const int H = a.H;
  const int64_t ldy = a.ldy ? a.ldy : (int64_t)H;
  floatx4 v[LN_MAXV];
  float sum = 0.f;
  const int64_t tok = (a.in_mode == 1 || a.in_mode == 3) ? a.ids[row] : 0;
  const int prow = a.pos_zero ? 0 : (row % a.S);
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    if (c < H) {
      floatx4 x;
      if (a.in_mode == 1) x = *(const floatx4*)(a.word + tok * H + c);
      else if (a.in_mode == 3) x = load4_of16<T>(a.x + tok * (a.ld_in ? a.ld_in : (int64_t)H), c);
      else x = load4<T>(a.x + (int64_t)(a.row_index ? a.row_index[row] : row) * H + c);
      if (a.in_mode != 0) x += *(const floatx4*)(a.pos + (int64_t)prow * H + c) + *(const floatx4*)(a.type0 + c);
      v[i] = x;
      sum += x[0] + x[1] + x[2] + x[3];
    }
  }
  const float mean = wave_sum(sum) / (float)H;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mean; sq += d * d; }
    }
  }
  const float var = wave_sum(sq) / (float)H;
  const float rstd = 1.0f / sqrtf(var + a.eps);
  if (lane == 0 && a.rstd != nullptr) a.rstd[row] = rstd;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      const floatx4 gm = *(const floatx4*)(a.gamma + c), bt = *(const floatx4*)(a.beta + c);
      floatx4 xh, y;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xh[j] = (v[i][j] - mean) * rstd;
        y[j] = xh[j] * gm[j] + bt[j];
      }
      y *= drop_mult4(a.drop.seed, a.drop.thresh, a.drop.scale, (uint32_t)row * (uint32_t)H + (uint32_t)c);       // H % 4 == 0
      if (a.xhat != nullptr) store4<T>(a.xhat + (int64_t)row * H + c, xh);
      store4<T>(a.y + (int64_t)row * ldy + c, y);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// bf16 fast path of the two kernels below (H % 256 == 0, H <= 1024, plain input): HALF a wave owns a row - 32 lanes x NV8 chunks
// of 8 consecutive columns - so every global access is 16 bytes per lane (the 8-byte accesses of the one-wave-per-row form run at
// 0.55-0.7 of that rate, MI355X_MICROARCH.md) and a wave-instruction covers two whole 512-byte row segments; a wave keeps RP
// row pairs in flight (all loads issued before the first reduction).  Reductions run inside the 32-lane half.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float half_sum(float v) {        // sum over the 32 lanes of this half-wave
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int NV8, int RP, bool DPP>
__global__ void __launch_bounds__(256) ln_fwd16_kernel(LnFwdArgs<bf16_t> a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
  const int H = a.H;
  const int row0 = (blockIdx.x * 4 + wave) * (2 * RP) + half;
  if (a.row_live != nullptr) {           // (the wave's 2 RP rows lie in one 16-row block: wave-uniform)
    static_assert(16 % (2 * RP) == 0, "a wave's rows must not straddle 16-row blocks");
    const uint4 lv = *(const uint4*)(a.row_live + (((blockIdx.x * 4 + wave) * (2 * RP)) & ~15));
    if ((lv.x | lv.y | lv.z | lv.w) == 0u) return;
  }
  uint4 raw[RP][NV8];
#pragma unroll
  for (int r = 0; r < RP; ++r) {
    const int row = row0 + 2 * r;
#pragma unroll
    for (int i = 0; i < NV8; ++i)
      raw[r][i] = row < a.rows ? *(const uint4*)((const char*)a.x + ((int64_t)row * H + (i * 32 + hl) * 8) * 2) : uint4{0u, 0u, 0u, 0u};
  }
  float gm[NV8][8], bt[NV8][8];
#pragma unroll
  for (int i = 0; i < NV8; ++i) {
    const int c = (i * 32 + hl) * 8;
    *(floatx4*)&gm[i][0] = *(const floatx4*)(a.gamma + c); *(floatx4*)&gm[i][4] = *(const floatx4*)(a.gamma + c + 4);
    *(floatx4*)&bt[i][0] = *(const floatx4*)(a.beta + c); *(floatx4*)&bt[i][4] = *(const floatx4*)(a.beta + c + 4);
  }
#pragma unroll
  for (int r = 0; r < RP; ++r) {
    const int row = row0 + 2 * r;
    float v[NV8][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV8; ++i) {
      unpack8(raw[r][i], v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    }
    const float mean = (DPP ? half_sum_dpp(sum, half) : half_sum(sum)) / (float)H;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NV8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; sq += d * d; }
    const float rstd = 1.0f / sqrtf((DPP ? half_sum_dpp(sq, half) : half_sum(sq)) / (float)H + a.eps);
    if (row >= a.rows) continue;
    if (hl == 0 && a.rstd != nullptr) a.rstd[row] = rstd;
#pragma unroll
    for (int i = 0; i < NV8; ++i) {
      const int c = (i * 32 + hl) * 8;
      float xh[8], y[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xh[j] = (v[i][j] - mean) * rstd;
        y[j] = xh[j] * gm[i][j] + bt[i][j];
      }
      if (a.drop.thresh != 0u) {
        const floatx4 d0 = drop_mult4(a.drop.seed, a.drop.thresh, a.drop.scale, (uint32_t)row * (uint32_t)H + (uint32_t)c);
        const floatx4 d1 = drop_mult4(a.drop.seed, a.drop.thresh, a.drop.scale, (uint32_t)row * (uint32_t)H + (uint32_t)c + 4u);
#pragma unroll
        for (int j = 0; j < 4; ++j) { y[j] *= d0[j]; y[4 + j] *= d1[j]; }
      }
      if (a.xhat != nullptr) *(uint4*)((char*)a.xhat + ((int64_t)row * H + c) * 2) = pack8(xh);
      *(uint4*)((char*)a.y + ((int64_t)row * H + c) * 2) = pack8(y);
    }
  }
}

template <typename T> int ln_fwd_fast(hipStream_t st, const LnFwdArgs<T>& a) { return -1; }
template <> int ln_fwd_fast<bf16_t>(hipStream_t st, const LnFwdArgs<bf16_t>& a) {
  if (!g_ln_fast || a.in_mode != 0 || a.row_index != nullptr || (a.H % 256) != 0 || a.H > 1024 || (a.ldy != 0 && a.ldy != a.H)) return -1;
  constexpr int RP = 2;
  const int blocks = (a.rows + 4 * 2 * RP - 1) / (4 * 2 * RP);
#define RL_LNF(NV) do { if (g_ln_v2) hipLaunchKernelGGL((ln_fwd16_kernel<NV, RP, true>), dim3(blocks), dim3(256), 0, st, a); \
                       else hipLaunchKernelGGL((ln_fwd16_kernel<NV, RP, false>), dim3(blocks), dim3(256), 0, st, a); } while (0)
  switch (a.H / 256) {
    case 1: RL_LNF(1); break;
    case 2: RL_LNF(2); break;
    case 3: RL_LNF(3); break;
    default: RL_LNF(4); break;
  }
#undef RL_LNF
  return RL_LAUNCH_CHECK();
}

template <typename T> int ln_fwd(hipStream_t st, const LnFwdArgs<T>& a) {
  if (a.rows <= 0) return RL_OK;
  if ((a.H & 3) || a.H > LN_MAXV * 256) return RL_ERR_ARG;
  if (a.in_mode == 3 && ((a.H & 7) || (a.ld_in & 7) || (a.ld_in != 0 && a.ld_in < a.H) || !a.ids || !a.x)) return RL_ERR_ARG;      // whole 16-byte chunks
  { const int rc = ln_fwd_fast<T>(st, a); if (rc >= 0) return rc; }
  hipLaunchKernelGGL((ln_fwd_kernel<T>), dim3((a.rows + 3) / 4), dim3(256), 0, st, a);
  return RL_LAUNCH_CHECK();
}
template int ln_fwd<bf16_t>(hipStream_t, const LnFwdArgs<bf16_t>&);
template int ln_fwd<float>(hipStream_t, const LnFwdArgs<float>&);

// ---------------------------------------------------------------------------------------------
// LayerNorm backward: dx = rstd * (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat)); dgamma/dbeta
// partials are kept in registers across a grid-stride loop over rows, reduced through LDS, then
// one atomicAdd per column per workgroup.
// ---------------------------------------------------------------------------------------------
template <typename T, int NV>
__global__ void __launch_bounds__(256) ln_bwd_kernel(LnBwdArgs<T> a) {
  __shared__ float red[2][4][NV * 256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int H = a.H;
  floatx4 dg[NV], db[NV], gm[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    dg[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    db[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    const int c = (i * 64 + lane) * 4;
    gm[i] = c < H ? *(const floatx4*)(a.gamma + c) : floatx4{0.f, 0.f, 0.f, 0.f};
  }
  // padding rows (row_live[row] == 0, a wave owns a row: wave-uniform): dy is an exact zero, so dx is - written without reading the row
  auto dead = [&](int row) -> bool { return a.row_live != nullptr && row < a.rows && a.row_live[row] == 0; };
  auto load_row = [&](int row, floatx4 (&dy)[NV], floatx4 (&xh)[NV]) {
    const bool skip = dead(row);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      dy[i] = floatx4{0.f, 0.f, 0.f, 0.f};
      xh[i] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (c < H && row < a.rows && !skip) {
        dy[i] = load4<T>(a.dy + (int64_t)row * H + c);
        xh[i] = load4<T>(a.xhat + (int64_t)row * H + c);
      }
    }
  };
  auto do_row = [&](int row, floatx4 (&dy)[NV], floatx4 (&xh)[NV]) {
    if (dead(row)) {
      const floatx4 z4 = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < H) { store4<T>(a.dx + (int64_t)row * H + c, z4); if (a.dx_drop != nullptr) store4<T>(a.dx_drop + (int64_t)row * H + c, z4); }
      }
      return;
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        const floatx4 dm_in = drop_mult4(a.in_drop.seed, a.in_drop.thresh, a.in_drop.scale, (uint32_t)row * (uint32_t)H + (uint32_t)c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dy[i][j] *= dm_in[j];
          const float t = dy[i][j] * gm[i][j];
          s1 += t;
          s2 += t * xh[i][j];
          dg[i][j] += dy[i][j] * xh[i][j];
          db[i][j] += dy[i][j];
        }
      }
    }
    s1 = wave_sum(s1) / (float)H;
    s2 = wave_sum(s2) / (float)H;
    const float rstd = a.rstd[row];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        floatx4 dx, dxd;
#pragma unroll
        for (int j = 0; j < 4; ++j) dx[j] = rstd * (dy[i][j] * gm[i][j] - s1 - xh[i][j] * s2);
        dxd = dx * drop_mult4(a.out_drop.seed, a.out_drop.thresh, a.out_drop.scale, (uint32_t)row * (uint32_t)H + (uint32_t)c);
        store4<T>(a.dx + (int64_t)row * H + c, dx);
        if (a.dx_drop != nullptr) store4<T>(a.dx_drop + (int64_t)row * H + c, dxd);
      }
    }
  };
  // two rows of a wave in flight: both rows' loads are issued before either row's reductions (one row at a time left the kernel at
  // 1.9 TB/s: load, two wave reductions, store, and only then the next row's loads)
  const int stride = gridDim.x * 4;
  for (int row = blockIdx.x * 4 + wave; row < a.rows; row += 2 * stride) {
    floatx4 dy0[NV], xh0[NV], dy1[NV], xh1[NV];
    load_row(row, dy0, xh0);
    load_row(row + stride, dy1, xh1);
    do_row(row, dy0, xh0);
    if (row + stride < a.rows) do_row(row + stride, dy1, xh1);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[0][wave][c + j] = dg[i][j]; red[1][wave][c + j] = db[i][j]; }
  }
  __syncthreads();
  // With scratch: this workgroup's [dgamma | dbeta] partial goes to its own record as plain stores and ln_fold_kernel adds the
  // records in a fixed order - no atomics, no zero-fill, bitwise reproducible.  Without scratch (few rows, C-ABI callers):
  // atomics straight into the gradients.
  float* rec = a.slots != nullptr ? a.slots + (int64_t)blockIdx.x * 2 * H : nullptr;
  for (int c = threadIdx.x; c < H; c += 256) {
    const float g = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c];
    const float b = red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c];
    if (rec != nullptr) { rec[c] = g; rec[H + c] = b; }
    else {
      if (a.dgamma != nullptr) atomicAdd(a.dgamma + c, g);
      if (a.dbeta != nullptr) atomicAdd(a.dbeta + c, b);
    }
  }
}

// bf16 fast path of LayerNorm backward (H % 16 == 0, H <= 1024).  The fused [dgamma | dbeta] accumulators are what costs registers
// here, and registers are what decides how many rows a CU keeps in flight (the 8-byte-per-lane form: 146 VGPRs, 3 waves per SIMD,
// 1.9 TB/s; a half-wave-per-row form with 24 columns per lane: 186 VGPRs, 2.2 TB/s).  This form gives a WAVE one row and a lane two
// 8-column chunks (columns 8l.. and H/2 + 8l..: H / 16 active lanes - 48 of 64 at H = 768; the idle quarter costs nothing on a
// memory-bound kernel): 16-byte accesses, 32 accumulator registers, and the next row's loads are issued before the current row is
// processed (two register sets, statically named), so every wave always has a row in flight.
struct LnRow16 { uint4 dy[2], xh[2]; float rstd; };      // (rstd rides with the row's data loads: loaded after the reductions it was an exposed latency per row)
template <bool DROP>
__global__ void __launch_bounds__(256, 3) ln_bwd16_kernel(LnBwdArgs<bf16_t> a) {
  // LDS: gamma [H] + one [4 waves][H] reduction buffer used twice (dgamma, then dbeta): 15 KB at H = 768.  The footprint matters
  // beyond occupancy: in a training step this kernel runs NEXT TO the grouped weight-gradient GEMM of the side stream, whose two
  // 64 KB workgroups leave 32 KB of a CU's LDS - with a 36 KB footprint these workgroups queued behind it (58 us per call under
  // overlap against 33 alone).
  extern __shared__ float ln_lds[];
  float* gsm = ln_lds;                 // [H]
  float* red = ln_lds + a.H;           // [4][H]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int H = a.H, HH = H >> 1;
  const bool active = lane * 16 < H;
  const int c0 = lane * 8, c1 = HH + lane * 8;
  // Row liveness of every row this wave will visit, fetched ONCE up front (lane k holds the flag of the wave's k-th row): read inside
  // the row loop, the flag byte was a dependent global load in front of every row's data loads - a memory latency per row on a
  // wave that only visits four.  It is also the FIRST load of the kernel, ahead of gamma: the first rows' data loads wait on it, and
  // they are issued before gamma goes to the LDS (gamma -> barrier -> flags -> rows was three memory latencies in a row on a
  // workgroup that lives for about ten).
  const int stride = gridDim.x * 4;
  const int row_first = blockIdx.x * 4 + wave;
  int live_reg = 1;
  if (a.row_live != nullptr) {
    const int64_t rk = (int64_t)row_first + (int64_t)lane * stride;
    live_reg = rk < a.rows ? (int)a.row_live[rk] : 0;
  }
  float gpre[4];                       // H <= 1024: at most four gamma elements per thread
#pragma unroll
  for (int i = 0; i < 4; ++i) { const int c = threadIdx.x + 256 * i; gpre[i] = c < H ? a.gamma[c] : 0.f; }
  float dg[2][8], db[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) { dg[i][j] = 0.f; db[i][j] = 0.f; }
  auto is_live = [&](int row) -> bool {          // wave-uniform
    if (a.row_live == nullptr) return true;
    const int k = (row - row_first) / stride;
    if (k < 64) return __builtin_amdgcn_readlane(live_reg, k) != 0;
    return row < a.rows && a.row_live[row] != 0;
  };
  auto load = [&](int row, LnRow16& r) {
    const bool ok = active && row < a.rows && is_live(row);
    const uint32_t o0 = ((uint32_t)row * (uint32_t)H + (uint32_t)c0) * 2u, o1 = o0 + (uint32_t)H;      // rows * H * 2 < 4 GiB (launcher)
    const uint4 z = uint4{0u, 0u, 0u, 0u};
    r.dy[0] = ok ? *(const uint4*)((const char*)a.dy + o0) : z; r.dy[1] = ok ? *(const uint4*)((const char*)a.dy + o1) : z;
    r.xh[0] = ok ? *(const uint4*)((const char*)a.xhat + o0) : z; r.xh[1] = ok ? *(const uint4*)((const char*)a.xhat + o1) : z;
    r.rstd = ok ? a.rstd[row] : 0.f;
  };
  auto process = [&](int row, LnRow16& r) {
    if (!is_live(row)) {      // a padding row (wave-uniform): dy = 0 -> dx = 0, no dgamma / dbeta term
      if (active) {
        const uint4 z = uint4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const uint32_t off = ((uint32_t)row * (uint32_t)H + (uint32_t)(i ? c1 : c0)) * 2u;
          *(uint4*)((char*)a.dx + off) = z;
          if (a.dx_drop != nullptr) *(uint4*)((char*)a.dx_drop + off) = z;
        }
      }
      return;
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = i ? c1 : c0;
      float dy[8], xh[8], gm[8];
      unpack8(r.dy[i], dy);
      unpack8(r.xh[i], xh);
      *(floatx4*)&gm[0] = *(const floatx4*)&gsm[active ? c : 0]; *(floatx4*)&gm[4] = *(const floatx4*)&gsm[active ? c + 4 : 4];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = dy[j] * gm[j];
        s1 += t;
        s2 += t * xh[j];
        dg[i][j] += dy[j] * xh[j];
        db[i][j] += dy[j];
      }
    }
    s1 = wave_sum(s1) / (float)H;
    s2 = wave_sum(s2) / (float)H;
    if (!active || row >= a.rows) return;
    const float rstd = r.rstd;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = i ? c1 : c0;
      float dy[8], xh[8], gm[8], dx[8];
      unpack8(r.dy[i], dy);
      unpack8(r.xh[i], xh);
      *(floatx4*)&gm[0] = *(const floatx4*)&gsm[c]; *(floatx4*)&gm[4] = *(const floatx4*)&gsm[c + 4];
#pragma unroll
      for (int j = 0; j < 8; ++j) dx[j] = rstd * (dy[j] * gm[j] - s1 - xh[j] * s2);
      const uint32_t off = ((uint32_t)row * (uint32_t)H + (uint32_t)c) * 2u;
      *(uint4*)((char*)a.dx + off) = pack8(dx);
      if (a.dx_drop != nullptr) {
        if constexpr (DROP) {
#pragma unroll
          for (int hq = 0; hq < 2; ++hq) {
            const floatx4 dm = drop_mult4(a.out_drop.seed, a.out_drop.thresh, a.out_drop.scale, (uint32_t)row * (uint32_t)H + (uint32_t)(c + 4 * hq));
#pragma unroll
            for (int j = 0; j < 4; ++j) dx[4 * hq + j] *= dm[j];
          }
        }
        *(uint4*)((char*)a.dx_drop + off) = pack8(dx);
      }
    }
  };
  int row = row_first;
  LnRow16 ra, rb;
  load(row, ra);
#pragma unroll
  for (int i = 0; i < 4; ++i) { const int c = threadIdx.x + 256 * i; if (c < H) gsm[c] = gpre[i]; }
  __syncthreads();
  while (row < a.rows) {
    load(row + stride, rb);
    process(row, ra);
    row += stride;
    if (row >= a.rows) break;
    load(row + stride, ra);
    process(row, rb);
    row += stride;
  }
  float* rec = a.slots != nullptr ? a.slots + (int64_t)blockIdx.x * 2 * H : nullptr;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();                   // (pass 0: the gamma reads of the row loop are done; pass 1: pass 0's sums are read)
    if (active) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = i ? c1 : c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) red[wave * H + c + j] = pass ? db[i][j] : dg[i][j];
      }
    }
    __syncthreads();
    float* out = pass ? a.dbeta : a.dgamma;
    for (int c = threadIdx.x; c < H; c += 256) {
      const float v = red[c] + red[H + c] + red[2 * H + c] + red[3 * H + c];
      if (rec != nullptr) rec[pass * H + c] = v;
      else if (out != nullptr) atomicAdd(out + c, v);
    }
  }
}
// Round 5: the same row arithmetic on a leaner skeleton.  tools/ln_probe.py's block sweep put the FIXED cost of a workgroup of the
// kernel above at ~8 us against ~1.5 us per row: a prologue of three dependent memory latencies (liveness flags -> first rows -> gamma
// through the LDS and a barrier), an epilogue of two LDS passes with four barriers, and per row two wave reductions of six
// ds_bpermute round trips each.  Here
//   * nothing waits before the first row: the flags, gamma (straight into 16 registers per lane - no LDS, no barrier) and the first
//     row's data are requested together (that row is fetched whether or not it is live; the later ones only when live);
//   * a wave keeps FOUR rows in flight (statically named register sets) and walks twice as many rows, so half as many workgroups
//     pay the fixed cost and write records;
//   * the row sums go through DPP (wave_sum_dpp);
//   * the epilogue is ONE barrier: every wave stores its 2 x 16 partial columns as 16-byte LDS writes, 256 threads add the four
//     waves in order and write the record as 16-byte stores.  LDS 32 H bytes (24 KB at H = 768), touched by the epilogue only.
// Same record layout ([dgamma | dbeta] per workgroup), same fold kernels; a wave's rows are summed in row order, the four waves in
// wave order: deterministic, but another order than the kernel above.
typedef __attribute__((ext_vector_type(4))) uint32_t ln_u32x4;
// STORES THE COMPILER DOES NOT TRACK.  hipcc's waitcnt insertion treats vmcnt as out of order as soon as loads and stores are pending
// together (one counter for both on gfx9; a younger store may indeed be acknowledged before an older load) and then waits with
// vmcnt(0): in a row loop that stores row k while rows k+1.. are in flight, EVERY use of a loaded row drained the whole queue - the
// prefetched rows included - which is why the round-3/4 kernel gained nothing from more rows in flight.  With the stores as inline asm
// the compiler sees only loads pending, which complete in issue order: it waits with exact counts (vmcnt(12) before row k = "the
// three younger rows may still be in flight"); the untracked stores can only make such a wait longer, never too short.  (The first
// form of this kernel did it the other way round - asm loads, counted waits by hand - and read garbage: the compiler is free to
// copy or spill a value it believes was defined by the asm statement while the load is still in flight.)  s_nop: the store-data
// hazard of a > 8-byte VMEM store followed by a write of its data registers, which the compiler cannot see through the asm.
__device__ __forceinline__ void ln_store16(ln_u32x4 v, uint32_t voff, uint32_t soff, __amdgpu_buffer_rsrc_t rsrc) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
#endif
}
struct LnRowA { ln_u32x4 dy[2], xh[2]; };

template <bool DROP>
__global__ void __launch_bounds__(256, 1) ln_bwd16v2_kernel(LnBwdArgs<bf16_t> a) {
  // Branch-free row path: every global access of the row loop is a raw buffer access - the row's byte offset in the SCALAR offset
  // operand, the lane's column offset in the vector operand, which is parked beyond the buffer for whatever must not happen (a lane
  // beyond H / 16, a row beyond this wave's last, the loads of a padding row): out-of-range loads return zeros and move no bytes,
  // out-of-range stores are dropped (the range check looks at the vector offset only).  A padding row runs the same arithmetic on
  // zeros (dx = 0 * (0 - 0 - 0) = 0, nothing added to dgamma / dbeta) and stores its zero row: the row loop is straight-line code.
  extern __shared__ float ln_lds[];          // [4 waves][2 H]: epilogue only
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int H = a.H, HH = H >> 1;
  const bool active = lane * 16 < H;
  constexpr uint32_t OOB = 0xFFFFFF00u;
  const uint32_t nbytes = (uint32_t)a.rows * (uint32_t)H * 2u;              // < 4 GiB - 256 (launcher)
  const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_xh = __builtin_amdgcn_make_buffer_rsrc((void*)a.xhat, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_dx = __builtin_amdgcn_make_buffer_rsrc((void*)a.dx, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_dd = __builtin_amdgcn_make_buffer_rsrc((void*)(a.dx_drop != nullptr ? a.dx_drop : a.dx), 0, a.dx_drop != nullptr ? (int)nbytes : 0, 0x00020000);
  const int c0 = active ? lane * 8 : 0, c1 = active ? HH + lane * 8 : 0;
  const uint32_t lo0 = active ? (uint32_t)c0 * 2u : OOB, lo1 = active ? (uint32_t)c1 * 2u : OOB;      // byte offsets inside a row; idle lanes parked
  const int stride = gridDim.x * 4;
  const int row_first = blockIdx.x * 4 + wave;
  const int nrow = row_first < a.rows ? (a.rows - row_first + stride - 1) / stride : 0;      // this wave's rows: row_first + k * stride, k < nrow <= 64
  const uint32_t row_bytes = (uint32_t)H * 2u;
  // (bit-ands, not &&: no short-circuit branches around the loads)
  auto load = [&](int k, LnRowA& r, int fetch) {
    const uint32_t row = (uint32_t)(row_first + k * stride);
    const uint32_t sbase = fetch ? row * row_bytes : 0u;
    const uint32_t v0 = fetch ? lo0 : OOB, v1 = fetch ? lo1 : OOB;
    r.dy[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_dy, v0, sbase, 0);
    r.dy[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_dy, v1, sbase, 0);
    r.xh[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_xh, v0, sbase, 0);
    r.xh[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_xh, v1, sbase, 0);
  };
  LnRowA r0, r1, r2, r3;
  // ---- prologue: the liveness flags (lane k: is the wave's k-th row live; no table: every row), gamma and the FIRST row's data are
  // requested together - one memory latency, not three in a row; that row is fetched whether or not it is live
  int live_reg = 1;
  if (a.row_live != nullptr) live_reg = lane < nrow ? (int)a.row_live[(int64_t)row_first + (int64_t)lane * stride] : 0;
  const float rstd_reg = lane < nrow ? a.rstd[(int64_t)row_first + (int64_t)lane * stride] : 0.f;      // lane k: rstd of the wave's k-th row
  float gm[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = i ? c1 : c0;
    *(floatx4*)&gm[i][0] = *(const floatx4*)(a.gamma + c); *(floatx4*)&gm[i][4] = *(const floatx4*)(a.gamma + c + 4);
  }
  load(0, r0, (int)(nrow > 0));
  const float rstd_keep = rstd_reg;
  auto live_k = [&](int k) -> int { return (int)(k < nrow) & (int)(__builtin_amdgcn_readlane(live_reg, k & 63) != 0); };      // k wave-uniform
  load(1, r1, live_k(1)); load(2, r2, live_k(2)); load(3, r3, live_k(3));
  float dg[2][8], db[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) { dg[i][j] = 0.f; db[i][j] = 0.f; }
  // keep = 0: a padding row (its loads were parked and returned zeros - except the wave's first row, fetched before the flags were known) or a row
  // beyond the wave's last: everything read for it counts as zeros
  auto process = [&](int k, const LnRowA& r, int keep) {
    const int store = (int)(k < nrow);
    const uint32_t row = (uint32_t)(row_first + k * stride);
    const uint32_t msk = keep ? 0xFFFFFFFFu : 0u;
    // (opaque to the loop optimiser: as row * H + c it became eight per-lane induction variables carried - and spilled - across the loop)
    const uint32_t row_h = (uint32_t)__builtin_amdgcn_readfirstlane((int)(row * (uint32_t)H));
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float dy[8], xh[8];
      unpack8(uint4{r.dy[i][0] & msk, r.dy[i][1] & msk, r.dy[i][2] & msk, r.dy[i][3] & msk}, dy);
      unpack8(uint4{r.xh[i][0] & msk, r.xh[i][1] & msk, r.xh[i][2] & msk, r.xh[i][3] & msk}, xh);      // (a stale xhat row may hold anything: 0 * NaN)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = dy[j] * gm[i][j];
        s1 += t;
        s2 += t * xh[j];
        dg[i][j] += dy[j] * xh[j];
        db[i][j] += dy[j];
      }
    }
    s1 = wave_sum_dpp(s1) / (float)H;
    s2 = wave_sum_dpp(s2) / (float)H;
    const float rstd = keep ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rstd_keep), k & 63)) : 0.f;      // (a padding row's saved rstd is as stale as its xhat)
    const uint32_t sbase = store ? row * row_bytes : 0u;
    // (fences: the dropout hashes and the second unpack are not to be hoisted above the reductions - they would all be live across them)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i) __builtin_amdgcn_sched_barrier(0);
      const int c = i ? c1 : c0;
      float dy[8], xh[8], dx[8];
      unpack8(uint4{r.dy[i][0] & msk, r.dy[i][1] & msk, r.dy[i][2] & msk, r.dy[i][3] & msk}, dy);
      unpack8(uint4{r.xh[i][0] & msk, r.xh[i][1] & msk, r.xh[i][2] & msk, r.xh[i][3] & msk}, xh);
#pragma unroll
      for (int j = 0; j < 8; ++j) dx[j] = rstd * (dy[j] * gm[i][j] - s1 - xh[j] * s2);
      const uint32_t voff = store ? (i ? lo1 : lo0) : OOB;
      ln_store16(__builtin_bit_cast(ln_u32x4, pack8(dx)), voff, sbase, rs_dx);
      if constexpr (DROP) {
#pragma unroll
        for (int hq = 0; hq < 2; ++hq) {
          const floatx4 dm = drop_mult4_nz(a.out_drop.seed, a.out_drop.thresh, a.out_drop.scale, row_h + (uint32_t)(c + 4 * hq));
#pragma unroll
          for (int j = 0; j < 4; ++j) dx[4 * hq + j] *= dm[j];
        }
      }
      ln_store16(__builtin_bit_cast(ln_u32x4, pack8(dx)), voff, sbase, rs_dd);      // (no dx_drop: a zero-size buffer drops it)
    }
  };
  // Row k is processed, then row k + 4 requested into its registers: four rows of a wave in flight.  The waits are the compiler's (exact
  // counts: only loads are pending as far as it knows).  sched_barrier: it must not interleave four rows' arithmetic (> 256 registers).
#define RL_LN_STEP(K, R, KEEP) do { __builtin_amdgcn_sched_barrier(0); process(K, R, KEEP); __builtin_amdgcn_sched_barrier(0); \
    load((K) + 4, R, live_k((K) + 4)); __builtin_amdgcn_sched_barrier(0); } while (0)
  for (int k = 0; k < nrow; k += 4) {
    RL_LN_STEP(k, r0, live_k(k));
    RL_LN_STEP(k + 1, r1, live_k(k + 1));
    RL_LN_STEP(k + 2, r2, live_k(k + 2));
    RL_LN_STEP(k + 3, r3, live_k(k + 3));
  }
#undef RL_LN_STEP
  // ---- epilogue: [dgamma | dbeta] of the workgroup = the four waves' partials added in wave order
  float* mine = ln_lds + (size_t)wave * 2 * H;
  if (active) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = i ? c1 : c0;
      *(floatx4*)(mine + c) = *(const floatx4*)&dg[i][0]; *(floatx4*)(mine + c + 4) = *(const floatx4*)&dg[i][4];
      *(floatx4*)(mine + H + c) = *(const floatx4*)&db[i][0]; *(floatx4*)(mine + H + c + 4) = *(const floatx4*)&db[i][4];
    }
  }
  __syncthreads();
  float* rec = a.slots != nullptr ? a.slots + (int64_t)blockIdx.x * 2 * H : nullptr;
  for (int q = threadIdx.x; q < 2 * H / 4; q += 256) {
    const floatx4 v = ((*(const floatx4*)(ln_lds + 4 * q) + *(const floatx4*)(ln_lds + 2 * H + 4 * q)) + *(const floatx4*)(ln_lds + 4 * H + 4 * q)) +
                      *(const floatx4*)(ln_lds + 6 * H + 4 * q);
    if (rec != nullptr) *(floatx4*)(rec + 4 * q) = v;
    else {
      float* out = 4 * q < H ? a.dgamma : a.dbeta;
      const int c = 4 * q < H ? 4 * q : 4 * q - H;
      if (out != nullptr) {
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(out + c + j, v[j]);
      }
    }
  }
}
// dgamma / dbeta += sum of the per-workgroup records: one float4 column group per 64 threads (record lanes k, k + 64, ...),
// four groups per block, fixed-order LDS tree.
__global__ void __launch_bounds__(256) ln_fold_kernel(const float* __restrict__ recs, int nrec, int H, float* dgamma, float* dbeta) {
  __shared__ floatx4 red[4][64];
  const int q = threadIdx.x >> 6, kl = threadIdx.x & 63;
  const int i = (blockIdx.x * 4 + q) * 4;                  // column in [0, 2H)
  floatx4 s = floatx4{0.f, 0.f, 0.f, 0.f};
  if (i < 2 * H)
    for (int k = kl; k < nrec; k += 64) s += *(const floatx4*)(recs + (int64_t)k * 2 * H + i);
  red[q][kl] = s;
  __syncthreads();
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    if (kl < w) red[q][kl] += red[q][kl + w];
    __syncthreads();
  }
  if (kl == 0 && i < 2 * H) {
    float* o = i < H ? dgamma + i : dbeta + (i - H);
    *(floatx4*)o += red[q][0];
  }
}
__global__ void __launch_bounds__(256) ln_fold_multi_kernel(LnFoldSites f) {
  __shared__ floatx4 red[4][64];
  const LnFoldSite site = f.s[blockIdx.y];
  const int H = f.H;
  const int q = threadIdx.x >> 6, kl = threadIdx.x & 63;
  const int i = (blockIdx.x * 4 + q) * 4;                  // column in [0, 2H)
  floatx4 s = floatx4{0.f, 0.f, 0.f, 0.f};
  if (i < 2 * H)
    for (int k = kl; k < site.nrec; k += 64) s += *(const floatx4*)(site.recs + (int64_t)k * 2 * H + i);
  red[q][kl] = s;
  __syncthreads();
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    if (kl < w) red[q][kl] += red[q][kl + w];
    __syncthreads();
  }
  if (kl == 0 && i < 2 * H) {
    float* o = i < H ? site.dgamma + i : site.dbeta + (i - H);
    *(floatx4*)o += red[q][0];
  }
}
int ln_fold_multi(hipStream_t st, const LnFoldSites& sites) {
  if (sites.n <= 0) return RL_OK;
  if (sites.n > LN_FOLD_MAX || (sites.H & 3)) return RL_ERR_ARG;
  hipLaunchKernelGGL(ln_fold_multi_kernel, dim3((2 * sites.H / 4 + 3) / 4, sites.n), dim3(256), 0, st, sites);
  return RL_LAUNCH_CHECK();
}

template <typename T> int ln_bwd(hipStream_t st, const LnBwdArgs<T>& a) {
  if (a.rows <= 0) return RL_OK;
  if ((a.H & 3) || a.H > LN_MAXV * 256) return RL_ERR_ARG;
  int blocks = (a.rows + 3) / 4;
  const int cap = a.H <= 512 ? 1024 : 768;   // resident workgroups: 4 (<= 110 VGPRs) or 3 (146 VGPRs with two rows in flight) waves per SIMD x 256 CUs
  if (blocks > cap) blocks = cap;
  LnBwdArgs<T> b = a;
  // records only from more than 96 workgroups that owe both gradients (else atomics); called again wherever a path settles on another `blocks`
  auto pick_slots = [&] { b.slots = (blocks <= 96 || a.dgamma == nullptr || a.dbeta == nullptr) ? nullptr : a.slots; };
  // the tail behind whichever row kernel was launched: the record count goes to the caller (deferred_records), or the records are folded here
  auto finish = [&]() -> int {
    if (a.deferred_records != nullptr) *a.deferred_records = b.slots != nullptr ? blocks : 0;
    else if (b.slots != nullptr) hipLaunchKernelGGL(ln_fold_kernel, dim3((2 * a.H / 4 + 3) / 4), dim3(256), 0, st, b.slots, blocks, a.H, a.dgamma, a.dbeta);
    return RL_LAUNCH_CHECK();
  };
  pick_slots();
  const int nv = (a.H + 255) / 256;
  if constexpr (sizeof(T) == 2) {
    if (g_ln_fast && a.in_drop.thresh == 0u && (a.H % 16) == 0 && a.H <= 1024 && ((int64_t)a.rows + 8192) * a.H * 2 < (1ll << 32) - 4096) {     // (the embedding LayerNorm, whose input gradient is dropout-masked first, keeps the general kernel)
      const int groups = (a.rows + 3) / 4;
      if (g_ln_v2) {
        blocks = groups < g_ln_bwd_blocks_v2 ? groups : g_ln_bwd_blocks_v2;
        if (blocks * 256 < a.rows) blocks = (a.rows + 255) / 256;       // a wave's rows must fit its 64 liveness lanes
        pick_slots();
        if (b.slots != nullptr && blocks > 1024) return RL_ERR_ARG;     // (LN_SLOT_FLOATS holds 1024 records)
        const size_t lds2 = (size_t)8 * a.H * sizeof(float);
        if (a.out_drop.thresh != 0u) hipLaunchKernelGGL((ln_bwd16v2_kernel<true>), dim3(blocks), dim3(256), lds2, st, b);
        else hipLaunchKernelGGL((ln_bwd16v2_kernel<false>), dim3(blocks), dim3(256), lds2, st, b);
        return finish();
      }
      blocks = groups < g_ln_bwd_blocks ? groups : g_ln_bwd_blocks;
      pick_slots();
      const size_t lds = (size_t)5 * a.H * sizeof(float);
      if (a.out_drop.thresh != 0u) hipLaunchKernelGGL((ln_bwd16_kernel<true>), dim3(blocks), dim3(256), lds, st, b);
      else hipLaunchKernelGGL((ln_bwd16_kernel<false>), dim3(blocks), dim3(256), lds, st, b);
      return finish();
    }
  }
  if (nv == 1) hipLaunchKernelGGL((ln_bwd_kernel<T, 1>), dim3(blocks), dim3(256), 0, st, b);
  else if (nv == 2) hipLaunchKernelGGL((ln_bwd_kernel<T, 2>), dim3(blocks), dim3(256), 0, st, b);
  else if (nv == 3) hipLaunchKernelGGL((ln_bwd_kernel<T, 3>), dim3(blocks), dim3(256), 0, st, b);
  else hipLaunchKernelGGL((ln_bwd_kernel<T, 4>), dim3(blocks), dim3(256), 0, st, b);
  return finish();
}
template int ln_bwd<bf16_t>(hipStream_t, const LnBwdArgs<bf16_t>&);
template int ln_bwd<float>(hipStream_t, const LnBwdArgs<float>&);

// ---------------------------------------------------------------------------------------------
// LayerNorm backward fused with the erf-GELU backward (BertPredictionHeadTransform, modeling_bert.py:419-431): between the decoder's
// data gradient and the transform's weight gradient there is no GEMM to carry an epilogue, so the two element-wise backwards are one
// row pass:  g = dy * gamma;  da = rstd (g - mean(g) - xhat mean(g xhat));  dz = da * gelu'(z);  dgamma += dy xhat;  dbeta += dy.
// Generic form (fp32 parity mode, any H % 4 == 0 up to 1024): a wave per row, grid-stride.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int lng_rows(const int rows, const int* n_dev) {
  if (n_dev == nullptr) return rows;
  const int n = *n_dev;
  return n < 0 ? 0 : (n < rows ? n : rows);
}
template <typename T, int NV>
__global__ void __launch_bounds__(256) ln_gelu_bwd_kernel(LnGeluBwdArgs<T> a) {
  __shared__ float red[2][4][NV * 256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int H = a.H;
  const int n = lng_rows(a.rows, a.n_dev);
  floatx4 dg[NV], db[NV], gm[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    dg[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    db[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    const int c = (i * 64 + lane) * 4;
    gm[i] = c < H ? *(const floatx4*)(a.gamma + c) : floatx4{0.f, 0.f, 0.f, 0.f};
  }
  for (int row = blockIdx.x * 4 + wave; row < n; row += gridDim.x * 4) {
    int srow = a.idx != nullptr ? a.idx[row] : row;
    srow = srow < 0 ? 0 : (srow >= a.saved_rows ? a.saved_rows - 1 : srow);
    floatx4 dy[NV], xh[NV], z[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      dy[i] = xh[i] = z[i] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (c < H) {
        dy[i] = load4<T>(a.dy + (int64_t)row * H + c);
        xh[i] = load4<T>(a.xhat + (int64_t)srow * H + c);
        z[i] = load4<T>(a.z + (int64_t)srow * H + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float t = dy[i][j] * gm[i][j];
          s1 += t;
          s2 += t * xh[i][j];
          dg[i][j] += dy[i][j] * xh[i][j];
          db[i][j] += dy[i][j];
        }
      }
    }
    s1 = wave_sum(s1) / (float)H;
    s2 = wave_sum(s2) / (float)H;
    const float rstd = a.rstd[srow];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        floatx4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = rstd * (dy[i][j] * gm[i][j] - s1 - xh[i][j] * s2) * gelu_bwd<T>(z[i][j]);
        store4<T>(a.dz + (int64_t)row * H + c, o);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[0][wave][c + j] = dg[i][j]; red[1][wave][c + j] = db[i][j]; }
  }
  __syncthreads();
  float* rec = a.slots != nullptr ? a.slots + (int64_t)blockIdx.x * 2 * H : nullptr;      // (a workgroup without rows writes a zero record: the fold adds them all)
  for (int c = threadIdx.x; c < H; c += 256) {
    const float g = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c];
    const float b = red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c];
    if (rec != nullptr) { rec[c] = g; rec[H + c] = b; }
    else if (n > 0) {
      if (a.dgamma != nullptr) atomicAdd(a.dgamma + c, g);
      if (a.dbeta != nullptr) atomicAdd(a.dbeta + c, b);
    }
  }
}
// bf16 fast path (H % 16 == 0, H <= 1024): ln_bwd16v2_kernel's skeleton with one more stream.  A wave owns rows row_first + k *
// stride (k < nrow <= 64), a lane two 8-column chunks (16-byte accesses), four rows of a wave are in flight in statically named
// register sets - row k + 4 is requested right after row k is processed -, every access of the row loop is a raw buffer access whose
// vector offset is parked beyond the buffer for what must not happen (an idle lane, a row beyond the wave's last: loads return
// zeros, stores are dropped), the dz stores are ln_store16 (inline asm: the compiler sees only loads pending and waits with exact
// counts), row sums through DPP, [dgamma | dbeta] as one record per workgroup through one LDS barrier.  What is new:
//   * z, the saved dense pre-activation, rides with xhat (6 instead of 4 16-byte loads per lane and row), and the GELU derivative
//     Phi(z) + z phi(z) multiplies the LayerNorm gradient in registers before the one store;
//   * the saved tensors may be addressed through a row index (the compacted classifier gradient of a dense forward): lane k holds
//     the saved row of the wave's k-th row and its rstd, fetched once in the prologue; the row's scalar offset comes from a readlane;
//   * the row count may live on the device (the rows that enter the loss): a wave's nrow follows it, workgroups beyond it only
//     write their zero record.
struct LnGRow { ln_u32x4 dy[2], xh[2], z[2]; };
__global__ void __launch_bounds__(256, 1) ln_gelu_bwd16_kernel(LnGeluBwdArgs<bf16_t> a) {
  extern __shared__ float ln_lds[];          // [4 waves][2 H]: epilogue only
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int H = a.H, HH = H >> 1;
  const bool active = lane * 16 < H;
  constexpr uint32_t OOB = 0xFFFFFF00u;
  const int n = lng_rows(a.rows, a.n_dev);
  const uint32_t nbytes = (uint32_t)a.rows * (uint32_t)H * 2u, sbytes = (uint32_t)a.saved_rows * (uint32_t)H * 2u;      // < 4 GiB - 256 (launcher)
  const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_dz = __builtin_amdgcn_make_buffer_rsrc((void*)a.dz, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_xh = __builtin_amdgcn_make_buffer_rsrc((void*)a.xhat, 0, (int)sbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_z = __builtin_amdgcn_make_buffer_rsrc((void*)a.z, 0, (int)sbytes, 0x00020000);
  const int c0 = active ? lane * 8 : 0, c1 = active ? HH + lane * 8 : 0;
  const uint32_t lo0 = active ? (uint32_t)c0 * 2u : OOB, lo1 = active ? (uint32_t)c1 * 2u : OOB;
  const int stride = gridDim.x * 4;
  const int row_first = blockIdx.x * 4 + wave;
  const int nrow = row_first < n ? (n - row_first + stride - 1) / stride : 0;      // <= 64 (launcher)
  const uint32_t row_bytes = (uint32_t)H * 2u;
  // ---- prologue: lane k = the saved row of the wave's k-th row and its rstd; gamma into registers
  int srow_reg = 0;
  float rstd_reg = 0.f;
  if (lane < nrow) {
    const int r = row_first + lane * stride;
    int s = a.idx != nullptr ? a.idx[r] : r;
    s = s < 0 ? 0 : (s >= a.saved_rows ? a.saved_rows - 1 : s);      // (a bad index must not leave the saved tensors: the scalar offset is not range-checked)
    srow_reg = s;
    rstd_reg = a.rstd[s];
  }
  float gm[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = i ? c1 : c0;
    *(floatx4*)&gm[i][0] = *(const floatx4*)(a.gamma + c); *(floatx4*)&gm[i][4] = *(const floatx4*)(a.gamma + c + 4);
  }
  const int srow_keep = srow_reg;
  const float rstd_keep = rstd_reg;
  // (bit-ands and selects, no short-circuit branches around the loads)
  auto load = [&](int k, LnGRow& r) {
    const int fetch = (int)(k < nrow);
    const uint32_t row = (uint32_t)(row_first + k * stride);
    const uint32_t srow = (uint32_t)__builtin_amdgcn_readlane(srow_keep, k & 63);
    const uint32_t sb = fetch ? row * row_bytes : 0u, ss = fetch ? srow * row_bytes : 0u;
    const uint32_t v0 = fetch ? lo0 : OOB, v1 = fetch ? lo1 : OOB;
    r.dy[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_dy, v0, sb, 0);
    r.dy[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_dy, v1, sb, 0);
    r.xh[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_xh, v0, ss, 0);
    r.xh[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_xh, v1, ss, 0);
    r.z[0] = __builtin_amdgcn_raw_buffer_load_b128(rs_z, v0, ss, 0);
    r.z[1] = __builtin_amdgcn_raw_buffer_load_b128(rs_z, v1, ss, 0);
  };
  LnGRow r0, r1, r2, r3;
  load(0, r0); load(1, r1); load(2, r2); load(3, r3);
  float dg[2][8], db[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) { dg[i][j] = 0.f; db[i][j] = 0.f; }
  // a row beyond the wave's last: its loads were parked and returned zeros - it adds nothing and its store is parked too
  auto process = [&](int k, const LnGRow& r) {
    const int store = (int)(k < nrow);
    const uint32_t row = (uint32_t)(row_first + k * stride);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float dy[8], xh[8];
      unpack8(uint4{r.dy[i][0], r.dy[i][1], r.dy[i][2], r.dy[i][3]}, dy);
      unpack8(uint4{r.xh[i][0], r.xh[i][1], r.xh[i][2], r.xh[i][3]}, xh);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = dy[j] * gm[i][j];
        s1 += t;
        s2 += t * xh[j];
        dg[i][j] += dy[j] * xh[j];
        db[i][j] += dy[j];
      }
    }
    s1 = wave_sum_dpp(s1) / (float)H;
    s2 = wave_sum_dpp(s2) / (float)H;
    const float rstd = store ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rstd_keep), k & 63)) : 0.f;
    const uint32_t sbase = store ? row * row_bytes : 0u;
    __builtin_amdgcn_sched_barrier(0);      // (the second unpack and the GELU terms are not to be hoisted above the reductions)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i) __builtin_amdgcn_sched_barrier(0);
      float dy[8], xh[8], z[8], o[8];
      unpack8(uint4{r.dy[i][0], r.dy[i][1], r.dy[i][2], r.dy[i][3]}, dy);
      unpack8(uint4{r.xh[i][0], r.xh[i][1], r.xh[i][2], r.xh[i][3]}, xh);
      unpack8(uint4{r.z[i][0], r.z[i][1], r.z[i][2], r.z[i][3]}, z);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = rstd * (dy[j] * gm[i][j] - s1 - xh[j] * s2) * gelu_bwd<bf16_t>(z[j]);
      ln_store16(__builtin_bit_cast(ln_u32x4, pack8(o)), store ? (i ? lo1 : lo0) : OOB, sbase, rs_dz);
    }
  };
#define RL_LNG_STEP(K, R) do { __builtin_amdgcn_sched_barrier(0); process(K, R); __builtin_amdgcn_sched_barrier(0); \
    load((K) + 4, R); __builtin_amdgcn_sched_barrier(0); } while (0)
  for (int k = 0; k < nrow; k += 4) {
    RL_LNG_STEP(k, r0);
    RL_LNG_STEP(k + 1, r1);
    RL_LNG_STEP(k + 2, r2);
    RL_LNG_STEP(k + 3, r3);
  }
#undef RL_LNG_STEP
  // ---- epilogue: [dgamma | dbeta] of the workgroup = the four waves' partials added in wave order
  float* mine = ln_lds + (size_t)wave * 2 * H;
  if (active) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = i ? c1 : c0;
      *(floatx4*)(mine + c) = *(const floatx4*)&dg[i][0]; *(floatx4*)(mine + c + 4) = *(const floatx4*)&dg[i][4];
      *(floatx4*)(mine + H + c) = *(const floatx4*)&db[i][0]; *(floatx4*)(mine + H + c + 4) = *(const floatx4*)&db[i][4];
    }
  }
  __syncthreads();
  float* rec = a.slots != nullptr ? a.slots + (int64_t)blockIdx.x * 2 * H : nullptr;
  if (rec == nullptr && blockIdx.x * 4 >= n) return;      // (no rows and no record to write; workgroup-uniform)
  for (int q = threadIdx.x; q < 2 * H / 4; q += 256) {
    const floatx4 v = ((*(const floatx4*)(ln_lds + 4 * q) + *(const floatx4*)(ln_lds + 2 * H + 4 * q)) + *(const floatx4*)(ln_lds + 4 * H + 4 * q)) +
                      *(const floatx4*)(ln_lds + 6 * H + 4 * q);
    if (rec != nullptr) *(floatx4*)(rec + 4 * q) = v;
    else {
      float* out = 4 * q < H ? a.dgamma : a.dbeta;
      const int c = 4 * q < H ? 4 * q : 4 * q - H;
      if (out != nullptr) {
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(out + c + j, v[j]);
      }
    }
  }
}
template <typename T> int ln_gelu_bwd(hipStream_t st, const LnGeluBwdArgs<T>& a) {
  if (a.rows <= 0) return RL_OK;
  if ((a.H & 3) || a.H > LN_MAXV * 256) return RL_ERR_ARG;      // the shapes ln_bwd refuses
  if (!a.dy || !a.xhat || !a.rstd || !a.z || !a.gamma || !a.dz) return RL_ERR_ARG;
  LnGeluBwdArgs<T> b = a;
  if (b.saved_rows <= 0) b.saved_rows = a.rows;
  if (a.idx == nullptr && b.saved_rows < a.rows) return RL_ERR_ARG;
  int blocks = (a.rows + 3) / 4;
  if constexpr (sizeof(T) == 2) {
    const int64_t most = a.rows > b.saved_rows ? a.rows : b.saved_rows;
    if (g_ln_fast && (a.H % 16) == 0 && (most + 8192) * a.H * 2 < (1ll << 32) - 4096) {
      blocks = blocks < g_ln_bwd_blocks_v2 ? blocks : g_ln_bwd_blocks_v2;
      if (blocks * 256 < a.rows) blocks = (a.rows + 255) / 256;       // a wave's rows must fit its 64 index lanes
      if (blocks <= 96 || a.dgamma == nullptr || a.dbeta == nullptr) b.slots = nullptr;
      if (b.slots != nullptr && blocks > 1024) return RL_ERR_ARG;     // (LN_SLOT_FLOATS holds 1024 records)
      hipLaunchKernelGGL(ln_gelu_bwd16_kernel, dim3(blocks), dim3(256), (size_t)8 * a.H * sizeof(float), st, b);
      if (b.slots != nullptr) hipLaunchKernelGGL(ln_fold_kernel, dim3((2 * a.H / 4 + 3) / 4), dim3(256), 0, st, b.slots, blocks, a.H, a.dgamma, a.dbeta);
      return RL_LAUNCH_CHECK();
    }
  }
  const int cap = a.H <= 512 ? 1024 : 768;
  if (blocks > cap) blocks = cap;
  if (blocks <= 96 || a.dgamma == nullptr || a.dbeta == nullptr) b.slots = nullptr;
  const int nv = (a.H + 255) / 256;
  if (nv == 1) hipLaunchKernelGGL((ln_gelu_bwd_kernel<T, 1>), dim3(blocks), dim3(256), 0, st, b);
  else if (nv == 2) hipLaunchKernelGGL((ln_gelu_bwd_kernel<T, 2>), dim3(blocks), dim3(256), 0, st, b);
  else if (nv == 3) hipLaunchKernelGGL((ln_gelu_bwd_kernel<T, 3>), dim3(blocks), dim3(256), 0, st, b);
  else hipLaunchKernelGGL((ln_gelu_bwd_kernel<T, 4>), dim3(blocks), dim3(256), 0, st, b);
  if (b.slots != nullptr) hipLaunchKernelGGL(ln_fold_kernel, dim3((2 * a.H / 4 + 3) / 4), dim3(256), 0, st, b.slots, blocks, a.H, a.dgamma, a.dbeta);
  return RL_LAUNCH_CHECK();
}
template int ln_gelu_bwd<bf16_t>(hipStream_t, const LnGeluBwdArgs<bf16_t>&);
template int ln_gelu_bwd<float>(hipStream_t, const LnGeluBwdArgs<float>&);

}  // namespace rl
