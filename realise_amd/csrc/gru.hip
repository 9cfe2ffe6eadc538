// Pinyin GRU (K6; the "pinyin GRU" section of ops.h): the gate math of one step forward and backward, the device-side pinyin batch
// (pho_prepare) with the token-id range check in front of it (sanitize_ids), and the [33][3H] input-projection table forward and
// backward.
#include "ops.h"
#include "launch.h"

namespace rl {

// ---------------------------------------------------------------------------------------------
// GRU (models.py:661-669, 818-826).  The input projection only ever sees 33 distinct embedding
// rows, so W_ih x + b_ih is a [33][3H] table computed once per forward (fp32, from the masters).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void gru_step_fwd_kernel(GruStepArgs<T> a) {    // grid (H/4/64, n_alive)
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int i = blockIdx.y;
  if (c >= a.H) return;
  if (a.n_alive_dev != nullptr && i >= *a.n_alive_dev) return;
  const int H = a.H;
  const int tok = a.perm[i];
  const int64_t v = a.pho_idx[(int64_t)tok * a.Tp + a.t];
  const float* gi = a.table + v * 3 * H + c;
  const floatx4 ir = *(const floatx4*)gi, iz = *(const floatx4*)(gi + H), in = *(const floatx4*)(gi + 2 * H);
  floatx4 hr, hz, hn, hp;
  if (a.gh != nullptr) {
    const T* gh = a.gh + (int64_t)i * 3 * H + c;
    hr = load4<T>(gh); hz = load4<T>(gh + H); hn = load4<T>(gh + 2 * H);
    hp = load4<T>(a.h_prev + (int64_t)i * H + c);
  } else {
    hr = *(const floatx4*)(a.b_hh + c); hz = *(const floatx4*)(a.b_hh + H + c); hn = *(const floatx4*)(a.b_hh + 2 * H + c);
    hp = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  floatx4 r, z, n, h;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float rj, zj, nj, hj;
    gru_unit<T>(ir[j], iz[j], in[j], hr[j], hz[j], hn[j], hp[j], rj, zj, nj, hj);
    r[j] = rj; z[j] = zj; n[j] = nj; h[j] = hj;
  }
  if (a.rzn != nullptr) {
    T* s = a.rzn + (int64_t)i * 3 * H + c;
    store4<T>(s, r); store4<T>(s + H, z); store4<T>(s + 2 * H, n);
  }
  store4<T>(a.h_new + (int64_t)i * H + c, h);
  if (a.lens[i] == a.t + 1) store4<T>(a.out + (int64_t)tok * H + c, h);
}
template <typename T> int gru_step_fwd(hipStream_t st, const GruStepArgs<T>& a) {
  if (a.n_alive <= 0) return RL_OK;
  if (a.H & 3) return RL_ERR_ARG;
  hipLaunchKernelGGL((gru_step_fwd_kernel<T>), dim3((a.H / 4 + 63) / 64, a.n_alive), dim3(64), 0, st, a);
  return RL_LAUNCH_CHECK();
}
// ---- device-side pinyin batch ----------------------------------------------------------------------------------------
// One 1024-thread workgroup: each thread owns a contiguous run of tokens (so ranks inside a length class follow the token
// order = a STABLE sort, like the host's argsort(-lens, kind="stable")); one block-wide exclusive scan per length class.
__global__ void __launch_bounds__(1024) pho_prepare_kernel(const int64_t* __restrict__ src, int T_, const int64_t* __restrict__ table,
                                                            const int32_t* __restrict__ vlens, int V, int Tw, int64_t* __restrict__ pho_idx,
                                                            int32_t* __restrict__ perm, int32_t* __restrict__ lens_sorted,
                                                            int32_t* __restrict__ n_alive) {
  __shared__ int wave_tot[16];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int per = (T_ + 1023) / 1024;
  const int t0 = min(T_, tid * per), t1 = min(T_, t0 + per);
  auto len_of = [&](int t) {
    const int64_t v = src[t];
    const int l = (v >= 0 && v < V) ? vlens[v] : 1;
    return min(max(l, 1), Tw);
  };
  // (the per-vocabulary rows are gathered by pho_gather_kernel, one thread per symbol: this workgroup only sorts)
  constexpr int CACHE = 16;                               // lengths of the thread's run, read once (T_ <= 16384; longer runs re-read)
  int myl[CACHE];
#pragma unroll
  for (int k = 0; k < CACHE; ++k) myl[k] = (per <= CACHE && t0 + k < t1) ? len_of(t0 + k) : 0;
  auto len_at = [&](int t) {
    if (per > CACHE) return len_of(t);
    int l = 0;
#pragma unroll
    for (int k = 0; k < CACHE; ++k) if (k == t - t0) l = myl[k];
    return l;
  };
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int L = Tw; L >= 1; --L) {                         // longest first
    int c = 0;
    for (int t = t0; t < t1; ++t) c += len_at(t) == L;
    int incl = c;                                         // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < 16; ++w) { const int x = wave_tot[w]; if (w < wv) before += x; total += x; }
    const int base = base_s;
    int pos = base + before + incl - c;
    for (int t = t0; t < t1; ++t)
      if (len_at(t) == L) { perm[pos] = t; lens_sorted[pos] = L; ++pos; }
    __syncthreads();
    if (tid == 0) {
      base_s = base + total;
      n_alive[L - 1] = base + total;                      // #{len > L - 1} = #{len >= L}
    }
    __syncthreads();
  }
}
__global__ void __launch_bounds__(256) pho_gather_kernel(const int64_t* __restrict__ src, int T_, const int64_t* __restrict__ table, int V, int Tw,
                                                         int64_t* __restrict__ pho_idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)T_ * Tw) return;
  const int t = (int)(i / Tw), k = (int)(i - (int64_t)t * Tw);
  const int64_t v = src[t];
  pho_idx[i] = (v >= 0 && v < V) ? table[v * Tw + k] : (k == 0 ? 32 : 0);
}
// Token-id range check (nn.Embedding raises on an id outside its table, modeling_bert.py:183-186; models.py:818,831): the engine
// reads CLEAN copies - ids clamped into [0, V) so that nothing downstream can index past a table - and a sticky flag (device- or
// host-mapped int) records that a bad id was seen; the module raises IndexError when it reads the flag.
__global__ void sanitize_ids_kernel(const int64_t* __restrict__ ids, int64_t n, int V, int64_t* __restrict__ out, int* flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = ids[i];
  const bool bad = v < 0 || v >= V;
  out[i] = bad ? 0 : v;
  if (bad && flag != nullptr) *flag = 1;
}
int sanitize_ids(hipStream_t st, const int64_t* ids, int64_t n, int V, int64_t* out, int* flag) {
  if (n <= 0) return RL_OK;
  hipLaunchKernelGGL(sanitize_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ids, n, V, out, flag);
  return hipGetLastError() == hipSuccess ? RL_OK : RL_ERR_LAUNCH;
}
int pho_prepare(hipStream_t st, const int64_t* src, int T_, const int64_t* table, const int32_t* vlens, int V, int Tw,
                int64_t* pho_idx, int32_t* perm, int32_t* lens_sorted, int32_t* n_alive) {
  if (T_ <= 0) return RL_OK;
  if (Tw < 1 || Tw > 16 || V < 1) return RL_ERR_ARG;
  hipLaunchKernelGGL(pho_gather_kernel, dim3((unsigned)(((int64_t)T_ * Tw + 255) / 256)), dim3(256), 0, st, src, T_, table, V, Tw, pho_idx);
  hipLaunchKernelGGL(pho_prepare_kernel, dim3(1), dim3(1024), 0, st, src, T_, table, vlens, V, Tw, pho_idx, perm, lens_sorted, n_alive);
  return RL_LAUNCH_CHECK();
}
template int gru_step_fwd<bf16_t>(hipStream_t, const GruStepArgs<bf16_t>&);
template int gru_step_fwd<float>(hipStream_t, const GruStepArgs<float>&);

// one BPTT step: consumes dL/dh_t (dh, or dout where the sequence ended at t), emits dGi, dGh,
// the one-hot of the input letter (for the table gradient GEMM) and dh * z into dh.
template <typename T>
__global__ void gru_step_bwd_kernel(GruStepArgs<T> a) {    // grid (H/4/64, n_alive)
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int i = blockIdx.y;
  if (c >= a.H) return;
  if (a.n_alive_dev != nullptr && i >= *a.n_alive_dev) return;
  const int H = a.H;
  const int tok = a.perm[i];
  const bool ends_here = a.lens[i] == a.t + 1;
  const floatx4 dh = ends_here ? load4<T>(a.dout + (int64_t)tok * H + c) : load4<T>(a.dh + (int64_t)i * H + c);
  const T* s = a.rzn + (int64_t)i * 3 * H + c;
  const floatx4 r = load4<T>(s), z = load4<T>(s + H), n = load4<T>(s + 2 * H);
  floatx4 hn, hp;
  if (a.gh != nullptr) {
    hn = load4<T>(a.gh + (int64_t)i * 3 * H + 2 * H + c);
    hp = load4<T>(a.h_prev + (int64_t)i * H + c);
  } else {
    hn = *(const floatx4*)(a.b_hh + 2 * H + c);
    hp = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  floatx4 dar, daz, dan, dhn, dhp;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float dn = dh[j] * (1.0f - z[j]);
    const float dz = dh[j] * (hp[j] - n[j]);
    dan[j] = dn * (1.0f - n[j] * n[j]);
    dar[j] = dan[j] * hn[j] * r[j] * (1.0f - r[j]);
    daz[j] = dz * z[j] * (1.0f - z[j]);
    dhn[j] = dan[j] * r[j];
    dhp[j] = dh[j] * z[j];
  }
  T* gi = a.dgi + (int64_t)i * 3 * H + c;
  store4<T>(gi, dar); store4<T>(gi + H, daz); store4<T>(gi + 2 * H, dan);
  T* gh = a.dgh + (int64_t)i * 3 * H + c;
  store4<T>(gh, dar); store4<T>(gh + H, daz); store4<T>(gh + 2 * H, dhn);
  store4<T>(a.dh + (int64_t)i * H + c, dhp);
  if (c < 64) {
    const int v = (int)a.pho_idx[(int64_t)tok * a.Tp + a.t];
    floatx4 oh;
#pragma unroll
    for (int j = 0; j < 4; ++j) oh[j] = (c + j) == v ? 1.0f : 0.0f;
    store4<T>(a.onehot + (int64_t)i * 64 + c, oh);
  }
}
template <typename T> int gru_step_bwd(hipStream_t st, const GruStepArgs<T>& a) {
  if (a.n_alive <= 0) return RL_OK;
  if ((a.H & 3) || a.H < 64) return RL_ERR_ARG;
  hipLaunchKernelGGL((gru_step_bwd_kernel<T>), dim3((a.H / 4 + 63) / 64, a.n_alive), dim3(64), 0, st, a);
  return RL_LAUNCH_CHECK();
}
template int gru_step_bwd<bf16_t>(hipStream_t, const GruStepArgs<bf16_t>&);
template int gru_step_bwd<float>(hipStream_t, const GruStepArgs<float>&);

// The pinyin alphabet has 33 symbols, so the GRU's input projection W_ih x + b_ih is a [V <= 64][3H] table (models.py:818-826).
// Forward, speed mode: one wave per output unit j keeps W_ih[j, :] in registers (H / 64 values per lane), and accumulates the V dot
// products with the embedding rows (L1-resident, 100 KB) - W_ih is read once, 7 MB; the general MFMA GEMM ran the 33-row problem as
// 18 workgroups of 128 x 128 tiles (56 us).
template <int NK>
__global__ void __launch_bounds__(256) gru_table_fwd_kernel(const float* __restrict__ emb, const float* __restrict__ w_ih, const float* __restrict__ b_ih,
                                                            int V, int H, int J, float* __restrict__ table) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + wave;
  if (j >= J) return;
  float w[NK];
#pragma unroll
  for (int i = 0; i < NK; ++i) { const int k = i * 64 + lane; w[i] = k < H ? w_ih[(int64_t)j * H + k] : 0.f; }
  const float bias = b_ih[j];
  // three symbols per trip: their 3 * NK embedding loads are in flight together (one symbol per trip paid an L2 latency per symbol: 35 us)
  for (int v0 = 0; v0 < V; v0 += 3) {
    float e[3][NK];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int i = 0; i < NK; ++i) { const int k = i * 64 + lane; e[u][i] = (k < H && v0 + u < V) ? emb[(int64_t)(v0 + u) * H + k] : 0.f; }
    float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int i = 0; i < NK; ++i) s[u] = fmaf(e[u][i], w[i], s[u]);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const float t = wave_sum(s[u]);
      if (lane == 0 && v0 + u < V) table[(int64_t)(v0 + u) * J + j] = t + bias;
    }
  }
}
int gru_table_fwd(hipStream_t st, const float* emb, const float* w_ih, const float* b_ih, int V, int H, float* table) {
  if (H > 1024 || V < 1) return RL_ERR_ARG;
  const int J = 3 * H, NK = (H + 63) / 64;
  const dim3 grid((J + 3) / 4), block(256);
  if (NK <= 4) hipLaunchKernelGGL((gru_table_fwd_kernel<4>), grid, block, 0, st, emb, w_ih, b_ih, V, H, J, table);
  else if (NK <= 8) hipLaunchKernelGGL((gru_table_fwd_kernel<8>), grid, block, 0, st, emb, w_ih, b_ih, V, H, J, table);
  else if (NK <= 12) hipLaunchKernelGGL((gru_table_fwd_kernel<12>), grid, block, 0, st, emb, w_ih, b_ih, V, H, J, table);
  else hipLaunchKernelGGL((gru_table_fwd_kernel<16>), grid, block, 0, st, emb, w_ih, b_ih, V, H, J, table);
  return RL_LAUNCH_CHECK();
}

// dTable [V][3H] -> d b_ih, d W_ih [3H][H], d Emb [V][H].  Every element of d W_ih has ONE owner thread (plain add, no atomics: 1.8 M
// atomics were the whole cost of this kernel); d Emb: a thread owns column k for ALL V rows over a chunk of 64 units, so W_ih is
// read once (7 MB; it was read once per symbol, 33 x) and the chunks meet in V atomics per thread.
__global__ void __launch_bounds__(256)
gru_table_bwd_w_kernel(const float* __restrict__ dt, int ldt, const float* __restrict__ emb, int V, int H,
                       float* d_w_ih, float* d_b_ih) {                  // block per output unit j, thread per k
  __shared__ float dcol[64];
  const int j = blockIdx.x;
  if (threadIdx.x < 64) dcol[threadIdx.x] = (int)threadIdx.x < V ? dt[(int64_t)threadIdx.x * ldt + j] : 0.f;
  __syncthreads();
  if (threadIdx.x == 0) {
    float bsum = 0.f;
    for (int v = 0; v < V; ++v) bsum += dcol[v];
    d_b_ih[j] += bsum;
  }
  for (int k = threadIdx.x; k < H; k += 256) {
    float s = 0.f;
    for (int v = 0; v < V; ++v) s = fmaf(dcol[v], emb[(int64_t)v * H + k], s);
    d_w_ih[(int64_t)j * H + k] += s;
  }
}
constexpr int GRU_TBE_CHUNK = 64, GRU_TBE_VG = 12;
__global__ void __launch_bounds__(256)
gru_table_bwd_e_kernel(const float* __restrict__ dt, int ldt, const float* __restrict__ w_ih, int V, int H, float* d_emb) {
  __shared__ float dts[GRU_TBE_VG][GRU_TBE_CHUNK];                        // this block's [12 symbols][64 units] slice of dTable
  const int k = blockIdx.x * 256 + threadIdx.x;                           // grid (H / 256, 3H / 64, V / 12)
  const int j0 = blockIdx.y * GRU_TBE_CHUNK, nj = min(GRU_TBE_CHUNK, 3 * H - j0);
  const int v0 = blockIdx.z * GRU_TBE_VG;
  for (int e = threadIdx.x; e < GRU_TBE_VG * GRU_TBE_CHUNK; e += 256) {
    const int v = e / GRU_TBE_CHUNK, jj = e - v * GRU_TBE_CHUNK;
    dts[v][jj] = (jj < nj && v0 + v < V) ? dt[(int64_t)(v0 + v) * ldt + j0 + jj] : 0.f;
  }
  __syncthreads();
  if (k >= H) return;
  float acc[GRU_TBE_VG];
#pragma unroll
  for (int v = 0; v < GRU_TBE_VG; ++v) acc[v] = 0.f;
  for (int jj = 0; jj < nj; ++jj) {
    const float w = w_ih[(int64_t)(j0 + jj) * H + k];
#pragma unroll
    for (int v = 0; v < GRU_TBE_VG; ++v) acc[v] = fmaf(dts[v][jj], w, acc[v]);
  }
#pragma unroll
  for (int v = 0; v < GRU_TBE_VG; ++v)                                    // padding_idx = 0 row gets no gradient
    if (v0 + v >= 1 && v0 + v < V) atomicAdd(d_emb + (int64_t)(v0 + v) * H + k, acc[v]);
}
int gru_table_bwd(hipStream_t st, const float* dtable, int ld_dtable, const float* emb, const float* w_ih, int V, int H,
                  float* d_emb, float* d_w_ih, float* d_b_ih) {
  if (V > 64) return RL_ERR_ARG;               // (gru_table_bwd_w_kernel keeps a symbol column of dTable in 64 LDS floats)
  hipLaunchKernelGGL(gru_table_bwd_w_kernel, dim3(3 * H), dim3(256), 0, st, dtable, ld_dtable, emb, V, H, d_w_ih, d_b_ih);
  hipLaunchKernelGGL(gru_table_bwd_e_kernel, dim3((H + 255) / 256, (3 * H + GRU_TBE_CHUNK - 1) / GRU_TBE_CHUNK, (V + GRU_TBE_VG - 1) / GRU_TBE_VG), dim3(256), 0, st,
                     dtable, ld_dtable, w_ih, V, H, d_emb);
  return RL_LAUNCH_CHECK();
}

}  // namespace rl
