// Ping-pong 8-wave NT GEMM for gfx950 (bf16 operands, K % 8 == 0, dense rows):  C[M,N] = A[M,K] . B[N,K]^T + fused epilogue.
//
// Why a second NT kernel: the LDS-DMA fill path delivers ~36-45 B/clk per CU whatever the tile shape, so the
// FLOPs one fetched byte feeds - the workgroup tile - decide how far the fill is from binding:
//   128 x 128 (gemm.hip, two 4-wave workgroups per CU)   64 FLOP/B
//   128 x 192 (this kernel, TWO workgroups per CU)        77 FLOP/B   <- every layer GEMM (N < 4096): the second workgroup's MFMAs run
//                                                                       under the first one's output write and fetch waits
//   256 x 192 / 256 x 256 (this kernel, one per CU)      110 / 128     <- the 21128-wide classifier
// Measured (tools/nt8_probe.cpp, profiles/round2_nt8_probe.log): MFMA, fill and output write are three comparable costs on the
// K = 768 shapes; with the fragment reads the LDS is ~100 % busy (reads queue behind the DMA writes), which is why dedicated
// loader waves changed nothing (measured), and the result sits level with hipBLASLt on the same shapes.
// A 512-thread workgroup, 2 waves per SIMD: waves 0-3 (group 0) and 4-7 (group 1) sit pairwise on the four SIMDs and
// run HALF A PHASE apart (group 1 executes one extra s_barrier up front), so on every SIMD one wave is in its MEMORY segment
// (fragment ds_reads + its share of the LDS-DMA fetches + the counted vmcnt wait) while its partner is in its MFMA segment
// (16 v_mfma_f32_16x16x32_bf16 on register-resident fragments, s_setprio 1).
//
// K-tile = 64 (one 128-byte LDS row per operand row, 16-byte chunks XOR-swizzled by row: KTile).  A K-tile is consumed in NPH
// phases: the HELD operand's fragments of the whole K-tile are read once (phase 0) and stay in registers, the STREAMED operand
// is read SQ 16-row tiles per phase.  The ring has NS K-tile stages; the 1-KiB pieces (8 rows) of a stage are fetched in the
// order the phases need them (held operand + streamed group 0 first) and are issued LEAD phases ahead of the phase that reads
// their tile's first fragment, a fixed number per phase, so every s_waitcnt vmcnt(N) in the loop is a compile-time count and
// never 0 in steady state.  Hazards (both groups, half a phase apart):
//   RAW  a piece is waited for (own vmcnt, then a barrier) in the phase BEFORE the one that reads it;
//   WAR  a region is re-filled >= 2 phases after the phase that read it last.
// Both are static_assert-ed on the schedule below.
#include "gemm_dev.h"
#include "nt8_cfg.h"
#include "prof.h"

namespace rl {

static int g_nt8_group_m = 0;
void set_nt8_group_m(int g) { g_nt8_group_m = g; }

// Logical tile id -> (tile row, tile column).  group_m <= 1: row-major (a run of consecutive ids walks along N: its tiles share
// few A rows but touch every B column panel).  group_m > 1: ids walk down group_m tile rows before moving to the next tile
// column, so the ~64 tiles an XCD has in flight form a group_m x (64 / group_m) block whose A and B panels fit its 4 MiB L2.
__device__ __forceinline__ void tile_coords(int tile, int tiles_n, int ntiles, int group_m, int& tm, int& tn) {
  if (group_m <= 1) { tm = tile / tiles_n; tn = tile - tm * tiles_n; return; }
  const int tiles_m = ntiles / tiles_n;
  const int per_group = group_m * tiles_n;
  const int g = tile / per_group, r = tile - g * per_group;
  const int rows = min(group_m, tiles_m - g * group_m);
  tn = r / rows;
  tm = g * group_m + (r - tn * rows);
}

// Row state of the GRU epilogue, fetched at kernel start so that the dependent chain perm -> pho_idx -> table row (three global
// latencies) and the h_prev rows run under the main loop instead of in front of every 16-row chunk of the epilogue.
struct GruRows { int tok[2]; int gi_off[2]; bool ends[2]; uint4 hp[2]; };
template <typename C>
__device__ __forceinline__ void nt8_gru_prefetch(const EpiParams<bf16_t>& ep, GruRows& gr, int mlive, int H, int m0, int tn, int wm, int wn, int lane) {
  const int r = lane >> 2, o = lane & 3;
  const int unit0 = tn * 64 + wn * 32 + o * 8;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int i = m0 + wm * C::RM + c * 16 + r;
    const bool ok = i < mlive;
    const int tok = ok ? ep.gru_perm[i] : 0;
    const int64_t v = ok ? ep.gru_pho_idx[(int64_t)tok * ep.gru_Tp + ep.gru_t] : 0;
    gr.tok[c] = tok;
    gr.gi_off[c] = (int)v * 3 * H + unit0;
    gr.ends[c] = ok && ep.gru_lens[i] == ep.gru_t + 1;
    gr.hp[c] = ok ? *(const uint4*)(ep.gru_hprev + (int64_t)i * H + unit0) : uint4{0u, 0u, 0u, 0u};
  }
}
template <typename C>
__device__ __forceinline__ void nt8_gru_epilogue(char* smem, const EpiParams<bf16_t>& ep, floatx4 (&acc)[C::MT][C::NT], const GruRows& gr, int mlive, int H,
                                                 int m0, int tn, int wave, int wm, int wn, int lane) {
  typedef bf16_t T;
  constexpr int RS = C::RS, ER = 16;
  static_assert(C::RN == 96 && C::RM == 32 && 8 * ER * RS * 4 <= C::LDS, "GRU epilogue geometry");
  const int g = lane >> 4, l15 = lane & 15;
  float* et = (float*)smem + wave * (ER * RS);
  const int r = lane >> 2, o = lane & 3;
  const int unit0 = tn * 64 + wn * 32 + o * 8;
#pragma unroll
  for (int c = 0; c < C::RM / ER; ++c) {
#pragma unroll
    for (int j = 0; j < C::NT; ++j) *(floatx4*)(et + l15 * RS + j * 16 + 4 * g) = acc[c][j];
    // (a wave reads back only what it wrote: no barrier, the LDS ops of a wave are in order)
    const int i = m0 + wm * C::RM + c * ER + r;
    if (i >= mlive) continue;
    float hr[8], hz[8], hn[8];
#pragma unroll
    for (int e = 0; e < 8; e += 4) {
      *(floatx4*)&hr[e] = *(const floatx4*)(et + r * RS + o * 8 + e);
      *(floatx4*)&hz[e] = *(const floatx4*)(et + r * RS + 32 + o * 8 + e);
      *(floatx4*)&hn[e] = *(const floatx4*)(et + r * RS + 64 + o * 8 + e);
    }
    const float* b = ep.bias + unit0;
    const float* gi = ep.gru_table + gr.gi_off[c];
    float br[8], bz[8], bn[8], ir[8], iz[8], in[8];
#pragma unroll
    for (int e = 0; e < 8; e += 4) {
      *(floatx4*)&br[e] = *(const floatx4*)(b + e); *(floatx4*)&bz[e] = *(const floatx4*)(b + H + e); *(floatx4*)&bn[e] = *(const floatx4*)(b + 2 * H + e);
      *(floatx4*)&ir[e] = *(const floatx4*)(gi + e); *(floatx4*)&iz[e] = *(const floatx4*)(gi + H + e); *(floatx4*)&in[e] = *(const floatx4*)(gi + 2 * H + e);
    }
    floatx4 p0, p1;
    unpack8(gr.hp[c], p0, p1);
    float rr[8], zz[8], nn[8], hh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      // bias, then the bf16 round trip of the two-launch form (GEMM stores bf16(acc + b_hh), the gate kernel reads it back)
      const float xr = bf2f(f2bf(hr[e] + br[e])), xz = bf2f(f2bf(hz[e] + bz[e]));
      hn[e] = bf2f(f2bf(hn[e] + bn[e]));
      const float hp = e < 4 ? p0[e] : p1[e - 4];
      gru_unit<T>(ir[e], iz[e], in[e], xr, xz, hn[e], hp, rr[e], zz[e], nn[e], hh[e]);
    }
    auto st8 = [&](T* p, const float (&x)[8]) { store8<T>(p, floatx4{x[0], x[1], x[2], x[3]}, floatx4{x[4], x[5], x[6], x[7]}); };
    if (ep.gru_rzn != nullptr) {
      T* s = ep.gru_rzn + (int64_t)i * 3 * H + unit0;
      st8(s, rr); st8(s + H, zz); st8(s + 2 * H, nn);
    }
    if (ep.gru_gh != nullptr) st8(ep.gru_gh + (int64_t)i * 3 * H + 2 * H + unit0, hn);
    st8(ep.out + (int64_t)i * H + unit0, hh);
    if (gr.ends[c]) st8(ep.gru_out + (int64_t)gr.tok[c] * H + unit0, hh);
  }
}

// XEPI: 0 = the standard epilogues (EpiParams::mode), 2 = K6 (GRU gate math on
// gate-interleaved B rows), 3 = the standard epilogues over a LIST of live 16-row blocks (EpiParams::live_list) - separate
// instantiations, so that the special forms' registers are not the layer GEMMs' problem; 4 = the same over a LIST of live ROWS
// (round 6, EpiParams::live_unit == 1: row-granular packing - a tile is ANY 128 listed rows, so no tile row is spent on the padding
// rows that complete a sentence's last 16-row block; the per-lane fetch offset of a piece and the output row of an epilogue item
// come from the list, nothing changes in the main loop)
template <typename C, bool KTAIL = false, int XEPI = 0>
__global__ void __launch_bounds__(512, 2 * C::WGS)
gemm_nt8_kernel(const bf16_t* __restrict__ A_, int64_t lda, const bf16_t* __restrict__ B_, int64_t ldb, int M, int N, int K, int tiles_n,
                int ntiles, int group_m, EpiParams<bf16_t> ep) {
  typedef bf16_t T;
  typedef MmaBF16 Mma;
  constexpr int NPW = C::NPW, NPH = C::NPH, NS = C::NS, LEAD = C::LEAD, SQ = C::SQ, HT = C::HT, MT = C::MT, NT = C::NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l15 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2;
  const int wm = wave / C::WN, wn = wave - wm * C::WN;
  // split-K launches (ep.ksplit > 1): ksplit x ntiles workgroups, split-major so that the tiles of one K-range - which share its
  // operand columns - sit behind the same L2s; the workgroup's K-range becomes its whole problem (operands advanced, K shortened)
  const bf16_t* __restrict__ A = A_;
  const bf16_t* __restrict__ B = B_;
  int tile, split = 0;
  if (!KTAIL && ep.ksplit > 1) {
    const int logical = xcd_remap(blockIdx.x, ntiles * ep.ksplit);
    split = logical / ntiles; tile = logical - split * ntiles;
    const int per = (((K + 63) >> 6) + ep.ksplit - 1) / ep.ksplit;
    const int k0 = split * per * 64;
    A += k0; B += k0; K = min(K - k0, per * 64);
  } else if constexpr (XEPI == 3 || XEPI == 4) {
    tile = 0;
  } else {
    tile = xcd_remap(blockIdx.x, ntiles);
  }
  int tm, tn;
  int nlive = 0;                                            // XEPI 3: live 16-row blocks; tile row tm owns list entries tm * BM / 16 ..
  constexpr bool LIVE = XEPI == 3 || XEPI == 4;
  constexpr int LUNIT = XEPI == 4 ? 1 : 16;                 // rows per list entry
  if constexpr (LIVE) {
    // the launch is sized for every block being live; the XCD split is made over the tiles that exist (made over the nominal count,
    // the surplus tiles - the tail of the logical order - would all sit on the last XCDs and leave them idle)
    nlive = *ep.live_count;
    const int tml = (nlive + C::BM / LUNIT - 1) / (C::BM / LUNIT);      // live tile rows
    const int ntl = tml * tiles_n;
    if (ep.xcd_gc > 1) {
      // 2-D XCD split (EpiParams::xcd_gc): XCD x = blockIdx % 8 (as dispatched today; another placement changes speed only) works on row
      // group x / gc x column group x % gc, row-major inside it
      const int gc = ep.xcd_gc, gr = 8 / gc, x = blockIdx.x & 7;
      const int j = blockIdx.x >> 3;
      const int rg = x / gc, cg = x - rg * gc, ncl = tiles_n / gc;
      const int r0 = (rg * tml) / gr, r1 = ((rg + 1) * tml) / gr;
      if (j >= (r1 - r0) * ncl) return;                     // (the whole workgroup leaves before any barrier)
      const int lr = j / ncl;
      tm = r0 + lr; tn = cg * ncl + (j - lr * ncl);
      tile = tm * tiles_n + tn;
    } else {
      if ((int)blockIdx.x >= ntl) return;                  // (the whole workgroup leaves before any barrier)
      tile = xcd_remap(blockIdx.x, ntl);
      tile_coords(tile, tiles_n, ntl, group_m, tm, tn);
    }
  } else {
    tile_coords(tile, tiles_n, ntiles, group_m, tm, tn);
  }
  const int m0 = tm * C::BM, n0 = tn * C::BN;
  const int mlive = ep.m_dev != nullptr ? *ep.m_dev : M;
  if (!LIVE && m0 >= mlive) return;                         // device-side live-row count: the whole workgroup leaves before any barrier
  const int mzero = ep.m_exact ? mlive : M;                 // A rows at or beyond it read as zeros
  GruRows gru_rows;
  if constexpr (XEPI == 2) nt8_gru_prefetch<C>(ep, gru_rows, mlive, N / 3, m0, tn, wave / C::WN, wave % C::WN, lane);
  const int nk = (K + 63) >> 6;
  const int ktail = KTAIL ? (K & 63) : 0;   // elements of a ragged last K-tile (multiple of 8); KTAIL = false: K % 64 == 0

  // ---- this wave's pieces: LDS offset inside a stage (scalar) and per-lane source offset (row clamped into the matrix: rows
  //      beyond M / N only feed accumulators that the epilogue never stores)
  const int lrow = lane >> 3;
  const int kchunk_b = (((lane & 7) ^ lrow) << 4);            // byte offset of the 16-byte chunk this lane fetches (source-side swizzle)
  int lo[NPW];
  uint32_t go[NPW];
#pragma unroll
  for (int s = 0; s < NPW; ++s) {
    const int p = s * 8 + wave;
    int row, is_b;
    if (s < C::HPW) { row = p * 8; is_b = C::HOLD_B ? 1 : 0; }
    else {
      const int pp = p - C::HP, q = pp / C::GP, rem = pp - q * C::GP, slice = rem / (SQ * 2), j = rem - slice * (SQ * 2);
      row = slice * C::SR + q * SQ * 16 + j * 8; is_b = C::HOLD_B ? 0 : 1;
    }
    lo[s] = (is_b ? C::A_BYTES : 0) + row * 128;
    int grow = is_b ? min(n0 + row + lrow, N - 1) : min(m0 + row + lrow, M - 1);
    if constexpr (XEPI == 2) {
      if (is_b) {                                 // gate-interleaved column tile: [r | z | n] x 32 units for each of the two wave columns
        const int c = row + lrow, half = c / 96, cc = c - half * 96, gate = cc >> 5;
        grow = gate * (N / 3) + tn * 64 + half * 32 + (cc & 31);
      }
    }
    bool park = !LIVE && !is_b && m0 + row + lrow >= mzero;
    if constexpr (XEPI == 4) {
      if (!is_b) {                                  // the lane's row of the piece is the list's entry (tile row tm owns entries tm * BM ..)
        const int j = tm * C::BM + row + lrow;
        const int r = j < nlive ? ep.live_list[j] : -1;
        grow = r < 0 ? 0 : r;
        park = r < 0;                               // list exhausted inside the last tile: zeros
      }
    }
    if constexpr (XEPI == 3) {
      if (!is_b) {                                  // a piece is 8 rows of ONE 16-row block (row % 8 == 0): wave-uniform list entry
        const int j = tm * (C::BM / 16) + (row >> 4);
        const int blk = j < nlive ? ep.live_list[j] : -1;
        grow = (blk < 0 ? 0 : blk) * 16 + ((row + lrow) & 15);
        park = blk < 0;                             // list exhausted inside the last tile: zeros
      }
    }
    go[s] = (uint32_t)((int64_t)grow * (is_b ? ldb : lda) * 2 + kchunk_b);
    if (park) go[s] = 0xFFFFFF00u;                  // beyond num_records: the buffer range check returns zeros
  }
  // Fetches are raw-buffer LDS-DMA loads: resource descriptor + K-tile byte offset in SGPRs, the per-lane row/chunk offset in
  // ONE 32-bit VGPR per piece - no vector ALU work per fetch (a 64-bit flat address costs two v_lshl_add_u64 each, which showed
  // up as +40 % on the fetch-only probe).  A ragged last K-tile (K % 64 != 0) parks the chunks past K on an offset beyond
  // num_records: the buffer range check returns zeros for them.
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, (int)(((int64_t)(M - 1) * lda + K) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)B, 0, (int)(((int64_t)(N - 1) * ldb + K) * 2), 0x00020000);
  const bool lane_past_k = KTAIL && ktail != 0 && kchunk_b >= 2 * ktail;
  auto issue = [&](auto s_c, int stage, int ktile) {
    constexpr int s = decltype(s_c)::value;
    constexpr bool is_b = (s < C::HPW) ? C::HOLD_B : !C::HOLD_B;
    uint32_t voff = go[s];
    if constexpr (KTAIL) { if (ktail != 0 && ktile == nk - 1) voff = lane_past_k ? 0xFFFFFF00u : voff; }
    // (round 6: the B fetches marked non-temporal - aux = 2 - so that a co-resident workgroup's A lines outlive them in the L1: the family
    // 6.5 -> 7.2 ms/step; the weight tiles live on their L2 / L1 residency.  profiles/round6_ab.log)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(is_b ? rsB : rsA, (__attribute__((address_space(3))) void*)(smem + stage * C::STAGE + lo[s]), 16,
                                             voff, ktile * 128, 0, 0);
  };

  // ---- fragment addressing: lane part (row l15 of a 16-row tile, chunk ks*4+g swizzled by the row) + wave slice
  int fa[2], fb[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int lane_sw = l15 * 128 + ((((ks << 2) + g) ^ (l15 & 7)) << 4);
    fa[ks] = wm * C::RM * 128 + lane_sw;
    fb[ks] = C::A_BYTES + wn * C::RN * 128 + lane_sw;
  }
  floatx4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  bf16x8_t hf[HT][2], sf[SQ][2];

  // ---- prologue: the pieces the steady state would have issued before phase 0
  static_for<C::PRO_TILES>([&](auto dt_c) {
    constexpr int dt = decltype(dt_c)::value;
    if (dt < nk) {
      static_for<NPW>([&](auto s_c) {
        constexpr int s = decltype(s_c)::value;
        if constexpr (C::in_prologue(dt, s)) issue(s_c, dt % NS, dt);
      });
    }
  });
  if (nk >= C::PRO_TILES) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::VM_PRO) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (grp == 1) { __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }     // group 1 runs half a phase behind

  auto phase = [&](auto par_c, auto q_c, int t) {
    constexpr int PAR = decltype(par_c)::value, q = decltype(q_c)::value;
    constexpr int dt2 = (q + LEAD) / NPH, q2 = (q + LEAD) % NPH, SBASE = PAR * C::STAGE;
    // ---------------- memory segment
    constexpr int dtw = (q + LEAD) / NPH;                             // tile of the last issue slot before this phase's wait
    const bool do_issue = t + dt2 < nk;
    auto issue_all = [&]() {
      if (do_issue) {
        static_for<NPW>([&](auto s_c) {
          constexpr int s = decltype(s_c)::value;
          if constexpr (s >= C::cum(q2) && s < C::cum(q2 + 1)) issue(s_c, (PAR + dt2) % NS, t + dt2);
        });
      }
    };
    if constexpr (q == 0) {
#pragma unroll
      for (int h = 0; h < HT; ++h)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          hf[h][ks] = *(const bf16x8_t*)(smem + SBASE + h * 2048 + (C::HOLD_B ? fb[ks] : fa[ks]));
    }
#pragma unroll
    for (int i = 0; i < SQ; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        sf[i][ks] = *(const bf16x8_t*)(smem + SBASE + (q * SQ + i) * 2048 + (C::HOLD_B ? fa[ks] : fb[ks]));
    __builtin_amdgcn_sched_barrier(0);
    issue_all();
    if (t + dtw < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::vm(q)) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // ---------------- MFMA segment
    constexpr int NM = 2 * SQ * HT;
    __builtin_amdgcn_s_setprio(1);
    static_for<NM>([&](auto m_c) {
      constexpr int m = decltype(m_c)::value, ks = m / (SQ * HT), i = (m / HT) % SQ, h = m % HT;
      if constexpr (C::HOLD_B) acc[q * SQ + i][h] = Mma::mma(hf[h][ks], sf[i][ks], acc[q * SQ + i][h]);
      else acc[h][q * SQ + i] = Mma::mma(sf[i][ks], hf[h][ks], acc[h][q * SQ + i]);
    });
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  for (int tb = 0; tb < nk; tb += NS) {
    static_for<NS>([&](auto par_c) {
      constexpr int PAR = decltype(par_c)::value;
      if (tb + PAR < nk) static_for<NPH>([&](auto q_c) { phase(par_c, q_c, tb + PAR); });
    });
  }
  if (grp == 0) { __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }     // barrier census: group 1 took one extra up front

  if constexpr (XEPI == 2) {             // (the ring is dead: both groups passed the loop's last barrier)
    nt8_gru_epilogue<C>(smem, ep, acc, gru_rows, mlive, N / 3, m0, tn, wave, wm, wn, lane);
    return;
  }
  // ---------------- epilogue: per-wave fp32 transpose through LDS, 8 consecutive columns (16 B of bf16) per lane
  constexpr int RS = C::RS, ER = C::ER, ITEMS = C::RN / 8, NIT = ER * ITEMS / 64;
  float* et = (float*)smem + wave * (ER * RS);
  const int row_w = m0 + wm * C::RM, col_w = n0 + wn * C::RN;
  // Round 5 (EpiParams::bias_first): alpha and the bias go into the accumulators BEFORE the transposes.  In the
  // MFMA layout a lane holds four consecutive columns of one row per tile, so NT float4 of bias serve all its accumulators - loaded
  // once, together, while nothing else is pending - instead of two float4 per item behind that item's predecessors' stores (hipcc
  // waits with vmcnt(0) whenever loads and stores are pending together: every item of a wave paid a bias latency plus the drain of
  // the stores before it; the bias-only epilogues - qkv, FFN-up - now run their items without a single wait).  Same (acc * alpha) +
  // bias per element as epilogue8: same bits.
  EpiParams<bf16_t> epx = ep;
  // row-granular list: the output row of every item this lane will store (NCH chunks x NIT items), requested here - before the first
  // store, so that no tracked load meets a pending store later -; -1 beyond the list
  constexpr int NCH_ = C::RM / ER;
  int rid[XEPI == 4 ? NCH_ : 1][XEPI == 4 ? NIT : 1];
  if constexpr (XEPI == 4) {
#pragma unroll
    for (int c = 0; c < NCH_; ++c)
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int e = lane + 64 * it, r = e / ITEMS;
        const int jr = tm * C::BM + wm * C::RM + c * ER + r;
        rid[c][it] = jr < nlive ? ep.live_list[jr] : -1;
      }
  }
  if constexpr (!KTAIL) {
    if (ep.bias_first && ep.slab == nullptr) {
      if (ep.alpha != 1.0f) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] *= ep.alpha;
      }
      if (ep.bias != nullptr) {
        floatx4 bq[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) bq[j] = *(const floatx4*)(ep.bias + min(col_w + j * 16 + 4 * g, N - 4));
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] += bq[j];
      }
      epx.alpha = 1.0f; epx.bias = nullptr;
    }
  }
  // Round 5 (same condition): the residual / pre-activation / accumulated-output octets of ALL of the wave's items are requested here, before
  // the first store, from addresses clamped into the matrix (unconditional loads: nothing between them for the compiler to wait on);
  // epilogue8_pre then runs item by item on registers.  Two-per-CU shape only (RM / ER chunks x NIT items = 6 octets = 24 registers).
  if constexpr (!KTAIL && (XEPI == 0 || LIVE) && C::WGS == 2) {
    const bool use_aux = ep.mode == EPI_DROP_RESID || ep.mode == EPI_GELU_BWD;
    const bool use_old = ep.mode == EPI_STORE && ep.accumulate != 0;
    if (ep.bias_first && ep.slab == nullptr && ep.rm_hw_shift < 0 && (use_aux || use_old) && !(ep.mode == EPI_GELU_BWD && ep.accumulate) &&
        (!use_aux || ep.aux != nullptr) && (N % 8) == 0) {
      constexpr int NCH = C::RM / ER;
      const bf16_t* src = use_aux ? ep.aux : (const bf16_t*)ep.out;
      const int64_t ld = use_aux ? ep.ldaux : ep.ldo;
      int rcs[NCH];
      bool cok[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        rcs[c] = row_w + c * ER; cok[c] = true;
        if constexpr (XEPI == 3) {
          const int j = tm * (C::BM / 16) + ((wm * C::RM + c * ER) >> 4);
          cok[c] = j < nlive;
          rcs[c] = cok[c] ? ep.live_list[j] * 16 : 0;
        }
      }
      EpiParams<bf16_t> e3 = ep;
      e3.bias = nullptr; e3.alpha = 1.0f;                  // (both are in the accumulators already: bias_first)
      typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;      // (a register-class type: HIP's uint4 struct cannot be an asm operand)
      u32x4_t pre[NCH][NIT];
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int e = lane + 64 * it, r = e / ITEMS, c8 = e - r * ITEMS;
          int prow = rcs[c] + r;
          if constexpr (XEPI == 4) prow = max(rid[c][it], 0);
          pre[c][it] = *(const u32x4_t*)(src + (int64_t)min(prow, M - 1) * ld + min(col_w + c8 * 8, N - 8));
        }
      // first transpose under the loads' latency, then ONE unconditional wait for all six octets: left to their first uses - inside the
      // items' bounds-check branches - the compiler could not prove them landed on every path and re-waited, with stores pending, by vmcnt(0)
#pragma unroll
      for (int i = 0; i < ER / 16; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) *(floatx4*)(et + (i * 16 + l15) * RS + j * 16 + 4 * g) = acc[i][j];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int it = 0; it < NIT; ++it) asm volatile("" : "+v"(pre[c][it]));
#endif
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (c > 0) {
#pragma unroll
          for (int i = 0; i < ER / 16; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) *(floatx4*)(et + (i * 16 + l15) * RS + j * 16 + 4 * g) = acc[c * (ER / 16) + i][j];
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int e = lane + 64 * it, r = e / ITEMS, c8 = e - r * ITEMS;
          const floatx4 v0 = *(const floatx4*)(et + r * RS + c8 * 8), v1 = *(const floatx4*)(et + r * RS + c8 * 8 + 4);
          if constexpr (XEPI == 4) {
            if (rid[c][it] >= 0) epilogue8_pre(e3, M, N, rid[c][it], col_w + c8 * 8, v0, v1, __builtin_bit_cast(uint4, pre[c][it]));
          } else {
            if (cok[c]) epilogue8_pre(e3, M, N, rcs[c] + r, col_w + c8 * 8, v0, v1, __builtin_bit_cast(uint4, pre[c][it]));
          }
        }
      }
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < C::RM / ER; ++c) {
    int row_c = row_w + c * ER;
    if constexpr (XEPI == 3) {                      // the chunk's 16 rows are one listed block (or lie beyond the list: nothing to store)
      static_assert(!LIVE || ER == 16, "live-row form: one 16-row block per epilogue chunk");
      const int j = tm * (C::BM / 16) + ((wm * C::RM + c * ER) >> 4);
      if (j >= nlive) continue;
      row_c = ep.live_list[j] * 16;
    }
#pragma unroll
    for (int i = 0; i < ER / 16; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) *(floatx4*)(et + (i * 16 + l15) * RS + j * 16 + 4 * g) = acc[c * (ER / 16) + i][j];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e = lane + 64 * it, r = e / ITEMS, c8 = e - r * ITEMS;
      const floatx4 v0 = *(const floatx4*)(et + r * RS + c8 * 8), v1 = *(const floatx4*)(et + r * RS + c8 * 8 + 4);
      if constexpr (XEPI == 4) {
        if (rid[c][it] >= 0) epilogue8<T>(epx, M, N, rid[c][it], col_w + c8 * 8, v0, v1);
      } else if (!KTAIL && ep.slab != nullptr) {
        const int row = row_c + r, col = col_w + c8 * 8;
        if (row < M && col < N) {
          float* o = ep.slab + (int64_t)split * ep.slab_stride + (int64_t)row * N + col;
          *(floatx4*)o = v0; *(floatx4*)(o + 4) = v1;
        }
      } else {
        epilogue8<T>(epx, M, N, row_c + r, col_w + c8 * 8, v0, v1);
      }
    }
  }
}


template <typename C, bool KTAIL = false, int XEPI = 0>
static int launch_nt8_cfg(hipStream_t st, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, int M, int N, int K,
                          const EpiParams<bf16_t>& ep) {
  const int tiles_m = (M + C::BM - 1) / C::BM, tiles_n = (N + C::BN - 1) / C::BN, ntiles = tiles_m * tiles_n;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)gemm_nt8_kernel<C, KTAIL, XEPI>, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS);
    attr_set = true;
  }
  ProfScope ps(st, PK_GEMM_NT, 2.0 * M * N * K);
  if (ep.m_dev != nullptr) prof_set_exec(ep.m_dev, 2.0 * N * K, C::BM, M);      // tiles that start at or beyond the count leave at once
  if constexpr (XEPI == 3) prof_set_exec(ep.live_count, 2.0 * N * K * 16.0, C::BM / 16, M / 16);      // (counted in 16-row blocks)
  if constexpr (XEPI == 4) prof_set_exec(ep.live_count, 2.0 * N * K, C::BM, M);                       // (counted in rows, whole tiles)
  EpiParams<bf16_t> epk = ep;
  epk.bias_first = (N % 4) == 0 && N >= 4;
  int grid = ntiles * (KTAIL || ep.ksplit < 1 ? 1 : ep.ksplit);
  if constexpr (XEPI == 3 || XEPI == 4) { if (ep.xcd_gc > 1) grid = (tiles_m + 8 / ep.xcd_gc) * tiles_n; }      // every row group rounded up to whole tile rows
  RL_LAUNCH((gemm_nt8_kernel<C, KTAIL, XEPI>), dim3(grid), dim3(512), C::LDS, st, A, lda, B, ldb, M, N, K, tiles_n, ntiles, g_nt8_group_m, epk);
  return hipGetLastError() == hipSuccess ? RL_OK : RL_ERR_LAUNCH;
}


//             BM   BN  WM WN hold_B SQ NS LEAD WGS
typedef Nt8Cfg<256, 192, 4, 2, false, 2, 2, 4> Cfg256x192;        // wave  64 x 96, 3 phases of 16 MFMAs
typedef Nt8Cfg<128, 192, 2, 4, true, 2, 3, 4> Cfg128x192;         // wave  64 x 48, 2 phases of 12 MFMAs, 3 stages
typedef Nt8Cfg<128, 192, 4, 2, false, 2, 2, 4, 2> Cfg128x192q;    // two workgroups per CU (80 KB each): one's epilogue and fetch
                                                                  //   waits run under the other's MFMAs

bool nt8_supported(int M, int N, int K, const EpiParams<bf16_t>& ep, int64_t lda, int64_t ldb) {
  if (ep.mode == EPI_AFFINE || ep.col_scale != nullptr) return false;      // (the 4-wave kernels' epilogues carry it)
  return (K % 8) == 0 && K >= 64 && (N % 8) == 0 && (ep.ldo % 8) == 0 && (ep.aux == nullptr || (ep.ldaux % 8) == 0) &&
         (lda % 8) == 0 && (ldb % 8) == 0 && M >= 1 && N >= 8 &&
         (int64_t)M * lda * 2 < 0xFFFFFF00ll && (int64_t)N * ldb * 2 < 0xFFFFFF00ll;
}

int gemm_nt8_gru(hipStream_t st, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, int M, int N, int K, const EpiParams<bf16_t>& ep) {
  const int H = N / 3;
  if (ep.gru_table == nullptr || ep.gru_pho_idx == nullptr || ep.gru_perm == nullptr || ep.gru_lens == nullptr || ep.gru_hprev == nullptr ||
      ep.out == nullptr || ep.gru_out == nullptr || ep.bias == nullptr || ep.mode != EPI_STORE || ep.accumulate || ep.slab != nullptr ||
      N != 3 * H || (H % 64) != 0 || (K % 64) != 0 || M < 1 || !nt8_supported(M, N, K, ep, lda, ldb))
    return RL_ERR_ARG;
  return launch_nt8_cfg<Cfg128x192q, false, 2>(st, A, lda, B, ldb, M, N, K, ep);
}

// the M dimension as a list of live 16-row blocks (EpiParams::live_list / live_count): see gemm.h
static int g_nt8_live_gc = 0;
void set_nt8_live_gc(int gc) { g_nt8_live_gc = (gc == 1 || gc == 2 || gc == 4 || gc == 8) ? gc : 0; }
int gemm_nt8_live(hipStream_t st, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, int M, int N, int K, const EpiParams<bf16_t>& ep) {
  if (ep.live_list == nullptr || ep.live_count == nullptr || ep.m_dev != nullptr || ep.slab != nullptr || ep.rm_hw_shift >= 0 ||
      ep.gru_table != nullptr || (K % 64) != 0 || (M % 16) != 0 || M < 16 || !nt8_supported(M, N, K, ep, lda, ldb))
    return RL_ERR_ARG;
  EpiParams<bf16_t> e2 = ep;
  // XCD split.  One row band per XCD streams the WHOLE weight panel through each of the eight L2s; a panel beyond ~2 MB (N x K x 2 B:
  // 3.5 MB qkv, 4.7 MB FFN-up) does not stay resident next to the A rows and is re-read per wave of workgroups.  With column groups
  // the slice an XCD needs (panel / gc) stays resident and the A rows are read by gc XCDs: traffic gc x A + (8 / gc) x W - for the
  // wide K = 768 outputs (A 9 MB) two groups are the minimum, for the N = 768 outputs (A 27-36 MB at K = 2304 / 3072) one is.
  const int tiles_n = (N + 191) / 192;
  int gc = 1;
  if ((int64_t)N * K * 2 > (int64_t)(2 << 20) && (int64_t)M * K < (int64_t)N * K * 4) gc = 2;
  if (g_nt8_live_gc) gc = g_nt8_live_gc;
  while (gc > 1 && (tiles_n % gc) != 0) gc >>= 1;
  e2.xcd_gc = gc;
  if (ep.live_unit == 1) return launch_nt8_cfg<Cfg128x192q, false, 4>(st, A, lda, B, ldb, M, N, K, e2);      // list of rows
  if (ep.live_unit != 16) return RL_ERR_ARG;
  return launch_nt8_cfg<Cfg128x192q, false, 3>(st, A, lda, B, ldb, M, N, K, e2);
}

int gemm_nt8_splitk(hipStream_t st, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, int M, int N, int K, int nsplit,
                    float* slab, int64_t slab_stride, const int* m_dev) {
  EpiParams<bf16_t> ep;
  ep.mode = EPI_STORE; ep.ldo = N; ep.m_dev = m_dev; ep.slab = slab; ep.slab_stride = slab_stride; ep.ksplit = nsplit;
  const int nk = K / 64;
  if (slab == nullptr || (K % 64) != 0 || nsplit < 1 || nsplit > 16 || (N % 8) != 0 || (lda % 8) != 0 || (ldb % 8) != 0 || M < 1 ||
      (int64_t)M * lda * 2 >= 0xFFFFFF00ll || (int64_t)N * ldb * 2 >= 0xFFFFFF00ll || slab_stride < (int64_t)M * N ||
      (nsplit - 1) * ((nk + nsplit - 1) / nsplit) >= nk)          // every K-range holds at least one K-tile
    return RL_ERR_ARG;
  return launch_nt8_cfg<Cfg128x192q>(st, A, lda, B, ldb, M, N, K, ep);
}

// tile: 0 = from the shape, 2 = 256x192, 4 = 128x192 (three stages), 6 = 128x192 two workgroups per CU.  Returns the tile that runs;
// 8: the ragged-K instantiation (one tile shape, 128x192 three stages, carries the tail code)
int nt8_tile(int N, int K, int tile) {
  if (K % 64) return 8;
  // outputs up to a few thousand columns: the two-workgroups-per-CU shape.  Its smaller tile fetches 43 % more bytes per flop
  // than 256x192, but the second workgroup's MFMAs run under the first one's output write (a third of a K = 768 GEMM's time with
  // one workgroup per CU) and under its fetch waits: qkv 39.6 -> 35.0 us, ffn1+GELU 56.1 -> 51.3, attn-out 14.6 -> 14.3, the
  // K = 2304 / 3072 shapes equal (tools/nt8_probe.cpp ws, profiles/round2_nt8_probe.log).  Wider outputs the persistent kernel does
  // not take: 256 x 192, one workgroup per CU.
  if (tile == 0) tile = N < 4096 ? 6 : 2;
  return tile;
}

int gemm_nt8(hipStream_t st, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, int M, int N, int K,
             const EpiParams<bf16_t>& ep, int tile) {
  if (!nt8_supported(M, N, K, ep, lda, ldb)) return RL_ERR_ARG;
  switch (nt8_tile(N, K, tile)) {
    case 8: return launch_nt8_cfg<Cfg128x192, true>(st, A, lda, B, ldb, M, N, K, ep);
    case 2: return launch_nt8_cfg<Cfg256x192>(st, A, lda, B, ldb, M, N, K, ep);
    case 6: return launch_nt8_cfg<Cfg128x192q>(st, A, lda, B, ldb, M, N, K, ep);
    case 4: return launch_nt8_cfg<Cfg128x192>(st, A, lda, B, ldb, M, N, K, ep);
    default: return RL_ERR_ARG;
  }
}

}  // namespace rl
