// The step engine: SpellBert.forward / SpellBertPho2ResArch3.forward (src/models.py:50-73, 806-870)
// and their backward as ONE host call each.  The engine owns the launch order, the activation
// workspace plan and the compute-dtype operand shadows; it enqueues every kernel on the caller's HIP
// stream and never synchronises or allocates, so a step is two C calls from Python (forward,
// backward) plus the optimizer call, independent of the ~900 kernels in between.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "attention.h"
#include "engine.h"
#include "gemm.h"
#include "layout.h"
#include "ops.h"

namespace rl {

// Weight-gradient overlap (default on): the four wgrad GEMMs of a BERT layer run on an engine-owned side stream while the caller's
// stream continues with the data-gradient chain (two dY buffer sets, by layer parity).  +2.3 % step throughput on top of the branch
// overlap below (bench.py: 23.6 -> 23.1 ms); identical results.  Per-kernel durations become overlap-dependent, so bench.py
// switches both overlaps off on the steps whose launches it brackets with events.
static int g_wgrad_overlap = 1;
void set_wgrad_overlap(int on) { g_wgrad_overlap = on; }
// Grouped weight gradients (default on): the four wgrad GEMMs of a transformer layer go out as ONE launch of 432 tiles with no
// reduction split (gemm_tn_group) once the layer's last dY exists, instead of four launches that each split the reduction 3-4 ways
// and fold the slabs afterwards.
static int g_wgrad_group = 1;
void set_wgrad_group(int on) { g_wgrad_group = on; }
// Stride-2 data gradients of the glyph ResNet by input-pixel parity classes (default on): four class GEMMs over a quarter of the rows
// with 1 / 2 / 2 / 4 taps instead of one GEMM over all rows with 9 taps of which 75 % are stride misses (zeros).
static int g_dgrad_parity = 1;
void set_dgrad_parity(int on) { g_dgrad_parity = on; }
// Branch overlap (default on): the three branches of SpellBertPho2ResArch3 that are independent between the inputs and the gate
// (models.py:816 bert, :818-827 pinyin GRU + pho_model, :829-838 glyph ResNet) - and their backward passes after the gate -
// run on three HIP streams (the caller's + two engine-owned ones), forked and joined with events inside one engine call.  The
// HBM-bound glyph kernels (BatchNorm passes, 64-channel convolutions) then fill the launch gaps / epilogue tails of the
// MFMA-bound BERT GEMMs and co-reside on the CUs next to them (tools/overlap_probe.py: -25 % of the glyph branch's time).
// Results are identical to the serial order (the branches touch disjoint tensors and scratch).
static int g_branch_overlap = 1;
void set_branch_overlap(int on) { g_branch_overlap = on; }
static int g_fwd_order = 0;
void set_fwd_order(int o) { g_fwd_order = o; }
// Priority classes of the engine-owned streams, applied when a stream is created (realise_set_engine keys 1..3, before the first
// forward): 0 = the device default, -1 = the highest priority the device offers, +1 = the lowest.  [0] pinyin branch, [1] glyph
// branch, [2] weight-gradient side stream.
static int g_skip_dead = 1;       // backward skips the rows of padding tokens: LayerNorm backward rows, blocks of the weight-gradient reductions (key 5;
                                  // 1: 16-row blocks in bf16, 2: whole 64-row tiles - the round-3 form, bit-identical to no skipping -, 0: off)
void set_skip_dead(int on) { g_skip_dead = on; }
static int g_cls_compact = 1;     // classifier backward over the rows that enter the loss only (realise_set_engine key 4)
void set_cls_compact(int on) { g_cls_compact = on; }
// Split-K of the classifier's data gradient (realise_set_engine key 6; bf16, compacted rows): K = 21184 vocabulary columns, N = 768,
// ~4.9 k live rows are 156 tiles of 128 x 192 on 512 workgroup slots - three K-ranges fill them (468), the fp32 partial planes are
// folded in plane order by the scatter that follows anyway.  0 = off (one launch over the whole K).
// K6 (realise_set_engine key 9): a GRU time step t > 0 as ONE launch - the recurrent projection with the gate math in its epilogue
// (bf16; gemm_nt8_gru).  0 = GEMM + gru_step_fwd.
static int g_gru_fuse = 1;
void set_gru_fuse(int on) { g_gru_fuse = on; }
static int g_cls_splitk = 3;
void set_cls_splitk(int n) { g_cls_splitk = n < 0 ? 0 : (n > 4 ? 4 : n); }
// Live rows (realise_set_engine key 10; bf16 training steps, needs the 16-row block lists of g_skip_dead = 1): the layer GEMMs of the
// three transformer stacks - forward AND data gradients - run over the live 16-row blocks of the batch only (gemm_nt8_live), the
// attention forward skips the query blocks and key rows beyond a sentence's last live row.  Rows after a sentence's last attended /
// loss position never reach the loss: no query attends to them (additive -10000 mask: their probabilities are exact fp32 zeros), the
// masked mean and the loss skip them, their gradient rows are exact zeros.  The reference computes them anyway; here their
// activations are simply not produced (the workspace rows keep old, finite values - the workspace is zero-filled when a plan is
// installed), the returned training logits of such rows are computed from those stale states and mean nothing, as the reference's
// mean nothing.  The loss, every live row's activations and every gradient are bit-identical to the dense pass (same kernels, same
// accumulation order per row; tests/test_round4_gpu.py).  Evaluation / inference forwards are always dense.
// Round 6, value 2 (DEFAULT): the list the layer GEMMs walk holds the live ROWS, not 16-row blocks (gemm_nt8_live, EpiParams::live_unit
// = 1): a GEMM tile is any 128 live rows.  The blocks that complete a sentence's last 16 rows cost 0.709 - 0.648 = 6 % of the batch's
// rows, and 42 instead of 46 tile rows put the 2304-wide qkv launch into ONE round of the 512 two-per-CU slots.  Every other consumer
// (LayerNorm, attention, the weight-gradient reductions) keeps the 16-row block tables: rows 16-row blocks hold beyond the live
// length are simply not produced by the GEMMs any more, and they are rows every consumer already treats as padding (row_live == 0).
// 1 = the round-4 / 5 form (16-row blocks), 0 = dense.
static int g_live_rows = 2;
void set_live_rows(int on) { g_live_rows = on; }
// K7 (realise_set_engine key 13, default 1; models.py:831-834): the glyph lookup `char_images_multifonts.index_select(0, ids)` is fused
// into the loaders of block 1's two forward convolutions - they gather the 3x3 / 1x1 taps straight from the NHWC glyph table through
// the list of distinct ids (ConvLoader::img_index: one index load per 8-row piece in the tile prologue, nothing in the K loop) - so
// the forward materialises no [U, 32, 32, 8] image batch.  A TRAINING step still needs the gathered images as the B operand of block
// 1's two weight-gradient reductions (an index load inside that kernel's K loop costs a full drain per fetch): they are
// gathered at the head of the backward, off the forward's path.  0 = gather_images in the forward, dense loaders (round 2-5 form).
static int g_glyph_fuse = 1;
void set_glyph_fuse(int on) { g_glyph_fuse = on; }
// K9, evaluation mode (realise_set_engine key 14): BatchNorm on running statistics applied in the convolutions' epilogues (resnet_forward)
static int g_bn_fold = 1;
void set_bn_fold(int on) { g_bn_fold = on; }
// realise_engine_adamw_pipelined runs as such (1, default; 2 / 3: diagnostics - every reader waits for the whole sweep / the sliced
// launches on the caller's stream) or as the plain sweep on the caller's stream (0): realise_set_engine key 15
static int g_opt_pipe = 1;
void set_opt_pipe(int on) { g_opt_pipe = on; }
static int g_stream_pri[3] = {0, 0, 0};
void set_stream_priority(int which, int pri) { if (which >= 0 && which < 3) g_stream_pri[which] = pri < 0 ? -1 : (pri > 0 ? 1 : 0); }
static hipError_t create_stream(hipStream_t* s, int which) {
  if (g_stream_pri[which] == 0) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  return hipStreamCreateWithPriority(s, hipStreamNonBlocking, g_stream_pri[which] < 0 ? greatest : least);
}

#define RL_TRY(expr) do { const int _rc = (expr); if (_rc != RL_OK) { fprintf(stderr, "[realise_hip] %s failed (%d) at %s:%d\n", #expr, _rc, __FILE__, __LINE__); return _rc; } } while (0)

static constexpr int64_t TN_SLAB_ELEMS = 16LL << 20;   // fp32 partial slabs of the split weight-gradient reductions (64 MiB)
static inline int64_t al256(int64_t x) { return (x + 255) & ~(int64_t)255; }
struct Bump {
  int64_t off = 0;
  int64_t take(int64_t bytes) { const int64_t o = off; off = al256(off + bytes); return o; }
};

static inline uint64_t splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

template <typename T> struct Engine : EngineBase {
  realise_config cfg;
  Variant vr;              // which branches this model has (layout.h: every branch decision reads this, not model_type)
  Layout L;
  float *P = nullptr, *G = nullptr, *PU = nullptr, *FZ = nullptr, *BF = nullptr;
  int64_t* BI = nullptr;
  char* sh = nullptr;      // shadow arena
  char* ws = nullptr;      // workspace
  int64_t ws_bytes = 0;
  int H, nh, I, V;
  int Vp;                  // V rounded up to 64: row pitch of dlogits and of the classifier's W^T shadow (128-byte aligned rows)

  // ---------------------------------------------------------------- shadows (offsets in bytes)
  struct LayerSh { int64_t qkv_w, qkv_wT, ao_w, ao_wT, in_w, in_wT, out_w, out_wT; };
  struct BlockSh { int64_t w1f, w1d, w1p, w2f, w2d, wsf, wsd; int cin_pad; };
  std::vector<LayerSh> sh_bert, sh_pho, sh_out;
  BlockSh sh_blk[TOWER_MAX_BLOCKS];      // the first L.tower.nblocks are in use
  int64_t sh_cls_w = 0, sh_cls_wT = 0, sh_gru_hh = 0, sh_gru_hhT = 0, sh_glyph = 0;
  int64_t sh_head_w = 0, sh_head_wT = 0;      // transform.dense of the MLM head (vr.mlm_head)
  int64_t sh_int_w = 0, sh_int_wT = 0;        // integrate of a concatenation model (vr.concat)
  int64_t shadow_total = 0;
  bool glyph_built = false, descs_built = false;
  int64_t sh_descs = 0, sh_fill = 0, sh_skip = 0;
  bool skip_built = false;
  static constexpr int ACHUNK_MAX = 8192, ACHUNK_LEN = 32768;
  std::vector<FillChunk> achunk_host;
  int n_achunks = 0;
  static constexpr int FILL_MAX = 2048;
  int n_descs = 0, desc_tiles = 0;
  std::vector<CastDesc> desc_host;

  // ---------------------------------------------------------------- workspace plan (byte offsets)
  struct LayerAct { int64_t qkv, lse, ctx, s1, rstd1, y1, pre, post, s2, rstd2, y2; };
  struct StackAct { int64_t emb_y, emb_xhat, emb_rstd; std::vector<LayerAct> layers; };
  struct BnAct { int64_t mean, rstd, scale, shift; };
  struct BlockAct { int64_t c1, h1, c2, cs, out; BnAct bn1, bn2, bns; int Hin, Hout, Pout; };
  struct Plan {
    int B = 0, S = 0, Tp = 0;
    int64_t total = 0;
    StackAct bert, pho, outb;
    BlockAct blk[TOWER_MAX_BLOCKS];
    int64_t mask_add, out_d, dlogits, count, loss_internal;
    int64_t cls_act, cls_inv, cls_nact, cls_xc, cls_gc, cls_slab;      // classifier backward over the rows that enter the loss only (stage_head)
    int64_t live_rows = 0;                // ascending list of the live rows (row-granular layer GEMMs)
    int64_t row_live, live_t64, live_t32, live_t16, live_n, live_rlen;          // padding rows: exact-zero gradient rows the backward skips (row_liveness)
    int64_t ids_clean = 0, pho_clean = 0;                 // range-checked copies of src_idx / pho_idx (sanitize_ids)
    int64_t gru_table, gru_hs, gru_rzn, gru_gh, gru_out;
    int64_t res_xhat, res_rstd, res_h, gate_mean, gate_msum, gate_g, fused;
    int64_t bn_sums, bn_slots;
    int64_t gu_first, gu_flag, gu_ids, gu_counts, gu_inv, gu_bounds, seg_acc, gu_dense;   // glyph dedup
    // backward: gA = the gradient that enters a stack; X1 / X2 / X3 = d bert / d pho / d res behind the fusion
    int64_t gA, X1, X2, X3, dz;
    // backward scratch of the three concurrent lanes: 0 = bert (+ head, output block), 1 = pho_model + GRU, 2 = glyph ResNet
    // (wC1 / wC2 / wD / wF: per-parity dY copies, tn_slab2: second slab - weight gradients on the side stream)
    struct Scratch { int64_t gB, gE, rowdot, tn_slab, tn_slab2, ln_slots, wC1[2], wC2[2], wD[2], wF[2]; } sc[3];
    std::vector<std::pair<int64_t, int64_t>> zero_once;      // (offset, bytes): self-cleaning accumulators, zero-filled when the plan is installed
    int64_t gru_dh, gru_dgi, gru_dgh, gru_onehot, gru_dtable;
    int64_t r_dout, r_dc2, r_dcs, r_dh1, r_dc1, r_dx;
    // MLM head (vr.mlm_head; taken last: no other offset moves): saved dense pre-activation, GELU output / LayerNorm xhat (in place), rstd,
    // LayerNorm output = the decoder's input; gathered head input rows, the fused backward's dz, the identity row map of the slab fold
    int64_t head_z = 0, head_x = 0, head_rstd = 0, head_y = 0, head_xc = 0, head_dz = 0, head_ident = 0;
  } pl;
  std::map<std::string, std::pair<int64_t, int64_t>> taps;   // name -> (byte offset, numel)

  // last forward
  realise_batch last;
  std::vector<int> last_alive;
  // weight-gradient overlap: the four wgrad GEMMs of a BERT layer run on an engine-owned side stream while the caller's
  // stream continues with the data-gradient chain (see layers_backward)
  hipStream_t side = nullptr;
  hipEvent_t ev_ready[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
  hipEvent_t ev_done[2] = {nullptr, nullptr};
  bool done_pending[2] = {false, false};
  int bw_layers = 0;
  bool side_ok() {
    if (side != nullptr) return true;
    if (create_stream(&side, 2) != hipSuccess) { side = nullptr; return false; }
    for (int p = 0; p < 2; ++p) {
      for (int k = 0; k < 4; ++k) (void)hipEventCreateWithFlags(&ev_ready[p][k], hipEventDisableTiming);
      (void)hipEventCreateWithFlags(&ev_done[p], hipEventDisableTiming);
    }
    return true;
  }
  int join_side(hipStream_t st) {
    for (int p = 0; p < 2; ++p)
      if (done_pending[p]) { if (hipStreamWaitEvent(st, ev_done[p], 0) != hipSuccess) return RL_ERR_LAUNCH; done_pending[p] = false; }
    return RL_OK;
  }
  ~Engine() override {
    if (bst[0] != nullptr) {
      for (int k = 0; k < 2; ++k) { (void)hipStreamSynchronize(bst[k]); (void)hipStreamDestroy(bst[k]); (void)hipEventDestroy(ev_join[k]); }
      (void)hipEventDestroy(ev_fork);
    }
    if (side != nullptr) {
      (void)hipStreamSynchronize(side);
      for (int p = 0; p < 2; ++p) { for (int k = 0; k < 4; ++k) (void)hipEventDestroy(ev_ready[p][k]); (void)hipEventDestroy(ev_done[p]); }
      (void)hipStreamDestroy(side);
    }
    for (hipEvent_t e : ev_sig) if (e != nullptr) (void)hipEventDestroy(e);
    if (ev_grads != nullptr) (void)hipEventDestroy(ev_grads);
    for (int k = 0; k < OPT_EV_MAX; ++k) if (ev_opt[k] != nullptr) (void)hipEventDestroy(ev_opt[k]);
    for (int k = 0; k < 2; ++k) if (ev_shadow[k] != nullptr) (void)hipEventDestroy(ev_shadow[k]);
  }
  // branch overlap: two engine-owned streams next to the caller's, fork / join events
  hipStream_t bst[2] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
  // What a backward helper enqueues with: a stream together with the scratch set and the pending LayerNorm folds that belong to it.
  // two_sets: the lane owns two dY buffer sets, so its layer weight gradients may go to the side stream (the bert lane only).
  struct Lane { hipStream_t st; const typename Plan::Scratch* sc; LnFoldSites* pend; bool two_sets; };
  Lane lane(int k, hipStream_t st) { return Lane{st, &pl.sc[k], &pend[k], k == 0}; }
  bool branches_ok() {
    if (bst[0] != nullptr) return true;
    for (int k = 0; k < 2; ++k)
      if (create_stream(&bst[k], k) != hipSuccess) { bst[0] = bst[1] = nullptr; return false; }
    (void)hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming);
    for (int k = 0; k < 2; ++k) (void)hipEventCreateWithFlags(&ev_join[k], hipEventDisableTiming);
    return true;
  }
  // the branch streams this model uses: bit 0 = bst[0] (pinyin branch), bit 1 = bst[1] (glyph branch); fork / join touch only those
  int branch_mask() const { return (vr.pho ? 1 : 0) | (vr.res ? 2 : 0); }
  int fork(hipStream_t st) {
    const int mask = branch_mask();
    if (mask == 0) return RL_OK;
    if (hipEventRecord(ev_fork, st) != hipSuccess) return RL_ERR_LAUNCH;
    for (int k = 0; k < 2; ++k) if ((mask >> k & 1) && hipStreamWaitEvent(bst[k], ev_fork, 0) != hipSuccess) return RL_ERR_LAUNCH;
    return RL_OK;
  }
  int join(hipStream_t st) {
    const int mask = branch_mask();
    for (int k = 0; k < 2; ++k)
      if ((mask >> k & 1) && (hipEventRecord(ev_join[k], bst[k]) != hipSuccess || hipStreamWaitEvent(st, ev_join[k], 0) != hipSuccess)) return RL_ERR_LAUNCH;
    return RL_OK;
  }
  const int32_t* alive_dev = nullptr;      // device-side n_alive[Tp] of the last batch (nullptr: host counts)
  bool have_fwd = false;
  bool dead_ok = false;                    // the last forward produced the row-liveness tables (training batch, B * S % 64 == 0)
  const uint8_t* live_rows() const { return dead_ok ? wp<uint8_t>(pl.row_live) : nullptr; }
  bool live16() const { return sizeof(T) == 2 && g_skip_dead == 1; }
  const int* live_tiles() const { return dead_ok ? wp<int>(sizeof(T) == 2 ? (live16() ? pl.live_t16 : pl.live_t64) : pl.live_t32) : nullptr; }
  const int* live_tile_count() const { return dead_ok ? wp<int>(pl.live_n) + (sizeof(T) == 2 ? (live16() ? 2 : 0) : 1) : nullptr; }
  int live_list_rows() const { return sizeof(T) == 2 ? (live16() ? 16 : 64) : 32; }
  bool rows_live = false;                  // the last forward ran its layer GEMMs over the live 16-row blocks (g_live_rows); the backward follows
  // a layer GEMM over the token rows: the live blocks of a live-row step (no dense fall-back: the dead rows of its operands are stale)
  // whole_blocks: the output is the dY operand of a weight-gradient reduction, which walks whole live 16-row BLOCKS - its rows behind a
  // sentence's last live row inside such a block must be (re)computed (exact zeros: their dY inputs are LayerNorm-backward zeros), not
  // left stale, so that launch keeps the block list (the GELU' data gradient of BertOutput, one of a layer's eight GEMMs).
  int nt_rows(hipStream_t st, const T* A, int64_t lda, const T* B, int64_t ldb, int M, int N, int K, const EpiParams<T>& ep, bool whole_blocks = false) {
    if constexpr (sizeof(T) == 2) {
      EpiParams<T> e2 = ep;
      if (rows_live && g_live_rows == 2 && !whole_blocks) { e2.live_list = wp<int>(pl.live_rows); e2.live_count = wp<int>(pl.live_n) + 3; e2.live_unit = 1; }
      else if (rows_live) { e2.live_list = wp<int>(pl.live_t16); e2.live_count = wp<int>(pl.live_n) + 2; }
      if (rows_live) return gemm_nt8_live(st, A, lda, B, ldb, M, N, K, e2);
    }
    return gemm_nt<T>(st, A, lda, B, ldb, M, N, K, ep);
  }
  // bf16x3 (realise_config.dtype == REALISE_F32_BF16X3: this engine is the float one with the flag set).  Every dense-loader GEMM the
  // engine issues is written gemm_nt<U>(...) / gemm_tn<U>(...) / gemm_tn_group<U>(...): inside the class those names are THESE members,
  // which hand the call to the launcher of gemm.h with the flag filled in - the one place it is set.  The gathered (ConvLoader) GEMMs,
  // attention and the 8-wave kernels are other functions and stay as they are.
  int x3() const { return cfg.dtype == REALISE_F32_BF16X3 ? 1 : 0; }
  template <typename U>
  int gemm_nt(hipStream_t st, const U* A, int64_t lda, const U* B, int64_t ldb, int M, int N, int K, EpiParams<U> ep, const int* rows_dev = nullptr) {
    if constexpr (sizeof(U) == 4) ep.x3 = x3();
    return rl::gemm_nt<U>(st, A, lda, B, ldb, M, N, K, ep, rows_dev);
  }
  template <typename U>
  int gemm_tn(hipStream_t st, const U* A, int64_t lda, const U* B, int64_t ldb, int P_, int I_, int J_, TnEpi ep, const int* rows_dev = nullptr) {
    if constexpr (sizeof(U) == 4) ep.x3 = x3();
    return rl::gemm_tn<U>(st, A, lda, B, ldb, P_, I_, J_, ep, rows_dev);
  }
  template <typename U>
  int gemm_tn_group(hipStream_t st, int n, const TnGroupProblem<U>* probs, int P_, float alpha, int overwrite, const int* tile_list,
                    const int* n_tiles, int list_rows) {
    return rl::gemm_tn_group<U>(st, n, probs, P_, alpha, overwrite, tile_list, n_tiles, list_rows, sizeof(U) == 4 ? x3() : 0);
  }
  const int* live_rlen() const { return dead_ok ? wp<int>(pl.live_rlen) : nullptr; }
  // What the last forward's head left for stage_head, its only record of that forward: reset at the top of forward(), filled on every
  // exit a backward may follow.
  struct HeadSaved {
    bool compact = false;                  // the gradient rows (pl.dlogits) are the compacted loss rows (pl.cls_act / cls_inv / cls_nact)
    const T* dec_in = nullptr;             // the classifier's (MLM head: the decoder's) input rows as its weight gradient reads them
    const T* head_in = nullptr;            // MLM head: the transform's input rows as its weight gradient reads them
    const int* row_map = nullptr;          // MLM head: compacted row r = saved row row_map[r] of head_z / head_x / head_rstd (null: identity)
  } hs;

  template <typename U> U* wp(int64_t off) const { return (U*)(ws + off); }
  template <typename U> U* sp(int64_t off) const { return (U*)(sh + off); }
  const float* pp(int64_t off) const { return P + off; }
  float* gp(int64_t off) const { return G + off; }

  Engine(const realise_config& c, float* p, float* g, float* pu, float* fz, float* bf, int64_t* bi)
      : cfg(c), vr(variant_of(c)), L(build_layout(c)), P(p), G(g), PU(pu), FZ(fz), BF(bf), BI(bi) {
    H = c.hidden; nh = c.heads; I = c.intermediate; V = c.vocab; Vp = (V + 63) & ~63;
    plan_shadows();
  }

  static int pad8(int c) { return (c + 7) & ~7; }

  void plan_shadows() {
    Bump b;
    const int64_t e = sizeof(T);
    auto plan_stack = [&](std::vector<LayerSh>& v, int n) {
      v.resize(n);
      for (int l = 0; l < n; ++l) {
        v[l].qkv_w = b.take(3LL * H * H * e); v[l].qkv_wT = b.take(3LL * H * H * e);
        v[l].ao_w = b.take((int64_t)H * H * e); v[l].ao_wT = b.take((int64_t)H * H * e);
        v[l].in_w = b.take((int64_t)I * H * e); v[l].in_wT = b.take((int64_t)I * H * e);
        v[l].out_w = b.take((int64_t)I * H * e); v[l].out_wT = b.take((int64_t)I * H * e);
      }
    };
    plan_stack(sh_bert, vr.bert ? cfg.bert_layers : 0);
    sh_cls_w = b.take((int64_t)V * H * e);
    sh_cls_wT = b.take((int64_t)Vp * H * e);      // [H][Vp], columns >= V stay zero (the shadow arena is zero-initialised)
    if (vr.pho) plan_stack(sh_pho, cfg.pho_layers);
    if (vr.arch) plan_stack(sh_out, cfg.out_layers);
    if (vr.pho) {
      sh_gru_hh = b.take(3LL * H * H * e);
      sh_gru_hhT = b.take(3LL * H * H * e);
    }
    if (vr.res) {
      for (int k = 0; k < L.tower.nblocks; ++k) {
        const BlockOff& o = L.blocks[k];
        BlockSh& s = sh_blk[k];
        s.cin_pad = pad8(o.cin);
        s.w1f = b.take((int64_t)o.cout * 9 * s.cin_pad * e);
        s.w1d = b.take((int64_t)s.cin_pad * 9 * o.cout * e);
        s.w1p = b.take((int64_t)s.cin_pad * 9 * o.cout * e);
        s.w2f = b.take((int64_t)o.cout * 9 * o.cout * e);
        s.w2d = b.take((int64_t)o.cout * 9 * o.cout * e);
        s.wsf = b.take((int64_t)o.cout * s.cin_pad * e);
        s.wsd = b.take((int64_t)s.cin_pad * o.cout * e);
      }
      const int gs = cfg.glyph_size;
      sh_glyph = b.take((int64_t)V * gs * gs * 8 * e);
    }
    sh_descs = b.take(256 * (int64_t)sizeof(CastDesc));      // device table for the one-launch refresh of the Linear weights
    sh_fill = b.take(FILL_MAX * (int64_t)sizeof(FillChunk));  // chunk table of the fresh-gradient zero fill
    sh_skip = b.take(ACHUNK_MAX * (int64_t)sizeof(FillChunk));   // chunk list of the parameters the tiled AdamW does NOT own (adamw_step)
    if (vr.mlm_head) { sh_head_w = b.take((int64_t)H * H * e); sh_head_wT = b.take((int64_t)H * H * e); }      // (last: every other offset stays put)
    if (vr.concat) { sh_int_w = b.take((int64_t)vr.nsrc * H * H * e); sh_int_wT = b.take((int64_t)vr.nsrc * H * H * e); }      // integrate [H][nH] and its transpose [nH][H]
    shadow_total = b.off;
  }

  int64_t shadow_bytes() const override { return shadow_total; }

  // descriptor table of the Linear weights -> (W, W^T) operand copies: group A = the bert stack (what the forward needs first), group
  // B = classifier, pinyin / output stacks, GRU; tile ids restart per group (one launch each)
  int ensure_descs(hipStream_t st) {
    if (descs_built) return RL_OK;
    std::vector<CastDesc>& d = desc_host;       // member: stays alive while the async upload is in flight
    d.clear();
    int tiles = 0;
    auto add = [&](int64_t src, int R, int C, int64_t dst, int64_t dstT, int ldT = 0) {
      CastDesc x;
      x.src = pp(src); x.dst = sp<T>(dst); x.dstT = sp<T>(dstT); x.R = R; x.C = C; x.ldT = ldT > 0 ? ldT : R;
      x.tile_begin = tiles; x.tiles_c = (C + 63) / 64;
      tiles += x.tiles_c * ((R + 63) / 64);
      d.push_back(x);
    };
    auto add_stack = [&](const StackOff& so, const std::vector<LayerSh>& v) {
      for (size_t l = 0; l < v.size(); ++l) {
        const LayerOff& o = so.layers[l];
        add(o.qkv_w, 3 * H, H, v[l].qkv_w, v[l].qkv_wT);
        add(o.ao_w, H, H, v[l].ao_w, v[l].ao_wT);
        add(o.in_w, I, H, v[l].in_w, v[l].in_wT);
        add(o.out_w, H, I, v[l].out_w, v[l].out_wT);
      }
    };
    add_stack(L.bert, sh_bert);
    n_descs_a = (int)d.size(); desc_tiles_a = tiles;
    tiles = 0;                                   // second group: its own launch, tile ids restart
    add(L.cls_w, V, H, sh_cls_w, sh_cls_wT, Vp);
    if (vr.mlm_head) add(L.head_w, H, H, sh_head_w, sh_head_wT);      // next to its decoder: the pipelined sweep steps the two in one piece
    if (vr.pho) add_stack(L.pho, sh_pho);
    if (vr.arch) add_stack(L.outb, sh_out);
    if (vr.pho) add(L.gru_w_hh, 3 * H, H, sh_gru_hh, sh_gru_hhT);
    if (vr.concat) add(L.int_w, H, vr.nsrc * H, sh_int_w, sh_int_wT);      // (in the piece of the pinyin / output stacks: the forward meets it at the fusion)
    if (d.size() > 256) return RL_ERR_ARG;
    if (hipMemcpyAsync(sh + sh_descs, d.data(), d.size() * sizeof(CastDesc), hipMemcpyHostToDevice, st) != hipSuccess) return RL_ERR_LAUNCH;
    n_descs = (int)d.size(); desc_tiles = tiles; descs_built = true;
    return RL_OK;
  }
  int refresh_shadows(hipStream_t st) override { return refresh_shadows_ex(st, 0); }
  // skip_linear != 0: the Linear weights' copies are current (adamw_step wrote them from the values it stored); only the conv-weight
  // copies (and the glyph table's image when it changed) are re-derived
  int refresh_shadows_ex(hipStream_t st, int skip_linear) override {
    if (!sh) return RL_ERR_ARG;
    RL_TRY(ensure_descs(st));
    // a pipelined optimizer sweep (adamw_step): the convolution weights this call reads are in its first piece; a full refresh reads everything
    RL_TRY(wait_opt(st, skip_linear ? 0 : -1));
    if (!skip_linear) opt_pending = false;
    // Three independent pieces on three streams (when the branch streams exist): the bert stack's copies on the caller's stream -
    // the forward that follows needs nothing else for its first 12 layers -, classifier + pinyin / output stacks + GRU on the pinyin
    // stream, the conv-weight launch (+ the glyph table when it changed) on the glyph stream, where the glyph branch of the
    // forward queues up behind it by itself.  ev_shadow[k] orders any OTHER consumer (a forward without branch streams, the
    // glyph-only entry points): wait_shadows().
    // (the ablation model: a stream only for a branch that exists - without the pinyin branch the second group goes on the caller's stream)
    const bool ovl = vr.arch && branch_mask() != 0 && g_branch_overlap && branches_ok() && shadow_events_ok();
    hipStream_t s_b = ovl && vr.pho ? bst[0] : st, s_c = ovl && vr.res ? bst[1] : st;
    if (ovl) RL_TRY(fork(st));
    const CastDesc* dd = (const CastDesc*)(sh + sh_descs);
    if (!skip_linear) {
      if (n_descs_a > 0) RL_TRY(cast_transpose_multi<T>(st, dd, n_descs_a, desc_tiles_a));
      RL_TRY(cast_transpose_multi<T>(s_b, dd + n_descs_a, n_descs - n_descs_a, desc_tiles));
    }
    if (vr.res) {
      ConvShadowDescs cd;
      auto addc = [&](const float* w, int Co, int Ci, int KHW, int Cpad, T* fwd, T* dgrad, const TapOrder& ord = TapOrder()) {
        ConvShadowDesc& x = cd.d[cd.n++];
        x.w = w; x.fwd = fwd; x.dgrad = dgrad; x.Co = Co; x.Ci = Ci; x.KHW = KHW; x.Cpad = Cpad; x.CiRows = Cpad; x.block_begin = 0; x.order = ord;
      };
      for (int k = 0; k < L.tower.nblocks; ++k) {
        const BlockOff& o = L.blocks[k];
        const BlockSh& s = sh_blk[k];
        addc(pp(o.w1), o.cout, o.cin, 9, s.cin_pad, sp<T>(s.w1f), sp<T>(s.w1d));
        {   // second data-gradient copy of the stride-2 conv with its taps stored parity class by parity class
          TapOrder ord; ord.n = 9; int first = 0;
          (void)conv_s2_class(3, 3, 1, 0, &first, ord.t);
          addc(pp(o.w1), o.cout, o.cin, 9, s.cin_pad, (T*)nullptr, sp<T>(s.w1p), ord);
        }
        addc(pp(o.w2), o.cout, o.cout, 9, o.cout, sp<T>(s.w2f), sp<T>(s.w2d));
        addc(pp(o.ws), o.cout, o.cin, 1, s.cin_pad, sp<T>(s.wsf), sp<T>(s.wsd));
      }
      RL_TRY(conv_weight_shadow_multi<T>(s_c, cd));
      // the glyph table is frozen (requires_grad=False, models.py:679): its NHWC image is rebuilt only after
      // invalidate_frozen() (load_state_dict / build_glyce_embed*)
      if (!glyph_built) {
        RL_TRY(glyph_shadow<T>(s_c, FZ + L.glyph, V, cfg.num_fonts, cfg.glyph_size * cfg.glyph_size, 8, sp<T>(sh_glyph)));
        glyph_built = true;
      }
    }
    shadows_pending = false;
    if (ovl) {
      for (int k = 0; k < 2; ++k) if ((branch_mask() >> k & 1) && hipEventRecord(ev_shadow[k], bst[k]) != hipSuccess) return RL_ERR_LAUNCH;
      shadows_pending = true;
    }
    return RL_OK;
  }
  // FusedAdamW's step as the engine runs it: the Linear weights (90 % of the parameters) in the tiles of the operand-copy kernel,
  // which stores the new fp32 value AND its compute-dtype W / W^T copies in the same pass; everything else by the flat grouped
  // kernel, told by a byte per 64 parameters what the tiled launches own.  The next forward then calls refresh_shadows_ex(st, 1).
  // ---- pipelined form (round 6, realise_engine_adamw_pipelined).  The sweep is 1.1 ms of pure HBM streaming (32 B per parameter) that
  // nothing could overlap while it sat between the backward and the next forward on the caller's stream.  Here it runs on the
  // engine's side stream in the order the next forward consumes the parameters - everything outside the Linear weights (biases,
  // LayerNorm, embeddings, convolution weights), the tied word table / classifier, BERT layers 0-1 | layers 2-3 | pinyin stack +
  // output stack + GRU | the remaining BERT layers two by two - with an event behind every piece, and the forward (and
  // refresh_shadows_ex) waits for a piece right in front of its first reader: the caller's stream is held for ~0.3 ms instead of the
  // whole sweep, the rest streams under the first layers of the forward.  Same kernels, same arithmetic per element: same bits.
  // Contract: between this call and the next forward / realise_engine_sync_optimizer nothing else may touch parameters, gradients or
  // moments (the module opts in per loop: pipeline_optimizer).
  static constexpr int OPT_EV_MAX = 16;
  hipEvent_t ev_opt[OPT_EV_MAX] = {}; hipEvent_t ev_grads = nullptr;
  int opt_groups = 0;                      // bert layer groups of the pending sweep: events 0 .. opt_groups - 1, event opt_groups = the other stacks
  bool opt_pending = false;
  bool opt_events_ok() {
    if (ev_grads != nullptr) return true;
    if (hipEventCreateWithFlags(&ev_grads, hipEventDisableTiming) != hipSuccess) { ev_grads = nullptr; return false; }
    for (int k = 0; k < OPT_EV_MAX; ++k)
      if (hipEventCreateWithFlags(&ev_opt[k], hipEventDisableTiming) != hipSuccess) return false;
    return true;
  }
  // order stream s behind piece k of the pending sweep (k < 0: behind all of it)
  int wait_opt(hipStream_t s, int k) {
    if (!opt_pending) return RL_OK;
    if (g_opt_pipe >= 2) k = -1;             // (diagnostics: every reader waits for the whole sweep)
    const int lo = k < 0 ? 0 : std::min(k, opt_groups), hi = k < 0 ? opt_groups : lo;
    for (int i = lo; i <= hi; ++i) if (hipStreamWaitEvent(s, ev_opt[i], 0) != hipSuccess) return RL_ERR_LAUNCH;
    return RL_OK;
  }
  int sync_optimizer(hipStream_t st) override {
    RL_TRY(wait_opt(st, -1));
    opt_pending = false;
    return RL_OK;
  }
  int adamw_step(hipStream_t st, float* m, float* v, const uint8_t* group_of_block, const AdamwGroups& gs, const float* norm_sq,
                 float max_norm, int pipelined) override {
    if (!sh || !m || !v || !group_of_block) return RL_ERR_ARG;
    RL_TRY(ensure_descs(st));
    const int64_t n = L.arena_elems[AR_TRAIN];
    if (!skip_built) {
      // everything outside the Linear weights, as chunks of at most ACHUNK_LEN floats (all boundaries are multiples of 64 elements)
      std::vector<std::pair<int64_t, int64_t>> own;
      for (const CastDesc& d : desc_host) {
        const int64_t off = d.src - P, cnt = (int64_t)d.R * d.C;
        if ((off % 64) != 0 || (cnt % 64) != 0 || (d.C % 4) != 0) return RL_ERR_ARG;
        own.push_back({off, off + cnt});
      }
      std::sort(own.begin(), own.end());
      achunk_host.clear();
      int64_t at = 0;
      auto emit = [&](int64_t b, int64_t e) {
        for (int64_t o = b; o < e; o += ACHUNK_LEN) achunk_host.push_back(FillChunk{o, (int32_t)std::min<int64_t>(ACHUNK_LEN, e - o), 0});
      };
      for (auto& r : own) { if (r.first > at) emit(at, r.first); at = std::max(at, r.second); }
      if (at < n) emit(at, n);
      if ((int)achunk_host.size() > ACHUNK_MAX) return RL_ERR_ARG;
      if (!achunk_host.empty() &&
          hipMemcpyAsync(sh + sh_skip, achunk_host.data(), achunk_host.size() * sizeof(FillChunk), hipMemcpyHostToDevice, st) != hipSuccess) return RL_ERR_LAUNCH;
      n_achunks = (int)achunk_host.size();
      skip_built = true;
    }
    RL_TRY(wait_shadows(st));           // (the previous refresh may still be writing the copies on the branch streams)
    const CastDesc* dd = (const CastDesc*)(sh + sh_descs);
    RL_TRY(sync_optimizer(st));         // (a pipelined sweep nobody waited for: two steps without a forward in between)
    const int Lb = (int)sh_bert.size();
    if (pipelined && g_opt_pipe && side_ok() && opt_events_ok() && (Lb + 1) / 2 + 1 <= OPT_EV_MAX && n_descs_a == 4 * Lb) {
      RL_TRY(join_side(st));
      hipStream_t side = g_opt_pipe == 3 ? st : this->side;      // (diagnostics, 3: the sliced launches on the caller's stream)
      if (hipEventRecord(ev_grads, st) != hipSuccess || hipStreamWaitEvent(side, ev_grads, 0) != hipSuccess) return RL_ERR_LAUNCH;
      auto tile_begin = [&](int i, bool group_b) -> int {      // descriptor i of group A (0 .. n_descs_a) / B (0 .. n_descs - n_descs_a); the end = the group's tile count
        if (!group_b) return i < n_descs_a ? desc_host[i].tile_begin : desc_tiles_a;
        return n_descs_a + i < n_descs ? desc_host[n_descs_a + i].tile_begin : desc_tiles;
      };
      auto bert_layers = [&](int l0, int l1) -> int {          // the Linear weights of BERT layers [l0, l1)
        const int a = 4 * l0, b = 4 * std::min(l1, Lb);
        if (b <= a) return RL_OK;
        return adamw_cast_multi<T>(side, dd + a, b - a, tile_begin(b, false) - tile_begin(a, false), P, G, m, v, group_of_block, gs, norm_sq, max_norm, tile_begin(a, false));
      };
      const int nb = n_descs - n_descs_a;                      // group B: [0] = tied word table / classifier, then pinyin / output stacks, GRU
      const int nc = vr.mlm_head ? 2 : 1;                      // the classifier's piece: [0], and with an MLM head [1] = its transform.dense
      opt_groups = (Lb + 1) / 2;
      RL_TRY(adamw_chunks(side, P, G, m, v, (const FillChunk*)(sh + sh_skip), n_achunks, group_of_block, gs, norm_sq, max_norm));
      RL_TRY(adamw_cast_multi<T>(side, dd + n_descs_a, nc, tile_begin(nc, true), P, G, m, v, group_of_block, gs, norm_sq, max_norm, 0));
      RL_TRY(bert_layers(0, 2));
      if (hipEventRecord(ev_opt[0], side) != hipSuccess) return RL_ERR_LAUNCH;
      for (int g = 1; g < opt_groups; ++g) {
        RL_TRY(bert_layers(2 * g, 2 * g + 2));
        if (hipEventRecord(ev_opt[g], side) != hipSuccess) return RL_ERR_LAUNCH;
        if (g == 1 && nb > nc) {
          RL_TRY(adamw_cast_multi<T>(side, dd + n_descs_a + nc, nb - nc, desc_tiles - tile_begin(nc, true), P, G, m, v, group_of_block, gs, norm_sq, max_norm, tile_begin(nc, true)));
          if (hipEventRecord(ev_opt[opt_groups], side) != hipSuccess) return RL_ERR_LAUNCH;
        }
      }
      if (opt_groups < 2 || nb <= nc) {                         // (a one- or two-layer stack, or no other stacks: the last event still has to exist)
        if (opt_groups < 2 && nb > nc)
          RL_TRY(adamw_cast_multi<T>(side, dd + n_descs_a + nc, nb - nc, desc_tiles - tile_begin(nc, true), P, G, m, v, group_of_block, gs, norm_sq, max_norm, tile_begin(nc, true)));
        if (hipEventRecord(ev_opt[opt_groups], side) != hipSuccess) return RL_ERR_LAUNCH;
      }
      opt_pending = true;
      return RL_OK;
    }
    if (n_descs_a > 0) RL_TRY(adamw_cast_multi<T>(st, dd, n_descs_a, desc_tiles_a, P, G, m, v, group_of_block, gs, norm_sq, max_norm));
    RL_TRY(adamw_cast_multi<T>(st, dd + n_descs_a, n_descs - n_descs_a, desc_tiles, P, G, m, v, group_of_block, gs, norm_sq, max_norm));
    return adamw_chunks(st, P, G, m, v, (const FillChunk*)(sh + sh_skip), n_achunks, group_of_block, gs, norm_sq, max_norm);
  }
  // operand copies refreshed on the branch streams: order `s` behind them (no-op when they ran on the caller's stream)
  hipEvent_t ev_shadow[2] = {nullptr, nullptr};
  bool shadows_pending = false;
  int n_descs_a = 0, desc_tiles_a = 0;
  bool shadow_events_ok() {
    for (int k = 0; k < 2; ++k)
      if (ev_shadow[k] == nullptr && hipEventCreateWithFlags(&ev_shadow[k], hipEventDisableTiming) != hipSuccess) return false;
    return true;
  }
  int wait_shadows(hipStream_t s) {
    if (!shadows_pending) return RL_OK;
    for (int k = 0; k < 2; ++k) if ((branch_mask() >> k & 1) && hipStreamWaitEvent(s, ev_shadow[k], 0) != hipSuccess) return RL_ERR_LAUNCH;
    return RL_OK;
  }

  // ---------------------------------------------------------------- workspace planning
  void tap(const std::string& name, int64_t off, int64_t numel) { taps[name] = {off, numel}; }

  // Tp < 0: glyph-only plan (BASELINE configs[3]: the CharResNet alone on B*S glyph stacks) - no BERT stacks, no logits
  Plan make_plan(int B, int S, int Tp) {
    Plan p;
    const bool glyph_only = Tp < 0;
    p.B = B; p.S = S; p.Tp = Tp;
    Bump b;
    const int64_t e = sizeof(T), Tk = (int64_t)B * S;
    taps.clear();
    auto plan_stack = [&](StackAct& a, int n, const std::string& name) {
      a.emb_y = b.take(Tk * H * e); a.emb_xhat = b.take(Tk * H * e); a.emb_rstd = b.take(Tk * 4);
      tap(name + ".emb", a.emb_y, Tk * H);
      a.layers.resize(n);
      for (int l = 0; l < n; ++l) {
        LayerAct& x = a.layers[l];
        x.qkv = b.take(Tk * 3 * H * e); x.lse = b.take((int64_t)B * nh * S * 4); x.ctx = b.take(Tk * H * e);
        x.s1 = b.take(Tk * H * e); x.rstd1 = b.take(Tk * 4); x.y1 = b.take(Tk * H * e);
        x.pre = b.take(Tk * I * e); x.post = b.take(Tk * I * e);
        x.s2 = b.take(Tk * H * e); x.rstd2 = b.take(Tk * 4); x.y2 = b.take(Tk * H * e);
        const std::string ln = name + ".layer." + std::to_string(l);
        tap(ln + ".qkv", x.qkv, Tk * 3 * H); tap(ln + ".ctx", x.ctx, Tk * H); tap(ln + ".attn_out", x.y1, Tk * H);
        tap(ln + ".inter", x.post, Tk * I); tap(ln + ".out", x.y2, Tk * H);
        tap(ln + ".sum1", x.s1, Tk * H); tap(ln + ".sum2", x.s2, Tk * H);      // (pre-LayerNorm sums; after a training forward: their xhat)
      }
    };
    p.mask_add = b.take(Tk * 4);
    p.ids_clean = b.take(Tk * 8);
    p.pho_clean = (!glyph_only && vr.pho) ? b.take(Tk * (int64_t)(Tp > 0 ? Tp : 1) * 8) : 0;
    if (!glyph_only) {
      if (vr.bert) plan_stack(p.bert, cfg.bert_layers, "bert");
      p.out_d = b.take(Tk * H * e);
      p.dlogits = b.take(Tk * Vp * e);
      tap("dlogits", p.dlogits, Tk * Vp);
      p.zero_once.push_back({p.dlogits, Tk * Vp * e});      // compacted gradient rows: the rows beyond the live count hold old (finite) values
    }
    p.count = b.take(256);
    p.loss_internal = b.take(Tk * 4 + 256);       // per-row loss terms (ordered fold: reproducible loss)
    p.cls_act = b.take(Tk * 4); p.cls_inv = b.take(Tk * 4); p.cls_nact = b.take(256);
    p.row_live = b.take(Tk + 64); p.live_t64 = b.take((Tk / 32 + 2) * 4); p.live_t32 = b.take((Tk / 32 + 2) * 4); p.live_t16 = b.take((Tk / 16 + 4) * 4); p.live_n = b.take(256); p.live_rlen = b.take(B * 4 + 64); p.live_rows = b.take((Tk + 128) * 4);
    p.cls_xc = b.take(Tk * H * e); p.cls_gc = b.take(Tk * H * e);
    p.zero_once.push_back({p.cls_xc, Tk * H * e}); p.zero_once.push_back({p.cls_gc, Tk * H * e});
    p.cls_slab = (!glyph_only && sizeof(T) == 2) ? b.take(4 * Tk * H * 4) : 0;      // fp32 planes of the split-K classifier data gradient
    // Backward scratch.  gA is the gradient that enters a stack; everything else is per lane (Plan::sc).  What a lane's set holds:
    //   SET_TWO   (the bert lane, and every stage of a serial pass): gB / gE / rowdot, two slabs and TWO sets of a layer's four dY
    //             matrices - operands of the deferred weight gradients: they live in the buffer set of the layer's parity until the
    //             side stream has consumed them
    //   SET_ONE   (the pinyin lane: its layers run next to the bert layers): the same with ONE dY set and one slab, named by both parities
    //   SET_GLYPH (the glyph lane): LayerNorm-backward output, slabs of the conv weight gradients, fold slots; the rest shared with set 0
    // The takes of a kind come in the order the workspace has always had them (it differs between the kinds): every offset stays put.
    const int64_t Tw = glyph_only ? 1 : Tk;               // the wide BERT scratch is not needed by the glyph-only plan
    enum { SET_TWO, SET_ONE, SET_GLYPH };
    auto take_scratch = [&](typename Plan::Scratch& s, int kind) {
      auto hid = [&](int64_t rows) { return b.take(rows * H * e); };
      auto rowdot = [&]() { return b.take((int64_t)B * nh * S * 4); };
      auto slab = [&]() { return b.take(TN_SLAB_ELEMS * 4); };
      auto slots = [&]() { return b.take((int64_t)(LN_FOLD_MAX + 1) * LN_SLOT_BYTES); };     // LN_FOLD_MAX deferred sites + one immediate region
      if (kind == SET_TWO) {
        s.gB = hid(Tk); s.wC1[0] = hid(Tk); s.gE = hid(Tk); s.wD[0] = b.take(Tw * I * e); s.wF[0] = b.take(Tw * 3 * H * e); s.rowdot = rowdot();
        s.wC2[0] = hid(Tw); s.wC1[1] = hid(Tw); s.wC2[1] = hid(Tw); s.wD[1] = b.take(Tw * I * e); s.wF[1] = b.take(Tw * 3 * H * e);
        s.tn_slab2 = slab(); s.tn_slab = slab(); s.ln_slots = slots();
      } else if (kind == SET_ONE) {
        s.gB = hid(Tk); s.gE = hid(Tk); s.rowdot = rowdot(); s.tn_slab = s.tn_slab2 = slab(); s.ln_slots = slots();
        s.wC1[0] = s.wC1[1] = hid(Tk); s.wC2[0] = s.wC2[1] = hid(Tk); s.wD[0] = s.wD[1] = b.take(Tk * I * e); s.wF[0] = s.wF[1] = b.take(Tk * 3 * H * e);
      } else {
        s.gE = hid(Tk); s.tn_slab = slab(); s.ln_slots = slots();
      }
    };
    p.gA = b.take(Tk * H * e);
    take_scratch(p.sc[0], SET_TWO);
    tap("d_x0", p.sc[0].gB, Tk * H);
    p.sc[1] = p.sc[2] = p.sc[0];                          // (a lane this model does not have, and what the glyph lane shares)
    if (vr.arch && vr.pho && !glyph_only) take_scratch(p.sc[1], SET_ONE);
    if (vr.arch && vr.res) take_scratch(p.sc[2], SET_GLYPH);
    if (vr.arch) {
      if (!glyph_only) {
        if (vr.pho) plan_stack(p.pho, cfg.pho_layers, "pho_model");
        plan_stack(p.outb, cfg.out_layers, "output_block");
        if (vr.pho) {
          p.gru_table = b.take(64LL * 3 * H * 4);
          p.gru_hs = b.take((int64_t)Tp * Tk * H * e);
          p.gru_rzn = b.take((int64_t)Tp * Tk * 3 * H * e);
          p.gru_gh = b.take((int64_t)Tp * Tk * 3 * H * e);
          p.gru_out = b.take(Tk * H * e);
          tap("pho_gru", p.gru_out, Tk * H);
        }
      }
      if (vr.res) {
      int hin = cfg.glyph_size;
      for (int k = 0; k < L.tower.nblocks; ++k) {
        BlockAct& a = p.blk[k];
        const int C = L.blocks[k].cout;
        a.Hin = hin; a.Hout = hin / 2; a.Pout = (int)(Tk * a.Hout * a.Hout);
        const int64_t n = (int64_t)a.Pout * C * e;
        a.c1 = b.take(n); a.h1 = b.take(n); a.c2 = b.take(n); a.cs = b.take(n); a.out = b.take(n);
        for (BnAct* q : {&a.bn1, &a.bn2, &a.bns}) {
          q->mean = b.take(C * 4); q->rstd = b.take(C * 4); q->scale = b.take(C * 4); q->shift = b.take(C * 4);
        }
        tap("resnet.block" + std::to_string(k + 1), a.out, (int64_t)a.Pout * C);
        tap("resnet.block" + std::to_string(k + 1) + ".h1", a.h1, (int64_t)a.Pout * C);
        hin = a.Hout;
      }
      p.bn_sums = b.take(2 * 1024 * 4);
      p.bn_slots = b.take((int64_t)COL_SLOT_BYTES);
      p.gu_first = b.take((int64_t)V * 4); p.gu_flag = b.take(Tk * 4); p.gu_ids = b.take(Tk * 8); p.gu_counts = b.take(Tk * 4);
      p.gu_inv = b.take(Tk * 4); p.gu_bounds = b.take(64); p.seg_acc = b.take(Tk * H * 4);
      p.gu_dense = b.take(Tk * (int64_t)cfg.glyph_size * cfg.glyph_size * 8 * e);      // the distinct glyph images, contiguous (NHWC, 8 channels)
      tap("glyph.bounds", p.gu_bounds, 64 / (int64_t)sizeof(T)); tap("glyph.inv", p.gu_inv, Tk * 4 / (int64_t)sizeof(T));
      tap("glyph.counts", p.gu_counts, Tk * 4 / (int64_t)sizeof(T)); tap("glyph.ids", p.gu_ids, Tk * 8 / (int64_t)sizeof(T));
      p.res_xhat = b.take(Tk * H * e); p.res_rstd = b.take(Tk * 4); p.res_h = b.take(Tk * H * e);
      tap("res_h", p.res_h, Tk * H);
      }
      if (vr.gate) {
        p.gate_mean = b.take((int64_t)B * H * 4); p.gate_msum = b.take(B * 4 + 256); p.gate_g = b.take(Tk * 16);
        tap("gate.g", p.gate_g, Tk * 16 / (int64_t)sizeof(T));      // the saved [B*S][4] fp32 gates (what the reference's show_gate.py dumps)
      }
      p.fused = b.take(Tk * H * e);
      tap("fused", p.fused, Tk * H);
      p.X1 = b.take(Tk * H * e);
      if (vr.pho) p.X2 = b.take(Tk * H * e);
      if (vr.res) p.X3 = b.take(Tk * H * e);
      if (vr.gate) p.dz = b.take(Tk * 16);
      if (vr.pho) {
        p.gru_dh = b.take(Tw * H * e); p.gru_dgi = b.take(Tw * 3 * H * e); p.gru_dgh = b.take(Tw * 3 * H * e);
        p.gru_onehot = b.take(Tw * 64 * e); p.gru_dtable = b.take(64LL * 3 * H * 4);
      }
      if (vr.res) {
        const int64_t big = (int64_t)p.blk[0].Pout * 64 * e;     // block 1 is the largest activation
        p.r_dout = b.take(big); p.r_dc2 = b.take(big); p.r_dcs = b.take(big); p.r_dh1 = b.take(big); p.r_dc1 = b.take(big);
        p.r_dx = b.take(big);
      }
    }
    if (vr.mlm_head && !glyph_only) {
      p.head_z = b.take(Tk * H * e); p.head_x = b.take(Tk * H * e); p.head_rstd = b.take(Tk * 4); p.head_y = b.take(Tk * H * e);
      p.head_xc = b.take(Tk * H * e); p.head_dz = b.take(Tk * H * e); p.head_ident = b.take(Tk * 4);
      tap("head.z", p.head_z, Tk * H); tap("head.y", p.head_y, Tk * H);
      tap("head.d_in", p.gA, Tk * H);      // d(head input) = d(top hidden) after stage_head
    }
    if (!vr.bert && vr.pho && !glyph_only) {      // Pho2Pretrain: the pinyin branch is the whole model (only a model_type 5 plan has these takes)
      plan_stack(p.pho, cfg.pho_layers, "pho_model");
      p.gru_table = b.take(64LL * 3 * H * 4);
      p.gru_hs = b.take((int64_t)Tp * Tk * H * e);
      p.gru_rzn = b.take((int64_t)Tp * Tk * 3 * H * e);
      p.gru_gh = b.take((int64_t)Tp * Tk * 3 * H * e);
      p.gru_out = b.take(Tk * H * e);
      tap("pho_gru", p.gru_out, Tk * H);
      p.gru_dh = b.take(Tk * H * e); p.gru_dgi = b.take(Tk * 3 * H * e); p.gru_dgh = b.take(Tk * 3 * H * e);
      p.gru_onehot = b.take(Tk * 64 * e); p.gru_dtable = b.take(64LL * 3 * H * 4);
    }
    p.total = b.off;
    return p;
  }

  int64_t workspace_bytes(int B, int S, int Tp) override {
    std::map<std::string, std::pair<int64_t, int64_t>> keep = taps;
    const Plan p = make_plan(B, S, Tp != 0 ? Tp : 1);
    taps = keep;
    return p.total;
  }
  // Workspace slots (round 6): a plan lives IN a workspace buffer (self-cleaning accumulators at zero, finite
  // stale rows where a live-row step leaves them), so the engine remembers, per caller buffer it has been bound to, the plan installed
  // there.  A caller that keeps one buffer per (B, S, Tp) key - modeling.py: train batch, eval batch, the short last batch, the
  // glyph-only plan - pays the zero fill of install_plan ONCE per key; re-binding a remembered buffer restores its plan as it was.
  // forget_workspace() before the caller frees a buffer (an allocator may hand the same address out again).
  struct Slot { char* ws; int64_t bytes; Plan pl; std::map<std::string, std::pair<int64_t, int64_t>> taps; uint64_t stamp; };
  std::vector<Slot> slots;
  uint64_t slot_clock = 0;
  static constexpr size_t MAX_SLOTS = 8;
  void stash_current() {
    if (ws == nullptr) return;
    Slot* s = nullptr;
    for (Slot& x : slots) if (x.ws == ws) s = &x;
    if (s == nullptr) {
      if (slots.size() >= MAX_SLOTS) {       // (callers forget what they free; this bound only guards a caller that never does)
        size_t old = 0;
        for (size_t i = 1; i < slots.size(); ++i) if (slots[i].stamp < slots[old].stamp) old = i;
        slots.erase(slots.begin() + old);
      }
      slots.push_back(Slot());
      s = &slots.back();
    }
    s->ws = ws; s->bytes = ws_bytes; s->pl = pl; s->taps = taps; s->stamp = ++slot_clock;
  }
  int bind(void* shadow, void* workspace, int64_t bytes) override {
    // everything the engine keeps inside the caller's shadow buffer (operand copies, the cast descriptor table, the chunk table of the
    // fresh-gradient zero fill) is rebuilt after a re-bind to another buffer
    if (shadow != (void*)sh) { glyph_built = false; descs_built = false; fill_built = false; n_fill = 0; skip_built = false; }
    stash_current();
    sh = (char*)shadow; ws = (char*)workspace; ws_bytes = bytes; pl = Plan(); have_fwd = false; have_glyph_fwd = false;
    for (Slot& x : slots)
      if (x.ws == ws && x.bytes == bytes) {
        pl = x.pl; taps = x.taps; x.stamp = ++slot_clock;
        break;
      }
    return RL_OK;
  }
  void forget_workspace(void* workspace) override {
    for (size_t i = 0; i < slots.size();) { if (slots[i].ws == (char*)workspace) slots.erase(slots.begin() + i); else ++i; }
    if (ws == (char*)workspace) { ws = nullptr; ws_bytes = 0; pl = Plan(); have_fwd = false; have_glyph_fwd = false; }
  }
  void invalidate_frozen() override { glyph_built = false; }
  int* id_flag = nullptr;
  void set_id_flag(int* flag) override { id_flag = flag; }
  int get_tap(const char* name, void** ptr, int64_t* numel) override {
    auto it = taps.find(name);
    if (it == taps.end() || !ws) return RL_ERR_ARG;
    *ptr = ws + it->second.first; *numel = it->second.second;
    return RL_OK;
  }

  // ---------------------------------------------------------------- dropout sites
  DropParams site(int id, float p) const {
    DropParams d;
    if (!last.training || p <= 0.f) return d;
    d.seed = (uint32_t)splitmix(last.seed * 0x100000001B3ull + (uint64_t)id);
    d.thresh = (uint32_t)((double)p * 4294967296.0);
    d.scale = 1.0f / (1.0f - p);
    return d;
  }
  static void set_drop(EpiParams<T>& ep, const DropParams& d) { ep.drop_seed = d.seed; ep.drop_thresh = d.thresh; ep.drop_scale = d.scale; }

  // ---------------------------------------------------------------- BERT stack
  int stack_forward(hipStream_t st, int sid, const StackOff& so, const std::vector<LayerSh>& shs, StackAct& a,
                    const int64_t* ids, const T* embeds, int pos_zero, const T** out, const T* tok_table = nullptr, int64_t tok_ld = 0) {
    const int B = pl.B, S = pl.S, Tk = B * S;
    {
      LnFwdArgs<T> ln;
      ln.rows = Tk; ln.H = H; ln.S = S;
      ln.in_mode = ids ? 1 : 2; ln.x = embeds; ln.ids = ids;
      if (tok_table != nullptr) { ln.in_mode = 3; ln.x = tok_table; ln.ld_in = tok_ld; ln.ids = last.src_idx; }      // embeds read by token id (token tables)
      ln.word = so.word >= 0 ? pp(so.word) : nullptr;
      ln.pos = pp(so.pos); ln.type0 = pp(so.type); ln.pos_zero = pos_zero;
      ln.gamma = pp(so.ln_g); ln.beta = pp(so.ln_b); ln.eps = cfg.ln_eps;
      ln.y = wp<T>(a.emb_y); ln.xhat = bwd_follows() ? wp<T>(a.emb_xhat) : nullptr; ln.rstd = wp<float>(a.emb_rstd);      // (xhat: the backward's operand)
      ln.drop = site(sid * 1000 + 900, cfg.hidden_dropout);
      RL_TRY(ln_fwd<T>(st, ln));
    }
    const T* x = wp<T>(a.emb_y);
    for (size_t l = 0; l < a.layers.size(); ++l) {
      // a pipelined optimizer sweep (adamw_step) steps the BERT layers two by two: wait in front of a pair's first reader
      if (sid == 0 && l >= 2 && (l % 2) == 0) RL_TRY(wait_opt(st, (int)l / 2));
      const LayerOff& o = so.layers[l];
      const LayerSh& w = shs[l];
      LayerAct& t = a.layers[l];
      {  // fused QKV projection (modeling_bert.py:221,231-232)
        EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = wp<T>(t.qkv); ep.ldo = 3 * H; ep.bias = pp(o.qkv_b);
        RL_TRY(nt_rows(st, x, H, sp<T>(w.qkv_w), H, Tk, 3 * H, H, ep));
      }
      {
        const DropParams d = site(sid * 1000 + (int)l * 10 + 1, cfg.attn_dropout);
        const T* q = wp<T>(t.qkv);
        // INVARIANT: rlen goes to the attention FORWARD on live-row steps only.  With rlen the kernels leave the
        // ctx / lse rows in [rlen[b], S) unwritten (attn_fwd_long: in some waves, zeros from others): only a step whose every consumer
        // skips or masks those rows (rows_live: the layer GEMMs walk the live blocks, the backward masks what it reads) may pass it;
        // a dense forward (evaluation, taps, engine:10=0) always gets nullptr and writes every row.
        RL_TRY(attn_fwd<T>(st, q, q + H, q + 2 * H, 3 * H, wp<float>(pl.mask_add), wp<T>(t.ctx), H, wp<float>(t.lse), B, nh, S,
                           d.seed, d.thresh, d.scale, rows_live ? live_rlen() : nullptr));
      }
      // BertSelfOutput: dense -> dropout -> + input -> LayerNorm (modeling_bert.py:273-277)
      RL_TRY(dense_resid_ln(st, wp<T>(t.ctx), H, sp<T>(w.ao_w), pp(o.ao_b), x, site(sid * 1000 + (int)l * 10 + 2, cfg.hidden_dropout),
                            pp(o.ao_ln_g), pp(o.ao_ln_b), wp<T>(t.s1), wp<float>(t.rstd1), wp<T>(t.y1)));
      {  // BertIntermediate (modeling_bert.py:326-329)
        // (the pre-activation is what the backward's GELU' reads: a forward nothing differentiates - evaluation, no_grad - does not store it)
        EpiParams<T> ep; ep.mode = EPI_GELU; ep.out = wp<T>(t.post); ep.out2 = bwd_follows() ? wp<T>(t.pre) : nullptr; ep.ldo = I; ep.bias = pp(o.in_b);
        RL_TRY(nt_rows(st, wp<T>(t.y1), H, sp<T>(w.in_w), H, Tk, I, H, ep));
      }
      // BertOutput (modeling_bert.py:339-343)
      RL_TRY(dense_resid_ln(st, wp<T>(t.post), I, sp<T>(w.out_w), pp(o.out_b), wp<T>(t.y1), site(sid * 1000 + (int)l * 10 + 3, cfg.hidden_dropout),
                            pp(o.out_ln_g), pp(o.out_ln_b), wp<T>(t.s2), wp<float>(t.rstd2), wp<T>(t.y2)));
      x = wp<T>(t.y2);
    }
    *out = x;
    return RL_OK;
  }

  // LayerNorm gamma / beta gradients: every ln_bwd leaves one record per workgroup; the records of up to LN_FOLD_MAX sites (the two
  // LayerNorms of four transformer layers) are folded by ONE launch at the end of the layer group instead of one fold per site
  // (38 launches of ~7 us on the critical chain per step).  Per scratch set (= per branch stream).
  LnFoldSites pend[3];
  float* ln_region(const Lane& la, int k) const { return wp<float>(la.sc->ln_slots) + (int64_t)k * LN_SLOT_FLOATS; }
  int flush_ln_folds(const Lane& la) {
    LnFoldSites& f = *la.pend;
    if (f.n == 0) return RL_OK;
    f.H = H;
    const int rc = ln_fold_multi(la.st, f);
    f.n = 0;
    return rc;
  }
  int ln_bwd_deferred(const Lane& la, LnBwdArgs<T>& ln) {
    LnFoldSites& f = *la.pend;
    int nrec = 0;
    ln.slots = ln_region(la, f.n);
    ln.deferred_records = &nrec;
    RL_TRY(ln_bwd<T>(la.st, ln));
    if (nrec > 0) {
      f.s[f.n++] = LnFoldSite{ln.slots, nrec, ln.dgamma, ln.dbeta};
      if (f.n == LN_FOLD_MAX) RL_TRY(flush_ln_folds(la));
    }
    return RL_OK;
  }

  // backward of layers [hi .. lo] of a stack; gA holds d(output of layer hi) on entry and d(input of layer lo) on exit
  int layers_backward(const Lane& la, int sid, const StackOff& so, const std::vector<LayerSh>& shs, StackAct& a, int hi, int lo,
                      T* gA) {
    const int B = pl.B, S = pl.S, Tk = B * S;
    const hipStream_t st = la.st;
    const typename Plan::Scratch& sc = *la.sc;
    T* gB = wp<T>(sc.gB); T* gE = wp<T>(sc.gE);
    const bool ov = g_wgrad_overlap && la.two_sets && side_ok();      // under branch overlap only the bert lane owns two dY sets
    for (int l = hi; l >= lo; --l) {
      const LayerOff& o = so.layers[l];
      const LayerSh& w = shs[l];
      LayerAct& t = a.layers[l];
      const T* x_in = l > 0 ? wp<T>(a.layers[l - 1].y2) : wp<T>(a.emb_y);
      const DropParams d3 = site(sid * 1000 + l * 10 + 3, cfg.hidden_dropout);
      const DropParams d2 = site(sid * 1000 + l * 10 + 2, cfg.hidden_dropout);
      const DropParams d1 = site(sid * 1000 + l * 10 + 1, cfg.attn_dropout);
      // Overlap: this layer's dY matrices go to the buffer set of its parity and stay untouched until the side stream has
      // run the four weight-gradient GEMMs on them; the caller's stream only waits before it re-uses that set (two layers
      // later).  Without overlap everything stays on `st` and set 0 is the plain scratch.
      const int p = ov ? (bw_layers++ & 1) : 0;
      T* gC1 = wp<T>(sc.wC1[p]); T* gC2 = wp<T>(sc.wC2[p]); T* gD = wp<T>(sc.wD[p]); T* gF = wp<T>(sc.wF[p]);
      if (ov && done_pending[p]) {
        if (hipStreamWaitEvent(st, ev_done[p], 0) != hipSuccess) return RL_ERR_LAUNCH;
        done_pending[p] = false;
      }
      const bool grouped = g_wgrad_group != 0;
      TnGroupProblem<T> gp4[4];
      auto wgrad = [&](int k, const T* dy, int64_t ldy, const T* x, int64_t ldx, int Iw, int Jw, float* bias_g, float* w_g) -> int {
        if (grouped) {        // collected; launched once after the attention backward produced the last dY
          gp4[k].A = dy; gp4[k].lda = ldy; gp4[k].B = x; gp4[k].ldb = ldx; gp4[k].I = Iw; gp4[k].J = Jw; gp4[k].out = w_g; gp4[k].ldo = Jw;
          gp4[k].colsum = bias_g;
          return RL_OK;
        }
        hipStream_t ws_ = st;
        TnEpi te; te.slab = wp<float>(sc.tn_slab); te.slab_elems = TN_SLAB_ELEMS; te.colsum = bias_g; te.out = w_g; te.ldo = Jw;
        if (ov) {
          if (hipEventRecord(ev_ready[p][k], st) != hipSuccess || hipStreamWaitEvent(side, ev_ready[p][k], 0) != hipSuccess) return RL_ERR_LAUNCH;
          ws_ = side; te.slab = wp<float>(sc.tn_slab2);
        }
        return gemm_tn<T>(ws_, dy, ldy, x, ldx, Tk, Iw, Jw, te);
      };
      const bool keep_dy = ov || grouped;      // the dense-output gradients must outlive the in-place updates of gA / gB
      {  // output LayerNorm: gA = d y2 -> gB = d s2 (residual part of d y1), gC1 = d(dense out) = d s2 * dropmask
        LnBwdArgs<T> ln; ln.rows = Tk; ln.H = H; ln.dy = gA; ln.xhat = wp<T>(t.s2); ln.rstd = wp<float>(t.rstd2); ln.row_live = live_rows();
        ln.gamma = pp(o.out_ln_g); ln.dx = gB; ln.dx_drop = (d3.thresh || keep_dy) ? gC1 : nullptr; ln.out_drop = d3;
        ln.dgamma = gp(o.out_ln_g); ln.dbeta = gp(o.out_ln_b);
        RL_TRY(ln_bwd_deferred(la, ln));
      }
      const T* dso = (d3.thresh || keep_dy) ? gC1 : gB;
      RL_TRY(wgrad(0, dso, H, wp<T>(t.post), I, H, I, gp(o.out_b), gp(o.out_w)));
      {  // d pre = (d s2' . W_out) * gelu'(pre)
        EpiParams<T> ep; ep.mode = EPI_GELU_BWD; ep.out = gD; ep.ldo = I; ep.aux = wp<T>(t.pre); ep.ldaux = I;
        RL_TRY(nt_rows(st, dso, H, sp<T>(w.out_wT), H, Tk, I, H, ep, true));      // gD feeds wgrad(1): whole live blocks
      }
      RL_TRY(wgrad(1, gD, I, wp<T>(t.y1), H, I, H, gp(o.in_b), gp(o.in_w)));
      {  // d y1 = d s2 + d pre . W_in
        EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = gB; ep.ldo = H; ep.accumulate = 1;
        RL_TRY(nt_rows(st, gD, I, sp<T>(w.in_wT), I, Tk, H, I, ep));
      }
      {  // attention-output LayerNorm: gB = d y1 -> gA = d s1, gC2 = d(dense out)
        LnBwdArgs<T> ln; ln.rows = Tk; ln.H = H; ln.dy = gB; ln.xhat = wp<T>(t.s1); ln.rstd = wp<float>(t.rstd1); ln.row_live = live_rows();
        ln.gamma = pp(o.ao_ln_g); ln.dx = gA; ln.dx_drop = (d2.thresh || keep_dy) ? gC2 : nullptr; ln.out_drop = d2;
        ln.dgamma = gp(o.ao_ln_g); ln.dbeta = gp(o.ao_ln_b);
        RL_TRY(ln_bwd_deferred(la, ln));
      }
      const T* dsa = (d2.thresh || keep_dy) ? gC2 : gA;
      RL_TRY(wgrad(2, dsa, H, wp<T>(t.ctx), H, H, H, gp(o.ao_b), gp(o.ao_w)));
      {  // d ctx = d s1' . W_ao
        EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = gE; ep.ldo = H;
        RL_TRY(nt_rows(st, dsa, H, sp<T>(w.ao_wT), H, Tk, H, H, ep));
      }
      {
        const T* q = wp<T>(t.qkv);
        RL_TRY(attn_bwd<T>(st, q, q + H, q + 2 * H, 3 * H, wp<float>(pl.mask_add), wp<T>(t.ctx), gE, H, wp<float>(t.lse),
                           wp<float>(sc.rowdot), gF, gF + H, gF + 2 * H, 3 * H, B, nh, S, d1.seed, d1.thresh, d1.scale, dead_ok ? wp<int>(pl.live_rlen) : nullptr));      // (backward: padding rows' gradients are exact zeros either way)
      }
      RL_TRY(wgrad(3, gF, 3 * H, x_in, H, 3 * H, H, gp(o.qkv_b), gp(o.qkv_w)));
      if (grouped) {
        hipStream_t ws_ = st;
        if (ov) {
          if (hipEventRecord(ev_ready[p][3], st) != hipSuccess || hipStreamWaitEvent(side, ev_ready[p][3], 0) != hipSuccess) return RL_ERR_LAUNCH;
          ws_ = side;
        }
        RL_TRY(gemm_tn_group<T>(ws_, 4, gp4, Tk, 1.0f, pass_overwrite ? 1 : 0, live_tiles(), live_tile_count(), live_list_rows()));
      }
      {  // d x_in = d s1 + d qkv . W_qkv
        EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = gA; ep.ldo = H; ep.accumulate = 1;
        RL_TRY(nt_rows(st, gF, 3 * H, sp<T>(w.qkv_wT), 3 * H, Tk, H, 3 * H, ep));
      }
      if (ov) {
        if (hipEventRecord(ev_done[p], side) != hipSuccess) return RL_ERR_LAUNCH;
        done_pending[p] = true;
      }
    }
    return flush_ln_folds(la);
  }

  // embeddings backward: gA = d(embedding output) -> dx (T*, d of the pre-LayerNorm sum) ; scatters table grads
  int emb_backward(const Lane& la, int sid, const StackOff& so, StackAct& a, const int64_t* ids, int pos_zero, const T* gA, T* dx) {
    const int B = pl.B, S = pl.S, Tk = B * S;
    const hipStream_t st = la.st;
    LnBwdArgs<T> ln; ln.slots = ln_region(la, LN_FOLD_MAX); ln.rows = Tk; ln.H = H; ln.dy = gA; ln.in_drop = site(sid * 1000 + 900, cfg.hidden_dropout);
    ln.xhat = wp<T>(a.emb_xhat); ln.rstd = wp<float>(a.emb_rstd); ln.gamma = pp(so.ln_g); ln.dx = dx;
    ln.dgamma = gp(so.ln_g); ln.dbeta = gp(so.ln_b);
    ln.row_live = live_rows();      // (padding rows: dy is an exact zero - dx written as zeros without reading the row's saved xhat)
    RL_TRY(ln_bwd<T>(st, ln));
    RL_TRY(embed_bwd<T>(st, dx, ids, B, S, H, (ids && so.word >= 0) ? gp(so.word) : nullptr, gp(so.pos), pos_zero, gp(so.type)));
    return RL_OK;
  }

  // ---------------------------------------------------------------- glyph ResNet (char_cnn.py)
  // rows_dev: device-side bound on the row space (glyph dedup: #distinct ids x pixels per image of that map)
  ConvLoader<T> geom(const T* src, const int64_t* index, int rows, int Hr, int Hs, int C, int ksz, int stride, int pad, int mode,
                     const int* rows_dev) const {
    ConvLoader<T> g;
    g.src = src; g.img_index = index; g.rows = rows; g.rows_dev = rows_dev; g.Hr = Hr; g.Wr = Hr; g.Hs = Hs; g.Ws = Hs; g.C = C;
    g.KH = ksz; g.KW = ksz; g.stride = stride; g.pad = pad; g.mode = mode; g.K = ksz * ksz * C;
    if (index != nullptr) g.index_rows = V;          // (gathers from the whole glyph table: the 32-bit offset span check uses the table size)
    return g;
  }
  // glyph dedup bookkeeping of block k's output map: device row bound, multiplicities, pixels per image
  RowBound rbound(int k) const {
    RowBound rb;
    rb.rows_dev = wp<int>(pl.gu_bounds) + 1 + k;
    rb.counts = wp<float>(pl.gu_counts);
    rb.hw = pl.blk[k].Hout * pl.blk[k].Hout;
    rb.slots = wp<float>(pl.bn_slots);
    return rb;
  }
  // Pn = B*S*Hout^2 is the TRUE sample count of the statistics (every token counts, PADs included, as in the
  // reference); the kernels visit only the distinct glyphs and weight them by their multiplicity.
  int bn_forward(hipStream_t st, const T* x, int Pn, int C, const BnOff& o, const BnAct& a, const RowBound& rb) {
    return bn_stats<T>(st, x, Pn, C, Pn, last.training, pp(o.g), pp(o.b), 1e-5f, 0.1f, BF + o.rmean, BF + o.rvar, BI + o.nbt, wp<float>(a.mean),
                       wp<float>(a.rstd), wp<float>(a.scale), wp<float>(a.shift), wp<float>(pl.bn_sums), rb);
  }
  // one normalisation of a block's backward (ops.h bn_backward): its saved input and statistics, where d(input) goes, its parameter gradients
  BnBranch<T> bn_branch(int64_t x, const BnOff& o, const BnAct& a, T* dx) {
    BnBranch<T> b;
    b.x = wp<T>(x); b.mean = wp<float>(a.mean); b.rstd = wp<float>(a.rstd); b.gamma = pp(o.g); b.dx = dx; b.dgamma = gp(o.g); b.dbeta = gp(o.b);
    return b;
  }
  bool glyph_gathered = false;             // gu_dense holds the distinct glyph images of the last resnet_forward
  int gather_glyphs(hipStream_t st) {
    return gather_images<T>(st, sp<T>(sh_glyph), wp<int64_t>(pl.gu_ids), wp<int>(pl.gu_bounds), pl.B * pl.S,
                            (int64_t)cfg.glyph_size * cfg.glyph_size * 8, wp<T>(pl.gu_dense));
  }
  int resnet_forward(hipStream_t st, const int64_t* ids, const T** out) {
    // The glyph stack of a token depends only on its id, so the ResNet runs once per DISTINCT id of the batch
    // (order of first occurrence) and BatchNorm weights each glyph by its multiplicity: identical statistics
    // to the reference's dense [B*S, F, 32, 32] pass, a fraction of the work (PAD alone is ~1/3 of the rows).
    {
      HwList hw; hw.n = L.tower.nblocks;
      for (int k = 0; k < hw.n; ++k) hw.v[k] = pl.blk[k].Hout * pl.blk[k].Hout;
      RL_TRY(glyph_unique(st, ids, pl.B * pl.S, V, wp<int>(pl.gu_first), wp<int>(pl.gu_flag), wp<int64_t>(pl.gu_ids),
                          wp<float>(pl.gu_counts), wp<int>(pl.gu_inv), wp<int>(pl.gu_bounds), hw));
    }
    const bool fuse7 = g_glyph_fuse != 0 && (int64_t)V * cfg.glyph_size * cfg.glyph_size * 8 * (int64_t)sizeof(T) < 0xFFFFFE00ll;
    glyph_gathered = !fuse7;
    if (!fuse7) RL_TRY(gather_glyphs(st));
    const T* x = fuse7 ? sp<T>(sh_glyph) : wp<T>(pl.gu_dense);
    const int64_t* index = fuse7 ? wp<int64_t>(pl.gu_ids) : nullptr;
    for (int k = 0; k < L.tower.nblocks; ++k) {
      const BlockOff& o = L.blocks[k];
      const BlockSh& s = sh_blk[k];
      BlockAct& a = pl.blk[k];
      const int Co = o.cout, Cin = s.cin_pad, Pn = a.Pout;
      const RowBound rb = rbound(k);
      if (!last.training && g_bn_fold) {
        // K9, evaluation (round 6; char_cnn.py:15-32 with BatchNorm2d on its running statistics = a per-channel affine map): the three
        // convolutions apply their BatchNorm in the epilogue - shortcut first (its normalised output is the second convolution's `aux`),
        // ReLU where the reference has one.  Three launches + three 1-workgroup scale / shift kernels per block, no pass over a raw
        // convolution output (was: 3 convolutions + 3 finalize + 2 apply launches, 5 extra passes over [Pn, Co]).
        RL_TRY(bn_finalize_eval(st, Co, pp(o.bns.g), pp(o.bns.b), 1e-5f, BF + o.bns.rmean, BF + o.bns.rvar, wp<float>(a.bns.scale), wp<float>(a.bns.shift)));
        RL_TRY(bn_finalize_eval(st, Co, pp(o.bn1.g), pp(o.bn1.b), 1e-5f, BF + o.bn1.rmean, BF + o.bn1.rvar, wp<float>(a.bn1.scale), wp<float>(a.bn1.shift)));
        RL_TRY(bn_finalize_eval(st, Co, pp(o.bn2.g), pp(o.bn2.b), 1e-5f, BF + o.bn2.rmean, BF + o.bn2.rvar, wp<float>(a.bn2.scale), wp<float>(a.bn2.shift)));
        EpiParams<T> ea; ea.mode = EPI_AFFINE; ea.ldo = Co;
        ea.out = wp<T>(a.cs); ea.col_scale = wp<float>(a.bns.scale); ea.bias = wp<float>(a.bns.shift); ea.relu = 0;
        RL_TRY(gemm_nt_conv<T>(st, geom(x, index, Pn, a.Hout, a.Hin, Cin, 1, 2, 0, 0, rb.rows_dev), sp<T>(s.wsf), Cin, Pn, Co, Cin, ea));
        ea.out = wp<T>(a.h1); ea.col_scale = wp<float>(a.bn1.scale); ea.bias = wp<float>(a.bn1.shift); ea.relu = 1;
        RL_TRY(gemm_nt_conv<T>(st, geom(x, index, Pn, a.Hout, a.Hin, Cin, 3, 2, 1, 0, rb.rows_dev), sp<T>(s.w1f), 9 * Cin, Pn, Co, 9 * Cin, ea));
        ea.out = wp<T>(a.out); ea.col_scale = wp<float>(a.bn2.scale); ea.bias = wp<float>(a.bn2.shift); ea.relu = 1;
        ea.aux = wp<T>(a.cs); ea.ldaux = Co;
        if (a.Hout == 1) RL_TRY(gemm_nt<T>(st, wp<T>(a.h1), Co, sp<T>(s.w2f) + 4 * Co, 9 * Co, Pn, Co, Co, ea, rb.rows_dev));
        else RL_TRY(gemm_nt_conv<T>(st, geom(wp<T>(a.h1), nullptr, Pn, a.Hout, a.Hout, Co, 3, 1, 1, 0, rb.rows_dev), sp<T>(s.w2f), 9 * Co, Pn, Co, 9 * Co, ea));
        x = wp<T>(a.out);
        index = nullptr;
        continue;
      }
      EpiParams<T> ep; ep.mode = EPI_STORE; ep.ldo = Co;
      // residual_function.0: 3x3 stride 2 pad 1 (char_cnn.py:16)
      ep.out = wp<T>(a.c1);
      RL_TRY(gemm_nt_conv<T>(st, geom(x, index, Pn, a.Hout, a.Hin, Cin, 3, 2, 1, 0, rb.rows_dev), sp<T>(s.w1f), 9 * Cin, Pn, Co, 9 * Cin, ep));
      RL_TRY(bn_forward(st, wp<T>(a.c1), Pn, Co, o.bn1, a.bn1, rb));
      RL_TRY(bn_apply<T>(st, wp<T>(a.c1), wp<float>(a.bn1.scale), wp<float>(a.bn1.shift), nullptr, nullptr, nullptr, wp<T>(a.h1), Pn, Co, 1, rb));
      // residual_function.3: 3x3 stride 1 pad 1 (char_cnn.py:19)
      ep.out = wp<T>(a.c2);
      if (a.Hout == 1) {
        // a 3x3 / pad 1 convolution on a 1x1 map touches only its centre tap (the other eight read padding): a dense GEMM against
        // the centre-tap slice of the [Co][tap][Ci] operand copy, 1/9 of the implicit-GEMM work (block 5: 113 -> ~15 us)
        RL_TRY(gemm_nt<T>(st, wp<T>(a.h1), Co, sp<T>(s.w2f) + 4 * Co, 9 * Co, Pn, Co, Co, ep, rb.rows_dev));
      } else {
        RL_TRY(gemm_nt_conv<T>(st, geom(wp<T>(a.h1), nullptr, Pn, a.Hout, a.Hout, Co, 3, 1, 1, 0, rb.rows_dev), sp<T>(s.w2f), 9 * Co, Pn, Co, 9 * Co, ep));
      }
      RL_TRY(bn_forward(st, wp<T>(a.c2), Pn, Co, o.bn2, a.bn2, rb));
      // shortcut: 1x1 stride 2 (char_cnn.py:26-28)
      ep.out = wp<T>(a.cs);
      RL_TRY(gemm_nt_conv<T>(st, geom(x, index, Pn, a.Hout, a.Hin, Cin, 1, 2, 0, 0, rb.rows_dev), sp<T>(s.wsf), Cin, Pn, Co, Cin, ep));
      RL_TRY(bn_forward(st, wp<T>(a.cs), Pn, Co, o.bns, a.bns, rb));
      RL_TRY(bn_apply<T>(st, wp<T>(a.c2), wp<float>(a.bn2.scale), wp<float>(a.bn2.shift), wp<T>(a.cs), wp<float>(a.bns.scale),
                         wp<float>(a.bns.shift), wp<T>(a.out), Pn, Co, 1, rb));
      x = wp<T>(a.out);
      index = nullptr;
    }
    *out = x;
    return RL_OK;
  }
  // d(flattened tower output) per token [B*S, 768] -> r_dout: d(top map) per DISTINCT glyph in the tower's NHWC storage order, summed
  // over the tokens that share the glyph (a 2x2 top undoes the reference's channel-major flatten on the way)
  int top_segment_sum(hipStream_t st, const T* d_res) {
    const int Tk = pl.B * pl.S;
    if (L.tower.top_pixels() == 4)
      return segment_sum_chw4<T>(st, d_res, wp<int>(pl.gu_inv), Tk, H, wp<float>(pl.seg_acc), wp<T>(pl.r_dout), wp<int>(pl.gu_bounds));
    return segment_sum<T>(st, d_res, wp<int>(pl.gu_inv), Tk, H, wp<float>(pl.seg_acc), wp<T>(pl.r_dout), wp<int>(pl.gu_bounds));
  }
  // d_top: gradient w.r.t. the last block's output per DISTINCT glyph [U, top pixels, top channels] (already summed over the tokens sharing it)
  int resnet_backward(const Lane& la, const T* d_top) {
    const hipStream_t st = la.st;
    float* sums = wp<float>(pl.bn_sums);
    const T* d_out = d_top;
    if (!glyph_gathered) { RL_TRY(gather_glyphs(st)); glyph_gathered = true; }      // K7: block 1's weight gradients read the gathered images
    for (int k = L.tower.nblocks - 1; k >= 0; --k) {
      const BlockOff& o = L.blocks[k];
      const BlockSh& s = sh_blk[k];
      BlockAct& a = pl.blk[k];
      const int Co = o.cout, Cin = s.cin_pad, Pn = a.Pout;
      const RowBound rb = rbound(k);
      const T* x_in = k > 0 ? wp<T>(pl.blk[k - 1].out) : wp<T>(pl.gu_dense);
      const int64_t* index = nullptr;
      T* dc2 = wp<T>(pl.r_dc2); T* dcs = wp<T>(pl.r_dcs); T* dh1 = wp<T>(pl.r_dh1); T* dc1 = wp<T>(pl.r_dc1);
      // out = relu(bn2(c2) + bns(cs))
      // bn2 and the shortcut's BN see the same incoming gradient and ReLU mask: bf16 reads them once for both (two passes over four
      // tensors instead of four passes over three)
      RL_TRY(bn_backward<T>(st, d_out, wp<T>(a.out), Pn, Co, Pn, bn_branch(a.c2, o.bn2, a.bn2, dc2), bn_branch(a.cs, o.bns, a.bns, dcs), sums, rb));
      // conv2 (3x3 s1): weight grad and data grad
      { TnEpi te; te.slab = wp<float>(la.sc->tn_slab); te.slab_elems = TN_SLAB_ELEMS; te.mode = TN_CONVW; te.out = gp(o.w2); te.Cin = Co; te.Cpad = Co; te.KHW = 9;
        if (a.Hout == 1) { te.tap0 = 4; RL_TRY(gemm_tn<T>(st, dc2, Co, wp<T>(a.h1), Co, Pn, Co, Co, te, rb.rows_dev)); }       // centre tap only
        else RL_TRY(gemm_tn_conv<T>(st, dc2, Co, geom(wp<T>(a.h1), nullptr, Pn, a.Hout, a.Hout, Co, 3, 1, 1, 0, rb.rows_dev), Pn, Co, 9 * Co, te)); }
      { EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = dh1; ep.ldo = Co;
        if (a.Hout == 1) RL_TRY(gemm_nt<T>(st, dc2, Co, sp<T>(s.w2d) + 4 * Co, 9 * Co, Pn, Co, Co, ep, rb.rows_dev));          // centre tap only
        else RL_TRY(gemm_nt_conv<T>(st, geom(dc2, nullptr, Pn, a.Hout, a.Hout, Co, 3, 1, 1, 1, rb.rows_dev), sp<T>(s.w2d), 9 * Co, Pn, Co, 9 * Co, ep)); }
      // h1 = relu(bn1(c1))
      RL_TRY(bn_backward<T>(st, dh1, wp<T>(a.h1), Pn, Co, Pn, bn_branch(a.c1, o.bn1, a.bn1, dc1), BnBranch<T>(), sums, rb));
      // conv1 (3x3 s2) and shortcut (1x1 s2) weight grads
      { TnEpi te; te.slab = wp<float>(la.sc->tn_slab); te.slab_elems = TN_SLAB_ELEMS; te.mode = TN_CONVW; te.out = gp(o.w1); te.Cin = o.cin; te.Cpad = Cin; te.KHW = 9;
        RL_TRY(gemm_tn_conv<T>(st, dc1, Co, geom(x_in, index, Pn, a.Hout, a.Hin, Cin, 3, 2, 1, 0, rb.rows_dev), Pn, Co, 9 * Cin, te)); }
      { TnEpi te; te.slab = wp<float>(la.sc->tn_slab); te.slab_elems = TN_SLAB_ELEMS; te.mode = TN_CONVW; te.out = gp(o.ws); te.Cin = o.cin; te.Cpad = Cin; te.KHW = 1;
        RL_TRY(gemm_tn_conv<T>(st, dcs, Co, geom(x_in, index, Pn, a.Hout, a.Hin, Cin, 1, 2, 0, 0, rb.rows_dev), Pn, Co, Cin, te)); }
      if (k > 0) {   // d x_in = dgrad(conv1) + dgrad(shortcut); the glyph table itself is frozen
        const int Pin = pl.blk[k - 1].Pout;
        const int* in_bound = rbound(k - 1).rows_dev;
        T* dx = (d_out == wp<T>(pl.r_dx)) ? wp<T>(pl.r_dout) : wp<T>(pl.r_dx);
        EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = dx; ep.ldo = Cin;
        if (g_dgrad_parity && a.Hin >= 2 && (a.Hin & (a.Hin - 1)) == 0) {
          // by parity class of the input pixel: only the taps that reach it, a quarter of the rows per launch; the 1x1 stride-2
          // shortcut reaches the (even, even) pixels only
          RL_TRY(conv_dgrad_s2<T>(st, geom(dc1, nullptr, Pin, a.Hin, a.Hout, Co, 3, 2, 1, 1, in_bound), sp<T>(s.w1p), 9 * Co, Cin, ep));
          ep.accumulate = 1;
          RL_TRY(conv_dgrad_s2<T>(st, geom(dcs, nullptr, Pin, a.Hin, a.Hout, Co, 1, 2, 0, 1, in_bound), sp<T>(s.wsd), Co, Cin, ep));
        } else {
          RL_TRY(gemm_nt_conv<T>(st, geom(dc1, nullptr, Pin, a.Hin, a.Hout, Co, 3, 2, 1, 1, in_bound), sp<T>(s.w1d), 9 * Co, Pin, Cin, 9 * Co, ep));
          ep.accumulate = 1;
          RL_TRY(gemm_nt_conv<T>(st, geom(dcs, nullptr, Pin, a.Hin, a.Hout, Co, 1, 2, 0, 1, in_bound), sp<T>(s.wsd), Co, Pin, Cin, Co, ep));
        }
        d_out = dx;
      }
    }
    return RL_OK;
  }

  // ---------------------------------------------------------------- pinyin GRU (models.py:818-826)
  int gru_forward(hipStream_t st) {
    const int N = pl.B * pl.S, Tp = last.Tp;
    // W_ih x + b_ih for the 33 pinyin symbols, from the fp32 masters.  Parity mode: one exact-fp32 MFMA GEMM ([33,768] x [2304,768]^T,
    // a k-ordered fmaf chain); speed mode: the dedicated table kernel (W_ih row in registers, 56 -> ~10 us)
    bool table_done = false;
    if constexpr (sizeof(T) == 2) table_done = gru_table_fwd(st, pp(L.pho_emb), pp(L.gru_w_ih), pp(L.gru_b_ih), cfg.pho_vocab, H, wp<float>(pl.gru_table)) == RL_OK;
    if (!table_done) {
      EpiParams<float> ep; ep.mode = EPI_STORE; ep.out = wp<float>(pl.gru_table); ep.ldo = 3 * H; ep.bias = pp(L.gru_b_ih);
      RL_TRY(gemm_nt<float>(st, pp(L.pho_emb), H, pp(L.gru_w_ih), H, cfg.pho_vocab, 3 * H, H, ep));
    }
    for (int t = 0; t < Tp; ++t) {
      const int n = last_alive[t];
      if (n <= 0) break;
      const int* nd = alive_dev ? (const int*)alive_dev + t : nullptr;
      T* hs_t = wp<T>(pl.gru_hs) + (int64_t)t * N * H;
      T* gh_t = wp<T>(pl.gru_gh) + (int64_t)t * N * 3 * H;
      const T* hs_prev = t > 0 ? wp<T>(pl.gru_hs) + (int64_t)(t - 1) * N * H : nullptr;
      if constexpr (sizeof(T) == 2) {
        if (t > 0 && g_gru_fuse && (H % 64) == 0) {      // recurrent projection + gate math in one launch
          EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = hs_t; ep.ldo = H; ep.bias = pp(L.gru_b_hh); ep.m_dev = nd;
          ep.gru_table = wp<float>(pl.gru_table); ep.gru_pho_idx = last.pho_idx; ep.gru_perm = last.pho_perm; ep.gru_lens = last.pho_lens_sorted;
          ep.gru_hprev = hs_prev; ep.gru_rzn = wp<T>(pl.gru_rzn) + (int64_t)t * N * 3 * H; ep.gru_gh = gh_t; ep.gru_out = wp<T>(pl.gru_out);
          ep.gru_Tp = Tp; ep.gru_t = t;
          const int rc = gemm_nt8_gru(st, hs_prev, H, sp<T>(sh_gru_hh), H, n, 3 * H, H, ep);
          if (rc == RL_OK) continue;
          if (rc != RL_ERR_ARG) return rc;
        }
      }
      if (t > 0) {
        EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = gh_t; ep.ldo = 3 * H; ep.bias = pp(L.gru_b_hh);
        RL_TRY(gemm_nt<T>(st, hs_prev, H, sp<T>(sh_gru_hh), H, n, 3 * H, H, ep, nd));
      }
      GruStepArgs<T> a;
      a.n_alive = n; a.n_alive_dev = nd; a.H = H; a.Tp = Tp; a.t = t; a.table = wp<float>(pl.gru_table); a.pho_idx = last.pho_idx;
      a.perm = last.pho_perm; a.lens = last.pho_lens_sorted; a.gh = t > 0 ? gh_t : nullptr; a.b_hh = pp(L.gru_b_hh);
      a.h_prev = hs_prev; a.h_new = hs_t; a.rzn = wp<T>(pl.gru_rzn) + (int64_t)t * N * 3 * H; a.out = wp<T>(pl.gru_out);
      RL_TRY(gru_step_fwd<T>(st, a));
    }
    return RL_OK;
  }
  int gru_backward(const Lane& la, const T* dout) {
    const hipStream_t st = la.st;
    const int N = pl.B * pl.S, Tp = last.Tp;
    float* dtable = wp<float>(pl.gru_dtable);
    RL_TRY(fill_f32(st, dtable, 0.f, 64LL * 3 * H));
    for (int t = Tp - 1; t >= 0; --t) {
      const int n = last_alive[t];
      if (n <= 0) continue;
      const int* nd = alive_dev ? (const int*)alive_dev + t : nullptr;
      const T* hs_prev = t > 0 ? wp<T>(pl.gru_hs) + (int64_t)(t - 1) * N * H : nullptr;
      T* gh_t = wp<T>(pl.gru_gh) + (int64_t)t * N * 3 * H;
      GruStepArgs<T> a;
      a.n_alive = n; a.n_alive_dev = nd; a.H = H; a.Tp = Tp; a.t = t; a.pho_idx = last.pho_idx; a.perm = last.pho_perm; a.lens = last.pho_lens_sorted;
      a.gh = t > 0 ? gh_t : nullptr; a.b_hh = pp(L.gru_b_hh); a.h_prev = hs_prev;
      a.rzn = wp<T>(pl.gru_rzn) + (int64_t)t * N * 3 * H; a.dout = dout; a.dh = wp<T>(pl.gru_dh); a.dgi = wp<T>(pl.gru_dgi);
      a.dgh = wp<T>(pl.gru_dgh); a.onehot = wp<T>(pl.gru_onehot);
      RL_TRY(gru_step_bwd<T>(st, a));
      { TnEpi te; te.slab = wp<float>(la.sc->tn_slab); te.slab_elems = TN_SLAB_ELEMS; te.out = dtable; te.ldo = 3 * H; RL_TRY(gemm_tn<T>(st, a.onehot, 64, a.dgi, 3 * H, n, 64, 3 * H, te, nd)); }
      // d b_hh = column sums of dgh: rides along the W_hh weight-gradient GEMM of the step (fused ones-vector MFMA, TnEpi::colsum) -
      // six column-reduction + fold launch pairs less; step 0 has no recurrent GEMM and keeps the reduction
      if (t == 0) RL_TRY(bias_grad<T>(st, a.dgh, 3 * H, n, 3 * H, gp(L.gru_b_hh), nd));
      if (t > 0) {
        { TnEpi te; te.slab = wp<float>(la.sc->tn_slab); te.slab_elems = TN_SLAB_ELEMS; te.out = gp(L.gru_w_hh); te.ldo = H; te.colsum = gp(L.gru_b_hh);
          RL_TRY(gemm_tn<T>(st, a.dgh, 3 * H, hs_prev, H, n, 3 * H, H, te, nd)); }
        EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = a.dh; ep.ldo = H; ep.accumulate = 1;
        RL_TRY(gemm_nt<T>(st, a.dgh, 3 * H, sp<T>(sh_gru_hhT), 3 * H, n, H, 3 * H, ep, nd));
      }
    }
    RL_TRY(gru_table_bwd(st, dtable, 3 * H, pp(L.pho_emb), pp(L.gru_w_ih), cfg.pho_vocab, H, gp(L.pho_emb), gp(L.gru_w_ih), gp(L.gru_b_ih)));
    return RL_OK;
  }

  GateArgs<T> gate_args() const {
    GateArgs<T> g;
    g.B = pl.B; g.S = pl.S; g.H = H; g.nsrc = vr.nsrc; g.softmax = vr.gate_softmax;
    g.bert = wp<T>(pl.bert.layers.back().y2);
    g.pho = vr.pho ? wp<T>(pl.pho.layers.back().y2) : nullptr;
    g.res = vr.res ? wp<T>(pl.res_h) : nullptr;
    g.masks = last.masks; g.W = pp(L.gate_w); g.bias = pp(L.gate_b);
    g.mean = wp<float>(pl.gate_mean); g.msum = wp<float>(pl.gate_msum); g.g = wp<float>(pl.gate_g); g.fused = wp<T>(pl.fused);
    return g;
  }

  // ---------------------------------------------------------------- forward
  // dense -> dropout -> + residual -> LayerNorm (modeling_bert.py:273-277, 339-343)
  // the forward being enqueued is one a backward can follow (realise_engine_backward checks the same): it must leave what that pass reads
  bool bwd_follows() const { return last.training && last.tgt_idx != nullptr && last.want_dlogits; }
  int dense_resid_ln(hipStream_t st, const T* a, int K, const T* w, const float* bias, const T* resid, const DropParams& drop,
                     const float* gamma, const float* beta, T* s_xhat, float* rstd, T* y) {
    const int Tk = pl.B * pl.S;
    EpiParams<T> ep; ep.mode = EPI_DROP_RESID; ep.out = s_xhat; ep.ldo = H; ep.bias = bias; ep.aux = resid; ep.ldaux = H; set_drop(ep, drop);
    RL_TRY(nt_rows(st, a, K, w, K, Tk, H, K, ep));
    LnFwdArgs<T> ln; ln.rows = Tk; ln.H = H; ln.x = s_xhat; ln.gamma = gamma; ln.beta = beta;
    ln.eps = cfg.ln_eps; ln.y = y; ln.xhat = bwd_follows() ? s_xhat : nullptr; ln.rstd = rstd;      // (a forward nothing differentiates does not store the normalised rows)
    if (rows_live && (Tk % 16) == 0) ln.row_live = live_rows();      // x holds fresh rows in the listed blocks only: the others are not worth a pass
    return ln_fwd<T>(st, ln);
  }
  int64_t plan_installs = 0;               // workspace zero fills so far (realise_engine_plan_installs: tests / bench count them)
  int64_t plan_install_count() const override { return plan_installs; }
  int cast_desc_info(int i, realise_cast_desc_info* out) const override {
    if (!descs_built || !sh) return -RL_ERR_ARG;
    const int n = (int)desc_host.size();
    if (out == nullptr) return n;
    if (i < 0 || i >= n) return -RL_ERR_ARG;
    const CastDesc& d = desc_host[i];
    auto off = [&](const void* q) -> int64_t { return q ? (int64_t)((const char*)q - (const char*)sh) : -1; };
    out->src_off = d.src - P; out->dst_off = off(d.dst); out->dstT_off = off(d.dstT);
    out->R = d.R; out->C = d.C; out->ldT = d.ldT; out->group = i < n_descs_a ? 0 : 1;
    return n;
  }
  int install_plan(hipStream_t st, const Plan& p) {
    if (p.total > ws_bytes) { fprintf(stderr, "[realise_hip] workspace too small: need %lld have %lld\n", (long long)p.total, (long long)ws_bytes); return RL_ERR_ARG; }
    pl = p;
    ++plan_installs;
    // The whole workspace starts at zero (once per plan): the self-cleaning accumulators need it (zero_once), and a live-row step
    // leaves the activation rows of padding tokens as they are - what they hold must be finite wherever a later pass multiplies it by
    // an exact zero (masked mean, gate gradients).
    if (hipMemsetAsync(ws, 0, (size_t)pl.total, st) != hipSuccess) return RL_ERR_LAUNCH;
    if (vr.mlm_head && pl.head_ident != 0) {      // row j -> j: the slab fold of the decoder's split-K data gradient keeps the compacted rows where they are
      ident_keep.emplace_back((size_t)pl.B * pl.S);      // (a vector per install: stays alive while its upload is in flight)
      std::vector<int>& id = ident_keep.back();
      for (size_t i = 0; i < id.size(); ++i) id[i] = (int)i;
      if (hipMemcpyAsync(ws + pl.head_ident, id.data(), id.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) return RL_ERR_LAUNCH;
    }
    return RL_OK;
  }
  std::vector<std::vector<int>> ident_keep;
  // ---------------------------------------------------------------- MLM head (vr.mlm_head; modeling_bert.py:419-462)
  // transform of `rows` rows of x (n_dev, nullable: a device-side count of the rows that matter): dense + erf GELU in the GEMM's epilogue,
  // then LayerNorm -> pl.head_y, the decoder's input.  A forward a backward can follow keeps the pre-activation and xhat (in place).
  // The LayerNorm takes no device count: it also normalises the stale (finite) rows behind *n_dev, which nothing reads.
  int head_forward(hipStream_t st, const T* x, int rows, const int* n_dev) {
    EpiParams<T> ep; ep.mode = EPI_GELU; ep.out = wp<T>(pl.head_x); ep.out2 = bwd_follows() ? wp<T>(pl.head_z) : nullptr; ep.ldo = H; ep.bias = pp(L.head_b);
    RL_TRY(gemm_nt<T>(st, x, H, sp<T>(sh_head_w), H, rows, H, H, ep, n_dev));
    LnFwdArgs<T> ln; ln.rows = rows; ln.H = H; ln.x = wp<T>(pl.head_x); ln.gamma = pp(L.head_ln_g); ln.beta = pp(L.head_ln_b); ln.eps = cfg.ln_eps;
    ln.y = wp<T>(pl.head_y); ln.xhat = bwd_follows() ? wp<T>(pl.head_x) : nullptr; ln.rstd = wp<float>(pl.head_rstd);
    return ln_fwd<T>(st, ln);
  }
  // the size conditions of a live-row step (g_live_rows): bf16 with the 16-row block lists, whole 64-row tiles in every GEMM dimension,
  // 32-bit byte offsets into the widest activation
  bool live_step_ok(int Tk) const {
    return g_live_rows && live16() && (Tk % 64) == 0 && (H % 64) == 0 && (I % 64) == 0 && (int64_t)Tk * I * 2 < 0xFFFFFF00ll;
  }
  // the row-liveness tables of batch b (row_live, the live 64- / 32- / 16-row block lists, their counts, live lengths, the live-row list)
  int fill_live_tables(hipStream_t st, const realise_batch& b) {
    return row_liveness(st, b.masks, b.loss_masks, pl.B, pl.S, wp<uint8_t>(pl.row_live), wp<int>(pl.live_t64), wp<int>(pl.live_t32),
                        wp<int>(pl.live_t16), wp<int>(pl.live_n), wp<int>(pl.live_rlen), wp<int>(pl.live_rows));
  }
  // The head's three forms, and every batch the head refuses - decided here, before forward() launches anything.
  //   HEAD_DECODE (predict()): no [B*S, V] tensor, the classifier GEMM's epilogue decodes (gemm_nt_decode); no backward follows.
  //   HEAD_LOSS_ROWS (K13, training without logits): the classifier over the loss rows only, written into the gradient buffer.
  //   HEAD_LOGITS: the logits of every row, and the loss when the batch brings targets.
  enum HeadMode { HEAD_DECODE, HEAD_LOSS_ROWS, HEAD_LOGITS };
  int head_mode(const realise_batch& b, HeadMode* mode) const {
    const bool loss_io = b.loss_masks && b.loss_out;
    if (b.logits_out != nullptr) { *mode = HEAD_LOGITS; return b.tgt_idx && !loss_io ? RL_ERR_ARG : RL_OK; }
    if (!b.training && dec_req.k != 0) { *mode = HEAD_DECODE; return b.tgt_idx && !(loss_io && dec_req.label_logit) ? RL_ERR_ARG : RL_OK; }
    *mode = HEAD_LOSS_ROWS;
    return sizeof(T) != 2 || !b.tgt_idx || !loss_io || !b.want_dlogits || !g_cls_compact || (int64_t)b.B * b.S > 65536 ? RL_ERR_ARG : RL_OK;
  }
  // The head (models.py:859-869): final dropout, [MLM transform,] tied vocabulary classifier, cross-entropy - and hs, what stage_head reads.
  int head_fwd(hipStream_t st, const realise_batch& b, HeadMode mode, const T* top) {
    const int Tk = b.B * b.S;
    const bool want_loss = b.tgt_idx != nullptr, loss_rows = mode == HEAD_LOSS_ROWS;
    const DropParams dfin = site(5000, cfg.hidden_dropout);
    const T* head_in = top;      // the rows that enter the transform (MLM head) or the classifier
    if (dfin.thresh) { RL_TRY(dropout_apply<T>(st, top, wp<T>(pl.out_d), Tk, H, dfin)); head_in = wp<T>(pl.out_d); }
    // Backward of the classifier over the rows that enter the loss only (loss_masks: no [CLS] / [SEP] / padding - 60 % of the
    // rows of a SIGHAN-shaped batch): the gradient rows are written compacted, the classifier input is gathered to match; the
    // other rows' gradients are exact zeros in the dense form, so the weight / bias / data gradients are the same sums.
    // (the padding rows the backward skips: row_liveness at the top of forward())
    const bool compact = loss_rows || (mode == HEAD_LOGITS && want_loss && g_cls_compact && b.want_dlogits && Tk <= 65536);
    int* const act = wp<int>(pl.cls_act);
    int* const n_act = wp<int>(pl.cls_nact);
    CeCompact cc;
    if (compact) { cc.act_idx = act; cc.inv = wp<int>(pl.cls_inv); cc.n_act = n_act; }
    // K13 (round 6; models.py:859-869 as the training loop consumes it, run.py:191 takes the loss alone): no [B*S, V] logits.  The
    // classifier runs over the rows that enter the loss only - listed first (phase 1), the head's input gathered to match - and writes
    // their logits rows, compacted and at the gradient's row pitch, INTO the gradient buffer; the cross-entropy kernel (phase 2) reads
    // each row once into registers and stores the row's gradient over it.  Same fp32 accumulators, same bf16 rounding, same row kernel
    // as the two-buffer form: loss and every gradient bit-identical (tests/test_round6_gpu.py).
    const int* n_rows = nullptr;      // device count of the rows the head computes (null: all Tk)
    if (loss_rows) {
      cc.phase = 1;
      RL_TRY(ce_loss<T>(st, nullptr, Vp, b.tgt_idx, b.loss_masks, Tk, V, b.loss_out, wp<float>(pl.count), wp<T>(pl.dlogits),
                        wp<float>(pl.loss_internal), Vp, cc));
      T* xc = wp<T>(vr.mlm_head ? pl.head_xc : pl.cls_xc);
      RL_TRY(gather_listed_rows<T>(st, head_in, act, n_act, Tk, H, xc));
      head_in = xc; n_rows = n_act;
    }
    const T* dec_in = head_in;
    if (vr.mlm_head) {      // the transform over the rows the classifier reads; the decoder reads its output
      RL_TRY(head_forward(st, head_in, Tk, n_rows));
      dec_in = wp<T>(pl.head_y);
    }
    if (mode == HEAD_DECODE) {
      // Inference (models.py:859-869 + np.argmax(preds, -1) of src/run.py:262-263 / src/test.py:143) without a [B*S, V] tensor: the
      // classifier GEMM's epilogue reduces its tiles to per-row candidates and softmax partials (gemm_nt_decode), every row, every dtype.
      DecodeOut o; o.k = dec_req.k; o.ids = dec_req.ids; o.values = dec_req.values; o.probs = dec_req.probs; o.lse = dec_req.lse;
      o.label_logit = dec_req.label_logit; o.scratch = dec_req.scratch; o.scratch_bytes = dec_req.scratch_bytes;
      RL_TRY(gemm_nt_decode<T>(st, dec_in, H, sp<T>(sh_cls_w), H, Tk, V, H, pp(L.cls_b), want_loss ? b.tgt_idx : nullptr, o, sizeof(T) == 4 ? x3() : 0));
      if (want_loss) RL_TRY(decode_loss(st, dec_req.lse, dec_req.label_logit, b.tgt_idx, b.loss_masks, Tk, b.loss_out));
      return RL_OK;
    }
    // tied vocabulary classifier (models.py:859): the loss rows into the gradient buffer, or every row into the caller's logits
    T* const logits = loss_rows ? wp<T>(pl.dlogits) : (T*)b.logits_out;
    const int64_t ldl = loss_rows ? Vp : V;
    EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = logits; ep.ldo = ldl; ep.bias = pp(L.cls_b);
    // logits_f32_out (round 6): the fp32 logits the reference returns (models.py:859) written by the classifier's own epilogue next
    // to the compute-dtype ones the loss reads - no cast pass over [B*S, V]; a shape the persistent kernel does not take is cast here
    const bool want_f32 = !loss_rows && b.logits_f32_out != nullptr;
    int rc = RL_ERR_ARG;
    if (want_f32 && sizeof(T) == 2) {
      EpiParams<T> e2 = ep; e2.out_f32 = b.logits_f32_out; e2.ldo_f32 = V;
      rc = gemm_nt<T>(st, dec_in, H, sp<T>(sh_cls_w), H, Tk, V, H, e2);
      if (rc != RL_OK && rc != RL_ERR_ARG) return rc;
    }
    if (rc != RL_OK) {
      RL_TRY(gemm_nt<T>(st, dec_in, H, sp<T>(sh_cls_w), H, Tk, V, H, ep, n_rows));
      if (want_f32) RL_TRY(cast_to_f32<T>(st, logits, b.logits_f32_out, (int64_t)Tk * V));
    }
    if (!want_loss) return RL_OK;
    if (loss_rows) { cc.phase = 2; cc.logits_compact = 1; }
    // a ranking request (realise_engine_set_pred; models.py:1343-1346): the cross-entropy pass also writes the arg-max of the active
    // rows, their labels and the hit count, entry j for the j-th active row.  Where the gradient rows are not compacted (an evaluation
    // forward with logits, key 4 off) the active rows are listed for the request alone.
    CePred pr;
    const bool ranking = pred_req.pred_ids != nullptr;
    if (ranking) {
      pr.pred = pred_req.pred_ids; pr.labels_out = pred_req.labels; pr.hits = pred_req.hits; pr.n_active = pred_req.n_active; pr.capacity = pred_req.capacity;
      if (!compact) {
        CeCompact c1; c1.act_idx = act; c1.inv = wp<int>(pl.cls_inv); c1.n_act = n_act; c1.phase = 1;
        RL_TRY(ce_loss<T>(st, nullptr, Vp, b.tgt_idx, b.loss_masks, Tk, V, b.loss_out, wp<float>(pl.count), wp<T>(pl.dlogits), wp<float>(pl.loss_internal), Vp, c1));
        pr.inv = wp<int>(pl.cls_inv); pr.n_src = n_act;
      }
    }
    RL_TRY(ce_loss<T>(st, logits, ldl, b.tgt_idx, b.loss_masks, Tk, V, b.loss_out, wp<float>(pl.count),
                      b.want_dlogits ? wp<T>(pl.dlogits) : nullptr, wp<float>(pl.loss_internal), Vp, cc, ranking ? &pr : nullptr));
    hs.compact = compact; hs.dec_in = dec_in; hs.head_in = head_in;
    if (compact && !loss_rows) {      // the weight gradients read their input rows compacted; the MLM head's saved tensors stay where they are
      RL_TRY(gather_listed_rows<T>(st, dec_in, act, n_act, Tk, H, wp<T>(pl.cls_xc)));
      hs.dec_in = wp<T>(pl.cls_xc);
      if (vr.mlm_head) {
        RL_TRY(gather_listed_rows<T>(st, head_in, act, n_act, Tk, H, wp<T>(pl.head_xc)));
        hs.head_in = wp<T>(pl.head_xc); hs.row_map = act;
      }
    }
    have_fwd = b.training && b.want_dlogits;
    return RL_OK;
  }
  // ---------------------------------------------------------------- token tables (evaluation: pho_gru and res_h rows by token id)
  realise_token_tables tok = realise_token_tables();      // both pointers NULL: none installed
  bool tok_on() const { return tok.pho != nullptr || tok.res != nullptr; }
  // what a table set must be for this model; set and fill refuse the same things
  bool tables_ok(const realise_token_tables& t) const {
    if (!vr.arch || (!vr.pho && !vr.res)) return false;                       // no side branch (SpellBert, the bare ablation), Pho2Pretrain
    if (t.rows != V || t.ld < H || (t.ld & 7) || (H & 7)) return false;
    return (t.pho != nullptr) == vr.pho && (t.res != nullptr) == vr.res;
  }
  int set_token_tables(const realise_token_tables* t) override {
    if (t == nullptr) { tok = realise_token_tables(); return RL_OK; }
    if (!tables_ok(*t)) return RL_ERR_ARG;
    tok = *t;
    return RL_OK;
  }
  // the glyph branch of a forward up to the row the fusion reads: tower over the distinct glyphs, resnet_layernorm per token -> pl.res_h
  int res_rows_forward(hipStream_t st) {
    const T* res = nullptr;
    RL_TRY(resnet_forward(st, last.src_idx, &res));
    LnFwdArgs<T> ln; ln.rows = pl.B * pl.S; ln.H = H; ln.x = res; ln.row_index = wp<int>(pl.gu_inv);      // token t reads its glyph's row
    ln.gamma = pp(L.res_ln_g); ln.beta = pp(L.res_ln_b); ln.eps = cfg.ln_eps;
    ln.y = wp<T>(pl.res_h); ln.xhat = bwd_follows() ? wp<T>(pl.res_xhat) : nullptr; ln.rstd = wp<float>(pl.res_rstd);
    // a 2x2 top (CharResNet1): the rows arrive [p][c], the LayerNorm stores them in the reference's c * 4 + p feature order
    if (L.tower.top_pixels() == 4) return ln_fwd_chw4<T>(st, ln);
    return ln_fwd<T>(st, ln);
  }
  // host / device counts of the GRU's live rows per step, from the batch (forward() and fill_token_tables())
  void take_alive(const realise_batch& b, int Tp) {
    last_alive.assign(Tp, 0);
    if (vr.pho) for (int t = 0; t < Tp; ++t) last_alive[t] = b.n_alive ? b.n_alive[t] : b.B * b.S;
    alive_dev = (vr.pho && !b.n_alive) ? b.n_alive_dev : nullptr;
  }
  int fill_token_tables(hipStream_t st, const realise_batch& b, const realise_token_tables& t) override {
    if (!sh || !ws || !tables_ok(t) || !b.src_idx) return RL_ERR_ARG;
    if (b.B < 1 || b.S < 1 || b.S > cfg.max_pos) return RL_ERR_ARG;
    const int Tp = vr.pho ? b.Tp : 1;
    if (vr.pho && (Tp < 1 || !b.pho_idx || !b.pho_perm || !b.pho_lens_sorted || (!b.n_alive && !b.n_alive_dev))) return RL_ERR_ARG;
    have_fwd = false; hs = HeadSaved(); have_glyph_fwd = false;      // the branch activations of an earlier forward are about to be overwritten
    if (pl.B != b.B || pl.S != b.S || pl.Tp != Tp) RL_TRY(install_plan(st, make_plan(b.B, b.S, Tp)));
    last = realise_batch();
    last.B = b.B; last.S = b.S; last.Tp = Tp; last.training = 0;
    last.pho_perm = b.pho_perm; last.pho_lens_sorted = b.pho_lens_sorted;
    dead_ok = false; rows_live = false;
    RL_TRY(sync_optimizer(st));
    RL_TRY(wait_shadows(st));
    take_alive(b, Tp);
    const int Tk = b.B * b.S;
    RL_TRY(sanitize_ids(st, b.src_idx, Tk, V, wp<int64_t>(pl.ids_clean), id_flag));
    last.src_idx = wp<int64_t>(pl.ids_clean);
    if (vr.pho) {
      RL_TRY(sanitize_ids(st, b.pho_idx, (int64_t)Tk * Tp, cfg.pho_vocab, wp<int64_t>(pl.pho_clean), id_flag));
      last.pho_idx = wp<int64_t>(pl.pho_clean);
      RL_TRY(gru_forward(st));
    }
    if (vr.res) RL_TRY(res_rows_forward(st));
    return token_scatter<T>(st, last.src_idx, Tk, H, vr.pho ? wp<T>(pl.gru_out) : nullptr, (T*)t.pho, vr.res ? wp<T>(pl.res_h) : nullptr,
                            (T*)t.res, t.ld);
  }
  int forward(hipStream_t st, const realise_batch& b) override {
    if (!sh || !ws) return RL_ERR_ARG;
    if (b.B < 1 || b.S < 1 || b.S > cfg.max_pos) return RL_ERR_ARG;       // (S > 128: the tiled attention kernels, attention.hip)
    if (tok_on() && b.training) return RL_ERR_ARG;                         // the tables stand for evaluation-form branches only
    const bool by_id = tok_on();                                           // neither the GRU nor the tower runs: the batch needs no pinyin
    const int Tp = vr.pho ? (by_id && b.Tp < 1 ? 1 : b.Tp) : 1;
    if (vr.pho && !by_id && (Tp < 1 || !b.pho_idx || !b.pho_perm || !b.pho_lens_sorted || (!b.n_alive && !b.n_alive_dev))) return RL_ERR_ARG;
    have_fwd = false; hs = HeadSaved();      // whatever happens below, a backward finds nothing of the forward before this one
    HeadMode mode;
    RL_TRY(head_mode(b, &mode));
    if (pl.B != b.B || pl.S != b.S || pl.Tp != Tp) {
      RL_TRY(install_plan(st, make_plan(b.B, b.S, Tp)));
    }
    last = b;
    last.Tp = Tp;
    RL_TRY(wait_opt(st, 0));           // a pipelined optimizer sweep: its first piece holds everything the first kernels read
    have_glyph_fwd = false;            // the activations a glyph_backward would read are about to be overwritten
    dead_ok = false; rows_live = false;
    // host counts (the reference's contract: pho_lens is a host list) or, after realise_build_pho, device counts: every
    // step is then launched over all B*S rows and bounded on the device
    if (by_id) { last_alive.assign(Tp, 0); alive_dev = nullptr; } else take_alive(b, Tp);
    last.n_alive = nullptr;
    const int Tk = b.B * b.S;
    RL_TRY(mask_to_additive(st, b.masks, wp<float>(pl.mask_add), Tk));
    // everything below (and the backward) reads range-checked copies of the ids: a bad id raises in the module, never faults here
    RL_TRY(sanitize_ids(st, b.src_idx, Tk, V, wp<int64_t>(pl.ids_clean), id_flag));
    last.src_idx = wp<int64_t>(pl.ids_clean);
    if (vr.pho && !by_id) {
      RL_TRY(sanitize_ids(st, b.pho_idx, (int64_t)Tk * Tp, cfg.pho_vocab, wp<int64_t>(pl.pho_clean), id_flag));
      last.pho_idx = wp<int64_t>(pl.pho_clean);
    } else {
      last.pho_idx = nullptr; last.pho_perm = nullptr; last.pho_lens_sorted = nullptr;      // (a batch may carry pinyin nobody reads)
    }
    // Rows after a sentence's last real / loss position are padding no query attends to and no loss term reads: every backward
    // activation row there is an exact zero (the embedding scatter has relied on it since round 1).  The backward skips them
    // (LayerNorm backward rows, blocks of the weight-gradient reductions), and a live-row step (g_live_rows) does not compute
    // their forward activations in the transformer stacks either.
    dead_ok = b.tgt_idx != nullptr && b.loss_masks != nullptr && g_skip_dead && b.want_dlogits && b.masks != nullptr && (Tk % 64) == 0 &&
              Tk / live_list_rows() <= TN_LIST_MAX_ENTRIES;      // (the weight-gradient kernels keep the block list in LDS: beyond 65536 bf16 token rows the step is dense)
    if (dead_ok) RL_TRY(fill_live_tables(st, b));
    // (the weight gradients of a live-row step must walk the same block list - only the grouped launch takes one: ADVICE round 4)
    rows_live = dead_ok && b.training && g_wgrad_group && live_step_ok(Tk);
    // Round 6, opt-in (realise_batch.eval_live_rows): an EVALUATION forward over the live rows as well.  The reference's evaluation reads
    // the predictions of a sentence's real tokens only (run.py:262-270 cuts them at `lengths`; the loss counts loss_masks rows), so the
    // transformer stacks need not compute the padding rows behind a sentence's last attended / loss position: their logits rows come
    // out finite and meaningless, every other row and the loss bit-identical to the dense forward's (same kernels per row).
    if (!b.training && !dead_ok && b.eval_live_rows && b.masks != nullptr && live_step_ok(Tk)) {
      RL_TRY(fill_live_tables(st, b));
      dead_ok = true; rows_live = true;      // (the tables exist; no backward follows an evaluation forward)
    }
    const T* bert_h = nullptr;
    // (with no side branch - the ablation model with neither - there is nothing to fork: everything stays on the caller's stream)
    const bool ovl = vr.arch && branch_mask() != 0 && g_branch_overlap && branches_ok();
    hipStream_t s_pho = ovl ? bst[0] : st, s_glyph = ovl ? bst[1] : st;
    // operand copies refreshed on the branch streams (refresh_shadows): with the branch streams in use below, each branch is already
    // ordered behind its own copies and the caller's stream meets the classifier / output-stack copies at the join; otherwise wait here
    if (!ovl) RL_TRY(wait_shadows(st));
    if (ovl) RL_TRY(fork(st));                                    // bert | pinyin GRU + pho_model | glyph ResNet
    // Enqueue order (g_fwd_order): the host needs ~0.6 ms to enqueue the 150 launches of the bert stack; enqueued first (0) the two
    // shorter branches reach the GPU only after that, enqueued last (1) they start at once and bert joins them ~0.4 ms later.
    if (vr.bert && !(ovl && g_fwd_order == 1)) RL_TRY(stack_forward(st, 0, L.bert, sh_bert, pl.bert, last.src_idx, nullptr, 0, &bert_h));
    const T* top = bert_h;
    if (!vr.bert) {      // Pho2Pretrain (models.py:1327-1336): pinyin GRU -> pho_model on the caller's stream - there is nothing to fork
      RL_TRY(sync_optimizer(st));
      RL_TRY(gru_forward(st));
      RL_TRY(stack_forward(st, 1, L.pho, sh_pho, pl.pho, nullptr, wp<T>(pl.gru_out), 0, &top));
    }
    if (vr.arch) {
      if (vr.pho) {
        RL_TRY(wait_opt(s_pho, opt_groups));                        // (pipelined sweep: pinyin / output stacks and the GRU are one piece)
        if (!by_id) RL_TRY(gru_forward(s_pho));
        const T* pho_h = nullptr;
        // token tables: the embedding LayerNorm of pho_model reads the GRU rows by token id - no GRU step, no pass of its own
        RL_TRY(stack_forward(s_pho, 1, L.pho, sh_pho, pl.pho, nullptr, wp<T>(pl.gru_out), 0, &pho_h, by_id ? (const T*)tok.pho : nullptr, tok.ld));
      }
      if (vr.res) {
        // token tables: res_h is a copy of the table's rows - no glyph gather, tower or resnet_layernorm
        if (by_id) RL_TRY(token_copy<T>(s_glyph, (const T*)tok.res, tok.ld, last.src_idx, Tk, H, wp<T>(pl.res_h), H));
        else RL_TRY(res_rows_forward(s_glyph));
      }
      if (ovl && g_fwd_order == 1) { RL_TRY(stack_forward(st, 0, L.bert, sh_bert, pl.bert, last.src_idx, nullptr, 0, &bert_h)); top = bert_h; }
      if (ovl) RL_TRY(join(st));
      RL_TRY(sync_optimizer(st));                                   // every piece of a pipelined sweep is now in front of this stream
      if (vr.gate) RL_TRY(gate_fwd<T>(st, gate_args()));
      else if (vr.concat) RL_TRY(concat_fwd(st, bert_h));
      else RL_TRY(sum_fuse_fwd<T>(st, bert_h, wp<T>(pl.pho.layers.back().y2), wp<T>(pl.res_h), wp<T>(pl.fused), Tk, H));
      RL_TRY(stack_forward(st, 2, L.outb, sh_out, pl.outb, nullptr, wp<T>(pl.fused), 1, &top));
    }
    RL_TRY(sync_optimizer(st));
    return head_fwd(st, b, mode, top);
  }

  // ---------------------------------------------------------------- glyph-only entry points (BASELINE configs[3])
  // CharResNet alone (src/char_cnn.py:46-55) on the B*S glyph stacks selected by src_idx (src/models.py:829-836):
  // res_out[t, :] = resnet(char_images_multifonts[src_idx[t]]), before resnet_layernorm.
  bool have_glyph_fwd = false;
  int glyph_forward(hipStream_t st, const int64_t* ids, int B, int S, int training, void* res_out) override {
    if (!sh || !ws || !vr.res || !ids || !res_out || B < 1 || S < 1) return RL_ERR_ARG;
    RL_TRY(sync_optimizer(st));
    if (pl.B != B || pl.S != S || pl.Tp != -1) {
      RL_TRY(install_plan(st, make_plan(B, S, -1)));
    }
    last = realise_batch();
    last.B = B; last.S = S; last.Tp = 1; last.training = training;
    RL_TRY(wait_shadows(st));
    RL_TRY(sanitize_ids(st, ids, (int64_t)B * S, V, wp<int64_t>(pl.ids_clean), id_flag));
    last.src_idx = wp<int64_t>(pl.ids_clean);
    have_fwd = false; have_glyph_fwd = false;
    const T* res = nullptr;
    RL_TRY(resnet_forward(st, last.src_idx, &res));
    if (L.tower.top_pixels() == 4) RL_TRY(gather_rows_chw4<T>(st, res, wp<int>(pl.gu_inv), B * S, H, (T*)res_out));
    else RL_TRY(gather_rows<T>(st, res, wp<int>(pl.gu_inv), B * S, H, (T*)res_out));
    have_glyph_fwd = training != 0;
    return RL_OK;
  }
  // accumulates the gradients of the 15 conv / BatchNorm parameter tensors for d_res [B*S, 768] (per token)
  int glyph_backward(hipStream_t st, const void* d_res) override {
    if (!have_glyph_fwd || !d_res) { fprintf(stderr, "[realise_hip] glyph_backward without a training glyph_forward\n"); return RL_ERR_ARG; }
    RL_TRY(sync_optimizer(st));
    RL_TRY(begin_gradient_pass(st, true));
    RL_TRY(top_segment_sum(st, (const T*)d_res));
    RL_TRY(resnet_backward(lane(0, st), wp<T>(pl.r_dout)));
    return RL_OK;
  }

  // ---------------------------------------------------------------- fresh gradients (zero_grad() without a 680 MB memset)
  // After zero_grad() the module only tells the engine that the gradient arena holds nothing (set_grads_fresh).  The next
  // backward then (a) zero-fills, in ONE launch, everything EXCEPT the Linear weight gradients of the transformer layers - 80 % of
  // the arena -, and (b) lets the grouped weight-gradient GEMM store those instead of adding to them: no fill of those bytes and no
  // read-modify-write in its epilogue.  Accumulating backwards (no zero_grad() in between) run exactly as before.
  bool grads_fresh = false, pass_overwrite = false, fill_built = false;
  int n_fill = 0;
  void set_grads_fresh(int fresh) override { grads_fresh = fresh != 0; }
  int begin_gradient_pass(hipStream_t st, bool glyph_only) {
    pass_overwrite = false;
    if (!grads_fresh) return RL_OK;
    grads_fresh = false;
    const int64_t total = L.arena_elems[AR_TRAIN];
    if (glyph_only || !g_wgrad_group || !sh) return fill_f32(st, G, 0.0f, total);
    if (!fill_built) {
      std::vector<std::pair<int64_t, int64_t>> skip;          // [begin, end) of the tensors the grouped launches overwrite
      auto add_stack = [&](const StackOff& so) {
        for (const LayerOff& o : so.layers) {
          skip.push_back({o.qkv_w, o.qkv_w + 3LL * H * H}); skip.push_back({o.ao_w, o.ao_w + (int64_t)H * H});
          skip.push_back({o.in_w, o.in_w + (int64_t)I * H}); skip.push_back({o.out_w, o.out_w + (int64_t)H * I});
        }
      };
      add_stack(L.bert);
      if (vr.pho) add_stack(L.pho);
      if (vr.arch) add_stack(L.outb);
      std::sort(skip.begin(), skip.end());
      fill_host.clear();
      int64_t at = 0;
      auto emit = [&](int64_t b, int64_t e) {
        for (int64_t o = b; o < e; o += (1 << 20)) fill_host.push_back(FillChunk{o, (int32_t)std::min<int64_t>(1 << 20, e - o), 0});
      };
      for (auto& r : skip) { if (r.first > at) emit(at, r.first); at = std::max(at, r.second); }
      if (at < total) emit(at, total);
      if ((int)fill_host.size() > FILL_MAX) return fill_f32(st, G, 0.0f, total);
      if (hipMemcpyAsync(sh + sh_fill, fill_host.data(), fill_host.size() * sizeof(FillChunk), hipMemcpyHostToDevice, st) != hipSuccess) return RL_ERR_LAUNCH;
      n_fill = (int)fill_host.size(); fill_built = true;
    }
    RL_TRY(zero_chunks(st, G, (const FillChunk*)(sh + sh_fill), n_fill));
    pass_overwrite = true;
    return RL_OK;
  }
  std::vector<FillChunk> fill_host;

  // ---------------------------------------------------------------- backward, in bucket-sized stages
  int n_stages() const { return (int)L.buckets.size(); }

  // d loss arriving at backward() as a DEVICE scalar (nullptr: 1): the head's three gradients are linear in it, so it is applied where
  // they leave the head - the classifier's weight / bias gradient epilogues (TnEpi::alpha_dev) and the scatter that writes d(top
  // hidden) - instead of a read-modify-write pass over the ~200 MB of cross-entropy gradient rows
  const float* loss_grad = nullptr;
  void set_loss_grad(const float* g) override { loss_grad = g; }
  realise_decode dec_req = realise_decode();      // k == 0: no decode request installed
  void set_decode(const realise_decode* d) override { if (d) dec_req = *d; else dec_req = realise_decode(); }
  realise_pred pred_req = realise_pred();         // pred_ids == nullptr: no ranking request installed
  void set_pred(const realise_pred* d) override { if (d) pred_req = *d; else pred_req = realise_pred(); }
  // The decoder's / classifier's data gradient (K = Vp: the padding columns are exact zeros on both sides), the one place that chooses
  // between its two forms and applies the loss-gradient scalar.  Compacted bf16 rows of 1024 and more: split-K over the vocabulary,
  // the planes folded in plane order through fold_map into fold_out, scaled, with fold_drop (*folded = true).  Otherwise, and when the
  // split launcher refuses the shape: one launch into `out`, scaled here (scale_out) or left to a scatter that scales as it stores.
  int head_dgrad(hipStream_t st, const int* n_act, T* out, bool scale_out, const int* fold_map, T* fold_out, const DropParams& fold_drop, bool* folded) {
    const int Tk = pl.B * pl.S;
    const T* dl = wp<T>(pl.dlogits);
    *folded = false;
    if constexpr (sizeof(T) == 2) {
      const int ns = g_cls_splitk;
      if (hs.compact && ns >= 2 && pl.cls_slab != 0 && Tk >= 1024 &&
          gemm_nt8_splitk(st, dl, Vp, sp<T>(sh_cls_wT), Vp, Tk, H, Vp, ns, wp<float>(pl.cls_slab), (int64_t)Tk * H, n_act) == RL_OK) {
        *folded = true;
        return scatter_rows_drop_slab<T>(st, wp<float>(pl.cls_slab), ns, (int64_t)Tk * H, fold_map, Tk, H, fold_out, fold_drop, loss_grad);
      }
    }
    EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = out; ep.ldo = H; ep.m_dev = n_act;
    RL_TRY(gemm_nt<T>(st, dl, Vp, sp<T>(sh_cls_wT), Vp, Tk, H, Vp, ep));
    if (scale_out && loss_grad != nullptr) RL_TRY(scale_by_dev<T>(st, out, (int64_t)Tk * H, loss_grad));      // (a pass over [T, H], not over the logits)
    return RL_OK;
  }
  // The head's backward; leaves d(top hidden) in gA.  Reads hs and nothing else about the forward.  Plain classifier: weight / bias
  // gradient, data gradient, the finish.  MLM head (modeling_bert.py:419-462): between the decoder's data gradient and the finish ONE row
  // pass for LayerNorm' and GELU' (ln_gelu_bwd), the transform's weight gradient with its bias gradient as the column sum, and its data
  // gradient.  The loss-gradient scalar reaches the decoder's weight and bias gradients in their epilogue; everything behind the
  // decoder gets it through the decoder's DATA gradient, scaled once where it is stored: dz, the transform's four gradients and
  // d(top hidden) are linear in it and get no factor of their own.  (The plain compacted form scales in the scatter that follows.)
  int stage_head(const Lane& la) {
    const hipStream_t st = la.st;
    const int Tk = pl.B * pl.S;
    T* gA = wp<T>(pl.gA);
    T* dy = wp<T>(pl.cls_gc);      // compacted rows, and the MLM head's dense ones: d(decoder input), then d(head input)
    const DropParams dfin = site(5000, cfg.hidden_dropout);
    const int* n_act = hs.compact ? wp<int>(pl.cls_nact) : nullptr;
    const int* inv = wp<int>(pl.cls_inv);
    { TnEpi te; te.slab = wp<float>(la.sc->tn_slab); te.slab_elems = TN_SLAB_ELEMS; te.colsum = gp(L.cls_b); te.out = gp(L.cls_w); te.ldo = H;
      te.alpha_dev = loss_grad;
      RL_TRY(gemm_tn<T>(st, wp<T>(pl.dlogits), Vp, hs.dec_in, H, Tk, V, H, te, n_act)); }
    const float* scale = nullptr;  // the loss-gradient scalar, where the scatter still has to apply it
    bool folded = false;
    if (vr.mlm_head) {             // the planes fold into the compacted rows where they are (head_ident)
      T* dz = wp<T>(pl.head_dz);
      RL_TRY(head_dgrad(st, n_act, dy, true, wp<int>(pl.head_ident), dy, DropParams(), &folded));
      { LnGeluBwdArgs<T> a; a.rows = Tk; a.H = H; a.n_dev = n_act; a.idx = hs.row_map; a.saved_rows = Tk;
        a.dy = dy; a.xhat = wp<T>(pl.head_x); a.rstd = wp<float>(pl.head_rstd); a.z = wp<T>(pl.head_z); a.gamma = pp(L.head_ln_g); a.dz = dz;
        a.dgamma = gp(L.head_ln_g); a.dbeta = gp(L.head_ln_b); a.slots = ln_region(la, LN_FOLD_MAX);
        RL_TRY(ln_gelu_bwd<T>(st, a)); }
      { TnEpi te; te.slab = wp<float>(la.sc->tn_slab); te.slab_elems = TN_SLAB_ELEMS; te.colsum = gp(L.head_b); te.out = gp(L.head_w); te.ldo = H;
        RL_TRY(gemm_tn<T>(st, dz, H, hs.head_in, H, Tk, H, H, te, n_act)); }
      EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = hs.compact ? dy : gA; ep.ldo = H; ep.m_dev = n_act;      // (dy is consumed: its buffer takes d(head input), compacted)
      RL_TRY(gemm_nt<T>(st, dz, H, sp<T>(sh_head_wT), H, Tk, H, H, ep));
    } else {                       // the planes fold straight into gA through cls_inv with the final dropout's map: that is the finish
      RL_TRY(head_dgrad(st, n_act, hs.compact ? dy : gA, !hs.compact, inv, gA, dfin, &folded));
      if (folded) return RL_OK;
      scale = loss_grad;
    }
    if (hs.compact) return scatter_rows_drop<T>(st, dy, inv, Tk, H, gA, dfin, scale);      // rows outside the loss: zero; + the final dropout's map
    if (dfin.thresh) RL_TRY(dropout_apply<T>(st, gA, gA, Tk, H, dfin));
    return RL_OK;
  }

  // stages = gradient buckets.  SpellBert: bert layer groups | bert embeddings.  The Arch3 family: 0 output_block | 1 fusion (+ glyph
  // ResNet) | 2 pinyin branch (when present) | bert layer groups | bert embeddings.  Pho2Pretrain (no bert stack): 0 head | 1 pinyin branch
  int first_bert_stage() const { return !vr.arch ? 0 : (vr.pho ? 3 : 2); }
  int stage_out_block(const Lane& la) {      // head + output_block; leaves d fused in gB (set 0)
    T* gA = wp<T>(pl.gA);
    RL_TRY(stage_head(la));
    RL_TRY(layers_backward(la, 2, L.outb, sh_out, pl.outb, cfg.out_layers - 1, 0, gA));
    RL_TRY(emb_backward(la, 2, L.outb, pl.outb, nullptr, 1, gA, wp<T>(pl.sc[0].gB)));
    return RL_OK;
  }
  // Concatenation fusion (models.py:628-629, :228-229): fused = integrate([bert | pho | res]) as ONE GEMM over the K-segmented operand
  // (gemm_nt_cat: no [T, nH] tensor), over the live rows of a live-row step like every layer GEMM.
  int concat_fwd(hipStream_t st, const T* bert_h) {
    const T* a[SEG_MAX] = {bert_h, wp<T>(pl.pho.layers.back().y2), vr.res ? wp<T>(pl.res_h) : nullptr};
    const int64_t lda[SEG_MAX] = {H, H, H};
    EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = wp<T>(pl.fused); ep.ldo = H; ep.bias = pp(L.int_b);
    if constexpr (sizeof(T) == 4) ep.x3 = x3();
    if constexpr (sizeof(T) == 2) {
      if (rows_live && g_live_rows == 2) { ep.live_list = wp<int>(pl.live_rows); ep.live_count = wp<int>(pl.live_n) + 3; ep.live_unit = 1; }
      else if (rows_live) { ep.live_list = wp<int>(pl.live_t16); ep.live_count = wp<int>(pl.live_n) + 2; ep.live_unit = 16; }
    }
    return gemm_nt_cat<T>(st, vr.nsrc, a, lda, H, sp<T>(sh_int_w), (int64_t)vr.nsrc * H, pl.B * pl.S, H, ep);
  }
  // Its backward needs no kernel of its own.  d A_s = d fused . W[:, sH:(s+1)H] is a plain NT GEMM against rows sH.. of the transposed
  // copy, written straight into X1 / X2 / X3.  The launches are DENSE in a live-row step too: d fused (the output block's embedding
  // LayerNorm backward) holds exact zeros in every padding row, so the product leaves exact zeros there - what the gate backward
  // guarantees - without a pass of its own.  All of them run here, in front of the fork: they read gB of set 0, which the bert lane's
  // layers re-use as soon as they start.  The weight gradient is one grouped TN launch - problem s = column slice s of dW (pitch nH) -
  // over the live reduction tiles, the bias gradient its column sum; it accumulates (integrate is not among the tensors a fresh pass stores).
  int concat_bwd(hipStream_t st) {
    const int Tk = pl.B * pl.S, n = vr.nsrc;
    const T* df = wp<T>(pl.sc[0].gB);
    T* dx[SEG_MAX] = {wp<T>(pl.X1), wp<T>(pl.X2), vr.res ? wp<T>(pl.X3) : nullptr};
    const T* x[SEG_MAX] = {wp<T>(pl.bert.layers.back().y2), wp<T>(pl.pho.layers.back().y2), vr.res ? wp<T>(pl.res_h) : nullptr};
    TnGroupProblem<T> gp3[SEG_MAX];
    for (int s = 0; s < n; ++s) {
      EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = dx[s]; ep.ldo = H;
      RL_TRY(gemm_nt<T>(st, df, H, sp<T>(sh_int_wT) + (int64_t)s * H * H, H, Tk, H, H, ep));
      gp3[s].A = df; gp3[s].lda = H; gp3[s].B = x[s]; gp3[s].ldb = H; gp3[s].I = H; gp3[s].J = H;
      gp3[s].out = gp(L.int_w) + (int64_t)s * H; gp3[s].ldo = (int64_t)n * H; gp3[s].colsum = s == 0 ? gp(L.int_b) : nullptr;
    }
    return gemm_tn_group<T>(st, n, gp3, Tk, 1.0f, 0, live_tiles(), live_tile_count(), live_list_rows());
  }
  int stage_fuse(hipStream_t st) {           // d fused -> X1 (d bert), X2 (d pho), X3 (d res) [+ gate_net / integrate gradients]
    if (vr.concat) return concat_bwd(st);
    if (!vr.gate) return sum_fuse_bwd<T>(st, wp<T>(pl.sc[0].gB), wp<T>(pl.X1), wp<T>(pl.X2), wp<T>(pl.X3), pl.B * pl.S, H, live_rows());
    GateArgs<T> g = gate_args();
    g.dfused = wp<T>(pl.sc[0].gB); g.dbert = wp<T>(pl.X1); g.dz = wp<float>(pl.dz);
    g.dpho = vr.pho ? wp<T>(pl.X2) : nullptr; g.dres = vr.res ? wp<T>(pl.X3) : nullptr;
    g.dW = gp(L.gate_w); g.dbias = gp(L.gate_b); g.row_live = live_rows();
    return gate_bwd<T>(st, g);
  }
  // (the glyph lane needs a gE of its own: the LayerNorm backward below writes it while the bert lane's layers keep d ctx in theirs)
  int stage_glyph(const Lane& la) {          // resnet LayerNorm, segment sum over the tokens of a glyph, glyph ResNet
    const int Tk = pl.B * pl.S;
    LnBwdArgs<T> ln; ln.slots = ln_region(la, LN_FOLD_MAX); ln.rows = Tk; ln.H = H; ln.dy = wp<T>(pl.X3); ln.xhat = wp<T>(pl.res_xhat); ln.rstd = wp<float>(pl.res_rstd);
    ln.row_live = live_rows();
    ln.gamma = pp(L.res_ln_g); ln.dx = wp<T>(la.sc->gE); ln.dgamma = gp(L.res_ln_g); ln.dbeta = gp(L.res_ln_b);
    RL_TRY(ln_bwd<T>(la.st, ln));
    RL_TRY(top_segment_sum(la.st, wp<T>(la.sc->gE)));
    return resnet_backward(la, wp<T>(pl.r_dout));
  }
  int stage_pho(const Lane& la) {            // pho_model + GRU
    T* g2 = wp<T>(vr.arch ? pl.X2 : pl.gA);      // the gradient arrives from the fusion in X2, from the head (Pho2Pretrain) in gA
    T* gE = wp<T>(la.sc->gE);
    RL_TRY(layers_backward(la, 1, L.pho, sh_pho, pl.pho, cfg.pho_layers - 1, 0, g2));
    RL_TRY(emb_backward(la, 1, L.pho, pl.pho, nullptr, 0, g2, gE));       // gE = d gru_out (original order)
    return gru_backward(la, gE);
  }
  // bert layer group g (SpellBert, where no output block did it: group 0 runs the head first), or (g == groups) the bert embeddings
  int stage_bert(const Lane& la, int g) {
    T* g1 = wp<T>(vr.arch ? pl.X1 : pl.gA);      // the gradient arrives from the fusion in X1, from the head in gA
    if (g < L.bert_groups) {
      if (!vr.arch && g == 0) RL_TRY(stage_head(la));
      const int hi = cfg.bert_layers - 1 - 4 * g, lo = std::max(hi - 3, 0);
      return layers_backward(la, 0, L.bert, sh_bert, pl.bert, hi, lo, g1);
    }
    return emb_backward(la, 0, L.bert, pl.bert, last.src_idx, 0, g1, wp<T>(pl.sc[0].gB));
  }

  // A "bucket final" signal per gradient bucket: evs[i] (caller-owned hipEvent_t) is recorded once every kernel that writes into
  // bucket i has been enqueued, on the stream that runs last for that bucket - so a data-parallel caller can start the all-reduce of
  // bucket i on its own stream (hipStreamWaitEvent) while the three model branches and the deferred weight gradients keep running.
  std::vector<hipEvent_t> ev_sig;       // one per bucket (any number of bert groups)
  int signal_bucket(void* ev, hipStream_t s, bool through_side, int slot) {
    hipEvent_t e = (hipEvent_t)ev;
    if ((int)ev_sig.size() <= slot) ev_sig.resize(slot + 1, nullptr);
    if (through_side && g_wgrad_overlap && side_ok()) {      // the bert branch: its weight gradients finish on the side stream
      if (ev_sig[slot] == nullptr && hipEventCreateWithFlags(&ev_sig[slot], hipEventDisableTiming) != hipSuccess) return RL_ERR_LAUNCH;
      if (hipEventRecord(ev_sig[slot], s) != hipSuccess || hipStreamWaitEvent(side, ev_sig[slot], 0) != hipSuccess ||
          hipEventRecord(e, side) != hipSuccess) return RL_ERR_LAUNCH;
      return RL_OK;
    }
    return hipEventRecord(e, s) == hipSuccess ? RL_OK : RL_ERR_LAUNCH;
  }
  // The schedule of the backward, its only copy: stages first .. last_stage in order, each followed by its bucket signal when the
  // caller brought events (evs == nullptr: no signals).
  // Serial form: every stage on lane 0 of the caller's stream.
  // Branched form - the whole pass of an Arch3 model in one call (no per-bucket gradient exchange in between): the same stages, with
  // the glyph and the pinyin stage on lanes of their own (bst[1] / bst[0]), forked behind the fusion and joined after the last bert
  // stage, so the three branches behind the gate run concurrently.  (A bucket-by-bucket caller would serialise the branches and join
  // the weight-gradient stream at every bucket boundary: data-parallel callers use the signalled whole pass instead.)
  int backward_pass(hipStream_t st, int first, int last_stage, void* const* evs) {
    const bool branched = vr.arch && first == 0 && last_stage == n_stages() - 1 && g_branch_overlap && (branch_mask() == 0 || branches_ok());
    const Lane bert = lane(0, st);
    const Lane glyph = branched && vr.res ? lane(2, bst[1]) : bert, pho = branched && vr.pho ? lane(1, bst[0]) : bert;
    const int b0 = first_bert_stage();
    int rc = RL_OK;
    for (int s = first; rc == RL_OK && s <= last_stage; ++s) {
      hipStream_t fin = st;                  // the stream that runs last for bucket s
      if (!vr.bert) rc = s == 0 ? stage_head(bert) : stage_pho(pho);      // Pho2Pretrain: 0 head | 1 pinyin branch, nothing else exists
      else if (s >= b0) rc = stage_bert(bert, s - b0);
      else if (s == 0) rc = stage_out_block(bert);
      else if (s == 1) {                     // fusion (before the fork) + glyph ResNet
        rc = stage_fuse(st);
        if (rc == RL_OK && branched) rc = fork(st);
        if (rc == RL_OK && vr.res) { rc = stage_glyph(glyph); fin = glyph.st; }
      } else { rc = stage_pho(pho); fin = pho.st; }
      if (evs == nullptr || rc != RL_OK) continue;
      // The one difference between the serial forms: with bucket signals the side stream is joined after every stage, before the
      // signal is recorded; without, once at the end.  Branched, nothing is joined in between: a bucket whose layers ran on the bert
      // lane (output block, bert stages) is signalled through the side stream, where its weight gradients finish.
      if (!branched) rc = join_side(st);
      if (rc == RL_OK) rc = signal_bucket(evs[s], fin, branched && (s == 0 || s >= b0), s);
    }
    if (!branched) return rc != RL_OK ? rc : join_side(st);          // the caller's stream owns every gradient of these stages once this returns
    const int rj = join(st);
    const int rs = join_side(st);
    return rc != RL_OK ? rc : (rj != RL_OK ? rj : rs);
  }
  int backward_signalled(hipStream_t st, void* const* evs, int n_events) override {
    if (!have_fwd) { fprintf(stderr, "[realise_hip] backward without a training forward (tgt_idx + want_dlogits)\n"); return RL_ERR_ARG; }
    const int n = n_stages();
    if (n_events != n || evs == nullptr) return RL_ERR_ARG;
    for (int i = 0; i < n; ++i) if (evs[i] == nullptr) return RL_ERR_ARG;
    RL_TRY(begin_gradient_pass(st, false));
    return backward_pass(st, 0, n - 1, evs);
  }
  int backward(hipStream_t st, int first, int last_stage) override {
    if (!have_fwd) { fprintf(stderr, "[realise_hip] backward without a training forward (tgt_idx + want_dlogits)\n"); return RL_ERR_ARG; }
    const int n = n_stages();
    if (last_stage < 0) last_stage = n - 1;
    if (first < 0 || last_stage >= n || first > last_stage) return RL_ERR_ARG;
    if (first == 0) RL_TRY(begin_gradient_pass(st, false));           // (a bucket-by-bucket caller starts its pass with stage 0)
    return backward_pass(st, first, last_stage, nullptr);
  }
};

EngineBase* make_engine(const realise_config& c, float* p, float* g, float* pu, float* fz, float* bf, int64_t* bi) {
  if (c.hidden % 64 || c.hidden / c.heads != 64 || c.hidden > 1024 || (c.intermediate % 8) || (c.vocab % 8)) return nullptr;
  if (!config_ok(c)) return nullptr;
  if (variant_of(c).res) {      // the flattened tower output is the hidden state: 768 x 1 x 1 (char_cnn.py:44) or 192 x 2 x 2 (char_cnn.py:74)
    if (c.hidden != tower_of(c).features()) return nullptr;
  }
  if (c.dtype == REALISE_BF16) return new Engine<bf16_t>(c, p, g, pu, fz, bf, bi);
  if (c.dtype == REALISE_F32 || c.dtype == REALISE_F32_BF16X3) return new Engine<float>(c, p, g, pu, fz, bf, bi);      // (x3(): the flag)
  return nullptr;
}

}  // namespace rl
