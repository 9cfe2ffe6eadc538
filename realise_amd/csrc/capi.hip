// extern "C" surface of librealise_hip.so (declared in include/realise_hip.h; diagnostics in include/realise_hip_debug.h).
#include <math.h>
#include <string.h>

#include "attention.h"
#include "engine.h"
#include "gemm.h"
#include "layout.h"
#include "ops.h"
#include "prof.h"
#include "../../include/realise_hip_debug.h"

using namespace rl;
#define RL_TRY(expr) do { const int _rc = (expr); if (_rc != RL_OK) return _rc; } while (0)

struct realise_engine { EngineBase* impl; };

namespace {
// The one dtype ladder of this file: returns the expression, compiled with E = bf16_t or E = float.  REALISE_F32_BF16X3 (fp32 buffers, the
// dense GEMMs multiply split-bf16: EpiParams::x3 / TnEpi::x3) becomes E = float with x3 = 1 here and nowhere else, and only where X3_OK
// is set: every other entry point refuses it like an unknown dtype.
#define RL_BY_DTYPE_OR(REFUSED, X3_OK, ...) do { \
    if (dtype == REALISE_BF16) { using E = bf16_t; const int x3 = 0; (void)x3; return (__VA_ARGS__); } \
    if (dtype == REALISE_F32 || ((X3_OK) && dtype == REALISE_F32_BF16X3)) { using E = float; const int x3 = dtype == REALISE_F32_BF16X3; (void)x3; return (__VA_ARGS__); } \
    return (REFUSED); } while (0)
#define RL_BY_DTYPE(X3_OK, ...) RL_BY_DTYPE_OR(RL_ERR_ARG, X3_OK, __VA_ARGS__)

template <typename T> EpiParams<T> to_epi(const realise_epilogue* e, int x3 = 0, const float* col_scale = nullptr, int relu = 0) {
  EpiParams<T> p;
  p.x3 = x3; p.col_scale = col_scale; p.relu = relu;
  if (!e) return p;
  p.mode = e->mode; p.accumulate = e->accumulate; p.out = (T*)e->out; p.ldo = e->ldo; p.out2 = (T*)e->out2;
  p.bias = e->bias; p.aux = (const T*)e->aux; p.ldaux = e->ldaux; p.alpha = e->alpha;
  p.drop_seed = e->drop_seed; p.drop_thresh = e->drop_thresh; p.drop_scale = e->drop_scale;
  return p;
}
template <typename T> ConvLoader<T> to_geom(const realise_conv_geom* g, const int* rows_dev = nullptr, int64_t index_rows = 0) {
  ConvLoader<T> c;
  c.src = (const T*)g->src; c.img_index = g->img_index; c.rows = g->rows; c.Hr = g->Hr; c.Wr = g->Wr; c.Hs = g->Hs; c.Ws = g->Ws;
  c.C = g->C; c.KH = g->KH; c.KW = g->KW; c.stride = g->stride; c.pad = g->pad; c.mode = g->mode;
  c.rows_dev = rows_dev; c.index_rows = index_rows;
  c.finalize();
  return c;
}
template <typename T> int cat_launch(hipStream_t st, const realise_gemm_cat* g, int x3) {      // (nsrc is in range: the caller checked)
  const T* a[SEG_MAX];
  for (int s = 0; s < g->nsrc; ++s) a[s] = (const T*)g->a[s];
  EpiParams<T> ep;
  ep.x3 = x3; ep.out = (T*)g->out; ep.ldo = g->ldo; ep.bias = g->bias;
  ep.live_list = g->live_list; ep.live_count = g->live_count; ep.live_unit = g->live_unit;
  return gemm_nt_cat<T>(st, g->nsrc, a, g->lda, g->Ks, (const T*)g->w, g->ldw, g->M, g->N, ep);
}
TnEpi with_x3(TnEpi te, int x3) { te.x3 = x3; return te; }
template <typename T>
int tn_grouped(hipStream_t st, int n, const realise_tn_problem* pr, int P, int x3, const int* live = nullptr, const int* n_live = nullptr,
               int list_rows = 0, int overwrite = 0) {
  if (n < 1 || n > TN_GROUP_MAX || pr == nullptr) return RL_ERR_ARG;
  TnGroupProblem<T> g[TN_GROUP_MAX];
  for (int k = 0; k < n; ++k) {
    g[k].A = (const T*)pr[k].A; g[k].lda = pr[k].lda; g[k].B = (const T*)pr[k].B; g[k].ldb = pr[k].ldb;
    g[k].I = pr[k].I; g[k].J = pr[k].J; g[k].out = pr[k].out; g[k].ldo = pr[k].ldo; g[k].colsum = pr[k].colsum;
  }
  return gemm_tn_group<T>(st, n, g, P, 1.0f, overwrite, live, n_live, list_rows, x3);
}
template <typename T>
LnFwdArgs<T> to_ln_fwd(const void* x, const float* gamma, const float* beta, float eps, void* y, void* xhat, float* rstd, int rows, int H,
                       const uint8_t* row_live = nullptr, const int32_t* row_index = nullptr) {
  LnFwdArgs<T> a; a.rows = rows; a.H = H; a.x = (const T*)x; a.row_index = (const int*)row_index; a.gamma = gamma; a.beta = beta; a.eps = eps;
  a.y = (T*)y; a.xhat = (T*)xhat; a.rstd = rstd; a.row_live = row_live;
  return a;
}
// the two gathers of an evaluation forward with token tables: every refusal here, before the first launch
template <typename T> int token_rows_launch(hipStream_t st, const realise_token_rows_args* a) {
  if (a->pho_table) {
    LnFwdArgs<T> ln;
    ln.rows = a->T; ln.H = a->H; ln.S = a->S; ln.in_mode = 3; ln.x = (const T*)a->pho_table; ln.ld_in = a->ld; ln.ids = a->ids;
    ln.pos = a->pos; ln.type0 = a->type0; ln.gamma = a->gamma; ln.beta = a->beta; ln.eps = a->eps;
    ln.y = (T*)a->pho_out; ln.ldy = a->ld_pho_out;
    const int rc = ln_fwd<T>(st, ln);
    if (rc != RL_OK) return rc;
  }
  if (a->res_table) return token_copy<T>(st, (const T*)a->res_table, a->ld, a->ids, a->T, a->H, (T*)a->res_out, a->ld_res_out);
  return RL_OK;
}
template <typename T>
LnBwdArgs<T> to_ln_bwd(const void* dy, const void* xhat, const float* rstd, const float* gamma, void* dx, float* dgamma, float* dbeta, int rows, int H,
                       void* dx_drop = nullptr, DropParams out_drop = DropParams(), float* slots = nullptr, const uint8_t* row_live = nullptr) {
  LnBwdArgs<T> a; a.rows = rows; a.H = H; a.dy = (const T*)dy; a.xhat = (const T*)xhat; a.rstd = rstd; a.gamma = gamma; a.dx = (T*)dx;
  a.dx_drop = (T*)dx_drop; a.out_drop = out_drop; a.dgamma = dgamma; a.dbeta = dbeta; a.slots = slots; a.row_live = row_live;
  return a;
}
template <typename T>
LnGeluBwdArgs<T> to_ln_gelu_bwd(const void* dy, const void* xhat, const float* rstd, const void* z, const float* gamma, void* dz, float* dgamma,
                                float* dbeta, int rows, int H, const int32_t* n_rows_dev, const int32_t* row_index, int saved_rows) {
  LnGeluBwdArgs<T> a; a.rows = rows; a.H = H; a.n_dev = n_rows_dev; a.idx = row_index; a.saved_rows = saved_rows;
  a.dy = (const T*)dy; a.xhat = (const T*)xhat; a.rstd = rstd; a.z = (const T*)z; a.gamma = gamma; a.dz = (T*)dz;
  a.dgamma = dgamma; a.dbeta = dbeta;
  return a;
}
template <typename T> GruStepArgs<T> to_gru(const realise_gru_step* g, const int32_t* n_alive_dev = nullptr) {
  GruStepArgs<T> a;
  a.n_alive_dev = (const int*)n_alive_dev;
  a.n_alive = g->n_alive; a.H = g->H; a.Tp = g->Tp; a.t = g->t; a.table = g->table; a.pho_idx = g->pho_idx; a.perm = g->perm; a.lens = g->lens;
  a.gh = (const T*)g->gh; a.b_hh = g->b_hh; a.h_prev = (const T*)g->h_prev; a.h_new = (T*)g->h_new; a.rzn = (T*)g->rzn; a.out = (T*)g->out;
  a.dout = (const T*)g->dout; a.dh = (T*)g->dh; a.dgi = (T*)g->dgi; a.dgh = (T*)g->dgh; a.onehot = (T*)g->onehot;
  return a;
}
template <typename T> GateArgs<T> to_gate(const realise_gate* g, bool softmax = false) {
  GateArgs<T> a;
  a.B = g->B; a.S = g->S; a.H = g->H; a.bert = (const T*)g->bert; a.pho = (const T*)g->pho; a.res = (const T*)g->res; a.masks = g->masks;
  a.W = g->W; a.bias = g->bias; a.mean = g->mean; a.msum = g->msum; a.g = g->g; a.fused = (T*)g->fused; a.dfused = (const T*)g->dfused;
  a.dbert = (T*)g->dbert; a.dpho = (T*)g->dpho; a.dres = (T*)g->dres; a.dz = g->dz; a.dW = g->dW; a.dbias = g->dbias;
  a.row_live = g->row_live; a.nsrc = g->nsrc == 0 ? 3 : g->nsrc;
  if (softmax) a.softmax = true;
  return a;
}
RowBound bn_rows(const int* rows_dev, const float* counts, int hw, float* slots) {
  RowBound rb; rb.rows_dev = rows_dev; rb.counts = counts; rb.hw = hw; rb.slots = slots;
  return rb;
}
template <typename T>
BnBranch<T> to_bn_branch(const void* x, const float* mean, const float* rstd, const float* gamma, void* dx, float* dgamma, float* dbeta) {
  BnBranch<T> b;
  b.x = (const T*)x; b.mean = mean; b.rstd = rstd; b.gamma = gamma; b.dx = (T*)dx; b.dgamma = dgamma; b.dbeta = dbeta;
  return b;
}
// realise_batchnorm_fwd: bn_stats without a RowBound (no record scratch: the atomics form) + bn_apply; scratch = [sums | sq | scale | shift]
template <typename T>
int bn_fwd_t(hipStream_t st, const T* x, int P, int C, const float* gamma, const float* beta, float eps, float momentum, float* rmean, float* rvar,
             int64_t* nbt, int training, int relu, T* y, float* save_mean, float* save_rstd, float* scratch) {
  float* scale = scratch + 2 * C; float* shift = scratch + 3 * C;
  RL_TRY(bn_stats<T>(st, x, P, C, P, training, gamma, beta, eps, momentum, rmean, rvar, nbt, save_mean, save_rstd, scale, shift, scratch));
  return bn_apply<T>(st, x, scale, shift, (const T*)nullptr, nullptr, nullptr, y, P, C, relu);
}
// the epilogue realise_debug_nt_path / realise_debug_conv_nt_path ask about
template <typename T> EpiParams<T> path_epi(int x3, int mode, int accumulate, int has_aux, int has_scale, int64_t ldo, int64_t ldaux) {
  static const uint64_t some_operand[2] = {0, 0};      // (only compared with nullptr)
  realise_epilogue e;
  memset(&e, 0, sizeof(e));
  e.mode = mode; e.accumulate = accumulate; e.out = (void*)some_operand; e.ldo = ldo; e.aux = has_aux ? (const void*)some_operand : nullptr;
  e.ldaux = ldaux; e.alpha = 1.0f; e.drop_scale = 1.0f;
  if (has_scale) e.bias = (const float*)some_operand;
  return to_epi<T>(&e, x3, has_scale ? (const float*)some_operand : nullptr);
}
}  // namespace
extern "C" {

const char* realise_version(void) { return "realise_hip 0.3 (gfx950)"; }

int realise_gemm_nt(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                    const realise_epilogue* ep) {
  if (!ep || !ep->out) return RL_ERR_ARG;
  RL_BY_DTYPE(1, gemm_nt<E>((hipStream_t)stream, (const E*)A, lda, (const E*)B, ldb, M, N, K, to_epi<E>(ep, x3)));
}
int realise_gemm_nt_cat(void* stream, int dtype, const realise_gemm_cat* g) {
  if (!g || !g->out || !g->w || g->nsrc < 2 || g->nsrc > SEG_MAX) return RL_ERR_ARG;
  RL_BY_DTYPE(1, cat_launch<E>((hipStream_t)stream, g, x3));
}
int realise_conv_nt(void* stream, int dtype, const realise_conv_geom* a, const void* B, int64_t ldb, int M, int N, int K,
                    const realise_epilogue* ep) {
  if (!ep || !ep->out || !a) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gemm_nt_conv<E>((hipStream_t)stream, to_geom<E>(a), (const E*)B, ldb, M, N, K, to_epi<E>(ep)));
}
int realise_conv_dgrad_s2(void* stream, int dtype, const realise_conv_geom* a, const void* B_classes, int64_t ldb, int Cin,
                          const realise_epilogue* ep) {
  return realise_conv_dgrad_s2_ex(stream, dtype, a, B_classes, ldb, Cin, ep, nullptr);
}
int realise_gemm_tn(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int P, int I, int J,
                    float* out, int64_t ldo, float* scratch, int64_t scratch_elems, float* colsum_out) {
  TnEpi te; te.out = out; te.ldo = ldo; te.slab = scratch; te.slab_elems = scratch_elems; te.colsum = colsum_out;
  RL_BY_DTYPE(1, gemm_tn<E>((hipStream_t)stream, (const E*)A, lda, (const E*)B, ldb, P, I, J, with_x3(te, x3)));
}
int realise_gemm_tn_grouped(void* stream, int dtype, int n, const realise_tn_problem* problems, int P) {
  RL_BY_DTYPE(1, tn_grouped<E>((hipStream_t)stream, n, problems, P, x3));
}
int realise_gemm_nt_rows(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                         const realise_epilogue* ep, const int* rows_dev) {
  if (!ep || !ep->out || !rows_dev) return RL_ERR_ARG;
  RL_BY_DTYPE(1, gemm_nt<E>((hipStream_t)stream, (const E*)A, lda, (const E*)B, ldb, M, N, K, to_epi<E>(ep, x3), rows_dev));
}
int realise_gemm_nt_live(void* stream, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                         const realise_epilogue* ep, const int* live_list, const int* live_count) {
  if (!ep || !ep->out || !live_list || !live_count) return RL_ERR_ARG;
  EpiParams<bf16_t> e = to_epi<bf16_t>(ep);
  e.live_list = live_list; e.live_count = live_count;
  return gemm_nt8_live((hipStream_t)stream, (const bf16_t*)A, lda, (const bf16_t*)B, ldb, M, N, K, e);
}
int realise_gemm_nt_live_rows(void* stream, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                              const realise_epilogue* ep, const int* row_list, const int* row_count) {
  if (!ep || !ep->out || !row_list || !row_count) return RL_ERR_ARG;
  EpiParams<bf16_t> e = to_epi<bf16_t>(ep);
  e.live_list = row_list; e.live_count = row_count; e.live_unit = 1;
  return gemm_nt8_live((hipStream_t)stream, (const bf16_t*)A, lda, (const bf16_t*)B, ldb, M, N, K, e);
}
int realise_gemm_nt_splitk(void* stream, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K, int nsplit,
                           float* slab, int64_t slab_stride, const int* m_dev) {
  return gemm_nt8_splitk((hipStream_t)stream, (const bf16_t*)A, lda, (const bf16_t*)B, ldb, M, N, K, nsplit, slab, slab_stride, m_dev);
}
int realise_gemm_tn_grouped_live(void* stream, int dtype, int n, const realise_tn_problem* problems, int P, const int* live,
                                 const int* n_live, int list_rows, int overwrite) {
  if (live == nullptr || n_live == nullptr) return RL_ERR_ARG;
  RL_BY_DTYPE(1, tn_grouped<E>((hipStream_t)stream, n, problems, P, x3, live, n_live, list_rows, overwrite));
}
int realise_conv_tn(void* stream, int dtype, const void* A, int64_t lda, const realise_conv_geom* b, int P, int Co, int Ci,
                    float* out, float* scratch, int64_t scratch_elems) {
  return realise_conv_tn_ex(stream, dtype, A, lda, b, P, Co, Ci, out, scratch, scratch_elems, 1.0f, nullptr, nullptr, 0);
}
void realise_set_tn_transpose_read(int enable) { set_tn_transpose_read(enable); }
void realise_set_nt_allow_n96(int on) { set_nt_allow_n96(on); }
void realise_set_nt_variant(int v) { set_nt_variant(v); }
void realise_set_nt_group_m(int g) { set_nt8_group_m(g); }
void realise_set_ln(int key, int value) {
  if (key == 0) set_ln_fast(value); else if (key == 1) set_ln_bwd_blocks(value); else if (key == 2) set_bn_fast(value); else if (key == 3) set_bn_chunks(value); else if (key == 4) set_ce_fast(value); else if (key == 5) set_ln_v2(value); else if (key == 6) set_adamw_reg(value);
}
void realise_set_engine(int key, int value) { if (key == 0) set_fwd_order(value); else if (key >= 1 && key <= 3) set_stream_priority(key - 1, value); else if (key == 4) set_cls_compact(value); else if (key == 5) set_skip_dead(value); else if (key == 6) set_cls_splitk(value); else if (key == 9) set_gru_fuse(value); else if (key == 10) set_live_rows(value); else if (key == 13) set_glyph_fuse(value); else if (key == 14) set_bn_fold(value); else if (key == 15) set_opt_pipe(value); }
void realise_set_nt8p(int key, int value) { if (key == 0) set_nt8p_order(value); else if (key == 1) set_nt8p_wgs(value); else if (key == 3) set_nt8_live_gc(value); }
void realise_set_tn_split(int n) { set_tn_split(n); }
void realise_set_wgrad_group(int on) { set_wgrad_group(on); }
void realise_set_dgrad_parity(int on) { set_dgrad_parity(on); }
void realise_set_conv_c64(int on) { set_conv_c64(on); }
void realise_set_glyph_dedup(int on) { set_glyph_dedup(on); }
void realise_set_wgrad_overlap(int on) { set_wgrad_overlap(on); }
void realise_set_branch_overlap(int on) { set_branch_overlap(on); }

int realise_attention_fwd(void* stream, int dtype, const void* q, const void* k, const void* v, int64_t ldq, const float* mask_add,
                          void* ctx, int64_t ldc, float* lse, int B, int nh, int S, uint32_t drop_seed, uint32_t drop_thresh,
                          float drop_scale) {
  RL_BY_DTYPE(0, attn_fwd<E>((hipStream_t)stream, (const E*)q, (const E*)k, (const E*)v, ldq, mask_add, (E*)ctx, ldc, lse, B, nh, S, drop_seed,
                             drop_thresh, drop_scale));
}
int realise_attention_bwd(void* stream, int dtype, const void* q, const void* k, const void* v, int64_t ldq, const float* mask_add,
                          const void* ctx, const void* dctx, int64_t ldc, const float* lse, float* rowdot, void* dq, void* dk,
                          void* dv, int64_t ldd, int B, int nh, int S, uint32_t drop_seed, uint32_t drop_thresh, float drop_scale) {
  RL_BY_DTYPE(0, attn_bwd<E>((hipStream_t)stream, (const E*)q, (const E*)k, (const E*)v, ldq, mask_add, (const E*)ctx, (const E*)dctx, ldc, lse, rowdot,
                             (E*)dq, (E*)dk, (E*)dv, ldd, B, nh, S, drop_seed, drop_thresh, drop_scale));
}
// the attention launchers and row_liveness as a live-row training step calls them (include/realise_hip_debug.h): no arithmetic of their own
int realise_attention_fwd_rows(void* stream, int dtype, const void* q, const void* k, const void* v, int64_t ldq, const float* mask_add,
                               void* ctx, int64_t ldc, float* lse, int B, int nh, int S, uint32_t drop_seed, uint32_t drop_thresh,
                               float drop_scale, const int32_t* rlen) {
  RL_BY_DTYPE(0, attn_fwd<E>((hipStream_t)stream, (const E*)q, (const E*)k, (const E*)v, ldq, mask_add, (E*)ctx, ldc, lse, B, nh, S, drop_seed,
                             drop_thresh, drop_scale, (const int*)rlen));
}
int realise_attention_bwd_rows(void* stream, int dtype, const void* q, const void* k, const void* v, int64_t ldq, const float* mask_add,
                               const void* ctx, const void* dctx, int64_t ldc, const float* lse, float* rowdot, void* dq, void* dk,
                               void* dv, int64_t ldd, int B, int nh, int S, uint32_t drop_seed, uint32_t drop_thresh, float drop_scale,
                               const int32_t* rlen) {
  RL_BY_DTYPE(0, attn_bwd<E>((hipStream_t)stream, (const E*)q, (const E*)k, (const E*)v, ldq, mask_add, (const E*)ctx, (const E*)dctx, ldc, lse, rowdot,
                             (E*)dq, (E*)dk, (E*)dv, ldd, B, nh, S, drop_seed, drop_thresh, drop_scale, (const int*)rlen));
}
int realise_row_liveness(void* stream, const int64_t* masks, const int64_t* loss_masks, int B, int S, uint8_t* row_live, int32_t* tiles64,
                         int32_t* tiles32, int32_t* tiles16, int32_t* n_tiles, int32_t* rlen, int32_t* rows) {
  return row_liveness((hipStream_t)stream, masks, loss_masks, B, S, row_live, (int*)tiles64, (int*)tiles32, (int*)tiles16, (int*)n_tiles, (int*)rlen,
                      (int*)rows);
}
int realise_mask_to_additive(void* stream, const int64_t* masks, float* out, int n) {
  return mask_to_additive((hipStream_t)stream, masks, out, n);
}

int realise_layernorm_fwd_live(void* stream, const void* x, const float* gamma, const float* beta, float eps, void* y, void* xhat, float* rstd,
                               const uint8_t* row_live, int rows, int H) {
  if (row_live == nullptr || (rows % 16) != 0) return RL_ERR_ARG;
  return ln_fwd<bf16_t>((hipStream_t)stream, to_ln_fwd<bf16_t>(x, gamma, beta, eps, y, xhat, rstd, rows, H, row_live));
}
int realise_layernorm_fwd(void* stream, int dtype, const void* x, const float* gamma, const float* beta, float eps, void* y,
                          void* xhat, float* rstd, int rows, int H) {
  RL_BY_DTYPE(0, ln_fwd<E>((hipStream_t)stream, to_ln_fwd<E>(x, gamma, beta, eps, y, xhat, rstd, rows, H)));
}
int realise_token_rows(void* stream, int dtype, const realise_token_rows_args* a) {
  if (!a || !a->ids || a->T <= 0 || a->S <= 0 || a->H < 8 || (a->H & 7) || a->H > 1024 || a->ld < a->H || (a->ld & 7)) return RL_ERR_ARG;
  if (!a->pho_table && !a->res_table) return RL_ERR_ARG;
  if (a->pho_table && (!a->pho_out || a->ld_pho_out < a->H || (a->ld_pho_out & 7) || !a->pos || !a->type0 || !a->gamma || !a->beta)) return RL_ERR_ARG;
  if (a->res_table && (!a->res_out || a->ld_res_out < a->H || (a->ld_res_out & 7))) return RL_ERR_ARG;
  RL_BY_DTYPE(0, token_rows_launch<E>((hipStream_t)stream, a));
}
int realise_layernorm_bwd(void* stream, int dtype, const void* dy, const void* xhat, const float* rstd, const float* gamma,
                          void* dx, float* dgamma, float* dbeta, int rows, int H) {
  RL_BY_DTYPE(0, ln_bwd<E>((hipStream_t)stream, to_ln_bwd<E>(dy, xhat, rstd, gamma, dx, dgamma, dbeta, rows, H)));
}
int realise_layernorm_gelu_bwd(void* stream, int dtype, const void* dy, const void* xhat, const float* rstd, const void* z, const float* gamma,
                               void* dz, float* dgamma, float* dbeta, int rows, int H, const int32_t* n_rows_dev, const int32_t* row_index,
                               int saved_rows) {
  if (rows < 0 || saved_rows < 0) return RL_ERR_ARG;
  RL_BY_DTYPE(0, ln_gelu_bwd<E>((hipStream_t)stream, to_ln_gelu_bwd<E>(dy, xhat, rstd, z, gamma, dz, dgamma, dbeta, rows, H, n_rows_dev, row_index,
                                                                        saved_rows)));
}
int realise_layernorm_bwd_ex(void* stream, const void* dy, const void* xhat, const float* rstd, const float* gamma, void* dx, void* dx_drop,
                             uint32_t drop_seed, uint32_t drop_thresh, float drop_scale, float* dgamma, float* dbeta, float* slots, int rows, int H) {
  return realise_layernorm_bwd_live(stream, dy, xhat, rstd, gamma, dx, dx_drop, drop_seed, drop_thresh, drop_scale, dgamma, dbeta, slots, nullptr, rows, H);
}
int realise_layernorm_bwd_live(void* stream, const void* dy, const void* xhat, const float* rstd, const float* gamma, void* dx, void* dx_drop,
                               uint32_t drop_seed, uint32_t drop_thresh, float drop_scale, float* dgamma, float* dbeta, float* slots,
                               const uint8_t* row_live, int rows, int H) {
  return ln_bwd<bf16_t>((hipStream_t)stream, to_ln_bwd<bf16_t>(dy, xhat, rstd, gamma, dx, dgamma, dbeta, rows, H, dx_drop,
                                                               DropParams{drop_seed, drop_thresh, drop_scale}, slots, row_live));
}
int realise_build_pho(void* stream, const int64_t* src_idx, int T, const int64_t* table, const int32_t* vlens, int V, int Tw,
                      int64_t* pho_idx, int32_t* perm, int32_t* lens_sorted, int32_t* n_alive_dev) {
  if (!src_idx || !table || !vlens || !pho_idx || !perm || !lens_sorted || !n_alive_dev) return RL_ERR_ARG;
  return pho_prepare((hipStream_t)stream, src_idx, T, table, vlens, V, Tw, pho_idx, perm, lens_sorted, n_alive_dev);
}
int realise_argmax(void* stream, int dtype, const void* logits, int64_t ld, int rows, int V, int64_t* ids) {
  RL_BY_DTYPE(0, argmax_rows<E>((hipStream_t)stream, (const E*)logits, ld, rows, V, ids));
}
// models.py:859-869 + np.argmax(preds, -1) (src/run.py:262-263, src/test.py:143) without the logits: see include/realise_hip.h
int64_t realise_gemm_nt_decode_scratch_bytes(int dtype, int M, int N, int K, int k) {
  RL_BY_DTYPE_OR(0, 1, nt_decode_scratch_bytes(gemm_nt_decode_path<E>(M, N, K, K, K, k, x3), M, N, k));
}
int realise_gemm_nt_decode(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                           const float* bias, const int64_t* labels, const realise_decode* d) {
  if (!d) return RL_ERR_ARG;
  DecodeOut o; o.k = d->k; o.ids = d->ids; o.values = d->values; o.probs = d->probs; o.lse = d->lse; o.label_logit = d->label_logit;
  o.scratch = d->scratch; o.scratch_bytes = d->scratch_bytes;
  RL_BY_DTYPE(1, gemm_nt_decode<E>((hipStream_t)stream, (const E*)A, lda, (const E*)B, ldb, M, N, K, bias, labels, o, x3));
}
int realise_masked_ce(void* stream, int dtype, const void* logits, int64_t ld, const int64_t* labels, const int64_t* loss_mask,
                      int rows, int V, float* loss_out, float* count_scratch, void* dlogits) {
  RL_BY_DTYPE(0, ce_loss<E>((hipStream_t)stream, (const E*)logits, ld, labels, loss_mask, rows, V, loss_out, count_scratch, (E*)dlogits));
}
int realise_masked_ce_pred(void* stream, int dtype, const void* logits, int64_t ld, const int64_t* labels, const int64_t* loss_mask,
                           int rows, int V, float* loss_out, float* count_scratch, void* dlogits, int64_t* pred_out, int32_t* hits) {
  if (pred_out == nullptr || hits == nullptr) return RL_ERR_ARG;
  CePred pr; pr.pred = pred_out; pr.hits = hits; pr.capacity = rows;
  RL_BY_DTYPE(0, ce_loss<E>((hipStream_t)stream, (const E*)logits, ld, labels, loss_mask, rows, V, loss_out, count_scratch, (E*)dlogits, nullptr, 0,
                            CeCompact(), &pr));
}

// ---- remaining fine-grained operators of the path (per-op parity tests call these) ------------------------------------------------
int realise_gru_step_fwd(void* stream, int dtype, const realise_gru_step* a) {
  if (!a) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gru_step_fwd<E>((hipStream_t)stream, to_gru<E>(a)));
}
int realise_gru_step_bwd(void* stream, int dtype, const realise_gru_step* a) {
  if (!a) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gru_step_bwd<E>((hipStream_t)stream, to_gru<E>(a)));
}
// the pinyin GRU as engine.hip gru_forward / gru_backward launch it (include/realise_hip_debug.h)
int realise_gru_table_fwd(void* stream, const float* emb, const float* w_ih, const float* b_ih, int V, int H, float* table) {
  if (!emb || !w_ih || !b_ih || !table) return RL_ERR_ARG;
  return gru_table_fwd((hipStream_t)stream, emb, w_ih, b_ih, V, H, table);
}
int realise_gru_table_bwd(void* stream, const float* dtable, int ld, const float* emb, const float* w_ih, int V, int H, float* d_emb,
                          float* d_w_ih, float* d_b_ih) {
  if (!dtable || !emb || !w_ih || !d_emb || !d_w_ih || !d_b_ih || V < 1 || H < 1 || ld < 3 * H) return RL_ERR_ARG;
  return gru_table_bwd((hipStream_t)stream, dtable, ld, emb, w_ih, V, H, d_emb, d_w_ih, d_b_ih);
}
int realise_gru_step_fwd_rows(void* stream, int dtype, const realise_gru_step* a, const int32_t* n_alive_dev) {
  if (!a || !n_alive_dev) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gru_step_fwd<E>((hipStream_t)stream, to_gru<E>(a, n_alive_dev)));
}
int realise_gru_step_bwd_rows(void* stream, int dtype, const realise_gru_step* a, const int32_t* n_alive_dev) {
  if (!a || !n_alive_dev) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gru_step_bwd<E>((hipStream_t)stream, to_gru<E>(a, n_alive_dev)));
}
int realise_gru_step_fused(void* stream, const realise_gru_step* a, const void* w_hh_bf16, int64_t ldb, const int32_t* n_alive_dev) {
  if (!a || !w_hh_bf16) return RL_ERR_ARG;
  typedef bf16_t T;
  const int H = a->H;
  EpiParams<T> ep; ep.mode = EPI_STORE; ep.out = (T*)a->h_new; ep.ldo = H; ep.bias = a->b_hh; ep.m_dev = (const int*)n_alive_dev;
  ep.gru_table = a->table; ep.gru_pho_idx = a->pho_idx; ep.gru_perm = a->perm; ep.gru_lens = a->lens;
  ep.gru_hprev = (const T*)a->h_prev; ep.gru_rzn = (T*)a->rzn; ep.gru_gh = (T*)a->gh; ep.gru_out = (T*)a->out;
  ep.gru_Tp = a->Tp; ep.gru_t = a->t;
  return gemm_nt8_gru((hipStream_t)stream, (const T*)a->h_prev, H, (const T*)w_hh_bf16, ldb, a->n_alive, 3 * H, H, ep);
}
int realise_gate_fwd(void* stream, int dtype, const realise_gate* a) {
  if (!a) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gate_fwd<E>((hipStream_t)stream, to_gate<E>(a)));
}
int realise_gate_bwd(void* stream, int dtype, const realise_gate* a) {
  if (!a) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gate_bwd<E>((hipStream_t)stream, to_gate<E>(a)));
}
// src/models.py:1139-1150 (SpellBertPho2ResArch4): softmax over the gate_net outputs; the struct is realise_gate as it is
int realise_gate_softmax_fwd(void* stream, int dtype, const realise_gate* a) {
  if (!a) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gate_fwd<E>((hipStream_t)stream, to_gate<E>(a, true)));
}
int realise_gate_softmax_bwd(void* stream, int dtype, const realise_gate* a) {
  if (!a) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gate_bwd<E>((hipStream_t)stream, to_gate<E>(a, true)));
}
int realise_sum_fuse_fwd(void* stream, int dtype, const void* bert, const void* pho, const void* res, void* fused, int rows, int H) {
  RL_BY_DTYPE(0, sum_fuse_fwd<E>((hipStream_t)stream, (const E*)bert, (const E*)pho, (const E*)res, (E*)fused, rows, H));
}
int realise_sum_fuse_bwd(void* stream, int dtype, const void* dfused, void* dbert, void* dpho, void* dres, int rows, int H,
                         const uint8_t* row_live) {
  RL_BY_DTYPE(0, sum_fuse_bwd<E>((hipStream_t)stream, (const E*)dfused, (E*)dbert, (E*)dpho, (E*)dres, rows, H, row_live));
}
int realise_batchnorm_fwd(void* stream, int dtype, const void* x, int P, int C, const float* gamma, const float* beta, float eps, float momentum,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked, int training, int relu, void* y,
                          float* save_mean, float* save_rstd, float* scratch) {
  if (!x || !y || !scratch || P < 1 || C < 4 || (C & 3)) return RL_ERR_ARG;
  RL_BY_DTYPE(0, bn_fwd_t<E>((hipStream_t)stream, (const E*)x, P, C, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, training,
                             relu, (E*)y, save_mean, save_rstd, scratch));
}
int realise_batchnorm_bwd(void* stream, int dtype, const void* dy, const void* relu_src, const void* x, const float* save_mean, const float* save_rstd,
                          const float* gamma, int P, int C, void* dx, float* dgamma, float* dbeta, float* scratch) {
  if (!dy || !x || !dx || !scratch || P < 1 || C < 4 || (C & 3)) return RL_ERR_ARG;
  RL_BY_DTYPE(0, bn_backward<E>((hipStream_t)stream, (const E*)dy, (const E*)relu_src, P, C, P,
                                to_bn_branch<E>(x, save_mean, save_rstd, gamma, dx, dgamma, dbeta), BnBranch<E>(), scratch));
}
// bn_stats / bn_backward, the functions the engine's glyph branch calls, in bf16 with the record scratch (include/realise_hip_debug.h)
int realise_batchnorm_stats_ex(void* stream, const void* x, int P, int C, int hw, const float* counts, int n_stat, const float* gamma, const float* beta,
                               float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd,
                               float* scale, float* shift, float* sq_scratch, float* slots) {
  if (!x || !mean || !rstd || !scale || !shift || !sq_scratch || !slots || !running_mean || !running_var || P < 1 || C < 4 || (C & 3) || hw < 1) return RL_ERR_ARG;
  // (with slots bn_stats touches only scratch[C, 2C): sq_scratch)
  return bn_stats<bf16_t>((hipStream_t)stream, (const bf16_t*)x, P, C, n_stat, 1, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked,
                          mean, rstd, scale, shift, sq_scratch - C, bn_rows(nullptr, counts, hw, slots));
}
int realise_batchnorm_bwd_ex(void* stream, const void* dy, const void* relu_src, int P, int C, int hw, const float* counts, int n_stat,
                             const void* xa, const float* mean_a, const float* rstd_a, const float* gamma_a, void* dxa, float* dgamma_a, float* dbeta_a,
                             const void* xb, const float* mean_b, const float* rstd_b, const float* gamma_b, void* dxb, float* dgamma_b, float* dbeta_b,
                             float* sums, float* slots) {
  if (!dy || !xa || !dxa || !sums || !slots || P < 1 || C < 4 || (C & 3) || hw < 1) return RL_ERR_ARG;
  return bn_backward<bf16_t>((hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)relu_src, P, C, n_stat,
                             to_bn_branch<bf16_t>(xa, mean_a, rstd_a, gamma_a, dxa, dgamma_a, dbeta_a),
                             to_bn_branch<bf16_t>(xb, mean_b, rstd_b, gamma_b, dxb, dgamma_b, dbeta_b), sums, bn_rows(nullptr, counts, hw, slots));
}
int realise_embedding_bwd(void* stream, int dtype, const void* de, const int64_t* ids, int B, int S, int H, float* word_grad, float* pos_grad,
                          int pos_zero, float* type_grad) {
  RL_BY_DTYPE(0, embed_bwd<E>((hipStream_t)stream, (const E*)de, ids, B, S, H, word_grad, pos_grad, pos_zero, type_grad));
}
int realise_glyph_unique(void* stream, const int64_t* ids, int T, int V, int32_t* first_scratch, int32_t* flag_scratch, int64_t* uniq_ids, float* counts,
                         int32_t* inv, int32_t* bounds, int nhw, const int32_t* hw) {
  if (!ids || T < 1 || V < 1 || nhw < 0 || nhw > 8 || (nhw > 0 && !hw)) return RL_ERR_ARG;
  HwList h; h.n = nhw;
  for (int k = 0; k < nhw; ++k) h.v[k] = hw[k];
  return glyph_unique((hipStream_t)stream, ids, T, V, (int*)first_scratch, (int*)flag_scratch, uniq_ids, counts, (int*)inv, (int*)bounds, h);
}
int realise_segment_sum(void* stream, int dtype, const void* x, const int32_t* inv, int T, int C, float* acc, void* out, const int32_t* nuniq_dev) {
  RL_BY_DTYPE(0, segment_sum<E>((hipStream_t)stream, (const E*)x, (const int*)inv, T, C, acc, (E*)out, (const int*)nuniq_dev));
}
int realise_layernorm_fwd_chw4(void* stream, int dtype, const void* x, const int32_t* row_index, const float* gamma, const float* beta, float eps,
                               void* y, void* xhat, float* rstd, int rows, int H) {
  if (!x || !gamma || !beta || !y) return RL_ERR_ARG;
  RL_BY_DTYPE(0, ln_fwd_chw4<E>((hipStream_t)stream, to_ln_fwd<E>(x, gamma, beta, eps, y, xhat, rstd, rows, H, nullptr, row_index)));
}
int realise_gather_rows_chw4(void* stream, int dtype, const void* x, const int32_t* inv, int T, int H, void* out) {
  if (!x || !inv || !out) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gather_rows_chw4<E>((hipStream_t)stream, (const E*)x, (const int*)inv, T, H, (E*)out));
}
int realise_segment_sum_chw4(void* stream, int dtype, const void* x, const int32_t* inv, int T, int H, float* acc, void* out, const int32_t* nuniq_dev) {
  if (!x || !inv || !acc || !out || !nuniq_dev) return RL_ERR_ARG;
  RL_BY_DTYPE(0, segment_sum_chw4<E>((hipStream_t)stream, (const E*)x, (const int*)inv, T, H, acc, (E*)out, (const int*)nuniq_dev));
}

// ---- layout --------------------------------------------------------------------------------------
int realise_layout_count(const realise_config* cfg) { return cfg && config_ok(*cfg) ? (int)build_layout(*cfg).tensors.size() : -1; }
int realise_layout_entry(const realise_config* cfg, int index, char* name, int name_cap, int32_t* arena, int64_t* offset,
                         int32_t* ndim, int64_t* shape4) {
  if (!cfg || !config_ok(*cfg)) return RL_ERR_ARG;
  const Layout L = build_layout(*cfg);
  if (index < 0 || index >= (int)L.tensors.size()) return RL_ERR_ARG;
  const TensorInfo& t = L.tensors[index];
  if ((int)t.name.size() + 1 > name_cap) return RL_ERR_ARG;
  strcpy(name, t.name.c_str());
  *arena = t.arena; *offset = t.offset; *ndim = t.ndim;
  for (int i = 0; i < 4; ++i) shape4[i] = t.shape[i];
  return RL_OK;
}
int64_t realise_arena_elems(const realise_config* cfg, int arena) {
  if (!cfg || !config_ok(*cfg) || arena < 0 || arena >= AR_COUNT) return -1;
  return build_layout(*cfg).arena_elems[arena];
}
int realise_bucket_count(const realise_config* cfg) { return cfg && config_ok(*cfg) ? (int)build_layout(*cfg).buckets.size() : -1; }
int realise_bucket_bounds(const realise_config* cfg, int bucket, int64_t* begin, int64_t* end) {
  if (!cfg || !config_ok(*cfg)) return RL_ERR_ARG;
  const Layout L = build_layout(*cfg);
  if (bucket < 0 || bucket >= (int)L.buckets.size()) return RL_ERR_ARG;
  *begin = L.buckets[bucket].first; *end = L.buckets[bucket].second;
  return RL_OK;
}

// ---- engine ----------------------------------------------------------------------------------------
realise_engine* realise_engine_create(const realise_config* cfg, float* params, float* grads, float* unused_params, float* frozen,
                                      float* buffers_f32, int64_t* buffers_i64) {
  if (!cfg) return nullptr;
  EngineBase* impl = make_engine(*cfg, params, grads, unused_params, frozen, buffers_f32, buffers_i64);
  if (!impl) return nullptr;
  realise_engine* e = new realise_engine;
  e->impl = impl;
  return e;
}
void realise_engine_destroy(realise_engine* e) { if (e) { delete e->impl; delete e; } }
int64_t realise_engine_shadow_bytes(const realise_engine* e) { return e ? e->impl->shadow_bytes() : -1; }
int64_t realise_engine_workspace_bytes(const realise_engine* e, int B, int S, int Tp) { return e ? e->impl->workspace_bytes(B, S, Tp) : -1; }
int realise_engine_bind(realise_engine* e, void* shadow, void* workspace, int64_t workspace_bytes) {
  return e ? e->impl->bind(shadow, workspace, workspace_bytes) : RL_ERR_ARG;
}
int realise_debug_tn_list_lds(int64_t entries) { return tn_list_lds_bytes(entries); }
int realise_debug_tn_plan(int dtype, int kind, int P, int I, int J, int Cin, int scratch_given, int64_t scratch_elems, realise_tn_plan* plan) {
  if (!plan || (dtype != REALISE_BF16 && dtype != REALISE_F32 && dtype != REALISE_F32_BF16X3) || kind < 0 || kind > 2) return RL_ERR_ARG;
  TnPlan pl;
  const int rc = tn_plan(dtype == REALISE_BF16 ? 2 : 4, kind == 2, P, I, J, Cin > 0, Cin, scratch_given != 0, scratch_elems, pl);
  plan->tile = pl.tile; plan->nsplit = pl.nsplit; plan->pchunk = pl.pchunk; plan->form = pl.how; plan->fold = pl.fold; plan->fold_sb = pl.fold_sb;
  return rc;
}
int realise_gemm_tn_ex(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int P, int I, int J,
                       float* out, int64_t ldo, float* scratch, int64_t scratch_elems, float* colsum_out, float alpha,
                       const float* alpha_dev, const int* rows_dev, int overwrite, int conv_Cin, int conv_Cpad, int conv_KHW, int tap0) {
  TnEpi te; te.out = out; te.ldo = ldo; te.slab = scratch; te.slab_elems = scratch_elems; te.colsum = colsum_out;
  te.alpha = alpha; te.alpha_dev = alpha_dev; te.overwrite = overwrite;
  if (conv_KHW > 0) { te.mode = TN_CONVW; te.Cin = conv_Cin; te.Cpad = conv_Cpad; te.KHW = conv_KHW; te.tap0 = tap0; }
  RL_BY_DTYPE(1, gemm_tn<E>((hipStream_t)stream, (const E*)A, lda, (const E*)B, ldb, P, I, J, with_x3(te, x3), rows_dev));
}
int realise_conv_tn_ex(void* stream, int dtype, const void* A, int64_t lda, const realise_conv_geom* b, int P, int Co, int Ci,
                       float* out, float* scratch, int64_t scratch_elems, float alpha, const float* alpha_dev, const int* rows_dev,
                       int64_t index_rows) {
  if (!b) return RL_ERR_ARG;
  TnEpi te; te.mode = TN_CONVW; te.out = out; te.Cin = Ci; te.Cpad = b->C; te.KHW = b->KH * b->KW;
  te.slab = scratch; te.slab_elems = scratch_elems; te.alpha = alpha; te.alpha_dev = alpha_dev;
  const int J = b->KH * b->KW * b->C;
  RL_BY_DTYPE(0, gemm_tn_conv<E>((hipStream_t)stream, (const E*)A, lda, to_geom<E>(b, rows_dev, index_rows), P, Co, J, te));
}
int realise_debug_nt_path(int dtype, int M, int N, int K, int mode, int accumulate, int has_aux, int64_t lda, int64_t ldb, int64_t ldo,
                          int64_t ldaux, int rows_dev_given) {
  if (mode == 16) RL_BY_DTYPE_OR(NT_PATH_REFUSED, 1, gemm_nt_decode_path<E>(M, N, K, lda, ldb, accumulate > 0 ? accumulate : 1, x3));
  RL_BY_DTYPE_OR(NT_PATH_REFUSED, 1, gemm_nt_path<E>(M, N, K, path_epi<E>(x3, mode, accumulate, has_aux, 0, ldo, ldaux), lda, ldb, rows_dev_given != 0));
}
int realise_debug_bn_plan(int dtype, int P, int C, int hw, int slots_given, int branches, realise_bn_plan* plan) {
  if (!plan || (dtype != REALISE_BF16 && dtype != REALISE_F32)) return RL_ERR_ARG;
  BnPlan pl;
  const int rc = bn_plan(dtype == REALISE_BF16 ? 2 : 4, P, C, hw, slots_given != 0, branches, pl);
  const BnPass* src[4] = {&pl.stats, &pl.apply, &pl.bwd_reduce, &pl.bwd_apply};
  realise_bn_pass* dst[4] = {&plan->stats, &plan->apply, &plan->bwd_reduce, &plan->bwd_apply};
  for (int k = 0; k < 4; ++k) {
    dst[k]->kernel = src[k]->kernel; dst[k]->g = src[k]->g; dst[k]->stride = src[k]->stride; dst[k]->fold_wgs = src[k]->fold_wgs;
    dst[k]->overwrite = src[k]->overwrite;
  }
  return rc;
}
int realise_debug_conv_nt_path(int dtype, const realise_conv_geom* a, int64_t ldb, int M, int N, int K, int mode, int accumulate, int has_aux,
                               int has_scale, int64_t ldo, int64_t ldaux) {
  if (!a) return NT_PATH_REFUSED;
  RL_BY_DTYPE_OR(NT_PATH_REFUSED, 0, conv_nt_path<E>(to_geom<E>(a), ldb, M, N, K, path_epi<E>(0, mode, accumulate, has_aux, has_scale, ldo, ldaux)));
}
// realise_conv_nt / realise_gemm_nt with what the engine's glyph branch passes: the extended epilogue and the device-side bound
int realise_conv_nt_ex(void* stream, int dtype, const realise_conv_geom* a, const void* B, int64_t ldb, int M, int N, int K,
                       const realise_epilogue* ep, const float* col_scale, int relu, const int* rows_dev, int64_t index_rows) {
  if (!ep || !ep->out || !a) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gemm_nt_conv<E>((hipStream_t)stream, to_geom<E>(a, rows_dev, index_rows), (const E*)B, ldb, M, N, K, to_epi<E>(ep, 0, col_scale, relu)));
}
int realise_conv_dgrad_s2_ex(void* stream, int dtype, const realise_conv_geom* a, const void* B_classes, int64_t ldb, int Cin,
                             const realise_epilogue* ep, const int* rows_dev) {
  if (!ep || !ep->out || !a) return RL_ERR_ARG;
  RL_BY_DTYPE(0, conv_dgrad_s2<E>((hipStream_t)stream, to_geom<E>(a, rows_dev), (const E*)B_classes, ldb, Cin, to_epi<E>(ep)));
}
int realise_gemm_nt_ex(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                       const realise_epilogue* ep, const float* col_scale, int relu, const int* rows_dev) {
  if (!ep || !ep->out) return RL_ERR_ARG;
  RL_BY_DTYPE(0, gemm_nt<E>((hipStream_t)stream, (const E*)A, lda, (const E*)B, ldb, M, N, K, to_epi<E>(ep, 0, col_scale, relu), rows_dev));
}
int realise_batchnorm_stats_rows(void* stream, int dtype, const void* x, int P, int C, int hw, const float* counts, const int* rows_dev, int n_stat,
                                 int training, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                                 float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd, float* scale, float* shift,
                                 float* scratch, float* slots) {
  if (!gamma || !beta || !scale || !shift || !running_mean || !running_var || P < 1 || C < 4 || (C & 3) || hw < 1) return RL_ERR_ARG;
  if (training && (!x || !mean || !rstd || !scratch)) return RL_ERR_ARG;
  RL_BY_DTYPE(0, bn_stats<E>((hipStream_t)stream, (const E*)x, P, C, n_stat, training, gamma, beta, eps, momentum, running_mean, running_var,
                             num_batches_tracked, mean, rstd, scale, shift, scratch, bn_rows(rows_dev, counts, hw, slots)));
}
int realise_batchnorm_apply_rows(void* stream, int dtype, const void* x1, const float* scale1, const float* shift1, const void* x2,
                                 const float* scale2, const float* shift2, void* y, int P, int C, int hw, int relu, const int* rows_dev) {
  if (!x1 || !scale1 || !shift1 || !y || (x2 && (!scale2 || !shift2)) || P < 1 || C < 4 || (C & 3) || hw < 1) return RL_ERR_ARG;
  RL_BY_DTYPE(0, bn_apply<E>((hipStream_t)stream, (const E*)x1, scale1, shift1, (const E*)x2, scale2, shift2, (E*)y, P, C, relu,
                             bn_rows(rows_dev, nullptr, hw, nullptr)));
}
int realise_batchnorm_bwd_rows(void* stream, int dtype, const void* dy, const void* relu_src, int P, int C, int hw, const float* counts,
                               const int* rows_dev, int n_stat,
                               const void* xa, const float* mean_a, const float* rstd_a, const float* gamma_a, void* dxa, float* dgamma_a, float* dbeta_a,
                               const void* xb, const float* mean_b, const float* rstd_b, const float* gamma_b, void* dxb, float* dgamma_b, float* dbeta_b,
                               float* sums, float* slots) {
  if (!dy || !xa || !dxa || !sums || P < 1 || C < 4 || (C & 3) || hw < 1 || (xb && !dxb)) return RL_ERR_ARG;
  RL_BY_DTYPE(0, bn_backward<E>((hipStream_t)stream, (const E*)dy, (const E*)relu_src, P, C, n_stat,
                                to_bn_branch<E>(xa, mean_a, rstd_a, gamma_a, dxa, dgamma_a, dbeta_a),
                                to_bn_branch<E>(xb, mean_b, rstd_b, gamma_b, dxb, dgamma_b, dbeta_b), sums, bn_rows(rows_dev, counts, hw, slots)));
}
int64_t realise_engine_plan_installs(const realise_engine* e) { return e ? e->impl->plan_install_count() : -1; }
int realise_debug_engine_cast_desc(const realise_engine* e, int i, realise_cast_desc_info* out) { return e ? e->impl->cast_desc_info(i, out) : -RL_ERR_ARG; }
void realise_engine_forget_workspace(realise_engine* e, void* workspace) { if (e) e->impl->forget_workspace(workspace); }
int realise_engine_refresh_shadows(realise_engine* e, void* stream) { return e ? e->impl->refresh_shadows((hipStream_t)stream) : RL_ERR_ARG; }
int realise_engine_refresh_shadows_ex(realise_engine* e, void* stream, int linear_current) {
  return e ? e->impl->refresh_shadows_ex((hipStream_t)stream, linear_current) : RL_ERR_ARG;
}
void realise_engine_invalidate_frozen(realise_engine* e) { if (e) e->impl->invalidate_frozen(); }
void realise_engine_set_grads_fresh(realise_engine* e, int fresh) { if (e) e->impl->set_grads_fresh(fresh); }
void realise_engine_set_id_flag(realise_engine* e, int32_t* flag) { if (e) e->impl->set_id_flag((int*)flag); }
void realise_engine_set_loss_grad(realise_engine* e, const float* grad_dev) { if (e) e->impl->set_loss_grad(grad_dev); }
void realise_engine_set_decode(realise_engine* e, const realise_decode* d) { if (e) e->impl->set_decode(d); }
void realise_engine_set_pred(realise_engine* e, const realise_pred* d) { if (e) e->impl->set_pred(d); }
int realise_engine_set_token_tables(realise_engine* e, const realise_token_tables* t) { return e ? e->impl->set_token_tables(t) : RL_ERR_ARG; }
int realise_engine_fill_token_tables(realise_engine* e, void* stream, const realise_batch* batch, const realise_token_tables* t) {
  return (e && batch && t) ? e->impl->fill_token_tables((hipStream_t)stream, *batch, *t) : RL_ERR_ARG;
}
int realise_engine_forward(realise_engine* e, void* stream, const realise_batch* batch) {
  return (e && batch) ? e->impl->forward((hipStream_t)stream, *batch) : RL_ERR_ARG;
}
int realise_engine_backward(realise_engine* e, void* stream, int first_bucket, int last_bucket) {
  return e ? e->impl->backward((hipStream_t)stream, first_bucket, last_bucket) : RL_ERR_ARG;
}
int realise_engine_backward_signalled(realise_engine* e, void* stream, void* const* bucket_events, int n_events) {
  return e ? e->impl->backward_signalled((hipStream_t)stream, bucket_events, n_events) : RL_ERR_ARG;
}
int realise_engine_glyph_forward(realise_engine* e, void* stream, const int64_t* src_idx, int B, int S, int training, void* res_out) {
  return e ? e->impl->glyph_forward((hipStream_t)stream, src_idx, B, S, training, res_out) : RL_ERR_ARG;
}
int realise_engine_glyph_backward(realise_engine* e, void* stream, const void* d_res) {
  return e ? e->impl->glyph_backward((hipStream_t)stream, d_res) : RL_ERR_ARG;
}
int realise_engine_tap(realise_engine* e, const char* name, void** ptr, int64_t* numel) {
  return (e && name && ptr && numel) ? e->impl->get_tap(name, ptr, numel) : RL_ERR_ARG;
}

// ---- optimizer ---------------------------------------------------------------------------------------
int realise_sumsq(void* stream, const float* g, int64_t n, float* out_accum) { return sumsq_accum((hipStream_t)stream, g, n, out_accum); }
int realise_adamw(void* stream, float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int64_t step, int correct_bias, const float* grad_norm_sq, float max_grad_norm) {
  float bc1 = 1.0f, bc2 = 1.0f;
  if (correct_bias) {
    bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  }
  return adamw_flat((hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, grad_norm_sq, max_grad_norm);
}
int realise_clip_scale(void* stream, float* g, int64_t n, const float* grad_norm_sq, float max_grad_norm) { return clip_scale((hipStream_t)stream, g, n, grad_norm_sq, max_grad_norm); }
static bool make_adamw_groups(const realise_adamw_group* groups, int n_groups, int64_t step, AdamwGroups& gs) {
  if (!groups || n_groups < 1 || n_groups > ADAMW_MAX_GROUPS) return false;
  gs.n = n_groups;
  for (int i = 0; i < n_groups; ++i) {
    const realise_adamw_group& h = groups[i];
    double bc1 = 1.0, bc2 = 1.0;
    if (h.correct_bias) { bc1 = 1.0 - pow((double)h.beta1, (double)step); bc2 = 1.0 - pow((double)h.beta2, (double)step); }
    gs.g[i] = AdamwGroup{h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, (float)(h.lr * sqrt(bc2) / bc1)};
  }
  return true;
}
int realise_adamw_grouped(void* stream, float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* group_of_block64,
                          const realise_adamw_group* groups, int n_groups, int64_t step, const float* grad_norm_sq, float max_grad_norm) {
  AdamwGroups gs;
  if (!make_adamw_groups(groups, n_groups, step, gs)) return RL_ERR_ARG;
  return adamw_grouped((hipStream_t)stream, p, g, m, v, n, group_of_block64, gs, grad_norm_sq, max_grad_norm);
}
int realise_engine_adamw(realise_engine* e, void* stream, float* m, float* v, const uint8_t* group_of_block64,
                         const realise_adamw_group* groups, int n_groups, int64_t step, const float* grad_norm_sq, float max_grad_norm) {
  AdamwGroups gs;
  if (!e || !make_adamw_groups(groups, n_groups, step, gs)) return RL_ERR_ARG;
  return e->impl->adamw_step((hipStream_t)stream, m, v, group_of_block64, gs, grad_norm_sq, max_grad_norm, 0);
}
int realise_engine_adamw_pipelined(realise_engine* e, void* stream, float* m, float* v, const uint8_t* group_of_block64,
                                   const realise_adamw_group* groups, int n_groups, int64_t step, const float* grad_norm_sq, float max_grad_norm) {
  AdamwGroups gs;
  if (!e || !make_adamw_groups(groups, n_groups, step, gs)) return RL_ERR_ARG;
  return e->impl->adamw_step((hipStream_t)stream, m, v, group_of_block64, gs, grad_norm_sq, max_grad_norm, 1);
}
int realise_engine_sync_optimizer(realise_engine* e, void* stream) { return e ? e->impl->sync_optimizer((hipStream_t)stream) : RL_ERR_ARG; }
int realise_profile_enable(int max_launches) { return prof_enable(max_launches); }
void realise_profile_pause(int paused) { prof_pause(paused); }
void realise_profile_mode(int attached) { prof_set_mode(attached); }
void realise_profile_disable(void) { prof_disable(); }
int realise_profile_dump(int kernel_family, int max_records, float* ms_out, double* work_out) { return prof_dump(kernel_family, max_records, ms_out, work_out); }
int realise_profile_dump_ex(int kernel_family, int max_records, float* ms_out, double* work_out, double* work_exec_out) {
  return prof_dump(kernel_family, max_records, ms_out, work_out, work_exec_out);
}
int realise_profile_read_ex(int kernel_family, long long* count, double* total_ms, double* total_work, double* total_work_executed) {
  if (kernel_family < 0 || kernel_family >= PK_COUNT || !count || !total_ms || !total_work || !total_work_executed) return RL_ERR_ARG;
  return prof_read(kernel_family, count, total_ms, total_work, total_work_executed);
}
int realise_profile_read(int kernel_family, long long* count, double* total_ms, double* total_work) {
  if (kernel_family < 0 || kernel_family >= PK_COUNT || !count || !total_ms || !total_work) return RL_ERR_ARG;
  return prof_read(kernel_family, count, total_ms, total_work);
}
int realise_cast_to_f32(void* stream, int dtype, const void* src, float* dst, int64_t n) {
  if (!src || !dst) return RL_ERR_ARG;
  RL_BY_DTYPE(0, cast_to_f32<E>((hipStream_t)stream, (const E*)src, dst, n));
}
int realise_fill_f32(void* stream, float* p, float value, int64_t n) { return fill_f32((hipStream_t)stream, p, value, n); }

}  // extern "C"
