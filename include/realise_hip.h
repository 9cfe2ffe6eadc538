/*
 * realise_hip.h - C ABI of the MI355X-native ReaLiSe hot path (librealise_hip.so).
 *
 * The reference (DaDaMrX/ReaLiSe) is 100 % Python on PyTorch; there is no FFI layer in it.  The
 * boundary this library sits behind is the nn.Module protocol of `SpellBertPho2ResArch3` /
 * `SpellBert` (src/models.py:652-870, :32-73) as consumed by src/run.py:191,200,258.  Each entry
 * point below names the reference call site(s) it replaces.  All pointers are DEVICE pointers
 * unless stated otherwise; `stream` is a hipStream_t; no torch types cross this boundary.
 * Every function returns 0 on success, non-zero on error (1 = bad argument, 2 = launch failure).
 * dtype: 0 = float32 (exact-fp32 parity mode, v_mfma_f32_16x16x4_f32), 1 = bfloat16 (speed mode,
 * v_mfma_f32_16x16x32_bf16; fp32 accumulation / statistics).
 */
#ifndef REALISE_HIP_H
#define REALISE_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REALISE_F32 0
#define REALISE_BF16 1
/* fp32 buffers; the dense (Linear) GEMMs split every operand value x in registers into hi = bf16(x), lo = bf16(x - hi) and form
 * hi.hi + hi.lo + lo.hi on the bf16 MFMA with fp32 accumulation (the lo.lo term is not computed).  Accepted by realise_gemm_nt,
 * realise_gemm_nt_decode (a form of it), realise_gemm_nt_rows, realise_gemm_tn, realise_gemm_tn_grouped (+ _live) and the realise_debug_* calls that describe them, and as
 * realise_config.dtype (every other kernel of that engine - convolutions, attention, row kernels - is the REALISE_F32 one); every
 * other operator refuses it. */
#define REALISE_F32_BF16X3 2

/* ------------------------------------------------------------------------------------------
 * Fine-grained operators (each one kernel family).  Used by the engine and by the parity tests.
 * ---------------------------------------------------------------------------------------- */

/* Epilogue of realise_gemm_nt / realise_conv_nt.  mode: 0 store(+bias,+accumulate), 1 bias+erf-GELU
 * (out2 = pre-activation), 2 dropout(acc+bias)+aux (residual), 4 acc * gelu'(aux).
 * The mode-2 mask is recomputed from a counter, never stored: element (row, col) of the M x N output has the counter
 * idx = (row * N + col) mod 2^32 - N the logical width, not the pitch ldo, and row the ORIGINAL row of the output (the live-row
 * launch forms address a listed row by its position in the matrix, not in the list) - and is kept when the 16-bit lane idx & 3 of
 * the hash of quad idx >> 2 is >= drop_thresh >> 16 (drop_thresh == 0: everything is kept, unscaled).  The LayerNorm backward
 * (realise_layernorm_bwd_ex, dx_drop) applies the same mask with N = H. */
typedef struct {
  int32_t mode;
  int32_t accumulate;
  void* out;
  int64_t ldo;
  void* out2;
  const float* bias;
  const void* aux;
  int64_t ldaux;
  float alpha;
  uint32_t drop_seed;
  uint32_t drop_thresh;   /* p * 2^32 ; 0 = no dropout */
  float drop_scale;       /* 1 / (1 - p) */
} realise_epilogue;

/* Implicit-im2col geometry over an NHWC tensor: rows are the pixels of an Hr x Wr map, K = KH*KW*C.
 * mode 0 = forward gather, 1 = data-gradient gather.  img_index (nullable) maps image n to a row
 * of `src` (glyph lookup char_images_multifonts.index_select, src/models.py:829-834). */
typedef struct {
  const void* src;
  const int64_t* img_index;
  int32_t rows, Hr, Wr, Hs, Ws, C, KH, KW, stride, pad, mode;
} realise_conv_geom;

/* C[M,N] = A[M,K] . B[N,K]^T  - nn.Linear forward (modeling_bert.py:221,231-232,273,326,339;
 * models.py:859), and its data gradient when B is the transposed weight. */
int realise_gemm_nt(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb,
                    int M, int N, int K, const realise_epilogue* ep);
/* The same product with a K-SEGMENTED A operand: out[M, N] = [A_0 | A_1 | .. | A_{nsrc-1}] . W^T + bias - the concatenation fusion
 * `integrate(torch.cat((bert, pho, res), -1))` of SpellBertPho2ResArch2 (src/models.py:628-629; :490-491, :228-229 and :140-141 are
 * the same line of its siblings) without the [M, nsrc * Ks] tensor, which is neither written nor read.  W is [N, nsrc * Ks] with row
 * pitch ldw, K-contiguous; segment s is [M, Ks] with its own base a[s] and row pitch lda[s]; nsrc is 2 or 3.  ONE launch and ONE fp32
 * accumulation over K = nsrc * Ks in the order s = 0 .. nsrc - 1 (the reference's arithmetic; no partial sum is rounded to the compute
 * dtype).  The 4-wave kernels of realise_gemm_nt: wherever realise_gemm_nt on the materialised concatenation runs those too (every bf16
 * shape below M = 1024 or N = 256; every fp32 / bf16x3 shape), the two outputs are equal bit for bit.  Not read: the columns of a
 * segment row from Ks to lda[s].  bias nullable.
 * live_list / live_count (both NULL: every row; device pointers): the M dimension is a list of rows (live_unit 1: *live_count row ids)
 * or of 16-row blocks (live_unit 16: block ids) - listed rows are read from and written at their ORIGINAL positions and hold the bits
 * of the dense launch, every other output row is left untouched, *live_count == 0 writes nothing.
 * Refused with the argument error, nothing launched: nsrc outside 2..3, a NULL a[s] below nsrc, NULL w or out, Ks not a positive
 * multiple of the K tile (64 elements for REALISE_BF16, 32 for REALISE_F32 and REALISE_F32_BF16X3: no staged tile straddles two
 * segments), N % 4 != 0, a pitch that is no multiple of 8 (bf16) / 4 (fp32) elements, one of live_list / live_count without the
 * other, a live_unit other than 1 and 16 with a list, a dtype outside 0..2.  M <= 0 or N <= 0 is an empty problem (0, nothing launched). */
typedef struct {
  int32_t M, N, Ks, nsrc;
  const void* a[3];
  int64_t lda[3];
  const void* w; int64_t ldw;
  const float* bias;
  void* out; int64_t ldo;
  const int32_t* live_list; const int32_t* live_count; int32_t live_unit;
} realise_gemm_cat;
int realise_gemm_nt_cat(void* stream, int dtype, const realise_gemm_cat* g);
/* Same with A gathered on the fly: nn.Conv2d forward / input gradient (src/char_cnn.py:15-28). */
int realise_conv_nt(void* stream, int dtype, const realise_conv_geom* a, const void* B, int64_t ldb,
                    int M, int N, int K, const realise_epilogue* ep);
/* Input gradient of a stride-2 nn.Conv2d (char_cnn.py:16,24 under loss.backward()) by parity classes of the input pixel: pixel
 * (2yy+py, 2xx+px) is reached only by the taps kh = ((py+pad)&1) + 2i, kw = ((px+pad)&1) + 2j, so four GEMMs over a quarter of the
 * pixels each with 1 / 2 / 2 / 4 taps (3x3, pad 1) replace one GEMM over all pixels with 9 taps of which 75 % are stride misses.
 * `a` is the full-map mode-1 geometry (rows = N*Hr*Wr, Hr = Wr a power of two, no img_index); B_classes is the [Cin][slot][Co]
 * weight copy whose tap slots are ordered class by class (class c = 2*py+px; inside a class i-major); the result rows are written
 * to their pixel positions.  With a 1x1 / pad 0 kernel only class 0 has a tap: ep->accumulate must be set. */
int realise_conv_dgrad_s2(void* stream, int dtype, const realise_conv_geom* a, const void* B_classes, int64_t ldb, int Cin,
                          const realise_epilogue* ep);
/* out[I,J] += sum_p A[p,i] * B[p,j] (fp32) - nn.Linear weight gradient.  The reduction over p is split
 * over workgroups; `scratch` (fp32, scratch_elems >= I*J, ideally several times that) receives the partial
 * slabs that a second kernel folds into `out` in a fixed order (two launches agree bit for bit; so does the unsplit launch, which
 * adds in place); scratch == NULL falls back to fp32 atomics (reproducible to rounding only).  The column sums are always atomics.
 * NOT READ, whatever they hold: the columns of A from I to lda and of B from J to ldb, every row at or beyond P.  The columns of out
 * between J and ldo are not written; ldo % 4 != 0 takes a scalar epilogue.  I, J, lda, ldb must be multiples of 8 (bf16) / 4 (fp32),
 * else the call is refused.  tests/test_tn_edges_gpu.py pins all of this element by element (P = 1, one vector of columns, ragged
 * tiles, every output form, NaN in everything that is not read). */
int realise_gemm_tn(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb,
                    int P, int I, int J, float* out, int64_t ldo, float* scratch, int64_t scratch_elems,
                    float* colsum_out /* nullable: colsum_out[i] += sum_p A[p,i], the matching bias gradient */);
/* Up to 4 Linear weight gradients that share the token count P in ONE launch (the four Linear layers of a transformer
 * layer: BertSelfAttention q/k/v packed, BertSelfOutput.dense, BertIntermediate.dense, BertOutput.dense,
 * modeling_bert.py:221-232,273,326,339 under loss.backward(), run.py:200): every workgroup owns one 128x128 tile of one
 * problem over the whole reduction, so there is no reduction split, no scratch and no fold pass.
 * out_k[I_k, J_k] += A_k^T B_k, colsum_k[i] += sum_p A_k[p,i] (nullable).  ldo % 4 == 0.  n < 1, n > 4, ldo % 4 != 0 or an I / J / pitch
 * that is no multiple of 8 (bf16) / 4 (fp32) is refused and nothing is written; padding columns and rows at or beyond P are not read
 * (tests/test_tn_edges_gpu.py). */
typedef struct realise_tn_problem {
  const void* A; int64_t lda;      /* dY [P, I] */
  const void* B; int64_t ldb;      /* X  [P, J] */
  int32_t I, J;
  float* out; int64_t ldo;
  float* colsum;
} realise_tn_problem;
int realise_gemm_tn_grouped(void* stream, int dtype, int n, const realise_tn_problem* problems, int P);
/* Conv2d weight gradient into the reference's [Co][Ci][KH][KW] layout: out += dY^T im2col(X) (A = dY [P, Co] with pitch lda, b the
 * forward geometry with C = the padded channel count of X; the columns of the padding channels Ci .. C - 1 are dropped).  Not read:
 * the padding columns of A, rows at or beyond P, table images img_index does not select, anything outside an image (the padding
 * taps, and in the 64-channel 16x16 kernel the halo rows above the first and below the last image row, are zeros that come from no
 * address).  tests/test_tn_edges_gpu.py pins it onto a non-zero `out`, on both kernels. */
int realise_conv_tn(void* stream, int dtype, const void* A, int64_t lda, const realise_conv_geom* b,
                    int P, int Co, int Ci, float* out, float* scratch, int64_t scratch_elems);
/* A/B knobs, probe modes and the per-launch timing hooks live in include/realise_hip_debug.h (diagnostics, not operators). */

/* BertSelfAttention core (modeling_bert.py:239-260): softmax(QK^T/8 + mask_add) -> dropout -> .V
 * q/k/v: [B*S][ldq] token-major, head h at columns 64h..64h+63; ctx [B*S][ldc]; lse [B][nh][S].
 * S <= 128: one workgroup per (batch, head), the whole score tile in registers; S > 128 (max_seq_length 256 / 512, run.py:304): tiles of
 * 128 keys / queries, the forward with a running row maximum and sum (B * nh * S * S < 2^32). */
/* lse[b][h][q] = log sum_{k < S} exp(q.k / 8 + mask_add[b][k]) in fp32, the mask added as the FINITE number it is: a masked key keeps its
 * term exp(.. - 10000), which underflows to an exact zero next to any live key, and a query whose every key is masked gets the softmax
 * over q.k / 8 - 10000 (finite, as the reference's) - there is no -inf and no special case.  The backward recomputes the probabilities as
 * exp(score - lse); rowdot[b][h][q] = sum_d dctx . ctx is its other saved row term (written for every q < S).  In a sentence with at
 * least one live key the dk / dv rows of masked keys are exact zeros. */
/* Dropout (drop_thresh != 0; 0 disables it and drop_scale is not applied): probability (b, h, q, key) is kept iff the 16 random bits
 * of counter idx = ((b * nh + h) * S + q) * S + key (mod 2^32; hence B * nh * S * S < 2^32) under drop_seed are >= drop_thresh >> 16 - the
 * counter rule of every dropout site of this library (csrc/common.h drop_mult) - and a kept probability is multiplied by drop_scale.
 * All six kernels - forward, dK / dV and dQ, one-tile and tiled - regenerate the mask from this one rule: the index is the absolute
 * (query, key) pair, whatever tile or lane computes it.  ctx = (p keep scale) V; the backward applies the same factor to dO V^T and to
 * the probabilities of dV.  tests/row_cases.py att_keep restates the rule; tests/test_row_edges_gpu.py reads it off the outputs of
 * each kernel. */
int realise_attention_fwd(void* stream, int dtype, const void* q, const void* k, const void* v, int64_t ldq,
                          const float* mask_add, void* ctx, int64_t ldc, float* lse, int B, int nh, int S,
                          uint32_t drop_seed, uint32_t drop_thresh, float drop_scale);
int realise_attention_bwd(void* stream, int dtype, const void* q, const void* k, const void* v, int64_t ldq,
                          const float* mask_add, const void* ctx, const void* dctx, int64_t ldc, const float* lse,
                          float* rowdot, void* dq, void* dk, void* dv, int64_t ldd, int B, int nh, int S,
                          uint32_t drop_seed, uint32_t drop_thresh, float drop_scale);
int realise_mask_to_additive(void* stream, const int64_t* masks, float* out, int n);

/* torch.nn.LayerNorm over the last dim (eps inside the sqrt), y/xhat of `dtype`, rstd fp32.  Two-pass statistics in fp32 (mean, then the
 * centred squares): a constant row gives xhat == 0 and y == beta exactly and rstd = 1 / sqrt(eps).  H % 4 == 0, H <= 1024.
 * realise_layernorm_bwd: dx is written; dgamma / dbeta are ACCUMULATED (+=, fp32 atomics or an ordered fold) onto what the buffers hold -
 * the caller zero-fills them once per step, not per call. */
int realise_layernorm_fwd(void* stream, int dtype, const void* x, const float* gamma, const float* beta, float eps,
                          void* y, void* xhat, float* rstd, int rows, int H);
int realise_layernorm_bwd(void* stream, int dtype, const void* dy, const void* xhat, const float* rstd,
                          const float* gamma, void* dx, float* dgamma, float* dbeta, int rows, int H);
/* LayerNorm backward fused with the erf-GELU backward in front of it: the element-wise part of BertPredictionHeadTransform's
 * backward (transformers/modeling_bert.py:419-431, dense -> erf GELU -> LayerNorm), between the decoder's data gradient and the
 * transform's weight gradient.  For a row with upstream dy, saved xhat / rstd and the saved dense pre-activation z:
 *   g = dy * gamma;  da = rstd * (g - mean(g) - xhat * mean(g * xhat));  dz = da * (Phi(z) + z * phi(z))   (fp32 statistics)
 *   dgamma += sum_rows dy * xhat;  dbeta += sum_rows dy   (accumulated, fp32)
 * dy / xhat / z / dz are `dtype`, H % 4 == 0 and H <= 1024 (anything else: REALISE_ERR_ARG, as realise_layernorm_bwd).
 * n_rows_dev (nullable): a device-side row count - only rows [0, min(rows, *n_rows_dev)) are processed, dz rows beyond it are left
 * as they are.  row_index (nullable, [rows] int32): xhat / rstd / z of row r are row row_index[r] of tensors with saved_rows rows
 * (saved_rows == 0: rows) - the compacted gradient rows of a forward that saved every row. */
int realise_layernorm_gelu_bwd(void* stream, int dtype, const void* dy, const void* xhat, const float* rstd, const void* z,
                               const float* gamma, void* dz, float* dgamma, float* dbeta, int rows, int H,
                               const int32_t* n_rows_dev, const int32_t* row_index, int saved_rows);
/* CrossEntropyLoss over rows with loss_mask == 1 (src/models.py:862-869); dlogits nullable.  A row enters the loss when loss_mask == 1 and
 * its label is not -100 (CrossEntropyLoss's default ignore_index): loss_out = the mean of those rows' terms, count_scratch[0] = how many,
 * dlogits (rows of pitch ld, like logits) = (softmax - onehot) / count on those rows and exact zeros on every other row.  The row maximum
 * is subtracted before the exponentials.  With ld > V the logits tail [V, ld) is never read and the dlogits tail [V, ld) is written as
 * exact zeros, so a padded gradient row can feed a GEMM as it is.  EMPTY SELECTION: when no row enters the loss, loss_out = 0,
 * count_scratch[0] = 0 and dlogits is all zeros - a deliberate difference from torch, whose mean over an empty selection is NaN (a
 * step whose batch happens to hold no loss position then adds a zero gradient instead of poisoning the weights).  Through this entry
 * point the rows' terms are added to loss_out by fp32 atomics: the loss is reproducible to rounding, not to the bit (the engine's
 * ordered fold is).  tests/test_row_edges_gpu.py pins all of this. */
int realise_masked_ce(void* stream, int dtype, const void* logits, int64_t ld, const int64_t* labels,
                      const int64_t* loss_mask, int rows, int V, float* loss_out, float* count_scratch, void* dlogits);
/* realise_masked_ce whose row pass also ranks (replaces `active_logits.argmax(dim=-1)`, src/models.py:1343-1346, and the comparison
 * run_pretrain.py:100-104 / 240-243 scores accuracy from): same arguments, same loss, count and gradient rows bit for bit, plus
 * pred_out [rows] - the arg-max column of every row that enters the loss, -1 for every other row - and hits[0] = how many of those
 * predictions equal their label.  Ranking rule (realise_argmax, realise_gemm_nt_decode): on the stored compute-dtype value a beats b
 * when a > b or a is NaN and b is not, the lower column wins on equal values, -0.0 ranks as +0.0, the tail [V, ld) enters nothing.
 * The row kernels keep each row in registers (bf16) or rank during the walk that finds the row maximum: no second read of the logits,
 * and the prediction is taken before a gradient row is stored.  EMPTY SELECTION: every pred_out entry is -1, hits[0] = 0, the loss as
 * documented above. */
int realise_masked_ce_pred(void* stream, int dtype, const void* logits, int64_t ld, const int64_t* labels,
                           const int64_t* loss_mask, int rows, int V, float* loss_out, float* count_scratch, void* dlogits,
                           int64_t* pred_out, int32_t* hits);

/* One time step of the pinyin GRU (nn.GRU over pack_padded_sequence, src/models.py:818-826) on the n_alive longest sequences
 * (tokens sorted by decreasing length: perm[i] = original token of sorted row i, lens[i] its length).  The input projection is a
 * table [33][3H] = W_ih Emb^T + b_ih (fp32); gh = h_prev W_hh^T + b_hh comes from realise_gemm_nt (NULL at t == 0: gh = b_hh,
 * h_prev = 0).  Forward: r, z, n gates -> h_new (sorted rows), rzn saved, out[perm[i]] = h when the sequence ends at this step.
 * Backward (one BPTT step): dh (sorted, in/out: running dL/dh; rows that end here start from dout[perm[i]]) -> dgi / dgh
 * [n_alive][3H] for the table / W_hh gradients, onehot[n_alive][64] of the step's pinyin id. */
typedef struct {
  int32_t n_alive, H, Tp, t;
  const float* table; const int64_t* pho_idx; const int32_t* perm; const int32_t* lens;
  const void* gh; const float* b_hh; const void* h_prev; void* h_new; void* rzn; void* out;
  const void* dout; void* dh; void* dgi; void* dgh; void* onehot;
} realise_gru_step;
int realise_gru_step_fwd(void* stream, int dtype, const realise_gru_step* a);
int realise_gru_step_bwd(void* stream, int dtype, const realise_gru_step* a);
/* Gated fusion (src/models.py:840-850): masked mean of the bert states per sentence, three sigmoid gates from
 * [bert | pho | res | mean] . W[3][4H] + bias, fused = g0 bert + g1 pho + g2 res.  Backward fills dbert / dpho / dres and
 * accumulates dW [3][4H], dbias [3]; mean [B][H], msum [B], g [B*S][4] are saved by the forward, dz [B*S][4] is scratch.
 * nsrc (0 = 3): the gate of the ablation model (src/models_abla.py:239-275) over nsrc = G sources - bert, then pho and res in that
 * order where present (a NULL pho / res is absent; nsrc = 2 takes exactly one of them): W [G][(G+1)H], bias [G], g / dz keep
 * their row pitch of 4.  row_live (nullable, [B*S] bytes): 0 marks a padding row whose d fused is an exact zero - the backward
 * writes its zeros without reading its forward activations. */
typedef struct {
  int32_t B, S, H;
  const void* bert; const void* pho; const void* res; const int64_t* masks; const float* W; const float* bias;
  float* mean; float* msum; float* g; void* fused;
  const void* dfused; void* dbert; void* dpho; void* dres; float* dz; float* dW; float* dbias;
  const uint8_t* row_live;
  int32_t nsrc;
} realise_gate;
int realise_gate_fwd(void* stream, int dtype, const realise_gate* a);
int realise_gate_bwd(void* stream, int dtype, const realise_gate* a);
/* The fusion gate of SpellBertPho2ResArch4 (src/models.py:1139-1150): the same masked mean, gate_net and weighted sum, but the nsrc
 * gates are ONE softmax over the gate_net outputs z (row maximum subtracted, fp32) instead of nsrc independent sigmoids, so g[t][0..nsrc)
 * is a distribution over the modalities.  Same struct, same buffers, same nsrc / row_live rules as realise_gate_fwd. */
int realise_gate_softmax_fwd(void* stream, int dtype, const realise_gate* a);
/* Its backward (autograd of src/models.py:1139-1150): with dg_k = <d fused, src_k>, dz_k = g_k (dg_k - sum_j g_j dg_j); the source
 * gradients g_d d fused + sum_k dz_k W[k][d], the mean's gradient and dW / dbias follow from dz exactly as in realise_gate_bwd. */
int realise_gate_softmax_bwd(void* stream, int dtype, const realise_gate* a);
/* Sum fusion of the ablation model (src/models_abla.py:278-279, fusion == "sum"): fused = (bert + pho) + res over rows x H, in fp32,
 * stored in `dtype`.  The backward hands the same d fused to each branch: dbert = dpho = dres = dfused (one launch, three copies -
 * the branch backwards run concurrently and two of them write into their incoming gradient buffer).  row_live (nullable, [rows]
 * bytes) as in realise_gate: a padding row gets exact zeros, its d fused row is not read. */
int realise_sum_fuse_fwd(void* stream, int dtype, const void* bert, const void* pho, const void* res, void* fused, int rows, int H);
int realise_sum_fuse_bwd(void* stream, int dtype, const void* dfused, void* dbert, void* dpho, void* dres, int rows, int H,
                         const uint8_t* row_live);
/* nn.BatchNorm2d over an NHWC activation viewed as [P = N*H*W][C] (src/char_cnn.py:17-28), optional fused ReLU.  training:
 * batch statistics (two passes: mean, then centred squares), running statistics updated with the unbiased variance and
 * `momentum`, num_batches_tracked += 1 (nullable), save_mean / save_rstd [C] for the backward.  scratch: 4*C floats.
 * Backward: relu_src = the forward's y when ReLU was fused (NULL otherwise); dgamma / dbeta are ACCUMULATED; scratch 2*C floats.
 * The forms the engine runs (device-side row bound, glyph multiplicities, record scratch, two inputs / two branches, eval finalize) are
 * realise_batchnorm_stats_rows / _apply_rows / _bwd_rows in realise_hip_debug.h; pinned element by element by
 * tests/test_tower_edges_gpu.py: the ReLU mask is relu_src > 0 (-0.0 and +0.0 mask, the smallest normal passes); rows at or behind the
 * bound are neither read nor written; eval leaves the running buffers and num_batches_tracked bit-unchanged. */
int realise_batchnorm_fwd(void* stream, int dtype, const void* x, int P, int C, const float* gamma, const float* beta, float eps, float momentum,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked, int training, int relu, void* y,
                          float* save_mean, float* save_rstd, float* scratch);
int realise_batchnorm_bwd(void* stream, int dtype, const void* dy, const void* relu_src, const void* x, const float* save_mean, const float* save_rstd,
                          const float* gamma, int P, int C, void* dx, float* dgamma, float* dbeta, float* scratch);
/* Gradient of BertEmbeddings' three table lookups (modeling_bert.py:183-190) from de = d(word + position + type sum) [B*S][H]:
 * word_grad[ids[t]] += de[t] (nullable), pos_grad[s] += sum_b de[b, s] (pos_zero: everything into row 0), type_grad[0] += sum_t de[t]. */
int realise_embedding_bwd(void* stream, int dtype, const void* de, const int64_t* ids, int B, int S, int H, float* word_grad, float* pos_grad,
                          int pos_zero, float* type_grad);
/* Glyph dedup bookkeeping (no reference counterpart: char_images_multifonts.index_select(0, ids) depends on the id only): the distinct
 * ids in order of first occurrence (uniq_ids), their multiplicities (counts), inv[t] = slot of token t, bounds[0] = #distinct,
 * bounds[1 + k] = #distinct * hw[k].  first_scratch: V ints, flag_scratch: T ints.  realise_segment_sum: out[u] = sum over tokens
 * with inv[t] == u of x[t] (acc: T*C floats of scratch; rows >= *nuniq_dev untouched). */
int realise_glyph_unique(void* stream, const int64_t* ids, int T, int V, int32_t* first_scratch, int32_t* flag_scratch, int64_t* uniq_ids, float* counts,
                         int32_t* inv, int32_t* bounds, int nhw, const int32_t* hw);
int realise_segment_sum(void* stream, int dtype, const void* x, const int32_t* inv, int T, int C, float* acc, void* out, const int32_t* nuniq_dev);
/* The flatten at the top of CharResNet1 (char_cnn.py:74 `h = h.view(h.shape[0], -1)` of an NCHW [N, C, 2, 2] tensor): the tower keeps its
 * maps NHWC, so a row of its top is [p][c] (p = 2y + x, C = H / 4 channels) while the reference's feature index is f = c * 4 + p.  The
 * three operators at that boundary permute inside registers; H % 16 == 0, H <= 1024.
 *   realise_layernorm_fwd_chw4 - resnet_layernorm (models.py:838) of the flattened rows: x holds storage-order rows, row r reads row
 *     row_index[r] of it (nullable: row r); gamma / beta and the outputs y / xhat (nullable) are in feature order, so the backward is
 *     realise_layernorm_bwd.
 *   realise_gather_rows_chw4 - the flatten itself with the per-token gather: out[t][c * 4 + p] = x[inv[t]][p * C + c].
 *   realise_segment_sum_chw4 - its gradient summed over the tokens of a glyph: x [T][H] in feature order,
 *     out[u][p * C + c] = sum over inv[t] == u of x[t][c * 4 + p] (acc: T*H floats of scratch; rows >= *nuniq_dev untouched). */
int realise_layernorm_fwd_chw4(void* stream, int dtype, const void* x, const int32_t* row_index, const float* gamma, const float* beta, float eps,
                               void* y, void* xhat, float* rstd, int rows, int H);
int realise_gather_rows_chw4(void* stream, int dtype, const void* x, const int32_t* inv, int T, int H, void* out);
int realise_segment_sum_chw4(void* stream, int dtype, const void* x, const int32_t* inv, int T, int H, float* acc, void* out, const int32_t* nuniq_dev);

/* Token rows (evaluation; no reference counterpart: pho_gru's last hidden state, models.py:818-826, and
 * resnet_layernorm(resnet(glyph[id])), models.py:829-838 on BatchNorm's running statistics, depend on nothing but the token id, so a
 * table [V, H] of each, in the storage of `dtype`, replaces the computation).  At most two row-kernel launches:
 *   pho_table != NULL:  x[t] = float(pho_table[ids[t]]) + pos[t % S] + type0,  pho_out[t] = LayerNorm(x[t]) * gamma + beta
 *                       - BertEmbeddings of pho_model on inputs_embeds (modeling_bert.py:183-193) with the GRU rows read by id.  Statistics
 *                       and arithmetic order are those of the embedding LayerNorm over rows given directly: the same bits.
 *   res_table != NULL:  res_out[t] = res_table[ids[t]]   (a copy)
 * ids [T] int64, each in [0, rows of the tables): NOT checked here (the engine passes its range-checked copy).  Both tables have the row
 * pitch ld, the outputs their own; every access is 16 bytes, so table and output rows are 16-byte aligned.
 * Accepts dtypes 0 and 1.  Refused with the argument error before anything is launched: H % 8 != 0, H < 8 or H > 1024; ld below H or
 * no multiple of 8; an output pitch below H or no multiple of 8; T <= 0 or S <= 0; both tables NULL; a table without its output; NULL ids;
 * a pho_table without pos / type0 / gamma / beta. */
typedef struct {
  const int64_t* ids;
  int32_t T, S, H;
  const void* pho_table; const void* res_table; int64_t ld;
  const float* pos; const float* type0; const float* gamma; const float* beta; float eps;
  void* pho_out; int64_t ld_pho_out;
  void* res_out; int64_t ld_res_out;
} realise_token_rows_args;
int realise_token_rows(void* stream, int dtype, const realise_token_rows_args* a);

/* Eval decode: ids[row] = argmax over the V logits of the row, first maximum wins - replaces
 * `logits.detach().cpu().numpy()` + `np.argmax(preds, axis=-1)` (src/run.py:262-263): only the ids cross PCIe. */
int realise_argmax(void* stream, int dtype, const void* logits, int64_t ld, int rows, int V, int64_t* ids);

/* Top-k decoding fused into the classifier GEMM: C = A . B^T + bias is never stored.  Replaces the [B, S, V] logits of
 * models.py:859-869 plus `np.argmax(preds, -1)` (src/run.py:262-263, src/test.py:143) where only the corrections - and how sure the
 * model is of them - are wanted.  Per row: the best k columns (ids), their logits (values), exp(value - lse) (probs), the row's
 * log-sum-exp over all N columns (lse) and, with `labels`, the logit at labels[row] (label_logit; a label outside [0, N) leaves its
 * entry unwritten).  Ranking is on the value the default forward would have stored - bf16(acc + bias) widened to fp32 for
 * REALISE_BF16 (what realise_batch.logits_f32_out holds), the fp32 value otherwise; a beats b when a > b or a is NaN and b is not,
 * the lower column on equal values (realise_argmax's rule and numpy's); -0.0 ranks, and is reported, as +0.0.  Columns >= N enter
 * nothing.  With k = 1 the launch takes the persistent 256 x 192 kernel exactly where realise_gemm_nt with a plain store to pitch N
 * would; otherwise, and for k > 1, the 4-wave 128 x 128 / 128 x 96 tile of the cost rule (realise_debug_nt_path, mode 16).  Where the
 * decode launch and the plain store run the same kernel, `values` are the stored logits bit for bit; where the plain store would take
 * another kernel (an 8-wave kernel of small N at M >= 1024, the 256 x 128 tile, the persistent kernel for k > 1), equality with the
 * stored logits holds up to accumulation order only.  Each (row, column slab of one wave) leaves one record in `scratch`
 * (16-byte aligned, realise_gemm_nt_decode_scratch_bytes of the same arguments, which is 0 for a refused shape); a merge kernel folds
 * them in ascending column order, so two launches agree bit for bit.  Refused (argument error, before any pointer is read): N <= 64,
 * N < k, N % 4 != 0, a K or pitch realise_gemm_nt refuses, k outside 1..4, a scratch that is too small. */
typedef struct {
  int32_t k;                 /* 1..4 */
  int64_t* ids;              /* [rows, k] */
  float* values;             /* [rows, k] logits as the default forward would have stored them */
  float* probs;              /* [rows, k] exp(value - lse) */
  float* lse;                /* [rows] */
  float* label_logit;        /* nullable, [rows]: the value at labels[row] */
  void* scratch; int64_t scratch_bytes;
} realise_decode;
int64_t realise_gemm_nt_decode_scratch_bytes(int dtype, int M, int N, int K, int k);
int realise_gemm_nt_decode(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb,
                           int M, int N, int K, const float* bias, const int64_t* labels /* nullable */,
                           const realise_decode* d);

/* ------------------------------------------------------------------------------------------
 * Whole-model engine: SpellBert.forward (models.py:50-73) / SpellBertPho2ResArch3.forward
 * (models.py:806-870) and their autograd (`loss.backward()`, run.py:200), one C call each.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t model_type;        /* 0 = SpellBert (BERT only), 1 = SpellBertPho2ResArch3, 2 = SpellBertPho2ResArch3Abla (models_abla.py:33-299),
                              * 3 = SpellBertPho2ResArch4 (models.py:1023-1170): Arch3's tensors and schedule with the softmax gate; its
                              * glyph table is the nn.Embedding [V, 1024] (models.py:1043,1134), so it needs num_fonts == 1, glyph_size == 32,
                              * 4 = SpellBertPho2ResArch3MLM (models.py:874-1020): Arch3 with one font whose classifier is BertOnlyMLMHead
                              * (cls.predictions.*: dense -> erf GELU -> LayerNorm -> untied decoder + bias); num_fonts == 1,
                              * glyph_size == 32 and tie_classifier == 0,
                              * 5 = Pho2Pretrain (models.py:1286-1347; run_pretrain.py's 'pho2-pretrain'): the pinyin branch alone -
                              * pho_embeddings, pho_gru, pho_model (pho_layers deep; bert_layers is carried and ignored) - under a
                              * BertOnlyMLMHead named cls2.  No bert stack, fusion, glyph tower or output block; src_idx is the batch's
                              * tgt_idx (models.py:1319); tie_classifier == 0, with_pho == 1 and with_res == 0 (the branches it has: a
                              * type-5 config that claims a glyph branch is refused); gradient buckets: 0 = cls2, 1 = the pinyin branch,
                              * 6 = SpellBertPho2ResArch2 (models.py:513-649): Arch3's branches - bert, pinyin GRU + pho_model, glyph tower +
                              * resnet_layernorm - fused by CONCATENATION: integrate = nn.Linear(3H, H) over torch.cat((bert, pho, res), -1)
                              * (models.py:628-629, one realise_gemm_nt_cat launch) in front of a TWO-layer output_block; no gate_net.  The
                              * config says what the model is: with_pho == 1, with_res == 1, fusion == 2, num_fonts == 1, glyph_size == 32
                              * (char_images.weight [V, 1024], models.py:533), out_layers == 2; image_model_type 0 or 1; tied or untied,
                              * 7 = SpellBertPho2 (models.py:163-249): the same without the glyph branch - integrate = nn.Linear(2H, H) over
                              * torch.cat((bert, pho), -1): with_pho == 1, with_res == 0, fusion == 2, out_layers == 2.
                              * Gradient buckets of 6 / 7: 0 = classifier + output_block, 1 = integrate (+ resnet_layernorm and the glyph
                              * tower), 2 = the pinyin branch, then the bert layer groups and the bert embeddings */
  int32_t dtype;
  int32_t hidden, heads, intermediate, vocab, max_pos, type_vocab;
  int32_t bert_layers, pho_layers, out_layers;
  int32_t num_fonts, glyph_size, pho_vocab;
  float hidden_dropout, attn_dropout, ln_eps;
  int32_t tie_classifier;    /* classifier.weight aliases bert word embeddings (models.py:700-701) */
  /* model_type 2, and model_type 5 as (1, 0, 0) (ignored otherwise; run.py:373-375): 1 = the pinyin branch / the glyph branch is present; fusion 0 = gate over
   * the G = 1 + with_pho + with_res sources (gate_net [G, (G+1)H]), 1 = sum (needs both branches), 2 = concatenation through
   * `integrate` (model_type 6 / 7 only, which require it) */
  int32_t with_pho, with_res, fusion;
  /* the glyph encoder (run.py:292,419-421 --image_model_type; models.py:681-686): 0 = CharResNet (char_cnn.py:36-55: five blocks,
   * num_fonts input channels, a [768, 1, 1] top), exactly what a zero-initialised field gave before it existed; 1 = CharResNet1
   * (char_cnn.py:57-75: four blocks 64-128-192-192, ONE input channel, a [192, 2, 2] top flattened channel-major to 768).  Read where
   * the configuration has a glyph branch: type 1 there needs num_fonts == 1 (the reference builds CharResNet1 with in_channels = 1
   * and dies at its first forward otherwise), hidden == 768 and glyph_size == 32.  Any other value is refused. */
  int32_t image_model_type;
} realise_config;

/* Parameter layout: the library is the source of truth for where each state_dict tensor of the
 * reference lives inside five flat arenas:
 *   0 trainable fp32 (ordered by backward completion, so DDP buckets are contiguous slices)
 *   1 trainable-but-never-used fp32 (poolers, unused word embeddings: no gradient, as in the reference)
 *   2 frozen fp32 (char_images_multifonts)   3 fp32 buffers (BN running stats)   4 int64 buffers */
int realise_layout_count(const realise_config* cfg);
int realise_layout_entry(const realise_config* cfg, int index, char* name, int name_cap, int32_t* arena,
                         int64_t* offset, int32_t* ndim, int64_t* shape4);
int64_t realise_arena_elems(const realise_config* cfg, int arena);
/* gradient-bucket boundaries (element offsets into arena 0, in backward completion order) */
int realise_bucket_count(const realise_config* cfg);
int realise_bucket_bounds(const realise_config* cfg, int bucket, int64_t* begin, int64_t* end);

typedef struct realise_engine realise_engine;
realise_engine* realise_engine_create(const realise_config* cfg, float* params, float* grads, float* unused_params,
                                      float* frozen, float* buffers_f32, int64_t* buffers_i64);
void realise_engine_destroy(realise_engine* e);
int64_t realise_engine_shadow_bytes(const realise_engine* e);
int64_t realise_engine_workspace_bytes(const realise_engine* e, int B, int S, int Tp);   /* Tp = -1: glyph-only plan */
/* hand the engine its operand-shadow arena and its activation workspace (caller-allocated).  The shadow arena must be
 * ZERO-FILLED by the caller: padded operand rows (the classifier's W^T copy is pitched to 64 columns) rely on it. */
int realise_engine_bind(realise_engine* e, void* shadow, void* workspace, int64_t workspace_bytes);
/* Workspace slots (round 6).  The engine installs one plan per (B, S, Tp) INTO the bound workspace (zero-filled once, then kept
 * self-cleaning) and remembers it per workspace address: a caller that keeps one buffer per batch shape (train batch, eval batch, the
 * short last batch of run.py:104-123's windows, the glyph-only plan) and re-binds the matching one before a forward pays the zero
 * fill once per shape instead of on every switch.  Call this before freeing a buffer the engine has been bound to. */
void realise_engine_forget_workspace(realise_engine* e, void* workspace);
/* re-derive the compute-dtype operand copies from the fp32 masters (after any parameter update) */
int realise_engine_refresh_shadows(realise_engine* e, void* stream);
/* the same, for a caller whose last parameter update was realise_engine_adamw (which wrote the Linear weights' copies itself):
 * linear_current != 0 re-derives only the conv-weight copies (and the glyph table's image when it changed) */
int realise_engine_refresh_shadows_ex(realise_engine* e, void* stream, int linear_current);
/* the frozen glyph table (arena 2) changed: rebuild its NHWC operand image at the next refresh */
void realise_engine_invalidate_frozen(realise_engine* e);
/* zero_grad() without the memset: fresh != 0 tells the engine that the gradient arena holds nothing the caller wants kept - the
 * next backward (or glyph backward) then zero-fills only what it accumulates into (one launch) and STORES the Linear weight
 * gradients of the transformer layers (80 % of the arena) instead of adding to them.  The flag clears itself at that backward;
 * without it gradients are accumulated into the arena as autograd does (run.py:200 under gradient_accumulation_steps). */
void realise_engine_set_grads_fresh(realise_engine* e, int fresh);
/* Token-id range errors.  nn.Embedding raises IndexError for an id outside its table (modeling_bert.py:183-186 word ids,
 * models.py:818 pinyin ids, :831 glyph lookup).  The engine never indexes with a caller's id: every forward first copies src_idx /
 * pho_idx into its workspace with out-of-range ids replaced by 0 and sets *flag = 1 (sticky; device memory or host-mapped pinned
 * memory, nullable) when it replaced one.  The caller reads the flag when it next touches the host (the Python module: at the
 * next forward / backward / decode) and raises; results of a flagged step are meaningless, but no memory outside the tables was read.
 * Only flag[0] is read or written, so a caller may pass a longer array. */
void realise_engine_set_id_flag(realise_engine* e, int32_t* flag);
/* The gradient arriving at the loss (`grad_output` of loss.backward(): 1, or 1 / gradient_accumulation_steps, src/run.py:197-200) as
 * a DEVICE fp32 scalar that realise_engine_backward reads when it runs (NULL = 1, the default).  It scales the three gradients that
 * leave the classifier head inside the kernels that store them; the host never reads it and the cross-entropy gradient rows are
 * not touched.  The pointer must stay valid until the backward's kernels have run; it stays installed until changed. */
void realise_engine_set_loss_grad(realise_engine* e, const float* grad_dev);
/* Inference without logits (replaces models.py:859-869 + src/run.py:262-263 / src/test.py:143 `np.argmax(preds, -1)`): with a decode
 * request installed, realise_engine_forward with training == 0 and logits_out == NULL runs the MLM transform over every row (where
 * the variant has one) and realise_gemm_nt_decode on the classifier input - rows = B * S, the outputs in `d` - and, with tgt_idx /
 * loss_masks, writes the masked mean of lse - label_logit to loss_out (d->label_logit is then required).  The struct is copied; NULL
 * clears the request.  Without a request a NULL logits_out behaves as before. */
void realise_engine_set_decode(realise_engine* e, const realise_decode* d);
/* What a pretraining loop reads next to the loss (replaces src/models.py:1343-1346 `active_logits.argmax(dim=-1)` and
 * `input_ids.view(-1)[active_loss]`, the second and third entry of Pho2Pretrain.forward's tuple): with a request installed, every
 * realise_engine_forward that computes the cross-entropy (logits or no-logits form; not the decode form) also writes, for the j-th
 * row that enters the loss in ascending row order, pred_ids[j] = the arg-max column of its logits (realise_masked_ce_pred's rule)
 * and labels[j] = its tgt_idx, n_active[0] = how many such rows, hits[0] = how many predictions equal their label.  All device
 * pointers, written on the forward's stream; entries j >= capacity are not written; labels / n_active / hits are nullable.  The
 * ranking rides the cross-entropy pass that holds the row: no [B*S, V] tensor is read again.  B * S <= 65536.  The struct is copied;
 * NULL clears the request.  Every model type takes it. */
typedef struct {
  int64_t* pred_ids; int64_t* labels; int32_t* n_active; int32_t* hits; int64_t capacity;
} realise_pred;
void realise_engine_set_pred(realise_engine* e, const realise_pred* d);

typedef struct {
  int32_t B, S, Tp;
  int32_t training;           /* dropout + BatchNorm batch statistics + keep activations for backward */
  int32_t want_dlogits;       /* compute d loss / d logits during the loss pass (needed before backward) */
  uint64_t seed;              /* dropout stream for this step */
  const int64_t* src_idx;     /* [B,S] */
  const int64_t* masks;       /* [B,S] */
  const int64_t* loss_masks;  /* [B,S] nullable when tgt_idx is null */
  const int64_t* tgt_idx;     /* [B,S] nullable */
  const int64_t* pho_idx;     /* [B*S,Tp] (arch3) */
  const int32_t* pho_perm;    /* [B*S] tokens sorted by decreasing pinyin length (device) */
  const int32_t* pho_lens_sorted; /* [B*S] (device) */
  const int32_t* n_alive;     /* HOST array [Tp]: #sequences with length > t; NULL when n_alive_dev is given */
  float* loss_out;            /* 1 float (device), nullable when tgt_idx is null */
  void* logits_out;           /* [B*S, vocab] in `dtype` (device).  A bf16 TRAINING call with tgt_idx, loss_masks, masks and want_dlogits set
                               * (B*S % 64 == 0) computes the transformer stacks only on the rows that precede a sentence's last position with
                               * masks == 1 or loss_masks == 1: the loss, those rows' logits and every gradient equal the dense computation bit
                               * for bit; the logits rows behind that position are finite and meaningless (the reference never reads them:
                               * src/run.py:200, :262-270).  Engine knob 10 = 0 (the setter is declared in include/realise_hip_debug.h) computes every row. */
  const int32_t* n_alive_dev; /* DEVICE array [Tp] written by realise_build_pho (used when n_alive == NULL) */
  int32_t eval_live_rows;     /* != 0 on an evaluation call (training == 0, bf16, B*S % 64 == 0): the transformer stacks run over the rows up to every
                               * sentence's last position with masks == 1 (or loss_masks == 1) only, as training steps do - those rows' logits and the
                               * loss are bit-identical to the dense forward's, the logits rows of the padding behind that position are finite and
                               * meaningless (the reference's evaluation cuts its predictions at `lengths`: src/run.py:262-270).  Default 0: dense. */
  float* logits_f32_out;      /* nullable: [B*S, vocab] fp32 (device) - the logits widened to fp32, the dtype the reference returns them in
                               * (src/models.py:859); bf16 engines write them from the classifier kernel's epilogue (the same bf16-rounded
                               * values as logits_out), no pass over logits_out.  Needs logits_out. */
} realise_batch;

/* Device-side `build_batch` (src/models.py:797-804 with the per-character Pinyin2.convert of src/utils.py:58-99 folded into
 * a per-vocabulary table built once on the host): for every token t of src_idx[T]
 *     pho_idx[t][0..Tw) = table[src_idx[t]][0..Tw),   len[t] = vlens[src_idx[t]]
 * then the tokens stably sorted by decreasing length (perm, lens_sorted) and n_alive[k] = #{t : len[t] > k}, all on the
 * device: no per-character host loop and no host list `pho_lens` in the forward contract.  Feed the outputs to
 * realise_batch {pho_idx, pho_perm, pho_lens_sorted, n_alive = NULL, n_alive_dev, Tp = Tw}. */
int realise_build_pho(void* stream, const int64_t* src_idx, int T, const int64_t* table, const int32_t* vlens, int V, int Tw,
                      int64_t* pho_idx, int32_t* perm, int32_t* lens_sorted, int32_t* n_alive_dev);
int realise_engine_forward(realise_engine* e, void* stream, const realise_batch* batch);
/* Token tables (evaluation / serving): the two branches of an evaluation forward that see no context, read by token id.
 *   pho[id] = the row pho_gru hands to pho_model (tap "pho_gru"),  res[id] = the row the fusion reads (tap "res_h": after
 *   resnet_layernorm, in the reference's feature order for both glyph encoders)
 * each [rows = vocab][ld] in the engine's storage dtype (bf16, or fp32 for REALISE_F32 / REALISE_F32_BF16X3), caller-owned, 16-byte
 * aligned, ld >= hidden and a multiple of 8.  A model has a table per side branch it has (the other pointer is NULL).
 * realise_engine_fill_token_tables runs the engine's own pinyin GRU, glyph tower and resnet_layernorm - in evaluation form, at the plan
 * of the batch's (B, S, Tp), nothing else - on the batch's src_idx / pho_* and stores row t at index src_idx[t] (range-checked) of each
 * table: a row is produced by the kernel instantiations a full forward of that shape runs.  The operand copies must be current
 * (realise_engine_refresh_shadows).  It needs no masks, targets or outputs in the batch.
 * realise_engine_set_token_tables installs the tables (the struct is copied; NULL switches them off, as realise_engine_set_decode):
 * every realise_engine_forward with training == 0 then runs neither the GRU nor the tower - pho_model's embedding LayerNorm reads
 * pho[src_idx] and res_h is a copy of res[src_idx] (realise_token_rows) - and accepts a batch without pho_idx / pho_perm /
 * pho_lens_sorted / n_alive*; a forward with training != 0 returns the argument error.  The tables are valid for the parameters,
 * buffers and glyph table they were filled from: the caller switches them off when any of those changes.  The taps "pho_gru",
 * "resnet.block*" and "glyph.*" then hold what an earlier forward left.  Workspace and shadow sizes do not change.
 * Refused (argument error; set: nothing is installed, what was installed stays): rows != vocab, ld < hidden or ld % 8 != 0, hidden % 8
 * != 0, a table for a branch the model lacks, a missing table for a branch it has, model_type 5 (its input is tgt_idx and its
 * evaluation is one short pass) and a model without a side branch. */
typedef struct { void* pho; void* res; int64_t ld; int32_t rows; } realise_token_tables;
int realise_engine_fill_token_tables(realise_engine* e, void* stream, const realise_batch* batch, const realise_token_tables* t);
int realise_engine_set_token_tables(realise_engine* e, const realise_token_tables* t);
/* gradients of the loss computed by the last training forward are ACCUMULATED into the grads arena.
 * Runs buckets [first_bucket, last_bucket] of the backward pass (see realise_bucket_bounds) so a
 * caller can overlap the all-reduce of finished buckets; pass 0, -1 for the whole pass. */
int realise_engine_backward(realise_engine* e, void* stream, int first_bucket, int last_bucket);
/* The whole pass (as first_bucket = 0, last_bucket = -1: the three model branches on three streams, weight gradients deferred
 * to the engine's side stream) that also tells a data-parallel caller when each gradient bucket is final: bucket_events[i]
 * (n_events = realise_bucket_count hipEvent_t handles owned by the caller) is recorded on the stream that finishes bucket i;
 * the caller's communication stream waits on it (hipStreamWaitEvent) and all-reduces the bucket while the rest of the backward
 * runs - what DistributedDataParallel's gradient hooks do for run.py:165-167,200.  On return the caller's stream is ordered after
 * the whole pass. */
int realise_engine_backward_signalled(realise_engine* e, void* stream, void* const* bucket_events, int n_events);
/* Glyph-only entry points (BASELINE configs[3], the glyph-CNN stress run): CharResNet.forward (src/char_cnn.py:46-55) on the
 * B*S glyph stacks char_images_multifonts[src_idx] (src/models.py:829-836), before resnet_layernorm.  res_out / d_res are
 * [B*S, 768] in the engine's compute dtype.  The workspace is sized with realise_engine_workspace_bytes(e, B, S, -1).
 * training != 0: BatchNorm uses batch statistics and updates the running buffers; realise_engine_glyph_backward then
 * ACCUMULATES the conv / BatchNorm parameter gradients for d_res into the grads arena. */
int realise_engine_glyph_forward(realise_engine* e, void* stream, const int64_t* src_idx, int B, int S, int training, void* res_out);
int realise_engine_glyph_backward(realise_engine* e, void* stream, const void* d_res);
/* named view of an internal activation (parity tests): returns 0 and fills ptr/numel if it exists */
int realise_engine_tap(realise_engine* e, const char* name, void** ptr, int64_t* numel);

/* ------------------------------------------------------------------------------------------
 * Optimizer step adjacent to the path (transformers/optimization.py:110-169, run.py:207-211)
 * ---------------------------------------------------------------------------------------- */
int realise_sumsq(void* stream, const float* g, int64_t n, float* out_accum);
int realise_adamw(void* stream, float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int64_t step, int correct_bias,
                  const float* grad_norm_sq, float max_grad_norm);
/* clip_grad_norm_ (run.py:207) for a caller that steps with a stock optimizer: g *= min(1, max_norm / (sqrt(*grad_norm_sq) + 1e-6)),
 * grad_norm_sq from realise_sumsq - no host synchronisation */
int realise_clip_scale(void* stream, float* g, int64_t n, const float* grad_norm_sq, float max_grad_norm);
/* The same sweep with per-group hyper-parameters (the trainer's decay / no-decay groups, run.py:146-151, with a non-zero
 * --weight_decay): group_of_block64[i / 64] is the group (index into `groups`, HOST array of <= 8) of elements [64 b, 64 b + 64)
 * - every tensor of the parameter arena starts on a 64-element boundary - and 255 marks elements no group holds. */
typedef struct { float lr, beta1, beta2, eps, weight_decay; int32_t correct_bias; } realise_adamw_group;
int realise_adamw_grouped(void* stream, float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* group_of_block64,
                          const realise_adamw_group* groups, int n_groups, int64_t step, const float* grad_norm_sq, float max_grad_norm);
/* The grouped sweep over the ENGINE's parameter / gradient arenas (transformers/optimization.py:110-169, run.py:207-211), with the
 * operand copies of the Linear weights written by the pass that updates them: those tensors (90 % of the parameters) are stepped in
 * the 64 x 64 tiles of the operand-copy kernel, which stores the new fp32 value and its compute-dtype W / W^T copies together; the
 * rest by the flat sweep.  m / v: the caller's moment arenas (same layout as the parameter arena).  Follow it with
 * realise_engine_refresh_shadows_ex(e, stream, 1) instead of the full refresh. */
int realise_engine_adamw(realise_engine* e, void* stream, float* m, float* v, const uint8_t* group_of_block64,
                         const realise_adamw_group* groups, int n_groups, int64_t step, const float* grad_norm_sq, float max_grad_norm);
/* realise_engine_adamw, PIPELINED across the step boundary (round 6; run.py:207-211 followed by the next iteration's run.py:191).  The
 * sweep streams 32 bytes per parameter and nothing overlaps it while it sits between the backward and the next forward on `stream`.
 * This form orders the engine's side stream behind `stream` (gradients and grad_norm_sq are final there) and runs the sweep on it in the
 * order the next forward consumes the parameters, an event behind every piece: [everything outside the Linear weights, the tied
 * word table / classifier, BERT layers 0-1] [layers 2-3] [pinyin + output stacks, GRU] [the remaining BERT layers two by two].
 * realise_engine_forward and realise_engine_refresh_shadows_ex make their streams wait for a piece right in front of its first reader
 * and for all of it before they return, so the caller's stream is held for the first piece only (~0.3 of the ~1.1 ms at the full model
 * size).  Same kernels and per-element arithmetic as realise_engine_adamw: the same bits.  CONTRACT: between this call and the next
 * realise_engine_forward / realise_engine_refresh_shadows_ex(e, s, 0) / realise_engine_sync_optimizer nothing else may read or write
 * the parameter, gradient or moment arenas on any stream.  (Engine knob 15 = 0, declared in realise_hip_debug.h, turns it into the plain sweep.) */
int realise_engine_adamw_pipelined(realise_engine* e, void* stream, float* m, float* v, const uint8_t* group_of_block64,
                                   const realise_adamw_group* groups, int n_groups, int64_t step, const float* grad_norm_sq, float max_grad_norm);
/* order `stream` behind every piece of a pending pipelined sweep (no-op without one): before a checkpoint, a state_dict, any access to
 * the arenas from outside the engine */
int realise_engine_sync_optimizer(realise_engine* e, void* stream);
int realise_fill_f32(void* stream, float* p, float value, int64_t n);
/* widen a compute-dtype tensor to fp32 (the reference returns fp32 logits, src/models.py:859); 16-byte aligned pointers */
int realise_cast_to_f32(void* stream, int dtype, const void* src, float* dst, int64_t n);

const char* realise_version(void);

#ifdef __cplusplus
}
#endif
#endif /* REALISE_HIP_H */
