/* realise_hip_debug.h - diagnostics of librealise_hip.so: A/B knobs and per-launch timing hooks.
 *
 * NOT part of the operator boundary (include/realise_hip.h): nothing here changes results unless its comment says so, the
 * defaults are the production configuration, and a drop-in user never needs to call any of it.  tools/*.cpp, bench.py
 * (roofline sampling) and the A/B tests do.
 */
#ifndef REALISE_HIP_DEBUG_H
#define REALISE_HIP_DEBUG_H
#include "realise_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 1: ds_read_b64_tr_b16 transposed operand reads in the TN kernel (bf16), 0: 16-bit LDS gathers. */
void realise_set_tn_transpose_read(int enable);
/* A/B knob: allow the 128x96 NT tile chosen by the chip-balance heuristic (default 1) */
void realise_set_nt_allow_n96(int on);
/* Diagnostics: force one NT kernel for dense bf16 GEMMs - 9 the 4-wave kernel, 12 / 14 / 16 the 8-wave 256 x 192 / 128 x 192 three-stage /
 * 128 x 192 two-per-CU tiles, 50 the persistent 256 x 192 kernel wherever it applies, 51 never the persistent kernel; 0 (default) and
 * any other value: chosen from the shape. */
void realise_set_nt_variant(int v);
/* step engine: key 0 = enqueue order of the three forward branches (0: bert stack first, 1: the shorter pinyin / glyph branches first);
 * keys 1 / 2 / 3 = priority class of the pinyin-branch / glyph-branch / weight-gradient stream (-1 highest, 0 device default, +1 lowest),
 * read when the engine creates the stream, i.e. to be set before the first forward; key 4 = classifier backward over the rows that
 * enter the loss only (1, default) or over all rows (0); key 5 = the backward skips the rows of padding tokens, whose gradient rows are
 * exact zeros (LayerNorm backward rows, blocks of the weight-gradient reductions; 1 default: live 16-row blocks packed four to a
 * reduction tile in bf16, 2: whole 64-row tiles only - bit-identical to 0 -, 0 off); key 6 = K-ranges of the split-K classifier data
 * gradient (bf16; default 3, 0 / 1 = one launch over the whole K = 21184); key 9 = a GRU time step as one launch (recurrent GEMM with
 * the gate math in its epilogue: 1, default) or as GEMM + gate kernel (0); key 10 = bf16 training steps run the layer GEMMs of the
 * transformer stacks (forward and data gradients) and the attention forward over the live rows of the padded batch only (2, default:
 * a list of live rows; 1: a list of live 16-row blocks; loss, live-row logits and gradients bit-identical to the dense step; the rows
 * behind a sentence's last attended / loss position keep stale activations) or over all rows (0); key 13 = K7, the glyph lookup fused
 * into the loaders of block 1's forward convolutions (1, default: no gathered image batch in the forward; a training step gathers it
 * at the head of the backward for the two weight-gradient reductions) or gather_images + dense loaders (0); key 14 = K9 in evaluation
 * mode: BatchNorm on its running statistics applied in the glyph convolutions' epilogues (1, default: per block three launches,
 * shortcut first, its normalised output added in the second convolution's epilogue) or as separate scale / shift and apply kernels
 * over the raw convolution outputs (0, the round-5 form); key 15 = realise_engine_adamw_pipelined runs pipelined (1, default) or as
 * the plain sweep on the caller's stream (0).  Other keys are ignored. */
void realise_set_engine(int key, int value);
/* realise_gemm_tn_grouped over a list of live reduction blocks, as the engine's backward calls it: live[k] (device, ascending) = index
 * of the k-th block of `list_rows` rows that holds anything but exact zeros in the A operands, *n_live (device) = how many; the other
 * blocks are not read.  list_rows = 64 (bf16) / 32 (fp32): whole reduction tiles; 16 (bf16): four live blocks form a reduction tile.
 * overwrite != 0: out = result instead of out += result (an empty list then stores exact zeros and leaves the column sums alone).
 * fp32 takes list_rows = 32 only; P must be a multiple of 64 (bf16) / 32 (fp32) and P / list_rows at most 4096 entries (16 KB of LDS;
 * beyond 1024 the launch reserves more than its default 4 KB), else the call is refused.  Pinned by tests/test_tn_edges_gpu.py with
 * NaN in the dead blocks of A and B and dead-block indices behind the count: neither is read. */
/* realise_gemm_nt bounded by a DEVICE-side row count, as the GRU steps of a device-built batch launch it: rows at or beyond
 * *rows_dev contribute zeros (an accumulating epilogue leaves them unchanged, a storing one writes bias-only rows in the last live
 * tile and nothing beyond it).  The contract as observed on both kernels a bf16 launch can reach (tests/test_gemm_edges_gpu.py,
 * counts 0, 1, 128, 129, M - 1, M; the A rows at or beyond the count hold NaN and are never read into anything):
 *   8-wave 128 x 192 with exact row masking (M >= 1024, N >= 256, K % 64 == 0; realise_debug_nt_path 11) and the 4-wave 128-row
 *   tiles (every other shape; paths 2 / 3), alike: rows below the count are the dense launch's; with accumulate every row at or
 *   beyond the count keeps its bits; without it the rows from the count to the end of the 128-row tile that holds the last live row
 *   (or to M) are overwritten with the bias-only row alpha * 0 + bias - finite whatever A holds there -, and every row of a later
 *   tile, every row when the count is 0, keeps what it held.  A caller that reads rows beyond the count after a storing launch
 *   must expect either. */
int realise_gemm_nt_rows(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                         const realise_epilogue* ep, const int* rows_dev);
/* realise_gemm_nt (bf16, K % 64 == 0, M % 16 == 0) over a device-side LIST of 16-row blocks, as a training step launches the layer GEMMs of
 * a padded batch: live_list[k] = index of the k-th listed block (ascending), *live_count = how many.  Rows of listed blocks are computed
 * exactly as the dense launch computes them (bit-identical) and read / written at their original positions; rows of the other blocks
 * are neither read nor written. */
int realise_gemm_nt_live(void* stream, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                         const realise_epilogue* ep, const int* live_list, const int* live_count);
/* Round 6: the same over a device-side list of ROWS (row-granular packing, what a training step launches by default): row_list[k] =
 * index of the k-th listed row (ascending), *row_count = how many; tile t of the 128 x 192 kernel works on rows row_list[128 t ..
 * 128 t + 127], so no tile row is spent on rows that merely complete a 16-row block.  Listed rows: bit-identical to the dense launch. */
int realise_gemm_nt_live_rows(void* stream, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                              const realise_epilogue* ep, const int* row_list, const int* row_count);
/* Split-K form of the 8-wave NT GEMM as the classifier's data gradient uses it (bf16, K % 64 == 0): slab[s][m][n] (fp32, row pitch N,
 * plane pitch slab_stride floats) = A[m, K-range s] . B[n, K-range s]^T; rows at or beyond *m_dev (device, nullable) are not computed. */
int realise_gemm_nt_splitk(void* stream, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K, int nsplit,
                           float* slab, int64_t slab_stride, const int* m_dev);
int realise_gemm_tn_grouped_live(void* stream, int dtype, int n, const realise_tn_problem* problems, int P, const int* live,
                                 const int* n_live, int list_rows, int overwrite);
/* LayerNorm backward exactly as the engine calls it (bf16): optional second output dx_drop = dx * dropout mask, per-workgroup
 * [dgamma | dbeta] records in `slots` (8 MiB scratch) folded in a fixed order.  tools/ln_probe.py times it. */
int realise_layernorm_bwd_ex(void* stream, const void* dy, const void* xhat, const float* rstd, const float* gamma, void* dx, void* dx_drop,
                             uint32_t drop_seed, uint32_t drop_thresh, float drop_scale, float* dgamma, float* dbeta, float* slots, int rows, int H);
/* realise_layernorm_fwd (bf16, rows % 16 == 0) as a live-row training step launches it: row_live = one byte per row (0 = padding).  A
 * 16-row block without a live row is not visited - its y / xhat / rstd rows keep what they held -, a block with one is computed whole. */
int realise_layernorm_fwd_live(void* stream, const void* x, const float* gamma, const float* beta, float eps, void* y, void* xhat, float* rstd,
                               const uint8_t* row_live, int rows, int H);
/* the same with the row-liveness bytes of a padded batch (row_live[r] == 0: dy[r] is an exact zero - the row is not read, its outputs are zeros) */
int realise_layernorm_bwd_live(void* stream, const void* dy, const void* xhat, const float* rstd, const float* gamma, void* dx, void* dx_drop,
                               uint32_t drop_seed, uint32_t drop_thresh, float drop_scale, float* dgamma, float* dbeta, float* slots,
                               const uint8_t* row_live, int rows, int H);
/* LayerNorm kernels: key 0 = bf16 fast path (half a wave per row, 16-byte accesses; default 1), key 1 = workgroups of its backward (default 512);
 * BatchNorm kernels: key 2 = bf16 fast paths (1, default: 16-byte accesses, paired bn2 + shortcut backward, one-pass training
 * statistics; 3: the same with two-pass statistics; 0: generic kernels), key 3 = row chunks of their
 * column reductions (default 1024) ; key 4 = bf16 masked cross-entropy with the logits row read once into registers
 * (1, default) or the generic three-walk kernel (0); key 5 = round-5 LayerNorm kernels (1, default: row reductions through DPP,
 * backward with four rows of a wave in flight, no barrier before the first row, one-barrier epilogue, 256 workgroups; 0: the round-4
 * kernels) - key 1 sets the workgroups of whichever backward is active */
void realise_set_ln(int key, int value);
/* BatchNorm training statistics and backward through the two host functions the engine's glyph branch calls (bn_stats / bn_backward
 * of csrc/ops.h; bf16, NHWC viewed as [P, C]; char_cnn.py:15-32): per-row-chunk partial records in `slots` (1 MiB scratch) folded in a fixed order; `counts` (nullable) =
 * multiplicity of each image of `hw` pixels (glyph dedup), n_stat = the true sample count of the statistics (0: P).
 * stats: mean / rstd / scale / shift [C], running buffers updated (unbiased variance), num_batches_tracked += 1; sq_scratch: C floats.
 * bwd: dx = gamma rstd (g - w sum(g) / n - xhat w sum(g xhat) / n) with g = dy masked by relu_src > 0; dgamma / dbeta are ADDED to;
 * xb != NULL: a second normalisation sharing dy and the mask (bn2 + shortcut BN of a BasicBlock; one pass reads dy and the mask for
 * both - taken while 4 C fits the engine's 2048-float sums scratch, realise_debug_bn_plan says which; otherwise a's reduction and map
 * run first, then b's -); sums: 4C floats of scratch.
 * tools/bn_probe.py times them; tests/test_ops_gpu.py checks fast against generic paths; the bounded forms below are pinned element by
 * element. */
int realise_batchnorm_stats_ex(void* stream, const void* x, int P, int C, int hw, const float* counts, int n_stat, const float* gamma, const float* beta,
                               float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd,
                               float* scale, float* shift, float* sq_scratch, float* slots);
int realise_batchnorm_bwd_ex(void* stream, const void* dy, const void* relu_src, int P, int C, int hw, const float* counts, int n_stat,
                             const void* xa, const float* mean_a, const float* rstd_a, const float* gamma_a, void* dxa, float* dgamma_a, float* dbeta_a,
                             const void* xb, const float* mean_b, const float* rstd_b, const float* gamma_b, void* dxb, float* dgamma_b, float* dbeta_b,
                             float* sums, float* slots);
/* persistent NT kernel (gemm_nt8p.hip): key 0 = tile walk (1 default: every XCD owns a band of tile rows, 0: chunked tile ids),
 * key 1 = workgroups launched (default 256 = one per CU); key 3 = column groups of the XCD split of the live-row layer GEMMs (0 default:
 * from the shape - 2 for the wide K = 768 outputs, 1 otherwise; 1 / 2 / 4 / 8 forced).  Other keys are ignored. */
void realise_set_nt8p(int key, int value);
void realise_set_nt_group_m(int g);        /* tile order of the 8-wave NT GEMM: 0 row-major, g: g tile rows per column step (L2 blocking) */
/* Diagnostics: force the number of reduction splits of the TN kernel (0 = heuristic). */
void realise_set_tn_split(int n);
void realise_set_conv_c64(int on);         /* 1 (default): the 64->64 channel 3x3 conv on 16x16 maps (forward, input and weight gradient) runs the LDS-resident kernels */
/* A/B knob: 1 (default) run the glyph ResNet once per distinct token id with multiplicity-weighted BatchNorm;
 * 0 run it densely over all B*S tokens like the reference (identical results) */
void realise_set_glyph_dedup(int on);
/* A/B knob: 1 (default) = the four weight-gradient GEMMs of each BERT layer run on an engine-owned side stream, overlapped with the
 * data-gradient chain on the caller's stream (joined before realise_engine_backward returns); 0 everything in order on the
 * caller's stream.  Identical results; +2 % throughput measured, per-kernel timings become overlap-dependent. */
void realise_set_wgrad_overlap(int on);
/* 1 (default): the three branches of SpellBertPho2ResArch3.forward that are independent between the inputs and the gate
 * (src/models.py:816 bert | :818-827 pinyin GRU + pho_model | :829-838 glyph ResNet), and their backward passes behind the
 * gate, run on three HIP streams (the caller's + two engine-owned), forked / joined with events inside the engine call; the
 * caller's stream owns every result when the call returns.  0: everything in order on the caller's stream.  Identical results. */
void realise_set_branch_overlap(int on);
void realise_set_dgrad_parity(int on);     /* 1 (default): stride-2 conv data gradients as four input-pixel parity-class GEMMs (no stride-miss taps) */
void realise_set_wgrad_group(int on);      /* 1 (default): the four weight gradients of a transformer layer as one grouped launch */

/* Per-launch timing of the MFMA kernel families with HIP events on the launch stream (bench.py roofline).
 * family: 0 gemm_nt, 1 conv_nt (implicit im2col), 2 gemm_tn, 3 conv_tn, 4 attention fwd, 5 attention bwd.
 * total_work = algorithmic FLOPs (2*M*N*K per GEMM launch). */
int realise_profile_enable(int max_launches);
/* 1 (default): the event pair is attached to the kernel dispatch (its own begin / end timestamps, what rocprofv3's kernel
 * trace reports); 0: two event markers recorded around the launch (adds the marker packets' processing to every sample) */
void realise_profile_mode(int attached);
void realise_profile_disable(void);
/* 1: stop bracketing launches but keep what was recorded, 0: resume (an event pair costs ~4 us of stream time per launch, so
 * bench.py samples every 10th timed step instead of all of them) */
void realise_profile_pause(int paused);
int realise_profile_read(int kernel_family, long long* count, double* total_ms, double* total_work);
/* per-launch records of one family in launch order (host arrays of max_records entries); returns the number written */
int realise_profile_dump(int kernel_family, int max_records, float* ms_out, double* work_out);
/* the same with the EXECUTED work next to the booked (nominal) one: launches bounded by a device-side row count (the loss rows of the
 * classifier's gradients, the live blocks of a padded batch in the weight-gradient reductions, the GRU's alive sequences) book
 * 2.M.N.K for the nominal M and execute fewer rows; the counters are read from the device when the records are read (valid while
 * the batch shape does not change between the sampled steps and the read) */
int realise_profile_read_ex(int kernel_family, long long* count, double* total_ms, double* total_work, double* total_work_executed);
int realise_profile_dump_ex(int kernel_family, int max_records, float* ms_out, double* work_out, double* work_executed_out);

/* Host-side support predicate of the listed weight-gradient launches, exported so that a CPU test can pin it: bytes of LDS a listed
 * TN launch reserves for `entries` live blocks, -1 when the list does not fit (the engine then runs dense reductions). */
int realise_debug_tn_list_lds(int64_t entries);
/* What an ungrouped weight-gradient launch decides on the host, with the knobs as they stand (realise_set_tn_split,
 * realise_set_conv_c64): the host functions the launchers themselves act on, exported so that tests can pin the path a case is meant
 * for (tests/tn_cases.py, tests/test_tn_edges_gpu.py; invariants swept in tests/test_tn_cases_cpu.py).
 * kind: 0 dense B operand (realise_gemm_tn), 1 gathered (realise_conv_tn), 2 gathered and the geometry is the 64 -> 64 channel 3x3 /
 * stride 1 / pad 1 convolution on 16x16 maps without img_index (the caller vouches for the geometry; dtype, P, I, the scratch and the
 * knob are checked here).  Cin > 0: the conv-weight output mapping with that many input channels (0: plain rows).
 * tile: 0 nothing to launch, 1 64 x 256, 2 128 x 128, 3 conv_wgrad_c64.  nsplit workgroups along the reduction, each owning pchunk rows
 * (before a device-side bound re-splits them inside the kernel).  form: 0 direct (out read-modify-written in place), 1 one slab plane
 * per split + fold, 2 fp32 atomics.  fold: 0 none, 1 tn_fold_plain_kernel, 2 tn_fold_convw_kernel, fold_sb its split-lane count
 * (1, 2, 4, 8, 16).  conv_wgrad_c64 always writes slab planes (form 1), a single split included.  Returns 0, or non-zero where the
 * launch would be refused. */
typedef struct realise_tn_plan { int32_t tile, nsplit, pchunk, form, fold, fold_sb; } realise_tn_plan;
int realise_debug_tn_plan(int dtype, int kind, int P, int I, int J, int Cin, int scratch_given, int64_t scratch_elems, realise_tn_plan* plan);
/* realise_gemm_tn exactly as the engine launches it, with the TnEpi fields the operator boundary hides: out (+)= alpha * *alpha_dev *
 * A^T B (alpha_dev: device scalar, nullable - the incoming loss gradient of the classifier's weight gradient), the reduction bounded by
 * *rows_dev (device, nullable: GRU alive count, loss rows, glyph dedup; rows at or beyond it are not read and the splits are re-cut
 * over the live rows inside the kernel), overwrite != 0: out = result (honoured by the direct form only, as in the engine), conv_KHW >
 * 0: the conv-weight output mapping out[(i * conv_Cin + ci) * conv_KHW + tap + tap0] for column j = tap * conv_Cpad + ci (the centre
 * tap of a 3x3 convolution on a 1x1 map is the dense launch J = conv_Cpad, conv_KHW = 9, tap0 = 4; the other taps are not touched).
 * tests/test_tn_edges_gpu.py: bounds 0, 1, BP, BP + 1, P - 1, P, P + 5 with NaN in the rows at or behind the bound, through the fold,
 * the atomics and the column sums. */
int realise_gemm_tn_ex(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int P, int I, int J,
                       float* out, int64_t ldo, float* scratch, int64_t scratch_elems, float* colsum_out, float alpha,
                       const float* alpha_dev, const int* rows_dev, int overwrite, int conv_Cin, int conv_Cpad, int conv_KHW, int tap0);
/* realise_conv_tn likewise: alpha, alpha_dev, the device-side bound on the pixel rows (whole images) and, with img_index, the number
 * of images in the table (the 32-bit span check; 0 = not checked). */
int realise_conv_tn_ex(void* stream, int dtype, const void* A, int64_t lda, const realise_conv_geom* b, int P, int Co, int Ci,
                       float* out, float* scratch, int64_t scratch_elems, float alpha, const float* alpha_dev, const int* rows_dev,
                       int64_t index_rows);
/* Which kernel realise_gemm_nt (rows_dev_given = 0) or realise_gemm_nt_rows (1) reaches for a shape, an epilogue (alpha = 1) and the
 * knobs as they stand (realise_set_nt_variant, realise_set_nt_allow_n96): the host function the launcher itself acts on, exported so
 * that tests can pin the kernel a case is meant for.  -1 refused (argument error), 0 nothing to launch; 4-wave kernels: 1 256 x 64,
 * 2 128 x 128, 3 128 x 96, 4 256 x 128 with spread fetches; 8-wave kernels: 5 256 x 192, 6 128 x 192 three-stage, 7 128 x 192
 * two-per-CU, 8 the ragged-K instantiation; 9 persistent 256 x 192, 10 the same bounded by the device-side row count; 11 8-wave
 * 128 x 192 two-per-CU with exact row masking under a device-side row count.
 * mode 16: the route of realise_gemm_nt_decode for (dtype, M, N, K, lda, ldb) and k = `accumulate` (0 counts as 1) - 9, 2 or 3, or
 * -1 where it is refused; has_aux, ldo, ldaux and rows_dev_given are ignored. */
int realise_debug_nt_path(int dtype, int M, int N, int K, int mode, int accumulate, int has_aux, int64_t lda, int64_t ldb, int64_t ldo,
                          int64_t ldaux, int rows_dev_given);

/* What the BatchNorm launches decide on the host for a [P, C] map of images of hw pixels, with the knobs as they stand
 * (realise_set_ln keys 2 and 3): the host functions the launchers themselves act on, exported so that tests can pin the kernel a case
 * is meant for (tests/tower_cases.py, tests/test_tower_edges_gpu.py; invariants swept in tests/test_tower_cases_cpu.py).
 * slots_given: the record scratch is passed (the engine always does); branches: 1, or 2 = the backward of bn2 + the shortcut's BN.
 * Per pass - stats (training statistics), apply, bwd_reduce, bwd_apply -: kernel 0 generic, 1 the 16-byte kernels, 2 the one-pass
 * statistics (bn_stats_train16; stats only), 3 the paired backward (bn_bwd_reduce2 / bn_bwd_apply2; both backward passes or neither);
 * reductions: g row chunks with one record of `stride` floats each, folded by fold_wgs workgroups (stride 0: no records - fp32
 * atomics); overwrite 1: the outputs are overwritten (records + fold), 0: accumulated (atomics).  Two-pass statistics run two
 * reductions of the reported plan.  Maps report g = stride = fold_wgs = 0, overwrite = 1.  Returns 0, or non-zero where a launch would
 * be refused. */
typedef struct realise_bn_pass { int32_t kernel, g, stride, fold_wgs, overwrite; } realise_bn_pass;
typedef struct realise_bn_plan { realise_bn_pass stats, apply, bwd_reduce, bwd_apply; } realise_bn_plan;
int realise_debug_bn_plan(int dtype, int P, int C, int hw, int slots_given, int branches, realise_bn_plan* plan);
/* Which kernel realise_conv_nt reaches for a gathered launch with the knobs as they stand (realise_set_conv_c64,
 * realise_set_nt_allow_n96): 12 = conv_c64_nt (bf16, the 64 -> 64 channel 3x3 / stride 1 / pad 1 convolution on 16x16 maps without
 * img_index, N = 64, ldb = K = 576, M = rows a multiple of 256, ldo = 64, alpha 1, a plain store or mode 8 with scale and shift),
 * else the realise_debug_nt_path id of the 4-wave kernel (1, 2, 3), 0 nothing to launch, -1 refused.  The host function
 * gemm_nt_conv itself acts on; src / img_index are only compared with NULL.  has_scale: mode 8 carries col_scale and the shift. */
int realise_debug_conv_nt_path(int dtype, const realise_conv_geom* a, int64_t ldb, int M, int N, int K, int mode, int accumulate, int has_aux,
                               int has_scale, int64_t ldo, int64_t ldaux);
/* realise_conv_nt and realise_gemm_nt exactly as the engine's glyph branch launches them, with what the operator boundary hides:
 * rows_dev (device, nullable) bounds the output rows - whole images of a gathered launch; rows at or behind it are not read -,
 * index_rows the number of images in the table behind img_index (the 32-bit span check; 0 = not checked), and the evaluation-mode
 * BatchNorm folded into the epilogue: mode 8, out = [relu](acc * col_scale[col] + ep->bias[col] (+ ep->aux)), the shift riding in
 * ep->bias.  col_scale is valid with mode 8 only.  The dense form with B = W + 4 Co, ldb = 9 Co is the centre tap of a 3x3 convolution
 * on 1x1 maps.  tests/test_tower_edges_gpu.py: bounds 0, one image, all with NaN in the images behind the bound, in the table images
 * img_index skips and in the padding channels' weights; the rows behind the bound keep their bits under the storing epilogues the
 * tests run (see realise_gemm_nt_rows above for the last live tile of a dense launch). */
int realise_conv_nt_ex(void* stream, int dtype, const realise_conv_geom* a, const void* B, int64_t ldb, int M, int N, int K,
                       const realise_epilogue* ep, const float* col_scale, int relu, const int* rows_dev, int64_t index_rows);
int realise_gemm_nt_ex(void* stream, int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                       const realise_epilogue* ep, const float* col_scale, int relu, const int* rows_dev);
/* realise_conv_dgrad_s2 under a device-side bound: conv_dgrad_s2 of csrc/gemm.h, the host function the engine's stride-2 data gradients
 * go through (class loop, tap-less classes, the one-tap 2x2 case).  *rows_dev (nullable) counts INPUT pixel rows (whole images); each parity-class launch takes a quarter of it.  Input rows at or behind the bound keep their bits in
 * every class (tests/test_tower_edges_gpu.py: bounds 0, one image, all, with NaN in the gradient rows of the images behind it). */
int realise_conv_dgrad_s2_ex(void* stream, int dtype, const realise_conv_geom* a, const void* B_classes, int64_t ldb, int Cin,
                             const realise_epilogue* ep, const int* rows_dev);
/* The BatchNorm passes of the engine's glyph branch, for fp32 and bf16: stats_rows and bwd_rows are bn_stats / bn_backward of
 * csrc/ops.h, the host functions the engine itself calls, apply_rows is bn_apply.  Every kernel is bounded by *rows_dev (device,
 * nullable; glyph dedup: distinct glyphs x hw - rows at or behind it are neither read nor written and do not enter a sum), `counts`
 * (nullable) the multiplicity of each image of hw pixels, n_stat the true sample count (0: P), `slots` the record scratch
 * (COL_SLOT_FLOATS = 262144 floats; NULL: the reductions use fp32 atomics on zero-filled scratch, as realise_batchnorm_fwd / _bwd do).
 * Pinned by tests/test_tower_edges_gpu.py with NaN in every row at or behind the bound, in the counts behind the last live glyph and
 * in the record scratch, and with guarded outputs whose rows behind the bound keep their bits.
 * stats_rows: training != 0: mean / rstd / scale / shift [C] from the batch, running buffers updated (unbiased variance, momentum),
 *   num_batches_tracked += 1 (nullable); training == 0: scale / shift from the running buffers, nothing else is touched (x may be
 *   NULL).  scratch: 2 C floats.
 * apply_rows: y = [relu](x1 sc1 + sh1 [+ x2 sc2 + sh2]) (x2 nullable: relu(bn2(c2) + bns(cs)) of a BasicBlock).
 * bwd_rows: as realise_batchnorm_bwd_ex (xb nullable: the second normalisation), any dtype, bounded; sums: 4 C floats. */
int realise_batchnorm_stats_rows(void* stream, int dtype, const void* x, int P, int C, int hw, const float* counts, const int* rows_dev, int n_stat,
                                 int training, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                                 float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd, float* scale, float* shift,
                                 float* scratch, float* slots);
int realise_batchnorm_apply_rows(void* stream, int dtype, const void* x1, const float* scale1, const float* shift1, const void* x2,
                                 const float* scale2, const float* shift2, void* y, int P, int C, int hw, int relu, const int* rows_dev);
int realise_batchnorm_bwd_rows(void* stream, int dtype, const void* dy, const void* relu_src, int P, int C, int hw, const float* counts,
                               const int* rows_dev, int n_stat,
                               const void* xa, const float* mean_a, const float* rstd_a, const float* gamma_a, void* dxa, float* dgamma_a, float* dbeta_a,
                               const void* xb, const float* mean_b, const float* rstd_b, const float* gamma_b, void* dxb, float* dgamma_b, float* dbeta_b,
                               float* sums, float* slots);

/* how many workspace plans the engine has installed (= whole-workspace zero fills) since it was created: a loop that alternates
 * batch shapes over per-shape workspace buffers (realise_engine_forget_workspace in realise_hip.h) must count one per shape */
int64_t realise_engine_plan_installs(const realise_engine* e);
/* Read-only: descriptor i of the engine's table of Linear weights and their operand copies (the CastDesc table the refresh and the
 * AdamW sweep launch over), so that a test can find the copies a sweep wrote (tests/test_optim_edges_gpu.py).  src_off: element offset
 * of the fp32 master W [R][C] inside the trainable parameter arena; dst_off / dstT_off: byte offsets inside the bound shadow buffer of
 * the compute-dtype copies W [R][C] and W^T [C][ldT] (ldT >= R: the classifier's W^T is padded to a multiple of 64 columns, which
 * stay zero), -1 for a copy the engine does not keep; group: 0 = the BERT stack's launch, 1 = classifier / head / pinyin and output
 * stacks / GRU (tile ids restart per group).  Returns the number of descriptors (out may be NULL to ask for it alone), or
 * -REALISE_ERR_ARG for a NULL engine, an index outside [0, count) with out != NULL, or before the engine has built the table (it does
 * at its first forward / refresh). */
typedef struct realise_cast_desc_info { int64_t src_off, dst_off, dstT_off; int32_t R, C, ldT, group; } realise_cast_desc_info;
int realise_debug_engine_cast_desc(const realise_engine* e, int i, realise_cast_desc_info* out);

/* The pinyin GRU as the engine launches it (engine.hip gru_forward / gru_backward): thin wrappers over the functions it calls, no
 * arithmetic of their own.  Pinned element by element by tests/test_gru_edges_gpu.py.
 * table_fwd: table[v][j] = b_ih[j] + emb[v, :] . w_ih[j, :], fp32, [V][3H]; H > 1024 or V < 1 is refused.
 * table_bwd: dtable [V][ld >= 3H] -> d_emb [V][H] (row 0, the padding symbol, is not touched), d_w_ih [3H][H], d_b_ih [3H], all
 *   ACCUMULATED onto what the buffers hold; V > 64 is refused.
 * step_*_rows: realise_gru_step_fwd / _bwd with the device-side row bound: a->n_alive is the launch bound, rows at or behind
 *   *n_alive_dev are skipped.
 * step_fused (bf16): one time step t > 0 as ONE launch - gh = h_prev . w_hh^T + b_hh with the gate math in the GEMM's epilogue; a->gh
 *   is an OUTPUT here (only its n third is written), a->h_prev the GEMM's A operand [n_alive][H], w_hh_bf16 the plain [3H][ldb]
 *   weight; H % 64 != 0 (and whatever else gemm_nt8_gru refuses) returns its REALISE_ERR_ARG. */
int realise_gru_table_fwd(void* stream, const float* emb, const float* w_ih, const float* b_ih, int V, int H, float* table);
int realise_gru_table_bwd(void* stream, const float* dtable, int ld, const float* emb, const float* w_ih, int V, int H, float* d_emb,
                          float* d_w_ih, float* d_b_ih);
int realise_gru_step_fwd_rows(void* stream, int dtype, const realise_gru_step* a, const int32_t* n_alive_dev);
int realise_gru_step_bwd_rows(void* stream, int dtype, const realise_gru_step* a, const int32_t* n_alive_dev);
int realise_gru_step_fused(void* stream, const realise_gru_step* a, const void* w_hh_bf16, int64_t ldb, const int32_t* n_alive_dev);


/* Attention and the row-liveness tables as a live-row training step launches them (engine.hip: attn_fwd / attn_bwd with the table
 * rlen, row_liveness): thin wrappers over the functions it calls, no arithmetic of their own.  Pinned element by element by
 * tests/test_row_edges_gpu.py.
 * attention_fwd_rows / attention_bwd_rows: realise_attention_fwd / _bwd plus rlen, a device pointer to B ints (NULL: the plain call).
 *   Rows at or beyond rlen[b] of sentence b are padding: masked as keys, never read as queries.  Forward: the q / k / v rows there are
 *   not read, and the ctx / lse rows of the 32-query blocks that start at or beyond rlen[b] keep what they held (the rows between
 *   rlen[b] and the end of the block that holds it are written with finite values nobody reads).  Backward: nothing read from such a
 *   row (q, k, v, ctx, dctx, lse) enters a result, and its dq / dk / dv rows are stored as exact zeros in every head; its rowdot rows
 *   are not promised.  Rows below rlen[b] are bit-identical to the plain call on the same input with the padding rows zero-filled.
 *   mask_add must mask every key at or beyond rlen[b].
 * row_liveness: row (b, s) is live iff s < 1 + the last position of sentence b with masks == 1 or loss_masks == 1 (loss_masks
 *   nullable).  row_live [B*S] bytes; rlen [B] (nullable) = live rows per sentence; tiles64 / tiles32 / tiles16 (nullable): ascending
 *   indices of the 64- / 32- / 16-row blocks of the B*S token rows that hold a live row, n_tiles[0..2] their counts; rows (nullable):
 *   the live rows themselves, ascending, n_tiles[3] of them.  Entries behind a count, and the count of a NULL list, are not written.
 *   B < 1, S < 1, B*S % 64 != 0 or masks == NULL is refused and nothing is written. */
int realise_attention_fwd_rows(void* stream, int dtype, const void* q, const void* k, const void* v, int64_t ldq,
                               const float* mask_add, void* ctx, int64_t ldc, float* lse, int B, int nh, int S,
                               uint32_t drop_seed, uint32_t drop_thresh, float drop_scale, const int32_t* rlen);
int realise_attention_bwd_rows(void* stream, int dtype, const void* q, const void* k, const void* v, int64_t ldq,
                               const float* mask_add, const void* ctx, const void* dctx, int64_t ldc, const float* lse,
                               float* rowdot, void* dq, void* dk, void* dv, int64_t ldd, int B, int nh, int S,
                               uint32_t drop_seed, uint32_t drop_thresh, float drop_scale, const int32_t* rlen);
int realise_row_liveness(void* stream, const int64_t* masks, const int64_t* loss_masks, int B, int S, uint8_t* row_live, int32_t* tiles64,
                         int32_t* tiles32, int32_t* tiles16, int32_t* n_tiles, int32_t* rlen, int32_t* rows);


#ifdef __cplusplus
}
#endif
#endif /* REALISE_HIP_DEBUG_H */
