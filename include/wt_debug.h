/* wt_debug.h — kernel-level taps for parity tests (host in / host out, synchronous).
 * NOT part of the drop-in boundary (wt_capi.h); they exist so that a parity failure of
 * the whole path can be localised to one gfx950 kernel.  epi bits: 1 bias, 2 GELU(erf),
 * 4 residual (R, same shape as the output), 8 positional add. */
#ifndef WT_DEBUG_H_
#define WT_DEBUG_H_
#include "wt_capi.h"
#ifdef __cplusplus
extern "C" {
#endif
/* C[M][N] = epi(A[M][K] . W[N][K]^T); needs N % 128 == 0, K % 32 == 0 */
int wt_dbg_gemm(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias,
                const float* R, const float* pos, int pos_period, int epi, float* C);
/* the default encoder GEMM on fp16 planes (k_gemm_planes.hip): A and W are split on the host with scales from the data;
 * planes_out != 0 returns the plane output reconstructed as (hi + lo) / scale; iters > 0 also times the launch */
int wt_dbg_gemm_planes(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias,
                       const float* R, const float* pos, int pos_period, int epi, int planes_out, int iters, float* C,
                       float* avg_ms, int n_cu /* CUs the tile choice assumes; 0 = all */);
/* Teacher forcing for step-by-step comparisons: ids [clips][32] (prompt first) that every following decode of exactly
 * `clips` clips (for a pair of pipelined batches: both, in chain order) feeds to the decoder instead of its own argmax
 * choices; logits, id counts and the EOT rule are computed as always, the returned ids are the given ones.  clips = 0
 * switches it off.  Ids outside the vocabulary are refused by the decode (WT_ERR_INVALID_ARG). */
int wt_dbg_set_forced_ids(wt_engine* h, const int64_t* ids, int clips);
/* schedule of the 384-column plane-GEMM tiles for subsequent launches of this process: 0 = gemm_planes_tile (both
 * wavefronts of a SIMD in step), 1 = gemm_planes_pp (ping-pong groups, 32 x 32 x 16), 2 = gemm_planes_pp16 (ping-pong groups on
 * 16 x 16 x 32 MFMAs; its persistent form where a CU runs several plane-output tiles: the default), 4 = the same without the
 * persistent form; A/B measurements in one process */
int wt_dbg_set_plane_gemm_mode(int mode);
/* the same GEMM (N = 384, fp32 output C, epi = bias | residual (5) or bias | gelu | pos (11)) with the LayerNorm of the
 * finished rows fused into its epilogue: ln_out [M][384] = LayerNorm(C row) * ln_g + ln_b reconstructed from the planes
 * the kernel wrote, ln_y32 (optional) its fp32 copy; *fused = 1 when a 384-column tile did it, 0 when the tile choice
 * (n_cu, M) took the narrow tile and nothing was written */
int wt_dbg_gemm_planes_ln(wt_engine* h, int M, int K, const float* A, const float* W, const float* bias, const float* R,
                          const float* pos, int pos_period, int epi, const float* ln_g, const float* ln_b, int n_cu,
                          float* C, float* ln_out, float* ln_y32, int* fused);
/* encoder attention on planes (k_attention_planes.hip): qkv fp32 [B*T][3*heads*64] is split on the host the way the
 * qkv GEMM's epilogue writes it; out [B*T][heads*64] reconstructed from the output planes */
int wt_dbg_encoder_attention_planes(wt_engine* h, int batch, int T, int heads, const float* qkv, int iters, float* out,
                                    float* avg_ms);
/* times `iters` back-to-back launches of the encoder GEMM on random operands (HIP events on the
 * engine's stream); variant selects the tile shape (k_gemm.hip) */
int wt_dbg_gemm_bench(wt_engine* h, int M, int N, int K, int epi, int variant, int iters, float* avg_ms);
/* (wt_dbg_dec_gemm_bench, below) times back-to-back launches of a decoder GEMM: kind 0 residual, 1 LayerNorm-fused (3: + logits and argmax records),
 * 2 combine + residual; rows = B x positions in the pass (<= 128) */
/* Interference probe: enqueues `n_enc` encoder passes over d_mel [batch][80][3000] on the encoder
 * stream and, concurrently, a chain of `chain_len` dependent trivial launches (`blocks` x 64
 * threads) on a decoder stream; returns the device time of each. */
int wt_dbg_interference(wt_engine* h, const float* d_mel, int batch, int n_enc, int chain_len, int blocks,
                        float* enc_ms, float* chain_ms);
/* Concurrency probe with the real kernels: `n_dec` (0..4) decodes over cached cross-KV slots next to
 * `n_enc` (0..4) pipelined encoder passes over d_mel (device, [batch][80][3000]); needs six
 * earlier batches so that every slot is populated. dec_ms[n_dec], enc_ms[1] = device times. */
int wt_dbg_concurrency(wt_engine* h, const float* d_mel, int batch, int n_dec, int n_enc, float* dec_ms,
                       float* enc_ms);
int wt_dbg_dec_gemm_bench(wt_engine* h, int kind, int B, int N, int K, int rows, int iters, float* avg_us);
/* decoder-step GEMM (k_decoder.hip), plain input X[B][K] (B <= 128 rows), W[N][K] (split into fp16 planes and tiled internally):
 * mode 0: Y = X.W^T + bias   1: gelu(...)   2: Y = R + bias + X.W^T (in-place residual form)
 * mode 3: Y = X.W^T and argmax_out[B] = last maximal column (reference tie rule) */
int wt_dbg_dec_gemm(wt_engine* h, int mode, int B, int N, int K, const float* X, const float* W,
                    const float* bias, const float* R, float* Y, int64_t* argmax_out);
/* LN-fused decoder GEMM: x = xin (or, when ids != NULL, x[b] = tok_emb[ids[b]] + pos_emb[pos], also
 * returned in xout); Y = act(LayerNorm(x).W^T + bias).  K in {128, 384, 512}. */
int wt_dbg_dec_ln_gemm(wt_engine* h, int B, int N, int K, const float* xin, const int64_t* ids, int pos,
                       const float* tok_emb, const float* pos_emb, int n_vocab, int n_pos,
                       const float* ln_g, const float* ln_b, const float* W, const float* bias,
                       int gelu, float* Y, float* xout);
int wt_dbg_layernorm(wt_engine* h, int M, int d, const float* x, const float* g, const float* b, float* y);
/* qkv [B*T][3*heads*64] -> out [B*T][heads*64] */
int wt_dbg_encoder_attention(wt_engine* h, int batch, int T, int heads, const float* qkv, float* out);
/* decoder cross attention with its fused query projection: x [nq*B][d] residual rows (row = p * B + b),
 * q = LayerNorm(x; ln_g, ln_b) . wq^T + bq (wq [d][d] row-major), kc/vc [B][heads][T][64] -> out [nq*B][d] */
int wt_dbg_cross_attention(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                           const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                           const float* vc, float* out);
/* launch_cross_attention ALONE, positions row0 .. row0 + n_rows - 1 of a buffer of nq positions (nq * batch <= 128): the
 * arguments of wt_dbg_cross_attention, x [nq * batch][d] whole; ws [nq * batch][heads][chunks][68] (o[64], m, l, pad per
 * record) is in / out: uploaded as given, written by the one launch at the rows of its positions (addressed as the
 * engine's position loop addresses them) and downloaded whole, so that every record the launch does not own comes back
 * as given.  What the launcher refuses (batch, heads or T below 1, chunks outside [1, T], n_rows outside [1, 4]:
 * WT_ERR_INVALID_ARG; a d = 64 heads other than 128, 384, 512: WT_ERR_FORMAT) is refused before anything is allocated
 * or launched, and so are a NULL array and positions outside the buffer (WT_ERR_INVALID_ARG). */
int wt_dbg_cross_attention_records(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                                   const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                                   const float* vc, int row0, int n_rows, float* ws);
/* the kProCombine prologue of dec_gemm alone, on given records [M][heads][chunks][68]: Y = R + bias + combine(records) . W^T
 * through launch_dec_gemm(kProCombine, kDecResid) with R aliasing Y, as in the engine; W [d][d], bias [d], R [M][d],
 * d = 64 heads, M = positions x B rows (M <= 128, M % B == 0), chunks in {1, 2, 4, 8}.  Y [M + guard_rows][d] is in / out:
 * rows < M are set to R before the launch, rows >= M are uploaded as given, and all come back. */
int wt_dbg_cross_combine(wt_engine* h, int M, int B, int heads, int chunks, const float* records, const float* W,
                         const float* bias, const float* R, int guard_rows, float* Y);
/* decoder self attention (self_attention_step): qkv [npos*B][3d] (row = p * B + b); caches [B][cap][d], cap <= 448,
 * updated in place at rows pos .. pos+npos-1; out [npos*B][d].  pos < 0, npos < 1, pos + npos > 32, pos + npos > cap, cap
 * outside [1, 448] and a batch or head count below 1 are WT_ERR_INVALID_ARG, before anything is launched. */
/* absorbed cross-attention (k_cross_absorbed.hip) + chunk combine with the heads' value projections: qp [nq * batch]
 * [heads * d] absorbed queries (log2 domain), E [batch][T][d] encoder output (split into planes on the host), wv [d][d],
 * bv [d]; out [nq * batch][d]: out[r][64 h + j] = Wv[64 h + j] . (sum_k softmax2_k(qp_h . e_k) e_k) + bv[64 h + j];
 * d = 64 * heads.  iters > 0 also times the attention launch. */
int wt_dbg_cross_absorbed(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* qp, const float* E,
                          const float* wv, const float* bv, float* out, int iters, float* avg_us);
/* the same with E as ONE bf16 plane (bf16 storage mode): queries and probabilities rounded to bf16 in the kernel */
int wt_dbg_cross_absorbed_bf16(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* qp, const float* E,
                               const float* wv, const float* bv, float* out, int iters, float* avg_us);
/* the absorbed cross-attention as a decoder chain runs it (Engine::decode's position loop, then cross_absorbed_combine):
 * bf16 != 0 selects the one-plane form.  n_src (1..4) encoder batches of `split` clips each, the last one shorter:
 * E_src[i] [clips of group i][T][d] on the host, every source a device allocation of its own with room for `batch`
 * clips at ONE plane stride and ONE e_scale (from the maximum over all sources); the clips a group does not have hold
 * NaN, so a wrong source or clip offset shows.  n_src == 1 needs split == batch.  qp [nq * batch][heads * d], wv [d][d],
 * bv [d].  out [nq * batch + 1][d] and ws [nq * batch + 1][heads][chunks][d + 4] (the raw workspace: c[d], m, l, pad per
 * record) are in / out, the last row of each a guard the kernels must not write.
 * mode 0: positions in steps of cross_absorbed_max_nq(heads), then combine; 1: ONE attention launch over positions
 * p0_only .. p0_only + nq_only - 1, then combine; 2: combine alone over the given ws (E_src, qp unused).
 * A shape the launcher refuses is WT_ERR_INVALID_ARG, before anything is launched. */
int wt_dbg_cross_absorbed_chain(wt_engine* h, int bf16, int batch, int heads, int T, int chunks, int nq, int split, int n_src,
                                const float* const* E_src, const float* qp, const float* wv, const float* bv, int mode,
                                int p0_only, int nq_only, float* out, float* ws);
/* the host fold of the absorbed query projection (absorbed_query_matrix, engine.cpp): wq, wk [d][d] row-major, bq [d],
 * d = 64 * heads -> A [heads * d][d] (A_h = c0 Wk_h^T Wq_h), av [heads * d] (a_h = c0 Wk_h^T bq_h),
 * c0 = 1/8 log2 e.  Needs no engine and no GPU. */
int wt_dbg_absorbed_query_matrix(int heads, int d, const float* wq, const float* bq, const float* wk, float* A, float* av);
int wt_dbg_self_attention(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                          float* kcache, float* vcache, float* out);
/* self_attention_long (k_attention.hip, option "max_positions"): ONE new position `pos` against caches [B][cap][d],
 * cap <= 448; qkv [B][3d], out [B][d]; the caches come back with row pos appended and nothing else changed.  pos < 0,
 * pos >= cap, cap > 448 and a batch or head count below 1 are WT_ERR_INVALID_ARG, before anything is launched. */
int wt_dbg_self_attention_long(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv, float* kcache,
                               float* vcache, float* out);
/* self_attention_prefill (k_attention.hip, wt_engine_set_context): npos >= 1 new positions pos .. pos + npos - 1 against
 * caches [B][cap][d], cap <= 448; qkv [npos * B][3d] and out [npos * B][d], rows p * B + b; the caches come back with rows
 * pos .. pos + npos - 1 appended and nothing else changed.  pos < 0, npos < 1, pos + npos > cap, cap > 448,
 * npos * batch > 128 and a batch or head count below 1 are WT_ERR_INVALID_ARG, before anything is launched. */
int wt_dbg_self_attention_prefill(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                  float* kcache, float* vcache, float* out);
/* The ragged forms of the two (wt_engine_set_contexts): the same arguments plus start [B] and P.  pos
 * counts slots and clip b is at Whisper position pos - start[b]; a position outside [0, P) is void: its `out` rows come
 * back zero and its caches untouched, every other clip's rows carry the bits of the unragged tap at the shifted
 * position.  The refusals are the unragged ones, except that the long form's slot may lie past the cache (below 896);
 * P outside [1, cap] and a NULL start are refused too. */
int wt_dbg_self_attention_long_ragged(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv, float* kcache,
                                      float* vcache, float* out, const int32_t* start, int P);
int wt_dbg_self_attention_prefill_ragged(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                         float* kcache, float* vcache, float* out, const int32_t* start, int P);
/* The bf16 forms of the two ragged taps (option full_bf16_all): the caches are float32 arrays of
 * bf16-representable values, as wt_dbg_self_attention_long_bf16 takes them.  A live clip's rows carry the bits of
 * wt_dbg_self_attention_long_bf16 / wt_dbg_self_attention_prefill_bf16 at the shifted position; the refusals are those of
 * the fp32 ragged taps. */
int wt_dbg_self_attention_long_ragged_bf16(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv, float* kcache,
                                           float* vcache, float* out, const int32_t* start, int P);
int wt_dbg_self_attention_prefill_ragged_bf16(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                              float* kcache, float* vcache, float* out, const int32_t* start, int P);
/* The gathered form of self_attention_long (full-length beam search): the arguments of
 * wt_dbg_self_attention_long — `rows` in the place of the batch, at most 128 — plus anc [rows][cap] bytes.  Row r reads
 * key k < pos from cache row min(anc[r][k], rows - 1) and appends key pos to its own row; entries at k >= pos are not
 * read.  With anc[r][k] = r the output and the caches carry the bits of wt_dbg_self_attention_long.  The refusals are
 * that tap's; rows > 128 and a NULL table are refused too. */
int wt_dbg_self_attention_long_gather(wt_engine* h, int rows, int heads, int cap, int pos, const float* qkv, float* kcache,
                                      float* vcache, float* out, const uint8_t* anc);
/* wt_dbg_dec_ln_gemm's embedding rows under a slot count: row b = tok_emb[ids[b]] + pos_emb[clamp(pos - pos_start[b], 0,
 * n_pos - 1)]; pos_start = NULL is wt_dbg_dec_ln_gemm with ids. */
int wt_dbg_dec_ln_gemm_ragged(wt_engine* h, int B, int N, int K, const int64_t* ids, int pos, const int32_t* pos_start,
                              const float* tok_emb, const float* pos_emb, int n_vocab, int n_pos, const float* ln_g,
                              const float* ln_b, const float* W, const float* bias, int gelu, float* Y, float* xout);
/* ragged_cap (k_misc.hip): finished[b] = 1 where pos - start[b] == P - 1, unchanged elsewhere; batch 1..64 */
int wt_dbg_ragged_cap(wt_engine* h, int batch, int pos, int P, const int32_t* start, int32_t* finished);
/* ts_partial + ts_select (k_timestamps.hip, option "timestamps"): one step of Whisper's timestamp
 * rules per row.  logits [B][V]; row b of ids [B][ids_stride] holds n_ids[b] ids, the first sample_begin of them the
 * prompt, and the step decides the id that follows them: token[b].  L [B] (optional) = rule 5's logsumexp of the allowed
 * timestamp logits, M [B] (optional) = the best allowed logit below beg; NaN where no such id is allowed.  The carried
 * state is derived from the id row on the device (ts_state_init).  Needs 0 <= eot < beg < V <= 262144, B <= 64 and
 * 1 <= sample_begin <= n_ids[b] <= ids_stride, else WT_ERR_INVALID_ARG before anything is launched. */
int wt_dbg_timestamp_select(wt_engine* h, int B, int V, const float* logits, const int64_t* ids, int ids_stride,
                            const int32_t* n_ids, int sample_begin, int eot, int beg, int max_initial_timestamp,
                            int64_t* token, double* L, float* M);
/* sample_partial + sample_select (k_sample.hip, option "temperature"): one sampling step per row.
 * logits, ids, n_ids, sample_begin, eot, beg, max_initial_timestamp, token, L and M as wt_dbg_timestamp_select;
 * timestamps = 0: the allowed set is the whole vocabulary (beg and max_initial_timestamp unused, L is NaN, M the row's
 * maximum).  temperature [B]: 0 = greedy (no random number is drawn), else the token is the argmax of
 * z / T + Gumbel noise from Philox4x32-10 under the key (seed & 0xffffffff, seed >> 32) and the counter
 * (id >> 2, position, clip_base + b, attempt); the position is `pos`, or n_ids[b] - 1 where pos < 0.
 * key [B] (optional) = the winning key as the kernel formed it.  Needs 0 <= eot < V (timestamps: eot < beg < V),
 * V <= 262144, B <= 64, temperature >= 0 and 1 <= sample_begin <= n_ids[b] <= ids_stride, else WT_ERR_INVALID_ARG
 * before anything is launched. */
int wt_dbg_sample_select(wt_engine* h, int B, int V, const float* logits, const int64_t* ids, int ids_stride,
                         const int32_t* n_ids, int sample_begin, int timestamps, int eot, int beg, int max_initial_timestamp,
                         const float* temperature, uint64_t seed, int attempt, int clip_base, int pos, int64_t* token,
                         double* L, float* M, float* key);
/* The grouped sampler (SampleArgs::group, option "best_of"): ONE launch over B rows that are `group`
 * samples of clips = ceil(B / group) clips, row r = sample r / clips of clip r % clips.  Arguments as
 * wt_dbg_sample_select, except: every row holds the same number n_ids of ids; temperature [clips] is per clip; row0 is the
 * first clip's entry of the parameter block.  Sample j draws under the attempt word attempt + (j << 16), clip c under the
 * clip word clip_base + row0 + c.  group = 1 is the ungrouped launch.  Needs group <= 8 and, for group > 1, B <= 128 and
 * row0 + clips <= 64 (group = 1: row0 + B <= 64), else WT_ERR_INVALID_ARG before anything is launched. */
int wt_dbg_sample_select_group(wt_engine* h, int B, int group, int V, const float* logits, const int64_t* ids, int ids_stride,
                               int n_ids, int sample_begin, int timestamps, int eot, int beg, int max_initial_timestamp,
                               const float* temperature, uint64_t seed, int attempt, int clip_base, int row0, int pos,
                               int64_t* token, double* L, float* M, float* key);
/* best_of_begin (k_best_of.hip): the start of a chain over N samples of `clips` clips, rows
 * r = j * clips + c.  All arrays are in / out with N * clips rows: ids [..][stride] (rows c < clips hold the clips' prompts
 * on entry), n_ids, finished, sum (float64), count, anc [..][cap] (bytes); frozen [clips] is optional.  Needs N <= 8,
 * N * clips <= 128, clips <= 64 and 1 <= n_prompt <= cap < stride, cap <= 448. */
int wt_dbg_best_of_begin(wt_engine* h, int clips, int N, int n_prompt, int stride, int cap, const int32_t* frozen,
                         int64_t* ids, int32_t* n_ids, int32_t* finished, double* sum, int32_t* count, uint8_t* anc);
/* best_of_pick (k_best_of.hip): per clip the first sample with the largest sum / count in float64 (a NaN or a count
 * below 1 never wins; sample 0 where none is left).  Inputs over N * clips rows, r = j * clips + c: ids [..][stride],
 * lp [..][stride], n_ids, sum, count.  Outputs, in / out over n_out rows of which c0 .. c0 + clips - 1 are written:
 * out_ids / out_lp [n_out][stride] (the winner's first n_ids entries, zeros behind them), out_n, out_sum, out_count,
 * picked, all_sum / all_count [n_out][8].  Needs N <= 8, N * clips <= 128, c0 + clips <= n_out <= 64, 2 <= stride <= 449. */
int wt_dbg_best_of_pick(wt_engine* h, int clips, int N, int c0, int n_out, int stride, const int64_t* ids, const float* lp,
                        const int32_t* n_ids, const double* sum, const int32_t* count, int64_t* out_ids, float* out_lp,
                        int32_t* out_n, double* out_sum, int32_t* out_count, int32_t* picked, double* all_sum,
                        int32_t* all_count);
/* score_partial + score_finish (k_scores.hip, option "scores") alone: the log-probability of the id
 * each row chose at one step.  logits [B][V]; row b of ids [B][ids_stride] holds n_ids[b] ids, the LAST of them the id
 * the step chose (any id in [0, V)), the first sample_begin the prompt.  timestamps = 0: every id is allowed; 1: the set
 * the timestamp rules leave behind the n_ids[b] - 1 earlier ids (state by ts_state_init, eot / beg / max_initial_timestamp
 * as wt_dbg_timestamp_select), rule 5 decided as ts_select decides it.  live [B]: 1 = the clip was live at the step.
 * sum [B] / count [B] in / out: the carried per-clip sum and count, advanced where live.  lp [B]; den [B] (optional) = the
 * float64 logsumexp of the allowed set.  B <= 64, n_ids[b] in [max(sample_begin, 0) + 1, ids_stride]. */
int wt_dbg_token_scores(wt_engine* h, int B, int V, const float* logits, const int64_t* ids, int ids_stride,
                        const int32_t* n_ids, int sample_begin, int timestamps, int eot, int beg, int max_initial_timestamp,
                        const int32_t* live, float* lp, double* sum, int32_t* count, double* den);
/* bf16 storage mode kernels (option "bf16"): operands are rounded to bf16 on the host, contracted by
 * gemm_bf16_planes / encoder_attention_planes<true>; bf16_out = 1 returns the kernel's bf16 output widened to fp32 */
int wt_dbg_gemm_bf16(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias,
                     const float* R, const float* pos, int pos_period, int epi, int bf16_out, int iters, float* C,
                     float* avg_ms);
/* x = R + bias + A . W^T on bf16 operands with the LayerNorm of the finished rows fused into the epilogue (whole-row tiles:
 * N 128 / 384 / 512): C = x (fp32), ln_out = LayerNorm(x) * ln_g + ln_b as the bf16 plane (returned as float), ln_y32 the
 * same in fp32; *fused = 0 when N has no whole-row tile (then only C is written). */
int wt_dbg_gemm_bf16_ln(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias, const float* R,
                        const float* ln_g, const float* ln_b, float* C, float* ln_out, float* ln_y32, int* fused);
int wt_dbg_encoder_attention_bf16(wt_engine* h, int batch, int T, int heads, const float* qkv, int iters, float* out,
                                  float* avg_ms);
/* the decoder's kernels in the bf16 storage mode (k_decoder.hip instantiations with BF = true): weights as one bf16 plane in
 * fragment order, activations rounded to bf16 in registers, fp32 accumulation; self-attention and cross-attention on
 * bf16 caches (the host passes fp32 arrays, the taps store them as bf16 and return the updated caches widened).  Same
 * arguments as the taps without the suffix. */
int wt_dbg_dec_gemm_bf16(wt_engine* h, int mode, int B, int N, int K, const float* X, const float* W, const float* bias,
                         const float* R, float* Y, int64_t* argmax_out);
int wt_dbg_dec_ln_gemm_bf16(wt_engine* h, int B, int N, int K, const float* xin, const int64_t* ids, int pos,
                            const float* tok_emb, const float* pos_emb, int n_vocab, int n_pos, const float* ln_g,
                            const float* ln_b, const float* W, const float* bias, int gelu, float* Y, float* xout);
int wt_dbg_self_attention_bf16(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                               float* kcache, float* vcache, float* out);
/* The bf16 forms of self_attention_long, its gathered form and self_attention_prefill (option "full_bf16", DESIGN
 * section 33): the arguments and the refusals of wt_dbg_self_attention_long, wt_dbg_self_attention_long_gather and
 * wt_dbg_self_attention_prefill.  The caches go in and come back as float32 arrays holding bf16-representable values, as
 * with wt_dbg_self_attention_bf16; the appended rows are the new k and v rounded to nearest even, and they are scored
 * as rounded. */
int wt_dbg_self_attention_long_bf16(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv, float* kcache,
                                    float* vcache, float* out);
int wt_dbg_self_attention_long_gather_bf16(wt_engine* h, int rows, int heads, int cap, int pos, const float* qkv,
                                           float* kcache, float* vcache, float* out, const uint8_t* anc);
int wt_dbg_self_attention_prefill_bf16(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                       float* kcache, float* vcache, float* out);
int wt_dbg_cross_attention_bf16(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                                const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                                const float* vc, float* out);
int wt_dbg_cross_attention_records_bf16(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                                        const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                                        const float* vc, int row0, int n_rows, float* ws);
int wt_dbg_cross_combine_bf16(wt_engine* h, int M, int B, int heads, int chunks, const float* records, const float* W,
                              const float* bias, const float* R, int guard_rows, float* Y);
/* beam search (k_beam.hip).  Rows are laid out row = k * clips + c; the per-clip state is the
 * engine's: live_sum / fin_sum / fin_len [64][8], fin_tok [64][8][32], n_fin / done [64], indexed by c0 + clip, all
 * in / out.  A shape the launcher refuses is WT_ERR_INVALID_ARG. */
/* beam_topk_partial: logits [rows][ldl] -> per (row, 4096-entry chunk) the maximum m [rows][chunks], the sum of
 * exp(z - m) s [rows][chunks] and the top kk keys [rows][chunks][kk] (order bits of the logit << 32 | id; 0 = none) */
int wt_dbg_beam_topk(wt_engine* h, int rows, int V, int ldl, int kk, const float* logits, float* m, float* s,
                     uint64_t* keys);
/* one step of decode_beam: beam_topk_partial over logits [n_live * clips][V], beam_select, then beam_reorder of the
 * id rows only (ids [n_live * clips][32] -> ids_next [K * clips][32]); parent [K * clips], token [K * clips] */
int wt_dbg_beam_step(wt_engine* h, int K, int clips, int c0, int n_live, int pos, int n_prompt, int V, int64_t eot,
                     const float* logits, const int64_t* ids, float* live_sum, int32_t* fin_tok, float* fin_sum,
                     int32_t* fin_len, int32_t* n_fin, int32_t* done, int32_t* parent, int64_t* token, int64_t* ids_next);
/* beam_reorder: kv_src [slabs][src_rows][cap][d]; kv_dst [slabs * dst_rows + 1][cap][d] in / out (the last row is a
 * guard that the kernel must not write); ids_src [src_rows][32]; ids_dst [128][32] in / out; parent [dst_rows],
 * token [dst_rows] */
int wt_dbg_beam_reorder(wt_engine* h, int src_rows, int dst_rows, int cap, int d, int slabs, int pos, int V,
                        const float* kv_src, float* kv_dst, const int64_t* ids_src, int64_t* ids_dst,
                        const int32_t* parent, const int64_t* token);
/* beam_finalize over ids [K * clips][32]; out_ids [64][32], out_n / out_sum / out_len [64] in / out */
int wt_dbg_beam_finalize(wt_engine* h, int K, int clips, int c0, int pos, int n_prompt, const int64_t* ids,
                         const float* live_sum, int32_t* fin_tok, float* fin_sum, int32_t* fin_len, int32_t* n_fin,
                         const int32_t* done, int64_t* out_ids, int32_t* out_n, float* out_sum, int32_t* out_len);
/* full-length beam search (k_beam_full.hip).  Rows are laid out row = k * clips + c; step
 * t = pos + 1 - n_prompt has `clips` live rows at t = 0 and K * clips afterwards.  The per-clip state is the engine's,
 * indexed by c0 + clip, all in / out.  A shape the launchers refuse is WT_ERR_INVALID_ARG. */
typedef struct wt_dbg_beam_full_args {
  int32_t K, clips, c0, pos, n_prompt, V, ldl, stride, cap, eot, beg, max_initial, timestamps;
  int32_t begin;              /* step: run beam_full_begin first (the state arrays are then outputs only) */
  const float* logits;        /* [live rows][ldl] */
  const int64_t* ids;         /* [live rows][stride] the live hypotheses' ids, */
  const float* lp;            /* [live rows][stride] log-probabilities (index = the id's position) */
  const uint8_t* anc;         /* [live rows][cap] and ancestor tables */
  int32_t* ts_state;          /* [128][3]: tick, last_is_ts, prev_is_ts per row */
  int32_t* n_live;            /* [64] */
  double* live_sum;           /* [64][8] */
  int32_t* fin_tok;           /* [64][8][stride] */
  float* fin_lp;              /* [64][8][stride] */
  double* fin_sum;            /* [64][8] */
  int32_t *fin_len, *n_fin, *done; /* [64][8], [64], [64] */
  int32_t* parent;            /* step, out: [K * clips] */
  int64_t* token;             /* [K * clips] */
  float* tok_lp;              /* [K * clips] */
  int64_t* ids_next;          /* [K * clips][stride], in / out (cells the kernel must not write come back as sent) */
  float* lp_next;             /* [K * clips][stride] */
  uint8_t* anc_next;          /* [K * clips][cap] */
  double* lse;                /* [live rows]: logsumexp_A, NaN where A is empty; untouched for rows that are not live */
  float* part_stats;          /* optional [live rows][chunks][4]: mt, st, ms, ss of beam_full_partial */
  uint64_t* part_keys;        /* optional [live rows][chunks][2][K + 1]: its text keys, then its timestamp keys */
  int64_t* out_ids;           /* finalize, out: [64][stride] */
  float* out_lp;              /* [64][stride] */
  int32_t *out_n, *out_len;   /* [64] */
  double* out_sum;            /* [64] */
} wt_dbg_beam_full_args;
/* one step of decode_beam_full: (beam_full_begin,) beam_full_partial, beam_full_select, beam_full_advance */
int wt_dbg_beam_full_step(wt_engine* h, const wt_dbg_beam_full_args* a);
/* beam_full_finalize; ids / lp: the [K * clips] rows after the last step's advance, pos that step's */
int wt_dbg_beam_full_finalize(wt_engine* h, const wt_dbg_beam_full_args* a);
/* the tail of a greedy decoder step kernel by kernel (k_decoder.hip, select_token in k_misc.hip); bf16 != 0 selects
 * the BF = true instantiation.  fc2 as the engine runs it with fc2_ksplit = 2 (M <= 128 rows = M / B positions x B
 * clips, K % 256 == 0): Y = R + bias + X[:, :K/2] . W[:, :K/2]^T and part = X[:, K/2:] . W[:, K/2:]^T, out of place;
 * R, Y, part [M][N] in / out (R must come back unwritten) */
int wt_dbg_dec_gemm_ksplit(wt_engine* h, int bf16, int M, int B, int N, int K, const float* X, const float* W,
                           const float* bias, float* R, float* Y, float* part);
/* LayerNorm prologue + GEMM over every row source: x = xin (LNMODE 0), xin + xpart (3), or, with ids [B][ids_stride],
 * row p * B + b = tok_emb[ids[b][pos + p]] + pos_emb[pos + p] for M = positions x B rows (2).  Y [M][N] =
 * act(LayerNorm(x) . W^T + bias); xout [M + 1][K] in / out: modes 2 and 3 store x there (block 0), the last row is a
 * guard the kernel must not write.  K in {128, 384, 512}. */
int wt_dbg_dec_ln_gemm_rows(wt_engine* h, int bf16, int M, int B, int N, int K, const float* xin, const float* xpart,
                            const int64_t* ids, int ids_stride, int pos, const float* tok_emb, const float* pos_emb,
                            int n_vocab, int n_pos, const float* ln_g, const float* ln_b, const float* W, const float* bias,
                            int gelu, float* Y, float* xout);
/* the final LayerNorm of xin (xpart == NULL) or xin + xpart, logits against E [V][K] and the per-tile argmax records
 * (dec_logits_persistent with `blocks` resident blocks, 0 = the default 512); logits [M + 1][V] (may be NULL) and
 * records [M + 1][ceil(V / 32)] in / out, the last row of each a guard the kernel must not write */
int wt_dbg_dec_logits(wt_engine* h, int bf16, int M, int V, int K, const float* xin, const float* xpart, const float* ln_g,
                      const float* ln_b, const float* E, int blocks, float* logits, uint64_t* records);
/* select_token over records [B][n_tiles]; ids [B][stride], n_ids [B], finished [B] in / out */
int wt_dbg_select_token(wt_engine* h, int B, int n_tiles, const uint64_t* records, int64_t* ids, int stride, int pos,
                        int32_t* n_ids, int32_t* finished, int64_t eot, int stop_at_eot, int keep_ids);
/* language_head (k_misc.hip) over host rows x [rows][d] (+ xpart [rows][d] or NULL), the final LayerNorm's ln_g, ln_b [d]
 * and an embedding table tok_emb [n_vocab][d] (n_vocab <= 4096) whose rows lang_lo .. lang_lo + n_lang - 1 are the
 * language rows: probs [rows][n_lang], lang [rows], lang_prob [rows]; ids [rows][ids_stride] in / out (may be NULL):
 * ids[b][1] = lang_lo + lang[b].  forced_lang >= 0: lang, lang_prob and the id report that language, not the argmax. */
int wt_dbg_language_head(wt_engine* h, int rows, int d, int n_vocab, int lang_lo, int n_lang, int forced_lang, const float* x,
                         const float* xpart, const float* ln_g, const float* ln_b, const float* tok_emb, float* probs,
                         int32_t* lang, float* lang_prob, int64_t* ids, int ids_stride);
/* language_head_rows (k_misc.hip) over host rows x [x_rows][d] (+ xpart or NULL): clip b reads row
 * b * x_rows_per_clip.  allow: four words, bit r = language r (NULL: all); hold [clips] (NULL: detect every clip).
 * probs [clips][n_lang], lang / lang_prob [clips].  ids0 / ids1 [ids_rows][ids_stride] in / out (ids1 or both may be
 * NULL): column id_pos of rows b * fan .. b * fan + fan - 1 = lang_lo + lang[b].  Sizes that the host buffers cannot
 * hold are refused here, everything else by the launcher (WT_ERR_INVALID_ARG both). */
int wt_dbg_language_head_rows(wt_engine* h, int clips, int x_rows, int x_rows_per_clip, int d, int n_vocab, int lang_lo,
                              int n_lang, const float* x, const float* xpart, const float* ln_g, const float* ln_b,
                              const float* tok_emb, const uint32_t* allow, const int32_t* hold, float* probs, int32_t* lang,
                              float* lang_prob, int64_t* ids0, int64_t* ids1, int ids_rows, int ids_stride, int id_pos,
                              int fan);
/* The log-mel front end, kernel by kernel (Engine::logmel, k_misc.hip; DESIGN "front end, kernel by kernel").
 * wt_dbg_frontend_dims: {frames T0, samples per clip, pcm_stride (samples + the zero tail), pw_ld, mel_n, mel_k, dft_n,
 * dft_k} of the engine's front end. */
int wt_dbg_frontend_dims(wt_engine* h, int32_t out[8]);
/* Runs Engine::logmel (the same function the product calls, no restatement) over pcm [batch][samples] with the given
 * valid_frames (-1 = all) and returns every stage; any output but mel may be NULL:
 * mel [batch][n_mels][T0] the result; planes [batch][pcm_stride] the PCM planes as (hi + lo) / scale, hi / lo
 * [batch][pcm_stride] their raw fp16 bits; pw [batch * T0][pw_ld] the power spectrum; melacc [batch * T0][mel_n];
 * raw [batch][n_mels][T0] the log-mel before mel_normalize; words [batch][4] the clip's partial-maximum words as the
 * kernel left them (0 = never written), maxima [batch][4] the floats they stand for (-inf for 0); basis [dft_n][dft_k]
 * the fp32 windowed DFT basis and mel_matrix [mel_n][mel_k] the engine built its device tables from. */
int wt_dbg_frontend_stages(wt_engine* h, int batch, const float* pcm, int valid_frames, float* mel, float* planes,
                           uint16_t* hi, uint16_t* lo, float* pw, float* melacc, float* raw, uint32_t* words, float* maxima,
                           float* basis, float* mel_matrix);
/* log_clipmax alone: melacc [B * T][ld] -> raw [B][n_mel][T] and the partial maxima over frames < t_valid (< 0: T) as
 * words / maxima [B][4] (either may be NULL), the words cleared first as the engine clears them.  Needs n_mel <= ld. */
int wt_dbg_log_clipmax(wt_engine* h, int B, int T, int n_mel, int ld, int t_valid, const float* melacc, float* raw,
                       uint32_t* words, float* maxima);
/* mel_normalize alone: logmel [B][n_mel][T] in / out against the partial-maximum words [B][4] */
int wt_dbg_mel_normalize(wt_engine* h, int B, int T, int n_mel, const uint32_t* words, float* logmel);
/* the hand-over of the log-mel to the encoder: mel [B][C][T] -> out [B][T + 2][ld], in / out (rows 0 and T + 1 and the
 * columns >= C belong to the caller and must come back as given).  planes 0: mel_transpose, out is fp32 and ld must be
 * C; 1: mel_transpose_planes<false>, out is the fp16 hi buffer followed by the lo buffer, values times scale; 2:
 * mel_transpose_planes<true>, out is one bf16 buffer (scale unused). */
int wt_dbg_mel_transpose(wt_engine* h, int planes, int B, int C, int T, int ld, float scale, const float* mel, void* out);
/* pcm_to_planes alone: pcm [batch][n] -> planes, in / out: hi [batch * out_stride + guard] then lo (same size) as fp16
 * bits; clip b is written at b * out_stride, everything else belongs to the caller.  n % 4 == 0, out_stride % 8 == 0,
 * out_stride >= n, (batch * out_stride + guard) % 4 == 0. */
int wt_dbg_pcm_to_planes(wt_engine* h, int batch, int n, int out_stride, int guard, float scale, float limit, const float* pcm,
                         uint16_t* planes);
/* The encoder GEMMs under the operand and output addressing Engine::encode_enqueue / encode_enqueue_bf16 give them
 * (conv1 over overlapping rows into a padded buffer, conv2 with stride 2, the q|k|v planes, the cross-KV scatter).  The
 * tap fills the launcher's argument struct from its parameters and calls the launcher; it restates no addressing.
 * kind 0: launch_gemm with the engine's gemm_variant option; 1: launch_gemm_planes; 2: launch_gemm_bf16_planes.
 * A [a_len] is ONE flat fp32 buffer, converted elementwise for the kind (1: two fp16 planes at one power-of-two scale from
 * the buffer's maximum, 2: one bf16 plane) and uploaded with 64 zero elements behind it; row m of the operand starts at
 * (m / a_rpb) * a_bs + (m % a_rpb) * lda and is K long.  W [N][K], bias [N], pos [pos_period][N] (kEpiPos) are laid out
 * per kind as wt_dbg_gemm / wt_dbg_gemm_planes / wt_dbg_gemm_bf16 do.
 * out is a flat buffer of c_len elements, in / out: uploaded as given, written by the kernel at base + c_off with c_rpb,
 * c_bs, ldc (kEpiKvLayout: the cache [N / kv_dmodel][kv_batch][kv_heads][c_rpb][64] at base + c_off), downloaded whole,
 * so that every cell the launch does not address comes back as given.  out_format 0: float [c_len] (kEpiResidual: R
 * is the output itself, in place); 1 (kind 1): fp16 bits [2][c_len], hi then lo, column n times out_scale[n / seg]
 * (seg = 0: one segment); 2 (kind 2): bf16 bits [c_len].
 * WT_ERR_INVALID_ARG before anything is launched: an a_len shorter than the last addressed row's end, an output the
 * buffer does not hold, an offset or (kind 0) a stride the 16-byte accesses cannot take, and whatever the launcher
 * itself refuses (c_rpb < 32, pos_period < 32 with kEpiPos, strides that are no multiple of 8 for kinds 1 and 2,
 * seg % 8 or more than three segments, kEpiKvLayout as fp32 from kind 2, an epilogue it has no kernel for). */
int wt_dbg_gemm_addressed(wt_engine* h, int kind, int epi, int M, int N, int K, const float* A, long a_len, int a_rpb,
                          long a_bs, int lda, const float* W, const float* bias, const float* pos, int pos_period,
                          int out_format, void* out, long c_len, long c_off, int c_rpb, long c_bs, int ldc,
                          const float* out_scale, int seg, int kv_batch, int kv_heads, int kv_dmodel, int n_cu);
/* What the encoder GEMM launchers WILL launch for a shape (plane_gemm_plan / bf16_gemm_plan in csrc/kernels.h, the
 * functions the launchers themselves launch from); no GPU work, no engine.  ln != 0: the LayerNorm outputs are set.
 * family 0 (launch_gemm_planes, under the current wt_dbg_set_plane_gemm_mode): plan = {tile (0 = 192 x 128, 1 = 192 x 384,
 * 2 = 256 x 384), schedule (0 = gemm_planes_tile, in step; 1 = gemm_planes_pp; 2 = gemm_planes_pp16; 3 =
 * gemm_planes_pp16_persist), LayerNorm fused (0 / 1), the mode}; c_rpb and ldc are not read.
 * family 1 (launch_gemm_bf16_planes; planes_out = bf16 output): plan = {tile columns, tile rows, whole-row tile with the
 * LayerNorm fused (0 / 1), 0}; K and n_cu are not read. */
int wt_dbg_plane_gemm_plan(int family, int M, int N, int K, int epi, int planes_out, int ln, int n_cu, int c_rpb, int ldc,
                           int32_t plan[4]);
/* An encoder GEMM with the LayerNorm of its finished rows fused into the epilogue, as Engine's fuse_ln launches it, with
 * guard rows behind every output.  family 0: launch_gemm_planes (K % 32 == 0), 1: launch_gemm_bf16_planes (K % 64 == 0);
 * epi 5 (bias | residual, R = C in place) or 11 (bias | gelu | pos).  A [a_len], a_rpb, a_bs, lda, W, bias, pos as in
 * wt_dbg_gemm_addressed.  Every output has M + guard_rows rows of N (guard_rows >= 256, one whole tile), in / out:
 * uploaded as given, downloaded whole.  C: fp32, written under c_rpb, c_bs, ldc (the fusion needs c_rpb >= M and ldc == N);
 * planes: the LayerNorm planes, fp16 bits [2][(M + guard_rows) * N] (hi, then lo, of y * ln_scale) or, family 1, bf16 bits
 * [(M + guard_rows) * N]; ln_y32 (may be NULL: the kernel writes no fp32 copy); p_out (usually NULL): a plane OUTPUT of
 * the GEMM itself, laid out like `planes`, which the fusion excludes.  ln_g, ln_b (may be NULL) and ln_scale go to the
 * launcher as they are.  *flag: the non-finite word, cleared first; *fused: what the launcher returned.
 * WT_ERR_INVALID_ARG before anything is launched: operands or outputs the buffers do not hold, and whatever the launcher
 * refuses (family 0: the LayerNorm outputs without gain or shift, ln_scale <= 0, ldc != N, c_rpb < M, p_out). */
int wt_dbg_gemm_ln_fused(wt_engine* h, int family, int epi, int M, int N, int K, const float* A, long a_len, int a_rpb, long a_bs,
                         int lda, const float* W, const float* bias, const float* pos, int pos_period, const float* ln_g,
                         const float* ln_b, float ln_scale, int n_cu, int guard_rows, int c_rpb, long c_bs, int ldc, float* C,
                         uint16_t* planes, float* ln_y32, uint16_t* p_out, int32_t* flag, int32_t* fused);
/* launch_layernorm_planes: x [M][d], g, b [d] -> planes in / out: fp16 bits [2][M * d + guard] (hi, then lo; y * scale)
 * or, bf16 != 0, bf16 bits [M * d + guard]; y32 [M * d + guard] in / out (may be NULL: the kernel writes no fp32 copy);
 * *nonfinite (may be NULL: no flag is passed) is cleared first and comes back 1 when a row's mean or variance was not
 * finite.  The guard elements belong to the caller; guard % 4 == 0.  A d the launcher has no kernel for is its
 * WT_ERR_FORMAT. */
int wt_dbg_layernorm_planes(wt_engine* h, int M, int d, const float* x, const float* g, const float* b, float scale, int bf16,
                            int guard, uint16_t* planes, float* y32, int32_t* nonfinite);
/* launch_f32_to_planes: x [M][ld] -> planes in / out, fp16 bits [2][M * ld + guard] of x * scales[n / seg] (seg = 0: one
 * segment, scales[0]); scales always holds three values.  guard % 4 == 0. */
int wt_dbg_f32_to_planes(wt_engine* h, int M, int ld, const float* x, const float* scales, int seg, int guard,
                         uint16_t* planes);
/* What Engine::upload_weights derived for the fp16-plane encoder, one record of 10 floats per contraction in the order
 * of the force_fallback bits: conv1, conv2, then per layer qkv, attention, out, fc1, fc2, then cross-KV.  Read-only, no
 * GPU work.  A GEMM record is {a_scale, w_scale, f16_ok, largest bound of the A operand, its typical magnitude, 0 ...};
 * an attention record is {q, k, v scales, attn_f16_ok, then largest bound and typical magnitude of q (both times
 * d_head^-1/2 log2 e, as the kernel splits it), of k and of v}.  The verdicts are the load-time ones, whatever
 * force_fallback is set to.  *n = the number of records; the first min(*n, cap) are written to rec [cap][10]. */
int wt_dbg_encoder_scales(wt_engine* h, float* rec, int cap, int* n);
/* f16_scale_for (csrc/kernels.h) itself: no engine, no GPU work. */
float wt_dbg_f16_scale_for(float bound);
/* launch_gemm_planes on dense operands with every scale GIVEN, where the other plane GEMM taps take the tightest scale
 * from the data: A [M][K], W [N][K], bias [N]; a_scale, w_scale, out_scale[3], seg, n_cu go to the launcher as they are.
 * A is split on the host as the producers split it, hi = fp16(x * a_scale), lo = fp16(x * a_scale - hi), with no clamping:
 * an element beyond fp16's range uploads as hi = inf, lo = -inf.  W goes through split_weight_planes at w_scale.
 * epi 1 (bias), 3 (bias | gelu) or, fp32 output only, 5 (bias | residual: the residual is `out` itself, in place).
 * out has M + guard_rows rows of N, in / out, uploaded as given and downloaded whole: float (planes_out = 0) or fp16 bits
 * [2][(M + guard_rows) * N], hi then lo, of column n times out_scale[n / seg] (seg = 0: one segment).  The tap fills the
 * launcher's arguments and calls it; it restates no addressing.  WT_ERR_INVALID_ARG before anything is launched: a null
 * pointer, another epilogue, N % 128, K % 32, and whatever the launcher refuses (a scale that is not positive, seg % 8 or
 * more than three segments). */
int wt_dbg_gemm_planes_scaled(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias, int epi,
                              float a_scale, float w_scale, const float out_scale[3], int seg, int n_cu, int planes_out,
                              int guard_rows, void* out);
/* The encoder attention launchers at a given shape, with given operand scales and with rows that belong to no clip
 * behind the last one.  The tap fills the launcher's arguments and calls the launcher; it restates no addressing.
 * kind 0: launch_encoder_attention with `variant` 0 (encoder_attention_f32) or 1 (encoder_attention_split<4, 3>), given
 * here and not through the attn_variant option; 1: launch_encoder_attention_planes; 2: launch_encoder_attention_bf16.
 * qkv [batch * T + guard_rows][3 * 64 * heads] fp32, uploaded whole: as it is (kind 0), multiplied by d_head^-1/2 log2(e)
 * scales[0] | scales[1] | scales[2] and split into two fp16 planes as wt_dbg_encoder_attention_planes does (kind 1), or
 * rounded to bf16 (kind 2).  scales = {q, k, v, out}, powers of two, read by kind 1 only (may be NULL otherwise).
 * out [batch * T + guard_rows][64 * heads] is in / out, uploaded as given and downloaded whole, so that every cell the
 * launch does not write comes back as given: float (kind 0), fp16 bits [2][rows * 64 * heads], hi then lo, of the
 * result times scales[3] (kind 1), bf16 bits (kind 2).
 * WT_ERR_INVALID_ARG before anything is launched: a null pointer, guard_rows < 0, a negative count, a scale that is no
 * power of two, a kind or variant the launchers do not have, and whatever the launcher refuses (batch, T or heads below
 * 1); out is then not written. */
int wt_dbg_encoder_attention_at(wt_engine* h, int kind, int variant, int batch, int T, int heads, int guard_rows,
                                const float* qkv, const float scales[4], void* out);
/* launch_align_scores (word-level timestamps): the attention weights of n_heads heads of one layer
 * for the np positions of one decoder pass.  qp [np * batch][H * 64 H] absorbed queries (row = p * batch + b), E [batch][T]
 * [64 H] the encoder output, split into fp16 planes on the host as wt_dbg_cross_absorbed does; head [n_heads] the heads'
 * indices in the layer, slot [n_heads] their places in W's head axis, F [batch] the clips' valid frames.
 * W [batch][heads_total][L_max][ld] is in / out, uploaded as given and downloaded whole: the kernel writes the frames
 * < T of the rows pos0 .. pos0 + np - 1 of the listed slots (softmax over t < F[b], zero behind) and nothing else.
 * The tap fills the launcher's arguments and calls the launcher.  WT_ERR_INVALID_ARG before anything is launched: a null
 * pointer, batch > 64, n_heads > 8, and whatever the launcher refuses: no heads, a head >= H or a slot >= heads_total,
 * an F[b] outside [1, T], np * batch > 128, pos0 + np > L_max, T % 4 != 0 or T > 1500, ld < T or ld % 4 != 0, an H
 * other than 2, 6 or 8, a head or a slot listed twice, a mode other than 0 (one wavefront sweeps all frames of its
 * columns, softmax in the same kernel) or 1 (blocks per 128 frames, then align_softmax_rows). */
int wt_dbg_align_scores(wt_engine* h, int batch, int H, int T, int np, int pos0, const float* qp, const float* E, int n_heads,
                        const int32_t* head, const int32_t* slot, int heads_total, const int32_t* F, int L_max, int ld, float* W,
                        int mode);
/* The bf16 form (option full_bf16_all): E is rounded to ONE bf16 plane on the host (to nearest even) and
 * q' to bf16 in the kernel, one bf16 MFMA per 32 columns and no operand scale.  Arguments and refusals are those above. */
int wt_dbg_align_scores_bf16(wt_engine* h, int batch, int H, int T, int np, int pos0, const float* qp, const float* E, int n_heads,
                             const int32_t* head, const int32_t* slot, int heads_total, const int32_t* F, int L_max, int ld,
                             float* W, int mode);
/* launch_f32_to_bf16 (k_misc.hip): x [n] -> ONE bf16 plane, rounded to nearest even.  out [n + guard] is in / out as
 * float32 holding bf16-representable values: uploaded as given, the first n cells written, the guard cells untouched.
 * n < 4 or n % 4 != 0 is WT_ERR_INVALID_ARG (the launcher's refusal), before anything is launched. */
int wt_dbg_f32_to_bf16(wt_engine* h, int n, int guard, const float* x, float* out);
/* launch_align_matrix (word-level timestamps): W [clips][heads][L_max][ld] attention weights ->
 * C [clips][N_max][ld] in / out and stats [clips][heads][2][ld] in / out (mean, then 1 / std; may be NULL), both
 * uploaded as given and downloaded whole, so that every cell the kernels do not write comes back as given.  L [clips] is
 * the clips' fed positions, F [clips] their valid frames; cost row r of a clip is W's row n_a + r and a clip has
 * L[b] - n_a - 1 of them.  The tap fills the launcher's arguments and calls the launcher; it restates no addressing.
 * WT_ERR_INVALID_ARG before anything is launched: a null pointer, an L[b] outside [n_a + 2, L_max], an F[b] outside
 * [1, ld], an N_max below a clip's row count, and whatever the launcher refuses (heads > 128, N_max > 447, ld > 1500). */
int wt_dbg_align_matrix(wt_engine* h, int clips, int heads, int L_max, int ld, int n_a, int N_max, const float* W,
                        const int32_t* L, const int32_t* F, float* C, float* stats);
/* launch_align_dtw: C [clips][N_max][ld], N [clips] rows and F [clips] frames of each clip -> jump [clips][N_max] in / out
 * (the kernel writes a clip's whole row: first frames, then zeros) and, when not NULL, trace [clips][N_max][ld] in / out,
 * the trace codes of the cells.  WT_ERR_INVALID_ARG before anything is launched: a null pointer, an N[b] outside
 * [0, N_max], an F[b] outside [1, ld], and what the launcher refuses (N_max > 447, ld > 1500). */
int wt_dbg_align_dtw(wt_engine* h, int clips, int N_max, int ld, const float* C, const int32_t* N, const int32_t* F,
                     int32_t* jump, uint8_t* trace);
/* launch_suppress_logits (k_suppress.hip, wt_engine_set_suppress): logits [rows][ldl] -> out
 * [rows][ldl], the padding columns V .. ldl - 1 included, with -inf at every id of ids [n] and, when first != 0, of
 * first_ids [n_first]; the two lists are uploaded as the engine keeps them, one buffer, the always-ids first.  The ids are
 * data to the kernel: one outside [0, V) changes nothing.  WT_ERR_INVALID_ARG before anything is launched: a null
 * pointer, and what the launcher refuses (rows outside 1..128, V < 1, ldl < V, a count outside 0..1024). */
int wt_dbg_suppress_logits(wt_engine* h, int rows, int V, int ldl, const float* logits, float* out, const int64_t* ids, int n,
                           const int64_t* first_ids, int n_first, int first);
/* Measurement and test handles of the alignment pass (word_timestamps): keep = 1 keeps what the pass forms per clip for
 * wt_dbg_last_alignment (it then synchronises and copies per clip); mode = the form of align_scores, 0 or 1 (default 1);
 * sub = the most clips per sub-group of the pass, 0 = as many as the weight workspace's bound allows (default).  A
 * negative argument leaves that setting as it is.  WT_ERR_INVALID_ARG for a value outside these. */
int wt_dbg_set_alignment(wt_engine* h, int keep, int mode, int sub);
/* What the alignment pass of the last decode with word_timestamps = 1, behind wt_dbg_set_alignment(h, 1, ..), formed for clip
 * `clip`: dims = {n_a, L, N, F, heads, T} (prompt ids, ids fed, cost rows, valid frames, alignment heads, n_audio_ctx);
 * row [L] the ids fed, W [heads][L][T] the attention weights, C [N][T] the cost (frames >= F are not the engine's),
 * jump [N] the first frame of every cost row.  After a seeking wt_transcribe_long_pcm `clip` is the window; a window
 * without words has L = 0.  Every output pointer may be NULL.  WT_ERR_INVALID_ARG when that decode kept nothing or has no
 * such clip. */
int wt_dbg_last_alignment(const wt_engine* h, int clip, int32_t dims[6], int64_t* row, float* W, float* C, int32_t* jump);
#ifdef __cplusplus
}
#endif
#endif
