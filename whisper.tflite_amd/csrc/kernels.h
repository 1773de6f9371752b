// Host-side launchers for the gfx950 kernels of the EncDec hot path.
// Every launcher enqueues on the given stream and never synchronises or
// allocates, so a caller may capture a sequence of them into a hipGraph.
// A shape outside a kernel's contract throws wt::Error (never abort()).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>
#include <vector>

#include "error.h"

namespace wt {

// Kernel-exact timing for the roofline figures (bench.py): while `start` is set, the launchers of the encoder's
// contraction kernels attach the two events to the dispatch itself (hipExtLaunchKernelGGL), so their difference is the
// kernel's own begin -> end interval, the figure rocprofv3 --kernel-trace reports.  An event pair recorded around the
// launch on the stream also counts the wait for CUs that decoder chains hold and the barrier packets of the events.
struct LaunchTimer {
  hipEvent_t start = nullptr, stop = nullptr;
};
extern thread_local LaunchTimer g_launch_timer;

#define WT_LAUNCH_TIMED(kernel, grid, block, smem, stream, ...)                                                      \
  do {                                                                                                                \
    if (::wt::g_launch_timer.start) {                                                                                 \
      hipExtLaunchKernelGGL(kernel, grid, block, smem, stream, ::wt::g_launch_timer.start, ::wt::g_launch_timer.stop, \
                            0, __VA_ARGS__);                                                                          \
    } else {                                                                                                          \
      hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);                                             \
    }                                                                                                                 \
  } while (0)

// ------------------------------------------------------------------ GEMM ---
// C = epilogue(A . W^T): A [M][K] activations (row m at
// A + (m / a_rpb) * a_bs + (m % a_rpb) * lda), W [N][K] row-major (torch Linear
// layout), fp32 in, fp32 out.  The contraction runs on the matrix cores in one of three forms selected
// by `variant` (k_gemm.hip): fp32 MFMA (v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain), or fp32
// operands split into three bf16 / two fp16 planes with fp32 accumulation (fp32-level error,
// bf16_split.h).  Requires N % 128 == 0 and K % 32 == 0; M is arbitrary.
enum GemmEpi : int {
  kEpiBias = 1,      // + bias[n]
  kEpiGelu = 2,      // exact erf GELU
  kEpiResidual = 4,  // + R[row m][n]  (R addressed like C; R may alias C)
  kEpiPos = 8,       // + pos[(m % pos_period)][n]   (encoder positional embedding)
  kEpiKvLayout = 16,  // scatter into the cross-attention KV cache layout (see below)
  // plane GEMM only: columns (2 k, 2 k + 1) hold the real and imaginary part of bin k; the output is |.|^2 per pair,
  // fp32 [M][N / 2] (row stride ldc): the front end's STFT-as-GEMM writes the power spectrum directly
  kEpiPower = 32
};

struct GemmArgs {
  const float* A = nullptr;
  const float* W = nullptr;
  float* C = nullptr;
  const float* bias = nullptr;
  const float* R = nullptr;
  const float* pos = nullptr;
  int M = 0, N = 0, K = 0;
  int a_rpb = 1 << 30;  // rows per batch item for A addressing
  long a_bs = 0;        // element stride between batch items of A
  int lda = 0;
  int c_rpb = 1 << 30;
  long c_bs = 0;
  int ldc = 0;
  int pos_period = 1;
  // kEpiKvLayout: column n = (slab * d_model + head * 64 + dd), row m = (b * T + t)
  //   -> C[((slab * kv_batch + b) * kv_heads + head) * T * 64 + t * 64 + dd]
  // where slab enumerates (layer, k|v); T = c_rpb.
  int kv_batch = 0, kv_heads = 0, kv_dmodel = 0;
  int variant = -1;  // contraction form (k_gemm.hip launch_gemm_t: 0, 11, 13, 16, 17, 18); -1 = auto
  // two-plane fp16 kernels (variants 17, 18): powers of two that bring the operands into fp16's normal
  // range, |A * a_scale| and |W * w_scale| <= 32768 (f16_scale_for); the epilogue divides them out
  float a_scale = 1.0f, w_scale = 64.0f;
};
void launch_gemm(const GemmArgs& a, int epi, hipStream_t s);
// largest power of two s with bound * s <= 16384 (a factor 4 below fp16's maximum), clamped to 2^+-24
float f16_scale_for(float bound);
// resident blocks per CU the runtime reports for a tile variant (diagnostics)
int gemm_occupancy(int variant);
// variants launch_gemm accepts: 0 fp32 MFMA, 11 bf16 operands, 13/16 three bf16 planes, 17/18 two fp16 planes
bool gemm_variant_supported(int variant);

// ------------------------------------------------------- GEMM on fp16 planes ---
// The default encoder GEMM (k_gemm_planes.hip): both operands are pairs of fp16 planes (hi = fp16(x * scale), lo =
// fp16(x * scale - hi); 4 bytes per element like fp32).  A planes: hi at A, lo at A + a_plane (element offsets, same
// row addressing as GemmArgs); W: both planes in the blocked layout of split_weight_planes().  Output: fp32 C
// (epilogues kEpiBias, | kEpiResidual, | kEpiGelu | kEpiPos, | kEpiKvLayout) or, when P != nullptr, planes of the
// result for the next contraction (kEpiBias, | kEpiGelu): column n multiplied by out_scale[n / seg] before the split.
// Requires N % 128 == 0, K % 32 == 0, lda / a_bs / ldc / c_bs multiples of 8 elements.
struct PlaneGemmArgs {
  const unsigned short* A = nullptr;
  long a_plane = 0;
  const unsigned short* W = nullptr;
  float* C = nullptr;
  unsigned short* P = nullptr;
  long p_plane = 0;
  const float* bias = nullptr;
  const float* R = nullptr;
  const float* pos = nullptr;
  int M = 0, N = 0, K = 0;
  int a_rpb = 1 << 30;
  long a_bs = 0;
  int lda = 0;
  int c_rpb = 1 << 30;
  long c_bs = 0;
  int ldc = 0;
  int pos_period = 1;
  int kv_batch = 0, kv_heads = 0, kv_dmodel = 0;
  float a_scale = 1.0f, w_scale = 1.0f;  // the powers of two baked into the A and W planes
  float out_scale[3] = {1.0f, 1.0f, 1.0f};
  int seg = 0;  // columns per out_scale segment (0 = one segment)
  int n_cu = 256;  // CUs the launching stream may use (tile choice, k_gemm_planes.hip)
  // LayerNorm fusion (fp32 output C with kEpiBias | kEpiResidual or kEpiBias | kEpiGelu | kEpiPos, N = 384, contiguous
  // [M][N] rows): the block that finishes a 384-column row also writes LayerNorm(row) * ln_g + ln_b, times ln_scale,
  // as planes (hi at ln_P, lo at ln_P + ln_plane) — the A operand of the next GEMM — and optionally as fp32 (ln_y32)
  // with the non-finite flag of launch_layernorm.  Only the 384-column tiles can do it: launch_gemm_planes returns
  // whether it did (false: the caller launches the LayerNorm kernel).
  const float *ln_g = nullptr, *ln_b = nullptr;
  unsigned short* ln_P = nullptr;
  long ln_plane = 0;
  float ln_scale = 1.0f;
  float* ln_y32 = nullptr;
  int* nonfinite = nullptr;
};
bool launch_gemm_planes(const PlaneGemmArgs& a, int epi, hipStream_t s);
// schedule of the 384-column plane tiles (0 in step, 1 ping-pong groups, 2 ping-pong groups on 16 x 16 x 32 MFMAs and
// persistent where a CU runs several plane-output tiles, 4 the same with one tile per block everywhere;
// k_gemm_planes.hip) — measurement knob
int plane_gemm_mode();
void set_plane_gemm_mode(int m);
// What launch_gemm_planes launches for a shape, and the only place that decides it (the launcher launches from this):
// tile 0 = 192 x 128, 1 = 192 x 384, 2 = 256 x 384; schedule 0 = gemm_planes_tile (in step), 1 = gemm_planes_pp,
// 2 = gemm_planes_pp16, 3 = gemm_planes_pp16_persist; fused = the LayerNorm is done in the epilogue.  `ln` = ln_P set,
// `mode` = plane_gemm_mode().  No GPU work; the measurement knob WT_PLANE_TILE is read here (once per process).
struct PlaneGemmPlan {
  int tile = 0, schedule = 0;
  bool fused = false;
};
PlaneGemmPlan plane_gemm_plan(int M, int N, int K, int epi, bool planes_out, bool ln, int n_cu, int mode);
// bf16 storage mode (k_gemm_bf16.hip): A, W single bf16 matrices (the plane offsets and scales of the struct are
// unused), K a multiple of 64; P set = bf16 output (row-major, or the cross-KV cache layout with kEpiKvLayout),
// else fp32 output C
// returns true when the LayerNorm fusion (a.ln_g ...: as in launch_gemm_planes, ONE bf16 plane at ln_P, ln_scale unused) was done
bool launch_gemm_bf16_planes(const PlaneGemmArgs& a, int epi, hipStream_t s);
// What launch_gemm_bf16_planes launches (it launches from this): block tile bm x bn; whole_row = the tile whose columns
// are the whole row, with the LayerNorm fused into its epilogue.  `ln` = ln_g, ln_b and ln_P all set.  WT_BF16_TILE and
// WT_BF16_LN_FUSE are read here (once per process).
struct Bf16GemmPlan {
  int bm = 192, bn = 128;
  bool whole_row = false;
};
Bf16GemmPlan bf16_gemm_plan(int M, int N, int epi, bool bf16_out, bool ln, int c_rpb, int ldc);
// W [N][K] fp32 -> bf16 [N][Kpad] (round to nearest even, zero filled)
std::vector<unsigned short> round_weights_bf16(const float* W, int N, int K, int Kpad);
// W [N][K] fp32 -> both fp16 planes, scaled by `scale`, as [N / 16][Kpad / 32][hi | lo][16 rows][32 k] with swizzled
// 16-byte chunks: the LDS image of the plane GEMM's staging instructions, 1 KiB contiguous each (Kpad >= K, zero filled)
std::vector<unsigned short> split_weight_planes(const float* W, int N, int K, int Kpad, float scale);

// Decoder-step GEMM: out[M][N] = epi(pro(x)[M][K] . W[N][K]^T), M = positions x B clips <= 128 rows (row =
// p * B + b), k_decoder.hip.  Wt is W as two fp16 planes in MFMA-fragment order, made by tile_weights_f16():
// [ceil(N/32)][K/16][plane hi|lo][64 lanes][8], scaled by w_scale.
enum DecPro : int {
  kProNone = 0,    // A operand = X [M][K] (ldx) from global memory
  kProLn = 1,      // A = LayerNorm(x) * ln_g + ln_b with x = xin, or (ids != nullptr) the token +
                   // positional embedding, which block 0 also stores to xout
  kProCombine = 2  // A = combine of the cross-attention key-chunk partials cross_ws
};
enum DecEpi : int {
  kDecResid = 0,     // Y = R + bias + acc   (R may alias Y: the residual stream, in place)
  kDecBias = 1,      // Y = acc + bias
  kDecBiasGelu = 2,  // Y = gelu(acc + bias)
  kDecLogits = 3     // (optional Y = acc) + per-tile argmax records best[m][tile], reference tie rule
};
struct DecGemmArgs {
  int logits_blocks = 0;  // resident blocks of the persistent logits kernel (0 = 512, two per CU; the pipeline asks for 256)
  const unsigned short* Wt = nullptr;
  float w_scale = 1.0f;  // power of two the planes were scaled by (tile_weights_f16)
  int N = 0, K = 0, B = 0;
  int M = 0;  // rows; 0 = B (one position)
  const float* X = nullptr;
  int ldx = 0;
  const float* xin = nullptr;
  float* xout = nullptr;
  const float* ln_g = nullptr;
  const float* ln_b = nullptr;
  const long long* ids = nullptr;  // kProLn embedding rows: row p * B + b = tok_emb[ids[b][pos + p]] + pos_emb[pos + p]
  int ids_stride = 0, pos = 0;
  const float* tok_emb = nullptr;
  const float* pos_emb = nullptr;  // the whole table [n_text_ctx][K]
  int n_vocab = 0;
  // ragged chain (optional, device [B]): `pos` counts slots, clip b's positional row is pos + p - pos_start[b] clamped
  // into [0, n_ctx); null = the rows above
  const int* pos_start = nullptr;
  int n_ctx = 0;  // rows of pos_emb (needed with pos_start)
  const float* cross_ws = nullptr;
  int heads = 0, chunks = 0;
  const float* bias = nullptr;
  const float* R = nullptr;
  float* Y = nullptr;
  int ldy = 0;
  unsigned long long* best = nullptr;
  int best_stride = 0;  // records per row; 0 = ceil(N / 32)
  // kProNone + kDecResid with ksplit = 2: twice the blocks, each over half of K (a K = 1536 GEMM on 12 column
  // tiles is bound by what one CU can stream).  Blocks of the first half write Y = R + bias + partial, blocks
  // of the second half write their raw partial to `part` [M][ldy]; the consumer adds the two (xpart below).
  int ksplit = 1;
  float* part = nullptr;
  // kProLn: rows = xin + xpart (the pending second half of the previous residual GEMM); block 0 stores the
  // completed rows to xout
  const float* xpart = nullptr;
  // bf16 storage mode: Wt is ONE bf16 plane in fragment order (tile_weights_bf16), w_scale unused
  bool bf16 = false;
};
void launch_dec_gemm(const DecGemmArgs& a, int pro, int epi, hipStream_t s);
// y = LayerNorm(x) * g + b : input rows of the logits GEMM
void launch_dec_finalize_ln(const float* xin, const float* g, const float* b, float* y, int B, int K,
                            hipStream_t s, const float* xpart = nullptr);

// ------------------------------------------------------------- LayerNorm ---
// y[m][:] = (x[m][:] - mean) * rstd * g + b, eps 1e-5, one wavefront per row.
void launch_layernorm(const float* x, float* y, const float* g, const float* b, int M, int d,
                      hipStream_t s, int* nonfinite = nullptr);
// Same rows, written as two fp16 planes of y * scale (hi at yp, lo at yp + plane) for the plane GEMM, and
// optionally (y32 != nullptr) also as fp32.
void launch_layernorm_planes(const float* x, unsigned short* yp, long plane, float scale, float* y32, const float* g,
                             const float* b, int M, int d, hipStream_t s, int* nonfinite = nullptr, bool bf16 = false);

// fp32 rows [M][ld] (contiguous) -> planes of x * scales[n / seg] (seg = 0: one segment), hi at yp, lo at yp + plane:
// the operand hand-over between a contraction on the fp32-storage fall-back kernels and one on the plane kernels
void launch_f32_to_planes(const float* x, unsigned short* yp, long plane, long M, int ld, const float* scales, int seg,
                          hipStream_t s);
// fp32 [n] -> ONE bf16 plane [n], round to nearest even (n % 4 == 0; 8-byte packed stores): what the bf16 form of
// align_scores reads when the decode ran the cached cross-attention form
void launch_f32_to_bf16(const float* x, unsigned short* y, long n, hipStream_t s);
// probe kernel of Engine::create_streams: one wavefront busy for `microseconds` (k_misc.hip)
void launch_spin(int microseconds, hipStream_t s);
// PCM [batch][n] fp32 -> fp16 planes of clamp(x, -limit, limit) * scale, [batch][out_stride] (columns >= n untouched:
// the caller zeroes them once — the reference's zero fill past the last sample, whisper.cpp:149-153): hi at yp, lo at
// yp + plane.  n % 4 == 0, out_stride % 8 == 0.
void launch_pcm_to_planes(const float* pcm, unsigned short* yp, long plane, float scale, float limit, int batch, long n,
                          long out_stride, hipStream_t s);

// ------------------------------------------------------ encoder attention ---
// qkv [B*T][3*d] (q | k | v, heads of 64 inside each third) -> out [B*T][d].
// Non-causal softmax(q k^T / 8) v per (clip, head), flash-style, on fp32 storage: the forms a layer falls back to
// when its operands leave the plane kernel's range.  `variant`: 0 = encoder_attention_f32 (fp32 MFMA), 1 =
// encoder_attention_split<4, 3> (three bf16 planes, six products, 128 queries per block); any other variant and
// batch, T or heads below 1 are kErrInvalidArg, before anything is launched.  q_scale, k_scale and v_scale are
// unused: both forms take the operands at their own magnitude.
void launch_encoder_attention(const float* qkv, float* out, int batch, int T, int heads, int variant,
                              hipStream_t stream, float q_scale = 1.0f, float k_scale = 1.0f, float v_scale = 1.0f);
// The same attention on pre-split operands (k_attention_planes.hip): qkv as fp16 planes [B*T][3d] (hi at qkv, lo at
// qkv + plane), q already multiplied by d_head^-1/2 * log2(e) * q_scale, k by k_scale, v by v_scale (the plane GEMM's
// out_scale); output planes of the attention result * out_scale, [B*T][d], hi at out, lo at out + out_plane.
void launch_encoder_attention_planes(const unsigned short* qkv, long plane, unsigned short* out, long out_plane,
                                     int batch, int T, int heads, float q_scale, float k_scale, float v_scale,
                                     float out_scale, hipStream_t stream);
// bf16 storage mode: qkv and out are single bf16 matrices; q arrives unscaled
void launch_encoder_attention_bf16(const unsigned short* qkv, unsigned short* out, int batch, int T, int heads,
                                   hipStream_t stream);

// ------------------------------------------------------------- front end ---
// one dependent link of a launch-latency chain (test tap): blocks x 64 threads, p[block] += 1
void launch_chain_probe(float* p, int blocks, hipStream_t stream);
// mel [B][n_mels][T] -> melT [B][T + 2][n_mels] rows 1..T (rows 0 and T+1 stay zero).
void launch_mel_transpose(const float* mel, float* melT, int batch, int n_mels, int T,
                          hipStream_t s);
// mel [B][n_mels][T] -> fp16 planes of melT * scale, [B][T + 2][ld] rows 1..T, columns [0, n_mels) (the rest and
// rows 0, T + 1 stay zero): hi at out, lo at out + plane
void launch_mel_transpose_planes(const float* mel, unsigned short* out, long plane, float scale, int batch, int n_mels,
                                 int T, int ld, hipStream_t s, bool bf16 = false);
// melacc [B*T][ld] (first n_mel columns) -> logmel [B][n_mel][T] = log10(max(x,1e-10)),
// and per-clip maximum over frames [0, t_valid) (t_valid < 0: all T) into clip_max[(b * kClipMaxWays + w) * kClipMaxStride], w < kClipMaxWays (ordered-uint
// encoding, pre-zeroed).
constexpr int kClipMaxStride = 32, kClipMaxWays = 4;  // a clip's maximum: kClipMaxWays partial maxima, one 128-byte line each
void launch_log_clipmax(const float* melacc, int ld, float* logmel, unsigned* clip_max, int batch,
                        int n_mel, int T, hipStream_t s, int t_valid = -1);
// in place: x = (max(x, clipmax[b] - 8) + 4) / 4
void launch_mel_normalize(float* logmel, const unsigned* clip_max, int batch, int n_mel, int T,
                          hipStream_t s);

// --------------------------------------------------------------- decoder ---
// Appends k, v of positions pos0 .. pos0 + npos - 1 (from qkv rows p * B + b, [.][3d]) to the self-attention
// cache [2][B][cap][d] and attends each new position's q causally over positions 0 .. pos0 + p.  out rows likewise.
// bf16: the cache holds bf16 elements (bf16 storage mode).
// Throws kErrInvalidArg for pos0 < 0, npos < 1, pos0 + npos > 32 (the rows the kernel stages), pos0 + npos > cap, cap < 1,
// batch < 1 or heads < 1 (check_self_attention), before anything is launched.
void check_self_attention(int cap, int pos0, int npos, int batch, int heads);
void launch_self_attention(const float* qkv, void* kcache, void* vcache, int cap, int pos0, int npos, float* out,
                           int batch, int heads, hipStream_t s, bool bf16 = false);
// Full-length decoding (option max_positions): ONE new position `pos` (any in [0, cap); the engine uses it from 32 on)
// against a cache [B][cap][d], cap <= kSelfLongCap, fp32.  Appends the position's k and v (qkv rows b, [.][3d]) at cache
// row pos and attends its q causally over rows 0 .. pos; out rows b.  Rows > pos are neither read nor written.
// Throws kErrInvalidArg for pos < 0, pos >= cap, cap > kSelfLongCap, batch < 1 or heads < 1 (check_self_attention_long).
constexpr int kSelfLongCap = 448;  // n_text_ctx of every Whisper
// bf16 (bf16 storage mode): the cache holds bf16 elements, [B][cap][d]; the new k and v are rounded to
// nearest even before they are scored and stored, so rows written by launch_self_attention(.., bf16) and by this launcher
// read alike.  check_self_attention_long_bf16 refuses exactly what check_self_attention_long refuses.
void check_self_attention_long(int cap, int pos, int batch, int heads);
void check_self_attention_long_bf16(int cap, int pos, int batch, int heads);
void launch_self_attention_long(const float* qkv, void* kcache, void* vcache, int cap, int pos, float* out, int batch,
                                int heads, hipStream_t s, bool bf16 = false);
// A prompt behind a context (wt_engine_set_context): np >= 1 new positions pos0 .. pos0 + np - 1 against a cache
// [B][cap][d], cap <= kSelfLongCap, fp32.  Appends their k and v (qkv rows p * B + b, [.][3d]) at cache rows pos0 + p,
// each row written once, and attends each q causally over rows 0 .. pos0 + p: rows < pos0 from the cache, the others from
// qkv; out rows p * B + b.  Cache rows >= pos0 are never read, rows >= pos0 + np neither read nor written.
// Throws kErrInvalidArg for pos0 < 0, np < 1, pos0 + np > cap, cap > kSelfLongCap, np * batch > kSelfPrefillRows, batch < 1
// or heads < 1 (check_self_attention_prefill).
constexpr int kSelfPrefillRows = 128;  // rows of one decoder pass (Engine::kDecRowsMax)
// bf16: the cache holds bf16 elements and every key row taken from qkv is rounded as the appended rows are, so one
// launch of np positions equals the same positions in two launches, bit for bit.  Same refusals.
void check_self_attention_prefill(int cap, int pos0, int np, int batch, int heads);
void check_self_attention_prefill_bf16(int cap, int pos0, int np, int batch, int heads);
void launch_self_attention_prefill(const float* qkv, void* kcache, void* vcache, int cap, int pos0, int np, float* out,
                                   int batch, int heads, hipStream_t s, bool bf16 = false);
// The ragged forms of the two: pos / pos0 count SLOTS, clip b is at Whisper position slot - start[b]
// (start: device [B]) and runs there exactly as above; a position outside [0, min(P, cap)) is void — zeros in `out`, no
// cache row read or written.  The refusals are those above, except that self_attention_long's slot may lie past the
// cache (below 2 x kSelfLongCap); P outside [1, cap] and a null `start` are refused too.
// bf16 (option full_bf16_all): the caches hold bf16 elements as in the unragged bf16 forms, and a live
// clip's output and cache rows are those forms' at its own position, bit for bit.  The _bf16 checks refuse exactly what
// the fp32 checks refuse.
void check_self_attention_long_ragged(int cap, int pos, int P, int batch, int heads);
void check_self_attention_long_ragged_bf16(int cap, int pos, int P, int batch, int heads);
void launch_self_attention_long_ragged(const float* qkv, void* kcache, void* vcache, int cap, int pos, const int* start,
                                       int P, float* out, int batch, int heads, hipStream_t s, bool bf16 = false);
void check_self_attention_prefill_ragged(int cap, int pos0, int np, int P, int batch, int heads);
void check_self_attention_prefill_ragged_bf16(int cap, int pos0, int np, int P, int batch, int heads);
void launch_self_attention_prefill_ragged(const float* qkv, void* kcache, void* vcache, int cap, int pos0, int np,
                                          const int* start, int P, float* out, int batch, int heads, hipStream_t s,
                                          bool bf16 = false);
// The gathered form of self_attention_long: `rows` <= kSelfGatherRows rows share the cache
// [rows][cap][d], and row r reads key k < pos from cache row min(anc[r][k], rows - 1) (anc: device [rows][cap] bytes;
// entries at k >= pos are not read).  Key pos is appended to row r itself and out rows are r, as above; with
// anc[r][k] = r output and cache are bit-identical to launch_self_attention_long's.  Refused: what
// check_self_attention_long refuses, rows > kSelfGatherRows and a null table.
constexpr int kSelfGatherRows = 128;  // rows of one decoder pass; a table entry is one byte
// bf16: the cache holds bf16 elements; with anc[r][k] = r bit-identical to launch_self_attention_long(.., bf16).  Same refusals.
void check_self_attention_long_gather(int cap, int pos, int rows, int heads);
void check_self_attention_long_gather_bf16(int cap, int pos, int rows, int heads);
void launch_self_attention_long_gather(const float* qkv, void* kcache, void* vcache, int cap, int pos,
                                       const unsigned char* anc, float* out, int rows, int heads, hipStream_t s,
                                       bool bf16 = false);
// Cross attention of nq (1..4) query rows per clip over T cached keys, the query projection included:
// q = LayerNorm(x[row]) . Wq^T + bq with x the residual stream [nq * B][d], rows p * B + b.  wq_t = Wq in the
// layout of cross_q_layout(); kc, vc [B][heads][T][64]; partial results per key chunk in ws
// [row][heads][chunks][68] (o[64], m, l, pad), combined by the out-projection's prologue (kProCombine).
struct CrossAttnArgs {
  const float* x = nullptr;
  const float *ln_g = nullptr, *ln_b = nullptr, *wq_t = nullptr, *bq = nullptr;
  const void *kc = nullptr, *vc = nullptr;  // [clip][head][T][64] fp32, or bf16 when `bf16`
  float* ws = nullptr;
  int batch = 0, heads = 0, T = 0, chunks = 1, nq = 1;
  bool bf16 = false;
};
// Throws before anything is launched (check_cross_attention): kErrInvalidArg for batch, heads or T below 1, chunks
// outside [1, T] and nq outside [1, 4]; kErrFormat for a d_model = 64 heads other than 128, 384 or 512.
void check_cross_attention(const CrossAttnArgs& a);
void launch_cross_attention(const CrossAttnArgs& a, hipStream_t s);
// Cross attention with the K / V projections absorbed (k_cross_absorbed.hip): scores and context are taken against
// the encoder output E itself (planes: hi at e, lo at e + e_plane, scaled by the power of two e_scale; [clip][T][d]),
// shared by all heads and layers.  qp [rows][heads * d]: absorbed queries q'_h = c0 Wk_h^T (Wq_h LN(x) + bq_h) with
// c0 = d_head^-1/2 log2(e) (row = p * batch + b; this launch handles positions p0 .. p0 + nq - 1, nq * heads <= 16).
// ws [rows][heads][chunks][d + 4]: per key chunk the unnormalised context c[d], m (natural log), l.
struct CrossAbsorbedArgs {
  const float* qp = nullptr;
  const unsigned short* e = nullptr;
  // set: the chain decodes several encoder batches of `split` clips each (the last may be shorter): clips
  // [split, 2 split) read e2, [2 split, 3 split) e3, [3 split, batch) e4 — every one indexed from 0
  const unsigned short* e2 = nullptr;
  const unsigned short* e3 = nullptr;
  const unsigned short* e4 = nullptr;
  int split = 0;
  long e_plane = 0;
  float e_scale = 1.0f;
  float* ws = nullptr;
  int batch = 0, heads = 0, d_model = 0, T = 0, chunks = 1, nq = 1, p0 = 0;
  bool bf16 = false;  // bf16 storage mode: e (and e2 .. e4) are ONE bf16 plane [clips * T][d_model]; e_plane and e_scale unused
};
void launch_cross_absorbed(const CrossAbsorbedArgs& a, hipStream_t s);
int cross_absorbed_max_nq(int heads);  // positions one launch can take
// out [rows][heads * 64] = Wv_h (chunk-combined, normalised context of head h) + bv_h: the A operand of the ordinary
// cross out-projection.  wv_t = cross_q_layout(Wv).
void launch_cross_absorbed_combine(const float* ws, const float* wv_t, const float* bv, float* out, int rows, int heads,
                                   int chunks, int d_model, hipStream_t s);
// Greedy selection after the logits GEMM: reduces the per-tile (value, column) records
// best[B][n_tiles], appends to ids and applies the EOT stop (reference whisper.cpp:397-399).
// keep_ids: the id rows are given (test tap): the token is selected, counted and checked for EOT but not written.
void launch_select_token(const unsigned long long* best, int n_tiles, long long* ids, int ids_stride,
                         int pos, int* n_ids, int* finished, long long eot, int stop_at_eot, int batch,
                         hipStream_t s, bool keep_ids = false);
// ragged chain: finished[b] = 1 where pos - start[b] == P - 1 (device arrays [batch]); runs after the selection of slot pos
void launch_ragged_cap(const int* start, int pos, int P, int* finished, int batch, hipStream_t s);

// Spoken-language head (k_misc.hip, option "language" = -1 and wt_detect_language_*): per clip the final LayerNorm of
// its position-0 residual row (x [rows][d], + xpart when a K-split fc2 left two halves), the logits against the fp32
// embedding rows lang_lo .. lang_lo + n_lang - 1, softmax over those alone and the argmax (larger logit, then larger
// id).  probs [rows][n_lang], lang / lang_prob [rows]; ids != nullptr: ids[b][id_pos] = lang_lo + lang[b].
// forced_lang >= 0 (test tap): lang, lang_prob and the id report that language instead of the argmax.
constexpr int kLangMax = 128;    // language tokens (Whisper has 99 or 100)
constexpr int kLangMaxD = 1280;  // d_model of the largest Whisper
struct LanguageHeadArgs {
  const float *x = nullptr, *xpart = nullptr, *ln_g = nullptr, *ln_b = nullptr;
  const float* tok_emb = nullptr;  // [n_vocab][d]
  int rows = 0, d = 0, n_vocab = 0, lang_lo = 0, n_lang = 0;
  float* probs = nullptr;
  int* lang = nullptr;
  float* lang_prob = nullptr;
  long long* ids = nullptr;
  int ids_stride = 0, id_pos = 1, forced_lang = -1;
};
void launch_language_head(const LanguageHeadArgs& a, hipStream_t s);

// language_head on 16-lane groups with float4 loads (k_misc.hip): what the full-length chains
// (option full_language) and every detecting path under a candidate list launch.  Over language_head it takes, all as
// device data: allow (four words, bit r = language r, nullptr = all; outside it the logit is -inf and the probability
// exactly 0), hold [clips] (>= 0: report that language, clamped, probs as detected; < 0 or nullptr: detect), and a
// row mapping: clip b reads row b * x_rows_per_clip of x / xpart (x_rows rows in all) and writes lang_lo + lang[b] at
// column id_pos of the id rows b * fan .. b * fan + fan - 1 of up to two tables (ids[t] [ids_rows[t]][ids_stride[t]]).
// The launcher refuses d % 4 != 0, d > kLangMaxD, n_lang > kLangMax and rows or columns outside the buffers.
struct LanguageRowsArgs {
  const float *x = nullptr, *xpart = nullptr, *ln_g = nullptr, *ln_b = nullptr;
  const float* tok_emb = nullptr;  // [n_vocab][d]
  int clips = 0, x_rows = 0, x_rows_per_clip = 1, d = 0, n_vocab = 0, lang_lo = 0, n_lang = 0;
  const unsigned* allow = nullptr;
  const int* hold = nullptr;
  float* probs = nullptr;  // [clips][n_lang]
  int* lang = nullptr;
  float* lang_prob = nullptr;
  long long* ids[2] = {nullptr, nullptr};
  int ids_rows[2] = {0, 0}, ids_stride[2] = {0, 0};
  int id_pos = 1, fan = 0;  // fan = 0 without id tables
};
void launch_language_head_rows(const LanguageRowsArgs& a, hipStream_t s);

// ----------------------------------------------------------- beam search ---
// k_beam.hip (option beam_size 2..8).  Rows of a step are laid out row = k * clips + c (hypothesis slot k of clip c);
// the id rows are [row][32] int64 and the self-attention caches [layer][k|v][row][cap][d] as in launch_self_attention.
constexpr int kBeamMax = 8;          // largest beam_size
constexpr int kBeamChunk = 4096;     // vocabulary entries per top-k block: fixed, so a row's sums have one order
constexpr int kBeamMaxChunks = 16;   // n_vocab <= 65536
constexpr int kBeamClipsMax = 64;    // clips of one synchronous call (the per-clip state is indexed by clip)
struct BeamPart {                    // one (row, chunk): max logit, sum of exp(logit - max), top K+1 keys
  float m, s;                        // key = order-preserving bits of the logit << 32 | id (0 = none)
  unsigned long long key[kBeamMax + 1];
};
int beam_chunks(int n_vocab);
// logits [rows][ldl] -> part [rows][beam_chunks(V)], kk = K + 1 keys per chunk
void launch_beam_topk(const float* logits, int ldl, int V, int rows, int kk, BeamPart* part, hipStream_t s);
// per-clip state [kBeamClipsMax][kBeamMax] (fin_tok [clip][slot][32] generated ids), indexed by c0 + clip
struct BeamStepArgs {
  const BeamPart* part = nullptr;
  int n_chunks = 0;
  const long long* ids = nullptr;  // id rows of the live hypotheses (step 0: the prompt rows, one per clip)
  int clips = 0, K = 0, n_live = 0, pos = 0, n_prompt = 0, V = 0, c0 = 0;  // pos: the position the logits belong to
  long long eot = 0;
  float* live_sum = nullptr;
  int* fin_tok = nullptr;
  float* fin_sum = nullptr;
  int *fin_len = nullptr, *n_fin = nullptr, *done = nullptr;
  int* parent = nullptr;       // [K * clips]: the row each new row continues
  long long* token = nullptr;  // [K * clips]: its id at pos + 1
};
void launch_beam_select(const BeamStepArgs& a, hipStream_t s);
struct BeamReorderArgs {
  const float* kv_src = nullptr;  // [slabs][src_rows][cap][d]
  float* kv_dst = nullptr;        // [slabs][dst_rows][cap][d]
  int src_rows = 0, dst_rows = 0, cap = 0, d = 0, slabs = 0, pos = 0, V = 0;  // slabs = 0: the id rows only
  const long long* ids_src = nullptr;
  long long* ids_dst = nullptr;
  const int* parent = nullptr;
  const long long* token = nullptr;
};
void launch_beam_reorder(const BeamReorderArgs& a, hipStream_t s);
struct BeamFinalArgs {
  const long long* ids = nullptr;  // id rows after the last step's reorder
  int clips = 0, K = 0, c0 = 0, pos = 0, n_prompt = 0;
  const float* live_sum = nullptr;
  int* fin_tok = nullptr;
  float* fin_sum = nullptr;
  int *fin_len = nullptr, *n_fin = nullptr;
  const int* done = nullptr;
  long long* out_ids = nullptr;  // [kBeamClipsMax][32]
  int* out_n = nullptr;
  float* out_sum = nullptr;
  int* out_len = nullptr;
};
void launch_beam_finalize(const BeamFinalArgs& a, hipStream_t s);

// ------------------------------------------------------------ timestamps ---
// k_timestamps.hip (option timestamps): Whisper's timestamp rules on a row of logits, then the greedy
// step of select_token.  With g the ids a clip has generated, tick(id) = id - beg, last_ts = g[-1] >= beg,
// pen_ts = |g| < 2 or g[-2] >= beg:  (1) eot < id < beg is masked;  (2) last_ts and pen_ts: id >= beg masked; last_ts and
// not pen_ts: id < eot masked;  (3) ticks below the last timestamp's (+ 1 unless last_ts and not pen_ts) masked;
// (4) |g| = 0: id < beg masked, and ticks above max_initial when that is >= 0;  (5) logsumexp of the allowed timestamps
// above the best allowed text logit: id < beg masked;  (6) argmax, larger id on equal logits.
constexpr int kTsChunk = 4096;     // vocabulary entries per ts_partial block: fixed, so a row's sums have one order
constexpr int kTsMaxChunks = 64;   // n_vocab <= 262144
struct TsState {                   // carried per clip from step to step
  int tick;                        // tick of the last timestamp generated, -1: none yet
  int last_is_ts, prev_is_ts;      // g[-1], g[-2] are timestamps (0 where they do not exist)
};
struct TsPart {                    // one (clip, chunk); key = order-preserving bits of the logit << 32 | id, 0 = none
  unsigned long long key_text, key_ts;  // best allowed id below beg, best allowed timestamp
  float m, s;                           // max of the allowed timestamps' logits, sum of exp(logit - m)
};
int ts_chunks(int n_vocab);
// state[b] from the ids [sample_begin, n) of row b, n = n_ids[b] (or n_fixed for every row when n_ids is nullptr)
void launch_ts_state_init(const long long* ids, int ids_stride, const int* n_ids, int n_fixed, int sample_begin, int V,
                          int beg, TsState* state, int batch, hipStream_t s);
struct TsSelectArgs {
  const float* logits = nullptr;  // [batch][ldl], ldl % 4 == 0, 16-byte aligned: the logits of position pos
  int ldl = 0, V = 0, batch = 0;
  int eot = 0, beg = 0, max_initial = -1;  // 0 <= eot < beg < V
  int n_gen = 0;                  // ids generated before this step: pos + 1 - sample_begin
  TsPart* part = nullptr;         // [batch][ts_chunks(V)]
  TsState* state = nullptr;       // [batch], read and advanced
  long long* ids = nullptr;       // ids[b][pos + 1] = the token
  int ids_stride = 0, pos = 0, stop_at_eot = 1;
  int *n_ids = nullptr, *finished = nullptr;  // as launch_select_token
  double* dbg_L = nullptr;        // optional [batch]: rule 5's logsumexp and best text logit, NaN where none is allowed
  float* dbg_M = nullptr;
};
void launch_ts_select(const TsSelectArgs& a, hipStream_t s);  // ts_partial + ts_select; throws kErrInvalidArg

// -------------------------------------------------------------- sampling ---
// k_sample.hip (option temperature): the selection step at a temperature.  The token is the argmax
// over the allowed ids of k_i = z_i * inv_t + g_i (ties: the larger id), g_i = -log(-log u_i), u_i from Philox4x32-10
// under the counter (i >> 2, rng_pos, clip_base + row0 + b, attempt) and the key (seed_lo, seed_hi); inv_t = 0: k_i =
// z_i, the step of select_token / ts_select.  The allowed set is the whole vocabulary (state == nullptr) or what the
// timestamp rules leave, rule 5 decided on the untempered logits exactly as ts_select decides it.
constexpr int kSampleClipsMax = 64;  // clips of one synchronous call
constexpr int kSampleGroupMax = 8;   // samples per clip of one launch (option best_of)
constexpr int kSampleRowsMax = 128;  // rows of a grouped launch (kDecRowsMax)
struct SampleParams {                // device memory, written ahead of a chain: nothing here is a kernel argument
  unsigned seed_lo, seed_hi, attempt, clip_base;
  float inv_t[kSampleClipsMax];      // 1 / T per clip, 0 = greedy
  // the ragged chain: the counter's position word is rng_pos - pos_off[clip] (the clip's own Whisper
  // position under a slot count) and its clip word clip_base + clip + clip_off[clip]; zeros give the words above
  int pos_off[kSampleClipsMax];
  int clip_off[kSampleClipsMax];
};
struct SamplePart {                  // one (clip, chunk); keys as TsPart's
  unsigned long long pkey_text, pkey_ts;  // best perturbed key over the allowed ids below beg / the allowed timestamps
  unsigned long long key_text, key_ts;    // ts_partial's record: the same bits
  float m, s;
};
struct SampleArgs {
  const float* logits = nullptr;  // as TsSelectArgs
  int ldl = 0, V = 0, batch = 0;
  int eot = 0, beg = 0, max_initial = -1, n_gen = 0;
  const SampleParams* params = nullptr;
  int row0 = 0;                   // clip b of this launch is clip row0 + b of the parameter block
  // group = N > 1: the batch rows are N samples of clips = ceil(batch / N) clips, row r = sample r / clips of clip
  // r % clips (k_beam_full.hip's row order); the block is indexed by row0 + clip and sample j draws under the attempt
  // word attempt + (j << 16), so sample 0 is the draw of group = 1.  batch <= 128, row0 + clips <= kSampleClipsMax.
  int group = 1;
  int rng_pos = -1;               // the counter's position word; -1 = pos
  SamplePart* part = nullptr;     // [batch][ts_chunks(V)]
  TsState* state = nullptr;       // [batch], read and advanced; nullptr = plain mode
  long long* ids = nullptr;
  int ids_stride = 0, pos = 0, stop_at_eot = 1;
  int *n_ids = nullptr, *finished = nullptr;
  double* dbg_L = nullptr;        // optional [batch], as TsSelectArgs
  float* dbg_M = nullptr;
  float* dbg_key = nullptr;       // optional [batch]: the winning key k
};
void launch_sample_select(const SampleArgs& a, hipStream_t s);  // sample_partial + sample_select; throws kErrInvalidArg

// ---------------------------------------------------------------- scores ---
// k_scores.hip (option scores): the log-probability of the id a greedy step chose,
// lp = z[tok] - logsumexp(z[i] : i allowed at that step), and a clip's no-speech probability.  The allowed set is the
// whole vocabulary (state == nullptr) or the one the timestamp rules left: rules 1 .. 4 from the clip's TsState BEFORE
// the step's ts_select advanced it, then rule 5 decided as ts_select decides it.
struct ScorePart {                 // one (clip, chunk of kTsChunk entries)
  float mt, st;                    // max of the allowed text logits, sum of exp(logit - mt)
  float ms, ss;                    // the same of the allowed timestamps
  int has_t, has_s;                // the clip's intervals are non-empty (equal in all its chunks)
};
struct ScoreArgs {
  const float* logits = nullptr;   // [batch][ldl], ldl % 4 == 0, 16-byte aligned: the logits of position pos
  int ldl = 0, V = 0, batch = 0;
  const TsState* state = nullptr;  // [batch] or nullptr = plain mode; with it eot, beg, max_initial, n_gen as TsSelectArgs
  int eot = 0, beg = 0, max_initial = -1, n_gen = 0;
  ScorePart* part = nullptr;       // [batch][ts_chunks(V)]
  // launch_score_finish only:
  const long long* ids = nullptr;  // ids[b][pos + 1] = the id the selection kernel wrote
  int ids_stride = 0, pos = 0;
  const int* n_ids = nullptr;      // after the selection kernel: n_ids[b] == pos + 2 where the clip was live
  float* token_logprob = nullptr;  // [batch][lp_stride]: token_logprob[b][pos + 1] = lp
  int lp_stride = 0;
  double* sum = nullptr;           // [batch] carried: += lp where the clip was live
  int* count = nullptr;            // [batch] carried: += 1 there
  double* dbg_den = nullptr;       // optional [batch]: the float64 logsumexp of the allowed set
};
void launch_score_partial(const ScoreArgs& a, hipStream_t s);  // throws kErrInvalidArg, as launch_ts_select
void launch_score_finish(const ScoreArgs& a, hipStream_t s);   // reads the records launch_score_partial wrote
// prob[b] = exp(z[b][nosp] - logsumexp(z[b][0 .. V - 1])): score_partial over the whole row + a finish kernel
void launch_no_speech_prob(const ScoreArgs& a, int nosp, float* prob, hipStream_t s);

// ----------------------------------------------------------- suppression ---
// k_suppress.hip (wt_engine_set_suppress): Whisper's SuppressTokens / SuppressBlank.  Row r of
// logits [rows][ldl] gets -inf at every id of ids[0 .. n) and, with first != 0 (the first generated position), of
// ids[n .. n + n_first).  ids is device memory, read at run time: its contents are no launch constant.  Nothing is read
// from the logits, an id outside [0, V) is skipped.
constexpr int kSuppressIdsMax = 1024;  // ids per list
constexpr int kSuppressRowsMax = 128;  // rows of one launch (kDecRowsMax)
struct SuppressArgs {
  float* logits = nullptr;
  int ldl = 0, V = 0, rows = 0;
  const int* ids = nullptr;  // [n + n_first]
  int n = 0, n_first = 0, first = 0;
};
void launch_suppress_logits(const SuppressArgs& a, hipStream_t s);  // throws kErrInvalidArg, as launch_ts_select

// ------------------------------------------------- full-length beam search ---
// k_beam_full.hip (option full_beam): beam search over up to full_cap() positions behind the timestamp
// rules.  Rows are laid out row = k * clips + c as in k_beam.hip; a row's ids [stride] int64, its log-probabilities
// [stride] float (index = position of the id) and its ancestor table [cap] bytes (launch_self_attention_long_gather) live
// in two halves of a double buffer: a step reads the live hypotheses from `src` and writes the next ones to `dst`.  No
// K / V moves.  Per step every live hypothesis applies its OWN allowed set A (the whole vocabulary, or rules 1 .. 5 of
// section 14 on its TsState), lp = z - logsumexp_A(z) in float64 from fp32 chunk sums merged in chunk order, and offers
// its top K+1 ids of A (a logit of -inf is never in A); beam_select's walk follows.  The number of live hypotheses of a
// clip is state: a walk that finds fewer than K non-EOT candidates leaves fewer, and a clip with none is done.
struct BeamFullPart {                // one (row, chunk of kBeamChunk entries); keys as BeamPart's
  float mt, st, ms, ss;              // max and sum of exp(logit - max) of the allowed text ids / the allowed timestamps
  unsigned long long kt[kBeamMax + 1], ks[kBeamMax + 1];  // their top K+1 keys, 0 = none
};
struct BeamFullArgs {
  int clips = 0, K = 0, c0 = 0;      // clips of the chain, beam size, the chain's first clip in the per-clip state
  int pos = 0, n_prompt = 0;         // the position the logits belong to; step t = pos + 1 - n_prompt has clips live rows
  int V = 0, ldl = 0, stride = 0, cap = 0;  // at t = 0 and K * clips afterwards; pos < cap < stride
  int eot = 0, beg = 0, max_initial = -1, timestamps = 0;
  const float* logits = nullptr;     // [live rows][ldl]
  BeamFullPart* part = nullptr;      // [live rows][beam_chunks(V)]
  const long long* ids_src = nullptr;
  long long* ids_dst = nullptr;
  const float* lp_src = nullptr;
  float* lp_dst = nullptr;
  const unsigned char* anc_src = nullptr;
  unsigned char* anc_dst = nullptr;
  TsState* ts = nullptr;             // [K * clips] per row, read and advanced in place
  // per-clip state, indexed by c0 + clip: [kBeamClipsMax] or [kBeamClipsMax][kBeamMax] (fin_tok / fin_lp: [..][stride],
  // the generated ids of a finished hypothesis and their log-probabilities)
  int* n_live = nullptr;
  double* live_sum = nullptr;
  int* fin_tok = nullptr;
  float* fin_lp = nullptr;
  double* fin_sum = nullptr;
  int *fin_len = nullptr, *n_fin = nullptr, *done = nullptr;
  int* parent = nullptr;             // [K * clips]: the row each new row continues, its id at pos + 1 and that id's lp
  long long* token = nullptr;
  float* tok_lp = nullptr;
  double* dbg_lse = nullptr;         // optional [live rows]: logsumexp_A of the live rows (NaN where A is empty)
  // launch_beam_full_finalize only: the chosen hypothesis per clip, indexed by c0 + clip
  long long* out_ids = nullptr;      // [kBeamClipsMax][stride]: prompt + generated ids
  float* out_lp = nullptr;           // [kBeamClipsMax][stride]
  int *out_n = nullptr, *out_len = nullptr;
  double* out_sum = nullptr;
};
// Every launcher throws kErrInvalidArg for a shape outside: K in [2, 8], K * clips <= 128, c0 + clips <= 64,
// 1 <= n_prompt <= pos + 1, pos < cap <= kSelfLongCap, cap < stride, V <= ldl, beam_chunks(V) <= kBeamMaxChunks and,
// with timestamps, 0 <= eot < beg < V.
void launch_beam_full_begin(const BeamFullArgs& a, hipStream_t s);     // a chain's start: state of the clips, rows c of dst
void launch_beam_full_partial(const BeamFullArgs& a, hipStream_t s);
void launch_beam_full_select(const BeamFullArgs& a, hipStream_t s);
void launch_beam_full_advance(const BeamFullArgs& a, hipStream_t s);
void launch_beam_full_finalize(const BeamFullArgs& a, hipStream_t s);  // src = the rows after the last step's advance

// ---------------------------------------------------------------- best of ---
// k_best_of.hip (option best_of): the two ends of a chain that decodes N samples of each of its
// clips.  Rows are laid out row = j * clips + c (sample j of clip c) as k_beam_full.hip's, a row's ids [stride] int64
// and log-probabilities [stride] float as there.  best_of_begin copies the clips' prompt rows (rows c, j = 0) into
// their other samples' rows, sets n_ids, finished (1 where frozen[c]), the score sums and counts, and writes the
// FIXED ancestor table of the gathered self_attention_long: anc[r][k] = r % clips for k < n_prompt - 1 (the prompt's
// K / V, which the narrow passes wrote to rows c), else r.  best_of_pick keeps, per clip, the first sample with the
// largest sum / count in float64 (a NaN, or a count below 1, never wins; sample 0 where none is left) and copies its
// row to the clip's output row c0 + c.
struct BestOfArgs {
  int clips = 0, N = 0, c0 = 0;      // clips of the chain, samples per clip, the chain's first clip in the output rows
  int n_prompt = 0, stride = 0, cap = 0;  // 1 <= n_prompt <= cap < stride
  long long* ids = nullptr;          // [N * clips][stride]; begin reads rows c < clips and writes the others
  float* lp = nullptr;               // [N * clips][stride]: pick reads it
  int* n_ids = nullptr;              // [N * clips]
  int* finished = nullptr;           // [N * clips]
  double* sum = nullptr;             // [N * clips]: score_finish's carried sum and count
  int* count = nullptr;
  // launch_best_of_begin only
  const int* frozen = nullptr;       // optional [clips]
  unsigned char* anc = nullptr;      // [N * clips][cap]
  // launch_best_of_pick only: indexed by c0 + clip
  long long* out_ids = nullptr;      // [..][stride]: the row's first n_ids ids, zeros behind them
  float* out_lp = nullptr;           // [..][stride]
  int *out_n = nullptr, *out_count = nullptr, *picked = nullptr;
  double* out_sum = nullptr;
  double* all_sum = nullptr;         // [..][kSampleGroupMax]: every sample's sum and count, zeros from N on
  int* all_count = nullptr;
};
// Both throw kErrInvalidArg outside N in [1, 8], N * clips <= 128, c0 + clips <= 64, 1 <= n_prompt <= cap < stride.
void launch_best_of_begin(const BestOfArgs& a, hipStream_t s);
void launch_best_of_pick(const BestOfArgs& a, hipStream_t s);

// ------------------------------------------------------------- alignment ---
// k_align.hip (word-level timestamps): from the cross-attention weights W of a teacher-forced pass
// to the frame at which every text id begins.  Per-clip sizes are read from device memory; a size outside its array's
// bounds is clamped to them by the kernels.
constexpr int kAlignHeadsMax = 128;    // alignment heads of one call
constexpr int kAlignRowsMax = 447;     // cost rows of a clip: <|notimestamps|> and its text ids
constexpr int kAlignFramesMax = 1500;  // encoder frames of a clip
constexpr int kAlignClipsMax = 64;     // clips of one launch
constexpr int kAlignLayerHeadsMax = 8; // alignment heads of one layer (d_model <= 512)
constexpr int kAlignChunkTiles = 8;    // mode 1: 16-frame tiles per block of align_scores (128 frames)
struct AlignScoresArgs {
  const float* qp = nullptr;       // [np * batch][H * d_model] absorbed queries of one pass of a layer, row = p * batch + b
  const unsigned short* e = nullptr;  // E as fp16 planes [batch][T][d_model]: hi at e, lo at e + e_plane, times e_scale
  long e_plane = 0;
  float e_scale = 1.0f;
  // bf16 storage mode (option full_bf16_all): e is ONE bf16 plane [batch][T][d_model], q' is rounded to
  // bf16 in the kernel; e_plane and e_scale are not read
  bool bf16 = false;
  int batch = 0, H = 0, d_model = 0, T = 0;  // T % 4 == 0
  int np = 0, pos0 = 0;            // the pass holds the fed positions pos0 .. pos0 + np - 1; np * batch <= 128
  int n_heads = 0;                 // alignment heads of this layer
  int head[kAlignLayerHeadsMax] = {}, slot[kAlignLayerHeadsMax] = {};  // their index in the layer and in W's head axis
  int F[kAlignClipsMax] = {};      // valid frames of every clip, 1 .. T
  float* W = nullptr;              // [batch][heads_total][L_max][ldw]: rows pos0 .. pos0 + np - 1 of the n_heads slots are
  int heads_total = 0, L_max = 0, ldw = 0;  // written whole, frames < T; ldw % 4 == 0, 16-byte aligned
  // 0: one wavefront sweeps all frames of its 16 columns, softmax in the same kernel; 1: blocks per chunk of
  // kAlignChunkTiles tiles store the scores, align_softmax_rows normalises them (one more launch)
  int mode = 1;
};
// W = softmax over t < F[b] of q' . e_t on the matrix cores, zero at F[b] <= t < T.  Head list and frame counts are
// launch constants; a head or a slot listed twice is refused.  Throws kErrInvalidArg before anything is launched.
void launch_align_scores(const AlignScoresArgs& a, hipStream_t s);
struct AlignMatrixArgs {
  const float* W = nullptr;   // [clips][heads][L_max][ldw]: softmax over the frames t < F[b], per head and fed position
  int clips = 0, heads = 0, L_max = 0, ldw = 0;
  const int* L = nullptr;     // device [clips]: fed positions of the clip, the rows its statistics run over
  const int* F = nullptr;     // device [clips]: valid frames
  int n_a = 0;                // cost row r is W's row n_a + r; a clip has N[b] = L[b] - n_a - 1 of them
  float* stats = nullptr;     // [clips][heads][2][ldw]: mean, then 1 / std (population; 0 for a column of equal values)
  float* C = nullptr;         // [clips][N_max][ldc]: rows < N[b], frames < F[b] are written, nothing else
  int N_max = 0, ldc = 0;
};
// align_column_stats, then align_filter_mean: C = -mean over the heads (ascending) of median7(Z) with reflect padding
// (no filter when F[b] <= 3), Z = (W - mean) / std.  Throws kErrInvalidArg.
void launch_align_matrix(const AlignMatrixArgs& a, hipStream_t s);
struct AlignDtwArgs {
  const float* C = nullptr;        // [clips][N_max][ldc]
  int clips = 0, N_max = 0, ldc = 0;
  const int* N = nullptr;          // device [clips]: rows of the clip (0: nothing to align)
  const int* F = nullptr;          // device [clips]: frames
  unsigned char* trace = nullptr;  // [clips][N_max][ldc] workspace: the trace codes of the cells
  int* jump = nullptr;             // [clips][N_max]: first frame of the path in each row < N[b], 0 behind them
};
// wt::dtw_path (words.h) per clip, bit for bit: one block per clip over the anti-diagonals, then the back-trace.
// N_max <= kAlignRowsMax, ldc <= kAlignFramesMax, else kErrInvalidArg.
void launch_align_dtw(const AlignDtwArgs& a, hipStream_t s);

// ---- load-time re-layouts of decoder weights (host) ----
// bf16 storage mode: W [N][K] fp32 -> ONE bf16 plane (round to nearest even) in the same fragment order,
// [ceil(N/32)][K/16][64 lanes][8]
std::vector<unsigned short> tile_weights_bf16(const float* W, int N, int K);
// W [N][K] fp32 -> two fp16 planes in MFMA-fragment order [ceil(N/32)][K/16][plane][64 lanes][8] (rows past N zero):
// lane (l & 31, l >> 5) of tile t, step s holds W[32t + (l & 31)][16s + 8(l >> 5) .. +7] * scale as hi = fp16(v),
// lo = fp16(v - hi).  *scale = f16_scale_for(max |W|).  K % 16 == 0.
std::vector<unsigned short> tile_weights_f16(const float* W, int N, int K, float* scale);
// Wq [d][d] -> [head][d / 4][64 outputs][4 k] for cross_attention_step's in-kernel query projection
std::vector<float> cross_q_layout(const float* Wq, int d);
// The absorbed cross-attention's fused query matrix (engine.cpp): A [heads * d][d], A_h = c0 Wk_h^T Wq_h, and
// av [heads * d], a_h = c0 Wk_h^T bq_h, c0 = d_head^-1/2 log2 e; wq, wk [d][d] row-major, bq [d].  Host only.
void absorbed_query_matrix(const float* wq, const float* bq, const float* wk, int heads, int d, std::vector<float>* A,
                           std::vector<float>* av);

}  // namespace wt
