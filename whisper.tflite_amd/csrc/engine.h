// Engine: weights resident in HBM + the launch sequence of the EncDec hot path
// (reference EncDec::transcribe, whisper.tflite/whisper.cpp:752-769), batch-first.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "decode_results.h"
#include "error.h"
#include "host_util.h"
#include "wtw_format.h"

namespace wt {

struct TsPart;   // kernels.h
struct TsState;

struct BeamPart;  // kernels.h
struct BeamFullPart;
struct ScorePart;
struct SamplePart;
struct SampleParams;

// WT_DEC_KERNEL_TIMERS diagnostics: the event pairs and launch classes of a slot's eager decoder launches
struct DecTimers {
  std::vector<hipEvent_t>& ev;
  std::vector<int>& cls;
  hipStream_t stream;
  size_t used = 0;
};

struct Timings {
  float logmel_ms = 0, encoder_ms = 0, cross_kv_ms = 0, decoder_ms = 0, total_ms = 0;
  int batch = 0, decoder_steps = 0;
};

// Per-kernel-class device time of the last encode(), from HIP event pairs recorded on the
// engine's stream around every launch of that class (bench.py's roofline figures).
struct KernelStat {
  const char* name;
  int launches;
  double ms;     // sum of launch durations
  double flops;  // algorithmic FLOPs of those launches
  double bytes;  // algorithmic bytes (bandwidth-bound kernels)
};
// kKcGemm / kKcEncAttn: the default plane kernels (or the bf16-storage ones); *Alt: contractions that ran on the
// fp32-storage kernels instead (a load-time fall-back of that contraction, or a forced gemm_variant / attn_variant);
// kKcConvert: the fp32 -> planes hand-over between the two kinds
enum KernelClass { kKcGemm = 0, kKcEncAttn, kKcLayerNorm, kKcTranspose, kKcGemmAlt, kKcEncAttnAlt, kKcConvert, kKcCount };

// Operand scales of the two-plane fp16 encoder kernels (powers of two, f16_scale_for): derived at load
// time from weight-only upper bounds of every contraction operand (LayerNorm output <= |g| sqrt(d-1) + |b|,
// Linear output <= sum |W| * input bound + |bias|, GELU(x) <= max(x, 0.17), attention output <= V bound),
// so no operand can overflow fp16 for an input mel inside Engine::kMelBound
struct GemmScale {
  float a = 1.0f, w = 64.0f;
  bool f16_ok = true;  // false: the operand's bound is too far above its typical magnitude (upload_weights)
};
// The weight side of one encoder contraction, in every form a kernel takes it (Engine::encode_enqueue picks one per launch)
struct EncLinear {
  const float* w32 = nullptr;           // [N][k32] fp32 row-major: the fp32-storage fall-back kernels (k_gemm.hip)
  const unsigned short* wp = nullptr;   // both fp16 planes, blocked (split_weight_planes), scaled by sc.w: the plane GEMM
  const unsigned short* wbf = nullptr;  // [N][kbf] bf16: bf16 storage mode; null until ensure_bf16_weights
  const float* bias = nullptr;
  // k: the contraction's own length; k32 / kp / kbf: what each form pads it to, zero filled (its k-tile: 32, 32 and
  // 64).  Only conv1's k = 3 n_mels is no multiple of them already.
  int N = 0, k = 0, k32 = 0, kp = 0, kbf = 0;
  GemmScale sc;
};
struct EncLayer {
  const float *attn_ln_g = nullptr, *attn_ln_b = nullptr, *mlp_ln_g = nullptr, *mlp_ln_b = nullptr;
  EncLinear qkv, out, fc1, fc2;      // qkv: query | key | value fused, [3d][d] (the key has no bias)
  float q = 1.0f, k = 1.0f, v = 1.0f;  // operand scales of the plane attention
  bool attn_f16_ok = true;
};
// decoder Linear weights: two fp16 planes in MFMA-fragment order (kernels.h tile_weights_f16) + their scale
struct TiledW {
  const unsigned short* w = nullptr;
  float scale = 1.0f;
};
struct DecBlockWeights {
  const float *attn_ln_g, *attn_ln_b, *bqkv, *bo;
  TiledW wqkv, wo;
  const float *cross_ln_g, *cross_ln_b, *cross_wq_t, *cross_bq, *cross_bo;  // cross_wq_t: cross_q_layout()
  TiledW cross_wo;
  // absorbed cross-attention (k_cross_absorbed.hip): the key projection folded into the query side, A_h = c0 Wk_h^T Wq_h
  // stacked over heads [H d][d] with its bias c0 Wk_h^T bq_h (upload_weights); the value projection is applied to the
  // combined context of each head by cross_absorbed_combine
  TiledW wq_abs;
  const float *bq_abs = nullptr, *cross_wv_t = nullptr, *cross_bv = nullptr;  // cross_wv_t: cross_q_layout(Wv)
  const float *mlp_ln_g, *mlp_ln_b, *b1, *b2;
  TiledW w1, w2;
};

// Opens a .wtw file and checks header, tensor table and length without touching a GPU; throws wt::Error (kErrIo /
// kErrFormat).  wt_engine_create uses it to decide whether a .wtw next to a .tflite pair must be rebuilt.
void check_wtw_file(const std::string& path);

class Engine {
 public:
  // Throws std::runtime_error with a message; the C ABI maps it to a status code.
  // monolith: the reference's other engine type (whisper.h:165-179) routed to the same encoder / decoder
  // kernels; it differs in the prompt only (prompt(), engine.cpp)
  // weights_path: the .wtw to load; empty = model_prefix + ".wtw"
  Engine(const std::string& model_prefix, const std::string& vocab_path, bool multilingual,
         int device_id, bool monolith = false, const std::string& weights_path = "");
  // front end only: log-mel kernels over `filters` (80 x 201), no weights; encode()/decode() must not be called
  Engine(const FilterBank& filters, int device_id);
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  const wtw::Dims& dims() const { return dims_; }
  const VocabData& vocab() const { return vocab_; }
  const FilterBank& filters() const { return filters_; }
  const Timings& timings() const { return timings_; }
  hipStream_t stream() const { return stream_; }
  hipStream_t decoder_stream(int i) const { return dstream_[i % n_dec_streams_]; }

  // options (reference hard-codes them, see wt_capi.h)
  long language = 2;  // language_id("de"); -1 = detected per clip on the device (language_head)
  long max_tokens = 30;
  long stop_at_eot = 1;
  long verbose = 0;
  // key chunks per (clip, head) of the decoder cross-attention: 1, 2, 4, 8, or 0 = as many as make clips x heads x
  // chunks reach 192 blocks (32 clips x 6 heads: one chunk — in the pipeline fewer, longer blocks with one query
  // prologue per (clip, head) measured 121.2 k audio-sec/s against 119.0 k with two chunks and 113.8 k with four; a
  // single clip needs the chunks to spread its 6 heads over the chip)
  long cross_chunks = 0;
  long attn_variant = 4;  // encoder attention: 4 = two fp16 planes (default), 1 = three bf16 planes (full range), 0 = fp32 MFMA
  long fc2_ksplit = 2;  // decoder fc2 (K = 4 d_model) over twice the blocks, halves summed by the consumer
  long use_graphs = 1;  // replay the decoder's launch sequence from a captured hipGraph
  // 1 = decoder cross-attention against the encoder output itself, K / V projections absorbed into the query and
  // output sides (k_cross_absorbed.hip: half the bytes per decoder position, no cross-KV GEMM in the encoder);
  // 0 = round 2's cross-KV cache.  Both storage modes run either form (absorb_active()); a flagged ln_post operand
  // (its planes are what the absorbed form streams) always takes the cache.
  long cross_absorb = 1;
  long abs_chunks = 0;  // key chunks per clip of the absorbed form: 1..16, 0 = by batch size and mode (decode_enqueue)
  // 1 = the pipeline decodes TWO consecutive submitted batches of equal size (<= 32 clips each, absorbed form) with
  // one decoder chain: the chain's ~1000 dependent launches then serve 64 clips, and the decoder streams stop being
  // what the pipeline waits for.  Results and their order are unchanged; a batch whose partner has
  // not been submitted yet is decoded alone as soon as it is collected.
  long dec_pair = 1;
  // batches per decoder chain when dec_pair is on: 2 (default), 3 or 4 — rows of a chain = group x batch <= 128 (the
  // decoder GEMMs' row contract); the pipeline needs about 3 x group + 3 batches in flight to keep three chains fed
  long dec_group = 2;
  long last_batches = 0;  // the next N submits are the last of a job: decoded one chain per batch (latency form); counts down
  // absorbed cross-attention in effect: the default mode needs E as fp16 planes (no fall-back on that operand); bf16
  // storage mode streams E as one bf16 plane
  bool absorb_active() const { return cross_absorb != 0 && (bf16 != 0 || (gemm_variant < 0 && cross_kv_.sc.f16_ok)); }
  // ... and chosen for a call: every pipelined batch (throughput: half the decoder's stream bytes, no cross-KV GEMM);
  // synchronous calls only from 32 clips on — below that the cached form's 7 launches per decoder layer beat the absorbed
  // form's 9 (single clip 7.2 against 9.0 ms, 16 clips 11.1 against 12.1 ms, 32 clips 15.2 against 15.0 ms)
  // (beam search: always, whatever the batch size; its K query rows per clip ride the absorbed form's position loop)
  bool absorb_for(int batch) const { return absorb_active() && (pipelined_call_ || batch >= 32 || beam_size > 1 || (max_positions > 0 && best_of_sampling())); }
  // 1 = greedy (the reference's argmax loop); 2..8 = beam search with that many hypotheses per clip on the synchronous
  // entry points (decode_beam).  Scope: stop_at_eot = 1, the absorbed cross-attention, fp32-accurate
  // storage; no pipeline, no forced ids, no logits tap (check_beam_call).
  long beam_size = 1;
  // throws kErrUnsupported when beam_size > 1 and the call or the options fall outside beam search's scope
  void check_beam_call(bool logits_tap, bool allow_bf16 = false) const;  // allow_bf16: the full-length chain under full_bf16
  // What the last decode call left for the wt_last_* getters, in groups with one flag each (decode_results.h, DESIGN
  // section 29).  Every entry point forgets its own mask of groups first and fills the groups its options ask for.
  DecodeResults last;
  // Spoken-language detection.  The language tokens are ids [kLangLo, kLangLo + lang_tokens()): lang_tokens() =
  // min(language_count(), token_translate - kLangLo), or 0 when the engine has none (English-only, or a vocabulary
  // that ends before them).  language = -1 makes every greedy decode detect per clip (decode_enqueue); scope:
  // no beam search, no caller prompt, no forced ids, no Monolith engine (check_language_call).
  static constexpr long kLangLo = 50259;
  int lang_tokens() const;
  // option "language": -1 .. language_count() - 1; -1 is kErrUnsupported on a Monolith engine or without language tokens
  void set_language(long value);
  void check_language_call() const;  // throws kErrUnsupported when language = -1 and the options fall outside that scope
  // encoder output of the last encode() -> one decoder pass over position 0 of [sot] + language_head, nothing else
  // decoded: lang [batch], probs [batch][lang_tokens()] (or nullptr), prob [batch] (or nullptr).  batch <= 64.
  void detect_language(int batch, int32_t* lang, float* probs, float* prob);
  // Full-length greedy decoding (decode_full).  0 = off: the max_tokens path above, 31 positions.
  // P in [32, full_cap()]: the oracle's max_positions — positions 0 .. P - 1 are fed, a row holds at most P + 1 ids —
  // on the synchronous full-length entry points and the text entry points.  Scope: greedy, fp32-accurate storage, a
  // prompt language; no pipeline, no forced ids, no logits tap (check_full_call).
  long max_positions = 0;
  int full_cap() const { return std::min(dims_.n_text_ctx, 448); }  // (448: kSelfLongCap, kernels.h)
  // arguments of a full-length token call: kErrInvalidArg without the option or for a batch outside [1, 64],
  // check_full_call(), kErrBuffer for ids_stride < max_positions + 1
  void check_full_args(int batch, int ids_stride) const;
  void check_full_call() const;  // throws kErrUnsupported when max_positions is set and the options fall outside that scope
  // encoder output of the last encode() -> ids [batch][ids_stride] (prompt + generated, zero-padded), n_ids [batch];
  // ids_stride >= max_positions + 1, batch <= 64.  Synchronises.
  // valid_samples (word timestamps): the samples each clip holds before its zero padding; nullptr = full-length clips
  void decode_full(int batch, int64_t* ids, int ids_stride, int32_t* n_ids, const std::vector<long long>* valid_samples = nullptr);
  void encode_full(const float* d_mel, int batch);  // encode() into slot 0: the slot every full-length call uses
  // Full-length beam search (decode_beam_full).  0: a full-length call with beam_size > 1 is refused.
  // 1: beam_size 2..8 with max_positions runs the beam chain to P positions, with or without timestamps, scores and
  // skip_silence; decode_full hands such a call over, so every full-length entry point honours the mode.  Scope:
  // beam search's (check_beam_call) and full-length decoding's, and no temperature (unless fallback_beam = 1), context,
  // seek, word timestamps or batched seeking (check_full_call).
  long full_beam = 0;
  // Automatic language behind max_positions.  0: a full-length call with language = -1 is refused.
  // 1: every clip is decoded behind [sot, <its language>, task, ..]; the language is the argmax over the allowed
  // language tokens of the logits at position 0 of [sot] alone — what detect_language returns for the clip, whatever
  // the context, temperature, seed, attempt, suppression lists, batch or use_graphs.  A chain without a context
  // reads it off its own position-0 pass (language_head_rows writes ids[b][1] before position 1 is embedded); behind
  // a context one pass over [sot] runs in front of the chain.  The long loops detect once per file, on its first
  // window, and hold that language for the file's later windows (clip_lang_hold).  Beam search and best_of build their
  // id rows on the host: for them one detect_language pass runs in front of the chains.  Scope: full-length
  // decoding's, and no caller prompt, forced ids or Monolith engine (check_full_call).
  long full_language = 0;
  // Full-length decoding in the bf16 storage mode.  0: a full-length call on a bf16 engine is
  // refused.  1: the three full-length chains (decode_full, beam_full_chains, the best-of chain) run with bf16 weights,
  // bf16 cross-attention operands and a bf16 self-attention cache (the first half of the fp32 allocation), on the bf16
  // forms of self_attention_long, its gathered form and self_attention_prefill.  Scope: full-length decoding's, and no
  // word_timestamps, per-clip contexts, batched seeking or automatic language (check_full_call) unless full_bf16_all is set.
  long full_bf16 = 0;
  // The rest of the full-length chains in the bf16 storage mode; means something only with bf16 = 1,
  // full_bf16 = 1 and max_positions > 0.  0: per-clip contexts (and wt_transcribe_long_batch), language = -1 and
  // word_timestamps are refused there, as under full_bf16 alone.  1: they run — the ragged bf16 forms of
  // self_attention_long and self_attention_prefill, the detecting chain and the detect_language pre-pass on bf16 weights,
  // and the alignment pass on the bf16 form of align_scores over the ONE bf16 plane of the encoder output.
  long full_bf16_all = 0;
  bool auto_full() const { return full_language != 0 && language < 0 && max_positions > 0; }
  // the long loops' per-clip prompt language of the next full-length calls, with the probability it was detected
  // with: clip b is decoded behind language clip_lang_hold[b] (>= 0) and nothing is detected for it; empty: detect all
  std::vector<int> clip_lang_hold;
  std::vector<float> clip_lang_hold_prob;
  // log-mel + encoder over `batch` host clips, then detect_language: what the long loops call on the first windows
  void detect_windows(const float* pcm, int batch, int32_t* lang, float* prob);
  // Language candidates (wt_engine_set_language_candidates): with a list set every detecting path — detect_language,
  // the 31-position automatic decode, the full-length chains — runs language_head_rows under the list's mask, so
  // probabilities are normalised over the candidates and exactly 0 elsewhere.  n = 0 clears; duplicates allowed; an id
  // outside [0, lang_tokens()) or n > kLangMax: kErrInvalidArg; no language tokens or a Monolith engine: kErrUnsupported.
  std::vector<int> language_candidates;  // distinct, ascending
  void set_language_candidates(const int32_t* langs, int n);
  // option "task": 0 = transcribe, 1 = translate (prompt() puts <|translate|> where <|transcribe|> stands); 1 is
  // kErrUnsupported on an English-only or Monolith engine or with token_translate outside the vocabulary, and a call
  // with a caller prompt is refused while it is set (check_task_call)
  long task = 0;
  void set_task(long value);
  void check_task_call() const;
  // Timestamp decoding.  1: the default prompt ends before <|notimestamps|> and decode_full applies
  // Whisper's timestamp rules on the device (k_timestamps.hip) in place of select_token.  Full-length greedy decoding
  // only: with the option set every decode call outside that scope is kErrUnsupported (check_timestamp_call; with
  // max_positions set, check_full_call and the refusals of the other entry points cover the rest).
  long timestamps = 0;
  long max_initial_timestamp = 50;  // ticks of 20 ms allowed for the first timestamp (Whisper's 1.0 s); -1 = no limit
  // the model's logits reach past <|0.00|>: ids token_beg .. n_vocab - 1 are the timestamps
  bool has_timestamp_tokens() const { return dims_.n_vocab > vocab_.token_beg + 1 && vocab_.token_eot >= 0 && vocab_.token_eot < vocab_.token_beg; }
  // every decode entry point (decode, check_full_args, submit, submit_pcm) calls this first; it therefore also carries
  // the one refusal of option task (check_task_call)
  void check_timestamp_call() const;
  // Decode confidence.  scores = 1: decode_full also forms, on the device inside the chain
  // (k_scores.hip), the log-probability of every generated id under the set it was chosen from, their sum and count per
  // clip, and the no-speech probability of the position-0 row.  Full-length greedy decoding only, with or without
  // timestamps; refused like timestamps outside that scope (check_timestamp_call).  skip_silence = 1 (needs scores):
  // a clip with no_speech_prob > no_speech_threshold / 1000 and not avg_logprob > logprob_threshold / 1000 (Whisper's
  // rule) yields empty text and no segments; its id row is returned as decoded.
  long scores = 0, skip_silence = 0;
  long no_speech_threshold = 600, logprob_threshold = -1000;  // thousandths
  // <|nospeech|> is the id the vocabulary calls token_solm (50361, multilingual 50362); the option needs it below n_vocab
  bool has_no_speech_token() const { return vocab_.token_solm >= 0 && vocab_.token_solm < dims_.n_vocab; }
  // Temperature sampling and fall-back.  temperature (thousandths) > 0 or temperature_fallback = 1:
  // decode_full selects with sample_partial + sample_select (k_sample.hip) in place of select_token / ts_select; the
  // parameters of an attempt (1 / T per clip, seed, attempt, clip_base) reach the kernels through a block in device
  // memory, so the segment graphs serve every attempt.  temperature_fallback = 1 (needs scores): Whisper's
  // decode_with_fallback over the schedule temperature, + temperature_increment, ... <= 1000; a clip is decoded again
  // while compression_ratio > compression_ratio_threshold / 1000 (0 = off) or avg_logprob < logprob_threshold / 1000,
  // unless it is silence (no_speech_prob > no_speech_threshold / 1000 and avg_logprob < logprob_threshold / 1000).
  // Scope and refusals: those of max_positions (check_timestamp_call, check_full_call).
  long temperature = 0, temperature_fallback = 0, temperature_increment = 200, compression_ratio_threshold = 2400;
  long seed = 0;
  long clip_base = 0;  // index of the call's first clip in the Philox counter (wt_transcribe_long_pcm: the window index)
  bool sampling() const { return temperature > 0 || temperature_fallback != 0; }
  // Several samples per clip.  best_of = N > 1: every attempt of a full-length decode whose
  // temperature is above 0 decodes N samples per clip (decode_best_of) and keeps the first with the largest
  // sum_logprob / n_generated in float64, EOT counted; an attempt at temperature 0 draws nothing and runs as ever.
  // With sampling() it is refused (kErrUnsupported, check_full_call) beside a context, seek, word_timestamps,
  // stop_at_eot = 0, the batched seeking entry point and a decoder without the absorbed cross-attention.
  long best_of = 1;
  bool best_of_sampling() const { return best_of > 1 && sampling(); }
  // Beam search inside the fall-back.  It means something only with full_beam = 1 and beam_size
  // 2..8.  0: such a call refuses a temperature and the fall-back (section 23).  1: an attempt at temperature 0 runs
  // the beam chain (beam_full_chains) over all clips, an attempt above 0 runs the sampler with best_of rows per clip and
  // ignores the beam; a fixed temperature > 0 without fall-back is then a sampling call.  The beam chain's own refusals
  // (context, seek, word_timestamps, stop_at_eot = 0, no absorbed cross-attention) and the batched seeking entry
  // point's stand.
  long fallback_beam = 0;
  bool beam_fallback() const { return fallback_beam != 0 && full_beam != 0 && beam_size > 1 && sampling(); }
  // bytes of text / bytes of zlib's compress() of it at the default level, 0 for empty text; zlib is loaded at first
  // use (libz.so.1): kErrUnsupported when it cannot be
  static bool zlib_available();
  static double compression_ratio(const std::string& text);
  long gemm_variant = -1;  // -1 = plane GEMM (per-contraction fall-back to 13/16); 0 = fp32 MFMA, 13 / 16 = three bf16 planes
  // 1 = bf16 STORAGE mode (BASELINE configs[3]): bf16 weights, activations and both KV caches, fp32 accumulation,
  // fp32 residual stream; k_gemm_bf16.hip and the BF variants of the attention / decoder kernels.  Set through
  // set_bf16(): the first switch uploads the bf16 weight copies.
  long bf16 = 0;
  void set_bf16(bool on);
  // encoder kernel-class timers (wt_last_kernel_stats): 0 = off, N = event pairs around every launch of every N-th
  // encoder pass; passes without them report zero launches
  long kernel_timers = 1;
  // non-empty: replaces the reference's hard-coded prompt (test-sized vocabularies)
  std::vector<long long> prompt_override;
  // test tap (wt_dbg_set_forced_ids): id rows [clips][32] every decode of exactly that many clips follows instead of its
  // own argmax (the argmax still runs: logits, counts and the EOT rule are unchanged); empty = off
  std::vector<long long> forced_ids;
  // ids the decoder starts from (prompt_override, or the reference's rule for the engine type)
  std::vector<long long> prompt() const;
  // A context in front of the prompt: Whisper's initial_prompt / condition_on_previous_text.  The
  // engine keeps the LAST context_keep() = n_text_ctx / 2 - 1 ids of what set_context is given (n = 0 clears; more than
  // kContextIdsMax ids or one outside the vocabulary: kErrInvalidArg; a vocabulary without <|startofprev|> or a Monolith
  // engine: kErrUnsupported) and decode_full feeds fed_prompt() = [prev] + context + prompt(): every count of the decode
  // — sample_begin, n_gen, the timestamp-rule state, the scores — starts behind all of it, and the no-speech
  // probability is read behind sot, wherever that is.  The prompt passes then take kDecRowsMax / batch positions each on
  // self_attention_prefill (prompt_group = 1: one position each), and the call runs eagerly: a context's length is a
  // launch constant of every pass, so its segments are not captured and graphs_cached() does not grow with the lengths seen.
  // Scope: wherever max_positions decoding is; every other decode call with a context set is kErrUnsupported
  // (check_timestamp_call, check_full_call), a prompt that leaves no position to generate kErrInvalidArg.
  static constexpr int kContextIdsMax = 4096;
  std::vector<long long> context_ids;
  int context_keep() const { return std::max(0, dims_.n_text_ctx / 2 - 1); }
  bool has_prev_token() const { return !monolith_ && vocab_.token_prev >= 0 && vocab_.token_prev < dims_.n_vocab; }
  void set_context(const int64_t* ids, int n);
  std::vector<long long> fed_prompt() const;
  long prompt_group = 0;
  // Per-clip contexts: clip b of every following full-length call is decoded behind
  // clip_contexts[b] (each cut to its last context_keep() ids; an empty one: that clip's fed prompt is prompt() alone).
  // The call's batch must equal their number.  Such a call is one RAGGED chain: the clips' fed prompts are right-aligned
  // in slots, clip b at Whisper position slot - start_b, so every clip starts generating at the same slot and only the
  // embedding, the self-attention and the sampler's counter see the per-clip position.  Runs eagerly, as a context does.
  // n_clips = 0 clears; setting either kind of context clears the other.  Refusals: set_context's, more than 64 clips
  // (kErrInvalidArg), word_timestamps (kErrUnsupported).
  std::vector<std::vector<long long>> clip_contexts;
  // the sampler's clip word of clip b is clip_base + b + clip_index_off[b] (empty: zeros); the batched seeking loop sets it
  std::vector<int> clip_index_off;
  void set_contexts(const int64_t* ids, const int32_t* offsets, int n_clips);
  std::vector<long long> fed_prompt_of(int clip) const;  // [prev] + clip_contexts[clip] + prompt(), or prompt() alone
  int graphs_cached() const { return int(graphs_.size()); }
  // Logit suppression: Whisper's SuppressTokens / SuppressBlank in front of every other decoding
  // rule of a full-length chain.  suppress_ids are masked at every generated position, suppress_first_ids at the first
  // one (n_gen == 0, behind the whole fed prompt).  set_suppress uploads both into ONE device buffer (always-ids, then
  // first-ids) that suppress_logits reads at run time: the counts are launch constants and part of the graph keys, the
  // contents are not.  0 .. kSuppressIdsMax ids per list, duplicates allowed; an id outside the model's vocabulary or EOT
  // among suppress_ids (the allowed set must never be empty): kErrInvalidArg; a Monolith engine: kErrUnsupported.
  // n = n_first = 0 clears, and every launch sequence, graph key and workspace is then what it is without the feature.
  // Scope: wherever max_positions decoding is (check_timestamp_call, check_full_call).
  std::vector<long long> suppress_ids, suppress_first_ids;
  bool suppressing() const { return !suppress_ids.empty() || !suppress_first_ids.empty(); }
  void set_suppress(const int64_t* ids, int n, const int64_t* first_ids, int n_first);
  void set_suppress_default(bool on);  // option suppress_default: host_util's default_suppress over the model's ids
  // Seeking long-audio transcription (wt_transcribe_long_pcm with seek = 1, longform.cpp): needs timestamps and
  // max_positions; condition_on_previous_text is read only then
  long seek = 0, condition_on_previous_text = 1;
  // Word-level timestamps.  word_timestamps = 1 (needs timestamps = 1, max_positions and the absorbed
  // cross-attention: check_word_call): after the decode, and after the fall-back loop, decode_full feeds every clip's
  // row prompt() + [<|notimestamps|>] + text + [eot] through the decoder once more, teacher-forced, keeps the
  // cross-attention weights of the alignment heads (align_scores), turns them into a cost matrix and a DTW path on the
  // device (k_align.hip) and cuts the path into words on the host (words.cpp).
  long word_timestamps = 0;
  // measurement and test handles (wt_dbg_set_alignment): keep what the pass formed per clip; the form of align_scores (0
  // fused softmax, 1 frame chunks + row kernel); clips per sub-group (0 = as many as kAlignWeightBytes allows)
  long keep_alignment = 0, align_mode = 1, align_sub = 0;
  std::vector<std::pair<int, int>> alignment_heads;  // (layer, head) pairs set by the caller; empty = Whisper's default
  // n = 0 restores the default: every head of the layers n_text_layer / 2 .. n_text_layer - 1.  kErrInvalidArg for a pair
  // outside the model, a duplicate or more than kAlignHeadsMax pairs.
  void set_alignment_heads(const int32_t* layer_head, int n);
  std::vector<std::pair<int, int>> alignment_heads_in_effect() const;  // sorted by (layer, head)
  void check_word_call() const;  // throws kErrUnsupported when word_timestamps is set outside its scope
  // The alignment pass over the id rows the last decode_full left on the host: segs = the segments whose ids below EOT
  // are the clips' text (clip = index in that call, id_begin an index into the clip's id row), valid_samples = the
  // samples of every clip (empty: full length).  Fills last.words (segment = index into segs) and, with keep_alignment,
  // appends to last.alignment.  decode_full calls it with its own segments unless defer_word_alignment is set: the
  // seeking loop sets that and aligns each window over the segments seek_step kept.
  void align_words(int batch, const std::vector<Segment>& segs, const std::vector<long long>& valid_samples);
  bool defer_word_alignment = false;

  int mel_frames() const { return 2 * dims_.n_audio_ctx; }
  size_t mel_elems() const { return size_t(dims_.n_mels) * mel_frames(); }
  size_t pcm_elems() const { return size_t(mel_frames()) * 160; }

  // d_pcm [B][pcm_elems] -> d_mel [B][n_mels][frames]; device pointers, async on stream().  valid_frames >= 0:
  // the normalisation maximum runs over frames [0, valid_frames) only (a clip shorter than the window)
  // d_raw (test tap, wt_dbg_frontend_stages): device [B][n_mels][frames] that receives the log-mel as log_clipmax left
  // it, copied out before mel_normalize works on d_mel in place; the launches are the same with and without it
  void logmel(const float* d_pcm, int batch, float* d_mel, int valid_frames = -1, float* d_raw = nullptr);
  // what logmel() left in the front end's workspace and the tables it contracts against (test tap); device pointers are
  // valid after a logmel() call, until the batch capacity grows
  struct FrontendView {
    const unsigned short* pcm_planes = nullptr;  // hi [clip][pcm_stride], lo at + pcm_plane
    long pcm_plane = 0, pcm_stride = 0;
    float pcm_scale = 1.0f;
    const float* pw = nullptr;         // [B * frames][pw_ld]
    const float* melacc = nullptr;     // [B * frames][mel_n]
    const unsigned* clip_max = nullptr;  // [(b * kClipMaxWays + w) * kClipMaxStride]
    int pw_ld = 0, mel_n = 0, mel_k = 0, dft_n = 0, dft_k = 0;
    const float* basis = nullptr;      // host, [dft_n][dft_k] fp32 (what the basis planes were split from)
    const float* mel_matrix = nullptr;  // host, [mel_n][mel_k]
  };
  FrontendView frontend_view() const;
  // d_mel -> encoder output (internal) -> cross KV cache of the next pipeline slot; async on
  // the encoder stream
  void encode(const float* d_mel, int batch);
  // greedy loop over the slot encode() just filled, on the decoder stream; synchronises and
  // returns ids [B][32], n [B].
  void decode(int batch, int64_t* ids, int32_t* n_ids, float* logits_host, int logits_steps_cap);
  // Pipeline, kSlots deep: submit() enqueues encoder (stream E) + decoder (one of the three
  // decoder streams in use, in rotation) for one batch and returns.  In steady state the MFMA-bound
  // encoder of the newest batch shares the chip with the latency-bound decoder chains of the
  // previous ones: a decoder's ~1000 tiny dependent launches leave most of the chip idle on
  // their own.  collect() waits for the OLDEST submitted batch.
  void submit(const float* d_mel, int batch);
  // same from PCM: the front end runs on the pipeline's encoder stream into the staging mel buffer
  void submit_pcm(const float* d_pcm, int batch);
  void collect(int64_t* ids, int32_t* n_ids);
  int in_flight() const { return int(inflight_.size()); }
  // contractions that were given the full-range bf16 three-plane kernels at load time (bound slack, engine.cpp)
  int f16_fallbacks() const { return n_f16_fallbacks_; }
  float f16_min_slack_bits() const { return f16_min_slack_bits_; }
  int f16_contractions() const { return int(load_ok_.size()); }
  // what upload_weights derived per contraction, in the order of force_fallback's bits (engine.cpp; wt_dbg_encoder_scales)
  std::vector<std::array<float, 10>> encoder_scales() const;
  // Test hook (option "force_fallback"): bit i treats contraction i — launch order: conv1, conv2, then per layer
  // qkv, attention, out, fc1, fc2, and last the cross-KV projection — as flagged by the load-time slack check, on top
  // of the contractions that check flagged itself.  Exercises every plane <-> fall-back hand-over on any weights.
  void set_force_fallback(long mask);
  long force_fallback() const { return force_fallback_; }
  // throws unless no submitted batch is waiting for collect(): every synchronous entry point calls it first
  void require_idle() const;
  void sync();
  // makes this engine's GPU the calling thread's current device (every C-ABI entry does it)
  void bind_device();

  const float* enc_out() const { return ws_.enc_out; }
  void ensure_batch(int batch);
  float* staging_mel(int batch);  // device buffer [B][mel_elems]
  float* staging_pcm(int batch);  // device buffer [B][pcm_elems]
  float* upload_pcm(const float* pcm, int batch);  // host [B][pcm_elems] -> staging_pcm(batch), async on stream()
  // `batch` host windows, already padded, through the front end, the encoder and the decoder: encode_full + decode_full
  // (valid_samples as decode_full takes them) into rows of max_positions + 1 ids when max_positions is set, else
  // encode + decode into rows of 32.  Synchronises every stream: pcm may be freed on return.
  void decode_windows(const float* pcm, int batch, const std::vector<long long>* valid_samples, std::vector<int64_t>* ids,
                      std::vector<int32_t>* n_ids);

  // test tap: `n_dec` decodes (slots 0..n_dec-1, whose cross-KV caches must hold a previous batch) next
  // to `n_enc` pipelined encoder passes; device time of each decode and of the encoder passes together
  void debug_concurrency(const float* d_mel, int batch, int n_dec, int n_enc, float* dec_ms, float* enc_ms);
  // raw device allocator for debug entry points
  float* dalloc(size_t n_floats);

  // Resolved by decode()/sync_stats(); index = KernelClass.
  const KernelStat* kernel_stats() const { return kstats_; }

 private:
  void open_device();     // selects the GPU, checks it is gfx950
  void create_streams();  // streams, events, pinned id buffers of the pipeline slots
  void release() noexcept;  // frees every device / host resource; idempotent (destructor and failed constructor)
  void upload_weights(const std::string& path);
  void ensure_bf16_weights();
  std::string weights_path_;
  bool bf16_ready_ = false;
  const float* dev(const std::string& name) const;
  float* upload(const std::vector<float>& host);
  TiledW upload_tiled(const float* W, int N, int K);
  void build_frontend_tables();

  // group > 1: the decoder chain takes the batches (same size) of `group` consecutive slots from `slot` together
  void decode_enqueue(int batch, int slot, float* logits_host, int logits_steps_cap, int group = 1, bool pipelined = false,
                      int stream_override = -1);
  void submit_decoder(int batch, int slot);  // decoder side of submit / submit_pcm: grouped, alone, or latency form
  int group_of(int batch) const;             // batches per decoder chain for pipelined batches of this size
  int n_spare_streams_ = 0;  // probe-selected decoder streams beyond n_dec_streams_ (latency form of the last batches)
  bool pipelined_call_ = false;  // set by select_stream: the batch being enqueued belongs to submit(), not to a synchronous call
  std::vector<int> pending_;  // consecutive slots submitted, encoder enqueued, decoder waiting for the rest of their group
  void flush_pending();
  void decode_collect(int slot, int64_t* ids, int32_t* n_ids);
  void finish_slot(int slot);  // decode_collect without the id rows: wait, non-finite flag, statistics, timings
  // beam search over the slot encode() just filled: consecutive chains of <= 128 / beam_size clips on one decoder stream
  void decode_beam(int batch, int slot_idx, int64_t* ids, int32_t* n_ids);
  struct BeamWorkspace {  // allocated on the first beam call, sized for 128 rows and 64 clips whatever the batch
    float* kv[2] = {nullptr, nullptr};          // self-attention caches [layer][k|v][row][cap][d], double-buffered
    long long* ids[2] = {nullptr, nullptr};     // id rows [128][32], double-buffered with them
    float* logits = nullptr;                    // [128][n_vocab]
    unsigned long long* best = nullptr;         // the logits GEMM's argmax records (unused here, written anyway)
    BeamPart* part = nullptr;                   // [128][chunks]
    int* parent = nullptr;
    long long* token = nullptr;
    float *live_sum = nullptr, *fin_sum = nullptr, *out_sum = nullptr;
    int *fin_tok = nullptr, *fin_len = nullptr, *n_fin = nullptr, *done = nullptr, *out_n = nullptr, *out_len = nullptr;
    long long* out_ids = nullptr;
    long long* h_prompt = nullptr;  // pinned [64][32]: the prompt rows a chain starts from
    float* h_sum = nullptr;         // pinned [64]
    int* h_len = nullptr;           // pinned [64]
  } bw_;
  void ensure_beam_workspace();
  // the chain behind decode_full when beam_size > 1 and full_beam = 1: consecutive chains of <= 128 / beam_size clips
  void decode_beam_full(int batch, int64_t* ids, int ids_stride, int32_t* n_ids);
  // its chains alone: the results stay in bf_'s pinned mirrors (h_ids, h_lp, h_n, h_len, h_sum, h_nosp); adds the
  // decoder steps to `steps`; first: the call's first chain records the slot's dec_begin
  void beam_full_chains(int batch, bool first, int& steps);
  struct BeamFullWorkspace {  // allocated on the first full-length beam call, sized for 128 rows and 64 clips
    float* kv = nullptr;                         // ONE self-attention cache [layer][k|v][128][full_cap()][d]: K / V never move
    long long* ids[2] = {nullptr, nullptr};      // id rows [128][full_cap() + 1], double-buffered
    float* lp[2] = {nullptr, nullptr};           // their log-probabilities, likewise
    unsigned char* anc[2] = {nullptr, nullptr};  // ancestor tables [128][full_cap()], likewise
    float* logits = nullptr;                     // [128][ldl], rows 16-byte aligned
    int ldl = 0;
    unsigned long long* best = nullptr;          // the logits GEMM's argmax records (unused here, written anyway)
    BeamFullPart* part = nullptr;                // [128][chunks]
    TsState* ts = nullptr;                       // [128]
    int *n_live = nullptr, *fin_tok = nullptr, *fin_len = nullptr, *n_fin = nullptr, *done = nullptr, *parent = nullptr;
    double *live_sum = nullptr, *fin_sum = nullptr, *out_sum = nullptr;
    float *fin_lp = nullptr, *tok_lp = nullptr, *out_lp = nullptr;
    long long *token = nullptr, *out_ids = nullptr;
    int *out_n = nullptr, *out_len = nullptr;
    ScorePart* sc_part = nullptr;                // option scores: the no-speech probability's records [64][chunks]
    float* nosp = nullptr;                       // [64]
    long long *h_prompt = nullptr, *h_ids = nullptr;  // pinned: the prompt rows [64][stride], the results
    float *h_lp = nullptr, *h_nosp = nullptr;
    double* h_sum = nullptr;
    int *h_n = nullptr, *h_len = nullptr, *h_done = nullptr;
  } bf_;
  void ensure_beam_full_workspace();
  // One attempt of decode_full's fall-back loop at a temperature above 0 with best_of = N > 1: consecutive chains of
  // <= 128 / N clips on bf_'s cache, rows j * nc + c, each ended by best_of_pick; the kept rows land in the mirrors
  // the loop merges from (fw_.h_ids, h_n, and with scores h_lp, h_sum, h_count, h_nosp).  frozen: clips that need no
  // result.  Adds the attempt's decoder steps to `steps`.
  void decode_best_of(int batch, const std::vector<long long>& prompt, const std::vector<int>* frozen, bool first, int& steps);
  struct BestOfWorkspace {  // beside bf_, allocated on the first such call: per row [128], per clip [64]
    ScorePart* sc_part = nullptr;    // [128][chunks]
    SamplePart* sm_part = nullptr;   // [128][chunks]
    int *n_ids = nullptr, *finished = nullptr, *count = nullptr;  // [128]
    double* sum = nullptr;           // [128]
    int *frozen = nullptr, *out_count = nullptr, *picked = nullptr, *all_count = nullptr;  // [64], all_count [64][8]
    double* all_sum = nullptr;       // [64][8]
    int *h_frozen = nullptr, *h_fin = nullptr, *h_picked = nullptr, *h_all_count = nullptr;  // pinned
    double* h_all_sum = nullptr;
  } bo_;
  void ensure_best_of_workspace();
  struct FullWorkspace {  // allocated on the first full-length call
    float* kv = nullptr;            // self-attention caches [layer][k|v][clip][full_cap()][d] for kv_clips clips
    int kv_clips = 0;               // the largest batch of a full-length call so far
    long long* ids = nullptr;       // id rows [64][full_cap() + 1]
    long long* h_ids = nullptr;     // pinned mirror of the id rows
    int *h_n = nullptr, *h_fin = nullptr;  // pinned [64]: id counts, finished flags after a segment
    // option timestamps (allocated on the first such call): the logits of a step [64][ts_ldl], rows 16-byte aligned,
    // the per-chunk records [64][ts_chunks(n_vocab)] and the carried state [64]
    float* ts_logits = nullptr;
    int ts_ldl = 0;
    TsPart* ts_part = nullptr;
    TsState* ts_state = nullptr;
    // option scores (allocated on the first such call; it shares ts_logits): the per-chunk records [64][chunks], the
    // token log-probabilities [64][full_cap() + 1], the carried sums and counts [64], the no-speech probabilities [64],
    // and their pinned mirrors
    ScorePart* sc_part = nullptr;
    float *sc_lp = nullptr, *sc_nosp = nullptr, *h_lp = nullptr, *h_nosp = nullptr;
    double *sc_sum = nullptr, *h_sum = nullptr;
    int *sc_count = nullptr, *h_count = nullptr;
    // sampling (allocated on the first such call; it shares ts_logits): the per-chunk records [64][chunks], the
    // parameter block and its pinned mirror
    SamplePart* sm_part = nullptr;
    SampleParams *sm_prm = nullptr, *h_prm = nullptr;
    // suppression without sampling or timestamps: the greedy step runs on the sampler's kernels at T = 0 under a
    // parameter block of zeros that is never written again (it shares ts_logits and sm_part)
    SampleParams* zero_prm = nullptr;
  } fw_;
  int* d_suppress_ = nullptr;  // [2 * kSuppressIdsMax]: the always-ids, then the first-ids (set_suppress)
  // suppress_logits over `rows` rows of a chain's logits; first: the step behind the fed prompt (n_gen == 0)
  void enqueue_suppress(float* logits, int ldl, int rows, bool first, hipStream_t st);
  // what SampleArgs, ScoreArgs and TsSelectArgs share in every chain: the logits rows and the model's constants
  template <class Args>
  void fill_rule_args(Args& a, const float* logits, int ldl) const {
    a.logits = logits; a.ldl = ldl; a.V = dims_.n_vocab;
    a.eot = vocab_.token_eot; a.beg = vocab_.token_beg; a.max_initial = int(max_initial_timestamp);
  }
  // What a full-length chain left on the host, for publish_full: id rows and token log-probabilities [clip][stride], id
  // counts, and per clip the sum and count of the log-probabilities and the no-speech probability (read with scores)
  struct FullResult {
    const long long* ids = nullptr;
    int stride = 0;
    const int* n = nullptr;
    const float* lp = nullptr;
    const double* sum = nullptr;
    const int* count = nullptr;
    const float* nosp = nullptr;
    std::function<int(int)> n_prompt;  // clip -> the ids of its fed prompt
  };
  // the caller's id rows and counts, and the scores and segments groups of `last` as the options ask: scores first, the
  // segment pass reads `skipped`
  void publish_full(const FullResult& r, int batch, int64_t* ids, int ids_stride, int32_t* n_ids);
  // Whisper's two silence tests on (no_speech_prob, avg_logprob).  They differ where avg_logprob equals the threshold:
  // transcribe() skips a clip unless avg > threshold (below = false), decode_with_fallback exempts a clip from another
  // attempt only when avg < threshold (below = true)
  bool silent(float no_speech_prob, float avg_logprob, bool below) const;
  static constexpr int kFullClipsMax = 64;  // rows of the full-length and the ragged id tables (a call's clips at most)
  void ensure_full_workspace(int batch);
  struct RaggedWorkspace {  // allocated by the first ragged call: the slot-space rows [64][ragged_stride()] and the starts [64]
    long long *ids = nullptr, *h_ids = nullptr;
    float *lp = nullptr, *h_lp = nullptr;  // option scores
    int *start = nullptr, *h_start = nullptr;
  } rw_;
  // a ragged chain runs at most N - min n_b + P < 2 full_cap() slots, and a selection writes the id of the slot behind it
  int ragged_stride() const { return 2 * full_cap() + 2; }
  void ensure_ragged_workspace();
  struct AlignWorkspace {  // allocated by the first call with word_timestamps, outside any capture
    float *W = nullptr, *stats = nullptr, *C = nullptr;
    size_t w_elems = 0, c_elems = 0, s_elems = 0;
    unsigned char* trace = nullptr;
    int *jump = nullptr, *lfn = nullptr;  // [64][kAlignRowsMax]; L | F | N [3][64]
    int *h_jump = nullptr, *h_lfn = nullptr;  // pinned mirrors
  } aw_;
  static constexpr size_t kAlignWeightBytes = size_t(256) << 20;  // bound of the weight workspace: clips go through in sub-groups
  static constexpr long long kFullKey = -1000;  // first entry of a full-length segment's graph key
  static constexpr long long kBeamFullKey = -2000;  // ... and of a full-length beam segment's
  static constexpr long long kBestOfKey = -3000;    // ... and of a best-of segment's
  // last entry of those three keys in the bf16 storage mode (option full_bf16), absent in fp32: the entries a key may end
  // with otherwise (suppression's two counts, the detecting chain's 1 or 2, the flags) are never negative
  static constexpr long long kBf16KeyMark = -16;

  int enc_cus_masked_ = 0;  // CUs the pipelined encoder stream may use
 public:
  int pipelined_encoder_cus() const { return enc_cus_masked_ > 0 ? enc_cus_masked_ : n_cu_; }
 private:
  int device_ = 0, n_cu_ = 0, reserve_ = 0;  // reserve_: CUs per XCD the pipelined encoder stream leaves free
  bool monolith_ = false, multilingual_ = true;
  hipStream_t stream_ = nullptr;   // encoder + front end: stream_full_ or stream_masked_ (select_stream)
  hipStream_t stream_full_ = nullptr, stream_masked_ = nullptr;
  hipEvent_t ev_switch_ = nullptr;
  void select_stream(bool pipelined);
  void pick_decoder_streams();  // decoder streams that do not share a hardware queue with the encoder stream
  // The encoder's one launch sequence, for the plane kernels, their per-contraction fall-back and bf16 storage mode
  // alike: every contraction is described once and takes its kernel from its EncLinear record and the mode.
  // default encoder GEMM: the k16 split kernel in its two-plane fp16 form, at 2 blocks per CU when decoders
  // share the chip (pipelined), at 3 blocks per CU otherwise
  void encode_enqueue(const float* d_mel, int batch);
  // slots (WT_PIPELINE_DEPTH): a multiple of 1, 2, 3 and 4 times the 3 decoder streams in use, so single batches AND
  // group leaders (every second / third / fourth slot) rotate evenly over them; a group's chain holds its slots for
  // several pipeline periods, so the encoder needs that many slots ahead of it to keep running
  static constexpr int kDecStreams = 8, kSlots = 24;
  int n_dec_streams_ = 3;  // decoder streams in use: one hardware queue each (the runtime multiplexes
                           // streams onto 4 queues per priority; two decoders sharing one serialise)
  hipStream_t dstream_[kDecStreams] = {};  // decoders (batches rotate over them)
  static constexpr int kEncAsDec = kDecStreams;  // decoder-stream index meaning "the pipelined encoder stream" (submit_decoder)
  hipStream_t dec_stream_at(int i) const { return i == kEncAsDec ? (stream_masked_ ? stream_masked_ : stream_full_) : dstream_[i]; }
  hipEvent_t ev_[2] = {nullptr, nullptr};  // front end begin / end
  struct Slot {
    float* cross_kv = nullptr;  // [layer][k|v][clip][head][t][64]
    unsigned short* e_planes = nullptr;  // absorbed cross-attention: planes of the encoder output [clip][T][d]
    bool absorbed = false;               // which of the two this slot's encoder pass filled
    int pair_leader = -1;  // decoded by another slot's chain (which copies this batch's ids into THIS slot's buffers)
    hipEvent_t enc_begin = nullptr, enc_mid = nullptr, enc_done = nullptr;
    hipEvent_t dec_begin = nullptr, dec_done = nullptr;
    long long* h_ids = nullptr;  // pinned [4096][32]
    int* h_n = nullptr;          // pinned [4096]
    int *h_flag = nullptr, *d_flag = nullptr;  // non-finite encoder output (pinned copy / device word)
    int batch = 0, steps = 0, dec = 0;  // dec: decoder stream / workspace of this batch
    bool used = false;
    std::vector<hipEvent_t> kt_events;
    std::vector<hipEvent_t> dt_events;  // WT_DEC_KERNEL_TIMERS diagnostics
    std::vector<int> dt_cls;
    std::vector<int> kt_cls;
    std::vector<double> kt_flops, kt_bytes;
  } slots_[kSlots];
  struct GraphEntry {
    hipGraphExec_t exec;
    int steps;
  };
  void need_cross_kv(Slot& slot);  // the cached decoder form's cross K/V cache of a slot, on first use
  std::map<std::vector<long long>, GraphEntry> graphs_;
  // Replays the graph cached under `key` on `st`, or runs enqueue() eagerly (which also performs the kernels' one-time
  // set-up) and, with `graphs`, captures it for the next calls; returns the steps enqueue() counted.  A failed capture
  // is not fatal: use_graphs drops to 0 and the message names the chain by `label`.  Every chain but decode_enqueue's
  // (all slots or none) goes through it.
  int replay_or_capture(const std::vector<long long>& key, hipStream_t st, bool graphs, const char* label,
                        const std::function<int()>& enqueue);
  struct DonePoll {  // "all done?" after a segment: n device flags and their pinned mirror; flags = nullptr: never asked
    const int* flags = nullptr;
    int n = 0;
    int* mirror = nullptr;
  };
  // A full-length chain's segments [lo, hi) of 32 positions up to `len`, each through replay_or_capture under
  // key_of(lo) with graphs = use_graphs && capturable, read again for every segment; adds the steps to `steps`.  Stops
  // behind the segment after which every flag of `poll` is set and returns that segment's hi (len: the chain ran out).
  int run_segments(int len, hipStream_t st, bool capturable, const char* label,
                   const std::function<std::vector<long long>(int)>& key_of,
                   const std::function<int(int, int)>& enqueue_segment, const DonePoll& poll, int& steps);
  hipEvent_t trace_base_ = nullptr;  // WT_TRACE_PIPELINE=1: origin of the per-batch device timeline
  int enc_slot_ = 0;        // slot the next encode() fills
  int last_enc_slot_ = 0;   // slot the last encode() filled
  std::vector<int> inflight_;
  wtw::Dims dims_{};
  VocabData vocab_;
  FilterBank filters_;
  Timings timings_;
  bool have_logmel_ = false;

  std::vector<void*> allocations_;  // device memory, freed by release()
  std::vector<void*> pinned_;       // pinned host memory, likewise
  void* dev_zeroed_bytes(size_t bytes);
  void* pinned_bytes(size_t bytes);
  // n zero-filled elements of device memory / n elements of pinned host memory, owned by the engine until release()
  template <class T> T* dev_zeroed(size_t n) { return static_cast<T*>(dev_zeroed_bytes(n * sizeof(T))); }
  template <class T> T* pinned(size_t n) { return static_cast<T*>(pinned_bytes(n * sizeof(T))); }
  std::map<std::string, const float*> tensors_;  // raw tensors by .wtw name

  // derived, re-laid-out weights
  // The encoder's contractions, one record each: conv1 and conv2 as implicit GEMMs ([co][kk * ci], fill_enc_linears),
  // the layers' four, and the cross K/V projections of all decoder layers as one matrix [L*2*d][d]
  EncLinear conv1_, conv2_, cross_kv_;
  std::vector<EncLayer> enc_layers_;
  const unsigned short* upload_planes(const float* W, int N, int K, int Kpad, float scale);
  const float* enc_pos = nullptr;
  std::vector<DecBlockWeights> dec_blocks_;
  std::vector<DecBlockWeights> dec_blocks_bf_;  // bf16 storage mode: TiledW members are single bf16 planes
  TiledW tok_emb_tiled_bf_;
  // Per contraction: the plane kernels unless the load-time slack check gave that contraction the full-range form
  // (GemmScale::f16_ok) or an explicit gemm_variant / attn_variant selects the fp32-storage kernels for all of them
  bool gemm_on_planes(const GemmScale& sc) const { return gemm_variant < 0 && sc.f16_ok; }
  static constexpr float kMelBound = 8.0f;
  static constexpr float kF16Slack = 4096.0f;  // largest bound / typical ratio the two-plane fp16 form is used for
  int n_f16_fallbacks_ = 0;
  float f16_min_slack_bits_ = 0.0f;  // smallest log2(kF16Slack * typical / bound) over the checked operands (load time)
  long force_fallback_ = 0;
  std::vector<bool> load_ok_;  // the slack check's own verdicts, in contraction order (set_force_fallback)
  std::vector<std::array<float, 6>> load_ops_;  // beside load_ok_: {largest bound, typical} of up to three operands
  std::vector<bool*> ok_flags();  // the records' f16_ok / attn_f16_ok in that order: a walk in launch order
  // the fp32-storage GEMM a contraction falls back to: the forced variant, else three bf16 planes (13; 16 = the same
  // at two blocks per CU beside the decoders of the pipeline)
  int alt_gemm_variant() const {
    if (gemm_variant >= 0) return int(gemm_variant);
    return (stream_ == stream_masked_ && stream_masked_) ? 16 : 13;
  }
  const float *enc_ln_post_g = nullptr, *enc_ln_post_b = nullptr;
  const float *tok_emb = nullptr, *dec_pos = nullptr, *dec_ln_g = nullptr, *dec_ln_b = nullptr;
  TiledW tok_emb_tiled;  // logits GEMM against the tied embedding
  // front end
  const unsigned short* dft_basis_p_ = nullptr;  // [dft_n][dft_k] windowed basis, rows (2 k, 2 k + 1) = (re, im) of bin k, as fp16 planes
  const float* dft_zero_bias_ = nullptr;
  float dft_w_scale_ = 1.0f;
  int pw_ld_ = 0;                    // row stride of the power spectrum (dft_n / 2)
  long pcm_plane_ = 0;               // elements between the hi and the lo plane of the PCM workspace
  static constexpr float kPcmBound = 32.0f;  // PCM is clamped to +-32 for the fp16 planes (audio lives in +-1)
  const float* mel_w = nullptr;      // [mel_n][mel_k]
  std::vector<float> dft_basis_host_, mel_w_host_;  // the fp32 tables the device copies were made from (frontend_view)
  int dft_n = 0, dft_k = 0, mel_n = 0, mel_k = 0;

  struct DecWorkspace {  // one per decoder stream
    float *xb = nullptr, *xpart = nullptr;  // fc2's K-split: first-half result / second-half partial
    float *xd = nullptr, *qkvd = nullptr, *attd = nullptr,
          *hd = nullptr, *cross_ws = nullptr, *self_kv = nullptr, *logits = nullptr;
    float *qp = nullptr, *abs_ws = nullptr, *cabs = nullptr;  // absorbed queries, per-chunk records, combined contexts
    unsigned long long* best = nullptr;
    long long* ids = nullptr;
    int *n_ids = nullptr, *finished = nullptr;
  } dws_[kDecStreams + 1];  // one per decoder stream, + one for a chain on the encoder stream (kEncAsDec)
  // What a decode chain may vary in a decoder pass (decoder_pass: the one launch sequence of the decoder layers)
  struct AlignSink {  // where a teacher-forced pass leaves the attention weights of the alignment heads
    float* W = nullptr;  // [B][heads_total][L_max][ldw]
    int heads_total = 0, L_max = 0, ldw = 0;
    int F[64] = {};                                            // valid frames of the pass's clips (kAlignClipsMax)
    std::vector<std::vector<std::pair<int, int>>> layer;       // per decoder layer: (head, slot in W's head axis)
  };
  struct DecPass {
    const AlignSink* align = nullptr;  // set: align_scores runs on dw.qp right after the qa GEMM of a layer that owns heads
    int pos0 = 0, np = 1;  // positions pos0 .. pos0 + np - 1
    int B = 0;             // rows per position (sequences): M = np * B rows, row = p * B + sequence
    const long long* ids = nullptr;  // id rows [B][ids_stride]
    float* self_kv = nullptr;        // self-attention caches [layer][k|v][B][self_cap][d] (bf16 elements when bf)
    int ids_stride = 32, self_cap = 32;
    bool self_long = false;  // self_attention_long (np = 1, any position below self_cap) instead of self_attention
    bool self_prefill = false;  // self_attention_prefill (np >= 1: a prompt behind a context) instead of either
    // full-length beam search: the cache holds self_rows >= B rows per slab (0: B), and with self_anc set every pass runs
    // the gathered form of self_attention_long over the B rows (np = 1), row r reading key k from row self_anc[r][k]
    int self_rows = 0;
    const unsigned char* self_anc = nullptr;
    // ragged chain: pos0 counts slots, sequence b is at Whisper position slot - pos_start[b] (device [B]) and may feed
    // positions [0, pos_limit); the embedding and the ragged self-attention kernels take both (self_prefill or the long form)
    const int* pos_start = nullptr;
    int pos_limit = 0;
    int clips = 0;           // clips the cross-attention sees: B, or fewer with M / clips query rows each (beam search)
    bool absorbed = false;   // cross-attention form: absorbed (e .. e4, e_split, n_abs) or cached (cross_kv, chunks)
    const unsigned short *e = nullptr, *e2 = nullptr, *e3 = nullptr, *e4 = nullptr;  // as in CrossAbsorbedArgs
    int e_split = 0, n_abs = 1, chunks = 1;
    float* cross_kv = nullptr;
    bool bf = false, split = false;  // bf16 storage mode; fc2 K-split (x is handed on as xb + xpart)
    const DecWorkspace* dw = nullptr;
    // best set: the final LayerNorm + logits GEMM of the last position's rows follows the layers (Y null: records only)
    unsigned long long* best = nullptr;
    float* Y = nullptr;
    int ldy = 0, logits_blocks = 0;
    DecTimers* timers = nullptr;  // per-launch event pairs: greedy's eager launches under WT_DEC_KERNEL_TIMERS
  };
  void decoder_pass(const DecPass& p, hipStream_t st);
  int cross_chunks_for(int batch) const;              // key chunks of the cached cross-attention (option cross_chunks)
  int abs_chunks_for(int clips, int blocks) const;    // key chunks of the absorbed one for ~`blocks` blocks (option abs_chunks)
  bool fc2_split() const { return fc2_ksplit == 2 && (4 * dims_.n_text_state) % 256 == 0; }
  void check_prompt_ids(const std::vector<long long>& prompt, int code) const;  // throws Error(code, ..) outside the vocabulary
  // language_head outputs, one set per decoder workspace (128 rows whatever the batch), and the pinned copies a
  // synchronous call reads; allocated by the first detecting call
  struct LangWorkspace {
    float *probs = nullptr, *prob = nullptr;  // [128][kLangMax], [128]
    int* lang = nullptr;                      // [128]
  } lw_[kDecStreams + 1];
  float *h_lang_probs_ = nullptr, *h_lang_prob_ = nullptr;
  int* h_lang_ = nullptr;
  void ensure_lang_workspace();
  bool detect_only_ = false;  // set by detect_language() around its decode_enqueue
  unsigned* d_lang_allow_ = nullptr;  // [4]: the candidate mask language_head_rows reads (set_language_candidates)
  struct FullLangWorkspace {  // option full_language: allocated by the first detecting full-length call
    int *hold = nullptr, *h_hold = nullptr;  // [64] device / pinned: the clips' held languages, -1 = detect
    long long* sot_ids = nullptr;            // [64][1]: the id rows of the pass over [sot] in front of a context
  } fl_;
  void ensure_full_language_workspace();
  // full_language: the language every clip of the running (or last) decode_full is decoded behind, for the chains and
  // passes that build id rows on the host: beam_full_chains, decode_best_of, align_words.  Empty: the option language.
  std::vector<int> call_lang_;
  // language_head_rows over the `batch` position-0 rows a decoder pass has just left in dw: the language of every clip
  // into column id_pos of ids [kFullClipsMax][stride] (fw_.ids or rw_.ids) and into lw_ / the pinned mirrors
  void enqueue_full_language(const DecWorkspace& dw, int dec, bool split, int batch, long long* ids, int stride, int id_pos,
                             hipStream_t st);
  struct Workspace {
    int batch = 0;
    float *melT = nullptr, *h1p = nullptr, *x = nullptr, *ln = nullptr, *qkv = nullptr,
          *att = nullptr, *hid = nullptr, *enc_out = nullptr;
    // plane path (fp16 hi | lo planes; ln / qkv / att / hid reuse the fp32 buffers above, same bytes): the two
    // zero-padded convolution inputs need buffers of their own (their pad rows sit elsewhere in the plane layout)
    unsigned short *melTp = nullptr, *h1pp = nullptr;
    // planes made by launch_f32_to_planes from the fp32 output of a fall-back contraction ([B T][4 d] elements)
    unsigned short* cvt = nullptr;
    // front end
    unsigned short* pcm_planes = nullptr;
    float *pw = nullptr, *melacc = nullptr;
    unsigned* clip_max = nullptr;
    float *mel_stage = nullptr, *pcm_stage = nullptr;
    std::vector<void*> owned;
  } ws_;
  // kernel-class timer (events live in the pipeline slot being encoded)
  bool kt_on_ = true;
  long enc_count_ = 0;
  void kt_begin(int cls, double flops, double bytes);
  void kt_end();
  void resolve_kernel_stats(int slot);
  KernelStat kstats_[kKcCount] = {{"gemm_planes_tile", 0, 0, 0, 0},     {"encoder_attention_planes", 0, 0, 0, 0},
                                  {"layernorm_rows", 0, 0, 0, 0},       {"mel_transpose", 0, 0, 0, 0},
                                  {"gemm_split16_tile", 0, 0, 0, 0},    {"encoder_attention_split", 0, 0, 0, 0},
                                  {"f32_to_planes", 0, 0, 0, 0}};
  int self_cap_ = 32;
  static constexpr int kDecRowsMax = 128;  // rows of one decoder pass (k_decoder.hip: up to four 32-row tiles)
};

}  // namespace wt
