/* wt_capi.h — C ABI of the MI355X (gfx950) Whisper EncDec engine.
 *
 * Drop-in boundary for the reference's engine surface (jerinphilip/whisper.tflite @ v2):
 * every entry point below is what a binding for that path would call instead of the
 * TFLite-interpreter-backed implementation.  Plain pointers and sizes only; nothing here
 * throws, exits or aborts: a file, shape or option the kernels do not support comes back as an int
 * status code plus wt_last_error().
 *
 * Threading contract = the reference's (an engine is NOT re-entrant; callers serialise,
 * cf. io/github/jerinphilip/whisper/Whisper.java:109-113): one in-flight call per handle,
 * one handle per GPU (device_id at create), one HIP stream per handle.
 */
#ifndef WT_CAPI_H_
#define WT_CAPI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wt_engine wt_engine;

enum wt_status {
  WT_OK = 0,
  WT_ERR_INVALID_ARG = 1,
  WT_ERR_IO = 2,          /* file missing / unreadable (reference: MmapFile throws, mmap_file.cpp:16-29) */
  WT_ERR_FORMAT = 3,      /* malformed weight or vocab file */
  WT_ERR_UNSUPPORTED = 4, /* e.g. an audio geometry other than the reference's fixed one */
  WT_ERR_DEVICE = 5,      /* no usable gfx950 device / HIP failure: the product has NO CPU fallback */
  WT_ERR_BUFFER = 6       /* caller buffer too small; *len still reports the needed size */
};

/* reference whisper.h:199-204 enum class EngineType */
enum wt_engine_type { WT_ENGINE_MONOLITH = 0, WT_ENGINE_ENCDEC = 1 };

/* Fixed audio geometry of the path (reference whisper.h:34-39). */
#define WT_SAMPLE_RATE 16000
#define WT_N_FFT 400
#define WT_HOP 160
#define WT_CHUNK_SAMPLES 480000 /* kSampleRate * kChunkSize */
#define WT_MAX_IDS 32           /* ids per clip: 4 prompt + <=27 generated (whisper.cpp:364-367), padded */

typedef struct wt_dims {
  int32_t n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
  int32_t n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} wt_dims;

/* Per-stage device time of the last batch call, from HIP events on the engine's stream. */
typedef struct wt_timings {
  float logmel_ms, encoder_ms, cross_kv_ms, decoder_ms, total_ms;
  int32_t batch, decoder_steps;
} wt_timings;

/* ---- lifecycle -------------------------------------------------------------------------
 * Replaces whisper::create_engine (whisper.h:259-260, whisper.cpp:778-790) and
 * EncDec::EncDec (whisper.cpp:740-750).  `model_prefix` resolves to "<prefix>.wtw" (this
 * build's weight file, standing in for "<prefix>.encoder.tflite"/"<prefix>.decoder.tflite",
 * whisper.cpp:743-744); `vocab_path` is the reference's filters+vocab .bin, byte-compatible.
 * When "<prefix>.wtw" does not exist but the reference's "<prefix>.encoder.tflite" and
 * "<prefix>.decoder.tflite" do, their weights are extracted (wt_convert_tflite below) into
 * "<prefix>.wtw" first.  WT_ENGINE_MONOLITH (reference Monolith, whisper.cpp:667-738: one graph with HF
 * generate() inside) runs the same encoder / decoder kernels from "<prefix>.wtw" with the prompt that
 * graph forces: [sot, notimestamps] for an English-only model (the head of kGoldenGeneratedIDs,
 * whisper.h:27-32), [sot, <|en|>, transcribe, notimestamps] for a multilingual one; ids are capped at the
 * engine's 31 positions where HF generate() allows 448.
 * On failure *out is NULL and wt_last_error(NULL) describes why. */
int wt_engine_create(int engine_type, const char* model_prefix, const char* vocab_path,
                     int multilingual, int device_id, wt_engine** out);
/* Replaces `delete engine` (bindings/java/whisper.tflite.cpp:36-42). NULL is a no-op. */
void wt_engine_destroy(wt_engine* h);
/* Message of the last failing call on `h` (or of the last failing create when h == NULL). */
const char* wt_last_error(const wt_engine* h);
int wt_engine_dims(const wt_engine* h, wt_dims* out);

/* Options (reference hard-codes them): "language" (prompt language id, whisper.cpp:327,
 * default language_id("de") = 2; WT_LANGUAGE_AUTO = -1: every greedy decode — synchronous, long-audio and pipelined —
 * detects the language of each clip on the device from the logits at the sot position and puts its token at ids[b][1],
 * DESIGN.md section 12; WT_ERR_UNSUPPORTED on a Monolith engine and without language tokens, and at the call together
 * with beam_size > 1, a caller prompt or the forced-ids tap), "max_tokens" (max decoder positions, whisper.cpp:364,
 * default 30), "max_positions" (0 = default: off, the max_tokens path with its 31 positions; 32 .. n_text_ctx = full-length
 * greedy decoding on the wt_*_tokens_full_batch* and the text entry points, see below and DESIGN.md section 13),
 * "timestamps" (0 = default: off; 1 = full-length greedy decoding behind Whisper's timestamp rules, see wt_last_segments
 * below and DESIGN.md section 14; WT_ERR_UNSUPPORTED when the model's vocabulary has no timestamp ids), "max_initial_timestamp"
 * (latest first timestamp in ticks of 20 ms, default 50 = 1.0 s, -1 = no limit, at most 1500),
 * "scores" (0 = default: off; 1 = full-length greedy decoding also returns token log-probabilities, avg_logprob and
 * no_speech_prob, see wt_last_scores below and DESIGN.md section 15; WT_ERR_UNSUPPORTED when the model's vocabulary has
 * no <|nospeech|> id), "skip_silence" (0 = default; 1 = a clip with no_speech_prob > "no_speech_threshold" / 1000
 * (default 600) and not avg_logprob > "logprob_threshold" / 1000 (default -1000) yields empty text and no segments; needs
 * "scores" = 1 at the call),
 * "temperature" (thousandths, 0 = default: greedy, up to 1000; full-length decoding samples every id from
 * softmax(logits / T) over the ids the step may choose, on the device, see wt_last_decode_info below and DESIGN.md
 * section 19), "seed" (default 0: the 64-bit key of the sampler's Philox4x32-10 stream; a decode is a function of the
 * audio, the options and the seed), "temperature_fallback" (0 = default; 1 = Whisper's temperature fall-back: a clip is
 * decoded again at "temperature" + "temperature_increment" (default 200), ... up to 1000 while its compression ratio
 * exceeds "compression_ratio_threshold" / 1000 (default 2400, 0 = off) or its avg_logprob lies below
 * "logprob_threshold" / 1000, unless it is silence by "no_speech_threshold"; needs "scores" = 1 at the call),
 * "stop_at_eot" (whisper.cpp:397-399, default 1), "verbose" (default 0),
 * "cross_chunks" (key chunks per (clip, head) in the decoder cross attention: 1, 2, 4, 8, or 0 = by batch size, the default).
 * Kernel selection (results stay within the fp32 error budget for every value): "gemm_variant"
 * (-1 = default: every encoder GEMM on the plane kernel, operands as two fp16 planes with power-of-two scales
 * from weight-derived bounds, csrc/bf16_split.h — except the contractions the load-time slack check flagged,
 * which run the full-range form by themselves; 13, 16 = all of them on three bf16 planes split in the loop, full
 * fp32 operand range, at 3 / 2 blocks per CU; 0 = fp32 MFMA), "attn_variant" (4 = default, two fp16 planes;
 * 1 = three bf16 planes; 0 = fp32 MFMA),
 * "fc2_ksplit" (2 = default: the decoder's fc2 GEMM over twice the blocks, halves added by the
 * consumer; 1 = one block per column tile), "use_graphs" (1 = default: the decoder's launch sequence is replayed from a hipGraph).
 * Decoder form: "cross_absorb" (1 = default: cross-attention scores the decoder's queries, pre-multiplied by Wk, directly
 * against the encoder output planes and applies Wv after the softmax, so no cross K/V cache is projected or streamed;
 * 0 = the cross-KV cache of whisper.cpp's graph; both the fp32-accurate and the bf16 storage mode run either form —
 * pipelined batches and synchronous calls of 32 clips or more the absorbed one, smaller synchronous calls the cached
 * one; "cross_absorb_active" reads what is in effect), "abs_chunks" (key chunks per clip of that form, 0 = by batch size), "dec_pair" (1 = default: two consecutive
 * pipelined batches of equal size <= 32 share one decoder chain; change only with nothing in flight), "dec_group" (2 =
 * default, 3 or 4: that many consecutive batches per chain, rows = group x batch <= 128; three or four want 3 x group + 4
 * or more batches in flight and pay off on long jobs only: +1 % at four),
 * Decoding: "beam_size" (1 = default: the reference's greedy argmax, unchanged; 2..8 = beam search with that many
 * hypotheses per clip on every synchronous entry point: per step each live hypothesis offers its top beam_size + 1 tokens
 * by log-softmax over the full vocabulary, the candidates are taken by sum of log-probabilities, an EOT candidate
 * finishes its hypothesis, a clip is done with beam_size finished ones, and the result is the finished hypothesis with
 * the best sum / generated ids (EOT included), DESIGN.md section 11.  Deliberate scope cuts, WT_ERR_UNSUPPORTED with
 * beam_size > 1: the pipelined wt_pipeline_submit* calls, the bf16 storage mode, cross_absorb = 0 (and weights or a
 * gemm_variant without the absorbed form), stop_at_eot = 0, the forced-ids debug tap and the logits tap of
 * wt_encdec_debug_batch),
 * "full_beam" (0 = default: a full-length call, "max_positions" set, with beam_size > 1 is WT_ERR_UNSUPPORTED; 1 = such a
 * call runs full-length beam search, DESIGN.md section 23: the walk, the finished list, the fill at the cap and the ranker
 * are beam_size's, but every live hypothesis first applies the step's allowed set to its OWN generated ids — the whole
 * vocabulary, or with "timestamps" what the timestamp rules leave — and a token's log-probability is its logit minus
 * the logsumexp over that set; a hypothesis offers its top beam_size + 1 allowed ids, fewer where fewer are allowed, a
 * clip then has fewer live hypotheses, and it is done with beam_size finished ones or none live.  It works with and
 * without "timestamps", "scores" and "skip_silence" on every full-length entry point, wt_transcribe_pcm / _file and
 * wt_transcribe_long_pcm with fixed windows included; with "scores" the sums, counts and token log-probabilities are the
 * chosen hypothesis's, and wt_last_beam_scores is valid too.  WT_ERR_UNSUPPORTED with full_beam = 1 and beam_size > 1:
 * what beam_size and "max_positions" refuse, "temperature" > 0 and "temperature_fallback" (unless "fallback_beam" = 1,
 * see wt_last_best_of below), either kind of context,
 * "seek", "word_timestamps" and wt_transcribe_long_batch; the engine stays usable after each),
 * "full_bf16" (0 = default: a full-length call, "max_positions" set, on an engine with "bf16" = 1 is WT_ERR_UNSUPPORTED;
 * 1 = such a call runs with bf16 weights, bf16 cross-attention operands and a bf16 self-attention cache, fp32
 * accumulation and an fp32 residual stream, DESIGN.md section 33.  It works with and without "timestamps",
 * "max_initial_timestamp", "scores", "skip_silence", "temperature", "seed", "temperature_fallback", the suppression
 * lists, wt_engine_set_context, wt_transcribe_long_pcm with fixed windows and with "seek", "full_beam" = 1 with
 * beam_size 2..8, "best_of", "fallback_beam", both cross-attention forms and "use_graphs" 0 and 1; a bf16 engine may
 * choose other ids than the fp32 one wherever two logits lie within the mode's rounding of each other.
 * WT_ERR_UNSUPPORTED with full_bf16 = 1, each with a text of its own that names the option, the engine stays usable:
 * "word_timestamps", wt_engine_set_contexts and wt_transcribe_long_batch, language = WT_LANGUAGE_AUTO (also with
 * "full_language" = 1); the pipeline, forced ids and the other refusals of "max_positions" stand, and so does
 * beam_size > 1 without "max_positions"),
 * "full_bf16_all" (0 = default: those refusals stand; 1, beside "bf16" = 1, "full_bf16" = 1 and "max_positions": they are
 * lifted — wt_engine_set_contexts and wt_transcribe_long_batch, language = WT_LANGUAGE_AUTO with "full_language" = 1 on every
 * path of that option, and "word_timestamps" run in the bf16 storage mode; anything but 0 or 1 is
 * WT_ERR_INVALID_ARG.  The cuts of other options keep their own texts: contexts with "word_timestamps"; contexts, "seek" or
 * "word_timestamps" behind "full_beam" / "best_of"; "best_of" / "fallback_beam" with wt_transcribe_long_batch; the pipeline
 * and forced ids),
 * "last_batches" (N = the next N pipelined submits are the last of a job: they are decoded one chain per batch, the very
 * last on the encoder's stream, so the pipeline drains sooner; counts down to 0 by itself, may be set with batches in
 * flight), "force_fallback" (test hook: bit mask of contractions sent to the full-range kernels, nothing in flight).
 * Read-only (wt_engine_get_option): "f16_fallbacks" = contractions that were given the full-range bf16
 * three-plane kernels at load time because an operand's weight-derived bound lies more than 2^12 above its
 * typical magnitude (csrc/engine.cpp, upload_weights) — only those leave the plane kernels, the others keep them; "in_flight" = submitted, uncollected batches; "pipelined_encoder_cus" = CUs the CU-masked encoder stream of the pipeline may use.
 * Environment, read at wt_engine_create: WT_ENC_CU_RESERVE (CUs per XCD the pipelined encoder
 * stream leaves to the decoders, default 8, 0 = none), WT_DEC_STREAMS (decoder streams, default 3),
 * WT_TRACE_PIPELINE (per-batch device timeline on stderr), WT_NO_STREAM_PROBE (skip the ~10 ms probe that picks decoder
 * streams which do not share a hardware queue with the encoder stream or with each other). */
int wt_engine_set_option(wt_engine* h, const char* key, long value);
int wt_engine_get_option(const wt_engine* h, const char* key, long* value);
/* Replaces the reference's hard-coded prompt [sot, 50259+language, transcribe, notimestamps]
 * (whisper.cpp:327-339) with n (1..8) caller ids; n = 0 restores the default.  Needed for
 * test-sized vocabularies that do not contain the multilingual special ids. */
int wt_engine_set_prompt(wt_engine* h, const int64_t* ids, int n);
/* A context in front of the prompt: Whisper's initial_prompt / condition_on_previous_text.  With
 * n (1..4096) ids set, every full-length decode ("max_positions") feeds [<|startofprev|>] + the LAST n_text_ctx / 2 - 1
 * of them + the prompt (the default one, the "timestamps" one, or wt_engine_set_prompt's), the same for every clip of the
 * call; generated ids, the timestamp rules and the scores all start behind the whole of it, and no_speech_prob is read at
 * sot's position.  n = 0 clears the context; the read-only option "context_ids" tells how many ids are kept.  An id outside
 * the vocabulary or n > 4096 is WT_ERR_INVALID_ARG, a vocabulary without <|startofprev|> (token_prev >= n_vocab) or a
 * Monolith engine WT_ERR_UNSUPPORTED.  It works with and without "timestamps", "scores", "temperature" and
 * "temperature_fallback".  With a context set a decode call is WT_ERR_UNSUPPORTED without "max_positions" and wherever
 * "max_positions" refuses one (the calls with rows of WT_MAX_IDS ids, the pipeline, beam_size > 1, the bf16 storage mode,
 * language = WT_LANGUAGE_AUTO, the forced-ids tap), and WT_ERR_INVALID_ARG when the fed prompt leaves no position to
 * generate (its length >= "max_positions"); the engine stays usable after each.  Such calls run their launches eagerly:
 * no decoder graph is captured for them ("graphs_cached", read-only, does not grow with the context lengths seen).
 * Option "prompt_group": 0 = the prompt passes take 128 / batch positions each (default), 1 = one position each; it
 * changes nothing without a context. */
int wt_engine_set_context(wt_engine* h, const int64_t* ids, int n);

/* Per-clip contexts: clip b of every following full-length call is decoded behind ids[offsets[b] .. offsets[b + 1])
 * (an empty range: that clip's fed prompt is the prompt alone).  n_clips 1..64; each clip keeps the last
 * n_text_ctx / 2 - 1 ids, as wt_engine_set_context.  n_clips = 0 clears.  Setting either kind of context clears the other.
 * The call is one ragged decoder chain: a clip's ids, scores and samples are those of a call of
 * its own behind wt_engine_set_context with its ids.  The read-only option "context_clips" tells n_clips.  An id outside
 * the vocabulary, offsets that decrease, more than 4096 ids for a clip or n_clips > 64 is WT_ERR_INVALID_ARG, a vocabulary
 * without <|startofprev|> or a Monolith engine WT_ERR_UNSUPPORTED as soon as some clip's range is not empty.  With contexts set a full-length call whose batch
 * differs from n_clips, or in which some clip's fed prompt is >= "max_positions", is WT_ERR_INVALID_ARG; "word_timestamps"
 * = 1 is WT_ERR_UNSUPPORTED (the alignment pass takes one prompt length per call), and so is every call that
 * "max_positions" or a wt_engine_set_context context refuses; the engine stays usable after each.  Such calls run
 * eagerly and capture no graph.  It works with and without "timestamps", "scores", "skip_silence", "temperature" and
 * "temperature_fallback". */
int wt_engine_set_contexts(wt_engine* h, const int64_t* ids, const int32_t* offsets, int n_clips);

/* Logit suppression: Whisper's SuppressTokens and SuppressBlank.  Every full-length decode
 * ("max_positions") sets the logits of `ids` to -inf at every generated position and those of `first_ids` at the first
 * one only (the position behind the whole fed prompt and context), on the device, behind the no-speech probability (read
 * from the unfiltered logits) and in front of every other rule: the timestamp rules, the log-softmax of the scores, the
 * sampler and every beam hypothesis's allowed set then see a vocabulary without them.  Both lists take 0..1024 ids,
 * duplicates allowed; n = n_first = 0 clears both, after which every call is what it was before.  WT_ERR_INVALID_ARG: an id
 * outside [0, n_vocab), EOT among `ids` (the allowed set must never be empty; EOT may be in `first_ids`), a count outside
 * 0..1024.  WT_ERR_UNSUPPORTED: a Monolith engine.  The read-only options "suppress_ids" and "suppress_first_ids" give
 * the counts in effect.  Option "suppress_default" = 1 installs the lists of wt_vocab_default_suppress over the engine's
 * vocabulary (ids below the model's n_vocab), 0 clears them.  With a list set a decode call is WT_ERR_UNSUPPORTED without
 * "max_positions" and wherever "max_positions" refuses one (the calls with rows of WT_MAX_IDS ids, the pipeline, the bf16
 * storage mode, language = WT_LANGUAGE_AUTO, the forced-ids tap) and on a model whose vocabulary holds no EOT id
 * (token_eot >= n_vocab: the selectors behind the filter take one); the engine stays usable after each.  It works with and
 * without "timestamps", "scores", "skip_silence", "temperature", "temperature_fallback" (every attempt), either kind of
 * context, "seek", wt_transcribe_long_pcm (every window), wt_transcribe_long_batch, "word_timestamps" (the alignment pass
 * is teacher-forced and unaffected) and "full_beam" = 1 with beam_size 2..8.  Call it with nothing in flight. */
int wt_engine_set_suppress(wt_engine* h, const int64_t* ids, int n, const int64_t* first_ids, int n_first);

/* ---- single-clip entry points (the reference's two virtuals) ----------------------------
 * Replace Engine::transcribe(std::vector<float>&) (whisper.h:160, whisper.cpp:752-769; JNI
 * transcribeBuffer, bindings/java/whisper.tflite.cpp:45-58) and
 * Engine::transcribe(const char*) (whisper.h:161, whisper.cpp:771-776; JNI transcribeFile
 * :61-71).  pcm is padded with zeros / truncated to 480000 samples like the reference
 * (whisper.cpp:753) but the caller's buffer is not modified.  Text is written without a
 * terminating NUL guarantee beyond min(len, cap-1); *len gets the full byte length. */
int wt_transcribe_pcm(wt_engine* h, const float* pcm, size_t n_samples, char* out, size_t cap,
                      size_t* len);
int wt_transcribe_file(wt_engine* h, const char* wav_path, char* out, size_t cap, size_t* len);

/* Long audio (the reference truncates to one 30 s window, whisper.cpp:753,773):
 * pcm is cut into consecutive 30 s windows (the last one zero-padded), the windows are
 * transcribed as batches of up to 32 clips, and the per-window texts — each exactly what
 * wt_transcribe_pcm returns for that window — are joined with '\n'. */
int wt_transcribe_long_pcm(wt_engine* h, const float* pcm, size_t n_samples, char* out, size_t cap,
                           size_t* len);

/* ---- batch entry points (the reference is batch 1; clips are independent) ---------------
 * Host-pointer forms copy over PCIe; *_dev forms take device pointers already in HBM (the
 * form bench.py times).  All are synchronous on return.
 *   pcm  [B][480000] fp32           mel [B][n_mels][2*n_audio_ctx] fp32 (reference Mel
 *   layout, whisper.cpp:184: [mel][frame])     ids [B][WT_MAX_IDS] int64, n_ids [B] int32.
 * ids rows hold prompt + generated ids exactly as Decoder::forward returns them
 * (whisper.cpp:402), zero-padded. */
/* Device buffers for the *_dev forms, allocated on the engine's GPU by the engine's own HIP runtime: a host program
 * (bench.py, the tests, a binding) needs no HIP of its own to keep its inputs resident in HBM.  upload / download are
 * synchronous copies (offset in bytes into the buffer); wt_device_synchronize returns once the device is idle. */
int wt_device_alloc(wt_engine* h, size_t bytes, void** d_ptr);
int wt_device_free(wt_engine* h, void* d_ptr);
int wt_device_upload(wt_engine* h, void* d_dst, size_t offset, const void* src, size_t bytes);
int wt_device_download(wt_engine* h, void* dst, const void* d_src, size_t offset, size_t bytes);
int wt_device_synchronize(wt_engine* h);
int wt_logmel_batch(wt_engine* h, const float* pcm, int batch, float* mel);
int wt_logmel_batch_dev(wt_engine* h, const float* d_pcm, int batch, float* d_mel);
int wt_encdec_tokens_batch(wt_engine* h, const float* mel, int batch, int64_t* ids, int32_t* n_ids);
int wt_encdec_tokens_batch_dev(wt_engine* h, const float* d_mel, int batch, int64_t* ids,
                               int32_t* n_ids);
/* PCM -> ids in one call (front end + encoder + decoder), device-resident input. */
int wt_transcribe_tokens_batch_dev(wt_engine* h, const float* d_pcm, int batch, int64_t* ids,
                                   int32_t* n_ids);

/* Full-length greedy decoding (option "max_positions" = P in [32, n_text_ctx]): positions 0 .. P - 1
 * are fed, so a row holds at most P + 1 ids (prompt + generated, zero-padded); ids [B][ids_stride] with ids_stride >=
 * P + 1 (else WT_ERR_BUFFER), B <= 64.  The decoder chain runs in segments of 32 positions and ends after the segment in
 * which the last clip emitted EOT; wt_timings.decoder_steps reports the steps run.  wt_transcribe_pcm / _file /
 * _long_pcm honour the option.  With max_positions = 0 these calls are WT_ERR_INVALID_ARG.  While the option is set, the
 * calls with rows of WT_MAX_IDS ids (wt_encdec_tokens_batch*, wt_transcribe_tokens_batch_dev, wt_encdec_debug_batch) and
 * wt_pipeline_submit* are WT_ERR_UNSUPPORTED, and so is a full-length call with beam_size > 1 (unless "full_beam" = 1:
 * full-length beam search), the bf16 storage mode, language = WT_LANGUAGE_AUTO or the forced-ids tap; the engine stays
 * usable after each. */
int wt_encdec_tokens_full_batch(wt_engine* h, const float* mel, int batch, int64_t* ids, int ids_stride, int32_t* n_ids);
int wt_encdec_tokens_full_batch_dev(wt_engine* h, const float* d_mel, int batch, int64_t* ids, int ids_stride,
                                    int32_t* n_ids);
int wt_transcribe_tokens_full_batch_dev(wt_engine* h, const float* d_pcm, int batch, int64_t* ids, int ids_stride,
                                        int32_t* n_ids);

/* Pipelined form of the same path: submit enqueues encoder (one HIP stream) and decoder (one
 * of three further streams, in rotation) for one device-resident batch and returns at once;
 * collect blocks until the OLDEST submitted batch has its ids on the host.  In steady state
 * the MFMA-bound encoder of the newest batch shares the chip with the latency/HBM-bound
 * decoder chains of the previous ones.  d_mel must stay valid until that batch is collected.
 * At most WT_PIPELINE_DEPTH uncollected submits (ten keep the default pipeline full); batch <= 64. */
#define WT_PIPELINE_DEPTH 24
int wt_pipeline_submit_dev(wt_engine* h, const float* d_mel, int batch);
/* Same from device-resident PCM [batch][480000]: the log-mel front end (whisper.cpp:109-216) runs
 * on the pipeline's encoder stream ahead of the encoder; d_pcm may be reused once the call returns
 * only after the batch is collected. */
int wt_pipeline_submit_pcm_dev(wt_engine* h, const float* d_pcm, int batch);
int wt_pipeline_collect(wt_engine* h, int64_t* ids, int32_t* n_ids);

/* Stage taps for parity tests: encoder output [B][n_audio_ctx][n_audio_state] and the
 * last-position logits of every argmax step [B][steps][n_vocab] (either may be NULL). */
int wt_encdec_debug_batch(wt_engine* h, const float* mel, int batch, int64_t* ids, int32_t* n_ids,
                          float* enc_out, float* logits, int logits_steps_cap);

int wt_last_timings(const wt_engine* h, wt_timings* out);

/* Spoken-language detection: softmax over the language tokens of the logits at the sot position. */
#define WT_LANGUAGE_AUTO (-1)
/* number of language tokens of this engine's vocabulary (99 for 51865), or -WT_ERR_UNSUPPORTED (an English-only engine,
 * or a vocabulary that ends before the language tokens) */
int wt_language_count(const wt_engine* h);
/* encoder + one decoder position + language head, nothing else decoded (beam_size and a caller prompt do not matter):
 * lang [B] (index into wt_lang_code), probs [B][wt_language_count()] or NULL */
int wt_detect_language_batch(wt_engine* h, const float* mel, int batch, int32_t* lang, float* probs);
int wt_detect_language_batch_dev(wt_engine* h, const float* d_mel, int batch, int32_t* lang, float* probs);
/* the same for one clip of PCM, padded or truncated to 30 s as wt_transcribe_pcm: *lang and its probability (prob may be NULL) */
int wt_detect_language_pcm(wt_engine* h, const float* pcm, size_t n_samples, int32_t* lang, float* prob);
/* after a synchronous decode with "language" = WT_LANGUAGE_AUTO (a batch call of up to 64 clips, wt_transcribe_pcm /
 * _file, or wt_transcribe_long_pcm: one entry per window): per clip the language used and its probability (at most cap
 * entries written).  Returns the clip count, or -WT_ERR_INVALID_ARG when the last synchronous decode did not detect
 * (as wt_last_beam_scores).  Pipelined batches carry the language in their ids: ids[b][1] - 50259. */
int wt_last_languages(const wt_engine* h, int32_t* lang, float* prob, int cap);
/* Automatic language behind "max_positions" (DESIGN.md section 32): option "full_language" (0 = default: a full-length
 * call with language = WT_LANGUAGE_AUTO is WT_ERR_UNSUPPORTED, as ever; 1 = every clip of such a call is decoded behind
 * [sot, <its language>, task, ..]).  The language is a function of the audio alone: the argmax over the allowed language
 * tokens of the logits at position 0 of [sot] — what wt_detect_language_batch returns for the clip — whatever the context,
 * temperature, seed, attempt, suppression lists, batch or "use_graphs".  It works with and without "timestamps",
 * "scores", "skip_silence", "temperature", "temperature_fallback" (every attempt), the suppression lists, either kind of
 * context, "seek", "full_beam" = 1 with beam_size 2..8, "best_of" and "fallback_beam" (every hypothesis and sample of a clip
 * carries the clip's language), "word_timestamps" (the alignment rows carry it too, and the word-splitting rule follows
 * it per clip), wt_transcribe_long_pcm and wt_transcribe_long_batch; the long calls follow Whisper's transcribe():
 * one language per file, detected on the file's first window and held for its later windows.  wt_last_languages then
 * reports per clip of a full-length call, and per window of a long call each window's file's value (next to
 * wt_last_window_files).  WT_ERR_UNSUPPORTED with full_language = 1 and language = WT_LANGUAGE_AUTO, the engine stays
 * usable: a caller prompt, the forced-ids tap, the bf16 storage mode and the pipeline (a Monolith engine or one without
 * language tokens already refuses language = WT_LANGUAGE_AUTO itself); beam_size > 1 without "max_positions" stays refused.
 * Language candidates: langs [n] ids in [0, wt_language_count()), duplicates allowed, n = 0 clears the list, n > 128 or
 * an id outside the range is WT_ERR_INVALID_ARG, a Monolith engine or one without language tokens WT_ERR_UNSUPPORTED.  With
 * a list set every detecting path — wt_detect_language_*, the automatic decode of the calls with rows of WT_MAX_IDS ids,
 * the pipeline included, and the full-length calls above — detects among the candidates only: probabilities are
 * normalised over them and exactly 0 elsewhere, and a one-entry list gives that language with probability 1.  The
 * read-only option "language_candidates" reports the number of distinct ids.  Call it with nothing in flight.
 * Option "task" (0 = default: transcribe; 1 = translate): every prompt the engine builds itself carries <|translate|>
 * where <|transcribe|> stands.  WT_ERR_UNSUPPORTED: an engine created with multilingual = 0, a Monolith engine, a
 * vocabulary whose <|translate|> id lies outside the model's; a decode call with a caller prompt while task = 1. */
int wt_engine_set_language_candidates(wt_engine* h, const int32_t* langs, int n);

/* Beam search (option "beam_size" > 1): for every clip of the last synchronous beam call, the chosen hypothesis's sum of
 * natural-log probabilities and its number of generated ids, EOT included (at most cap entries written).  Returns the
 * clip count, or -WT_ERR_INVALID_ARG when the last synchronous decode was not a beam search (negative, so that it cannot
 * be taken for a count of one clip). */
int wt_last_beam_scores(const wt_engine* h, float* sum_logprob, int32_t* n_generated, int cap);

/* Timestamp decoding (option "timestamps" = 1 together with "max_positions").  The default prompt
 * then ends before <|notimestamps|> ([sot, language, transcribe]; a Monolith engine on an English vocabulary [sot]; a
 * caller prompt is used as given), and every step of a full-length greedy decode is filtered on the device by Whisper's
 * timestamp rules: timestamps come in pairs, never decrease, the first id is a timestamp of at most
 * "max_initial_timestamp" ticks, and a timestamp is chosen when the timestamps' summed probability exceeds every text
 * token's.  The ids come back as from any full-length call, timestamp ids (token_beg + tick, 20 ms per tick) among them;
 * the text entry points print those as the vocabulary's own token strings.  With the option set, a decode call is
 * WT_ERR_UNSUPPORTED without "max_positions" and wherever "max_positions" refuses one (the calls with rows of WT_MAX_IDS
 * ids, the pipeline, beam_size > 1, the bf16 storage mode, language = WT_LANGUAGE_AUTO, the forced-ids tap); the engine
 * stays usable after each.
 * A segment is the text between an opening and a closing timestamp: ids[id_begin .. id_begin + id_count) of the clip's
 * row, spoken from t0_ms to t1_ms.  Two consecutive timestamps close one segment and open the next; text left unclosed
 * at the end of the row (EOT or the position cap) closes at the window end, 30 000 ms, with open = 1; an opening
 * timestamp without text yields no segment. */
typedef struct wt_segment {
  int32_t clip, t0_ms, t1_ms, id_begin, id_count, open;
} wt_segment;
/* the segments of every clip of the last synchronous timestamp decode, in clip order (at most cap written).  After
 * wt_transcribe_long_pcm: clip = the window's index, and 30 000 ms x that index is added to both times.  Returns the
 * segment count, or -WT_ERR_INVALID_ARG when the last synchronous decode ran without timestamps (as wt_last_beam_scores). */
int wt_last_segments(const wt_engine* h, wt_segment* out, int cap);
/* the text of segment `index` of that list: its ids decoded as wt_decode_text does with omit_special_tokens = 0 */
int wt_last_segment_text(const wt_engine* h, int index, char* out, size_t cap, size_t* len);

/* Decode confidence (option "scores" = 1 together with "max_positions", with or without "timestamps"; DESIGN.md section
 * 15).  Formed on the device inside the decoder chain.  The log-probability of a generated id is its fp32 logit minus the
 * float64 logsumexp of the logits of the ids that step chose from: the whole vocabulary, or with "timestamps" what the
 * timestamp rules left.  sum_logprob sums it over the n_generated ids of the clip, the EOT that ended it included;
 * avg_logprob = sum_logprob / n_generated; no_speech_prob is the softmax probability of <|nospeech|> (50361, multilingual
 * 50362) at position 0, behind sot alone, over the whole vocabulary.  skipped = 1: option "skip_silence" blanked the clip
 * in the text entry points and in wt_last_segments; the id-returning calls return its ids as decoded.  With the option
 * set, a decode call is WT_ERR_UNSUPPORTED without "max_positions" and wherever "max_positions" refuses one; the engine
 * stays usable after each. */
typedef struct wt_clip_score { float sum_logprob, avg_logprob, no_speech_prob; int32_t n_generated, skipped; } wt_clip_score;
/* every clip of the last synchronous decode with "scores" = 1 (after wt_transcribe_long_pcm: one per window);
 * returns the clip count, or -WT_ERR_INVALID_ARG when that decode ran without scores (as wt_last_beam_scores) */
int wt_last_scores(const wt_engine* h, wt_clip_score* out, int cap);
/* log-probabilities aligned with the id rows: out[b][i] belongs to ids[b][i]; 0 for prompt ids and padding (at most
 * cap_clips rows of `stride` floats written, columns past the decode's own row length zero).  Returns the clip count or
 * -WT_ERR_INVALID_ARG as above. */
int wt_last_token_logprobs(const wt_engine* h, float* out, int stride, int cap_clips);
/* mean token log-probability over the text ids of each segment of wt_last_segments, same order (at most cap written).
 * Returns the segment count, or -WT_ERR_INVALID_ARG unless the last synchronous decode ran with scores and timestamps. */
int wt_last_segment_scores(const wt_engine* h, float* avg_logprob, int cap);

/* Temperature sampling and fall-back (options "temperature", "seed", "temperature_fallback" together with
 * "max_positions", with or without "timestamps" and "scores").  The token of a step is the argmax
 * over the allowed ids of logit / T + Gumbel noise (Philox4x32-10 under the key "seed" and the counter (id / 4, position,
 * clip index, attempt)), which is a sample from softmax(logits / T); the timestamp rules and the scores work on the
 * untempered logits.  T = 0 is the greedy step.  With fall-back a clip's result is that of the first temperature of
 * the schedule after which it needs no further attempt, or of the last.  temperature_milli: the temperature the kept
 * result was decoded at; attempts: decodes the clip took; needs_fallback: 1 when the kept result still met the
 * fall-back condition (the schedule was exhausted); compression_ratio: bytes of the clip's text (its generated ids below
 * EOT, decoded as wt_decode_text does with omit_special_tokens = 1) over bytes of zlib's compress() of it, 0 for empty
 * text and where zlib (libz.so.1, loaded at first use) is not available — a nonzero "compression_ratio_threshold" is
 * then WT_ERR_UNSUPPORTED at a fall-back call.  With sampling or fall-back set, a decode call is WT_ERR_UNSUPPORTED
 * without "max_positions" and wherever "max_positions" refuses one; the engine stays usable after each. */
typedef struct wt_clip_decode { int32_t temperature_milli, attempts, needs_fallback; float compression_ratio; } wt_clip_decode;
/* every clip of the last synchronous decode that sampled or ran fall-back (after wt_transcribe_long_pcm: one per window,
 * whose clip index in the counter is its index in the file); returns the clip count, or -WT_ERR_INVALID_ARG when that
 * decode did neither (as wt_last_scores) */
int wt_last_decode_info(const wt_engine* h, wt_clip_decode* out, int cap);

/* Several samples per clip (option "best_of" = N, 1 = default .. 8).  In a full-length decode every
 * attempt whose temperature is above 0 — a fixed "temperature" > 0, or the later attempts of "temperature_fallback" —
 * decodes N samples of every clip in one chain and keeps the FIRST sample with the largest sum_logprob / n_generated in
 * float64 (every generated id counted, EOT included: the avg_logprob of wt_last_scores; Whisper's ranker divides by the
 * length without EOT).  A sample whose average is NaN never wins; where all are, sample 0 is kept.  Sample j draws from
 * the Philox stream of wt_last_decode_info's counter with the attempt word attempt + (j << 16): sample 0 is the decode
 * of "best_of" = 1 under the same seed, bit for bit.  An attempt at temperature 0 draws nothing and ignores the option,
 * as Whisper does; "best_of" > 1 with "temperature" = 0 and no fall-back changes nothing.  Thresholds, scores, segments
 * and wt_last_decode_info are those of the kept sample.  With sampling or fall-back set, "best_of" > 1 is
 * WT_ERR_UNSUPPORTED (the engine stays usable) beside a context of either kind, "seek", "word_timestamps",
 * "stop_at_eot" = 0, wt_transcribe_long_batch, a decoder without the absorbed cross-attention ("cross_absorb" = 0), and
 * wherever "max_positions" refuses a call; with "beam_size" > 1 a temperature is refused as before, unless:
 * option "fallback_beam" (0 = default, 1; it means something only with "full_beam" = 1 and beam_size 2..8).  At 1 such a
 * call accepts "temperature" and "temperature_fallback": an attempt at temperature 0 — the schedule's first when
 * "temperature" = 0 — is full-length beam search over all clips, its chosen hypothesis's ids, token log-probabilities,
 * float64 sum, length (EOT counted) and no-speech probability judged by the thresholds like any attempt's; an attempt
 * above 0 runs the sampler with "best_of" rows per clip and ignores the beam, as Whisper does; a fixed "temperature" > 0
 * without fall-back is a sampling call.  wt_last_beam_scores is not valid after such a call: wt_last_scores and
 * wt_last_decode_info tell what each clip was kept with.  Everything else "full_beam" refuses stays refused.  The options
 * of Whisper's default command line: beam_size 5, full_beam 1, fallback_beam 1, best_of 5, temperature_fallback 1.
 * wt_last_best_of: per clip of the last synchronous decode (after wt_transcribe_long_pcm with fixed windows: per window)
 * the kept sample picked[i] and every sample's sum_logprob[i][8] / n_generated[i][8] (zeros from N on; a clip whose kept
 * attempt ran at temperature 0: sample 0 alone, with "scores" its own sum and count).  Returns the clip count (at most cap
 * clips written), or -WT_ERR_INVALID_ARG when no clip of that decode was kept from an attempt that ran N > 1 samples. */
int wt_last_best_of(const wt_engine* h, int32_t* picked, double* sum_logprob, int32_t* n_generated, int cap);

/* Seeking long-audio transcription (option "seek" = 1 together with "timestamps" = 1 and "max_positions", else a decode
 * call is WT_ERR_UNSUPPORTED).  wt_transcribe_long_pcm then decodes one window at a time as Whisper's
 * transcribe() does: window w is pcm[seek : seek + 480000) zero-padded, decoded as one clip (all decode options apply; its
 * clip index in the sampling counter is w) behind the context, cut into segments by wt_vocab_seek_step, and the next
 * window starts advance_samples later: at the last closed timestamp, or at the window's end.  The kept ids (those of the
 * kept segments, timestamps included) are the window's line of text and are appended to the context of the next window;
 * "condition_on_previous_text" = 0 (default 1), or a window whose kept result was decoded above temperature 0.5, empties
 * the context instead.  A window "skip_silence" blanked keeps nothing and advances by the whole window.  The caller's
 * wt_engine_set_context ids seed the first window and are the engine's context again after the call.  The log-mel of a
 * window is the front end's on that slice of PCM, as for any clip.
 * After such a call wt_last_segments holds the kept segments (clip = w, times in the file: seek / 16 ms + tick x 20 ms,
 * ids[id_begin .. id_begin + id_count) of the window's id row, the segment's timestamps included), wt_last_scores,
 * wt_last_token_logprobs and wt_last_decode_info one entry per window, wt_last_segment_scores the mean over each
 * segment's ids below EOT, and wt_last_windows one record per window. */
typedef struct wt_window {
  int64_t seek_sample;
  int32_t advance_samples, n_context, n_prompt, n_kept_ids, skipped, temperature_milli;
} wt_window;
/* returns the window count (at most cap written), or -WT_ERR_INVALID_ARG when the last synchronous decode was not a
 * seeking one */
int wt_last_windows(const wt_engine* h, wt_window* out, int cap);

/* Seeking transcription of n_files (1..64) recordings side by side (options as for wt_transcribe_long_pcm with "seek" = 1;
 * the option "seek" itself is not read).  Every round decodes the next window of every file still running as ONE batch
 * behind per-clip contexts (wt_engine_set_contexts), then every file takes the step of the seeking loop on its own clip;
 * a file that has reached its end leaves the batch.  A file's result is by definition what wt_transcribe_long_pcm with
 * "seek" = 1 gives for that file alone: window w of a file has clip index w in the sampling counter, the caller's
 * wt_engine_set_context ids seed every file's first window, and both kinds of context are the caller's again after the
 * call.  wt_last_windows then lists the windows file by file and wt_last_window_files is parallel to it;
 * wt_last_segments has clip = index into that list and times in the file; wt_last_scores, wt_last_token_logprobs,
 * wt_last_segment_scores and wt_last_decode_info have one entry per window in the same order; wt_last_file_text returns
 * a file's lines joined by '\n'.  WT_ERR_UNSUPPORTED: "word_timestamps" = 1, more than 64 files, "condition_on_previous_text"
 * = 1 on a vocabulary without <|startofprev|> (as wt_transcribe_long_pcm), and whatever full-length decoding refuses (the bf16 storage mode, the pipeline, beam_size > 1,
 * language = WT_LANGUAGE_AUTO). */
int wt_transcribe_long_batch(wt_engine* h, const float* const* pcm, const size_t* n_samples, int n_files);
/* text of file `file` of the last wt_transcribe_long_batch (as wt_last_text: *len = its length, WT_ERR_BUFFER when cap
 * is too small); WT_ERR_INVALID_ARG when the last synchronous decode was another call or for a file outside it */
int wt_last_file_text(const wt_engine* h, int file, char* out, size_t cap, size_t* len);
/* parallel to wt_last_windows: the file of every window; returns the window count (at most cap written), or
 * -WT_ERR_INVALID_ARG when the last synchronous decode was not wt_transcribe_long_batch */
int wt_last_window_files(const wt_engine* h, int32_t* file, int cap);

/* Per-kernel-class device time of the encoder phase of the last batch call: HIP event pairs
 * recorded on the engine's stream around every launch of the class.  flops / bytes are the
 * ALGORITHMIC work of those launches (2*M*N*K per GEMM with the true K, 4*B*H*T*T*64 per
 * attention, read+write bytes for bandwidth-bound kernels).  Returns the number of classes
 * (<= cap entries written). */
typedef struct wt_kernel_stat {
  char name[48];
  int32_t launches;
  int32_t reserved;
  double ms, flops, bytes;
} wt_kernel_stat;
int wt_last_kernel_stats(const wt_engine* h, wt_kernel_stat* out, int cap);

/* ---- host-side helpers of the path ------------------------------------------------------ */
/* whisper.cpp:634-665 decode() over the engine's vocab. */
int wt_decode_text(wt_engine* h, const int64_t* ids, int n, int omit_special_tokens, char* out,
                   size_t cap, size_t* len);
/* whisper.cpp:510-515 / :517 language table (returns the table size, 100, when absent). */
int wt_language_id(const char* code);
const char* wt_lang_code(int id);
/* wav_util.cpp:18-87 wav_read_legacy: *n gets the sample count (WT_ERR_IO when the reference
 * would return an empty vector); at most cap samples are written. */
int wt_wav_read_legacy(const char* path, float* out, size_t cap, size_t* n);
/* token ids the engine uses: out[0..8] = n_vocab, eot, sot, translate, transcribe, prev,
 * solm, not, beg (whisper.h:69-91 after whisper.cpp:218-226). */
int wt_vocab_info(const wt_engine* h, int32_t out[9]);
/* mel filter bank as loaded from the vocab file: [n_mel][n_fft]; returns element count. */
int wt_filters(const wt_engine* h, float* out, size_t cap, int32_t* n_mel, int32_t* n_fft);

/* ---- vocab / filter file on the host (no GPU needed) --------------------------------------
 * Replace MmapFile + Reader::read (mmap_file.cpp:13-31, whisper.cpp:519-611, :746-749), Vocab
 * (whisper.h:44-94) and decode() (whisper.cpp:634-665) for callers that only need the tables. */
typedef struct wt_vocab wt_vocab;
int wt_vocab_open(const char* vocab_path, int multilingual, wt_vocab** out);
void wt_vocab_close(wt_vocab* v);
/* out[0..8] as wt_vocab_info */
int wt_vocab_get_info(const wt_vocab* v, int32_t out[9]);
/* as wt_filters */
int wt_vocab_get_filters(const wt_vocab* v, float* out, size_t cap, int32_t* n_mel, int32_t* n_fft);
/* number of id -> token entries (file tokens + synthesised specials) */
int wt_vocab_size(const wt_vocab* v);
/* bytes of one token (WT_ERR_INVALID_ARG when the id has no entry) */
int wt_vocab_token(const wt_vocab* v, int id, char* out, size_t cap, size_t* len);
int wt_vocab_decode(const wt_vocab* v, const int64_t* ids, int n, int omit_special_tokens, char* out,
                    size_t cap, size_t* len);
/* the segments (see wt_last_segments; clip = 0) of one id row of n ids whose first sample_begin are the prompt; no GPU.
 * Returns the segment count (at most cap written), or -WT_ERR_INVALID_ARG. */
int wt_vocab_segments(const wt_vocab* v, const int64_t* ids, int n, int sample_begin, wt_segment* out, int cap);
/* Whisper's seek rule on the n ids g a window generated before its first EOT; no GPU.  ts(i) = g[i] >= token_beg,
 * tick(id) = id - token_beg clamped to [0, win_ticks]; seg_ticks (<= win_ticks) = the ticks of audio the window holds.
 * With pairs of consecutive timestamps the row is cut at the second of each pair, and at n when it ends in a single
 * timestamp; every slice is a segment from the tick of its first id to the tick of its last, *advance_ticks = the tick of
 * the id before the last cut (seg_ticks when the row ends in a single timestamp), and ids behind the last cut belong to
 * no segment.  Without a pair the whole row is one segment from 0 to the last timestamp's tick, or to seg_ticks with
 * open = 1 when there is none or it is tick 0, and *advance_ticks = seg_ticks.  A segment with no id below EOT or with
 * t0 == t1 is dropped; an advance of 0 becomes seg_ticks.  Segments: clip = 0, times = tick x 20 ms, g[id_begin ..
 * id_begin + id_count) the slice, timestamps included.  Returns the segment count (at most cap written), or
 * -WT_ERR_INVALID_ARG. */
int wt_vocab_seek_step(const wt_vocab* v, const int64_t* g, int n, int win_ticks, int seg_ticks, wt_segment* out, int cap,
                       int32_t* advance_ticks);

/* Whisper's default suppression lists from a vocabulary; no GPU.  first_ids: the id whose bytes are exactly " " (if the
 * vocabulary has one) and EOT.  ids: those of sot, translate, transcribe, <|startoflm|> (the id in front of prev: 50360
 * multilingual; wt_vocab_info does not name it), prev and solm (this table's name of the <|nospeech|> id; multilingual
 * 50258 and 50358 .. 50362) that lie below n_vocab, then the non-speech symbols, typed out in csrc/host_util.cpp: for every symbol s of
 * Whisper's non_speech_tokens list the id whose bytes are exactly s and the one whose bytes are exactly " " + s, the exact
 * " -" and " '", and for the musical symbols ♩♪♫♬♭♮♯ a string without an exact match gives the longest token whose
 * bytes are a proper prefix of it (behind the leading space of " " + s the prefix must reach into the symbol: the bare
 * " " is never taken), the smallest id on equal length.  Text matches are ids below EOT.  This prefix rule is NOT
 * byte-pair encoding: the list equals Whisper's wherever Whisper's encoder yields that prefix token first, which holds
 * for its own vocabularies, and may differ on another vocabulary.  Both lists come back sorted and unique; *n and
 * *n_first get the full counts, at most cap / first_cap ids are written, WT_ERR_BUFFER when either is too small. */
int wt_vocab_default_suppress(const wt_vocab* v, int64_t* ids, int cap, int32_t* n, int64_t* first_ids, int first_cap,
                              int32_t* n_first);

/* ---- word-level timestamps -------------------------------------------
 * Option "word_timestamps" = 1 (default 0; needs "timestamps" = 1, "max_positions" and the absorbed cross-attention the
 * default weights and gemm_variant give: otherwise every decode call is WT_ERR_UNSUPPORTED and the engine stays usable).  After the decode, and after the temperature fall-back, every clip's row prompt + <|notimestamps|>
 * + text + EOT is fed through the decoder once more, teacher-forced; the cross-attention weights of the alignment heads
 * over the clip's valid frames are normalised per frame over the positions, median-filtered (7 wide, reflect padding),
 * averaged over the heads and dynamic-time-warped against the ids on the device (Whisper's find_alignment), and the path
 * is cut into words by wt_vocab_split_words and wt_vocab_merge_punctuation.  text = the ids below EOT of the clip's
 * segments; at most n_text_ctx - prompt - 2 of them are aligned, the rest form no words.  A clip that came in as PCM
 * (wt_transcribe_pcm, _file, _long_pcm) is aligned over the frames of its own samples, floor(samples / 320), at least 1;
 * any other clip over all n_audio_ctx frames.  Not reproduced from Whisper: the duration heuristics of
 * add_word_timestamps, moving the seek position to the last word, other punctuation sets.
 * Alignment heads: n (layer, head) pairs, at most 128; n = 0 restores the default, every head of the upper half of the
 * decoder layers.  WT_ERR_INVALID_ARG for a pair outside the model, a duplicate or n > 128.  The read-only option
 * "alignment_heads" gives the count in effect. */
int wt_engine_set_alignment_heads(wt_engine* h, const int32_t* layer_head /* [n][2] */, int n);
/* One word: ids[id_begin .. id_begin + id_count) of clip `clip`'s id row (a word that spans a timestamp id counts it),
 * spoken from t0_ms to t1_ms (20 ms steps), inside segment `segment` of wt_last_segments (that of its first id);
 * probability = the mean over its ids of exp(token log-probability) of the decode itself (wt_last_token_logprobs), 0
 * when the decode ran without "scores".  After wt_transcribe_long_pcm clip is the window index and the times are the
 * file's: 30 000 ms per window, or with "seek" = 1 the window's seek_sample / 16 ms, the text being the ids below EOT of
 * the segments wt_vocab_seek_step kept of the window. */
typedef struct wt_word {
  int32_t clip, segment, t0_ms, t1_ms, id_begin, id_count;
  float probability;
} wt_word;
/* the words of the last synchronous decode, in clip order: returns their count (at most cap written), or
 * -WT_ERR_INVALID_ARG when that decode ran without "word_timestamps" */
int wt_last_words(const wt_engine* h, wt_word* out, int cap);
/* the ids below EOT of word `index`, decoded */
int wt_last_word_text(const wt_engine* h, int index, char* out, size_t cap, size_t* len);

/* ---- word-level timestamps: the host half (no GPU needed) -----------
 * Whisper's split_to_word_tokens on a row of n ids (a clip's text ids, then EOT): word_len_out gets the id counts of
 * the words, in order; they add up to n.  First the ids are grouped into complete UTF-8 sequences over the vocabulary's
 * bytes: a group is closed when it decodes without U+FFFD, or when the whole row has U+FFFD at the place of the group's
 * first one (ill-formed bytes are replaced as Python's decode(errors="replace") replaces them).  unicode_only != 0
 * (zh, ja, th, lo, my, yue): these groups are the words.  Otherwise a group starts a word when it is the first, its first
 * id is >= EOT, its bytes begin with a space or, stripped of ASCII white space, are one ASCII punctuation character;
 * any other group joins the word before it.  Returns the word count (at most cap written), or -WT_ERR_INVALID_ARG. */
int wt_vocab_split_words(const wt_vocab* v, const int64_t* ids, int n, int unicode_only, int32_t* word_len_out, int cap);
/* Whisper's merge_punctuations with its default marks on the words word_len[0 .. n_words) of a row of n ids (counts
 * that add up to n).  From the back, a word that begins with a space and is otherwise one of  " ' “ ¿ ( [ { -  is put in
 * front of the word behind it; then, from the front, a word that is exactly one of  " ' . 。 , ， ! ！ ? ？ : ： ” ) ] } 、
 * is put behind the word before it unless that one ends in a space.  merged_len_out gets the id counts of the merged
 * words, in order (they add up to n: a merged word is the id run of its parts).  Returns the merged word count (at most
 * cap written), or -WT_ERR_INVALID_ARG. */
int wt_vocab_merge_punctuation(const wt_vocab* v, const int64_t* ids, int n, const int32_t* word_len, int n_words,
                               int32_t* merged_len_out, int cap);
/* Dynamic time warping as Whisper's find_alignment runs it, in fp32, over cost [N][F]: D[0][0] = 0, the rest of row 0 and
 * column 0 +inf, D[i][j] = cost[i - 1][j - 1] + min(c0, c1, c2) with c0 = D[i - 1][j - 1], c1 = D[i - 1][j], c2 = D[i][j - 1];
 * the step taken is c0's when c0 < c1 and c0 < c2, else c1's when c1 < c0 and c1 < c2, else c2's, and the path runs back
 * from (N, F).  jump [N] gets the first frame of the path in each row; path_out (may be NULL) the (row, frame) pairs from
 * (0, 0) to (N - 1, F - 1), at most path_cap pairs.  1 <= N <= 447, 1 <= F <= 1500.  Returns the number of path cells, or
 * -WT_ERR_INVALID_ARG. */
int wt_dtw_path(const float* cost, int N, int F, int32_t* jump, int32_t* path_out, int path_cap);

/* ---- the log-mel front end as a free function ---------------------------------------------
 * Replaces whisper::log_mel_spectrogram (whisper.h:123, whisper.cpp:109-216) for callers that hold a
 * Filters table but no engine: the same gfx950 kernels the engine uses, on `device_id`, through a
 * process-wide front-end context created at the first call.  Only the reference's fixed geometry is
 * provided (16 kHz, fft 400, hop 160, 80 x 201 filters, n_samples <= 480000), anything else is
 * WT_ERR_UNSUPPORTED.  mel_out [n_mel][n_len] with n_len = n_samples / 160, the layout of Mel::data.
 * At most four contexts (device x filter table) are kept, least recently used evicted; wt_shutdown() releases
 * them (call it before unloading the library / at exit, ahead of the HIP runtime's own teardown). */
void wt_shutdown(void);
int wt_log_mel_spectrogram(const float* samples, int n_samples, const float* filters, int n_mel,
                           int n_fft_bins, int device_id, float* mel_out, size_t cap, int* n_len);

/* ---- asset tooling (stand-ins for the reference's offline export) -------- */
/* Weight extractor: reads the reference's model pair "<prefix>.encoder.tflite" + "<prefix>.decoder.tflite"
 * (TFLite FlatBuffers, parsed by hand; float32 / float16 constants and dynamic-range int8 weights with
 * per-tensor or per-axis scales are de-quantised) and writes "<out_path>" in .wtw format.  Tensors are
 * identified by shape and by their position in each graph's operator order (csrc/tflite_extract.cpp). */
int wt_convert_tflite(const char* model_prefix, const char* out_path);
/* Deterministic random-init weights of a named architecture ("tiny", "tiny.en", "base",
 * "micro") -> "<path>" in .wtw format. */
int wt_write_synthetic_weights(const char* path, const char* arch, uint64_t seed);
/* filters+vocab .bin in the reference layout with a Slaney 80x201 bank and n_tokens
 * synthetic tokens. */
int wt_write_synthetic_vocab(const char* path, int n_tokens);

#ifdef __cplusplus
}
#endif
#endif /* WT_CAPI_H_ */
