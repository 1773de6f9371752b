// extern "C" boundary (include/wt_capi.h): exception-free wrappers over wt::Engine.
#include "wt_capi.h"

#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "kernels.h"
#include "longform.h"
#include "tflite_extract.h"
#include "weights_gen.h"
#include "words.h"

namespace {
thread_local std::string g_create_error;
}  // namespace

int fail(wt_engine* h, int code, const std::string& msg) {
  if (h) {
    h->last_error = msg;
  } else {
    g_create_error = msg;
  }
  return code;
}

namespace {
int copy_text(const std::string& s, char* out, size_t cap, size_t* len) {
  if (len) *len = s.size();
  if (out && cap > 0) {
    const size_t n = std::min(s.size(), cap - 1);
    std::memcpy(out, s.data(), n);
    out[n] = 0;
  }
  return (out && s.size() + 1 <= cap) ? WT_OK : WT_ERR_BUFFER;
}

// the token calls with rows of WT_MAX_IDS ids cannot return a full-length decode
void refuse_fixed_rows(const wt::Engine& e) {
  e.check_timestamp_call();
  if (e.max_positions > 0) {
    throw wt::Error(WT_ERR_UNSUPPORTED, "max_positions is set: rows of WT_MAX_IDS ids cannot hold the result, use the "
                                        "wt_*_tokens_full_batch* entry points (or set max_positions to 0)");
  }
}

}  // namespace

namespace {
// Where a converted model goes when its own directory is read-only: $XDG_CACHE_HOME/whisper-tflite-amd (or
// ~/.cache/..., or a per-uid directory under $TMPDIR), created 0700 and accepted only if it IS a directory owned by this
// user that nobody else may write (a predictable name in a shared /tmp could be pre-planted, also as a symlink).
std::string cache_path_for(const std::string& prefix, bool create = true) {
  std::string dir;
  const char* x = getenv("XDG_CACHE_HOME");
  const char* home = getenv("HOME");
  const char* t = getenv("TMPDIR");
  if (x && *x) dir = std::string(x) + "/whisper-tflite-amd";
  else if (home && *home) dir = std::string(home) + "/.cache/whisper-tflite-amd";
  else dir = std::string(t && *t ? t : "/tmp") + "/whisper-tflite-amd-" + std::to_string(static_cast<long>(::getuid()));
  struct stat st;
  if (create) {
    const size_t slash = dir.rfind('/');
    if (slash != std::string::npos && slash > 0) (void)::mkdir(dir.substr(0, slash).c_str(), 0700);  // ~/.cache itself
    (void)::mkdir(dir.c_str(), 0700);
  }
  if (::lstat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || st.st_uid != ::getuid() || (st.st_mode & 022) != 0) {
    if (!create) return std::string();
    throw wt::Error(wt::kErrIo, "no private cache directory for the converted model: " + dir);
  }
  return dir + "/wt-" + std::to_string(std::hash<std::string>{}(prefix)) + ".wtw";
}
}  // namespace

extern "C" {

int wt_engine_create(int engine_type, const char* model_prefix, const char* vocab_path,
                     int multilingual, int device_id, wt_engine** out) {
  if (!out) return fail(nullptr, WT_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  if (!model_prefix || !vocab_path) return fail(nullptr, WT_ERR_INVALID_ARG, "NULL path");
  if (engine_type != WT_ENGINE_ENCDEC && engine_type != WT_ENGINE_MONOLITH) {
    return fail(nullptr, WT_ERR_INVALID_ARG, "Unknown engine-type");
  }
  std::unique_ptr<wt_engine> h(new wt_engine);
  const int rc = guarded(nullptr, [&] {
    const std::string prefix(model_prefix);
    // the reference's users hold <prefix>.encoder.tflite / .decoder.tflite (whisper.cpp:743-744): extract
    // their weights once when no .wtw sits next to them.  The converted file is renamed into place atomically
    // (wtw::write_tensors), so ranks that start together on one prefix never read a half-written file; a model
    // directory that cannot be written falls back to a file under $TMPDIR; and a .wtw that is there but broken (a
    // conversion killed before the atomic writer existed, a truncated copy) is rebuilt from the pair once.
    const bool have_pair = wt::file_exists(prefix + ".encoder.tflite") && wt::file_exists(prefix + ".decoder.tflite");
    std::string wpath = prefix + ".wtw";
    bool converted = false;
    auto convert = [&] {
      try {
        wt::convert_tflite(prefix, wpath);
      } catch (const wt::Error& e) {
        if (e.code != wt::kErrIo) throw;
        wpath = cache_path_for(prefix);  // a per-user 0700 directory: nobody else can plant or swap the file
        wt::convert_tflite(prefix, wpath);
      }
      converted = true;
    };
    // a model directory that cannot be written: an earlier run's conversion in the user's cache is taken as it is when it
    // passes the header check (a read-only directory no longer means converting the model at every start)
    if (!wt::file_exists(wpath) && have_pair) {
      const std::string cached = cache_path_for(prefix, false);
      if (!cached.empty() && wt::file_exists(cached)) {
        try {
          wt::check_wtw_file(cached);
          wpath = cached;
        } catch (const wt::Error&) {
        }
      }
    }
    if (!wt::file_exists(wpath) && have_pair) convert();
    if (have_pair && !converted) {
      try {
        wt::check_wtw_file(wpath);  // host-only: header, tensor table, length
      } catch (const wt::Error& e) {
        if (e.code != wt::kErrFormat) throw;
        convert();
      }
    }
    auto make = [&] {
      h->impl.reset(new wt::Engine(prefix, vocab_path, multilingual != 0, device_id, engine_type == WT_ENGINE_MONOLITH, wpath));
    };
    try {
      make();
    } catch (const wt::Error& e) {
      if (e.code != wt::kErrFormat || !have_pair || converted) throw;
      convert();
      make();
    }
  });
  if (rc != WT_OK) return rc;
  *out = h.release();
  return WT_OK;
}

void wt_engine_destroy(wt_engine* h) { delete h; }

const char* wt_last_error(const wt_engine* h) {
  return h ? h->last_error.c_str() : g_create_error.c_str();
}

int wt_engine_dims(const wt_engine* h, wt_dims* out) {
  if (!h || !out) return WT_ERR_INVALID_ARG;
  static_assert(sizeof(wt_dims) == sizeof(wtw::Dims), "wt_dims mirrors wtw::Dims");
  std::memcpy(out, &h->impl->dims(), sizeof(wt_dims));
  return WT_OK;
}

int wt_engine_set_option(wt_engine* h, const char* key, long value) {
  if (!h || !key) return WT_ERR_INVALID_ARG;
  wt::Engine& e = *h->impl;
  const std::string k(key);
  if (k == "language") {
    try {  // WT_LANGUAGE_AUTO (-1): detected per clip; unsupported on a Monolith engine or without language tokens
      e.set_language(value);
    } catch (const wt::Error& err) {
      return fail(h, err.code, err.what());
    }
  } else if (k == "max_tokens") {
    if (value < 4 || value > 31) return fail(h, WT_ERR_INVALID_ARG, "max_tokens must be in [4, 31]");
    e.max_tokens = value;
  } else if (k == "max_positions") {
    // full-length greedy decoding: 0 = off, else the positions fed per clip
    if (value != 0 && (value < 32 || value > e.full_cap())) {
      return fail(h, WT_ERR_INVALID_ARG, "max_positions must be 0 (off) or in [32, n_text_ctx] (at most 448)");
    }
    e.max_positions = value;
  } else if (k == "timestamps") {
    // timestamp decoding: full-length greedy decoding behind Whisper's timestamp rules
    if (value != 0 && value != 1) return fail(h, WT_ERR_INVALID_ARG, "timestamps must be 0 or 1");
    if (value == 1 && !e.has_timestamp_tokens()) {
      return fail(h, WT_ERR_UNSUPPORTED, "timestamps: the model's vocabulary has no timestamp ids (n_vocab <= token_beg + 1)");
    }
    e.timestamps = value;
  } else if (k == "scores") {
    // decode confidence: token log-probabilities, avg_logprob and no_speech_prob of a full-length decode
    if (value != 0 && value != 1) return fail(h, WT_ERR_INVALID_ARG, "scores must be 0 or 1");
    if (value == 1 && !e.has_no_speech_token()) {
      return fail(h, WT_ERR_UNSUPPORTED, "scores: the model's vocabulary has no <|nospeech|> id (token_solm >= n_vocab)");
    }
    e.scores = value;
  } else if (k == "skip_silence") {
    if (value != 0 && value != 1) return fail(h, WT_ERR_INVALID_ARG, "skip_silence must be 0 or 1");
    e.skip_silence = value;
  } else if (k == "no_speech_threshold") {
    if (value < 0 || value > 1000) return fail(h, WT_ERR_INVALID_ARG, "no_speech_threshold must be in [0, 1000] (thousandths)");
    e.no_speech_threshold = value;
  } else if (k == "logprob_threshold") {
    if (value > 0 || value < -1000000) return fail(h, WT_ERR_INVALID_ARG, "logprob_threshold must be in [-1000000, 0] (thousandths)");
    e.logprob_threshold = value;
  } else if (k == "temperature") {
    // temperature sampling, thousandths: 0 = greedy
    if (value < 0 || value > 1000) return fail(h, WT_ERR_INVALID_ARG, "temperature must be in [0, 1000] (thousandths)");
    e.temperature = value;
  } else if (k == "temperature_fallback") {
    if (value != 0 && value != 1) return fail(h, WT_ERR_INVALID_ARG, "temperature_fallback must be 0 or 1");
    e.temperature_fallback = value;
  } else if (k == "temperature_increment") {
    if (value < 1 || value > 1000) return fail(h, WT_ERR_INVALID_ARG, "temperature_increment must be in [1, 1000] (thousandths)");
    e.temperature_increment = value;
  } else if (k == "compression_ratio_threshold") {
    if (value < 0 || value > 1000000) return fail(h, WT_ERR_INVALID_ARG, "compression_ratio_threshold must be in [0, 1000000] (thousandths, 0 = off)");
    e.compression_ratio_threshold = value;
  } else if (k == "seed") {
    e.seed = value;  // all 64 bits are the Philox key
  } else if (k == "best_of") {
    // samples per clip of an attempt above temperature 0 in a full-length decode, 1 = one
    if (value < 1 || value > wt::kSampleGroupMax) return fail(h, WT_ERR_INVALID_ARG, "best_of must be in [1, 8]");
    e.best_of = value;
  } else if (k == "fallback_beam") {
    // with full_beam = 1 and beam_size 2..8: the fall-back's attempt at temperature 0 is beam search
    if (value < 0 || value > 1) return fail(h, WT_ERR_INVALID_ARG, "fallback_beam must be 0 or 1");
    e.fallback_beam = value;
  } else if (k == "max_initial_timestamp") {
    if (value < -1 || value > 1500) return fail(h, WT_ERR_INVALID_ARG, "max_initial_timestamp must be in [-1, 1500] (ticks of 20 ms, -1 = no limit)");
    e.max_initial_timestamp = value;
  } else if (k == "prompt_group") {
    // prompt passes behind a context: 0 = as many positions as a pass takes, 1 = one position each
    if (value != 0 && value != 1) return fail(h, WT_ERR_INVALID_ARG, "prompt_group must be 0 (grouped) or 1 (one position per pass)");
    e.prompt_group = value;
  } else if (k == "seek") {
    // seeking long-audio transcription: wt_transcribe_long_pcm follows the timestamps
    if (value != 0 && value != 1) return fail(h, WT_ERR_INVALID_ARG, "seek must be 0 or 1");
    e.seek = value;
  } else if (k == "condition_on_previous_text") {
    if (value != 0 && value != 1) return fail(h, WT_ERR_INVALID_ARG, "condition_on_previous_text must be 0 or 1");
    e.condition_on_previous_text = value;
  } else if (k == "word_timestamps") {
    // word-level timestamps: the alignment pass behind a timestamp decode
    if (value != 0 && value != 1) return fail(h, WT_ERR_INVALID_ARG, "word_timestamps must be 0 or 1");
    e.word_timestamps = value;
  } else if (k == "stop_at_eot") {
    e.stop_at_eot = value != 0;
  } else if (k == "verbose") {
    e.verbose = value;
  } else if (k == "cross_chunks") {
    if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8) return fail(h, WT_ERR_INVALID_ARG, "cross_chunks must be 0 (by batch size), 1, 2, 4 or 8");
    e.cross_chunks = value;
  } else if (k == "attn_variant") {
    if (value != 0 && value != 1 && value != 4) return fail(h, WT_ERR_INVALID_ARG, "attn_variant must be 4 (default: two fp16 planes), 1 (three bf16 planes, full range) or 0 (fp32 MFMA)");
    e.attn_variant = value;
  } else if (k == "fc2_ksplit") {
    if (value != 1 && value != 2) return fail(h, WT_ERR_INVALID_ARG, "fc2_ksplit must be 1 or 2");
    e.fc2_ksplit = value;
  } else if (k == "use_graphs") {
    e.use_graphs = value != 0;
  } else if (k == "cross_absorb") {
    e.cross_absorb = value != 0;
  } else if (k == "last_batches") {
    if (value < 0 || value > WT_PIPELINE_DEPTH) return fail(h, WT_ERR_INVALID_ARG, "last_batches: 0..24");
    e.last_batches = value;
  } else if (k == "dec_pair") {
    if (h->impl->in_flight() > 0) return fail(h, WT_ERR_INVALID_ARG, "collect the submitted batches before changing dec_pair");
    e.dec_pair = value != 0;
  } else if (k == "dec_group") {
    if (h->impl->in_flight() > 0) return fail(h, WT_ERR_INVALID_ARG, "collect the submitted batches before changing dec_group");
    if (value < 2 || value > 4) return fail(h, WT_ERR_INVALID_ARG, "dec_group: 2, 3 or 4 batches per decoder chain (dec_pair = 0 turns grouping off)");
    e.dec_group = value;
  } else if (k == "abs_chunks") {
    if (value < 0 || value > 16) return fail(h, WT_ERR_INVALID_ARG, "abs_chunks must be 0 (automatic) or 1..16");
    e.abs_chunks = value;
  } else if (k == "gemm_variant") {
    if (value != -1 && !wt::gemm_variant_supported(int(value))) {
      return fail(h, WT_ERR_INVALID_ARG, "gemm_variant must be -1 (default: plane GEMM), 0 (fp32 MFMA), 13 or 16 (three bf16 planes)");
    }
    e.gemm_variant = value;
  } else if (k == "force_fallback") {
    // test hook: bit i flags contraction i (launch order) as if the load-time slack check had (engine.h)
    try {
      e.set_force_fallback(value);
    } catch (const wt::Error& err) {
      return fail(h, err.code, err.what());
    }
  } else if (k == "kernel_timers") {
    if (value < 0 || value > 1024) return fail(h, WT_ERR_INVALID_ARG, "kernel_timers must be in [0, 1024]");
    e.kernel_timers = value;
  } else if (k == "beam_size") {
    if (value < 1 || value > wt::kBeamMax) return fail(h, WT_ERR_INVALID_ARG, "beam_size must be in [1, 8] (1 = greedy)");
    e.beam_size = value;
  } else if (k == "full_beam") {
    if (value < 0 || value > 1) return fail(h, WT_ERR_INVALID_ARG, "full_beam must be 0 or 1");
    e.full_beam = value;
  } else if (k == "full_bf16") {
    // full-length decoding in the bf16 storage mode: 0 = such a call is refused, 1 = it runs
    if (value < 0 || value > 1) return fail(h, WT_ERR_INVALID_ARG, "full_bf16 must be 0 or 1");
    e.full_bf16 = value;
  } else if (k == "full_bf16_all") {
    // contexts, batched seeking, automatic language and word timestamps in that mode: 0 = refused
    if (value < 0 || value > 1) return fail(h, WT_ERR_INVALID_ARG, "full_bf16_all must be 0 or 1");
    e.full_bf16_all = value;
  } else if (k == "full_language") {
    // automatic language behind max_positions: 0 = such a call is refused, 1 = detected per clip
    if (value < 0 || value > 1) return fail(h, WT_ERR_INVALID_ARG, "full_language must be 0 or 1");
    e.full_language = value;
  } else if (k == "task") {
    try {  // 0 = transcribe, 1 = translate; unsupported on an English-only or Monolith engine or without <|translate|>
      e.set_task(value);
    } catch (const wt::Error& err) {
      return fail(h, err.code, err.what());
    }
  } else if (k == "language_candidates") {
    return fail(h, WT_ERR_INVALID_ARG, "language_candidates is read-only: wt_engine_set_language_candidates sets the list");
  } else if (k == "suppress_default") {
    // logit suppression: 1 = Whisper's default lists from the engine's vocabulary, 0 = none
    if (value < 0 || value > 1) return fail(h, WT_ERR_INVALID_ARG, "suppress_default must be 0 or 1");
    try {
      e.set_suppress_default(value == 1);
    } catch (const wt::Error& err) {
      return fail(h, err.code, err.what());
    } catch (const std::exception& err) {
      return fail(h, WT_ERR_DEVICE, err.what());
    }
  } else if (k == "bf16") {
    // bf16 storage mode (BASELINE configs[3]); the first switch reads the weight file again for the bf16 copies
    try {
      e.bind_device();
      e.set_bf16(value != 0);
    } catch (const wt::Error& err) {
      return fail(h, err.code, err.what());
    } catch (const std::exception& err) {
      return fail(h, WT_ERR_DEVICE, err.what());
    }
  } else {
    return fail(h, WT_ERR_INVALID_ARG, "unknown option: " + k);
  }
  return WT_OK;
}

int wt_engine_set_prompt(wt_engine* h, const int64_t* ids, int n) {
  if (!h || n < 0 || n > 8 || (n && !ids)) return WT_ERR_INVALID_ARG;
  h->impl->prompt_override.assign(ids, ids + n);
  return WT_OK;
}

int wt_engine_set_context(wt_engine* h, const int64_t* ids, int n) {
  if (!h) return WT_ERR_INVALID_ARG;
  try {
    h->impl->set_context(ids, n);
  } catch (const wt::Error& err) {
    return fail(h, err.code, err.what());
  }
  return WT_OK;
}

int wt_engine_set_contexts(wt_engine* h, const int64_t* ids, const int32_t* offsets, int n_clips) {
  if (!h) return WT_ERR_INVALID_ARG;
  try {
    h->impl->set_contexts(ids, offsets, n_clips);
  } catch (const wt::Error& err) {
    return fail(h, err.code, err.what());
  }
  return WT_OK;
}

int wt_engine_set_suppress(wt_engine* h, const int64_t* ids, int n, const int64_t* first_ids, int n_first) {
  if (!h) return WT_ERR_INVALID_ARG;
  try {
    h->impl->set_suppress(ids, n, first_ids, n_first);
  } catch (const wt::Error& err) {
    return fail(h, err.code, err.what());
  } catch (const std::exception& err) {
    return fail(h, WT_ERR_DEVICE, err.what());
  }
  return WT_OK;
}

int wt_engine_set_alignment_heads(wt_engine* h, const int32_t* layer_head, int n) {
  if (!h) return WT_ERR_INVALID_ARG;
  try {
    h->impl->set_alignment_heads(layer_head, n);
  } catch (const wt::Error& err) {
    return fail(h, err.code, err.what());
  }
  return WT_OK;
}

int wt_engine_get_option(const wt_engine* h, const char* key, long* value) {
  if (!h || !key || !value) return WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  const std::string k(key);
  if (k == "language") *value = e.language;
  else if (k == "max_tokens") *value = e.max_tokens;
  else if (k == "max_positions") *value = e.max_positions;
  else if (k == "timestamps") *value = e.timestamps;
  else if (k == "max_initial_timestamp") *value = e.max_initial_timestamp;
  else if (k == "scores") *value = e.scores;
  else if (k == "skip_silence") *value = e.skip_silence;
  else if (k == "no_speech_threshold") *value = e.no_speech_threshold;
  else if (k == "logprob_threshold") *value = e.logprob_threshold;
  else if (k == "temperature") *value = e.temperature;
  else if (k == "temperature_fallback") *value = e.temperature_fallback;
  else if (k == "temperature_increment") *value = e.temperature_increment;
  else if (k == "compression_ratio_threshold") *value = e.compression_ratio_threshold;
  else if (k == "seed") *value = e.seed;
  else if (k == "best_of") *value = e.best_of;
  else if (k == "fallback_beam") *value = e.fallback_beam;
  else if (k == "prompt_group") *value = e.prompt_group;
  else if (k == "seek") *value = e.seek;
  else if (k == "condition_on_previous_text") *value = e.condition_on_previous_text;
  else if (k == "word_timestamps") *value = e.word_timestamps;
  else if (k == "alignment_heads") *value = long(e.alignment_heads_in_effect().size());  // read-only: the count in effect
  else if (k == "context_ids") *value = long(e.context_ids.size());  // read-only: ids kept by wt_engine_set_context
  else if (k == "context_clips") *value = long(e.clip_contexts.size());  // read-only: clips given to wt_engine_set_contexts
  else if (k == "suppress_ids") *value = long(e.suppress_ids.size());  // read-only: the lists of wt_engine_set_suppress in effect
  else if (k == "suppress_first_ids") *value = long(e.suppress_first_ids.size());
  else if (k == "graphs_cached") *value = e.graphs_cached();          // read-only: captured decoder graphs held
  else if (k == "stop_at_eot") *value = e.stop_at_eot;
  else if (k == "verbose") *value = e.verbose;
  else if (k == "cross_chunks") *value = e.cross_chunks;
  else if (k == "gemm_variant") *value = e.gemm_variant;
  else if (k == "use_graphs") *value = e.use_graphs;
  else if (k == "cross_absorb") *value = e.cross_absorb;
  else if (k == "abs_chunks") *value = e.abs_chunks;
  else if (k == "dec_pair") *value = e.dec_pair;
  else if (k == "dec_group") *value = e.dec_group;
  else if (k == "last_batches") *value = e.last_batches;
  else if (k == "cross_absorb_active") *value = e.absorb_active() ? 1 : 0;  // read-only
  else if (k == "bf16") *value = e.bf16;
  else if (k == "beam_size") *value = e.beam_size;
  else if (k == "full_beam") *value = e.full_beam;
  else if (k == "full_language") *value = e.full_language;
  else if (k == "full_bf16") *value = e.full_bf16;
  else if (k == "full_bf16_all") *value = e.full_bf16_all;
  else if (k == "task") *value = e.task;
  else if (k == "language_candidates") *value = long(e.language_candidates.size());
  else if (k == "kernel_timers") *value = e.kernel_timers;
  else if (k == "fc2_ksplit") *value = e.fc2_ksplit;
  else if (k == "attn_variant") *value = e.attn_variant;
  else if (k == "force_fallback") *value = e.force_fallback();
  else if (k == "f16_fallbacks") *value = e.f16_fallbacks();  // read-only
  else if (k == "f16_contractions") *value = e.f16_contractions();  // read-only: contractions the load-time check looked at
  else if (k == "f16_min_slack_millibits") *value = long(std::lround(1000.0 * e.f16_min_slack_bits()));  // read-only
  else if (k == "in_flight") *value = e.in_flight();          // read-only
  else if (k == "pipelined_encoder_cus") *value = e.pipelined_encoder_cus();  // read-only: CUs of the masked encoder stream
  else return WT_ERR_INVALID_ARG;
  return WT_OK;
}

// ------------------------------------------------------------- batches ---

int wt_device_alloc(wt_engine* h, size_t bytes, void** d_ptr) {
  if (!h || !d_ptr) return WT_ERR_INVALID_ARG;
  *d_ptr = nullptr;
  return guarded(h, [&] {
    h->impl->bind_device();
    hipchk(hipMalloc(d_ptr, bytes > 0 ? bytes : 4), "hipMalloc");
  });
}

int wt_device_free(wt_engine* h, void* d_ptr) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    h->impl->bind_device();
    if (d_ptr) hipchk(hipFree(d_ptr), "hipFree");
  });
}

int wt_device_upload(wt_engine* h, void* d_dst, size_t offset, const void* src, size_t bytes) {
  if (!h || !d_dst || (!src && bytes)) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    h->impl->bind_device();
    if (bytes) hipchk(hipMemcpy(static_cast<char*>(d_dst) + offset, src, bytes, hipMemcpyHostToDevice), "H2D");
  });
}

int wt_device_download(wt_engine* h, void* dst, const void* d_src, size_t offset, size_t bytes) {
  if (!h || !d_src || (!dst && bytes)) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    h->impl->bind_device();
    if (bytes) hipchk(hipMemcpy(dst, static_cast<const char*>(d_src) + offset, bytes, hipMemcpyDeviceToHost), "D2H");
  });
}

int wt_device_synchronize(wt_engine* h) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    h->impl->bind_device();
    hipchk(hipDeviceSynchronize(), "hipDeviceSynchronize");
  });
}

int wt_logmel_batch_dev(wt_engine* h, const float* d_pcm, int batch, float* d_mel) {
  if (!h || !d_pcm || !d_mel) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    h->impl->require_idle();
    h->impl->logmel(d_pcm, batch, d_mel);
    h->impl->sync();
  });
}

int wt_logmel_batch(wt_engine* h, const float* pcm, int batch, float* mel) {
  if (!h || !pcm || !mel) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    float* d_mel = e.staging_mel(batch);
    e.logmel(e.upload_pcm(pcm, batch), batch, d_mel);
    hipchk(hipMemcpyAsync(mel, d_mel, size_t(batch) * e.mel_elems() * sizeof(float), hipMemcpyDeviceToHost, e.stream()), "D2H mel");
    e.sync();
  });
}

int wt_encdec_tokens_batch_dev(wt_engine* h, const float* d_mel, int batch, int64_t* ids,
                               int32_t* n_ids) {
  if (!h || !d_mel || !ids || !n_ids || batch < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    refuse_fixed_rows(e);
    if (batch <= 64) {  // one encoder pass + one decode (the decoder kernels take up to 64 clips per pass)
      e.encode(d_mel, batch);
      e.decode(batch, ids, n_ids, nullptr, 0);
      return;
    }
    if (e.beam_size > 1) {  // beam search is synchronous: consecutive calls of up to 64 clips, their scores joined
      std::vector<float> sums;
      std::vector<int> lens;
      for (int b0 = 0; b0 < batch; b0 += 64) {
        const int nb = std::min(64, batch - b0);
        e.encode(d_mel + size_t(b0) * e.mel_elems(), nb);
        e.decode(nb, ids + size_t(b0) * WT_MAX_IDS, n_ids + b0, nullptr, 0);
        sums.insert(sums.end(), e.last.beam_sum.begin(), e.last.beam_sum.end());
        lens.insert(lens.end(), e.last.beam_len.begin(), e.last.beam_len.end());
      }
      e.last.beam_sum = sums;
      e.last.beam_len = lens;
      return;
    }
    // larger batches run as pipelined sub-batches of 32 clips: the encoder of a later
    // sub-batch overlaps the decoders of the earlier ones
    const int n_sub = (batch + 31) / 32;
    int submitted = 0, collected = 0;
    auto collect_one = [&] {
      e.collect(ids + size_t(collected) * 32 * WT_MAX_IDS, n_ids + size_t(collected) * 32);
      ++collected;
    };
    while (submitted < n_sub) {
      const int b0 = submitted * 32, nb = std::min(32, batch - b0);
      e.submit(d_mel + size_t(b0) * e.mel_elems(), nb);
      ++submitted;
      if (submitted - collected == 12) collect_one();  // (twelve in flight keep the pipeline full; WT_PIPELINE_DEPTH is the limit)
    }
    while (collected < submitted) collect_one();
  });
}

int wt_pipeline_submit_dev(wt_engine* h, const float* d_mel, int batch) {
  if (!h || !d_mel) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] { h->impl->submit(d_mel, batch); });
}

int wt_pipeline_submit_pcm_dev(wt_engine* h, const float* d_pcm, int batch) {
  if (!h || !d_pcm) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] { h->impl->submit_pcm(d_pcm, batch); });
}

int wt_pipeline_collect(wt_engine* h, int64_t* ids, int32_t* n_ids) {
  if (!h || !ids || !n_ids) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] { h->impl->collect(ids, n_ids); });
}

int wt_encdec_tokens_batch(wt_engine* h, const float* mel, int batch, int64_t* ids, int32_t* n_ids) {
  if (!h || !mel || !ids || !n_ids || batch < 1) return WT_ERR_INVALID_ARG;
  if (batch <= 32) return wt_encdec_debug_batch(h, mel, batch, ids, n_ids, nullptr, nullptr, 0);
  float* d_mel = nullptr;
  const int rc = guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    refuse_fixed_rows(e);
    d_mel = e.staging_mel(batch);
    hipchk(hipMemcpyAsync(d_mel, mel, size_t(batch) * e.mel_elems() * sizeof(float), hipMemcpyHostToDevice, e.stream()), "H2D mel");
  });
  if (rc != WT_OK) return rc;
  return wt_encdec_tokens_batch_dev(h, d_mel, batch, ids, n_ids);
}

int wt_transcribe_tokens_batch_dev(wt_engine* h, const float* d_pcm, int batch, int64_t* ids,
                                   int32_t* n_ids) {
  if (!h || !d_pcm || !ids || !n_ids) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    refuse_fixed_rows(e);
    float* d_mel = e.staging_mel(batch);
    e.logmel(d_pcm, batch, d_mel);
    e.encode(d_mel, batch);
    e.decode(batch, ids, n_ids, nullptr, 0);
  });
}

// full-length greedy decoding (option max_positions = P): ids rows of ids_stride >= P + 1
int wt_encdec_tokens_full_batch_dev(wt_engine* h, const float* d_mel, int batch, int64_t* ids, int ids_stride,
                                    int32_t* n_ids) {
  if (!h || !d_mel || !ids || !n_ids) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    e.check_full_args(batch, ids_stride);  // before anything is enqueued
    e.encode_full(d_mel, batch);
    e.decode_full(batch, ids, ids_stride, n_ids);
  });
}

int wt_encdec_tokens_full_batch(wt_engine* h, const float* mel, int batch, int64_t* ids, int ids_stride, int32_t* n_ids) {
  if (!h || !mel || !ids || !n_ids) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    e.check_full_args(batch, ids_stride);  // before anything is enqueued
    float* d_mel = e.staging_mel(batch);
    hipchk(hipMemcpyAsync(d_mel, mel, size_t(batch) * e.mel_elems() * sizeof(float), hipMemcpyHostToDevice, e.stream()), "H2D mel");
    e.encode_full(d_mel, batch);
    e.decode_full(batch, ids, ids_stride, n_ids);
    e.sync();  // mel is read by the H2D copy on the encoder stream
  });
}

int wt_transcribe_tokens_full_batch_dev(wt_engine* h, const float* d_pcm, int batch, int64_t* ids, int ids_stride,
                                        int32_t* n_ids) {
  if (!h || !d_pcm || !ids || !n_ids) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    e.check_full_args(batch, ids_stride);  // before anything is enqueued
    float* d_mel = e.staging_mel(batch);
    e.logmel(d_pcm, batch, d_mel);
    e.encode_full(d_mel, batch);
    e.decode_full(batch, ids, ids_stride, n_ids);
  });
}

int wt_encdec_debug_batch(wt_engine* h, const float* mel, int batch, int64_t* ids, int32_t* n_ids,
                          float* enc_out, float* logits, int logits_steps_cap) {
  if (!h || !mel || !ids || !n_ids) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    refuse_fixed_rows(e);
    e.check_language_call();
    e.check_beam_call(logits != nullptr);  // (before the encoder pass)
    float* d_mel = e.staging_mel(batch);
    hipchk(hipMemcpyAsync(d_mel, mel, size_t(batch) * e.mel_elems() * sizeof(float), hipMemcpyHostToDevice, e.stream()), "H2D mel");
    e.encode(d_mel, batch);
    if (enc_out) {
      const size_t n = size_t(batch) * e.dims().n_audio_ctx * e.dims().n_audio_state;
      hipchk(hipMemcpyAsync(enc_out, e.enc_out(), n * sizeof(float), hipMemcpyDeviceToHost, e.stream()), "D2H enc_out");
    }
    e.decode(batch, ids, n_ids, logits, logits_steps_cap);
    e.sync();  // the enc_out copy rides the encoder stream
  });
}

int wt_last_timings(const wt_engine* h, wt_timings* out) {
  if (!h || !out) return WT_ERR_INVALID_ARG;
  const wt::Timings& t = h->impl->timings();
  out->logmel_ms = t.logmel_ms;
  out->encoder_ms = t.encoder_ms;
  out->cross_kv_ms = t.cross_kv_ms;
  out->decoder_ms = t.decoder_ms;
  out->total_ms = t.total_ms;
  out->batch = t.batch;
  out->decoder_steps = t.decoder_steps;
  return WT_OK;
}

int wt_last_beam_scores(const wt_engine* h, float* sum_logprob, int32_t* n_generated, int cap) {
  if (!h || cap < 0 || (cap > 0 && (!sum_logprob || !n_generated))) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.beam_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last.beam_sum.size());
  for (int i = 0; i < n && i < cap; ++i) {
    sum_logprob[i] = e.last.beam_sum[i];
    n_generated[i] = e.last.beam_len[i];
  }
  return n;
}

static int copy_segments(const std::vector<wt::Segment>& v, wt_segment* out, int cap) {
  static_assert(sizeof(wt_segment) == sizeof(wt::Segment), "wt_segment mirrors wt::Segment");
  for (int i = 0; i < int(v.size()) && i < cap; ++i) std::memcpy(&out[i], &v[i], sizeof(wt_segment));
  return int(v.size());
}

int wt_last_segments(const wt_engine* h, wt_segment* out, int cap) {
  if (!h || cap < 0 || (cap > 0 && !out)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.segments_valid) return -WT_ERR_INVALID_ARG;
  return copy_segments(e.last.segments, out, cap);
}

int wt_last_segment_text(const wt_engine* h, int index, char* out, size_t cap, size_t* len) {
  if (!h) return WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.segments_valid || index < 0 || size_t(index) >= e.last.segment_text.size()) {
    if (len) *len = 0;
    return WT_ERR_INVALID_ARG;
  }
  return copy_text(e.last.segment_text[size_t(index)], out, cap, len);
}

int wt_last_words(const wt_engine* h, wt_word* out, int cap) {
  static_assert(sizeof(wt_word) == sizeof(wt::Word), "wt_word mirrors wt::Word");
  if (!h || cap < 0 || (cap > 0 && !out)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.words_valid) return -WT_ERR_INVALID_ARG;
  for (int i = 0; i < int(e.last.words.size()) && i < cap; ++i) std::memcpy(&out[i], &e.last.words[size_t(i)], sizeof(wt_word));
  return int(e.last.words.size());
}

int wt_last_word_text(const wt_engine* h, int index, char* out, size_t cap, size_t* len) {
  if (!h) return WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.words_valid || index < 0 || size_t(index) >= e.last.word_text.size()) {
    if (len) *len = 0;
    return WT_ERR_INVALID_ARG;
  }
  return copy_text(e.last.word_text[size_t(index)], out, cap, len);
}

int wt_last_scores(const wt_engine* h, wt_clip_score* out, int cap) {
  static_assert(sizeof(wt_clip_score) == sizeof(wt::ClipScore), "wt_clip_score mirrors wt::ClipScore");
  if (!h || cap < 0 || (cap > 0 && !out)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.scores_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last.scores.size());
  for (int i = 0; i < n && i < cap; ++i) std::memcpy(&out[i], &e.last.scores[size_t(i)], sizeof(wt_clip_score));
  return n;
}

int wt_last_decode_info(const wt_engine* h, wt_clip_decode* out, int cap) {
  static_assert(sizeof(wt_clip_decode) == sizeof(wt::ClipDecode), "wt_clip_decode mirrors wt::ClipDecode");
  if (!h || cap < 0 || (cap > 0 && !out)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.decode_info_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last.decode_info.size());
  for (int i = 0; i < n && i < cap; ++i) std::memcpy(&out[i], &e.last.decode_info[size_t(i)], sizeof(wt_clip_decode));
  return n;
}

int wt_last_best_of(const wt_engine* h, int32_t* picked, double* sum_logprob, int32_t* n_generated, int cap) {
  if (!h || cap < 0 || (cap > 0 && (!picked || !sum_logprob || !n_generated))) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.best_of_valid) return -WT_ERR_INVALID_ARG;
  static_assert(wt::kBestOfSlots == wt::kSampleGroupMax, "a best-of row holds one slot per sample of a launch");
  const int n = int(e.last.picked.size()), G = wt::kBestOfSlots;
  for (int i = 0; i < n && i < cap; ++i) {
    picked[i] = e.last.picked[size_t(i)];
    for (int j = 0; j < G; ++j) {
      sum_logprob[i * G + j] = e.last.best_of_sum[size_t(i) * G + j];
      n_generated[i * G + j] = e.last.best_of_count[size_t(i) * G + j];
    }
  }
  return n;
}

int wt_last_windows(const wt_engine* h, wt_window* out, int cap) {
  static_assert(sizeof(wt_window) == sizeof(wt::Window), "wt_window mirrors wt::Window");
  if (!h || cap < 0 || (cap > 0 && !out)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.windows_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last.windows.size());
  for (int i = 0; i < n && i < cap; ++i) std::memcpy(&out[i], &e.last.windows[size_t(i)], sizeof(wt_window));
  return n;
}

int wt_last_window_files(const wt_engine* h, int32_t* file, int cap) {
  if (!h || cap < 0 || (cap > 0 && !file)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.windows_valid || e.last.window_files.size() != e.last.windows.size()) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last.window_files.size());
  for (int i = 0; i < n && i < cap; ++i) file[i] = e.last.window_files[size_t(i)];
  return n;
}

int wt_last_token_logprobs(const wt_engine* h, float* out, int stride, int cap_clips) {
  if (!h || cap_clips < 0 || stride < 0 || (cap_clips > 0 && stride > 0 && !out)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.scores_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last.scores.size()), own = e.last.lp_stride;
  for (int b = 0; b < n && b < cap_clips; ++b) {
    for (int i = 0; i < stride; ++i) out[size_t(b) * stride + i] = i < own ? e.last.token_logprob[size_t(b) * own + i] : 0.0f;
  }
  return n;
}

int wt_last_segment_scores(const wt_engine* h, float* avg_logprob, int cap) {
  if (!h || cap < 0 || (cap > 0 && !avg_logprob)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.scores_valid || !e.last.segments_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last.segment_score.size());
  for (int i = 0; i < n && i < cap; ++i) avg_logprob[i] = e.last.segment_score[size_t(i)];
  return n;
}

// ------------------------------------------------- language detection ---

int wt_language_count(const wt_engine* h) {
  if (!h) return -WT_ERR_INVALID_ARG;
  const int n = h->impl->lang_tokens();
  return n > 0 ? n : -WT_ERR_UNSUPPORTED;
}

int wt_engine_set_language_candidates(wt_engine* h, const int32_t* langs, int n) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] { h->impl->set_language_candidates(langs, n); });
}

int wt_detect_language_batch_dev(wt_engine* h, const float* d_mel, int batch, int32_t* lang, float* probs) {
  if (!h || !d_mel || !lang || batch < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    const int n_lang = e.lang_tokens();
    if (n_lang < 1) throw wt::Error(WT_ERR_UNSUPPORTED, "language detection: this engine's vocabulary has no language tokens");
    for (int b0 = 0; b0 < batch; b0 += 64) {  // one encoder pass + one decoder position per 64 clips
      const int nb = std::min(64, batch - b0);
      e.encode(d_mel + size_t(b0) * e.mel_elems(), nb);
      e.detect_language(nb, lang + b0, probs ? probs + size_t(b0) * n_lang : nullptr, nullptr);
    }
  });
}

int wt_detect_language_batch(wt_engine* h, const float* mel, int batch, int32_t* lang, float* probs) {
  if (!h || !mel || !lang || batch < 1) return WT_ERR_INVALID_ARG;
  float* d_mel = nullptr;
  const int rc = guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    if (e.lang_tokens() < 1) throw wt::Error(WT_ERR_UNSUPPORTED, "language detection: this engine's vocabulary has no language tokens");
    d_mel = e.staging_mel(batch);
    hipchk(hipMemcpyAsync(d_mel, mel, size_t(batch) * e.mel_elems() * sizeof(float), hipMemcpyHostToDevice, e.stream()), "H2D mel");
  });
  if (rc != WT_OK) return rc;
  return wt_detect_language_batch_dev(h, d_mel, batch, lang, probs);  // (its decoder pass waits for the copy's stream)
}

int wt_detect_language_pcm(wt_engine* h, const float* pcm, size_t n_samples, int32_t* lang, float* prob) {
  if (!h || (!pcm && n_samples) || !lang) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    if (e.lang_tokens() < 1) throw wt::Error(WT_ERR_UNSUPPORTED, "language detection: this engine's vocabulary has no language tokens");
    std::vector<float> clip(e.pcm_elems(), 0.0f);  // one 30 s window, as wt_transcribe_pcm
    std::memcpy(clip.data(), pcm, std::min(n_samples, clip.size()) * sizeof(float));
    float* d_mel = e.staging_mel(1);
    e.logmel(e.upload_pcm(clip.data(), 1), 1, d_mel);
    e.encode(d_mel, 1);
    e.detect_language(1, lang, nullptr, prob);
    e.sync();
  });
}

int wt_last_languages(const wt_engine* h, int32_t* lang, float* prob, int cap) {
  if (!h || cap < 0 || (cap > 0 && (!lang || !prob))) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.lang_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last.lang.size());
  for (int i = 0; i < n && i < cap; ++i) {
    lang[i] = e.last.lang[i];
    prob[i] = e.last.lang_prob[i];
  }
  return n;
}

int wt_last_kernel_stats(const wt_engine* h, wt_kernel_stat* out, int cap) {
  if (!h || (!out && cap > 0)) return 0;
  const wt::KernelStat* k = h->impl->kernel_stats();
  for (int i = 0; i < wt::kKcCount && i < cap; ++i) {
    std::memset(&out[i], 0, sizeof(out[i]));
    std::snprintf(out[i].name, sizeof(out[i].name), "%s", k[i].name);
    out[i].launches = k[i].launches;
    out[i].ms = k[i].ms;
    out[i].flops = k[i].flops;
    out[i].bytes = k[i].bytes;
  }
  return wt::kKcCount;
}

// --------------------------------------------------------- single clip ---

int wt_transcribe_pcm(wt_engine* h, const float* pcm, size_t n_samples, char* out, size_t cap,
                      size_t* len) {
  if (!h || (!pcm && n_samples)) return WT_ERR_INVALID_ARG;
  std::string text;
  const int rc = guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    e.check_timestamp_call();  // before anything is enqueued
    // pad with zeros or truncate to one 30 s window (whisper.cpp:753)
    std::vector<float> clip(e.pcm_elems(), 0.0f);
    std::memcpy(clip.data(), pcm, std::min(n_samples, clip.size()) * sizeof(float));
    const std::vector<long long> valid{(long long)std::min(n_samples, clip.size())};  // word timestamps: the window's own frames
    std::vector<int64_t> ids;  // full-length decoding: a row of max_positions + 1 ids
    std::vector<int32_t> n;
    e.decode_windows(clip.data(), 1, &valid, &ids, &n);
    bool missing = false;
    // omit_special_tokens = false, as EncDec::transcribe passes (whisper.cpp:766-767)
    text = wt::decode_tokens(e.vocab(), ids.data(), n[0], false, &missing);
    // option skip_silence: a silent window (only a call that itself ran with scores has them)
    if (e.max_positions > 0 && e.scores && e.last.scores_valid && !e.last.scores.empty() && e.last.scores[0].skipped) text.clear();
    if (missing && e.verbose) std::fprintf(stderr, "[wt] token id without a vocab entry skipped\n");
  });
  if (rc != WT_OK) {
    if (len) *len = 0;
    if (out && cap) out[0] = 0;
    return rc;
  }
  return copy_text(text, out, cap, len);
}

int wt_transcribe_long_batch(wt_engine* h, const float* const* pcm, const size_t* n_samples, int n_files) {
  if (!h || !pcm || !n_samples) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    e.check_timestamp_call();  // before anything is enqueued
    e.check_full_call();
    if (e.bf16 && e.max_positions > 0 && !e.full_bf16_all) throw wt::Error(WT_ERR_UNSUPPORTED, "full-length decoding in the bf16 storage mode (full_bf16): not with wt_transcribe_long_batch (the ragged self-attention kernels have no bf16 form)");
    if (e.best_of_sampling()) throw wt::Error(WT_ERR_UNSUPPORTED, "best_of: not with wt_transcribe_long_batch (contexts and seeking are outside the best-of chain)");
    if (e.beam_fallback()) throw wt::Error(WT_ERR_UNSUPPORTED, "fallback_beam: not with wt_transcribe_long_batch (contexts and seeking are outside the beam chain)");
    wt::transcribe_seek_batch(e, pcm, n_samples, n_files);
  });
}

int wt_last_file_text(const wt_engine* h, int file, char* out, size_t cap, size_t* len) {
  if (!h) return WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last.windows_valid || file < 0 || size_t(file) >= e.last.file_text.size()) return WT_ERR_INVALID_ARG;
  return copy_text(e.last.file_text[size_t(file)], out, cap, len);
}

int wt_transcribe_long_pcm(wt_engine* h, const float* pcm, size_t n_samples, char* out, size_t cap,
                           size_t* len) {
  if (!h || (!pcm && n_samples)) return WT_ERR_INVALID_ARG;
  std::string text;
  const int rc = guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    e.check_timestamp_call();  // before anything is enqueued
    // seek: one window at a time, each starting at the last closed timestamp of the one before; else 32 at a time (longform.cpp)
    if (e.seek) wt::transcribe_seek(e, pcm, n_samples, &text);
    else wt::transcribe_windows(e, pcm, n_samples, &text);
  });
  if (rc != WT_OK) {
    if (len) *len = 0;
    if (out && cap) out[0] = 0;
    return rc;
  }
  return copy_text(text, out, cap, len);
}

int wt_transcribe_file(wt_engine* h, const char* wav_path, char* out, size_t cap, size_t* len) {
  if (!h || !wav_path) return WT_ERR_INVALID_ARG;
  std::vector<float> pcm;
  // an unreadable WAV yields an empty vector in the reference and is then padded to 30 s
  // of silence (whisper.cpp:772-773); same here
  (void)wt::wav_read_legacy(wav_path, &pcm, h->impl->verbose != 0);
  return wt_transcribe_pcm(h, pcm.data(), pcm.size(), out, cap, len);
}

// -------------------------------------------------------------- helpers ---

int wt_decode_text(wt_engine* h, const int64_t* ids, int n, int omit_special_tokens, char* out,
                   size_t cap, size_t* len) {
  if (!h || (!ids && n)) return WT_ERR_INVALID_ARG;
  bool missing = false;
  const std::string s = wt::decode_tokens(h->impl->vocab(), ids, n, omit_special_tokens != 0, &missing);
  if (missing) {
    if (len) *len = 0;
    return fail(h, WT_ERR_INVALID_ARG, "token id without a vocab entry");
  }
  return copy_text(s, out, cap, len);
}

int wt_language_id(const char* code) { return code ? wt::language_id(code) : wt::language_count(); }
const char* wt_lang_code(int id) {
  return (id >= 0 && id < wt::language_count()) ? wt::lang_code(size_t(id)).c_str() : "";
}

int wt_wav_read_legacy(const char* path, float* out, size_t cap, size_t* n) {
  if (!path || !n) return WT_ERR_INVALID_ARG;
  std::vector<float> s;
  if (!wt::wav_read_legacy(path, &s, false)) {
    *n = 0;
    return WT_ERR_IO;
  }
  *n = s.size();
  if (out) std::memcpy(out, s.data(), std::min(cap, s.size()) * sizeof(float));
  return WT_OK;
}

static void vocab_info_of(const wt::VocabData& v, int32_t out[9]);
int wt_vocab_info(const wt_engine* h, int32_t out[9]) {
  if (!h || !out) return WT_ERR_INVALID_ARG;
  vocab_info_of(h->impl->vocab(), out);
  return WT_OK;
}

int wt_filters(const wt_engine* h, float* out, size_t cap, int32_t* n_mel, int32_t* n_fft) {
  if (!h) return 0;
  const wt::FilterBank& f = h->impl->filters();
  if (n_mel) *n_mel = f.n_mel;
  if (n_fft) *n_fft = f.n_fft;
  if (out) std::memcpy(out, f.data.data(), std::min(cap, f.data.size()) * sizeof(float));
  return static_cast<int>(f.data.size());
}

// ------------------------------------------------ vocab file on the host ---

}  // extern "C"

struct wt_vocab {
  wt::VocabData vocab;
  wt::FilterBank filters;
};

extern "C" {

int wt_vocab_open(const char* vocab_path, int multilingual, wt_vocab** out) {
  if (!out) return fail(nullptr, WT_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  if (!vocab_path) return fail(nullptr, WT_ERR_INVALID_ARG, "NULL path");
  std::unique_ptr<wt_vocab> v(new wt_vocab);
  const int rc = guarded(nullptr, [&] { wt::read_vocab_file(vocab_path, multilingual != 0, &v->filters, &v->vocab); });
  if (rc != WT_OK) return rc;
  *out = v.release();
  return WT_OK;
}

void wt_vocab_close(wt_vocab* v) { delete v; }

static void vocab_info_of(const wt::VocabData& v, int32_t out[9]) {
  const int32_t vals[9] = {v.n_vocab,    v.token_eot,  v.token_sot, v.token_translate, v.token_transcribe,
                           v.token_prev, v.token_solm, v.token_not, v.token_beg};
  std::memcpy(out, vals, sizeof(vals));
}

int wt_vocab_get_info(const wt_vocab* v, int32_t out[9]) {
  if (!v || !out) return WT_ERR_INVALID_ARG;
  vocab_info_of(v->vocab, out);
  return WT_OK;
}

int wt_vocab_get_filters(const wt_vocab* v, float* out, size_t cap, int32_t* n_mel, int32_t* n_fft) {
  if (!v) return 0;
  if (n_mel) *n_mel = v->filters.n_mel;
  if (n_fft) *n_fft = v->filters.n_fft;
  if (out) std::memcpy(out, v->filters.data.data(), std::min(cap, v->filters.data.size()) * sizeof(float));
  return static_cast<int>(v->filters.data.size());
}

int wt_vocab_size(const wt_vocab* v) { return v ? static_cast<int>(v->vocab.id_to_token.size()) : 0; }

int wt_vocab_token(const wt_vocab* v, int id, char* out, size_t cap, size_t* len) {
  if (!v) return WT_ERR_INVALID_ARG;
  auto it = v->vocab.id_to_token.find(id);
  if (it == v->vocab.id_to_token.end()) {
    if (len) *len = 0;
    return fail(nullptr, WT_ERR_INVALID_ARG, "token id without a vocab entry");
  }
  return copy_text(it->second, out, cap, len);
}

int wt_vocab_decode(const wt_vocab* v, const int64_t* ids, int n, int omit_special_tokens, char* out,
                    size_t cap, size_t* len) {
  if (!v || (!ids && n)) return WT_ERR_INVALID_ARG;
  bool missing = false;
  const std::string s = wt::decode_tokens(v->vocab, ids, n, omit_special_tokens != 0, &missing);
  if (missing) {  // the reference asserts (whisper.cpp:642)
    if (len) *len = 0;
    return fail(nullptr, WT_ERR_INVALID_ARG, "token id without a vocab entry");
  }
  return copy_text(s, out, cap, len);
}

int wt_vocab_segments(const wt_vocab* v, const int64_t* ids, int n, int sample_begin, wt_segment* out, int cap) {
  if (!v || n < 0 || (!ids && n) || sample_begin < 0 || cap < 0 || (cap > 0 && !out)) return -WT_ERR_INVALID_ARG;
  std::vector<wt::Segment> segs;
  wt::parse_segments(v->vocab, ids, n, sample_begin, 0, &segs);
  return copy_segments(segs, out, cap);
}

int wt_vocab_seek_step(const wt_vocab* v, const int64_t* g, int n, int win_ticks, int seg_ticks, wt_segment* out, int cap,
                       int32_t* advance_ticks) {
  if (!v || n < 0 || (!g && n) || win_ticks < 1 || seg_ticks < 0 || seg_ticks > win_ticks || cap < 0 || (cap > 0 && !out) ||
      !advance_ticks) {
    return -WT_ERR_INVALID_ARG;
  }
  std::vector<wt::Segment> segs;
  *advance_ticks = wt::seek_step(v->vocab, g, n, win_ticks, seg_ticks, &segs);
  return copy_segments(segs, out, cap);
}

int wt_vocab_default_suppress(const wt_vocab* v, int64_t* ids, int cap, int32_t* n, int64_t* first_ids, int first_cap,
                              int32_t* n_first) {
  if (!v || !n || !n_first || cap < 0 || first_cap < 0 || (cap > 0 && !ids) || (first_cap > 0 && !first_ids)) {
    return WT_ERR_INVALID_ARG;
  }
  std::vector<long long> a, f;
  wt::default_suppress(v->vocab, v->vocab.n_vocab, &a, &f);
  *n = int32_t(a.size()), *n_first = int32_t(f.size());
  for (size_t i = 0; i < a.size() && i < size_t(cap); ++i) ids[i] = a[i];
  for (size_t i = 0; i < f.size() && i < size_t(first_cap); ++i) first_ids[i] = f[i];
  return a.size() <= size_t(cap) && f.size() <= size_t(first_cap) ? WT_OK : WT_ERR_BUFFER;
}

static int copy_counts(const std::vector<int>& counts, int32_t* out, int cap) {
  for (int i = 0; i < int(counts.size()) && i < cap; ++i) out[i] = counts[size_t(i)];
  return int(counts.size());
}

int wt_vocab_split_words(const wt_vocab* v, const int64_t* ids, int n, int unicode_only, int32_t* word_len_out, int cap) {
  if (!v || n < 0 || (!ids && n) || cap < 0 || (cap > 0 && !word_len_out)) return -WT_ERR_INVALID_ARG;
  return copy_counts(wt::split_words(v->vocab, ids, n, unicode_only != 0), word_len_out, cap);
}

int wt_vocab_merge_punctuation(const wt_vocab* v, const int64_t* ids, int n, const int32_t* word_len, int n_words,
                               int32_t* merged_len_out, int cap) {
  if (!v || n < 0 || (!ids && n) || n_words < 0 || (!word_len && n_words) || cap < 0 || (cap > 0 && !merged_len_out)) {
    return -WT_ERR_INVALID_ARG;
  }
  long total = 0;
  for (int k = 0; k < n_words; ++k) {
    if (word_len[k] < 1) return -WT_ERR_INVALID_ARG;
    total += word_len[k];
  }
  if (total != n) return -WT_ERR_INVALID_ARG;
  return copy_counts(wt::merge_punctuation(v->vocab, ids, n, word_len, n_words), merged_len_out, cap);
}

int wt_dtw_path(const float* cost, int N, int F, int32_t* jump, int32_t* path_out, int path_cap) {
  if (!cost || !jump || N < 1 || N > 447 || F < 1 || F > 1500 || path_cap < 0 || (path_cap > 0 && !path_out)) {
    return -WT_ERR_INVALID_ARG;
  }
  std::vector<int32_t> path;
  const int cells = wt::dtw_path(cost, N, F, F, jump, path_out ? &path : nullptr, nullptr);
  if (path_out) std::memcpy(path_out, path.data(), size_t(std::min(cells, path_cap)) * 2 * sizeof(int32_t));
  return cells;
}

// ------------------------------------------- log-mel as a free function ---

namespace {
struct LogmelCtx {
  int device = 0;
  std::vector<float> filters;
  std::unique_ptr<wt::Engine> eng;
  std::mutex mu;
  unsigned long stamp = 0;
};
std::mutex g_logmel_mu;
std::vector<std::shared_ptr<LogmelCtx>> g_logmel_ctxs;
}  // namespace

void wt_shutdown(void) {
  std::lock_guard<std::mutex> lock(g_logmel_mu);
  g_logmel_ctxs.clear();
}

int wt_log_mel_spectrogram(const float* samples, int n_samples, const float* filters, int n_mel,
                           int n_fft_bins, int device_id, float* mel_out, size_t cap, int* n_len) {
  if ((!samples && n_samples) || !filters || !mel_out || n_samples < 0) return fail(nullptr, WT_ERR_INVALID_ARG, "NULL argument");
  if (n_mel != 80 || n_fft_bins != 201 || n_samples > WT_CHUNK_SAMPLES) {
    return fail(nullptr, WT_ERR_UNSUPPORTED,
                "log_mel_spectrogram: only the reference's fixed geometry (80 x 201 filters, <= 480000 samples at "
                "16 kHz, fft 400, hop 160) runs on the gfx950 front end");
  }
  // Front-end contexts (DFT basis + mel matrix in HBM, streams, staging buffers), one per (device, filter table), at
  // most kMaxCtx of them: the least recently used one is destroyed when a new table arrives, so a caller that varies
  // its filters cannot grow the cache without bound.  The table lock is held only to find / create the context; the
  // GPU round trip runs under the context's own lock, so callers on different devices do not serialise.
  // wt_shutdown() releases the contexts before the HIP runtime is torn down.
  constexpr size_t kMaxCtx = 4;
  return guarded(nullptr, [&] {
    const size_t nf = size_t(n_mel) * n_fft_bins;
    std::shared_ptr<LogmelCtx> c;
    {
      std::lock_guard<std::mutex> lock(g_logmel_mu);
      static unsigned long clock = 0;
      for (auto& x : g_logmel_ctxs)
        if (x->device == device_id && std::memcmp(x->filters.data(), filters, nf * sizeof(float)) == 0) c = x;
      if (!c) {
        if (g_logmel_ctxs.size() >= kMaxCtx) {  // evict the least recently used context nobody is inside
          size_t victim = g_logmel_ctxs.size();
          for (size_t i = 0; i < g_logmel_ctxs.size(); ++i)
            if (g_logmel_ctxs[i].use_count() == 1 && (victim == g_logmel_ctxs.size() || g_logmel_ctxs[i]->stamp < g_logmel_ctxs[victim]->stamp)) victim = i;
          if (victim < g_logmel_ctxs.size()) g_logmel_ctxs.erase(g_logmel_ctxs.begin() + long(victim));
        }
        c = std::make_shared<LogmelCtx>();
        c->device = device_id;
        c->filters.assign(filters, filters + nf);
        wt::FilterBank fb;
        fb.n_mel = n_mel;
        fb.n_fft = n_fft_bins;
        fb.data = c->filters;
        c->eng.reset(new wt::Engine(fb, device_id));
        g_logmel_ctxs.push_back(c);
      }
      c->stamp = ++clock;
    }
    std::lock_guard<std::mutex> ctx_lock(c->mu);
    wt::Engine& e = *c->eng;
    e.bind_device();
    const int frames = n_samples / WT_HOP;  // Mel::n_len (whisper.cpp:123)
    if (n_len) *n_len = frames;
    if (cap < size_t(n_mel) * frames) throw wt::Error(WT_ERR_BUFFER, "mel_out too small");
    std::vector<float> clip(e.pcm_elems(), 0.0f);
    std::memcpy(clip.data(), samples, size_t(n_samples) * sizeof(float));
    float* d_mel = e.staging_mel(1);
    // frames past n_len exist only in the 30 s window the kernels work on: they take no part in the
    // reference's maximum (whisper.cpp:198-203 runs over n_mel * n_len values)
    e.logmel(e.upload_pcm(clip.data(), 1), 1, d_mel, frames);
    std::vector<float> full(e.mel_elems());
    hipchk(hipMemcpyAsync(full.data(), d_mel, full.size() * sizeof(float), hipMemcpyDeviceToHost, e.stream()), "D2H mel");
    e.sync();
    const size_t T0 = size_t(e.mel_frames());
    for (int j = 0; j < n_mel; ++j) std::memcpy(mel_out + size_t(j) * frames, full.data() + size_t(j) * T0, size_t(frames) * sizeof(float));
  });
}

int wt_convert_tflite(const char* model_prefix, const char* out_path) {
  if (!model_prefix || !out_path) return fail(nullptr, WT_ERR_INVALID_ARG, "NULL path");
  return guarded(nullptr, [&] { wt::convert_tflite(model_prefix, out_path); });
}

int wt_write_synthetic_weights(const char* path, const char* arch, uint64_t seed) {
  if (!path || !arch) return WT_ERR_INVALID_ARG;
  wtw::Dims dims;
  if (!wtw::dims_by_name(arch, &dims)) return fail(nullptr, WT_ERR_INVALID_ARG, std::string("unknown arch: ") + arch);
  std::string err;
  const int rc = wtw::write_synthetic(path, dims, seed, &err);
  if (rc != 0) return fail(nullptr, rc == 1 ? WT_ERR_INVALID_ARG : WT_ERR_IO, err);
  return WT_OK;
}

int wt_write_synthetic_vocab(const char* path, int n_tokens) {
  if (!path || n_tokens < 0) return WT_ERR_INVALID_ARG;
  return guarded(nullptr, [&] {
    wt::write_vocab_file(path, wt::make_slaney_filterbank(80, 400, 16000), wt::make_synthetic_tokens(n_tokens));
  });
}

}  // extern "C"
