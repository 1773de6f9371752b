// extern "C" boundary (include/wt_capi.h): exception-free wrappers over wt::Engine.
#include "wt_capi.h"

#include <hip/hip_runtime.h>

#include <functional>

#include <cstdio>
#include <cstdlib>
#include <sys/stat.h>
#include <unistd.h>
#include <cmath>
#include <limits>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <mutex>

#include "engine.h"
#include "tflite_extract.h"
#include "weights_gen.h"
#include "wt_debug.h"
#include "kernels.h"

struct wt_engine {
  std::unique_ptr<wt::Engine> impl;
  std::string last_error;
};

namespace {
thread_local std::string g_create_error;

int fail(wt_engine* h, int code, const std::string& msg) {
  if (h) {
    h->last_error = msg;
  } else {
    g_create_error = msg;
  }
  return code;
}

// Runs fn, translating every exception into a status code.
template <class F>
int guarded(wt_engine* h, F&& fn) {
  try {
    if (h && h->impl) h->impl->bind_device();  // one handle per GPU: launches go to its device
    fn();
    if (h) h->last_error.clear();
    return WT_OK;
  } catch (const wt::Error& e) {
    return fail(h, e.code, e.what());
  } catch (const std::bad_alloc&) {
    return fail(h, WT_ERR_DEVICE, "out of host memory");
  } catch (const std::exception& e) {
    const std::string w = e.what();
    return fail(h, w.rfind("Failed to open", 0) == 0 ? WT_ERR_IO : WT_ERR_FORMAT, w);
  } catch (...) {
    return fail(h, WT_ERR_DEVICE, "unknown failure");
  }
}

int copy_text(const std::string& s, char* out, size_t cap, size_t* len) {
  if (len) *len = s.size();
  if (out && cap > 0) {
    const size_t n = std::min(s.size(), cap - 1);
    std::memcpy(out, s.data(), n);
    out[n] = 0;
  }
  return (out && s.size() + 1 <= cap) ? WT_OK : WT_ERR_BUFFER;
}

void hipchk(hipError_t e, const char* what) {
  if (e != hipSuccess) throw wt::Error(WT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
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
  } else if (k == "max_initial_timestamp") {
    if (value < -1 || value > 1500) return fail(h, WT_ERR_INVALID_ARG, "max_initial_timestamp must be in [-1, 1500] (ticks of 20 ms, -1 = no limit)");
    e.max_initial_timestamp = value;
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
    float* d_pcm = e.staging_pcm(batch);
    float* d_mel = e.staging_mel(batch);
    hipchk(hipMemcpyAsync(d_pcm, pcm, size_t(batch) * e.pcm_elems() * sizeof(float), hipMemcpyHostToDevice, e.stream()), "H2D pcm");
    e.logmel(d_pcm, batch, d_mel);
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
        sums.insert(sums.end(), e.beam_sum.begin(), e.beam_sum.end());
        lens.insert(lens.end(), e.beam_len.begin(), e.beam_len.end());
      }
      e.beam_sum = sums;
      e.beam_len = lens;
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
  if (!e.beam_scores_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.beam_sum.size());
  for (int i = 0; i < n && i < cap; ++i) {
    sum_logprob[i] = e.beam_sum[i];
    n_generated[i] = e.beam_len[i];
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
  if (!e.last_segments_valid) return -WT_ERR_INVALID_ARG;
  return copy_segments(e.last_segments, out, cap);
}

int wt_last_segment_text(const wt_engine* h, int index, char* out, size_t cap, size_t* len) {
  if (!h) return WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last_segments_valid || index < 0 || size_t(index) >= e.last_segment_text.size()) {
    if (len) *len = 0;
    return WT_ERR_INVALID_ARG;
  }
  return copy_text(e.last_segment_text[size_t(index)], out, cap, len);
}

int wt_last_scores(const wt_engine* h, wt_clip_score* out, int cap) {
  static_assert(sizeof(wt_clip_score) == sizeof(wt::ClipScore), "wt_clip_score mirrors wt::ClipScore");
  if (!h || cap < 0 || (cap > 0 && !out)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last_scores_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last_scores.size());
  for (int i = 0; i < n && i < cap; ++i) std::memcpy(&out[i], &e.last_scores[size_t(i)], sizeof(wt_clip_score));
  return n;
}

int wt_last_decode_info(const wt_engine* h, wt_clip_decode* out, int cap) {
  static_assert(sizeof(wt_clip_decode) == sizeof(wt::Engine::ClipDecode), "wt_clip_decode mirrors wt::Engine::ClipDecode");
  if (!h || cap < 0 || (cap > 0 && !out)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last_decode_info_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last_decode_info.size());
  for (int i = 0; i < n && i < cap; ++i) std::memcpy(&out[i], &e.last_decode_info[size_t(i)], sizeof(wt_clip_decode));
  return n;
}

int wt_last_token_logprobs(const wt_engine* h, float* out, int stride, int cap_clips) {
  if (!h || cap_clips < 0 || stride < 0 || (cap_clips > 0 && stride > 0 && !out)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last_scores_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last_scores.size()), own = e.last_lp_stride;
  for (int b = 0; b < n && b < cap_clips; ++b) {
    for (int i = 0; i < stride; ++i) out[size_t(b) * stride + i] = i < own ? e.last_token_logprob[size_t(b) * own + i] : 0.0f;
  }
  return n;
}

int wt_last_segment_scores(const wt_engine* h, float* avg_logprob, int cap) {
  if (!h || cap < 0 || (cap > 0 && !avg_logprob)) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last_scores_valid || !e.last_segments_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last_segment_score.size());
  for (int i = 0; i < n && i < cap; ++i) avg_logprob[i] = e.last_segment_score[size_t(i)];
  return n;
}

// ------------------------------------------------- language detection ---

int wt_language_count(const wt_engine* h) {
  if (!h) return -WT_ERR_INVALID_ARG;
  const int n = h->impl->lang_tokens();
  return n > 0 ? n : -WT_ERR_UNSUPPORTED;
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
    float* d_pcm = e.staging_pcm(1);
    float* d_mel = e.staging_mel(1);
    hipchk(hipMemcpyAsync(d_pcm, clip.data(), clip.size() * sizeof(float), hipMemcpyHostToDevice, e.stream()), "H2D pcm");
    e.logmel(d_pcm, 1, d_mel);
    e.encode(d_mel, 1);
    e.detect_language(1, lang, nullptr, prob);
    e.sync();
  });
}

int wt_last_languages(const wt_engine* h, int32_t* lang, float* prob, int cap) {
  if (!h || cap < 0 || (cap > 0 && (!lang || !prob))) return -WT_ERR_INVALID_ARG;
  const wt::Engine& e = *h->impl;
  if (!e.last_lang_valid) return -WT_ERR_INVALID_ARG;
  const int n = int(e.last_lang.size());
  for (int i = 0; i < n && i < cap; ++i) {
    lang[i] = e.last_lang[i];
    prob[i] = e.last_lang_prob[i];
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
    float* d_pcm = e.staging_pcm(1);
    float* d_mel = e.staging_mel(1);
    hipchk(hipMemcpyAsync(d_pcm, clip.data(), clip.size() * sizeof(float), hipMemcpyHostToDevice, e.stream()), "H2D pcm");
    e.logmel(d_pcm, 1, d_mel);
    const bool full = e.max_positions > 0;  // full-length decoding: rows of max_positions + 1 ids
    std::vector<int64_t> ids(full ? size_t(e.max_positions) + 1 : size_t(WT_MAX_IDS));
    int32_t n = 0;
    if (full) {
      e.encode_full(d_mel, 1);
      e.decode_full(1, ids.data(), int(ids.size()), &n);
    } else {
      e.encode(d_mel, 1);
      e.decode(1, ids.data(), &n, nullptr, 0);
    }
    bool missing = false;
    // omit_special_tokens = false, as EncDec::transcribe passes (whisper.cpp:766-767)
    text = wt::decode_tokens(e.vocab(), ids.data(), n, false, &missing);
    // option skip_silence: a silent window (only a call that itself ran with scores has them)
    if (full && e.scores && e.last_scores_valid && !e.last_scores.empty() && e.last_scores[0].skipped) text.clear();
    if (missing && e.verbose) std::fprintf(stderr, "[wt] token id without a vocab entry skipped\n");
  });
  if (rc != WT_OK) {
    if (len) *len = 0;
    if (out && cap) out[0] = 0;
    return rc;
  }
  return copy_text(text, out, cap, len);
}

int wt_transcribe_long_pcm(wt_engine* h, const float* pcm, size_t n_samples, char* out, size_t cap,
                           size_t* len) {
  if (!h || (!pcm && n_samples)) return WT_ERR_INVALID_ARG;
  std::string text;
  const int rc = guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    e.check_timestamp_call();  // before anything is enqueued
    const size_t win = e.pcm_elems();
    const size_t n_win = std::max<size_t>(1, (n_samples + win - 1) / win);
    std::vector<int> langs;  // automatic language: every window's, joined over the batches
    std::vector<float> lang_probs;
    std::vector<wt::Segment> segments;  // option timestamps: every window's, clip = window index, times in the file
    std::vector<std::string> segment_text;
    std::vector<wt::ClipScore> scores;  // option scores: every window's
    std::vector<float> token_logprob, segment_score;
    std::vector<wt::Engine::ClipDecode> decode_info;  // sampling / fall-back: every window's
    struct ClipBase {  // a window's Philox clip index is its index in the file, however the windows are batched
      wt::Engine& e;
      ~ClipBase() { e.clip_base = 0; }
    } clip_base{e};
    for (size_t w0 = 0; w0 < n_win; w0 += 32) {
      const int B = int(std::min<size_t>(32, n_win - w0));
      std::vector<float> clips(size_t(B) * win, 0.0f);
      for (int b = 0; b < B; ++b) {
        const size_t off = (w0 + b) * win;
        if (off < n_samples) std::memcpy(&clips[size_t(b) * win], pcm + off, std::min(win, n_samples - off) * sizeof(float));
      }
      float* d_pcm = e.staging_pcm(B);
      float* d_mel = e.staging_mel(B);
      hipchk(hipMemcpyAsync(d_pcm, clips.data(), clips.size() * sizeof(float), hipMemcpyHostToDevice, e.stream()), "H2D pcm");
      e.logmel(d_pcm, B, d_mel);
      const bool full = e.max_positions > 0;
      const size_t row = full ? size_t(e.max_positions) + 1 : size_t(WT_MAX_IDS);
      std::vector<int64_t> ids(size_t(B) * row);
      std::vector<int32_t> n(B);
      if (full) {
        e.encode_full(d_mel, B);
        e.clip_base = long(w0);
        e.decode_full(B, ids.data(), int(row), n.data());
      } else {
        e.encode(d_mel, B);
        e.decode(B, ids.data(), n.data(), nullptr, 0);
      }
      e.sync();  // clips[] is read by the H2D copy on the encoder stream
      if (e.last_decode_info_valid) decode_info.insert(decode_info.end(), e.last_decode_info.begin(), e.last_decode_info.end());
      if (e.last_lang_valid) {
        langs.insert(langs.end(), e.last_lang.begin(), e.last_lang.end());
        lang_probs.insert(lang_probs.end(), e.last_lang_prob.begin(), e.last_lang_prob.end());
      }
      if (e.last_segments_valid) {
        for (wt::Segment sg : e.last_segments) {
          sg.clip += int(w0);
          sg.t0_ms += wt::kWindowMs * sg.clip, sg.t1_ms += wt::kWindowMs * sg.clip;
          segments.push_back(sg);
        }
        segment_text.insert(segment_text.end(), e.last_segment_text.begin(), e.last_segment_text.end());
      }
      const bool scored = full && e.scores && e.last_scores_valid && e.last_scores.size() == size_t(B);  // THIS batch ran with scores
      if (scored) {
        scores.insert(scores.end(), e.last_scores.begin(), e.last_scores.end());
        token_logprob.insert(token_logprob.end(), e.last_token_logprob.begin(), e.last_token_logprob.end());
        segment_score.insert(segment_score.end(), e.last_segment_score.begin(), e.last_segment_score.end());
      }
      for (int b = 0; b < B; ++b) {
        if (w0 + b) text += '\n';
        if (scored && e.last_scores[size_t(b)].skipped) continue;  // option skip_silence: an empty line
        bool missing = false;
        text += wt::decode_tokens(e.vocab(), &ids[size_t(b) * row], n[b], false, &missing);
      }
    }
    if (e.last_scores_valid) e.last_scores = scores, e.last_token_logprob = token_logprob, e.last_segment_score = segment_score;
    if (e.last_decode_info_valid) e.last_decode_info = decode_info;
    if (e.last_lang_valid) e.last_lang = langs, e.last_lang_prob = lang_probs;
    if (e.last_segments_valid) e.last_segments = segments, e.last_segment_text = segment_text;
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
    float* d_pcm = e.staging_pcm(1);
    float* d_mel = e.staging_mel(1);
    hipchk(hipMemcpyAsync(d_pcm, clip.data(), clip.size() * sizeof(float), hipMemcpyHostToDevice, e.stream()), "H2D pcm");
    // frames past n_len exist only in the 30 s window the kernels work on: they take no part in the
    // reference's maximum (whisper.cpp:198-203 runs over n_mel * n_len values)
    e.logmel(d_pcm, 1, d_mel, frames);
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

// ------------------------------------------------- kernel-level debug taps ---
// Host in / host out wrappers around single kernels so that a parity failure can be
// localised (tests/test_gpu_kernels.py).  Not part of the drop-in boundary.

namespace {
struct DevBuf {
  float* p = nullptr;
  explicit DevBuf(size_t n) { hipchk(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(float)), "hipMalloc"); }
  DevBuf(const float* host, size_t n) : DevBuf(n) {
    if (host && n) hipchk(hipMemcpy(p, host, n * sizeof(float), hipMemcpyHostToDevice), "H2D");
  }
  ~DevBuf() { (void)hipFree(p); }
  void to_host(float* host, size_t n) const { hipchk(hipMemcpy(host, p, n * sizeof(float), hipMemcpyDeviceToHost), "D2H"); }
};
}  // namespace

namespace {
// W [N][K] as device-resident fp16 planes in the decoder GEMM's fragment order
struct DevTiled {
  void* p = nullptr;
  float scale = 1.0f;
  DevTiled(const float* W, int N, int K, bool bf16 = false) {
    const std::vector<unsigned short> planes = bf16 ? wt::tile_weights_bf16(W, N, K) : wt::tile_weights_f16(W, N, K, &scale);
    hipchk(hipMalloc(&p, std::max<size_t>(planes.size(), 1) * 2), "hipMalloc");
    hipchk(hipMemcpy(p, planes.data(), planes.size() * 2, hipMemcpyHostToDevice), "H2D");
  }
  ~DevTiled() { (void)hipFree(p); }
  const unsigned short* w() const { return static_cast<const unsigned short*>(p); }
};
}  // namespace

int wt_dbg_gemm(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias,
                const float* R, const float* pos, int pos_period, int epi, float* C) {
  if (!h || N % 128 || K % 32) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    DevBuf dA(A, size_t(M) * K), dW(W, size_t(N) * K), dB(bias, N), dC(R ? R : nullptr, size_t(M) * N),
        dP(pos, pos ? size_t(pos_period) * N : 0);
    wt::GemmArgs g;
    g.A = dA.p; g.lda = K; g.W = dW.p; g.bias = dB.p; g.C = dC.p; g.R = dC.p; g.ldc = N;
    g.pos = dP.p; g.pos_period = pos_period > 0 ? pos_period : 1;
    g.M = M; g.N = N; g.K = K; g.variant = int(h->impl->gemm_variant);
    wt::launch_gemm(g, epi, h->impl->stream());
    h->impl->sync();
    dC.to_host(C, size_t(M) * N);
  });
}

namespace {
// fp32 [n] -> device planes: hi [n] then lo [n] halfs of x * scale
struct DevPlanes {
  void* p = nullptr;
  long plane = 0;
  DevPlanes(const float* x, size_t n, float scale, size_t pad = 64) : plane(long(n + pad)) {
    std::vector<unsigned short> host(2 * (n + pad), 0);
    for (size_t i = 0; x && i < n; ++i) {
      const float v = x[i] * scale;
      const _Float16 hi = static_cast<_Float16>(v), lo = static_cast<_Float16>(v - static_cast<float>(hi));
      std::memcpy(&host[i], &hi, 2);
      std::memcpy(&host[n + pad + i], &lo, 2);
    }
    hipchk(hipMalloc(&p, host.size() * 2), "hipMalloc");
    hipchk(hipMemcpy(p, host.data(), host.size() * 2, hipMemcpyHostToDevice), "H2D");
  }
  ~DevPlanes() { (void)hipFree(p); }
  unsigned short* ptr() const { return static_cast<unsigned short*>(p); }
  // device planes -> fp32 (hi + lo) / scale
  void to_host(float* out, size_t n, float scale) const {
    std::vector<unsigned short> host(size_t(2) * plane);
    hipchk(hipMemcpy(host.data(), p, host.size() * 2, hipMemcpyDeviceToHost), "D2H");
    for (size_t i = 0; i < n; ++i) {
      _Float16 hi, lo;
      std::memcpy(&hi, &host[i], 2);
      std::memcpy(&lo, &host[size_t(plane) + i], 2);
      out[i] = (static_cast<float>(hi) + static_cast<float>(lo)) / scale;
    }
  }
};
// W [N][K] as the plane GEMM takes it: split_weight_planes()'s blocked layout on the device
struct DevWeightPlanes {
  void* p = nullptr;
  DevWeightPlanes(const float* W, int N, int K, float scale) {
    const std::vector<unsigned short> host = wt::split_weight_planes(W, N, K, K, scale);
    hipchk(hipMalloc(&p, host.size() * 2 + 256), "hipMalloc");
    hipchk(hipMemcpy(p, host.data(), host.size() * 2, hipMemcpyHostToDevice), "H2D");
  }
  ~DevWeightPlanes() { (void)hipFree(p); }
  unsigned short* ptr() const { return static_cast<unsigned short*>(p); }
};
float max_abs(const float* x, size_t n) {
  float m = 0.0f;
  for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(x[i]));
  return m;
}
}  // namespace

int wt_dbg_gemm_planes(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias,
                       const float* R, const float* pos, int pos_period, int epi, int planes_out, int iters, float* C,
                       float* avg_ms, int n_cu) {
  if (!h || !A || !W || !C || N % 128 || K % 32 || M < 1 || n_cu < 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const float sa = wt::f16_scale_for(max_abs(A, size_t(M) * K)), sw = wt::f16_scale_for(max_abs(W, size_t(N) * K));
    const DevPlanes dA(A, size_t(M) * K, sa);
    const DevWeightPlanes dW(W, N, K, sw);
    DevBuf dB(bias, N), dC(R ? R : nullptr, size_t(M) * N), dP(pos, pos ? size_t(pos_period) * N : 0);
    // plane output: scale from the fp64-free bound sum |a||w| is overkill for a test tap; 2^10 / max |bias| + ... is not
    // known here, so the caller's outputs are assumed O(max|A| max|W| K): use a conservative power of two
    const float out_bound = max_abs(A, size_t(M) * K) * max_abs(W, size_t(N) * K) * float(K) + (bias ? max_abs(bias, N) : 0.0f);
    const float so = wt::f16_scale_for(out_bound);
    DevPlanes dO(nullptr, size_t(M) * N, 1.0f);
    wt::PlaneGemmArgs g;
    g.A = dA.ptr(); g.a_plane = dA.plane; g.lda = K; g.W = dW.ptr(); g.bias = dB.p;
    g.C = dC.p; g.R = dC.p; g.ldc = N; g.pos = dP.p; g.pos_period = pos_period > 0 ? pos_period : 1;
    g.M = M; g.N = N; g.K = K; g.a_scale = sa; g.w_scale = sw; g.n_cu = n_cu;
    if (planes_out) { g.P = dO.ptr(); g.p_plane = dO.plane; g.out_scale[0] = so; }
    hipStream_t st = h->impl->stream();
    wt::launch_gemm_planes(g, epi, st);
    h->impl->sync();
    if (planes_out) dO.to_host(C, size_t(M) * N, so); else dC.to_host(C, size_t(M) * N);
    if (avg_ms && iters > 0) {  // (C has been copied out: a residual epilogue may keep accumulating in place)
      hipEvent_t e0, e1;
      hipchk(hipEventCreate(&e0), "event");
      hipchk(hipEventCreate(&e1), "event");
      for (int i = 0; i < 3; ++i) wt::launch_gemm_planes(g, epi, st);
      hipchk(hipEventRecord(e0, st), "record");
      for (int i = 0; i < iters; ++i) wt::launch_gemm_planes(g, epi, st);
      hipchk(hipEventRecord(e1, st), "record");
      hipchk(hipEventSynchronize(e1), "sync");
      float ms = 0;
      hipchk(hipEventElapsedTime(&ms, e0, e1), "elapsed");
      *avg_ms = ms / iters;
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
    }
  });
}

int wt_dbg_set_forced_ids(wt_engine* h, const int64_t* ids, int clips) {
  if (!h || clips < 0 || clips > 4096 || (clips && !ids)) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    h->impl->forced_ids.assign(ids, ids + size_t(clips) * 32);
    for (long long v : h->impl->forced_ids)
      if (v < 0) throw wt::Error(wt::kErrInvalidArg, "forced ids must be token ids");
  });
}

int wt_dbg_set_plane_gemm_mode(int mode) {
  if (mode < 0 || mode > 4) return WT_ERR_INVALID_ARG;
  wt::set_plane_gemm_mode(mode);
  return WT_OK;
}

int wt_dbg_gemm_planes_ln(wt_engine* h, int M, int K, const float* A, const float* W, const float* bias, const float* R,
                          const float* pos, int pos_period, int epi, const float* ln_g, const float* ln_b, int n_cu,
                          float* C, float* ln_out, float* ln_y32, int* fused) {
  const int N = 384;
  if (!h || !A || !W || !C || !ln_g || !ln_b || !ln_out || !fused || K % 32 || M < 1 || n_cu < 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const float sa = wt::f16_scale_for(max_abs(A, size_t(M) * K)), sw = wt::f16_scale_for(max_abs(W, size_t(N) * K));
    const DevPlanes dA(A, size_t(M) * K, sa);
    const DevWeightPlanes dW(W, N, K, sw);
    DevBuf dB(bias, N), dC(R ? R : nullptr, size_t(M) * N), dP(pos, pos ? size_t(pos_period) * N : 0), dG(ln_g, N), dS(ln_b, N),
        dY(size_t(M) * N), dF(1);
    hipchk(hipMemset(dF.p, 0, 4), "memset");
    const float so = 64.0f;  // LayerNorm output is O(|g| sqrt(N))
    DevPlanes dO(nullptr, size_t(M) * N, 1.0f);
    wt::PlaneGemmArgs g;
    g.A = dA.ptr(); g.a_plane = dA.plane; g.lda = K; g.W = dW.ptr(); g.bias = dB.p;
    g.C = dC.p; g.R = dC.p; g.ldc = N; g.pos = dP.p; g.pos_period = pos_period > 0 ? pos_period : 1;
    g.M = M; g.N = N; g.K = K; g.a_scale = sa; g.w_scale = sw; g.n_cu = n_cu;
    g.ln_g = dG.p; g.ln_b = dS.p; g.ln_P = dO.ptr(); g.ln_plane = dO.plane; g.ln_scale = so;
    g.ln_y32 = ln_y32 ? dY.p : nullptr; g.nonfinite = reinterpret_cast<int*>(dF.p);
    *fused = wt::launch_gemm_planes(g, epi, h->impl->stream()) ? 1 : 0;
    h->impl->sync();
    dC.to_host(C, size_t(M) * N);
    if (*fused) {
      dO.to_host(ln_out, size_t(M) * N, so);
      if (ln_y32) dY.to_host(ln_y32, size_t(M) * N);
    }
  });
}

int wt_dbg_encoder_attention_planes(wt_engine* h, int batch, int T, int heads, const float* qkv, int iters, float* out,
                                    float* avg_ms) {
  if (!h || !qkv || !out) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64, rows = size_t(batch) * T;
    float mq = 0.0f, mk = 0.0f, mv = 0.0f;
    for (size_t r = 0; r < rows; ++r) {
      const float* row = qkv + r * 3 * d;
      for (size_t c = 0; c < d; ++c) {
        mq = std::max(mq, std::fabs(row[c]));
        mk = std::max(mk, std::fabs(row[d + c]));
        mv = std::max(mv, std::fabs(row[2 * d + c]));
      }
    }
    constexpr float kQ = 0.125f * 1.44269504088896340736f;
    const float sq = wt::f16_scale_for(mq * kQ), sk = wt::f16_scale_for(mk), sv = wt::f16_scale_for(mv), so = wt::f16_scale_for(mv);
    // planes as the qkv GEMM's epilogue writes them: q * kQ * sq | k * sk | v * sv
    std::vector<float> scaled(rows * 3 * d);
    for (size_t r = 0; r < rows; ++r)
      for (size_t c = 0; c < 3 * d; ++c)
        scaled[r * 3 * d + c] = qkv[r * 3 * d + c] * (c < d ? kQ * sq : c < 2 * d ? sk : sv);
    const DevPlanes dQ(scaled.data(), scaled.size(), 1.0f);
    DevPlanes dO(nullptr, rows * d, 1.0f);
    hipStream_t st = h->impl->stream();
    wt::launch_encoder_attention_planes(dQ.ptr(), dQ.plane, dO.ptr(), dO.plane, batch, T, heads, sq, sk, sv, so, st);
    h->impl->sync();
    dO.to_host(out, rows * d, so);
    if (avg_ms && iters > 0) {
      hipEvent_t e0, e1;
      hipchk(hipEventCreate(&e0), "event");
      hipchk(hipEventCreate(&e1), "event");
      hipchk(hipEventRecord(e0, st), "record");
      for (int i = 0; i < iters; ++i)
        wt::launch_encoder_attention_planes(dQ.ptr(), dQ.plane, dO.ptr(), dO.plane, batch, T, heads, sq, sk, sv, so, st);
      hipchk(hipEventRecord(e1, st), "record");
      hipchk(hipEventSynchronize(e1), "sync");
      float ms = 0;
      hipchk(hipEventElapsedTime(&ms, e0, e1), "elapsed");
      *avg_ms = ms / iters;
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
    }
  });
}

namespace {
// fp32 [n] -> device bf16 [n + pad] (round to nearest even) and back
struct DevBf16 {
  void* p = nullptr;
  size_t n = 0;
  static unsigned short rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return static_cast<unsigned short>((u >> 16) | 0x40u);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return static_cast<unsigned short>(u >> 16);
  }
  DevBf16(const float* x, size_t n_, size_t pad = 256) : n(n_) {
    std::vector<unsigned short> host(n + pad, 0);
    for (size_t i = 0; x && i < n; ++i) host[i] = rne(x[i]);
    hipchk(hipMalloc(&p, host.size() * 2), "hipMalloc");
    hipchk(hipMemcpy(p, host.data(), host.size() * 2, hipMemcpyHostToDevice), "H2D");
  }
  ~DevBf16() { (void)hipFree(p); }
  unsigned short* ptr() const { return static_cast<unsigned short*>(p); }
  void to_host(float* out, size_t count) const {
    std::vector<unsigned short> host(count);
    hipchk(hipMemcpy(host.data(), p, count * 2, hipMemcpyDeviceToHost), "D2H");
    for (size_t i = 0; i < count; ++i) {
      const uint32_t u = uint32_t(host[i]) << 16;
      std::memcpy(&out[i], &u, 4);
    }
  }
};
float time_launches(hipStream_t st, int iters, const std::function<void()>& f) {
  hipEvent_t e0, e1;
  hipchk(hipEventCreate(&e0), "event");
  hipchk(hipEventCreate(&e1), "event");
  for (int i = 0; i < 3; ++i) f();
  hipchk(hipEventRecord(e0, st), "record");
  for (int i = 0; i < iters; ++i) f();
  hipchk(hipEventRecord(e1, st), "record");
  hipchk(hipEventSynchronize(e1), "sync");
  float ms = 0;
  hipchk(hipEventElapsedTime(&ms, e0, e1), "elapsed");
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return ms / iters;
}
}  // namespace

int wt_dbg_gemm_bf16(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias,
                     const float* R, const float* pos, int pos_period, int epi, int bf16_out, int iters, float* C,
                     float* avg_ms) {
  if (!h || !A || !W || !C || N % 128 || K % 64 || M < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const DevBf16 dA(A, size_t(M) * K), dW(W, size_t(N) * K);
    DevBuf dB(bias, N), dC(R ? R : nullptr, size_t(M) * N), dP(pos, pos ? size_t(pos_period) * N : 0);
    const DevBf16 dO(nullptr, size_t(M) * N);
    wt::PlaneGemmArgs g;
    g.A = dA.ptr(); g.lda = K; g.W = dW.ptr(); g.bias = dB.p;
    g.C = dC.p; g.R = dC.p; g.ldc = N; g.pos = dP.p; g.pos_period = pos_period > 0 ? pos_period : 1;
    g.M = M; g.N = N; g.K = K;
    if (bf16_out) g.P = dO.ptr();
    hipStream_t st = h->impl->stream();
    wt::launch_gemm_bf16_planes(g, epi, st);
    h->impl->sync();
    if (bf16_out) dO.to_host(C, size_t(M) * N); else dC.to_host(C, size_t(M) * N);
    if (avg_ms && iters > 0) {  // (C has been copied out: a residual epilogue may keep accumulating in place)
      *avg_ms = time_launches(st, iters, [&] { wt::launch_gemm_bf16_planes(g, epi, st); });
    }
  });
}

int wt_dbg_gemm_bf16_ln(wt_engine* h, int M, int N, int K, const float* A, const float* W, const float* bias, const float* R,
                        const float* ln_g, const float* ln_b, float* C, float* ln_out, float* ln_y32, int* fused) {
  if (!h || !A || !W || !bias || !R || !ln_g || !ln_b || !C || !ln_out || !ln_y32 || !fused || N % 128 || K % 64 || M < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const DevBf16 dA(A, size_t(M) * K), dW(W, size_t(N) * K);
    DevBuf dB(bias, N), dC(R, size_t(M) * N), dG(ln_g, N), dS(ln_b, N), dY(size_t(M) * N);
    const DevBf16 dL(nullptr, size_t(M) * N);
    wt::PlaneGemmArgs g;  // x += A . W^T + bias, LayerNorm(x) as a bf16 plane and as fp32
    g.A = dA.ptr(); g.lda = K; g.W = dW.ptr(); g.bias = dB.p; g.C = dC.p; g.R = dC.p; g.ldc = N;
    g.M = M; g.N = N; g.K = K;
    g.ln_g = dG.p; g.ln_b = dS.p; g.ln_P = dL.ptr(); g.ln_y32 = dY.p;
    hipStream_t st = h->impl->stream();
    *fused = wt::launch_gemm_bf16_planes(g, wt::kEpiBias | wt::kEpiResidual, st) ? 1 : 0;
    h->impl->sync();
    dC.to_host(C, size_t(M) * N);
    dL.to_host(ln_out, size_t(M) * N);
    dY.to_host(ln_y32, size_t(M) * N);
  });
}

int wt_dbg_encoder_attention_bf16(wt_engine* h, int batch, int T, int heads, const float* qkv, int iters, float* out,
                                  float* avg_ms) {
  if (!h || !qkv || !out) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64, rows = size_t(batch) * T;
    const DevBf16 dQ(qkv, rows * 3 * d), dO(nullptr, rows * d);
    hipStream_t st = h->impl->stream();
    wt::launch_encoder_attention_bf16(dQ.ptr(), dO.ptr(), batch, T, heads, st);
    h->impl->sync();
    dO.to_host(out, rows * d);
    if (avg_ms && iters > 0) {
      *avg_ms = time_launches(st, iters, [&] { wt::launch_encoder_attention_bf16(dQ.ptr(), dO.ptr(), batch, T, heads, st); });
    }
  });
}

int wt_dbg_gemm_bench(wt_engine* h, int M, int N, int K, int epi, int variant, int iters, float* avg_ms) {
  if (!h || N % 128 || K % 32 || iters < 1 || !avg_ms) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    // random operands (zero-filled ones would run at a higher clock and flatter the kernel)
    std::vector<float> hostA(size_t(M) * K), hostW(size_t(N) * K), hostB(N);
    uint64_t x = 88172645463325252ull;
    auto rnd = [&x] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return float(int64_t(x % 2000001) - 1000000) * 1e-6f; };
    for (auto& v : hostA) v = rnd();
    for (auto& v : hostW) v = rnd() * 0.05f;
    for (auto& v : hostB) v = rnd();
    DevBuf dA(hostA.data(), hostA.size()), dW(hostW.data(), hostW.size()), dB(hostB.data(), N), dC(size_t(M) * N);
    hipchk(hipMemset(dC.p, 0, size_t(M) * N * 4), "memset");
    wt::GemmArgs g;
    g.A = dA.p; g.lda = K; g.W = dW.p; g.bias = dB.p; g.C = dC.p; g.R = dC.p; g.ldc = N;
    g.M = M; g.N = N; g.K = K; g.variant = variant;
    g.a_scale = wt::f16_scale_for(1.0f);
    g.w_scale = wt::f16_scale_for(0.05f);
    hipStream_t st = h->impl->stream();
    hipEvent_t e0, e1;
    hipchk(hipEventCreate(&e0), "event");
    hipchk(hipEventCreate(&e1), "event");
    for (int i = 0; i < 3; ++i) wt::launch_gemm(g, epi, st);
    hipchk(hipEventRecord(e0, st), "record");
    for (int i = 0; i < iters; ++i) wt::launch_gemm(g, epi, st);
    hipchk(hipEventRecord(e1, st), "record");
    hipchk(hipEventSynchronize(e1), "sync");
    float ms = 0;
    hipchk(hipEventElapsedTime(&ms, e0, e1), "elapsed");
    *avg_ms = ms / iters;
    if (getenv("WT_VERBOSE_OCCUPANCY")) fprintf(stderr, "[wt] gemm variant %d: %d blocks per CU\n", g.variant, wt::gemm_occupancy(g.variant));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  });
}

int wt_dbg_interference(wt_engine* h, const float* d_mel, int batch, int n_enc, int chain_len, int blocks,
                        float* enc_ms, float* chain_ms) {
  if (!h || !d_mel || !enc_ms || !chain_ms || batch < 1 || batch > 64 || n_enc < 0 || n_enc > 8 ||
      chain_len < 0 || blocks < 1 || blocks > 4096)
    return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.sync();
    DevBuf buf(size_t(4096));
    hipStream_t es = e.stream(), ds = e.decoder_stream(0);
    hipEvent_t ev[4];
    for (auto& x : ev) hipchk(hipEventCreate(&x), "event");
    hipchk(hipEventRecord(ev[0], es), "record");
    for (int i = 0; i < n_enc; ++i) e.encode(d_mel, batch);
    hipchk(hipEventRecord(ev[1], es), "record");
    hipchk(hipEventRecord(ev[2], ds), "record");
    for (int i = 0; i < chain_len; ++i) wt::launch_chain_probe(buf.p, blocks, ds);
    hipchk(hipEventRecord(ev[3], ds), "record");
    hipchk(hipEventSynchronize(ev[1]), "sync");
    hipchk(hipEventSynchronize(ev[3]), "sync");
    hipchk(hipEventElapsedTime(enc_ms, ev[0], ev[1]), "elapsed");
    hipchk(hipEventElapsedTime(chain_ms, ev[2], ev[3]), "elapsed");
    for (auto& x : ev) (void)hipEventDestroy(x);
  });
}

int wt_dbg_concurrency(wt_engine* h, const float* d_mel, int batch, int n_dec, int n_enc, float* dec_ms,
                       float* enc_ms) {
  if (!h || !d_mel || !dec_ms || !enc_ms || batch < 1 || batch > 64) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] { h->impl->debug_concurrency(d_mel, batch, n_dec, n_enc, dec_ms, enc_ms); });
}

int wt_dbg_dec_gemm_bench(wt_engine* h, int kind, int B, int N, int K, int rows, int iters, float* avg_us) {
  if (!h || !avg_us || B < 1 || B > 64 || iters < 1 || rows < B || rows % B != 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    // kind 0: residual GEMM, 1: LayerNorm-fused GEMM (+bias), 2: combine + residual GEMM, 3: LayerNorm + logits + argmax records
    std::vector<float> hostW(size_t(N) * K), hostX(size_t(rows) * std::max(K, N));
    uint64_t x = 88172645463325252ull;
    auto rnd = [&x] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return float(int64_t(x % 2000001) - 1000000) * 1e-6f; };
    for (auto& v : hostW) v = rnd() * 0.05f;
    for (auto& v : hostX) v = rnd();
    const DevTiled dW(hostW.data(), N, K);
    const int heads = K / 64, chunks = 2;
    DevBuf dX(hostX.data(), size_t(rows) * K), dB(hostX.data(), N), dG(hostX.data(), K);
    DevBuf dY(hostX.data(), size_t(rows) * N), dWs(size_t(rows) * heads * chunks * 68);
    std::vector<float> ws(size_t(rows) * heads * chunks * 68);
    for (auto& v : ws) v = rnd();
    hipchk(hipMemcpy(dWs.p, ws.data(), ws.size() * 4, hipMemcpyHostToDevice), "H2D");
    wt::DecGemmArgs g;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = N; g.K = K; g.B = B; g.M = rows; g.bias = dB.p; g.Y = dY.p; g.ldy = N;
    int pro = wt::kProNone, epi = wt::kDecResid;
    DevBuf dPart(size_t(rows) * N), dR(hostX.data(), size_t(rows) * N);
    if (kind == 0) { g.X = dX.p; g.ldx = K; g.R = dY.p; }
    if (kind == 0 && K > 1024) { g.ksplit = 2; g.part = dPart.p; g.R = dR.p; }  // fc2: K split over twice the blocks
    if (kind == 1) { pro = wt::kProLn; epi = wt::kDecBias; g.xin = dX.p; g.ln_g = dG.p; g.ln_b = dG.p; }
    if (kind == 2) { pro = wt::kProCombine; g.cross_ws = dWs.p; g.heads = heads; g.chunks = chunks; g.R = dY.p; }
    DevBuf dBest(kind == 3 ? size_t(rows) * 2 * size_t((N + 31) / 32) : 1);
    if (kind == 3) {  // final LayerNorm + logits + argmax records (the persistent kernel; no logits written)
      pro = wt::kProLn; epi = wt::kDecLogits; g.xin = dX.p; g.ln_g = dG.p; g.ln_b = dG.p; g.Y = nullptr; g.bias = nullptr;
      g.best = reinterpret_cast<unsigned long long*>(dBest.p);
    }
    hipStream_t st = h->impl->stream();
    hipEvent_t e0, e1;
    hipchk(hipEventCreate(&e0), "event");
    hipchk(hipEventCreate(&e1), "event");
    for (int i = 0; i < 5; ++i) wt::launch_dec_gemm(g, pro, epi, st);
    hipchk(hipEventRecord(e0, st), "record");
    for (int i = 0; i < iters; ++i) wt::launch_dec_gemm(g, pro, epi, st);
    hipchk(hipEventRecord(e1, st), "record");
    hipchk(hipEventSynchronize(e1), "sync");
    float ms = 0;
    hipchk(hipEventElapsedTime(&ms, e0, e1), "elapsed");
    *avg_us = 1e3f * ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  });
}

static int dbg_dec_gemm_impl(wt_engine* h, int mode, int B, int N, int K, const float* X, const float* W, const float* bias,
                             const float* R, float* Y, int64_t* argmax_out, bool bf) {
  if (!h || mode < 0 || mode > 3 || B < 1 || B > 128 || (mode == 2 && !R)) {
    return WT_ERR_INVALID_ARG;
  }
  // B rows in all; more than 64 rows are presented as positions x clips (the kernels' row = p * B + b)
  const int rows_per = B > 64 ? (B % 4 == 0 ? B / 4 : (B % 2 == 0 ? B / 2 : 0)) : B;
  if (rows_per == 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const DevTiled dW(W, N, K, bf);
    const int n_tiles = (N + 31) / 32;
    DevBuf dX(X, size_t(B) * K), dB(bias, N);
    DevBuf dY(mode == 2 ? R : nullptr, size_t(B) * N);
    DevBuf dBest(size_t(B) * 2 * n_tiles);
    hipchk(hipMemset(dBest.p, 0, size_t(B) * 8 * n_tiles), "memset");
    wt::DecGemmArgs g;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = N; g.K = K; g.B = rows_per > 0 ? rows_per : B; g.M = B; g.X = dX.p; g.ldx = K;
    g.bf16 = bf;
    g.bias = dB.p; g.R = dY.p; g.Y = dY.p; g.ldy = N;  // residual in place, as the engine does
    g.best = reinterpret_cast<unsigned long long*>(dBest.p);
    const int epi = mode == 0 ? wt::kDecBias : mode == 1 ? wt::kDecBiasGelu : mode == 2 ? wt::kDecResid : wt::kDecLogits;
    wt::launch_dec_gemm(g, wt::kProNone, epi, h->impl->stream());
    h->impl->sync();
    dY.to_host(Y, size_t(B) * N);
    if (argmax_out && mode == 3) {
      // reduce the per-tile records exactly as select_token does (max of the packed keys)
      std::vector<unsigned long long> best(size_t(B) * n_tiles);
      hipchk(hipMemcpy(best.data(), dBest.p, best.size() * 8, hipMemcpyDeviceToHost), "D2H");
      for (int b = 0; b < B; ++b) {
        unsigned long long m = 0;
        for (int t = 0; t < n_tiles; ++t) m = std::max(m, best[size_t(b) * n_tiles + t]);
        argmax_out[b] = int64_t(m & 0xffffffffull);
      }
    }
  });
}

int wt_dbg_dec_gemm(wt_engine* h, int mode, int B, int N, int K, const float* X, const float* W,
                    const float* bias, const float* R, float* Y, int64_t* argmax_out) {
  return dbg_dec_gemm_impl(h, mode, B, N, K, X, W, bias, R, Y, argmax_out, false);
}
int wt_dbg_dec_gemm_bf16(wt_engine* h, int mode, int B, int N, int K, const float* X, const float* W,
                         const float* bias, const float* R, float* Y, int64_t* argmax_out) {
  return dbg_dec_gemm_impl(h, mode, B, N, K, X, W, bias, R, Y, argmax_out, true);
}

static int dbg_dec_ln_gemm_impl(wt_engine* h, int B, int N, int K, const float* xin, const int64_t* ids, int pos,
                                const float* tok_emb, const float* pos_emb, int n_vocab, int n_pos, const float* ln_g,
                                const float* ln_b, const float* W, const float* bias, int gelu, float* Y, float* xout, bool bf) {
  if (!h || B < 1 || B > 64 || (K != 128 && K != 384 && K != 512) || (!xin && !ids) || pos < 0 || (ids && pos >= n_pos)) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const DevTiled dW(W, N, K, bf);
    DevBuf dxin(xin, xin ? size_t(B) * K : 0);
    DevBuf dtok(tok_emb, ids ? size_t(n_vocab) * K : 0), dpos(pos_emb, ids ? size_t(n_pos) * K : 0);
    DevBuf dg(ln_g, K), db(ln_b, K), dB(bias, N), dY(size_t(B) * N), dxo(size_t(B) * K);
    // the kernel reads ids[b][pos]: one row of pos + 1 ids per clip, the given id in its last column
    std::vector<long long> idrows(size_t(B) * (pos + 1), 0);
    if (ids)
      for (int b = 0; b < B; ++b) idrows[size_t(b) * (pos + 1) + pos] = ids[b];
    DevBuf dids(idrows.size() * 2);
    hipchk(hipMemcpy(dids.p, idrows.data(), idrows.size() * 8, hipMemcpyHostToDevice), "H2D ids");
    hipchk(hipMemset(dxo.p, 0, size_t(B) * K * 4), "memset");
    wt::DecGemmArgs g;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = N; g.K = K; g.B = B; g.bf16 = bf;
    g.xin = dxin.p; g.xout = dxo.p; g.ln_g = dg.p; g.ln_b = db.p;
    if (ids) {
      g.ids = reinterpret_cast<const long long*>(dids.p); g.ids_stride = pos + 1; g.pos = pos;
      g.tok_emb = dtok.p; g.pos_emb = dpos.p; g.n_vocab = n_vocab;
    }
    g.bias = dB.p; g.Y = dY.p; g.ldy = N;
    wt::launch_dec_gemm(g, wt::kProLn, gelu ? wt::kDecBiasGelu : wt::kDecBias, h->impl->stream());
    h->impl->sync();
    dY.to_host(Y, size_t(B) * N);
    if (xout) dxo.to_host(xout, size_t(B) * K);
  });
}

int wt_dbg_dec_ln_gemm(wt_engine* h, int B, int N, int K, const float* xin, const int64_t* ids, int pos,
                       const float* tok_emb, const float* pos_emb, int n_vocab, int n_pos,
                       const float* ln_g, const float* ln_b, const float* W, const float* bias,
                       int gelu, float* Y, float* xout) {
  return dbg_dec_ln_gemm_impl(h, B, N, K, xin, ids, pos, tok_emb, pos_emb, n_vocab, n_pos, ln_g, ln_b, W, bias, gelu, Y, xout, false);
}
int wt_dbg_dec_ln_gemm_bf16(wt_engine* h, int B, int N, int K, const float* xin, const int64_t* ids, int pos,
                            const float* tok_emb, const float* pos_emb, int n_vocab, int n_pos,
                            const float* ln_g, const float* ln_b, const float* W, const float* bias,
                            int gelu, float* Y, float* xout) {
  return dbg_dec_ln_gemm_impl(h, B, N, K, xin, ids, pos, tok_emb, pos_emb, n_vocab, n_pos, ln_g, ln_b, W, bias, gelu, Y, xout, true);
}

int wt_dbg_layernorm(wt_engine* h, int M, int d, const float* x, const float* g, const float* b, float* y) {
  if (!h || d > 512) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    DevBuf dx(x, size_t(M) * d), dg(g, d), db(b, d), dy(size_t(M) * d);
    wt::launch_layernorm(dx.p, dy.p, dg.p, db.p, M, d, h->impl->stream());
    h->impl->sync();
    dy.to_host(y, size_t(M) * d);
  });
}

int wt_dbg_encoder_attention(wt_engine* h, int batch, int T, int heads, const float* qkv, float* out) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64;
    DevBuf dq(qkv, size_t(batch) * T * 3 * d), dout(size_t(batch) * T * d);
    float mq = 0.0f, mk = 0.0f, mv = 0.0f;  // operand scales of variant 4 from the data
    for (size_t r = 0; r < size_t(batch) * T; ++r) {
      const float* row = qkv + r * 3 * d;
      for (size_t c = 0; c < d; ++c) {
        mq = std::max(mq, std::fabs(row[c]));
        mk = std::max(mk, std::fabs(row[d + c]));
        mv = std::max(mv, std::fabs(row[2 * d + c]));
      }
    }
    (void)mq; (void)mk; (void)mv;
    // fp32-storage forms only (0, 1); the default plane kernel has its own tap (wt_dbg_encoder_attention_planes)
    wt::launch_encoder_attention(dq.p, dout.p, batch, T, heads, h->impl->attn_variant == 4 ? 1 : int(h->impl->attn_variant),
                                 h->impl->stream());
    h->impl->sync();
    dout.to_host(out, size_t(batch) * T * d);
  });
}

static int dbg_cross_attention_impl(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                                    const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                                    const float* vc, float* out, bool bf) {
  if (!h || (chunks != 1 && chunks != 2 && chunks != 4 && chunks != 8) || batch < 1 || nq < 1 || nq * batch > 128 ||
      !x || !ln_g || !ln_b || !wq || !bq || !kc || !vc || !out)
    return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64, rows = size_t(nq) * batch;
    DevBuf dx(x, rows * d), dg(ln_g, d), db(ln_b, d), dbq(bq, d), dk(bf ? nullptr : kc, bf ? 0 : size_t(batch) * T * d),
        dv(bf ? nullptr : vc, bf ? 0 : size_t(batch) * T * d);
    const DevBf16 dkb(bf ? kc : nullptr, bf ? size_t(batch) * T * d : 0), dvb(bf ? vc : nullptr, bf ? size_t(batch) * T * d : 0);
    const std::vector<float> wqt = wt::cross_q_layout(wq, int(d));
    DevBuf dwq(wqt.data(), wqt.size());
    DevBuf dws(rows * heads * chunks * 68), dout(rows * d), dzero(d);
    hipchk(hipMemset(dout.p, 0, rows * d * 4), "memset");
    hipchk(hipMemset(dzero.p, 0, d * 4), "memset");
    // the product combines the chunk partials in the out-projection's prologue; an identity
    // projection onto a zero residual exposes exactly that combined row
    std::vector<float> eye(d * d, 0.0f);
    for (size_t i = 0; i < d; ++i) eye[i * d + i] = 1.0f;
    const DevTiled dW(eye.data(), int(d), int(d));
    wt::CrossAttnArgs ca;
    ca.x = dx.p; ca.ln_g = dg.p; ca.ln_b = db.p; ca.wq_t = dwq.p; ca.bq = dbq.p;
    ca.kc = bf ? static_cast<const void*>(dkb.ptr()) : dk.p; ca.vc = bf ? static_cast<const void*>(dvb.ptr()) : dv.p; ca.bf16 = bf;
    ca.ws = dws.p; ca.batch = batch; ca.heads = heads; ca.T = T; ca.chunks = chunks; ca.nq = nq;
    wt::launch_cross_attention(ca, h->impl->stream());
    wt::DecGemmArgs g;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = int(d); g.K = int(d); g.B = batch; g.M = int(rows);
    g.cross_ws = dws.p; g.heads = heads; g.chunks = chunks;
    g.bias = dzero.p; g.R = dout.p; g.Y = dout.p; g.ldy = int(d);
    wt::launch_dec_gemm(g, wt::kProCombine, wt::kDecResid, h->impl->stream());
    h->impl->sync();
    dout.to_host(out, rows * d);
  });
}

int wt_dbg_cross_attention(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                           const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                           const float* vc, float* out) {
  return dbg_cross_attention_impl(h, batch, heads, T, chunks, nq, x, ln_g, ln_b, wq, bq, kc, vc, out, false);
}
int wt_dbg_cross_attention_bf16(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* x,
                                const float* ln_g, const float* ln_b, const float* wq, const float* bq, const float* kc,
                                const float* vc, float* out) {
  return dbg_cross_attention_impl(h, batch, heads, T, chunks, nq, x, ln_g, ln_b, wq, bq, kc, vc, out, true);
}

static int dbg_cross_absorbed_impl(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* qp, const float* E,
                                   const float* wv, const float* bv, float* out, int iters, float* avg_us, bool bf) {
  if (!h || !qp || !E || !wv || !bv || !out || batch < 1 || heads < 1 || T < 1 || nq < 1 || chunks < 1 || chunks > 16) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64, rows = size_t(nq) * batch;
    const float se = bf ? 1.0f : wt::f16_scale_for(max_abs(E, size_t(batch) * T * d));
    const DevPlanes dEp(bf ? nullptr : E, bf ? 0 : size_t(batch) * T * d, se);
    const DevBf16 dEb(bf ? E : nullptr, bf ? size_t(batch) * T * d : 0);
    struct { const unsigned short* p; long plane; const unsigned short* ptr() const { return p; } } dE{bf ? dEb.ptr() : dEp.ptr(), bf ? 0 : dEp.plane};
    const std::vector<float> wvt = wt::cross_q_layout(wv, int(d));
    DevBuf dq(qp, rows * heads * d), dws(rows * heads * chunks * (d + 4)), dout(rows * d), dwv(wvt.data(), wvt.size()), dbv(bv, d);
    const int nq_max = wt::cross_absorbed_max_nq(heads);
    for (int p0 = 0; p0 < nq; p0 += nq_max) {
      wt::CrossAbsorbedArgs a;
      a.qp = dq.p; a.e = dE.ptr(); a.e_plane = dE.plane; a.e_scale = se; a.ws = dws.p; a.bf16 = bf;
      a.batch = batch; a.heads = heads; a.d_model = int(d); a.T = T; a.chunks = chunks; a.nq = std::min(nq_max, nq - p0); a.p0 = p0;
      wt::launch_cross_absorbed(a, h->impl->stream());
    }
    wt::launch_cross_absorbed_combine(dws.p, dwv.p, dbv.p, dout.p, int(rows), heads, chunks, int(d), h->impl->stream());
    h->impl->sync();
    dout.to_host(out, rows * d);
    if (iters > 0 && avg_us) {
      wt::CrossAbsorbedArgs a;
      a.qp = dq.p; a.e = dE.ptr(); a.e_plane = dE.plane; a.e_scale = se; a.ws = dws.p; a.bf16 = bf;
      a.batch = batch; a.heads = heads; a.d_model = int(d); a.T = T; a.chunks = chunks; a.nq = std::min(nq_max, nq); a.p0 = 0;
      hipStream_t st = h->impl->stream();
      hipEvent_t e0, e1;
      hipchk(hipEventCreate(&e0), "event");
      hipchk(hipEventCreate(&e1), "event");
      for (int i = 0; i < 3; ++i) wt::launch_cross_absorbed(a, st);
      hipchk(hipEventRecord(e0, st), "record");
      for (int i = 0; i < iters; ++i) wt::launch_cross_absorbed(a, st);
      hipchk(hipEventRecord(e1, st), "record");
      hipchk(hipEventSynchronize(e1), "sync");
      float ms = 0;
      hipchk(hipEventElapsedTime(&ms, e0, e1), "elapsed");
      *avg_us = 1e3f * ms / iters;
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
    }
  });
}

int wt_dbg_cross_absorbed(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* qp, const float* E,
                          const float* wv, const float* bv, float* out, int iters, float* avg_us) {
  return dbg_cross_absorbed_impl(h, batch, heads, T, chunks, nq, qp, E, wv, bv, out, iters, avg_us, false);
}

int wt_dbg_cross_absorbed_bf16(wt_engine* h, int batch, int heads, int T, int chunks, int nq, const float* qp, const float* E,
                               const float* wv, const float* bv, float* out, int iters, float* avg_us) {
  return dbg_cross_absorbed_impl(h, batch, heads, T, chunks, nq, qp, E, wv, bv, out, iters, avg_us, true);
}

static int dbg_self_attention_impl(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                                   float* kcache, float* vcache, float* out, bool bf) {
  if (!h || npos < 1 || pos < 0 || pos + npos > cap || cap > 64) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64, rows = size_t(npos) * batch, nc = size_t(batch) * cap * d;
    DevBuf dq(qkv, rows * 3 * d), dk(bf ? nullptr : kcache, bf ? 0 : nc), dv(bf ? nullptr : vcache, bf ? 0 : nc), dout(rows * d);
    const DevBf16 dkb(bf ? kcache : nullptr, bf ? nc : 0), dvb(bf ? vcache : nullptr, bf ? nc : 0);  // bf16 caches (storage mode)
    wt::launch_self_attention(dq.p, bf ? static_cast<void*>(dkb.ptr()) : dk.p, bf ? static_cast<void*>(dvb.ptr()) : dv.p, cap, pos,
                              npos, dout.p, batch, heads, h->impl->stream(), bf);
    h->impl->sync();
    dout.to_host(out, rows * d);
    if (bf) {
      dkb.to_host(kcache, nc);
      dvb.to_host(vcache, nc);
    } else {
      dk.to_host(kcache, nc);
      dv.to_host(vcache, nc);
    }
  });
}
int wt_dbg_self_attention(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                          float* kcache, float* vcache, float* out) {
  return dbg_self_attention_impl(h, batch, heads, cap, pos, npos, qkv, kcache, vcache, out, false);
}
int wt_dbg_self_attention_bf16(wt_engine* h, int batch, int heads, int cap, int pos, int npos, const float* qkv,
                               float* kcache, float* vcache, float* out) {
  return dbg_self_attention_impl(h, batch, heads, cap, pos, npos, qkv, kcache, vcache, out, true);
}
int wt_dbg_self_attention_long(wt_engine* h, int batch, int heads, int cap, int pos, const float* qkv, float* kcache,
                               float* vcache, float* out) {
  if (!h) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::check_self_attention_long(cap, pos, batch, heads);  // the launcher's own refusals, before anything is allocated
    if (!qkv || !kcache || !vcache || !out) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_self_attention_long: NULL array");
    const size_t d = size_t(heads) * 64, nc = size_t(batch) * cap * d;
    DevBuf dq(qkv, size_t(batch) * 3 * d), dk(kcache, nc), dv(vcache, nc), dout(size_t(batch) * d);
    wt::launch_self_attention_long(dq.p, dk.p, dv.p, cap, pos, dout.p, batch, heads, h->impl->stream());
    h->impl->sync();
    dout.to_host(out, size_t(batch) * d);
    dk.to_host(kcache, nc);
    dv.to_host(vcache, nc);
  });
}

}  // extern "C"

namespace {
// device copy of a host array of n elements of T (n = 0 or host = nullptr: uninitialised, at least one element)
template <class T>
struct DevArr {
  T* p = nullptr;
  size_t n = 0;
  explicit DevArr(size_t n_, const T* host = nullptr) : n(n_) {
    hipchk(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T)), "hipMalloc");
    if (host && n) hipchk(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice), "H2D");
  }
  ~DevArr() { (void)hipFree(p); }
  void to_host(T* host) const {
    if (host && n) hipchk(hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost), "D2H");
  }
};

// the engine's per-clip beam state (ensure_beam_workspace), host in / host out
struct DevBeamState {
  static constexpr size_t C = wt::kBeamClipsMax, S = wt::kBeamMax;
  DevArr<float> live_sum, fin_sum;
  DevArr<int> fin_tok, fin_len, n_fin, done;
  DevBeamState(const float* ls, const int32_t* ft, const float* fs, const int32_t* fl, const int32_t* nf, const int32_t* dn)
      : live_sum(C * S, ls), fin_sum(C * S, fs), fin_tok(C * S * 32, ft), fin_len(C * S, fl), n_fin(C, nf), done(C, dn) {}
};
}  // namespace

extern "C" {

int wt_dbg_beam_topk(wt_engine* h, int rows, int V, int ldl, int kk, const float* logits, float* m, float* s,
                     uint64_t* keys) {
  if (!h || !logits || !m || !s || !keys || rows < 1 || V < 1 || ldl < V || kk < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const int chunks = wt::beam_chunks(V);
    DevArr<float> dz(size_t(rows) * ldl, logits);
    DevArr<wt::BeamPart> dp(size_t(rows) * chunks);
    hipchk(hipMemset(dp.p, 0, dp.n * sizeof(wt::BeamPart)), "memset");
    wt::launch_beam_topk(dz.p, ldl, V, rows, kk, dp.p, h->impl->stream());
    h->impl->sync();
    std::vector<wt::BeamPart> part(dp.n);
    dp.to_host(part.data());
    for (size_t i = 0; i < part.size(); ++i) {
      m[i] = part[i].m;
      s[i] = part[i].s;
      for (int r = 0; r < kk; ++r) keys[i * kk + r] = part[i].key[r];
    }
  });
}

int wt_dbg_beam_step(wt_engine* h, int K, int clips, int c0, int n_live, int pos, int n_prompt, int V, int64_t eot,
                     const float* logits, const int64_t* ids, float* live_sum, int32_t* fin_tok, float* fin_sum,
                     int32_t* fin_len, int32_t* n_fin, int32_t* done, int32_t* parent, int64_t* token, int64_t* ids_next) {
  if (!h || !logits || !ids || !live_sum || !fin_tok || !fin_sum || !fin_len || !n_fin || !done || !parent || !token ||
      !ids_next || K < 1 || clips < 1 || n_live < 1 || V < 1 || size_t(K) * clips > 128 || size_t(n_live) * clips > 128) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    hipStream_t st = h->impl->stream();
    const int src_rows = n_live * clips, dst_rows = K * clips;
    DevArr<float> dz(size_t(src_rows) * V, logits);
    DevArr<wt::BeamPart> dp(size_t(src_rows) * wt::beam_chunks(V));
    DevArr<long long> dids(size_t(src_rows) * 32, reinterpret_cast<const long long*>(ids)), dnext(size_t(dst_rows) * 32);
    DevArr<int> dparent(dst_rows);
    DevArr<long long> dtoken(dst_rows);
    DevBeamState bs(live_sum, fin_tok, fin_sum, fin_len, n_fin, done);
    wt::launch_beam_topk(dz.p, V, V, src_rows, K + 1, dp.p, st);
    wt::BeamStepArgs sa;
    sa.part = dp.p; sa.n_chunks = wt::beam_chunks(V); sa.ids = dids.p;
    sa.clips = clips; sa.K = K; sa.n_live = n_live; sa.pos = pos; sa.n_prompt = n_prompt; sa.V = V; sa.c0 = c0;
    sa.eot = eot;
    sa.live_sum = bs.live_sum.p; sa.fin_tok = bs.fin_tok.p; sa.fin_sum = bs.fin_sum.p; sa.fin_len = bs.fin_len.p;
    sa.n_fin = bs.n_fin.p; sa.done = bs.done.p; sa.parent = dparent.p; sa.token = dtoken.p;
    wt::launch_beam_select(sa, st);
    wt::BeamReorderArgs ra;  // the id rows only, as after decode_beam's last step
    ra.src_rows = src_rows; ra.dst_rows = dst_rows; ra.cap = 32; ra.d = 4; ra.slabs = 0; ra.pos = pos; ra.V = V;
    ra.ids_src = dids.p; ra.ids_dst = dnext.p; ra.parent = dparent.p; ra.token = dtoken.p;
    wt::launch_beam_reorder(ra, st);
    h->impl->sync();
    bs.live_sum.to_host(live_sum);
    bs.fin_tok.to_host(fin_tok);
    bs.fin_sum.to_host(fin_sum);
    bs.fin_len.to_host(fin_len);
    bs.n_fin.to_host(n_fin);
    bs.done.to_host(done);
    dparent.to_host(parent);
    dtoken.to_host(reinterpret_cast<long long*>(token));
    dnext.to_host(reinterpret_cast<long long*>(ids_next));
  });
}

int wt_dbg_beam_reorder(wt_engine* h, int src_rows, int dst_rows, int cap, int d, int slabs, int pos, int V,
                        const float* kv_src, float* kv_dst, const int64_t* ids_src, int64_t* ids_dst,
                        const int32_t* parent, const int64_t* token) {
  if (!h || !ids_src || !ids_dst || !parent || !token || src_rows < 1 || dst_rows < 1 || cap < 1 || d < 1 || slabs < 0 ||
      src_rows > 128 || dst_rows > 128 || (slabs > 0 && (!kv_src || !kv_dst))) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t row = size_t(cap) * d;
    DevArr<float> dsrc(slabs > 0 ? size_t(slabs) * src_rows * row : 0, kv_src);
    DevArr<float> ddst(slabs > 0 ? (size_t(slabs) * dst_rows + 1) * row : 0, kv_dst);
    DevArr<long long> dids_src(size_t(src_rows) * 32, reinterpret_cast<const long long*>(ids_src));
    DevArr<long long> dids_dst(size_t(128) * 32, reinterpret_cast<const long long*>(ids_dst));
    DevArr<int> dparent(dst_rows, parent);
    DevArr<long long> dtoken(dst_rows, reinterpret_cast<const long long*>(token));
    wt::BeamReorderArgs ra;
    ra.kv_src = slabs > 0 ? dsrc.p : nullptr; ra.kv_dst = slabs > 0 ? ddst.p : nullptr;
    ra.src_rows = src_rows; ra.dst_rows = dst_rows; ra.cap = cap; ra.d = d; ra.slabs = slabs; ra.pos = pos; ra.V = V;
    ra.ids_src = dids_src.p; ra.ids_dst = dids_dst.p; ra.parent = dparent.p; ra.token = dtoken.p;
    wt::launch_beam_reorder(ra, h->impl->stream());
    h->impl->sync();
    if (slabs > 0) ddst.to_host(kv_dst);
    dids_dst.to_host(reinterpret_cast<long long*>(ids_dst));
  });
}

int wt_dbg_beam_finalize(wt_engine* h, int K, int clips, int c0, int pos, int n_prompt, const int64_t* ids,
                         const float* live_sum, int32_t* fin_tok, float* fin_sum, int32_t* fin_len, int32_t* n_fin,
                         const int32_t* done, int64_t* out_ids, int32_t* out_n, float* out_sum, int32_t* out_len) {
  if (!h || !ids || !live_sum || !fin_tok || !fin_sum || !fin_len || !n_fin || !done || !out_ids || !out_n || !out_sum ||
      !out_len || K < 1 || clips < 1 || size_t(K) * clips > 128) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    constexpr size_t C = wt::kBeamClipsMax;
    DevArr<long long> dids(size_t(K) * clips * 32, reinterpret_cast<const long long*>(ids));
    DevBeamState bs(live_sum, fin_tok, fin_sum, fin_len, n_fin, done);
    DevArr<long long> dout(C * 32, reinterpret_cast<const long long*>(out_ids));
    DevArr<int> dn(C, out_n), dlen(C, out_len);
    DevArr<float> dsum(C, out_sum);
    wt::BeamFinalArgs fa;
    fa.ids = dids.p; fa.clips = clips; fa.K = K; fa.c0 = c0; fa.pos = pos; fa.n_prompt = n_prompt;
    fa.live_sum = bs.live_sum.p; fa.fin_tok = bs.fin_tok.p; fa.fin_sum = bs.fin_sum.p; fa.fin_len = bs.fin_len.p;
    fa.n_fin = bs.n_fin.p; fa.done = bs.done.p;
    fa.out_ids = dout.p; fa.out_n = dn.p; fa.out_sum = dsum.p; fa.out_len = dlen.p;
    wt::launch_beam_finalize(fa, h->impl->stream());
    h->impl->sync();
    bs.fin_tok.to_host(fin_tok);
    bs.fin_sum.to_host(fin_sum);
    bs.fin_len.to_host(fin_len);
    bs.n_fin.to_host(n_fin);
    dout.to_host(reinterpret_cast<long long*>(out_ids));
    dn.to_host(out_n);
    dsum.to_host(out_sum);
    dlen.to_host(out_len);
  });
}

// ------------------------------------------- the greedy step's tail, kernel by kernel ---
int wt_dbg_dec_gemm_ksplit(wt_engine* h, int bf16, int M, int B, int N, int K, const float* X, const float* W,
                           const float* bias, float* R, float* Y, float* part) {
  if (!h || !X || !W || !bias || !R || !Y || !part || B < 1 || M < B || M > 128 || M % B != 0 || N < 1 || K < 1) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const bool bf = bf16 != 0;
    const DevTiled dW(W, N, K, bf);
    const size_t mn = size_t(M) * N;
    DevArr<float> dX(size_t(M) * K, X), dB(N, bias), dR(mn, R), dY(mn, Y), dP(mn, part);
    wt::DecGemmArgs g;  // the engine's fc2 with fc2_ksplit = 2: out of place, second K-half into `part`
    g.bf16 = bf;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = N; g.K = K; g.B = B; g.M = M; g.X = dX.p; g.ldx = K;
    g.bias = dB.p; g.R = dR.p; g.Y = dY.p; g.ldy = N; g.ksplit = 2; g.part = dP.p;
    wt::launch_dec_gemm(g, wt::kProNone, wt::kDecResid, h->impl->stream());
    h->impl->sync();
    dR.to_host(R);
    dY.to_host(Y);
    dP.to_host(part);
  });
}

int wt_dbg_dec_ln_gemm_rows(wt_engine* h, int bf16, int M, int B, int N, int K, const float* xin, const float* xpart,
                            const int64_t* ids, int ids_stride, int pos, const float* tok_emb, const float* pos_emb,
                            int n_vocab, int n_pos, const float* ln_g, const float* ln_b, const float* W, const float* bias,
                            int gelu, float* Y, float* xout) {
  if (!h || !ln_g || !ln_b || !W || !bias || !Y || !xout || B < 1 || M < B || M > 128 || M % B != 0 || N < 1 ||
      (K != 128 && K != 384 && K != 512) || (ids ? (xin || xpart) : !xin)) {
    return WT_ERR_INVALID_ARG;
  }
  const int np = M / B;
  if (ids && (!tok_emb || !pos_emb || n_vocab < 1 || pos < 0 || pos + np > ids_stride || pos + np > n_pos)) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const bool bf = bf16 != 0;
    const DevTiled dW(W, N, K, bf);
    const size_t mk = size_t(M) * K;
    DevArr<float> dxin(xin ? mk : 0, xin), dxp(xpart ? mk : 0, xpart);
    DevArr<long long> dids(ids ? size_t(B) * ids_stride : 0, reinterpret_cast<const long long*>(ids));
    DevArr<float> dtok(ids ? size_t(n_vocab) * K : 0, tok_emb), dpos(ids ? size_t(n_pos) * K : 0, pos_emb);
    DevArr<float> dg(K, ln_g), db(K, ln_b), dB(N, bias), dY(size_t(M) * N);
    DevArr<float> dxo(mk + K, xout);  // [M + 1][K]: the last row is a guard the kernel must not write
    wt::DecGemmArgs g;
    g.bf16 = bf;
    g.Wt = dW.w(); g.w_scale = dW.scale; g.N = N; g.K = K; g.B = B; g.M = M;
    g.ln_g = dg.p; g.ln_b = db.p; g.xout = dxo.p;
    if (ids) {  // LNMODE 2: row p * B + b = tok_emb[ids[b][pos + p]] + pos_emb[pos + p]
      g.ids = dids.p; g.ids_stride = ids_stride; g.pos = pos; g.tok_emb = dtok.p; g.pos_emb = dpos.p; g.n_vocab = n_vocab;
    } else {    // LNMODE 0 (xin) or 3 (xin + xpart)
      g.xin = dxin.p; g.xpart = xpart ? dxp.p : nullptr;
    }
    g.bias = dB.p; g.Y = dY.p; g.ldy = N;
    wt::launch_dec_gemm(g, wt::kProLn, gelu ? wt::kDecBiasGelu : wt::kDecBias, h->impl->stream());
    h->impl->sync();
    dY.to_host(Y);
    dxo.to_host(xout);
  });
}

int wt_dbg_dec_logits(wt_engine* h, int bf16, int M, int V, int K, const float* xin, const float* xpart, const float* ln_g,
                      const float* ln_b, const float* E, int blocks, float* logits, uint64_t* records) {
  if (!h || !xin || !ln_g || !ln_b || !E || !records || M < 1 || M > 128 || V < 1 || blocks < 0 ||
      (K != 128 && K != 384 && K != 512)) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const bool bf = bf16 != 0;
    const int n_tiles = (V + 31) / 32;
    const DevTiled dE(E, V, K, bf);
    const size_t mk = size_t(M) * K;
    DevArr<float> dxin(mk, xin), dxp(xpart ? mk : 0, xpart), dg(K, ln_g), db(K, ln_b);
    // [M + 1][V] and [M + 1][n_tiles]: the last row of each is a guard the kernel must not write
    DevArr<float> dY(logits ? (size_t(M) + 1) * V : 0, logits);
    DevArr<unsigned long long> dBest((size_t(M) + 1) * n_tiles, reinterpret_cast<const unsigned long long*>(records));
    wt::DecGemmArgs g;  // the engine's final LayerNorm + logits + argmax records
    g.bf16 = bf;
    g.logits_blocks = blocks;
    g.Wt = dE.w(); g.w_scale = dE.scale; g.N = V; g.K = K; g.B = M; g.M = M;
    g.xin = dxin.p; g.xpart = xpart ? dxp.p : nullptr; g.ln_g = dg.p; g.ln_b = db.p;
    g.Y = logits ? dY.p : nullptr; g.ldy = V; g.best = dBest.p;
    wt::launch_dec_gemm(g, wt::kProLn, wt::kDecLogits, h->impl->stream());
    h->impl->sync();
    if (logits) dY.to_host(logits);
    dBest.to_host(reinterpret_cast<unsigned long long*>(records));
  });
}

int wt_dbg_select_token(wt_engine* h, int B, int n_tiles, const uint64_t* records, int64_t* ids, int stride, int pos,
                        int32_t* n_ids, int32_t* finished, int64_t eot, int stop_at_eot, int keep_ids) {
  if (!h || !records || !ids || !n_ids || !finished || B < 1 || n_tiles < 1 || pos < 0 || pos + 1 >= stride) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    DevArr<unsigned long long> dRec(size_t(B) * n_tiles, reinterpret_cast<const unsigned long long*>(records));
    DevArr<long long> dids(size_t(B) * stride, reinterpret_cast<const long long*>(ids));
    DevArr<int> dn(B, n_ids), dfin(B, finished);
    wt::launch_select_token(dRec.p, n_tiles, dids.p, stride, pos, dn.p, dfin.p, eot, stop_at_eot, B, h->impl->stream(),
                            keep_ids != 0);
    h->impl->sync();
    dids.to_host(reinterpret_cast<long long*>(ids));
    dn.to_host(n_ids);
    dfin.to_host(finished);
  });
}

int wt_dbg_timestamp_select(wt_engine* h, int B, int V, const float* logits, const int64_t* ids, int ids_stride,
                            const int32_t* n_ids, int sample_begin, int eot, int beg, int max_initial_timestamp,
                            int64_t* token, double* L, float* M) {
  if (!h || !logits || !ids || !n_ids || !token || B < 1 || B > 64 || V < 2 || ids_stride < 1 || sample_begin < 0) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    // every row decides the step behind ITS n_ids[b] ids; the kernels take one step count per launch, so runs of
    // consecutive rows with equal n_ids are launched together (a run's launch sees only its own rows: same grid-independent arithmetic)
    const int ldl = (V + 3) & ~3;
    for (int b = 0; b < B; ++b) {
      if (n_ids[b] < sample_begin || n_ids[b] > ids_stride) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_timestamp_select: n_ids outside [sample_begin, ids_stride]");
    }
    std::vector<float> padded(size_t(B) * ldl, 0.0f);
    for (int b = 0; b < B; ++b) std::memcpy(&padded[size_t(b) * ldl], logits + size_t(b) * V, size_t(V) * sizeof(float));
    // id rows with one more column: the kernel writes the token at ids[b][n_ids[b]]
    const int stride = ids_stride + 1;
    std::vector<long long> rows(size_t(B) * stride, 0);
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < n_ids[b]; ++i) rows[size_t(b) * stride + i] = ids[size_t(b) * ids_stride + i];
    DevArr<float> dlog(padded.size(), padded.data());
    DevArr<long long> dids(rows.size(), rows.data());
    DevArr<int> dn(B, n_ids), dfin(B);
    DevArr<wt::TsPart> dpart(size_t(B) * wt::ts_chunks(V));
    DevArr<wt::TsState> dstate(B);
    DevArr<double> dL(B);
    DevArr<float> dM(B);
    hipchk(hipMemsetAsync(dfin.p, 0, size_t(B) * sizeof(int), h->impl->stream()), "memset");
    wt::launch_ts_state_init(dids.p, stride, dn.p, 0, sample_begin, V, beg, dstate.p, B, h->impl->stream());
    for (int b0 = 0, b1 = 0; b0 < B; b0 = b1 + 1) {
      b1 = b0;  // the run of consecutive rows with n_ids[b0]
      while (b1 + 1 < B && n_ids[b1 + 1] == n_ids[b0]) ++b1;
      wt::TsSelectArgs t;
      t.logits = dlog.p + size_t(b0) * ldl; t.ldl = ldl; t.V = V; t.batch = b1 - b0 + 1;
      t.eot = eot; t.beg = beg; t.max_initial = max_initial_timestamp;
      t.n_gen = n_ids[b0] - sample_begin; t.part = dpart.p + size_t(b0) * wt::ts_chunks(V); t.state = dstate.p + b0;
      t.ids = dids.p + size_t(b0) * stride; t.ids_stride = stride; t.pos = n_ids[b0] - 1; t.stop_at_eot = 1;
      t.n_ids = dn.p + b0; t.finished = dfin.p + b0;
      t.dbg_L = dL.p + b0; t.dbg_M = dM.p + b0;
      wt::launch_ts_select(t, h->impl->stream());
    }
    h->impl->sync();
    dids.to_host(rows.data());
    for (int b = 0; b < B; ++b) token[b] = rows[size_t(b) * stride + n_ids[b]];
    if (L) dL.to_host(L);
    if (M) dM.to_host(M);
  });
}

int wt_dbg_sample_select(wt_engine* h, int B, int V, const float* logits, const int64_t* ids, int ids_stride,
                         const int32_t* n_ids, int sample_begin, int timestamps, int eot, int beg, int max_initial_timestamp,
                         const float* temperature, uint64_t seed, int attempt, int clip_base, int pos, int64_t* token,
                         double* L, float* M, float* key) {
  if (!h || !logits || !ids || !n_ids || !token || !temperature || B < 1 || B > wt::kSampleClipsMax || V < 2 ||
      ids_stride < 1 || sample_begin < 1 || attempt < 0 || clip_base < 0) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    // as wt_dbg_timestamp_select: runs of consecutive rows with equal n_ids are launched together
    const int ldl = (V + 3) & ~3;
    wt::SampleParams prm{};
    prm.seed_lo = unsigned(seed & 0xffffffffull), prm.seed_hi = unsigned(seed >> 32);
    prm.attempt = unsigned(attempt), prm.clip_base = unsigned(clip_base);
    for (int b = 0; b < B; ++b) {
      if (n_ids[b] < sample_begin || n_ids[b] > ids_stride) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_sample_select: n_ids outside [sample_begin, ids_stride]");
      if (!(temperature[b] >= 0.0f) || std::isinf(temperature[b])) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_sample_select: a temperature is negative or not finite");
      prm.inv_t[b] = temperature[b] > 0.0f ? 1.0f / temperature[b] : 0.0f;
    }
    std::vector<float> padded(size_t(B) * ldl, 0.0f);
    for (int b = 0; b < B; ++b) std::memcpy(&padded[size_t(b) * ldl], logits + size_t(b) * V, size_t(V) * sizeof(float));
    const int stride = ids_stride + 1;  // the kernel writes the token at ids[b][n_ids[b]]
    std::vector<long long> rows(size_t(B) * stride, 0);
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < n_ids[b]; ++i) rows[size_t(b) * stride + i] = ids[size_t(b) * ids_stride + i];
    DevArr<float> dlog(padded.size(), padded.data());
    DevArr<long long> dids(rows.size(), rows.data());
    DevArr<int> dn(B, n_ids), dfin(B);
    DevArr<wt::SamplePart> dpart(size_t(B) * wt::ts_chunks(V));
    DevArr<wt::TsState> dstate(B);
    DevArr<wt::SampleParams> dprm(1, &prm);
    DevArr<double> dL(B);
    DevArr<float> dM(B), dK(B);
    hipchk(hipMemsetAsync(dfin.p, 0, size_t(B) * sizeof(int), h->impl->stream()), "memset");
    if (timestamps) wt::launch_ts_state_init(dids.p, stride, dn.p, 0, sample_begin, V, beg, dstate.p, B, h->impl->stream());
    for (int b0 = 0, b1 = 0; b0 < B; b0 = b1 + 1) {
      b1 = b0;
      while (b1 + 1 < B && n_ids[b1 + 1] == n_ids[b0]) ++b1;
      wt::SampleArgs t;
      t.logits = dlog.p + size_t(b0) * ldl; t.ldl = ldl; t.V = V; t.batch = b1 - b0 + 1;
      t.eot = eot; t.beg = beg; t.max_initial = max_initial_timestamp;
      t.n_gen = n_ids[b0] - sample_begin; t.part = dpart.p + size_t(b0) * wt::ts_chunks(V);
      t.state = timestamps ? dstate.p + b0 : nullptr;
      t.params = dprm.p; t.row0 = b0; t.rng_pos = pos;
      t.ids = dids.p + size_t(b0) * stride; t.ids_stride = stride; t.pos = n_ids[b0] - 1; t.stop_at_eot = 1;
      t.n_ids = dn.p + b0; t.finished = dfin.p + b0;
      t.dbg_L = dL.p + b0; t.dbg_M = dM.p + b0; t.dbg_key = dK.p + b0;
      wt::launch_sample_select(t, h->impl->stream());
    }
    h->impl->sync();
    dids.to_host(rows.data());
    for (int b = 0; b < B; ++b) token[b] = rows[size_t(b) * stride + n_ids[b]];
    if (L) dL.to_host(L);
    if (M) dM.to_host(M);
    if (key) dK.to_host(key);
  });
}

int wt_dbg_token_scores(wt_engine* h, int B, int V, const float* logits, const int64_t* ids, int ids_stride,
                        const int32_t* n_ids, int sample_begin, int timestamps, int eot, int beg, int max_initial_timestamp,
                        const int32_t* live, float* lp, double* sum, int32_t* count, double* den) {
  if (!h || !logits || !ids || !n_ids || !live || !lp || !sum || !count || B < 1 || B > 64 || V < 2 || ids_stride < 1 ||
      sample_begin < 0) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const int ldl = (V + 3) & ~3;
    for (int b = 0; b < B; ++b) {
      if (n_ids[b] < sample_begin + 1 || n_ids[b] > ids_stride) throw wt::Error(WT_ERR_INVALID_ARG, "wt_dbg_token_scores: n_ids outside [sample_begin + 1, ids_stride]");
    }
    std::vector<float> padded(size_t(B) * ldl, 0.0f);
    for (int b = 0; b < B; ++b) std::memcpy(&padded[size_t(b) * ldl], logits + size_t(b) * V, size_t(V) * sizeof(float));
    // device rows are the caller's behind one more leading column, so that the chosen id (the last of the row) sits at
    // pos + 1 with pos = n_ids[b] - 1 >= 0 even when it is the only id
    const int stride = ids_stride + 1, sb = sample_begin + 1;
    std::vector<long long> rows(size_t(B) * stride, 0);
    std::vector<int> n_before(B), n_after(B);
    for (int b = 0; b < B; ++b) {
      for (int i = 0; i < n_ids[b]; ++i) rows[size_t(b) * stride + 1 + i] = ids[size_t(b) * ids_stride + i];
      n_before[b] = n_ids[b];                  // the device row's ids before the chosen one
      n_after[b] = live[b] ? n_ids[b] + 1 : 0;  // what the selection kernel leaves where the clip was live: pos + 2
    }
    DevArr<float> dlog(padded.size(), padded.data()), dlp(size_t(B) * stride);
    DevArr<long long> dids(rows.size(), rows.data());
    DevArr<int> dn0(B, n_before.data()), dn1(B, n_after.data()), dcount(B, count);
    DevArr<double> dsum(B, sum), dden(B);
    DevArr<wt::ScorePart> dpart(size_t(B) * wt::ts_chunks(V));
    DevArr<wt::TsState> dstate(B);
    hipStream_t st = h->impl->stream();
    hipchk(hipMemsetAsync(dlp.p, 0, size_t(B) * stride * sizeof(float), st), "memset");
    if (timestamps) wt::launch_ts_state_init(dids.p, stride, dn0.p, 0, sb, V, beg, dstate.p, B, st);
    for (int b0 = 0, b1 = 0; b0 < B; b0 = b1 + 1) {  // runs of consecutive rows with equal n_ids: one step count per launch
      b1 = b0;
      while (b1 + 1 < B && n_ids[b1 + 1] == n_ids[b0]) ++b1;
      wt::ScoreArgs a;
      a.logits = dlog.p + size_t(b0) * ldl; a.ldl = ldl; a.V = V; a.batch = b1 - b0 + 1;
      a.state = timestamps ? dstate.p + b0 : nullptr; a.eot = eot; a.beg = beg; a.max_initial = max_initial_timestamp;
      a.n_gen = n_ids[b0] - 1 - sample_begin; a.part = dpart.p + size_t(b0) * wt::ts_chunks(V);
      a.ids = dids.p + size_t(b0) * stride; a.ids_stride = stride; a.pos = n_ids[b0] - 1; a.n_ids = dn1.p + b0;
      a.token_logprob = dlp.p + size_t(b0) * stride; a.lp_stride = stride; a.sum = dsum.p + b0; a.count = dcount.p + b0;
      a.dbg_den = dden.p + b0;
      wt::launch_score_partial(a, st);
      wt::launch_score_finish(a, st);
    }
    h->impl->sync();
    std::vector<float> hlp(size_t(B) * stride);
    dlp.to_host(hlp.data());
    for (int b = 0; b < B; ++b) lp[b] = hlp[size_t(b) * stride + n_ids[b]];
    dsum.to_host(sum);
    dcount.to_host(count);
    if (den) dden.to_host(den);
  });
}

int wt_dbg_language_head(wt_engine* h, int rows, int d, int n_vocab, int lang_lo, int n_lang, int forced_lang, const float* x,
                         const float* xpart, const float* ln_g, const float* ln_b, const float* tok_emb, float* probs,
                         int32_t* lang, float* lang_prob, int64_t* ids, int ids_stride) {
  if (!h || !x || !ln_g || !ln_b || !tok_emb || !probs || !lang || !lang_prob || rows < 1 || rows > 128 || d < 1 ||
      d > wt::kLangMaxD || n_vocab < 1 || n_vocab > 4096 || lang_lo < 0 || n_lang < 1 || n_lang > wt::kLangMax ||
      lang_lo + n_lang > n_vocab || forced_lang >= n_lang || (ids && ids_stride < 2)) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t rd = size_t(rows) * d;
    DevArr<float> dx(rd, x), dxp(xpart ? rd : 0, xpart), dg(d, ln_g), db(d, ln_b), demb(size_t(n_vocab) * d, tok_emb);
    DevArr<float> dprobs(size_t(rows) * n_lang), dprob(rows);
    DevArr<int> dlang(rows);
    DevArr<long long> dids(ids ? size_t(rows) * ids_stride : 0, reinterpret_cast<const long long*>(ids));
    wt::LanguageHeadArgs a;
    a.x = dx.p; a.xpart = xpart ? dxp.p : nullptr; a.ln_g = dg.p; a.ln_b = db.p; a.tok_emb = demb.p;
    a.rows = rows; a.d = d; a.n_vocab = n_vocab; a.lang_lo = lang_lo; a.n_lang = n_lang;
    a.probs = dprobs.p; a.lang = dlang.p; a.lang_prob = dprob.p; a.forced_lang = forced_lang;
    if (ids) a.ids = dids.p, a.ids_stride = ids_stride, a.id_pos = 1;
    wt::launch_language_head(a, h->impl->stream());
    h->impl->sync();
    dprobs.to_host(probs);
    dprob.to_host(lang_prob);
    dlang.to_host(lang);
    if (ids) dids.to_host(reinterpret_cast<long long*>(ids));
  });
}

int wt_dbg_cross_absorbed_chain(wt_engine* h, int bf16, int batch, int heads, int T, int chunks, int nq, int split, int n_src,
                                const float* const* E_src, const float* qp, const float* wv, const float* bv, int mode,
                                int p0_only, int nq_only, float* out, float* ws) {
  if (!h || !wv || !bv || !out || !ws || batch < 1 || heads < 1 || heads > 8 || T < 1 || nq < 1 || chunks < 1 || chunks > 16 ||
      size_t(nq) * batch > 128 || mode < 0 || mode > 2) {
    return WT_ERR_INVALID_ARG;
  }
  if (mode != 2) {
    if (!qp || !E_src || n_src < 1 || n_src > 4 || split < 1 || split > batch || (n_src == 1 && split != batch)) return WT_ERR_INVALID_ARG;
    for (int i = 0; i < n_src; ++i)
      if (!E_src[i]) return WT_ERR_INVALID_ARG;
    // a single launch must stay inside the nq positions ws and qp were sized for
    if (mode == 1 && (p0_only < 0 || nq_only < 1 || p0_only + nq_only > nq)) return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const bool bf = bf16 != 0;
    const size_t d = size_t(heads) * 64, rows = size_t(nq) * batch, clip = size_t(T) * d;
    const std::vector<float> wvt = wt::cross_q_layout(wv, int(d));
    DevArr<float> dwv(wvt.size(), wvt.data()), dbv(d, bv), dq(mode != 2 ? rows * heads * d : 0, qp);
    // [rows + 1][...]: the last row of each is a guard the kernels must not write
    DevArr<float> dws((rows + 1) * heads * chunks * (d + 4), ws), dout((rows + 1) * d, out);
    hipStream_t st = h->impl->stream();
    // Every source is an allocation of its own with room for `batch` clips at ONE plane stride; the clips a group does
    // not have hold NaN halfs, so a wrong source or clip offset reads poison instead of some other clip's bytes.
    const size_t plane = size_t(batch) * clip + 64;
    std::vector<std::unique_ptr<DevArr<unsigned short>>> src;
    float se = 1.0f;
    if (mode != 2) {
      const auto clips_of = [&](int i) { return std::max(0, std::min(split, batch - i * split)); };
      float mx = 0.0f;
      for (int i = 0; i < n_src; ++i) mx = std::max(mx, max_abs(E_src[i], size_t(clips_of(i)) * clip));
      se = bf ? 1.0f : wt::f16_scale_for(mx);  // one scale for all sources, as the engine's sc_cross_kv_
      for (int i = 0; i < n_src; ++i) {
        const size_t n = size_t(clips_of(i)) * clip;
        std::vector<unsigned short> host((bf ? 1 : 2) * plane, bf ? 0x7FC0 : 0x7E00);
        for (size_t k = 0; k < n; ++k) {
          if (bf) {
            host[k] = DevBf16::rne(E_src[i][k]);
          } else {
            const float v = E_src[i][k] * se;
            const _Float16 hi = static_cast<_Float16>(v), lo = static_cast<_Float16>(v - static_cast<float>(hi));
            std::memcpy(&host[k], &hi, 2);
            std::memcpy(&host[plane + k], &lo, 2);
          }
        }
        src.push_back(std::make_unique<DevArr<unsigned short>>(host.size(), host.data()));
      }
      const int nq_max = wt::cross_absorbed_max_nq(heads);
      const auto launch = [&](int p0, int n) {
        wt::CrossAbsorbedArgs a;
        a.qp = dq.p; a.e = src[0]->p; a.e_plane = long(plane); a.e_scale = se; a.ws = dws.p; a.bf16 = bf;
        if (n_src > 1) {
          a.split = split;
          a.e2 = src[1]->p;
          if (n_src > 2) a.e3 = src[2]->p;
          if (n_src > 3) a.e4 = src[3]->p;
        }
        a.batch = batch; a.heads = heads; a.d_model = int(d); a.T = T; a.chunks = chunks; a.nq = n; a.p0 = p0;
        wt::launch_cross_absorbed(a, st);
      };
      if (mode == 1) {
        launch(p0_only, nq_only);
      } else {
        for (int p0 = 0; p0 < nq; p0 += nq_max) launch(p0, std::min(nq_max, nq - p0));  // Engine::decode's loop
      }
    }
    wt::launch_cross_absorbed_combine(dws.p, dwv.p, dbv.p, dout.p, int(rows), heads, chunks, int(d), st);
    h->impl->sync();
    dout.to_host(out);
    dws.to_host(ws);
  });
}

int wt_dbg_absorbed_query_matrix(int heads, int d, const float* wq, const float* bq, const float* wk, float* A, float* av) {
  if (heads < 1 || d != heads * 64 || !wq || !bq || !wk || !A || !av) return WT_ERR_INVALID_ARG;
  return guarded(nullptr, [&] {
    std::vector<float> Am, am;
    wt::absorbed_query_matrix(wq, bq, wk, heads, d, &Am, &am);
    std::memcpy(A, Am.data(), Am.size() * sizeof(float));
    std::memcpy(av, am.data(), am.size() * sizeof(float));
  });
}

// --- the log-mel front end, kernel by kernel (tests/test_gpu_frontend_kernels.py) ---

}  // extern "C"

namespace {
// a partial-maximum word of log_clipmax (order-preserving bits of a float; 0 = no block wrote it) -> the float
float clip_max_word_value(unsigned o) {
  if (o == 0u) return -std::numeric_limits<float>::infinity();
  const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// device words [(b * kClipMaxWays + w) * kClipMaxStride] -> words [B][kClipMaxWays] (+ their values)
void clip_max_to_host(const unsigned* d_words, int B, uint32_t* words, float* maxima) {
  std::vector<unsigned> host(size_t(B) * wt::kClipMaxWays * wt::kClipMaxStride);
  hipchk(hipMemcpy(host.data(), d_words, host.size() * sizeof(unsigned), hipMemcpyDeviceToHost), "D2H clip_max");
  for (size_t i = 0; i < size_t(B) * wt::kClipMaxWays; ++i) {
    if (words) words[i] = host[i * wt::kClipMaxStride];
    if (maxima) maxima[i] = clip_max_word_value(host[i * wt::kClipMaxStride]);
  }
}
float half_bits_to_float(unsigned short b) {
  _Float16 x;
  std::memcpy(&x, &b, 2);
  return static_cast<float>(x);
}
}  // namespace

extern "C" {

int wt_dbg_frontend_dims(wt_engine* h, int32_t out[8]) {
  if (!h || !out) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const wt::Engine& e = *h->impl;
    const wt::Engine::FrontendView v = e.frontend_view();
    if (v.dft_n == 0) throw wt::Error(WT_ERR_FORMAT, "vocab file carries no 80x201 mel filter bank");
    const int32_t d[8] = {e.mel_frames(), int32_t(e.pcm_elems()), int32_t(v.pcm_stride), v.pw_ld, v.mel_n, v.mel_k, v.dft_n, v.dft_k};
    std::memcpy(out, d, sizeof(d));
  });
}

int wt_dbg_frontend_stages(wt_engine* h, int batch, const float* pcm, int valid_frames, float* mel, float* planes,
                           uint16_t* hi, uint16_t* lo, float* pw, float* melacc, float* raw, uint32_t* words, float* maxima,
                           float* basis, float* mel_matrix) {
  if (!h || !pcm || !mel || batch < 1 || valid_frames < -1 || valid_frames > h->impl->mel_frames()) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    wt::Engine& e = *h->impl;
    e.require_idle();
    const size_t nb = size_t(batch), T0 = size_t(e.mel_frames());
    float* d_pcm = e.staging_pcm(batch);
    float* d_mel = e.staging_mel(batch);
    DevBuf d_raw(nb * e.mel_elems());
    hipchk(hipMemcpyAsync(d_pcm, pcm, nb * e.pcm_elems() * sizeof(float), hipMemcpyHostToDevice, e.stream()), "H2D pcm");
    e.logmel(d_pcm, batch, d_mel, valid_frames, d_raw.p);
    e.sync();
    const wt::Engine::FrontendView v = e.frontend_view();
    hipchk(hipMemcpy(mel, d_mel, nb * e.mel_elems() * sizeof(float), hipMemcpyDeviceToHost), "D2H mel");
    if (raw) d_raw.to_host(raw, nb * e.mel_elems());
    if (planes || hi || lo) {
      const size_t n = nb * size_t(v.pcm_stride);
      std::vector<unsigned short> hh(n), hl(n);
      hipchk(hipMemcpy(hh.data(), v.pcm_planes, n * 2, hipMemcpyDeviceToHost), "D2H pcm hi");
      hipchk(hipMemcpy(hl.data(), v.pcm_planes + v.pcm_plane, n * 2, hipMemcpyDeviceToHost), "D2H pcm lo");
      if (hi) std::memcpy(hi, hh.data(), n * 2);
      if (lo) std::memcpy(lo, hl.data(), n * 2);
      for (size_t i = 0; planes && i < n; ++i) planes[i] = (half_bits_to_float(hh[i]) + half_bits_to_float(hl[i])) / v.pcm_scale;
    }
    if (pw) hipchk(hipMemcpy(pw, v.pw, nb * T0 * size_t(v.pw_ld) * sizeof(float), hipMemcpyDeviceToHost), "D2H pw");
    if (melacc) hipchk(hipMemcpy(melacc, v.melacc, nb * T0 * size_t(v.mel_n) * sizeof(float), hipMemcpyDeviceToHost), "D2H melacc");
    if (words || maxima) clip_max_to_host(v.clip_max, batch, words, maxima);
    if (basis) std::memcpy(basis, v.basis, size_t(v.dft_n) * v.dft_k * sizeof(float));
    if (mel_matrix) std::memcpy(mel_matrix, v.mel_matrix, size_t(v.mel_n) * v.mel_k * sizeof(float));
  });
}

int wt_dbg_log_clipmax(wt_engine* h, int B, int T, int n_mel, int ld, int t_valid, const float* melacc, float* raw,
                       uint32_t* words, float* maxima) {
  if (!h || !melacc || !raw || B < 1 || T < 1 || n_mel < 1 || ld < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    DevArr<float> din(size_t(B) * T * ld, melacc), dout(size_t(B) * n_mel * T);
    DevArr<unsigned> dmax(size_t(B) * wt::kClipMaxWays * wt::kClipMaxStride);
    hipchk(hipMemsetAsync(dmax.p, 0, dmax.n * sizeof(unsigned), h->impl->stream()), "memset");  // as Engine::logmel clears them, on the launch's stream
    wt::launch_log_clipmax(din.p, ld, dout.p, dmax.p, B, n_mel, T, h->impl->stream(), t_valid);
    h->impl->sync();
    dout.to_host(raw);
    clip_max_to_host(dmax.p, B, words, maxima);
  });
}

int wt_dbg_mel_normalize(wt_engine* h, int B, int T, int n_mel, const uint32_t* words, float* logmel) {
  if (!h || !words || !logmel || B < 1 || T < 1 || n_mel < 1) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    DevArr<float> dx(size_t(B) * n_mel * T, logmel);
    std::vector<unsigned> host(size_t(B) * wt::kClipMaxWays * wt::kClipMaxStride, 0u);
    for (size_t i = 0; i < size_t(B) * wt::kClipMaxWays; ++i) host[i * wt::kClipMaxStride] = words[i];
    DevArr<unsigned> dmax(host.size(), host.data());
    wt::launch_mel_normalize(dx.p, dmax.p, B, n_mel, T, h->impl->stream());
    h->impl->sync();
    dx.to_host(logmel);
  });
}

int wt_dbg_mel_transpose(wt_engine* h, int planes, int B, int C, int T, int ld, float scale, const float* mel, void* out) {
  if (!h || !mel || !out || planes < 0 || planes > 2 || B < 1 || C < 1 || T < 1 || ld < 1 || (planes == 0 && ld != C)) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    const size_t n = size_t(B) * (size_t(T) + 2) * ld;
    DevArr<float> din(size_t(B) * C * T, mel);
    if (planes == 0) {
      DevArr<float> dout(n, static_cast<const float*>(out));
      wt::launch_mel_transpose(din.p, dout.p, B, C, T, h->impl->stream());
      h->impl->sync();
      dout.to_host(static_cast<float*>(out));
    } else {
      DevArr<unsigned short> dout(planes == 1 ? 2 * n : n, static_cast<const unsigned short*>(out));
      wt::launch_mel_transpose_planes(din.p, dout.p, planes == 1 ? long(n) : 0, planes == 1 ? scale : 1.0f, B, C, T, ld,
                                      h->impl->stream(), planes == 2);
      h->impl->sync();
      dout.to_host(static_cast<unsigned short*>(out));
    }
  });
}

int wt_dbg_pcm_to_planes(wt_engine* h, int batch, int n, int out_stride, int guard, float scale, float limit, const float* pcm,
                         uint16_t* planes) {
  if (!h || !pcm || !planes || batch < 1 || n < 1 || out_stride < 1 || guard < 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t plane = size_t(batch) * out_stride + guard;
    DevArr<float> din(size_t(batch) * n, pcm);
    DevArr<unsigned short> dout(2 * plane, planes);
    wt::launch_pcm_to_planes(din.p, dout.p, long(plane), scale, limit, batch, long(n), long(out_stride), h->impl->stream());
    h->impl->sync();
    dout.to_host(planes);
  });
}

}  // extern "C"

namespace {
// one past the last element that rows 0 .. M - 1 of `width` elements reach when row m starts at
// (m / rpb) * bs + (m % rpb) * ld: the last row, or the last row of the last whole group of rpb rows
long rows_extent(int M, int rpb, long bs, long ld, long width) {
  const long last = long((M - 1) / rpb) * bs + long((M - 1) % rpb) * ld;
  const long whole = M >= rpb ? long(M / rpb - 1) * bs + long(rpb - 1) * ld : 0;
  return std::max(last, whole) + width;
}
}  // namespace

extern "C" {

int wt_dbg_gemm_addressed(wt_engine* h, int kind, int epi, int M, int N, int K, const float* A, long a_len, int a_rpb,
                          long a_bs, int lda, const float* W, const float* bias, const float* pos, int pos_period,
                          int out_format, void* out, long c_len, long c_off, int c_rpb, long c_bs, int ldc,
                          const float* out_scale, int seg, int kv_batch, int kv_heads, int kv_dmodel, int n_cu) {
  if (!h || !A || !W || !out || kind < 0 || kind > 2 || M < 1 || N < 1 || K < 1 || a_rpb < 1 || a_bs < 0 || lda < 0 ||
      c_rpb < 1 || c_bs < 0 || ldc < 0 || c_off < 0 || c_len < 1 || n_cu < 0 || seg < 0 || ((epi & wt::kEpiBias) && !bias) ||
      ((epi & wt::kEpiPos) && (!pos || pos_period < 1)) || (out_format != 0 && out_format != kind) ||
      (out_format == 1 && !out_scale)) {
    return WT_ERR_INVALID_ARG;
  }
  // nothing is launched over operands or an output the buffers do not hold, or at an address the 16-byte accesses of
  // the kernels cannot take; what the launchers check themselves (rows per clip, multiples of 8, segments) is left to them
  if (a_len < rows_extent(M, a_rpb, a_bs, lda, K)) return WT_ERR_INVALID_ARG;
  const bool kv = (epi & wt::kEpiKvLayout) != 0;
  if (kv) {
    if (kv_batch < 1 || kv_heads < 1 || kv_dmodel != 64 * kv_heads || N % kv_dmodel != 0 || long(kv_batch) * c_rpb < M ||
        c_off + long(N / kv_dmodel) * kv_batch * kv_heads * c_rpb * 64 > c_len) {
      return WT_ERR_INVALID_ARG;
    }
  } else if (c_off + rows_extent(M, c_rpb, c_bs, ldc, N) > c_len) {
    return WT_ERR_INVALID_ARG;
  }
  const int align = out_format == 0 ? 4 : 8;
  if (c_off % align != 0 || (out_format == 1 && c_len % 8 != 0) ||
      (kind == 0 && (lda % 4 != 0 || a_bs % 4 != 0 || ldc % 4 != 0 || c_bs % 4 != 0))) {
    return WT_ERR_INVALID_ARG;
  }
  return guarded(h, [&] {
    DevBuf dB(bias, N), dP(pos, pos ? size_t(pos_period) * N : 0);
    hipStream_t st = h->impl->stream();
    if (kind == 0) {
      DevArr<float> dA(size_t(a_len) + 64), dC(size_t(c_len), static_cast<const float*>(out));
      // (cleared on the launch's own stream: it does not wait for the null stream, and hipMemset may return early)
      hipchk(hipMemsetAsync(dA.p + a_len, 0, 64 * sizeof(float), st), "memset");
      hipchk(hipMemcpy(dA.p, A, size_t(a_len) * sizeof(float), hipMemcpyHostToDevice), "H2D");
      DevBuf dW(W, size_t(N) * K);
      wt::GemmArgs g;
      g.A = dA.p; g.a_rpb = a_rpb; g.a_bs = a_bs; g.lda = lda; g.W = dW.p; g.bias = dB.p;
      g.C = dC.p + c_off; g.R = g.C; g.c_rpb = c_rpb; g.c_bs = c_bs; g.ldc = ldc;
      g.pos = dP.p; g.pos_period = pos_period > 0 ? pos_period : 1;
      g.kv_batch = kv_batch; g.kv_heads = kv_heads; g.kv_dmodel = kv_dmodel;
      g.M = M; g.N = N; g.K = K; g.variant = int(h->impl->gemm_variant);
      wt::launch_gemm(g, epi, st);
      h->impl->sync();
      dC.to_host(static_cast<float*>(out));
      return;
    }
    wt::PlaneGemmArgs g;
    g.a_rpb = a_rpb; g.a_bs = a_bs; g.lda = lda; g.bias = dB.p;
    g.c_rpb = c_rpb; g.c_bs = c_bs; g.ldc = ldc; g.pos = dP.p; g.pos_period = pos_period > 0 ? pos_period : 1;
    g.kv_batch = kv_batch; g.kv_heads = kv_heads; g.kv_dmodel = kv_dmodel;
    g.M = M; g.N = N; g.K = K; g.n_cu = n_cu;
    DevArr<float> dC(out_format == 0 ? size_t(c_len) : 0, static_cast<const float*>(out));
    DevArr<unsigned short> dO(out_format == 1 ? 2 * size_t(c_len) : out_format == 2 ? size_t(c_len) : 0,
                              static_cast<const unsigned short*>(out));
    if (out_format == 0) {
      g.C = dC.p + c_off; g.R = g.C;
    } else {
      g.P = dO.p + c_off; g.p_plane = c_len; g.seg = seg;
      if (out_format == 1) g.out_scale[0] = out_scale[0], g.out_scale[1] = out_scale[1], g.out_scale[2] = out_scale[2];
    }
    if (kind == 1) {
      const float sa = wt::f16_scale_for(max_abs(A, size_t(a_len))), sw = wt::f16_scale_for(max_abs(W, size_t(N) * K));
      const DevPlanes dA(A, size_t(a_len), sa);
      const DevWeightPlanes dW(W, N, K, sw);
      g.A = dA.ptr(); g.a_plane = dA.plane; g.W = dW.ptr(); g.a_scale = sa; g.w_scale = sw;
      wt::launch_gemm_planes(g, epi, st);
      h->impl->sync();
    } else {
      const DevBf16 dA(A, size_t(a_len)), dW(W, size_t(N) * K);
      g.A = dA.ptr(); g.W = dW.ptr();
      wt::launch_gemm_bf16_planes(g, epi, st);
      h->impl->sync();
    }
    if (out_format == 0) dC.to_host(static_cast<float*>(out)); else dO.to_host(static_cast<unsigned short*>(out));
  });
}

int wt_dbg_layernorm_planes(wt_engine* h, int M, int d, const float* x, const float* g, const float* b, float scale, int bf16,
                            int guard, uint16_t* planes, float* y32, int32_t* nonfinite) {
  if (!h || !x || !g || !b || !planes || M < 1 || d < 1 || guard < 0 || guard % 4 != 0 || !(scale > 0.0f)) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t plane = size_t(M) * d + guard;
    DevArr<float> dx(size_t(M) * d, x), dg(size_t(d), g), db(size_t(d), b), dy(y32 ? plane : 0, y32);
    DevArr<unsigned short> dout(bf16 ? plane : 2 * plane, planes);
    DevArr<int> dflag(1);
    // cleared on the launch's own stream, as the engine clears its flag: that stream does not wait for the null stream, on
    // which a hipMemset may still be pending when the kernel sets the word
    hipchk(hipMemsetAsync(dflag.p, 0, sizeof(int), h->impl->stream()), "memset");
    wt::launch_layernorm_planes(dx.p, dout.p, bf16 ? 0 : long(plane), scale, y32 ? dy.p : nullptr, dg.p, db.p, M, d,
                                h->impl->stream(), nonfinite ? dflag.p : nullptr, bf16 != 0);
    h->impl->sync();
    dout.to_host(planes);
    dy.to_host(y32);
    if (nonfinite) dflag.to_host(nonfinite);
  });
}

int wt_dbg_f32_to_planes(wt_engine* h, int M, int ld, const float* x, const float* scales, int seg, int guard,
                         uint16_t* planes) {
  if (!h || !x || !scales || !planes || M < 0 || ld < 1 || seg < 0 || guard < 0 || guard % 4 != 0) return WT_ERR_INVALID_ARG;
  return guarded(h, [&] {
    const size_t plane = size_t(M) * ld + guard;
    DevArr<float> dx(size_t(M) * ld, x);
    DevArr<unsigned short> dout(2 * plane, planes);
    wt::launch_f32_to_planes(dx.p, dout.p, long(plane), M, ld, scales, seg, h->impl->stream());
    h->impl->sync();
    dout.to_host(planes);
  });
}

int wt_dbg_encoder_attention_at(wt_engine* h, int kind, int variant, int batch, int T, int heads, int guard_rows,
                                const float* qkv, const float scales[4], void* out) {
  if (!h || !qkv || !out || kind < 0 || kind > 2 || guard_rows < 0 || batch < 0 || T < 0 || heads < 0 || (kind == 1 && !scales)) {
    return WT_ERR_INVALID_ARG;
  }
  if (kind == 1) {
    for (int i = 0; i < 4; ++i) {
      int e = 0;
      if (!(scales[i] > 0.0f) || !std::isfinite(scales[i]) || std::frexp(scales[i], &e) != 0.5f) return WT_ERR_INVALID_ARG;
    }
  }
  // batch, T or heads of zero, and a variant it does not have, are the launcher's to refuse: it throws before it launches,
  // and nothing is downloaded behind a throw
  return guarded(h, [&] {
    const size_t d = size_t(heads) * 64, rows = size_t(batch) * T + guard_rows, n_in = rows * 3 * d, n_out = rows * d;
    hipStream_t st = h->impl->stream();
    if (kind == 0) {
      const DevArr<float> dQ(n_in, qkv), dO(n_out, static_cast<const float*>(out));
      wt::launch_encoder_attention(dQ.p, dO.p, batch, T, heads, variant, st);
      h->impl->sync();
      dO.to_host(static_cast<float*>(out));
    } else if (kind == 1) {
      constexpr float kQ = 0.125f * 1.44269504088896340736f;
      // planes as the qkv GEMM's epilogue writes them: q * kQ * q_scale | k * k_scale | v * v_scale
      std::vector<float> scaled(n_in);
      for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < 3 * d; ++c)
          scaled[r * 3 * d + c] = qkv[r * 3 * d + c] * (c < d ? kQ * scales[0] : c < 2 * d ? scales[1] : scales[2]);
      const DevPlanes dQ(scaled.data(), n_in, 1.0f);
      const DevArr<unsigned short> dO(2 * n_out, static_cast<const unsigned short*>(out));
      wt::launch_encoder_attention_planes(dQ.ptr(), dQ.plane, dO.p, long(n_out), batch, T, heads, scales[0], scales[1],
                                          scales[2], scales[3], st);
      h->impl->sync();
      dO.to_host(static_cast<unsigned short*>(out));
    } else {
      const DevBf16 dQ(qkv, n_in);
      const DevArr<unsigned short> dO(n_out, static_cast<const unsigned short*>(out));
      wt::launch_encoder_attention_bf16(dQ.ptr(), dO.p, batch, T, heads, st);
      h->impl->sync();
      dO.to_host(static_cast<unsigned short*>(out));
    }
  });
}

}  // extern "C"
