// Engine, second part: full-length decoding (DESIGN sections 13 .. 28) — the checks and workspaces of a max_positions
// call, decode_full with its fall-back loop, the full-length beam and best-of chains, and the word alignment pass.
// The engine's life cycle, the encoder, the decoder pass and the 31-position chains are in engine.cpp.
#include <dlfcn.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "kernels.h"
#include "words.h"

namespace wt {

// ------------------------------------------------ full-length decoding ---

// option timestamps outside full-length decoding: every decode call is refused (with max_positions set, the refusals
// of check_full_call and of the other entry points apply as they are)
// (options scores and skip_silence live in the same scope and are refused here with it)
void Engine::check_timestamp_call() const {
  check_task_call();  // (every decode entry point passes here: see the note in engine.h)
  if (timestamps && max_positions <= 0) {
    throw Error(kErrUnsupported, "timestamps: full-length greedy decoding only, set the option max_positions (32 .. n_text_ctx)");
  }
  if (scores && max_positions <= 0) {
    throw Error(kErrUnsupported, "scores: full-length greedy decoding only, set the option max_positions (32 .. n_text_ctx)");
  }
  if (skip_silence && !scores) throw Error(kErrUnsupported, "skip_silence: needs the option scores = 1");
  if (sampling() && max_positions <= 0) {
    throw Error(kErrUnsupported, "temperature: full-length decoding only, set the option max_positions (32 .. n_text_ctx)");
  }
  if (seek && (!timestamps || max_positions <= 0)) {
    throw Error(kErrUnsupported, "seek: needs the options timestamps = 1 and max_positions (32 .. n_text_ctx)");
  }
  if (!context_ids.empty() && max_positions <= 0) {
    throw Error(kErrUnsupported, "context: full-length decoding only, set the option max_positions (32 .. n_text_ctx) or clear the context");
  }
  if (!clip_contexts.empty() && max_positions <= 0) {
    throw Error(kErrUnsupported, "contexts: full-length decoding only, set the option max_positions (32 .. n_text_ctx) or clear the contexts");
  }
  if (suppressing() && max_positions <= 0) {
    throw Error(kErrUnsupported, "suppress: full-length decoding only, set the option max_positions (32 .. n_text_ctx) or clear the lists");
  }
  if (!clip_contexts.empty() && word_timestamps) {
    throw Error(kErrUnsupported, "contexts: not with word_timestamps (the alignment pass takes one prompt length per call)");
  }
  check_word_call();
  if (temperature_fallback && !scores) throw Error(kErrUnsupported, "temperature_fallback: needs the option scores = 1");
  if (temperature_fallback && compression_ratio_threshold != 0 && !zlib_available()) {
    throw Error(kErrUnsupported, "compression_ratio_threshold: libz.so.1 could not be loaded; set the threshold to 0 (off)");
  }
}

void Engine::check_word_call() const {
  if (!word_timestamps) return;
  auto no = [](const char* why) { throw Error(kErrUnsupported, std::string("word_timestamps: ") + why); };
  if (!timestamps || max_positions <= 0) no("needs the options timestamps = 1 and max_positions (32 .. n_text_ctx)");
  if (!cross_absorb) no("needs the absorbed cross-attention (cross_absorb = 1)");
  if (!absorb_active()) no("the absorbed cross-attention is not available with these weights or this gemm_variant");
  if (vocab_.token_not < 0 || vocab_.token_not >= dims_.n_vocab) no("the model's vocabulary has no <|notimestamps|> id");
  if (dims_.n_audio_ctx % 4 != 0 || dims_.n_audio_ctx > kAlignFramesMax) no("n_audio_ctx must be a multiple of 4, at most 1500");
  if (alignment_heads.empty() && (dims_.n_text_layer - dims_.n_text_layer / 2) * dims_.n_text_head > kAlignHeadsMax) {
    no("the default of every head of the upper layers is more than 128 heads: set them with wt_engine_set_alignment_heads");
  }
}

void Engine::set_alignment_heads(const int32_t* layer_head, int n) {
  if (n < 0 || n > kAlignHeadsMax || (n > 0 && !layer_head)) throw Error(kErrInvalidArg, "alignment heads: 0 (the default) to 128 (layer, head) pairs");
  std::vector<std::pair<int, int>> v;
  for (int i = 0; i < n; ++i) {
    const std::pair<int, int> lh{layer_head[2 * i], layer_head[2 * i + 1]};
    if (lh.first < 0 || lh.first >= dims_.n_text_layer || lh.second < 0 || lh.second >= dims_.n_text_head) {
      throw Error(kErrInvalidArg, "alignment heads: a (layer, head) pair outside the model");
    }
    if (std::find(v.begin(), v.end(), lh) != v.end()) throw Error(kErrInvalidArg, "alignment heads: a pair is listed twice");
    v.push_back(lh);
  }
  alignment_heads = v;
}

std::vector<std::pair<int, int>> Engine::alignment_heads_in_effect() const {
  std::vector<std::pair<int, int>> v = alignment_heads;
  if (v.empty()) {
    for (int l = dims_.n_text_layer / 2; l < dims_.n_text_layer; ++l)
      for (int h = 0; h < dims_.n_text_head; ++h) v.emplace_back(l, h);
  }
  std::sort(v.begin(), v.end());
  return v;
}

// zlib through dlopen: no header and no link-time dependency a machine may lack
namespace {
struct Zlib {
  unsigned long (*bound)(unsigned long) = nullptr;
  int (*compress)(unsigned char*, unsigned long*, const unsigned char*, unsigned long) = nullptr;
  Zlib() {
    void* const lib = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!lib) return;
    bound = reinterpret_cast<decltype(bound)>(dlsym(lib, "compressBound"));
    compress = reinterpret_cast<decltype(compress)>(dlsym(lib, "compress"));
    if (!bound || !compress) bound = nullptr, compress = nullptr;
  }
};
const Zlib& zlib() {
  static const Zlib z;  // loaded at first use
  return z;
}
}  // namespace

bool Engine::zlib_available() { return zlib().compress != nullptr; }

double Engine::compression_ratio(const std::string& text) {
  if (text.empty()) return 0.0;
  const Zlib& z = zlib();
  if (!z.compress) throw Error(kErrUnsupported, "compression ratio: libz.so.1 could not be loaded");
  unsigned long n = z.bound(static_cast<unsigned long>(text.size()));
  std::vector<unsigned char> out(n);
  if (z.compress(out.data(), &n, reinterpret_cast<const unsigned char*>(text.data()), static_cast<unsigned long>(text.size())) != 0 || n == 0) {
    throw Error(kErrDevice, "compression ratio: zlib's compress() failed");
  }
  return double(text.size()) / double(n);
}

void Engine::check_full_args(int batch, int ids_stride) const {
  check_timestamp_call();
  if (max_positions <= 0) throw Error(kErrInvalidArg, "the full-length entry points need the option max_positions (32 .. n_text_ctx)");
  check_full_call();
  if (batch < 1 || batch > 64) throw Error(kErrInvalidArg, "decoder batches are limited to 64 clips per call");
  if (ids_stride < max_positions + 1) throw Error(kErrBuffer, "ids_stride is smaller than max_positions + 1");
  if (!clip_contexts.empty() && size_t(batch) != clip_contexts.size()) {
    throw Error(kErrInvalidArg, "contexts: the call's batch differs from the number of clips wt_engine_set_contexts was given");
  }
}

void Engine::check_full_call() const {
  if (max_positions <= 0) return;
  auto no = [](const char* why) { throw Error(kErrUnsupported, std::string("full-length decoding (max_positions): ") + why); };
  if (beam_size > 1 && !full_beam) no("greedy only, not with beam search (beam_size > 1) unless the option full_beam = 1 is set");
  if (bf16 && !full_bf16) no("not in the bf16 storage mode unless the option full_bf16 = 1 is set");
  if (bf16 && !full_bf16_all) {  // full_bf16 = 1 alone: what stays refused until full_bf16_all = 1 (DESIGN sections 33, 34)
    auto nf = [](const char* why) { throw Error(kErrUnsupported, std::string("full-length decoding in the bf16 storage mode (full_bf16): ") + why); };
    if (word_timestamps) nf("not with word_timestamps (the alignment pass reads the fp16 planes of the encoder output)");
    if (!clip_contexts.empty()) nf("not with per-clip contexts (the ragged self-attention kernels have no bf16 form)");
    if (language < 0) nf("not with automatic language detection (language = -1)");
  }
  if (language < 0 && !full_language) no("not with automatic language detection (language = -1)");
  if (!forced_ids.empty()) no("not with forced ids");
  if (language < 0) {  // full_language = 1: the scope of the automatic language behind max_positions
    auto nl = [](const char* why) { throw Error(kErrUnsupported, std::string("full-length automatic language (full_language): ") + why); };
    // (a Monolith engine or one without language tokens never gets here: set_language refuses -1 on them)
    if (!prompt_override.empty()) nl("not with a caller prompt (wt_engine_set_prompt)");
    if (!clip_lang_hold.empty() && clip_lang_hold.size() != clip_lang_hold_prob.size()) nl("the held languages and their probabilities differ in number");
  }
  if (beam_size > 1) {  // full_beam = 1: beam search's own scope, and what the beam chain does not run
    auto nb = [](const char* why) { throw Error(kErrUnsupported, std::string("full-length beam search (full_beam): ") + why); };
    check_beam_call(false, full_bf16 != 0);
    // (fallback_beam = 1: the beam chain is the fall-back's attempt at temperature 0; every other
    // refusal here and in check_beam_call holds for it as it stands)
    if (!fallback_beam && (sampling() || temperature_fallback)) nb("not with a temperature or the temperature fall-back");
    if (!context_ids.empty() || !clip_contexts.empty()) nb("not with a context");
    if (seek) nb("not with seek");
    if (word_timestamps) nb("not with word_timestamps");
  }
  if (best_of_sampling()) {  // the best-of chain's own scope
    auto nb = [](const char* why) { throw Error(kErrUnsupported, std::string("best_of: ") + why); };
    if (!context_ids.empty() || !clip_contexts.empty()) nb("not with a context");
    if (seek) nb("not with seek");
    if (word_timestamps) nb("not with word_timestamps");
    if (!stop_at_eot) nb("not with stop_at_eot = 0");
    if (!cross_absorb || !absorb_active()) nb("needs the absorbed cross-attention (cross_absorb = 1, weights and gemm_variant that allow it)");
    if (vocab_.token_eot < 0 || vocab_.token_eot >= dims_.n_vocab) nb("the model's vocabulary has no EOT id (token_eot >= n_vocab)");
  }
  // (a suppressed row is selected by ts_select or by the sampler's greedy step: both take an EOT inside the vocabulary)
  if (suppressing() && (vocab_.token_eot < 0 || vocab_.token_eot >= dims_.n_vocab)) no("suppress: the model's vocabulary has no EOT id (token_eot >= n_vocab)");
  if (timestamps && !has_timestamp_tokens()) no("timestamps: the model's vocabulary has no timestamp ids");
  if (scores && !has_no_speech_token()) no("scores: the model's vocabulary has no <|nospeech|> id");
  if (!context_ids.empty() && long(fed_prompt().size()) >= max_positions) {
    throw Error(kErrInvalidArg, "context: the prompt behind it leaves no position to generate (prompt ids >= max_positions)");
  }
  for (size_t b = 0; b < clip_contexts.size(); ++b) {
    if (long(fed_prompt_of(int(b)).size()) >= max_positions) {
      throw Error(kErrInvalidArg, "contexts: a clip's prompt leaves no position to generate (prompt ids >= max_positions)");
    }
  }
}

// A full-length call is synchronous and finds the engine idle, so it may choose its pipeline slot: always slot 0, and
// one set of segment graphs serves every call (a greedy call rotates over the slots and captures all of them at once).
// The rotation of the other calls goes on where it was.
void Engine::encode_full(const float* d_mel, int batch) {
  require_idle();
  check_full_call();
  const int next = enc_slot_;
  enc_slot_ = 0;
  try {
    encode(d_mel, batch);
  } catch (...) {
    enc_slot_ = next;
    throw;
  }
  enc_slot_ = next;
}

// The self-attention cache is sized by the largest batch a full-length call has had: layers x 2 x clips x cap x d
// floats (tiny: 5.5 MB per clip, 352 MB at 64 clips; large-v3's 32 layers of d = 1280: 147 MB per clip).  A larger
// batch frees it, and with it the segment graphs that hold its address.  Rows written by an earlier call, at whatever
// batch stride, are never read: the kernels read cache rows <= pos only, all written by the running chain.
void Engine::ensure_full_workspace(int batch) {
  const wtw::Dims& c = dims_;
  const size_t C = kFullClipsMax, cap = size_t(full_cap()), d = c.n_text_state;
  if (batch > fw_.kv_clips) {
    if (fw_.kv) {
      HIPCHK(hipStreamSynchronize(stream_));
      for (auto& ds : dstream_) HIPCHK(hipStreamSynchronize(ds));
      // every full-length segment graph, whatever its batch, holds the old cache's base address in its kernel
      // arguments: all of them go with it (greedy's and beam's graphs never see this cache and stay)
      for (auto it = graphs_.begin(); it != graphs_.end();) {
        if (it->first[0] == kFullKey) {
          (void)hipGraphExecDestroy(it->second.exec);
          it = graphs_.erase(it);
        } else {
          ++it;
        }
      }
      allocations_.erase(std::remove(allocations_.begin(), allocations_.end(), static_cast<void*>(fw_.kv)), allocations_.end());
      (void)hipFree(fw_.kv);
      fw_.kv = nullptr, fw_.kv_clips = 0;
    }
    fw_.kv = dev_zeroed<float>(size_t(c.n_text_layer) * 2 * size_t(batch) * cap * d);
    fw_.kv_clips = batch;
  }
  if ((timestamps || scores || sampling() || suppressing()) && !fw_.ts_logits) {  // the logits of a step: the timestamp rules, the scores and the suppression work on whole rows
    const size_t ldl = (size_t(c.n_vocab) + 3) & ~size_t(3);
    fw_.ts_ldl = int(ldl);
    fw_.ts_logits = dev_zeroed<float>(C * ldl);
  }
  if (timestamps && !fw_.ts_state) {  // (allocated last of the two)
    fw_.ts_part = dev_zeroed<TsPart>(C * size_t(ts_chunks(c.n_vocab)));
    fw_.ts_state = dev_zeroed<TsState>(C);
  }
  if (scores) {  // (every buffer is its own sentinel: a failed allocation leaves the earlier ones in place for the next call)
    if (!fw_.sc_part) fw_.sc_part = dev_zeroed<ScorePart>(C * size_t(ts_chunks(c.n_vocab)));
    if (!fw_.sc_lp) fw_.sc_lp = dev_zeroed<float>(C * (cap + 1));
    if (!fw_.sc_nosp) fw_.sc_nosp = dev_zeroed<float>(C);
    if (!fw_.sc_sum) fw_.sc_sum = dev_zeroed<double>(C);
    if (!fw_.sc_count) fw_.sc_count = dev_zeroed<int>(C);
    if (!fw_.h_lp) fw_.h_lp = pinned<float>(C * (cap + 1));
    if (!fw_.h_nosp) fw_.h_nosp = pinned<float>(C);
    if (!fw_.h_sum) fw_.h_sum = pinned<double>(C);
    if (!fw_.h_count) fw_.h_count = pinned<int>(C);
  }
  if (suppressing() && !timestamps && !sampling()) {  // the greedy step on the sampler's kernels (alloc clears: T = 0)
    if (!fw_.sm_part) fw_.sm_part = dev_zeroed<SamplePart>(C * size_t(ts_chunks(c.n_vocab)));
    if (!fw_.zero_prm) fw_.zero_prm = dev_zeroed<SampleParams>(1);
  }
  if (sampling()) {
    if (!fw_.sm_part) fw_.sm_part = dev_zeroed<SamplePart>(C * size_t(ts_chunks(c.n_vocab)));
    if (!fw_.sm_prm) fw_.sm_prm = dev_zeroed<SampleParams>(1);
    if (!fw_.h_prm) fw_.h_prm = pinned<SampleParams>(1);
  }
  if (fw_.h_fin) return;  // (allocated last)
  fw_.ids = dev_zeroed<long long>(C * (cap + 1));
  fw_.h_ids = pinned<long long>(C * (cap + 1));
  fw_.h_n = pinned<int>(C);
  fw_.h_fin = pinned<int>(C);
}

void Engine::ensure_ragged_workspace() {
  const size_t C = kFullClipsMax, S = size_t(ragged_stride());
  if (!rw_.ids) rw_.ids = dev_zeroed<long long>(C * S);
  if (!rw_.h_ids) rw_.h_ids = pinned<long long>(C * S);
  if (!rw_.start) rw_.start = dev_zeroed<int>(C);
  if (!rw_.h_start) rw_.h_start = pinned<int>(C);
  if (scores) {
    if (!rw_.lp) rw_.lp = dev_zeroed<float>(C * S);
    if (!rw_.h_lp) rw_.h_lp = pinned<float>(C * S);
  }
}

void Engine::enqueue_suppress(float* logits, int ldl, int rows, bool first, hipStream_t st) {
  SuppressArgs u;
  u.logits = logits; u.ldl = ldl; u.V = dims_.n_vocab; u.rows = rows; u.ids = d_suppress_;
  u.n = int(suppress_ids.size()); u.n_first = int(suppress_first_ids.size()); u.first = first;  // launch constants; the ids are device data
  launch_suppress_logits(u, st);
}

namespace {
// avg_logprob as every consumer sees it, rounded to float once.  Every live clip generates at least one id
// (max_positions > the prompt): a count of 0 is a device-side error.
float avg_logprob(double sum, int count) {
  if (count < 1) throw Error(kErrDevice, "scores: a clip came back with no generated id counted");
  return float(sum / double(count));
}
}  // namespace

bool Engine::silent(float no_speech_prob, float avg_lp, bool below) const {
  const double avg = double(avg_lp), thr = double(logprob_threshold) / 1000.0;
  return double(no_speech_prob) > double(no_speech_threshold) / 1000.0 && (below ? avg < thr : !(avg > thr));
}

void Engine::publish_full(const FullResult& r, int batch, int64_t* ids, int ids_stride, int32_t* n_ids) {
  const bool ts = timestamps != 0, sc = scores != 0;
  const int stride = r.stride, out_stride = full_cap() + 1;
  if (sc) {
    last.scores.assign(size_t(batch), ClipScore{});
    last.lp_stride = out_stride;
    last.token_logprob.assign(size_t(batch) * out_stride, 0.0f);
    for (int b = 0; b < batch; ++b) {
      ClipScore& s = last.scores[size_t(b)];
      s.avg_logprob = avg_logprob(r.sum[b], r.count[b]);
      s.n_generated = r.count[b];
      s.sum_logprob = float(r.sum[b]);
      s.no_speech_prob = r.nosp[b];
      // Whisper's rule: silence unless the text itself is confident
      s.skipped = skip_silence && silent(s.no_speech_prob, s.avg_logprob, false);
      for (int i = r.n_prompt(b); i < std::min(r.n[b], out_stride); ++i) {
        last.token_logprob[size_t(b) * out_stride + i] = r.lp[size_t(b) * stride + i];
      }
    }
    last.segment_score.clear();
    last.scores_valid = true;
  }
  for (int b = 0; b < batch; ++b) {
    n_ids[b] = r.n[b];
    for (int i = 0; i < ids_stride; ++i) {
      ids[size_t(b) * ids_stride + i] = i < r.n[b] && i < stride ? r.ids[size_t(b) * stride + i] : 0;
    }
  }
  if (ts) {
    last.segments.clear();
    last.segment_text.clear();
    for (int b = 0; b < batch; ++b) {
      if (sc && last.scores[size_t(b)].skipped) continue;  // a silent clip has no segments
      const int64_t* const row = reinterpret_cast<const int64_t*>(r.ids + size_t(b) * stride);
      const size_t first = last.segments.size();
      parse_segments(vocab_, row, std::min(r.n[b], stride), r.n_prompt(b), b, &last.segments);
      for (size_t i = first; i < last.segments.size(); ++i) {
        bool missing = false;
        last.segment_text.push_back(decode_tokens(vocab_, row + last.segments[i].id_begin, last.segments[i].id_count, false, &missing));
        if (sc) {  // the mean log-probability of the segment's text ids
          double sum = 0.0;
          for (int k = 0; k < last.segments[i].id_count; ++k) sum += double(r.lp[size_t(b) * stride + last.segments[i].id_begin + k]);
          last.segment_score.push_back(float(sum / double(std::max(last.segments[i].id_count, 1))));
        }
      }
    }
    last.segments_valid = true;
  }
}

// Full-length greedy decoding: decode_enqueue's passes — the prompt grouped by np_max, then one
// pass per position — continued to P = max_positions, over a self-attention cache of full_cap() rows and id rows of
// stride full_cap() + 1.  Positions 0 .. 31 run self_attention_step on that cache, later ones self_attention_long; the
// cross-attention form is the one the slot's encoder pass prepared.  The chain is enqueued in segments of 32 positions;
// a segment's launch sequence is fixed for its key and replayed from a hipGraph of the calling slot.  After each
// segment the finished flags come back, and the chain ends once every clip has emitted EOT (stop_at_eot = 1).
void Engine::decode_full(int batch, int64_t* ids, int ids_stride, int32_t* n_ids, const std::vector<long long>* valid_samples) {
  require_idle();
  check_full_args(batch, ids_stride);
  const int P = int(max_positions), slot_idx = last_enc_slot_;
  last.forget(kForgetFullDecode);
  // (full_beam = 1: check_full_call; fallback_beam = 1 with a temperature: the beam chain is the attempt at 0 below)
  const bool bfb = beam_fallback();
  // option full_language: clip b's prompt language is hold[b] when the long loop holds one, else it is
  // detected: off the chain's own position-0 pass, or behind a context off one pass over [sot] in front of the chain.
  // The chains that carry several rows per clip — beam search and best_of — take their prompts from the host: for them
  // one detect_language pass runs first, and every hypothesis, sample and attempt of a clip carries the clip's language.
  const bool autol = auto_full();
  std::vector<int> hold(size_t(batch), -1);
  std::vector<float> hold_prob(size_t(batch), 0.0f);
  if (autol && !clip_lang_hold.empty()) {
    if (clip_lang_hold.size() != size_t(batch)) throw Error(kErrInvalidArg, "full_language: the held languages are for another number of clips");
    for (int b = 0; b < batch; ++b) {
      hold[size_t(b)] = std::min(clip_lang_hold[size_t(b)], lang_tokens() - 1);
      hold_prob[size_t(b)] = clip_lang_hold_prob[size_t(b)];
    }
  }
  auto undetected = [&] { return autol && std::any_of(hold.begin(), hold.end(), [](int h) { return h < 0; }); };
  if (undetected() && (beam_size > 1 || best_of_sampling())) {
    std::vector<int32_t> dl(static_cast<size_t>(batch), 0);
    std::vector<float> dp(static_cast<size_t>(batch), 0.0f);
    detect_language(batch, dl.data(), nullptr, dp.data());
    for (int b = 0; b < batch; ++b) {
      if (hold[size_t(b)] < 0) hold[size_t(b)] = dl[size_t(b)], hold_prob[size_t(b)] = dp[size_t(b)];
    }
  }
  const bool det = undetected();
  call_lang_ = autol ? hold : std::vector<int>();  // (a detecting chain fills the open entries once it has run)
  auto publish_languages = [&] {  // per clip the language it was decoded behind: detected by the chain (the pinned mirrors), or held
    if (!autol) return;
    last.lang.assign(size_t(batch), 0);
    last.lang_prob.assign(size_t(batch), 0.0f);
    for (int b = 0; b < batch; ++b) {
      last.lang[size_t(b)] = call_lang_[size_t(b)] = hold[size_t(b)] >= 0 ? hold[size_t(b)] : h_lang_[b];
      last.lang_prob[size_t(b)] = hold[size_t(b)] >= 0 ? hold_prob[size_t(b)] : h_lang_prob_[b];
    }
    last.lang_valid = true;
  };
  if (beam_size > 1 && !bfb) {
    decode_beam_full(batch, ids, ids_stride, n_ids);
    return publish_languages();
  }
  const bool ts = timestamps != 0, sc = scores != 0, smp = sampling(), sup = suppressing();
  const int n_sup = int(suppress_ids.size()), n_sup_first = int(suppress_first_ids.size());
  ensure_batch(batch);
  ensure_full_workspace(batch);  // (before any capture: nothing may be allocated inside one)
  const bool bo = best_of_sampling();  // attempts above temperature 0 decode best_of samples per clip
  if (bo) {
    if (!slots_[slot_idx].absorbed) throw Error(kErrUnsupported, "best_of: the encoder pass did not prepare the absorbed cross-attention");
    ensure_best_of_workspace();
  }
  if (bfb) ensure_beam_full_workspace();
  // per-clip contexts (set_contexts): the chain runs in slots, the fed prompts right-aligned so that
  // every clip's prompt ends at slot n_prompt - 1; `stride`, `n_prompt`, `sot_idx` and the chain's length are in slots,
  // and the rows come back to the caller's layout when the chain has ended (run_chain)
  const bool rag = !clip_contexts.empty();
  if (rag) ensure_ragged_workspace();
  if (det) ensure_full_language_workspace();  // (before any capture)
  Slot& slot = slots_[slot_idx];
  const int V = dims_.n_vocab, cap = full_cap(), stride = rag ? ragged_stride() : cap + 1;
  // with a context (set_context): [prev] + context + prompt(), every count below starts behind all of it
  const bool ctx = !context_ids.empty() || rag;
  const std::vector<long long> prompt = fed_prompt();
  std::vector<std::vector<long long>> prompts;  // ragged: the clips' fed prompts
  int n_prompt = int(prompt.size()), n_min = n_prompt;
  if (rag) {
    n_prompt = 0, n_min = 1 << 30;
    for (int b = 0; b < batch; ++b) {
      prompts.push_back(fed_prompt_of(b));
      check_prompt_ids(prompts.back(), kErrInvalidArg);
      n_prompt = std::max(n_prompt, int(prompts.back().size()));
      n_min = std::min(n_min, int(prompts.back().size()));
    }
    for (int b = 0; b < batch; ++b) rw_.h_start[b] = n_prompt - int(prompts[size_t(b)].size());
  }
  auto np_of = [&](int b) { return rag ? int(prompts[size_t(b)].size()) : n_prompt; };  // clip b's fed prompt, in Whisper terms
  // Whisper's sot_index: the no-speech logits are read there
  const int sot_idx = rag ? n_prompt - int(this->prompt().size()) : !context_ids.empty() ? 1 + int(context_ids.size()) : 0;
  const int PS = rag ? n_prompt - n_min + P : P;  // the chain's length: the clip behind the shortest prompt reaches its cap last
  long long* const d_ids = rag ? rw_.ids : fw_.ids;
  long long* const h_ids = rag ? rw_.h_ids : fw_.h_ids;
  float* const d_lp = rag ? rw_.lp : fw_.sc_lp;
  float* const h_lp = rag ? rw_.h_lp : fw_.h_lp;
  check_prompt_ids(prompt, kErrInvalidArg);
  slot.dec = slot_idx % n_dec_streams_;
  slot.pair_leader = -1;
  DecWorkspace& dw = dws_[slot.dec];
  hipStream_t const st = dec_stream_at(slot.dec);
  const int chunks = cross_chunks_for(batch);  // as decode_enqueue chooses them for a synchronous call of this size
  const bool absorbed = slot.absorbed;
  const int n_abs = abs_chunks_for(batch, 256);
  // prompt positions per pass: four without a context (self_attention_step's launch), as many rows as a pass takes
  // with one (self_attention_prefill); option prompt_group = 1: one position per pass, the A/B handle
  const int np_max = ctx ? (prompt_group == 1 ? 1 : std::max(1, kDecRowsMax / batch)) : std::max(1, std::min(4, kDecRowsMax / batch));
  const int prompt_end = std::min(n_prompt, PS);
  // (a context's length is part of every launch: such calls run eagerly, DESIGN section 20 — run_chain)

  DecPass p;
  p.B = p.clips = batch; p.ids = d_ids; p.ids_stride = stride; p.self_kv = fw_.kv; p.self_cap = cap;
  if (rag) p.pos_start = rw_.start, p.pos_limit = P;
  p.absorbed = absorbed; p.n_abs = n_abs; p.chunks = chunks; p.e = slot.e_planes; p.cross_kv = slot.cross_kv;
  p.split = fc2_split(); p.dw = &dw; p.ldy = V;
  p.bf = bf16 != 0;  // option full_bf16: bf16 weights and operands, and fw_.kv holds bf16 rows (the first half of it)
  // the timestamp rules, the scores and the sampler read the whole row, the suppression writes into it
  if (ts || sc || smp || sup) p.Y = fw_.ts_logits, p.ldy = fw_.ts_ldl;
  ScoreArgs sa;
  if (sc) {
    fill_rule_args(sa, fw_.ts_logits, fw_.ts_ldl);
    sa.batch = batch; sa.part = fw_.sc_part;
    sa.ids = d_ids; sa.ids_stride = stride; sa.n_ids = dw.n_ids; sa.token_logprob = d_lp; sa.lp_stride = stride;
    sa.sum = fw_.sc_sum; sa.count = fw_.sc_count;
  }
  // the passes whose first position lies in [lo, hi); returns the argmax steps among them
  auto enqueue_segment = [&](int lo, int hi) {
    int seg_steps = 0;
    for (int pos0 = 0, np = 1; pos0 < hi; pos0 += np) {
      np = pos0 < prompt_end ? std::min(np_max, prompt_end - pos0) : 1;
      if (sc && pos0 <= sot_idx) np = std::min(np, sot_idx - pos0 + 1);  // a pass ends at sot, with logits: the no-speech probability
      if (det && !ctx && pos0 == 0) np = 1;  // the language is read off position 0 before position 1 can be embedded
      if (pos0 < lo) continue;
      const int last = pos0 + np - 1;
      const bool logits = last >= n_prompt - 1;  // then the token of the last position's rows
      const bool nosp = sc && last == sot_idx;
      p.pos0 = pos0; p.np = np; p.best = logits || nosp ? dw.best : nullptr;
      p.self_prefill = ctx && pos0 < prompt_end;  // the prompt behind a context, whatever np is
      // (np == 1 there: a prompt without a context has at most 8 ids; the ragged chain has no step form)
      p.self_long = !p.self_prefill && (rag || pos0 + np > 32);
      decoder_pass(p, st);
      if (nosp) {
        sa.state = nullptr;
        launch_no_speech_prob(sa, vocab_.token_solm, fw_.sc_nosp, st);
      }
      // position 0's residual rows -> ids[b][1], before any pass embeds position 1 (the logits GEMM leaves them as they are)
      if (det && !ctx && pos0 == 0) enqueue_full_language(dw, slot.dec, p.split, batch, d_ids, stride, 1, st);
      if (logits) {
        // Whisper's SuppressTokens / SuppressBlank, behind the no-speech probability and in front of every rule
        if (sup) enqueue_suppress(fw_.ts_logits, fw_.ts_ldl, batch, last + 1 - n_prompt == 0, st);
        if (sc) {  // the partial sums of the allowed set, from the state BEFORE the selection advances it
          sa.state = ts ? fw_.ts_state : nullptr; sa.n_gen = last + 1 - n_prompt; sa.pos = last;
          launch_score_partial(sa, st);
        }
        // a sample at the temperature the parameter block holds (0: the greedy step), in both modes; a suppressed row
        // without timestamps takes the same kernels under the block of zeros: the fused argmax records of the logits
        // GEMM were formed before the filter, and T = 0 here is select_token's rule (larger logit, then larger id)
        if (smp || (sup && !ts)) {
          SampleArgs t;
          fill_rule_args(t, fw_.ts_logits, fw_.ts_ldl);
          t.batch = batch; t.n_gen = last + 1 - n_prompt; t.params = smp ? fw_.sm_prm : fw_.zero_prm; t.part = fw_.sm_part;
          t.state = ts ? fw_.ts_state : nullptr;
          t.ids = d_ids; t.ids_stride = stride; t.pos = last; t.stop_at_eot = int(stop_at_eot);
          t.n_ids = dw.n_ids; t.finished = dw.finished;
          launch_sample_select(t, st);
        } else if (ts) {
          TsSelectArgs t;
          fill_rule_args(t, fw_.ts_logits, fw_.ts_ldl);
          t.batch = batch; t.n_gen = last + 1 - n_prompt; t.part = fw_.ts_part; t.state = fw_.ts_state;
          t.ids = d_ids; t.ids_stride = stride; t.pos = last; t.stop_at_eot = int(stop_at_eot);
          t.n_ids = dw.n_ids; t.finished = dw.finished;
          launch_ts_select(t, st);
        } else {
          launch_select_token(dw.best, (V + 31) / 32, d_ids, stride, last, dw.n_ids, dw.finished, vocab_.token_eot,
                              int(stop_at_eot), batch, st);
        }
        if (sc) launch_score_finish(sa, st);
        if (rag) launch_ragged_cap(rw_.start, last, P, dw.finished, batch, st);  // a clip that has fed its position P - 1 stops counting
        ++seg_steps;
      }
    }
    return seg_steps;
  };

  // One decoder chain over the slot's encoder output; the results come back in the pinned mirrors fw_.h_*.
  // frozen (sampling only): clips that start with finished = 1 — accepted by an earlier attempt — so that the chain
  // ends when the others end; their device rows are overwritten and their counts stay at zero.
  int steps = 0;
  auto run_chain = [&](const std::vector<int>* frozen, bool first) {
    for (int b = 0; b < batch; ++b) {
      for (int i = 0; i < stride; ++i) {
        if (rag) {  // right-aligned: slots in front of the clip's prompt hold id 0 and are void
          const int k = i - rw_.h_start[b];
          h_ids[size_t(b) * stride + i] = k >= 0 && i < n_prompt ? prompts[size_t(b)][size_t(k)] : 0;
        } else {
          h_ids[size_t(b) * stride + i] = i < n_prompt ? prompt[i] : 0;
        }
      }
      fw_.h_n[b] = n_prompt;
      // (behind sot, at the same slot for every clip: the held language, or a placeholder the device overwrites)
      if (autol) h_ids[size_t(b) * stride + sot_idx + 1] = kLangLo + std::max(hold[size_t(b)], 0);
      if (det) fl_.h_hold[b] = hold[size_t(b)];
    }
    HIPCHK(hipStreamWaitEvent(st, slot.enc_done, 0));
    if (first) HIPCHK(hipEventRecord(slot.dec_begin, st));
    HIPCHK(hipMemcpyAsync(d_ids, h_ids, size_t(batch) * stride * sizeof(long long), hipMemcpyHostToDevice, st));
    if (rag) HIPCHK(hipMemcpyAsync(rw_.start, rw_.h_start, size_t(batch) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dw.n_ids, fw_.h_n, size_t(batch) * sizeof(int), hipMemcpyHostToDevice, st));
    if (frozen) {
      for (int b = 0; b < batch; ++b) fw_.h_fin[b] = (*frozen)[size_t(b)];
      HIPCHK(hipMemcpyAsync(dw.finished, fw_.h_fin, size_t(batch) * sizeof(int), hipMemcpyHostToDevice, st));
    } else {
      HIPCHK(hipMemsetAsync(dw.finished, 0, size_t(batch) * sizeof(int), st));
    }
    if (smp) HIPCHK(hipMemcpyAsync(fw_.sm_prm, fw_.h_prm, sizeof(SampleParams), hipMemcpyHostToDevice, st));
    if (det) HIPCHK(hipMemcpyAsync(fl_.hold, fl_.h_hold, size_t(batch) * sizeof(int), hipMemcpyHostToDevice, st));
    if (det && ctx) {
      // one pass over [sot] at position 0 for all clips, as detect_language runs it, and the language into the slot
      // behind sot.  It leaves row 0 of every clip's self-attention cache behind; the chain reads cache rows only
      // after writing them itself (ensure_full_workspace), so nothing of this pass reaches it.
      DecPass q = p;
      q.ids = fl_.sot_ids; q.ids_stride = 1; q.pos0 = 0; q.np = 1; q.best = nullptr;
      q.self_prefill = q.self_long = false; q.pos_start = nullptr; q.pos_limit = 0;
      decoder_pass(q, st);
      enqueue_full_language(dw, slot.dec, p.split, batch, d_ids, stride, sot_idx + 1, st);
    }
    if (ts) {  // the carried state of the timestamp rules: nothing generated yet
      launch_ts_state_init(d_ids, stride, nullptr, n_prompt, n_prompt, V, vocab_.token_beg, fw_.ts_state, batch, st);
    }
    if (sc) {  // the carried sums and counts of the scores: nothing generated yet
      HIPCHK(hipMemsetAsync(fw_.sc_sum, 0, size_t(batch) * sizeof(double), st));
      HIPCHK(hipMemsetAsync(fw_.sc_count, 0, size_t(batch) * sizeof(int), st));
    }
    // (greedy's keys start with the slot, a beam key with -beam_size; a full-length key starts with kFullKey)
    // (the sampling kernels are one entry; temperature, seed and attempt are data, never part of the key)
    auto key_of = [&](int lo) {
      std::vector<long long> key{kFullKey, slot_idx, batch, lo, P, n_prompt, chunks, long(stop_at_eot), fc2_ksplit,
                                 absorbed ? 1 : 0, n_abs, slot.dec, ts ? 1 : 0, ts ? max_initial_timestamp : 0, sc ? 1 : 0,
                                 smp ? 1 : 0};
      if (sup) key.push_back(n_sup), key.push_back(n_sup_first);  // launch constants; the ids themselves are device data
      // (one entry more, where suppression adds two: the detecting chain, under a candidate list or not; the mask, the
      // held languages and the languages themselves are device data)
      if (det) key.push_back(language_candidates.empty() ? 1 : 2);
      // (last, and in the bf16 storage mode only: the fp32 keys stay what they were, and no entry above is negative)
      if (p.bf) key.push_back(kBf16KeyMark);
      return key;
    };
    // every clip finished (ragged: or capped): the chain ends behind that segment
    const DonePoll poll = stop_at_eot || rag ? DonePoll{dw.finished, batch, fw_.h_fin} : DonePoll{};
    run_segments(PS, st, !ctx, "full-length", key_of, enqueue_segment, poll, steps);
    HIPCHK(hipMemcpyAsync(h_ids, d_ids, size_t(batch) * stride * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(fw_.h_n, dw.n_ids, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, st));
    if (sc) {  // the scores come down with the ids: no further synchronisation point
      HIPCHK(hipMemcpyAsync(h_lp, d_lp, size_t(batch) * stride * sizeof(float), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(fw_.h_sum, fw_.sc_sum, size_t(batch) * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(fw_.h_count, fw_.sc_count, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(fw_.h_nosp, fw_.sc_nosp, size_t(batch) * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipEventRecord(slot.dec_done, st));
    slot.steps = steps;  // (summed over the attempts)
    finish_slot(slot_idx);  // waits; the encoder's non-finite flag, timings
    if (rag) {  // back to the caller's layout: row b starts at its own prompt, counts in Whisper terms
      for (int b = 0; b < batch; ++b) {
        const int s0 = rw_.h_start[b];
        long long* const r = h_ids + size_t(b) * stride;
        std::copy(r + s0, r + stride, r);
        std::fill(r + (stride - s0), r + stride, 0ll);
        if (sc) {
          float* const q = h_lp + size_t(b) * stride;
          std::copy(q + s0, q + stride, q);
          std::fill(q + (stride - s0), q + stride, 0.0f);
        }
        fw_.h_n[b] -= s0;
      }
    }
  };

  if (!smp) {
    run_chain(nullptr, true);
  } else {
    // Whisper's decode_with_fallback: the schedule's temperatures in turn, every attempt over the clips that still
    // need one; the host keeps what a clip was accepted with and puts the merged result back into the mirrors
    std::vector<long> temps{temperature};
    if (temperature_fallback) {
      for (long t = temperature + temperature_increment; t <= 1000; t += temperature_increment) temps.push_back(t);
    }
    std::vector<int> frozen(size_t(batch), 0);
    std::vector<long long> m_ids(size_t(batch) * stride, 0);
    std::vector<int> m_n(size_t(batch), 0), m_count(size_t(batch), 0);
    std::vector<float> m_lp(sc ? size_t(batch) * stride : 0, 0.0f), m_nosp(size_t(batch), 0.0f);
    std::vector<double> m_sum(size_t(batch), 0.0);
    // best_of: the kept sample and every sample's sum and count, from the attempt a clip was kept with
    const size_t G = kSampleGroupMax;
    std::vector<int32_t> m_picked(size_t(batch), 0), m_bo_count(bo ? size_t(batch) * G : 0, 0);
    std::vector<double> m_bo_sum(bo ? size_t(batch) * G : 0, 0.0);
    bool any_wide = false;
    last.decode_info.assign(size_t(batch), ClipDecode{0, 0, 0, 0.0f});
    for (size_t attempt = 0; attempt < temps.size(); ++attempt) {
      SampleParams& prm = *fw_.h_prm;
      const unsigned long long sd = static_cast<unsigned long long>(seed);
      prm.seed_lo = unsigned(sd & 0xffffffffull), prm.seed_hi = unsigned(sd >> 32);
      prm.attempt = unsigned(attempt), prm.clip_base = unsigned(clip_base);
      const float T = float(temps[attempt]) / 1000.0f;
      for (int b = 0; b < kSampleClipsMax; ++b) {
        prm.inv_t[b] = temps[attempt] > 0 ? 1.0f / T : 0.0f;
        // ragged: the counter takes the clip's own Whisper position, and the clip index the caller gave it
        prm.pos_off[b] = rag && b < batch ? rw_.h_start[b] : 0;
        prm.clip_off[b] = rag && size_t(b) < clip_index_off.size() ? clip_index_off[size_t(b)] : 0;
      }
      const bool wide = bo && temps[attempt] > 0;  // (an attempt at temperature 0 draws nothing: one row per clip)
      if (wide) {
        decode_best_of(batch, prompt, attempt == 0 ? nullptr : &frozen, attempt == 0, steps);
      } else if (bfb && temps[attempt] == 0) {
        // fallback_beam: beam search over all clips (temperature 0 is the schedule's first entry only), its results
        // into the mirrors an attempt leaves; the length counts EOT as the scores' count does.  (The fall-back needs
        // scores, so the log-probabilities and the no-speech probability are there.)
        beam_full_chains(batch, true, steps);
        std::copy(bf_.h_ids, bf_.h_ids + size_t(batch) * stride, h_ids);
        std::copy(bf_.h_n, bf_.h_n + batch, fw_.h_n);
        std::copy(bf_.h_lp, bf_.h_lp + size_t(batch) * stride, h_lp);
        std::copy(bf_.h_sum, bf_.h_sum + batch, fw_.h_sum);
        std::copy(bf_.h_len, bf_.h_len + batch, fw_.h_count);
        std::copy(bf_.h_nosp, bf_.h_nosp + batch, fw_.h_nosp);
      } else {
        run_chain(attempt == 0 ? nullptr : &frozen, attempt == 0);
      }
      bool again = false;
      for (int b = 0; b < batch; ++b) {
        if (frozen[size_t(b)]) continue;
        if (bo) {
          m_picked[size_t(b)] = wide ? bo_.h_picked[b] : 0;
          for (size_t j = 0; j < G; ++j) {
            m_bo_sum[size_t(b) * G + j] = wide ? bo_.h_all_sum[size_t(b) * G + j] : j == 0 && sc ? fw_.h_sum[b] : 0.0;
            m_bo_count[size_t(b) * G + j] = wide ? bo_.h_all_count[size_t(b) * G + j] : j == 0 && sc ? fw_.h_count[b] : 0;
          }
        }
        std::copy(h_ids + size_t(b) * stride, h_ids + size_t(b + 1) * stride, m_ids.begin() + size_t(b) * stride);
        m_n[size_t(b)] = fw_.h_n[b];
        ClipDecode& info = last.decode_info[size_t(b)];
        info.temperature_milli = int32_t(temps[attempt]);
        info.attempts = int32_t(attempt) + 1;
        info.needs_fallback = 0;
        const int n_row = std::min(fw_.h_n[b], stride);
        std::vector<int64_t> gen;  // the generated ids below eot: the clip's text
        for (int i = np_of(b); i < n_row; ++i) {
          if (h_ids[size_t(b) * stride + i] < vocab_.token_eot) gen.push_back(h_ids[size_t(b) * stride + i]);
        }
        const double ratio = zlib_available() ? compression_ratio(decode_tokens(vocab_, gen.data(), int(gen.size()), true, nullptr)) : 0.0;
        info.compression_ratio = float(ratio);
        float avg = 0.0f;
        if (sc) {
          avg = avg_logprob(fw_.h_sum[b], fw_.h_count[b]);  // (a live clip without a counted id throws here)
          std::copy(h_lp + size_t(b) * stride, h_lp + size_t(b + 1) * stride, m_lp.begin() + size_t(b) * stride);
          m_sum[size_t(b)] = fw_.h_sum[b], m_count[size_t(b)] = fw_.h_count[b], m_nosp[size_t(b)] = fw_.h_nosp[b];
        }
        if (temperature_fallback) {  // (needs scores: check_timestamp_call)
          bool need = double(avg) < double(logprob_threshold) / 1000.0;
          if (compression_ratio_threshold != 0 && ratio > double(compression_ratio_threshold) / 1000.0) need = true;
          if (silent(fw_.h_nosp[b], avg, true)) need = false;
          info.needs_fallback = need ? 1 : 0;
        }
        if (info.needs_fallback && attempt + 1 < temps.size()) again = true;
        else frozen[size_t(b)] = 1, any_wide = any_wide || wide;  // accepted, or the schedule is exhausted: the last result is kept
      }
      if (!again) break;
    }
    std::copy(m_ids.begin(), m_ids.end(), h_ids);
    std::copy(m_n.begin(), m_n.end(), fw_.h_n);
    if (sc) {
      std::copy(m_lp.begin(), m_lp.end(), h_lp);
      std::copy(m_sum.begin(), m_sum.end(), fw_.h_sum);
      std::copy(m_count.begin(), m_count.end(), fw_.h_count);
      std::copy(m_nosp.begin(), m_nosp.end(), fw_.h_nosp);
    }
    last.decode_info_valid = true;
    if (any_wide) last.picked = m_picked, last.best_of_sum = m_bo_sum, last.best_of_count = m_bo_count, last.best_of_valid = true;
  }
  FullResult r;
  r.ids = h_ids; r.stride = stride; r.n = fw_.h_n; r.lp = h_lp;
  r.sum = fw_.h_sum; r.count = fw_.h_count; r.nosp = fw_.h_nosp; r.n_prompt = np_of;
  publish_full(r, batch, ids, ids_stride, n_ids);
  publish_languages();
  if (word_timestamps && !defer_word_alignment) {
    align_words(batch, last.segments, valid_samples ? *valid_samples : std::vector<long long>());
  }
}

// ------------------------------------------- full-length beam search ---

void Engine::ensure_beam_full_workspace() {
  if (bf_.h_done) return;  // (allocated last)
  const wtw::Dims& c = dims_;
  const size_t R = kDecRowsMax, d = c.n_text_state, V = c.n_vocab, C = kBeamClipsMax, S = kBeamMax;
  const size_t cap = size_t(full_cap()), stride = cap + 1, chunks = size_t(beam_chunks(int(V)));
  bf_.kv = dev_zeroed<float>(size_t(c.n_text_layer) * 2 * R * cap * d);
  for (int i = 0; i < 2; ++i) {
    bf_.ids[i] = dev_zeroed<long long>(R * stride);
    bf_.lp[i] = dev_zeroed<float>(R * stride);
    bf_.anc[i] = dev_zeroed<unsigned char>(R * cap);
  }
  bf_.ldl = int((V + 3) & ~size_t(3));
  bf_.logits = dev_zeroed<float>(R * size_t(bf_.ldl));
  bf_.best = dev_zeroed<unsigned long long>(R * ((V + 31) / 32));
  bf_.part = dev_zeroed<BeamFullPart>(R * chunks);
  bf_.ts = dev_zeroed<TsState>(R);
  bf_.n_live = dev_zeroed<int>(C);
  bf_.live_sum = dev_zeroed<double>(C * S);
  bf_.fin_tok = dev_zeroed<int>(C * S * stride);
  bf_.fin_lp = dev_zeroed<float>(C * S * stride);
  bf_.fin_sum = dev_zeroed<double>(C * S);
  bf_.fin_len = dev_zeroed<int>(C * S);
  bf_.n_fin = dev_zeroed<int>(C);
  bf_.done = dev_zeroed<int>(C);
  bf_.parent = dev_zeroed<int>(R);
  bf_.token = dev_zeroed<long long>(R);
  bf_.tok_lp = dev_zeroed<float>(R);
  bf_.out_ids = dev_zeroed<long long>(C * stride);
  bf_.out_lp = dev_zeroed<float>(C * stride);
  bf_.out_n = dev_zeroed<int>(C);
  bf_.out_len = dev_zeroed<int>(C);
  bf_.out_sum = dev_zeroed<double>(C);
  bf_.sc_part = dev_zeroed<ScorePart>(C * size_t(ts_chunks(int(V))));
  bf_.nosp = dev_zeroed<float>(C);
  bf_.h_prompt = pinned<long long>(C * stride);
  bf_.h_ids = pinned<long long>(C * stride);
  bf_.h_lp = pinned<float>(C * stride);
  bf_.h_nosp = pinned<float>(C);
  bf_.h_sum = pinned<double>(C);
  bf_.h_n = pinned<int>(C);
  bf_.h_len = pinned<int>(C);
  bf_.h_done = pinned<int>(C);
}

// Full-length beam search: decode_beam's chains — nc <= 128 / K clips, the prompt over nc rows, then
// one position per pass over K * nc rows, row = k * nc + c — continued to P = max_positions in decode_full's segments of
// 32 positions.  The hypotheses share ONE self-attention cache of 128 rows: the prompt's K / V land in rows c (the
// clips' slot 0), every later pass writes row r's new position in place and reads the earlier ones through the row's
// ancestor table (the gathered form of self_attention_long), so a step moves id, log-probability and table rows only.
// Between the logits GEMM and the next pass: beam_full_partial, beam_full_select, beam_full_advance (k_beam_full.hip).
// After each segment the clips' done flags come back and a chain ends once every clip is done.  beam_full_chains leaves
// the results in bf_'s pinned mirrors; decode_beam_full publishes them as a call's (ids, beam scores, scores, segments),
// and decode_full's fall-back loop merges them as its attempt at temperature 0 (option fallback_beam).
void Engine::decode_beam_full(int batch, int64_t* ids, int ids_stride, int32_t* n_ids) {
  int steps = 0;
  beam_full_chains(batch, true, steps);
  const int stride = full_cap() + 1, n_prompt = int(prompt().size());
  last.beam_sum.assign(size_t(batch), 0.0f);
  last.beam_len.assign(bf_.h_len, bf_.h_len + batch);
  for (int b = 0; b < batch; ++b) last.beam_sum[size_t(b)] = float(bf_.h_sum[b]);
  last.beam_valid = true;
  FullResult r;
  r.ids = bf_.h_ids; r.stride = stride; r.n = bf_.h_n; r.lp = bf_.h_lp;
  r.sum = bf_.h_sum; r.count = bf_.h_len; r.nosp = bf_.h_nosp; r.n_prompt = [n_prompt](int) { return n_prompt; };
  publish_full(r, batch, ids, ids_stride, n_ids);
}

void Engine::beam_full_chains(int batch, bool first, int& steps) {
  const int K = int(beam_size), P = int(max_positions), slot_idx = last_enc_slot_;
  Slot& slot = slots_[slot_idx];
  if (!slot.absorbed) throw Error(kErrUnsupported, "full-length beam search: the encoder pass did not prepare the absorbed cross-attention");
  ensure_batch(batch);
  ensure_beam_full_workspace();  // (before any capture: nothing may be allocated inside one)
  const wtw::Dims& c = dims_;
  const int d = c.n_text_state, T = c.n_audio_ctx, V = c.n_vocab, cap = full_cap(), stride = cap + 1;
  const bool ts = timestamps != 0, sc = scores != 0, sup = suppressing();
  const int n_sup = int(suppress_ids.size()), n_sup_first = int(suppress_first_ids.size());
  const std::vector<long long> prompt = this->prompt();
  const int n_prompt = int(prompt.size());
  check_prompt_ids(prompt, kErrInvalidArg);
  if (n_prompt >= P) throw Error(kErrInvalidArg, "full-length beam search: the prompt leaves no position to generate");
  const int per_chain = kDecRowsMax / K, sot_idx = 0;  // Whisper's sot_index: the no-speech logits are read there
  slot.dec = slot_idx % n_dec_streams_;
  slot.pair_leader = -1;
  DecWorkspace& dw = dws_[slot.dec];
  hipStream_t const st = dec_stream_at(slot.dec);
  for (int b = 0; b < kBeamClipsMax; ++b) {
    for (int i = 0; i < stride; ++i) bf_.h_prompt[size_t(b) * stride + i] = i < n_prompt ? prompt[size_t(i)] : 0;
    // full_language: the clip's own language behind sot (decode_full detected or holds it)
    if (size_t(b) < call_lang_.size()) bf_.h_prompt[size_t(b) * stride + 1] = kLangLo + std::max(call_lang_[size_t(b)], 0);
  }
  HIPCHK(hipStreamWaitEvent(st, slot.enc_done, 0));
  if (first) HIPCHK(hipEventRecord(slot.dec_begin, st));
  for (int c0 = 0; c0 < batch; c0 += per_chain) {
    const int nc = std::min(per_chain, batch - c0), rows = K * nc;
    const int n_abs = abs_chunks_for(nc, 256);
    BeamFullArgs fa;
    fa.clips = nc; fa.K = K; fa.c0 = c0; fa.n_prompt = n_prompt; fa.pos = n_prompt - 1; fa.V = V; fa.ldl = bf_.ldl;
    fa.stride = stride; fa.cap = cap; fa.eot = vocab_.token_eot; fa.beg = vocab_.token_beg;
    fa.max_initial = int(max_initial_timestamp); fa.timestamps = ts ? 1 : 0;
    fa.logits = bf_.logits; fa.part = bf_.part; fa.ts = bf_.ts; fa.n_live = bf_.n_live; fa.live_sum = bf_.live_sum;
    fa.fin_tok = bf_.fin_tok; fa.fin_lp = bf_.fin_lp; fa.fin_sum = bf_.fin_sum; fa.fin_len = bf_.fin_len; fa.n_fin = bf_.n_fin;
    fa.done = bf_.done; fa.parent = bf_.parent; fa.token = bf_.token; fa.tok_lp = bf_.tok_lp;
    fa.out_ids = bf_.out_ids; fa.out_lp = bf_.out_lp; fa.out_n = bf_.out_n; fa.out_len = bf_.out_len; fa.out_sum = bf_.out_sum;
    // step t = pos + 1 - n_prompt reads the half t & 1 of the double buffers and writes the other
    auto halves = [&](int t) {
      const int cur = t & 1;
      fa.ids_src = bf_.ids[cur]; fa.ids_dst = bf_.ids[cur ^ 1]; fa.lp_src = bf_.lp[cur]; fa.lp_dst = bf_.lp[cur ^ 1];
      fa.anc_src = bf_.anc[cur]; fa.anc_dst = bf_.anc[cur ^ 1];
    };
    DecPass p;
    p.clips = nc; p.ids_stride = stride; p.self_kv = bf_.kv; p.self_cap = cap; p.self_rows = kDecRowsMax;
    p.absorbed = true; p.n_abs = n_abs; p.e = slot.e_planes + size_t(c0) * T * d; p.split = fc2_split(); p.dw = &dw;
    p.Y = bf_.logits; p.ldy = bf_.ldl;
    p.bf = bf16 != 0;  // option full_bf16: bf_.kv holds bf16 rows (the first half of it)
    ScoreArgs sa;
    sa.logits = bf_.logits; sa.ldl = bf_.ldl; sa.V = V; sa.batch = nc; sa.part = bf_.sc_part;
    const int np_max = std::max(1, std::min(4, kDecRowsMax / nc));
    // the passes whose first position lies in [lo, hi), each with its step; returns the steps among them
    auto enqueue_segment = [&](int lo, int hi) {
      int seg_steps = 0;
      for (int pos0 = 0, np = 1; pos0 < hi; pos0 += np) {
        np = pos0 < n_prompt ? std::min(np_max, n_prompt - pos0) : 1;
        if (sc && pos0 <= sot_idx) np = std::min(np, sot_idx - pos0 + 1);  // a pass ends at sot, with logits: the no-speech probability
        if (pos0 < lo) continue;
        const int last = pos0 + np - 1, t = last + 1 - n_prompt;
        const bool logits = t >= 0, nosp = sc && last == sot_idx;
        if (pos0 < n_prompt) {  // the prompt: nc rows, their K / V into rows c of the shared cache
          p.B = nc; p.ids = bf_.ids[0]; p.self_anc = nullptr;
        } else {  // the id the step before chose, over the K * nc rows that step wrote
          p.B = rows; p.ids = bf_.ids[t & 1]; p.self_anc = bf_.anc[t & 1];
        }
        p.pos0 = pos0; p.np = np; p.best = logits || nosp ? bf_.best : nullptr;
        decoder_pass(p, st);
        if (nosp) launch_no_speech_prob(sa, vocab_.token_solm, bf_.nosp + c0, st);
        if (logits) {
          fa.pos = last;
          halves(t);
          // behind the no-speech probability, in front of every hypothesis's allowed set
          if (sup) enqueue_suppress(bf_.logits, bf_.ldl, p.B, t == 0, st);
          launch_beam_full_partial(fa, st);
          launch_beam_full_select(fa, st);
          launch_beam_full_advance(fa, st);
          ++seg_steps;
        }
      }
      return seg_steps;
    };
    HIPCHK(hipMemcpyAsync(bf_.ids[0], bf_.h_prompt + size_t(c0) * stride, size_t(nc) * stride * sizeof(long long), hipMemcpyHostToDevice, st));
    halves(1);  // (begin writes the prompt's table entries into the half step 0 reads)
    launch_beam_full_begin(fa, st);
    // (greedy's keys start with the slot, a beam key with -beam_size, a full-length key with kFullKey)
    auto key_of = [&](int lo) {
      std::vector<long long> key{kBeamFullKey, slot_idx, c0, nc, lo, P, n_prompt, K, fc2_ksplit, n_abs, slot.dec, ts ? 1 : 0,
                                 ts ? max_initial_timestamp : 0, sc ? 1 : 0};
      if (sup) key.push_back(n_sup), key.push_back(n_sup_first);  // launch constants; the ids themselves are device data
      if (p.bf) key.push_back(kBf16KeyMark);  // (last, in the bf16 storage mode only)
      return key;
    };
    // the position behind the last pass that ran: every clip done ends the chain behind that segment
    const int end = run_segments(P, st, true, "full-length beam", key_of, enqueue_segment, DonePoll{bf_.done + c0, nc, bf_.h_done}, steps);
    fa.pos = end - 1;  // the last step that ran; its advance wrote the half the NEXT step would read
    halves(end - n_prompt + 1);
    launch_beam_full_finalize(fa, st);
  }
  HIPCHK(hipMemcpyAsync(bf_.h_ids, bf_.out_ids, size_t(batch) * stride * sizeof(long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(bf_.h_lp, bf_.out_lp, size_t(batch) * stride * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(bf_.h_n, bf_.out_n, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(bf_.h_len, bf_.out_len, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(bf_.h_sum, bf_.out_sum, size_t(batch) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (sc) HIPCHK(hipMemcpyAsync(bf_.h_nosp, bf_.nosp, size_t(batch) * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(slot.dec_done, st));
  slot.steps = steps;  // (summed over the attempts of a fall-back)
  finish_slot(slot_idx);  // waits; the encoder's non-finite flag, timings
}

// ------------------------------------------------ several samples per clip ---

void Engine::ensure_best_of_workspace() {
  ensure_beam_full_workspace();  // the 128-row cache, id rows, log-probabilities, table, logits and output rows
  if (bo_.h_all_sum) return;     // (allocated last)
  const size_t R = kDecRowsMax, C = kSampleClipsMax, G = kSampleGroupMax, chunks = size_t(ts_chunks(dims_.n_vocab));
  bo_.sc_part = dev_zeroed<ScorePart>(R * chunks);
  bo_.sm_part = dev_zeroed<SamplePart>(R * chunks);
  bo_.n_ids = dev_zeroed<int>(R);
  bo_.finished = dev_zeroed<int>(R);
  bo_.count = dev_zeroed<int>(R);
  bo_.sum = dev_zeroed<double>(R);
  bo_.frozen = dev_zeroed<int>(C);
  bo_.out_count = dev_zeroed<int>(C);
  bo_.picked = dev_zeroed<int>(C);
  bo_.all_count = dev_zeroed<int>(C * G);
  bo_.all_sum = dev_zeroed<double>(C * G);
  bo_.h_frozen = pinned<int>(C);
  bo_.h_fin = pinned<int>(R);
  bo_.h_picked = pinned<int>(C);
  bo_.h_all_count = pinned<int>(C * G);
  bo_.h_all_sum = pinned<double>(C * G);
}

// Several samples per clip: decode_beam_full's chains with the sampler in the beam's place.  A chain
// decodes nc <= 128 / N clips on rows j * nc + c of bf_'s ONE cache.  The prompt positions 0 .. n_prompt - 2 run over the
// nc clips into cache rows c; from position n_prompt - 1 on every pass runs over the N * nc rows on the gathered
// self_attention_long under the FIXED table best_of_begin wrote (the prompt's K / V from row c, the rest from the row
// itself), so the first sampling step already has one logits row per sample and no K / V is copied.  Per step:
// suppression, score_partial, the grouped sampler, score_finish (the ranking needs the sums whether or not scores are
// published).  best_of_pick ends a chain.  The attempt's parameter block is decode_full's; a chain's clips are its
// entries c0 .. c0 + nc - 1.
void Engine::decode_best_of(int batch, const std::vector<long long>& prompt, const std::vector<int>* frozen, bool first, int& steps) {
  const int N = int(best_of), P = int(max_positions), slot_idx = last_enc_slot_;
  Slot& slot = slots_[slot_idx];
  const wtw::Dims& c = dims_;
  const int d = c.n_text_state, T = c.n_audio_ctx, V = c.n_vocab, cap = full_cap(), stride = cap + 1;
  const bool ts = timestamps != 0, sc = scores != 0, sup = suppressing();
  const int n_sup = int(suppress_ids.size()), n_sup_first = int(suppress_first_ids.size());
  const int n_prompt = int(prompt.size());
  const int per_chain = kDecRowsMax / N, sot_idx = 0;  // Whisper's sot_index: the no-speech logits are read there
  DecWorkspace& dw = dws_[slot.dec];
  hipStream_t const st = dec_stream_at(slot.dec);
  for (int b = 0; b < kBeamClipsMax; ++b) {
    for (int i = 0; i < stride; ++i) bf_.h_prompt[size_t(b) * stride + i] = i < n_prompt ? prompt[size_t(i)] : 0;
    // full_language: the clip's own language behind sot (decode_full detected or holds it)
    if (size_t(b) < call_lang_.size()) bf_.h_prompt[size_t(b) * stride + 1] = kLangLo + std::max(call_lang_[size_t(b)], 0);
  }
  for (int b = 0; b < batch; ++b) bo_.h_frozen[b] = frozen ? (*frozen)[size_t(b)] : 0;
  HIPCHK(hipStreamWaitEvent(st, slot.enc_done, 0));
  if (first) HIPCHK(hipEventRecord(slot.dec_begin, st));
  HIPCHK(hipMemcpyAsync(fw_.sm_prm, fw_.h_prm, sizeof(SampleParams), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(bo_.frozen, bo_.h_frozen, size_t(batch) * sizeof(int), hipMemcpyHostToDevice, st));
  for (int c0 = 0; c0 < batch; c0 += per_chain) {
    const int nc = std::min(per_chain, batch - c0), rows = N * nc;
    bool any = false;
    for (int b = c0; b < c0 + nc; ++b) any = any || !bo_.h_frozen[b];
    if (!any) continue;  // every clip of the range was accepted by an earlier attempt
    const int n_abs = abs_chunks_for(nc, 256);
    BestOfArgs ba;
    ba.clips = nc; ba.N = N; ba.c0 = c0; ba.n_prompt = n_prompt; ba.stride = stride; ba.cap = cap;
    ba.ids = bf_.ids[0]; ba.lp = bf_.lp[0]; ba.n_ids = bo_.n_ids; ba.finished = bo_.finished; ba.sum = bo_.sum; ba.count = bo_.count;
    ba.frozen = bo_.frozen + c0; ba.anc = bf_.anc[0];
    ba.out_ids = bf_.out_ids; ba.out_lp = bf_.out_lp; ba.out_n = bf_.out_n; ba.out_count = bo_.out_count; ba.picked = bo_.picked;
    ba.out_sum = bf_.out_sum; ba.all_sum = bo_.all_sum; ba.all_count = bo_.all_count;
    DecPass p;
    p.clips = nc; p.ids = bf_.ids[0]; p.ids_stride = stride; p.self_kv = bf_.kv; p.self_cap = cap; p.self_rows = kDecRowsMax;
    p.absorbed = true; p.n_abs = n_abs; p.e = slot.e_planes + size_t(c0) * T * d; p.split = fc2_split(); p.dw = &dw;
    p.Y = bf_.logits; p.ldy = bf_.ldl;
    p.bf = bf16 != 0;  // option full_bf16, as in beam_full_chains
    ScoreArgs sa;
    fill_rule_args(sa, bf_.logits, bf_.ldl);
    sa.part = bo_.sc_part;
    sa.ids = bf_.ids[0]; sa.ids_stride = stride; sa.n_ids = bo_.n_ids; sa.token_logprob = bf_.lp[0]; sa.lp_stride = stride;
    sa.sum = bo_.sum; sa.count = bo_.count;
    const int wide0 = n_prompt - 1;  // the first position that runs over all the rows
    const int np_max = std::max(1, std::min(4, kDecRowsMax / nc));
    // the chain's passes: the prompt below wide0 over the nc clips (a pass ends at sot, with logits: the no-speech
    // probability), then one position per pass over all the rows.  Where the wide passes begin at sot (a prompt of one
    // id) the narrow pass at sot still runs for the no-speech probability and the wide pass repeats that position.
    struct Pass {
      int pos0, np;
      bool narrow, nosp;
    };
    std::vector<Pass> passes;
    for (int pos0 = 0, np = 1; pos0 < wide0; pos0 += np) {
      np = std::min(np_max, wide0 - pos0);
      if (sc && pos0 <= sot_idx) np = std::min(np, sot_idx - pos0 + 1);
      passes.push_back(Pass{pos0, np, true, sc && pos0 + np - 1 == sot_idx});
    }
    if (sc && wide0 <= sot_idx) passes.push_back(Pass{sot_idx, 1, true, true});
    for (int pos0 = wide0; pos0 < P; ++pos0) passes.push_back(Pass{pos0, 1, false, false});
    // the passes whose first position lies in [lo, hi), each wide one with its step; returns the steps among them
    auto enqueue_segment = [&](int lo, int hi) {
      int seg_steps = 0;
      for (const Pass& q : passes) {
        if (q.pos0 < lo || q.pos0 >= hi) continue;
        const int last = q.pos0 + q.np - 1, t = last + 1 - n_prompt;
        p.B = q.narrow ? nc : rows; p.self_anc = q.narrow ? nullptr : bf_.anc[0];
        p.pos0 = q.pos0; p.np = q.np; p.best = !q.narrow || q.nosp ? bf_.best : nullptr;
        decoder_pass(p, st);
        if (q.nosp) {
          sa.batch = nc; sa.state = nullptr;
          launch_no_speech_prob(sa, vocab_.token_solm, bf_.nosp + c0, st);
        }
        if (q.narrow) continue;
        // behind the no-speech probability, in front of every sample's allowed set
        if (sup) enqueue_suppress(bf_.logits, bf_.ldl, rows, t == 0, st);
        // the partial sums of the allowed set, from the state BEFORE the selection advances it
        sa.batch = rows; sa.state = ts ? bf_.ts : nullptr; sa.n_gen = t; sa.pos = last;
        launch_score_partial(sa, st);
        SampleArgs g;
        fill_rule_args(g, bf_.logits, bf_.ldl);
        g.batch = rows; g.group = N;
        g.n_gen = t; g.params = fw_.sm_prm; g.row0 = c0; g.part = bo_.sm_part; g.state = ts ? bf_.ts : nullptr;
        g.ids = bf_.ids[0]; g.ids_stride = stride; g.pos = last; g.stop_at_eot = 1;
        g.n_ids = bo_.n_ids; g.finished = bo_.finished;
        launch_sample_select(g, st);
        launch_score_finish(sa, st);
        ++seg_steps;
      }
      return seg_steps;
    };
    HIPCHK(hipMemcpyAsync(bf_.ids[0], bf_.h_prompt + size_t(c0) * stride, size_t(nc) * stride * sizeof(long long), hipMemcpyHostToDevice, st));
    launch_best_of_begin(ba, st);
    if (ts) launch_ts_state_init(bf_.ids[0], stride, nullptr, n_prompt, n_prompt, V, vocab_.token_beg, bf_.ts, rows, st);
    auto key_of = [&](int lo) {
      std::vector<long long> key{kBestOfKey, slot_idx, N, c0, nc, lo, P, n_prompt, fc2_ksplit, n_abs, slot.dec, ts ? 1 : 0,
                                 ts ? max_initial_timestamp : 0, sc ? 1 : 0};
      if (sup) key.push_back(n_sup), key.push_back(n_sup_first);  // launch constants; the ids themselves are device data
      if (p.bf) key.push_back(kBf16KeyMark);  // (last, in the bf16 storage mode only)
      return key;
    };
    // every row finished: the chain ends behind that segment
    run_segments(P, st, true, "best-of", key_of, enqueue_segment, DonePoll{bo_.finished, rows, bo_.h_fin}, steps);
    launch_best_of_pick(ba, st);
  }
  HIPCHK(hipMemcpyAsync(fw_.h_ids, bf_.out_ids, size_t(batch) * stride * sizeof(long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(fw_.h_n, bf_.out_n, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(bo_.h_picked, bo_.picked, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(bo_.h_all_sum, bo_.all_sum, size_t(batch) * kSampleGroupMax * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(bo_.h_all_count, bo_.all_count, size_t(batch) * kSampleGroupMax * sizeof(int), hipMemcpyDeviceToHost, st));
  if (sc) {
    HIPCHK(hipMemcpyAsync(fw_.h_lp, bf_.out_lp, size_t(batch) * stride * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(fw_.h_sum, bf_.out_sum, size_t(batch) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(fw_.h_count, bo_.out_count, size_t(batch) * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(fw_.h_nosp, bf_.nosp, size_t(batch) * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipEventRecord(slot.dec_done, st));
  slot.steps = steps;  // (summed over the attempts)
  finish_slot(slot_idx);  // waits; the encoder's non-finite flag, timings
}

// Word-level timestamps: the alignment pass over the kept results of a timestamp decode.  Clips go
// through in sub-groups whose weight workspace [clips][heads][L][T] stays below kAlignWeightBytes; a sub-group's rows are
// fed in passes of kDecRowsMax / clips positions on self_attention_prefill and the absorbed cross-attention, eagerly (the
// row lengths are launch constants, as a context's are), without logits.  The self-attention cache and the id rows are
// the decode's own: its results are on the host by now.
void Engine::align_words(int batch, const std::vector<Segment>& segs, const std::vector<long long>& valid_samples) {
  Slot& slot = slots_[last_enc_slot_];
  static_assert(kAlignClipsMax >= 64, "a full-length call has up to 64 clips");
  const wtw::Dims& c = dims_;
  const int T = c.n_audio_ctx, d = c.n_text_state, cap = full_cap(), stride = cap + 1;
  const std::vector<long long> A = prompt();
  const int n_a = int(A.size());
  const std::vector<std::pair<int, int>> heads = alignment_heads_in_effect();
  const int n_heads = int(heads.size());
  const int text_cap = cap - n_a - 2;
  if (text_cap < 1) throw Error(kErrInvalidArg, "word_timestamps: the prompt leaves no position for text");
  const bool scored = scores != 0 && last.scores_valid;
  // the language a clip was decoded behind: the option, or with full_language what decode_full left per clip
  auto lang_of = [&](int b) { return language >= 0 ? language : size_t(b) < call_lang_.size() ? long(call_lang_[size_t(b)]) : -1l; };
  auto unicode_only_of = [&](int b) {  // Whisper's word-splitting rule for the languages written without spaces
    const long l = lang_of(b);
    const std::string lang = l >= 0 && l < language_count() ? lang_code(size_t(l)) : std::string("en");
    return lang == "zh" || lang == "ja" || lang == "th" || lang == "lo" || lang == "my" || lang == "yue";
  };

  // ---- the rows: per clip the text ids of its segments (below EOT, timestamps removed) and where they sit in its id row
  struct Clip {
    std::vector<long long> text;
    std::vector<int> at, seg;  // index in the id row, index in last.segments
    int L = 0, N = 0, F = 0;
  };
  std::vector<Clip> clips(static_cast<size_t>(batch));
  for (size_t i = 0; i < segs.size(); ++i) {
    const Segment& sg = segs[i];
    if (sg.clip < 0 || sg.clip >= batch || sg.id_begin < 0 || sg.id_begin + sg.id_count > stride) {
      throw Error(kErrInvalidArg, "word_timestamps: a segment outside the call's id rows");
    }
    Clip& cl = clips[size_t(sg.clip)];
    for (int k = 0; k < sg.id_count; ++k) {
      const long long id = fw_.h_ids[size_t(sg.clip) * stride + sg.id_begin + k];
      if (id >= vocab_.token_eot || int(cl.text.size()) >= text_cap) continue;
      cl.text.push_back(id), cl.at.push_back(sg.id_begin + k), cl.seg.push_back(int(i));
    }
  }
  int L_max = 0;
  for (int b = 0; b < batch; ++b) {
    Clip& cl = clips[size_t(b)];
    cl.N = int(cl.text.size()) + 1;
    cl.L = n_a + 1 + int(cl.text.size()) + 1;
    const long long vs = size_t(b) < valid_samples.size() ? valid_samples[size_t(b)] : (long long)T * 320;
    cl.F = int(std::min<long long>(T, std::max<long long>(1, vs / 320)));
    L_max = std::max(L_max, cl.L);
  }
  const int N_max = L_max - n_a - 1;
  for (int b = 0; b < batch; ++b) {  // rows padded with EOT: causality keeps the padding out of a clip's own positions
    const Clip& cl = clips[size_t(b)];
    long long* row = fw_.h_ids + size_t(b) * stride;
    for (int i = 0; i < stride; ++i) row[i] = vocab_.token_eot;
    std::copy(A.begin(), A.end(), row);
    if (language < 0 && lang_of(b) >= 0 && n_a > 1) row[1] = kLangLo + lang_of(b);  // full_language: the clip's own language token
    row[n_a] = vocab_.token_not;
    std::copy(cl.text.begin(), cl.text.end(), row + n_a + 1);
  }

  // ---- workspaces (outside any capture; this pass captures nothing)
  const size_t per_clip = size_t(n_heads) * L_max * T;
  int sub = int(std::max<size_t>(1, std::min<size_t>(size_t(batch), kAlignWeightBytes / (per_clip * sizeof(float)))));
  if (align_sub > 0) sub = int(std::min<long>(sub, align_sub));
  auto grow = [&](auto*& ptr, size_t& have, size_t want) {
    if (want <= have) return;
    if (ptr) {
      HIPCHK(hipStreamSynchronize(dec_stream_at(slot.dec)));
      allocations_.erase(std::remove(allocations_.begin(), allocations_.end(), static_cast<void*>(ptr)), allocations_.end());
      (void)hipFree(ptr);
      ptr = nullptr, have = 0;
    }
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, want * sizeof(*ptr)));
    allocations_.push_back(q);
    ptr = static_cast<std::remove_reference_t<decltype(ptr)>>(q), have = want;
  };
  grow(aw_.W, aw_.w_elems, size_t(sub) * per_clip);
  grow(aw_.stats, aw_.s_elems, size_t(sub) * n_heads * 2 * T);
  {
    const size_t want = size_t(batch) * N_max * T, had = aw_.c_elems;
    grow(aw_.C, aw_.c_elems, want);
    size_t t_have = had;
    grow(aw_.trace, t_have, want);
  }
  if (!aw_.h_lfn) {  // (committed together, the last pointer is the sentinel: a failure half way leaves nothing behind)
    void *j = nullptr, *l = nullptr, *hj = nullptr, *hl = nullptr;
    const bool ok = hipMalloc(&j, size_t(64) * kAlignRowsMax * sizeof(int)) == hipSuccess &&
                    hipMalloc(&l, size_t(3) * 64 * sizeof(int)) == hipSuccess &&
                    hipHostMalloc(&hj, size_t(64) * kAlignRowsMax * sizeof(int), 0) == hipSuccess &&
                    hipHostMalloc(&hl, size_t(3) * 64 * sizeof(int), 0) == hipSuccess;
    if (!ok) {
      (void)hipFree(j), (void)hipFree(l), (void)hipHostFree(hj), (void)hipHostFree(hl);
      (void)hipGetLastError();
      throw Error(kErrDevice, "word_timestamps: out of memory for the alignment workspace");
    }
    allocations_.push_back(j), allocations_.push_back(l), pinned_.push_back(hj), pinned_.push_back(hl);
    aw_.jump = static_cast<int*>(j), aw_.lfn = static_cast<int*>(l);
    aw_.h_jump = static_cast<int*>(hj), aw_.h_lfn = static_cast<int*>(hl);
  }

  DecWorkspace& dw = dws_[slot.dec];
  hipStream_t const st = dec_stream_at(slot.dec);
  for (int b = 0; b < batch; ++b) aw_.h_lfn[b] = clips[size_t(b)].L, aw_.h_lfn[64 + b] = clips[size_t(b)].F, aw_.h_lfn[128 + b] = clips[size_t(b)].N;
  HIPCHK(hipMemcpyAsync(aw_.lfn, aw_.h_lfn, size_t(3) * 64 * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(fw_.ids, fw_.h_ids, size_t(batch) * stride * sizeof(long long), hipMemcpyHostToDevice, st));
  if (!slot.absorbed && bf16) {  // the decode ran the cached form: the ONE bf16 plane the bf16 absorbed form reads
    launch_f32_to_bf16(ws_.enc_out, slot.e_planes, long(batch) * T * d, st);
  } else if (!slot.absorbed) {  // the planes the absorbed form reads, from the fp32 encoder output
    launch_f32_to_planes(ws_.enc_out, slot.e_planes, long(ws_.batch) * T * d, long(batch) * T, d, &cross_kv_.sc.a, 0, st);
  }
  AlignSink sink;
  sink.heads_total = n_heads; sink.L_max = L_max; sink.ldw = T; sink.W = aw_.W;
  sink.layer.resize(size_t(c.n_text_layer));
  for (int a = 0; a < n_heads; ++a) sink.layer[size_t(heads[size_t(a)].first)].emplace_back(heads[size_t(a)].second, a);
  const size_t keep0 = last.alignment.size();  // (the seeking loop appends window after window)
  if (keep_alignment) last.alignment.resize(keep0 + size_t(batch));
  for (int c0 = 0; c0 < batch; c0 += sub) {
    const int nb = std::min(sub, batch - c0);
    for (int b = 0; b < nb; ++b) sink.F[b] = clips[size_t(c0 + b)].F;
    DecPass p;
    p.B = p.clips = nb; p.ids = fw_.ids + size_t(c0) * stride; p.ids_stride = stride; p.self_kv = fw_.kv; p.self_cap = cap;
    p.absorbed = true; p.n_abs = abs_chunks_for(nb, 256); p.e = slot.e_planes + size_t(c0) * T * d;
    p.split = fc2_split(); p.dw = &dw; p.self_prefill = true; p.align = &sink; p.best = nullptr;
    p.bf = bf16 != 0;  // option full_bf16_all: the decode's own bf16 weights and cache (the first half of fw_.kv)
    const int group = std::max(1, kDecRowsMax / nb);
    for (int pos0 = 0; pos0 < L_max; pos0 += group) {
      p.pos0 = pos0; p.np = std::min(group, L_max - pos0);
      decoder_pass(p, st);
    }
    AlignMatrixArgs am;
    am.W = aw_.W; am.clips = nb; am.heads = n_heads; am.L_max = L_max; am.ldw = T; am.L = aw_.lfn + c0; am.F = aw_.lfn + 64 + c0;
    am.n_a = n_a; am.stats = aw_.stats; am.C = aw_.C + size_t(c0) * N_max * T; am.N_max = N_max; am.ldc = T;
    launch_align_matrix(am, st);
    if (keep_alignment) {
      HIPCHK(hipStreamSynchronize(st));
      for (int b = 0; b < nb; ++b) {
        ClipAlignment& ka = last.alignment[keep0 + size_t(c0 + b)];
        const Clip& cl = clips[size_t(c0 + b)];
        ka.n_a = n_a, ka.L = cl.L, ka.N = cl.N, ka.F = cl.F, ka.heads = n_heads, ka.T = T;
        ka.row.assign(fw_.h_ids + size_t(c0 + b) * stride, fw_.h_ids + size_t(c0 + b) * stride + cl.L);
        ka.W.resize(size_t(n_heads) * cl.L * T);
        for (int a = 0; a < n_heads; ++a) {
          HIPCHK(hipMemcpy(ka.W.data() + size_t(a) * cl.L * T, aw_.W + (size_t(b) * n_heads + a) * L_max * T, size_t(cl.L) * T * sizeof(float), hipMemcpyDeviceToHost));
        }
        ka.C.resize(size_t(cl.N) * T);
        HIPCHK(hipMemcpy(ka.C.data(), aw_.C + size_t(c0 + b) * N_max * T, ka.C.size() * sizeof(float), hipMemcpyDeviceToHost));
      }
    }
  }
  AlignDtwArgs ad;
  ad.C = aw_.C; ad.clips = batch; ad.N_max = N_max; ad.ldc = T; ad.N = aw_.lfn + 128; ad.F = aw_.lfn + 64; ad.trace = aw_.trace; ad.jump = aw_.jump;
  launch_align_dtw(ad, st);
  HIPCHK(hipMemcpyAsync(aw_.h_jump, aw_.jump, size_t(batch) * N_max * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));

  // ---- words on the host
  last.words.clear();
  last.word_text.clear();
  for (int b = 0; b < batch; ++b) {
    const Clip& cl = clips[size_t(b)];
    const int* jump = aw_.h_jump + size_t(b) * N_max;
    if (keep_alignment) last.alignment[keep0 + size_t(b)].jump.assign(jump, jump + cl.N);
    const int n_text = int(cl.text.size());
    if (n_text == 0) continue;  // no segments (nothing decoded, or skip_silence blanked the clip): no words
    std::vector<int64_t> ids(cl.text.begin(), cl.text.end());
    ids.push_back(vocab_.token_eot);
    std::vector<int> words = split_words(vocab_, ids.data(), n_text + 1, unicode_only_of(b));
    // the final EOT served as the last end time; ids that share its word (none: a special id starts a word) stay
    int covered = 0;
    std::vector<int> kept;
    for (int len : words) {
      if (covered + len > n_text) len = n_text - covered;
      if (len > 0) kept.push_back(len);
      covered += len;
    }
    const std::vector<int> merged = merge_punctuation(vocab_, ids.data(), n_text, kept.data(), int(kept.size()));
    int s0 = 0;
    for (int len : merged) {
      Word w{};
      w.clip = b; w.segment = cl.seg[size_t(s0)];
      w.t0_ms = jump[s0] * 20; w.t1_ms = jump[s0 + len] * 20;
      w.id_begin = cl.at[size_t(s0)]; w.id_count = cl.at[size_t(s0 + len - 1)] - cl.at[size_t(s0)] + 1;
      if (scored) {
        double sum = 0.0;
        for (int k = 0; k < len; ++k) sum += std::exp(double(last.token_logprob[size_t(b) * last.lp_stride + cl.at[size_t(s0 + k)]]));
        w.probability = float(sum / double(len));
      }
      last.words.push_back(w);
      last.word_text.push_back(decode_tokens(vocab_, ids.data() + s0, len, true, nullptr));
      s0 += len;
    }
  }
  last.words_valid = true;
}

}  // namespace wt
