// Seeking long-audio transcription: the host side of DESIGN section 20 (longform.h).
#include "longform.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "engine.h"

namespace wt {

int seek_step(const VocabData& vocab, const int64_t* g, int n, int win_ticks, int seg_ticks, std::vector<Segment>* out) {
  const int64_t beg = vocab.token_beg, eot = vocab.token_eot;
  auto ts = [&](int i) { return g[i] >= beg; };
  auto tick = [&](int64_t id) { return int(std::min<int64_t>(std::max<int64_t>(id - beg, 0), win_ticks)); };
  auto push = [&](int first, int end, int t0, int t1, int open) {
    bool text = false;
    for (int i = first; i < end; ++i) text = text || g[i] < eot;
    if (text && t0 != t1) out->push_back(Segment{0, t0 * 20, t1 * 20, first, end - first, open});
  };
  const bool single_end = n >= 2 && ts(n - 1) && !ts(n - 2);
  std::vector<int> cuts;
  for (int i = 1; i < n; ++i) {
    if (ts(i - 1) && ts(i)) cuts.push_back(i);
  }
  int advance = seg_ticks;
  if (!cuts.empty()) {
    if (single_end) cuts.push_back(n);
    int last = 0;
    for (int cur : cuts) {
      push(last, cur, tick(g[last]), tick(g[cur - 1]), 0);
      last = cur;
    }
    if (!single_end) advance = tick(g[last - 1]);
  } else {
    int t1 = seg_ticks, open = 1;
    for (int i = n - 1; i >= 0; --i) {
      if (!ts(i)) continue;
      if (tick(g[i]) != 0) t1 = tick(g[i]), open = 0;
      break;
    }
    push(0, n, 0, t1, open);
  }
  return advance == 0 ? seg_ticks : advance;
}

namespace {

// What the seeking loop carries for one file, and what it leaves in the engine's last_* results
struct SeekFile {
  std::vector<int64_t> ctx;  // the ids kept so far: the next window's context
  size_t seek = 0;
  int w = 0;                 // windows decoded
  std::string text;          // the windows' lines, joined by '\n'
  std::vector<Segment> segments;  // clip = the window's index in the file, times in the file
  std::vector<std::string> segment_text;
  std::vector<ClipScore> scores;
  std::vector<float> token_logprob, segment_score;
  std::vector<Engine::ClipDecode> decode_info;
  std::vector<Engine::Window> windows;
  int lp_stride = 0;
  bool scored = false, sampled = false;
};

// One window's step, for the single-file loop and the batched one alike: clip `b` of the decode_full call that has just
// returned is the window of `fl` at fl.seek, row[0 .. n) its ids behind a fed prompt of n_prompt ids (n_context of them
// the context).  Cuts the row by the seek rule, keeps segments, scores and the window record, appends the kept ids to the
// file's context (or empties it) and advances the file.  on_segments(segs) sees the kept segments before they are
// renumbered (clip 0, id_begin behind the prompt): the word timestamps of the single-file loop.  Returns `skipped`.
template <class F>
bool seek_window_step(Engine& e, SeekFile& fl, size_t n_samples, int b, const int64_t* row, int n, int row_len, int n_context,
                      int n_prompt, F&& on_segments) {
  const VocabData& vocab = e.vocab();
  const int win_ticks = int(e.pcm_elems() / 320);
  const int seg_ticks = int(std::min<size_t>(size_t(win_ticks), (n_samples - std::min(fl.seek, n_samples) + 319) / 320));
  int n_gen = 0;  // the generated ids before the first EOT
  while (n_prompt + n_gen < std::min(n, row_len) && row[size_t(n_prompt + n_gen)] != vocab.token_eot) ++n_gen;
  const int64_t* const g = row + n_prompt;
  const bool has_scores = e.scores && e.last_scores_valid && size_t(b) < e.last_scores.size();
  const bool skipped = has_scores && e.last_scores[size_t(b)].skipped;
  Engine::Window rec{int64_t(fl.seek), 0, int32_t(n_context), n_prompt, 0, skipped ? 1 : 0, 0};
  if (e.last_decode_info_valid && size_t(b) < e.last_decode_info.size()) {
    rec.temperature_milli = e.last_decode_info[size_t(b)].temperature_milli;
    fl.decode_info.push_back(e.last_decode_info[size_t(b)]);
    fl.sampled = true;
  }
  const float* const lp = has_scores ? e.last_token_logprob.data() + size_t(b) * e.last_lp_stride : nullptr;
  if (has_scores) {
    fl.scores.push_back(e.last_scores[size_t(b)]);
    fl.lp_stride = e.last_lp_stride;
    fl.token_logprob.insert(fl.token_logprob.end(), lp, lp + fl.lp_stride);
    fl.scored = true;
  }
  int advance = seg_ticks;
  std::vector<int64_t> kept;
  if (!skipped) {
    std::vector<Segment> segs;
    advance = seek_step(vocab, g, n_gen, win_ticks, seg_ticks, &segs);
    on_segments(segs);
    for (Segment sg : segs) {
      kept.insert(kept.end(), g + sg.id_begin, g + sg.id_begin + sg.id_count);
      sg.clip = fl.w;
      sg.id_begin += n_prompt;  // an index into the window's id row
      sg.t0_ms += int32_t(fl.seek / 16), sg.t1_ms += int32_t(fl.seek / 16);
      fl.segments.push_back(sg);
      fl.segment_text.push_back(decode_tokens(vocab, row + sg.id_begin, sg.id_count, false, nullptr));
      if (has_scores) {  // the mean log-probability of the segment's ids below EOT
        double sum = 0.0;
        int cnt = 0;
        for (int k = 0; k < sg.id_count; ++k) {
          if (row[size_t(sg.id_begin + k)] < vocab.token_eot) sum += double(lp[size_t(sg.id_begin + k)]), ++cnt;
        }
        fl.segment_score.push_back(float(sum / double(std::max(cnt, 1))));
      }
    }
  }
  if (fl.w) fl.text += '\n';
  fl.text += decode_tokens(vocab, kept.data(), int(kept.size()), false, nullptr);
  fl.ctx.insert(fl.ctx.end(), kept.begin(), kept.end());
  if (!skipped && (!e.condition_on_previous_text || rec.temperature_milli > 500)) fl.ctx.clear();
  if (fl.ctx.size() > size_t(Engine::kContextIdsMax)) fl.ctx.erase(fl.ctx.begin(), fl.ctx.end() - Engine::kContextIdsMax);
  rec.advance_samples = advance * 320;
  rec.n_kept_ids = int32_t(kept.size());
  fl.windows.push_back(rec);
  fl.seek += size_t(advance) * 320;
  ++fl.w;
  return skipped;
}

}  // namespace

void transcribe_seek(Engine& e, const float* pcm, size_t n_samples, std::string* text) {
  if (!e.timestamps || e.max_positions <= 0) {
    throw Error(kErrUnsupported, "seek: needs the options timestamps = 1 and max_positions (32 .. n_text_ctx)");
  }
  e.check_word_call();
  if (e.condition_on_previous_text && !e.has_prev_token()) {
    throw Error(kErrUnsupported, "seek: condition_on_previous_text needs a vocabulary with <|startofprev|> and an EncDec engine");
  }
  const size_t win = e.pcm_elems();
  struct Restore {  // the caller's contexts and clip index come back however the loop ends
    Engine& e;
    std::vector<long long> context;
    std::vector<std::vector<long long>> clip_contexts;
    ~Restore() { e.context_ids = context, e.clip_contexts = clip_contexts, e.clip_base = 0, e.defer_word_alignment = false; }
  } restore{e, e.context_ids, e.clip_contexts};
  e.clip_contexts.clear();  // (per-clip contexts belong to the caller's own full-length calls, not to this loop)
  SeekFile fl;
  fl.ctx.assign(e.context_ids.begin(), e.context_ids.end());
  std::vector<Engine::Word> words;  // option word_timestamps: every window's, aligned over the segments seek_step kept
  std::vector<std::string> word_text;
  std::vector<Engine::ClipAlignment> kept_alignment;
  e.defer_word_alignment = true;  // decode_full leaves the id row; the pass runs below, once the kept segments are known
  const size_t row = size_t(e.max_positions) + 1;
  std::vector<int64_t> ids(row);
  std::vector<float> clip(win);
  do {
    const size_t have = fl.seek < n_samples ? std::min(win, n_samples - fl.seek) : 0;
    std::fill(clip.begin(), clip.end(), 0.0f);
    if (have) std::memcpy(clip.data(), pcm + fl.seek, have * sizeof(float));
    e.set_context(fl.ctx.data(), int(fl.ctx.size()));
    float* d_pcm = e.staging_pcm(1);
    float* d_mel = e.staging_mel(1);
    if (hipMemcpyAsync(d_pcm, clip.data(), win * sizeof(float), hipMemcpyHostToDevice, e.stream()) != hipSuccess) {
      throw Error(kErrDevice, "H2D pcm");
    }
    e.logmel(d_pcm, 1, d_mel);
    e.encode_full(d_mel, 1);
    e.clip_base = fl.w;
    int32_t n = 0;
    e.decode_full(1, ids.data(), int(row), &n);
    e.sync();  // clip[] is read by the H2D copy on the encoder stream
    const int n_prompt = int(e.fed_prompt().size());
    const int w = fl.w;
    const size_t seek = fl.seek;
    const bool skipped = seek_window_step(e, fl, n_samples, 0, ids.data(), n, int(row), int(e.context_ids.size()), n_prompt,
                                          [&](const std::vector<Segment>& segs) {
      if (!e.word_timestamps) return;  // the window's words: clip = window, times in the file, segment = index in the whole call
      std::vector<Segment> in_row = segs;
      for (Segment& sg : in_row) sg.clip = 0, sg.id_begin += n_prompt;
      e.last_alignment.clear();
      e.align_words(1, in_row, std::vector<long long>{(long long)have});
      for (Engine::Word wd : e.last_words) {
        wd.clip = w;
        wd.segment += int(fl.segments.size());
        wd.t0_ms += int32_t(seek / 16), wd.t1_ms += int32_t(seek / 16);
        words.push_back(wd);
      }
      word_text.insert(word_text.end(), e.last_word_text.begin(), e.last_word_text.end());
    });
    if (e.word_timestamps && e.keep_alignment) {  // one record per window, empty for a window without words
      kept_alignment.push_back(!skipped && !e.last_alignment.empty() ? e.last_alignment.back() : Engine::ClipAlignment());
    }
  } while (fl.seek < n_samples);
  *text = fl.text;
  e.last_segments = fl.segments, e.last_segment_text = fl.segment_text, e.last_segments_valid = true;
  if (fl.scored) {
    e.last_scores = fl.scores, e.last_token_logprob = fl.token_logprob, e.last_segment_score = fl.segment_score;
    e.last_lp_stride = fl.lp_stride, e.last_scores_valid = true;
  }
  if (fl.sampled) e.last_decode_info = fl.decode_info, e.last_decode_info_valid = true;
  e.last_windows = fl.windows, e.last_windows_valid = true;
  if (e.word_timestamps) {
    e.last_words = words, e.last_word_text = word_text, e.last_words_valid = true;
    e.last_alignment = kept_alignment;
  }
}

void transcribe_seek_batch(Engine& e, const float* const* pcm, const size_t* n_samples, int n_files) {
  if (n_files < 1) throw Error(kErrInvalidArg, "batched seek: needs at least one file");
  if (n_files > 64) throw Error(kErrUnsupported, "batched seek: at most 64 files per call");
  if (!e.timestamps || e.max_positions <= 0) {
    throw Error(kErrUnsupported, "batched seek: needs the options timestamps = 1 and max_positions (32 .. n_text_ctx)");
  }
  if (e.word_timestamps) throw Error(kErrUnsupported, "batched seek: not with word_timestamps (the alignment pass takes one prompt length per call)");
  if (e.condition_on_previous_text && !e.has_prev_token()) {
    throw Error(kErrUnsupported, "batched seek: condition_on_previous_text needs a vocabulary with <|startofprev|> and an EncDec engine");
  }
  for (int f = 0; f < n_files; ++f) {
    if (!pcm || (!pcm[f] && n_samples[f])) throw Error(kErrInvalidArg, "batched seek: NULL pcm");
  }
  const size_t win = e.pcm_elems();
  struct Restore {  // the caller's contexts and clip indices come back however the loop ends
    Engine& e;
    std::vector<long long> context;
    std::vector<std::vector<long long>> clip_contexts;
    ~Restore() { e.context_ids = context, e.clip_contexts = clip_contexts, e.clip_base = 0, e.clip_index_off.clear(); }
  } restore{e, e.context_ids, e.clip_contexts};
  std::vector<SeekFile> files(static_cast<size_t>(n_files));
  std::vector<bool> done(static_cast<size_t>(n_files), false);
  for (SeekFile& fl : files) fl.ctx.assign(e.context_ids.begin(), e.context_ids.end());  // the caller's context seeds every file
  const size_t row = size_t(e.max_positions) + 1;
  e.clip_base = 0;
  std::vector<int> active;
  std::vector<float> clips;
  std::vector<int64_t> ids, flat;
  std::vector<int32_t> n_ids, offsets;
  for (;;) {
    active.clear();
    for (int f = 0; f < n_files; ++f) {
      if (!done[size_t(f)]) active.push_back(f);
    }
    if (active.empty()) break;
    const int B = int(active.size());
    clips.assign(size_t(B) * win, 0.0f);
    flat.clear();
    offsets.assign(1, 0);
    e.clip_index_off.assign(size_t(B), 0);
    for (int b = 0; b < B; ++b) {
      const SeekFile& fl = files[size_t(active[size_t(b)])];
      const size_t ns = n_samples[active[size_t(b)]];
      const size_t have = fl.seek < ns ? std::min(win, ns - fl.seek) : 0;
      if (have) std::memcpy(&clips[size_t(b) * win], pcm[active[size_t(b)]] + fl.seek, have * sizeof(float));
      flat.insert(flat.end(), fl.ctx.begin(), fl.ctx.end());
      offsets.push_back(int32_t(flat.size()));
      e.clip_index_off[size_t(b)] = fl.w - b;  // window w of a file has clip index w in the sampler's counter
    }
    e.set_contexts(flat.data(), offsets.data(), B);
    float* d_pcm = e.staging_pcm(B);
    float* d_mel = e.staging_mel(B);
    if (hipMemcpyAsync(d_pcm, clips.data(), clips.size() * sizeof(float), hipMemcpyHostToDevice, e.stream()) != hipSuccess) {
      throw Error(kErrDevice, "H2D pcm");
    }
    e.logmel(d_pcm, B, d_mel);
    e.encode_full(d_mel, B);
    ids.assign(size_t(B) * row, 0);
    n_ids.assign(size_t(B), 0);
    e.decode_full(B, ids.data(), int(row), n_ids.data());
    e.sync();  // clips[] is read by the H2D copy on the encoder stream
    for (int b = 0; b < B; ++b) {
      const int f = active[size_t(b)];
      seek_window_step(e, files[size_t(f)], n_samples[f], b, ids.data() + size_t(b) * row, n_ids[size_t(b)], int(row),
                       int(e.clip_contexts[size_t(b)].size()), int(e.fed_prompt_of(b).size()), [](const std::vector<Segment>&) {});
      done[size_t(f)] = !(files[size_t(f)].seek < n_samples[f]);
    }
  }
  // the windows file by file
  e.last_segments.clear(), e.last_segment_text.clear();
  e.last_scores.clear(), e.last_token_logprob.clear(), e.last_segment_score.clear();
  e.last_decode_info.clear(), e.last_windows.clear(), e.last_window_files.clear(), e.last_file_text.clear();
  bool scored = false, sampled = false;
  int lp_stride = 0;
  for (int f = 0; f < n_files; ++f) {
    const SeekFile& fl = files[size_t(f)];
    const int base = int(e.last_windows.size());
    for (Segment sg : fl.segments) {
      sg.clip += base;
      e.last_segments.push_back(sg);
    }
    e.last_segment_text.insert(e.last_segment_text.end(), fl.segment_text.begin(), fl.segment_text.end());
    e.last_scores.insert(e.last_scores.end(), fl.scores.begin(), fl.scores.end());
    e.last_token_logprob.insert(e.last_token_logprob.end(), fl.token_logprob.begin(), fl.token_logprob.end());
    e.last_segment_score.insert(e.last_segment_score.end(), fl.segment_score.begin(), fl.segment_score.end());
    e.last_decode_info.insert(e.last_decode_info.end(), fl.decode_info.begin(), fl.decode_info.end());
    e.last_windows.insert(e.last_windows.end(), fl.windows.begin(), fl.windows.end());
    e.last_window_files.insert(e.last_window_files.end(), fl.windows.size(), f);
    e.last_file_text.push_back(fl.text);
    scored = scored || fl.scored, sampled = sampled || fl.sampled;
    if (fl.scored) lp_stride = fl.lp_stride;
  }
  e.last_segments_valid = true;
  e.last_lp_stride = scored ? lp_stride : 0, e.last_scores_valid = scored;
  e.last_decode_info_valid = sampled;
  e.last_windows_valid = true;
}

}  // namespace wt
