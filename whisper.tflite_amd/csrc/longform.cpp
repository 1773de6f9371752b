// Seeking long-audio transcription: the host side of DESIGN section 20 (longform.h).
#include "longform.h"

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

// The loops below set the engine's contexts and clip numbering window by window.  However one ends, the caller's two
// kinds of context come back, and the clip numbering and the deferred alignment are off again (cleared, not restored).
struct LoopScope {
  Engine& e;
  std::vector<long long> context = e.context_ids;
  std::vector<std::vector<long long>> clip_contexts = e.clip_contexts;
  ~LoopScope() {
    e.context_ids = std::move(context), e.clip_contexts = std::move(clip_contexts);
    e.clip_base = 0, e.clip_index_off.clear(), e.defer_word_alignment = false;
    e.clip_lang_hold.clear(), e.clip_lang_hold_prob.clear();
  }
};

// option full_language: Whisper's transcribe() detects one language per file, on the file's first
// window, and decodes every window behind it.  The first windows of the n files go through one detection pass; the
// loops then hold each file's language (Engine::clip_lang_hold) for every window they decode.
void detect_files(Engine& e, const float* const* pcm, const size_t* n_samples, int n_files, std::vector<int32_t>* lang,
                  std::vector<float>* prob) {
  const size_t win = e.pcm_elems();
  std::vector<float> clips(size_t(n_files) * win, 0.0f);
  for (int f = 0; f < n_files; ++f) {
    const size_t have = std::min(win, n_samples[f]);
    if (have) std::memcpy(&clips[size_t(f) * win], pcm[f], have * sizeof(float));
  }
  lang->assign(size_t(n_files), 0);
  prob->assign(size_t(n_files), 0.0f);
  e.detect_windows(clips.data(), n_files, lang->data(), prob->data());
}

// What a seeking loop carries for one file, and what the file leaves for Engine::last
struct SeekFile {
  std::vector<int64_t> ctx;  // the ids kept so far: the next window's context
  size_t seek = 0;
  int w = 0;                 // windows decoded
  std::string text;          // the windows' lines, joined by '\n'
  DecodeResults results;     // one entry per window: clip = the window's index in the file, times in the file
};

// One window's step, for the single-file loop and the batched one alike: clip `b` of the decode_full call that has just
// returned, read from e.last, is the window of `fl` at fl.seek; row[0 .. n) its ids behind a fed prompt of n_prompt ids
// (n_context of them the context).  Cuts the row by the seek rule, keeps segments, scores and the window record in
// fl.results, appends the kept ids to the file's context (or empties it) and advances the file.  on_segments(segs) sees
// the kept segments before they are renumbered (clip 0, id_begin behind the prompt): the word timestamps of the
// single-file loop.  Returns `skipped`.
template <class F>
bool seek_window_step(Engine& e, SeekFile& fl, size_t n_samples, int b, const int64_t* row, int n, int row_len, int n_context,
                      int n_prompt, F&& on_segments) {
  const VocabData& vocab = e.vocab();
  const int win_ticks = int(e.pcm_elems() / 320);
  const int seg_ticks = int(std::min<size_t>(size_t(win_ticks), (n_samples - std::min(fl.seek, n_samples) + 319) / 320));
  int n_gen = 0;  // the generated ids before the first EOT
  while (n_prompt + n_gen < std::min(n, row_len) && row[size_t(n_prompt + n_gen)] != vocab.token_eot) ++n_gen;
  const int64_t* const g = row + n_prompt;
  const bool has_scores = e.scores && e.last.scores_valid && size_t(b) < e.last.scores.size();
  const bool skipped = has_scores && e.last.scores[size_t(b)].skipped;
  Window rec{int64_t(fl.seek), 0, int32_t(n_context), n_prompt, 0, skipped ? 1 : 0, 0};
  DecodeResults& out = fl.results;
  if (e.last.decode_info_valid && size_t(b) < e.last.decode_info.size()) {
    rec.temperature_milli = e.last.decode_info[size_t(b)].temperature_milli;
    out.decode_info.push_back(e.last.decode_info[size_t(b)]);
    out.decode_info_valid = true;
  }
  if (e.last.lang_valid && size_t(b) < e.last.lang.size()) {  // full_language: the window carries its file's language
    out.lang.push_back(e.last.lang[size_t(b)]);
    out.lang_prob.push_back(e.last.lang_prob[size_t(b)]);
    out.lang_valid = true;
  }
  const float* const lp = has_scores ? e.last.token_logprob.data() + size_t(b) * e.last.lp_stride : nullptr;
  if (has_scores) {
    out.scores.push_back(e.last.scores[size_t(b)]);
    out.lp_stride = e.last.lp_stride;
    out.token_logprob.insert(out.token_logprob.end(), lp, lp + out.lp_stride);
    out.scores_valid = true;
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
      out.segments.push_back(sg);
      out.segment_text.push_back(decode_tokens(vocab, row + sg.id_begin, sg.id_count, false, nullptr));
      if (has_scores) {  // the mean log-probability of the segment's ids below EOT
        double sum = 0.0;
        int cnt = 0;
        for (int k = 0; k < sg.id_count; ++k) {
          if (row[size_t(sg.id_begin + k)] < vocab.token_eot) sum += double(lp[size_t(sg.id_begin + k)]), ++cnt;
        }
        out.segment_score.push_back(float(sum / double(std::max(cnt, 1))));
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
  out.windows.push_back(rec);
  out.segments_valid = out.windows_valid = true;
  fl.seek += size_t(advance) * 320;
  ++fl.w;
  return skipped;
}

}  // namespace

void transcribe_windows(Engine& e, const float* pcm, size_t n_samples, std::string* text) {
  const size_t win = e.pcm_elems();
  const size_t n_win = std::max<size_t>(1, (n_samples + win - 1) / win);
  const bool full = e.max_positions > 0;
  LoopScope scope{e};
  DecodeResults acc;  // every window's results: clip = window index, times in the file
  std::vector<float> clips;
  std::vector<long long> valid;  // word timestamps: every window's own samples
  std::vector<int64_t> ids;
  std::vector<int32_t> n;
  std::vector<int32_t> file_lang;
  std::vector<float> file_prob;
  if (e.auto_full()) detect_files(e, &pcm, &n_samples, 1, &file_lang, &file_prob);
  for (size_t w0 = 0; w0 < n_win; w0 += 32) {
    const int B = int(std::min<size_t>(32, n_win - w0));
    if (!file_lang.empty()) e.clip_lang_hold.assign(size_t(B), file_lang[0]), e.clip_lang_hold_prob.assign(size_t(B), file_prob[0]);
    clips.assign(size_t(B) * win, 0.0f);
    valid.assign(size_t(B), 0);
    for (int b = 0; b < B; ++b) {
      const size_t off = (w0 + b) * win;
      if (off >= n_samples) continue;
      valid[size_t(b)] = (long long)std::min(win, n_samples - off);
      std::memcpy(&clips[size_t(b) * win], pcm + off, size_t(valid[size_t(b)]) * sizeof(float));
    }
    if (full) e.clip_base = long(w0);  // a window's Philox clip index is its index in the file, however the windows are batched
    e.decode_windows(clips.data(), B, &valid, &ids, &n);
    acc.forget(kResBeam | kResAlignment);  // (these two have always reported the file's last batch alone)
    acc.append(e.last, B, {int(w0), int(acc.segments.size()), kWindowMs});
    const bool scored = full && e.scores && e.last.scores_valid && e.last.scores.size() == size_t(B);  // THIS batch ran with scores
    const size_t row = ids.size() / size_t(B);
    for (int b = 0; b < B; ++b) {
      if (w0 + b) *text += '\n';
      if (scored && e.last.scores[size_t(b)].skipped) continue;  // option skip_silence: an empty line
      *text += decode_tokens(e.vocab(), &ids[size_t(b) * row], n[size_t(b)], false, nullptr);
    }
  }
  e.last = std::move(acc);
}

void transcribe_seek(Engine& e, const float* pcm, size_t n_samples, std::string* text) {
  if (!e.timestamps || e.max_positions <= 0) {
    throw Error(kErrUnsupported, "seek: needs the options timestamps = 1 and max_positions (32 .. n_text_ctx)");
  }
  e.check_word_call();
  if (e.condition_on_previous_text && !e.has_prev_token()) {
    throw Error(kErrUnsupported, "seek: condition_on_previous_text needs a vocabulary with <|startofprev|> and an EncDec engine");
  }
  const size_t win = e.pcm_elems();
  LoopScope scope{e};
  e.clip_contexts.clear();  // (per-clip contexts belong to the caller's own full-length calls, not to this loop)
  SeekFile fl;
  fl.ctx.assign(e.context_ids.begin(), e.context_ids.end());
  e.defer_word_alignment = true;  // decode_full leaves the id row; the pass runs below, once the kept segments are known
  std::vector<int64_t> ids;
  std::vector<int32_t> n;
  std::vector<float> clip(win);
  if (e.auto_full()) {
    std::vector<int32_t> file_lang;
    std::vector<float> file_prob;
    detect_files(e, &pcm, &n_samples, 1, &file_lang, &file_prob);
    e.clip_lang_hold.assign(1, file_lang[0]), e.clip_lang_hold_prob.assign(1, file_prob[0]);
  }
  do {
    const size_t have = fl.seek < n_samples ? std::min(win, n_samples - fl.seek) : 0;
    std::fill(clip.begin(), clip.end(), 0.0f);
    if (have) std::memcpy(clip.data(), pcm + fl.seek, have * sizeof(float));
    e.set_context(fl.ctx.data(), int(fl.ctx.size()));
    e.clip_base = fl.w;
    e.decode_windows(clip.data(), 1, nullptr, &ids, &n);  // (no valid samples: the alignment below takes `have`)
    const int n_prompt = int(e.fed_prompt().size());
    const int w = fl.w;
    const size_t seek = fl.seek;
    const bool skipped = seek_window_step(e, fl, n_samples, 0, ids.data(), n[0], int(ids.size()), int(e.context_ids.size()), n_prompt,
                                          [&](const std::vector<Segment>& segs) {
      if (!e.word_timestamps) return;  // the window's words: clip = window, times in the file, segment = index in the whole call
      std::vector<Segment> in_row = segs;
      for (Segment& sg : in_row) sg.clip = 0, sg.id_begin += n_prompt;
      e.last.alignment.clear();
      e.align_words(1, in_row, std::vector<long long>{(long long)have});
      for (Word wd : e.last.words) {
        wd.clip = w;
        wd.segment += int(fl.results.segments.size());
        wd.t0_ms += int32_t(seek / 16), wd.t1_ms += int32_t(seek / 16);
        fl.results.words.push_back(wd);
      }
      fl.results.word_text.insert(fl.results.word_text.end(), e.last.word_text.begin(), e.last.word_text.end());
    });
    fl.results.words_valid = e.word_timestamps != 0;
    if (e.word_timestamps && e.keep_alignment) {  // one record per window, empty for a window without words
      fl.results.alignment.push_back(!skipped && !e.last.alignment.empty() ? e.last.alignment.back() : ClipAlignment());
    }
  } while (fl.seek < n_samples);
  *text = fl.text;
  e.last = std::move(fl.results);
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
  LoopScope scope{e};
  std::vector<SeekFile> files(static_cast<size_t>(n_files));
  std::vector<bool> done(static_cast<size_t>(n_files), false);
  for (SeekFile& fl : files) fl.ctx.assign(e.context_ids.begin(), e.context_ids.end());  // the caller's context seeds every file
  e.clip_base = 0;
  std::vector<int32_t> file_lang;
  std::vector<float> file_prob;
  if (e.auto_full()) detect_files(e, pcm, n_samples, n_files, &file_lang, &file_prob);
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
    if (!file_lang.empty()) {
      e.clip_lang_hold.assign(size_t(B), 0), e.clip_lang_hold_prob.assign(size_t(B), 0.0f);
      for (int b = 0; b < B; ++b) {
        e.clip_lang_hold[size_t(b)] = file_lang[size_t(active[size_t(b)])];
        e.clip_lang_hold_prob[size_t(b)] = file_prob[size_t(active[size_t(b)])];
      }
    }
    e.set_contexts(flat.data(), offsets.data(), B);
    e.decode_windows(clips.data(), B, nullptr, &ids, &n_ids);
    const size_t row = ids.size() / size_t(B);
    for (int b = 0; b < B; ++b) {
      const int f = active[size_t(b)];
      seek_window_step(e, files[size_t(f)], n_samples[f], b, ids.data() + size_t(b) * row, n_ids[size_t(b)], int(row),
                       int(e.clip_contexts[size_t(b)].size()), int(e.fed_prompt_of(b).size()), [](const std::vector<Segment>&) {});
      done[size_t(f)] = !(files[size_t(f)].seek < n_samples[f]);
    }
  }
  DecodeResults all;  // the windows file by file: Segment::clip an index into the whole list
  for (int f = 0; f < n_files; ++f) {
    SeekFile& fl = files[size_t(f)];
    fl.results.window_files.assign(fl.results.windows.size(), f);
    fl.results.file_text.assign(1, fl.text);
    all.append(fl.results, fl.w, {int(all.windows.size()), 0, 0});
  }
  e.last = std::move(all);
}

}  // namespace wt
