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

void transcribe_seek(Engine& e, const float* pcm, size_t n_samples, std::string* text) {
  if (!e.timestamps || e.max_positions <= 0) {
    throw Error(kErrUnsupported, "seek: needs the options timestamps = 1 and max_positions (32 .. n_text_ctx)");
  }
  e.check_word_call();
  if (e.condition_on_previous_text && !e.has_prev_token()) {
    throw Error(kErrUnsupported, "seek: condition_on_previous_text needs a vocabulary with <|startofprev|> and an EncDec engine");
  }
  const size_t win = e.pcm_elems();
  const int win_ticks = int(win / 320);
  const VocabData& vocab = e.vocab();
  struct Restore {  // the caller's context and clip index come back however the loop ends
    Engine& e;
    std::vector<long long> context;
    ~Restore() { e.context_ids = context, e.clip_base = 0, e.defer_word_alignment = false; }
  } restore{e, e.context_ids};
  std::vector<int64_t> ctx(e.context_ids.begin(), e.context_ids.end());
  std::vector<Segment> segments;
  std::vector<std::string> segment_text;
  std::vector<ClipScore> scores;
  std::vector<float> token_logprob, segment_score;
  std::vector<Engine::ClipDecode> decode_info;
  std::vector<Engine::Window> windows;
  std::vector<Engine::Word> words;  // option word_timestamps: every window's, aligned over the segments seek_step kept
  std::vector<std::string> word_text;
  std::vector<Engine::ClipAlignment> kept_alignment;
  e.defer_word_alignment = true;  // decode_full leaves the id row; the pass runs below, once the kept segments are known
  const size_t row = size_t(e.max_positions) + 1;
  std::vector<int64_t> ids(row);
  std::vector<float> clip(win);
  bool scored = false, sampled = false;
  int lp_stride = 0;
  size_t seek = 0;
  int w = 0;
  text->clear();
  do {
    const size_t have = seek < n_samples ? std::min(win, n_samples - seek) : 0;
    std::fill(clip.begin(), clip.end(), 0.0f);
    if (have) std::memcpy(clip.data(), pcm + seek, have * sizeof(float));
    const int seg_ticks = int(std::min<size_t>(size_t(win_ticks), (n_samples - std::min(seek, n_samples) + 319) / 320));
    e.set_context(ctx.data(), int(ctx.size()));
    float* d_pcm = e.staging_pcm(1);
    float* d_mel = e.staging_mel(1);
    if (hipMemcpyAsync(d_pcm, clip.data(), win * sizeof(float), hipMemcpyHostToDevice, e.stream()) != hipSuccess) {
      throw Error(kErrDevice, "H2D pcm");
    }
    e.logmel(d_pcm, 1, d_mel);
    e.encode_full(d_mel, 1);
    e.clip_base = w;
    int32_t n = 0;
    e.decode_full(1, ids.data(), int(row), &n);
    e.sync();  // clip[] is read by the H2D copy on the encoder stream
    const int n_prompt = int(e.fed_prompt().size());
    int n_gen = 0;  // the generated ids before the first EOT
    while (n_prompt + n_gen < std::min<int>(n, int(row)) && ids[size_t(n_prompt + n_gen)] != vocab.token_eot) ++n_gen;
    const int64_t* const g = ids.data() + n_prompt;
    const bool has_scores = e.scores && e.last_scores_valid && e.last_scores.size() == 1;
    const bool skipped = has_scores && e.last_scores[0].skipped;
    Engine::Window rec{int64_t(seek), 0, int32_t(e.context_ids.size()), n_prompt, 0, skipped ? 1 : 0, 0};
    if (e.last_decode_info_valid && !e.last_decode_info.empty()) {
      rec.temperature_milli = e.last_decode_info[0].temperature_milli;
      decode_info.push_back(e.last_decode_info[0]);
      sampled = true;
    }
    if (has_scores) {
      scores.push_back(e.last_scores[0]);
      lp_stride = e.last_lp_stride;
      token_logprob.insert(token_logprob.end(), e.last_token_logprob.begin(), e.last_token_logprob.begin() + lp_stride);
      scored = true;
    }
    int advance = seg_ticks;
    std::vector<int64_t> kept;
    if (!skipped) {
      std::vector<Segment> segs;
      advance = seek_step(vocab, g, n_gen, win_ticks, seg_ticks, &segs);
      if (e.word_timestamps) {  // the window's words: clip = window, times in the file, segment = index in the whole call
        std::vector<Segment> in_row = segs;
        for (Segment& sg : in_row) sg.clip = 0, sg.id_begin += n_prompt;
        e.last_alignment.clear();
        e.align_words(1, in_row, std::vector<long long>{(long long)have});
        for (Engine::Word wd : e.last_words) {
          wd.clip = w;
          wd.segment += int(segments.size());
          wd.t0_ms += int32_t(seek / 16), wd.t1_ms += int32_t(seek / 16);
          words.push_back(wd);
        }
        word_text.insert(word_text.end(), e.last_word_text.begin(), e.last_word_text.end());
      }
      for (Segment sg : segs) {
        kept.insert(kept.end(), g + sg.id_begin, g + sg.id_begin + sg.id_count);
        sg.clip = w;
        sg.id_begin += n_prompt;  // an index into the window's id row
        sg.t0_ms += int32_t(seek / 16), sg.t1_ms += int32_t(seek / 16);
        segments.push_back(sg);
        segment_text.push_back(decode_tokens(vocab, ids.data() + sg.id_begin, sg.id_count, false, nullptr));
        if (has_scores) {  // the mean log-probability of the segment's ids below EOT
          double sum = 0.0;
          int cnt = 0;
          for (int k = 0; k < sg.id_count; ++k) {
            if (ids[size_t(sg.id_begin + k)] < vocab.token_eot) sum += double(e.last_token_logprob[size_t(sg.id_begin + k)]), ++cnt;
          }
          segment_score.push_back(float(sum / double(std::max(cnt, 1))));
        }
      }
    }
    if (w) *text += '\n';
    *text += decode_tokens(vocab, kept.data(), int(kept.size()), false, nullptr);
    ctx.insert(ctx.end(), kept.begin(), kept.end());
    if (!skipped && (!e.condition_on_previous_text || rec.temperature_milli > 500)) ctx.clear();
    if (ctx.size() > size_t(Engine::kContextIdsMax)) ctx.erase(ctx.begin(), ctx.end() - Engine::kContextIdsMax);
    if (e.word_timestamps && e.keep_alignment) {  // one record per window, empty for a window without words
      kept_alignment.push_back(!skipped && !e.last_alignment.empty() ? e.last_alignment.back() : Engine::ClipAlignment());
    }
    rec.advance_samples = advance * 320;
    rec.n_kept_ids = int32_t(kept.size());
    windows.push_back(rec);
    seek += size_t(advance) * 320;
    ++w;
  } while (seek < n_samples);
  e.last_segments = segments, e.last_segment_text = segment_text, e.last_segments_valid = true;
  if (scored) {
    e.last_scores = scores, e.last_token_logprob = token_logprob, e.last_segment_score = segment_score;
    e.last_lp_stride = lp_stride, e.last_scores_valid = true;
  }
  if (sampled) e.last_decode_info = decode_info, e.last_decode_info_valid = true;
  e.last_windows = windows, e.last_windows_valid = true;
  if (e.word_timestamps) {
    e.last_words = words, e.last_word_text = word_text, e.last_words_valid = true;
    e.last_alignment = kept_alignment;
  }
}

}  // namespace wt
