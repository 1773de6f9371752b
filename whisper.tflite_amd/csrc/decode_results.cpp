// DecodeResults: forget and append (decode_results.h).
#include "decode_results.h"

namespace wt {

void DecodeResults::forget(unsigned groups) {
  if (groups & kResLanguage) lang.clear(), lang_prob.clear(), lang_valid = false;
  if (groups & kResBeam) beam_sum.clear(), beam_len.clear(), beam_valid = false;
  if (groups & kResSegments) segments.clear(), segment_text.clear(), segments_valid = false;
  if (groups & kResScores) scores.clear(), token_logprob.clear(), segment_score.clear(), lp_stride = 0, scores_valid = false;
  if (groups & kResDecodeInfo) decode_info.clear(), decode_info_valid = false;
  if (groups & kResBestOf) picked.clear(), best_of_sum.clear(), best_of_count.clear(), best_of_valid = false;
  if (groups & kResWords) words.clear(), word_text.clear(), words_valid = false;
  if (groups & kResAlignment) alignment.clear();
  if (groups & kResWindows) windows.clear(), window_files.clear(), file_text.clear(), windows_valid = false;
}

void DecodeResults::append(const DecodeResults& b, int n_clips, const Renumber& r) {
  auto cat = [](auto& to, const auto& from) { to.insert(to.end(), from.begin(), from.end()); };
  auto renumbered = [&r](auto x) {
    x.clip += r.clip0;
    x.t0_ms += r.ms_per_clip * x.clip, x.t1_ms += r.ms_per_clip * x.clip;
    return x;
  };
  if (b.lang_valid) cat(lang, b.lang), cat(lang_prob, b.lang_prob), lang_valid = true;
  if (b.beam_valid) cat(beam_sum, b.beam_sum), cat(beam_len, b.beam_len), beam_valid = true;
  if (b.words_valid) {
    for (Word w : b.words) {
      w.segment += r.segment0;
      words.push_back(renumbered(w));
    }
    cat(word_text, b.word_text), words_valid = true;
  }
  if (b.segments_valid) {
    for (const Segment& s : b.segments) segments.push_back(renumbered(s));
    cat(segment_text, b.segment_text), segments_valid = true;
  }
  if (b.scores_valid && b.scores.size() == size_t(n_clips)) {
    cat(scores, b.scores), cat(token_logprob, b.token_logprob), cat(segment_score, b.segment_score);
    lp_stride = b.lp_stride, scores_valid = true;
  }
  if (b.decode_info_valid) cat(decode_info, b.decode_info), decode_info_valid = true;
  if (b.best_of_valid || best_of_valid) {  // rows of zeros for the batches before this one, or for this one, that have none
    const size_t G = size_t(kBestOfSlots), rows = size_t(r.clip0) + (b.best_of_valid ? 0 : size_t(n_clips));
    picked.resize(rows, 0), best_of_sum.resize(rows * G, 0.0), best_of_count.resize(rows * G, 0);
    if (b.best_of_valid) cat(picked, b.picked), cat(best_of_sum, b.best_of_sum), cat(best_of_count, b.best_of_count), best_of_valid = true;
  }
  cat(alignment, b.alignment);
  if (b.windows_valid) cat(windows, b.windows), cat(window_files, b.window_files), cat(file_text, b.file_text), windows_valid = true;
}

}  // namespace wt
