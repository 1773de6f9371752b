// Host check of DecodeResults::append / forget (csrc/decode_results.h) under the sanitizers; no GPU, no engine:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iwhisper.tflite_amd/csrc
//       tools/decode_results_check.cpp whisper.tflite_amd/csrc/decode_results.cpp -o decode_results_check
// (one command) and run ./decode_results_check.
// Two batches by hand — a scored one of 2 clips, then one of 3 clips without best-of rows — appended behind 32 clips.
#include <cstdio>
#include <cstdlib>

#include "decode_results.h"

using namespace wt;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

static DecodeResults batch(int clips, bool scored, bool best_of) {
  DecodeResults b;
  for (int c = 0; c < clips; ++c) {
    b.lang.push_back(c), b.lang_prob.push_back(0.5f);
    b.beam_sum.push_back(-1.0f * c), b.beam_len.push_back(c + 1);
    b.segments.push_back(Segment{c, 100, 200, 3, 4, 0}), b.segment_text.push_back("s");
    b.words.push_back(Word{c, c, 100, 150, 3, 1, 0.5f}), b.word_text.push_back("w");
    b.decode_info.push_back(ClipDecode{200, 2, 0, 1.5f});
    b.alignment.emplace_back();
    b.windows.push_back(Window{c * 1000, 1000, 0, 3, 4, 0, 0}), b.window_files.push_back(0);
    if (scored) b.scores.push_back(ClipScore{-2.0f, -0.5f, 0.1f, 4, 0}), b.segment_score.push_back(-0.5f);
    if (scored) b.token_logprob.insert(b.token_logprob.end(), 5, -0.25f);
    if (best_of) b.picked.push_back(1), b.best_of_sum.resize(b.best_of_sum.size() + kBestOfSlots, -3.0), b.best_of_count.resize(b.best_of_count.size() + kBestOfSlots, 7);
  }
  b.file_text.push_back("file");
  b.lang_valid = b.beam_valid = b.segments_valid = b.words_valid = b.decode_info_valid = b.windows_valid = true;
  b.scores_valid = scored, b.lp_stride = scored ? 5 : 0, b.best_of_valid = best_of;
  return b;
}

int main() {
  DecodeResults acc;
  acc.append(batch(2, true, true), 2, {32, 0, kWindowMs});
  CHECK(acc.picked.size() == 34 && acc.picked[31] == 0 && acc.picked[33] == 1 && acc.best_of_count[32 * kBestOfSlots] == 7);
  acc.append(batch(3, false, false), 3, {34, int(acc.segments.size()), kWindowMs});
  CHECK(acc.lang_valid && acc.lang.size() == 5 && acc.lang_prob.size() == 5 && acc.beam_valid && acc.beam_sum.size() == 5 && acc.beam_len[4] == 3);
  CHECK(acc.segments_valid && acc.segments.size() == 5 && acc.segment_text.size() == 5);
  CHECK(acc.segments[1].clip == 33 && acc.segments[1].t0_ms == 100 + 33 * kWindowMs && acc.segments[4].clip == 36 && acc.segments[4].t1_ms == 200 + 36 * kWindowMs);
  CHECK(acc.words_valid && acc.words.size() == 5 && acc.word_text.size() == 5 && acc.words[1].segment == 1 && acc.words[4].segment == 2 + 2);
  CHECK(acc.words[4].clip == 36 && acc.words[4].t0_ms == 100 + 36 * kWindowMs && acc.words[4].t1_ms == 150 + 36 * kWindowMs);
  CHECK(acc.scores_valid && acc.scores.size() == 2 && acc.token_logprob.size() == 10 && acc.lp_stride == 5 && acc.segment_score.size() == 2);
  CHECK(acc.decode_info_valid && acc.decode_info.size() == 5 && acc.decode_info[4].attempts == 2);
  CHECK(acc.best_of_valid && acc.picked.size() == 37 && acc.best_of_sum.size() == 37 * size_t(kBestOfSlots) && acc.best_of_count.size() == acc.best_of_sum.size());
  CHECK(acc.picked[36] == 0 && acc.best_of_sum[36 * kBestOfSlots + 7] == 0.0 && acc.best_of_count[33 * kBestOfSlots + 7] == 7);
  CHECK(acc.alignment.size() == 5 && acc.windows_valid && acc.windows.size() == 5 && acc.window_files.size() == 5 && acc.file_text.size() == 2);
  DecodeResults wrong = batch(2, true, false);  // scores that are not one per clip of the call are not taken
  acc.append(wrong, 3, {37, 0, 0});
  CHECK(acc.scores.size() == 2 && acc.picked.size() == 40);
  acc.forget(kForgetSyncDecode);
  CHECK(acc.words_valid && acc.words.size() == 7 && acc.alignment.size() == 7 && !acc.segments_valid && acc.segments.empty());
  CHECK(!acc.lang_valid && !acc.beam_valid && !acc.scores_valid && acc.lp_stride == 0 && !acc.decode_info_valid && !acc.best_of_valid && !acc.windows_valid);
  acc.forget(kForgetFullDecode);
  CHECK(!acc.words_valid && acc.words.empty() && acc.word_text.empty() && acc.alignment.empty() && acc.file_text.empty() && acc.picked.empty());
  DecodeResults moved = batch(1, true, true);
  acc = std::move(moved);
  CHECK(acc.scores_valid && acc.scores.size() == 1);
  std::puts("decode_results_check OK");
  return 0;
}
