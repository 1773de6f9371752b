// What a decode call leaves behind for the wt_last_* getters: ONE record, Engine::last, in groups that
// are valid together.  Every entry point forgets a fixed set of groups of the call before it (the masks below), the long
// loops build a record of their own window by window (append) and install it by assignment.  Pure host code.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "host_util.h"

namespace wt {

// option scores: one clip of a full-length decode (wt_clip_score mirrors it)
struct ClipScore {
  float sum_logprob, avg_logprob, no_speech_prob;
  int32_t n_generated, skipped;
};
struct ClipDecode {  // (wt_clip_decode)
  int32_t temperature_milli, attempts, needs_fallback;
  float compression_ratio;
};
struct Word {  // (wt_word)
  int32_t clip, segment, t0_ms, t1_ms, id_begin, id_count;
  float probability;
};
struct Window {  // (wt_window)
  int64_t seek_sample;
  int32_t advance_samples, n_context, n_prompt, n_kept_ids, skipped, temperature_milli;
};
struct ClipAlignment {  // keep_alignment: what the alignment pass formed for one clip
  std::vector<long long> row;  // the L ids fed
  int n_a = 0, L = 0, N = 0, F = 0, heads = 0, T = 0;
  std::vector<float> W, C;     // [heads][L][T], [N][T]
  std::vector<int> jump;       // [N]
};

enum : unsigned {  // the groups of DecodeResults
  kResLanguage = 1u << 0, kResBeam = 1u << 1, kResSegments = 1u << 2, kResScores = 1u << 3, kResDecodeInfo = 1u << 4,
  kResBestOf = 1u << 5, kResWords = 1u << 6, kResAlignment = 1u << 7, kResWindows = 1u << 8, kResAll = (1u << 9) - 1
};
// What each entry point forgets of the call before it.  Engine::decode (the 31-position calls) leaves the words and the
// alignment tap of an earlier full-length call standing, submit / submit_pcm also its segments, beam scores and windows.
constexpr unsigned kForgetNoScores = kResScores | kResDecodeInfo | kResBestOf;  // a decode that forms none of the three
constexpr unsigned kForgetSyncDecode = kResLanguage | kResBeam | kResSegments | kResWindows | kForgetNoScores;
constexpr unsigned kForgetSubmit = kResLanguage | kForgetNoScores;
constexpr unsigned kForgetFullDecode = kResAll;
// (the long loops: every window batch is one of the calls above; their own record replaces Engine::last at the end)

constexpr int kBestOfSlots = 8;  // samples per clip a best-of row holds (kSampleGroupMax, kernels.h)

struct DecodeResults {
  // language = -1: the language used per clip and its probability
  std::vector<int> lang;
  std::vector<float> lang_prob;
  bool lang_valid = false;
  // beam search: per clip the chosen hypothesis's sum of log-probabilities and generated ids (EOT included)
  std::vector<float> beam_sum;
  std::vector<int> beam_len;
  bool beam_valid = false;
  // option timestamps: the segments of every clip (clip = index in the call; the long loops: the window) and their text
  std::vector<Segment> segments;
  std::vector<std::string> segment_text;
  bool segments_valid = false;
  // option scores: per clip; token log-probabilities [clips][lp_stride] aligned with the id rows (0 for prompt ids and
  // padding); the mean over each segment's text ids
  std::vector<ClipScore> scores;
  std::vector<float> token_logprob, segment_score;
  int lp_stride = 0;
  bool scores_valid = false;
  // per clip of a decode that sampled or ran fall-back
  std::vector<ClipDecode> decode_info;
  bool decode_info_valid = false;
  // a decode in which some clip's kept attempt ran best_of > 1 samples: per clip the kept sample, and every sample's sum
  // and count [clips][kBestOfSlots] (a clip kept from an attempt at temperature 0: sample 0, its own sum and count)
  std::vector<int32_t> picked, best_of_count;
  std::vector<double> best_of_sum;
  bool best_of_valid = false;
  // option word_timestamps (segment = index into segments)
  std::vector<Word> words;
  std::vector<std::string> word_text;
  bool words_valid = false;
  // the alignment tap: one record per clip held, no flag of its own
  std::vector<ClipAlignment> alignment;
  // a seeking call: one record per window; the batched one also the file of each and every file's text
  std::vector<Window> windows;
  std::vector<int32_t> window_files;
  std::vector<std::string> file_text;
  bool windows_valid = false;

  // drops the flag of every group in the mask and empties its vectors
  void forget(unsigned groups);
  // How append renumbers a batch: its clips follow clip0 clips already held, its words' segment indices follow segment0
  // segments, and the times of clip c move by ms_per_clip * c (c counted in the whole record)
  struct Renumber {
    int clip0 = 0, segment0 = 0, ms_per_clip = 0;
  };
  // Appends the valid groups of one decode call over n_clips clips behind what is held.  The scores are taken only from a
  // batch that holds one record per clip; a batch without best-of rows gets rows of zeros when another one has them.
  void append(const DecodeResults& batch, int n_clips, const Renumber& r);
};

}  // namespace wt
