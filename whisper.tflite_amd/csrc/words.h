// Word-level timestamps, the host side: Whisper's split_to_word_tokens and merge_punctuations on
// the vocabulary's bytes, and the dynamic time warping of find_alignment as a plain fp32 function.  No engine, no GPU:
// wt_vocab_split_words, wt_vocab_merge_punctuation and wt_dtw_path (include/wt_capi.h) are these functions.
#pragma once
#include <cstdint>
#include <vector>

#include "host_util.h"

namespace wt {

// The code points of `n` bytes read as UTF-8 with every ill-formed sequence replaced by ONE U+FFFD per maximal
// subpart (Unicode 3.9, what Python's bytes.decode("utf-8", "replace") yields, which Whisper's tokenizer calls).
std::vector<uint32_t> decode_utf8_replace(const unsigned char* s, size_t n);

// Whisper's split_tokens_on_unicode: ids are accumulated and a group is closed when the decoded group has no U+FFFD, or
// when the decoded whole row has a U+FFFD at the place of the group's first one (a token that really holds that
// character, or a sequence the row never completes).  An id without a vocabulary entry has no bytes.  Ids that are
// still open at the end of the row form a last group, so the counts always add up to n.
std::vector<int> split_unicode(const VocabData& vocab, const int64_t* ids, int n);

// Whisper's split_to_word_tokens: the id counts of the row's words, in order (they add up to n).  unicode_only: the
// groups of split_unicode are the words (languages written without spaces).  Otherwise a group starts a word when it
// is the first one, its first id is >= eot, its bytes begin with a space, or its bytes without leading and trailing
// ASCII white space are a single ASCII punctuation character; every other group joins the word before it.
std::vector<int> split_words(const VocabData& vocab, const int64_t* ids, int n, bool unicode_only);

// Whisper's merge_punctuations on the words word_len[0 .. n_words) of a row (counts adding up to n).  From the back, a
// word that begins with a space and is otherwise one of  " ' “ ¿ ( [ { -  goes in front of the word behind it; then from
// the front a word that is exactly one of  " ' . 。 , ， ! ！ ? ？ : ： ” ) ] } 、  goes behind the word before it unless
// that one ends in a space.  Returns the id counts of the merged words, in order; they still add up to n.
std::vector<int> merge_punctuation(const VocabData& vocab, const int64_t* ids, int n, const int* word_len, int n_words);

// find_alignment's dynamic time warping over cost [N][F] (row stride ld), in fp32 with this recurrence: D[0][0] = 0,
// D[0][j > 0] = D[i > 0][0] = +inf, D[i][j] = cost[i - 1][j - 1] + min(c0, c1, c2) with c0 = D[i - 1][j - 1], c1 =
// D[i - 1][j], c2 = D[i][j - 1]; trace = 0 if c0 < c1 and c0 < c2, else 1 if c1 < c0 and c1 < c2, else 2; the path runs
// back from (N, F) by 0: (i - 1, j - 1), 1: (i - 1, j), 2: (i, j - 1).  jump[i] = the first frame of the path in row i.
// path, when given, receives the (row, frame) pairs from (0, 0) to (N - 1, F - 1); trace, when given, the codes of the
// cells [N][F].  Returns the number of path cells (at most N + F - 1).
int dtw_path(const float* cost, int N, int F, long ld, int32_t* jump, std::vector<int32_t>* path, unsigned char* trace);

}  // namespace wt
