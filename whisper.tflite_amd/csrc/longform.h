// Seeking long-audio transcription: Whisper's transcribe() loop around the window decode.  The rule
// that turns a window's generated ids into segments and the advance of the seek position is a host function of its
// own (wt_vocab_seek_step: no engine, no GPU); transcribe_seek is the loop of wt_transcribe_long_pcm with seek = 1,
// transcribe_windows the one with seek = 0.  Each loop builds a DecodeResults of its own and installs it as Engine::last.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "host_util.h"

namespace wt {

class Engine;

// g[0 .. n): the ids a window generated before its first EOT.  ts(i) = g[i] >= token_beg; tick(id) = id - token_beg
// clamped to [0, win_ticks].  Whisper's rule: with pairs of consecutive timestamps the row is cut behind the first of
// each pair (and at n when it ends in a single timestamp), every slice a segment from the tick of its first id to the
// tick of its last, and the advance is the tick of the id before the last cut (seg_ticks when the row ends in a single
// timestamp); ids behind the last cut belong to no segment.  Without a pair the whole row is one segment from 0 to the
// last timestamp's tick (to seg_ticks, open = 1, when there is none or it is tick 0) and the advance is seg_ticks.
// A segment without an id below EOT or with t0 == t1 is dropped; an advance of 0 becomes seg_ticks (Whisper's loop
// would stand still).  Appends Segment{0, t0 * 20, t1 * 20, first index, id count (timestamps included), open} to *out
// and returns the advance in ticks.
int seek_step(const VocabData& vocab, const int64_t* g, int n, int win_ticks, int seg_ticks, std::vector<Segment>* out);

// wt_transcribe_long_pcm with the option seek = 1: one window at a time, each starting where the last closed timestamp
// of the previous one left off and decoded behind the ids kept so far (condition_on_previous_text).  Leaves in
// Engine::last segments, scores, decode info and windows, one entry per window, and the engine's context as it was.
void transcribe_seek(Engine& e, const float* pcm, size_t n_samples, std::string* text);

// wt_transcribe_long_pcm with seek = 0: consecutive windows, 32 per decode call, their lines joined by '\n' in *text.
// Leaves in Engine::last every window's results joined: clip = the window's index, times in the file.
void transcribe_windows(Engine& e, const float* pcm, size_t n_samples, std::string* text);

// wt_transcribe_long_batch: the same loop over n_files recordings side by side.  A round cuts the next
// window of every file still running, and the windows go through the front end, the encoder and ONE ragged decoder chain
// (Engine::set_contexts: every file's own context); then every file takes transcribe_seek's step with its clip's
// result and a file that has reached its end leaves the batch.  A file's result is transcribe_seek's for that file
// alone.  Leaves Engine::last one entry per window, the windows listed file by file (window_files parallel to windows,
// Segment::clip an index into that list), file_text one text per file, and both kinds of context as they were.
void transcribe_seek_batch(Engine& e, const float* const* pcm, const size_t* n_samples, int n_files);

}  // namespace wt
