// What the engine's translation units (engine.cpp, engine_full.cpp) share and nobody else sees: the HIP status check
// and the graph capture.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "engine.h"

namespace wt {

inline void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    throw Error(5, std::string("HIP failure in ") + what + ": " + hipGetErrorString(e));
  }
}
#define HIPCHK(x) ::wt::hip_check((x), #x)

// begin-capture, enqueue(), end-capture, instantiate: the executable graph of what enqueue() put on the stream.
// Throws what enqueue() throws, or kErrDevice; nothing stays captured or allocated then.
template <class F>
hipGraphExec_t capture_graph(hipStream_t s, F&& enqueue) {
  hipGraph_t graph = nullptr;
  hipGraphExec_t ge = nullptr;
  HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  try {
    enqueue();
  } catch (...) {
    (void)hipStreamEndCapture(s, &graph);
    if (graph) (void)hipGraphDestroy(graph);
    throw;
  }
  HIPCHK(hipStreamEndCapture(s, &graph));
  const hipError_t ie = hipGraphInstantiate(&ge, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ie != hipSuccess) throw Error(kErrDevice, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
  return ge;
}

}  // namespace wt
