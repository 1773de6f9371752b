// What the two halves of the extern "C" boundary share: capi.cpp (include/wt_capi.h) and capi_debug.cpp
// (include/wt_debug.h).  Private to csrc/; everything here has internal or hidden linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "engine.h"
#include "error.h"
#include "wt_capi.h"

struct wt_engine {
  std::unique_ptr<wt::Engine> impl;
  std::string last_error;
};

// records msg as h's last error (h == nullptr: the calling thread's creation error) and returns code; capi.cpp
__attribute__((visibility("hidden"))) int fail(wt_engine* h, int code, const std::string& msg);

// Runs fn, translating every exception into a status code.
template <class F>
static int guarded(wt_engine* h, F&& fn) {
  try {
    if (h && h->impl) h->impl->bind_device();  // one handle per GPU: launches go to its device
    fn();
    if (h) h->last_error.clear();
    return WT_OK;
  } catch (const wt::Error& e) {
    return fail(h, e.code, e.what());
  } catch (const std::bad_alloc&) {
    return fail(h, WT_ERR_DEVICE, "out of host memory");
  } catch (const std::exception& e) {
    const std::string w = e.what();
    return fail(h, w.rfind("Failed to open", 0) == 0 ? WT_ERR_IO : WT_ERR_FORMAT, w);
  } catch (...) {
    return fail(h, WT_ERR_DEVICE, "unknown failure");
  }
}

static inline void hipchk(hipError_t e, const char* what) {
  if (e != hipSuccess) throw wt::Error(WT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
