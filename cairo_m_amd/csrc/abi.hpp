// What every extern "C" entry point of the library shares (host code only): the exception-to-status guard, the casts from the
// header's opaque integers to what they stand for, and the default PCS configuration.  None of it is an exported symbol.
#pragma once
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include <exception>
#include <type_traits>
#include <vector>

extern "C" int32_t cm_set_last_error(const char* msg);   // capi.hip: the calling thread's error string; returns 1

#define CM_INTERNAL __attribute__((visibility("hidden")))

namespace cm {

// The body of a C-ABI call: 0 (or what a body that reports verdicts of its own returns), or the error's status (1 when it has
// none) with its message left for cm_last_error().  Nothing thrown leaves the extern "C" function.  Bind: hipSetDevice is per
// host thread, so the entry points of capi.hip select the library's device first; the others do it where their bodies need it.
template <bool Bind, class F>
CM_INTERNAL int32_t abi_guard_impl(F&& f) {
  try {
    if (Bind) bind_thread_to_library_device();
    if constexpr (std::is_void<decltype(f())>::value) { f(); return 0; }
    else return f();
  }
  catch (const CmError& e) { cm_set_last_error(e.what()); return e.code ? e.code : 1; }
  catch (const std::exception& e) { cm_set_last_error(e.what()); return 1; }
  catch (...) { cm_set_last_error("unknown error"); return 1; }
}
template <class F>
CM_INTERNAL int32_t abi_guard(F&& f) { return abi_guard_impl<false>(f); }
template <class F>
CM_INTERNAL int32_t abi_guard_bound(F&& f) { return abi_guard_impl<true>(f); }

CM_INTERNAL inline hipStream_t as_stream(cm_stream_t s) { return (hipStream_t)(uintptr_t)s; }
CM_INTERNAL inline hipStream_t stream_or_own(cm_stream_t s) { return s ? as_stream(s) : thread_main_stream(); }
CM_INTERNAL inline uint32_t* as_words(cm_handle h) { return (uint32_t*)(uintptr_t)h; }
// n column handles as device pointers; a null one is refused
CM_INTERNAL inline std::vector<uint32_t*> handles(const cm_handle* h, int n) {
  std::vector<uint32_t*> v(n);
  for (int i = 0; i < n; i++) { v[i] = as_words(h[i]); CM_CHECK(v[i], "null column handle"); }
  return v;
}
CM_INTERNAL inline cm_pcs_config default_cfg() { return cm_pcs_config{16, 1, 0, 80}; }

}  // namespace cm
