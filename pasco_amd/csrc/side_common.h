// Host plumbing shared by the side surfaces (attn_grad.hip, eval.hip, field.hip, frame.hip, grad.hip, knn.hip, label.hip, match.hip, norm.hip, optim.hip, pool.hip, rowgrad.hip, semloss.hip, target.hip, view.hip, waffle.hip): the error text behind a
// family's `last_error`, the checks after a launch or a runtime call, and the two exports every family has.  Included after
// the family's own header; independent of the core ABI (no ph_common.h, no pasco_hip.h).  Everything lives in an unnamed
// namespace, so every translation unit has its OWN error buffer: one family never shows another family's text.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

namespace {

thread_local char g_err[512];

int fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return 1;
}

}  // namespace

// Macros, so that __FILE__ and __LINE__ name the place in the .hip file.
#define SIDE_CHECK_HIP(expr)                                                                                   \
  do {                                                                                                         \
    hipError_t _e = (expr);                                                                                    \
    if (_e != hipSuccess) return fail("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));    \
  } while (0)

#define SIDE_CHECK_LAUNCH(what)                                                                                \
  do {                                                                                                         \
    hipError_t _e = hipGetLastError();                                                                         \
    if (_e != hipSuccess) return fail("%s:%d: %s -> %s", __FILE__, __LINE__, what, hipGetErrorString(_e));     \
  } while (0)

// `FN(abi_version)` and `FN(last_error)` of a family: FN = its P?_FN, VERSION = its P?_ABI_VERSION.
#define SIDE_EXPORTS(FN, VERSION)                              \
  extern "C" int FN(abi_version)(void) { return VERSION; }     \
  extern "C" const char *FN(last_error)(void) { return g_err; }
