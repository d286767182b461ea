// What the stand-alone refusal programs (X_refusals_main.cpp, `make X-refusals`) share.  Each of them calls entry points of X.hip
// with arguments the host-side checks refuse, so no kernel launch is reached and no GPU is needed; it is built with ASAN + UBSAN
// on the host code and exits 0 when every call came back with the expected code and message.  CPU machines only.
#pragma once
#include "../../include/snerf_hip.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

static char g_error[512];

namespace snerf {
// the library's set_error (api.hip), which these programs do not link
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}
}  // namespace snerf

static int failures = 0;
static int what_width = 44;       // the column of the printed case names

// One refused (or, with want = SNERF_OK, accepted) call: the code is `want`, the message contains `needle` (NULL: any message, none
// included) and begins with `prefix` (NULL: anywhere).
static void expect(const char* what, int rc, int want, const char* needle, const char* prefix) {
  const bool ok = rc == want && (needle == nullptr || strstr(g_error, needle) != nullptr) &&
                  (prefix == nullptr || strstr(g_error, prefix) == g_error);
  printf("%-*s rc = %d  \"%s\"%s\n", what_width, what, rc, g_error, ok ? "" : "   <-- UNEXPECTED");
  if (!ok) ++failures;
  g_error[0] = 0;
}

// the same under the prefix in force: a program sets g_prefix to "snerf_X: " before the cases of entry X, and to NULL for accepted calls
static const char* g_prefix = nullptr;
static void expect(const char* what, int rc, int want, const char* needle) { expect(what, rc, want, needle, g_prefix); }

// the verdict line and the program's exit status
static int verdict(const char* name) {
  printf("%s refusals: %s\n", name, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
