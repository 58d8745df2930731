// What every other file of the library calls: the error plumbing behind CNN_REQUIRE and
// cnnitmo_check_launch, the device's compute-unit count, and the ABI's version queries.
#include <cstdarg>
#include <cstdio>

#include "common.h"

// ----------------------------------------------------------------------------
// Error plumbing (thread-local message for cnnitmo_last_error).
// ----------------------------------------------------------------------------
static thread_local char g_err[512];
void cnnitmo_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int cnnitmo_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    cnnitmo_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return CNNITMO_ELAUNCH;
  }
  return CNNITMO_OK;
}
int cnnitmo_cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      return 256;
    return v;
  }();
  return n;
}
extern "C" const char* cnnitmo_last_error(void) { return g_err; }
// 2: CNNITMO_CONSUMER_ROWS 16 -> 64 (query it with cnnitmo_consumer_rows) and cnnitmo_bn_apply's
//    scale / shift must be 16-byte aligned
extern "C" int cnnitmo_version(void) { return 2; }
extern "C" int cnnitmo_consumer_rows(void) { return CNNITMO_CONSUMER_ROWS; }
