// staged_test.cc -- the staged call of the handle forms (csrc/nhip_host.h, Staged) on its first-failure path.  Run with no
// HIP device visible (tests/test_staged_cpp.py hides them): every hipMalloc then fails cleanly, so the first in / out is the
// call's first error.  Built with the host sanitizers (Makefile, staged_test): what is checked besides the asserts below is
// that nothing is read, written or released that should not be.
#include <cstdio>
#include <cstring>
#include <vector>

#include "nhip_common.h"
#include "nhip_host.h"

using namespace nhip;

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      return 1;                                                 \
    }                                                           \
  } while (0)

static bool all_are(const std::vector<int32_t> &v, int32_t want) {
  for (int32_t x : v)
    if (x != want) return false;
  return true;
}

int main() {
  if (require_device() != NHIP_ERR_NODEV) {
    printf("staged_test: a HIP device is visible; this program is about the path without one\n");
    return 2;
  }
  const std::vector<int32_t> src(100, 7);
  std::vector<int32_t> dst(100, -3);
  {
    // the first upload fails: NHIP_ERR_ALLOC, its message kept; everything after it does nothing
    Staged st;
    CHECK(st.ok());
    const int32_t *a = st.in(src.data(), src.size());
    CHECK(a == nullptr && !st.ok());
    const std::string first = nhip_last_error();
    CHECK(first.find("hipMalloc") != std::string::npos);
    CHECK(st.out<double>(1000) == nullptr);
    CHECK(st.inout(dst.data(), dst.size()) == nullptr);
    CHECK(st.in<float>(nullptr, 0) == nullptr && st.out<uint8_t>(0) == nullptr);
    st.fetch(dst.data(), a, dst.size());                 // (a null device pointer)
    st.fetch(dst.data(), src.data(), dst.size());        // (a pointer that could be read: still nothing, the call has failed)
    st.fetch(static_cast<int32_t *>(nullptr), a, 5);
    CHECK(all_are(dst, -3));
    CHECK(st.finish() == NHIP_ERR_ALLOC && st.finish() == NHIP_ERR_ALLOC);
    CHECK(first == nhip_last_error());
  }  // (destruction after a failure: nothing enqueued, nothing to wait for, one empty buffer record)
  {
    // the first call is an output; a launcher's code after the failure does not replace the first error
    Staged st;
    CHECK(st.out<int64_t>(STATS_WORDS) == nullptr && !st.ok());
    const std::string first = nhip_last_error();
    st.launched(NHIP_ERR_ARG);  // (a form asks ok() first; a stray code must not win either)
    CHECK(st.finish() == NHIP_ERR_ALLOC && first == nhip_last_error());
  }  // (destruction of a call marked in flight: the wait's error is swallowed)
  {
    // zero counts and null hosts are arguments like any other: without a device they are the call's first allocation
    Staged st;
    CHECK(st.in<float>(nullptr, 0) == nullptr);
    CHECK(st.finish() == NHIP_ERR_ALLOC);
    Staged none;  // a call that staged nothing
    none.fetch(dst.data(), static_cast<const int32_t *>(nullptr), 0);
    CHECK(none.ok() && none.finish() == NHIP_OK && all_are(dst, -3));
  }
  CHECK(aligned(nullptr, 256) && aligned(reinterpret_cast<void *>(uintptr_t(48)), 16) && !aligned(reinterpret_cast<void *>(uintptr_t(40)), 16));
  printf("STAGED_OK\n");
  return 0;
}
