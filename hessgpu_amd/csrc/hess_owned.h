// hess_owned.h -- runtime handles destroyed with their owner, for the extraction context (hess_ctx.h, which adds the ROCr
// signal) and the matcher (hess_match.hip).  HIP only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

namespace hess {

// A runtime handle destroyed with its owner: a stream, an event, a completion signal.  A null handle owns nothing.
template <class H, class R, R (*destroy)(H)>
struct Owned {
  H h{};
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { if (*this) (void)destroy(h); }
  operator H() const { return h; }
  explicit operator bool() const { H none{}; return memcmp(&h, &none, sizeof(H)) != 0; }
  void forget() { h = H{}; }  // given up without being destroyed (a signal that a lost copy may still write)
};
using Stream = Owned<hipStream_t, hipError_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipError_t, hipEventDestroy>;
// e's event, created on first need.
inline hipError_t ensure(Event& e) { return e ? hipSuccess : hipEventCreate(&e.h); }

}  // namespace hess
