// hess_stager.h -- helper threads that stage pageable pixels into pinned memory.  Standard headers only: no HIP, no context
// (tests/test_stager_cpu.py runs the protocol under ThreadSanitizer without either).
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

namespace hess {

// Persistent helper threads that copy pageable input pixels into the context's pinned staging buffer
// (hess_submit_host).  The calling thread walks the chunks in ascending order -- staging the ones nobody has claimed,
// enqueueing every chunk's transfer as soon as it is staged -- while the helpers claim chunks from the END, so the
// early chunks are ready first.  Started at the first pageable submission, reused afterwards: starting threads per
// call cost more than staging one image.
struct Stager {
  static constexpr int kHelpers = 3;
  std::thread th[kHelpers];
  int nth = 0;
  bool tried = false;
  std::mutex mu;
  std::condition_variable cv_job, cv_done;
  bool stop = false;
  unsigned long long gen = 0;
  const char* src = nullptr;
  char* dst = nullptr;
  size_t bytes = 0, chunk = 0;
  int nchunk = 0, active = 0;
  std::vector<std::atomic<int>> state;  // per chunk: 0 free, 1 claimed, 2 staged
  std::atomic<int> next_hi{-1};
};

void stager_start(Stager& sg);  // (stager_run starts the helpers itself; once per Stager, fewer than kHelpers may come up)
void stager_stop(Stager& sg);   // joins every helper
bool stager_run_fn(Stager& sg, const void* src, void* dst, size_t bytes, size_t chunk, bool helped,
                   void (*on_staged)(void* arg, size_t offset, size_t length), void* arg);

// One job, the calling thread's side: `bytes` from src to dst in chunks of `chunk`, with the helper threads when `helped`
// (and more than one chunk).  on_staged(offset, length) is called on the calling thread once per chunk, in ascending order,
// as soon as that chunk is staged.  Returns after the helpers have left the job; false (nothing copied, nothing called) when
// the per-chunk state cannot grow.  Nothing is thrown, and nothing allocates once the state holds a job's chunks.
template <class F>
bool stager_run(Stager& sg, const void* src, void* dst, size_t bytes, size_t chunk, bool helped, F&& on_staged) {
  using Fn = std::remove_reference_t<F>;
  return stager_run_fn(sg, src, dst, bytes, chunk, helped,
                       [](void* f, size_t offset, size_t length) { (*static_cast<Fn*>(f))(offset, length); },
                       const_cast<void*>(static_cast<const void*>(&on_staged)));
}

}  // namespace hess
