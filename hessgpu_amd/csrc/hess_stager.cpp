// hess_stager.cpp -- both sides of the staging protocol (see hess_stager.h): the helper threads and the calling thread's walk.
#include "hess_stager.h"

#include <algorithm>
#include <cstring>

namespace hess {

static void stager_copy(Stager& sg, int k) {
  const size_t off = (size_t)k * sg.chunk, len = std::min(sg.chunk, sg.bytes - off);
  memcpy(sg.dst + off, sg.src + off, len);
  { std::lock_guard<std::mutex> lk(sg.mu); sg.state[k].store(2, std::memory_order_release); }
  sg.cv_done.notify_all();
}

static void stager_main(Stager* sgp) {
  Stager& sg = *sgp;
  unsigned long long seen = 0;
  std::unique_lock<std::mutex> lk(sg.mu);
  for (;;) {
    sg.cv_job.wait(lk, [&] { return sg.stop || sg.gen != seen; });
    if (sg.stop) return;
    seen = sg.gen;
    lk.unlock();
    for (;;) {
      const int k = sg.next_hi.fetch_sub(1, std::memory_order_acq_rel);
      if (k < 0) break;
      int expect = 0;
      if (sg.state[k].compare_exchange_strong(expect, 1, std::memory_order_acq_rel)) stager_copy(sg, k);
      else break;  // met the calling thread coming up: everything is claimed
    }
    lk.lock();
    sg.active--;
    sg.cv_done.notify_all();
  }
}

void stager_start(Stager& sg) {
  if (sg.tried) return;
  sg.tried = true;
  for (int t = 0; t < Stager::kHelpers; t++) {
    try { sg.th[sg.nth] = std::thread(stager_main, &sg); sg.nth++; } catch (...) { break; }  // fewer helpers: the caller copies more
  }
}

void stager_stop(Stager& sg) {
  if (!sg.nth) return;
  { std::lock_guard<std::mutex> lk(sg.mu); sg.stop = true; }
  sg.cv_job.notify_all();
  for (int t = 0; t < sg.nth; t++) sg.th[t].join();
  sg.nth = 0;
}

bool stager_run_fn(Stager& sg, const void* src, void* dst, size_t bytes, size_t chunk, bool helped,
                   void (*on_staged)(void* arg, size_t offset, size_t length), void* arg) {
  const int nchunk = (int)((bytes + chunk - 1) / chunk);
  helped = helped && nchunk > 1;
  if (helped) stager_start(sg);
  try {  // (no helper is inside a job: the job before ended with active == 0)
    if ((int)sg.state.size() < nchunk) { std::vector<std::atomic<int>> grown(nchunk); sg.state.swap(grown); }
  } catch (...) { return false; }
  {
    std::lock_guard<std::mutex> lk(sg.mu);
    for (int k = 0; k < nchunk; k++) sg.state[k].store(0, std::memory_order_relaxed);
    sg.src = (const char*)src; sg.dst = (char*)dst; sg.bytes = bytes; sg.chunk = chunk; sg.nchunk = nchunk;
    sg.next_hi.store(helped ? nchunk - 1 : -1, std::memory_order_release);
    sg.active = helped ? sg.nth : 0;
    if (helped && sg.nth) sg.gen++;
  }
  if (helped && sg.nth) sg.cv_job.notify_all();
  for (int k = 0; k < nchunk; k++) {
    int expect = 0;
    if (sg.state[k].compare_exchange_strong(expect, 1, std::memory_order_acq_rel)) stager_copy(sg, k);
    else if (sg.state[k].load(std::memory_order_acquire) != 2) {
      std::unique_lock<std::mutex> lk(sg.mu);
      sg.cv_done.wait(lk, [&] { return sg.state[k].load(std::memory_order_acquire) == 2; });
    }
    const size_t off = (size_t)k * chunk;
    on_staged(arg, off, std::min(chunk, bytes - off));
  }
  // the helpers are done with this job's bookkeeping before the next one rewrites it
  std::unique_lock<std::mutex> lk(sg.mu);
  sg.cv_done.wait(lk, [&] { return sg.active == 0; });
  return true;
}

}  // namespace hess
