// hess_slot_pipeline.h -- the double-buffered delivery loop of the matcher's pair-list entry points, without HIP (standard
// headers only; tests/slot_pipeline_main.cpp drives it on the CPU).  A call is n units (run_pairs: chunks; run_verify: groups
// of chunks), unit k going through slot k & 1 of two: while the device works on unit k the host delivers unit k - 1.
#ifndef HESS_SLOT_PIPELINE_H
#define HESS_SLOT_PIPELINE_H
#include <cstddef>

namespace hess {

// enqueue(k, slot) puts unit k's work in flight, collect(k, slot) waits for unit k and delivers it; both return a Status,
// `ok` for success.  Order: enqueue(0), enqueue(1), collect(0), enqueue(2), collect(1), ..., collect(n - 1).  The first
// status other than `ok` ends the loop -- nothing more is called -- and is returned; `ok` otherwise (also for n == 0).
template <class Status, class Enqueue, class Collect>
Status slot_pipeline(size_t n, Status ok, Enqueue&& enqueue, Collect&& collect) {
  for (size_t k = 0; k < n; k++) {
    Status s = enqueue(k, (int)(k & 1));
    if (s == ok && k > 0) s = collect(k - 1, (int)((k - 1) & 1));
    if (!(s == ok)) return s;
  }
  return n ? collect(n - 1, (int)((n - 1) & 1)) : ok;
}

}  // namespace hess

#endif  // HESS_SLOT_PIPELINE_H
