// hess_matcher_int.h -- what hess_match.hip and hess_geom.hip share.  struct hess_matcher stays in hess_match.hip; the estimator
// reads it through this view and keeps its own scratch buffers behind one pointer the matcher owns.  The buffer types of both.
#ifndef HESS_MATCHER_INT_H
#define HESS_MATCHER_INT_H
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/hess_abi.h"

struct hess_matcher;
struct hess_geom_state;  // hess_geom.hip: created there on first use, destroyed with the matcher
void hess_geom_state_destroy(hess_geom_state* g);
struct hess_geom_state_delete { void operator()(hess_geom_state* g) const { hess_geom_state_destroy(g); } };
using hess_geom_state_ptr = std::unique_ptr<hess_geom_state, hess_geom_state_delete>;

struct hess_matcher_view {
  int device;
  hipStream_t st;
  hipEvent_t e0, e1;
  std::string& err;
  float* last_ms;
  const float2* loc[2];  // hess_matcher_set_locations of the two single-pair slots
  int nloc[2];           // their rows (the slot's descriptors), -1: the slot has no locations
  bool bank_built;       // descriptors were loaded into the bank (possibly none)
  const std::vector<int>*bank_num, *bank_cnt, *bank_first;  // per set: rows kept, rows the caller counted, first kept row
  // hess_matcher_bank_set_locations: one (x, y) per kept row in the caller's order, set s from bank_first[s] on -- NOT padded
  // like the descriptors.  NULL with bank_have_loc false when there are none (and NULL with true for a bank without rows).
  const float2* bank_loc;
  bool bank_have_loc;
  hess_geom_state_ptr* geom;
};

hess_matcher_view hess_matcher_view_of(hess_matcher* m);

// Estimates over matches that are on the device already (hess_matcher_verify_pairs): nothing here waits for the stream.
// The np pairs of a chunk: pair q has counts[q] matches (row of set 1, row of set 2) at matches + q * mm and its mask bytes at
// mask + q * mm, its sets' locations from row lalb[q].x and .y of the bank's locations on, seed0 + q as its seed; its
// result goes to results[q].  All pointers are device memory; counts and matches are read in stream order.
struct hess_geom_device_pairs {
  int np, mm;
  const int2* lalb;
  const int* counts;
  const int2* matches;
  uint32_t seed0;
  hess_geom_result* results;
  unsigned char* mask;
};
// What hess_matcher_estimate_pairs refuses in its params, with `what` as the entry point's name in the error text.
int hess_geom_params_check(hess_matcher* m, const hess_geom_params* P, const char* what);
// Grows the estimator's own buffers (tables, block entries, the refit's candidate masks) for chunks of up to np pairs of
// up to mm matches: 0 or a negative hess_status with the error text set.  Before the first launch of a call.
int hess_geom_reserve(hess_matcher* m, const hess_geom_params& P, int np, int mm);
// Enqueues the table fill and the score, finish and (P.refit > 0) refit kernels of d on the matcher's stream.  The bank has
// locations and hess_geom_reserve covered d (the caller checked both).
hipError_t hess_geom_enqueue(hess_matcher* m, const hess_geom_params& P, const hess_geom_device_pairs& d);

// A failed HIP call ends the function with HESS_ERR_DEVICE and the call's text in m->err (m: a matcher or a pointer to its view).
#define M_TRY(m, expr)                                                                       \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      (m)->err = std::string(#expr) + " failed: " + hipGetErrorString(e_);                   \
      return HESS_ERR_DEVICE;                                                                \
    }                                                                                        \
  } while (0)

// A device buffer of at least n elements after grow(n): kept when it is large enough, else replaced (its contents are not
// carried over).  Freed with its owner.  What must outlive a failed replacement is built in a buffer of its own and swapped in.
template <class T>
struct DeviceBuf {
  T* p = nullptr;
  size_t cap = 0;
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  ~DeviceBuf() { reset(); }
  void reset() {
    (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  void swap(DeviceBuf& o) {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  hipError_t grow(size_t n) {
    if (n <= cap) return hipSuccess;
    reset();
    const hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
};

// Two pinned host buffers of at least n elements each, by the same rule.
template <class T>
struct PinnedSlots {
  T* p[2] = {nullptr, nullptr};
  size_t cap = 0;
  PinnedSlots() = default;
  PinnedSlots(const PinnedSlots&) = delete;
  PinnedSlots& operator=(const PinnedSlots&) = delete;
  ~PinnedSlots() { reset(); }
  void reset() {
    for (int k = 0; k < 2; k++) { (void)hipHostFree(p[k]); p[k] = nullptr; }
    cap = 0;
  }
  hipError_t grow(size_t n) {
    if (n <= cap) return hipSuccess;
    reset();
    for (int k = 0; k < 2; k++) {
      const hipError_t e = hipHostMalloc(&p[k], n * sizeof(T), hipHostMallocDefault);
      if (e != hipSuccess) return e;
    }
    cap = n;
    return hipSuccess;
  }
};

#endif  // HESS_MATCHER_INT_H
