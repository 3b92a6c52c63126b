// hess_matcher_int.h -- what hess_geom.hip needs of a matcher.  struct hess_matcher stays in hess_match.hip; the estimator
// reads it through this view and keeps its own state (bank locations, buffers) behind one pointer the matcher owns.
#ifndef HESS_MATCHER_INT_H
#define HESS_MATCHER_INT_H
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/hess_abi.h"

struct hess_matcher;
struct hess_geom_state;  // hess_geom.hip

struct hess_matcher_view {
  int device;
  hipStream_t st;
  hipEvent_t e0, e1;
  std::string* err;
  float* last_ms;
  const float2* loc[2];  // hess_matcher_set_locations of the two single-pair slots
  int nloc[2];           // their rows (the slot's descriptors), -1: the slot has no locations
  bool bank_built;       // descriptors were loaded into the bank (possibly none)
  const std::vector<int>*bank_num, *bank_cnt, *bank_first;  // per set: rows kept, rows the caller counted, first kept row
  hess_geom_state** geom;  // created by hess_geom.hip on first use
};

hess_matcher_view hess_matcher_view_of(hess_matcher* m);
// The pointer check of hess_matcher_bank_set_device: `bytes` from p on are device memory of the matcher's device within one
// allocation, or HESS_ERR_ARG with the error text set.
int hess_matcher_device_range(hess_matcher* m, const void* p, size_t bytes, const char* what, const char* noun);

// hess_geom.hip, called by the matcher: the bank's descriptors were replaced (its locations go with them); the matcher dies.
void hess_geom_drop_bank_locations(hess_geom_state* g);
void hess_geom_state_destroy(hess_geom_state* g);
// The bank's locations for guided pair lists: false without any (g may be NULL); else *loc = one (x, y) per kept row in the
// caller's order, set s from DescSets::first[s] on -- NOT padded like the descriptors (NULL for a bank without rows).
bool hess_geom_bank_locations(const hess_geom_state* g, const float2** loc);

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

// A device buffer of at least n elements: kept when it is large enough, else replaced (its contents are not carried over).
template <class T>
hipError_t grow_device(T*& p, size_t& cap, size_t n) {
  if (n <= cap) return hipSuccess;
  (void)hipFree(p);
  p = nullptr;
  cap = 0;
  const hipError_t e = hipMalloc(&p, n * sizeof(T));
  if (e == hipSuccess) cap = n;
  return e;
}

#endif  // HESS_MATCHER_INT_H
