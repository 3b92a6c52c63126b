// hess_matcher_int.h -- what hess_geom.hip needs of a matcher.  struct hess_matcher stays in hess_match.hip; the estimator
// reads it through this view and keeps its own state (bank locations, buffers) behind one pointer the matcher owns.
#ifndef HESS_MATCHER_INT_H
#define HESS_MATCHER_INT_H
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

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
