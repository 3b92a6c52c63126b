// slot_pipeline_main.cpp -- drives the matcher's double-buffered delivery loop (hessgpu_amd/csrc/hess_slot_pipeline.h) with
// recording callables and prints what it called.  Built with -fsanitize=address,undefined and run by
// tests/test_slot_pipeline_cpu.py, which holds the printed sequences against the ones written out there by hand.
//
// For every n of the command line (the units of a call), one line per run: all calls succeeding, then for each unit k enqueue k
// failing and collect k failing.  A failing call returns a status of its own: 100 + k from enqueue k, 200 + k from collect k.
//   N ok|eK|cK : CALLS -> STATUS      CALLS: eK.S = enqueue(K, slot S), cK.S = collect(K, slot S), in the order they happened
// Exit status 1 if anything was called after a failing call.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "hess_slot_pipeline.h"

struct Run {
  char fail_kind;  // 'e', 'c' or 0
  size_t fail_k;
  std::string calls;
  bool failed = false;
  int call(char kind, size_t k, int slot) {
    if (failed) {
      fprintf(stderr, "%c%zu called after the failing call (%s)\n", kind, k, calls.c_str());
      exit(1);
    }
    calls += (calls.empty() ? "" : " ") + std::string(1, kind) + std::to_string(k) + "." + std::to_string(slot);
    failed = kind == fail_kind && k == fail_k;
    return failed ? (kind == 'e' ? 100 : 200) + (int)k : 0;
  }
};

static void run(size_t n, char kind, size_t k) {
  Run r{kind, k};
  const int status = hess::slot_pipeline(
      n, 0, [&](size_t u, int slot) { return r.call('e', u, slot); }, [&](size_t u, int slot) { return r.call('c', u, slot); });
  if (kind) printf("%zu %c%zu : %s -> %d\n", n, kind, k, r.calls.c_str(), status);
  else printf("%zu ok : %s -> %d\n", n, r.calls.c_str(), status);
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    const size_t n = (size_t)atoi(argv[a]);
    run(n, 0, 0);
    for (size_t k = 0; k < n; k++) {
      run(n, 'e', k);
      run(n, 'c', k);
    }
  }
  return 0;
}
