// stager_main.cpp -- drives one Stager (hessgpu_amd/csrc/hess_stager.h) through jobs of several shapes back to back, so that the
// hand-over between jobs is exercised too.  Built with -fsanitize=thread and run by tests/test_stager_cpu.py; exit status 0 = every
// job copied its bytes, called on_staged once per chunk in ascending order, and stager_stop joined the helpers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hess_stager.h"

using namespace hess;

static const size_t kGuard = 64;
static unsigned g_seed = 1;

static bool job(Stager& sg, const char* name, size_t bytes, size_t chunk, bool helped) {
  std::vector<unsigned char> src(bytes), dst(bytes + kGuard, 0xA5);
  for (size_t i = 0; i < bytes; i++) src[i] = (unsigned char)((i * 131 + g_seed * 17 + (i >> 8)) & 0xFF);
  g_seed++;
  const size_t nchunk = (bytes + chunk - 1) / chunk;
  size_t calls = 0, next = 0;  // `next`: where the next pair must begin
  bool in_order = true;
  const bool ran = stager_run(sg, src.data(), dst.data(), bytes, chunk, helped, [&](size_t off, size_t len) {
    in_order = in_order && off == next && len > 0 && len <= chunk && (off + len == bytes || len == chunk) &&
               !memcmp(dst.data() + off, src.data() + off, len);  // (staged by the time it is announced)
    next = off + len;
    calls++;
  });
  bool ok = true;
  auto check = [&](bool cond, const char* what) {
    if (!cond) { fprintf(stderr, "job %s (%zu bytes, chunks of %zu): %s\n", name, bytes, chunk, what); ok = false; }
  };
  check(ran, "stager_run returned false");
  check(calls == nchunk, "on_staged was not called exactly once per chunk");
  check(in_order, "the (offset, length) pairs are not ascending, whole chunks that were staged when announced");
  check(next == bytes, "the (offset, length) pairs do not tile [0, bytes)");
  check(!memcmp(dst.data(), src.data(), bytes), "dst differs from src");
  for (size_t i = 0; i < kGuard; i++) check(dst[bytes + i] == 0xA5, "bytes past the end of dst were written");
  return ok;
}

int main(int argc, char** argv) {
  const int repeats = argc > 1 ? atoi(argv[1]) : 200;
  const size_t chunk = 4096;
  Stager sg;
  bool ok = job(sg, "1", 1, chunk, false);
  ok = job(sg, "2", chunk, chunk, true) && ok;
  ok = job(sg, "3", 3 * chunk + 1, chunk, true) && ok;
  ok = job(sg, "4", 257 * 64, 64, true) && ok;  // small chunks: the caller and the helpers collide; the state vector grows
  ok = job(sg, "5", 2 * chunk, chunk, false) && ok;  // fewer chunks than before: the old state entries are stale
  for (int i = 0; i < repeats; i++) ok = job(sg, "6", 257 * 64, 64, true) && ok;
  if (sg.nth < 1) { fprintf(stderr, "no helper thread came up: the helped jobs ran alone\n"); ok = false; }
  stager_stop(sg);
  if (sg.nth != 0) { fprintf(stderr, "stager_stop left helpers behind\n"); ok = false; }
  for (std::thread& t : sg.th)
    if (t.joinable()) { fprintf(stderr, "stager_stop did not join every helper\n"); ok = false; }
  if (ok) printf("STAGER OK\n");
  return ok ? 0 : 1;
}
