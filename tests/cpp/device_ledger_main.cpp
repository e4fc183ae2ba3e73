// The ledger of device resources (csrc/device_ledger.h) shown to count what it is told: live allocations and their bytes after a scripted
// sequence, a double and a foreign free once each, an address handed out again after its free live once, events / streams / handles,
// a failed release that keeps its entry - and four threads that record and release 10 000 entries each ending at zero live with totals
// that add up.  tests/test_device_ledger_cpu.py builds this file under the host sanitizers (address + undefined, then thread) and runs it.
#include <stdio.h>

#include <thread>
#include <vector>

#include "device_ledger.h"

using namespace ledger;

static int failures = 0;
#define CHECK(expr, want)                                                                            \
  do {                                                                                               \
    const long long got__ = (long long)(expr);                                                       \
    if (got__ != (long long)(want)) {                                                                \
      printf("line %d: %s = %lld, expected %lld\n", __LINE__, #expr, got__, (long long)(want));      \
      failures++;                                                                                    \
    }                                                                                                \
  } while (0)

struct Snap {
  int64_t v[COUNT];
  explicit Snap(const DeviceLedger& l) { CHECK(l.snapshot(v, COUNT), COUNT); }
  int64_t operator[](int f) const { return v[f]; }
};
// addresses are never dereferenced: the ledger keys on the value
static const void* addr(uintptr_t a) { return (const void*)a; }

static void scripted() {
  DeviceLedger l;
  for (int f = 0; f < COUNT; f++) CHECK(Snap(l)[f], 0);
  l.alloc(addr(0x1000), 100);
  l.alloc(addr(0x2000), 4096);
  l.alloc(addr(0x3000), 1);
  l.alloc(nullptr, 77);  // a failed allocation records nothing
  { Snap s(l); CHECK(s[ALLOCS_LIVE], 3); CHECK(s[BYTES_LIVE], 4197); CHECK(s[ALLOCS_TOTAL], 3); CHECK(s[FREES_TOTAL], 0); }
  l.free(addr(0x2000), true);
  { Snap s(l); CHECK(s[ALLOCS_LIVE], 2); CHECK(s[BYTES_LIVE], 101); CHECK(s[FREES_TOTAL], 1); CHECK(s[FREES_UNKNOWN], 0); }
  l.free(addr(0x2000), true);  // a second free of the same pointer: counted once, nothing else moves
  { Snap s(l); CHECK(s[ALLOCS_LIVE], 2); CHECK(s[BYTES_LIVE], 101); CHECK(s[FREES_TOTAL], 1); CHECK(s[FREES_UNKNOWN], 1); }
  l.free(addr(0x9000), true);  // a pointer never recorded
  { Snap s(l); CHECK(s[ALLOCS_LIVE], 2); CHECK(s[FREES_TOTAL], 1); CHECK(s[FREES_UNKNOWN], 2); }
  l.free(nullptr, true);       // free(NULL) is no release
  { Snap s(l); CHECK(s[FREES_TOTAL], 1); CHECK(s[FREES_UNKNOWN], 2); CHECK(s[RELEASE_ERRORS], 0); }
  l.alloc(addr(0x2000), 8);    // the freed address handed out again: live once, with its new size
  { Snap s(l); CHECK(s[ALLOCS_LIVE], 3); CHECK(s[BYTES_LIVE], 109); CHECK(s[ALLOCS_TOTAL], 4); CHECK(s[FREES_UNKNOWN], 2); }
  l.free(addr(0x1000), false);  // the runtime refused the release: the entry stays
  { Snap s(l); CHECK(s[ALLOCS_LIVE], 3); CHECK(s[BYTES_LIVE], 109); CHECK(s[RELEASE_ERRORS], 1); CHECK(s[FREES_TOTAL], 1); }
  l.alloc(addr(0x3000), 50);    // an address recorded again while held: live once, the lost release counted
  { Snap s(l); CHECK(s[ALLOCS_LIVE], 3); CHECK(s[BYTES_LIVE], 158); CHECK(s[ALLOCS_TOTAL], 5); CHECK(s[FREES_TOTAL], 2); CHECK(s[FREES_UNKNOWN], 3); }
  // events, streams, handles: none of them moves an allocation count
  l.event_create(addr(0x10)); l.event_create(addr(0x20)); l.stream_create(addr(0x30));
  l.handle(CTX, +1); l.handle(MODEL, +1); l.handle(MODEL, +1); l.handle(SESSION, +1);
  {
    Snap s(l);
    CHECK(s[EVENTS_LIVE], 2); CHECK(s[STREAMS_LIVE], 1); CHECK(s[CTX_LIVE], 1); CHECK(s[MODELS_LIVE], 2); CHECK(s[SESSIONS_LIVE], 1);
    CHECK(s[ALLOCS_LIVE], 3); CHECK(s[ALLOCS_TOTAL], 5);
  }
  l.event_destroy(addr(0x10), true);
  l.event_destroy(addr(0x10), true);   // twice
  l.stream_destroy(addr(0x20), true);  // an event's handle is no stream
  l.event_destroy(addr(0x20), false);  // refused: it stays
  { Snap s(l); CHECK(s[EVENTS_LIVE], 1); CHECK(s[STREAMS_LIVE], 1); CHECK(s[FREES_UNKNOWN], 5); CHECK(s[RELEASE_ERRORS], 2); }
  l.event_destroy(addr(0x20), true); l.stream_destroy(addr(0x30), true);
  l.handle(CTX, -1); l.handle(MODEL, -1); l.handle(MODEL, -1); l.handle(SESSION, -1);
  l.free(addr(0x1000), true); l.free(addr(0x2000), true); l.free(addr(0x3000), true);
  {
    Snap s(l);
    for (int f = ALLOCS_LIVE; f <= SESSIONS_LIVE; f++) CHECK(s[f], 0);
    CHECK(s[ALLOCS_TOTAL], 5); CHECK(s[FREES_TOTAL], 5); CHECK(s[FREES_UNKNOWN], 5); CHECK(s[RELEASE_ERRORS], 2);
  }
  // a short output array takes the leading fields only
  int64_t two[3] = {-1, -1, -1};
  l.alloc(addr(0x5000), 9);
  CHECK(l.snapshot(two, 2), COUNT); CHECK(two[0], 1); CHECK(two[1], 9); CHECK(two[2], -1);
}

static void threaded() {
  DeviceLedger l;
  const int T = 4, N = 10000;
  l.alloc(addr(0x8), 5);  // held across the whole run
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++)
    th.emplace_back([&l, t] {
      const uintptr_t base = ((uintptr_t)(t + 1) << 32);
      for (int i = 0; i < N; i++) {
        const void* p = addr(base + 256 * (uintptr_t)(i % 64 + 1));  // 64 addresses per thread, each handed out again and again
        l.alloc(p, (size_t)i + 1);
        if (i % 3 == 0) l.event_create(p);
        if (i % 5 == 0) l.stream_create(p);
        l.handle((Handle)(i % 3), +1);
        int64_t v[COUNT];
        if (i % 97 == 0) l.snapshot(v, COUNT);
        l.handle((Handle)(i % 3), -1);
        if (i % 5 == 0) l.stream_destroy(p, true);
        if (i % 3 == 0) l.event_destroy(p, true);
        l.free(p, true);
      }
    });
  for (std::thread& x : th) x.join();
  Snap s(l);
  CHECK(s[ALLOCS_LIVE], 1); CHECK(s[BYTES_LIVE], 5);
  for (int f = EVENTS_LIVE; f <= SESSIONS_LIVE; f++) CHECK(s[f], 0);
  CHECK(s[ALLOCS_TOTAL], (long long)T * N + 1); CHECK(s[FREES_TOTAL], (long long)T * N);
  CHECK(s[ALLOCS_TOTAL] - s[FREES_TOTAL], s[ALLOCS_LIVE]);
  CHECK(s[FREES_UNKNOWN], 0); CHECK(s[RELEASE_ERRORS], 0);
}

int main() {
  scripted();
  threaded();
  if (failures) return 1;
  printf("device_ledger: scripted sequence and 4 x 10000 threaded entries add up\n");
  return 0;
}
