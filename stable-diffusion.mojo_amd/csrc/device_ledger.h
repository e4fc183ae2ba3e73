// device_ledger.h - the book the library keeps of the device resources it holds: every allocation (pointer -> bytes), event and stream that
// is live, how many contexts, models and sessions are, and what went wrong on a release.  The dev_* wrappers of runtime.cpp call HIP and
// then record here; tsd_debug_device_ledger reads a snapshot.  The ledger only counts: no call behaves differently for what it holds.
// Host only: no HIP, no common.h (tests/cpp/device_ledger_main.cpp compiles it alone, under the host sanitizers).  One mutex guards it all:
// contexts driven from different host threads record into the same ledger.
#pragma once
#include <stdint.h>

#include <mutex>
#include <unordered_map>
#include <unordered_set>

namespace ledger {
// Order and meaning of tsd_device_ledger_field (include/tsd.h); runtime.cpp asserts that the two agree.
enum Field {
  ALLOCS_LIVE = 0,  // device allocations recorded and not released
  BYTES_LIVE,       // their sizes, summed
  EVENTS_LIVE,
  STREAMS_LIVE,
  CTX_LIVE, MODELS_LIVE, SESSIONS_LIVE,  // handles created and not destroyed
  ALLOCS_TOTAL,     // allocations ever recorded (monotone)
  FREES_TOTAL,      // entries ever released (monotone): ALLOCS_LIVE == ALLOCS_TOTAL - FREES_TOTAL at all times
  FREES_UNKNOWN,    // releases of a pointer, event or stream the ledger does not hold: a double or a foreign release (monotone)
  RELEASE_ERRORS,   // releases for which the runtime returned an error; the entry stays (monotone)
  COUNT
};
enum Handle { CTX = 0, MODEL, SESSION };

class DeviceLedger {
 public:
  void alloc(const void* p, size_t bytes) {
    if (!p) return;
    std::lock_guard<std::mutex> g(mu_);
    auto it = allocs_.find(p);
    if (it != allocs_.end()) {  // the address is handed out again while held: its release never came here
      bytes_live_ -= (int64_t)it->second;
      allocs_.erase(it);
      frees_total_++; frees_unknown_++;
    }
    allocs_.emplace(p, bytes);
    bytes_live_ += (int64_t)bytes;
    allocs_total_++;
  }
  // ok: the runtime released it.  A NULL pointer is no release at all.
  void free(const void* p, bool ok) {
    if (!p) return;
    std::lock_guard<std::mutex> g(mu_);
    if (!ok) { release_errors_++; return; }
    auto it = allocs_.find(p);
    if (it == allocs_.end()) { frees_unknown_++; return; }
    bytes_live_ -= (int64_t)it->second;
    allocs_.erase(it);
    frees_total_++;
  }
  void event_create(const void* e) { insert(events_, e); }
  void event_destroy(const void* e, bool ok) { remove(events_, e, ok); }
  void stream_create(const void* s) { insert(streams_, s); }
  void stream_destroy(const void* s, bool ok) { remove(streams_, s, ok); }
  void handle(Handle h, int delta) {
    std::lock_guard<std::mutex> g(mu_);
    handles_[h] += delta;
  }
  // the first min(n, COUNT) fields in the order of Field; returns COUNT
  int snapshot(int64_t* out, int n) const {
    std::lock_guard<std::mutex> g(mu_);
    const int64_t v[COUNT] = {(int64_t)allocs_.size(), bytes_live_, (int64_t)events_.size(), (int64_t)streams_.size(),
                              handles_[CTX], handles_[MODEL], handles_[SESSION], allocs_total_, frees_total_, frees_unknown_, release_errors_};
    for (int i = 0; i < n && i < COUNT; i++) out[i] = v[i];
    return COUNT;
  }

 private:
  typedef std::unordered_set<const void*> Set;
  void insert(Set& s, const void* h) {
    if (!h) return;
    std::lock_guard<std::mutex> g(mu_);
    if (!s.insert(h).second) frees_unknown_++;  // created again while held: its destroy never came here
  }
  void remove(Set& s, const void* h, bool ok) {
    if (!h) return;
    std::lock_guard<std::mutex> g(mu_);
    if (!ok) { release_errors_++; return; }
    if (!s.erase(h)) frees_unknown_++;
  }
  mutable std::mutex mu_;
  std::unordered_map<const void*, size_t> allocs_;
  Set events_, streams_;
  int64_t handles_[3] = {0, 0, 0};
  int64_t bytes_live_ = 0, allocs_total_ = 0, frees_total_ = 0, frees_unknown_ = 0, release_errors_ = 0;
};
}  // namespace ledger
