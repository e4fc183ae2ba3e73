// replay_scan.h - the one rule the replay entries (api_replay.cpp) hold a launch to: every element that is no logical output element
// holds after the launch what it held before it - the fill pattern in the guard bands and in an output's pitch gaps, the uploaded
// payload where an output was started from one (rows processed in place, C aliased with R).  Host buffers only: no HIP, no common.h
// (tests/cpp/replay_scan_main.cpp compiles it alone, under the host sanitizers).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace replay {
constexpr uint16_t NAN16 = 0x7E5A;       // fp16 quiet NaN
constexpr uint32_t NAN32 = 0x7FC5A5A5u;  // fp32 quiet NaN (a byte-wise fill that is an fp16 NaN is a finite fp32)

// The logical elements of an output: `batch` boxes `stride` apart, each `rows` rows `pitch` apart of `width` elements.  The rest of the
// extent is pitch gap; an input has no logical element (Box()).
struct Box {
  int64_t batch = 0, stride = 0, rows = 0, pitch = 0, width = 0;
  static Box dense(int64_t n) { return Box{1, 0, 1, 0, n}; }
};

// img: `guard` elements, `ext` elements, `guard` elements of `es` (2 or 4) bytes, as read back after the launch.  before: the `ext`
// elements uploaded before it, or NULL when the extent held the fill.  Returns how many non-logical elements changed.
inline int64_t scan_changed(const void* img, int64_t guard, int64_t ext, int es, const Box& box, const void* before) {
  std::vector<char> logical((size_t)ext, 0);
  for (int64_t b = 0; b < box.batch; b++)
    for (int64_t r = 0; r < box.rows; r++) {
      const int64_t off = b * box.stride + r * box.pitch;
      if (off >= ext) break;
      memset(&logical[(size_t)off], 1, (size_t)std::min(box.width, ext - off));
    }
  const char* fill = es == 2 ? (const char*)&NAN16 : (const char*)&NAN32;
  int64_t changed = 0;
  for (int64_t i = 0; i < ext + 2 * guard; i++) {
    const int64_t j = i - guard;
    const bool inside = j >= 0 && j < ext;
    if (inside && logical[(size_t)j]) continue;
    const char* was = inside && before ? (const char*)before + j * es : fill;
    if (memcmp((const char*)img + i * es, was, (size_t)es)) changed++;
  }
  return changed;
}
}  // namespace replay
