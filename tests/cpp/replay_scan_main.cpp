// The scan of the replay entries (csrc/replay_scan.h) shown to report a write where there is one.  Host buffers are built the way
// tsd_debug_gemm_run / _norm_run / _attn_run lay their operands out - guard band, extent, guard band, filled with the NaN pattern of
// the element size - and single elements are flipped: the count is 0 on an untouched image, 1 for every flip outside the logical
// elements, and 0 for any flip inside them.  tests/test_replay_scan_cpu.py builds this file under the host sanitizers and runs it.
#include <stdio.h>

#include "replay_scan.h"

using replay::Box;

static int failures = 0;
#define CHECK(expr, want)                                                                            \
  do {                                                                                               \
    const long long got__ = (long long)(expr);                                                       \
    if (got__ != (long long)(want)) {                                                                \
      printf("line %d: %s = %lld, expected %lld\n", __LINE__, #expr, got__, (long long)(want));      \
      failures++;                                                                                    \
    }                                                                                                \
  } while (0)

// One operand as an entry reads it back: `guard` elements, `ext` elements, `guard` elements of T (uint16_t or uint32_t)
template <class T>
struct Image {
  static constexpr T FILL = sizeof(T) == 2 ? (T)replay::NAN16 : (T)replay::NAN32;
  int64_t guard, ext;
  Box box;
  std::vector<T> img, before;  // before: the payload an in-place output was started from (empty: it held the fill)
  Image(int64_t g, int64_t e, const Box& b, bool inplace) : guard(g), ext(e), box(b), img((size_t)(2 * g + e), FILL) {
    if (inplace) {
      for (int64_t j = 0; j < e; j++) before.push_back((T)(0x3C00 + j));
      std::copy(before.begin(), before.end(), img.begin() + g);
    }
  }
  int64_t scan(const std::vector<T>& v) const {
    return replay::scan_changed(v.data(), guard, ext, (int)sizeof(T), box, before.empty() ? nullptr : before.data());
  }
  // the count after element `i` of the image (bands included) was set to `v`
  int64_t with(int64_t i, T v) const {
    std::vector<T> c = img;
    c[(size_t)i] = v;
    return scan(c);
  }
  bool logical(int64_t j) const {
    for (int64_t b = 0; b < box.batch; b++)
      for (int64_t r = 0; r < box.rows; r++) {
        const int64_t off = b * box.stride + r * box.pitch;
        if (j >= off && j < off + box.width) return true;
      }
    return false;
  }
};

// every element of the image flipped on its own: counted exactly once outside the logical elements, never inside them
template <class T>
static void every_flip(const Image<T>& m, int64_t gaps_expected) {
  CHECK(m.scan(m.img), 0);
  int64_t gaps = 0;
  for (int64_t i = 0; i < (int64_t)m.img.size(); i++) {
    const int64_t j = i - m.guard;
    const bool in = j >= 0 && j < m.ext && m.logical(j);
    if (j >= 0 && j < m.ext && !in) gaps++;
    CHECK(m.with(i, (T)(m.img[(size_t)i] ^ 1)), in ? 0 : 1);
  }
  CHECK(gaps, gaps_expected);
}

int main() {
  // fp16, a pitched output: 3 rows of 5 in a pitch of 8 (the last row ends the extent), 6 gap elements
  const Image<uint16_t> y(16, 2 * 8 + 5, Box{1, 0, 3, 8, 5}, false);
  every_flip(y, 6);
  CHECK(y.with(0, 0), 1);                                    // leading band, element 0
  CHECK(y.with(2 * 16 + y.ext - 1, 0x3C00), 1);              // trailing band, last element
  CHECK(y.with(16 + 5, 0x3C00), 1);                          // first pitch gap
  CHECK(y.with(16 + 8 + 2, replay::NAN16), 0);               // a logical element rewritten with the very fill
  CHECK(y.with(3, 0x7E5B), 1);                               // a band element rewritten with another NaN payload
  CHECK(y.with(16 + 7, 0x7E00), 1);                          // ... and a gap element
  // fp32, a batch-strided box: 2 batches 30 apart of 2 rows of 3 in a pitch of 4, then a batch gap
  const Image<uint32_t> o(8, 30 + 4 + 3, Box{2, 30, 2, 4, 3}, false);
  every_flip(o, 37 - 12);
  CHECK(o.with(8 + 3, 0), 1);                                // pitch gap of batch 0
  CHECK(o.with(8 + 7, 0), 1);                                // batch gap
  CHECK(o.with(8 + 30, 0), 0);                               // first logical element of batch 1
  CHECK(o.with(8 + 31, replay::NAN32), 0);
  CHECK(o.with(7, 0x7FC5A5A4u), 1);                          // band, one payload bit off the fill
  CHECK(o.with(8 + 37, 0x7E5A7E5Au), 1);                     // trailing band, the fp16 fill twice is not the fp32 fill
  // fp32 dense (a statistics table): no gap at all
  every_flip(Image<uint32_t>(4, 10, Box::dense(10), false), 0);
  // an input: its two bands back to back, no extent, no logical element
  every_flip(Image<uint16_t>(32, 0, Box(), false), 0);
  // fp16 rows processed in place: the gaps hold the caller's payload, the bands the fill
  const Image<uint16_t> x(16, 3 * 6 + 4, Box{1, 0, 4, 6, 4}, true);
  every_flip(x, 6);
  CHECK(x.with(16 + 4, replay::NAN16), 1);                   // a gap of an in-place image set to the fill: it held the payload
  CHECK(x.with(16 + 4, x.before[4]), 0);
  CHECK(x.with(16 + 6, replay::NAN16), 0);                   // logical
  CHECK(x.with(15, x.before[0]), 1);                         // the band of an in-place image holds the fill, not the payload
  // several writes are all counted; an empty box makes every element of the extent a gap (a launch over no rows)
  std::vector<uint16_t> c = y.img;
  c[0] = c[16 + 5] = c[16 + 6] = c[c.size() - 1] = 0;
  c[16] = 0;                                                 // logical
  CHECK(y.scan(c), 4);
  const Image<uint16_t> none(8, 12, Box{1, 12, 0, 6, 4}, false);
  every_flip(none, 12);
  if (failures) return 1;
  printf("replay_scan: every flip outside the logical elements counted once, none inside\n");
  return 0;
}
