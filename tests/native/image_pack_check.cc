// The host packer of host/image_view.h reads the addressed samples and no
// other byte: every source here is allocated at exactly the span of the
// samples its descriptor addresses (negative strides put `data` at the far
// end), so that AddressSanitizer sees any read outside it, and the packed
// image is compared with a plain triple loop over the definition.
// Built by tests/test_image_host.py with -fsanitize=address,undefined.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host/image_view.h"

namespace {

uint32_t g_rng = 12345u;
uint32_t Next() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

// q of one sample, written from the definition (not the header's helpers).
uint8_t PlainQuant(int sample, const uint8_t* p) {
  if (sample == gz::kSampleU8) return *p;
  if (sample == gz::kSampleU16) {
    uint16_t v;
    memcpy(&v, p, 2);
    return static_cast<uint8_t>(v >> 8);
  }
  float f;
  if (sample == gz::kSampleF32) {
    memcpy(&f, p, 4);
  } else {
    uint16_t v;
    memcpy(&v, p, 2);
    const int e = (v >> 10) & 31, m = v & 1023;
    f = e == 31 ? (m ? NAN : INFINITY) : e == 0 ? ldexpf(static_cast<float>(m), -24)
                                                : ldexpf(static_cast<float>(m + 1024), e - 25);
    if (v & 0x8000) f = -f;
  }
  if (f != f) return 0;
  const float t = fminf(fmaxf(f, 0.0f), 1.0f);
  return static_cast<uint8_t>(nearbyintf(t * 255.0f));
}

int Blend(int v, int a) { return (v * a + 128) / 255; }

struct Layout {
  const char* name;
  int w, h, channels, sample;
  ptrdiff_t row_stride, pixel_stride, offset[4];  // in samples
};

bool Check(const Layout& l) {
  const ptrdiff_t sb = gz::SampleBytes(l.sample);
  // the span of the addressed samples, relative to data
  ptrdiff_t lo = 0, hi = 0;
  bool first = true;
  for (int y = 0; y < l.h; y += l.h > 1 ? l.h - 1 : 1)
    for (int x = 0; x < l.w; x += l.w > 1 ? l.w - 1 : 1)
      for (int c = 0; c < l.channels; ++c) {
        const ptrdiff_t at = (y * l.row_stride + x * l.pixel_stride + l.offset[c]) * sb;
        if (first || at < lo) lo = at;
        if (first || at + sb > hi) hi = at + sb;
        first = false;
      }
  const size_t span = static_cast<size_t>(hi - lo);
  uint8_t* mem = static_cast<uint8_t*>(malloc(span));
  for (size_t i = 0; i < span; ++i) mem[i] = static_cast<uint8_t>(Next());
  if (l.sample == gz::kSampleF32) {
    // floats on both sides of [0, 1] rather than random exponents
    for (size_t i = 0; i + 4 <= span; i += 4) {
      const float f = static_cast<float>(Next() % 3001) / 2000.0f - 0.25f;
      memcpy(mem + i, &f, 4);
    }
  }
  gz::ImageView v;
  v.data = mem - lo;
  v.w = l.w;
  v.h = l.h;
  v.channels = l.channels;
  v.sample = l.sample;
  v.row_stride = l.row_stride * sb;
  v.pixel_stride = l.pixel_stride * sb;
  for (int c = 0; c < 4; ++c) v.channel_offset[c] = l.offset[c] * sb;
  if (const char* bad = gz::ImageError(v)) {
    printf("%s: refused: %s\n", l.name, bad);
    free(mem);
    return false;
  }
  std::vector<uint8_t> got(static_cast<size_t>(3) * l.w * l.h), want(got.size());
  gz::PackImage(v, got.data());
  for (int y = 0; y < l.h; ++y)
    for (int x = 0; x < l.w; ++x) {
      int q[4] = {0, 0, 0, 0};
      for (int c = 0; c < l.channels; ++c)
        q[c] = PlainQuant(l.sample, v.data + y * v.row_stride + x * v.pixel_stride + v.channel_offset[c]);
      uint8_t* d = &want[(static_cast<size_t>(y) * l.w + x) * 3];
      for (int c = 0; c < 3; ++c)
        d[c] = static_cast<uint8_t>(l.channels == 1   ? q[0]
                                    : l.channels == 2 ? Blend(q[0], q[1])
                                    : l.channels == 3 ? q[c]
                                                      : Blend(q[c], q[3]));
    }
  free(mem);
  if (got != want) {
    printf("%s: packed image differs from the definition\n", l.name);
    return false;
  }
  printf("%s: ok (%zu source bytes)\n", l.name, span);
  return true;
}

}  // namespace

int main() {
  const Layout layouts[] = {
      {"hwc_rgb_u8_tight", 7, 5, 3, gz::kSampleU8, 21, 3, {0, 1, 2, 0}},
      {"hwc_bgra_u16_mirrored", 9, 4, 4, gz::kSampleU16, 40, -4, {2, 1, 0, 3}},
      {"chw_rgb_f32_bottom_up", 6, 7, 3, gz::kSampleF32, -6, 1, {0, 42, 84, 0}},
      {"gray_f16_step_slice", 11, 3, 1, gz::kSampleF16, 70, 3, {0, 0, 0, 0}},
      {"gray_u8_broadcast_to_rgb", 13, 2, 3, gz::kSampleU8, 13, 1, {0, 0, 0, 0}},
      {"la_u8_both_negative", 5, 6, 2, gz::kSampleU8, -10, -2, {0, 1, 0, 0}},
      {"argb_f32_planar_reversed_planes", 4, 3, 4, gz::kSampleF32, 4, 1, {-12, -24, -36, 0}},
      {"row_broadcast_u16", 8, 5, 1, gz::kSampleU16, 0, 1, {0, 0, 0, 0}},
      {"one_pixel_f16", 1, 1, 2, gz::kSampleF16, 0, 0, {1, 0, 0, 0}},
  };
  bool ok = true;
  for (const Layout& l : layouts) ok = Check(l) && ok;
  return ok ? 0 : 1;
}
