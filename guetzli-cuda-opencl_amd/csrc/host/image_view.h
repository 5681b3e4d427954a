// An input image as the caller holds it (gz_image of the C ABI): 1 to 4
// channels of u8, u16, f16 or f32 samples at any byte strides, in host memory
// or in HBM.  Sample c of pixel (x, y) is at
//   data + y * row_stride + x * pixel_stride + channel_offset[c],
// which covers HWC and CHW, BGR / BGRA / ARGB (the offsets), gray, crops and
// step slices, bottom-up and mirrored rows (negative strides) and broadcasts
// (a stride of 0).
//
// The image an encode starts from is its tight RGB8 form P, defined here
// once for the host packer (PackImage) and the device import kernel
// (k_import_image) alike: every sample becomes 8 bits by Sample<S>::Quant,
// then the channels combine as the PNG reader's do (quantise first, blend on
// black second).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "frame.h"

namespace gz {

enum ImageSample { kSampleU8 = 0, kSampleU16 = 1, kSampleF16 = 2, kSampleF32 = 3 };

GZ_HOST_DEVICE inline int SampleBytes(int sample) {
  return sample == kSampleU8 ? 1 : sample == kSampleF32 ? 4 : 2;
}

// The bits of the f32 that equals the f16 with bits h (every f16 is an f32).
GZ_HOST_DEVICE inline uint32_t HalfBitsToFloatBits(uint16_t h) {
  const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16;
  const uint32_t exp = (h >> 10) & 31u, man = h & 1023u;
  if (exp == 31u) return sign | 0x7f800000u | (man << 13);  // inf, NaN
  if (exp != 0u) return sign | ((exp + 112u) << 23) | (man << 13);
  if (man == 0u) return sign;
  // subnormal: man * 2^-24, its leading one moved to the implicit position
  const uint32_t shift = static_cast<uint32_t>(__builtin_clz(man)) - 21u;
  return sign | ((113u - shift) << 23) | (((man << shift) & 1023u) << 13);
}

GZ_HOST_DEVICE inline float FloatFromBits(uint32_t bits) {
  float f;
  memcpy(&f, &bits, sizeof(f));
  return f;
}

// NaN -> 0, else rint(min(max(s, 0), 1) * 255): one IEEE f32 multiply, then
// round to nearest, ties to even.  (-0, negatives and -inf give 0; values at
// or above 1 and +inf give 255.)
GZ_HOST_DEVICE inline uint8_t QuantF32(float s) {
  if (!(s > 0.0f)) return 0;
  if (s >= 1.0f) return 255;
  return static_cast<uint8_t>(rintf(s * 255.0f));
}

// Raw: a sample as it lies in memory; Quant: its 8-bit value.
template <int S>
struct Sample;
template <>
struct Sample<kSampleU8> {
  typedef uint8_t Raw;
  GZ_HOST_DEVICE static uint8_t Quant(Raw s) { return s; }
};
template <>
struct Sample<kSampleU16> {  // the PNG reader's STRIP_16
  typedef uint16_t Raw;
  GZ_HOST_DEVICE static uint8_t Quant(Raw s) { return static_cast<uint8_t>(s >> 8); }
};
template <>
struct Sample<kSampleF16> {
  typedef uint16_t Raw;
  GZ_HOST_DEVICE static uint8_t Quant(Raw s) { return QuantF32(FloatFromBits(HalfBitsToFloatBits(s))); }
};
template <>
struct Sample<kSampleF32> {
  typedef float Raw;
  GZ_HOST_DEVICE static uint8_t Quant(Raw s) { return QuantF32(s); }
};

// P's pixel from the quantised channels q (R, G, B, A; gray: V, A).
GZ_HOST_DEVICE inline void RgbFromQuant(int channels, const uint8_t q[4], uint8_t out[3]) {
  if (channels == 3) {
    out[0] = q[0], out[1] = q[1], out[2] = q[2];
  } else if (channels == 4) {
    out[0] = BlendOnBlack(q[0], q[3]), out[1] = BlendOnBlack(q[1], q[3]), out[2] = BlendOnBlack(q[2], q[3]);
  } else {
    out[0] = out[1] = out[2] = channels == 2 ? BlendOnBlack(q[0], q[1]) : q[0];
  }
}

// P's pixel from the pixel at address p: one load per sample, of the
// sample's own bytes.
template <int S>
GZ_HOST_DEVICE inline void ImagePixel(const uint8_t* p, int channels, const ptrdiff_t offset[4], uint8_t out[3]) {
  typedef typename Sample<S>::Raw Raw;
  uint8_t q[4] = {0, 0, 0, 0};
  for (int c = 0; c < 4; ++c)
    if (c < channels) q[c] = Sample<S>::Quant(*reinterpret_cast<const Raw*>(p + offset[c]));
  RgbFromQuant(channels, q, out);
}

struct ImageView {
  const uint8_t* data = nullptr;  // the address the offsets are relative to
  int w = 0, h = 0;
  int channels = 3;  // 1: gray, 2: gray + alpha, 3: RGB, 4: RGBA
  int sample = kSampleU8;
  ptrdiff_t row_stride = 0, pixel_stride = 0;  // bytes; literal: 0 is a broadcast
  ptrdiff_t channel_offset[4] = {0, 0, 0, 0};  // entries at index >= channels are ignored
  bool on_device = false;
};

// nullptr if the view describes an image, else what is wrong with it (the
// field by its gz_image name).  Every sample must be naturally aligned.
inline const char* ImageError(const ImageView& v) {
  if (!v.data) return "data is null";
  if (v.w <= 0 || v.h <= 0) return "width and height must be positive";
  if (v.w >= (1 << 16) || v.h >= (1 << 16)) return "width and height must be below 65536";
  if (v.channels < 1 || v.channels > 4) return "channels must be 1 (gray), 2 (gray + alpha), 3 (RGB) or 4 (RGBA)";
  if (v.sample < kSampleU8 || v.sample > kSampleF32) return "sample must be GZ_SAMPLE_U8, _U16, _F16 or _F32";
  const ptrdiff_t sb = SampleBytes(v.sample);
  if (reinterpret_cast<uintptr_t>(v.data) % sb != 0) return "data is not aligned to the sample size";
  if (v.row_stride % sb != 0) return "row_stride is not a multiple of the sample size";
  if (v.pixel_stride % sb != 0) return "pixel_stride is not a multiple of the sample size";
  for (int c = 0; c < v.channels; ++c)
    if (v.channel_offset[c] % sb != 0) return "channel_offset is not a multiple of the sample size";
  return nullptr;
}

template <int S>
inline void PackImageRows(const ImageView& v, uint8_t* out) {
  for (int y = 0; y < v.h; ++y) {
    const uint8_t* row = v.data + static_cast<ptrdiff_t>(y) * v.row_stride;
    uint8_t* d = out + static_cast<size_t>(y) * v.w * 3;
    for (int x = 0; x < v.w; ++x, d += 3)
      ImagePixel<S>(row + static_cast<ptrdiff_t>(x) * v.pixel_stride, v.channels, v.channel_offset, d);
  }
}

// P of an image in host memory (ImageError(v) == nullptr): 3 * w * h bytes.
inline void PackImage(const ImageView& v, uint8_t* out) {
  switch (v.sample) {
    case kSampleU8: return PackImageRows<kSampleU8>(v, out);
    case kSampleU16: return PackImageRows<kSampleU16>(v, out);
    case kSampleF16: return PackImageRows<kSampleF16>(v, out);
    default: return PackImageRows<kSampleF32>(v, out);
  }
}

}  // namespace gz
