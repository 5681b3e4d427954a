// An input frame as the caller holds it (gz_frame of the C ABI): interleaved
// 8-bit RGB or RGBA, rows `stride` bytes apart, in host memory or in HBM.
// The image an encode starts from is its tight RGB8 form P: the pixels as
// they are for 3 channels, blended on black for 4 (the reference's ReadPNG
// rule, guetzli.cc:47-49).  BlendOnBlack is that rule for the PNG reader, the
// host packer below and the device import kernel (k_import_rgb8) alike.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIP__
#define GZ_HOST_DEVICE __host__ __device__
#else
#define GZ_HOST_DEVICE
#endif

namespace gz {

GZ_HOST_DEVICE inline uint8_t BlendOnBlack(uint8_t v, uint8_t a) {  // guetzli.cc:47-49
  return static_cast<uint8_t>((static_cast<int>(v) * static_cast<int>(a) + 128) / 255);
}

struct FrameView {
  const uint8_t* data = nullptr;  // first byte of the top-left pixel
  int w = 0, h = 0;
  int channels = 3;   // 3: RGB, 4: RGBA
  size_t stride = 0;  // bytes from one row to the next (never 0 here)
  bool on_device = false;

  size_t row_bytes() const { return static_cast<size_t>(w) * channels; }
  // Already P: the existing entry points' input.
  bool tight_rgb() const { return channels == 3 && stride == row_bytes(); }
};

// nullptr if the view describes a frame, else what is wrong with it.
inline const char* FrameError(const FrameView& f) {
  if (!f.data) return "null frame data";
  if (f.w <= 0 || f.h <= 0) return "frame sizes must be positive";
  if (f.w >= (1 << 16) || f.h >= (1 << 16)) return "frame sizes must be below 65536";
  if (f.channels != 3 && f.channels != 4) return "channels must be 3 (RGB) or 4 (RGBA)";
  if (f.stride < f.row_bytes()) return "row_stride is below width * channels";
  return nullptr;
}

// P of a frame in host memory: 3 * w * h bytes.
inline void PackFrame(const FrameView& f, uint8_t* out) {
  for (int y = 0; y < f.h; ++y) {
    const uint8_t* s = f.data + static_cast<size_t>(y) * f.stride;
    uint8_t* d = out + static_cast<size_t>(y) * f.w * 3;
    if (f.channels == 3) {
      for (size_t i = 0; i < f.row_bytes(); ++i) d[i] = s[i];
    } else {
      for (int x = 0; x < f.w; ++x, s += 4, d += 3) {
        d[0] = BlendOnBlack(s[0], s[3]);
        d[1] = BlendOnBlack(s[1], s[3]);
        d[2] = BlendOnBlack(s[2], s[3]);
      }
    }
  }
}

}  // namespace gz
