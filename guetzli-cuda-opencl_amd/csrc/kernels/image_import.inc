// An image as the caller holds it in HBM (host/image_view.h: any strides,
// 1-4 channels, u8 / u16 / f16 / f32 samples) -> its tight RGB8 image P and
// the planar linear image k_rgb_to_linear forms from that: the two planes
// k_import_rgb8 leaves, in one pass over the source.  The per-sample and
// per-pixel arithmetic is host/image_view.h's, the host packer's own.
//
// Block (bx, y) works on row y; consecutive lanes take consecutive pixels.
// Two paths, chosen on the host (ImportImagePaths) and passed as kernel
// arguments, so every branch on them is wave-uniform:
//   generic  any strides, offsets and alignment the descriptor admits; a
//            lane takes one pixel and issues one load per sample.
//   wide     pixel_stride == the sample size (planar images, row-contiguous
//            gray) with the row stride and every channel's first sample
//            aligned to four samples: a lane takes four consecutive pixels
//            with one load of four samples per channel.  The lane at a row's
//            tail (w % 4 pixels) loads them sample by sample, so no load
//            covers a byte the descriptor does not address.
//   wstore   (wide only) w % 4 == 0: the lane's 12 bytes of P go out as three
//            dwords and its four linear values per plane as one 16-byte store.
// Included by gz_device.hip.
#pragma once

#include "../host/image_view.h"

namespace gz {

struct ImportImageArgs {
  const uint8_t* data;
  long long row_stride, pixel_stride, offset[4];
  int channels, w, h;
  int wide, wstore;
};

// Four consecutive samples of one channel, as one load.
template <int S>
struct alignas(4 * sizeof(typename Sample<S>::Raw)) SampleQuad {
  typename Sample<S>::Raw v[4];
};

__device__ __forceinline__ void store_pixel(const uint8_t px[3], size_t i, size_t n, uint8_t* __restrict__ rgb,
                                            float* __restrict__ lin) {
  rgb[3 * i] = px[0];
  rgb[3 * i + 1] = px[1];
  rgb[3 * i + 2] = px[2];
  if (lin) {
    lin[i] = c_tab.srgb[px[0]];
    lin[n + i] = c_tab.srgb[px[1]];
    lin[2 * n + i] = c_tab.srgb[px[2]];
  }
}

// lin == nullptr: P alone (images too small for an engine).
template <int S>
__global__ __launch_bounds__(256) void k_import_image(ImportImageArgs a, uint8_t* __restrict__ rgb,
                                                      float* __restrict__ lin) {
  typedef typename Sample<S>::Raw Raw;
  const int y = blockIdx.y;
  if (y >= a.h) return;
  const uint8_t* row = a.data + static_cast<long long>(y) * a.row_stride;
  const size_t n = static_cast<size_t>(a.w) * a.h;
  ptrdiff_t off[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) off[c] = static_cast<ptrdiff_t>(a.offset[c]);

  if (!a.wide) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= a.w) return;
    uint8_t px[3];
    ImagePixel<S>(row + static_cast<long long>(x) * a.pixel_stride, a.channels, off, px);
    store_pixel(px, static_cast<size_t>(y) * a.w + x, n, rgb, lin);
    return;
  }

  const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (x0 >= a.w) return;
  const int cnt = a.w - x0 < 4 ? a.w - x0 : 4;
  const uint8_t* p = row + static_cast<size_t>(x0) * sizeof(Raw);
  uint8_t q[4][4];  // [pixel][channel]
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c) q[k][c] = 0;
  if (cnt == 4) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < a.channels) {
        const SampleQuad<S> v = *reinterpret_cast<const SampleQuad<S>*>(p + off[c]);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k][c] = Sample<S>::Quant(v.v[k]);
      }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < cnt) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < a.channels)
            q[k][c] = Sample<S>::Quant(*reinterpret_cast<const Raw*>(p + k * sizeof(Raw) + off[c]));
      }
  }
  uint8_t px[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) RgbFromQuant(a.channels, q[k], px[k]);
  const size_t i = static_cast<size_t>(y) * a.w + x0;
  if (a.wstore) {
    // (w % 4 == 0: cnt == 4, and 3 * i and every plane's i are multiples of 4)
    uint32_t* d = reinterpret_cast<uint32_t*>(rgb + 3 * i);
    d[0] = px[0][0] | px[0][1] << 8 | px[0][2] << 16 | static_cast<uint32_t>(px[1][0]) << 24;
    d[1] = px[1][1] | px[1][2] << 8 | px[2][0] << 16 | static_cast<uint32_t>(px[2][1]) << 24;
    d[2] = px[2][2] | px[3][0] << 8 | px[3][1] << 16 | static_cast<uint32_t>(px[3][2]) << 24;
    if (lin) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(lin + c * n + i) = make_float4(c_tab.srgb[px[0][c]], c_tab.srgb[px[1][c]],
                                                                   c_tab.srgb[px[2][c]], c_tab.srgb[px[3][c]]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) store_pixel(px[k], i + k, n, rgb, lin);
  }
}

// The path selectors of an image (the eligibility conditions above).
inline void ImportImagePaths(const ImageView& v, int* wide, int* wstore) {
  const ptrdiff_t quad = 4 * SampleBytes(v.sample);
  bool ok = v.pixel_stride == SampleBytes(v.sample) && v.row_stride % quad == 0;
  for (int c = 0; c < v.channels; ++c)
    ok = ok && reinterpret_cast<uintptr_t>(v.data + v.channel_offset[c]) % quad == 0;
  *wide = ok;
  *wstore = ok && v.w % 4 == 0;
}

// Launches the import of v (ImageError(v) == nullptr, v in this device's HBM)
// on stream s; rgb: 3 * w * h bytes, lin: 3 * w * h floats or nullptr, both
// 16-byte aligned.
inline void LaunchImportImage(const ImageView& v, uint8_t* rgb, float* lin, hipStream_t s) {
  ImportImageArgs a;
  a.data = v.data;
  a.row_stride = v.row_stride;
  a.pixel_stride = v.pixel_stride;
  for (int c = 0; c < 4; ++c) a.offset[c] = c < v.channels ? v.channel_offset[c] : 0;
  a.channels = v.channels;
  a.w = v.w;
  a.h = v.h;
  ImportImagePaths(v, &a.wide, &a.wstore);
  const int per_block = a.wide ? 1024 : 256;
  const dim3 grid((v.w + per_block - 1) / per_block, v.h);
  switch (v.sample) {
    case kSampleU8: k_import_image<kSampleU8><<<grid, 256, 0, s>>>(a, rgb, lin); break;
    case kSampleU16: k_import_image<kSampleU16><<<grid, 256, 0, s>>>(a, rgb, lin); break;
    case kSampleF16: k_import_image<kSampleF16><<<grid, 256, 0, s>>>(a, rgb, lin); break;
    default: k_import_image<kSampleF32><<<grid, 256, 0, s>>>(a, rgb, lin); break;
  }
}

}  // namespace gz
