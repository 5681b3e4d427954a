// Full-image Butteraugli distance (the `Comparator::Compare` pass) as CDNA4
// HIP kernels.  Reference semantics: clguetzli/clbutter_comparator.cpp
// DiffmapOpsinDynamicsImageOpt (:1387-1417) and its callees; see
// oracle/gz_oracle.c for the scalar restatement every kernel is tested
// against bit-for-bit.
//
// Layout in HBM: planar f32, one plane per channel, row-major with row
// stride == width.  "res" arrays are interleaved xyz per res point
// (3 * rw * rh), rw = ceil(w/3) (kButteraugliStep = 3).
//
// Parallelisation rule: every output element is produced by one thread that
// accumulates its terms in the reference's order (blur taps ascending, FFT
// butterflies verbatim, block sums sequential) -- we parallelise across
// outputs, never inside a floating-point sum.
// Included by gz_device.hip (single device translation unit: c_tab is shared).
#pragma once

namespace gz {



// ---------------------------------------------------------------------------
// Candidate coefficients -> sRGB pixels, packed r | g << 8 | b << 16 per
// pixel (4 B instead of three linear floats: the linear value is the sRGB
// LUT entry of the byte, which k_opsin_mhic_stream looks up from LDS)
// (OutputImage::ToLinearRGB, output_image.cc:642-716; pixels == IDCT<<4, so
//  the ToPixels rounding (p + 8 - (x&1)) >> 4 returns the IDCT byte itself).
// The integer IDCT (idct.cc:142-160) sums M[r][u] * v[u] in wrapping 32-bit
// arithmetic -- exact and order-free -- so a thread forms a whole column,
// then a whole row, with the matrix as immediates (no table loads).  One
// workgroup = 8 horizontally adjacent 8x8 blocks: coefficients staged with
// 16-B loads, column and row passes by 64 threads per component, then every
// thread converts 2 pixels; a wave stores one 64-pixel row (256-B segments).
// ---------------------------------------------------------------------------

constexpr int kIdctM[64] = {  // idct.cc:29-38 (kIDCTMatrix), row r = output r
    8192, 11363, 10703, 9633,   8192,  6437,   4433,   2260,   8192, 9633,  4433,  -2259, -8192,
    -11362, -10704, -6436, 8192, 6437, -4433,  -11362, -8192, 2261,   10704,  9633, 8192,  2260,
    -10703, -6436, 8192, 9633,  -4433, -11363, 8192,   -2260, -10703, 6436,   8192, -9633, -4433,
    11363,  8192,  -6437, -4433, 11362, -8192, -2261,  10704, -9633,  8192,   -9633, 4433, 2259,
    -8192,  11362, -10704, 6436, 8192,  -11363, 10703, -9633, 8192,   -6437,  4433,  -2260,
};
// M[r] . v in wrapping 32-bit arithmetic as 4 packed 16-bit dot products
// (v_dot2c_i32_i16: |M| < 2^14 and the operands are int16, so every partial
// sum is the same 32-bit value the 8 separate products sum to).
typedef short c2l_v2s __attribute__((ext_vector_type(2)));
// The rounding bias seeds the sum (addition mod 2^32 is order-free).
__device__ __forceinline__ int c2l_dot8(int r, const c2l_v2s (&v)[4], int bias) {
  int acc = bias;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    acc = __builtin_amdgcn_sdot2(c2l_v2s{static_cast<short>(kIdctM[8 * r + 2 * k]),
                                         static_cast<short>(kIdctM[8 * r + 2 * k + 1])},
                                 v[k], acc, false);
  return acc;
}
constexpr int kC2lBlocks = 8;   // blocks per workgroup (one block row)
constexpr int kC2lStride = 72;  // int16 per staged block (bank spread)

// chroma != nullptr (4:2:0): Cb / Cr are the factor-2 pixel planes' state
// ([2][w*h] 16-bit, ToPixels' rounding) instead of an IDCT of components 1, 2.
__global__ __launch_bounds__(256) void k_coeffs_to_srgb8(const int16_t* __restrict__ coeffs,
                                                         int w, int h, int bw, int nblocks,
                                                         uint32_t* __restrict__ px8,
                                                         const uint16_t* __restrict__ chroma) {
  __shared__ int16_t s_coef[3][kC2lBlocks][kC2lStride];
  __shared__ int16_t s_col[3][kC2lBlocks][kC2lStride];
  __shared__ uint8_t s_pix[3][8][kC2lBlocks * 8];
  const int t = threadIdx.x;
  const int by = blockIdx.y, bx0 = blockIdx.x * kC2lBlocks;
  const int nthr = chroma ? 64 : 192;  // 64 threads per IDCT'd component
  const int c = t >> 6, b = (t >> 3) & 7, i8 = t & 7;
  if (t < nthr) {  // 16 B of a block per thread: the component's 8 blocks are contiguous
    const int bx = bx0 + b;
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (bx < bw)
      u = reinterpret_cast<const uint4*>(coeffs + (static_cast<size_t>(c) * nblocks +
                                                   static_cast<size_t>(by) * bw + bx) * 64)[i8];
    uint32_t* d = reinterpret_cast<uint32_t*>(&s_coef[c][b][8 * i8]);
    d[0] = u.x;
    d[1] = u.y;
    d[2] = u.z;
    d[3] = u.w;
  }
  __syncthreads();
  if (t < nthr) {  // column ix = i8: col[r][ix] = (M[r] . block[:, ix] + 1024) >> 11
    c2l_v2s v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = c2l_v2s{s_coef[c][b][16 * k + i8], s_coef[c][b][16 * k + 8 + i8]};
#pragma unroll
    for (int r = 0; r < 8; ++r)
      s_col[c][b][8 * r + i8] = static_cast<int16_t>(c2l_dot8(r, v, 1 << 10) >> 11);
  }
  __syncthreads();
  if (t < nthr) {  // row iy = i8: px[iy][x] = clamp((M[x] . col[iy, :] + (257 << 17)) >> 18)
    const uint4 q = *reinterpret_cast<const uint4*>(&s_col[c][b][8 * i8]);  // 16-B aligned
    const c2l_v2s v[4] = {__builtin_bit_cast(c2l_v2s, q.x), __builtin_bit_cast(c2l_v2s, q.y),
                          __builtin_bit_cast(c2l_v2s, q.z), __builtin_bit_cast(c2l_v2s, q.w)};
#pragma unroll
    for (int x = 0; x < 8; ++x)
      s_pix[c][i8][8 * b + x] = static_cast<uint8_t>(clamp255(c2l_dot8(x, v, 257 << 17) >> 18));
  }
  __syncthreads();
  const size_t n = static_cast<size_t>(w) * h;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = t + 256 * j, iy = p >> 6, xx = p & 63;
    const int x = bx0 * 8 + xx, y = by * 8 + iy;
    if (x >= w || y >= h) continue;
    const size_t q = static_cast<size_t>(y) * w + x;
    int cb, cr;
    if (chroma) {
      cb = pixel_byte(chroma[q], x);
      cr = pixel_byte(chroma[n + q], x);
    } else {
      cb = s_pix[1][iy][xx];
      cr = s_pix[2][iy][xx];
    }
    // YCbCr -> RGB with libjpeg's table entries formed arithmetically (the
    // same integer operations as BuildTables' entries)
    const int yv = s_pix[0][iy][xx], xr = cr - 128, xb = cb - 128;
    const int r = clamp255(yv + ((kFixCrR * xr + 32768) >> 16));
    const int g = clamp255(yv + ((-kFixCrG * xr + (-kFixCbG * xb + 32768)) >> 16));
    const int bl = clamp255(yv + ((kFixCbB * xb + 32768) >> 16));
    px8[q] = static_cast<uint32_t>(r) | (static_cast<uint32_t>(g) << 8) | (static_cast<uint32_t>(bl) << 16);
  }
}

// RGB8 interleaved -> packed sRGB pixels (the candidate given as pixels).
__global__ __launch_bounds__(256) void k_rgb_to_srgb8(const uint8_t* __restrict__ rgb, size_t n,
                                                      uint32_t* __restrict__ px8) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  px8[i] = static_cast<uint32_t>(rgb[3 * i]) | (static_cast<uint32_t>(rgb[3 * i + 1]) << 8) |
           (static_cast<uint32_t>(rgb[3 * i + 2]) << 16);
}

// Packed sRGB pixels -> planar linear (the stage dumps' candidate planes).
__global__ __launch_bounds__(256) void k_srgb8_to_linear(const uint32_t* __restrict__ px8, size_t n,
                                                         float* __restrict__ lin) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = px8[i];
  lin[i] = c_tab.srgb[v & 255];
  lin[n + i] = c_tab.srgb[(v >> 8) & 255];
  lin[2 * n + i] = c_tab.srgb[(v >> 16) & 255];
}

// RGB8 interleaved -> planar linear (butteraugli_comparator.cc:37-44).
__global__ __launch_bounds__(256) void k_rgb_to_linear(const uint8_t* __restrict__ rgb, size_t n,
                                                       float* __restrict__ lin) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  lin[i] = c_tab.srgb[rgb[3 * i]];
  lin[n + i] = c_tab.srgb[rgb[3 * i + 1]];
  lin[2 * n + i] = c_tab.srgb[rgb[3 * i + 2]];
}

// A pitched RGB / RGBA frame in HBM (host/frame.h) -> its tight RGB8 image
// and the planar linear image k_rgb_to_linear forms from that, in one pass
// over the source.  Block (bx, y) takes 256 consecutive pixels of row y, so
// consecutive lanes read consecutive pixels.  channels and dword are kernel
// arguments (wave-uniform branches); dword: 4 channels with base and stride
// 4-byte aligned, one load per pixel.  Reads the pixels' own bytes only.
__global__ __launch_bounds__(256) void k_import_rgb8(const uint8_t* __restrict__ src, size_t stride,
                                                     int channels, int dword, int w, int h,
                                                     uint8_t* __restrict__ rgb, float* __restrict__ lin) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w || y >= h) return;
  const uint8_t* p = src + static_cast<size_t>(y) * stride + static_cast<size_t>(x) * channels;
  uint8_t r, g, b;
  if (channels == 4) {
    uint8_t a;
    if (dword) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
      r = v & 255, g = (v >> 8) & 255, b = (v >> 16) & 255, a = v >> 24;
    } else {
      r = p[0], g = p[1], b = p[2], a = p[3];
    }
    r = BlendOnBlack(r, a), g = BlendOnBlack(g, a), b = BlendOnBlack(b, a);
  } else {
    r = p[0], g = p[1], b = p[2];
  }
  const size_t n = static_cast<size_t>(w) * h, i = static_cast<size_t>(y) * w + x;
  rgb[3 * i] = r;
  rgb[3 * i + 1] = g;
  rgb[3 * i + 2] = b;
  lin[i] = c_tab.srgb[r];
  lin[n + i] = c_tab.srgb[g];
  lin[2 * n + i] = c_tab.srgb[b];
}

// Stages the H x W window of plane `src` at (x0, y0) into LDS `dst` (row
// stride DS), +0 outside the image.  A thread issues all its loads before its
// first LDS store (a load -> store -> load loop keeps one load in flight).
template <int H, int W, int DS>
__device__ __forceinline__ void stage_window(const float* __restrict__ src, int w, int h, int x0,
                                             int y0, float* dst) {
  constexpr int N = H * W, IT = (N + 255) / 256;
  float v[IT];
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int i = threadIdx.x + 256 * k;
    const int ry = i / W, rx = i - ry * W;
    const int y = y0 + ry, x = x0 + rx;
    v[k] = (i < N && x >= 0 && x < w && y >= 0 && y < h) ? src[static_cast<size_t>(y) * w + x] : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < N) {
      const int ry = i / W, rx = i - ry * W;
      dst[ry * DS + rx] = v[k];
    }
  }
}

// ---------------------------------------------------------------------------
// Separable blur, BlurOpt / ConvolutionOpt (clbutter_comparator.cpp:25-94).
// Pass 1 (horizontal) produces tmp[y][ox] at x = ox*step; pass 2 (vertical)
// produces down[oy][ox] at y = oy*step.  Consumers read the nearest-upsampled
// image as down[y/step][x/step] instead of materialising it.
// ---------------------------------------------------------------------------

// Border-renormalised scale of output position `pos` along an axis of `size`.
__device__ __forceinline__ float blur_scale(const BlurSpec& s, int pos, int size, int* lo, int* hi) {
  const int r = s.radius;
  const int minx = pos < r ? 0 : pos - r;
  const int maxx = (size < pos + r + 1 ? size : pos + r + 1) - 1;
  float weight = 0.0f;
  for (int j = minx; j <= maxx; ++j) weight += s.taps[j - pos + r];
  // (1.0 - br) * weight is evaluated in double, br * weight_no_border is a
  // float product (both operands float), then the double sum is rounded.
  weight = static_cast<float>((1.0 - static_cast<double>(s.border_ratio)) * weight +
                              static_cast<double>(s.border_ratio * s.weight_no_border));
  *lo = minx;
  *hi = maxx;
  return static_cast<float>(1.0 / static_cast<double>(weight));
}

// Per-position border scales of every blur, precomputed once per engine:
// scales[(sig * 2 + axis) * stride + pos] for pos < the axis size (w / h;
// the diffmap blur runs on the (w-5)x(h-5) crop).
__global__ __launch_bounds__(256) void k_blur_scales(int w, int h, int stride,
                                                     float* __restrict__ scales) {
  const int sig = blockIdx.y >> 1, axis = blockIdx.y & 1;
  const int pos = blockIdx.x * 256 + threadIdx.x;
  int size = axis ? h : w;
  if (sig == kSigDiffmap) size -= 5;
  if (pos >= size) return;
  int lo, hi;
  scales[static_cast<size_t>(blockIdx.y) * stride + pos] = blur_scale(c_tab.blur[sig], pos, size, &lo, &hi);
}

// Horizontal pass, LDS-tiled.  A workgroup produces 256 consecutive
// (down-sampled) outputs of one row: it stages the input span once
// (coalesced), zero-padded outside the row and de-interleaved by phase
// (x mod step) so that each tap's LDS reads are bank-conflict free, then
// every lane runs the taps in the reference's order.  Zero padding is
// exact: the sum starts at +0, cannot become -0, and x + (+0) == x.
constexpr int kBlurTile = 256;
constexpr int kBlurLds = 1152;  // >= (kBlurTile-1)*step + 2*radius + 1 + step for every spec

struct RowsPlain {  // row y of plane p: in[p][y*w + x]
  const float* in[kMaxBlurPlanes];
  int w;
  __device__ float at(int p, int y, int x) const { return in[p][static_cast<size_t>(y) * w + x]; }
  __device__ const float* row(int p, int y) const { return in[p] + static_cast<size_t>(y) * w; }
  __device__ static float get(const float* r, int x) { return r[x]; }
  static constexpr bool kPlain = true;
};
struct RowsDiffmap {  // the splatted, cropped diffmap: resval[(y/3)*rw + x/3]
  const float* resval;
  int rw;
  __device__ float at(int, int y, int x) const { return resval[static_cast<size_t>(y / 3) * rw + x / 3]; }
  __device__ const float* row(int, int y) const { return resval + static_cast<size_t>(y / 3) * rw; }
  __device__ static float get(const float* r, int x) { return r[x / 3]; }
  static constexpr bool kPlain = false;
};

// Which blur of the pass a launch is (a template tag, so that every blur
// has its own kernel symbol in profiles; the code is the same).
enum BlurStage : int {
  kBlurRefOpsin = 0, kBlurOpsin, kBlurEdge, kBlurLowFreq, kBlurMask, kBlurDiffmap,
  kBlurLfMask,  // the sigma-14 planes and the mask planes of a Compare pass in one launch
};

// (plane, tile, row) of this workgroup in a packed blur grid; kXcd: XCD-aware
// numbering (pays where a pass re-reads many rows -- the sigma-14 vertical
// pass -- and costs where it does not: concentrating each XCD on one band
// of rows loses the spread over HBM channels of the plain order).
// Horizontal pass, register-blocked: every lane produces 4 adjacent
// (down-sampled) outputs of one row, so a wave covers 256 outputs and the
// 2r + 1 taps of its four outputs come from 4 + 2r/step staged values per
// phase instead of 4 * (2r + 1).  A wave stages its row span in its own LDS
// region, de-interleaved by phase (x mod step) with each phase row 16-byte
// aligned, and reads its values back with ds_read_b128 (conflict-free: lane
// l reads from float 4l of each phase row).  The four outputs form two
// packed pairs (v_pk_mul/add, each half an IEEE f32 op); every output still
// adds its taps in ascending order from +0, zero outside the row, then
// takes its border scale -- ConvolutionOpt's arithmetic (clbutter_comparator.cpp:25-55), bit for bit.
// Row stride of a horizontal pass's output (the vertical pass's input):
// even for the down-sampled blurs, so that k_blur_vstream's column pairs are
// 8-byte aligned (the rows still fit the planes: (w/step + 1) * h <= w * h).
template <int kSig>
__host__ __device__ constexpr int blur_hstride(int dx) {
  return BlurGeom<kSig>::STEP > 1 ? (dx + 1) & ~1 : dx;
}

// Input rows per stored row of a horizontal pass's output: the diffmap blur
// reads the 3x3-splatted res map, whose image rows 3j .. 3j + 2 are all res
// row j -- their horizontal sums (and x border scales) are equal, so one
// stored row serves the three.
template <int kSig> struct HRowRep { static constexpr int N = 1; };
template <> struct HRowRep<kSigDiffmap> { static constexpr int N = 3; };

template <int kSig, int K>
struct H4Geom {
  static constexpr int STEP = BlurGeom<kSig>::STEP, R = BlurGeom<kSig>::R, NT = 2 * R + 1;
  static constexpr int OUT = 64 * K;                          // outputs of a wave
  static constexpr int SPAN = OUT * STEP + 2 * R;             // staged elements of a row
  static constexpr int NV = (K + (NT - 1) / STEP + K - 1) / K;  // K-wide reads per phase
  static constexpr int PMIN = OUT + K * NV;                   // phase row length read
  // phase row stride: multiple of 4 (16-byte rows), == 8 mod 32 so the
  // de-interleaving stores of a half-wave spread over the banks
  static constexpr int PST = STEP == 1 ? (PMIN + 3) / 4 * 4 : ((PMIN + 23) / 32) * 32 + 8;
  static constexpr int LDS = STEP * PST;                      // floats per wave
};
constexpr int kH4MaxLds = 688;  // >= H4Geom<s, H4K<s>::K>::LDS for every sigma used (static_assert)
// outputs per lane of each sigma's horizontal pass (2: fewer registers, more waves)
template <int kSig> struct H4K { static constexpr int K = 2; };

template <int kSig, int K, class Rows>
__device__ __forceinline__ void blur_h4_row(const Rows& rows, float* __restrict__ out, int p, int band,
                                            int y, int w, int lane,
                                            const float* __restrict__ scales, int stride,
                                            float* lds) {
  using G = H4Geom<kSig, K>;
  constexpr int STEP = G::STEP, R = G::R, NT = G::NT, NV = G::NV, PST = G::PST;
  constexpr int IT = (G::SPAN + 63) / 64;
  static_assert(G::LDS <= kH4MaxLds, "H4 LDS region");
  static_assert(K == 2 || K == 4, "2 or 4 outputs per lane");
  const BlurSpec& s = c_tab.blur[kSig];
  const int dx = (w + STEP - 1) / STEP;
  const int ox0 = band * G::OUT;
  const int x_begin = ox0 * STEP - R;
  // (the diffmap input repeats each res row over 3 image rows, so its
  // horizontal pass runs on image rows 3 * yr only and stores row yr)
  const float* src = rows.row(p, kSig == kSigDiffmap ? 3 * y : y);
  float v[IT];
  if (Rows::kPlain && x_begin >= 0 && x_begin + IT * 64 <= w) {
    // interior band: one base address, immediate offsets
    const float* b = src + x_begin + lane;
#pragma unroll
    for (int k = 0; k < IT; ++k) v[k] = b[64 * k];
  } else {
#pragma unroll
    for (int k = 0; k < IT; ++k) {  // unconditional loads from clamped columns, zero outside
      const int e = lane + 64 * k, x = x_begin + e;
      const int xc = x < 0 ? 0 : (x < w ? x : w - 1);
      const float t = Rows::get(src, xc);
      v[k] = (e < G::SPAN && x >= 0 && x < w) ? t : 0.0f;
    }
  }
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int e = lane + 64 * k;
    if (e < G::SPAN) lds[(e % STEP) * PST + e / STEP] = v[k];
  }
  // phase rows past the span are read (never used) by the last lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float a[STEP][NV * K];
#pragma unroll
  for (int ph = 0; ph < STEP; ++ph)
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      if constexpr (K == 4) {
        const float4 q = *reinterpret_cast<const float4*>(lds + ph * PST + 4 * lane + 4 * m);
        a[ph][4 * m] = q.x;
        a[ph][4 * m + 1] = q.y;
        a[ph][4 * m + 2] = q.z;
        a[ph][4 * m + 3] = q.w;
      } else {
        const float2 q = *reinterpret_cast<const float2*>(lds + ph * PST + 2 * lane + 2 * m);
        a[ph][2 * m] = q.x;
        a[ph][2 * m + 1] = q.y;
      }
    }
  f32x2 s01 = {0.0f, 0.0f}, s23 = {0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ph = t % STEP, i = t / STEP;
    const float tap = s.taps[t];
    s01 += f32x2{a[ph][i], a[ph][i + 1]} * tap;
    if constexpr (K == 4) s23 += f32x2{a[ph][i + 2], a[ph][i + 3]} * tap;
  }
  const int ox = ox0 + K * lane;
  const float* sx = scales + static_cast<size_t>(kSig * 2) * stride + ox * STEP;
  float* o = out + static_cast<size_t>(y) * blur_hstride<kSig>(dx) + ox;
  const float r[4] = {s01.x, s01.y, s23.x, s23.y};
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (ox + j < dx) o[j] = r[j] * sx[j * STEP];
}

// One wave per (plane, 64*K-output band, row); planes packed along one grid
// axis (bp.tiles = bands per row, bp.start in waves).
template <int kStage, class Rows>
__global__ __launch_bounds__(256) void k_blur_h4(Rows rows, BlurPlanes bp, int w, int h,
                                                 const float* __restrict__ scales, int stride) {
  __shared__ __attribute__((aligned(16))) float lds[4][kH4MaxLds];
  const int wv = wave_id(), lane = threadIdx.x & 63;
  const int item = static_cast<int>(blockIdx.x) * 4 + wv;
  if (item >= bp.start[bp.nplanes]) return;
  int q = 0;
  while (q + 1 < bp.nplanes && item >= bp.start[q + 1]) ++q;
  const int local = item - bp.start[q];
  const int band = local % bp.tiles[q], y = local / bp.tiles[q];
#define GZ_H4(S) blur_h4_row<S, H4K<S>::K>(rows, bp.out[q], q, band, y, w, lane, scales, stride, lds[wv])
  if constexpr (kStage == kBlurLowFreq) {
    GZ_H4(kSigLowFreq);
  } else if constexpr (kStage == kBlurMask || kStage == kBlurLfMask) {
    switch (bp.sig[q]) {
      case kSigLowFreq: if constexpr (kStage == kBlurLfMask) GZ_H4(kSigLowFreq); break;
      case kSigMaskX: GZ_H4(kSigMaskX); break;
      case kSigMaskY: GZ_H4(kSigMaskY); break;
      case kSigMaskBSub: GZ_H4(kSigMaskBSub); break;
      default: GZ_H4(kSigMaskB); break;
    }
  } else {
    GZ_H4(kSigDiffmap);
  }
#undef GZ_H4
}

// Vertical pass on the horizontally down-sampled planes: out[oy][ox] from
// in[j][ox], j in the window of y = oy*step.
// Vertical pass, row streaming with scattered accumulation: a lane owns two
// adjacent down-sampled columns and VsRows<kSig> consecutive outputs; it
// walks down the input rows of that segment once (each row one coalesced
// 8-byte load per lane) and adds the row, times the tap it has for each
// output whose window holds it, into that output's accumulator pair (packed
// f32: the two columns' IEEE results in one instruction).  Rows arrive in
// ascending order, so every output still sums its taps in ascending order
// from +0 -- ConvolutionOpt's column sums bit for bit (rows outside the image are
// +0 and leave a sum unchanged: a sum started at +0 is never -0).  An
// output's window spans A = 2r/step + 1 periods of `step` rows: per period
// acc[d] holds output m - d; the oldest completes in the period and the
// window slides by one at its end.  Rows are loaded VsAhead periods ahead.
// No LDS, no barriers: the four waves of a workgroup are independent items.
// Outputs per lane (measured at 4K: 16 for the sigma-14 pass; 8 for the
// mask and diffmap passes, whose planes give fewer column groups).
template <int kSig> struct VsRows { static constexpr int N = 8; };
template <> struct VsRows<kSigLowFreq> { static constexpr int N = 16; };
// Periods of rows loaded ahead: 4, and 2 for the step-3 mask X blur, whose
// 4 x 3 rows in flight (with its 15 live output pairs and the LUT epilogue)
// would spill in the merged Compare-pass launch.
template <int kSig> struct VsAhead { static constexpr int N = 4; };
template <> struct VsAhead<kSigMaskX> { static constexpr int N = 2; };
constexpr int kVsCols = 128;  // down-sampled columns of a wave
template <int kSig>
struct VsGeom {
  static constexpr int STEP = BlurGeom<kSig>::STEP, R = BlurGeom<kSig>::R;
  static constexpr int A = 2 * R / STEP + 1;   // live outputs per row
  static constexpr int S = VsRows<kSig>::N;    // outputs per lane
  static constexpr int PERIODS = S + A - 1;
};
template <int kSig>
__host__ __device__ constexpr int vstream_segments(int h) {
  return ((h + BlurGeom<kSig>::STEP - 1) / BlurGeom<kSig>::STEP + VsRows<kSig>::N - 1) /
         VsRows<kSig>::N;
}

// Row y (clamped into the image; the caller zeroes rows outside it when it
// consumes them, so that the load is not waited for here).
template <int kSig>
__device__ __forceinline__ void vstream_load(const float* plane, int ds, int h, int y, int ox0,
                                             int ox1, f32x2* v) {
  const int yc = y < 0 ? 0 : (y < h ? y : h - 1);
  const float* r = row_ptr(plane, HRowRep<kSig>::N == 1 ? yc : yc / HRowRep<kSig>::N, ds);
  if constexpr (BlurGeom<kSig>::STEP > 1) {  // even row stride: one 8-byte load
    *v = *reinterpret_cast<const f32x2*>(r + static_cast<unsigned>(ox0));
  } else {
    *v = f32x2{r[static_cast<unsigned>(ox0)], r[static_cast<unsigned>(ox1)]};
  }
}

template <int kSig, bool kLut = false>
__device__ __forceinline__ void blur_vstream_item(const BlurPlanes& bp, int p, int local, int w,
                                                  int h, int lane, const float* __restrict__ scales,
                                                  int stride) {
  using G = VsGeom<kSig>;
  constexpr int STEP = G::STEP, R = G::R, A = G::A, S = G::S, kVsAhead = VsAhead<kSig>::N;
  const BlurSpec& s = c_tab.blur[kSig];
  const int dx = (w + STEP - 1) / STEP, dy = (h + STEP - 1) / STEP;
  const int segs = vstream_segments<kSig>(h);
  const int seg = local % segs, g = local / segs;
  const int ox = g * kVsCols + 2 * lane;
  const bool in0 = ox < dx, in1 = ox + 1 < dx;
  // (an even input row stride for the paired loads, see blur_hstride)
  const int ds = blur_hstride<kSig>(dx);
  const int ox0 = in0 ? ox : (dx - 1) & ~(STEP > 1 ? 1 : 0), ox1 = in1 ? ox + 1 : dx - 1;
  const int oy0 = seg * S;
  const int y_first = oy0 * STEP - R;
  const float* plane = bp.in[p];
  const float* sy = scales + static_cast<size_t>(kSig * 2 + 1) * stride;
  float* out = bp.out[p] + ox;
  // (kLut: compiled only into the merged Compare-pass launch; a plane with
  // out2 set takes the LUT epilogue)
  float* out2 = kLut && bp.out2[p] ? bp.out2[p] + ox : nullptr;
  const bool lut = kLut && out2 != nullptr;
  f32x2 acc[A];
#pragma unroll
  for (int k = 0; k < A; ++k) acc[k] = f32x2{0.0f, 0.0f};
  // rows of periods m .. m + kVsAhead - 1, in register sets that take turns
  // by unrolling (a copy between them would wait for the newer load)
  f32x2 q[kVsAhead][STEP];
#pragma unroll
  for (int k = 0; k < kVsAhead; ++k)
#pragma unroll
    for (int j = 0; j < STEP; ++j)
      vstream_load<kSig>(plane, ds, h, y_first + k * STEP + j, ox0, ox1, &q[k][j]);
  auto period = [&](int m, f32x2* qm) {
    f32x2 cur[STEP];
#pragma unroll
    for (int j = 0; j < STEP; ++j) {
      const int y = y_first + m * STEP + j;
      const bool yin = y >= 0 && y < h;
      cur[j] = f32x2{masked(qm[j].x, yin), masked(qm[j].y, yin)};
      vstream_load<kSig>(plane, ds, h, y + kVsAhead * STEP, ox0, ox1, &qm[j]);  // period m + kVsAhead
    }
    acc[0] = f32x2{0.0f, 0.0f};  // output m starts
#pragma unroll
    for (int j = 0; j < STEP; ++j) {
#pragma unroll
      for (int d = 0; d < A; ++d) {  // output m - d, tap d*STEP + j
        const int t = d * STEP + j;
        if (t <= 2 * R) acc[d] += cur[j] * s.taps[t];
      }
    }
    // output m - (A - 1) took its last tap (2r = (A - 1) * step + 2r mod step)
    const int o = m - (A - 1);
    if (o >= 0 && oy0 + o < dy && o < S) {
      const float sc = sy[(oy0 + o) * STEP];
      const size_t off = static_cast<size_t>(oy0 + o) * dx;
      float* po = out + off;
      const float v0 = acc[A - 1].x * sc, v1 = acc[A - 1].y * sc;
      if (lut) {  // mask planes: the LUT pair of each sample (wave-uniform)
        const int c = kSig == kSigMaskX ? 0 : (kSig == kSigMaskY ? 1 : 2);
        float* pd = out2 + off;
        if (in0) mask_lut_pair(c, v0, &po[0], &pd[0]);
        if (in1) mask_lut_pair(c, v1, &po[1], &pd[1]);
      } else {
        if (in0) po[0] = v0;
        if (in1) po[1] = v1;
      }
    }
#pragma unroll
    for (int d = A - 1; d > 0; --d) acc[d] = acc[d - 1];
  };
  // (extra periods past the last output store nothing: their index is >= S)
  for (int m = 0; m < G::PERIODS; m += kVsAhead) {
#pragma unroll
    for (int k = 0; k < kVsAhead; ++k) period(m + k, q[k]);
  }
}

template <int kStage>
__global__ __launch_bounds__(256, 4) void k_blur_vstream(BlurPlanes bp, int w, int h,
                                                      const float* __restrict__ scales, int stride) {
  const int item = static_cast<int>(blockIdx.x) * 4 + wave_id();
  const int lane = threadIdx.x & 63;
  if (item >= bp.start[bp.nplanes]) return;
  int q = 0;
  while (q + 1 < bp.nplanes && item >= bp.start[q + 1]) ++q;
  const int local = item - bp.start[q];
#define GZ_VS(S) blur_vstream_item<S>(bp, q, local, w, h, lane, scales, stride)
#define GZ_VSL(S) blur_vstream_item<S, kStage == kBlurLfMask>(bp, q, local, w, h, lane, scales, stride)
  if constexpr (kStage == kBlurLowFreq) {
    GZ_VS(kSigLowFreq);
  } else if constexpr (kStage == kBlurMask || kStage == kBlurLfMask) {
    switch (bp.sig[q]) {
      case kSigLowFreq: if constexpr (kStage == kBlurLfMask) GZ_VS(kSigLowFreq); break;
      case kSigMaskX: GZ_VSL(kSigMaskX); break;
      case kSigMaskY: GZ_VSL(kSigMaskY); break;
      case kSigMaskBSub: GZ_VSL(kSigMaskBSub); break;
      default: GZ_VSL(kSigMaskB); break;
    }
  } else {
    GZ_VS(kSigDiffmap);
  }
#undef GZ_VS
#undef GZ_VSL
}

// ---------------------------------------------------------------------------
// Fused 2-D separable blur for the step-1 blurs of small radius (edge
// detector sigmas 1.5 / 0.586 / 0.4; radius <= kB2MaxR): both passes in one
// kernel, the horizontally blurred rows never reach HBM.
// ---------------------------------------------------------------------------
constexpr int kB2MaxR = 3;

struct Blur2DPlanes {
  const float* in[6];
  float* out[6];
  int sig[6];
  int nplanes, tiles_x, tiles_y;  // per plane (all planes share the image size)
};

// Register streaming: a wave covers 64 adjacent
// input columns (lane l = column x0 - kB2MaxR + l) and walks down the rows of
// its segment; the horizontal taps come from lane shuffles (lanes kB2MaxR ..
// 63 - kB2MaxR produce outputs: kBsCols columns per strip), the vertical taps
// from a register queue of the last 2r+1 horizontally blurred rows, and input
// rows are loaded kBsPf rows ahead (unconditional loads from clamped
// addresses, zero-selected outside the image: no branches, no LDS).  Taps
// in ascending order per pass, the intermediate rounded to f32 and scaled
// by its border factor as in the two-pass form; zero padding outside the
// image is exact (the sum starts at +0 and x + (+0) == x): bit-identical to
// BlurOpt's two ConvolutionOpt passes (clbutter_comparator.cpp:25-94).
constexpr int kBsCols = 64 - 2 * kB2MaxR, kBsPf = 8, kBsRows = 32;  // (64 rows: same)

template <int kSig>
__device__ __forceinline__ void blur_stream_strip(const float* __restrict__ in, float* __restrict__ out,
                                                  int w, int h, int x0, int y0, int rows, int lane,
                                                  const float* __restrict__ scales, int stride) {
  constexpr int R = BlurGeom<kSig>::R, NT = 2 * R + 1;
  const BlurSpec& s = c_tab.blur[kSig];
  const int x = x0 - kB2MaxR + lane;
  const bool xin = x >= 0 && x < w;
  const int xc = xin ? x : 0;
  const bool emit = lane >= kB2MaxR && lane < kB2MaxR + kBsCols && x < w;
  const float sxv = x < w ? scales[static_cast<size_t>(kSig * 2) * stride + xc] : 0.0f;
  const float* sy = scales + static_cast<size_t>(kSig * 2 + 1) * stride;
  const int y_end = min(y0 + rows, h);
  const int ya = y0 - R, yb = y_end + R;  // input rows
  auto load = [&](int y) {  // zero outside the image by a bit mask (no branch)
    const bool ok = xin && y >= 0 && y < h;
    const int yc = y < 0 ? 0 : (y < h ? y : h - 1);
    const float v = row_ptr(in, yc, w)[static_cast<unsigned>(xc)];
    return masked(v, ok);
  };
  float pm[kBsPf];
#pragma unroll
  for (int k = 0; k < kBsPf; ++k) pm[k] = load(ya + k);
  // hv[0 .. NT]: horizontally blurred rows y - 2R - 1 .. y + 1 after a pair step
  float hv[NT + 1];
#pragma unroll
  for (int t = 0; t <= NT; ++t) hv[t] = 0.0f;
  // two input rows per step: their horizontal sums, then the two vertical
  // outputs they complete, each as one packed f32 pair
  for (int y = ya; y < yb; y += 2) {
    const float m0 = pm[0], m1 = pm[1];
#pragma unroll
    for (int k = 0; k + 2 < kBsPf; ++k) pm[k] = pm[k + 2];
    pm[kBsPf - 2] = load(y + kBsPf);
    pm[kBsPf - 1] = load(y + kBsPf + 1);
    float a0[NT], a1[NT];  // lane + (t - R)'s values (DPP shifts by the whole wave)
    a0[R] = m0;
    a1[R] = m1;
#pragma unroll
    for (int k = 1; k <= R; ++k) {
      a0[R + k] = wave_next(a0[R + k - 1]);
      a1[R + k] = wave_next(a1[R + k - 1]);
      a0[R - k] = wave_prev(a0[R - k + 1]);
      a1[R - k] = wave_prev(a1[R - k + 1]);
    }
    f32x2 hs = {0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < NT; ++t) hs += f32x2{a0[t], a1[t]} * s.taps[t];
    hs *= sxv;  // x >= w: 0
#pragma unroll
    for (int t = 0; t + 2 <= NT; ++t) hv[t] = hv[t + 2];
    hv[NT - 1] = hs.x;
    hv[NT] = hs.y;
    const int yo = y - R;  // outputs yo (window hv[0..NT-1]) and yo + 1 (hv[1..NT])
    if (yo + 1 >= y0) {
      f32x2 acc = {0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < NT; ++t) acc += f32x2{hv[t], hv[t + 1]} * s.taps[t];
      if (emit && yo >= y0) row_ptr(out, yo, w)[static_cast<unsigned>(x)] = acc.x * sy[yo];
      if (emit && yo + 1 < y_end) row_ptr(out, yo + 1, w)[static_cast<unsigned>(x)] = acc.y * sy[yo + 1];
    }
  }
}

template <int kStage>
__global__ __launch_bounds__(256) void k_blur_stream(Blur2DPlanes bp, int w, int h, int rows,
                                                     const float* __restrict__ scales, int stride) {
  const int lane = threadIdx.x & 63, wv = wave_id();
  const int item = blockIdx.x * 4 + wv;
  const int per_plane = bp.tiles_x * bp.tiles_y;
  if (item >= bp.nplanes * per_plane) return;
  const int p = item / per_plane, t = item % per_plane;
  const int x0 = (t % bp.tiles_x) * kBsCols, y0 = (t / bp.tiles_x) * rows;
#define GZ_BS(S) blur_stream_strip<S>(bp.in[p], bp.out[p], w, h, x0, y0, rows, lane, scales, stride)
  switch (bp.sig[p]) {
    case kSigEdgeX: GZ_BS(kSigEdgeX); break;
    case kSigEdgeY: GZ_BS(kSigEdgeY); break;
    case kSigEdgeB: GZ_BS(kSigEdgeB); break;
    default: GZ_BS(kSigOpsin); break;
  }
#undef GZ_BS
}

// OpsinDynamicsImageOpt (:881-912) as one fused kernel: the sigma-1.1 blur
// (radius 2, step 1) of the three linear planes in 2-D tiles (horizontal
// pass into LDS per plane, vertical pass from LDS) and the opsin transform of
// each pixel from the three blurred values and the linear values.
constexpr int kOpTX = 64, kOpTY = 32, kOpR = 2;
constexpr int kOpInW = kOpTX + 2 * kOpR, kOpInH = kOpTY + 2 * kOpR;

__global__ __launch_bounds__(256) void k_opsin2d(const float* __restrict__ lin, int w, int h,
                                                 int tiles_x, float* __restrict__ xyb,
                                                 const float* __restrict__ scales, int stride) {
  __shared__ float in_t[kOpInH * kOpInW];
  __shared__ float h_t[3][kOpInH * kOpTX];
  const int x0 = (blockIdx.x % tiles_x) * kOpTX, y0 = (blockIdx.x / tiles_x) * kOpTY;
  const BlurSpec& s = c_tab.blur[kSigOpsin];
  const int ntap = 2 * kOpR + 1;
  const size_t n = static_cast<size_t>(w) * h;
  const float* sx = scales + static_cast<size_t>(kSigOpsin * 2) * stride;
  for (int c = 0; c < 3; ++c) {
    stage_window<kOpInH, kOpInW, kOpInW>(lin + c * n, w, h, x0 - kOpR, y0 - kOpR, in_t);
    __syncthreads();
    #pragma unroll
    for (int k_ = 0; k_ < (kOpInH * kOpTX + 255) / 256; ++k_) {
      const int i = threadIdx.x + 256 * k_;
      if (i >= kOpInH * kOpTX) break;
      const int ry = i / kOpTX, ox = i - ry * kOpTX;
      const int x = x0 + ox;
      float v = 0.0f;
      if (x < w) {
        const float* row = in_t + ry * kOpInW + ox;
        float sum = 0.0f;
        for (int k = 0; k < ntap; ++k) sum += row[k] * s.taps[k];
        v = sum * sx[x];
      }
      h_t[c][i] = v;
    }
    __syncthreads();
  }
  const float* sy = scales + static_cast<size_t>(kSigOpsin * 2 + 1) * stride;
  #pragma unroll
  for (int k_ = 0; k_ < (kOpTY * kOpTX + 255) / 256; ++k_) {
    const int i = threadIdx.x + 256 * k_;
    if (i >= kOpTY * kOpTX) break;
    const int oy = i / kOpTX, ox = i - oy * kOpTX;
    const int x = x0 + ox, y = y0 + oy;
    if (x >= w || y >= h) continue;
    const size_t p = static_cast<size_t>(y) * w + x;
    float blurred[3], l[3], out[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* col = h_t[c] + oy * kOpTX + ox;
      float sum = 0.0f;
      for (int k = 0; k < ntap; ++k) sum += col[k * kOpTX] * s.taps[k];
      blurred[c] = sum * sy[y];
      l[c] = lin[c * n + p];
    }
    opsin_pixel(blurred, l, out);
    xyb[p] = out[0];
    xyb[n + p] = out[1];
    xyb[2 * n + p] = out[2];
  }
}

// The candidate's OpsinDynamicsImageOpt fused with MaskHighIntensityChangeOpt
// (:729-781; c0 = reference XYB from HBM, c1 = the candidate XYB computed here): the
// opsin values of the tile + 1-pixel halo (the Y neighbours MHIC reads) stay
// in LDS and only m0 / m1 reach HBM (xyb_out, if set, gets the tile's XYB
// for the stage tests).  Blur and opsin arithmetic as in k_opsin2d.
constexpr int kOmTX = 64, kOmTY = 16;
constexpr int kOmXW = kOmTX + 2, kOmXH = kOmTY + 2;  // XYB tile + halo, origin (x0-1, y0-1)
constexpr int kOmInW = kOmXW + 2 * kOpR, kOmInH = kOmXH + 2 * kOpR;

// The same fused opsin + MHIC pass as register streaming (no LDS, no
// barriers): a wave owns 64 adjacent columns (lane l = column x0 - 3 + l)
// and walks down the rows of its segment.  Per input row: the three linear
// values (zero outside the image), their sigma-1.1 horizontal sums from DPP
// lane shifts (radius 2), and a 5-row queue of horizontally blurred rows for
// the vertical sums; the opsin transform of row y - 2 from its blurred and
// linear values; MHIC of row y - 3 from a 3-row queue of candidate XYB and
// the reference rows (left / right neighbours by DPP).  Lanes 3 .. 60 store
// (kOsCols columns per strip).  Every value is formed by the operations of
// OpsinDynamicsImageOpt / MaskHighIntensityChangeOpt (:729-912) in the same
// order, bit for bit.
constexpr int kOsCols = 58;
constexpr int kDmMaxWords = 64;  // k_diffmap's maxima words (see k_diffmap)
#ifndef GZ_OS_PF
#define GZ_OS_PF 2
#endif
constexpr int kOsPf = GZ_OS_PF;  // rows loaded ahead
// rows per wave: enough waves to cover latency (the image's strip count
// times segments), few enough that the 2-row opsin halo stays small
// (round 5, with the rows loaded two ahead: 12 at 1080p -- 8 / 10 / 14 / 16
// measured 7-18 % slower there; 16 at 4K, 12 / 20 / 24 no faster:
// profiles/round5_stream_rows_ab.txt)
inline int OpsinStreamRows(int w, int h) {
  const long waves16 = static_cast<long>((w + kOsCols - 1) / kOsCols) * ((h + 15) / 16);
  return waves16 >= 8192 ? 16 : 12;
}

#ifndef GZ_OS_WAVES
#define GZ_OS_WAVES 1
#endif
__global__ __launch_bounds__(256, GZ_OS_WAVES) void k_opsin_mhic_stream(const uint32_t* __restrict__ px8,
                                                           const float* __restrict__ ref_xyb, int w,
                                                           int h, int strips, int segs, int rows,
                                                           float* __restrict__ m0,
                                                           float* __restrict__ m1,
                                                           float* __restrict__ xyb_out,
                                                           const float* __restrict__ scales,
                                                           int stride, uint32_t* __restrict__ dmax_zero) {
  __shared__ float s_srgb[256];  // the sRGB LUT: the candidate's linear values from its bytes
  s_srgb[threadIdx.x] = c_tab.srgb[threadIdx.x];
  // (this pass's k_diffmap maxima start from +0; the previous pass's coder,
  // earlier in the stream, has read them)
  if (blockIdx.x == 0 && threadIdx.x < kDmMaxWords) dmax_zero[threadIdx.x] = 0u;
  __syncthreads();
  const int item = blockIdx.x * 4 + wave_id();
  if (item >= strips * segs) return;
  const int lane = threadIdx.x & 63;
  const int x0 = (item % strips) * kOsCols, ys = (item / strips) * rows;
  const int ye = min(ys + rows, h);
  const int x = x0 - 3 + lane;
  const bool xin = x >= 0 && x < w;
  const int xc = x < 0 ? 0 : (x < w ? x : w - 1);
  const bool emit = lane >= 3 && lane < 3 + kOsCols && x < w;
  const bool xl = x > 0, xr = x + 1 < w;
  const size_t n = static_cast<size_t>(w) * h;
  const BlurSpec& s = c_tab.blur[kSigOpsin];
  const float sxv = scales[static_cast<size_t>(kSigOpsin * 2) * stride + xc];
  const float* sy = scales + static_cast<size_t>(kSigOpsin * 2 + 1) * stride;
  const float* ryp = ref_xyb + n;
  float hq[3][5], lq[3][3], xq[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int t = 0; t < 5; ++t) hq[c][t] = 0.0f;
#pragma unroll
    for (int t = 0; t < 3; ++t) lq[c][t] = xq[c][t] = 0.0f;
  }
  // reference Y of rows yo - 1, yo (rotated in before any MHIC row is formed)
  float rY_up = 0.0f, rY = 0.0f;
  // Loads kOsPf rows ahead (clamped rows, used only where the row is valid):
  // the candidate's pixels of row y, the reference Y of row y - 2 and its X /
  // B of row y - 3, instead of each iteration waiting for its own loads
  // (4K: -6 % for this kernel at 2 rows ahead; 4 rows cost occupancy, and
  // 1080p's 4.5 waves per SIMD see no change: profiles/round5_opsin_prefetch_ab.txt).
  auto ldr = [&](const float* p, int yy) {
    return row_ptr(p, yy < 0 ? 0 : (yy < h ? yy : h - 1), w)[static_cast<unsigned>(xc)];
  };
  auto ldp = [&](int yy) {
    return row_ptr(px8, yy < 0 ? 0 : (yy < h ? yy : h - 1), w)[static_cast<unsigned>(xc)];
  };
  // The segment reads the pixels of rows ys - 3 .. ye + 2 (the opsin blur
  // of rows ys - 1 .. ye), the reference Y of rows ys - 1 .. ye (MHIC's
  // neighbours) and its X / B of rows ys .. ye - 1; a queue slot of any
  // other row is never used.  Its load takes the nearest row read anyway (an
  // L2 hit, no HBM read) -- round 5 loaded 24 rows of each plane per 16-row
  // segment at 4K; skipping the loads instead broke their pipelining.
  auto load_row = [&](int yy, uint32_t& p, float& ry, float& rx, float& rb) {
    p = ldp(min(yy, ye + 2));
    ry = ldr(ryp, min(max(yy - 2, ys - 1), ye));
    rx = ldr(ref_xyb, min(max(yy - 3, ys), ye - 1));
    rb = ldr(ref_xyb + 2 * n, min(max(yy - 3, ys), ye - 1));
  };
  uint32_t fp[kOsPf];
  float fy[kOsPf], fx[kOsPf], fb[kOsPf];
#pragma unroll
  for (int k = 0; k < kOsPf; ++k) load_row(ys - 3 + k, fp[k], fy[k], fx[k], fb[k]);
  for (int y = ys - 3; y <= ye + 2; ++y) {
    const bool yin = y >= 0 && y < h;
    const uint32_t v = fp[0];
    const float ry_y2 = fy[0], rx_y3 = fx[0], rb_y3 = fb[0];
#pragma unroll
    for (int k = 0; k + 1 < kOsPf; ++k) {
      fp[k] = fp[k + 1];
      fy[k] = fy[k + 1];
      fx[k] = fx[k + 1];
      fb[k] = fb[k + 1];
    }
    load_row(y + kOsPf, fp[kOsPf - 1], fy[kOsPf - 1], fx[kOsPf - 1], fb[kOsPf - 1]);
    float l[3];
    {
#pragma unroll
      for (int c = 0; c < 3; ++c) l[c] = masked(s_srgb[(v >> (8 * c)) & 255], xin && yin);
    }
    // horizontal sigma-1.1 sums (taps at x-2 .. x+2, ascending)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float p1 = wave_prev(l[c]), p2 = wave_prev(p1);
      const float n1 = wave_next(l[c]), n2 = wave_next(n1);
      float sum = 0.0f;
      sum += p2 * s.taps[0];
      sum += p1 * s.taps[1];
      sum += l[c] * s.taps[2];
      sum += n1 * s.taps[3];
      sum += n2 * s.taps[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) hq[c][t] = hq[c][t + 1];
      hq[c][4] = sum * sxv;
#pragma unroll
      for (int t = 0; t < 2; ++t) lq[c][t] = lq[c][t + 1];
      lq[c][2] = l[c];
    }
    // opsin of row yv = y - 2 (its blurred rows yv-2 .. yv+2 are in hq)
    const int yv = y - 2;
    if (yv < ys - 1) continue;
    float xyb[3];
    {
      float blurred[3], lv[3];
      const float syv = sy[yv < 0 ? 0 : (yv < h ? yv : h - 1)];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float sum = 0.0f;
#pragma unroll
        for (int t = 0; t < 5; ++t) sum += hq[c][t] * s.taps[t];
        blurred[c] = sum * syv;
        lv[c] = lq[c][0];
      }
      opsin_pixel(blurred, lv, xyb);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      xq[c][0] = xq[c][1];
      xq[c][1] = xq[c][2];
      xq[c][2] = xyb[c];
    }
    if (xyb_out && emit && yv >= ys && yv < ye) {
#pragma unroll
      for (int c = 0; c < 3; ++c) row_ptr(xyb_out + c * n, yv, w)[static_cast<unsigned>(x)] = xyb[c];
    }
    // MHIC of row yo = yv - 1 (neighbour order left, right, up, down, :746-760)
    const int yo = yv - 1;
    const float rY_dn = ry_y2;  // reference Y of row yo + 1 (clamped)
    if (yo >= ys && yo < ye) {
      float ra[3], b[3], ave[3];
      ra[0] = rx_y3;
      ra[1] = rY;
      ra[2] = rb_y3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        b[c] = xq[c][1];
        ave[c] = mhic_ave(ra[c], b[c]);
      }
      const float rl = wave_prev(rY), rr = wave_next(rY);
      const float cl = wave_prev(xq[1][1]), cr = wave_next(xq[1][1]);
      float sq = -1.0f;
      {
        const float d = mhic_sqdiff(rl, cl, ave[1]);
        sq = (xl && sq < d) ? d : sq;
      }
      {
        const float d = mhic_sqdiff(rr, cr, ave[1]);
        sq = (xr && sq < d) ? d : sq;
      }
      {
        const float d = mhic_sqdiff(rY_up, xq[1][0], ave[1]);
        sq = (yo > 0 && sq < d) ? d : sq;
      }
      {
        const float d = mhic_sqdiff(rY_dn, xq[1][2], ave[1]);
        sq = (yo + 1 < h && sq < d) ? d : sq;
      }
      float o0[3], o1[3];
      mhic_mix(ra, b, ave, sq, o0, o1);
      if (emit) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          row_ptr(m0 + c * n, yo, w)[static_cast<unsigned>(x)] = o0[c];
          row_ptr(m1 + c * n, yo, w)[static_cast<unsigned>(x)] = o1[c];
        }
      }
    }
    rY_up = rY;
    rY = rY_dn;
  }
}

// k_opsin_mhic_stream with two rows per step (round 6): the rows y, y + 1 of
// an iteration travel as the two halves of f32x2 values, so every
// per-pixel float operation is one packed instruction for two pixels
// (opsin_pixel2 / mhic_mix2 / the blur sums; each half's operations are
// those of the one-row kernel, in the same order).  The row queues hold row
// pairs: horizontal sums H0..H2 = rows (y-4, y-3), (y-2, y-1), (y, y+1); the
// vertical sums of rows (y-2, y-1) read them and the straddling pairs
// (y-3, y-2), (y-1, y); the XYB pair of rows (y-2, y-1) and the previous one
// give MHIC rows (y-3, y-2) with their up / down neighbours; the reference
// Y pairs R = rows (y-2, y-1) likewise.  Loads run one pair (two rows) ahead,
// as the one-row kernel's.
#ifndef GZ_OS_PAIR
#define GZ_OS_PAIR 1
#endif
__global__ __launch_bounds__(256) void k_opsin_mhic_stream2(const uint32_t* __restrict__ px8,
                                                            const float* __restrict__ ref_xyb, int w, int h,
                                                            int strips, int segs, int rows,
                                                            float* __restrict__ m0, float* __restrict__ m1,
                                                            float* __restrict__ xyb_out,
                                                            const float* __restrict__ scales, int stride,
                                                            uint32_t* __restrict__ dmax_zero) {
  __shared__ float s_srgb[256];
  s_srgb[threadIdx.x] = c_tab.srgb[threadIdx.x];
  if (blockIdx.x == 0 && threadIdx.x < kDmMaxWords) dmax_zero[threadIdx.x] = 0u;
  __syncthreads();
  const int item = blockIdx.x * 4 + wave_id();
  if (item >= strips * segs) return;
  const int lane = threadIdx.x & 63;
  const int x0 = (item % strips) * kOsCols, ys = (item / strips) * rows;
  const int ye = min(ys + rows, h);
  const int x = x0 - 3 + lane;
  const bool xin = x >= 0 && x < w;
  const int xc = x < 0 ? 0 : (x < w ? x : w - 1);
  const bool emit = lane >= 3 && lane < 3 + kOsCols && x < w;
  const bool xl = x > 0, xr = x + 1 < w;
  const size_t n = static_cast<size_t>(w) * h;
  const BlurSpec& s = c_tab.blur[kSigOpsin];
  const float sxv = scales[static_cast<size_t>(kSigOpsin * 2) * stride + xc];
  const float* sy = scales + static_cast<size_t>(kSigOpsin * 2 + 1) * stride;
  const float* ryp = ref_xyb + n;
  auto ldr = [&](const float* p, int yy) {
    return row_ptr(p, yy < 0 ? 0 : (yy < h ? yy : h - 1), w)[static_cast<unsigned>(xc)];
  };
  auto ldp = [&](int yy) {
    return row_ptr(px8, yy < 0 ? 0 : (yy < h ? yy : h - 1), w)[static_cast<unsigned>(xc)];
  };
  // the loads of input rows yy, yy + 1 (the one-row kernel's load_row of each)
  struct Pair {
    uint32_t pa, pb;
    float ry0, ry1, rx0, rx1, rb0, rb1;
  };
  auto load_pair = [&](int yy, Pair& q) {
    q.pa = ldp(min(yy, ye + 2));
    q.pb = ldp(min(yy + 1, ye + 2));
    q.ry0 = ldr(ryp, min(max(yy - 2, ys - 1), ye));
    q.ry1 = ldr(ryp, min(max(yy - 1, ys - 1), ye));
    q.rx0 = ldr(ref_xyb, min(max(yy - 3, ys), ye - 1));
    q.rx1 = ldr(ref_xyb, min(max(yy - 2, ys), ye - 1));
    q.rb0 = ldr(ref_xyb + 2 * n, min(max(yy - 3, ys), ye - 1));
    q.rb1 = ldr(ref_xyb + 2 * n, min(max(yy - 2, ys), ye - 1));
  };
  f32x2 H[3][3], Lp[3], Xp[3], Rp = {0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    H[c][0] = H[c][1] = H[c][2] = f32x2{0.0f, 0.0f};
    Lp[c] = Xp[c] = f32x2{0.0f, 0.0f};
  }
  Pair nx;
  load_pair(ys - 3, nx);
  for (int y = ys - 3; y <= ye + 2; y += 2) {
    const Pair cu = nx;
    load_pair(y + 2, nx);
    const bool ya = y >= 0 && y < h, yb = y + 1 >= 0 && y + 1 < h;
    f32x2 l[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      l[c] = f32x2{masked(s_srgb[(cu.pa >> (8 * c)) & 255], xin && ya),
                   masked(s_srgb[(cu.pb >> (8 * c)) & 255], xin && yb)};
    // horizontal sigma-1.1 sums of both rows (taps at x-2 .. x+2, ascending)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x2 p1 = {wave_prev(l[c].x), wave_prev(l[c].y)};
      const f32x2 p2 = {wave_prev(p1.x), wave_prev(p1.y)};
      const f32x2 n1 = {wave_next(l[c].x), wave_next(l[c].y)};
      const f32x2 n2 = {wave_next(n1.x), wave_next(n1.y)};
      f32x2 sum = {0.0f, 0.0f};
      sum += p2 * splat2(s.taps[0]);
      sum += p1 * splat2(s.taps[1]);
      sum += l[c] * splat2(s.taps[2]);
      sum += n1 * splat2(s.taps[3]);
      sum += n2 * splat2(s.taps[4]);
      H[c][0] = H[c][1];
      H[c][1] = H[c][2];
      H[c][2] = sum * splat2(sxv);
    }
    // the linear values of rows y - 2, y - 1 (the previous pair's)
    f32x2 lv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lv[c] = Lp[c];
      Lp[c] = l[c];
    }
    const f32x2 R = {cu.ry0, cu.ry1};  // reference Y of rows y - 2, y - 1 (clamped)
    // opsin of rows yv = y - 2, y - 1 (the one-row kernel's first is ys - 1)
    if (y + 1 < ys + 2) {
      Rp = R;
      continue;
    }
    const int yv = y - 2;
    f32x2 xyb[3];
    {
      f32x2 blurred[3];
      const f32x2 syv = {sy[yv < 0 ? 0 : (yv < h ? yv : h - 1)], sy[yv + 1 < 0 ? 0 : (yv + 1 < h ? yv + 1 : h - 1)]};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        // rows yv - 2 + t of the horizontal sums, t = 0..4, for both rows
        const f32x2 q0 = {H[c][0].y, H[c][1].x}, q1 = {H[c][1].y, H[c][2].x};
        f32x2 sum = {0.0f, 0.0f};
        sum += H[c][0] * splat2(s.taps[0]);
        sum += q0 * splat2(s.taps[1]);
        sum += H[c][1] * splat2(s.taps[2]);
        sum += q1 * splat2(s.taps[3]);
        sum += H[c][2] * splat2(s.taps[4]);
        blurred[c] = sum * syv;
      }
      opsin_pixel2(blurred, lv, xyb);
    }
    if (xyb_out && emit) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (yv >= ys && yv < ye) row_ptr(xyb_out + c * n, yv, w)[static_cast<unsigned>(x)] = xyb[c].x;
        if (yv + 1 >= ys && yv + 1 < ye) row_ptr(xyb_out + c * n, yv + 1, w)[static_cast<unsigned>(x)] = xyb[c].y;
      }
    }
    // MHIC of rows yo = yv - 1, yv (neighbour order left, right, up, down)
    const int yo = yv - 1;
    const bool oa = yo >= ys && yo < ye, ob = yo + 1 >= ys && yo + 1 < ye;
    if (oa || ob) {
      const f32x2 rY = {Rp.y, R.x};  // reference Y of rows yo, yo + 1
      f32x2 ra[3], b[3], ave[3];
      ra[0] = f32x2{cu.rx0, cu.rx1};
      ra[1] = rY;
      ra[2] = f32x2{cu.rb0, cu.rb1};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        b[c] = f32x2{Xp[c].y, xyb[c].x};
        ave[c] = mhic_ave2(ra[c], b[c]);
      }
      const f32x2 rl = {wave_prev(rY.x), wave_prev(rY.y)}, rr = {wave_next(rY.x), wave_next(rY.y)};
      const f32x2 cl = {wave_prev(b[1].x), wave_prev(b[1].y)}, cr = {wave_next(b[1].x), wave_next(b[1].y)};
      f32x2 sq = {-1.0f, -1.0f};
      {
        const f32x2 d = mhic_sqdiff2(rl, cl, ave[1]);
        sq = sel2(xl && sq.x < d.x, xl && sq.y < d.y, d, sq);
      }
      {
        const f32x2 d = mhic_sqdiff2(rr, cr, ave[1]);
        sq = sel2(xr && sq.x < d.x, xr && sq.y < d.y, d, sq);
      }
      {
        const f32x2 d = mhic_sqdiff2(Rp, Xp[1], ave[1]);  // rows yo - 1, yo
        sq = sel2(yo > 0 && sq.x < d.x, yo + 1 > 0 && sq.y < d.y, d, sq);
      }
      {
        const f32x2 d = mhic_sqdiff2(R, xyb[1], ave[1]);  // rows yo + 1, yo + 2
        sq = sel2(yo + 1 < h && sq.x < d.x, yo + 2 < h && sq.y < d.y, d, sq);
      }
      f32x2 o0[3], o1[3];
      mhic_mix2(ra, b, ave, sq, o0, o1);
      if (emit) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (oa) {
            row_ptr(m0 + c * n, yo, w)[static_cast<unsigned>(x)] = o0[c].x;
            row_ptr(m1 + c * n, yo, w)[static_cast<unsigned>(x)] = o1[c].x;
          }
          if (ob) {
            row_ptr(m0 + c * n, yo + 1, w)[static_cast<unsigned>(x)] = o0[c].y;
            row_ptr(m1 + c * n, yo + 1, w)[static_cast<unsigned>(x)] = o1[c].y;
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) Xp[c] = xyb[c];
    Rp = R;
  }
}

// ---------------------------------------------------------------------------
// EdgeDetectorMapOpt (:1456-1485) + Butteraugli8x8CornerEdgeDetectorDiffOpt
// (:638-687).  b0/b1: blurred m0/m1 (full resolution planes).
// ---------------------------------------------------------------------------

// The corner edge term of res point (i, j) (needs ry + 5 < h, rx + 5 < w):
// per corner k of the 8x8 window, the horizontal pair (x - 3, x + 3) then
// the vertical pair (y - 3, y + 3), each where it lies inside the image,
// folded into local[] in that order.  The loads of two corners' pairs are
// issued together from clamped positions (48 loads in flight) and masked
// afterwards: the pairs' conditional blocks otherwise waited out their
// loads one block at a time.
__device__ __forceinline__ void edge_point(const float* __restrict__ b0, const float* __restrict__ b1,
                                           int w, int h, int rw, int i, int j, const float* lf_dy,
                                           float* __restrict__ edge) {
  const int rx = 3 * i, ry = 3 * j;
  const size_t n = static_cast<size_t>(w) * h;
  const int px = rx < w - 8 ? rx : w - 8;
  const int py = ry < h - 8 ? ry : h - 8;
  int count = 0;
  float local[3] = {0.0f, 0.0f, 0.0f};
  const float wgt = 0.711100840192f;
  const int offx[4] = {0, 0, 7, 7}, offy[4] = {0, 7, 0, 7};
#pragma unroll
  for (int k0 = 0; k0 < 4; k0 += 2) {
    // pair q = 2 (k - k0) + dir: dir 0 horizontal, 1 vertical
    float va[4][3][2], vb[4][3][2];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + (q >> 1);
      const int x = px + offx[k], y = py + offy[k];
      size_t ix, ix2;
      if ((q & 1) == 0) {
        ok[q] = x >= 3 && x + 3 < w;
        const int xa = ok[q] ? x - 3 : 0;
        ix = static_cast<size_t>(y) * w + xa;
        ix2 = ok[q] ? ix + 6 : ix;
      } else {
        ok[q] = y >= 3 && y + 3 < h;
        const int ya = ok[q] ? y - 3 : 0;
        ix = static_cast<size_t>(ya) * w + x;
        ix2 = ok[q] ? ix + 6 * static_cast<size_t>(w) : ix;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        va[q][c][0] = b0[c * n + ix];
        va[q][c][1] = b0[c * n + ix2];
        vb[q][c][0] = b1[c * n + ix];
        vb[q][c][1] = b1[c * n + ix2];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!ok[q]) continue;
      float a[3], bb[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        a[c] = wgt * (va[q][c][0] - va[q][c][1]);
        bb[c] = wgt * (vb[q][c][0] - vb[q][c][1]);
      }
      lowfreq_sq_f(a, bb, 1.0f, local, lf_dy);
      ++count;
    }
  }
  const float mul = static_cast<float>(static_cast<double>(0.01617112696f) * 8.0 / count);
  const size_t r = static_cast<size_t>(j) * rw + i;
#pragma unroll
  for (int c = 0; c < 3; ++c) edge[3 * r + c] = 0.0f + mul * local[c];
}

// edge_point with one corner's pairs in flight at a time and 32-bit byte
// offsets from the planes' bases (k_block_diff2's 64-VGPR budget; the same
// operations in the same order).
template <class Tab>
__device__ __forceinline__ void edge_point_lean(const float* __restrict__ b0, const float* __restrict__ b1,
                                                int w, int h, int rw, int i, int j, const Tab* lf_dy,
                                                float* __restrict__ edge) {
  const int rx = 3 * i, ry = 3 * j;
  const unsigned nb = 4u * static_cast<unsigned>(w * h);  // a plane's bytes
  const int px = rx < w - 8 ? rx : w - 8;
  const int py = ry < h - 8 ? ry : h - 8;
  int count = 0;
  float local[3] = {0.0f, 0.0f, 0.0f};
  const float wgt = 0.711100840192f;
  const int offx[4] = {0, 0, 7, 7}, offy[4] = {0, 7, 0, 7};
  const char* c0 = reinterpret_cast<const char*>(b0);
  const char* c1 = reinterpret_cast<const char*>(b1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // pair dir 0 horizontal, 1 vertical
    float va[2][3][2], vb[2][3][2];
    bool ok[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int x = px + offx[k], y = py + offy[k];
      unsigned ix, ix2;
      if (d == 0) {
        ok[d] = x >= 3 && x + 3 < w;
        const int xa = ok[d] ? x - 3 : 0;
        ix = 4u * static_cast<unsigned>(y * w + xa);
        ix2 = ok[d] ? ix + 24u : ix;
      } else {
        ok[d] = y >= 3 && y + 3 < h;
        const int ya = ok[d] ? y - 3 : 0;
        ix = 4u * static_cast<unsigned>(ya * w + x);
        ix2 = ok[d] ? ix + 24u * static_cast<unsigned>(w) : ix;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        va[d][c][0] = *reinterpret_cast<const float*>(c0 + c * nb + ix);
        va[d][c][1] = *reinterpret_cast<const float*>(c0 + c * nb + ix2);
        vb[d][c][0] = *reinterpret_cast<const float*>(c1 + c * nb + ix);
        vb[d][c][1] = *reinterpret_cast<const float*>(c1 + c * nb + ix2);
      }
    }
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      if (!ok[d]) continue;
      float a[3], bb[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        a[c] = wgt * (va[d][c][0] - va[d][c][1]);
        bb[c] = wgt * (vb[d][c][0] - vb[d][c][1]);
      }
      lowfreq_sq_f(a, bb, 1.0f, local, lf_dy);
      ++count;
    }
  }
  const float mul = static_cast<float>(static_cast<double>(0.01617112696f) * 8.0 / count);
  const size_t r = static_cast<size_t>(j) * rw + i;
#pragma unroll
  for (int c = 0; c < 3; ++c) edge[3 * r + c] = 0.0f + mul * local[c];
}

__global__ __launch_bounds__(256) void k_edge_map(const float* __restrict__ b0,
                                                  const float* __restrict__ b1, int w, int h,
                                                  int rw, int rh, float* __restrict__ edge) {
  // the interpolation table in LDS (per-lane indices: a vector-cache gather
  // per read from c_tab)
  __shared__ float s_lf[21];
  if (threadIdx.x < 21) s_lf[threadIdx.x] = c_tab.lf_dy[threadIdx.x];
  __syncthreads();
  const BlockId B = xcd_block_id();
  const int i = B.x * 256 + threadIdx.x;
  const int j = B.y;
  if (i >= rw) return;
  if (!(3 * j + 5 < h && 3 * i + 5 < w)) return;
  edge_point(b0, b1, w, h, rw, i, j, s_lf, edge);
}

// ---------------------------------------------------------------------------
// BlockDiffMapOpt (:1419-1454) + ButteraugliBlockDiffOpt (:551-633), tiled.
// A 256-lane workgroup owns 16x16 res points (stride 3, one 8x8 window
// each).  Per FFT operand the tile's pixel window (<= 53x53) is staged in LDS
// once, the 8-point row FFTs are computed once per (pixel row, res column) --
// vertically adjacent windows share 5 of their 8 rows -- and each lane then
// runs the column FFTs of its own window and the order-sensitive sums in the
// reference's order.  Every value is produced by the same operations on the
// same operands as the per-window computation.
// ---------------------------------------------------------------------------

#ifndef GZ_BD_T
#define GZ_BD_T 16
#endif
constexpr int kBdT = GZ_BD_T;              // res points per tile side
constexpr int kBdThreads = kBdT * kBdT;    // res points per workgroup
constexpr int kBdP = 3 * (kBdT - 1) + 8;   // pixels per tile side (53)

// Column FFTs of a lane's window (transposed layout of :527-545: spectrum
// row r of the window = bin r of its 8 row FFTs), |F|^2 * global_mul at
// k = 4..36 in increasing k: kOp 1 / 3 the X / B sums, 2 keeps sqrt(|F|^2)
// of the Y difference, 0 combines the Y average with it (:612-632).
//
// Two lanes per res point (512-lane workgroups; round 6: one lane per res
// point took 57.6 us per 1080p launch, this 56.2 -- the kernel is VALU-issue
// bound, so halving each lane's chain gains little).  Lane half A (waves
// 0-3) takes column bins r = 0..2 of each operand (k = 4..23) and the DC
// means, half B (waves 4-7) bins r = 3, 4 (k = 24..36) and the corner edge
// term.  The in-order sums stay in order: A sums k = 4..23 from zero, B
// forms its 13 terms, then continues A's sum (handed over through LDS at the
// next barrier) with them in k order -- the same float additions.  The Y
// difference's per-k values stay with the half that owns k.  Fills and row
// FFTs are shared by all 512 lanes.
// The power-of-two factors moved out of the sums -- the row
// FFTs on the unhalved tile (the FFT's adds and its sqrt(1/2) products scale
// exactly by 2, and |F|^2 by 4: the 0.000064 factor takes its exact quarter)
// and the DC mean as the sequential sum of the tile times 2^-6 (each partial
// sum is the reference's times 64, exactly: the tile values are differences
// of the MHIC planes, nonzero ones far above 2^-100, so no partial sum or
// term comes near the subnormal range where power-of-two scaling and
// rounding would not commute) -- the same floats, fewer multiplies
using BdHfT = float2;  // (a[i], a[i + 1] - a[i]) of hf_dy / lf_dy (interp_pair_f)
// The Y operands' square roots: sqrt_cr_big on the input scaled by 2^32
// (exact; the inputs are far below 2^96), so the correction runs on what the
// generic sequence runs on for inputs below 2^-96 and on exactly scaled
// normal numbers otherwise -- correctly rounded for every x in [0, 2^96)
// without the generic form's input test and class test
// (tests/native/sqrt_check.hip checks every such float).  The scalings are
// folded into the constants around it: the 2^32 into the |F|^2 factor, the
// result's 2^-16 into remove_range's range and the interpolation's argument
// factor (all exact powers of two; the remove_range decisions and results
// scale with its operands).
constexpr float kBdVScale = 0.000064f * 0.25f;  // (the unhalved tile: the exact quarter)
constexpr float kBdVScaleY = kBdVScale * 0x1p32f;
constexpr float kBdRangeY = 0.04f * 0x1p16f;
constexpr float kBdArgY = 1.51983458269f * 0x1p-16f;
template <int kOp, int R0, int R1>
__device__ __forceinline__ void bd_columns_part(const float (*spec)[kBdP][kBdT], int oy, int li, float* yh,
                                                float& acc, float* terms, const BdHfT* hf_dy) {
  const float kSqrtHalf = 0.70710678118654752440084436210484903f;
  constexpr int kLo = R0 == 0 ? 4 : 8 * R0;  // first k of the part
#pragma unroll
  for (int r = R0; r < R1; ++r) {
    // (one column FFT's reads in flight at a time: hoisting every r's spectrum
    // reads to the start overran the 64-VGPR budget)
    __builtin_amdgcn_sched_barrier(0);
    float re[8], im[8];
    if (r == 0 || r == 4) {
      float in[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) in[x] = spec[r][oy + x][li];
      real_fft8(in, re, im, kSqrtHalf);
    } else {
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        re[x] = spec[r][oy + x][li];
        im[x] = spec[4 + r][oy + x][li];
      }
      fft8_inplace(re, im, kSqrtHalf);
    }
    // |F|^2 times the reference's 0.000064f -- its exact quarter, as the row
    // FFTs ran on the unhalved tile (re, im exactly twice the reference's) --
    // and for the Y operands times 2^32 besides (the square roots' input scaling)
    float v[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      v[x] = re[x] * re[x] + im[x] * im[x];
      v[x] *= (kOp == 0 || kOp == 2) ? kBdVScaleY : kBdVScale;
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const int k = 8 * r + x;
      if (k >= 4 && k < 37) {
        const int q = k - kLo;
        float term = 0.0f;
        if (kOp == 1) {
          term = c_tab.csf_xb[0][k] * v[x];  // (block_csf[k] * 64.8f) * v
        } else if (kOp == 3) {
          term = c_tab.csf_xb[1][k] * v[x];  // (block_csf[k] * 2.4f) * v
        } else if (kOp == 2) {
          yh[q] = sqrt_cr_big(v[x]);  // the reference's sqrt times 2^16
          continue;
        } else {
          const float ya = sqrt_cr_big(v[x]);  // (times 2^16, as yh)
          const float d = c_tab.block_csf[k];
          float y0 = ya - yh[q], y1 = ya + yh[q];
          y0 = remove_range(y0, kBdRangeY);
          y1 = remove_range(y1, kBdRangeY);
          // (no branch on y0 != y1: equal arguments give v0 - v1 = +0 and a
          // term of +0, the value the reference's skipped branch leaves)
          const float v0 = interp_pair_f(hf_dy, 21, y0 * kBdArgY);
          const float v1 = interp_pair_f(hf_dy, 21, y1 * kBdArgY);
          const float vy = 1.753123908348329f * (v0 - v1);
          term = d * vy * vy;
        }
        if (R0 == 0) acc += term;  // half A: the sum from k = 4
        else terms[q] = term;      // half B: added after A's sum
      }
    }
  }
}

constexpr int kBd2Threads = 2 * kBdThreads;
#ifndef GZ_BD_EDGE_HALF
#define GZ_BD_EDGE_HALF 0
#endif
constexpr int kBdEdgeHalf = GZ_BD_EDGE_HALF;
#ifndef GZ_BD_ROWMAP
#define GZ_BD_ROWMAP 1  // (0: rows r, r + 1 per half-wave; profiles/round6_block_diff_rowmap_ab.txt)
#endif  // the half that forms the corner edge term
constexpr int kBdA = 20, kBdB = 13;  // k values per half (4..23, 24..36)
struct Bd2Lds {
  float tile[kBdP][kBdP];
  float spec[8][kBdP][kBdT];
  float acc[kBdThreads];  // half A's sums, handed to half B
  BdHfT hf[21];
  BdHfT lf[21];
};

// One half's whole program (kB: half B).  The halves run as separate code
// paths with the same barriers in the same order, so each keeps its own
// registers (one kernel body branching per phase merged the halves' per-k
// values and spilled them).
template <bool kB>
__device__ __forceinline__ void bd2_half(Bd2Lds& L, const float* __restrict__ m0, const float* __restrict__ m1,
                                         int w, int h, int rw, int rh, int i0, int j0, float* __restrict__ dc_out,
                                         float* __restrict__ ac_out, const float* __restrict__ eb0,
                                         const float* __restrict__ eb1, float* __restrict__ edge_out) {
  const float kSqrtHalf = 0.70710678118654752440084436210484903f;
  const int x0 = min(3 * i0, w - 8), y0 = min(3 * j0, h - 8);
  const int tw = min(3 * (i0 + kBdT - 1), w - 8) + 8 - x0;
  const int th = min(3 * (j0 + kBdT - 1), h - 8) + 8 - y0;
  const size_t n = static_cast<size_t>(w) * h;
  // (the thread index re-read per phase, as an opaque value: per-lane
  // addresses are formed where they are used instead of being held in
  // registers across the whole kernel)
  auto fresh_t = [&]() {
    int v = threadIdx.x;
    asm volatile("" : "+v"(v));
    return v;
  };
  auto point = [&](int& li, int& lj) {
    const int pt = fresh_t() & (kBdThreads - 1);
    li = pt % kBdT;
    lj = pt / kBdT;
  };
  auto is_valid = [&]() {
    int li, lj;
    point(li, lj);
    const int i = i0 + li, j = j0 + lj;
    return i < rw && j < rh && 3 * j + 4 < h && 3 * i + 4 < w;
  };
  auto fill = [&](int c, bool sum) {
    __builtin_amdgcn_sched_barrier(0);
    const float* a = m0 + c * n;
    const float* b = m1 + c * n;
    const int t = fresh_t();
    constexpr int IT = (kBdP * kBdP + kBd2Threads - 1) / kBd2Threads;
    float va[IT], vb[IT];
    // element e = t + 512 k of the tile: (yy, xx) stepped from t's (one
    // division per fill instead of one per element), loads from clamped
    // positions (no branch per element), stores where the element is inside
    // the tile (flat index e of L.tile)
    int yy = t / kBdP, xx = t - yy * kBdP;
    unsigned inside = 0u;
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      inside |= (yy < th && xx < tw) ? 1u << k : 0u;
      const int yc = min(yy, th - 1), xc = min(xx, tw - 1);
      // (a 32-bit byte offset from the plane's uniform base)
      const unsigned g = 4u * static_cast<unsigned>((y0 + yc) * w + x0 + xc);
      va[k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(a) + g);
      vb[k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(b) + g);
      xx += kBd2Threads % kBdP;
      yy += kBd2Threads / kBdP;
      if (xx >= kBdP) {
        xx -= kBdP;
        ++yy;
      }
    }
    float* flat = &L.tile[0][0];
#pragma unroll
    for (int k = 0; k < IT; ++k)
      if (inside & (1u << k)) flat[t + kBd2Threads * k] = sum ? va[k] + vb[k] : va[k] - vb[k];
  };
  // DC: sequential mean of the difference (:561-581)
  auto dc_mean = [&]() {
    float acc = 0.0f;
    int li, lj;
    point(li, lj);
    const int ox = min(3 * (i0 + li), w - 8) - x0, oy = min(3 * (j0 + lj), h - 8) - y0;
    if (is_valid()) {
      for (int y = 0; y < 8; ++y) {
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += L.tile[oy + y][ox + x];
      }
    }
    return acc * (1.0f / 64.0f);
  };
  auto rows = [&]() {
#if GZ_BD_ROWMAP
    // (each 32-lane half of a wave takes rows r and r + 16 of the tile: their
    // reads, 53 x 16 words apart, fall on disjoint LDS banks -- rows r and r
    // + 1 shared 9 of every 16)
#pragma unroll 1
    for (int job = fresh_t(); job < 64 * kBdT; job += kBd2Threads) {
      const int g = job >> 5, ci = job & 15;
      const int yy = (g & 15) + 32 * (g >> 4) + 16 * ((job >> 4) & 1);
      if (yy >= th) continue;
#else
#pragma unroll 1
    for (int job = fresh_t(); job < th * kBdT; job += kBd2Threads) {
      const int yy = job / kBdT, ci = job % kBdT;
#endif
      const int cx = min(3 * (i0 + ci), w - 8) - x0;
      float in[8], re[8], im[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) in[x] = L.tile[yy][cx + x];
      real_fft8(in, re, im, kSqrtHalf);
#pragma unroll
      for (int k = 0; k < 5; ++k) L.spec[k][yy][ci] = re[k];
#pragma unroll
      for (int k = 1; k < 4; ++k) L.spec[4 + k][yy][ci] = im[k];
    }
  };
  float yh[kB ? kBdB : kBdA], tb[kBdB];
  // an operand's column bins of this half; A: the sum from k = 4 handed to
  // B through LDS; B: its terms kept for the sum after the next barrier
  auto cols = [&](auto op, float& acc) {
    constexpr int kOp = decltype(op)::value;
    int li, lj;
    point(li, lj);
    const int oy = min(3 * (j0 + lj), h - 8) - y0;
    if (!is_valid()) return;
    if constexpr (!kB) {
      acc = 0.0f;
      bd_columns_part<kOp, 0, 3>(L.spec, oy, li, yh, acc, tb, L.hf);
      if (kOp != 2) L.acc[fresh_t() & (kBdThreads - 1)] = acc;
    } else {
      bd_columns_part<kOp, 3, 5>(L.spec, oy, li, yh, acc, tb, L.hf);
    }
  };
  auto finish_b = [&]() {
    float acc = L.acc[fresh_t() & (kBdThreads - 1)];
#pragma unroll
    for (int q = 0; q < kBdB; ++q) acc += tb[q];
    return acc;
  };
  using Op0 = std::integral_constant<int, 0>;
  using Op1 = std::integral_constant<int, 1>;
  using Op2 = std::integral_constant<int, 2>;
  using Op3 = std::integral_constant<int, 3>;
  float avg0 = 0.0f, avg1 = 0.0f, avg2 = 0.0f, acc = 0.0f, out_x = 0.0f, out_b = 0.0f;
  // X difference
  fill(0, false);
  __syncthreads();
  if constexpr (!kB) avg0 = dc_mean();
  rows();
  __syncthreads();
  cols(Op1{}, acc);
  // B difference
  fill(2, false);
  __syncthreads();
  if constexpr (kB) out_x = is_valid() ? finish_b() : 0.0f;
  if constexpr (!kB) avg2 = dc_mean();
  rows();
  __syncthreads();
  cols(Op3{}, acc);
  // Y difference (each half keeps its k's values)
  fill(1, false);
  __syncthreads();
  if constexpr (kB) out_b = is_valid() ? finish_b() : 0.0f;
  if constexpr (!kB) avg1 = dc_mean();
  rows();
  __syncthreads();
  cols(Op2{}, acc);
  // Y sum
  fill(1, true);
  __syncthreads();
  rows();
  __syncthreads();
  cols(Op0{}, acc);
  __syncthreads();
  int li, lj;
  point(li, lj);
  const int i = i0 + li, j = j0 + lj;
  const size_t r = static_cast<size_t>(j) * rw + i;
  if constexpr (!kB) {
    if (is_valid()) {
      float dc[3] = {0.0f, 0.0f, 0.0f};
      lowfreq_sq_zero_f(avg0, avg1, avg2, c_tab.block_csf[0], dc);
      dc_out[3 * r] = dc[0];
      dc_out[3 * r + 1] = dc[1];
      dc_out[3 * r + 2] = dc[2];
    }
    // (half A's last work, while B finishes the Y sum: its loads in flight
    // need the registers the per-k values held)
    if (kBdEdgeHalf == 0 && eb0 && i < rw && j < rh && 3 * j + 5 < h && 3 * i + 5 < w)
      edge_point_lean(eb0, eb1, w, h, rw, i, j, L.lf, edge_out);
  } else {
    if (is_valid()) {
      ac_out[3 * r] = out_x;
      ac_out[3 * r + 1] = finish_b();
      ac_out[3 * r + 2] = out_b;
    }
    if (kBdEdgeHalf == 1 && eb0 && i < rw && j < rh && 3 * j + 5 < h && 3 * i + 5 < w)
      edge_point_lean(eb0, eb1, w, h, rw, i, j, L.lf, edge_out);
  }
}

#ifndef GZ_BD2_MINW
#define GZ_BD2_MINW 8
#endif
__global__ __launch_bounds__(kBd2Threads, GZ_BD2_MINW) void k_block_diff2(const float* __restrict__ m0,
                                                                const float* __restrict__ m1, int w, int h,
                                                                int rw, int rh, float* __restrict__ dc_out,
                                                                float* __restrict__ ac_out,
                                                                const float* __restrict__ eb0,
                                                                const float* __restrict__ eb1,
                                                                float* __restrict__ edge_out) {
  __shared__ Bd2Lds L;
  const BlockId B = xcd_block_id();
  const int t = threadIdx.x;
  // (the paired tables, published by the first barrier)
  if (t < 21) L.hf[t] = float2{c_tab.hf_dy[t], t < 20 ? c_tab.hf_dy[t + 1] - c_tab.hf_dy[t] : 0.0f};
  if (t < 21) L.lf[t] = float2{c_tab.lf_dy[t], t < 20 ? c_tab.lf_dy[t + 1] - c_tab.lf_dy[t] : 0.0f};
  if (__builtin_amdgcn_readfirstlane(t >> 8) != 0)
    bd2_half<true>(L, m0, m1, w, h, rw, rh, B.x * kBdT, B.y * kBdT, dc_out, ac_out, eb0, eb1, edge_out);
  else
    bd2_half<false>(L, m0, m1, w, h, rw, rh, B.x * kBdT, B.y * kBdT, dc_out, ac_out, eb0, eb1, edge_out);
}

// ---------------------------------------------------------------------------
// EdgeDetectorLowFreqOpt (:1487-1540).  d0/d1: sigma-14 blurred m0/m1 in
// downsampled form (step 4): value at pixel (y,x) = d[(y/4)*dx + x/4].
// ---------------------------------------------------------------------------

// The term of res point (i, j) (its x = 3i, y = 3j; needs x + 8 < w and
// y + 8 < h): the max over four corner pairs of the squared low-frequency
// differences, per channel.
__device__ __forceinline__ void low_freq_max(const float* __restrict__ d0,
                                             const float* __restrict__ d1, int w, int h, int i,
                                             int j, const float* lf_dy, float mx[3]) {
  const int x = 3 * i, y = 3 * j;
  // (compile-time step: the divisions below become shifts; c_tab's step is
  // checked against kBlurGeomStep when the tables are built)
  constexpr int step = BlurGeom<kSigLowFreq>::STEP;
  const int dx = (w + step - 1) / step, dy = (h + step - 1) / step;
  const size_t dn = static_cast<size_t>(dx) * dy;
  auto at = [&](const float* d, int c, int yy, int xx) {
    return d[c * dn + static_cast<size_t>(yy / step) * dx + xx / step];
  };
  // (every load unconditional -- the x - 6 corner from a clamped column --
  // so that all 30 are in flight at once)
  const int xm = x < 8 ? x : x - 6;
  float v0[5][3], v1[5][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v0[0][c] = at(d0, c, y, x);
    v1[0][c] = at(d1, c, y, x);
    v0[1][c] = at(d0, c, y, x + 8);
    v1[1][c] = at(d1, c, y, x + 8);
    v0[2][c] = at(d0, c, y + 8, x);
    v1[2][c] = at(d1, c, y + 8, x);
    v0[3][c] = at(d0, c, y + 6, x + 6);
    v1[3][c] = at(d1, c, y + 6, x + 6);
    v0[4][c] = at(d0, c, y + 6, xm);
    v1[4][c] = at(d1, c, y + 6, xm);
  }
  float diff[4][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float base = v1[0][c] - v0[0][c];
    diff[0][c] = base + (v0[1][c] - v1[1][c]);
    diff[1][c] = base + (v0[2][c] - v1[2][c]);
    diff[2][c] = base + (v0[3][c] - v1[3][c]);
    diff[3][c] = x < 8 ? 0.0f : base + (v0[4][c] - v1[4][c]);
  }
  mx[0] = mx[1] = mx[2] = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float dd[3] = {0.0f, 0.0f, 0.0f};
    lowfreq_sq_zero_f(diff[k][0], diff[k][1], diff[k][2], 1.0f, dd, lf_dy);
#pragma unroll
    for (int c = 0; c < 3; ++c) mx[c] = mx[c] < dd[c] ? dd[c] : mx[c];
  }
}

__global__ __launch_bounds__(256) void k_low_freq(const float* __restrict__ d0,
                                                  const float* __restrict__ d1, int w, int h,
                                                  int rw, float* __restrict__ ac) {
  __shared__ float s_lf[21];  // (as k_edge_map)
  if (threadIdx.x < 21) s_lf[threadIdx.x] = c_tab.lf_dy[threadIdx.x];
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (!(3 * i + 8 < w && 3 * j + 8 < h)) return;
  float mx[3];
  low_freq_max(d0, d1, w, h, i, j, s_lf, mx);
  const size_t r = static_cast<size_t>(j) * rw + (i + 2);
#pragma unroll
  for (int c = 0; c < 3; ++c) ac[3 * r + c] += 10.0f * mx[c];
}

// ---------------------------------------------------------------------------
// MaskOpt front half (:1156-1233, butteraugli.cc:1379-1438, :1070-1101)
// ---------------------------------------------------------------------------

// DiffPrecompute -> _Average5x5 -> MinSquareValOpt(4, 0), fused and
// register-streamed: a wave owns 64 adjacent columns
// (lane l = column x0 - 1 + l) and walks down the rows of its segment; row
// neighbours come from lane shuffles, column neighbours from a few rows kept
// in registers, so there is no LDS tile and no workgroup barrier.  Lanes
// 1..58 produce outputs (columns x0 .. x0 + 57): the horizontal chain (diff
// -> 3x3 average -> 4-minimum) reaches 1 column left and 5 right.  The 3x3
// average is the gather form of _Average5x5 whose per-output addition order
// is the reference's scatter order (oracle/gz_oracle.c average5x5); the
// minima compare in the reference's order (signed zeros).  Image borders as
// the reference: right / down differences become left / up on the last
// column / row, the average drops missing neighbours, the minima clip.
constexpr int kMsCols = 58, kMsRows = 32;  // rows per wave (VALU-bound: longer strips recompute fewer halo rows)


// |mask_diff_val(c, d)|: the interpolated tables (InterpolateOpt, :195-210)
// are non-negative and odd in their argument, so the magnitude is the table
// at |d| * scale (|d * s| == |d| * s exactly for s > 0).  The table lives in
// LDS as (a[i], a[i+1] - a[i]) pairs, the last entry (a[20], 0): a[base] +
// mix * (a[base+1] - a[base]) with the same float operands as the reference,
// and above the table a[20] + mix * 0 == a[20].
template <int C>
__device__ __forceinline__ float mask_diff_abs(const float2* tab, float d) {
  if constexpr (C == 2) {
    return 1.87816926918f * fabsf(d);
  } else {
    // mix = ix - base == fract(ix) below the table end (exact: base <= ix <
    // base + 1 < 2^23); past it the slope entry is 0 and any finite mix gives a[20]
    const float ix = fabsf(d) * (C == 0 ? 0.758304045695f : 2.28148649801f);
    const int base = min(static_cast<int>(ix), 20);
    const float2 e = tab[base];
    return e.x + __builtin_amdgcn_fractf(ix) * e.y;
  }
}

template <int C>
__device__ __forceinline__ void mask_front_wave(const float* __restrict__ pa, const float* __restrict__ pb,
                                                int w, int h, int x0, int ys, int kRows,
                                                const float2* tab, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int ye = min(ys + kRows, h);
  const int x = x0 - 1 + lane;
  const bool xin = x >= 0 && x < w;
  const int xc = xin ? x : (x < 0 ? 0 : w - 1);
  const bool xl = x > 0, xr = x + 1 < w, xr2 = x + 2 < w, xr3 = x + 3 < w;
  const bool emit = lane >= 1 && lane <= kMsCols && x < w;
  // Loads from clamped addresses, not zeroed: values of lanes outside the
  // image and of rows -1 / h only reach results that are never stored (see
  // the border rules above), and an unconditional load keeps the compiler
  // from turning it into a branch that waits on it at once.
  auto ld = [&](const float* p, int y) {
    const int yc = y < 0 ? 0 : (y < h ? y : h - 1);
    return row_ptr(p, yc, w)[static_cast<unsigned>(xc)];
  };
  const float wt = 0.679144890667f;
  const float scale = 1.0f / (5.0f + 4 * wt);
  const bool tiny = w < 4 || h < 4;
  const int yd0 = ys - 1, yd1 = min(ye + 3, h);
  float ap = ld(pa, yd0 - 1), bp = ld(pb, yd0 - 1);
  float ac = ld(pa, yd0), bc = ld(pb, yd0);
  float an = ld(pa, yd0 + 1), bn = ld(pb, yd0 + 1);
  float d0 = 0.0f, d0l = 0.0f, d0r = 0.0f, d1 = 0.0f, d1l = 0.0f, d1r = 0.0f;  // dd rows yd-2, yd-1
  float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f;  // averages of rows yA-3 .. yA-1
  // the 4-minimum of one row from its window's average minimum (columns clip)
  auto min4 = [&](float mn) {
    const float m1 = wave_next(mn), m2 = wave_next(m1), m3 = wave_next(m2);
    float o = mn;
    o = (xr && m1 < o) ? m1 : o;
    o = (xr2 && m2 < o) ? m2 : o;
    o = (xr3 && m3 < o) ? m3 : o;
    return o;
  };
#pragma unroll 3
  for (int yd = yd0; yd <= yd1; ++yd) {
    const float an2 = ld(pa, yd + 2), bn2 = ld(pb, yd + 2);  // next iteration's "next"
    // differences at row yd (used where 0 <= yd < h)
    float dv;
    {
      // both shifts by every lane (a DPP read from a lane that is masked off
      // returns 0), then the select
      const float an_x = wave_next(ac), ap_x = wave_prev(ac);
      const float bn_x = wave_next(bc), bp_x = wave_prev(bc);
      const float ah = xr ? an_x : ap_x;
      const float bh = xr ? bn_x : bp_x;
      const bool down = yd + 1 < h;
      const float av = down ? an : ap, bv = down ? bn : bp;
      const float s0 = mask_diff_abs<C>(tab, ac - ah) + mask_diff_abs<C>(tab, ac - av);
      const float s1 = mask_diff_abs<C>(tab, bc - bh) + mask_diff_abs<C>(tab, bc - bv);
      dv = s1 < s0 ? s1 : s0;
    }
    const float dl = wave_prev(dv), dr = wave_next(dv);
    // 3x3 average at row yA = yd - 1 from dd rows yd-2 (d0), yd-1 (d1), yd (dv);
    // missing neighbours add +0 (all terms are >= +0, so x + 0 == x)
    const int yA = yd - 1;
    if (yA >= ys && yA < h) {
      float acc = d1;
      if (!tiny) {
        if (yA > 0) {
          acc += xl ? d0l * wt : 0.0f;
          acc += d0;
          acc += xr ? d0r * wt : 0.0f;
        }
        acc += xl ? d1l : 0.0f;
        acc += xr ? d1r : 0.0f;
        if (yA + 1 < h) {
          acc += xl ? dl * wt : 0.0f;
          acc += dv;
          acc += xr ? dr * wt : 0.0f;
        }
        acc = acc * scale;
      }
      // vertical 4-minimum of row yM = yA - 3 (complete: rows yM .. yA)
      const int yM = yA - 3;
      if (yM >= ys && yM < ye) {
        float mn = q0;
        if (q1 < mn) mn = q1;
        if (q2 < mn) mn = q2;
        if (acc < mn) mn = acc;
        const float o = min4(mn);
        if (emit) row_ptr(out, yM, w)[static_cast<unsigned>(x)] = o;
      }
      q0 = q1;
      q1 = q2;
      q2 = acc;
    }
    d0 = d1; d0l = d1l; d0r = d1r;
    d1 = dv; d1l = dl; d1r = dr;
    ap = ac; bp = bc;
    ac = an; bc = bn;
    an = an2; bn = bn2;
  }
  // rows whose 4-window runs past the bottom of the image: yM in
  // [max(ys, h - 3), ye), window yM .. h - 1 (the last averages are q0..q2)
  const int last = min(ye + 3, h) - 1;  // last average row computed (= q2)
  for (int yM = max(ys, last - 2); yM < ye; ++yM) {
    if (yM + 3 <= last) continue;  // already produced in the loop
    float mn = yM == last - 2 ? q0 : (yM == last - 1 ? q1 : q2);
    if (yM <= last - 2 && q1 < mn) mn = q1;
    if (yM <= last - 1 && q2 < mn) mn = q2;
    const float o = min4(mn);
    if (emit) row_ptr(out, yM, w)[static_cast<unsigned>(x)] = o;
  }
}

__global__ __launch_bounds__(256) void k_mask_stream(const float* __restrict__ a,
                                                     const float* __restrict__ b, int w, int h,
                                                     int strips, int segs, int kRows,
                                                     float* __restrict__ out) {
  __shared__ float2 tab[2][21];
  if (threadIdx.x < 42) {
    const int c = threadIdx.x / 21, i = threadIdx.x % 21;
    const float* t = c == 0 ? c_tab.hf_dx : c_tab.hf_dy;
    tab[c][i] = make_float2(t[i], i < 20 ? t[i + 1] - t[i] : 0.0f);
  }
  __syncthreads();
  const int item = blockIdx.x * 4 + wave_id();
  if (item >= 3 * strips * segs) return;
  const int c = item / (strips * segs), r0 = item % (strips * segs);
  const int x0 = (r0 % strips) * kMsCols, ys = (r0 / strips) * kRows;
  const size_t n = static_cast<size_t>(w) * h;
  const float* pa = a + c * n;
  const float* pb = b + c * n;
  float* po = out + c * n;
  if (c == 0) mask_front_wave<0>(pa, pb, w, h, x0, ys, kRows, tab[0], po);
  else if (c == 1) mask_front_wave<1>(pa, pb, w, h, x0, ys, kRows, tab[1], po);
  else mask_front_wave<2>(pa, pb, w, h, x0, ys, kRows, nullptr, po);
}

// The edge detector's blurs (S4, EdgeDetectorMapOpt :1456-1485: channel c
// of both MHIC outputs with sigma kSigEdgeX + c) and the mask front (S9-S11,
// DiffPrecomputeOpt + _Average5x5 + MinSquareValOpt on the same channel)
// fused: one wave per (channel, 56-column strip, row segment) reads its
// rows of m0[c] and m1[c] once and runs both register pipelines on them --
// the blur of k_blur_stream with the two planes as the packed pair (one
// input row per step), and the mask front of mask_front_wave one row later
// in its window.  Lane l is column x0 - 3 + l; both emit lanes 3 .. 58.
// Every value is formed by the same operations in the same order as the two
// separate kernels (blur taps ascending from +0 with zero outside the
// image, mask loads from clamped rows and columns), bit for bit.
constexpr int kEmCols = 56, kEmPf = 4;
// rows per wave: 32 where the strips x segments give enough waves (4K:
// 14k), else 16 (1080p: 32 rows leave 3.5k waves; 16 measured 5 % faster)
inline int EdgeMaskRows(int w, int h) {
  const long waves32 = 3L * ((w + kEmCols - 1) / kEmCols) * ((h + 31) / 32);
  return waves32 >= 8192 ? 32 : 16;
}

template <int C>
__device__ __forceinline__ void edge_mask_wave(const float* __restrict__ pa, const float* __restrict__ pb,
                                               float* __restrict__ ea, float* __restrict__ eb,
                                               float* __restrict__ mout, int w, int h, int x0, int ys,
                                               int rows, const float2* tab,
                                               const float* __restrict__ scales, int stride) {
  constexpr int kSig = kSigEdgeX + C;
  constexpr int R = BlurGeom<kSig>::R, NT = 2 * R + 1;
  static_assert(R <= 3, "edge blur radius");
  const BlurSpec& s = c_tab.blur[kSig];
  const int lane = threadIdx.x & 63;
  const int ye = min(ys + rows, h);
  const int x = x0 - 3 + lane;
  const bool xin = x >= 0 && x < w;
  const int xc = xin ? x : (x < 0 ? 0 : w - 1);
  const bool xl = x > 0, xr = x + 1 < w, xr2 = x + 2 < w, xr3 = x + 3 < w;
  const bool emit = lane >= 3 && lane < 3 + kEmCols && x < w;
  const float sxv = x < w ? scales[static_cast<size_t>(kSig * 2) * stride + (x < 0 ? 0 : x)] : 0.0f;
  const float* sy = scales + static_cast<size_t>(kSig * 2 + 1) * stride;
  auto ld = [&](const float* p, int y) {  // clamped row and column, unmasked
    const int yc = y < 0 ? 0 : (y < h ? y : h - 1);
    return row_ptr(p, yc, w)[static_cast<unsigned>(xc)];
  };
  // ---- mask front state (mask_front_wave) ----
  const float wt = 0.679144890667f;
  const float scale = 1.0f / (5.0f + 4 * wt);
  const bool tiny = w < 4 || h < 4;
  const int yd0 = ys - 1, yd1 = min(ye + 3, h);
  float d0 = 0.0f, d0l = 0.0f, d0r = 0.0f, d1 = 0.0f, d1l = 0.0f, d1r = 0.0f;
  float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f;
  auto min4 = [&](float mn) {
    const float m1 = wave_next(mn), m2 = wave_next(m1), m3 = wave_next(m2);
    float o = mn;
    o = (xr && m1 < o) ? m1 : o;
    o = (xr2 && m2 < o) ? m2 : o;
    o = (xr3 && m3 < o) ? m3 : o;
    return o;
  };
  // ---- edge blur state: horizontally blurred rows y - NT + 1 .. y ----
  f32x2 hq[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) hq[t] = f32x2{0.0f, 0.0f};
  // rows y - 3 .. y of both planes (clamped values), and kEmPf rows ahead
  const int Y0 = ys - 3, Y1 = max(ye + R - 1, yd1 + 2);
  // Rows y - 3 .. y of both planes (clamped values) and kEmPf rows ahead, as
  // 4-slot rings whose phase is the loop's unrolling position: the row loop
  // runs in groups of four calls of step<Q>, where logical row y - 3 + k sits
  // in slot (Q + k) & 3 -- no register moves to shift the rings (they were a
  // third of the loop's VALU instructions).
  static_assert(kEmPf == 4, "ring of 4");
  float ra[4], rb[4], fa[4], fb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ra[k] = rb[k] = 0.0f;
    // (the phase before the first step is 3: ahead row Y0 + k in slot (3 + k) & 3)
    fa[(3 + k) & 3] = ld(pa, Y0 + k);
    fb[(3 + k) & 3] = ld(pb, Y0 + k);
  }
  auto step = [&](auto phase, int y) {
    constexpr int Q = decltype(phase)::value;
    // the ring shift: the slot of the oldest row takes the next row, whose
    // ahead slot takes row y + kEmPf
    ra[(Q + 3) & 3] = fa[(Q + 3) & 3];
    rb[(Q + 3) & 3] = fb[(Q + 3) & 3];
    // (rows past the segment's last, Y1, are never read: the load takes row
    // Y1 again -- an L2 hit, no HBM read -- instead of skipping it, which
    // cost more than the traffic it saved: the loads' pipelining)
    fa[(Q + 3) & 3] = ld(pa, min(y + kEmPf, Y1));
    fb[(Q + 3) & 3] = ld(pb, min(y + kEmPf, Y1));
    const float r0a = ra[Q & 3], r1a = ra[(Q + 1) & 3], r2a = ra[(Q + 2) & 3], r3a = ra[(Q + 3) & 3];
    const float r0b = rb[Q & 3], r1b = rb[(Q + 1) & 3], r2b = rb[(Q + 2) & 3], r3b = rb[(Q + 3) & 3];
    // ---- edge blur: row y into the queue, output row y - R ----
    {
      const bool ok = xin && y >= 0 && y < h;
      float a0[NT], a1[NT];
      a0[R] = masked(r3a, ok);
      a1[R] = masked(r3b, ok);
#pragma unroll
      for (int k = 1; k <= R; ++k) {
        a0[R + k] = wave_next(a0[R + k - 1]);
        a1[R + k] = wave_next(a1[R + k - 1]);
        a0[R - k] = wave_prev(a0[R - k + 1]);
        a1[R - k] = wave_prev(a1[R - k + 1]);
      }
      f32x2 hs = {0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < NT; ++t) hs += f32x2{a0[t], a1[t]} * s.taps[t];
      hs *= sxv;
#pragma unroll
      for (int t = 0; t + 1 < NT; ++t) hq[t] = hq[t + 1];
      hq[NT - 1] = hs;
      const int yo = y - R;
      if (yo >= ys && yo < ye) {
        f32x2 acc = {0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < NT; ++t) acc += hq[t] * s.taps[t];
        const float sc = sy[yo];
        if (emit) {
          row_ptr(ea, yo, w)[static_cast<unsigned>(x)] = acc.x * sc;
          row_ptr(eb, yo, w)[static_cast<unsigned>(x)] = acc.y * sc;
        }
      }
    }
    // ---- mask front step at row yd = y - 2 (rows yd - 1 .. yd + 2 in r*) ----
    const int yd = y - 2;
    if (yd < yd0 || yd > yd1) return;
    const float ap = r0a, ac = r1a, an = r2a;
    const float bp = r0b, bc = r1b, bn = r2b;
    float dv;
    {
      const float an_x = wave_next(ac), ap_x = wave_prev(ac);
      const float bn_x = wave_next(bc), bp_x = wave_prev(bc);
      const float ah = xr ? an_x : ap_x;
      const float bh = xr ? bn_x : bp_x;
      const bool down = yd + 1 < h;
      const float av = down ? an : ap, bv = down ? bn : bp;
      const float s0 = mask_diff_abs<C>(tab, ac - ah) + mask_diff_abs<C>(tab, ac - av);
      const float s1 = mask_diff_abs<C>(tab, bc - bh) + mask_diff_abs<C>(tab, bc - bv);
      dv = s1 < s0 ? s1 : s0;
    }
    const float dl = wave_prev(dv), dr = wave_next(dv);
    const int yA = yd - 1;
    if (yA >= ys && yA < h) {
      float acc = d1;
      if (!tiny) {
        if (yA > 0) {
          acc += xl ? d0l * wt : 0.0f;
          acc += d0;
          acc += xr ? d0r * wt : 0.0f;
        }
        acc += xl ? d1l : 0.0f;
        acc += xr ? d1r : 0.0f;
        if (yA + 1 < h) {
          acc += xl ? dl * wt : 0.0f;
          acc += dv;
          acc += xr ? dr * wt : 0.0f;
        }
        acc = acc * scale;
      }
      const int yM = yA - 3;
      if (yM >= ys && yM < ye) {
        float mn = q0;
        if (q1 < mn) mn = q1;
        if (q2 < mn) mn = q2;
        if (acc < mn) mn = acc;
        const float o = min4(mn);
        if (emit) row_ptr(mout, yM, w)[static_cast<unsigned>(x)] = o;
      }
      q0 = q1;
      q1 = q2;
      q2 = acc;
    }
    d0 = d1; d0l = d1l; d0r = d1r;
    d1 = dv; d1l = dl; d1r = dr;
  };
  for (int y = Y0; y <= Y1; y += 4) {  // (wave-uniform bounds)
    step(std::integral_constant<int, 0>{}, y);
    if (y + 1 <= Y1) step(std::integral_constant<int, 1>{}, y + 1);
    if (y + 2 <= Y1) step(std::integral_constant<int, 2>{}, y + 2);
    if (y + 3 <= Y1) step(std::integral_constant<int, 3>{}, y + 3);
  }
  const int last = min(ye + 3, h) - 1;  // last average row computed (= q2)
  for (int yM = max(ys, last - 2); yM < ye; ++yM) {
    if (yM + 3 <= last) continue;
    float mn = yM == last - 2 ? q0 : (yM == last - 1 ? q1 : q2);
    if (yM <= last - 2 && q1 < mn) mn = q1;
    if (yM <= last - 1 && q2 < mn) mn = q2;
    const float o = min4(mn);
    if (emit) row_ptr(mout, yM, w)[static_cast<unsigned>(x)] = o;
  }
}

// m0 / m1: the MHIC outputs (3 planes each); edge: the 6 blurred planes (c:
// m0's channel c, 3 + c: m1's); mask: the mask front's 3 planes.
#ifndef GZ_EM_WAVES
#define GZ_EM_WAVES 1
#endif
__global__ __launch_bounds__(256, GZ_EM_WAVES) void k_edge_mask_stream(const float* __restrict__ m0,
                                                          const float* __restrict__ m1, int w,
                                                          int h, int strips, int segs, int rows,
                                                          float* __restrict__ edge,
                                                          float* __restrict__ mask,
                                                          const float* __restrict__ scales,
                                                          int stride) {
  __shared__ float2 tab[2][21];
  if (threadIdx.x < 42) {
    const int c = threadIdx.x / 21, i = threadIdx.x % 21;
    const float* t = c == 0 ? c_tab.hf_dx : c_tab.hf_dy;
    tab[c][i] = make_float2(t[i], i < 20 ? t[i + 1] - t[i] : 0.0f);
  }
  __syncthreads();
  const int item = blockIdx.x * 4 + wave_id();
  if (item >= 3 * strips * segs) return;
  const int c = item / (strips * segs), r0 = item % (strips * segs);
  const int x0 = (r0 % strips) * kEmCols, ys = (r0 / strips) * rows;
  const size_t n = static_cast<size_t>(w) * h;
  const float* pa = m0 + c * n;
  const float* pb = m1 + c * n;
  float* ea = edge + c * n;
  float* eb = edge + (3 + c) * n;
  float* po = mask + c * n;
  if (c == 0) edge_mask_wave<0>(pa, pb, ea, eb, po, w, h, x0, ys, rows, tab[0], scales, stride);
  else if (c == 1) edge_mask_wave<1>(pa, pb, ea, eb, po, w, h, x0, ys, rows, tab[1], scales, stride);
  else edge_mask_wave<2>(pa, pb, ea, eb, po, w, h, x0, ys, rows, nullptr, scales, stride);
}

// ---------------------------------------------------------------------------
// CombineChannelsOpt (:1542-1565) fused with the mask LUT tail of MaskOpt and
// the square-root step of CalculateDiffmapOpt (:944-946).  mk[c] is the
// blurred mask plane c in downsampled form for sigma id kSigMaskX + c.
// ---------------------------------------------------------------------------

struct MaskPlanes {
  const float* p[3];
  int step[3];  // down-sampling of each plane (kSigMaskBSub: B every 3rd row / column)
};

__device__ __forceinline__ float mask_at(const MaskPlanes& mk, int c, int w, int h, int y, int x) {
  const int step = mk.step[c];
  const int dx = (w + step - 1) / step;
  return mk.p[c][static_cast<size_t>(y / step) * dx + x / step];
}

__global__ __launch_bounds__(256) void k_combine(MaskPlanes mk, const float* __restrict__ dc,
                                                 const float* __restrict__ ac,
                                                 const float* __restrict__ edge, int w, int h,
                                                 int rw, int rh, float* __restrict__ resval,
                                                 float* __restrict__ combined_dbg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (i >= rw) return;
  const int rx = 3 * i, ry = 3 * j;
  const size_t r = static_cast<size_t>(j) * rw + i;
  if (!(ry + 5 < h && rx + 5 < w)) {
    resval[r] = 0.0f;
    if (combined_dbg) combined_dbg[r] = 0.0f;
    return;
  }
  float m[3], mdc[3];
  mask_luts(mask_at(mk, 0, w, h, ry + 3, rx + 3), mask_at(mk, 1, w, h, ry + 3, rx + 3),
            mask_at(mk, 2, w, h, ry + 3, rx + 3), m, mdc);
  const float* pd = dc + 3 * r;
  const float* pa = ac + 3 * r;
  const float* pe = edge + 3 * r;
  const float v = (pd[0] * mdc[0] + pd[1] * mdc[1] + pd[2] * mdc[2]) +
                  (pa[0] * m[0] + pa[1] * m[1] + pa[2] * m[2]) +
                  (pe[0] * m[0] + pe[1] * m[1] + pe[2] * m[2]);
  if (combined_dbg) combined_dbg[r] = v;
  const float kSlope = 100.0f;
  resval[r] = static_cast<double>(v) < (1.0 / static_cast<double>(kSlope * kSlope)) ? kSlope * v
                                                                                    : sqrtf(v);
}

// Mask scale at each 8x8 block's top-left pixel for the per-block search
// (ButteraugliComparator::CompareBlock, butteraugli_comparator.cc:148-151).
// CombineChannelsOpt + the square root of CalculateDiffmapOpt when the
// vertical mask pass already applied MaskOpt's LUTs (mk: the masks, mkdc:
// the DC masks, both per blurred sample): k_combine without the S13 tail.
// lf0 / lf1 (non-null): EdgeDetectorLowFreq's term is added here instead of
// by k_low_freq -- point (i, j) takes the term of k_low_freq's thread
// (i - 2, j), the same float add onto block_diff's AC value.
constexpr int kMaskStepSub[3] = {BlurGeom<kSigMaskX>::STEP, BlurGeom<kSigMaskY>::STEP,
                                 BlurGeom<kSigMaskBSub>::STEP};
__global__ __launch_bounds__(256) void k_combine_channels(MaskPlanes mk, MaskPlanes mkdc,
                                                          const float* __restrict__ dc,
                                                          const float* __restrict__ ac,
                                                          const float* __restrict__ edge, int w,
                                                          int h, int rw, int rh,
                                                          float* __restrict__ resval,
                                                          const float* __restrict__ lf0,
                                                          const float* __restrict__ lf1) {
  __shared__ float s_lf[21];
  if (threadIdx.x < 21) s_lf[threadIdx.x] = c_tab.lf_dy[threadIdx.x];
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (i >= rw) return;
  const int rx = 3 * i, ry = 3 * j;
  const size_t r = static_cast<size_t>(j) * rw + i;
  if (!(ry + 5 < h && rx + 5 < w)) {
    resval[r] = 0.0f;
    return;
  }
  // (the search's planes, MaskPlanesOf(.., sub_b = true): compile-time
  // steps, so each plane index is a few multiplies, shared by mk and mkdc;
  // the launch checks mk.step / mkdc.step against kMaskStepSub)
  float m[3], mdc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int st = kMaskStepSub[c];
    const size_t q = static_cast<size_t>((ry + 3) / st) * ((w + st - 1) / st) + (rx + 3) / st;
    m[c] = mk.p[c][q];
    mdc[c] = mkdc.p[c][q];
  }
  const float* pd = dc + 3 * r;
  const float* pe = edge + 3 * r;
  float pa[3] = {ac[3 * r], ac[3 * r + 1], ac[3 * r + 2]};
  if (lf0 && w >= 9 && h >= 9) {  // (smaller: no point has the term)
    // (its loads from a clamped point when the term does not apply, so that
    // they issue with the ones above instead of behind a branch)
    const bool lf = i >= 2 && 3 * (i - 2) + 8 < w && 3 * j + 8 < h;
    float mx[3];
    low_freq_max(lf0, lf1, w, h, lf ? i - 2 : 0, lf ? j : 0, s_lf, mx);
    if (lf) {
#pragma unroll
      for (int c = 0; c < 3; ++c) pa[c] += 10.0f * mx[c];
    }
  }
  const float v = (pd[0] * mdc[0] + pd[1] * mdc[1] + pd[2] * mdc[2]) +
                  (pa[0] * m[0] + pa[1] * m[1] + pa[2] * m[2]) +
                  (pe[0] * m[0] + pe[1] * m[1] + pe[2] * m[2]);
  const float kSlope = 100.0f;
  resval[r] = static_cast<double>(v) < (1.0 / static_cast<double>(kSlope * kSlope)) ? kSlope * v
                                                                                    : sqrtf(v);
}

__global__ __launch_bounds__(256) void k_mask_scale(MaskPlanes mk, int w, int h, int bw, int nb,
                                                    float* __restrict__ scale) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  const int x = 8 * (b % bw), y = 8 * (b / bw);
  float m[3], mdc[3];
  mask_luts(mask_at(mk, 0, w, h, y, x), mask_at(mk, 1, w, h, y, x), mask_at(mk, 2, w, h, y, x),
            m, mdc);
  scale[3 * b] = m[0];
  scale[3 * b + 1] = m[1];
  scale[3 * b + 2] = m[2];
}

// ---------------------------------------------------------------------------
// CalculateDiffmapOpt (:923-978).  The splatted map restricted to the crop
// (w-5)x(h-5) at offset (2,2) is resval[(y/3)*rw + x/3]; its sigma-8.85
// blur (step 2, border ratio .0303) runs on that implicit image.
// ---------------------------------------------------------------------------

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// CalculateDiffmapOpt's blur, the final map, its 8x8-block maxima and the
// image maximum in one launch (round 5; four launches before: the blur's
// two passes through HBM, the final pixels, the maximum -- 34 us of a 1080p
// Compare pass, latency-bound).  A workgroup owns a kDmTile x kDmTile pixel
// tile.  The horizontal pass runs once per res row (image rows 3j .. 3j + 2
// repeat res row j, so their sums are equal) over that row expanded to
// pixels in LDS with zeros outside the (w-5) x (h-5) crop, for the tile's
// step-2 columns; its outputs are written to each pixel row they stand for
// (zero rows outside the crop), so that the vertical pass, for the tile's
// step-2 samples, and the horizontal one read each tap with one LDS load at
// an immediate offset.  Then the final pixels (:967-978: the splatted value
// plus 24.82 x the blurred one, times 1 / (1 + 24.82)) and the maxima of the
// tile's 8x8 blocks (ButteraugliComparator's block maxima,
// butteraugli_comparator.cc:177-191).  Each blur output sums its 39 taps in
// ascending order from +0 (zero outside the crop), then takes its border
// scale -- ConvolutionOpt's arithmetic, as the two-pass kernels.  The image
// maximum (ButteraugliScoreFromDiffmap, butteraugli.cc:1233-1240): each
// workgroup stores its maximum into mapped host memory (the host folds them:
// Engine::CompareFinish) and adds it by an atomic max into one of kDmMaxWords
// device words (k_jpeg_code's skip test folds those).  An atomic max per
// workgroup on ONE word serialised into tens of us at 2040 workgroups (4K),
// arrival counting in every workgroup cost more than a fold launch, and the
// fold launch (k_distance, rounds 4-5) cost ~4 us per pass; spread over 64
// words the atomics are ~32 per word at 4K.  The words are zeroed by the
// pass's first kernel (k_opsin_mhic_stream); values are >= +0, so their bits
// order as the floats do.
constexpr int kDmTile = 64;                          // pixels per tile side (8 x 8 blocks; 32: 2040 workgroups at 1080p, 1.4x slower)
constexpr int kDmOut = kDmTile / 2;                  // step-2 samples per tile side
constexpr int kDmSpan = 2 * (kDmOut - 1) + 2 * 19 + 1;  // pixels under a tile's taps (101)
constexpr int kDmRes = (kDmSpan + 2) / 3 + 2;        // res rows / columns under them
#ifndef GZ_DM_T
#define GZ_DM_T 512
#endif
// threads per tile: 510 tiles at 1080p leave 2 per CU, so the waves per tile
// set the latency hiding (256 -> 512: 15.4 -> 10.9 us at 1080p, 36.6 -> 29.5
// at 4K; 1024: 10.4 / 35.6 -- profiles/round5_diffmap_threads_ab.txt)
constexpr int kDmThreads = GZ_DM_T;
static_assert(kDmThreads % 64 == 0 && kDmThreads <= 1024, "whole waves");
__global__ __launch_bounds__(kDmThreads) void k_diffmap(const float* __restrict__ resval, int rw, int rh, int w, int h,
                                                 int bw, int bh, const float* __restrict__ scales, int stride,
                                                 float* __restrict__ distmap, float* __restrict__ block_max,
                                                 float* __restrict__ wg_host, uint32_t* __restrict__ dmax) {
  constexpr int R = BlurGeom<kSigDiffmap>::R, NT = 2 * R + 1;
  static_assert(BlurGeom<kSigDiffmap>::STEP == 2, "step-2 samples");
  constexpr int kPx = kDmSpan + 3;  // (row stride)
  __shared__ float s_px[kDmRes][kPx];          // res rows expanded to crop pixels xs .. xs + kDmSpan - 1
  __shared__ float s_hb[kDmSpan][kDmOut];      // horizontal outputs per crop row ys .. ys + kDmSpan - 1
  __shared__ float s_dd[kDmOut][kDmOut];
  __shared__ float s_res[kDmTile / 3 + 3][kDmTile / 3 + 3];  // the tile's own res values (splatted term)
  static_assert(kDmTile % 8 == 0 && kDmThreads % ((kDmTile / 8) * (kDmTile / 8)) == 0, "whole blocks per tile");
  __shared__ float s_w[kDmThreads / 64];
  const BlurSpec& sp = c_tab.blur[kSigDiffmap];
  const int t = threadIdx.x;
  const int X0 = static_cast<int>(blockIdx.x) * kDmTile, Y0 = static_cast<int>(blockIdx.y) * kDmTile;
  const int wc = w - 5, hc = h - 5;  // the crop, at offset (2, 2)
  // the tile's crop coordinates and step-2 samples
  const int xc0 = max(0, X0 - 2), xc1 = min(wc - 1, X0 + kDmTile - 3);
  const int yc0 = max(0, Y0 - 2), yc1 = min(hc - 1, Y0 + kDmTile - 3);
  const bool any = xc0 <= xc1 && yc0 <= yc1;
  const int ox0 = xc0 >> 1, ox1 = xc1 >> 1, oy0 = yc0 >> 1, oy1 = yc1 >> 1;
  const int xs = 2 * ox0 - R, ys = 2 * oy0 - R;  // first crop column / row under the taps
  // res rows of the crop rows ys .. ys + kDmSpan - 1 that lie in the crop
  const int r0 = max(0, ys) / 3, r1 = min(hc - 1, ys + kDmSpan - 1) / 3;
  const int nr = any ? r1 - r0 + 1 : 0;
  // the tile's own res values (pixel (x, y): res ((y - 2) / 3, (x - 2) / 3))
  const int q0 = (max(Y0, 2) - 2) / 3, p0 = (max(X0, 2) - 2) / 3;
  const int q1 = min(rh - 1, (max(min(Y0 + kDmTile - 1, h - 1), 2) - 2) / 3);
  const int p1 = min(rw - 1, (max(min(X0 + kDmTile - 1, w - 1), 2) - 2) / 3);
  // staging: every load of the thread issued before its first LDS store (a
  // load-then-store loop waits out each load in turn: 63 % of the wave
  // cycles were waits)
  constexpr int kResIt = ((kDmTile / 3 + 3) * (kDmTile / 3 + 3) + kDmThreads - 1) / kDmThreads;
  constexpr int kPxIt = (kDmRes * kDmSpan + kDmThreads - 1) / kDmThreads;
  const int nq = q1 - q0 + 1, np = p1 - p0 + 1;
  float vr[kResIt], vp[kPxIt];
#pragma unroll
  for (int it = 0; it < kResIt; ++it) {
    const int k = t + kDmThreads * it;
    vr[it] = k < nq * np ? resval[static_cast<size_t>(q0 + k / np) * rw + p0 + k % np] : 0.0f;
  }
#pragma unroll
  for (int it = 0; it < kPxIt; ++it) {
    const int k = t + kDmThreads * it, rr = k / kDmSpan, x = xs + k % kDmSpan;
    const bool in = k < nr * kDmSpan && x >= 0 && x < wc;
    vp[it] = in ? resval[static_cast<size_t>(r0 + rr) * rw + x / 3] : 0.0f;
  }
  // the border scales of the tile's samples
  __shared__ float s_sx[kDmOut], s_sy[kDmOut];
  float sc = 0.0f;
  if (any && t < 2 * kDmOut) {
    const int q = t & (kDmOut - 1);
    sc = t < kDmOut ? (ox0 + q <= ox1 ? scales[static_cast<size_t>(kSigDiffmap * 2) * stride + 2 * (ox0 + q)] : 0.0f)
                    : (oy0 + q <= oy1 ? scales[static_cast<size_t>(kSigDiffmap * 2 + 1) * stride + 2 * (oy0 + q)]
                                      : 0.0f);
  }
#pragma unroll
  for (int it = 0; it < kResIt; ++it) {
    const int k = t + kDmThreads * it;
    if (k < nq * np) s_res[k / np][k % np] = vr[it];
  }
#pragma unroll
  for (int it = 0; it < kPxIt; ++it) {
    const int k = t + kDmThreads * it;
    if (k < nr * kDmSpan) s_px[k / kDmSpan][k % kDmSpan] = vp[it];
  }
  if (any && t < 2 * kDmOut) (t < kDmOut ? s_sx : s_sy)[t & (kDmOut - 1)] = sc;
  // crop rows outside the crop: zero rows of the vertical pass's input
  if (any)
    for (int k = t; k < kDmSpan * kDmOut; k += kDmThreads) {
      const int y = ys + k / kDmOut;
      if (y < 0 || y >= hc) s_hb[k / kDmOut][k % kDmOut] = 0.0f;
    }
  __syncthreads();
  if (any) {
    // horizontal pass: res row r0 + rr, sample ox0 + q (crop x = 2 ox:
    // taps from s_px[rr][2 q])
    for (int k = t; k < nr * kDmOut; k += kDmThreads) {
      const int rr = k / kDmOut, q = k % kDmOut, ox = ox0 + q;
      if (ox > ox1) continue;
      const float* src = &s_px[rr][2 * q];
      float sum = 0.0f;
#pragma unroll
      for (int i = 0; i < NT; ++i) sum += src[i] * sp.taps[i];
      const float hv = sum * s_sx[q];
      // the crop rows of res row r0 + rr inside the vertical pass's span
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const int y = 3 * (r0 + rr) + d;
        if (y >= ys && y < ys + kDmSpan && y < hc) s_hb[y - ys][q] = hv;
      }
    }
  }
  __syncthreads();
  if (any) {
    // vertical pass: sample (oy0 + pr, ox0 + q), crop rows 2 oy - R + i =
    // s_hb rows 2 pr + i
    for (int k = t; k < kDmOut * kDmOut; k += kDmThreads) {
      const int pr = k / kDmOut, q = k % kDmOut, oy = oy0 + pr;
      if (oy > oy1 || ox0 + q > ox1) continue;
      const float* src = &s_hb[2 * pr][q];
      float acc = 0.0f;
#pragma unroll
      for (int i = 0; i < NT; ++i) acc += src[i * kDmOut] * sp.taps[i];
      s_dd[pr][q] = acc * s_sy[pr];
    }
  }
  __syncthreads();
  // the final pixels: kDmThr threads per 8x8 block, kDmPx pixels each
  constexpr int kDmBlk = kDmTile / 8, kDmThr = kDmThreads / (kDmBlk * kDmBlk), kDmPx = 64 / kDmThr;
  const int blk = t / kDmThr, sub = t % kDmThr;
  const int bx = static_cast<int>(blockIdx.x) * kDmBlk + (blk % kDmBlk);
  const int by = static_cast<int>(blockIdx.y) * kDmBlk + (blk / kDmBlk);
  const float scale = static_cast<float>(1.0 / (1.0 + static_cast<double>(24.8235314874f)));
  float m = 0.0f;
#pragma unroll
  for (int u = 0; u < kDmPx; ++u) {
    const int p = sub * kDmPx + u, iy = p >> 3, ix = p & 7;
    const int y = by * 8 + iy, x = bx * 8 + ix;
    float v = 0.0f;
    if (x < w && y < h) {
      float dval = 0.0f;
      if (x >= 2 && y >= 2) {
        const int ry = (y - 2) / 3, rx = (x - 2) / 3;
        if (3 * ry + 5 < h && 3 * rx + 5 < w) dval = s_res[ry - q0][rx - p0];
      }
      if (x >= 2 && y >= 2 && x < w - 3 && y < h - 3)
        dval += 24.8235314874f * s_dd[((y - 2) >> 1) - oy0][((x - 2) >> 1) - ox0];
      v = dval * scale;
      if (distmap) distmap[static_cast<size_t>(y) * w + x] = v;
    }
    m = fmaxf(m, v);
  }
#pragma unroll
  for (int o = 1; o < kDmThr; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (sub == 0 && bx < bw && by < bh) block_max[static_cast<size_t>(by) * bw + bx] = m;
  m = wave_max(m);
  if ((t & 63) == 0) s_w[t >> 6] = m;
  __syncthreads();
  if (t == 0) {
    const int g = blockIdx.y * gridDim.x + blockIdx.x;
    float mm = s_w[0];
#pragma unroll
    for (int i = 1; i < kDmThreads / 64; ++i) mm = fmaxf(mm, s_w[i]);
    wg_host[g] = mm;
    atomicMax(&dmax[g % kDmMaxWords], __float_as_uint(mm));
  }
}

}  // namespace gz
