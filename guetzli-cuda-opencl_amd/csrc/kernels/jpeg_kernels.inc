// Entropy coding of a candidate on the device (the per-iteration
// SaveToJpegData + WriteJpeg of processor.cc:319-323, 899-904, which the
// search runs only to size and keep the best candidate).  Two passes over
// the blocks of the HBM-resident coefficients:
//   k_jpeg_stage  DC/AC symbol histograms of the coefficients quantized as
//                 SaveToJpegData divides them (LDS then global atomics) and
//                 the count of non-zero chroma coefficients -- not needed
//                 when the host already knows the histograms (the search
//                 back end tracks them exactly);
//   -- host: clustering + Huffman code lengths (tiny) and the header --
//   k_jpeg_code   the scan in one launch from the coefficients themselves
//                 (quantized on the fly): every MCU's bits, their offsets
//                 (a decoupled look-back over workgroups), the bits at those
//                 offsets (words stored byte-swapped so the buffer is the
//                 MSB-first byte stream), the last byte padded, and the
//                 count of the bytes stuffing doubles (so the file size is
//                 known without the bytes);
//   -- host, for the kept candidate only: 0xff stuffing, EOI --
// The symbols and codes are those of jpeg_data_writer.cc:447-538 (and of the
// host writer, host/jpeg_writer.cc), so the bytes are identical.  Both
// kernels also work on a range of MCUs at a bit offset of the stream (one
// rank's part of a frame split over ranks, host/strips.h).
// Included by gz_device.hip.
#pragma once

namespace gz {

struct JpegQuantF {      // quant value at each zigzag position, as float
  float qz[3][64];
};

// The Huffman codes of a scan, passed by value as k_jpeg_code's kernel
// argument (2.4 KB of the 4 KB kernarg segment: the launch carries them, no
// copy launch per candidate): per component and symbol 3 bytes, code low /
// code high / length; DC categories 0..16, AC symbols 0..255.
constexpr int kJDcSyms = 17;
struct JpegCodesArg {
  uint8_t dc[3][kJDcSyms][3];
  uint8_t ac[3][256][3];
};

constexpr int c_natural_order[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};

__device__ __forceinline__ int log2_floor_nz(uint32_t v) { return 31 - __clz(v); }

// A stored coefficient quantized as SaveToJpegData divides it: |stored| <=
// 2^15, q < 2^16, so the f32 quotient truncates to the exact integer
// quotient (see host/jpeg_writer.cc CoeffImageLoader).
__device__ __forceinline__ int16_t jpeg_quant(int16_t v, float q) {
  return static_cast<int16_t>(static_cast<int>(static_cast<float>(v) / q));
}

// jpeg_quant by the reciprocal: |v| * (1/q) rounds to within one of the
// quotient (|v| <= 2^15, relative error below 2^-22), and one multiply-compare
// each way settles the truncated quotient -- the same integer as the
// division, in a third of its instructions.
__device__ __forceinline__ int16_t jpeg_quant_rcp(int16_t v, int q, float rq) {
  const int a = v < 0 ? -static_cast<int>(v) : static_cast<int>(v);
  int n = static_cast<int>(static_cast<float>(a) * rq);
  n -= n * q > a ? 1 : 0;
  n += (n + 1) * q <= a ? 1 : 0;
  return static_cast<int16_t>(v < 0 ? -n : n);
}

// Quantized DC of block b of component c (0 before the first block).
__device__ __forceinline__ int16_t jpeg_dc(const int16_t* __restrict__ cur, const JpegQuantF& q,
                                           int nb, int c, int b) {
  if (b < 0) return 0;
  return jpeg_quant(cur[(static_cast<size_t>(c) * nb + b) * 64], q.qz[c][0]);
}

// hist: kJHistCopies copies of the device counts (6 x 256 each), then as
// many chroma non-zero counts (u64), all zero on entry.  Workgroup g adds
// into copy g % kJHistCopies: the common symbols are non-zero in every
// workgroup, and same-address device atomics serialise, so one copy would
// take one add per workgroup per symbol in turn.  k_hist_fold, the next
// launch, sums the copies into host_out (mapped pinned memory: counts, then
// the chroma count) and leaves the device words zero for the next
// candidate -- no fill and no copy in the stream.  (Round 4 folded them in
// the last workgroup to arrive; counting the arrivals of every workgroup
// cost more than the one-workgroup launch.)
constexpr int kJHistCopies = 8;
__global__ __launch_bounds__(1024) void k_hist_fold(uint32_t* __restrict__ hist, uint32_t* __restrict__ host_out,
                                                    int chroma) {
  for (int i = threadIdx.x; i < 6 * 256; i += 1024) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < kJHistCopies; ++k) {
      v += hist[k * (6 * 256) + i];
      hist[k * (6 * 256) + i] = 0u;
    }
    host_out[i] = v;
  }
  if (chroma && threadIdx.x == 0) {
    unsigned long long* chroma_nz = reinterpret_cast<unsigned long long*>(hist + kJHistCopies * 6 * 256);
    unsigned long long cn = 0;
    for (int k = 0; k < kJHistCopies; ++k) {
      cn += chroma_nz[k];
      chroma_nz[k] = 0ull;
    }
    host_out[6 * 256] = static_cast<uint32_t>(cn);
    host_out[6 * 256 + 1] = static_cast<uint32_t>(cn >> 32);
  }
}
__host__ __device__ constexpr size_t jhist_device_bytes(size_t stage_groups) {
  return kJHistCopies * 6 * 256 * 4 + kJHistCopies * 8 + (2 + stage_groups / 64 + 1) * 4;
}
// A workgroup takes 256 consecutive blocks (of the component-major
// [3][blocks] order), staged in LDS with one coalesced pass; each of its 16
// waves then takes one quarter (16 zigzag positions) of 64 of the blocks, so
// the quarter -- and with it every natural-order offset -- is uniform per
// wave (kQuarter below) and the per-thread work is a quarter of a block.
// The quarters' non-zero masks meet in LDS; each coefficient's AC symbol
// then comes from the block's mask alone (the run back to the previous
// non-zero), so the histogram counts equal the sequential run-length loop's.
constexpr int kStageBlocks = 256;
constexpr int kStageThreads = 4 * kStageBlocks;  // a wave per quarter of 64 blocks
constexpr int kStageStride = 33;  // words per staged block (bank spread)

template <int kQuarter>
__device__ __forceinline__ void jpeg_stage_quarter(const uint32_t* __restrict__ sb, int c,
                                                   const JpegQuantF& q, int16_t z[16], uint32_t* m16,
                                                   int* nz_stored) {
  const int16_t* v = reinterpret_cast<const int16_t*>(sb);
  uint32_t m = 0;
  int nz = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = 16 * kQuarter + i;
    const int16_t sv = v[c_natural_order[k]];
    nz += sv != 0;
    z[i] = jpeg_quant(sv, q.qz[c][k]);
    m |= static_cast<uint32_t>(z[i] != 0) << i;
  }
  *m16 = m;
  *nz_stored = nz;
}

// AC symbols of the quarter's non-zero coefficients (k >= 1) into hac.
template <int kQuarter>
__device__ __forceinline__ void jpeg_stage_symbols(const int16_t z[16], uint64_t m64,
                                                   uint32_t* __restrict__ hac) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = 16 * kQuarter + i;
    if (k == 0 || z[i] == 0) continue;
    const uint64_t below = m64 & ~1ull & ((1ull << k) - 1);
    const int prev = below ? 63 - __clzll(below) : 0;
    const int run = k - prev - 1;
    if (run > 15) atomicAdd(&hac[0xf0], static_cast<uint32_t>(run >> 4));
    const int a = z[i] < 0 ? -z[i] : z[i];
    atomicAdd(&hac[((run & 15) << 4) + log2_floor_nz(a) + 1], 1u);
  }
}

// Blocks [m0, m1) of every component (a rank's owned MCUs of a frame split
// over ranks; the whole image otherwise); the DC predictor of block m0 is
// block m0 - 1 (0 for the first block).
__global__ __launch_bounds__(kStageThreads) void k_jpeg_stage(const int16_t* __restrict__ cur, JpegQuantF q,
                                                     int nb, int m0, int m1,
                                                     uint32_t* __restrict__ hist) {
  unsigned long long* chroma_nz = reinterpret_cast<unsigned long long*>(hist + kJHistCopies * 6 * 256);
  // four histogram copies, one per wave & 3 (LDS atomics of a wave collide
  // on the common symbols; the EOB count goes by ballot)
  __shared__ uint32_t lh_all[4][6 * 256];
  __shared__ uint32_t sblk[kStageBlocks * kStageStride];
  __shared__ uint16_t smask[kStageBlocks][4];
  __shared__ int nz_red[kStageThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < 4 * 6 * 256; i += kStageThreads) (&lh_all[0][0])[i] = 0;
  const int nr = m1 - m0;
  const int ntot = 3 * nr;
  const int t0 = blockIdx.x * kStageBlocks;
  // stage the workgroup's blocks: 2 x 16 B per thread, coalesced
  {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int j = tid + kStageThreads * r;  // 16-B piece j of the workgroup's blocks
      const int lb = j >> 3, part = j & 7;
      if (t0 + lb < ntot) {
        const int tt = t0 + lb, cc = tt / nr;
        const uint4 u = reinterpret_cast<const uint4*>(
            cur + (static_cast<size_t>(cc) * nb + m0 + (tt - cc * nr)) * 64)[part];
        uint32_t* d = &sblk[lb * kStageStride + 4 * part];
        d[0] = u.x;
        d[1] = u.y;
        d[2] = u.z;
        d[3] = u.w;
      }
    }
  }
  __syncthreads();
  const int quarter = wv & 3;
  const int lb = 64 * (wv >> 2) + lane;
  const bool on = t0 + lb < ntot;
  const int c = on ? (t0 + lb) / nr : 0;
  const int t = c * nb + m0 + (t0 + lb - c * nr);  // (component, block) in the [3][nb] layout
  int16_t z[16];
  uint32_t m16 = 0;
  int nz_stored = 0;
  if (on) {
    const uint32_t* sb = &sblk[lb * kStageStride];
    switch (quarter) {  // wave-uniform
      case 0: jpeg_stage_quarter<0>(sb, c, q, z, &m16, &nz_stored); break;
      case 1: jpeg_stage_quarter<1>(sb, c, q, z, &m16, &nz_stored); break;
      case 2: jpeg_stage_quarter<2>(sb, c, q, z, &m16, &nz_stored); break;
      default: jpeg_stage_quarter<3>(sb, c, q, z, &m16, &nz_stored); break;
    }
    smask[lb][quarter] = static_cast<uint16_t>(m16);
  }
  __syncthreads();
  uint32_t* lh = lh_all[wv & 3];
  int eob_c = -1;  // component whose AC histogram gets this block's EOB
  if (on) {
    const uint64_t m64 = static_cast<uint64_t>(smask[lb][0]) | (static_cast<uint64_t>(smask[lb][1]) << 16) |
                         (static_cast<uint64_t>(smask[lb][2]) << 32) |
                         (static_cast<uint64_t>(smask[lb][3]) << 48);
    uint32_t* hac = lh + (2 * c + 1) * 256;
    switch (quarter) {
      case 0: {
        // DC symbol (BuildDCHistograms: Log2Floor(|dc - last|) + 1)
        const int b = t - c * nb;
        const int d = static_cast<int>(z[0]) - static_cast<int>(jpeg_dc(cur, q, nb, c, b - 1));
        const int ad = d < 0 ? -d : d;
        atomicAdd(&lh[(2 * c) * 256 + (ad ? log2_floor_nz(ad) + 1 : 0)], 1u);
        jpeg_stage_symbols<0>(z, m64, hac);
        break;
      }
      case 1: jpeg_stage_symbols<1>(z, m64, hac); break;
      case 2: jpeg_stage_symbols<2>(z, m64, hac); break;
      default:
        jpeg_stage_symbols<3>(z, m64, hac);
        if (!(m64 >> 63)) eob_c = c;  // coefficient 63 is zero: the block ends with an EOB
        break;
    }
  }
  // EOBs: per component, one count per wave
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) {
    const uint64_t bal = __ballot(eob_c == cc);
    if (lane == 0 && bal) atomicAdd(&lh[(2 * cc + 1) * 256], static_cast<uint32_t>(__popcll(bal)));
  }
  // chroma non-zeros (stored values): one atomic per workgroup
  int s = wave_sum_i(c > 0 ? nz_stored : 0);
  if (lane == 0) nz_red[wv] = s;
  __syncthreads();
  if (tid == 0) {
    s = 0;
    for (int i = 0; i < kStageThreads / 64; ++i) s += nz_red[i];
    if (s) atomicAdd(&chroma_nz[blockIdx.x % kJHistCopies], static_cast<unsigned long long>(s));
  }
  uint32_t* hcopy = hist + (blockIdx.x % kJHistCopies) * (6 * 256);
  for (int i = tid; i < 6 * 256; i += kStageThreads) {
    const uint32_t v = lh_all[0][i] + lh_all[1][i] + lh_all[2][i] + lh_all[3][i];
    if (v) atomicAdd(&hcopy[i], v);
  }
}

// Bits of coefficient k (= lane) of one block, EncodeDCTBlockSequential
// (jpeg_data_writer.cc:447-500) taken apart by position: lane 0 the DC
// difference (code + magnitude), a non-zero AC lane its ZRL codes, run/size
// code and magnitude (the run back to the previous non-zero comes from the
// wave's non-zero mask), lane 63 also the EOB when the last non-zero is
// before 63.  Laid end to end in lane order these are the block's bits.
// Split in two so that an MCU's three blocks issue their table loads
// together: jpeg_lane_sym (no memory) then jpeg_lane_bits (one lookup).
struct JpegLaneSym {
  int idx;           // table index of the lane's code (DC: size, AC: 256 + run/size), -1: none
  int nzrl;          // ZRL codes before the symbol
  int len1;          // magnitude bits
  uint32_t v1;
  bool eob;          // lane 63: EOB code after everything
};
struct JpegLaneBits {
  int n;             // total bits of the lane
  int nzrl;
  int len0, len1;    // code / magnitude bits (len0 = 0: nothing)
  uint32_t v0, v1;
  int eob_len;
  uint32_t eob;
};

__device__ __forceinline__ JpegLaneSym jpeg_lane_sym(int16_t zk, int lane, uint64_t m, int16_t last_dc) {
  JpegLaneSym r{-1, 0, 0, 0u, false};
  if (lane == 0) {
    int16_t diff = static_cast<int16_t>(zk - last_dc);
    int16_t dbits = diff;
    if (diff < 0) {
      diff = static_cast<int16_t>(-diff);
      --dbits;
    }
    const int nbd = diff ? log2_floor_nz(static_cast<uint32_t>(static_cast<int>(diff))) + 1 : 0;
    r.idx = nbd;
    r.len1 = nbd;
    r.v1 = nbd > 0 ? static_cast<uint32_t>(dbits & ((1 << nbd) - 1)) : 0u;
  } else if (zk != 0) {
    const uint64_t below = m & ~1ull & ((1ull << lane) - 1);
    const int prev = below ? 63 - __clzll(below) : 0;
    const int run = lane - prev - 1;
    int16_t v = zk;
    int16_t vb;
    if (v < 0) {
      v = static_cast<int16_t>(-v);
      vb = static_cast<int16_t>(~v);
    } else {
      vb = v;
    }
    const int nbits = log2_floor_nz(static_cast<uint32_t>(static_cast<int>(v))) + 1;
    r.idx = 256 + ((run & 15) << 4) + nbits;
    r.nzrl = run >> 4;
    r.len1 = nbits;
    r.v1 = static_cast<uint32_t>(vb & ((1 << nbits) - 1));
  }
  r.eob = lane == 63 && !(m >> 63);  // coefficient 63 is not the last non-zero
  return r;
}

// e: the lane's table entry (0 when idx < 0); zrl / eob: the component's
// ZRL and EOB entries (wave-uniform).
__device__ __forceinline__ JpegLaneBits jpeg_lane_bits(const JpegLaneSym& y, uint32_t e,
                                                       uint32_t zrl, uint32_t eob) {
  JpegLaneBits r;
  r.nzrl = y.nzrl;
  r.len0 = static_cast<int>(e >> 16);
  r.v0 = e & 0xffffu;
  r.len1 = y.len1;
  r.v1 = y.v1;
  r.eob_len = y.eob ? static_cast<int>(eob >> 16) : 0;
  r.eob = eob & 0xffffu;
  r.n = r.nzrl * static_cast<int>(zrl >> 16) + r.len0 + r.len1 + r.eob_len;
  return r;
}

// ORs the n (<= 16) low bits of v, MSB first, at bit p of the LDS words.
__device__ __forceinline__ void lds_put_bits(uint32_t* lw, int& p, int n, uint32_t v) {
  if (n <= 0) return;
  const int i = p >> 5, sh = p & 31;
  const uint64_t x = static_cast<uint64_t>(v) << (64 - n - sh);
  atomicOr(&lw[i], static_cast<uint32_t>(x >> 32));
  if (sh + n > 32) atomicOr(&lw[i + 1], static_cast<uint32_t>(x));
  p += n;
}

// ORs the n (<= 64) low bits of v, MSB first, at bit p of the LDS words:
// the (up to three) words the piece touches, each with one atomic (none for
// a word whose share of the piece is all zero bits).
__device__ __forceinline__ void lds_put_bits64(uint32_t* lw, int p, int n, uint64_t v) {
  if (n <= 0) return;
  const int i = p >> 5, sh = p & 31;
  const uint64_t x = v << (64 - n);  // the piece top-aligned
  const uint32_t w0 = static_cast<uint32_t>(x >> (32 + sh));
  const uint32_t w1 = static_cast<uint32_t>(x >> sh);
  const uint32_t w2 = sh ? static_cast<uint32_t>((x << (64 - sh)) >> 32) : 0u;
  if (w0) atomicOr(&lw[i], w0);
  if (w1) atomicOr(&lw[i + 1], w1);
  if (w2) atomicOr(&lw[i + 2], w2);
}

// Inclusive sum over the wave's lanes in lane order by DPP alone: shifts
// within the 16-lane rows, then the row totals carried by row_bcast:15 /
// row_bcast:31 (lanes without a source read 0).  Two 16-bit counts packed
// in one word sum independently while neither total reaches 2^16.
__device__ __forceinline__ uint32_t wave_incl_sum_u32(uint32_t v) {
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x111, 0xf, 0xf, false));
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x112, 0xf, 0xf, false));
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x114, 0xf, 0xf, false));
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x118, 0xf, 0xf, false));
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x142, 0xa, 0xf, false));
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x143, 0xc, 0xf, false));
  return v;
}

// ---------------------------------------------------------------------------
// k_jpeg_code: the scan in one pass -- bit lengths, their prefix, the bits
// themselves and the 0xff count -- with a decoupled look-back over
// workgroups instead of separate bits / scan / emit / count launches.
//
// Workgroup = 4 waves x 4 MCUs = 16 consecutive MCUs of [m0, m1), in
// workgroup index order.  Pass A: each wave codes its MCUs' symbols once and keeps
// them packed in registers (two words per lane and component) with the
// MCUs' bit lengths; the workgroup's total is published at once (flag 1).
// Pass B lays the bits out in LDS at workgroup-local offsets while wave 0
// looks back over the predecessors' published totals for the workgroup's
// start bit (flag 2 = an inclusive prefix, which ends the look-back).  The
// bits then go out shifted to that start: words the workgroup covers alone
// by plain stores (their 0xff bytes counted here); a last word shared with
// the next workgroup is published to it, and the first word, shared with
// the previous one, is completed here with the predecessor's published bits
// (the predecessor publishes them right after its own look-back, which
// never waits on a successor).  All cross-workgroup state moves by device-scope
// atomics (coherent across the XCDs' L2s; no device-scope fence); the
// part's totals go straight to mapped host memory (see below).  The scan
// starts at bit `base` of the stream (a strip of
// a frame split over ranks); with pad_end the last byte is padded with ones
// as the writer does before EOI.  The DC predictor of MCU m0 is block m0-1.
// ---------------------------------------------------------------------------
constexpr int kCodeMcusPerWave = 4;
constexpr int kCodeMcus = 4 * kCodeMcusPerWave;  // per workgroup
// The seam handling of k_jpeg_code (a word shared by at most two workgroups,
// completed by the second to arrive) needs every workgroup but the last to
// cover >= 32 bits.  An MCU codes >= 2 bits even in a one-component scan
// (a DC code of >= 1 bit plus an EOB or an AC code of >= 1 bit), so
// kCodeMcus MCUs give kCodeMcus * 2 bits: 8 MCUs per workgroup (16 bits)
// let three workgroups share one word, which is how kCodeMcusPerWave = 2
// changed coder bytes in round 5.
constexpr int kCodeMinBitsPerMcu = 2;
static_assert(kCodeMcus * kCodeMinBitsPerMcu >= 32,
              "k_jpeg_code: a workgroup must span >= 32 bits so that no word is shared by three");
// The workgroup's bits in LDS: any kCodeMcus MCUs of the coefficient domain
// (runtime/engine.h: kCodeMaxMcuBits = 3 x (30 + 63 x 29) = 5571 each), and
// the two words past a piece's first that lds_put_bits64 may address.
constexpr int kCodeLdsWords = (kCodeMcus * kCodeMaxMcuBits + 31) / 32 + 2;
static_assert(32 * (kCodeLdsWords - 2) >= kCodeMcus * kCodeMaxMcuBits,
              "k_jpeg_code: the LDS bit buffer holds a workgroup's worst MCUs");
// jpeg_lane_pack's fields: a magnitude length (len1) in 5 bits, a lane's
// total (n) in 7 -- its worst is three ZRLs, a code, a DC difference and the EOB.
static_assert(kCodeMaxDcSize < 32 && 3 * kCodeMaxCodeLen + kCodeMaxCodeLen + kCodeMaxDcSize + kCodeMaxCodeLen < 128,
              "k_jpeg_code: jpeg_lane_pack's len1 and n fields");
// 8 workgroups per CU (amdgpu_waves_per_eu(8, 8)) within 160 KiB of LDS:
// the bit buffer and the code / quant tables of one workgroup
static_assert(4 * kCodeLdsWords + 4 * (3 * 512 + 2 * 3 * 64 + kCodeMcus) + 64 <= 20480,
              "k_jpeg_code: 8 workgroups' LDS per CU");
constexpr uint64_t kCodeValueMask = (1ull << 48) - 1;
constexpr int kCodeHostBits = 0, kCodeHostFirst = 2, kCodeHostLast = 3, kCodeHostFf = 8;
constexpr int kJCodeHost = 6 * 256 + 4;  // the coder's words in the engine's mapped h_jhist_ (after the stage's)
constexpr int kCodeFfCopies = 32;  // 0xff counters (workgroup t adds into t % 32)

// Status word of workgroup t: flag (62..63: 1 total, 2 inclusive end bit),
// launch epoch (48..61), value (0..47).
__device__ __forceinline__ uint64_t code_status(uint32_t flag, uint32_t epoch, uint64_t v) {
  return (static_cast<uint64_t>(flag) << 62) | (static_cast<uint64_t>(epoch & 0x3fff) << 48) | v;
}

__device__ __forceinline__ void code_store(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t code_load(uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A shared word published for a neighbour: (launch epoch << 32) | word.
__device__ __forceinline__ uint64_t code_tagged(uint32_t epoch, uint32_t v) {
  return (static_cast<uint64_t>(epoch) << 32) | v;
}

__device__ __forceinline__ int count_ff_bytes(uint32_t v, int nbytes) {
  int c = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) c += (q < nbytes && ((v >> (8 * q)) & 0xff) == 0xff) ? 1 : 0;
  return c;
}

// The lane's bits of one component of an MCU from the codes in LDS, packed:
// p0 = n | nzrl << 7 | len0 << 9 | len1 << 14 | eob_len << 19, p1 = v0 | v1 << 16.
__device__ __forceinline__ void jpeg_lane_pack(const JpegLaneSym& y, uint32_t e, uint32_t zrl,
                                               uint32_t eob, uint32_t* p0, uint32_t* p1) {
  const JpegLaneBits r = jpeg_lane_bits(y, e, zrl, eob);
  *p0 = static_cast<uint32_t>(r.n) | (static_cast<uint32_t>(r.nzrl) << 7) |
        (static_cast<uint32_t>(r.len0) << 9) | (static_cast<uint32_t>(r.len1) << 14) |
        (static_cast<uint32_t>(r.eob_len) << 19);
  *p1 = (r.v0 & 0xffffu) | (r.v1 << 16);
}

// Bits of MCU b (< m1) with the codes in LDS, in the calling wave (nat:
// the lane's natural-order index): the sum of what pass A below packs for
// it.  The look-back's fallback for a predecessor that has not been
// dispatched (a pure function of the coefficients and the code table, so
// the same total the predecessor publishes itself).
__device__ __noinline__ int jpeg_mcu_bits(const int16_t* __restrict__ cur, const int* qi, const float* rq,
                                          int nat, int nb, int ncomp, const uint32_t* lcode, int b, int lane) {
  int bits = 0;
  for (int c = 0; c < ncomp; ++c) {
    const size_t tb = static_cast<size_t>(c) * nb + b;
    const int16_t zk = jpeg_quant_rcp(cur[tb * 64 + nat], qi[64 * c + lane], rq[64 * c + lane]);
    const int16_t last =
        b > 0 ? jpeg_quant_rcp(cur[(tb - 1) * 64], qi[64 * c], rq[64 * c]) : static_cast<int16_t>(0);
    const JpegLaneSym y = jpeg_lane_sym(zk, lane, __ballot(zk != 0), last);
    const uint32_t e = y.idx >= 0 ? lcode[c * 512 + y.idx] : 0u;
    uint32_t p0, p1;
    jpeg_lane_pack(y, e, lcode[c * 512 + 256 + 0xf0], lcode[c * 512 + 256], &p0, &p1);
    bits += wave_sum_i(static_cast<int>(p0 & 0x7f));
  }
  return bits;
}

// Spin budgets of the look-back before it computes a missing predecessor's
// total itself (rounds of status loads, each about a memory round trip):
// short for a workgroup that has not started (it may not be dispatched
// before this one ends: its slots can be held by any kernel on the device),
// long for one that has (it publishes its total after pass A, which waits on
// nothing; a long wait means it was preempted).
constexpr int kLookSpinUnstarted = 8;
constexpr int kLookSpinStarted = 256;

// status: per workgroup (epoch-tagged, zero at allocation); side: per
// workgroup [2t] the head half of its first word when shared with workgroup
// t - 1 (workgroup 0: the part's shared start, for the host), [2t+1] the
// tail half of its last word when shared with t + 1 (the last workgroup:
// the part's open end, for the host); seam: per workgroup t, the arrivals at
// the word shared by t - 1 and t (zero on entry, reset by the second).
// host (mapped pinned memory, read once the launch is done): [kCodeHostBits]
// total bits (u64, the last workgroup), [kCodeHostFirst] the part's first
// word when shared (workgroup 0), [kCodeHostLast] its open last word (its
// completer), [kCodeHostFf + t] workgroup t's 0xff bytes (the host sums
// them: no arrival counting, no fold launch).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_jpeg_code(
    const int16_t* __restrict__ cur, const JpegQuantF q, int nb, int m0, int m1, int ncomp,
    const JpegCodesArg codes, unsigned long long base, int pad_end,
    uint32_t* __restrict__ words, uint32_t* __restrict__ host,
    uint64_t* __restrict__ status, uint64_t* __restrict__ side, uint32_t* __restrict__ seam,
    uint32_t epoch, const uint32_t* __restrict__ dist_words, float skip_at) {
  // A candidate that cannot become the output whatever its size above the
  // host's lower bound (the distance of the Compare just before it at or
  // above skip_at, processor.cc:151-160 with ScoreJPEG monotone in both):
  // not coded, every workgroup leaves before touching any state.  skip_at =
  // +inf (the default: no test) never skips, whatever the distance -- a
  // +inf distance included; -inf always does.
  if (skip_at != __builtin_inff()) {
    // the distance: the maximum of k_diffmap's kDmMaxWords words (every wave
    // folds them itself: one load per lane)
    uint32_t u = dist_words[threadIdx.x & (kDmMaxWords - 1)];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) u = max(u, static_cast<uint32_t>(__shfl_xor(static_cast<int>(u), o, 64)));
    if (__uint_as_float(u) >= skip_at) return;
  }
  __shared__ uint32_t lcode[3 * 512];
  __shared__ int lqi[3 * 64];    // the quant values (zigzag order)
  __shared__ float lrq[3 * 64];  // and their reciprocals
  __shared__ uint32_t lw[kCodeLdsWords];
  __shared__ int mlen[kCodeMcus];
  __shared__ unsigned long long s_start;
  __shared__ int s_ff[4];
  __shared__ uint32_t s_head, s_tail;
  const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
  const int groups = (m1 - m0 + kCodeMcus - 1) / kCodeMcus;
  // The tile is blockIdx.x, whatever order the workgroups are dispatched in:
  // no workgroup ever waits without bound on another.  A successor's
  // look-back waits a bounded time for a missing total and then computes it
  // (jpeg_mcu_bits), and the word two workgroups share is completed by
  // whichever of the two gets there second (seam counters), so a workgroup
  // finishes even while its predecessors cannot be dispatched -- e.g. their
  // XCD's slots held by other kernels' workgroups (the 8-queue stall of
  // round 3: profiles/round3_queue_sweep.txt).
  const int t = static_cast<int>(blockIdx.x);
  if (tid == 0) code_store(&status[t], code_status(0, epoch, 0));  // started
  // (both read in place from the kernel arguments: indexing a by-value
  // struct directly would copy it to private memory)
  if (tid < 3 * 64) {
    const float qv = reinterpret_cast<const float*>(&q)[tid];
    lqi[tid] = static_cast<int>(qv);
    lrq[tid] = 1.0f / qv;
  }
  for (int i = tid; i < 3 * 512; i += 256) {
    // lcode[c * 512 + j]: (length << 16) | code; j < 256 DC, else AC j - 256
    const int c = i >> 9, j = i & 511;
    const bool on = j >= 256 || j < kJDcSyms;
    // (byte offset into the argument: no copy of it to private memory)
    const int off = j >= 256 ? static_cast<int>(offsetof(JpegCodesArg, ac)) + 3 * (256 * c + j - 256)
                             : 3 * (kJDcSyms * c + (on ? j : 0));
    const uint8_t* e = reinterpret_cast<const uint8_t*>(&codes) + off;
    lcode[i] = on ? (static_cast<uint32_t>(e[2]) << 16) | (static_cast<uint32_t>(e[1]) << 8) | e[0] : 0u;
  }
  __syncthreads();
  const int g0 = m0 + t * kCodeMcus;
  const int nat = c_natural_order[lane];  // the lane's zigzag position in natural order
  // ---- pass A: symbols + lengths of this wave's MCUs (packed in registers)
  uint32_t pk0[kCodeMcusPerWave][3], pk1[kCodeMcusPerWave][3];
  // every coefficient and predictor load of the wave's MCUs first, so the
  // four MCUs' memory latencies overlap
  int16_t zk[kCodeMcusPerWave][3], last[kCodeMcusPerWave][3];
#pragma unroll
  for (int j = 0; j < kCodeMcusPerWave; ++j) {
    const int b = g0 + kCodeMcusPerWave * wv + j;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t tb = static_cast<size_t>(c) * nb + (b < m1 ? b : m1 - 1);
      const bool on = c < ncomp && b < m1;
      zk[j][c] = on ? jpeg_quant_rcp(cur[tb * 64 + nat], lqi[64 * c + lane], lrq[64 * c + lane])
                    : static_cast<int16_t>(0);
      // the DC predictor: block b - 1's DC -- the previous MCU's lane 0 after
      // the wave's first MCU
      if (j == 0) {
        last[j][c] = on && b > 0 ? jpeg_quant_rcp(cur[(tb - 1) * 64], lqi[64 * c], lrq[64 * c])
                                 : static_cast<int16_t>(0);
      } else {
        last[j][c] = static_cast<int16_t>(__builtin_amdgcn_readlane(static_cast<int>(zk[j - 1][c]), 0));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kCodeMcusPerWave; ++j) {
    const int b = g0 + kCodeMcusPerWave * wv + j;
    int bits = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pk0[j][c] = 0;
      pk1[j][c] = 0;
    }
    if (b < m1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (c >= ncomp) break;
        const JpegLaneSym y = jpeg_lane_sym(zk[j][c], lane, __ballot(zk[j][c] != 0), last[j][c]);
        const uint32_t e = y.idx >= 0 ? lcode[c * 512 + y.idx] : 0u;
        jpeg_lane_pack(y, e, lcode[c * 512 + 256 + 0xf0], lcode[c * 512 + 256], &pk0[j][c], &pk1[j][c]);
      }
      // (the MCU's total: the packed scans pass B redoes for its offsets)
      const uint32_t s01 = wave_incl_sum_u32((pk0[j][0] & 0x7f) | ((pk0[j][1] & 0x7f) << 16));
      const uint32_t s2 = wave_incl_sum_u32(pk0[j][2] & 0x7f);
      const uint32_t t01 = __builtin_amdgcn_readlane(s01, 63), t2 = __builtin_amdgcn_readlane(s2, 63);
      bits = static_cast<int>((t01 & 0xffffu) + (t01 >> 16) + t2);
    }
    if (lane == 0) mlen[kCodeMcusPerWave * wv + j] = bits;
  }
  __syncthreads();
  // workgroup total; publish it (workgroup 0: its end is known already)
  int agg = 0;
#pragma unroll
  for (int i = 0; i < kCodeMcus; ++i) agg += mlen[i];
  if (tid == 0) {
    code_store(&status[t], t == 0 ? code_status(2, epoch, base + agg) : code_status(1, epoch, agg));
  }
  const int nwl = (agg + 31) / 32 + 1;
  for (int i = tid; i < nwl; i += 256) lw[i] = 0;
  __syncthreads();
  // ---- pass B: the bits at workgroup-local offsets
  {
    int loc = 0;
    for (int i = 0; i < kCodeMcusPerWave * wv; ++i) loc += mlen[i];
#pragma unroll
    for (int j = 0; j < kCodeMcusPerWave; ++j) {
      const int b = g0 + kCodeMcusPerWave * wv + j;
      if (b >= m1) break;
      // every lane's bit offset in the MCU: the packed inclusive scans of
      // the components' counts, less the lane's own, after the components
      // before it
      const uint32_t n01 = (pk0[j][0] & 0x7f) | ((pk0[j][1] & 0x7f) << 16), n2 = pk0[j][2] & 0x7f;
      const uint32_t s01 = wave_incl_sum_u32(n01), s2 = wave_incl_sum_u32(n2);
      const uint32_t t01 = __builtin_amdgcn_readlane(s01, 63), t2 = __builtin_amdgcn_readlane(s2, 63);
      const uint32_t e01 = s01 - n01, e2 = s2 - n2;  // exclusive (no borrow: each field >= its own count)
      const int start[3] = {static_cast<int>(e01 & 0xffffu),
                            static_cast<int>((t01 & 0xffffu) + (e01 >> 16)),
                            static_cast<int>((t01 & 0xffffu) + (t01 >> 16) + e2)};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (c >= ncomp) break;
        const uint32_t p0 = pk0[j][c], p1 = pk1[j][c];
        int p = loc + start[c];
        const uint32_t zrl = lcode[c * 512 + 256 + 0xf0];
        const int zl = static_cast<int>(zrl >> 16);
        const int nzrl = static_cast<int>((p0 >> 7) & 3);
        for (int z = 0; z < nzrl; ++z) lds_put_bits(lw, p, zl, zrl & 0xffffu);
        // the lane's code, magnitude and (lane 63) EOB as one piece
        const int len0 = static_cast<int>((p0 >> 9) & 31), len1 = static_cast<int>((p0 >> 14) & 31);
        const int len2 = static_cast<int>((p0 >> 19) & 31);
        const uint64_t piece = (((static_cast<uint64_t>(p1 & 0xffffu) << len1) | (p1 >> 16)) << len2) |
                               (len2 ? (lcode[c * 512 + 256] & 0xffffu) : 0u);
        lds_put_bits64(lw, p, len0 + len1 + len2, piece);
      }
      loc += static_cast<int>((t01 & 0xffffu) + (t01 >> 16) + t2);
    }
  }
  // ---- look-back (wave 0) for the workgroup's start bit
  if (wv == 0) {
    unsigned long long start = base;
    if (t > 0) {
      // Each round reads kLookRounds x 64 predecessors at once (lane l, row r:
      // distance 64 r + l from j), so a workgroup far from the nearest
      // inclusive status waits on few dependent memory round trips.
      constexpr int kLookRounds = 4;
      unsigned long long sum = 0;
      int j = t - 1;
      for (;;) {
        uint64_t s[kLookRounds];
#pragma unroll
        for (int r = 0; r < kLookRounds; ++r) {
          const int idx = j - 64 * r - lane;
          s[r] = idx >= 0 ? code_load(&status[idx]) : code_status(2, epoch, base);
        }
        int k;  // distance of the nearest inclusive predecessor (or 64 x rounds)
        int spins = 0;
        for (;;) {
          // ready up to the nearest inclusive predecessor is enough
          int ki = 64 * kLookRounds, kw = 64 * kLookRounds;
          uint64_t sw = 0;  // the status of the nearest predecessor not ready
#pragma unroll
          for (int r = kLookRounds - 1; r >= 0; --r) {
            const bool cur = ((s[r] >> 48) & 0x3fff) == (epoch & 0x3fff);
            const bool ready = (s[r] >> 62) != 0 && cur;
            const uint64_t incl = __ballot(ready && (s[r] >> 62) == 2);
            const uint64_t wait = __ballot(!ready);
            if (incl) ki = 64 * r + __builtin_ctzll(incl);
            if (wait) {
              const int l = __builtin_ctzll(wait);
              kw = 64 * r + l;
              sw = (static_cast<uint64_t>(__builtin_amdgcn_readlane(static_cast<int>(s[r] >> 32), l)) << 32) |
                   static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(s[r]), l));
            }
          }
          if (ki < kw || kw == 64 * kLookRounds) {
            k = ki;
            break;
          }
          const bool started = ((sw >> 48) & 0x3fff) == (epoch & 0x3fff);
          if (++spins > (started ? kLookSpinStarted : kLookSpinUnstarted)) {
            // fallback: the nearest missing total, computed here
            const int idx = j - kw;
            const int b0 = m0 + idx * kCodeMcus, b1 = min(b0 + kCodeMcus, m1);
            int tot = 0;
            for (int b = b0; b < b1; ++b) tot += jpeg_mcu_bits(cur, lqi, lrq, nat, nb, ncomp, lcode, b, lane);
            const uint64_t v = code_status(1, epoch, static_cast<uint64_t>(tot));
#pragma unroll
            for (int r = 0; r < kLookRounds; ++r)
              if (64 * r + lane == kw) s[r] = v;
            spins = 0;
            continue;
          }
          __builtin_amdgcn_s_sleep(1);
#pragma unroll
          for (int r = 0; r < kLookRounds; ++r) {
            const bool ready = (s[r] >> 62) != 0 && ((s[r] >> 48) & 0x3fff) == (epoch & 0x3fff);
            const int idx = j - 64 * r - lane;
            if (!ready && idx >= 0) s[r] = code_load(&status[idx]);
          }
        }
        unsigned long long v = 0;
#pragma unroll
        for (int r = 0; r < kLookRounds; ++r)
          if (64 * r + lane <= k) v += s[r] & kCodeValueMask;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        sum += v;
        if (k < 64 * kLookRounds) break;
        j -= 64 * kLookRounds;
      }
      start = sum;
      if (lane == 0) code_store(&status[t], code_status(2, epoch, start + agg));
    }
    if (lane == 0) s_start = start;
  }
  __syncthreads();
  // ---- the workgroup's words, shifted to its start bit
  const unsigned long long S = s_start, E = S + agg;
  const int sh = static_cast<int>(S & 31);
  const unsigned long long fw = S >> 5, lwd = (E - 1) >> 5;
  const int nw = static_cast<int>(lwd - fw) + 1;
  const bool last_wg = t == groups - 1;
  const bool pad = last_wg && pad_end;
  // the first word is shared with the previous workgroup (or part), the last
  // with the next one (or is the part's open end).  A workgroup other than
  // the last has kCodeMcus MCUs of >= 2 bits each (static_assert at
  // kCodeMinBitsPerMcu), so it spans two words when its start is unaligned:
  // a word is never shared by three workgroups.
  const bool head_shared = sh != 0;
  const bool tail_shared = (E & 31) != 0 && !pad;
  const int end_bytes = (E & 31) != 0 ? static_cast<int>(((E & 31) + 7) / 8) : 4;
  const unsigned long long wbase = base >> 5;  // words[0] is the stream's word base >> 5
  int ff = 0;
  for (int i = tid; i < nw; i += 256) {
    uint32_t v = lw[i] >> sh;
    if (sh && i > 0) v |= lw[i - 1] << (32 - sh);
    const bool head = i == 0 && head_shared;
    const bool tail = i == nw - 1 && (E & 31) != 0;
    int nbytes = 4;
    if (tail && pad) {
      // pad the last byte with ones; bytes past it are not in the stream
      const int used = static_cast<int>(E & 31);
      v |= (0xffffffffu >> used) & ~(end_bytes < 4 ? 0xffffffffu >> (8 * end_bytes) : 0u);
      nbytes = end_bytes;
    }
    v = __builtin_bswap32(v);
    if (head) {
      s_head = v;  // (also the tail when nw == 1)
    } else if (tail && !pad) {
      s_tail = v;
    } else {
      words[fw + i - wbase] = v;
      ff += count_ff_bytes(v, nbytes);
    }
  }
  ff = wave_sum_i(ff);
  if (lane == 0) s_ff[wv] = ff;
  __syncthreads();
  if (tid == 0) {
    int f = s_ff[0] + s_ff[1] + s_ff[2] + s_ff[3];
    // A shared word: each side stores its half, then counts its arrival at
    // the seam; the second completes the word (the halves are disjoint bit
    // ranges, so it is their OR) and resets the counter.  The half is
    // acknowledged (device scope) before the arrival is counted.
    // Head half info (bits 32..): 0..2 the word's byte count for the 0xff
    // count, bit 3: the word is also the part's open end.
    const bool one = nw == 1;
    if (head_shared) {
      if (t == 0) {
        // the part's first word, shared with the previous rank's part: the host
        host[kCodeHostFirst] = s_head;
      } else {
        const uint64_t info = (one && tail_shared) ? 8u : static_cast<uint64_t>(one ? end_bytes : 4);
        code_store(&side[2 * t], (info << 32) | s_head);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (atomicAdd(&seam[t], 1u) == 1u) {
          asm volatile("" ::: "memory");  // the other half is read after the count
          atomicExch(&seam[t], 0u);
          const uint32_t v = static_cast<uint32_t>(code_load(&side[2 * t - 1])) | s_head;
          if (info & 8u) {
            host[kCodeHostLast] = v;  // the part's open end
          } else {
            words[fw - wbase] = v;
            f += count_ff_bytes(v, static_cast<int>(info));
          }
        }
      }
    }
    if (tail_shared && !(one && head_shared)) {
      if (last_wg) {
        host[kCodeHostLast] = s_tail;  // the part's open end
      } else {
        code_store(&side[2 * t + 1], static_cast<uint64_t>(s_tail));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (atomicAdd(&seam[t + 1], 1u) == 1u) {
          asm volatile("" ::: "memory");
          atomicExch(&seam[t + 1], 0u);
          const uint64_t h = code_load(&side[2 * (t + 1)]);
          const uint32_t v = static_cast<uint32_t>(h) | s_tail;
          const uint32_t info = static_cast<uint32_t>(h >> 32);
          if (info & 8u) {
            host[kCodeHostLast] = v;  // the part's open end (the next workgroup's single word)
          } else {
            words[lwd - wbase] = v;
            f += count_ff_bytes(v, static_cast<int>(info));
          }
        }
      }
    }
    host[kCodeHostFf + t] = static_cast<uint32_t>(f);
    if (last_wg) {
      const unsigned long long total = E - base;
      host[kCodeHostBits] = static_cast<uint32_t>(total);
      host[kCodeHostBits + 1] = static_cast<uint32_t>(total >> 32);
    }
  }
}


// The back end's bulk prefix on the device copy (the first changes of an
// iteration of SelectFrequencyBackEnd, processor.cc:850-889, which the host
// takes as a set -- see Processor::SelectFrequencyBackEnd) and the change it
// makes to the AC symbol histograms.  Block b takes cnt[b] changes from
// last[b] in `direction`: candidate cand_idx[offset + i] zeroed (up) or
// restored to Quantize(orig, quant) (down), i = last[b], last[b] + direction,
// ... -- the host loop's writes.  A block's candidates are distinct
// coefficients (at most 3 x 63), so its changes are applied at once.  A
// wave takes one block at a time, lane = zigzag position: each changed
// component's AC symbols before and after (UpdateACHistogramForBlock,
// jpeg_data_writer.cc) go into the workgroup's LDS histogram with weights
// -1 / +1 -- the same delta as the host's per-change updates -- and meet
// as k_jpeg_stage's counts do; the last workgroup hands the deltas (u32
// wrapping = i32) to the host through host_out.  Replaces a full histogram
// pass over the changed image.
constexpr int kBulkThreads = 1024;
constexpr int kBulkWaves = kBulkThreads / 64;

// The AC symbols of one block (lane = zigzag position, z its quantized
// value) added into h with weight w.
__device__ __forceinline__ void bulk_symbols(int16_t z, int lane, uint32_t* h, uint32_t w) {
  const uint64_t m = __ballot(z != 0) & ~1ull;
  if (lane > 0 && z != 0) {
    const uint64_t below = m & ((1ull << lane) - 1);
    const int prev = below ? 63 - __clzll(below) : 0;
    const int run = lane - prev - 1;
    if (run > 15) atomicAdd(&h[0xf0], w * static_cast<uint32_t>(run >> 4));
    const int a = z < 0 ? -z : z;
    atomicAdd(&h[((run & 15) << 4) + log2_floor_nz(a) + 1], w);
  }
  if (lane == 63 && !(m >> 63)) atomicAdd(&h[0], w);  // EOB: coefficient 63 is zero
}

__global__ __launch_bounds__(kBulkThreads) void k_bulk_apply(
    const uint8_t* __restrict__ cnt, const int* __restrict__ last, const int* __restrict__ off, int cand_n,
    const uint8_t* __restrict__ cand_idx, int nb, int direction, const int16_t* __restrict__ orig,
    const QuantMatrix qm, const JpegQuantF q, int16_t* __restrict__ cur, uint32_t* __restrict__ hist,
    const uint32_t* __restrict__ sel, const uint8_t* __restrict__ last8, uint8_t* __restrict__ cnt_host) {
  // last8 (non-null): the last indexes as the host's bytes (mapped memory;
  // a frame split over ranks, whose back end has no device order), else
  // `last` (the device order's copy).
  // sel (the device selection of the prefix, order_kernels.inc): nothing to
  // apply when it left the prefix open (the host takes the exact path);
  // cnt (its counts) includes the tie block's share of the K*-keyed
  // entries.  cnt_host (non-null): the counts handed to the host (mapped).
  if (sel && reinterpret_cast<const SelState*>(sel + SelLayout::state)->open) return;
  __shared__ uint32_t lh[3 * 256];
  __shared__ float lq[3 * 64];  // zigzag order
  __shared__ int lqm[3 * 64];   // natural order
  __shared__ uint8_t lchg[kBulkWaves][3 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
  for (int i = tid; i < 3 * 256; i += kBulkThreads) lh[i] = 0;
  // (read in place from the kernel arguments: indexing a by-value struct
  // directly would copy it to private memory)
  if (tid < 3 * 64) {
    lq[tid] = reinterpret_cast<const float*>(&q)[tid];
    lqm[tid] = reinterpret_cast<const int*>(&qm)[tid];
  }
  __syncthreads();
  const int nat = c_natural_order[lane];
  uint8_t* chg = lchg[wv];
  const int back = direction < 0 ? -1 : 0;
  // The wave's blocks b_j = w + j * nw (j < 64): lane j loads b_j's count
  // (mapped host memory: one round trip for all of them), offset and
  // last index; then the blocks with changes, one after another, each with
  // its candidate and coefficient loads issued together.
  const int nw = static_cast<int>(gridDim.x) * kBulkWaves;
  const int w = static_cast<int>(blockIdx.x) * kBulkWaves + wv;
  for (int b0 = w; b0 < nb; b0 += 64 * nw) {
    const int bl = b0 + lane * nw;
    const int my_n = bl < nb ? cnt[bl] : 0;
    if (cnt_host && bl < nb) cnt_host[bl] = static_cast<uint8_t>(my_n);
    const int my_off = my_n ? max(0, min(off[bl], cand_n - 1)) : 0;
    const int my_li = my_n ? (last8 ? static_cast<int>(last8[bl]) : last[bl]) : 0;
    uint64_t todo = __ballot(my_n != 0);
    while (todo) {
      const int j = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int b = b0 + j * nw;
      const int n = __builtin_amdgcn_readlane(my_n, j);
      const int first = __builtin_amdgcn_readlane(my_off, j) + __builtin_amdgcn_readlane(my_li, j) + back;
      int16_t v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = cur[(static_cast<size_t>(c) * nb + b) * 64 + nat];
      int ci[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) ci[r] = lane + 64 * r < n ? cand_idx[first + (lane + 64 * r) * direction] : -1;
      chg[lane] = 0;
      chg[64 + lane] = 0;
      chg[128 + lane] = 0;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (this wave's LDS only)
#pragma unroll
      for (int r = 0; r < 3; ++r)
        if (ci[r] >= 0) chg[ci[r]] = 1;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const bool ch = chg[64 * c + nat] != 0;
        if (!__ballot(ch)) continue;
        const size_t e = (static_cast<size_t>(c) * nb + b) * 64 + nat;
        int16_t nv = v[c];
        if (ch) {
          nv = direction > 0 ? static_cast<int16_t>(0) : quantize_coeff(orig[e], lqm[64 * c + nat]);
          cur[e] = nv;
        }
        const float qq = lq[64 * c + lane];
        const int16_t z0 = jpeg_quant(v[c], qq), z1 = jpeg_quant(nv, qq);
        if (!__ballot(z0 != z1)) continue;
        bulk_symbols(z0, lane, &lh[256 * c], ~0u);
        bulk_symbols(z1, lane, &lh[256 * c], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t* hcopy = hist + (blockIdx.x % kJHistCopies) * (6 * 256);
  for (int i = tid; i < 3 * 256; i += kBulkThreads) {
    const uint32_t v = lh[i];
    if (v) atomicAdd(&hcopy[(2 * (i >> 8) + 1) * 256 + (i & 255)], v);
  }
}

}  // namespace gz
