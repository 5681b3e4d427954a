// Internal to the host search (processor.cc, backend.cc): class Processor
// and the change-loop helpers its 4:4:4 and 4:2:0 back ends share.  Not
// installed, not part of include/guetzli_hip.h.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "host/host_util.h"
#include "host/jpeg_encode.h"
#include "host/jpeg_writer.h"
#include "host/processor.h"
#include "host/strips.h"

namespace gz {

struct QuantData {
  int q[3][kDCTBlockSize];
  size_t jpg_size;
  bool dist_ok;
};

// host/backend.cc
size_t ComputeEntropyCodes(const std::vector<JpegHistogram>& histograms, std::vector<uint8_t>* depths);
size_t EntropyCodedDataSize(const std::vector<JpegHistogram>& histograms,
                            const std::vector<uint8_t>& depths);

// The change loop's control for one back-end iteration (processor.cc:
// 836-905), shared by the 4:4:4 and the 4:2:0 back ends: the thresholds
// from the iteration's order, the decades whose entropy codes are read, when
// the size estimate is read and the break test.  The estimate is only read
// once changed > min_coeffs (and at the last step), and a decade's codes
// only if such a step reads them, so the codes of other decades are never
// built -- the same values wherever they are read.
struct ChangeLoop {
  size_t n_order;
  int min_coeffs;  // min_coeffs_to_change
  double min_size_delta;
  int changed = 0;
  float val_threshold = 0.0f;
  // factor: the searched blocks' size in 8x8 blocks (4:2:0 chroma: 2);
  // *first_up_iter: the first up iteration's floor on min_coeffs (the count
  // of keys below 0.75 x the block error limit), then cleared.
  // (n_total / below: the frame's entry count and count below the floor
  // when `order` holds only this rank's entries; else taken from order)
  ChangeLoop(int direction, bool distance_ok, int base_size, int factor, int blocks_to_change,
             bool* first_up_iter, float block_error_limit,
             const std::vector<std::pair<int, float>>& order, size_t n_total = SIZE_MAX,
             int64_t below_floor = -1)
      : n_order(n_total == SIZE_MAX ? order.size() : n_total) {
    double rel_size_delta = direction > 0 ? 0.01 : 0.0005;
    if (direction > 0 && distance_ok) rel_size_delta = 0.05;
    min_size_delta = base_size * rel_size_delta;
    const float per_block = direction > 0 ? 2.0f : factor * factor * 0.2f;
    min_coeffs = static_cast<int>(per_block * blocks_to_change);
    if (*first_up_iter) {
      const float limit = 0.75f * block_error_limit;
      // partition_point(key < limit) of the sorted order == count of keys below limit
      int below = static_cast<int>(below_floor);
      if (below_floor < 0) {
        below = 0;
        for (const auto& e : order) below += e.second < limit ? 1 : 0;
      }
      min_coeffs = std::max<int>(min_coeffs, below);
      *first_up_iter = false;
    }
  }
  void Applied(float key) {
    val_threshold = key;
    ++changed;
  }
  // after change i: its decade's codes are read (rebuild them), the estimate is read
  bool CodesRead(size_t i) const {
    return i % 10 == 0 && (i + 9 >= static_cast<size_t>(std::max(0, min_coeffs)) || i + 10 >= n_order);
  }
  bool EstimateRead(size_t i) const { return changed > min_coeffs || i + 1 == n_order; }
  bool Stop(int est, int prev) const { return changed > min_coeffs && std::abs(est - prev) > min_size_delta; }
};

// The AC histogram update of one coefficient change in the search loop
// (UpdateACHistogram(-1, block) / change / UpdateACHistogram(+1, block),
// processor.cc:491-515 and :869-874) done locally: in zigzag order a block's
// AC symbols are, per non-zero coefficient, the ZRLs and run/size symbol of
// the zero run before it, then EOB if zeros trail.  Changing the
// coefficient at zigzag position z only re-forms the symbols of the segment
// from the previous non-zero p to the next non-zero nx, so only those are
// removed and re-added (same counts as the full rescans).  raw_bits tracks
// sum_i (counts[i]/2) * (depth[i] + (i & 0xf)) -- HistogramEntropyCost
// before rounding -- for the current depths.
struct AcBlockModel {
  std::vector<uint64_t> nz;  // [c * blocks + b]: bit z set <=> zigzag coefficient z non-zero
  float inv_q[3][kDCTBlockSize];  // 1 / quant (natural order), for Size

  void Build(const CoeffImage& img) {
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < kDCTBlockSize; ++k) inv_q[c][k] = 1.0f / static_cast<float>(img.quant[c][k]);
    nz.assign(static_cast<size_t>(3) * img.blocks, 0);
    for (int c = 0; c < 3; ++c)
      for (int b = 0; b < img.blocks; ++b) {
        const coeff_t* blk = img.block(c, b);
        uint64_t m = 0;
        for (int z = 0; z < 64; ++z) m |= static_cast<uint64_t>(blk[kJPEGNaturalOrder[z]] != 0) << z;
        nz[static_cast<size_t>(c) * img.blocks + b] = m;
      }
  }

  static int Size(coeff_t v, int q) { return Log2FloorNonZero(std::abs(v / q)) + 1; }
  // Size(v, q) without the integer division: |v| / q rounded through the
  // float reciprocal is within one of the quotient (|v| < 2^16, relative
  // error < 2^-22), and one multiply-compare settles it on the truncated one.
  static int SizeInv(coeff_t v, int q, float inv) {
    const int a = std::abs(static_cast<int>(v));
    int n = static_cast<int>(static_cast<float>(a) * inv + 0.5f);
    if (n * q > a) --n;
    return Log2FloorNonZero(static_cast<uint32_t>(n)) + 1;
  }

  // weight * symbols of the segment after non-zero position p (0 = none /
  // DC) through the non-zeros `mid` (0: none) and `nx` (0: none; then EOB
  // if the last one is below 63).
  // H: the histogram (JpegHistogram) or a recorder of the same Add calls.
  // kRaw = false: the histogram only (the bulk prefix, whose raw bits are
  // recomputed from the summed histograms)
  template <class H, bool kRaw = true>
  static void Segment(int weight, int p, int mid, int mid_size, int nx, int nx_size,
                      const uint8_t* depth, H* h, int64_t* raw) {
    int last = p;
    int64_t bits = 0;
    auto put = [&](int pos, int size) {
      int run = pos - last - 1;
      while (run > 15) {
        h->Add(0xf0, weight);
        if (kRaw) bits += depth[0xf0];
        run -= 16;
      }
      const int sym = (run << 4) + size;
      h->Add(sym, weight);
      if (kRaw) bits += depth[sym] + (sym & 0xf);
      last = pos;
    };
    if (mid) put(mid, mid_size);
    if (nx) {
      put(nx, nx_size);
    } else if (last < 63) {
      h->Add(0, weight);
      if (kRaw) bits += depth[0];
    }
    if (kRaw) *raw += weight * bits;
  }

  // The 4:2:0 image's blocks (Y, then Cb, Cr at factor 2): slot base[c] + b.
  void Build(const Image420& img, size_t base[3]) {
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < kDCTBlockSize; ++k) inv_q[c][k] = 1.0f / static_cast<float>(img.quant[c][k]);
    base[0] = 0;
    base[1] = static_cast<size_t>(img.Blocks(0));
    base[2] = base[1] + static_cast<size_t>(img.Blocks(1));
    nz.assign(base[2] + static_cast<size_t>(img.Blocks(2)), 0);
    for (int c = 0; c < 3; ++c)
      for (int b = 0; b < img.Blocks(c); ++b) {
        const coeff_t* blk = img.block(c, b);
        uint64_t m = 0;
        for (int z = 0; z < 64; ++z) m |= static_cast<uint64_t>(blk[kJPEGNaturalOrder[z]] != 0) << z;
        nz[base[c] + b] = m;
      }
  }

  // block[k] := newval with the histogram / raw-bit bookkeeping.
  template <class H, bool kRaw = true>
  void Change(int c, int bix, int blocks, coeff_t* block, int k, coeff_t newval, const int* q,
              const uint8_t* depth, H* h, int64_t* raw) {
    ChangeAt<H, kRaw>(static_cast<size_t>(c) * blocks + bix, c, block, k, newval, q, depth, h, raw);
  }
  template <class H, bool kRaw = true>
  void ChangeAt(size_t slot, int c, coeff_t* block, int k, coeff_t newval, const int* q, const uint8_t* depth,
                H* h, int64_t* raw) {
    const coeff_t old = block[k];
    block[k] = newval;
    const int z = kJPEGZigZagOrder[k];
    if (z == 0 || old == newval) return;  // DC is not an AC symbol
    uint64_t& m = nz[slot];
    const uint64_t below = m & ((1ull << z) - 1) & ~1ull;
    const uint64_t above = z < 63 ? m & ~((2ull << z) - 1) : 0;
    const int p = below ? 63 - __builtin_clzll(below) : 0;
    const int nx = above ? __builtin_ctzll(above) : 0;
    const int knx = kJPEGNaturalOrder[nx];
    const int nx_size = nx ? SizeInv(block[knx], q[knx], inv_q[c][knx]) : 0;
    Segment<H, kRaw>(-1, p, old ? z : 0, old ? SizeInv(old, q[k], inv_q[c][k]) : 0, nx, nx_size, depth, h,
                     raw);
    Segment<H, kRaw>(1, p, newval ? z : 0, newval ? SizeInv(newval, q[k], inv_q[c][k]) : 0, nx, nx_size, depth,
                     h, raw);
    if (newval) m |= 1ull << z; else m &= ~(1ull << z);
  }
};

// The symbol updates of one change, as the partitioned back end publishes
// them (the AcBlockModel::Change calls recorded instead of applied).
struct SymbolLog {
  uint8_t n = 0;
  uint8_t sym[32];
  int8_t weight[32];
  void Add(int s, int w) {
    sym[n] = static_cast<uint8_t>(s);
    weight[n] = static_cast<int8_t>(w);
    ++n;
  }
};

class BackEnd;  // host/backend.cc

class Processor {
 public:
  Processor(const ProcessParams& p, Comparator* cmp, ProcessResult* res, Partition* part)
      : params_(p), cmp_(cmp), res_(res), part_(part), scratch_(NewScanScratch(), FreeScanScratch) {}
  ~Processor() {
    if (writer_.joinable()) writer_.join();
  }
  int Run(const JpegData& jpg_in, std::string* err);

 private:
  friend class BackEnd;  // SelectFrequencyBackEnd's steps
  bool Fail(std::string* err) {
    if (err) *err = internal_err_.empty() ? cmp_->error() : internal_err_;
    return false;
  }
  // an inconsistency found by the loop itself, not by the comparator
  std::string internal_err_;
  void OutputJpeg(const JpegData& jpg, std::string* out) {
    const auto t0 = Clock::now();
    out->clear();
    WriteJpeg(jpg, params_.clear_metadata, out);
    const double dt = Since(t0);
    res_->seconds_write += dt;
    res_->detail["write_jpeg_s"] += dt;
  }
  // Output of a search candidate: SaveToJpegData(img) over jpg + OutputJpeg
  // + MaybeOutput, pipelined.  BeginOutput stages img (quantize + count, on
  // the pool) and encodes it on a helper thread while the caller runs the
  // Compare and, in the back end, the next iteration's selection.  The
  // MaybeOutput of a candidate must see the distance of the Compare that
  // followed it, so it is applied by FlushOutput, which runs before the next
  // Compare (at the next BeginOutput) or explicitly.
  bool BeginOutput(const JpegData& jpg, const CoeffImage& img, std::string* err) {
    FlushOutput();
    const auto t0 = Clock::now();
    pending_.clear();
    if (cmp_->HasDeviceWriter()) {
      // entropy coded on the device from its resident copy (sub-ms), no
      // helper thread needed; the bytes stay there unless kept
      if (!cmp_->DeviceEncode(img, jpg, params_.clear_metadata, &pending_size_)) return Fail(err);
      has_pending_ = true;
      pending_device_ = true;
      const double dt = Since(t0);
      res_->seconds_write += dt;
      res_->detail["write_device_s"] += dt;
      return true;
    }
    pending_device_ = false;
    StageCoeffImage(img, jpg, scratch_.get());
    writer_ = std::thread([this] {
      const auto t = Clock::now();
      EncodeStaged(scratch_.get(), params_.clear_metadata, &pending_);
      encode_s_ = Since(t);
    });
    has_pending_ = true;
    const double dt = Since(t0);
    res_->seconds_write += dt;
    res_->detail["write_stage_s"] += dt;
    return true;
  }
  // BeginOutput(img) followed by the Compare of img; with a device writer
  // both run as one overlapped device call (the candidate's size and its
  // distance come back together).
  bool EncodeAndCompare(const JpegData& jpg, const CoeffImage& img, std::string* err) {
    if (!cmp_->HasDeviceWriter()) {
      if (!BeginOutput(jpg, img, err)) return false;
      return cmp_->Compare(img) || Fail(err);
    }
    FlushOutput();
    const auto t0 = Clock::now();
    size_t size = 0;
    if (!cmp_->DeviceEncodeAndCompare(img, jpg, params_.clear_metadata, &size)) return Fail(err);
    pending_.clear();
    pending_size_ = size;
    has_pending_ = true;
    pending_device_ = true;
    res_->detail["encode_compare_s"] += Since(t0);
    return true;
  }
  // EncodeAndCompare of a back-end candidate with its histograms known: the
  // DC ones of the back end's start (DC coefficients do not change) and the
  // tracked AC ones; the components SaveToJpegData keeps -- one when the
  // chroma has become all zero (no chroma DC symbol but category 0, no
  // chroma AC symbol with a magnitude) -- as the histogram pass would count.
  bool EncodeAndCompareKnown(const JpegData& jpg, const CoeffImage& img, int saved0, const JpegHistogram dc0[3],
                             const std::vector<JpegHistogram>& ac, std::string* err) {
    FlushOutput();
    const auto t0 = Clock::now();
    int ncomp = 1;
    if (saved0 > 1) {
      for (int c = 1; c < 3 && c < static_cast<int>(ac.size()) && ncomp == 1; ++c) {
        for (int i = 1; i < 256 && ncomp == 1; ++i)
          if (dc0[c].counts[i] || ((i & 0xf) && ac[c].counts[i])) ncomp = 3;
      }
    }
    JpegHistogram ach[3];
    for (int c = 0; c < ncomp && c < static_cast<int>(ac.size()); ++c) ach[c] = ac[c];
    size_t size = 0;
    bool skipped = false;
    // (FlushOutput above: final_score_ includes every earlier candidate)
    if (!cmp_->DeviceEncodeAndCompareKnown(img, jpg, params_.clear_metadata, dc0, ach, ncomp, final_score_, &size,
                                           &skipped))
      return Fail(err);
    pending_.clear();
    pending_size_ = size;
    has_pending_ = true;
    pending_device_ = true;
    pending_skipped_ = skipped;
    res_->detail["encode_compare_s"] += Since(t0);
    res_->detail["encode_known_histograms"] += 1;
    if (skipped) res_->detail["scans_skipped"] += 1;
    return true;
  }
  // Joins the pending encode and applies its MaybeOutput; returns its size.
  size_t FlushOutput() {
    if (!has_pending_) return 0;
    if (writer_.joinable()) {
      const auto t0 = Clock::now();
      writer_.join();
      const double dt = Since(t0);
      res_->seconds_write += dt;
      res_->detail["write_wait_s"] += dt;
      res_->detail["write_encode_s"] += encode_s_;
    }
    has_pending_ = false;
    if (pending_skipped_) {  // its score is not below final_score_: MaybeOutput keeps nothing
      pending_skipped_ = false;
      return 0;
    }
    if (pending_device_) {
      MaybeOutputDevice(pending_size_);
      return pending_size_;
    }
    MaybeOutput(pending_);
    return pending_.size();
  }
  // processor.cc:899-904 (the score depends on the size alone)
  void MaybeOutput(const std::string& encoded) {
    const double score = cmp_->ScoreOutputSize(static_cast<int>(encoded.size()));
    if (score < final_score_ || final_score_ < 0) {
      res_->jpeg = encoded;
      final_score_ = score;
      best_size_ = encoded.size();
      kept_on_device_ = false;
    }
  }
  void MaybeOutputDevice(size_t size) {
    const double score = cmp_->ScoreOutputSize(static_cast<int>(size));
    if (score < final_score_ || final_score_ < 0) {
      cmp_->DeviceKeepEncoded();
      final_score_ = score;
      best_size_ = size;
      kept_on_device_ = true;
    }
  }
  bool TryQuantMatrix(const JpegData& jpg_in, float target_mul, const int q[3][kDCTBlockSize],
                      CoeffImage* img, QuantData* data, std::string* err);
  bool SelectQuantMatrix(const JpegData& jpg_in, bool downsample, int best_q[3][kDCTBlockSize],
                         CoeffImage* img, bool* ok, std::string* err);
  bool SelectFrequencyMasking(const JpegData& jpg, CoeffImage* img, int comp_mask,
                              double target_mul, bool stop_early, std::string* err);
  bool SelectFrequencyBackEnd(const JpegData& jpg, CoeffImage* img, int comp_mask,
                              double target_mul, bool stop_early,
                              const std::vector<int>& offsets, const std::vector<uint8_t>& coeffs,
                              const std::vector<float>& errors, std::string* err);
  bool GatherEntries(std::vector<std::pair<int, float>>* entries, int own_lo, int own_hi, int gbase,
                     int* blocks_to_change);
  // The change entries of one back-end iteration (processor.cc:776-834), for
  // both back ends: the block weights at rblock = 1..4 until some block has
  // entries, every (owned) block's entries in block order -- built in
  // parallel over chunks of blocks -- and on a partitioned frame the frame's
  // entries from every rank.  factor: the searched blocks' size in 8x8
  // blocks; bmax: their distance maxima.  False: a failed exchange.
  bool BuildChangeOrder(int direction, int factor, double target_mul, int num_blocks, int own_lo,
                        int own_hi, int gbase, const std::vector<float>& bmax,
                        const std::vector<int>& last_indexes, const std::vector<int>& offsets,
                        const std::vector<float>& cand_err, const std::vector<float>& max_block_error,
                        std::vector<std::pair<int, float>>* order, std::vector<float>* block_weight,
                        int* blocks_to_change, size_t* frame_entries = nullptr);
  // The 4:2:0 pass (processor.cc:989-1016, downsample = 1) on the host model
  // Image420, entropy coded on the host.
  int Run420(const JpegData& jpg_in, std::string* err);
  bool TryQuantMatrix420(const JpegData& jpg, float target_mul, const int q[3][kDCTBlockSize],
                         Image420* img, QuantData* data, std::string* err);
  bool SelectFrequencyMasking420(const JpegData& jpg, Image420* img, int comp_mask,
                                 double target_mul, bool stop_early, std::string* err);
  void BeginOutput420(const JpegData& jpg, Image420* img);

  ProcessParams params_;
  Comparator* cmp_;
  ProcessResult* res_;
  Partition* part_;  // nullptr: the whole frame is this process's
  std::unique_ptr<ScanScratch, void (*)(ScanScratch*)> scratch_;
  std::thread writer_;
  std::string pending_;
  bool has_pending_ = false;
  bool pending_device_ = false;
  bool pending_skipped_ = false;  // a back-end candidate that could not win, not coded
  size_t pending_size_ = 0;
  bool kept_on_device_ = false;  // the best candidate so far is the device's kept slot
  size_t best_size_ = 0;
  double encode_s_ = 0.0;
  double final_score_ = -1;
  std::vector<int> bulk_cnt_;  // per-block change counts of a back-end bulk prefix
  size_t tail_len_[2] = {0, 0};  // the last back-end tail's length per direction (up, down)
  static constexpr int kOrderChunk = 1024;     // blocks per parallel back-end work item
  static constexpr size_t kMinBulkChanges = 64;
};

}  // namespace gz
