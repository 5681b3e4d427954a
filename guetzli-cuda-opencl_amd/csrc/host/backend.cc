// Portions restate Guetzli (Copyright 2016 Google Inc., Apache License 2.0,
// http://www.apache.org/licenses/LICENSE-2.0) as modified in
// yyamamoto79/guetzli-cuda-opencl: processor.cc, quality.cc, score.cc and butteraugli_comparator.cc
// (QuantMatrixGenerator, the back end's control flow, kLocalMaxWeight).
// Byte-exact output forces their operation order and constants; the
// code around them is this repository's own.
// The change-order back end of the 4:4:4 search (guetzli/processor.cc:
// 723-919): the entropy-size model, the order of a frame split over ranks
// (StripOrder) and the back end itself, on one engine and on row strips.
#include "host/processor_impl.h"

#include <limits>
#include <optional>

#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "guetzli_hip.h"
#include "host/lazy_sort.h"
#include "host/thread_pool.h"

namespace gz {

size_t ComputeEntropyCodes(const std::vector<JpegHistogram>& histograms, std::vector<uint8_t>* depths) {
  // processor.cc:517-536
  std::vector<JpegHistogram> clustered = histograms;
  size_t num = histograms.size();
  std::vector<int> indexes(num);
  std::vector<uint8_t> cdepths(num * JpegHistogram::kSize);
  ClusterHistograms(clustered.data(), &num, indexes.data(), cdepths.data());
  depths->resize(cdepths.size());
  for (size_t i = 0; i < histograms.size(); ++i)
    std::memcpy(&(*depths)[i * JpegHistogram::kSize], &cdepths[indexes[i] * JpegHistogram::kSize],
                JpegHistogram::kSize);
  size_t size = 0;
  for (size_t i = 0; i < num; ++i) size += HistogramHeaderCost(clustered[i]) / 8;
  return size;
}

namespace {

int64_t HistogramRawBits(const JpegHistogram& h, const uint8_t* depth) {
  int64_t bits = 0;
  for (int i = 0; i + 1 < JpegHistogram::kSize; ++i)
    bits += static_cast<int64_t>(h.counts[i] / 2) * (depth[i] + (i & 0xf));
  return bits;
}

// EntropyCodedDataSize from the per-histogram raw bit sums
// (HistogramEntropyCost's rounding applied per histogram).
int EntropySizeFromRaw(const std::vector<int64_t>& raw) {
  int64_t bits = 0;
  for (int64_t b : raw) bits += b + ((b * 3 + 512) >> 10);
  return static_cast<int>((bits + 7) / 8);
}

}  // namespace

size_t EntropyCodedDataSize(const std::vector<JpegHistogram>& histograms,
                            const std::vector<uint8_t>& depths) {
  size_t bits = 0;
  for (size_t i = 0; i < histograms.size(); ++i)
    bits += HistogramEntropyCost(histograms[i], &depths[i * JpegHistogram::kSize]);
  return (bits + 7) / 8;
}

namespace {

// The order of one back-end iteration's change entries on a frame split
// over ranks (host/strips.h), from every rank's own entries.  std::sort
// (processor.cc:840-843) is not stable, so where keys are equal its order
// is that of libstdc++'s introsort over the frame's array -- the exact path
// (LazyStdSort on every rank, after an all-gather of every entry).  But the
// loop consumes a prefix as a set and then a short tail in order, and those
// are functions of the keys alone wherever no key is shared by entries of
// two blocks (entries of one block are interchangeable: a change takes the
// block's next candidate, whichever entry named it).  So:
//   * Prefix: the bulk-th smallest key K* by a radix selection over every
//     rank's keys (three small all-sums of bucket counts); the prefix is
//     every key below K* plus the K*-keyed entries it reaches -- all of them,
//     or some of one block's; K* shared by several blocks across the
//     boundary leaves the set open (the caller takes the exact path);
//   * Next: the tail in windows, each rank's next entries (smallest first)
//     merged on every rank; a position is certified when no rank can still
//     hold a smaller key, and a tie of several blocks among the certified
//     entries ends the window there (open: the caller takes the exact path
//     from that position on -- the positions before it are the same in
//     std::sort's order).
// No rank gathers or sorts the frame's entries unless a tie leaves the
// order open.
class StripOrder {
 public:
  // Order-preserving bits of a float key (equal keys -- both zeros -- give
  // equal bits).
  static uint32_t Bits(float k) {
    if (k == 0.0f) return 0x80000000u;
    uint32_t u;
    std::memcpy(&u, &k, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }

  // cnt (num_blocks, local indices) := per owned block its entries among the
  // first `bulk` of the frame's order.  1: done; 0: open; -1: failed exchange.
  int Prefix(const std::vector<std::pair<int, float>>& local, size_t bulk, Partition* part, int gbase,
             int num_blocks, std::vector<int>* cnt) {
    // radix selection of the key of rank bulk - 1: 12 + 12 + 8 bits
    static const int kShift[3] = {20, 8, 0}, kBits[3] = {12, 12, 8};
    uint32_t prefix = 0;
    int64_t below = 0, eq = 0;
    const int64_t target = static_cast<int64_t>(bulk) - 1;
    for (int round = 0; round < 3; ++round) {
      const int sh = kShift[round], nb = kBits[round];
      std::vector<int64_t> h(static_cast<size_t>(1) << nb, 0);
      const int hi_sh = sh + nb;
      for (const auto& e : local) {
        const uint32_t u = Bits(e.second);
        if (hi_sh < 32 && (u >> hi_sh) != prefix) continue;
        ++h[(u >> sh) & ((1u << nb) - 1)];
      }
      if (!part->SumAll(h.data(), static_cast<int>(h.size()))) return -1;
      int64_t cum = below;
      uint32_t j = 0;
      for (; j + 1 < h.size() && cum + h[j] <= target; ++j) cum += h[j];
      below = cum;
      eq = h[j];
      prefix = (prefix << nb) | j;
    }
    kbits_ = prefix;
    tie_block_ = -1;
    take_ = 0;
    if (TestOpen() == 1) return 0;
    if (below + eq > static_cast<int64_t>(bulk)) {
      // K* straddles the boundary: determined only if one block holds every
      // entry keyed K* (local entries are in block order)
      std::vector<uint8_t> mine;
      int last = -1;
      for (const auto& e : local)
        if (Bits(e.second) == kbits_ && e.first != last) {
          last = e.first;
          mine.insert(mine.end(), reinterpret_cast<const uint8_t*>(&last),
                      reinterpret_cast<const uint8_t*>(&last) + 4);
        }
      std::vector<std::vector<uint8_t>> all;
      if (!part->coll->AllGatherV(mine, &all)) return -1;
      size_t blocks = 0;
      for (const auto& m : all) {
        blocks += m.size() / 4;
        if (m.size() >= 4) std::memcpy(&tie_block_, m.data(), 4);
      }
      if (blocks != 1) return 0;
      take_ = static_cast<int64_t>(bulk) - below;
    }
    cnt->assign(num_blocks, 0);
    for (const auto& e : local) {
      const uint32_t u = Bits(e.second);
      if (u < kbits_ || (u == kbits_ && tie_block_ < 0)) ++(*cnt)[e.first - gbase];
    }
    if (tie_block_ >= 0 && tie_block_ - gbase >= 0 && tie_block_ - gbase < num_blocks) {
      // (only the owner has entries of it; a halo block is never searched here)
      bool owner = false;
      for (const auto& e : local) owner = owner || e.first == tie_block_;
      if (owner) (*cnt)[tie_block_ - gbase] += static_cast<int>(take_);
    }
    have_prefix_ = true;
    return 1;
  }

  // This rank's entries after the prefix (all, without one), for Next.
  void StartTail(const std::vector<std::pair<int, float>>& local, bool after_prefix) {
    rem_.clear();
    int64_t skip = take_;
    for (const auto& e : local) {
      const uint32_t u = Bits(e.second);
      if (after_prefix) {
        if (u < kbits_) continue;
        if (u == kbits_) {
          if (tie_block_ < 0) continue;   // all K*-keyed entries are in the prefix
          if (skip > 0) {                 // the prefix's share of tie_block_'s
            --skip;
            continue;
          }
        }
      }
      rem_.push_back(Entry{u, e.first, e.second});
    }
    pos_ = 0;
    sorted_ = 0;
    static const size_t kFirst = static_cast<size_t>(EnvInt("GZ_STRIP_WINDOW", 1024));  // (tests: small windows)
    window_ = kFirst;
  }

  // The next certified positions of the frame's order.  *open: the position
  // after them starts a tie of several blocks.  1: ok; 0: every rank's
  // entries are consumed; -1: failed exchange.
  int Next(Partition* part, std::vector<int>* blocks, std::vector<float>* keys, bool* open) {
    *open = false;
    for (;;) {
      const size_t k = std::min(window_, rem_.size() - pos_);
      if (pos_ + k > sorted_) {
        // the smallest entries left, sorted, a good way ahead of the window
        const size_t want = std::min(rem_.size(), pos_ + std::max<size_t>(4 * k, 1 << 16));
        auto less = [](const Entry& a, const Entry& b) {
          return a.bits != b.bits ? a.bits < b.bits : a.block < b.block;
        };
        if (want < rem_.size()) std::nth_element(rem_.begin() + pos_, rem_.begin() + want, rem_.end(), less);
        std::sort(rem_.begin() + pos_, rem_.begin() + want, less);
        sorted_ = want;
      }
      std::vector<uint8_t> send(1 + 12 * k);
      send[0] = pos_ + k < rem_.size() ? 1 : 0;
      for (size_t i = 0; i < k; ++i) {
        const Entry& e = rem_[pos_ + i];
        std::memcpy(&send[1 + 12 * i], &e.bits, 4);
        std::memcpy(&send[5 + 12 * i], &e.block, 4);
        std::memcpy(&send[9 + 12 * i], &e.key, 4);
      }
      std::vector<std::vector<uint8_t>> all;
      if (!part->coll->AllGatherV(send, &all)) return -1;
      uint64_t bound = uint64_t{1} << 32;
      size_t sent = 0;
      for (const auto& m : all) {
        if (m.empty() || (m.size() - 1) % 12) return -1;
        const size_t n = (m.size() - 1) / 12;
        sent += n;
        if (m[0] && n) {
          uint32_t b;
          std::memcpy(&b, &m[1 + 12 * (n - 1)], 4);
          bound = std::min<uint64_t>(bound, b);
        }
      }
      if (sent == 0) return 0;
      struct M {
        uint32_t bits;
        int rank;
        size_t idx;
        int block;
        float key;
      };
      std::vector<M> merged;
      for (int r = 0; r < static_cast<int>(all.size()); ++r) {
        const auto& m = all[r];
        for (size_t i = 0; i < (m.size() - 1) / 12; ++i) {
          M x{0, r, i, 0, 0.0f};
          std::memcpy(&x.bits, &m[1 + 12 * i], 4);
          std::memcpy(&x.block, &m[5 + 12 * i], 4);
          std::memcpy(&x.key, &m[9 + 12 * i], 4);
          if (x.bits < bound) merged.push_back(x);
        }
      }
      if (merged.empty()) {  // every sent key at the bound: wider windows
        window_ *= 2;
        continue;
      }
      std::sort(merged.begin(), merged.end(), [](const M& a, const M& b) {
        return a.bits != b.bits ? a.bits < b.bits : (a.rank != b.rank ? a.rank < b.rank : a.idx < b.idx);
      });
      // the first tie of several blocks ends the certified positions at its group's start
      size_t end = merged.size();
      for (size_t t = 1; t < merged.size(); ++t)
        if (merged[t].bits == merged[t - 1].bits && merged[t].block != merged[t - 1].block) {
          size_t g = t - 1;
          while (g > 0 && merged[g - 1].bits == merged[t].bits) --g;
          end = g;
          *open = true;
          break;
        }
      if (TestOpen() == 2 && end > 1) {  // (tests: the fallback in mid-tail)
        end /= 2;
        *open = true;
      }
      const int me = part->rank;
      blocks->clear();
      keys->clear();
      mine_.clear();
      for (size_t t = 0; t < end; ++t) {
        blocks->push_back(merged[t].block);
        keys->push_back(merged[t].key);
        mine_.push_back(merged[t].rank == me ? 1 : 0);
      }
      return 1;
    }
  }

  // GZ_STRIP_TEST_OPEN=prefix / tail: report the prefix / the middle of the
  // first tail window as open, so that tests take the exact path from there
  // (the result must not change).
  static int TestOpen() {
    static const int v = EnvIs("GZ_STRIP_TEST_OPEN", "prefix") ? 1 : EnvIs("GZ_STRIP_TEST_OPEN", "tail") ? 2 : 0;
    return v;
  }

  // The caller processed the first n positions of the last window.
  void Consumed(size_t n) {
    for (size_t t = 0; t < n && t < mine_.size(); ++t) pos_ += mine_[t];
    window_ = std::min<size_t>(window_ * 2, size_t{1} << 16);
  }

 private:
  struct Entry {
    uint32_t bits;
    int block;
    float key;
  };
  uint32_t kbits_ = 0;
  bool have_prefix_ = false;
  int tie_block_ = -1;
  int64_t take_ = 0;
  std::vector<Entry> rem_;
  size_t pos_ = 0, sorted_ = 0, window_ = 1024;
  std::vector<uint8_t> mine_;
};

// GZ_STRIP_ORDER=exact: every iteration on the exact path (A/B and tests).
bool StripFastOrder() {
  static const bool fast = !EnvIs("GZ_STRIP_ORDER", "exact");
  return fast;
}

}  // namespace

// The 4:4:4 back end of one SelectFrequencyMasking call (processor.cc:
// 723-919).  With a partition (a frame split over ranks by block rows,
// host/strips.h) img is this rank's strip: the entries, bulk changes and
// tail changes of its owned blocks are made here, and the frame-wide
// quantities -- the sorted change order, the histograms, the entropy
// estimate -- are exchanged or replicated.
//
// Run() reads as the algorithm: sizes and histograms once (Init), then per
// direction and iteration build the order, apply the bulk prefix, run the
// tail, advance the thresholds, encode and compare.  Every step that fails
// has set *err and returns false; on a split frame every rank makes the same
// exchanges in the same sequence on every path.
class BackEnd {
 public:
  BackEnd(Processor* p, const JpegData& jpg, CoeffImage* img, double target_mul, bool stop_early,
          const std::vector<int>& offsets, const std::vector<uint8_t>& cand, const std::vector<float>& cand_err,
          std::string* err)
      : p_(*p), cmp_(p->cmp_), res_(p->res_), part_(p->part_), jpg_(jpg), img_(img), target_mul_(target_mul),
        stop_early_(stop_early), offsets_(offsets), cand_(cand), cand_err_(cand_err), err_(err),
        ncomp_(static_cast<int>(jpg.components.size())), block_width_(img->block_w),
        num_blocks_(block_width_ * img->block_h), own_lo_(part_ ? part_->OwnLo() : 0),
        own_hi_(part_ ? part_->OwnHi() : num_blocks_),
        gbase_(part_ ? part_->LocalBase() : 0),  // frame index of local block 0
        own_chunks_((own_hi_ - own_lo_ + Processor::kOrderChunk - 1) / Processor::kOrderChunk) {}
  bool Run();

 private:
  // Where an iteration's change order comes from: the host's std::sort of
  // every entry (LazyStdSort), the device's selections, and on a frame split
  // over ranks the ranks' own entries merged (StripOrder), every rank's
  // entries gathered and sorted, or the device's selections over the ranks.
  enum class Order { kHost, kDevice, kStripFast, kStripExact, kStripDevice };
  // Where the bulk prefix is applied: the host's parallel apply, the device
  // that selected it, or this rank's device from the host's counts.
  enum class Apply { kHost, kDevice, kStripDevice };

  // The histograms after a step whose entropy codes are read, and the codes.
  struct Snap {
    size_t step;
    JpegHistogram h[3];
    std::vector<uint8_t> depths;
    int size = 0;
    int64_t raw[3] = {0, 0, 0};
  };

  // What lives for one pass of the iteration loop.
  struct Iteration {
    explicit Iteration(int dir) : direction(dir) {}
    const int direction;
    Order source = Order::kHost;
    // global_order holds the frame's entries and sorter their std::sort
    // order.  Set from the start for the host and strip-exact sources; the
    // others switch to it (FetchExact, GoExact) where the keys leave the
    // order open, and stay there for the rest of the iteration.
    bool exact = false;
    std::vector<std::pair<int, float>> global_order;
    int blocks_to_change = 0;
    std::vector<float> block_weight;
    size_t frame_n = 0;  // the frame's entry count (n_order)
    int64_t below_floor = -1;
    // std::sort(global_order) by key (processor.cc:840-843), materialised
    // lazily: only the prefix the change loop consumes gets sorted.
    std::unique_ptr<LazyStdSort> sorter;
    std::optional<ChangeLoop> loop;
    int est_jpg_size = 0;
    size_t bulk = 0;
    // The device order's window of the tail:
    std::vector<std::pair<int, float>> win;  // the tail from position win_base on, in order
    size_t win_base = 0;
    size_t win_ok = 0;                       // ... its positions certified to be std::sort's
    bool win_last = false;                   // ... and it holds every entry left
    std::vector<Snap> snaps;
    double codes_s = 0.0, sort_s = 0.0;
    int n_codes = 0;

    int TailBlock(size_t s) const { return exact ? global_order[s].first : win[s - win_base].first; }
    float TailKey(size_t s) const { return exact ? global_order[s].second : win[s - win_base].second; }
  };

  bool ExchangeFailed() {
    if (err_) *err_ = "strip exchange failed";
    return false;
  }
  bool Fail() { return p_.Fail(err_); }
  bool Split() const { return part_ && part_->world > 1; }
  // a device applies the bulk prefix: the host copy of a block follows lazily (Init)
  bool LazyHost() const { return apply_ != Apply::kHost; }
  // The iteration's mode, decided once: the order source here, the apply
  // target in Init (it cannot change between iterations).
  // A frame split over ranks: by default every rank keeps its own entries
  // (StripOrder) and the frame's std::sort order is derived from them where
  // the consumed entries' keys decide it alone; kStripExact: the whole
  // frame's entries on every rank (the fallback).
  Order OrderSource() const {
    if (device_order_) return Split() ? Order::kStripDevice : Order::kDevice;
    if (!Split()) return Order::kHost;
    return StripFastOrder() ? Order::kStripFast : Order::kStripExact;
  }
  // (the window: twice the last one / the last tail of this direction, 512 ..
  // 8192 entries -- sorted in one workgroup on the device)
  static size_t TailWindowSize(size_t n) { return std::min<size_t>(8192, std::max<size_t>(512, 2 * n)); }

  bool Init();
  void RefreshRaw() {
    for (int c = 0; c < ncomp_; ++c)
      raw_bits_[c] = HistogramRawBits(ac_histograms_[c], &ac_depths_[c * JpegHistogram::kSize]);
  }
  void Materialize(int bix, bool journal = false);
  void MaterializeHaloBand();
  bool FetchExact(Iteration& it);
  bool GoExact(Iteration& it);
  bool BuildOrder(Iteration& it);
  bool StartChangeLoop(Iteration& it);
  bool BulkOnDevice(Iteration& it);
  bool OpenPrefixOnDevice(Iteration& it);
  bool OpenPrefixOnStrips(Iteration& it);
  bool PrefixCounts(Iteration& it, Clock::time_point tbk);
  bool ApplyOwnedPrefixOnDevice(Iteration& it);
  bool BulkOnStripDevice(Iteration& it);
  bool BulkOnHost(Iteration& it);
  size_t RunSteps(Iteration& it, size_t i0, size_t n, const uint8_t* comp, const SymbolLog* logs,
                  const float* keys, bool* stop);
  void ApplyNext(int direction, int bix, SymbolLog* log);
  bool NextDeviceWindow(Iteration& it, size_t pos, bool* failed);
  bool TailReady(Iteration& it, size_t s);
  void PrefetchChunk(const Iteration& it, size_t lo, size_t hi);
  bool TailSingle(Iteration& it);
  bool TailWindow(Iteration& it, const int* blocks, const float* keys, size_t W, size_t i0, bool* stop,
                  size_t* done);
  bool TailStrips(Iteration& it);
  void FinishBulk(Iteration& it) {
    it.loop->changed = static_cast<int>(it.bulk);
    res_->detail["backend_bulk_changes"] += static_cast<double>(it.bulk);
  }

  Processor& p_;
  Comparator* const cmp_;
  ProcessResult* const res_;
  Partition* const part_;  // nullptr: the whole frame is this process's
  const JpegData& jpg_;
  CoeffImage* const img_;
  const double target_mul_;
  const bool stop_early_;
  const std::vector<int>& offsets_;
  const std::vector<uint8_t>& cand_;
  const std::vector<float>& cand_err_;
  std::string* const err_;
  const int ncomp_, block_width_, num_blocks_, own_lo_, own_hi_, gbase_, own_chunks_;

  std::vector<JpegHistogram> ac_histograms_;
  int jpg_header_size_ = 0, dc_size_ = 0;
  // the components SaveToJpegData keeps at the start, and the DC histograms
  // (the back end changes AC coefficients only: they stay as they are)
  int saved0_ = 3;
  JpegHistogram dc0_[3];
  std::vector<uint8_t> ac_depths_;
  int ac_histogram_size_ = 0;
  int base_size_ = 0, prev_size_ = 0;
  std::vector<int64_t> raw_bits_;
  AcBlockModel acm_;
  std::vector<float> max_block_error_;
  std::vector<int> last_indexes_;
  std::vector<float> zero_block_max_;
  bool first_up_iter_ = true;
  bool device_order_ = false;
  Apply apply_ = Apply::kHost;
  std::vector<int> mat_li_;
  std::vector<uint8_t> bulk_cnt8_;
  StripOrder strip_order_;  // (a frame split over ranks)
  // a strip window's tentative changes of owned blocks (TailWindow)
  struct Undo {
    size_t i;
    int bix, c, k;
    coeff_t old;
    uint64_t nz;
  };
  std::vector<Undo> undo_;
};

bool BackEnd::Run() {
  if (!Init()) return false;
  for (int direction : {1, -1}) {
    for (;;) {
      if (stop_early_) p_.FlushOutput();  // best_size_ must be current
      if (stop_early_ && direction == -1 && prev_size_ > 1.01 * p_.best_size_) break;
      const auto tb = Clock::now();
      Iteration it(direction);
      if (!BuildOrder(it)) return false;
      res_->detail["backend_order_s"] += Since(tb);
      res_->detail["backend_order_entries"] += static_cast<double>(it.frame_n);
      if (it.frame_n == 0) {
        res_->seconds_backend += Since(tb);
        break;
      }
      if (it.exact) it.sorter.reset(new LazyStdSort(it.global_order.data(), it.global_order.size()));
      const auto tc = Clock::now();
      if (!StartChangeLoop(it)) return false;
      // the bulk prefix, by the apply target (the device selection also
      // fetches the tail's window, so it runs without a prefix too)
      if (apply_ == Apply::kDevice) {
        if (!BulkOnDevice(it)) return false;
      } else if (it.bulk) {
        if (!(apply_ == Apply::kStripDevice ? BulkOnStripDevice(it) : BulkOnHost(it))) return false;
      }
      if (!(Split() ? TailStrips(it) : TailSingle(it))) return false;
      if (device_order_) p_.tail_len_[direction > 0 ? 0 : 1] = static_cast<size_t>(it.loop->changed) - it.bulk;
      res_->detail["backend_changes_s"] += Since(tc);
      res_->detail["backend_codes_s"] += it.codes_s;
      res_->detail["backend_sort_s"] += it.sort_s;
      res_->detail["backend_entropy_codes"] += it.n_codes;
      res_->detail["backend_changes"] += it.loop->changed;
      if (device_order_) {
        if (!cmp_->DeviceOrderAdvance(it.loop->val_threshold, direction)) return Fail();
      } else {
        for (int i = 0; i < num_blocks_; ++i)
          max_block_error_[i] += it.block_weight[i] * it.loop->val_threshold * direction;
      }
      ++res_->iterations;
      if (direction > 0) ++res_->iterations_up; else ++res_->iterations_down;
      res_->seconds_backend += Since(tb);
      if (cmp_->HasKnownHistogramEncode()) {
        // the candidate's histograms are the tracked ones: no histogram pass
        if (!p_.EncodeAndCompareKnown(jpg_, *img_, saved0_, dc0_, ac_histograms_, err_)) return false;
      } else if (!p_.EncodeAndCompare(jpg_, *img_, err_)) {
        return false;
      }
      prev_size_ = it.est_jpg_size;
    }
  }
  if (LazyHost()) {
    // the device copy is the image now; nothing after the back end reads
    // the host copy before the next bulk rewrite (CopyFromJpegData) -- a
    // mirror that would have to read it fails instead (host_valid)
    img_->host_valid = false;
    img_->host_partial = false;
  }
  p_.FlushOutput();
  return true;
}

// The sizes that do not change, the AC histograms and their codes at the
// start, and the call's apply target.
bool BackEnd::Init() {
  ac_histograms_.resize(ncomp_);
  {
    JpegHistogram dc_h[3], ac_h[3];
    int saved = cmp_->DeviceHistograms(*img_, dc_h, ac_h);
    if (saved < 0 && cmp_->HasDeviceWriter()) return Fail();
    if (saved < 0) saved = CoeffImageHistograms(*img_, p_.scratch_.get(), dc_h, ac_h);
    saved0_ = saved;
    for (int c = 0; c < 3; ++c) dc0_[c] = dc_h[c];
    JpegData out;
    out.app_data = jpg_.app_data;
    out.com_data = jpg_.com_data;
    img_->SaveHeaderToJpegData(saved, &out);
    if (part_) {
      out.width = part_->width;
      out.height = part_->height;
    }
    jpg_header_size_ = static_cast<int>(JpegHeaderSize(out, p_.params_.clear_metadata));
    size_t num = saved;
    int idx[3];
    std::vector<uint8_t> depths(saved * JpegHistogram::kSize);
    dc_size_ = static_cast<int>(ClusterHistograms(dc_h, &num, idx, depths.data()));
    for (int c = 0; c < ncomp_ && c < 3; ++c) ac_histograms_[c] = ac_h[c];
  }
  ac_histogram_size_ = static_cast<int>(ComputeEntropyCodes(ac_histograms_, &ac_depths_));
  base_size_ = jpg_header_size_ + dc_size_ + ac_histogram_size_ +
               static_cast<int>(EntropyCodedDataSize(ac_histograms_, ac_depths_));
  raw_bits_.resize(ncomp_);
  RefreshRaw();
  acm_.Build(*img_);
  prev_size_ = base_size_;
  max_block_error_.assign(num_blocks_, 0.0f);
  last_indexes_.assign(num_blocks_, 0);
  zero_block_max_.assign(num_blocks_, 0.0f);
  // the change order on the device (weights, entries, max_block_error there;
  // the frame's candidates and block maxima are resident) unless the
  // comparator has no device.
  // A frame split over ranks with the device order (round 6): every rank's
  // engine builds its owned blocks' entries; the selections exchange their
  // counts and candidates (the comparator's scope, Engine::OrderSelect), so
  // the bulk prefix, the windows and their certification are the frame's on
  // every rank; the owners apply the changes (their device bulk, the tail's
  // windows through TailWindow below).
  if (cmp_->HasDeviceBulk() && !cmp_->DeviceOrderReset(&device_order_)) return Fail();
  // With the device order the bulk prefix is selected and applied on the
  // device too (DeviceSelectBulk), with the change of the AC histograms
  // counted there.
  // The host copy of a block then follows lazily: a block's coefficients are a function of
  // its last_indexes alone -- its first last_indexes[b] candidates zeroed,
  // the others as quantized (up iterations zero candidates in order, down
  // iterations restore them in reverse) -- so mat_li[b], the last_indexes the
  // host copy reflects, is brought up to date (Materialize) before the tail
  // reads or changes the block.
  // A frame split over ranks applies its owned blocks' bulk prefix on its
  // own device too (from the host's counts and last_indexes), its host copy
  // then following lazily as with the device order -- except the blocks
  // within the halo band of a strip edge, which the neighbours' halos need:
  // those are brought up to date and journalled at once (SyncHalo ships the
  // journal).  (GZ_STRIP_HOST_BULK=1: the host applies it, for A/B runs.)
  static const bool strip_host_bulk = EnvFlag("GZ_STRIP_HOST_BULK");
  if (device_order_) {
    apply_ = Apply::kDevice;
  } else if (part_ && !strip_host_bulk && cmp_->HasDeviceBulkLocal()) {
    apply_ = Apply::kStripDevice;
  }
  if (LazyHost()) mat_li_.assign(num_blocks_, 0);
  return true;
}

void BackEnd::Materialize(int bix, bool journal) {
  int m = mat_li_[bix];
  const int li = last_indexes_[bix];
  if (m == li) return;
  const int offset = std::max(0, std::min(offsets_[bix], static_cast<int>(cand_.size()) - 1));
  const int bx = bix % block_width_, by = bix / block_width_;
  for (; m != li; m += m < li ? 1 : -1) {
    const int idx = cand_[offset + (m < li ? m : m - 1)];
    const int c = idx / kDCTBlockSize, k = idx % kDCTBlockSize;
    coeff_t v = 0;
    if (m > li) {
      const JpegComponent& comp = jpg_.components[c];
      v = QuantizeCoeff(comp.coeffs[static_cast<size_t>(by * comp.width_in_blocks + bx) * 64 + k], img_->quant[c][k]);
    }
    img_->block(c, bix)[k] = v;
    if (journal) img_->MarkChanged(c, bix, k);
    uint64_t& nzm = acm_.nz[static_cast<size_t>(c) * num_blocks_ + bix];
    const int z = kJPEGZigZagOrder[k];
    if (v) nzm |= 1ull << z; else nzm &= ~(1ull << z);
  }
  mat_li_[bix] = li;
}

// (a strip: the blocks within the halo band of its edges, which the
// neighbours' halos need, brought up to date and journalled at once)
void BackEnd::MaterializeHaloBand() {
  const int band = (kStripHalo / 8) * block_width_;
  for (int bix = own_lo_; bix < std::min(own_hi_, own_lo_ + band); ++bix) Materialize(bix, true);
  for (int bix = std::max(own_lo_ + band, own_hi_ - band); bix < own_hi_; ++bix) Materialize(bix, true);
}

// device order: the entries come to the host (all of them, in block
// order, for std::sort's exact permutation) only where the keys leave
// the order open
bool BackEnd::FetchExact(Iteration& it) {
  const auto tf = Clock::now();
  if (!cmp_->DeviceOrderEntries(&it.global_order)) return false;
  if (it.global_order.size() != it.frame_n) {
    p_.internal_err_ = "device order: entry count mismatch";
    return false;
  }
  it.sorter.reset(new LazyStdSort(it.global_order.data(), it.global_order.size()));
  it.exact = true;
  res_->detail["backend_order_fetches"] += 1;
  res_->detail["backend_order_fetch_s"] += Since(tf);
  return true;
}

// a split frame: this rank's entries, global_order, become the frame's (the
// exact path) when their keys leave std::sort's order open
bool BackEnd::GoExact(Iteration& it) {
  const auto tg = Clock::now();
  int btc = it.blocks_to_change;
  // (the device order: this rank's entries come from its engine first)
  if (it.source == Order::kStripDevice && !cmp_->DeviceOrderEntries(&it.global_order)) return false;
  if (!p_.GatherEntries(&it.global_order, own_lo_, own_hi_, gbase_, &btc)) return false;
  it.sorter.reset(new LazyStdSort(it.global_order.data(), it.global_order.size()));
  it.exact = true;
  res_->detail["strip_order_fallbacks"] += 1;
  res_->detail["strip_order_fallback_s"] += Since(tg);
  return true;
}

// The iteration's change entries: on the device (they stay there), or in
// global_order -- the frame's, or with kStripFast this rank's own.
bool BackEnd::BuildOrder(Iteration& it) {
  it.source = OrderSource();
  it.exact = it.source == Order::kHost || it.source == Order::kStripExact;
  if (device_order_) {
    // (the entries stay on the device; the first up iteration's count of
    // keys below its floor comes back with their count)
    const float floor_limit = first_up_iter_ ? 0.75f * cmp_->BlockErrorLimit() : -HUGE_VALF;
    if (!cmp_->DeviceChangeOrder(it.direction, target_mul_, first_up_iter_, last_indexes_, floor_limit, &it.frame_n,
                                 &it.blocks_to_change, first_up_iter_ ? &it.below_floor : nullptr))
      return Fail();
    return true;
  }
  if (!first_up_iter_ && (cmp_->block_max_distance(), cmp_->block_max_failed())) return Fail();
  const bool own_entries = it.source == Order::kStripFast;
  if (!p_.BuildChangeOrder(it.direction, 1, target_mul_, num_blocks_, own_lo_, own_hi_, gbase_,
                           first_up_iter_ ? zero_block_max_ : cmp_->block_max_distance(), last_indexes_,
                           offsets_, cand_err_, max_block_error_, &it.global_order, &it.block_weight,
                           &it.blocks_to_change, own_entries ? &it.frame_n : nullptr))
    return ExchangeFailed();
  if (!own_entries) it.frame_n = it.global_order.size();
  return true;
}

// The change loop's control for this order, and the length of its bulk prefix.
bool BackEnd::StartChangeLoop(Iteration& it) {
  // (the frame's count of keys below the first up iteration's floor: the
  // device order's came back with the order)
  if (it.source == Order::kStripFast && first_up_iter_) {
    const float limit = 0.75f * cmp_->BlockErrorLimit();
    it.below_floor = 0;
    for (const auto& e : it.global_order) it.below_floor += e.second < limit ? 1 : 0;
    if (!part_->SumAll(&it.below_floor, 1)) return ExchangeFailed();
  }
  it.loop.emplace(it.direction, cmp_->DistanceOK(1.0), base_size_, 1, it.blocks_to_change, &first_up_iter_,
                  cmp_->BlockErrorLimit(), it.global_order, it.frame_n, it.below_floor);
  it.est_jpg_size = prev_size_;
  // Changes before the loop's first read of an entropy code or size
  // estimate (first_read: the first i % 10 == 0 step whose codes are
  // read, the first step with changed > min_coeffs_to_change, or
  // the last one) only accumulate; their effect -- block states, AC
  // histograms, last_indexes -- depends on which changes they are, not
  // on their order.  So [0, first_read) is taken as std::sort's first
  // first_read entries as a set (LazyStdSort::SetPrefix: partitioning
  // only, no sort of the prefix) and applied per block in parallel.
  const long m = std::max(0, it.loop->min_coeffs);
  const long n = static_cast<long>(it.frame_n);
  const long lo = std::max(0L, std::min(m - 9, n - 10));
  const long first_code = (lo + 9) / 10 * 10;
  const long first_read = std::min(std::min(first_code, m), n - 1);
  if (first_read >= Processor::kMinBulkChanges) it.bulk = static_cast<size_t>(first_read);
  it.win_base = it.bulk;
  return true;
}

// The device order's selection: the bulk prefix as a set from the keys
// (applied on the device) and the tail's window of the next entries.
bool BackEnd::BulkOnDevice(Iteration& it) {
  const auto tbk = Clock::now();
  // (the window: TailWindowSize of the last tail of this direction;
  // GZ_TAIL_WINDOW: a fixed size, for tests)
  static const size_t fixed_window = static_cast<size_t>(EnvInt("GZ_TAIL_WINDOW", 0));
  const size_t last_tail = p_.tail_len_[it.direction > 0 ? 0 : 1];
  const size_t kTailWindow = fixed_window ? fixed_window : TailWindowSize(last_tail);
  Engine::OrderSelection sel;
  JpegHistogram ac_now[3];
  for (int c = 0; c < ncomp_ && c < 3; ++c) ac_now[c] = ac_histograms_[c];
  if (!cmp_->DeviceSelectBulk(*img_, it.bulk, kTailWindow, it.direction, &sel, ac_now)) return Fail();
  if (it.bulk && sel.applied) {
    for (int c = 0; c < ncomp_ && c < 3; ++c) ac_histograms_[c] = ac_now[c];
    // (the counts include the tie block's share of the K*-keyed entries)
    for (int bix = 0; bix < num_blocks_; ++bix) last_indexes_[bix] += sel.cnt[bix] * it.direction;
    img_->host_partial = true;
    if (it.source == Order::kStripDevice) MaterializeHaloBand();
    RefreshRaw();
    FinishBulk(it);
    res_->detail["backend_bulk_device"] += 1;
  } else if (it.bulk) {
    // K* shared by several blocks across the prefix's end: std::sort's
    // tie order decides which of them the prefix takes -- the exact
    // path (every entry, LazyStdSort), applied with the host's counts
    res_->detail["backend_select_open"] += 1;
    if (!(it.source == Order::kStripDevice ? OpenPrefixOnStrips(it) : OpenPrefixOnDevice(it))) return false;
    FinishBulk(it);
    res_->detail["backend_bulk_device"] += 1;
  }
  if (!it.exact && !sel.window_overflow) {
    // the window, sorted on the device: std::sort's order for its first
    // window_ok positions (up to the first key shared by entries of
    // several blocks; entries of one block are interchangeable: a
    // change takes the block's next candidate)
    it.win.swap(sel.window);
    it.win_ok = sel.window_ok;
    it.win_last = sel.window_last;
  }
  res_->detail["backend_bulk_s"] += Since(tbk);
  return true;
}

// An open prefix on one engine: every entry fetched, the prefix's per-block
// counts from std::sort's order applied by the device.
bool BackEnd::OpenPrefixOnDevice(Iteration& it) {
  if (!FetchExact(it)) return Fail();
  it.sorter->SetPrefix(it.bulk);
  bulk_cnt8_.assign(num_blocks_, 0);
  for (size_t i = 0; i < it.bulk; ++i) ++bulk_cnt8_[it.global_order[i].first];
  for (int bix = 0; bix < num_blocks_; ++bix) last_indexes_[bix] += bulk_cnt8_[bix] * it.direction;
  JpegHistogram ac_now[3];
  for (int c = 0; c < ncomp_ && c < 3; ++c) ac_now[c] = ac_histograms_[c];
  if (!cmp_->DeviceBulkApply(*img_, it.direction, bulk_cnt8_.data(), ac_now)) return Fail();
  for (int c = 0; c < ncomp_ && c < 3; ++c) ac_histograms_[c] = ac_now[c];
  img_->host_partial = true;
  RefreshRaw();
  return true;
}

// An open prefix on a split frame: the frame's entries on every rank, the
// owned blocks' prefix share applied on each rank's device, the histogram
// change summed
bool BackEnd::OpenPrefixOnStrips(Iteration& it) {
  if (!GoExact(it)) return ExchangeFailed();
  it.sorter->SetPrefix(it.bulk);
  bulk_cnt8_.assign(num_blocks_, 0);
  for (size_t i = 0; i < it.bulk; ++i) {
    const int b = it.global_order[i].first - gbase_;
    if (b >= own_lo_ && b < own_hi_) ++bulk_cnt8_[b];
  }
  return ApplyOwnedPrefixOnDevice(it);
}

// bulk_cnt8_ (this rank's owned blocks' shares of the prefix) applied on this
// rank's device; its histogram delta summed over the ranks, last_indexes and
// the halo bands brought along.
bool BackEnd::ApplyOwnedPrefixOnDevice(Iteration& it) {
  int32_t delta[3][256] = {};
  // (a failure on one rank fails every rank at the all-sum below:
  // its status travels with the delta)
  const bool ok = cmp_->DeviceBulkApplyLocal(*img_, it.direction, bulk_cnt8_.data(), last_indexes_, delta);
  std::vector<int64_t> hsum(3 * (JpegHistogram::kSize - 1) + 1, 0);
  for (int c = 0; c < ncomp_ && c < 3; ++c)
    for (int q = 0; q + 1 < JpegHistogram::kSize; ++q) hsum[c * (JpegHistogram::kSize - 1) + q] = delta[c][q];
  hsum.back() = ok ? 0 : 1;
  if (!part_->SumAll(hsum.data(), static_cast<int>(hsum.size()))) return ExchangeFailed();
  if (!ok) return Fail();
  if (hsum.back()) {
    if (err_) *err_ = "a rank's device bulk prefix failed";
    return false;
  }
  for (int bix = own_lo_; bix < own_hi_; ++bix) last_indexes_[bix] += bulk_cnt8_[bix] * it.direction;
  img_->host_partial = true;
  // the halo bands' blocks now, journalled (the neighbours' halos)
  MaterializeHaloBand();
  // (the counts are stored doubled, JpegHistogram::Add)
  for (int c = 0; c < ncomp_ && c < 3; ++c)
    for (int q = 0; q + 1 < JpegHistogram::kSize; ++q)
      ac_histograms_[c].counts[q] += 2u * static_cast<uint32_t>(hsum[c * (JpegHistogram::kSize - 1) + q]);
  RefreshRaw();
  return true;
}

// The host order's prefix as a set, and p_.bulk_cnt_: per owned block its
// entries among the prefix.  (tbk: the bulk step's start.)
bool BackEnd::PrefixCounts(Iteration& it, Clock::time_point tbk) {
  if (it.source == Order::kStripFast) {
    // the prefix as a set from the keys alone (StripOrder::Prefix);
    // open (tied keys of several blocks across its boundary): exact
    const int r = strip_order_.Prefix(it.global_order, it.bulk, part_, gbase_, num_blocks_, &p_.bulk_cnt_);
    if (r < 0) return ExchangeFailed();
    if (r == 0 && !GoExact(it)) return ExchangeFailed();
  }
  if (it.exact) it.sorter->SetPrefix(it.bulk);
  res_->detail["backend_setprefix_s"] += Since(tbk);
  // per-block counts of the prefix's owned entries (parallel; blocks
  // are spread, so the atomic increments rarely meet)
  if (it.exact) {
    p_.bulk_cnt_.assign(num_blocks_, 0);
    const size_t bulk = it.bulk;
    const int kSlices = bulk >= (size_t{1} << 18) ? 64 : 1;
    int* cnt = p_.bulk_cnt_.data();
    const std::pair<int, float>* order = it.global_order.data();
    ParallelFor(kSlices, [&](int sl) {
      for (size_t i = bulk * sl / kSlices; i < bulk * (sl + 1) / kSlices; ++i) {
        const int b = order[i].first - gbase_;
        if (b >= own_lo_ && b < own_hi_) __atomic_fetch_add(&cnt[b], 1, __ATOMIC_RELAXED);
      }
    });
  }
  return true;
}

// The host order's prefix on a split frame: the owned blocks' share on this
// rank's device; its histogram delta summed over the ranks
bool BackEnd::BulkOnStripDevice(Iteration& it) {
  const auto tbk = Clock::now();
  if (!PrefixCounts(it, tbk)) return false;
  const auto td = Clock::now();
  bulk_cnt8_.assign(num_blocks_, 0);
  for (int bix = own_lo_; bix < own_hi_; ++bix) bulk_cnt8_[bix] = static_cast<uint8_t>(p_.bulk_cnt_[bix]);
  if (!ApplyOwnedPrefixOnDevice(it)) return false;
  it.loop->changed = static_cast<int>(it.bulk);
  res_->detail["backend_bulk_s"] += Since(tbk);
  res_->detail["backend_bulk_device_s"] += Since(td);
  res_->detail["backend_bulk_changes"] += static_cast<double>(it.bulk);
  res_->detail["backend_bulk_device"] += 1;
  return true;
}

// The host order's prefix applied on the host, per chunk of owned blocks in
// parallel; the chunks' histogram deltas summed (over the ranks too).
bool BackEnd::BulkOnHost(Iteration& it) {
  const auto tbk = Clock::now();
  if (!PrefixCounts(it, tbk)) return false;
  struct ChunkDelta {
    JpegHistogram h[3];
    std::vector<uint32_t> changed;
  };
  const int direction = it.direction;
  const std::vector<int>& bulk_cnt = p_.bulk_cnt_;
  std::vector<ChunkDelta> deltas(own_chunks_);
  ParallelFor(own_chunks_, [&](int ch) {
    ChunkDelta& d = deltas[ch];
    int64_t raw_unused = 0;
    const int b0 = own_lo_ + ch * Processor::kOrderChunk, b1 = std::min(own_hi_, b0 + Processor::kOrderChunk);
    size_t total = 0;
    for (int bix = b0; bix < b1; ++bix) total += bulk_cnt[bix];
    d.changed.reserve(total);
    // the touched blocks are scattered over three 2-byte-per-coefficient
    // planes much larger than the caches: fetch a block a few touched
    // blocks ahead (its first change's plane, the mask word, and for
    // direction < 0 the original coefficients)
    constexpr int kAhead = 6;
    auto prefetch = [&](int b) {
      const int off = std::max(0, std::min(offsets_[b], static_cast<int>(cand_.size()) - 1));
      const int ci = off + last_indexes_[b] + std::min(direction, 0);
      if (ci < 0 || ci >= static_cast<int>(cand_.size())) return;
      const int c = cand_[ci] / kDCTBlockSize;
      const coeff_t* blk = img_->block(c, b);
      __builtin_prefetch(blk, 1);
      __builtin_prefetch(blk + 32, 1);
      __builtin_prefetch(&acm_.nz[static_cast<size_t>(c) * num_blocks_ + b], 1);
      if (direction < 0) {
        const JpegComponent& comp = jpg_.components[c];
        const coeff_t* o = comp.coeffs.data() +
                           static_cast<size_t>((b / block_width_) * comp.width_in_blocks + b % block_width_) * 64;
        __builtin_prefetch(o);
        __builtin_prefetch(o + 32);
      }
    };
    int ahead = b0, pending = 0;  // next block to prefetch; touched blocks in flight
    for (int bix = b0; bix < b1; ++bix) {
      for (; ahead < b1 && pending < kAhead; ++ahead)
        if (bulk_cnt[ahead]) {
          prefetch(ahead);
          ++pending;
        }
      const int cnt = bulk_cnt[bix];
      if (!cnt) continue;
      --pending;
      const int bx = bix % block_width_, by = bix / block_width_;
      const int offset = std::max(0, std::min(offsets_[bix], static_cast<int>(cand_.size()) - 1));
      int li = last_indexes_[bix];
      for (int t = 0; t < cnt; ++t) {
        const int idx = cand_[offset + li + std::min(direction, 0)];
        const int c = idx / kDCTBlockSize, k = idx % kDCTBlockSize;
        const int* quant = img_->quant[c];
        int newval = 0;
        if (direction < 0) {
          const JpegComponent& comp = jpg_.components[c];
          const int jpg_bix = by * comp.width_in_blocks + bx;
          newval = QuantizeCoeff(comp.coeffs[static_cast<size_t>(jpg_bix) * 64 + k], quant[k]);
        }
        acm_.Change<JpegHistogram, false>(c, bix, num_blocks_, img_->block(c, bix), k,
                                          static_cast<coeff_t>(newval), quant,
                                          &ac_depths_[c * JpegHistogram::kSize], &d.h[c], &raw_unused);
        d.changed.push_back(static_cast<uint32_t>((static_cast<size_t>(c) * num_blocks_ + bix) * 64 + k));
        li += direction;
      }
      last_indexes_[bix] = li;
    }
  });
  // (symbols only: the last slot is the histogram's fixed sentinel count)
  std::vector<int64_t> hsum(3 * (JpegHistogram::kSize - 1), 0);
  for (const ChunkDelta& d : deltas) {
    for (int c = 0; c < ncomp_ && c < 3; ++c)
      for (int q = 0; q + 1 < JpegHistogram::kSize; ++q)
        hsum[c * (JpegHistogram::kSize - 1) + q] += static_cast<int32_t>(d.h[c].counts[q]);
    img_->changed.insert(img_->changed.end(), d.changed.begin(), d.changed.end());
  }
  // (the counts wrap: a chunk's removals are negative deltas)
  if (part_ && !part_->SumAll(hsum.data(), static_cast<int>(hsum.size()))) return ExchangeFailed();
  for (int c = 0; c < ncomp_ && c < 3; ++c)
    for (int q = 0; q + 1 < JpegHistogram::kSize; ++q)
      ac_histograms_[c].counts[q] += static_cast<uint32_t>(hsum[c * (JpegHistogram::kSize - 1) + q]);
  RefreshRaw();
  it.loop->changed = static_cast<int>(it.bulk);
  res_->detail["backend_bulk_s"] += Since(tbk);
  res_->detail["backend_bulk_changes"] += static_cast<double>(it.bulk);
  return true;
}

// The bookkeeping of steps [i0, i0 + n) whose changes' symbol updates
// are known (step k: component comp[k], updates logs[k]; key keys[k]),
// in speculative batches.  The entropy codes read at step i (i % 10
// == 0) are a function of the AC histograms after step i alone, and
// the histograms after every step follow from the steps' symbol
// updates, which need no codes.  So the histograms are advanced over
// the steps first, copied at every step whose codes are read, those
// codes built on the pool at once, then the estimate and the break
// test run over the steps in order with the same values as the
// one-at-a-time loop; the histograms of the steps past
// the break are taken back.  Returns the steps processed (through the
// break when *stop).
size_t BackEnd::RunSteps(Iteration& it, size_t i0, size_t n, const uint8_t* comp, const SymbolLog* logs,
                         const float* keys, bool* stop) {
  ChangeLoop& loop = *it.loop;
  std::vector<Snap>& snaps = it.snaps;
  const int ncomp = ncomp_;
  *stop = false;
  size_t ns = 0;
  for (size_t k = 0; k < n; ++k) {
    const SymbolLog& lg = logs[k];
    for (int e = 0; e < lg.n; ++e) ac_histograms_[comp[k]].Add(lg.sym[e], lg.weight[e]);
    if (loop.CodesRead(i0 + k)) {
      if (ns == snaps.size()) snaps.emplace_back();
      Snap& sn = snaps[ns++];
      sn.step = i0 + k;
      for (int c = 0; c < ncomp && c < 3; ++c) sn.h[c] = ac_histograms_[c];
    }
  }
  // (a task takes two consecutive rebuilds: the code-length caches are per thread)
  if (ns) {
    const auto te = Clock::now();
    const int tasks = static_cast<int>((ns + 1) / 2);
    auto build = [&](int t) {
      for (size_t q = 2 * static_cast<size_t>(t); q < std::min(ns, 2 * static_cast<size_t>(t) + 2); ++q) {
        Snap& sn = snaps[q];
        std::vector<JpegHistogram> hv(sn.h, sn.h + ncomp);
        sn.size = static_cast<int>(ComputeEntropyCodes(hv, &sn.depths));
        for (int c = 0; c < ncomp; ++c) sn.raw[c] = HistogramRawBits(sn.h[c], &sn.depths[c * JpegHistogram::kSize]);
      }
    };
    if (tasks == 1) build(0); else ParallelFor(tasks, build);
    it.codes_s += Since(te);
    it.n_codes += static_cast<int>(ns);
  }
  size_t q = 0, k = 0;
  for (; k < n; ++k) {
    const size_t s = i0 + k;
    loop.Applied(keys[k]);
    if (q < ns && snaps[q].step == s) {
      const Snap& sn = snaps[q++];
      ac_histogram_size_ = sn.size;
      ac_depths_ = sn.depths;
      for (int c = 0; c < ncomp; ++c) raw_bits_[c] = sn.raw[c];
    } else {
      const SymbolLog& lg = logs[k];
      const uint8_t* d = &ac_depths_[comp[k] * JpegHistogram::kSize];
      for (int e = 0; e < lg.n; ++e)
        raw_bits_[comp[k]] += static_cast<int64_t>(lg.weight[e]) * (d[lg.sym[e]] + (lg.sym[e] & 0xf));
    }
    if (!loop.EstimateRead(s)) continue;
    it.est_jpg_size = jpg_header_size_ + dc_size_ + ac_histogram_size_ + EntropySizeFromRaw(raw_bits_);
    if (loop.Stop(it.est_jpg_size, prev_size_)) {
      *stop = true;
      break;
    }
  }
  if (*stop) {
    for (size_t u = k + 1; u < n; ++u)
      for (int e = 0; e < logs[u].n; ++e) ac_histograms_[comp[u]].Add(logs[u].sym[e], -logs[u].weight[e]);
    res_->detail["backend_spec_wasted_codes"] += static_cast<double>(ns - q);
    return k + 1;
  }
  return n;
}

// the change of the next entry of owned block bix applied to img: its
// symbol updates into the frame's histograms, or (log) recorded
void BackEnd::ApplyNext(int direction, int bix, SymbolLog* log) {
  if (LazyHost()) Materialize(bix);
  const int bx = bix % block_width_, by = bix / block_width_;
  const int last_idx = last_indexes_[bix];
  const int offset = std::max(0, std::min(offsets_[bix], static_cast<int>(cand_.size()) - 1));
  const int idx = cand_[offset + last_idx + std::min(direction, 0)];
  const int c = idx / kDCTBlockSize, k = idx % kDCTBlockSize;
  const int* quant = img_->quant[c];
  const JpegComponent& comp = jpg_.components[c];
  const int jpg_bix = by * comp.width_in_blocks + bx;
  const int newval = direction > 0 ? 0 : QuantizeCoeff(comp.coeffs[static_cast<size_t>(jpg_bix) * 64 + k], quant[k]);
  if (log) {
    int64_t raw_unused = 0;
    acm_.Change(c, bix, num_blocks_, img_->block(c, bix), k, static_cast<coeff_t>(newval), quant,
                &ac_depths_[c * JpegHistogram::kSize], log, &raw_unused);
  } else {
    acm_.Change(c, bix, num_blocks_, img_->block(c, bix), k, static_cast<coeff_t>(newval), quant,
                &ac_depths_[c * JpegHistogram::kSize], &ac_histograms_[c], &raw_bits_[c]);
  }
  img_->MarkChanged(c, bix, k);
  last_indexes_[bix] += direction;
  if (LazyHost()) mat_li_[bix] = last_indexes_[bix];
}

// The device window ran out at position pos without a tie: asks the device
// for the next one from rank pos.  Returns whether pos is now certified;
// false also when there is nothing to continue (no window at all -- the
// selection's candidates overflowed, or its prefix was open -- a tie, or the
// last window) or the next window is open or overflowed: the caller goes to
// the exact order.  *failed: the device call failed.
bool BackEnd::NextDeviceWindow(Iteration& it, size_t pos, bool* failed) {
  *failed = false;
  if (it.win.empty() || it.win_ok != it.win.size() || it.win_last || pos != it.win_base + it.win_ok) return false;
  Engine::OrderSelection next;
  const size_t want = TailWindowSize(it.win.size());
  const auto tw = Clock::now();
  if (!cmp_->DeviceSelectWindow(pos, want, it.direction, &next)) {
    *failed = true;
    return false;
  }
  res_->detail["backend_tail_windows"] += 1;
  res_->detail["backend_tail_window_s"] += Since(tw);
  if (next.open || next.window_overflow) return false;
  it.win.swap(next.window);
  it.win_base = pos;
  it.win_ok = next.window_ok;
  it.win_last = next.window_last;
  return pos < it.win_base + it.win_ok;
}

// The single-rank tail's entry at position s is known: the device window's
// certified positions, else (past them, or without a window) std::sort's
// exact order -- all entries fetched once, LazyStdSort with the prefix set
// aside; the window's positions before are the same in it (see above)
bool BackEnd::TailReady(Iteration& it, size_t s) {
  if (!it.exact) {
    if (s < it.win_base + it.win_ok) return true;
    bool failed = false;
    if (NextDeviceWindow(it, s, &failed)) return true;
    if (failed) return false;
    const bool no_window = it.win.empty();
    if (!FetchExact(it)) return false;
    const auto tp = Clock::now();
    if (it.bulk) it.sorter->SetPrefix(it.bulk);
    res_->detail["backend_setprefix_s"] += Since(tp);
    res_->detail["backend_tail_exact"] += 1;
    if (!it.bulk && no_window) res_->detail["backend_tail_exact_nobulk"] += 1;
  }
  if (s >= it.sorter->sorted()) {
    const auto ts = Clock::now();
    it.sorter->EnsureSorted(s);
    it.sort_s += Since(ts);
  }
  return true;
}

// Prefetch window: when the lazy sort hands out a new sorted chunk, the
// chunk's per-block state is touched ahead of the (serial) changes in
// three dependent passes -- block bookkeeping, then the candidate byte,
// then the coefficient block and its non-zero mask -- so the cache
// misses of a chunk overlap instead of chaining.  Values are only
// prefetched; the tail reads them as before.
void BackEnd::PrefetchChunk(const Iteration& it, size_t lo, size_t hi) {
  const int direction = it.direction;
  for (size_t j = lo; j < hi; ++j) {
    const int b = it.TailBlock(j);
    __builtin_prefetch(&last_indexes_[b]);
    __builtin_prefetch(&offsets_[b]);
  }
  for (size_t j = lo; j < hi; ++j) {
    const int b = it.TailBlock(j);
    const int off = std::max(0, std::min(offsets_[b], static_cast<int>(cand_.size()) - 1));
    const int ci = off + last_indexes_[b] + std::min(direction, 0);
    if (ci >= 0 && ci < static_cast<int>(cand_.size())) __builtin_prefetch(&cand_[ci]);
  }
  for (size_t j = lo; j < hi; ++j) {
    const int b = it.TailBlock(j);
    const int off = std::max(0, std::min(offsets_[b], static_cast<int>(cand_.size()) - 1));
    const int ci = off + last_indexes_[b] + std::min(direction, 0);
    if (ci < 0 || ci >= static_cast<int>(cand_.size())) continue;
    const int c = cand_[ci] / kDCTBlockSize;
    __builtin_prefetch(img_->block(c, b), 1);
    __builtin_prefetch(&acm_.nz[static_cast<size_t>(c) * num_blocks_ + b], 1);
  }
}

// The tail on one engine, in speculative batches.  The entropy codes read at change
// i (i % 10 == 0) are a function of the AC histograms after change i
// alone, and the histograms after every change follow from the
// changes' symbol updates, which need no codes.  So a batch applies
// its changes first (recording each one's symbol updates and what
// undoes it), copies the histograms at every step whose codes are
// read, builds those codes on the pool at once, then runs the
// estimate and the break test over the batch in order with the same
// values as the one-at-a-time loop; the changes past the break are
// undone.  Batches grow from 4 to kMaxDecades rebuilds (capped by
// the pool workers this encode may use), so a tail that stops early
// wastes at most a few rebuilds.
bool BackEnd::TailSingle(Iteration& it) {
  const int direction = it.direction;
  const size_t n_order = it.frame_n;
  size_t prefetched = it.bulk;
  struct Spec {
    int bix, k;
    coeff_t old;
    uint64_t nz;
  };
  std::vector<Spec> spec;
  std::vector<uint8_t> sp_comp;
  std::vector<SymbolLog> sp_log;
  std::vector<float> sp_key;
  const int workers = std::max(1, PoolWorkerCap());
  constexpr int kMaxDecades = 32;
  // (GZ_SPEC_DECADES: a fixed batch, for A/B runs and tests; set to anything
  // but a positive count: 1)
  static const int fixed_decades = EnvInt("GZ_SPEC_DECADES", std::getenv("GZ_SPEC_DECADES") ? 1 : 0);
  int decades = fixed_decades ? fixed_decades : std::min(4, 2 * workers);
  size_t i = it.bulk;
  bool stop = false;
  while (!stop && i < n_order) {
    const size_t first_code = (i + 9) / 10 * 10;
    const size_t j = std::min(n_order, first_code + 10 * static_cast<size_t>(decades));
    spec.clear();
    sp_comp.clear();
    sp_log.clear();
    sp_key.clear();
    // A: the batch's changes, their symbol updates into the histograms
    for (size_t s = i; s < j; ++s) {
      if (!TailReady(it, s)) return Fail();
      if (s >= prefetched) {
        prefetched = it.exact ? std::max(it.sorter->sorted(), s + 1) : std::min(it.win_base + it.win_ok, s + 256);
        PrefetchChunk(it, s, std::min(prefetched, n_order));
      }
      const int bix = it.TailBlock(s);
      if (LazyHost()) Materialize(bix);
      const int off = std::max(0, std::min(offsets_[bix], static_cast<int>(cand_.size()) - 1));
      const int li = last_indexes_[bix] + std::min(direction, 0);
      if (li < 0 || off + li >= offsets_[bix + 1]) {  // (an order entry without a candidate: a bug)
        if (err_) *err_ = "back end: change order names a block without candidates left";
        return false;
      }
      const int idx = cand_[off + li];
      Spec sp;
      sp.bix = bix;
      const int c = idx / kDCTBlockSize;
      sp.k = idx % kDCTBlockSize;
      sp.old = img_->block(c, bix)[sp.k];
      sp.nz = acm_.nz[static_cast<size_t>(c) * num_blocks_ + bix];
      sp_log.emplace_back();
      ApplyNext(direction, bix, &sp_log.back());
      spec.push_back(sp);
      sp_comp.push_back(static_cast<uint8_t>(c));
      sp_key.push_back(it.TailKey(s));
    }
    // B, C: the histograms, the codes of every read step (on the pool),
    // the estimate and the break test; the changes past the break undone
    // (newest first; their journal entries stay: they name positions
    // whose values are current)
    const size_t done = RunSteps(it, i, j - i, sp_comp.data(), sp_log.data(), sp_key.data(), &stop);
    if (stop) {
      for (size_t u = j - i; u-- > done;) {
        const Spec& sp = spec[u];
        img_->block(sp_comp[u], sp.bix)[sp.k] = sp.old;
        acm_.nz[static_cast<size_t>(sp_comp[u]) * num_blocks_ + sp.bix] = sp.nz;
        last_indexes_[sp.bix] -= direction;
        if (LazyHost()) mat_li_[sp.bix] = last_indexes_[sp.bix];
      }
      res_->detail["backend_spec_undone"] += static_cast<double>(j - i - done);
    }
    i = j;
    if (!fixed_decades) decades = std::min(std::min(kMaxDecades, std::max(4, 2 * workers)), decades * 2);
  }
  return true;
}

// The tail on a partitioned frame, a window of entries at a time: the
// owners apply theirs tentatively and publish the symbol updates,
// every rank replays them in order into the frame's histograms and
// finds the break; the owners undo what lies past it.
// the window of order positions i0 .. i0 + W - 1 (frame blocks /
// keys); *done: positions processed (through the break if *stop)
bool BackEnd::TailWindow(Iteration& it, const int* blocks, const float* keys, size_t W, size_t i0, bool* stop,
                         size_t* done) {
  const int direction = it.direction;
  std::vector<uint8_t> rec;
  undo_.clear();
  for (size_t j = 0; j < W; ++j) {
    const int bix = blocks[j] - gbase_;
    if (bix < own_lo_ || bix >= own_hi_) continue;
    if (LazyHost()) Materialize(bix);  // (the undo records current values)
    const int off = std::max(0, std::min(offsets_[bix], static_cast<int>(cand_.size()) - 1));
    const int idx = cand_[off + last_indexes_[bix] + std::min(direction, 0)];
    const int c = idx / kDCTBlockSize, k = idx % kDCTBlockSize;
    undo_.push_back(Undo{i0 + j, bix, c, k, img_->block(c, bix)[k],
                         acm_.nz[static_cast<size_t>(c) * num_blocks_ + bix]});
    SymbolLog log;
    ApplyNext(direction, bix, &log);
    const uint32_t pos = static_cast<uint32_t>(j);
    rec.insert(rec.end(), reinterpret_cast<const uint8_t*>(&pos),
               reinterpret_cast<const uint8_t*>(&pos) + 4);
    rec.push_back(static_cast<uint8_t>(c));
    rec.push_back(log.n);
    for (int e = 0; e < log.n; ++e) {
      rec.push_back(log.sym[e]);
      rec.push_back(static_cast<uint8_t>(log.weight[e]));
    }
  }
  const auto tx = Clock::now();
  std::vector<std::vector<uint8_t>> all;
  if (!part_->coll->AllGatherV(rec, &all)) return false;
  res_->detail["strip_tail_exchange_s"] += Since(tx);
  std::vector<const uint8_t*> at(W, nullptr);
  for (const auto& m : all)
    for (const uint8_t* p = m.data(); p < m.data() + m.size();) {
      uint32_t pos;
      std::memcpy(&pos, p, 4);
      if (pos >= W) return false;
      at[pos] = p + 4;
      p += 6 + 2 * p[5];
    }
  // every rank runs the window's bookkeeping from the owners' symbol
  // updates (the speculative batches of the single-rank tail)
  std::vector<uint8_t> comp(W);
  std::vector<SymbolLog> logs(W);
  for (size_t q = 0; q < W; ++q) {
    const uint8_t* r = at[q];
    if (!r || r[1] > 32) return false;
    comp[q] = r[0];
    logs[q].n = r[1];
    for (int e = 0; e < r[1]; ++e) {
      logs[q].sym[e] = r[2 + 2 * e];
      logs[q].weight[e] = static_cast<int8_t>(r[3 + 2 * e]);
    }
  }
  size_t j = 0;
  for (size_t q0 = 0; q0 < W && !*stop;) {
    // (batches of about kMaxDecades rebuilds, ending before a read step)
    const size_t i = i0 + q0;
    const size_t first_code = (i + 9) / 10 * 10;
    const size_t q1 = std::min(W, first_code + 10 * 32 - i0);
    const size_t d = RunSteps(it, i, q1 - q0, comp.data() + q0, logs.data() + q0, keys + q0, stop);
    q0 += d;
    j = q0 - (*stop ? 1 : 0);
  }
  if (*stop) {
    for (auto u = undo_.rbegin(); u != undo_.rend() && u->i > i0 + j; ++u) {
      img_->block(u->c, u->bix)[u->k] = u->old;
      acm_.nz[static_cast<size_t>(u->c) * num_blocks_ + u->bix] = u->nz;
      last_indexes_[u->bix] -= direction;
      if (LazyHost()) mat_li_[u->bix] = last_indexes_[u->bix];
    }
  }
  *done = *stop ? j + 1 : W;
  return true;
}

// The tail on a split frame: windows of the frame's order from the
// iteration's source, each through TailWindow --
//   * kStripDevice: the device's windows of the frame's order (certified
//     positions); a window run out without a tie asks for the next, a tie or
//     an overflow switches to the exact order (every rank's entries);
//   * kStripFast: windows merged from every rank's next entries
//     (StripOrder::Next); positions whose entry the keys leave open (a tie
//     of several blocks) switch to the exact order;
//   * exact: chunks of std::sort's order, doubling from 4096 entries.
bool BackEnd::TailStrips(Iteration& it) {
  const size_t n_order = it.frame_n;
  const bool started_fast = it.source == Order::kStripFast && !it.exact;
  if (started_fast) strip_order_.StartTail(it.global_order, it.bulk > 0);
  std::vector<int> blocks;
  std::vector<float> keys;
  size_t exact_window = 4096;
  size_t i = it.bulk;
  bool stop = false;
  while (!stop && i < n_order) {
    size_t W = 0;
    bool open = false;  // (kStripFast) the position after this window starts a tie of several blocks
    const bool merged = !it.exact && it.source == Order::kStripFast;
    const char* timer = it.exact ? "strip_exact_window_s" : "strip_window_s";
    if (it.exact) {
      W = std::min(exact_window, n_order - i);
      exact_window *= 2;
      if (i + W > it.sorter->sorted()) {
        const auto ts = Clock::now();
        it.sorter->EnsureSorted(i + W - 1);
        it.sort_s += Since(ts);
      }
      blocks.resize(W);
      keys.resize(W);
      for (size_t j = 0; j < W; ++j) {
        blocks[j] = it.global_order[i + j].first;
        keys[j] = it.global_order[i + j].second;
      }
    } else if (merged) {
      const auto tn = Clock::now();
      const int r = strip_order_.Next(part_, &blocks, &keys, &open);
      res_->detail["strip_next_s"] += Since(tn);
      if (r < 0) return ExchangeFailed();
      if (r == 0) break;  // (no entries left on any rank)
      W = std::min(blocks.size(), n_order - i);
    } else {
      if (i >= it.win_base + it.win_ok) {
        bool failed = false;
        if (!NextDeviceWindow(it, i, &failed)) {
          if (failed) return Fail();
          if (!GoExact(it)) return ExchangeFailed();
          if (it.bulk) it.sorter->SetPrefix(it.bulk);
          res_->detail["backend_tail_exact"] += 1;
          continue;
        }
      }
      W = std::min(it.win_base + it.win_ok, n_order) - i;
      blocks.resize(W);
      keys.resize(W);
      for (size_t j = 0; j < W; ++j) {
        blocks[j] = it.win[i - it.win_base + j].first;
        keys[j] = it.win[i - it.win_base + j].second;
      }
    }
    size_t done = 0;
    const auto tw = Clock::now();
    if (W && !TailWindow(it, blocks.data(), keys.data(), W, i, &stop, &done)) return ExchangeFailed();
    res_->detail[timer] += Since(tw);
    i += done;
    if (merged) {
      strip_order_.Consumed(done);
      if (!stop && open) {
        if (!GoExact(it)) return ExchangeFailed();
        if (it.bulk) it.sorter->SetPrefix(it.bulk);
      }
    }
  }
  if (started_fast) res_->detail["strip_order_fast_iters"] += it.exact ? 0 : 1;
  return true;
}

bool Processor::SelectFrequencyBackEnd(const JpegData& jpg, CoeffImage* img, int comp_mask,
                                       double target_mul, bool stop_early,
                                       const std::vector<int>& offsets,
                                       const std::vector<uint8_t>& cand,
                                       const std::vector<float>& cand_err, std::string* err) {
  (void)comp_mask;
  return BackEnd(this, jpg, img, target_mul, stop_early, offsets, cand, cand_err, err).Run();
}

bool Processor::BuildChangeOrder(int direction, int factor, double target_mul, int num_blocks,
                                 int own_lo, int own_hi, int gbase, const std::vector<float>& bmax,
                                 const std::vector<int>& last_indexes, const std::vector<int>& offsets,
                                 const std::vector<float>& cand_err,
                                 const std::vector<float>& max_block_error,
                                 std::vector<std::pair<int, float>>* order,
                                 std::vector<float>* block_weight, int* blocks_to_change,
                                 size_t* frame_entries) {
  const int own_chunks = (own_hi - own_lo + kOrderChunk - 1) / kOrderChunk;
  const int cand_n = static_cast<int>(cand_err.size());
  std::vector<float>& weight = *block_weight;
  for (int rblock = 1; rblock <= 4; ++rblock) {
    weight.assign(num_blocks, 0.0f);
    cmp_->ComputeBlockErrorAdjustmentWeights(direction, rblock, target_mul, factor, factor, bmax, &weight);
    // entry counts per chunk of blocks, their prefix sums, then each chunk
    // fills its own range
    std::vector<size_t> chunk_start(own_chunks + 1, 0);
    std::vector<int> chunk_btc(own_chunks, 0);
    auto block_entries = [&](int bix) -> int {
      if (weight[bix] == 0) return 0;
      const int last_index = last_indexes[bix];
      const int offset = std::max(0, std::min(offsets[bix], cand_n - 1));
      const int num_candidates = offsets[bix + 1] - offset;
      return direction > 0 ? std::max(0, num_candidates - last_index) : last_index;
    };
    ParallelFor(own_chunks, [&](int ch) {
      size_t n = 0;
      int btc = 0;
      for (int bix = own_lo + ch * kOrderChunk; bix < std::min(own_hi, own_lo + (ch + 1) * kOrderChunk); ++bix) {
        const int e = block_entries(bix);
        n += e;
        btc += e > 0 ? 1 : 0;
      }
      chunk_start[ch + 1] = n;
      chunk_btc[ch] = btc;
    });
    *blocks_to_change = 0;
    for (int ch = 0; ch < own_chunks; ++ch) {
      chunk_start[ch + 1] += chunk_start[ch];
      *blocks_to_change += chunk_btc[ch];
    }
    order->resize(chunk_start[own_chunks]);
    ParallelFor(own_chunks, [&](int ch) {
      std::pair<int, float>* out = order->data() + chunk_start[ch];
      for (int bix = own_lo + ch * kOrderChunk; bix < std::min(own_hi, own_lo + (ch + 1) * kOrderChunk); ++bix) {
        if (weight[bix] == 0) continue;
        const int last_index = last_indexes[bix];
        const int offset = std::max(0, std::min(offsets[bix], cand_n - 1));
        const int num_candidates = offsets[bix + 1] - offset;
        const float* errs = cand_err.data() + offset;
        const float max_err = max_block_error[bix];
        const int g = gbase + bix;
        if (direction > 0) {
          for (int i = last_index; i < num_candidates; ++i)
            *out++ = std::make_pair(g, (errs[i] - max_err) / weight[bix]);
        } else {
          for (int i = last_index - 1; i >= 0; --i)
            *out++ = std::make_pair(g, (max_err - errs[i]) / weight[bix]);
        }
      }
    });
    if (part_ && part_->world > 1 && frame_entries) {
      // this rank's entries only (StripOrder); the frame's totals
      int64_t t[2] = {static_cast<int64_t>(order->size()), *blocks_to_change};
      if (!part_->SumAll(t, 2)) return false;
      *frame_entries = static_cast<size_t>(t[0]);
      *blocks_to_change = static_cast<int>(t[1]);
      if (t[0] > 0) break;
      continue;
    }
    if (part_ && part_->world > 1) {
      // the frame's order: every rank's entries in rank (= block) order; a
      // rank sends its keys and a count per owned block
      const auto tx = Clock::now();
      if (!GatherEntries(order, own_lo, own_hi, gbase, blocks_to_change)) return false;
      res_->detail["strip_entries_s"] += Since(tx);
    }
    if (!order->empty()) break;
  }
  return true;
}

// The frame's change entries of one back-end iteration from every rank's
// owned ones (each rank sends its keys and an entry count per owned block;
// the pairs are rebuilt in rank order, which is block order).  *entries holds
// this rank's on entry, the frame's on return; *blocks_to_change becomes the
// frame's count.  Packing and unpacking run on the host pool.
bool Processor::GatherEntries(std::vector<std::pair<int, float>>* entries, int own_lo, int own_hi,
                              int gbase, int* blocks_to_change) {
  const int nown = own_hi - own_lo;
  const size_t n = entries->size();
  std::vector<uint8_t> send(8 + nown + n * 4, 0);
  const uint32_t n32 = static_cast<uint32_t>(n), btc = static_cast<uint32_t>(*blocks_to_change);
  std::memcpy(send.data(), &n32, 4);
  std::memcpy(send.data() + 4, &btc, 4);
  uint8_t* cnt = send.data() + 8;
  uint8_t* keys = send.data() + 8 + nown;
  constexpr int kSlices = 64;
  ParallelFor(kSlices, [&](int sl) {
    // (entries of one block are contiguous; a slice counts the blocks whose
    // first entry it holds, through the block's end)
    size_t i = n * sl / kSlices;
    const size_t end = n * (sl + 1) / kSlices;
    if (i > 0)
      while (i < end && (*entries)[i].first == (*entries)[i - 1].first) ++i;
    while (i < end) {
      const int b = (*entries)[i].first;
      size_t k = i;
      while (k < n && (*entries)[k].first == b) {
        std::memcpy(keys + 4 * k, &(*entries)[k].second, 4);
        ++k;
      }
      cnt[b - gbase - own_lo] = static_cast<uint8_t>(k - i);
      i = k;
    }
  });
  std::vector<std::vector<uint8_t>> all;
  if (!part_->coll->AllGatherV(send, &all)) return false;
  const int world = part_->world, bw = part_->bw;
  std::vector<size_t> rank_at(world + 1, 0);
  int frame_btc = 0;
  for (int r = 0; r < world; ++r) {
    uint32_t v;
    std::memcpy(&v, all[r].data(), 4);
    rank_at[r + 1] = rank_at[r] + v;
    std::memcpy(&v, all[r].data() + 4, 4);
    frame_btc += static_cast<int>(v);
  }
  entries->resize(rank_at[world]);
  // work items: (rank, 4096-block chunk), each filling its own range
  constexpr int kChunk = 4096;
  std::vector<std::pair<int, int>> items;
  std::vector<size_t> item_at;
  for (int r = 0; r < world; ++r) {
    const int nb = (part_->row0[r + 1] - part_->row0[r]) * bw;
    const uint8_t* c = all[r].data() + 8;
    size_t at = rank_at[r];
    for (int b0 = 0; b0 < nb; b0 += kChunk) {
      items.emplace_back(r, b0);
      item_at.push_back(at);
      for (int b = b0; b < std::min(nb, b0 + kChunk); ++b) at += c[b];
    }
  }
  ParallelFor(static_cast<int>(items.size()), [&](int it) {
    const int r = items[it].first, b0 = items[it].second;
    const int nb = (part_->row0[r + 1] - part_->row0[r]) * bw, base = part_->row0[r] * bw;
    const uint8_t* c = all[r].data() + 8;
    size_t at = item_at[it];
    const uint8_t* k = all[r].data() + 8 + nb + 4 * (at - rank_at[r]);
    for (int b = b0; b < std::min(nb, b0 + kChunk); ++b)
      for (int j = 0; j < c[b]; ++j, ++at, k += 4) {
        float key;
        std::memcpy(&key, k, 4);
        (*entries)[at] = std::make_pair(base + b, key);
      }
  });
  *blocks_to_change = frame_btc;
  return true;
}

}  // namespace gz
