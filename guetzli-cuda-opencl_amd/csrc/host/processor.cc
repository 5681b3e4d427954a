// Portions restate Guetzli (Copyright 2016 Google Inc., Apache License 2.0,
// http://www.apache.org/licenses/LICENSE-2.0) as modified in
// yyamamoto79/guetzli-cuda-opencl: processor.cc, quality.cc, score.cc and butteraugli_comparator.cc
// (QuantMatrixGenerator, the back end's control flow, kLocalMaxWeight).
// Byte-exact output forces their operation order and constants; the
// code around them is this repository's own.
// The Guetzli search loop on the host (guetzli/processor.cc), driving the GPU
// comparator.  Control flow, heuristics and every floating-point decision are
// those of the reference's CPU_OPT (`guetzli --c`) path so the output bytes
// are identical; only the expensive work (Butteraugli passes, per-block
// greedy zeroing, global quantization) runs on the device.
#include "host/processor_impl.h"

#include <algorithm>
#include <limits>
#include <time.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <thread>
#include <utility>

#include <hip/hip_runtime.h>

#include "guetzli_hip.h"
#include "host/jpeg_encode.h"
#include "host/jpeg_reader.h"
#include "host/jpeg_writer.h"
#include "host/lazy_sort.h"
#include "host/thread_pool.h"

namespace gz {

// ---------------------------------------------------------------------------
// quality.cc / score.cc
// ---------------------------------------------------------------------------

double ButteraugliScoreForQuality(double quality) {
  static const double kScoreForQuality[] = {
      2.810761, 2.729300, 2.689687, 2.636811, 2.547863, 2.525400, 2.473416, 2.366133, 2.338078,
      2.318654, 2.201674, 2.145517, 2.087322, 2.009328, 1.945456, 1.900112, 1.805701, 1.750194,
      1.644175, 1.562165, 1.473608, 1.382021, 1.294298, 1.185402, 1.066781, 0.971769, 0.852901,
      0.724544, 0.611302, 0.443185, 0.211578, 0.209462, 0.207346, 0.205230, 0.203114, 0.200999,
      0.198883, 0.196767, 0.194651, 0.192535, 0.190420, 0.190420,
  };
  const int kLowest = 70, kHighest = 110;
  if (quality < kLowest) quality = kLowest;
  if (quality > kHighest) quality = kHighest;
  const int index = static_cast<int>(quality);
  const double mix = quality - index;
  return kScoreForQuality[index - kLowest] * (1 - mix) + kScoreForQuality[index - kLowest + 1] * mix;
}

double ScoreJPEG(double distance, int size, double target) {
  const double kScale = 50, kMaxExponent = 10, kLargeSize = 1e30;
  const double diff = distance - target;
  if (diff <= 0.0) return size;
  const double exponent = kScale * diff;
  if (exponent > kMaxExponent) return kLargeSize * std::exp(kMaxExponent) * diff + size;
  return std::exp(exponent) * size;
}

// ---------------------------------------------------------------------------
// Processor
// ---------------------------------------------------------------------------

namespace {


double ContrastSensitivity(int k) { return 1.0 / (1.0 + kJPEGZigZagOrder[k] / 2.0); }

double QuantMatrixHeuristicScore(const int q[3][kDCTBlockSize]) {
  double score = 0.0;
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < kDCTBlockSize; ++k) score += 0.5 * (q[c][k] - 1.0) * ContrastSensitivity(k);
  return score;
}

// -1 / 0 / 1 / 2 ordering of two quant matrices (processor.cc:168-190).
int CompareQuantMatrices(const int* a, const int* b) {
  const int n = 3 * kDCTBlockSize;
  int i = 0;
  while (i < n && a[i] == b[i]) ++i;
  if (i == n) return 0;
  if (a[i] < b[i]) {
    for (++i; i < n; ++i)
      if (a[i] > b[i]) return 2;
    return -1;
  }
  for (++i; i < n; ++i)
    if (a[i] < b[i]) return 2;
  return 1;
}

bool CompareQuantData(const QuantData& a, const QuantData& b) {
  if (a.dist_ok && !b.dist_ok) return true;
  if (!a.dist_ok && b.dist_ok) return false;
  return a.jpg_size < b.jpg_size;
}

// Binary search over the heuristic quantization "score" (processor.cc:206-308).
class QuantMatrixGenerator {
 public:
  explicit QuantMatrixGenerator(bool downsample = false) : downsample_(downsample) {
    for (int k = 0; k < kDCTBlockSize; ++k) total_csf_ += 3.0 * ContrastSensitivity(k);
  }
  bool GetNext(int q[3][kDCTBlockSize]) {
    for (int iter = 0; iter < 1000; iter++) {
      double hscore;
      if (hscore_b_ == -1.0) {
        if (hscore_a_ == -1.0) {
          hscore = downsample_ ? 0.0 : total_csf_;
        } else if (hscore_a_ < 5.0 * total_csf_) {
          hscore = hscore_a_ + total_csf_;
        } else {
          hscore = 2 * (hscore_a_ + total_csf_);
        }
        if (hscore > 100 * total_csf_) return false;
      } else if (hscore_b_ == 0.0) {
        return false;
      } else if (hscore_a_ == -1.0) {
        hscore = 0.0;
      } else {
        int lower_q[3][kDCTBlockSize], upper_q[3][kDCTBlockSize];
        constexpr double kEps = 0.05;
        MatrixForScore((1 - kEps) * hscore_a_ + kEps * 0.5 * (hscore_a_ + hscore_b_), lower_q);
        MatrixForScore((1 - kEps) * hscore_b_ + kEps * 0.5 * (hscore_a_ + hscore_b_), upper_q);
        if (CompareQuantMatrices(&lower_q[0][0], &upper_q[0][0]) == 0) return false;
        hscore = (hscore_a_ + hscore_b_) * 0.5;
      }
      MatrixForScore(hscore, q);
      bool retry = false;
      for (const QuantData& d : quants_) {
        if (CompareQuantMatrices(&q[0][0], &d.q[0][0]) == 0) {
          if (d.dist_ok) hscore_a_ = hscore; else hscore_b_ = hscore;
          retry = true;
          break;
        }
      }
      if (!retry) return true;
    }
    return false;
  }
  void Add(const QuantData& d) {
    quants_.push_back(d);
    const double hscore = QuantMatrixHeuristicScore(d.q);
    if (d.dist_ok) hscore_a_ = std::max(hscore_a_, hscore);
    else hscore_b_ = hscore_b_ == -1.0 ? hscore : std::min(hscore_b_, hscore);
  }

 private:
  void MatrixForScore(double score, int q[3][kDCTBlockSize]) const {
    const int level = static_cast<int>(score / total_csf_);
    score -= level * total_csf_;
    for (int k = kDCTBlockSize - 1; k >= 0; --k) {
      for (int c = 0; c < 3; ++c) q[c][kJPEGNaturalOrder[k]] = 2 * level + (score > 0.0 ? 3 : 1);
      score -= 3.0 * ContrastSensitivity(kJPEGNaturalOrder[k]);
    }
  }
  bool downsample_;
  double hscore_a_ = -1.0, hscore_b_ = -1.0, total_csf_ = 0.0;
  std::vector<QuantData> quants_;
};

}  // namespace

bool Processor::TryQuantMatrix(const JpegData& jpg_in, float target_mul,
                               const int q[3][kDCTBlockSize], CoeffImage* img, QuantData* data,
                               std::string* err) {
  // processor.cc:310-338
  std::memcpy(data->q, q, sizeof(data->q));
  const auto tq = Clock::now();
  if (!cmp_->QuantizeFromOriginal(q, img, /*need_host=*/!cmp_->HasDeviceWriter())) return Fail(err);
  res_->seconds_quantize += Since(tq);
  ++res_->iterations;
  if (!EncodeAndCompare(jpg_in, *img, err)) return false;
  data->dist_ok = cmp_->DistanceOK(target_mul);
  data->jpg_size = FlushOutput();
  return true;
}

bool Processor::SelectQuantMatrix(const JpegData& jpg_in, bool downsample,
                                  int best_q[3][kDCTBlockSize], CoeffImage* img, bool* ok,
                                  std::string* err) {
  // processor.cc:340-372
  QuantMatrixGenerator qgen(downsample);
  const float target_mul_high = 0.97f, target_mul_low = 0.95f;
  QuantData best;
  if (!TryQuantMatrix(jpg_in, target_mul_high, best_q, img, &best, err)) return false;
  for (;;) {
    int q_next[3][kDCTBlockSize];
    if (!qgen.GetNext(q_next)) break;
    QuantData data;
    if (!TryQuantMatrix(jpg_in, target_mul_high, q_next, img, &data, err)) return false;
    qgen.Add(data);
    if (CompareQuantData(data, best)) {
      best = data;
      if (data.dist_ok && !cmp_->DistanceOK(target_mul_low)) break;
    }
  }
  std::memcpy(best_q, best.q, sizeof(best.q));
  *ok = best.dist_ok;
  return true;
}

bool Processor::SelectFrequencyMasking(const JpegData& jpg, CoeffImage* img, int comp_mask,
                                       double target_mul, bool stop_early, std::string* err) {
  // processor.cc:559-721 (the CPU_OPT loop runs as one batched device call)
  if (!cmp_->StartBlockComparisons()) return Fail(err);
  std::vector<int> offsets;
  std::vector<uint8_t> cand;
  std::vector<float> cand_err;
  if (!cmp_->BlockZeroingCandidates(*img, jpg, comp_mask, params_.zeroing_greedy_lookahead,
                                    params_.new_zeroing_model,
                                    &offsets, &cand, &cand_err))
    return Fail(err);
  cmp_->FinishBlockComparisons();
  res_->detail["candidates"] = static_cast<double>(cand.size());
  const double c0 = ThreadCpu();
  const bool ok = SelectFrequencyBackEnd(jpg, img, comp_mask, target_mul, stop_early, offsets, cand,
                                         cand_err, err);
  res_->detail["backend_thread_cpu_s"] += ThreadCpu() - c0;
  return ok;
}

namespace {

// RemoveOriginalQuantization, processor.cc:94-107: coefficients times their
// quantization, quant tables of ones; q_in receives the originals.
void RemoveOriginalQuantization(JpegData* jpg, int q_in[3][kDCTBlockSize]) {
  for (int i = 0; i < 3; ++i) {
    JpegComponent& c = jpg->components[i];
    const int* q = jpg->quant[c.quant_idx].values;
    std::memcpy(q_in[i], q, sizeof(q_in[i]));
    bool ones = true;  // (RGB input: the q=1 originals -- nothing to multiply)
    for (int k = 0; k < kDCTBlockSize; ++k) ones = ones && q[k] == 1;
    if (ones) continue;
    for (size_t j = 0; j < c.coeffs.size(); ++j) c.coeffs[j] = static_cast<coeff_t>(c.coeffs[j] * q[j % 64]);
  }
  int ones[3][kDCTBlockSize];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < kDCTBlockSize; ++j) ones[i][j] = 1;
  SaveQuantTables(ones, jpg);
}

// IsGrayscale, processor.cc:921-929
// The 4:4:4 JpegData of a 4:2:0 one whose chroma is all zero: Y cropped to
// the image's blocks (a 4:2:0 file pads it to whole 16-pixel MCUs), chroma
// zero at full resolution.
JpegData Gray444Of420(const JpegData& jpg) {
  JpegData g = jpg;
  const int bw = (jpg.width + 7) / 8, bh = (jpg.height + 7) / 8;
  g.max_h_samp_factor = g.max_v_samp_factor = 1;
  g.mcu_cols = bw;
  g.mcu_rows = bh;
  for (int c = 0; c < 3; ++c) {
    JpegComponent& comp = g.components[c];
    comp.h_samp_factor = comp.v_samp_factor = 1;
    comp.width_in_blocks = bw;
    comp.height_in_blocks = bh;
    comp.coeffs.assign(static_cast<size_t>(bw) * bh * kDCTBlockSize, 0);
    if (c != 0) continue;
    const JpegComponent& y = jpg.components[0];
    for (int by = 0; by < bh; ++by)
      std::memcpy(&comp.coeffs[static_cast<size_t>(by) * bw * kDCTBlockSize],
                  &y.coeffs[static_cast<size_t>(by) * y.width_in_blocks * kDCTBlockSize],
                  static_cast<size_t>(bw) * kDCTBlockSize * sizeof(coeff_t));
  }
  return g;
}

bool IsGrayscale(const JpegData& jpg) {
  for (int c = 1; c < 3; ++c)
    for (coeff_t v : jpg.components[c].coeffs)
      if (v != 0) return false;
  return true;
}

// UpdateACHistogram, processor.cc:491-515
void UpdateACHistogram(int weight, const coeff_t* coeffs, const int* q, JpegHistogram* h) {
  int r = 0;
  for (int k = 1; k < 64; ++k) {
    const int k_nat = kJPEGNaturalOrder[k];
    const coeff_t coeff = coeffs[k_nat];
    if (coeff == 0) {
      ++r;
      continue;
    }
    while (r > 15) {
      h->Add(0xf0, weight);
      r -= 16;
    }
    h->Add((r << 4) + Log2FloorNonZero(std::abs(coeff / q[k_nat])) + 1, weight);
    r = 0;
  }
  if (r > 0) h->Add(0, weight);
}

}  // namespace

int Processor::Run(const JpegData& jpg_in, std::string* err) {
  // ProcessJpegData, processor.cc:931-1020
  if (params_.butteraugli_target > 2.0f) {
    if (err) *err = "butteraugli target above 2.0 (quality below 84) is not supported";
    return GZ_ERR_INVALID_ARG;
  }
  if (jpg_in.components.size() != 3 || !HasYCbCrColorSpace(jpg_in)) {
    if (err) *err = "Only YUV color space input jpeg is supported";
    return GZ_ERR_UNSUPPORTED;
  }
  const bool input_is_420 = JpegIs420(jpg_in);
  if (!input_is_420 && !JpegIs444(jpg_in)) {
    if (err) *err = "Unsupported sampling factors";
    return GZ_ERR_UNSUPPORTED;
  }
  // The original's output (processor.cc:965-967) is written here on the
  // host unless the device coder can give it (DeviceEncodeOriginalAndCompare)
  std::string encoded;
  bool ones = true;
  for (const QuantTable& t : jpg_in.quant)
    for (int k = 0; k < kDCTBlockSize; ++k) ones = ones && t.values[k] == 1;
  const bool orig_on_device = cmp_ && cmp_->HasDeviceWriter() && !input_is_420 && ones;
  if (!orig_on_device) OutputJpeg(jpg_in, &encoded);
  final_score_ = -1;
  if (cmp_ == nullptr) {  // image too small for Butteraugli
    res_->jpeg = encoded;
    return GZ_OK;
  }
  int q_in[3][kDCTBlockSize];
  JpegData jpg = jpg_in;
  RemoveOriginalQuantization(&jpg, q_in);
  auto device_error = [&]() {
    Fail(err);
    return GZ_ERR_DEVICE;
  };
  CoeffImage img;
  // A 4:2:0 input whose chroma is all zero: DownsampleImage leaves it and
  // SaveToJpegData keeps its one component (processor.cc:990-1016), so its
  // search is the grayscale pass below on the 4:4:4 image it equals (zero
  // chroma upsamples to the same pixels at either factor)
  const bool gray420 = input_is_420 && IsGrayscale(jpg);
  JpegData jpg444;
  if (!input_is_420) {
    if (!cmp_->SetOriginalCoeffs(jpg)) return device_error();
    img.Init(jpg.width, jpg.height);
    img.CopyFromJpegData(jpg);
    if (orig_on_device) {
      size_t size = 0;
      bool used = false;
      if (!cmp_->DeviceEncodeOriginalAndCompare(img, jpg_in, params_.clear_metadata, &size, &used))
        return device_error();
      if (used) {
        MaybeOutputDevice(size);  // the first output: always kept
        if (getenv("GZ_CHECK_ORIGINAL_OUTPUT")) {  // test hook: bytes vs the host writer
          std::string host, dev;
          OutputJpeg(jpg_in, &host);
          if (!cmp_->DeviceFetchKept(&dev)) return device_error();
          if (host != dev || host.size() != size) {
            if (err) *err = "device-coded original output differs from the host writer's";
            return GZ_ERR_INTERNAL;
          }
        }
      } else {
        OutputJpeg(jpg_in, &encoded);
        MaybeOutput(encoded);
      }
    } else {
      if (!cmp_->Compare(img)) return device_error();
      MaybeOutput(encoded);
    }
  } else {
    Image420 im;
    im.Init(jpg.width, jpg.height);
    im.CopyFromJpegData(jpg);
    if (!cmp_->Compare420(im)) return device_error();
    MaybeOutput(encoded);
  }
  const int try_420 = (input_is_420 || params_.force_420 || (params_.try_420 && !IsGrayscale(jpg_in))) ? 1 : 0;
  const int force_420 = (input_is_420 || params_.force_420) ? 1 : 0;
  // DownsampleImage leaves an image whose chroma is all zero at 4:4:4
  // (output_image.cc:535-539) and SaveToJpegData keeps its one component, so
  // the "4:2:0" pass of such an image is the 4:4:4 machinery on a
  // one-component JpegData: the downsampling quantization generator, then the
  // Y search alone with ymul 1.0 (processor.cc:994-1016).
  const bool gray_pass = (!input_is_420 || gray420) && IsGrayscale(jpg);
  if (gray420) {  // (after the 4:2:0 Compare of the input above)
    jpg444 = Gray444Of420(jpg);
    if (!cmp_->SetOriginalCoeffs(jpg444)) return device_error();
    img.Init(jpg.width, jpg.height);
  }
  for (int downsample = force_420; downsample <= try_420; ++downsample) {
    if (downsample && !gray_pass) {
      const int rc = Run420(jpg_in, err);
      if (rc != GZ_OK) return rc;
      continue;
    }
    const JpegData& src = gray420 ? jpg444 : jpg;
    JpegData gray;
    const JpegData* pass_jpg = &src;
    if (downsample) {
      gray = src;
      gray.components.resize(1);
      pass_jpg = &gray;
    }
    img.CopyFromJpegData(src);
    int best_q[3][kDCTBlockSize];
    std::memcpy(best_q, q_in, sizeof(best_q));
    bool ok = false;
    if (!SelectQuantMatrix(*pass_jpg, downsample != 0, best_q, &img, &ok, err)) return GZ_ERR_DEVICE;
    if (!ok)
      for (int c = 0; c < 3; ++c)
        for (int i = 0; i < kDCTBlockSize; ++i) best_q[c][i] = 1;
    if (!cmp_->QuantizeFromOriginal(best_q, &img)) return device_error();
    if (!SelectFrequencyMasking(*pass_jpg, &img, downsample ? 1 : 7, 1.0, false, err))
      return GZ_ERR_DEVICE;
  }
  FlushOutput();
  if (kept_on_device_ && !cmp_->DeviceFetchKept(&res_->jpeg)) return device_error();
  return GZ_OK;
}

int Processor::Run420(const JpegData& jpg_in, std::string* err) {
  // processor.cc:990-1016 with downsample = 1
  FlushOutput();
  int q_in[3][kDCTBlockSize];
  JpegData jpg = jpg_in;
  RemoveOriginalQuantization(&jpg, q_in);
  JpegData jpg420;
  if (JpegIs420(jpg)) {
    // already subsampled (DownsampleImage leaves it): OutputImage of it,
    // saved back (whole MCUs, padding blocks re-derived)
    Image420 t;
    t.Init(jpg.width, jpg.height);
    t.CopyFromJpegData(jpg);
    jpg420.app_data = jpg.app_data;
    jpg420.com_data = jpg.com_data;
    t.SaveToJpegData(&jpg420);
  } else if (!DownsampleToJpegData420(jpg, params_.use_silver_screen, &jpg420)) {
    // (all-zero chroma: the reference keeps 4:4:4 and continues with one
    // grayscale component)
    if (err) *err = "4:2:0 pass of an image without chroma is not supported";
    return GZ_ERR_UNSUPPORTED;
  }
  if (jpg420.components.size() != 3) {
    if (err) *err = "4:2:0 pass of an image without chroma is not supported";
    return GZ_ERR_UNSUPPORTED;
  }
  auto device_error = [&]() {
    Fail(err);
    return GZ_ERR_DEVICE;
  };
  if (!cmp_->SetOriginalCoeffs420(jpg420)) return device_error();
  Image420 img;
  // (a candidate's bytes may still be in the writer thread, which reads
  // img's saved JpegData: joined before img goes out of scope on every
  // return -- the normal one applies its MaybeOutput first, below)
  struct JoinWriter {
    std::thread* t;
    ~JoinWriter() {
      if (t->joinable()) t->join();
    }
  } join_writer{&writer_};
  img.Init(jpg420.width, jpg420.height);
  // SelectQuantMatrix (processor.cc:340-372) with the downsampling generator
  int best_q[3][kDCTBlockSize];
  std::memcpy(best_q, q_in, sizeof(best_q));
  {
    QuantMatrixGenerator qgen(true);
    const float target_mul_high = 0.97f, target_mul_low = 0.95f;
    QuantData best;
    if (!TryQuantMatrix420(jpg420, target_mul_high, best_q, &img, &best, err)) return GZ_ERR_DEVICE;
    for (;;) {
      int q_next[3][kDCTBlockSize];
      if (!qgen.GetNext(q_next)) break;
      QuantData data;
      if (!TryQuantMatrix420(jpg420, target_mul_high, q_next, &img, &data, err)) return GZ_ERR_DEVICE;
      qgen.Add(data);
      if (CompareQuantData(data, best)) {
        best = data;
        if (data.dist_ok && !cmp_->DistanceOK(target_mul_low)) break;
      }
    }
    std::memcpy(best_q, best.q, sizeof(best.q));
    if (!best.dist_ok)
      for (int c = 0; c < 3; ++c)
        for (int i = 0; i < kDCTBlockSize; ++i) best_q[c][i] = 1;
  }
  const auto tq = Clock::now();
  img.CopyFromJpegData(jpg420);
  img.ApplyGlobalQuantization(best_q);
  res_->seconds_quantize += Since(tq);
  if (!SelectFrequencyMasking420(jpg420, &img, 1, 0.97f, false, err)) return GZ_ERR_DEVICE;
  if (!SelectFrequencyMasking420(jpg420, &img, 6, 1.0, true, err)) return GZ_ERR_DEVICE;
  FlushOutput();  // (the last candidate's MaybeOutput, with its own Compare's distance)
  return GZ_OK;
}

bool Processor::TryQuantMatrix420(const JpegData& jpg, float target_mul, const int q[3][kDCTBlockSize],
                                  Image420* img, QuantData* data, std::string* err) {
  // processor.cc:310-338
  std::memcpy(data->q, q, sizeof(data->q));
  const auto tq = Clock::now();
  img->CopyFromJpegData(jpg);
  img->ApplyGlobalQuantization(q);
  res_->seconds_quantize += Since(tq);
  FlushOutput();
  // the candidate's bytes on a helper thread while its Compare runs (the
  // size is needed at once: joined before the return)
  const auto te = Clock::now();
  const JpegData& out = img->SavedJpegData(jpg);
  res_->detail["r420_stage_s"] += Since(te);
  std::string encoded;
  double enc_s = 0.0;
  std::thread wr([&] {
    const auto t = Clock::now();
    WriteJpeg(out, params_.clear_metadata, &encoded);
    enc_s = Since(t);
  });
  ++res_->iterations;
  const auto tc = Clock::now();
  const bool ok = cmp_->Compare420(*img);
  res_->detail["r420_compare_s"] += Since(tc);
  const auto tw = Clock::now();
  wr.join();
  res_->detail["write_wait_s"] += Since(tw);
  res_->seconds_write += enc_s;
  res_->detail["write_jpeg_s"] += enc_s;
  if (!ok) return Fail(err);
  data->dist_ok = cmp_->DistanceOK(target_mul);
  data->jpg_size = encoded.size();
  MaybeOutput(encoded);
  return true;
}

// A 4:2:0 back-end candidate's output (processor.cc:899-904 after the
// iteration's changes): its bytes formed on the helper thread while the
// Compare that scores it and the next iteration's selection run;
// FlushOutput applies its MaybeOutput before the next Compare.
void Processor::BeginOutput420(const JpegData& jpg, Image420* img) {
  FlushOutput();
  const auto te = Clock::now();
  const JpegData& out = img->SavedJpegData(jpg);
  res_->detail["r420_stage_s"] += Since(te);
  pending_.clear();
  pending_device_ = false;
  pending_skipped_ = false;
  writer_ = std::thread([this, &out] {
    const auto t = Clock::now();
    WriteJpeg(out, params_.clear_metadata, &pending_);
    encode_s_ = Since(t);
  });
  has_pending_ = true;
}

bool Processor::SelectFrequencyMasking420(const JpegData& jpg, Image420* img, int comp_mask,
                                          double target_mul, bool stop_early, std::string* err) {
  // processor.cc:559-721 and the back end :723-919 for one pass of the 4:2:0
  // image (comp_mask 1: Y at factor 1; 6: Cb + Cr at factor 2), serial as
  // in the reference
  const int ncomp = static_cast<int>(jpg.components.size());
  const int last_c = Log2FloorNonZero(static_cast<uint32_t>(comp_mask));
  if (last_c >= ncomp) return true;
  const int factor = last_c == 0 ? 1 : 2;
  const int w = img->w, h = img->h;
  const int block_width = (w + 8 * factor - 1) / (8 * factor);
  const int block_height = (h + 8 * factor - 1) / (8 * factor);
  const int num_blocks = block_width * block_height;
  FlushOutput();  // (the last candidate's MaybeOutput sees its own Compare's distance)
  const auto tz = Clock::now();
  if (!cmp_->StartBlockComparisons()) return Fail(err);
  std::vector<int> offsets;
  std::vector<uint8_t> cand;
  std::vector<float> cand_err;
  if (!cmp_->BlockZeroingCandidates420(img, comp_mask, params_.zeroing_greedy_lookahead,
                                       params_.new_zeroing_model, &offsets, &cand, &cand_err))
    return Fail(err);
  cmp_->FinishBlockComparisons();
  res_->detail[comp_mask == 1 ? "r420_zeroing_y_s" : "r420_zeroing_c_s"] += Since(tz);
  res_->detail["candidates"] += static_cast<double>(cand.size());
  const auto tb0 = Clock::now();
  std::vector<JpegHistogram> ac_histograms(ncomp);
  int jpg_header_size, dc_size;
  {
    JpegData out;
    out.app_data = jpg.app_data;
    out.com_data = jpg.com_data;
    img->SaveToJpegData(&out);
    jpg_header_size = static_cast<int>(JpegHeaderSize(out, params_.clear_metadata));
    std::vector<JpegHistogram> dc(out.components.size());
    BuildDCHistograms(out, dc.data());
    size_t num = dc.size();
    std::vector<int> idx(num);
    std::vector<uint8_t> depths(num * JpegHistogram::kSize);
    dc_size = static_cast<int>(ClusterHistograms(dc.data(), &num, idx.data(), depths.data()));
    ac_histograms.resize(out.components.size());
    BuildACHistograms(out, ac_histograms.data());
  }
  std::vector<uint8_t> ac_depths;
  int ac_histogram_size = static_cast<int>(ComputeEntropyCodes(ac_histograms, &ac_depths));
  const int base_size = jpg_header_size + dc_size + ac_histogram_size +
                        static_cast<int>(EntropyCodedDataSize(ac_histograms, ac_depths));
  int prev_size = base_size;
  std::vector<float> max_block_error(num_blocks, 0.0f);
  std::vector<int> last_indexes(num_blocks, 0);
  // (a change's symbol updates from its neighbours in zigzag order, as the
  // 4:4:4 back end; UpdateACHistogram's two passes over the block give the
  // same counts)
  AcBlockModel acm;
  size_t acm_base[3];
  acm.Build(*img, acm_base);
  size_t chroma_updates = 0;
  res_->seconds_backend += Since(tb0);
  bool first_up_iter = true;
  for (int direction : {1, -1}) {
    for (;;) {
      if (stop_early && direction == -1) {
        FlushOutput();
        if (prev_size > 1.01 * best_size_) break;
      }
      const auto tb = Clock::now();
      std::vector<std::pair<int, float>> global_order;
      int blocks_to_change = 0;
      std::vector<float> block_weight;
      // the distance map's maximum per searched block (all zero on the first
      // up iteration, processor.cc:777-780)
      std::vector<float> bmax(num_blocks, 0.0f);
      if (!first_up_iter) {
        const std::vector<float>& m8 = cmp_->block_max_distance();
        if (cmp_->block_max_failed()) return Fail(err);
        const int bw8 = (w + 7) / 8, bh8 = (h + 7) / 8;
        for (int by = 0; by < bh8; ++by)
          for (int bx = 0; bx < bw8; ++bx) {
            float& d = bmax[(by / factor) * block_width + bx / factor];
            d = std::max(d, m8[by * bw8 + bx]);
          }
      }
      if (!BuildChangeOrder(direction, factor, target_mul, num_blocks, 0, num_blocks, 0, bmax,
                            last_indexes, offsets, cand_err, max_block_error, &global_order,
                            &block_weight, &blocks_to_change))
        return Fail(err);
      res_->detail["r420_order_s"] += Since(tb);
      if (global_order.empty()) {
        res_->seconds_backend += Since(tb);
        break;
      }
      // std::sort(global_order) (processor.cc:825-828), materialised lazily:
      // only the prefix the change loop consumes gets sorted (host/lazy_sort.h)
      LazyStdSort sorter(global_order.data(), global_order.size());
      ChangeLoop loop(direction, cmp_->DistanceOK(1.0), base_size, factor, blocks_to_change,
                      &first_up_iter, cmp_->BlockErrorLimit(), global_order);
      int est_jpg_size = prev_size;
      const size_t n_order = global_order.size();
      for (size_t i = 0; i < n_order; ++i) {
        if (i >= sorter.sorted()) sorter.EnsureSorted(i);
        const int bix = global_order[i].first;
        const int bx = bix % block_width, by = bix / block_width;
        const int last_idx = last_indexes[bix];
        const int offset = std::max(0, std::min(offsets[bix], static_cast<int>(cand.size()) - 1));
        const int idx = cand[offset + last_idx + std::min(direction, 0)];
        const int c = idx / kDCTBlockSize, k = idx % kDCTBlockSize;
        const int* quant = img->quant[c];
        const JpegComponent& comp = jpg.components[c];
        const int jpg_bix = by * comp.width_in_blocks + bx;
        const int newval =
            direction > 0 ? 0 : QuantizeCoeff(comp.coeffs[static_cast<size_t>(jpg_bix) * 64 + k], quant[k]);
        coeff_t* block = img->block(c, bix);
        acm.ChangeAt<JpegHistogram, false>(acm_base[c] + bix, c, block, k, static_cast<coeff_t>(newval), quant,
                                           nullptr, &ac_histograms[c], nullptr);
        img->SetCoeffBlock(c, bix, block);  // (the chroma's pixel update: 0.5 us, 0.17 s of a 1080p force_420)
        chroma_updates += c != 0;
        last_indexes[bix] += direction;
        loop.Applied(global_order[i].second);
        if (loop.CodesRead(i)) ac_histogram_size = static_cast<int>(ComputeEntropyCodes(ac_histograms, &ac_depths));
        if (!loop.EstimateRead(i)) continue;
        est_jpg_size = jpg_header_size + dc_size + ac_histogram_size +
                       static_cast<int>(EntropyCodedDataSize(ac_histograms, ac_depths));
        if (loop.Stop(est_jpg_size, prev_size)) break;
      }
      for (int i = 0; i < num_blocks; ++i) max_block_error[i] += block_weight[i] * loop.val_threshold * direction;
      ++res_->iterations;
      if (direction > 0) ++res_->iterations_up; else ++res_->iterations_down;
      res_->detail["backend420_changes"] += loop.changed;
      res_->detail["backend420_chroma_updates"] += static_cast<double>(chroma_updates);
      chroma_updates = 0;
      res_->seconds_backend += Since(tb);
      BeginOutput420(jpg, img);
      const auto tc = Clock::now();
      if (!cmp_->Compare420(*img)) return Fail(err);
      res_->detail["r420_compare_s"] += Since(tc);
      prev_size = est_jpg_size;
    }
  }
  return true;
}

void EncodeRGBToJpegData(const uint8_t* rgb, int w, int h, JpegData* jpg) {
  InitJpegDataYUV444(w, h, jpg);
  for (auto& q : jpg->quant)
    for (int k = 0; k < kDCTBlockSize; ++k) q.values[k] = 1;
  const size_t nb = static_cast<size_t>(jpg->mcu_cols) * jpg->mcu_rows;
  std::vector<coeff_t> all(nb * 64 * 3);
  RgbToCoeffsQ1(rgb, w, h, all.data());
  for (int c = 0; c < 3; ++c)
    std::memcpy(jpg->components[c].coeffs.data(), all.data() + c * nb * 64, nb * 64 * sizeof(coeff_t));
}

int ProcessJpegData(const ProcessParams& params, const JpegData& jpg, Comparator* cmp,
                    ProcessResult* result, std::string* err, Partition* part) {
  if (part && (params.try_420 || params.force_420)) {
    if (err) *err = "4:2:0 output of a strip-decomposed frame is not supported";
    return GZ_ERR_UNSUPPORTED;
  }
  ActiveEncode active;  // (the host pool's worker cap)
  Processor proc(params, cmp, result, cmp ? part : nullptr);
  return proc.Run(jpg, err);
}

namespace {
// The tight RGB8 image of a frame, on the host: a device frame's rows come
// over with one (pitched) copy, RGBA is blended by PackFrame.
bool HostPackedFrame(int device, const FrameView& frame, std::vector<uint8_t>* rgb, std::string* err) {
  FrameView f = frame;
  std::vector<uint8_t> rows;
  if (f.on_device) {
    rows.resize(f.row_bytes() * f.h);
    if (hipSetDevice(device) != hipSuccess ||
        (f.stride == f.row_bytes()
             ? hipMemcpy(rows.data(), f.data, rows.size(), hipMemcpyDeviceToHost)
             : hipMemcpy2D(rows.data(), f.row_bytes(), f.data, f.stride, f.row_bytes(), f.h,
                           hipMemcpyDeviceToHost)) != hipSuccess) {
      if (err) *err = "device rgb copy failed";
      return false;
    }
    f.data = rows.data();
    f.stride = f.row_bytes();
    f.on_device = false;
    if (f.channels == 3) {
      rgb->swap(rows);
      return true;
    }
  }
  rgb->resize(static_cast<size_t>(3) * f.w * f.h);
  PackFrame(f, rgb->data());
  return true;
}

// The comparator's counters and timers of a finished search.
void FillSearchStats(const HipButteraugliComparator& cmp, ProcessResult* result) {
  result->compares = cmp.compares;
  result->seconds_compare = cmp.seconds_compare;
  result->seconds_zeroing = cmp.seconds_zeroing;
  result->detail["compare_thread_cpu_s"] = cmp.cpu_compare;
  result->detail["compare_wait_s"] = cmp.seconds_wait;
  result->detail["compare_wait_cpu_s"] = cmp.cpu_wait;
  result->detail["scan_bound_mismatches"] = cmp.scan_bound_mismatches;
}
}  // namespace

int Process(int device, const ProcessParams& params, const uint8_t* rgb, bool device_ptr, int w,
            int h, ProcessResult* result, std::string* err) {
  FrameView f;
  f.data = rgb;
  f.w = w;
  f.h = h;
  f.stride = f.row_bytes();
  f.on_device = device_ptr;
  return Process(device, params, f, result, err);
}

int PackFrameRgb(int device, const FrameView& frame, uint8_t* rgb_out, std::string* err) {
  if (const char* bad = FrameError(frame)) {
    if (err) *err = bad;
    return GZ_ERR_INVALID_ARG;
  }
  const size_t bytes = static_cast<size_t>(3) * frame.w * frame.h;
  if (frame.on_device && frame.w >= 32 && frame.h >= 32) {
    // what an encode's comparator holds after its import (or its copy)
    std::string e;
    auto cmp = HipButteraugliComparator::Create(device, frame, 1.0f, &e);
    if (!cmp || !cmp->engine()->ReferenceRgb(rgb_out)) {
      if (err) *err = cmp ? cmp->engine()->error() : e;
      return GZ_ERR_DEVICE;
    }
    return 0;
  }
  if (!frame.on_device) {
    PackFrame(frame, rgb_out);
    return 0;
  }
  std::vector<uint8_t> rgb;
  if (!HostPackedFrame(device, frame, &rgb, err)) return GZ_ERR_DEVICE;
  std::memcpy(rgb_out, rgb.data(), bytes);
  return 0;
}

int Process(int device, const ProcessParams& params, const FrameView& frame, ProcessResult* result,
            std::string* err) {
  // guetzli::Process(params, stats, rgb, w, h, out), processor.cc:1157-1185
  const auto t0 = Clock::now();
  const double c0 = ThreadCpu();
  const int w = frame.w, h = frame.h;
  if (w <= 0 || h <= 0 || w >= (1 << 16) || h >= (1 << 16)) {
    if (err) *err = "Could not create jpg data from rgb pixels";
    return GZ_ERR_INVALID_ARG;
  }
  if (const char* bad = FrameError(frame)) {
    if (err) *err = bad;
    return GZ_ERR_INVALID_ARG;
  }
  if (params.butteraugli_target > 2.0f) {
    // ProcessJpegData's first check (processor.cc:939-945), made before any
    // device work so that the answer does not depend on a device being there
    if (err) *err = "butteraugli target above 2.0 (quality below 84) is not supported";
    return GZ_ERR_INVALID_ARG;
  }
  JpegData jpg;
  std::unique_ptr<HipButteraugliComparator> cmp;
  const bool search = w >= 32 && h >= 32;
  // Packed on the host: a host frame that is not tight RGB already, and any
  // device frame of an image too small for the search.
  FrameView f = frame;
  std::vector<uint8_t> host_rgb;
  if (search ? !f.on_device && !f.tight_rgb() : f.on_device || !f.tight_rgb()) {
    if (!HostPackedFrame(device, frame, &host_rgb, err)) return GZ_ERR_DEVICE;
    f = FrameView();
    f.data = host_rgb.data();
    f.w = w;
    f.h = h;
    f.stride = f.row_bytes();
  }
  if (search) {
    // q=1 coefficients on the device from the resident reference image
    std::string e;
    cmp = HipButteraugliComparator::Create(device, f, params.butteraugli_target, &e);
    if (!cmp || !cmp->OriginalJpegData(&jpg)) {
      if (err) *err = cmp ? cmp->error() : e;
      return GZ_ERR_DEVICE;
    }
  } else {
    // Below 32 px guetzli::Process skips Butteraugli and writes the q=1
    // encode; that is the host encoder's job (no device work to mirror).
    EncodeRGBToJpegData(f.data, w, h, &jpg);
  }
  result->seconds_setup = Since(t0);
  const int rc = ProcessJpegData(params, jpg, cmp.get(), result, err);
  if (cmp) FillSearchStats(*cmp, result);
  result->seconds_total = Since(t0);
  result->detail["thread_cpu_s"] = ThreadCpu() - c0;
  return rc;
}

int PackImageRgb(int device, const ImageView& image, uint8_t* rgb_out, std::string* err) {
  if (const char* bad = ImageError(image)) {
    if (err) *err = bad;
    return GZ_ERR_INVALID_ARG;
  }
  if (!image.on_device) {
    PackImage(image, rgb_out);
    return 0;
  }
  if (image.w >= 32 && image.h >= 32) {
    // what an encode's comparator holds after its import
    std::string e;
    auto cmp = HipButteraugliComparator::Create(device, image, 1.0f, &e);
    if (!cmp || !cmp->engine()->ReferenceRgb(rgb_out)) {
      if (err) *err = cmp ? cmp->engine()->error() : e;
      return GZ_ERR_DEVICE;
    }
    return 0;
  }
  return ImportImageRgb(device, image, rgb_out, err) ? 0 : GZ_ERR_DEVICE;
}

int Process(int device, const ProcessParams& params, const ImageView& image, ProcessResult* result,
            std::string* err) {
  const auto t0 = Clock::now();
  const double c0 = ThreadCpu();
  if (const char* bad = ImageError(image)) {
    if (err) *err = bad;
    return GZ_ERR_INVALID_ARG;
  }
  if (params.butteraugli_target > 2.0f) {
    // (before any device work, as for a frame)
    if (err) *err = "butteraugli target above 2.0 (quality below 84) is not supported";
    return GZ_ERR_INVALID_ARG;
  }
  const int w = image.w, h = image.h;
  if (!image.on_device || w < 32 || h < 32) {
    // P on the host, then the tight-RGB encode
    std::vector<uint8_t> rgb(static_cast<size_t>(3) * w * h);
    const int rc = PackImageRgb(device, image, rgb.data(), err);
    if (rc != 0) return rc;
    const double pack = Since(t0);
    const int rc2 = Process(device, params, rgb.data(), false, w, h, result, err);
    result->seconds_setup += pack;
    result->seconds_total += pack;
    return rc2;
  }
  // q=1 coefficients on the device from the reference image the import left
  JpegData jpg;
  std::string e;
  auto cmp = HipButteraugliComparator::Create(device, image, params.butteraugli_target, &e);
  if (!cmp || !cmp->OriginalJpegData(&jpg)) {
    if (err) *err = cmp ? cmp->error() : e;
    return GZ_ERR_DEVICE;
  }
  result->seconds_setup = Since(t0);
  const int rc = ProcessJpegData(params, jpg, cmp.get(), result, err);
  FillSearchStats(*cmp, result);
  result->seconds_total = Since(t0);
  result->detail["thread_cpu_s"] = ThreadCpu() - c0;
  return rc;
}

int ProcessJpeg(int device, const ProcessParams& params, const uint8_t* data, size_t len,
                ProcessResult* result, std::string* err) {
  // guetzli::Process(params, stats, data, jpg_out), processor.cc:1029-1066
  const auto t0 = Clock::now();
  const double c0 = ThreadCpu();
  JpegData jpg;
  std::string rerr;
  if (!ReadJpeg(data, len, &jpg, &rerr)) {
    if (err) *err = "Can't read jpg data from input file: " + rerr;
    return GZ_ERR_INVALID_ARG;
  }
  if (!CheckJpegSanity(jpg)) {
    if (err) *err = "Unsupported input JPEG (unexpectedly large coefficient values)";
    return GZ_ERR_INVALID_ARG;
  }
  // ProcessJpegData's input checks (processor.cc:939-963), ahead of the
  // decode
  if (params.butteraugli_target > 2.0f) {
    if (err) *err = "butteraugli target above 2.0 (quality below 84) is not supported";
    return GZ_ERR_INVALID_ARG;
  }
  if (jpg.components.size() != 3 || !HasYCbCrColorSpace(jpg)) {
    if (err) *err = "Only YUV color space input jpeg is supported";
    return GZ_ERR_UNSUPPORTED;
  }
  if (!JpegIs444(jpg) && !JpegIs420(jpg)) {
    if (err) *err = "Unsupported sampling factors";
    return GZ_ERR_UNSUPPORTED;
  }

  std::vector<uint8_t> rgb;
  if (!DecodeJpegToRGB(jpg, &rgb)) {
    if (err) *err = "input JPEG could not be decoded";
    return GZ_ERR_UNSUPPORTED;
  }
  std::unique_ptr<HipButteraugliComparator> cmp;
  if (jpg.width >= 32 && jpg.height >= 32) {
    std::string e;
    cmp = HipButteraugliComparator::Create(device, jpg.width, jpg.height, rgb.data(), false,
                                           params.butteraugli_target, &e);
    if (!cmp) {
      if (err) *err = e;
      return GZ_ERR_DEVICE;
    }
  }
  result->seconds_setup = Since(t0);
  const int rc = ProcessJpegData(params, jpg, cmp.get(), result, err);
  if (cmp) FillSearchStats(*cmp, result);
  result->seconds_total = Since(t0);
  result->detail["thread_cpu_s"] = ThreadCpu() - c0;
  return rc;
}

}  // namespace gz
