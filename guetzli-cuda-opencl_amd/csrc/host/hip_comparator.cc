// Portions restate Guetzli (Copyright 2016 Google Inc., Apache License 2.0,
// http://www.apache.org/licenses/LICENSE-2.0) as modified in
// yyamamoto79/guetzli-cuda-opencl: processor.cc, quality.cc, score.cc and butteraugli_comparator.cc
// (QuantMatrixGenerator, the back end's control flow, kLocalMaxWeight).
// Byte-exact output forces their operation order and constants; the
// code around them is this repository's own.
// guetzli::ButteraugliComparator on the HIP engine: the Comparator surface of
// host/processor.h over the engine's device passes, and the device forms of
// the entropy coder the search uses.
#include "host/processor.h"

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
#include "host/host_util.h"
#include "host/strips.h"
#include "host/thread_pool.h"


namespace gz {

// ---------------------------------------------------------------------------
// HipButteraugliComparator
// ---------------------------------------------------------------------------

std::unique_ptr<HipButteraugliComparator> HipButteraugliComparator::Create(
    int device, int w, int h, const uint8_t* rgb, bool device_ptr, float target, std::string* err) {
  FrameView f;
  f.data = rgb;
  f.w = w;
  f.h = h;
  f.stride = f.row_bytes();
  f.on_device = device_ptr;
  return Create(device, f, target, err);
}

std::unique_ptr<HipButteraugliComparator> HipButteraugliComparator::Create(int device, const FrameView& f,
                                                                           float target, std::string* err) {
  std::unique_ptr<HipButteraugliComparator> c(new HipButteraugliComparator);
  c->engine_ = AcquireEngine(device, f.w, f.h, err);
  if (!c->engine_) return nullptr;
  if (!(f.tight_rgb() ? c->engine_->SetReference(f.data, f.on_device)
                      : c->engine_->SetReferenceFrame(f.data, f.channels, f.stride))) {
    if (err) *err = c->engine_->error();
    return nullptr;
  }
  c->w_ = f.w;
  c->h_ = f.h;
  c->target_ = target;
  c->block_max_.assign(c->engine_->blocks(), 0.0f);
  return c;
}

std::unique_ptr<HipButteraugliComparator> HipButteraugliComparator::Create(int device, const ImageView& image,
                                                                           float target, std::string* err) {
  std::unique_ptr<HipButteraugliComparator> c(new HipButteraugliComparator);
  c->engine_ = AcquireEngine(device, image.w, image.h, err);
  if (!c->engine_) return nullptr;
  if (!c->engine_->SetReferenceImage(image)) {
    if (err) *err = c->engine_->error();
    return nullptr;
  }
  c->w_ = image.w;
  c->h_ = image.h;
  c->target_ = target;
  c->block_max_.assign(c->engine_->blocks(), 0.0f);
  return c;
}

bool HipButteraugliComparator::OriginalJpegData(JpegData* jpg) {
  InitJpegDataYUV444(w_, h_, jpg);
  for (auto& q : jpg->quant)
    for (int k = 0; k < kDCTBlockSize; ++k) q.values[k] = 1;
  const size_t per = static_cast<size_t>(engine_->blocks()) * 64;
  if (orig_.size() != 3 * per) orig_.reset(3 * per);
  if (!engine_->ComputeOriginalCoeffs(orig_.data())) {
    err_ = engine_->error();
    return false;
  }
  for (int c = 0; c < 3; ++c)
    std::memcpy(jpg->components[c].coeffs.data(), orig_.data() + c * per, per * sizeof(coeff_t));
  orig_on_device_ = true;
  return true;
}

bool HipButteraugliComparator::SetOriginalCoeffs(const JpegData& jpg) {
  const size_t per = static_cast<size_t>(engine_->blocks()) * 64;
  if (orig_on_device_ && orig_.size() == 3 * per) {
    // already resident (OriginalJpegData) unless the caller changed them
    bool same = true;
    for (int c = 0; c < 3 && same; ++c)
      same = jpg.components[c].coeffs.size() == per &&
             std::memcmp(jpg.components[c].coeffs.data(), orig_.data() + c * per,
                         per * sizeof(coeff_t)) == 0;
    if (same) return true;
  }
  orig_on_device_ = false;
  size_t total = 0;
  for (int c = 0; c < 3; ++c) total += jpg.components[c].coeffs.size();
  orig_.reset(total);
  coeff_t* all = orig_.data();
  for (int c = 0; c < 3; ++c) {
    std::memcpy(all, jpg.components[c].coeffs.data(), jpg.components[c].coeffs.size() * sizeof(coeff_t));
    all += jpg.components[c].coeffs.size();
  }
  if (!engine_->SetOriginalCoeffs(orig_.data(), false)) {
    err_ = engine_->error();
    return false;
  }
  return true;
}

// img holds exactly the q=1 originals resident on the device (d_orig_).
bool HipButteraugliComparator::IsOriginal(const CoeffImage& img) const {
  if (!orig_on_device_ || img.coeffs.size() != orig_.size()) return false;
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < kDCTBlockSize; ++k)
      if (img.quant[c][k] != 1) return false;
  return std::memcmp(img.coeffs.data(), orig_.data(), orig_.size() * sizeof(coeff_t)) == 0;
}

// Brings the device copy of the coefficients up to date with img: the
// journalled edits when it is in img's epoch, else everything.
bool HipButteraugliComparator::SyncCoeffs(const CoeffImage& img) {
  if (device_.Current(img)) return true;
  // A short journal is replayed, a long one replaced by a full upload --
  // except while the host copy is partial (the back end's lazily
  // materialised blocks): then only the journalled values are current, so
  // the journal is replayed whatever its length.  (GZ_REPLAY_DIV: the
  // journal length above which the full upload is chosen, as a fraction
  // 1/GZ_REPLAY_DIV of the coefficients; tests force long tails with it.)
  static const size_t replay_div = static_cast<size_t>(EnvInt("GZ_REPLAY_DIV", 8));
  const bool short_journal = img.changed.size() - device_.pos < img.coeffs.size() / replay_div;
  const bool replay = device_.CanReplay(img) && (short_journal || img.host_partial);
  if (!img.host_valid || (img.host_partial && !replay)) {
    err_ = "coefficients are current on neither side";
    return false;
  }
  bool ok;
  if (replay) {
    const size_t n = img.changed.size() - device_.pos;
    const uint32_t* idx = img.changed.data() + device_.pos;
    delta_val_.resize(n);
    for (size_t i = 0; i < n; ++i) delta_val_[i] = img.coeffs[idx[i]];
    ok = engine_->UploadCoeffDelta(idx, delta_val_.data(), n);
  } else if (IsOriginal(img)) {
    // the search's first image (CopyFromJpegData of the q=1 originals) is
    // already resident: an HBM copy instead of a pageable upload
    ok = engine_->CurrentFromOriginal();
  } else {
    ok = engine_->UploadCoeffs(img.coeffs.data());
  }
  if (!ok) {
    err_ = engine_->error();
    return false;
  }
  device_.Set(img);
  return true;
}

const std::vector<float>& HipButteraugliComparator::block_max_distance() const {
  if (block_max_stale_) {
    float d = 0.0f;
    block_max_failed_ = false;
    if (engine_->CompareFinish(&d, block_max_.data())) {
      block_max_stale_ = false;
    } else {
      block_max_failed_ = true;
      err_ = engine_->error();
      std::fill(block_max_.begin(), block_max_.end(), std::numeric_limits<float>::infinity());
    }
  }
  return block_max_;
}

bool HipButteraugliComparator::Compare(const CoeffImage& img) {
  const auto t0 = Clock::now();
  if (!SyncCoeffs(img)) return false;
  if (!engine_->Compare(&distance_, nullptr, nullptr)) {
    err_ = engine_->error();
    return false;
  }
  block_max_stale_ = true;
  ++compares;
  seconds_compare += Since(t0);
  return true;
}

bool HipButteraugliComparator::QuantizeFromOriginal(const int q[3][kDCTBlockSize], CoeffImage* img,
                                                    bool need_host) {
  // CopyFromJpegData(q=1) + ApplyGlobalQuantization (processor.cc:316-317)
  // on the device copy of the originals; the host copy (a pinned DMA) only
  // when the caller will read it.
  if (!engine_->QuantizeFromOriginal(q, need_host ? img->coeffs.data() : nullptr)) {
    err_ = engine_->error();
    return false;
  }
  for (int c = 0; c < 3; ++c) std::memcpy(img->quant[c], q[c], sizeof(img->quant[c]));
  img->BulkChanged();
  img->host_valid = need_host;
  device_.Set(*img);
  return true;
}

int DeviceJpegHistograms(Engine* e, const int q[3][kDCTBlockSize], JpegHistogram dc[3],
                         JpegHistogram ac[3], std::string* err) {
  uint32_t hist[6 * 256];
  uint64_t chroma = 0;
  if (!e->JpegStage(q, hist, &chroma)) {
    if (err) *err = e->error();
    return -1;
  }
  return HistogramsFromStage(hist, chroma, dc, ac);
}

int HistogramsFromStage(const uint32_t* hist, uint64_t chroma, JpegHistogram dc[3],
                        JpegHistogram ac[3]) {
  const int ncomp = chroma > 0 ? 3 : 1;  // SaveToJpegData drops all-zero chroma
  for (int c = 0; c < 3; ++c) {
    dc[c].Clear();
    ac[c].Clear();
    if (c >= ncomp) continue;
    for (int i = 0; i < 256; ++i) {
      dc[c].counts[i] = 2 * hist[(2 * c) * 256 + i];
      ac[c].counts[i] = 2 * hist[(2 * c + 1) * 256 + i];
    }
  }
  return ncomp;
}

bool PrepareScanFor(const JpegData& hdr, bool strip_metadata, int ncomp, JpegHistogram* dc_h,
                    JpegHistogram* ac_h, std::string* prologue, JpegCodeTables* codes) {
  HuffCodeTable dc_tab[3], ac_tab[3];
  prologue->clear();
  if (!WriteJpegPrologue(hdr, strip_metadata, dc_h, ac_h, dc_tab, ac_tab, prologue)) return false;
  std::memset(codes, 0, sizeof(*codes));
  for (int c = 0; c < ncomp; ++c)
    for (int i = 0; i < 256; ++i) {
      codes->dc_len[c][i] = dc_tab[c].depth[i];
      codes->ac_len[c][i] = ac_tab[c].depth[i];
      codes->dc_code[c][i] = static_cast<uint16_t>(dc_tab[c].code[i]);
      codes->ac_code[c][i] = static_cast<uint16_t>(ac_tab[c].code[i]);
    }
  return true;
}

bool PrepareScan(int w, int h, const int q[3][kDCTBlockSize], const JpegData& meta,
                 bool strip_metadata, int ncomp, JpegHistogram* dc_h, JpegHistogram* ac_h,
                 std::string* prologue, JpegCodeTables* codes) {
  JpegData hdr;
  hdr.app_data = meta.app_data;
  hdr.com_data = meta.com_data;
  JpegHeaderFor(w, h, q, ncomp, &hdr);
  return PrepareScanFor(hdr, strip_metadata, ncomp, dc_h, ac_h, prologue, codes);
}

bool DeviceEncodeJpeg(Engine* e, int w, int h, const int q[3][kDCTBlockSize], const JpegData& meta,
                      bool strip_metadata, std::string* prologue, size_t* size, std::string* err) {
  JpegHistogram dc_h[3], ac_h[3];
  const int ncomp = DeviceJpegHistograms(e, q, dc_h, ac_h, err);
  if (ncomp < 0) return false;
  JpegCodeTables codes;
  if (!PrepareScan(w, h, q, meta, strip_metadata, ncomp, dc_h, ac_h, prologue, &codes)) {
    if (err) *err = "jpeg header";
    return false;
  }
  uint64_t nbits = 0, ff = 0;
  if (!e->JpegScan(ncomp, q, codes, &nbits, &ff)) {
    if (err) *err = e->error();
    return false;
  }
  // prologue + scan bytes (padded) + a stuffed 0x00 per 0xff + EOI
  *size = prologue->size() + static_cast<size_t>((nbits + 7) / 8 + ff) + 2;
  return true;
}

bool DeviceFetchJpeg(Engine* e, bool kept, const std::string& prologue, size_t size,
                     std::string* out, std::string* err) {
  const uint8_t* bytes = nullptr;
  uint64_t nbits = 0;
  if (!e->JpegFetch(kept, &bytes, &nbits)) {
    if (err) *err = e->error();
    return false;
  }
  *out = prologue;
  AppendStuffedScan(bytes, nbits, out);
  if (out->size() != size) {  // the device's size prediction is what the search scored
    if (err) *err = "device JPEG size prediction mismatch";
    return false;
  }
  return true;
}

bool DeviceWriteJpeg(Engine* e, int w, int h, const int q[3][kDCTBlockSize], const JpegData& meta,
                     bool strip_metadata, std::string* out, std::string* err) {
  std::string prologue;
  size_t size = 0;
  return DeviceEncodeJpeg(e, w, h, q, meta, strip_metadata, &prologue, &size, err) &&
         DeviceFetchJpeg(e, false, prologue, size, out, err);
}

int HipButteraugliComparator::DeviceHistograms(const CoeffImage& img, JpegHistogram dc[3],
                                               JpegHistogram ac[3]) {
  if (!SyncCoeffs(img)) return -1;
  return DeviceJpegHistograms(engine_.get(), img.quant, dc, ac, &err_);
}

bool HipButteraugliComparator::DeviceWriteJpeg(const CoeffImage& img, const JpegData& meta,
                                               bool strip_metadata, std::string* out) {
  if (!SyncCoeffs(img)) return false;
  return gz::DeviceWriteJpeg(engine_.get(), w_, h_, img.quant, meta, strip_metadata, out, &err_);
}

bool HipButteraugliComparator::DeviceEncodeAndCompare(const CoeffImage& img,
                                                      const JpegData& meta, bool strip_metadata,
                                                      size_t* size) {
  return EncodeAndCompareWith(img, meta, nullptr, strip_metadata, size);
}

// The reference's first output, OutputJpeg(jpg_in) (processor.cc:965-967),
// when jpg_in holds img's coefficients as they are (every quant value 1, as
// for RGB input, one block per MCU): its scan is the device coder's scan of
// img, only the headers are jpg_in's own (three quant tables where
// SaveToJpegData shares one), so the size -- and, if it is kept, the bytes --
// come from the device with jpg_in's prologue.  Not used (*used = false;
// the Compare is done) when SaveToJpegData would drop all-zero chroma that
// jpg_in keeps.
bool HipButteraugliComparator::DeviceEncodeOriginalAndCompare(const CoeffImage& img,
                                                              const JpegData& jpg_in,
                                                              bool strip_metadata, size_t* size,
                                                              bool* used) {
  JpegData hdr;
  JpegHeaderOf(jpg_in, &hdr);
  *used = true;
  if (!EncodeAndCompareWith(img, jpg_in, &hdr, strip_metadata, size)) {
    if (err_ != "jpeg header components") return false;
    err_.clear();
    *used = false;
  }
  return true;
}

bool HipButteraugliComparator::EncodeAndCompareWith(const CoeffImage& img, const JpegData& meta,
                                                    const JpegData* hdr, bool strip_metadata,
                                                    size_t* size) {
  // One stream order: histogram stage, Compare pass, then the scan; the host
  // builds the Huffman codes from the staged histograms while the Compare
  // pass runs, and waits once for both results.
  const auto t0 = Clock::now();
  const double c0 = ThreadCpu();
  if (!SyncCoeffs(img)) return false;
  Engine* e = engine_.get();
  uint32_t hist[6 * 256];
  uint64_t chroma = 0;
  if (!e->JpegStageEnqueue(img.quant) || !e->CompareEnqueue()) {
    err_ = e->error();
    return false;
  }
  const auto tw0 = Clock::now();
  const double cw0 = ThreadCpu();
  if (!e->JpegStageWait(hist, &chroma)) {
    err_ = e->error();
    return false;
  }
  seconds_wait += Since(tw0);
  cpu_wait += ThreadCpu() - cw0;
  JpegHistogram dc_h[3], ac_h[3];
  const int ncomp = HistogramsFromStage(hist, chroma, dc_h, ac_h);
  JpegCodeTables codes;
  if (hdr && static_cast<int>(hdr->components.size()) != ncomp) {
    // (the Compare is in the stream: finish it)
    if (!e->Sync()) {
      err_ = e->error();
      return false;
    }
    (void)e->CompareFinish(&distance_, nullptr);
    block_max_stale_ = true;
    ++compares;
    seconds_compare += Since(t0);
    cpu_compare += ThreadCpu() - c0;
    err_ = "jpeg header components";
    return false;
  }
  if (!(hdr ? PrepareScanFor(*hdr, strip_metadata, ncomp, dc_h, ac_h, &cur_prologue_, &codes)
            : PrepareScan(w_, h_, img.quant, meta, strip_metadata, ncomp, dc_h, ac_h, &cur_prologue_,
                          &codes))) {
    err_ = "jpeg header";
    return false;
  }
  seconds_encode += Since(t0);
  uint64_t nbits = 0, ff = 0;
  if (!e->JpegScanEnqueue(ncomp, img.quant, codes)) {
    err_ = e->error();
    return false;
  }
  const auto tw1 = Clock::now();
  const double cw1 = ThreadCpu();
  if (!e->Sync() || !e->JpegScanFinish(&nbits, &ff)) {
    err_ = e->error();
    return false;
  }
  seconds_wait += Since(tw1);
  cpu_wait += ThreadCpu() - cw1;
  (void)e->CompareFinish(&distance_, nullptr);
  block_max_stale_ = true;
  ++compares;
  // prologue + scan bytes (padded) + a stuffed 0x00 per 0xff + EOI
  cur_size_ = cur_prologue_.size() + static_cast<size_t>((nbits + 7) / 8 + ff) + 2;
  *size = cur_size_;
  seconds_compare += Since(t0);
  cpu_compare += ThreadCpu() - c0;
  return true;
}

bool HipButteraugliComparator::DeviceEncode(const CoeffImage& img, const JpegData& meta,
                                            bool strip_metadata, size_t* size) {
  if (!SyncCoeffs(img)) return false;
  if (!DeviceEncodeJpeg(engine_.get(), w_, h_, img.quant, meta, strip_metadata, &cur_prologue_,
                        &cur_size_, &err_))
    return false;
  *size = cur_size_;
  return true;
}

void HipButteraugliComparator::DeviceKeepEncoded() {
  engine_->JpegKeep();
  kept_prologue_.swap(cur_prologue_);
  kept_size_ = cur_size_;
}

bool HipButteraugliComparator::DeviceFetchKept(std::string* out) {
  return DeviceFetchJpeg(engine_.get(), true, kept_prologue_, kept_size_, out, &err_);
}

bool HipButteraugliComparator::StartBlockComparisons() {
  if (!engine_->StartBlockComparisons(nullptr)) {
    err_ = engine_->error();
    return false;
  }
  return true;
}

bool HipButteraugliComparator::BlockZeroingOrders(const CoeffImage& img, const JpegData&,
                                                  int comp_mask, int lookahead, bool new_model,
                                                  std::vector<CoeffData>* out) {
  const auto t0 = Clock::now();
  if (!SyncCoeffs(img)) return false;
  out->resize(static_cast<size_t>(img.blocks) * 192);
  static_assert(sizeof(CoeffData) == sizeof(CoeffDataHost), "CoeffData layout");
  if (!engine_->BlockZeroingOrders(comp_mask, target_, lookahead, new_model,
                                   reinterpret_cast<CoeffDataHost*>(out->data()))) {
    err_ = engine_->error();
    return false;
  }
  seconds_zeroing += Since(t0);
  return true;
}

bool Comparator::BlockZeroingCandidates(const CoeffImage& img, const JpegData& orig_jpg,
                                        int comp_mask, int lookahead, bool new_model,
                                        std::vector<int>* offsets, std::vector<uint8_t>* idx,
                                        std::vector<float>* err) {
  std::vector<CoeffData> order;
  if (!BlockZeroingOrders(img, orig_jpg, comp_mask, lookahead, new_model, &order)) return false;
  const float limit = BlockErrorLimit();
  offsets->assign(img.blocks + 1, 0);
  idx->clear();
  err->clear();
  for (int b = 0; b < img.blocks; ++b) {
    const CoeffData* p = &order[static_cast<size_t>(b) * 192];
    (*offsets)[b] = static_cast<int>(idx->size());
    for (int i = 0; i < 192; ++i) {
      if (p[i].block_err > 0 && p[i].block_err <= limit) {
        idx->push_back(static_cast<uint8_t>(p[i].idx));
        err->push_back(p[i].block_err);
      }
    }
  }
  (*offsets)[img.blocks] = static_cast<int>(idx->size());
  return true;
}

bool HipButteraugliComparator::BlockZeroingCandidates(const CoeffImage& img, const JpegData&,
                                                      int comp_mask, int lookahead, bool new_model,
                                                      std::vector<int>* offsets,
                                                      std::vector<uint8_t>* idx,
                                                      std::vector<float>* err) {
  const auto t0 = Clock::now();
  if (!SyncCoeffs(img)) return false;
  if (!engine_->BlockZeroingCandidates(comp_mask, target_, lookahead, new_model, offsets, idx,
                                       err)) {
    err_ = engine_->error();
    return false;
  }
  seconds_zeroing += Since(t0);
  return true;
}

bool HipButteraugliComparator::SetOriginalCoeffs420(const JpegData& jpg420) {
  // the luma at the engine's block width (the 4:2:0 file pads Y to whole
  // MCUs), the chroma as stored; q = 1, so these are the raw values the
  // zeroing keys and the back end read (processor.cc:653-657, 865-868)
  const int bw = engine_->block_w(), bh = engine_->block_h();
  const int cbw = (w_ + 15) / 16, cbh = (h_ + 15) / 16;
  if (jpg420.components.size() != 3) {
    err_ = "4:2:0 originals need 3 components";
    return false;
  }
  std::vector<coeff_t> y(static_cast<size_t>(bw) * bh * 64), c[2];
  const JpegComponent& jy = jpg420.components[0];
  for (int by = 0; by < bh; ++by)
    std::memcpy(&y[static_cast<size_t>(by) * bw * 64], &jy.coeffs[static_cast<size_t>(by) * jy.width_in_blocks * 64],
                static_cast<size_t>(bw) * 64 * sizeof(coeff_t));
  for (int k = 0; k < 2; ++k) {
    const JpegComponent& jc = jpg420.components[1 + k];
    c[k].resize(static_cast<size_t>(cbw) * cbh * 64);
    for (int by = 0; by < cbh; ++by)
      std::memcpy(&c[k][static_cast<size_t>(by) * cbw * 64], &jc.coeffs[static_cast<size_t>(by) * jc.width_in_blocks * 64],
                  static_cast<size_t>(cbw) * 64 * sizeof(coeff_t));
  }
  orig_on_device_ = false;  // (the 4:4:4 originals are gone from the device)
  device_ = CoeffCursor();
  if (!engine_->SetOriginal420(y.data(), c[0].data(), c[1].data())) {
    err_ = engine_->error();
    return false;
  }
  return true;
}

bool HipButteraugliComparator::Compare420(const Image420& img) {
  const auto t0 = Clock::now();
  device_ = CoeffCursor();
  if (!engine_->Set420(img.y.data(), img.c[0].data(), img.c[1].data(), img.plane[0].px.data(),
                       img.plane[1].px.data()) ||
      !engine_->Compare(&distance_, nullptr, nullptr)) {
    err_ = engine_->error();
    return false;
  }
  block_max_stale_ = true;
  ++compares;
  seconds_compare += Since(t0);
  return true;
}

bool HipButteraugliComparator::BlockZeroingCandidates420(Image420* img, int comp_mask, int lookahead,
                                                         bool new_model, std::vector<int>* offsets,
                                                         std::vector<uint8_t>* idx,
                                                         std::vector<float>* err) {
  const auto t0 = Clock::now();
  device_ = CoeffCursor();
  if (!engine_->Set420(img->y.data(), img->c[0].data(), img->c[1].data(), img->plane[0].px.data(),
                       img->plane[1].px.data()) ||
      !engine_->BlockZeroingCandidates420(comp_mask, target_, lookahead, new_model, offsets, idx, err,
                                          img->plane[0].px.data(), img->plane[1].px.data())) {
    err_ = engine_->error();
    return false;
  }
  seconds_zeroing += Since(t0);
  return true;
}

bool HipButteraugliComparator::DeviceOrderReset(bool* available) {
  *available = false;
  if (!engine_->HasOrderCandidates()) return true;
  // (an allocation failure leaves the order on the host; a stream or launch
  // error fails the encode)
  bool unavailable = false;
  if (!engine_->OrderReset(&unavailable)) {
    err_ = engine_->error();
    return false;
  }
  *available = !unavailable;
  return true;
}

bool HipButteraugliComparator::DeviceChangeOrder(int direction, double target_mul, bool zero_bmax,
                                                 const std::vector<int>& last_indexes, float floor_limit,
                                                 size_t* n_entries, int* blocks_to_change, int64_t* below_floor) {
  // (ComputeBlockErrorAdjustmentWeights' target distance: target * target_mul
  // in double, butteraugli_comparator.cc:175)
  const double td = target_ * target_mul;
  *n_entries = 0;
  for (int rblock = 1; rblock <= 4; ++rblock) {
    // (the entries are filled with the counts: one wait per radius)
    const bool ok = engine_->OrderBuild(direction, rblock, td, zero_bmax, last_indexes, n_entries,
                                        blocks_to_change, floor_limit, below_floor);
    if (!ok) err_ = engine_->error();
    if (order_x_) {
      // a frame split over ranks: the radius is the first with entries
      // anywhere in the frame; the counts are the frame's
      uint32_t t[4] = {static_cast<uint32_t>(ok ? *n_entries : 0), static_cast<uint32_t>(ok ? *blocks_to_change : 0),
                       static_cast<uint32_t>(ok && below_floor ? *below_floor : 0), 0};
      if (!order_x_->SumU32(ok, t, 3)) {
        if (ok) err_ = "change order: a rank failed";
        return false;
      }
      *n_entries = t[0];
      *blocks_to_change = static_cast<int>(t[1]);
      if (below_floor) *below_floor = t[2];
      engine_->SetOrderFrameEntries(*n_entries);
    }
    if (!ok) return false;
    if (*n_entries) break;
  }
  return true;
}

void HipButteraugliComparator::SetDeviceOrderScope(int own_lo, int own_hi, int gbase, Engine::OrderExchange* x) {
  order_x_ = x;
  order_gbase_ = x ? gbase : 0;
  if (x) engine_->SetOrderScope(own_lo, own_hi, gbase, x);
  else engine_->SetOrderScope(0, 1 << 30, 0, nullptr);
}

bool HipButteraugliComparator::DeviceSetBlockMax(const std::vector<float>& bmax) {
  if (static_cast<int>(bmax.size()) != engine_->blocks() || !engine_->SetBlockMax(bmax.data())) {
    err_ = bmax.size() != static_cast<size_t>(engine_->blocks()) ? "DeviceSetBlockMax: size" : engine_->error();
    return false;
  }
  return true;
}

bool HipButteraugliComparator::DeviceOrderEntries(std::vector<std::pair<int, float>>* order) {
  const auto t0 = Clock::now();
  order->resize(engine_->OrderEntryCount());
  if (!engine_->OrderFetch(order->data(), order->size())) {
    err_ = engine_->error();
    return false;
  }
  // (a strip's entries in frame block indices, as the host build's)
  if (order_gbase_)
    for (auto& e : *order) e.first += order_gbase_;
  seconds_bulk += Since(t0);
  return true;
}

bool HipButteraugliComparator::DeviceSelectBulk(const CoeffImage& img, size_t bulk, size_t window, int direction,
                                                Engine::OrderSelection* sel, JpegHistogram ac[3]) {
  const auto t0 = Clock::now();
  if (bulk && !SyncCoeffs(img)) return false;
  int32_t delta[3][256];
  const bool ok = engine_->OrderSelect(bulk, window, direction, img.quant, true, sel, delta);
  if (!ok) err_ = engine_->error();
  if (order_x_ && (!ok || sel->applied)) {
    // a frame split over ranks: the frame's histogram change (every rank's
    // applies to its owned blocks; the same `applied` on every rank)
    std::vector<uint32_t> d(3 * 256);
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < 256; ++i) d[c * 256 + i] = ok ? static_cast<uint32_t>(delta[c][i]) : 0u;
    if (!order_x_->SumU32(ok, d.data(), 3 * 256)) {
      if (ok) err_ = "bulk prefix: a rank failed";
      return false;
    }
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < 256; ++i) delta[c][i] = static_cast<int32_t>(d[c * 256 + i]);
  }
  if (!ok) return false;
  if (sel->applied) {
    // (the counts are stored doubled, JpegHistogram::Add)
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < 256; ++i) ac[c].counts[i] += 2u * static_cast<uint32_t>(delta[c][i]);
  }
  seconds_bulk += Since(t0);
  return true;
}

bool HipButteraugliComparator::DeviceSelectWindow(size_t from, size_t window, int direction,
                                                  Engine::OrderSelection* sel) {
  const auto t0 = Clock::now();
  int32_t delta[3][256];
  const int q[3][kDCTBlockSize] = {};
  if (!engine_->OrderSelect(from, window, direction, q, false, sel, delta)) {
    err_ = engine_->error();
    return false;
  }
  seconds_bulk += Since(t0);
  return true;
}

bool HipButteraugliComparator::DeviceBulkApplyLocal(const CoeffImage& img, int direction, const uint8_t* cnt,
                                                    const std::vector<int>& last_indexes, int32_t delta[3][256]) {
  const auto t0 = Clock::now();
  if (!SyncCoeffs(img)) return false;
  if (!engine_->BulkApply(direction, img.quant, cnt, delta, &last_indexes)) {
    err_ = engine_->error();
    return false;
  }
  seconds_bulk += Since(t0);
  return true;
}

bool HipButteraugliComparator::DeviceBulkApply(const CoeffImage& img, int direction, const uint8_t* cnt,
                                               JpegHistogram ac[3]) {
  const auto t0 = Clock::now();
  if (!SyncCoeffs(img)) return false;
  int32_t delta[3][256];
  if (!engine_->BulkApply(direction, img.quant, cnt, delta)) {
    err_ = engine_->error();
    return false;
  }
  // (the counts are stored doubled, JpegHistogram::Add)
  for (int c = 0; c < 3; ++c)
    for (int i = 0; i < 256; ++i) ac[c].counts[i] += 2u * static_cast<uint32_t>(delta[c][i]);
  seconds_bulk += Since(t0);
  return true;
}

// The scan's bit count from the histograms the candidate is coded with:
// every symbol's code length plus its extra bits (the DC category; an AC
// symbol's low nibble).  Without the 0xff stuffing and the padding this is
// what k_jpeg_code counts, so prologue + ceil(bits / 8) + EOI bounds the
// candidate's size from below.
uint64_t ScanBits(const JpegHistogram dc[3], const JpegHistogram ac[3], int ncomp,
                  const JpegCodeTables& codes) {
  uint64_t bits = 0;
  for (int c = 0; c < ncomp; ++c)
    for (int i = 0; i < 256; ++i) {
      // (the counts are stored doubled, JpegHistogram::Add)
      bits += static_cast<uint64_t>(dc[c].counts[i] / 2) * (codes.dc_len[c][i] + i);
      bits += static_cast<uint64_t>(ac[c].counts[i] / 2) * (codes.ac_len[c][i] + (i & 15));
    }
  return bits;
}

// The distance at and above which ScoreJPEG(distance, size, target) >= best
// for every size >= size_lb (processor.cc:151-160 keeps a candidate only
// when its score is below the best; ScoreJPEG, score.cc:23-34, grows with the
// distance and with the size), with a margin; -inf when no size from size_lb
// up can beat best at any distance.
static double HopelessDistance(double best, size_t size_lb, double target) {
  const double s = static_cast<double>(size_lb);
  if (s >= best) return -HUGE_VAL;
  const double kScale = 50, kMaxExponent = 10, kLargeSize = 1e30;
  double diff = std::log(best / s) / kScale;  // exp(kScale * diff) * size_lb >= best
  if (diff > kMaxExponent / kScale)           // above it the linear branch decides
    diff = std::max(kMaxExponent / kScale, (best - s) / (kLargeSize * std::exp(kMaxExponent)));
  return target + diff + 1e-6;
}

bool HipButteraugliComparator::DeviceEncodeAndCompareKnown(const CoeffImage& img, const JpegData& meta,
                                                           bool strip_metadata, const JpegHistogram dc[3],
                                                           const JpegHistogram ac[3], int ncomp,
                                                           double best_score, size_t* size, bool* skipped) {
  // the Compare pass first; the codes on the host while it runs; the scan
  // behind it (not coded when the pass's distance shows the candidate
  // cannot become the output); one wait
  const auto t0 = Clock::now();
  const double c0 = ThreadCpu();
  *skipped = false;
  if (!SyncCoeffs(img)) return false;
  Engine* e = engine_.get();
  if (!e->CompareEnqueue()) {
    err_ = e->error();
    return false;
  }
  JpegHistogram dc_h[3], ac_h[3];
  for (int c = 0; c < ncomp; ++c) {
    dc_h[c] = dc[c];
    ac_h[c] = ac[c];
  }
  JpegCodeTables codes;
  if (!PrepareScan(w_, h_, img.quant, meta, strip_metadata, ncomp, dc_h, ac_h, &cur_prologue_, &codes)) {
    err_ = "jpeg header";
    return false;
  }
  const uint64_t bound_bits = ScanBits(dc, ac, ncomp, codes);
  const size_t size_lb = cur_prologue_.size() + static_cast<size_t>((bound_bits + 7) / 8) + 2;
  float skip_at = HUGE_VALF;
  if (best_score >= 0 && scan_bound_mismatches == 0) {
    const double d = HopelessDistance(best_score, size_lb, target_);
    if (d <= -HUGE_VAL) {
      skip_at = -HUGE_VALF;
    } else if (d < 1e30) {
      skip_at = std::nextafter(static_cast<float>(d), HUGE_VALF);
    }
  }
  seconds_encode += Since(t0);
  uint64_t nbits = 0, ff = 0;
  if (!e->JpegScanEnqueue(ncomp, img.quant, codes, skip_at)) {
    err_ = e->error();
    return false;
  }
  const auto tw = Clock::now();
  const double cw = ThreadCpu();
  if (!e->Sync()) {
    err_ = e->error();
    return false;
  }
  seconds_wait += Since(tw);
  cpu_wait += ThreadCpu() - cw;
  (void)e->CompareFinish(&distance_, nullptr);
  block_max_stale_ = true;
  ++compares;
  if (skip_at != HUGE_VALF && distance_ >= skip_at) {  // (k_jpeg_code's own test, on the same float)
    if (ScoreJPEG(distance_, static_cast<int>(size_lb), target_) >= best_score) {
      *skipped = true;
      ++scans_skipped;
      seconds_compare += Since(t0);
      cpu_compare += ThreadCpu() - c0;
      return true;
    }
    // (the margin makes this unreachable; code the scan after all)
    if (!e->JpegScanEnqueue(ncomp, img.quant, codes) || !e->Sync()) {
      err_ = e->error();
      return false;
    }
  }
  if (!e->JpegScanFinish(&nbits, &ff)) {
    err_ = e->error();
    return false;
  }
  if (nbits != bound_bits) ++scan_bound_mismatches;
  cur_size_ = cur_prologue_.size() + static_cast<size_t>((nbits + 7) / 8 + ff) + 2;
  *size = cur_size_;
  seconds_compare += Since(t0);
  cpu_compare += ThreadCpu() - c0;
  return true;
}

bool HipButteraugliComparator::DeviceOrderAdvance(float val_threshold, int direction) {
  if (!engine_->OrderAdvance(val_threshold, direction)) {
    err_ = engine_->error();
    return false;
  }
  return true;
}

double HipButteraugliComparator::ScoreOutputSize(int size) const {
  return ScoreJPEG(distance_, size, target_);
}

void HipButteraugliComparator::ComputeBlockErrorAdjustmentWeights(
    int direction, int max_block_dist, double target_mul, int factor_x, int factor_y,
    const std::vector<float>& max_dist_per_block, std::vector<float>* block_weight) {
  BlockErrorAdjustmentWeights(w_, h_, target_, direction, max_block_dist, target_mul, factor_x,
                              factor_y, max_dist_per_block, block_weight);
}

void BlockErrorAdjustmentWeights(int w, int h, float target, int direction, int max_block_dist,
                                 double target_mul, int factor_x, int factor_y,
                                 const std::vector<float>& max_dist_per_block,
                                 std::vector<float>* block_weight) {
  // butteraugli_comparator.cc:169-233 (block maxima come from the device).
  // Rows of blocks in parallel; the direction < 0 scatter of the reference
  // (every over-target block raises its neighbours to 1 / (d + 1)) is formed
  // as the equivalent gather -- a max over the same values, order-free.
  const double target_distance = target * target_mul;
  const int sizex = 8 * factor_x, sizey = 8 * factor_y;
  const int bw = (w + sizex - 1) / sizex, bh = (h + sizey - 1) / sizey;
  const int r = max_block_dist;
  constexpr int kRows = 8;
  const int chunks = (bh + kRows - 1) / kRows;
  const size_t nblk = static_cast<size_t>(bw) * bh;
  // max_local(bx, by) = max(target, block maxima within Chebyshev radius r),
  // separably: the row maxima over [bx - r, bx + r], then their maximum over
  // [by - r, by + r] (a max of the same values: exact)
  std::vector<float> rowmax(nblk), local(nblk);
  ParallelFor(chunks, [&](int ch) {
    for (int by = ch * kRows; by < std::min(bh, (ch + 1) * kRows); ++by)
      for (int bx = 0; bx < bw; ++bx) {
        float m = static_cast<float>(target_distance);
        for (int x = std::max(0, bx - r); x < std::min(bw, bx + 1 + r); ++x)
          m = std::max(m, max_dist_per_block[by * bw + x]);
        rowmax[by * bw + bx] = m;
      }
  });
  ParallelFor(chunks, [&](int ch) {
    for (int by = ch * kRows; by < std::min(bh, (ch + 1) * kRows); ++by)
      for (int bx = 0; bx < bw; ++bx) {
        float m = static_cast<float>(target_distance);
        for (int y = std::max(0, by - r); y < std::min(bh, by + 1 + r); ++y) m = std::max(m, rowmax[y * bw + bx]);
        local[by * bw + bx] = m;
      }
  });
  if (direction > 0) {
    ParallelFor(chunks, [&](int ch) {
      for (int by = ch * kRows; by < std::min(bh, (ch + 1) * kRows); ++by)
        for (int bx = 0; bx < bw; ++bx) {
          const int bix = by * bw + bx;
          if (max_dist_per_block[bix] <= target_distance && local[bix] <= 1.1 * target_distance)
            (*block_weight)[bix] = 1.0;
        }
    });
    return;
  }
  constexpr double kLocalMaxWeight = 0.5;
  std::vector<uint8_t> active(nblk);
  ParallelFor(chunks, [&](int ch) {
    for (int by = ch * kRows; by < std::min(bh, (ch + 1) * kRows); ++by)
      for (int bx = 0; bx < bw; ++bx) {
        const int bix = by * bw + bx;
        active[bix] = !(max_dist_per_block[bix] <=
                        (1 - kLocalMaxWeight) * target_distance + kLocalMaxWeight * local[bix]);
      }
  });
  // every active block within Chebyshev distance d <= r raises the weight to
  // 1 / (d + 1): the largest such term is the nearest active block's, found
  // separably (nearest active in the row, then min over rows of
  // max(|dy|, that)); the weight is the max of the same float terms as the
  // per-neighbour loop
  std::vector<int> hx(nblk);
  ParallelFor(chunks, [&](int ch) {
    for (int by = ch * kRows; by < std::min(bh, (ch + 1) * kRows); ++by)
      for (int bx = 0; bx < bw; ++bx) {
        int d = r + 1;
        for (int x = std::max(0, bx - r); x < std::min(bw, bx + 1 + r); ++x)
          if (active[by * bw + x]) d = std::min(d, std::abs(x - bx));
        hx[by * bw + bx] = d;
      }
  });
  ParallelFor(chunks, [&](int ch) {
    for (int by = ch * kRows; by < std::min(bh, (ch + 1) * kRows); ++by)
      for (int bx = 0; bx < bw; ++bx) {
        const int ix = by * bw + bx;
        int d = r + 1;
        for (int y = std::max(0, by - r); y < std::min(bh, by + 1 + r); ++y)
          d = std::min(d, std::max(std::abs(y - by), hx[y * bw + bx]));
        if (d <= r) (*block_weight)[ix] = std::max<float>((*block_weight)[ix], 1.0f / (d + 1.0f));
      }
  });
}

}  // namespace gz
