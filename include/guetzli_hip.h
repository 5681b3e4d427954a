/*
 * guetzli_hip.h — C ABI of the MI355X-native Guetzli search path
 * (libguetzli_hip.so, built from guetzli-cuda-opencl_amd/csrc).
 *
 * Drop-in boundary for the reference's hot path (yyamamoto79/guetzli-cuda-
 * opencl): the library-level encode call `guetzli::Process`
 * (guetzli/processor.h:62-64) and the comparator that the search loop talks
 * to (`guetzli::Comparator`, guetzli/comparator.h:29-96, implemented by
 * `guetzli::ButteraugliComparator`, guetzli/butteraugli_comparator.h:33-81),
 * plus the batched per-block zeroing entry of the reference GPU fast path
 * (`cuComputeBlockZeroingOrder`, clguetzli/cuguetzli.h:30-40).
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every call returns gz_status; on failure
 *    gz_last_error() (thread-local) describes it.  No call silently falls
 *    back to the CPU: without a usable HIP device they fail with
 *    GZ_ERR_DEVICE.
 *  - Images: 8-bit RGB, interleaved, row-major, no padding (3*w*h bytes);
 *    the frame entries (gz_frame) also take padded rows and RGBA, the image
 *    entries (gz_image) any strides, channel order and sample type.
 *  - Coefficients: int16, [3][blocks][64], natural (row-major) order inside
 *    a block, blocks row-major with ceil(w/8) blocks per row (the layout of
 *    guetzli::JPEGComponent::coeffs, guetzli/jpeg_data.h:138-204).
 *  - One gz_comparator owns one HIP stream and its device buffers; distinct
 *    comparators may be used from distinct host threads.  A gz_encoder is a
 *    queue of encodes on one device: its worker threads each run one encode
 *    at a time on a pooled engine (a stream and buffers of its own), and
 *    every one of its entry points may be called from any thread.
 */
#ifndef GUETZLI_HIP_H_
#define GUETZLI_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int gz_status;
enum {
  GZ_OK = 0,
  GZ_ERR_INVALID_ARG = 1,
  GZ_ERR_DEVICE = 2,
  GZ_ERR_OUT_OF_MEMORY = 3,
  GZ_ERR_UNSUPPORTED = 4,
  GZ_ERR_INTERNAL = 5,
};

/* guetzli::CoeffData (guetzli/processor.h:29-32). */
typedef struct {
  int idx;
  float block_err;
} gz_coeff_data;

/* guetzli::Params (guetzli/processor.h:34-42); same defaults via
 * gz_params_init().  try_420 / force_420 / use_silver_screen run the 4:2:0
 * pass of ProcessJpegData (processor.cc:986-1016); on an image whose chroma
 * is all zero that pass keeps one component at 4:4:4, as the reference does
 * (output_image.cc:535-539).  A butteraugli_target above 2.0 (quality below
 * 84) returns GZ_ERR_INVALID_ARG (processor.cc:939-945).  The strip
 * decomposition of one frame (gz_process_rgb_strips) supports the 4:4:4
 * search only. */
typedef struct {
  float butteraugli_target;
  int clear_metadata;
  int try_420;
  int force_420;
  int use_silver_screen;
  int zeroing_greedy_lookahead;
  int new_zeroing_model;
} gz_params;

/* guetzli::ProcessStats counters (guetzli/stats.h:26-41). */
typedef struct {
  int iterations;        /* "number of iterations" */
  int iterations_up;     /* "number of iterations up" */
  int iterations_down;   /* "number of iterations down" */
  int compares;          /* full-image Butteraugli passes */
  double seconds_compare;   /* wall time inside Compare calls */
  double seconds_zeroing;   /* wall time of the per-block search */
  double seconds_total;
  double seconds_setup;     /* initial coefficients, device context, reference */
  double seconds_write;     /* JPEG serialisation of every candidate */
  double seconds_quantize;  /* device quantization + coefficient download */
  double seconds_backend;   /* host coefficient selection / size estimation */
} gz_process_stats;

/* Stage dumps of one compare (parity tests); any pointer may be NULL.
 * Plane arrays are 3*w*h floats, res arrays 3*ceil(w/3)*ceil(h/3). */
typedef struct {
  float* cand_linear;
  float* cand_xyb;
  float* mhic0;
  float* mhic1;
  float* edge;
  float* block_dc;
  float* block_ac;
  float* block_ac_lf;
  float* mask;
  float* mask_dc;
  float* combined;   /* ceil(w/3)*ceil(h/3) */
  float* distmap;    /* w*h */
} gz_compare_stages;

typedef struct gz_comparator gz_comparator;

/* ---- library ---------------------------------------------------------- */
const char* gz_last_error(void);
const char* gz_build_info(void);
/* Number of visible HIP devices (0 when none; never fails). */
int gz_device_count(void);
void gz_params_init(gz_params* params);
/* guetzli::ButteraugliScoreForQuality (guetzli/quality.cc:78-87). */
double gz_butteraugli_score_for_quality(double quality);
void gz_free(void* p);

/* ---- encode (guetzli::Process, guetzli/processor.h:62-64) -------------- */
/* Encodes an RGB image; *jpeg_out is allocated by the library (gz_free).
 * Images under 32 pixels in either dimension are written at quantization 1
 * without a search and without device work (processor.cc:1170-1181). */
gz_status gz_process_rgb(int device, const gz_params* params, const uint8_t* rgb, int width,
                         int height, uint8_t** jpeg_out, size_t* jpeg_size,
                         gz_process_stats* stats);
/* Same, with the RGB image already resident on `device` (HBM pointer). */
gz_status gz_process_rgb_device(int device, const gz_params* params, const uint8_t* rgb_dev,
                                int width, int height, uint8_t** jpeg_out, size_t* jpeg_size,
                                gz_process_stats* stats);

/* ---- frames: padded rows, RGBA, host memory or HBM --------------------- */
/* An input image as the caller holds it.  The image that is encoded is its
 * tight RGB8 form P: P[y][x][c] = src[y][x][c] for 3 channels, and for 4
 * channels the pixel blended on black as the reference's ReadPNG does
 * (guetzli.cc:47-49): P[y][x][c] = (src[y][x][c] * src[y][x][3] + 128) / 255.
 * Any byte alignment of data and row_stride is legal.  A device frame has
 * been completely written before the call that names it. */
typedef struct {
  const void* data;     /* first byte of the top-left pixel */
  int width, height;
  int channels;         /* 3: RGB, 4: RGBA (8 bit, interleaved) */
  size_t row_stride;    /* bytes from one row to the next; 0 = width*channels */
  int on_device;        /* 0: host memory, 1: HBM of the device the call names */
} gz_frame;

/* The bytes gz_process_rgb returns for P.  A tight 3-channel frame takes the
 * path of gz_process_rgb / gz_process_rgb_device.  Any other device frame
 * with both sides >= 32 px is read where it lies by one import kernel (no
 * repacking copy); host frames, and device frames under 32 px after a
 * pitched copy, are packed on the host.  GZ_ERR_INVALID_ARG: a null pointer,
 * channels outside {3, 4}, a row_stride that is neither 0 nor at least
 * width*channels, sizes that are not positive or not below 65536. */
gz_status gz_process_frame(int device, const gz_params* params, const gz_frame* frame,
                           uint8_t** jpeg_out, size_t* jpeg_size, gz_process_stats* stats);
/* P itself (3*w*h bytes, host memory of the caller), produced by the code an
 * encode of `frame` uses. */
gz_status gz_frame_pack(int device, const gz_frame* frame, uint8_t* rgb_out);

/* ---- images: any strides, CHW / BGR / gray, 16-bit and float samples ---- */
typedef enum { GZ_SAMPLE_U8 = 0, GZ_SAMPLE_U16 = 1, GZ_SAMPLE_F16 = 2, GZ_SAMPLE_F32 = 3 } gz_sample;

/* An input image as the caller holds it, read where it lies.  Sample c of
 * pixel (x, y) is at data + y*row_stride + x*pixel_stride + channel_offset[c].
 * Strides are literal: there is no "0 means tight" here, a stride of 0 is a
 * broadcast.  One struct describes HWC and CHW; BGR, BGRA and ARGB (the
 * offsets); gray and gray + alpha; crops and step slices; bottom-up and
 * mirrored rows (negative strides); gray expanded to three channels (offsets
 * {0, 0, 0}).  The library reads the bytes of the addressed samples and no
 * other byte.
 *
 * The image that is encoded is the tight RGB8 image P.  A sample s becomes
 * 8 bits by q:
 *   u8   s
 *   u16  s >> 8 (what ReadPNG's STRIP_16 keeps)
 *   f32  NaN gives 0; otherwise rint(min(max(s, 0), 1) * 255), one IEEE f32
 *        multiply rounded to nearest with ties to even (0.5 gives 0, 1.5
 *        gives 2); -0, negatives and -inf give 0, values >= 1 and +inf 255
 *   f16  widened exactly to f32, then the f32 rule
 * and then, quantised first and blended second as ReadPNG does:
 *   3 channels  P = (q R, q G, q B)
 *   4 channels  P[c] = (q c * q A + 128) / 255
 *   1 channel   R = G = B = q V
 *   2 channels  R = G = B = (q V * q A + 128) / 255 */
typedef struct {
  const void* data;            /* the address every offset below is relative to */
  int width, height;
  int channels;                /* 1: gray, 2: gray + alpha, 3: RGB, 4: RGBA */
  int sample;                  /* gz_sample */
  ptrdiff_t row_stride;        /* bytes from a pixel to the one below it; any sign, may be 0 */
  ptrdiff_t pixel_stride;      /* bytes from a pixel to the one right of it; any sign, may be 0 */
  ptrdiff_t channel_offset[4]; /* bytes from a pixel's address to its R, G, B, A sample
                                  (gray: V, A); entries at index >= channels are ignored */
  int on_device;               /* 0: host memory, 1: HBM of the device the call names */
} gz_image;

/* The bytes gz_process_rgb returns for P.  A device image with both sides
 * >= 32 px is read in place by one import kernel (no repacking copy, no host
 * round trip); a smaller device image is packed by the same kernel into
 * 3*w*h bytes, a host image on the host.  GZ_ERR_INVALID_ARG, with the field
 * named: a null struct or null data; sizes that are not positive or not below
 * 65536; channels outside 1..4; sample outside the enum; data, a stride or a
 * used offset that is not a multiple of the sample size (every sample must be
 * naturally aligned). */
gz_status gz_process_image(int device, const gz_params* params, const gz_image* image,
                           uint8_t** jpeg_out, size_t* jpeg_size, gz_process_stats* stats);
/* P itself (3*w*h bytes, host memory of the caller), produced by the code an
 * encode of `image` uses. */
gz_status gz_image_pack(int device, const gz_image* image, uint8_t* rgb_out);

/* ---- encoder: a queue that keeps N encodes in flight ------------------- */
/* The library's throughput needs several frames in flight on a device (about
 * 8); a gz_encoder is the worker pool and result table for that.
 *  - Starting: jobs start in submission order on max_in_flight worker
 *    threads; each runs the code of gz_process_frame / gz_process_jpeg.
 *  - Lazy device use: creating an encoder does no device work and succeeds
 *    without a GPU; a job that needs one then fails on its own with
 *    GZ_ERR_DEVICE, and images under 32 px keep working.
 *  - Backpressure: submit blocks while queue_capacity accepted jobs have
 *    not started.
 *  - Inputs: params is copied at submit; the pixel or file memory is
 *    borrowed and must stay valid and unchanged until that job's result has
 *    been delivered.
 *  - Delivery: every result is delivered exactly once, by wait (that job) or
 *    by next (finished results in completion order).  next with block == 0
 *    and nothing finished returns GZ_OK with out->job == 0; with block == 1
 *    it waits for a result, or returns at once with job == 0 when nothing is
 *    outstanding, so `while (next(enc, 1, &r) == GZ_OK && r.job)` drains.
 *    wait on an id that is unknown or already delivered returns
 *    GZ_ERR_INVALID_ARG.  The return value of wait / next describes that
 *    call; the encode's own outcome is out->status and out->error.  A failed
 *    job never affects another.  Release a delivered result with
 *    gz_encode_result_free.
 *  - Threads: every entry point may be called from any threads at once,
 *    except that destroy must not race with other calls on its encoder.
 *  - Destroy: accepts nothing more, drops the jobs that have not started,
 *    lets running encodes finish (none is cancelled), frees undelivered
 *    results and returns when the workers have exited.
 *  - No exception leaves a worker thread, and the CPU check of the other
 *    entry points applies to every job.
 *  - One device per encoder: with several GPUs create one encoder each.
 * More than 8 same-size frames in flight make the engine pool create and
 * destroy the extra engines per frame (it keeps 8 idle per size). */
typedef struct gz_encoder gz_encoder;
typedef struct {
  int device;
  int max_in_flight;    /* frames encoding at once = worker threads; 0 = 8; clamped to [1, 32] */
  int queue_capacity;   /* accepted jobs not yet started; 0 = 2 * max_in_flight */
} gz_encoder_options;

typedef struct {
  uint64_t job;         /* id from submit; ids start at 1; 0 = "no result" */
  uint64_t tag;         /* the caller's */
  gz_status status;     /* of the encode */
  char* error;          /* NULL when status == GZ_OK */
  uint8_t* jpeg;
  size_t jpeg_size;
  gz_process_stats stats;
  double seconds_queued;   /* submit -> a worker took it */
  char* detail;            /* the JSON gz_last_process_detail would give */
} gz_encode_result;

gz_status gz_encoder_create(const gz_encoder_options* options, gz_encoder** out);
gz_status gz_encoder_submit(gz_encoder* enc, const gz_params* params, const gz_frame* frame,
                            uint64_t tag, uint64_t* job);
/* The same for an image (the struct is copied at submit, its memory is
 * borrowed until delivery); the job runs the code of gz_process_image. */
gz_status gz_encoder_submit_image(gz_encoder* enc, const gz_params* params, const gz_image* image,
                                  uint64_t tag, uint64_t* job);
/* PNG or JPEG file bytes: a PNG is decoded (gz_png_decode) and encoded from
 * its RGB, anything else is taken as a JPEG file (gz_process_jpeg). */
gz_status gz_encoder_submit_file(gz_encoder* enc, const gz_params* params, const uint8_t* data,
                                 size_t len, uint64_t tag, uint64_t* job);
gz_status gz_encoder_wait(gz_encoder* enc, uint64_t job, gz_encode_result* out);
gz_status gz_encoder_next(gz_encoder* enc, int block, gz_encode_result* out);
/* Frees error, jpeg and detail and zeroes the struct. */
void gz_encode_result_free(gz_encode_result* result);
void gz_encoder_destroy(gz_encoder* enc);

/* Encodes a JPEG file: guetzli::Process(params, stats, jpeg_bytes, out)
 * (guetzli/processor.h:44-46, processor.cc:1029-1066) -- the input's own
 * coefficients and quantization start the search, its decoded pixels are the
 * Butteraugli reference.  Baseline / extended / progressive Huffman JPEGs with
 * 4:4:4 or 4:2:0 YCbCr sampling (4:2:0 forces the downsampled search); other
 * layouts and 1-component files return GZ_ERR_UNSUPPORTED (the reference's
 * Process returns false for them), unreadable input GZ_ERR_INVALID_ARG.  *jpeg_out: library-allocated
 * (gz_free). */
gz_status gz_process_jpeg(int device, const gz_params* params, const uint8_t* jpeg, size_t jpeg_len,
                          uint8_t** jpeg_out, size_t* jpeg_size, gz_process_stats* stats);
/* ReadJpeg (guetzli/jpeg_data_reader.cc:931-1079, JPEG_READ_ALL) and
 * DecodeJpegToRGB (jpeg_data_decoder.cc:45-55) of a JPEG file, host only:
 * *coeffs_out the quantized coefficients of every component ([comp][blocks]
 * [64], natural order, MCU-padded grid; *ncoeffs values), *rgb_out the RGB8
 * image for 4:4:4 and 4:2:0 YCbCr inputs, else NULL.  Both library-allocated (gz_free). */
gz_status gz_jpeg_decode(const uint8_t* jpeg, size_t jpeg_len, int* width, int* height,
                         int* ncomp, int16_t** coeffs_out, size_t* ncoeffs, uint8_t** rgb_out);

/* ReadPNG of the reference CLI (guetzli/guetzli.cc:51-156; libpng with
 * PACKING | EXPAND | STRIP_16, alpha blended on black), host only: every PNG
 * colour type and bit depth, interlaced or not, tRNS.  *rgb_out: RGB8,
 * 3*w*h bytes, library-allocated (gz_free).  GZ_ERR_INVALID_ARG for what
 * ReadPNG rejects (the CLI then fails, guetzli.cc:326-330). */
gz_status gz_png_decode(const uint8_t* png, size_t png_len, int* width, int* height,
                        uint8_t** rgb_out);

/* ---- one frame over several GPUs (row strips + halo) ------------------ */
/* The exchange a multi-rank encode needs: an equal-size all-gather (every
 * rank contributes `bytes` bytes, `recv` receives world*bytes in rank order);
 * returns 0 on success.  Bound to torch.distributed (RCCL over xGMI, or gloo)
 * by the Python package. */
typedef struct {
  void* ctx;
  int rank;
  int world;
  int (*allgather)(void* ctx, const void* send, size_t bytes, void* recv);
} gz_collectives;
/* guetzli::Process (processor.h:62-64) for one frame whose Butteraugli passes
 * are split over the ranks of `coll` by rows: every rank passes the whole
 * RGB frame (host memory) and its own device, and receives the same bytes as
 * gz_process_rgb.  A rank computes its owned rows plus a 96-row halo. */
gz_status gz_process_rgb_strips(int device, const gz_params* params, const uint8_t* rgb, int width,
                                int height, const gz_collectives* coll, uint8_t** jpeg_out,
                                size_t* jpeg_size, gz_process_stats* stats);
/* Rows rank `rank` owns [y0, y1) and computes [e0, e1). */
gz_status gz_strip_layout(int width, int height, int world, int rank, int* y0, int* y1, int* e0,
                          int* e1);
/* Exercises `coll` (fixed- and variable-size gathers); GZ_OK if consistent. */
gz_status gz_collectives_selftest(const gz_collectives* coll);
/* gz_collectives over RCCL (NCCL's API on ROCm: all-gathers over xGMI
 * between the GPUs of a node), for C/C++ callers running one process per
 * GPU without torch.distributed (the reference has no collectives,
 * SURVEY.md §5).  One rank calls gz_rccl_unique_id and
 * hands the 128 bytes to the others by its own means (MPI, a file, a
 * socket); every rank then calls gz_rccl_create (ncclCommInitRank: returns
 * when all have), which fills *coll for gz_process_rgb_strips.  RCCL is
 * loaded on first use: the librccl beside the HIP runtime the process has
 * mapped (torch's own in a process that imported torch, else ROCm's), then
 * librccl.so.1 from the search path.  gz_rccl_destroy after the last encode
 * that uses *coll. */
typedef struct gz_rccl gz_rccl;
gz_status gz_rccl_unique_id(uint8_t id[128]);
gz_status gz_rccl_create(int device, int rank, int world, const uint8_t id[128], gz_rccl** out,
                         gz_collectives* coll);
void gz_rccl_destroy(gz_rccl* comm);
/* Path of the librccl loaded (empty before the first gz_rccl_* call or if
 * none could be loaded). */
const char* gz_rccl_library(void);

/* ---- comparator (guetzli::ButteraugliComparator) ---------------------- */
/* ButteraugliComparator(w, h, rgb, target, stats) ctor
 * (guetzli/butteraugli_comparator.cc:48-58); width, height >= 8. */
gz_status gz_comparator_create(int device, int width, int height, const uint8_t* rgb,
                               float target_distance, gz_comparator** out);
void gz_comparator_destroy(gz_comparator* cmp);
/* Comparator::Compare (guetzli/butteraugli_comparator.cc:60-70) on the image
 * whose DCT coefficients are `coeffs`; distance = distmap_aggregate(). */
gz_status gz_comparator_compare(gz_comparator* cmp, const int16_t* coeffs, float* distance);
/* Comparator::Compare of an image given as its sRGB pixels (3*w*h bytes,
 * RGB interleaved -- OutputImage::ToSRGB(), output_image.cc:654-701): the
 * entry for images whose pixels are not a function of their coefficients
 * alone (4:2:0: the subsampled components' upsampled pixels are state). */
gz_status gz_comparator_compare_rgb(gz_comparator* cmp, const uint8_t* rgb, float* distance);
/* Compare of a 4:2:0 candidate (OutputImage with factor-2 chroma,
 * output_image.cc:642-716): Y coefficients ([blocks][64]), Cb / Cr
 * coefficients ([ceil(w/16)*ceil(h/16)][64] each; NULL = zeros -- the
 * Compare pass reads the chroma from the planes) and the factor-2 components'
 * 16-bit pixel state (w*h each, wrapping: ToPixels' byte is
 * ((p + 8 - (x & 1)) >> 4) & 0xff, output_image.cc:83). */
gz_status gz_comparator_compare_420(gz_comparator* cmp, const int16_t* y, const int16_t* cb,
                                    const int16_t* cr, const uint16_t* plane_cb, const uint16_t* plane_cr,
                                    float* distance);
/* Same, with stage dumps. */
gz_status gz_comparator_compare_stages(gz_comparator* cmp, const int16_t* coeffs,
                                       gz_compare_stages* stages, float* distance);
/* Same, dumped from the search's own (fused) kernel variants instead of the
 * stand-alone dump kernels -- the corner edge term as k_block_diff leaves it,
 * block_ac before the low-frequency term, the distance map after the fused
 * combine (low-frequency term, subsampled B mask, LUT'd mask samples).  Only
 * mhic0, mhic1, edge, block_dc, block_ac and distmap may be non-NULL
 * (GZ_ERR_INVALID_ARG otherwise).  Parity evidence for the kernels the search
 * runs (clbutter_comparator.cpp:1387-1417). */
gz_status gz_comparator_compare_stages_production(gz_comparator* cmp, const int16_t* coeffs,
                                                  gz_compare_stages* stages, float* distance);
/* EncodeRGBToJpeg's q=1 coefficients of the comparator's reference image
 * ([3][blocks][64] int16, natural order) computed on the device: YUV16 +
 * integer FDCT + q=1 quantizer (guetzli/jpeg_data_encoder.cc:66-136,
 * guetzli/fdct.cc). */
gz_status gz_comparator_original_coeffs(gz_comparator* cmp, int16_t* out);
/* Comparator::distmap() (comparator.h:71-75): the distance map of the last
 * gz_comparator_compare (w*h floats; recomputed on the device from the same
 * candidate -- the search's own passes keep only per-block maxima). */
gz_status gz_comparator_distmap(gz_comparator* cmp, float* out);
/* Per-8x8-block maxima of the last distance map (ceil(w/8)*ceil(h/8)). */
gz_status gz_comparator_block_max(gz_comparator* cmp, float* out);
/* ComputeBlockErrorAdjustmentWeights (butteraugli_comparator.cc:169-233) on
 * the host: per-(8*factor)-block maxima of `distmap` (width*height floats),
 * then the neighbourhood weights.  block_weight (one float per block) is
 * updated in place -- the caller zero-fills it first, as the search loop does
 * (processor.cc:779-783).  No device needed. */
gz_status gz_block_error_adjustment_weights(int width, int height, float target, int direction,
                                            int max_block_dist, double target_mul, int factor_x,
                                            int factor_y, const float* distmap,
                                            float* block_weight);
/* Comparator::DistanceOK (butteraugli_comparator.h:52-54). */
int gz_comparator_distance_ok(gz_comparator* cmp, double target_mul);
/* Comparator::ScoreOutputSize (butteraugli_comparator.cc:235-237). */
double gz_comparator_score_output_size(gz_comparator* cmp, int size);
/* StartBlockComparisons (butteraugli_comparator.cc:72-79); mask_scale may be
 * NULL, else receives 3 floats per block (mask_xyz at the block corner). */
gz_status gz_comparator_start_block_comparisons(gz_comparator* cmp, float* mask_scale);
/* Batched per-block greedy zeroing of SelectFrequencyMasking's CPU_OPT loop
 * (processor.cc:376-487, 641-672) for the candidate `cur_coeffs` against
 * the original q=1 coefficients `orig_coeffs`; out: blocks*192 entries,
 * zero-filled tails.  Replaces cuComputeBlockZeroingOrder
 * (clguetzli/cuguetzli.h:30-40).  comp_mask: components searched (the
 * others keep cur_coeffs' values in the pixels); lookahead /
 * new_zeroing_model: Params::zeroing_greedy_lookahead / new_zeroing_model
 * (0: the old candidate key of processor.cc:400-405). */
gz_status gz_comparator_block_zeroing_orders(gz_comparator* cmp, const int16_t* cur_coeffs,
                                             const int16_t* orig_coeffs, int comp_mask,
                                             float limit, int lookahead, int new_zeroing_model,
                                             gz_coeff_data* out);

/* SwitchBlock(bx, by, 1, 1) + CompareBlock(img, 0, 0, candidate, comp_mask)
 * (butteraugli_comparator.cc:85-163) for n requests at once: request i
 * compares 8x8 block blocks[i] (row-major block index) of the reference image
 * with candidate coefficients cand[192*i ..] -- [3][64], natural order,
 * dequantized, every component as the image holds it (the masked
 * components' candidate values, the image's current values for the others)
 * -- and err[i] receives CompareBlock's double.  Uses the activity mask of
 * StartBlockComparisons (run first if needed).  The per-block entry of the
 * comparator-level drop-in; the search itself uses the
 * batched gz_comparator_block_zeroing_orders. */
gz_status gz_comparator_compare_blocks(gz_comparator* cmp, int n, const int* blocks,
                                       const int16_t* cand, double* err);
/* The same with each candidate given as its 8x8 sRGB window rgb[192*i ..]
 * (row major, RGB interleaved, as OutputImage::ToSRGB(8 bx, 8 by, 8, 8)
 * returns it, edge pixels replicated): CompareBlock(img, off_x, off_y, ...)
 * of any image, subsampled components included (butteraugli_comparator.cc:
 * 113-163 reads the image only through ToLinearRGB). */
gz_status gz_comparator_compare_blocks_rgb(gz_comparator* cmp, int n, const int* blocks,
                                           const uint8_t* rgb, double* err);

/* SaveToJpegData + WriteJpeg (guetzli/output_image.cc:579-640,
 * jpeg_data_writer.cc:540-553) of dequantized coefficients `coeffs`
 * ([3][blocks][64], multiples of quant) with quant tables `quant` ([3][64],
 * natural order), entropy coded on the comparator's device; metadata
 * stripped.  *jpeg_out is allocated by the library (gz_free).
 *
 * The coefficient domain.  A JPEG input may carry any |coefficient x quant|
 * <= 4096 at every position (CheckJpegSanity, processor.cc:118-131) -- four
 * times the range of the coefficients of 8-bit pixels -- and the entropy
 * coders are sized for exactly that: AC symbols of at most 13 bits, DC
 * differences of at most 14.  Both writer entries refuse a coefficient
 * outside [-4096, 4096] with GZ_ERR_INVALID_ARG, on the host, before
 * anything is uploaded or launched.  The other comparator entries (compare*,
 * compare_blocks, block_zeroing_orders) take any int16: their integer IDCT
 * wraps as the reference's does (idct.cc: a 32-bit sum, an int16 column
 * pass), so they stay defined on every input; the tests pin them against
 * that arithmetic for |coefficient| <= 4096. */
gz_status gz_comparator_write_jpeg(gz_comparator* cmp, const int16_t* coeffs, const int* quant,
                                   uint8_t** jpeg_out, size_t* jpeg_size);
/* The same on the host (the library's serial writer; no device needed). */
gz_status gz_write_jpeg_host(int width, int height, const int16_t* coeffs, const int* quant,
                             uint8_t** jpeg_out, size_t* jpeg_size);

/* ---- device memory ---------------------------------------------------- */
/* Encodes keep their per-size engines (HBM buffers, stream, graph) in a
 * process-wide pool for reuse: least recently used first out, capped at
 * GZ_ENGINE_POOL_BYTES (environment, default 16 GiB) and 8 per image size;
 * engines whose last operation failed are never pooled.  trim destroys idle
 * engines until at most keep_bytes remain and returns the bytes released. */
size_t gz_engine_pool_trim(size_t keep_bytes);
size_t gz_engine_pool_idle_bytes(void);

/* ---- measurement ------------------------------------------------------ */
/* Per-launch timing with HIP events on each object's own stream (off by
 * default).  Regions are named after the pass stage ("block_diff",
 * "mask_blur_h", "block_zeroing", ... and "compare_pass" for a whole
 * Butteraugli pass). */
void gz_profile_enable(int enable);
void gz_profile_reset(void);
/* Returns 1 and fills count / total milliseconds if `name` was recorded. */
int gz_profile_get(const char* name, long* count, double* total_ms);
/* Comma-separated recorded region names; returns the length needed. */
size_t gz_profile_names(char* buf, size_t cap);
/* JSON object of host-side timers / counters of this thread's last encode;
 * returns the length needed. */
size_t gz_last_process_detail(char* buf, size_t cap);

/* ---- helpers used by the host search loop ----------------------------- */
/* Synthetic sRGB test frame (SURVEY.md §8d generator), 3*w*h bytes. */
gz_status gz_synthetic_frame(uint64_t seed, int width, int height, uint8_t* rgb_out);
/* EncodeRGBToJpeg at q=1 (guetzli/jpeg_data_encoder.cc:66-136): coefficient
 * planes [3][blocks][64]. */
gz_status gz_rgb_to_coeffs(const uint8_t* rgb, int width, int height, int16_t* coeffs_out);

#ifdef __cplusplus
}
#endif

#endif /* GUETZLI_HIP_H_ */
