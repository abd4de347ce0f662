/* libstereotrack_hip - the JPEG reader's ABI.
 *
 * A header of its own beside stereotrack.h, same conventions:
 *   - every function returns 0 on success, a negative status otherwise, and st_last_error() (stereotrack.h) holds the
 *     message of the calling thread's last failure;
 *   - structs start with struct_size = sizeof(the struct) as the caller compiled it; another value is refused;
 *   - `_dev` pointers are device memory, everything else is host memory;
 *   - the one launch entry takes the stream as its last argument, enqueues on it and never waits for the device.
 *
 * What "decode" means: baseline / extended-sequential Huffman JPEG (SOF0, SOF1), 8-bit samples, one scan; gray, or
 * YCbCr with luma sampling 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and 1x1 chroma.  The arithmetic is libjpeg-turbo's
 * default decode: the JDCT_ISLOW inverse DCT, "fancy" chroma upsampling, the 16-bit fixed-point YCbCr -> RGB conversion
 * (csrc/jpeg_core.h is the one text of it, for the host and the device).  Everything else is refused:
 *   ST_ERR_UNSUPPORTED  a JPEG feature outside that set (progressive, arithmetic, lossless, 12-bit, CMYK / 4 components,
 *                       Adobe transform 0, other sampling factors, several scans); the message names the feature
 *   ST_ERR_INVALID      not a JPEG, a bad segment, truncated or corrupt entropy data (nothing is filled with zeros)
 */
#ifndef STEREOTRACK_JPEG_H_
#define STEREOTRACK_JPEG_H_

#include <stddef.h>
#include <stdint.h>

#include "stereotrack.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ST_ERR_UNSUPPORTED (-6) /* a valid file that uses a feature this decoder does not have */

enum StJpegSampling {
  ST_JPEG_GRAY = 0, /* one component                        */
  ST_JPEG_444 = 1,  /* Y 1x1, Cb 1x1, Cr 1x1                */
  ST_JPEG_422 = 2,  /* Y 2x1: chroma at half width          */
  ST_JPEG_420 = 3   /* Y 2x2: chroma at half width, height  */
};

typedef struct StJpegInfo {
  int struct_size;
  int height, width;    /* of the image, 1 .. 65535 */
  int components;       /* 1 or 3 */
  int sampling;         /* StJpegSampling */
  int restart_interval; /* MCUs between RSTn markers, 0 = none */
  int mcus_x, mcus_y;   /* MCU grid (an MCU covers 8x8, 16x8 or 16x16 pixels) */
  int blocks_w[3];      /* 8x8-block grid of each component, padded to whole MCUs */
  int blocks_h[3];
  int comp_w[3];        /* true sample size of each component: ceil(width / 2) where subsampled */
  int comp_h[3];
  int reserved;
  size_t coef_offset[3]; /* first int16 of each component in the coefficient array */
  size_t coef_count;     /* int16 elements of one image: 64 * sum(blocks_w * blocks_h) */
  size_t coef_bytes;     /* coef_count * 2: what the caller allocates for st_jpeg_entropy_decode */
  size_t work_bytes;     /* device work memory of ONE image for st_jpeg_reconstruct (st_jpeg_work_bytes(info, 1)) */
} StJpegInfo;

/* Marker parse only (up to and including the scan header): fills *info (info->struct_size set by the caller). */
int st_jpeg_info(const uint8_t* data, size_t nbytes, StJpegInfo* info);

/* Entropy decode of the whole scan into caller memory; allocates nothing, keeps no global state, reentrant.
 *   coef_out   coef_count int16: the QUANTISED coefficients in natural (de-zigzagged) order,
 *              [component][block_row][block_col][64] over the padded block grids of st_jpeg_info; every element is
 *              written (also on failure paths nothing outside it is)
 *   quant_out  3 x 64 uint16: the quantisation table of each component in natural order (components a gray file does
 *              not have are zero) */
int st_jpeg_entropy_decode(const uint8_t* data, size_t nbytes, int16_t* coef_out, uint16_t* quant_out);

/* Dequantise, inverse DCT, upsample, convert - on the host, in plain C++: the CPU product path and the executable
 * specification of the kernels.  Writes sample (y, x) of plane p (0, 1, 2 = B, G, R; rgb_order != 0: R, G, B) to
 * out[p * plane_stride + y * row_stride + x * pixel_stride] (strides in bytes), y < height, x < width only.  Gray gives
 * three equal planes.  `info` must be what st_jpeg_info returns for its width / height / components / sampling: both
 * reconstruction entries index memory with its grids and refuse any other struct (ST_ERR_INVALID). */
int st_jpeg_reconstruct_host(const int16_t* coef, const uint16_t* quant, const StJpegInfo* info, uint8_t* out,
                             ptrdiff_t plane_stride, ptrdiff_t row_stride, ptrdiff_t pixel_stride, int rgb_order);

/* Device work memory (component planes) of a batch of N images of this geometry; 0 on a bad argument. */
size_t st_jpeg_work_bytes(const StJpegInfo* info, int N);

/* The same on the device for N images of ONE geometry and sampling class, two launches on `stream`:
 *   coef_dev   N x coef_count int16 (image n at n * coef_count), 16-byte aligned
 *   quant_dev  N x 3 x 64 uint16, one set of tables per image, 16-byte aligned
 *   work_dev   work_bytes >= st_jpeg_work_bytes(info, N), 16-byte aligned; arbitrary bits before, garbage after
 *   out_dev    uint8, sample (y, x) of plane p of image n at n * image_stride + p * plane_stride + y * row_stride + x
 *              (strides in bytes, row_stride >= width); only y < height, x < width is written
 * Reads nothing outside those extents, never waits for the device.  Results equal st_jpeg_reconstruct_host's, byte for
 * byte, for every int16 coefficient and uint16 table value. */
int st_jpeg_reconstruct(const int16_t* coef_dev, const uint16_t* quant_dev, int N, const StJpegInfo* info, void* work_dev,
                        size_t work_bytes, uint8_t* out_dev, ptrdiff_t image_stride, ptrdiff_t plane_stride,
                        ptrdiff_t row_stride, int rgb_order, st_stream_t stream);

/* ---- entropy decode on the device (opt-in; DESIGN.md 25 "Entropy decode on the device") -----------------------------
 *
 * st_jpeg_entropy_decode above is the specification: for every byte string the device path gives the same coefficients,
 * the same tables and the same accept / refuse verdict.  The host only parses the headers (st_jpeg_entropy_prepare,
 * O(header)) and copies the scan bytes; markers inside the scan are found on the device.
 *
 * One call takes ONE blob, the same bytes in page-locked host memory and (after the caller's H2D copy, enqueued on the
 * same stream in front of the call) in device memory:
 *   [0, N * sizeof(StJpegEntropyDesc))   the descriptors, image n at n * sizeof(StJpegEntropyDesc)
 *   desc[n].blob_offset ...              the file's bytes from scan_offset to its end (scan_bytes of them), at a
 *                                        16-byte aligned offset the caller chooses and writes into the descriptor */
typedef struct StJpegHuffLut {
  uint16_t fast[512];  /* 9-bit prefix -> (length << 8) | symbol, 0 = longer than 9 bits */
  int32_t maxcode[18]; /* largest code of each length, -1 = none; [17] = INT32_MAX */
  int32_t valptr[17], mincode[17];
  uint8_t vals[256];
} StJpegHuffLut;

typedef struct StJpegEntropyDesc {
  int struct_size;
  int components, sampling, restart_interval; /* as in StJpegInfo */
  int mcus_x, mcus_y;
  int dc_slot[3], ac_slot[3]; /* component -> index into dc[] / ac[] */
  unsigned scan_offset;       /* first entropy-coded byte in the file */
  unsigned scan_bytes;        /* file bytes from there to the end of the file (trailing markers included) */
  unsigned blob_offset;       /* where the caller put those bytes in the blob; st_jpeg_entropy_prepare writes 0 */
  int reserved;
  uint16_t quant[3][64]; /* natural order, per component (absent components: zero) */
  StJpegHuffLut dc[3], ac[3];
} StJpegEntropyDesc;

typedef struct StJpegEntropyTuning {
  int struct_size;
  int subseq_bytes; /* raw scan bytes per thread, 8 .. 512; 0 = default (32) */
  int tile;         /* subsequences per tile, 1 .. 256; 0 = default (256); subseq_bytes * tile <= 32768 */
} StJpegEntropyTuning;

typedef struct StJpegEntropyStats { /* one per image, at the start of the work memory */
  int tiles, subsequences;
  int max_passes; /* most decode passes any tile needed before its exits settled (>= 1; 0 for an empty scan) */
  int sum_passes; /* over all tiles */
} StJpegEntropyStats;

/* Header parse of one file into *desc (desc->struct_size set by the caller).  Refuses exactly what st_jpeg_info and the
 * table checks of st_jpeg_entropy_decode refuse, with the same status and message (and files of 256 MiB and more: raw
 * bit positions are 32-bit); never reads the scan bytes. */
int st_jpeg_entropy_prepare(const uint8_t* data, size_t nbytes, StJpegEntropyDesc* desc);

/* Device work memory of a call over N images: N StJpegEntropyStats, rounded up to 256 bytes; 0 on a bad argument. */
size_t st_jpeg_entropy_work_bytes(const StJpegInfo* info, int N);

/* Entropy decode of N images of ONE geometry and sampling class on `stream` (two launches, no wait, no D2H copy):
 *   blob_host    the blob in host memory: only its descriptors are read, to refuse on the host, before any launch, a
 *                descriptor that does not match *info or whose scan does not lie inside [N * sizeof(desc), blob_bytes)
 *   blob_dev     the same blob on the device, 16-byte aligned
 *   coef_dev     N x coef_count int16, the layout of st_jpeg_entropy_decode; every element of an accepted image is
 *                written, a refused image's are unspecified (nothing outside its own extent is written)
 *   quant_dev    N x 3 x 64 uint16
 *   status_dev   N int32: 0 = accepted, non-zero (ST_JPEG_E_* bits) exactly when st_jpeg_entropy_decode refuses the
 *                file's entropy data
 *   work_dev     >= st_jpeg_entropy_work_bytes(info, N), 16-byte aligned; arbitrary bits before, the stats after
 *   tuning       NULL = defaults
 * Reads nothing outside the blob, writes nothing outside coef / quant / status / work. */
#define ST_JPEG_E_CODE 1      /* a code not in the table */
#define ST_JPEG_E_RUN 2       /* a run past coefficient 63, a ZRL past 64 */
#define ST_JPEG_E_DC 4        /* a DC predictor outside int16 */
#define ST_JPEG_E_SHORT 8     /* the data (or a restart interval) ends before its MCUs do */
#define ST_JPEG_E_LEFTOVER 16 /* 8 or more bits before an expected RSTn */
#define ST_JPEG_E_MARKER 32   /* the expected RSTn is missing or misnumbered */
int st_jpeg_entropy_decode_dev(const uint8_t* blob_host, const uint8_t* blob_dev, size_t blob_bytes, int N,
                               const StJpegInfo* info, const StJpegEntropyTuning* tuning, int16_t* coef_dev,
                               uint16_t* quant_dev, int32_t* status_dev, void* work_dev, size_t work_bytes,
                               st_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* STEREOTRACK_JPEG_H_ */
