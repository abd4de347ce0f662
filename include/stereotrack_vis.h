/* libstereotrack_hip - the annotated-frame writer's ABI: the JPEG forward path and the track
 * overlay.
 *
 * A header of its own beside stereotrack_jpeg.h, same conventions:
 *   - every function returns 0 on success, a negative status otherwise, and st_last_error() (stereotrack.h) holds the
 *     message of the calling thread's last failure;
 *   - structs start with struct_size = sizeof(the struct) as the caller compiled it; another value is refused;
 *   - `_dev` pointers are device memory, everything else is host memory;
 *   - the launch entries take the stream as their last argument, enqueue on it and never wait for the device.
 *
 * What "encode" means: baseline JFIF (SOF0), 8-bit, one scan, the Annex K Huffman tables; gray, or YCbCr 4:4:4 / 4:2:2 /
 * 4:2:0.  The arithmetic is libjpeg-turbo's default compress path (csrc/jpeg_fwd_core.h is the one text of it, for the
 * host and the device) and the file's bytes are what libjpeg-turbo writes for the same pixels, quality and sampling.
 * The encoder shares the reader's StJpegInfo: block grids padded to whole MCUs, coefficients as
 * [component][block_row][block_col][64] int16 in natural order.
 */
#ifndef STEREOTRACK_VIS_H_
#define STEREOTRACK_VIS_H_

#include <stddef.h>
#include <stdint.h>

#include "stereotrack_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fills *info (info->struct_size set by the caller) for an image to be written: height, width 1 .. 65535; components 1
 * with ST_JPEG_GRAY, or 3 with ST_JPEG_444 / 422 / 420; restart_interval 0 .. 65535 MCUs.  The result is what
 * st_jpeg_info returns for the written file. */
int st_jpeg_encode_geometry(int height, int width, int components, int sampling, int restart_interval, StJpegInfo* info);

/* The Annex K quantisation tables at IJG `quality` (clamped to 1 .. 100, baseline: entries 1 .. 255) ->
 * quant_out, 3 x 64 uint16 in natural order, one table per component (luma, chroma, chroma). */
int st_jpeg_quant_tables(int quality, uint16_t* quant_out);

/* Pixels -> quantised coefficients on the host, in plain C++: the CPU product path and the executable specification of
 * st_jpeg_forward.  Sample (y, x) of plane p (0, 1, 2 = B, G, R; rgb_order != 0: R, G, B; one plane for gray) is read
 * from pixels[p * plane_stride + y * row_stride + x * pixel_stride] (strides in bytes), y < height, x < width only.
 *   quant     3 x 64 uint16, natural order, per component (an entry of 0 counts as 1)
 *   coef_out  info->coef_count int16, every element written: dummy blocks (beyond ceil(true size / 8) of the padded
 *             grid) carry AC 0 and the DC of the previous block of their MCU */
int st_jpeg_forward_host(const uint8_t* pixels, ptrdiff_t plane_stride, ptrdiff_t row_stride, ptrdiff_t pixel_stride,
                         int rgb_order, const uint16_t* quant, const StJpegInfo* info, int16_t* coef_out);

/* The same on the device for N images of ONE geometry, one launch on `stream`:
 *   in_dev     uint8, sample (y, x) of plane p of image n at n * image_stride + p * plane_stride + y * row_stride + x
 *              (strides in bytes, row_stride >= width); only y < height, x < width is read, byte by byte
 *   quant_dev  3 x 64 uint16, ONE set of tables for the batch, 16-byte aligned
 *   coef_dev   N x coef_count int16 (image n at n * coef_count), 16-byte aligned; every element is written
 * Writes nothing else, needs no work memory, never waits for the device.  Results equal st_jpeg_forward_host's for
 * every pixel and every uint16 table value. */
int st_jpeg_forward(const uint8_t* in_dev, ptrdiff_t image_stride, ptrdiff_t plane_stride, ptrdiff_t row_stride,
                    int rgb_order, const uint16_t* quant_dev, int N, const StJpegInfo* info, int16_t* coef_dev,
                    st_stream_t stream);

/* Capacity that st_jpeg_entropy_encode asks for: 1024 bytes of headers, 416 per block (64 coefficients of at most 26
 * bits, every byte stuffed) and 4 per MCU (padding and a restart marker).  0 on a bad argument. */
size_t st_jpeg_encode_bound(const StJpegInfo* info);

/* Coefficients, tables and geometry -> the whole file (SOI .. EOI) in caller memory.  Host code; allocates nothing, keeps
 * no global state, reentrant.
 *   coef       info->coef_count int16 in the layout above (DC -1024 .. 1023 quantised, |AC| <= 1023; others are refused)
 *   quant      3 x 64 uint16, entries 1 .. 255 (baseline)
 *   out        capacity bytes; capacity < st_jpeg_encode_bound(info) is refused with ST_ERR_WORKSPACE
 *   out_bytes  the file's length */
int st_jpeg_entropy_encode(const int16_t* coef, const uint16_t* quant, const StJpegInfo* info, uint8_t* out,
                           size_t capacity, size_t* out_bytes);

/* ---- track overlay ---------------------------------------------------------------------------------------------------
 *
 * One box: an outline `line_width` pixels wide centred on the edges of the box rounded to the nearest pixel, and (label_len
 * > 0) a tag: a filled rectangle at (x1, y1) + line_width that carries the label in black, in the built-in 5x7 font at
 * `zoom`, with a margin of one font cell: (6 * label_len + 1) * zoom by 9 * zoom pixels.  Outline and tag background are
 * blended: out = (a * colour + (256 - a) * pixel + 128) >> 8; the ink is opaque.  Glyphs: 0-9 . | - and space; any
 * other byte draws as space. */
#define ST_DRAW_LABEL_MAX 15

typedef struct StDrawBox {
  float x1, y1, x2, y2;  /* a box with a non-finite coordinate, or x2 < x1 or y2 < y1 after rounding, draws nothing */
  uint8_t colour[3];     /* per PLANE of the frame (plane 0 first) */
  uint8_t zoom;          /* 1 .. 8 (0 counts as 1) */
  uint8_t label_len;     /* 0 .. ST_DRAW_LABEL_MAX */
  uint8_t label[ST_DRAW_LABEL_MAX];
} StDrawBox; /* 36 bytes, read field by field */

/* Draws in place into N uint8 planar frames (3 planes), one launch on `stream` (none when max_boxes is 0):
 *   frames_dev  sample (y, x) of plane p of frame n at n * image_stride + p * plane_stride + y * row_stride + x (bytes);
 *               only y < height, x < width is read or written, byte by byte
 *   boxes_dev   N x max_boxes StDrawBox, 4-byte aligned
 *   counts_dev  N int32: boxes of frame n (clamped to 0 .. max_boxes)
 *   line_width  1 .. 64;  alpha256 = round(alpha * 256), 0 .. 256
 * Boxes apply in list order, one thread owns one pixel: the result does not depend on the launch geometry. */
int st_draw_tracks(uint8_t* frames_dev, int N, int height, int width, ptrdiff_t image_stride, ptrdiff_t plane_stride,
                   ptrdiff_t row_stride, const StDrawBox* boxes_dev, const int32_t* counts_dev, int max_boxes,
                   int line_width, int alpha256, st_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* STEREOTRACK_VIS_H_ */
