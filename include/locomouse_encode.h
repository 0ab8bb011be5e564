/* locomouse_encode.h — baseline JPEG encoding on the device, and the overlay
 * that draws tracks on the corrected frame: the two stages behind the annotated
 * preview video (LM_PREVIEW).  Part of liblocomouse_hip.so;
 * statuses and lm_last_error are locomouse_hip.h's.
 *
 * The encoder is sequential Huffman JPEG, 8-bit, with the Annex K tables: one
 * grey component, or RGB24 as YCbCr 4:2:0.  Every frame's file, SOI to EOI, is
 * byte for byte what host/JpegEncode.hpp's encode_jpeg writes (and so what
 * libjpeg writes with its defaults at that quality), whatever else is in the
 * batch, whatever max_batch is, and whatever was encoded before.
 *
 * Buffer sizes.  With the Annex K tables a block's entropy-coded bits are at
 * most 22 for the DC coefficient (an 11-bit code and an 11-bit value) and 26
 * for each of the 63 AC coefficients (a 16-bit code and a 10-bit value; a ZRL
 * or EOB code is no longer than the coefficients it stands for): 1660 bits,
 * held in LM_ENC_BLOCK_WORDS = 52 words of 32 bits.  A frame of B blocks has
 * an unstuffed stream of at most 52 * B words (plus one spare).  Byte stuffing
 * at most doubles it, the header (SOI .. SOS) is at most LM_ENC_MAX_HEADER
 * bytes and EOI is 2:
 *
 *   lm_enc_slot_bytes = LM_ENC_MAX_HEADER + 2 * 4 * (52 * B + 1) + 2
 *
 * Every device buffer is sized from this worst case, so no frame can overflow
 * and there is no overflow path.  B is ceil(rows / 8) * ceil(cols / 8) for
 * grey and 6 * ceil(rows / 16) * ceil(cols / 16) for colour.
 *
 * Restart intervals (lm_enc_create_restart).  With a restart interval of Ri
 * MCUs (an MCU is one block for grey and six for colour) the scan has
 * I = ceil(MCUs / Ri) intervals.  Every interval but the last ends in a 1-bit
 * fill to a byte boundary, at most 7 bits, and an unstuffed 2-byte marker; the
 * last ends in the frame's own fill, at most 7 bits as before.  The bound above
 * spends 52 * 32 - 1660 = 4 spare bits per block on the frame's one fill, which
 * an interval of one block outgrows: 1660 + 7 bits.  So the fills get words of
 * their own, a byte each:
 *
 *   unstuffed bits  <= 1660 * B + 7 * I <= 32 * (52 * B + ceil(I / 4))
 *   W               =  52 * B + ceil(I / 4) + 1 words (one spare, as above)
 *   lm_enc_slot_bytes_restart = LM_ENC_MAX_HEADER + 2 * 4 * W + 2 * (I - 1) + 2
 *
 * that is at most 415 * B + 4 per interval of stream: a fill byte may be FF and
 * is stuffed like any other (2 bytes), and the marker is 2.  The header with
 * its DRI segment is 629 bytes.  Every device buffer of such a context is sized
 * from this bound, so again no frame can overflow. */
#ifndef LOCOMOUSE_ENCODE_H
#define LOCOMOUSE_ENCODE_H

#include <stddef.h>
#include <stdint.h>

#include "locomouse_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LM_ENC_GRAY8 0 /* a frame is rows x cols u8 */
#define LM_ENC_RGB24 1 /* a frame is rows x cols x 3 u8 (R, G, B), encoded as YCbCr 4:2:0 */

#define LM_ENC_BLOCK_WORDS 52
#define LM_ENC_MAX_HEADER 640
#define LM_ENC_MAX_BLOCKS (1 << 20) /* blocks of one frame (the bit offsets stay below 2^31) */
#define LM_ENC_MAX_BATCH 4096
#define LM_ENC_MAX_RADIUS 64

/* The overlay's colours (R, G, B), by a mark's colour index. */
#define LM_ENC_PALETTE_SIZE 8
static const uint8_t LM_ENC_PALETTE[LM_ENC_PALETTE_SIZE][3] = {
    {255, 0, 0},   /* 0 red */
    {0, 255, 0},   /* 1 green */
    {0, 128, 255}, /* 2 blue */
    {255, 255, 0}, /* 3 yellow */
    {255, 0, 255}, /* 4 magenta */
    {0, 255, 255}, /* 5 cyan */
    {255, 128, 0}, /* 6 orange */
    {255, 255, 255} /* 7 white */
};

typedef struct lm_enc_ctx lm_enc_ctx;

/* The files of one call: frame i is data[offset[i] .. offset[i] + size[i]), in
 * page-locked host memory the context owns; valid until the context's next
 * encode call or its destruction. */
typedef struct {
  int32_t n;
  int32_t reserved;
  const uint8_t* data;
  const uint32_t* offset;
  const uint32_t* size;
} lm_enc_result;

typedef struct {
  int64_t bytes_out; /* compressed bytes of the last call (all frames) */
  double device_ms;  /* its kernels, first to last, from HIP events */
  int32_t frames;
  int32_t reserved;
} lm_enc_stats;

/* A filled square of side 2 * radius + 1 centred on column x, row y of the
 * canvas, clipped to it.  radius in 0..LM_ENC_MAX_RADIUS, colour below
 * LM_ENC_PALETTE_SIZE, |x| and |y| below 2^20. */
typedef struct {
  int32_t x, y, radius, colour;
} lm_enc_mark;

/* The geometry the detector sees a raw frame through (lm_setup's): */
typedef struct {
  const int32_t* cal;             /* calib_rows x calib_cols indices into a raw frame, copied */
  int32_t src_rows, src_cols;     /* raw frame size */
  int32_t calib_rows, calib_cols; /* the canvas: equal to the context's rows x cols */
  int32_t flip;
  int32_t reserved;
} lm_enc_overlay;

/* Worst case of one frame's file in bytes (above); -1 for sizes out of range. */
int64_t lm_enc_slot_bytes(int32_t rows, int32_t cols, int32_t format);

/* The same for a context with a restart interval of restart_interval MCUs
 * (0..65535; 0 gives lm_enc_slot_bytes); -1 for arguments out of range. */
int64_t lm_enc_slot_bytes_restart(int32_t rows, int32_t cols, int32_t format, int32_t restart_interval);

/* An encoder for frames of rows x cols (1..65535 each, at most
 * LM_ENC_MAX_BLOCKS blocks) in `format`, at `quality` (1..100), at most
 * max_batch (1..LM_ENC_MAX_BATCH) frames per call, on HIP device `device`.
 * max_batch * lm_enc_slot_bytes must stay below 2^31. */
lm_status lm_enc_create(int32_t device, int32_t rows, int32_t cols, int32_t format, int32_t quality, int32_t max_batch,
                        lm_enc_ctx** out);
/* The same with restart intervals, as libjpeg writes them (restart_interval in
 * MCUs, 0..65535): a DRI segment in front of SOS; after every restart_interval
 * MCUs but the frame's last, the 1-bit fill to a byte boundary (stuffed like any
 * other byte), the marker FF D0 + (j mod 8) for the j-th interval end, and DC
 * predictors that start again from 0.  The files are host/JpegEncode.hpp's
 * encode_jpeg with that restart_interval.  An interval of at least the frame's
 * MCU count writes the DRI segment and no marker.  0 is lm_enc_create: the
 * same files, buffers and kernels.  max_batch * lm_enc_slot_bytes_restart must
 * stay below 2^31. */
lm_status lm_enc_create_restart(int32_t device, int32_t rows, int32_t cols, int32_t format, int32_t quality,
                                int32_t max_batch, int32_t restart_interval, lm_enc_ctx** out);
void lm_enc_destroy(lm_enc_ctx* ctx);

/* Encodes n <= max_batch frames: frame i at base + i * pitch, tightly packed
 * rows, pitch >= the frame's bytes.  lm_enc_encode_device takes device memory
 * (read on the context's stream; the call returns when the files are in host
 * memory); lm_enc_encode takes host memory and uploads it first.  Only the
 * files and their sizes are copied back. */
lm_status lm_enc_encode_device(lm_enc_ctx* ctx, const uint8_t* d_frames, int64_t pitch, int32_t n, lm_enc_result* out);
lm_status lm_enc_encode(lm_enc_ctx* ctx, const uint8_t* h_frames, int64_t pitch, int32_t n, lm_enc_result* out);

/* Sets the overlay's geometry (an LM_ENC_RGB24 context whose rows x cols are
 * calib_rows x calib_cols).  Every cal entry must index a raw frame. */
lm_status lm_enc_set_overlay(lm_enc_ctx* ctx, const lm_enc_overlay* geometry);

/* Renders n raw frames (channel 0 of the video in device memory: frame i at
 * d_raw + i * pitch, src_rows x src_cols u8, as lm_detect_submit_device takes
 * them) and encodes the canvases without leaving the device:
 *   canvas[r][c] = raw[cal[r * calib_cols + (flip ? calib_cols - 1 - c : c)]]
 * as R = G = B, then frame i's marks, marks[mark_offset[i] .. mark_offset[i + 1])
 * (host memory; mark_offset has n + 1 non-decreasing entries from 0), in
 * order: a later mark overwrites an earlier one. */
lm_status lm_enc_render_encode_device(lm_enc_ctx* ctx, const uint8_t* d_raw, int64_t pitch, int32_t n,
                                      const lm_enc_mark* marks, const int32_t* mark_offset, lm_enc_result* out);
/* The same for raw frames in host memory, uploaded first (page-locked memory from lm_host_alloc is copied by DMA). */
lm_status lm_enc_render_encode(lm_enc_ctx* ctx, const uint8_t* h_raw, int64_t pitch, int32_t n, const lm_enc_mark* marks,
                               const int32_t* mark_offset, lm_enc_result* out);

/* Test access: the same canvases, not encoded, into h_rgb (n x rows x cols x 3 bytes, host). */
lm_status lm_enc_render_device(lm_enc_ctx* ctx, const uint8_t* d_raw, int64_t pitch, int32_t n, const lm_enc_mark* marks,
                               const int32_t* mark_offset, uint8_t* h_rgb);

void* lm_enc_stream(lm_enc_ctx* ctx); /* hipStream_t of the kernels */
lm_status lm_enc_last_stats(lm_enc_ctx* ctx, lm_enc_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* LOCOMOUSE_ENCODE_H */
