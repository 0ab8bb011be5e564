/* locomouse_jpeg.h — MJPEG frames decoded on the device, from their compressed
 * bytes to channel 0 of the BGR rendering in device memory (what
 * lm_detect_submit_device and lm_bb_push_device take).  Part of
 * liblocomouse_hip.so; statuses and lm_last_error are locomouse_hip.h's.
 *
 * The pixels are the host decoder's (locomouse_cpp_amd/host/Jpeg.cpp), byte
 * for byte, for every frame the device takes.  It takes: SOF0/SOF1, 8-bit
 * samples, 8-bit quantisation tables, one component or YCbCr at 4:4:4, 4:2:2
 * or 4:2:0 in one interleaved scan, any restart interval, with or without
 * DHT, of the context's frame size.  Everything else the host decoder accepts
 * — and any frame whose scan is damaged — comes back as LM_JPEG_NEEDS_HOST:
 * decode it with the host decoder and copy it into its slot.  What the host
 * decoder rejects is LM_JPEG_REJECTED, with the host's message. */
#ifndef LOCOMOUSE_JPEG_H
#define LOCOMOUSE_JPEG_H

#include <stddef.h>
#include <stdint.h>

#include "locomouse_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-frame status of lm_jpeg_decode_device. */
#define LM_JPEG_OK 0          /* the frame is in d_out */
#define LM_JPEG_NEEDS_HOST 1  /* out of the device's scope, or damaged: its slot in d_out is undefined */
#define LM_JPEG_REJECTED 2    /* not decodable at all (lm_jpeg_probe gives the reason) */

#define LM_JPEG_SUBSEQ_MIN 4       /* smallest subseq_bytes */
#define LM_JPEG_SUBSEQ_DEFAULT 64  /* what subseq_bytes = 0 selects */
#define LM_JPEG_CHUNK 128          /* subsequences one workgroup decodes at once */

typedef struct lm_jpeg_ctx lm_jpeg_ctx;

typedef struct lm_jpeg_info {
  int32_t rows, cols;
  int32_t components;        /* 1 or 3 */
  int32_t h_samp, v_samp;    /* first component's sampling factors */
  int32_t restart_interval;  /* MCUs, 0 = none */
  int32_t status;            /* LM_JPEG_OK = in the device's scope (for a context of rows x cols) */
  int32_t reserved;
  int64_t scan_bytes;        /* entropy-coded bytes of the first scan */
  char reason[128];          /* why the status is not LM_JPEG_OK */
} lm_jpeg_info;

typedef struct lm_jpeg_stats {  /* the last lm_jpeg_decode_device call */
  int64_t subsequences;         /* over all frames */
  int64_t sync_rounds;          /* over all frames and chunks */
  int32_t max_subsequences;     /* largest frame */
  int32_t max_chunk_rounds;     /* most rounds any chunk needed (<= LM_JPEG_CHUNK) */
  int32_t frames_needing_host;  /* LM_JPEG_NEEDS_HOST + LM_JPEG_REJECTED */
  int32_t table_sets;           /* distinct Huffman table sets uploaded */
  double device_ms;             /* upload, kernels and status read-back on the stream (HIP events) */
} lm_jpeg_stats;

/* A decoder for frames of rows x cols, at most max_batch per call.
 * subseq_bytes: bytes of scan per lane; 0 = LM_JPEG_SUBSEQ_DEFAULT, otherwise
 * >= LM_JPEG_SUBSEQ_MIN.  A frame whose scan exceeds 8 * rows * cols + 4096
 * bytes is LM_JPEG_NEEDS_HOST. */
lm_status lm_jpeg_create(int32_t device, int32_t rows, int32_t cols, int32_t max_batch, int32_t subseq_bytes,
                         lm_jpeg_ctx** out);
void lm_jpeg_destroy(lm_jpeg_ctx* ctx);

/* Decodes n <= max_batch JPEG images (host memory) into d_out (device memory):
 * frame i at d_out + i * pitch, rows x cols u8, row-major; pitch >= rows *
 * cols.  Returns after the context's stream is synchronised; status[i] tells
 * which frames d_out holds.  The call fails only for bad arguments or HIP
 * errors, never for bad frames. */
lm_status lm_jpeg_decode_device(lm_jpeg_ctx* ctx, const uint8_t* const* jpeg, const size_t* size, int32_t n,
                                uint8_t* d_out, int64_t pitch, int32_t* status);

/* Host only, no GPU call: what a frame is.  info->status is LM_JPEG_OK when a
 * context of the frame's own size would decode it on the device. */
lm_status lm_jpeg_probe(const uint8_t* data, size_t size, lm_jpeg_info* info);

/* Frame buffers for callers that do not use HIP themselves (the host mirror):
 * device memory on the context's device, released by lm_jpeg_device_free or
 * with the context; and a host -> device copy on the context's stream, waited
 * for (a frame decoded on the host goes into its slot with it). */
lm_status lm_jpeg_device_alloc(lm_jpeg_ctx* ctx, size_t bytes, uint8_t** d_out);
lm_status lm_jpeg_device_free(lm_jpeg_ctx* ctx, uint8_t* d);
lm_status lm_jpeg_upload(lm_jpeg_ctx* ctx, uint8_t* d_dst, const uint8_t* src, size_t bytes);

void* lm_jpeg_stream(lm_jpeg_ctx* ctx); /* hipStream_t of the decode kernels */
lm_status lm_jpeg_debug_stats(lm_jpeg_ctx* ctx, lm_jpeg_stats* out);

/* The interval path.  A frame with a DRI segment and more than one restart
 * interval is decoded one lane per interval: behind a restart marker the
 * decoder's state is known and DC prediction starts again, so no lane guesses
 * and none waits for another.  A frame whose markers are not exactly those its
 * header asks for, or one of whose intervals does not decode cleanly into
 * exactly its blocks, is handed to the subsequence path on the device, within
 * the same call; statuses and pixels are the subsequence path's, always.
 * lm_jpeg_set_interval_path switches the path (the default is on; the
 * environment variable LM_JPEG_RST=0, read when the context is created, makes
 * the default off): the A/B switch on one build. */
lm_status lm_jpeg_set_interval_path(lm_jpeg_ctx* ctx, int32_t on);

typedef struct lm_jpeg_interval_stats { /* the last lm_jpeg_decode_device call */
  int32_t frames_interval;        /* frames the interval path decoded */
  int32_t frames_handed_over;     /* restart frames it handed to the subsequence path (marker count, irregular lane) */
  int64_t intervals;              /* lanes it ran, over all frames */
  int32_t longest_interval_bytes; /* over those lanes */
  int32_t reserved;
  double parse_ms;                /* host: header parse of the batch, the marker index included */
} lm_jpeg_interval_stats;
lm_status lm_jpeg_debug_interval_stats(lm_jpeg_ctx* ctx, lm_jpeg_interval_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* LOCOMOUSE_JPEG_H */
