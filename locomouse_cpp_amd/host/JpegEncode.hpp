// JpegEncode.hpp — baseline sequential JPEG encoding (8-bit, Huffman, the
// Annex K tables, no optimised coding): one grey component, or RGB24 as YCbCr
// 4:2:0.  Not in the reference, which leaves looking at results to its MATLAB
// GUI; here it writes the annotated preview video (LM_PREVIEW)
// and states what the device encoder (include/locomouse_encode.h) must give.
//
// The arithmetic restates libjpeg's defaults (csrc/lm_jpeg_enc_core.h), and
// the file, SOI to EOI, equals Pillow's Image.save(f, "JPEG", quality=q) for
// mode L and Image.save(f, "JPEG", quality=q, subsampling=2) for mode RGB
// (tests/test_jpeg_encode.py).
#ifndef LOCOMOUSE_HOST_JPEG_ENCODE_HPP
#define LOCOMOUSE_HOST_JPEG_ENCODE_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

namespace locomouse {

enum class JpegInput { Gray8 = 0, Rgb24 = 1 };

// One image (rows x cols samples of 1 or 3 bytes, row-major, tightly packed) as
// a JPEG file appended to `out`.  rows and cols in 1..65535, quality in
// 1..100; throws std::invalid_argument otherwise.
//
// restart_interval (0..65535, in MCUs: 8 x 8 pixels for grey, 16 x 16 for
// colour) > 0 writes the stream as libjpeg does with that restart_interval
// (Pillow's restart_marker_blocks): a DRI segment in front of SOS, and after
// every restart_interval MCUs but the frame's last the 1-bit fill to a byte
// boundary (stuffed like any other byte), the marker FF D0 + (j mod 8) for the
// j-th interval end, and DC predictors that start again from 0.  An interval of
// at least the frame's MCU count writes the DRI segment and no marker.
void encode_jpeg(const uint8_t* pixels, int rows, int cols, JpegInput format, int quality, std::vector<uint8_t>& out,
                 int restart_interval = 0);

// Test access: the quantised coefficients of every block in scan order, 64
// int16 each in zig-zag order (what the device encoder's first kernel writes).
void encode_jpeg_coefficients(const uint8_t* pixels, int rows, int cols, JpegInput format, int quality,
                              std::vector<int16_t>& coef);

}  // namespace locomouse

#endif
