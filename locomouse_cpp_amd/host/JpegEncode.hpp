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
void encode_jpeg(const uint8_t* pixels, int rows, int cols, JpegInput format, int quality, std::vector<uint8_t>& out);

// Test access: the quantised coefficients of every block in scan order, 64
// int16 each in zig-zag order (what the device encoder's first kernel writes).
void encode_jpeg_coefficients(const uint8_t* pixels, int rows, int cols, JpegInput format, int quality,
                              std::vector<int16_t>& coef);

}  // namespace locomouse

#endif
