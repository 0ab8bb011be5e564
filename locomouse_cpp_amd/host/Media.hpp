// Media.hpp — the image and video readers behind the reference's CLI
// (SURVEY.md §8(f) row 2), native because OpenCV is absent:
//
//   read_png_gray  cv::imread(BKG_FILE, CV_LOAD_IMAGE_GRAYSCALE)  (LocoMouse_class.cpp:405-419)
//   write_png_gray the estimated background (Background.hpp) as a file read_png_gray reads; not in the reference
//   AviReader      cv::VideoCapture(VIDEO_FILE); V >> F; extractChannel(F, F, 0)
//                  (:376-403, :1273-1293) for uncompressed AVI (BI_RGB 24-bit
//                  BGR or 8-bit palettised, and 8-bit 'Y800'/'GREY') and MJPEG
//                  AVI ('MJPG'/'JPEG'/'AVI1': sequential Huffman JPEG per
//                  frame, Jpeg.hpp); channel 0 of the decoded BGR frame is
//                  blue.  Other codecs (H.264 …) are not decoded: opening
//                  such a file fails like a VideoCapture that cannot open it.
//   MjpegAviWriter the annotated preview video (LM_PREVIEW): an
//                  MJPG AVI that AviReader and ordinary players open; not in
//                  the reference
#ifndef LOCOMOUSE_HOST_MEDIA_HPP
#define LOCOMOUSE_HOST_MEDIA_HPP

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace locomouse {

// 8-bit PNG (grey, grey+alpha, RGB, RGBA; no interlace, no palette) as one
// grey channel.  Colour is reduced with libpng's png_set_rgb_to_gray(1,
// 0.299, 0.587) fixed-point weights (what OpenCV's PNG decoder requests for
// IMREAD_GRAYSCALE; exact byte parity with a given libpng build is unpinned).
// Returns false when the file cannot be read or decoded (!BKG.data).
bool read_png_gray(const std::string& path, int& rows, int& cols, std::vector<uint8_t>& pixels);

// rows x cols grey pixels as an 8-bit greyscale PNG: no interlace, filter type
// 0 on every row, one zlib stream, so read_png_gray and any other PNG reader
// return the same bytes.  Returns false when the file cannot be written.
bool write_png_gray(const std::string& path, int rows, int cols, const uint8_t* pixels);

class AviReader {
 public:
  AviReader() = default;
  ~AviReader();
  AviReader(const AviReader&) = delete;
  AviReader& operator=(const AviReader&) = delete;

  bool open(const std::string& path);  // V.isOpened()
  int rows() const { return height_; }
  int cols() const { return width_; }
  uint32_t frame_count() const { return (uint32_t)frames_.size(); }  // CAP_PROP_FRAME_COUNT
  bool read(uint8_t* channel0);        // V >> F + extractChannel(F, F, 0); false at the end
  void rewind() { next_ = 0; }         // V.set(CV_CAP_PROP_POS_FRAMES, 0)
  // Frame `index` (0-based) without moving the read position; safe to call
  // from several threads at once (pread on the file descriptor).
  bool read_at(size_t index, uint8_t* channel0) const;
  // MJPEG ('MJPG'/'JPEG'/'AVI1'): every frame chunk is one JPEG image.
  bool is_mjpeg() const { return mjpeg_; }
  // Frames per second of the video stream (dwRate / dwScale of its 'strh', rounded), 0 when the file does not say.
  int fps() const { return fps_; }
  // The raw bytes of frame `index`'s chunk (a JPEG image when is_mjpeg()),
  // without moving the read position; thread-safe like read_at.
  bool read_chunk(size_t index, std::vector<uint8_t>& bytes) const;

 private:
  std::FILE* f_ = nullptr;
  int width_ = 0, height_ = 0, bits_ = 0;
  bool bottom_up_ = true;
  bool mjpeg_ = false;
  int fps_ = 0;
  std::vector<uint8_t> palette_blue_;  // 8-bit palettised: blue of each entry
  std::vector<std::pair<long, uint32_t>> frames_;  // (file offset, size) of each frame chunk
  size_t next_ = 0;
};

// MJPEG AVI: one JPEG image per '00dc' chunk of the 'movi' list, an 'idx1'
// index behind it, and the 'avih' / 'strh' / 'strf' fields AviReader reads back
// (compression 'MJPG', 24 bits, cols x rows).  Frames are appended as they
// come; close() writes the index and the counts into the headers.
class MjpegAviWriter {
 public:
  MjpegAviWriter() = default;
  ~MjpegAviWriter();
  MjpegAviWriter(const MjpegAviWriter&) = delete;
  MjpegAviWriter& operator=(const MjpegAviWriter&) = delete;

  bool open(const std::string& path, int rows, int cols, int fps);  // fps >= 1
  bool add(const uint8_t* jpeg, size_t size);  // false: not open, write error, or the file would pass 4 GiB
  // Whether a frame of `size` bytes still fits: RIFF sizes are 32 bits, so headers, frames and index stay below 4 GiB.
  bool fits(size_t size) const;
  bool close();                                // false when anything could not be written
  uint32_t frame_count() const { return (uint32_t)index_.size(); }

 private:
  std::FILE* f_ = nullptr;
  int width_ = 0, height_ = 0, fps_ = 30;
  bool ok_ = true;
  uint64_t movi_bytes_ = 4;  // 'movi' + the chunks
  uint32_t largest_ = 0;
  std::vector<std::pair<uint32_t, uint32_t>> index_;  // (offset from 'movi', size) of each chunk
};

}  // namespace locomouse

#endif
