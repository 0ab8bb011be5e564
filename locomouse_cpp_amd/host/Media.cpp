// Media.cpp — see Media.hpp.
#include "Media.hpp"

#include "Jpeg.hpp"

#include <zlib.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include <unistd.h>

namespace locomouse {

namespace {

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
uint32_t le32(const uint8_t* p) { return (uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0]; }
uint16_t le16(const uint8_t* p) { return (uint16_t)(p[1] << 8 | p[0]); }

int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

}  // namespace

bool read_png_gray(const std::string& path, int& rows, int& cols, std::vector<uint8_t>& pixels) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  if (d.size() < 8 || std::memcmp(d.data(), sig, 8) != 0) return false;
  uint32_t w = 0, h = 0;
  int depth = 0, ctype = -1, interlace = 0;
  std::vector<uint8_t> z;
  for (size_t p = 8; p + 12 <= d.size();) {
    const uint32_t len = be32(&d[p]);
    if (p + 12 + (size_t)len > d.size()) return false;
    const char* type = (const char*)&d[p + 4];
    const uint8_t* body = &d[p + 8];
    if (!std::memcmp(type, "IHDR", 4) && len >= 13) {
      w = be32(body);
      h = be32(body + 4);
      depth = body[8];
      ctype = body[9];
      interlace = body[12];
    } else if (!std::memcmp(type, "IDAT", 4)) {
      z.insert(z.end(), body, body + len);
    } else if (!std::memcmp(type, "IEND", 4)) {
      break;
    }
    p += 12 + len;
  }
  int ch = ctype == 0 ? 1 : ctype == 4 ? 2 : ctype == 2 ? 3 : ctype == 6 ? 4 : 0;
  if (!w || !h || depth != 8 || !ch || interlace) return false;
  const size_t stride = (size_t)w * ch;
  std::vector<uint8_t> raw((stride + 1) * h);
  uLongf out_len = (uLongf)raw.size();
  if (uncompress(raw.data(), &out_len, z.data(), (uLong)z.size()) != Z_OK || out_len != raw.size()) return false;
  std::vector<uint8_t> img(stride * h), zero(stride, 0);
  for (uint32_t y = 0; y < h; ++y) {  // unfilter (PNG spec §9)
    const uint8_t ft = raw[y * (stride + 1)];
    const uint8_t* src = &raw[y * (stride + 1) + 1];
    uint8_t* cur = &img[y * stride];
    const uint8_t* up = y ? &img[(y - 1) * stride] : zero.data();
    for (size_t x = 0; x < stride; ++x) {
      const int a = x >= (size_t)ch ? cur[x - ch] : 0, b = up[x], c = x >= (size_t)ch ? up[x - ch] : 0;
      int v = src[x];
      switch (ft) {
        case 0: break;
        case 1: v += a; break;
        case 2: v += b; break;
        case 3: v += (a + b) >> 1; break;
        case 4: v += paeth(a, b, c); break;
        default: return false;
      }
      cur[x] = (uint8_t)v;
    }
  }
  rows = (int)h;
  cols = (int)w;
  pixels.resize((size_t)w * h);
  // png_set_rgb_to_gray_fixed(29900, 58700): 15-bit weights 9797, 19234, 3737
  const uint32_t rc = 9797, gc = 19234, bc = 32768 - 9797 - 19234;
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    const uint8_t* px = &img[i * ch];
    if (ch <= 2) {
      pixels[i] = px[0];  // alpha dropped
    } else {
      const uint32_t r = px[0], g = px[1], b = px[2];
      pixels[i] = (r == g && r == b) ? (uint8_t)r : (uint8_t)((rc * r + gc * g + bc * b) >> 15);
    }
  }
  return true;
}

bool write_png_gray(const std::string& path, int rows, int cols, const uint8_t* pixels) {
  if (rows <= 0 || cols <= 0 || !pixels) return false;
  const size_t stride = (size_t)cols;
  std::vector<uint8_t> raw((stride + 1) * (size_t)rows);
  for (int y = 0; y < rows; ++y) {  // filter type 0 (None) on every row
    raw[(size_t)y * (stride + 1)] = 0;
    std::memcpy(&raw[(size_t)y * (stride + 1) + 1], pixels + (size_t)y * stride, stride);
  }
  uLongf zlen = compressBound((uLong)raw.size());
  std::vector<uint8_t> z(zlen);
  if (compress2(z.data(), &zlen, raw.data(), (uLong)raw.size(), 6) != Z_OK) return false;
  std::vector<uint8_t> out = {137, 80, 78, 71, 13, 10, 26, 10};
  auto put32 = [&](uint32_t v) {
    for (int s = 24; s >= 0; s -= 8) out.push_back((uint8_t)(v >> s));
  };
  auto chunk = [&](const char* type, const uint8_t* body, size_t len) {
    put32((uint32_t)len);
    const size_t at = out.size();
    out.insert(out.end(), type, type + 4);
    out.insert(out.end(), body, body + len);
    put32((uint32_t)crc32(0L, &out[at], (uInt)(4 + len)));
  };
  uint8_t ihdr[13] = {0, 0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0};  // 8-bit grey, deflate, adaptive filtering, no interlace
  for (int k = 0; k < 4; ++k) {
    ihdr[k] = (uint8_t)((uint32_t)cols >> (24 - 8 * k));
    ihdr[4 + k] = (uint8_t)((uint32_t)rows >> (24 - 8 * k));
  }
  chunk("IHDR", ihdr, sizeof ihdr);
  chunk("IDAT", z.data(), (size_t)zlen);
  chunk("IEND", ihdr, 0);
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
  return std::fclose(f) == 0 && ok;
}

AviReader::~AviReader() {
  if (f_) std::fclose(f_);
}

bool AviReader::open(const std::string& path) {
  if (f_) std::fclose(f_);
  f_ = std::fopen(path.c_str(), "rb");
  if (!f_) return false;
  frames_.clear();
  next_ = 0;
  fps_ = 0;
  uint8_t hdr[12];
  if (std::fread(hdr, 1, 12, f_) != 12 || std::memcmp(hdr, "RIFF", 4) || std::memcmp(hdr + 8, "AVI ", 4)) return false;
  std::fseek(f_, 0, SEEK_END);
  const long file_end = std::ftell(f_);
  bool have_format = false;
  int video_stream = -1, stream_index = -1;
  uint32_t compression = 0;
  // Walk the chunk tree: hdrl/strl for the format, movi for the frames.
  struct Span {
    long pos, end;
    bool movi;
  };
  std::vector<Span> stack{{12, std::min<long>(file_end, 8 + (long)le32(hdr + 4)), false}};
  while (!stack.empty()) {
    Span& s = stack.back();
    if (s.pos + 8 > s.end) {
      stack.pop_back();
      continue;
    }
    uint8_t ck[12];
    std::fseek(f_, s.pos, SEEK_SET);
    if (std::fread(ck, 1, 8, f_) != 8) return false;
    const uint32_t size = le32(ck + 4);
    const long body = s.pos + 8, next = body + (long)size + (size & 1);
    const bool in_movi = s.movi;
    s.pos = next;
    if (!std::memcmp(ck, "LIST", 4)) {
      if (std::fread(ck + 8, 1, 4, f_) != 4) return false;
      stack.push_back({body + 4, std::min(next, file_end), in_movi || !std::memcmp(ck + 8, "movi", 4)});
      continue;
    }
    if (in_movi) {
      // ##db / ##dc of the video stream (stream number in the first two characters)
      if ((ck[2] == 'd' && (ck[3] == 'b' || ck[3] == 'c')) && ck[0] >= '0' && ck[0] <= '9' && ck[1] >= '0' &&
          ck[1] <= '9' && (ck[0] - '0') * 10 + (ck[1] - '0') == video_stream)
        frames_.emplace_back(body, size);
      continue;
    }
    std::vector<uint8_t> b(std::min<uint32_t>(size, 4096));
    if (!b.empty() && std::fread(b.data(), 1, b.size(), f_) != b.size()) return false;
    if (!std::memcmp(ck, "strh", 4) && b.size() >= 8) {
      ++stream_index;
      if (!std::memcmp(b.data(), "vids", 4) && video_stream < 0) {
        video_stream = stream_index;
        const uint64_t scale = b.size() >= 28 ? le32(&b[20]) : 0, rate = b.size() >= 28 ? le32(&b[24]) : 0;
        if (scale > 0) fps_ = (int)std::min<uint64_t>((rate + scale / 2) / scale, 1000000);  // dwRate / dwScale, rounded
      }
    } else if (!std::memcmp(ck, "strf", 4) && stream_index == video_stream && video_stream >= 0 && !have_format &&
               b.size() >= 40) {
      width_ = (int)le32(&b[4]);
      const int32_t hh = (int32_t)le32(&b[8]);
      bottom_up_ = hh > 0;
      height_ = hh > 0 ? hh : -hh;
      bits_ = le16(&b[14]);
      compression = le32(&b[16]);
      uint32_t n_pal = le32(&b[32]);
      if (bits_ == 8 && compression == 0) {
        if (!n_pal) n_pal = 256;
        palette_blue_.assign(256, 0);
        for (uint32_t k = 0; k < n_pal && 40 + 4 * k < b.size(); ++k) palette_blue_[k] = b[40 + 4 * k];
      }
      have_format = true;
    }
  }
  const bool grey = compression == 0x30303859u /* 'Y800' */ || compression == 0x59455247u /* 'GREY' */;
  mjpeg_ = compression == 0x47504A4Du /* 'MJPG' */ || compression == 0x67706A6Du /* 'mjpg' */ ||
           compression == 0x4745504Au /* 'JPEG' */ || compression == 0x6765706Au /* 'jpeg' */ ||
           compression == 0x31495641u /* 'AVI1' */;
  const bool ok = have_format && width_ > 0 && height_ > 0 &&
                  ((compression == 0 && (bits_ == 24 || bits_ == 8)) || (grey && bits_ == 8) || mjpeg_);
  if (!ok) {
    std::fclose(f_);
    f_ = nullptr;
    return false;
  }
  if (grey || mjpeg_) palette_blue_.clear(), bottom_up_ = false;
  return true;
}

bool AviReader::read(uint8_t* channel0) {
  if (!f_ || next_ >= frames_.size()) return false;
  return read_at(next_++, channel0);
}

bool AviReader::read_chunk(size_t index, std::vector<uint8_t>& bytes) const {
  if (!f_ || index >= frames_.size()) return false;
  const auto fr = frames_[index];
  bytes.resize(fr.second);
  for (size_t got = 0; got < fr.second;) {
    const ssize_t r = pread(fileno(f_), bytes.data() + got, fr.second - got, (off_t)(fr.first + (long)got));
    if (r <= 0) return false;
    got += (size_t)r;
  }
  return true;
}

bool AviReader::read_at(size_t index, uint8_t* channel0) const {
  if (!f_ || index >= frames_.size()) return false;
  const auto fr = frames_[index];
  if (mjpeg_) {  // one JPEG image per chunk, decoded to channel 0 of its BGR rendering (Jpeg.hpp)
    thread_local std::vector<uint8_t> jpg;
    jpg.resize(fr.second);
    for (size_t got = 0; got < fr.second;) {
      const ssize_t r = pread(fileno(f_), jpg.data() + got, fr.second - got, (off_t)(fr.first + (long)got));
      if (r <= 0) return false;
      got += (size_t)r;
    }
    return decode_jpeg_channel0_into(jpg.data(), jpg.size(), height_, width_, channel0);
  }
  const size_t bpp = (size_t)bits_ / 8, stride = ((size_t)width_ * bpp + 3) & ~(size_t)3;
  const size_t tight = (size_t)width_ * bpp;
  const bool padded = fr.second >= stride * (size_t)height_;
  const size_t row_bytes = padded ? stride : tight;
  if (fr.second < row_bytes * (size_t)height_) return false;
  const bool direct = bpp == 1 && palette_blue_.empty() && !bottom_up_ && row_bytes == (size_t)width_;
  thread_local std::vector<uint8_t> buf;
  uint8_t* data = channel0;
  if (!direct) {
    buf.resize(row_bytes * (size_t)height_);
    data = buf.data();
  }
  const size_t want = row_bytes * (size_t)height_;
  for (size_t got = 0; got < want;) {
    const ssize_t r = pread(fileno(f_), data + got, want - got, (off_t)(fr.first + (long)got));
    if (r <= 0) return false;
    got += (size_t)r;
  }
  if (direct) return true;
  bool identity = !palette_blue_.empty();
  for (int k = 0; identity && k < 256; ++k) identity = palette_blue_[k] == k;
  for (int y = 0; y < height_; ++y) {
    const uint8_t* src = data + (size_t)(bottom_up_ ? height_ - 1 - y : y) * row_bytes;
    uint8_t* dst = channel0 + (size_t)y * width_;
    if (bpp == 3) {
      for (int x = 0; x < width_; ++x) dst[x] = src[3 * x];  // B of BGR
    } else if (!palette_blue_.empty() && !identity) {
      const uint8_t* lut = palette_blue_.data();
      for (int x = 0; x < width_; ++x) dst[x] = lut[src[x]];
    } else {
      std::memcpy(dst, src, (size_t)width_);  // grey, or a palette whose blue is the index
    }
  }
  return true;
}

// ---- MjpegAviWriter
namespace {

void put32(std::vector<uint8_t>& b, uint32_t v) {
  for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
void put16(std::vector<uint8_t>& b, uint32_t v) {
  b.push_back((uint8_t)v);
  b.push_back((uint8_t)(v >> 8));
}
void put_tag(std::vector<uint8_t>& b, const char* t) { b.insert(b.end(), t, t + 4); }

constexpr uint32_t kAviHeaderBytes = 224;  // RIFF .. the 'movi' tag: the chunks start here

// RIFF / hdrl (avih, strl: strh + strf) / the head of the movi list.
std::vector<uint8_t> avi_header(int w, int h, int fps, uint32_t n, uint32_t largest, uint64_t movi_bytes, uint64_t idx_bytes) {
  std::vector<uint8_t> b;
  put_tag(b, "RIFF");
  put32(b, (uint32_t)(kAviHeaderBytes - 12 + movi_bytes + idx_bytes));
  put_tag(b, "AVI ");
  put_tag(b, "LIST");
  put32(b, 192);
  put_tag(b, "hdrl");
  put_tag(b, "avih");
  put32(b, 56);
  for (uint32_t v : {1000000u / (uint32_t)fps, 0u, 0u, 0x10u /* AVIF_HASINDEX */, n, 0u, 1u, largest, (uint32_t)w, (uint32_t)h,
                     0u, 0u, 0u, 0u})
    put32(b, v);
  put_tag(b, "LIST");
  put32(b, 116);
  put_tag(b, "strl");
  put_tag(b, "strh");
  put32(b, 56);
  put_tag(b, "vids");
  put_tag(b, "MJPG");
  put32(b, 0);  // flags
  put16(b, 0);  // priority
  put16(b, 0);  // language
  for (uint32_t v : {0u, 1u /* scale */, (uint32_t)fps /* rate */, 0u, n, largest, 0xFFFFFFFFu, 0u}) put32(b, v);
  for (uint32_t v : {0u, 0u, (uint32_t)w, (uint32_t)h}) put16(b, v);
  put_tag(b, "strf");
  put32(b, 40);
  put32(b, 40);
  put32(b, (uint32_t)w);
  put32(b, (uint32_t)h);
  put16(b, 1);
  put16(b, 24);
  put_tag(b, "MJPG");
  put32(b, (uint32_t)w * (uint32_t)h * 3u);
  for (int i = 0; i < 4; ++i) put32(b, 0);
  put_tag(b, "LIST");
  put32(b, (uint32_t)movi_bytes);
  put_tag(b, "movi");
  return b;
}

}  // namespace

MjpegAviWriter::~MjpegAviWriter() {
  if (f_) close();
}

bool MjpegAviWriter::open(const std::string& path, int rows, int cols, int fps) {
  if (f_) close();
  if (rows < 1 || cols < 1 || fps < 1) return false;
  f_ = std::fopen(path.c_str(), "wb");
  if (!f_) return false;
  width_ = cols;
  height_ = rows;
  fps_ = fps;
  ok_ = true;
  movi_bytes_ = 4;
  largest_ = 0;
  index_.clear();
  const std::vector<uint8_t> h = avi_header(width_, height_, fps_, 0, 0, movi_bytes_, 0);
  ok_ = h.size() == kAviHeaderBytes && std::fwrite(h.data(), 1, h.size(), f_) == h.size();
  return ok_;
}

bool MjpegAviWriter::fits(size_t size) const {
  // headers + movi + this chunk + the index with its entry
  const uint64_t padded = (uint64_t)size + (size & 1);
  return (uint64_t)kAviHeaderBytes + movi_bytes_ + 8 + padded + 8 + 16 * (uint64_t)(index_.size() + 1) <= 0xFFFFFFF0ull;
}

bool MjpegAviWriter::add(const uint8_t* jpeg, size_t size) {
  if (!f_ || !ok_ || !jpeg) return false;
  const uint64_t padded = (uint64_t)size + (size & 1);
  if (!fits(size)) return ok_ = false;
  uint8_t ck[8] = {'0', '0', 'd', 'c', (uint8_t)size, (uint8_t)(size >> 8), (uint8_t)(size >> 16), (uint8_t)(size >> 24)};
  ok_ = std::fwrite(ck, 1, 8, f_) == 8 && std::fwrite(jpeg, 1, size, f_) == size;
  if (ok_ && (size & 1)) ok_ = std::fputc(0, f_) != EOF;
  index_.emplace_back((uint32_t)movi_bytes_, (uint32_t)size);
  movi_bytes_ += 8 + padded;
  largest_ = std::max(largest_, (uint32_t)size);
  return ok_;
}

bool MjpegAviWriter::close() {
  if (!f_) return false;
  std::vector<uint8_t> idx;
  put_tag(idx, "idx1");
  put32(idx, (uint32_t)(16 * index_.size()));
  for (const auto& e : index_) {
    put_tag(idx, "00dc");
    put32(idx, 0x10);  // AVIIF_KEYFRAME
    put32(idx, e.first);
    put32(idx, e.second);
  }
  ok_ = ok_ && std::fwrite(idx.data(), 1, idx.size(), f_) == idx.size();
  const std::vector<uint8_t> h = avi_header(width_, height_, fps_, (uint32_t)index_.size(), largest_, movi_bytes_, idx.size());
  ok_ = ok_ && std::fseek(f_, 0, SEEK_SET) == 0 && std::fwrite(h.data(), 1, h.size(), f_) == h.size();
  ok_ = (std::fclose(f_) == 0) && ok_;
  f_ = nullptr;
  return ok_;
}

}  // namespace locomouse
