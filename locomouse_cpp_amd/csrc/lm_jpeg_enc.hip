// lm_jpeg_enc.hip — baseline JPEG encoding and the track overlay
// (include/locomouse_encode.h).  The arithmetic is lm_jpeg_enc_core.h's, which
// the host encoder runs too.  One batch of n frames goes through:
//
//   k_enc_canvas    (overlay only) canvas = raw through the calibration map, R = G = B
//   k_enc_marks     (overlay only) one workgroup per frame fills its marks in order
//   k_enc_coef      8 lanes per block: colour conversion, downsampling and edge
//                   rules in the sample fetch, the row pass, a transpose through
//                   LDS, the column pass, quantisation; int16 coefficients in
//                   zig-zag order, blocks in scan order
//   k_enc_scan      one workgroup per frame: each block's code length and the
//                   exclusive prefix sum of the lengths (the bit offsets)
//   k_enc_pack      one thread per block writes its codes at its bit offset into the
//                   frame's zeroed, unstuffed stream (vector atomicOr on the two
//                   words it shares with its neighbours, plain stores between)
//   k_enc_count     one workgroup per frame counts the FF bytes: the file's size
//   k_enc_offsets   the files' offsets in the batch's output (a sum over n)
//   k_enc_write     one workgroup per frame: header, the stuffed stream (a prefix
//                   sum of FF counts places every byte), the 1-bit fill, EOI
//
// A context with restart intervals (lm_enc_create_restart) launches the <true>
// instantiations of k_enc_scan, k_enc_pack and k_enc_write: the bit
// offsets are rounded up to a byte at every interval end and the DC prediction
// starts again behind it, the pack writes the 1-bit fill, and the write puts
// the unstuffed marker in front of the interval's first byte: byte k of the
// unstuffed stream lands at k, plus the FF bytes in front of it, plus twice the
// intervals that ended in front of it.
//
// Safety.  Per frame the coefficient buffer has nblk * 64 entries, the offsets
// nblk, the unstuffed stream W = 52 * nblk + 1 words, and the batch's output
// max_batch * slot bytes (locomouse_encode.h derives both).  The size
// categories are clamped (lje_cat_dc / lje_cat_ac), so a block's codes are at
// most 1660 bits whatever the coefficient buffer holds: the bit offsets stay
// below 52 * 32 * nblk, every word index below W, and a file's size is at most
// the slot.  With restart intervals W and the slot grow by the fills and the
// markers (locomouse_encode.h derives that too), the marker index reads the
// offsets of blocks (m + 1) * bpi for m below the marker count only, and those
// are below nblk.  Files are packed at the running sum of their sizes, which the sum
// of the slots bounds.  Frames are read at i * pitch + [0, frame bytes) for
// i < n only; pitch, n, and every mark and calibration index are checked on the
// host before anything is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "locomouse_encode.h"
#include "lm_jpeg_enc_core.h"
#include "lm_host.h"

static_assert(LM_ENC_GRAY8 == LJE_GRAY8 && LM_ENC_RGB24 == LJE_RGB24, "the header's formats are the core's");
static_assert(LM_ENC_BLOCK_WORDS == LJE_BLOCK_WORDS && LM_ENC_MAX_HEADER == LJE_MAX_HEADER, "the header's sizes are the core's");
static_assert(((int64_t)LM_ENC_MAX_BLOCKS * LJE_BLOCK_WORDS + LM_ENC_MAX_BLOCKS / 4 + 1) * 32 < ((int64_t)1 << 31),
              "bit offsets fit 31 bits, with a fill byte for every block");

namespace {

constexpr int kThreads = 256;
constexpr int kBlocksPerGroup = kThreads / 8;  // k_enc_coef: 8 lanes per block
constexpr int kWriteBytes = 16;                // k_enc_write: bytes per thread and round

__global__ __launch_bounds__(kThreads) void k_enc_canvas(const uint8_t* __restrict__ raw, int64_t pitch,
                                                         const int32_t* __restrict__ cal, int rows, int cols, int flip,
                                                         uint8_t* __restrict__ canvas) {
  const uint32_t npix = (uint32_t)rows * (uint32_t)cols;
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= npix) return;
  const uint32_t r = p / (uint32_t)cols, c = p % (uint32_t)cols;
  const uint8_t v = raw[(int64_t)blockIdx.y * pitch + cal[r * (uint32_t)cols + (flip ? (uint32_t)cols - 1 - c : c)]];
  uint8_t* o = canvas + ((size_t)blockIdx.y * npix + p) * 3;
  o[0] = v;
  o[1] = v;
  o[2] = v;
}

__global__ __launch_bounds__(kThreads) void k_enc_marks(const lm_enc_mark* __restrict__ marks,
                                                        const int32_t* __restrict__ mark_offset, int rows, int cols,
                                                        uint8_t* __restrict__ canvas, const uint8_t* __restrict__ palette) {
  uint8_t* img = canvas + (size_t)blockIdx.x * (size_t)rows * (size_t)cols * 3;
  const int m0 = mark_offset[blockIdx.x], m1 = mark_offset[blockIdx.x + 1];
  for (int m = m0; m < m1; ++m) {
    const lm_enc_mark k = marks[m];
    const int side = 2 * k.radius + 1;
    const uint8_t cr = palette[3 * k.colour], cg = palette[3 * k.colour + 1], cb = palette[3 * k.colour + 2];
    for (int i = threadIdx.x; i < side * side; i += kThreads) {
      const int y = k.y - k.radius + i / side, x = k.x - k.radius + i % side;
      if (y < 0 || y >= rows || x < 0 || x >= cols) continue;
      uint8_t* o = img + ((size_t)y * (size_t)cols + (size_t)x) * 3;
      o[0] = cr;
      o[1] = cg;
      o[2] = cb;
    }
    __syncthreads();  // the next mark overwrites this one where they overlap
  }
}

__global__ __launch_bounds__(kThreads) void k_enc_coef(const uint8_t* __restrict__ frames, int64_t pitch, LjeGeom g,
                                                       const LjeTables* __restrict__ T, int16_t* __restrict__ coef) {
  __shared__ int32_t tile[kBlocksPerGroup][8][9];
  const int bl = threadIdx.x >> 3, lane = threadIdx.x & 7;
  const uint32_t b = blockIdx.x * kBlocksPerGroup + bl;
  const bool active = b < g.nblk;
  const uint8_t* f = frames + (int64_t)blockIdx.y * pitch;
  LjeBlock k = {0, 0, 0, 0};
  int32_t d[8];
  if (active) {
    k = lje_block(g, b);
#pragma unroll
    for (int c = 0; c < 8; ++c) d[c] = lje_sample(f, g, k.comp, 8 * k.br + lane, 8 * k.bc + c);
    lje_fdct8<1>(d);
#pragma unroll
    for (int c = 0; c < 8; ++c) tile[bl][lane][c] = d[c];
  }
  __syncthreads();
  if (!active) return;
#pragma unroll
  for (int r = 0; r < 8; ++r) d[r] = tile[bl][r][lane];
  lje_fdct8<2>(d);
  int16_t* out = coef + ((size_t)blockIdx.y * g.nblk + b) * 64;
  const int t = k.comp ? 1 : 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int i = 8 * r + lane;
    const int32_t q = lje_quant(d[r], T->div[t][i]);
    out[T->pos[i]] = (int16_t)((k.dummy && i) ? 0 : q);
  }
}

// jchuff.c encode_one_block over block c (64 zig-zag int16, 16-byte aligned)
// with the DC predictor `pred`: emit(code, length) for every code and value
// field, length <= 16.  e: the component's 272 table entries.
template <class Emit>
__device__ inline void walk_block(const int16_t* __restrict__ c, int32_t pred, const uint32_t* e, Emit&& emit) {
  int run = 0;
  auto ac = [&](int32_t v) {
    if (!v) {
      ++run;
      return;
    }
    for (; run > 15; run -= 16) emit(e[16 + 0xF0] >> 5, e[16 + 0xF0] & 31u);
    const int nb = lje_cat_ac(32 - __clz(v < 0 ? -v : v));
    const uint32_t s = e[16 + ((run << 4 | nb) & 255)];
    emit(s >> 5, s & 31u);
    emit((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u), (uint32_t)nb);
    run = 0;
  };
  const uint4* v4 = reinterpret_cast<const uint4*>(c);
#pragma unroll 1
  for (int j = 0; j < 8; ++j) {
    const uint4 w = v4[j];
    const int32_t c0 = (int16_t)(w.x & 0xFFFFu), c1 = (int16_t)(w.x >> 16), c2 = (int16_t)(w.y & 0xFFFFu),
                  c3 = (int16_t)(w.y >> 16), c4 = (int16_t)(w.z & 0xFFFFu), c5 = (int16_t)(w.z >> 16),
                  c6 = (int16_t)(w.w & 0xFFFFu), c7 = (int16_t)(w.w >> 16);
    if (j == 0) {
      const int32_t diff = c0 - pred;
      const int nb = lje_cat_dc(32 - __clz(diff < 0 ? -diff : diff));
      emit(e[nb] >> 5, e[nb] & 31u);
      if (nb) emit((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u), (uint32_t)nb);
    } else {
      ac(c0);
    }
    ac(c1);
    ac(c2);
    ac(c3);
    ac(c4);
    ac(c5);
    ac(c6);
    ac(c7);
  }
  if (run) emit(e[16] >> 5, e[16] & 31u);
}

__device__ inline int32_t dc_pred(const int16_t* __restrict__ fcoef, const LjeGeom& g, uint32_t b) {
  const int64_t p = lje_dc_pred_block(g, b);
  return p < 0 ? 0 : (int32_t)fcoef[(size_t)p * 64];
}

// Restart intervals (RST).  The kernels that know about them are second
// instantiations of k_enc_scan, k_enc_pack and k_enc_write, so a context
// without restarts launches the code it always did (RstArgs<false> is empty).
// Block b ends an interval when the next one begins with a marker.
template <bool RST>
struct RstArgs;
template <>
struct RstArgs<false> {
  static constexpr uint32_t bpi = 0, nmark = 0, nblk = 0;
  static constexpr const uint32_t* bit_off = nullptr;
};
template <>
struct RstArgs<true> {
  const uint32_t* bit_off;  // every frame's bit offsets (k_enc_write's marker index)
  uint32_t nblk;
  uint32_t bpi;    // blocks of an interval: restart_interval * bpm > 0
  uint32_t nmark;  // markers of a frame: its intervals - 1
};
template <bool RST>
__device__ inline int32_t dc_pred_of(const int16_t* __restrict__ fcoef, const LjeGeom& g, uint32_t b, uint32_t bpi) {
  if (!RST) return dc_pred(fcoef, g, b);
  const int64_t p = lje_dc_pred_block_rst(g, b, bpi / (uint32_t)g.bpm);
  return p < 0 ? 0 : (int32_t)fcoef[(size_t)p * 64];
}
__device__ inline bool ends_interval(const LjeGeom& g, uint32_t b, uint32_t bpi) {
  return (b + 1u) % bpi == 0u && b + 1u < g.nblk;
}

__device__ inline void load_ehuf(const LjeTables* __restrict__ T, uint32_t* s_e) {
  for (int i = threadIdx.x; i < 2 * LJE_EHUF_STRIDE; i += kThreads) s_e[i] = T->ehuf[i];
  __syncthreads();
}

// A run of blocks as the bit offsets see it with restart intervals: from the
// position s in front of it, the position behind it is s + head when no block
// of the run ends an interval, and roundup8(s + head) + rest when one does
// (head: the bits up to the first interval end, which is rounded up to a whole
// byte; everything behind it starts at a byte boundary, so rest does not depend
// on s).  Runs combine associatively, which is all the scan needs.
struct RstRun {
  uint32_t head, rest, ends;
};
__device__ inline uint32_t roundup8(uint32_t v) { return (v + 7u) & ~7u; }
__device__ inline RstRun rst_join(const RstRun& a, const RstRun& b) {
  if (!a.ends) return {a.head + b.head, b.rest, b.ends};
  return {a.head, b.ends ? roundup8(a.rest + b.head) + b.rest : a.rest + b.head, 1u};
}
__device__ inline uint32_t rst_behind(const RstRun& r, uint32_t s) {
  return r.ends ? roundup8(s + r.head) + r.rest : s + r.head;
}

template <bool RST>
__global__ __launch_bounds__(kThreads) void k_enc_scan(const int16_t* __restrict__ coef, LjeGeom g,
                                                       const LjeTables* __restrict__ T, uint32_t* __restrict__ bit_off,
                                                       uint32_t* __restrict__ bits, RstArgs<RST> rst) {
  const uint32_t bpi = rst.bpi;
  __shared__ uint32_t s_e[2 * LJE_EHUF_STRIDE];
  __shared__ uint32_t s_scan[2][kThreads];
  __shared__ uint32_t s_rest[RST ? 2 : 1][RST ? kThreads : 1], s_ends[RST ? 2 : 1][RST ? kThreads : 1];
  load_ehuf(T, s_e);
  const int16_t* fcoef = coef + (size_t)blockIdx.x * g.nblk * 64;
  uint32_t* foff = bit_off + (size_t)blockIdx.x * g.nblk;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < g.nblk; base += kThreads) {
    const uint32_t b = base + threadIdx.x;
    uint32_t len = 0;
    if (b < g.nblk) {
      const uint32_t* e = s_e + ((g.bpm == 6 && b % 6u >= 4u) ? LJE_EHUF_STRIDE : 0);
      walk_block(fcoef + (size_t)b * 64, dc_pred_of<RST>(fcoef, g, b, bpi), e, [&](uint32_t, uint32_t l) { len += l; });
    }
    int cur = 0;
    s_scan[0][threadIdx.x] = len;
    if (RST) {
      s_rest[0][threadIdx.x] = 0;
      s_ends[0][threadIdx.x] = (b < g.nblk && ends_interval(g, b, bpi)) ? 1u : 0u;
    }
    __syncthreads();
    for (int step = 1; step < kThreads; step <<= 1) {  // inclusive scan of the 256 lengths (RST: runs)
      if (RST) {
        RstRun v = {s_scan[cur][threadIdx.x], s_rest[cur][threadIdx.x], s_ends[cur][threadIdx.x]};
        if ((int)threadIdx.x >= step) {
          const int t = threadIdx.x - step;
          v = rst_join(RstRun{s_scan[cur][t], s_rest[cur][t], s_ends[cur][t]}, v);
        }
        s_scan[cur ^ 1][threadIdx.x] = v.head;
        s_rest[cur ^ 1][threadIdx.x] = v.rest;
        s_ends[cur ^ 1][threadIdx.x] = v.ends;
      } else {
        uint32_t v = s_scan[cur][threadIdx.x];
        if ((int)threadIdx.x >= step) v += s_scan[cur][threadIdx.x - step];
        s_scan[cur ^ 1][threadIdx.x] = v;
      }
      cur ^= 1;
      __syncthreads();
    }
    if (RST) {
      // a block begins where the run of the blocks in front of it in this round ends
      if (b < g.nblk) {
        const int t = (int)threadIdx.x - 1;
        foff[b] = t < 0 ? carry : rst_behind(RstRun{s_scan[cur][t], s_rest[cur][t], s_ends[cur][t]}, carry);
      }
      carry = rst_behind(RstRun{s_scan[cur][kThreads - 1], s_rest[cur][kThreads - 1], s_ends[cur][kThreads - 1]}, carry);
    } else {
      if (b < g.nblk) foff[b] = carry + s_scan[cur][threadIdx.x] - len;
      carry += s_scan[cur][kThreads - 1];
    }
    __syncthreads();  // s_scan is rewritten by the next round
  }
  if (threadIdx.x == 0) bits[blockIdx.x] = carry;
}

template <bool RST>
__global__ __launch_bounds__(kThreads) void k_enc_pack(const int16_t* __restrict__ coef, LjeGeom g,
                                                       const LjeTables* __restrict__ T,
                                                       const uint32_t* __restrict__ bit_off, uint32_t* __restrict__ words,
                                                       uint32_t wpf, RstArgs<RST> rst) {
  const uint32_t bpi = rst.bpi;
  __shared__ uint32_t s_e[2 * LJE_EHUF_STRIDE];
  load_ehuf(T, s_e);
  const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= g.nblk) return;
  const int16_t* fcoef = coef + (size_t)blockIdx.y * g.nblk * 64;
  uint32_t* fw = words + (size_t)blockIdx.y * wpf;
  const uint32_t off = bit_off[(size_t)blockIdx.y * g.nblk + b];
  uint32_t widx = off >> 5;
  uint32_t nacc = off & 31u;  // bits of the current word in front of this block's (other blocks')
  uint64_t acc = 0;           // the block's bits, left-aligned behind them
  // Only the block's first word (the block in front ends in it) and its last, partial one (the next block begins
  // in it) hold other blocks' bits: those are ORed in atomically, the words between are this block's alone.
  bool shared = true;
  const uint32_t* e = s_e + ((g.bpm == 6 && b % 6u >= 4u) ? LJE_EHUF_STRIDE : 0);
  auto put = [&](uint32_t code, uint32_t l) {
    if (!l) return;
    acc |= (uint64_t)code << (64u - nacc - l);  // nacc <= 31 and l <= 16
    nacc += l;
    if (nacc >= 32u) {
      if (widx < wpf) {
        if (shared)
          atomicOr(fw + widx, (uint32_t)(acc >> 32));
        else
          fw[widx] = (uint32_t)(acc >> 32);
      }
      shared = false;
      ++widx;
      acc <<= 32;
      nacc -= 32u;
    }
  };
  walk_block(fcoef + (size_t)b * 64, dc_pred_of<RST>(fcoef, g, b, bpi), e, put);
  if (RST && ends_interval(g, b, bpi)) {  // the interval's 1-bit fill: words begin at byte boundaries
    const uint32_t pad = (8u - (nacc & 7u)) & 7u;
    put((1u << pad) - 1u, pad);
  }
  if (nacc && widx < wpf) atomicOr(fw + widx, (uint32_t)(acc >> 32));
}


// Byte k of a frame's unstuffed stream of `bits` bits (k below its byte count),
// the last one filled up with 1-bits.
__device__ inline uint32_t stream_byte(uint32_t word, uint32_t k, uint32_t bits) {
  uint32_t v = (word >> (24u - 8u * (k & 3u))) & 255u;
  if (k == ((bits + 7u) >> 3) - 1u && (bits & 7u)) v |= (1u << (8u - (bits & 7u))) - 1u;
  return v;
}

__global__ __launch_bounds__(kThreads) void k_enc_count(const uint32_t* __restrict__ words, uint32_t wpf,
                                                        const uint32_t* __restrict__ bits, uint32_t hdr_len,
                                                        uint32_t* __restrict__ size) {
  __shared__ uint32_t s_sum[kThreads];
  const uint32_t* fw = words + (size_t)blockIdx.x * wpf;
  const uint32_t nbits = bits[blockIdx.x], nbytes = (nbits + 7u) >> 3;
  uint32_t ff = 0;
  for (uint32_t w = threadIdx.x; w < wpf && 4u * w < nbytes; w += kThreads) {
    const uint32_t v = fw[w];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
      if (4u * w + j < nbytes && stream_byte(v, 4u * w + j, nbits) == 255u) ++ff;
  }
  s_sum[threadIdx.x] = ff;
  __syncthreads();
  for (int step = kThreads / 2; step > 0; step >>= 1) {
    if ((int)threadIdx.x < step) s_sum[threadIdx.x] += s_sum[threadIdx.x + step];
    __syncthreads();
  }
  if (threadIdx.x == 0) size[blockIdx.x] = hdr_len + nbytes + s_sum[0] + 2u;
}

__global__ void k_enc_offsets(const uint32_t* __restrict__ size, int n, uint32_t* __restrict__ offset) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t sum = 0;
  for (int i = 0; i < n; ++i) {
    offset[i] = sum;
    sum += size[i];
  }
}

// RST: nmark markers, marker m (from 0) in front of the byte at which block (m + 1) * bpi begins (its bit offset,
// a whole number of bytes).  Every block has at least 4 bits, so these bytes differ and all lie below nbytes.
// foff: the frame's bit offsets.
template <bool RST>
__global__ __launch_bounds__(kThreads) void k_enc_write(const uint32_t* __restrict__ words, uint32_t wpf,
                                                        const uint32_t* __restrict__ bits,
                                                        const uint8_t* __restrict__ hdr, uint32_t hdr_len,
                                                        const uint32_t* __restrict__ offset, uint8_t* __restrict__ out,
                                                        RstArgs<RST> rst) {
  const uint32_t* foff = RST ? rst.bit_off + (size_t)blockIdx.x * rst.nblk : nullptr;
  const uint32_t bpi = rst.bpi, nmark = rst.nmark;
  __shared__ uint32_t s_scan[2][kThreads];
  const uint32_t* fw = words + (size_t)blockIdx.x * wpf;
  const uint32_t nbits = bits[blockIdx.x], nbytes = (nbits + 7u) >> 3;
  uint8_t* o = out + offset[blockIdx.x];
  for (uint32_t i = threadIdx.x; i < hdr_len; i += kThreads) o[i] = hdr[i];
  o += hdr_len;
  uint32_t carry = 0;  // FF bytes (RST: and marker bytes) in front of this round
  for (uint32_t base = 0; base < nbytes; base += kThreads * kWriteBytes) {
    const uint32_t k0 = base + threadIdx.x * kWriteBytes;
    uint32_t w[kWriteBytes / 4];
    uint32_t ff = 0;
#pragma unroll
    for (uint32_t j = 0; j < kWriteBytes / 4; ++j) {
      const uint32_t wi = (k0 >> 2) + j;
      w[j] = (wi < wpf && 4u * wi < nbytes) ? fw[wi] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < kWriteBytes; ++j)
      if (k0 + j < nbytes && stream_byte(w[j >> 2], k0 + j, nbits) == 255u) ++ff;
    uint32_t mark = 0;  // RST: the markers in front of byte k0
    if (RST && k0 < nbytes) {
      uint32_t lo = 0, hi = nmark;  // the first marker whose byte is not below k0
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((foff[(size_t)(mid + 1u) * bpi] >> 3) < k0)
          lo = mid + 1u;
        else
          hi = mid;
      }
      mark = lo;
      const uint32_t kend = k0 + kWriteBytes < nbytes ? k0 + kWriteBytes : nbytes;
      for (uint32_t m = mark; m < nmark && (foff[(size_t)(m + 1u) * bpi] >> 3) < kend; ++m) ff += 2u;  // at most 16
    }
    int cur = 0;
    s_scan[0][threadIdx.x] = ff;
    __syncthreads();
    for (int step = 1; step < kThreads; step <<= 1) {
      uint32_t v = s_scan[cur][threadIdx.x];
      if ((int)threadIdx.x >= step) v += s_scan[cur][threadIdx.x - step];
      s_scan[cur ^ 1][threadIdx.x] = v;
      cur ^= 1;
      __syncthreads();
    }
    uint32_t pos = k0 + carry + s_scan[cur][threadIdx.x] - ff;
    uint32_t next = (RST && k0 < nbytes && mark < nmark) ? foff[(size_t)(mark + 1u) * bpi] >> 3 : 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t j = 0; j < kWriteBytes; ++j) {
      if (k0 + j < nbytes) {
        if (RST && k0 + j == next) {
          o[pos++] = 0xFF;
          o[pos++] = (uint8_t)(0xD0u + (mark & 7u));
          ++mark;
          next = mark < nmark ? foff[(size_t)(mark + 1u) * bpi] >> 3 : 0xFFFFFFFFu;
        }
        const uint32_t v = stream_byte(w[j >> 2], k0 + j, nbits);
        o[pos++] = (uint8_t)v;
        if (v == 255u) o[pos++] = 0;
      }
    }
    carry += s_scan[cur][kThreads - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    o[nbytes + carry] = 0xFF;
    o[nbytes + carry + 1] = 0xD9;
  }
}

}  // namespace

struct lm_enc_ctx {
  int device = 0;
  int max_batch = 0, quality = 0;
  LjeGeom g{};
  size_t frame_bytes = 0;  // of one input frame
  uint32_t wpf = 0;        // words of one frame's unstuffed stream
  size_t slot = 0;
  uint32_t hdr_len = 0;
  uint32_t bpi = 0, nmark = 0;  // restart intervals: blocks per interval (0: none), markers per frame
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DevBuf<LjeTables> d_tables;
  DevBuf<uint8_t> d_hdr, d_out, d_palette;
  DevBuf<int16_t> d_coef;
  DevBuf<uint32_t> d_off, d_words, d_meta;  // d_meta: bits, size, offset (max_batch each)
  DevBuf<uint8_t> d_stage;                  // lm_enc_encode: the batch's frames (allocated at the first host call)
  HostBuf<uint32_t> h_meta;                 // size, offset
  HostBuf<uint8_t> h_out;                   // grown to the largest batch seen
  // overlay
  bool has_overlay = false;
  int src_rows = 0, src_cols = 0, flip = 0;
  DevBuf<int32_t> d_cal, d_mark_off;
  DevBuf<uint8_t> d_canvas;
  DevBuf<uint8_t> d_raw_stage;  // lm_enc_render_encode: the batch's raw frames (allocated at the first host call)
  DevBuf<lm_enc_mark> d_marks;
  lm_enc_stats stats{};
  ~lm_enc_ctx() {
    if (stream) {
      (void)hipSetDevice(device);
      (void)hipStreamSynchronize(stream);
      if (ev0) (void)hipEventDestroy(ev0);
      if (ev1) (void)hipEventDestroy(ev1);
      (void)hipStreamDestroy(stream);
    }
  }
};

namespace {

int64_t blocks_of(int32_t rows, int32_t cols, int32_t format) {
  if (rows < 1 || cols < 1 || rows > 65535 || cols > 65535) return -1;
  if (format != LM_ENC_GRAY8 && format != LM_ENC_RGB24) return -1;
  const int64_t n = format == LM_ENC_GRAY8 ? (int64_t)((rows + 7) / 8) * ((cols + 7) / 8)
                                           : 6 * (int64_t)((rows + 15) / 16) * ((cols + 15) / 16);
  return n > LM_ENC_MAX_BLOCKS ? -1 : n;
}

void check_batch(const lm_enc_ctx* c, int64_t pitch, int n, size_t frame_bytes) {
  if (n < 1 || n > c->max_batch) throw std::invalid_argument("n must be in 1..max_batch");
  if (pitch < (int64_t)frame_bytes) throw std::invalid_argument("pitch is smaller than a frame");
}

// The kernels over n frames at d_frames (device memory), then the files to the host.
void encode_on_device(lm_enc_ctx* c, const uint8_t* d_frames, int64_t pitch, int n, bool timed_from_here,
                      lm_enc_result* out) {
  const LjeGeom& g = c->g;
  uint32_t* d_bits = c->d_meta.p;
  uint32_t* d_size = c->d_meta.p + c->max_batch;
  uint32_t* d_offs = c->d_meta.p + 2 * (size_t)c->max_batch;
  if (timed_from_here) HIPCHK(hipEventRecord(c->ev0, c->stream));
  HIPCHK(hipMemsetAsync(c->d_words.p, 0, sizeof(uint32_t) * (size_t)c->wpf * (size_t)n, c->stream));
  hipLaunchKernelGGL(k_enc_coef, dim3((g.nblk + kBlocksPerGroup - 1) / kBlocksPerGroup, n), dim3(kThreads), 0, c->stream,
                     d_frames, pitch, g, c->d_tables.p, c->d_coef.p);
  const dim3 pack_grid((g.nblk + kThreads - 1) / kThreads, n);
  if (c->bpi) {
    const RstArgs<true> rst{c->d_off.p, g.nblk, c->bpi, c->nmark};
    hipLaunchKernelGGL(k_enc_scan<true>, dim3(n), dim3(kThreads), 0, c->stream, c->d_coef.p, g, c->d_tables.p, c->d_off.p,
                       d_bits, rst);
    hipLaunchKernelGGL(k_enc_pack<true>, pack_grid, dim3(kThreads), 0, c->stream, c->d_coef.p, g, c->d_tables.p, c->d_off.p,
                       c->d_words.p, c->wpf, rst);
    // every frame has the same count of markers: k_enc_count takes their bytes with the header's
    hipLaunchKernelGGL(k_enc_count, dim3(n), dim3(kThreads), 0, c->stream, c->d_words.p, c->wpf, d_bits,
                       c->hdr_len + 2u * c->nmark, d_size);
    hipLaunchKernelGGL(k_enc_offsets, dim3(1), dim3(64), 0, c->stream, d_size, n, d_offs);
    hipLaunchKernelGGL(k_enc_write<true>, dim3(n), dim3(kThreads), 0, c->stream, c->d_words.p, c->wpf, d_bits, c->d_hdr.p,
                       c->hdr_len, d_offs, c->d_out.p, rst);
  } else {
    const RstArgs<false> none{};
    hipLaunchKernelGGL(k_enc_scan<false>, dim3(n), dim3(kThreads), 0, c->stream, c->d_coef.p, g, c->d_tables.p, c->d_off.p,
                       d_bits, none);
    hipLaunchKernelGGL(k_enc_pack<false>, pack_grid, dim3(kThreads), 0, c->stream, c->d_coef.p, g, c->d_tables.p,
                       c->d_off.p, c->d_words.p, c->wpf, none);
    hipLaunchKernelGGL(k_enc_count, dim3(n), dim3(kThreads), 0, c->stream, c->d_words.p, c->wpf, d_bits, c->hdr_len, d_size);
    hipLaunchKernelGGL(k_enc_offsets, dim3(1), dim3(64), 0, c->stream, d_size, n, d_offs);
    hipLaunchKernelGGL(k_enc_write<false>, dim3(n), dim3(kThreads), 0, c->stream, c->d_words.p, c->wpf, d_bits, c->d_hdr.p,
                       c->hdr_len, d_offs, c->d_out.p, none);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  // sizes and offsets (adjacent in d_meta), then exactly the files' bytes
  COPY_SYNC(c->h_meta.p, d_size, sizeof(uint32_t) * 2 * (size_t)c->max_batch, hipMemcpyDeviceToHost, c->stream);
  const uint32_t* h_size = c->h_meta.p;
  const uint32_t* h_offs = c->h_meta.p + c->max_batch;
  const size_t total = (size_t)h_offs[n - 1] + h_size[n - 1];
  if (total > c->slot * (size_t)n) throw std::runtime_error("the encoded batch passed its worst case");
  if (c->h_out.n < total) c->h_out.alloc(total + total / 2);
  COPY_SYNC(c->h_out.p, c->d_out.p, total, hipMemcpyDeviceToHost, c->stream);
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->stats.bytes_out = (int64_t)total;
  c->stats.device_ms = ms;
  c->stats.frames = n;
  out->n = n;
  out->reserved = 0;
  out->data = c->h_out.p;
  out->offset = h_offs;
  out->size = h_size;
}

// Checks the marks, uploads them, and draws n canvases into d_canvas.
void render_on_device(lm_enc_ctx* c, const uint8_t* d_raw, int64_t pitch, int n, const lm_enc_mark* marks,
                      const int32_t* mark_offset) {
  if (!c->has_overlay) throw std::invalid_argument("lm_enc_set_overlay was not called");
  check_batch(c, pitch, n, (size_t)c->src_rows * (size_t)c->src_cols);
  if (mark_offset[0] != 0) throw std::invalid_argument("mark_offset[0] must be 0");
  for (int i = 0; i < n; ++i)
    if (mark_offset[i + 1] < mark_offset[i]) throw std::invalid_argument("mark_offset must not decrease");
  const int nm = mark_offset[n];
  if (nm > 0 && !marks) throw std::invalid_argument("marks is NULL");
  for (int m = 0; m < nm; ++m) {
    const lm_enc_mark& k = marks[m];
    if (k.radius < 0 || k.radius > LM_ENC_MAX_RADIUS) throw std::invalid_argument("a mark's radius must be in 0..LM_ENC_MAX_RADIUS");
    if (k.colour < 0 || k.colour >= LM_ENC_PALETTE_SIZE) throw std::invalid_argument("a mark's colour is not in the palette");
    if (k.x <= -(1 << 20) || k.x >= (1 << 20) || k.y <= -(1 << 20) || k.y >= (1 << 20))
      throw std::invalid_argument("a mark's coordinates are out of range");
  }
  HIPCHK(hipSetDevice(c->device));
  if (c->d_marks.n < (size_t)nm) {
    HIPCHK(hipStreamSynchronize(c->stream));
    c->d_marks.alloc((size_t)nm + (size_t)nm / 2);
  }
  if (nm) COPY_SYNC(c->d_marks.p, marks, sizeof(lm_enc_mark) * (size_t)nm, hipMemcpyHostToDevice, c->stream);
  COPY_SYNC(c->d_mark_off.p, mark_offset, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream);
  HIPCHK(hipEventRecord(c->ev0, c->stream));  // the kernels only: the uploads above are not in device_ms
  const uint32_t npix = (uint32_t)c->g.rows * (uint32_t)c->g.cols;
  hipLaunchKernelGGL(k_enc_canvas, dim3((npix + kThreads - 1) / kThreads, n), dim3(kThreads), 0, c->stream, d_raw, pitch,
                     c->d_cal.p, c->g.rows, c->g.cols, c->flip, c->d_canvas.p);
  hipLaunchKernelGGL(k_enc_marks, dim3(n), dim3(kThreads), 0, c->stream, c->d_marks.p, c->d_mark_off.p, c->g.rows, c->g.cols,
                     c->d_canvas.p, c->d_palette.p);
  HIPCHK(hipGetLastError());
}

}  // namespace

LM_API int64_t lm_enc_slot_bytes(int32_t rows, int32_t cols, int32_t format) {
  const int64_t nblk = blocks_of(rows, cols, format);
  return nblk < 0 ? -1 : LM_ENC_MAX_HEADER + 2 * 4 * (LM_ENC_BLOCK_WORDS * nblk + 1) + 2;
}

namespace {

// Words of one frame's unstuffed stream with restart intervals (locomouse_encode.h derives it).
int64_t words_restart(int64_t nblk, int64_t intervals) { return LM_ENC_BLOCK_WORDS * nblk + (intervals + 3) / 4 + 1; }

int64_t intervals_of(int64_t nblk, int32_t format, int32_t restart_interval) {
  const int64_t nmcu = nblk / (format == LM_ENC_RGB24 ? 6 : 1);
  return (nmcu + restart_interval - 1) / restart_interval;
}

}  // namespace

LM_API int64_t lm_enc_slot_bytes_restart(int32_t rows, int32_t cols, int32_t format, int32_t restart_interval) {
  if (restart_interval < 0 || restart_interval > 65535) return -1;
  if (restart_interval == 0) return lm_enc_slot_bytes(rows, cols, format);
  const int64_t nblk = blocks_of(rows, cols, format);
  if (nblk < 0) return -1;
  const int64_t ni = intervals_of(nblk, format, restart_interval);
  return LM_ENC_MAX_HEADER + 2 * 4 * words_restart(nblk, ni) + 2 * (ni - 1) + 2;
}

LM_API lm_status lm_enc_create(int32_t device, int32_t rows, int32_t cols, int32_t format, int32_t quality,
                               int32_t max_batch, lm_enc_ctx** out) {
  return lm_enc_create_restart(device, rows, cols, format, quality, max_batch, 0, out);
}

LM_API lm_status lm_enc_create_restart(int32_t device, int32_t rows, int32_t cols, int32_t format, int32_t quality,
                                       int32_t max_batch, int32_t restart_interval, lm_enc_ctx** out) {
  if (!out) return fail(LM_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (format != LM_ENC_GRAY8 && format != LM_ENC_RGB24) return fail(LM_ERR_INVALID_ARGUMENT, "format must be LM_ENC_GRAY8 or LM_ENC_RGB24");
  if (rows < 1 || cols < 1 || rows > 65535 || cols > 65535) return fail(LM_ERR_INVALID_ARGUMENT, "rows and cols must be in 1..65535");
  if (restart_interval < 0 || restart_interval > 65535) return fail(LM_ERR_INVALID_ARGUMENT, "restart_interval must be in 0..65535");
  const int64_t slot = lm_enc_slot_bytes_restart(rows, cols, format, restart_interval);
  if (slot < 0) return fail(LM_ERR_INVALID_ARGUMENT, "frame too large: more than LM_ENC_MAX_BLOCKS blocks");
  if (quality < 1 || quality > 100) return fail(LM_ERR_INVALID_ARGUMENT, "quality must be in 1..100");
  if (max_batch < 1 || max_batch > LM_ENC_MAX_BATCH) return fail(LM_ERR_INVALID_ARGUMENT, "max_batch must be in 1..LM_ENC_MAX_BATCH");
  if (slot * max_batch >= (int64_t)1 << 31) return fail(LM_ERR_INVALID_ARGUMENT, "max_batch * lm_enc_slot_bytes must stay below 2^31");
  if (device < 0) return fail(LM_ERR_INVALID_ARGUMENT, "invalid HIP device index");
  lm_enc_ctx* c = new lm_enc_ctx();
  lm_status s = guarded([&] {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device >= ndev) throw HipError("invalid HIP device index");
    c->device = device;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    c->g = lje_geom(rows, cols, format);
    c->max_batch = max_batch;
    c->quality = quality;
    c->frame_bytes = (size_t)rows * (size_t)cols * (format == LM_ENC_RGB24 ? 3 : 1);
    c->wpf = (uint32_t)(LM_ENC_BLOCK_WORDS * c->g.nblk + 1);
    if (restart_interval) {
      const uint32_t ni = lje_intervals(c->g, (uint32_t)restart_interval);
      c->bpi = (uint32_t)restart_interval * (uint32_t)c->g.bpm;
      c->nmark = ni - 1;
      c->wpf = (uint32_t)words_restart(c->g.nblk, ni);
    }
    c->slot = (size_t)slot;
    LjeTables T;
    lje::make_tables(quality, T);
    const std::vector<uint8_t> h = lje::header(rows, cols, format, quality, restart_interval);
    if (h.size() > LM_ENC_MAX_HEADER) throw std::runtime_error("the JPEG header passed LM_ENC_MAX_HEADER");
    c->hdr_len = (uint32_t)h.size();
    c->d_tables.alloc(1);
    c->d_hdr.alloc(h.size());
    c->d_palette.alloc(3 * LM_ENC_PALETTE_SIZE);
    c->d_coef.alloc((size_t)max_batch * c->g.nblk * 64);
    c->d_off.alloc((size_t)max_batch * c->g.nblk);
    c->d_words.alloc((size_t)max_batch * c->wpf);
    c->d_meta.alloc(3 * (size_t)max_batch);
    c->d_out.alloc((size_t)max_batch * c->slot);
    c->h_meta.alloc(2 * (size_t)max_batch);
    COPY_SYNC(c->d_tables.p, &T, sizeof(T), hipMemcpyHostToDevice, c->stream);
    COPY_SYNC(c->d_hdr.p, h.data(), h.size(), hipMemcpyHostToDevice, c->stream);
    COPY_SYNC(c->d_palette.p, &LM_ENC_PALETTE[0][0], 3 * LM_ENC_PALETTE_SIZE, hipMemcpyHostToDevice, c->stream);
  });
  if (s != LM_OK) {
    delete c;
    return s;
  }
  *out = c;
  return LM_OK;
}

LM_API void lm_enc_destroy(lm_enc_ctx* ctx) { delete ctx; }

LM_API lm_status lm_enc_encode_device(lm_enc_ctx* ctx, const uint8_t* d_frames, int64_t pitch, int32_t n, lm_enc_result* out) {
  if (!ctx || !d_frames || !out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    check_batch(ctx, pitch, n, ctx->frame_bytes);
    HIPCHK(hipSetDevice(ctx->device));
    encode_on_device(ctx, d_frames, pitch, n, true, out);
  });
}

LM_API lm_status lm_enc_encode(lm_enc_ctx* ctx, const uint8_t* h_frames, int64_t pitch, int32_t n, lm_enc_result* out) {
  if (!ctx || !h_frames || !out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    check_batch(ctx, pitch, n, ctx->frame_bytes);
    HIPCHK(hipSetDevice(ctx->device));
    const size_t fb = ctx->frame_bytes;
    if (!ctx->d_stage.p) ctx->d_stage.alloc(fb * (size_t)ctx->max_batch);
    HIPCHK(hipMemcpy2DAsync(ctx->d_stage.p, fb, h_frames, (size_t)pitch, fb, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    encode_on_device(ctx, ctx->d_stage.p, (int64_t)fb, n, true, out);
  });
}

LM_API lm_status lm_enc_set_overlay(lm_enc_ctx* ctx, const lm_enc_overlay* geo) {
  if (!ctx || !geo || !geo->cal) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  if (ctx->g.format != LM_ENC_RGB24) return fail(LM_ERR_INVALID_ARGUMENT, "the overlay needs an LM_ENC_RGB24 context");
  if (geo->calib_rows != ctx->g.rows || geo->calib_cols != ctx->g.cols)
    return fail(LM_ERR_INVALID_ARGUMENT, "calib_rows x calib_cols must equal the context's rows x cols");
  if (geo->src_rows < 1 || geo->src_cols < 1 || geo->src_rows > 65535 || geo->src_cols > 65535)
    return fail(LM_ERR_INVALID_ARGUMENT, "src_rows and src_cols must be in 1..65535");
  const int64_t nsrc = (int64_t)geo->src_rows * geo->src_cols, ncal = (int64_t)geo->calib_rows * geo->calib_cols;
  if (nsrc > INT32_MAX) return fail(LM_ERR_INVALID_ARGUMENT, "raw frame too large");
  for (int64_t i = 0; i < ncal; ++i)
    if (geo->cal[i] < 0 || geo->cal[i] >= nsrc) return fail(LM_ERR_INVALID_ARGUMENT, "Calibration mapping indices out of range.");
  return guarded([&] {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->has_overlay = false;
    ctx->d_raw_stage.release();  // sized from the raw frame at the next host call
    ctx->d_cal.alloc((size_t)ncal);
    if (!ctx->d_canvas.p) ctx->d_canvas.alloc(ctx->frame_bytes * (size_t)ctx->max_batch);
    if (!ctx->d_mark_off.p) ctx->d_mark_off.alloc((size_t)ctx->max_batch + 1);
    COPY_SYNC(ctx->d_cal.p, geo->cal, sizeof(int32_t) * (size_t)ncal, hipMemcpyHostToDevice, ctx->stream);
    ctx->src_rows = geo->src_rows;
    ctx->src_cols = geo->src_cols;
    ctx->flip = geo->flip ? 1 : 0;
    ctx->has_overlay = true;
  });
}

LM_API lm_status lm_enc_render_encode_device(lm_enc_ctx* ctx, const uint8_t* d_raw, int64_t pitch, int32_t n,
                                             const lm_enc_mark* marks, const int32_t* mark_offset, lm_enc_result* out) {
  if (!ctx || !d_raw || !mark_offset || !out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    render_on_device(ctx, d_raw, pitch, n, marks, mark_offset);
    encode_on_device(ctx, ctx->d_canvas.p, (int64_t)ctx->frame_bytes, n, false, out);
  });
}

LM_API lm_status lm_enc_render_encode(lm_enc_ctx* ctx, const uint8_t* h_raw, int64_t pitch, int32_t n, const lm_enc_mark* marks,
                                      const int32_t* mark_offset, lm_enc_result* out) {
  if (!ctx || !h_raw || !mark_offset || !out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    if (!ctx->has_overlay) throw std::invalid_argument("lm_enc_set_overlay was not called");
    const size_t fb = (size_t)ctx->src_rows * (size_t)ctx->src_cols;
    check_batch(ctx, pitch, n, fb);
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->d_raw_stage.n < fb * (size_t)ctx->max_batch) ctx->d_raw_stage.alloc(fb * (size_t)ctx->max_batch);
    HIPCHK(hipMemcpy2DAsync(ctx->d_raw_stage.p, fb, h_raw, (size_t)pitch, fb, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    render_on_device(ctx, ctx->d_raw_stage.p, (int64_t)fb, n, marks, mark_offset);
    encode_on_device(ctx, ctx->d_canvas.p, (int64_t)ctx->frame_bytes, n, false, out);
  });
}

LM_API lm_status lm_enc_render_device(lm_enc_ctx* ctx, const uint8_t* d_raw, int64_t pitch, int32_t n,
                                      const lm_enc_mark* marks, const int32_t* mark_offset, uint8_t* h_rgb) {
  if (!ctx || !d_raw || !mark_offset || !h_rgb) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    render_on_device(ctx, d_raw, pitch, n, marks, mark_offset);
    COPY_SYNC(h_rgb, ctx->d_canvas.p, ctx->frame_bytes * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  });
}

LM_API void* lm_enc_stream(lm_enc_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

LM_API lm_status lm_enc_last_stats(lm_enc_ctx* ctx, lm_enc_stats* out) {
  if (!ctx || !out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  *out = ctx->stats;
  return LM_OK;
}
