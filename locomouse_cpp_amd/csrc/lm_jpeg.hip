// lm_jpeg.hip — MJPEG frames decoded on the device (include/locomouse_jpeg.h):
// compressed bytes in, channel-0 frames out in device memory.
//
//   k_jpeg_scan   one workgroup per frame, one lane per subsequence of the
//                 entropy-coded segment, LMJ_LANES subsequences (a chunk) at a
//                 time: guess, sync rounds, block-count prefix sum, final pass
//                 (lm_jpeg_scan.h).  The last lane's settled exit state and the
//                 block / restart counts carry into the next chunk.
//   k_jpeg_scan_rst  the interval path, in front of k_jpeg_scan: one lane per
//                 (frame, restart interval), flattened over the batch through
//                 a per-frame exclusive offset table.  A lane starts behind its
//                 marker from the known state, with no guess, sync round or
//                 prefix sum, and must complete exactly its interval's blocks
//                 (lmj_decode_interval).  The host builds the marker index while
//                 lmj::parse walks the scan.  A frame whose index count is off,
//                 or one of whose lanes is irregular, is flagged in device
//                 memory; k_jpeg_scan returns at once for the other frames of
//                 the path and decodes the flagged ones as if the path had not
//                 run (it zeroes what the lanes wrote first), with no host round
//                 trip.
//   k_jpeg_dc     DC prediction: segmented prefix sum of the DC differences
//                 per component, restarted at each restart interval.
//   k_jpeg_idct   one thread per 8x8 block: dequantise + ISLOW IDCT into the
//                 component planes (padded to whole MCUs).
//   k_jpeg_pix    one thread per output sample: fancy upsampling of Cb and
//                 B = clamp(Y + CbToB[Cb]); Y alone for grey frames.
//
// Safety: every frame's scan is decoded from bytes [0, len) of its own slice
// (lmj_peek / lmj_advance check every index), coefficient writes are guarded
// by the frame's block count (<= max_blk, the context's allocation), sync
// rounds are bounded by the chunk's lanes, symbols by the bits of the
// subsequence.  A damaged scan ends in error bits, which become
// LM_JPEG_NEEDS_HOST.  The interval path's lanes run the same loop between two
// offsets of the marker index, which lmj_decode_interval checks against the
// scan's length before a byte is read; the index is read at lanes below the
// offset table's total only, and a lane's frame index is below n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "locomouse_jpeg.h"
#include "lm_host.h"
#include "lm_jpeg_hdr.h"
#include "lm_jpeg_scan.h"

namespace {

struct JFrame {  // one frame of the batch, as the kernels see it
  LmjScan sc;    // sc.d: device address of the scan's bytes
  int32_t tset;  // index of its Huffman table set
  int32_t active;
  uint16_t qt[2][64];  // Y and Cb quantisation tables, natural order
};

struct JOut {
  uint32_t err, rounds, max_rounds, pad;
};

static_assert(sizeof(LmjTableSet) % 4 == 0, "copied to LDS by dwords");

// Per-frame flag of the interval path, in device memory.
constexpr uint32_t kRstDone = 0;    // the interval path decodes the frame: k_jpeg_scan skips it
constexpr uint32_t kRstNone = 1;    // not on the interval path: k_jpeg_scan decodes it, its buffers are clean
constexpr uint32_t kRstFailed = 2;  // a lane of the interval path was irregular: k_jpeg_scan zeroes and decodes

// ioff: n + 1 entries, the exclusive sum of the frames' interval counts (0 for a frame that is not on the path);
// starts: ioff[n] entries, for each lane the byte of its frame's scan at which it starts (0, then the byte behind
// each marker).  Lane g belongs to the frame f with ioff[f] <= g < ioff[f + 1].
__global__ __launch_bounds__(LMJ_LANES) void k_jpeg_scan_rst(const JFrame* __restrict__ frames,
                                                             const LmjTableSet* __restrict__ tsets, int16_t* coef_all,
                                                             int32_t* dc_all, uint32_t max_blk,
                                                             const uint32_t* __restrict__ ioff, int n,
                                                             const uint32_t* __restrict__ starts, uint32_t* flag) {
  __shared__ LmjTableSet T;
  const int tid = threadIdx.x;
  const uint32_t total = ioff[n];
  const uint32_t g0 = blockIdx.x * (uint32_t)LMJ_LANES;
  if (g0 >= total) return;  // uniform over the workgroup
  auto frame_of = [&](uint32_t g) {  // g < total = ioff[n]
    int lo = 0, hi = n;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (ioff[mid] <= g)
        lo = mid;
      else
        hi = mid;
    }
    return lo;
  };
  // the table set of the workgroup's first lane goes to LDS; a lane of a frame with another set reads global memory
  const int32_t tset0 = frames[frame_of(g0)].tset;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tsets + tset0);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&T);
    for (uint32_t i = tid; i < sizeof(LmjTableSet) / 4; i += LMJ_LANES) dst[i] = src[i];
  }
  __syncthreads();
  const uint32_t g = g0 + (uint32_t)tid;
  if (g >= total) return;
  const int f = frame_of(g);
  const JFrame& F = frames[f];
  LmjScan sc = F.sc;
  if (sc.nblk > max_blk) sc.nblk = max_blk;  // (the host never asks for more)
  const uint32_t j = g - ioff[f], nint = ioff[f + 1] - ioff[f];
  const uint32_t start = starts[g], end = j + 1 < nint ? starts[g + 1] : sc.len;
  int16_t* coef = coef_all + (uint64_t)f * max_blk * 64;
  int32_t* dcd = dc_all + (uint64_t)f * max_blk;
  const bool ok = F.active && (F.tset == tset0 ? lmj_decode_interval(sc, T, j, nint, start, end, coef, dcd)
                                               : lmj_decode_interval(sc, tsets[F.tset], j, nint, start, end, coef, dcd));
  if (!ok) atomicOr(&flag[f], kRstFailed);
}

__global__ __launch_bounds__(LMJ_LANES) void k_jpeg_scan(const JFrame* __restrict__ frames,
                                                         const LmjTableSet* __restrict__ tsets, int16_t* coef_all,
                                                         int32_t* dc_all, uint32_t max_blk, JOut* out,
                                                         const uint32_t* __restrict__ flag) {
  __shared__ LmjTableSet T;
  __shared__ LmjState ex[LMJ_LANES];
  __shared__ uint32_t sblk[LMJ_LANES], srst[LMJ_LANES];
  __shared__ uint32_t s_err;
  const int tid = threadIdx.x;
  const JFrame& F = frames[blockIdx.x];
  if (!F.active) return;  // uniform over the workgroup
  const uint32_t fl = flag[blockIdx.x];
  if (fl == kRstDone) return;  // the interval path finished this frame
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tsets + F.tset);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&T);
    for (uint32_t i = tid; i < sizeof(LmjTableSet) / 4; i += LMJ_LANES) dst[i] = src[i];
  }
  if (tid == 0) s_err = 0;
  LmjScan sc = F.sc;
  if (sc.nblk > max_blk) sc.nblk = max_blk;  // (the host never asks for more)
  int16_t* coef = coef_all + (uint64_t)blockIdx.x * max_blk * 64;
  int32_t* dcd = dc_all + (uint64_t)blockIdx.x * max_blk;
  if (fl & kRstFailed) {  // what the interval path's lanes left: back to the zeroes this path starts from
    uint4* c4 = reinterpret_cast<uint4*>(coef);  // (a frame's coefficients begin at a multiple of 128 bytes)
    for (uint32_t i = tid; i < sc.nblk * 8u; i += LMJ_LANES) c4[i] = make_uint4(0, 0, 0, 0);
    for (uint32_t i = tid; i < sc.nblk; i += LMJ_LANES) dcd[i] = 0;
  }
  __syncthreads();

  LmjState carry{0, 0, 0};
  uint32_t blk0 = 0, rst0 = 0, err = 0, rounds = 0, max_rounds = 0;
  for (uint32_t base = 0; base < sc.nsub; base += LMJ_LANES) {
    const int m = (int)(sc.nsub - base < (uint32_t)LMJ_LANES ? sc.nsub - base : (uint32_t)LMJ_LANES);
    const bool on = tid < m;
    const uint32_t end_bit = on ? lmj_end_bit(sc, base + tid) : 0;
    LmjState in = carry, mine = carry;
    LmjLane lane{0, 0, 0};
    if (on) {
      if (tid) in = lmj_guess(sc, base + tid);
      mine = lmj_decode_subseq<false>(sc, T, in, end_bit, 0, 0, nullptr, nullptr, lane);
      ex[tid] = mine;
    }
    __syncthreads();
    uint32_t r = 0;
    bool settled = false;
    while (r + 1 < (uint32_t)m && !settled) {  // round r settles lane r at the latest: m - 1 rounds suffice
      ++r;
      int changed = 0;
      LmjState next = mine;
      if (on && tid) {
        const LmjState prev = ex[tid - 1];
        if (!lmj_same(prev, in)) {
          in = prev;
          next = lmj_decode_subseq<false>(sc, T, in, end_bit, 0, 0, nullptr, nullptr, lane);
          changed = !lmj_same(next, mine);
        }
      }
      __syncthreads();  // every lane has read its neighbour
      if (on) ex[tid] = next;
      mine = next;
      settled = !__syncthreads_or(changed);
    }
    rounds += r;
    max_rounds = r > max_rounds ? r : max_rounds;

    // first output block / restart count of each lane: exclusive prefix sums
    sblk[tid] = on ? lane.nblk : 0;
    srst[tid] = on ? lane.nrst : 0;
    __syncthreads();
    for (int off = 1; off < LMJ_LANES; off <<= 1) {
      const uint32_t a = tid >= off ? sblk[tid - off] : 0, b = tid >= off ? srst[tid - off] : 0;
      __syncthreads();
      sblk[tid] += a;
      srst[tid] += b;
      __syncthreads();
    }
    if (on) {
      LmjLane o;
      lmj_decode_subseq<true>(sc, T, in, end_bit, blk0 + sblk[tid] - lane.nblk, rst0 + srst[tid] - lane.nrst, coef, dcd,
                              o);
      err |= o.err;
    }
    carry = ex[m - 1];
    blk0 += sblk[LMJ_LANES - 1];
    rst0 += srst[LMJ_LANES - 1];
    __syncthreads();  // ex / sblk / srst are rewritten by the next chunk
  }
  if (blk0 != sc.nblk || carry.k != 0 || carry.b != 0) err |= LMJ_E_BLOCKS;
  if (rst0 != lmj_expected_rst(F.sc)) err |= LMJ_E_RST;  // a marker the interval asks for is missing
  if (err) atomicOr(&s_err, err);
  __syncthreads();
  if (tid == 0) {
    JOut o;
    o.err = s_err;
    o.rounds = rounds;
    o.max_rounds = max_rounds;
    o.pad = 0;
    out[blockIdx.x] = o;
  }
}

#define LMJ_DC_THREADS 256

__global__ __launch_bounds__(LMJ_DC_THREADS) void k_jpeg_dc(const JFrame* __restrict__ frames, int16_t* coef_all,
                                                            const int32_t* __restrict__ dc_all, uint32_t max_blk) {
  __shared__ int32_t ssum[LMJ_DC_THREADS][2];
  __shared__ int32_t sflag[LMJ_DC_THREADS];
  const int tid = threadIdx.x;
  const JFrame& F = frames[blockIdx.x];
  if (!F.active) return;
  LmjScan sc = F.sc;
  if (sc.nblk > max_blk) sc.nblk = max_blk;
  int16_t* coef = coef_all + (uint64_t)blockIdx.x * max_blk * 64;
  const int32_t* dcd = dc_all + (uint64_t)blockIdx.x * max_blk;
  const uint32_t per = (sc.nblk + LMJ_DC_THREADS - 1) / LMJ_DC_THREADS;
  const uint32_t b0 = (uint32_t)tid * per < sc.nblk ? (uint32_t)tid * per : sc.nblk;
  const uint32_t b1 = b0 + per < sc.nblk ? b0 + per : sc.nblk;
  uint32_t sum[2] = {0, 0};  // unsigned: wraps like the host's int on two's complement
  int flag = 0;
  for (uint32_t blk = b0; blk < b1; ++blk) {
    if (lmj_dc_reset(sc, blk)) {
      sum[0] = sum[1] = 0;
      flag = 1;
    }
    const int c = (int)lmj_comp_of(sc, blk % sc.bpm);
    if (c < 2) sum[c] += (uint32_t)dcd[blk];
  }
  ssum[tid][0] = (int32_t)sum[0];
  ssum[tid][1] = (int32_t)sum[1];
  sflag[tid] = flag;
  __syncthreads();
  if (tid == 0) {  // segmented exclusive scan over the threads' runs
    uint32_t run[2] = {0, 0};
    for (int t = 0; t < LMJ_DC_THREADS; ++t) {
      const uint32_t s0 = (uint32_t)ssum[t][0], s1 = (uint32_t)ssum[t][1];
      ssum[t][0] = (int32_t)run[0];
      ssum[t][1] = (int32_t)run[1];
      if (sflag[t]) {
        run[0] = s0;
        run[1] = s1;
      } else {
        run[0] += s0;
        run[1] += s1;
      }
    }
  }
  __syncthreads();
  uint32_t pred[2] = {(uint32_t)ssum[tid][0], (uint32_t)ssum[tid][1]};
  for (uint32_t blk = b0; blk < b1; ++blk) {
    if (lmj_dc_reset(sc, blk)) pred[0] = pred[1] = 0;
    const int c = (int)lmj_comp_of(sc, blk % sc.bpm);
    if (c >= 2) continue;
    pred[c] += (uint32_t)dcd[blk];
    coef[(uint64_t)blk * 64] = (int16_t)(int32_t)pred[c];
  }
}

__global__ __launch_bounds__(256) void k_jpeg_idct(const JFrame* __restrict__ frames, const int16_t* __restrict__ coef_all,
                                                   uint32_t max_blk, int W, int H, uint8_t* planes_y, uint64_t ysz,
                                                   uint8_t* planes_c, uint64_t csz) {
  const JFrame& F = frames[blockIdx.y];
  if (!F.active) return;
  const uint32_t blk = blockIdx.x * 256u + threadIdx.x;
  const uint32_t nblk = F.sc.nblk < max_blk ? F.sc.nblk : max_blk;
  if (blk >= nblk) return;
  const LmjPlanes P = lmj_planes(W, H, F.sc.nc, F.sc.hx, F.sc.vx);
  int comp, bx, by;
  lmj_block_pos(F.sc, P, blk, comp, bx, by);
  if (comp >= 2) return;
  const int pitch = comp ? P.pitch_c : P.pitch_y, rows = comp ? P.rows_c : P.rows_y;
  if (bx * 8 + 8 > pitch || by * 8 + 8 > rows) return;
  if ((uint64_t)pitch * rows > (comp ? csz : ysz)) return;
  uint8_t* plane = comp ? planes_c + blockIdx.y * csz : planes_y + blockIdx.y * ysz;
  lmj_idct_islow(coef_all + ((uint64_t)blockIdx.y * max_blk + blk) * 64, F.qt[comp],
                 plane + (int64_t)by * 8 * pitch + bx * 8, pitch);
}

__global__ __launch_bounds__(256) void k_jpeg_pix(const JFrame* __restrict__ frames, int W, int H,
                                                  const uint8_t* __restrict__ planes_y, uint64_t ysz,
                                                  const uint8_t* __restrict__ planes_c, uint64_t csz, uint8_t* out,
                                                  int64_t pitch) {
  const JFrame& F = frames[blockIdx.y];
  if (!F.active) return;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (uint32_t)W * (uint32_t)H) return;
  const int x = (int)(i % (uint32_t)W), y = (int)(i / (uint32_t)W);
  const LmjPlanes P = lmj_planes(W, H, F.sc.nc, F.sc.hx, F.sc.vx);
  out[blockIdx.y * pitch + i] =
      lmj_channel0(planes_y + blockIdx.y * ysz, planes_c + blockIdx.y * csz, P, F.sc.nc, F.sc.hx, F.sc.vx, x, y);
}

}  // namespace

struct lm_jpeg_ctx {
  int device = 0;
  int rows = 0, cols = 0, max_batch = 0, subseq = LMJ_SUBSEQ_DEFAULT;
  size_t scan_limit = 0;
  uint32_t max_blk = 0;
  uint64_t ysz = 0, csz = 0;
  hipStream_t stream = nullptr;
  DevBuf<uint8_t> d_bytes, d_py, d_pc;
  HostBuf<uint8_t> h_bytes;
  DevBuf<JFrame> d_frames;
  HostBuf<JFrame> h_frames;
  DevBuf<LmjTableSet> d_tsets;
  HostBuf<LmjTableSet> h_tsets;
  DevBuf<int16_t> d_coef;
  DevBuf<int32_t> d_dc;
  DevBuf<JOut> d_out;
  HostBuf<JOut> h_out;
  // interval path: ioff (max_batch + 1 entries) then flag (max_batch) in one buffer; starts grows on demand
  bool rst_on = true;
  DevBuf<uint32_t> d_rst, d_starts;
  HostBuf<uint32_t> h_rst, h_starts;
  std::vector<uint32_t> index;  // one frame's marker index
  lm_jpeg_interval_stats istats{};
  lm_jpeg_stats stats{};
  std::vector<std::unique_ptr<DevBuf<uint8_t>>> user;  // lm_jpeg_device_alloc
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~lm_jpeg_ctx() {
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

void jpeg_decode(lm_jpeg_ctx* c, const uint8_t* const* jpeg, const size_t* size, int n, uint8_t* d_out, int64_t pitch,
                 int32_t* status) {
  if (n < 0 || n > c->max_batch) throw std::invalid_argument("n exceeds the context's max_batch");
  if (pitch < (int64_t)c->rows * c->cols) throw std::invalid_argument("pitch is smaller than a frame");
  c->stats = lm_jpeg_stats{};
  c->istats = lm_jpeg_interval_stats{};
  if (n == 0) return;
  HIPCHK(hipSetDevice(c->device));
  std::vector<lmj::Header> hdr((size_t)n);
  std::map<std::string, int> sets;  // identical table sets are uploaded once
  size_t total = 0;
  int n_active = 0;
  // interval path: the lanes' start bytes, frame after frame (h_starts grows below, once the counts are known)
  std::vector<uint32_t> starts;
  uint32_t* h_ioff = c->h_rst.p;
  uint32_t* h_flag = c->h_rst.p + c->max_batch + 1;
  const auto t_parse = std::chrono::steady_clock::now();
  for (int i = 0; i < n; ++i) {
    if (!jpeg[i]) throw std::invalid_argument("jpeg[i] is NULL");
    lmj::Header& h = hdr[(size_t)i];
    lmj::parse(jpeg[i], size[i], h, c->rst_on ? &c->index : nullptr);  // the index: one more store per marker
    if (h.cls == lmj::kInScope && (h.H != c->rows || h.W != c->cols)) h.cls = lmj::kNeedsHost;
    if (h.cls == lmj::kInScope && h.scan_len > c->scan_limit) h.cls = lmj::kNeedsHost;
    status[i] = h.cls == lmj::kInScope ? LM_JPEG_OK : h.cls == lmj::kNeedsHost ? LM_JPEG_NEEDS_HOST : LM_JPEG_REJECTED;
    if (h.cls == lmj::kRejected && g_err.empty()) g_err = h.why;
    h_ioff[i] = (uint32_t)starts.size();
    h_flag[i] = kRstNone;
    if (c->rst_on && h.cls == lmj::kInScope && h.restart > 0) {
      const uint32_t expected = lmj_expected_rst(lmj::make_scan(h, (uint32_t)c->subseq));
      if (expected > 0 && c->index.size() == expected) {  // one lane per interval
        h_flag[i] = kRstDone;
        starts.push_back(0);
        uint32_t prev = 0;
        for (uint32_t off : c->index) {
          starts.push_back(off);
          c->istats.longest_interval_bytes = std::max(c->istats.longest_interval_bytes, (int32_t)(off - 2 - prev));
          prev = off;
        }
        c->istats.longest_interval_bytes =
            std::max(c->istats.longest_interval_bytes, (int32_t)((uint32_t)h.scan_len - prev));
      } else if (expected > 0) {
        ++c->istats.frames_handed_over;  // a marker is missing, or one too many: the index count differs
      }
    }
    if (h.cls == lmj::kInScope) {
      total += (h.scan_len + 15) & ~(size_t)15;
      ++n_active;
    }
  }
  h_ioff[n] = (uint32_t)starts.size();
  c->istats.parse_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_parse).count();
  if (n_active) {
    if (c->h_starts.n < starts.size()) {
      const size_t cap = starts.size() + starts.size() / 2 + 1024;
      c->h_starts.alloc(cap);
      c->d_starts.alloc(cap);
    }
    if (!starts.empty()) std::memcpy(c->h_starts.p, starts.data(), sizeof(uint32_t) * starts.size());
    if (c->h_bytes.n < total) {
      const size_t cap = total + total / 2 + 4096;
      c->h_bytes.alloc(cap);
      c->d_bytes.alloc(cap);
    }
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
      const lmj::Header& h = hdr[(size_t)i];
      JFrame& F = c->h_frames.p[i];
      std::memset(&F, 0, sizeof(F));
      if (h.cls != lmj::kInScope) continue;
      const std::string key(reinterpret_cast<const char*>(h.huff), sizeof(h.huff));  // the six built tables
      auto it = sets.find(key);
      if (it == sets.end()) {
        const int id = (int)sets.size();
        lmj::make_tables(h, c->h_tsets.p[id]);
        it = sets.emplace(key, id).first;
      }
      F.sc = lmj::make_scan(h, (uint32_t)c->subseq);
      if (F.sc.nblk > c->max_blk) {  // (not reached: the frame has the context's size.  Its lanes, if any, see an
        status[i] = LM_JPEG_NEEDS_HOST;  // inactive frame and only raise its flag)
        continue;
      }
      std::memcpy(c->h_bytes.p + off, jpeg[i] + h.scan_off, h.scan_len);
      F.sc.d = c->d_bytes.p + off;
      off += (h.scan_len + 15) & ~(size_t)15;
      F.tset = it->second;
      F.active = 1;
      std::memcpy(F.qt, h.qt, sizeof(F.qt));
      c->stats.subsequences += F.sc.nsub;
      if ((int32_t)F.sc.nsub > c->stats.max_subsequences) c->stats.max_subsequences = (int32_t)F.sc.nsub;
    }
    c->stats.table_sets = (int32_t)sets.size();
    hipStream_t st = c->stream;
    HIPCHK(hipEventRecord(c->ev0, st));
    if (off) HIPCHK(hipMemcpyAsync(c->d_bytes.p, c->h_bytes.p, off, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->d_frames.p, c->h_frames.p, sizeof(JFrame) * (size_t)n, hipMemcpyHostToDevice, st));
    if (!sets.empty())
      HIPCHK(hipMemcpyAsync(c->d_tsets.p, c->h_tsets.p, sizeof(LmjTableSet) * sets.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(c->d_coef.p, 0, sizeof(int16_t) * 64 * (size_t)c->max_blk * (size_t)n, st));
    HIPCHK(hipMemsetAsync(c->d_dc.p, 0, sizeof(int32_t) * (size_t)c->max_blk * (size_t)n, st));
    HIPCHK(hipMemsetAsync(c->d_out.p, 0, sizeof(JOut) * (size_t)n, st));
    const uint32_t lanes = h_ioff[n];
    uint32_t* d_ioff = c->d_rst.p;
    uint32_t* d_flag = c->d_rst.p + c->max_batch + 1;
    HIPCHK(hipMemcpyAsync(c->d_rst.p, c->h_rst.p, sizeof(uint32_t) * (2 * (size_t)c->max_batch + 1), hipMemcpyHostToDevice, st));
    const int W = c->cols, H = c->rows;
    if (lanes) {
      HIPCHK(hipMemcpyAsync(c->d_starts.p, c->h_starts.p, sizeof(uint32_t) * lanes, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_jpeg_scan_rst, dim3((lanes + LMJ_LANES - 1) / LMJ_LANES), dim3(LMJ_LANES), 0, st, c->d_frames.p,
                         c->d_tsets.p, c->d_coef.p, c->d_dc.p, c->max_blk, d_ioff, n, c->d_starts.p, d_flag);
    }
    hipLaunchKernelGGL(k_jpeg_scan, dim3((unsigned)n), dim3(LMJ_LANES), 0, st, c->d_frames.p, c->d_tsets.p, c->d_coef.p,
                       c->d_dc.p, c->max_blk, c->d_out.p, d_flag);
    hipLaunchKernelGGL(k_jpeg_dc, dim3((unsigned)n), dim3(LMJ_DC_THREADS), 0, st, c->d_frames.p, c->d_coef.p, c->d_dc.p,
                       c->max_blk);
    hipLaunchKernelGGL(k_jpeg_idct, dim3((c->max_blk + 255) / 256, (unsigned)n), dim3(256), 0, st, c->d_frames.p,
                       c->d_coef.p, c->max_blk, W, H, c->d_py.p, c->ysz, c->d_pc.p, c->csz);
    hipLaunchKernelGGL(k_jpeg_pix, dim3(((unsigned)(W * H) + 255) / 256, (unsigned)n), dim3(256), 0, st, c->d_frames.p,
                       W, H, c->d_py.p, c->ysz, c->d_pc.p, c->csz, d_out, pitch);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_out.p, c->d_out.p, sizeof(JOut) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (lanes) HIPCHK(hipMemcpyAsync(h_flag, d_flag, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(c->ev1, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->stats.device_ms = ms;
    c->istats.intervals = lanes;
    for (int i = 0; i < n; ++i) {
      if (!c->h_frames.p[i].active) continue;
      if (h_ioff[i + 1] > h_ioff[i]) ++(h_flag[i] == kRstDone ? c->istats.frames_interval : c->istats.frames_handed_over);
      const JOut& o = c->h_out.p[i];
      if (o.err) status[i] = LM_JPEG_NEEDS_HOST;
      c->stats.sync_rounds += o.rounds;
      if ((int32_t)o.max_rounds > c->stats.max_chunk_rounds) c->stats.max_chunk_rounds = (int32_t)o.max_rounds;
    }
  }
  for (int i = 0; i < n; ++i)
    if (status[i] != LM_JPEG_OK) ++c->stats.frames_needing_host;
}

}  // namespace

LM_API lm_status lm_jpeg_create(int32_t device, int32_t rows, int32_t cols, int32_t max_batch, int32_t subseq_bytes,
                                lm_jpeg_ctx** out) {
  if (!out) return fail(LM_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (max_batch <= 0 || max_batch > 65535)  // (frames are the grid's y dimension)
    return fail(LM_ERR_INVALID_ARGUMENT, "max_batch must be in 1..65535");
  if (rows <= 0 || cols <= 0 || rows > 65535 || cols > 65535)
    return fail(LM_ERR_INVALID_ARGUMENT, "rows and cols must be in 1..65535");
  if (subseq_bytes != 0 && (subseq_bytes < LM_JPEG_SUBSEQ_MIN || subseq_bytes > (1 << 20)))
    return fail(LM_ERR_INVALID_ARGUMENT, "subseq_bytes must be 0 or in 4..1048576");
  // (bit positions in a scan are 32-bit: 8 * (8 * rows * cols + 4096) must fit)
  if ((int64_t)rows * cols > (int64_t)1 << 25) return fail(LM_ERR_INVALID_ARGUMENT, "frame too large");
  lm_jpeg_ctx* c = new lm_jpeg_ctx();
  lm_status s = guarded([&] {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) throw HipError("invalid HIP device index");
    c->device = device;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    c->rows = rows;
    c->cols = cols;
    c->max_batch = max_batch;
    c->subseq = subseq_bytes ? subseq_bytes : LMJ_SUBSEQ_DEFAULT;
    // three components of noise at quality 100 come to about 4 bytes per pixel; the byte buffers grow on demand
    c->scan_limit = (size_t)8 * rows * cols + 4096;
    // the largest layouts over the samplings in scope
    const int sam[4][3] = {{1, 1, 1}, {3, 1, 1}, {3, 2, 1}, {3, 2, 2}};
    for (const auto& s4 : sam) {
      const LmjPlanes P = lmj_planes(cols, rows, s4[0], s4[1], s4[2]);
      const uint32_t bpm = s4[0] == 1 ? 1u : (uint32_t)(s4[1] * s4[2] + 2);
      c->max_blk = std::max(c->max_blk, (uint32_t)P.mcux * (uint32_t)P.mcuy * bpm);
      c->ysz = std::max(c->ysz, (uint64_t)P.pitch_y * P.rows_y);
      c->csz = std::max(c->csz, (uint64_t)P.pitch_c * P.rows_c);
    }
    const size_t nb = (size_t)max_batch;
    c->d_py.alloc(c->ysz * nb);
    c->d_pc.alloc(c->csz * nb);
    c->d_frames.alloc(nb);
    c->h_frames.alloc(nb);
    c->d_tsets.alloc(nb);
    c->h_tsets.alloc(nb);
    c->d_coef.alloc((size_t)c->max_blk * 64 * nb);
    c->d_dc.alloc((size_t)c->max_blk * nb);
    c->d_out.alloc(nb);
    c->h_out.alloc(nb);
    c->d_rst.alloc(2 * nb + 1);
    c->h_rst.alloc(2 * nb + 1);
    const char* env = std::getenv("LM_JPEG_RST");  // "0": the interval path is off by default (the A/B switch)
    c->rst_on = !(env && std::strcmp(env, "0") == 0);
  });
  if (s != LM_OK) {
    delete c;
    return s;
  }
  *out = c;
  return LM_OK;
}

LM_API void lm_jpeg_destroy(lm_jpeg_ctx* ctx) { delete ctx; }

LM_API lm_status lm_jpeg_decode_device(lm_jpeg_ctx* ctx, const uint8_t* const* jpeg, const size_t* size, int32_t n,
                                       uint8_t* d_out, int64_t pitch, int32_t* status) {
  if (!ctx || !jpeg || !size || !d_out || !status) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  g_err.clear();
  return guarded([&] { jpeg_decode(ctx, jpeg, size, n, d_out, pitch, status); });
}

LM_API lm_status lm_jpeg_probe(const uint8_t* data, size_t size, lm_jpeg_info* info) {
  if (!data || !info) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  std::memset(info, 0, sizeof(*info));
  lmj::Header h;
  lmj::parse(data, size, h);
  info->rows = h.H;
  info->cols = h.W;
  info->components = h.nc;
  info->h_samp = h.h[0];
  info->v_samp = h.v[0];
  info->restart_interval = h.restart;
  info->scan_bytes = (int64_t)h.scan_len;
  info->status = h.cls == lmj::kInScope ? LM_JPEG_OK : h.cls == lmj::kNeedsHost ? LM_JPEG_NEEDS_HOST : LM_JPEG_REJECTED;
  std::strncpy(info->reason, h.why.c_str(), sizeof(info->reason) - 1);
  return LM_OK;
}

LM_API lm_status lm_jpeg_device_alloc(lm_jpeg_ctx* ctx, size_t bytes, uint8_t** d_out) {
  if (!ctx || !d_out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  *d_out = nullptr;
  return guarded([&] {
    HIPCHK(hipSetDevice(ctx->device));
    auto b = std::make_unique<DevBuf<uint8_t>>();
    b->alloc(bytes);
    *d_out = b->p;
    ctx->user.push_back(std::move(b));
  });
}

LM_API lm_status lm_jpeg_device_free(lm_jpeg_ctx* ctx, uint8_t* d) {
  if (!ctx) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  for (auto it = ctx->user.begin(); it != ctx->user.end(); ++it)
    if ((*it)->p == d) {
      (void)hipSetDevice(ctx->device);
      ctx->user.erase(it);
      return LM_OK;
    }
  return fail(LM_ERR_INVALID_ARGUMENT, "not a buffer of this context");
}

LM_API lm_status lm_jpeg_upload(lm_jpeg_ctx* ctx, uint8_t* d_dst, const uint8_t* src, size_t bytes) {
  if (!ctx || !d_dst || !src) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  return guarded([&] {
    HIPCHK(hipSetDevice(ctx->device));
    COPY_SYNC(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream);
  });
}

LM_API void* lm_jpeg_stream(lm_jpeg_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

LM_API lm_status lm_jpeg_set_interval_path(lm_jpeg_ctx* ctx, int32_t on) {
  if (!ctx) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  ctx->rst_on = on != 0;
  return LM_OK;
}

LM_API lm_status lm_jpeg_debug_interval_stats(lm_jpeg_ctx* ctx, lm_jpeg_interval_stats* out) {
  if (!ctx || !out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  *out = ctx->istats;
  return LM_OK;
}

LM_API lm_status lm_jpeg_debug_stats(lm_jpeg_ctx* ctx, lm_jpeg_stats* out) {
  if (!ctx || !out) return fail(LM_ERR_INVALID_ARGUMENT, "null argument");
  *out = ctx->stats;
  return LM_OK;
}
