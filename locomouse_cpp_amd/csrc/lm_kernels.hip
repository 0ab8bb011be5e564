// lm_kernels.hip — gfx950 kernels of the LocoMouse per-frame detection path.
//
// Batch pipeline (one launch each, grid over frame slots; see lm_device.h):
//   k_minmax      per-frame min/max of sat(F - BKG), frames split over workgroups
//   k_lut         -> normalize LUT (+ TM imadjust)
//                 LocoMouse_class.cpp:1304-1310, TM.cpp:247, :3204-3242
//   k_ingest      calibration gather + flip + LUT (+ the in-place grey-level LUT of
//                 transform_gray_values) -> extended padded crops (u8)
//                 :1316-1327 (correctImage :1337-1406), cropBoundingBox :1408-1478;
//                 with them the pixel range of every aligned block of 8 columns
//   k_tile_bound  every detector's 40 x 4 tiles whose scores are not proven
//                 negative (lm_tail_bound.h, from those ranges), listed and
//                 flagged for k_corr (k_tile_bound_ref: from the crops)
//   k_corr        all six filter2D detectors, fp32 row-major FMA chains, LDS-tiled;
//                 epilogue: brightness mask + score>0 compaction / tail binarisation
//                 :845, :860, :2575-2576, :782, :817, :849, :864, :2593-2598
//   k_tail        largest connected component (bottom, then side AND column mask),
//                 TAIL_MASK, 15-segment binary moments  :2558-2767
//   k_nms         tail-mask filter, sort (bitonic; libstdc++ introsort replica on
//                 exact ties), nmsMax (bottom) / peakClustering (side)  :1610-1905
//   k_post        unary costs, pairwise CSC, side<->bottom matching with the
//                 motion criterion  :873-919, :999-1267, :1909-2070
//   k_carry       previous frame's bottom candidates into slot 0 of the next batch
//
// All floating-point code is compiled with -ffp-contract=off; the correlation
// uses explicit fmaf in the reference's row-major tap order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "lm_device.h"
#include "lm_introsort.h"

#include "lm_dev_common.h"
#include "lm_match_core.h"
#include "lm_corr_narrow.h"
#include "lm_tail_bound.h"
#include "lm_tile_plan.h"

// ------------------------------------------------------------------ helpers

// (ipad_pixel: lm_dev_common.h, shared with lm_train.hip's gather)

// --------------------------------------------------------------- k_minmax
// normalize(F, F, 0, 255, NORM_MINMAX, CV_8UC1) after subtract(F, BKG, F)
// (LocoMouse_class.cpp:1304-1310) needs min and max of sat(F - BKG) per frame.
// Each frame is split over LM_MM_SPLIT workgroups (16-byte loads of frame and
// background, wave and block reductions); each workgroup writes its partial
// min/max pair, and k_lut folds the LM_MM_SPLIT pairs of a slot into its LUT.
__global__ __launch_bounds__(LM_MM_THREADS) void k_minmax(const uint8_t* const* __restrict__ frame_ptr,
                                                          const uint8_t* __restrict__ bkg, int npix, int s0,
                                                          unsigned* __restrict__ mm) {
  const int slot = s0 + blockIdx.y;
  const lm_gu8* __restrict__ F = as_global(frame_ptr[slot]);
  const int nvec = npix >> 4;
  const int per = (nvec + LM_MM_SPLIT - 1) / LM_MM_SPLIT;
  const int v0 = blockIdx.x * per, v1 = min(nvec, v0 + per);
  const lm_gu4* F4 = reinterpret_cast<const lm_gu4*>(F);
  const uint4* B4 = reinterpret_cast<const uint4*>(bkg);
  unsigned mn = 255, mx = 0;
  auto fold = [&](unsigned fw, unsigned bw) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned fv = (fw >> (8 * k)) & 255u, bv = (bw >> (8 * k)) & 255u;
      const unsigned d = fv > bv ? fv - bv : 0u;
      mn = min(mn, d);
      mx = max(mx, d);
    }
  };
  int i = v0 + threadIdx.x;
  for (; i + 3 * LM_MM_THREADS < v1; i += 4 * LM_MM_THREADS) {  // four 16-byte loads in flight per lane
    lm_u32x4 f[4];
    uint4 b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      f[u] = F4[i + u * LM_MM_THREADS];
      b[u] = B4[i + u * LM_MM_THREADS];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      fold(f[u].x, b[u].x);
      fold(f[u].y, b[u].y);
      fold(f[u].z, b[u].z);
      fold(f[u].w, b[u].w);
    }
  }
  for (; i < v1; i += LM_MM_THREADS) {
    const lm_u32x4 f = F4[i];
    const uint4 b = B4[i];
    fold(f.x, b.x);
    fold(f.y, b.y);
    fold(f.z, b.z);
    fold(f.w, b.w);
  }
  if (blockIdx.x == LM_MM_SPLIT - 1)  // the bytes past the last 16-byte word
    for (int q = (nvec << 4) + threadIdx.x; q < npix; q += LM_MM_THREADS) {
      const unsigned fv = F[q], bv = bkg[q];
      const unsigned d = fv > bv ? fv - bv : 0u;
      mn = min(mn, d);
      mx = max(mx, d);
    }
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, (unsigned)__shfl_xor((int)mn, o));
    mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
  }
  __shared__ unsigned smn[LM_MM_THREADS / 64], smx[LM_MM_THREADS / 64];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    smn[wid] = mn;
    smx[wid] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < LM_MM_THREADS / 64; ++w) {
      mn = min(mn, smn[w]);
      mx = max(mx, smx[w]);
    }
    mm[2 * (slot * LM_MM_SPLIT + blockIdx.x)] = mn;
    mm[2 * (slot * LM_MM_SPLIT + blockIdx.x) + 1] = mx;
  }
}

// Entry p of a frame's LUT from its min/max: normalize(NORM_MINMAX) ->
// convertTo(CV_8U, scale, shift) = sat_u8(cvRound((float)p*(float)scale +
// (float)shift)) (OpenCV 3.x, unfused), the noScale copy when scale == 1 and
// shift == 0, then the LocoMouse_TM imadjust LUT (methods 1/2, TM.cpp:247).
DEV int norm_lut_entry(unsigned mnv, unsigned mxv, int p, const uint8_t* adj, int use_adj) {
  const double smin = (double)mnv, smax = (double)mxv, dmin = 0.0, dmax = 255.0;
  const double scale = (dmax - dmin) * (smax - smin > 2.220446049250313e-16 ? 1. / (smax - smin) : 0.0);
  const double shift = dmin - smin * scale;
  int v;
  if (fabs(scale - 1.0) < 2.220446049250313e-16 && fabs(shift) < 2.220446049250313e-16) {
    v = p;  // convertTo noScale -> copy
  } else {
    const float sf = (float)scale, hf = (float)shift;
    float t = __fmul_rn((float)p, sf);
    t = __fadd_rn(t, hf);
    const int iv = (int)rintf(t);
    v = iv < 0 ? 0 : (iv > 255 ? 255 : iv);
  }
  return use_adj ? adj[v] : v;
}

// k_lut: the 256-entry LUT of every slot from k_minmax's partial min/max
// pairs.  4 slots per block.
__global__ __launch_bounds__(256) void k_lut(const unsigned* __restrict__ mm, int s0, int s_end,
                                             const uint8_t* __restrict__ adj, int use_adj, uint8_t* __restrict__ luts) {
  for (int s = s0 + blockIdx.x * 4; s < min(s_end, s0 + (int)blockIdx.x * 4 + 4); ++s) {
    unsigned mn = 255, mx = 0;
#pragma unroll
    for (int b = 0; b < LM_MM_SPLIT; ++b) {
      mn = min(mn, mm[2 * (s * LM_MM_SPLIT + b)]);
      mx = max(mx, mm[2 * (s * LM_MM_SPLIT + b) + 1]);
    }
    luts[s * 256 + threadIdx.x] = (uint8_t)norm_lut_entry(mn, mx, threadIdx.x, adj, use_adj);
  }
}

// I_PAD(R, C) of frame slot `sl` as the per-frame steps after
// cropBoundingBox see it: transform_gray_values with a CV_8U table rewrites
// the frame's bottom crop I_BOTTOM_MOUSE in place (LUT(I_BOTTOM_MOUSE, table,
// I_BOTTOM_MOUSE), LocoMouse_class.cpp:1445-1448), so that rectangle of I_PAD
// holds table[v] for the rest of the frame and in I_PREV_PAD for the next.
struct GrayRect {  // the LmConst fields in_gray_rect reads
  int32_t unpad_y[1], unpad_x[1], bb_bottom_h, bb_bottom_w;
};
template <class KT>
DEV bool in_gray_rect(const KT& K, const LmSlot& sl, int R, int C) {
  const int y = R - sl.crop_y[0] - K.unpad_y[0], x = C - sl.crop_x[0] - K.unpad_x[0];
  return (unsigned)y < (unsigned)K.bb_bottom_h && (unsigned)x < (unsigned)K.bb_bottom_w;
}

template <class FP>
DEV uint8_t ipad_pixel_t(FP __restrict__ F, const uint8_t* __restrict__ bkg, const int32_t* __restrict__ cal,
                         const uint8_t* lut, const LmConst& K, const LmSlot& sl, int R, int C) {
  const uint8_t v = ipad_pixel(F, bkg, cal, lut, K, R, C);
  // a matched context: the slot's own table (k_match), match_off bytes after its normalisation table -- so `lut`
  // must point into the lane's global table buffer (luts + 256 slot), never at a copy of the table in LDS or
  // elsewhere; k_post's motion test and k_match_crop, the callers, pass exactly that
  if (K.match_on) return in_gray_rect(K, sl, R, C) ? lut[K.match_off + v] : v;
  return K.gray_lut_on && in_gray_rect(K, sl, R, C) ? K.gray_lut[v] : v;
}

// ---------------------------------------------------------------- k_ingest
// Builds the extended padded crops of both views for LM_INGEST_FB consecutive
// slots: every I_PAD pixel any detector tap reads (readFrame's correctImage +
// flip, :1316-1327 / :1337-1406; cropBoundingBox, :1408-1478).  One workgroup
// per (view, 8-row band of the view's ext crop, slot group): the bands are
// aligned with the dark-tile flag grid (band b holds the point detectors'
// output rows 8b .. 8b + 7), so the workgroup that writes a tile row's pixels
// also decides which of its LM_FW x LM_FH output tiles are bright (some I_*_MOUSE
// pixel > 25, LocoMouse_class.cpp:782, :817), writes their flag bytes and
// appends the bright ones to the view's tile list -- no second pass over the
// crops.  Each thread owns 16 consecutive crop bytes of the band (one 16-byte
// store per frame).  The calibration index and background byte of each are
// loaded once and reused for every slot whose crop sits at the same place
// (always, with a provided bounding box); per frame only the frame gather, the
// LUTs and the store remain.  Where the 16 source pixels are consecutive in
// the frame (a calibration map that is locally a translation, flipped or not)
// the gather is five aligned dword loads instead of sixteen byte loads.
// (LM_INGEST_VEC, LM_INGEST_MAXTX: lm_tile_plan.h)

// Gather index of crop pixel I_PAD (R, C) (-1 outside I_UNPAD).
DEV int ingest_index(const LmConst& K, const int32_t* __restrict__ cal, int R, int C) {
  const int r = R - K.pad_pre_rows;
  int c = C - K.pad_pre_cols;
  if (r < 0 || r >= K.n_rows || c < 0 || c >= K.n_cols) return -1;
  if (K.flip) c = K.n_cols - 1 - c;
  return cal[r * K.n_cols + c];
}

// Gather indices and background bytes of the 16 crop pixels that start at
// I_PAD (R, C0) (0 background outside I_UNPAD).  inside: bit k set when
// pixel k lies inside I_UNPAD.  Returns 1 when the inside pixels are a run
// idx[k] = lo + k, -1 when idx[k] = lo + 15 - k (a flipped translation) --
// a chunk at the pad's edge is a run too, its outside bytes masked to 0
// after the LUT (I_PAD is zero outside I_UNPAD), and a chunk with no inside
// pixel is an empty run -- else 0 (a gather).  lo is the first source byte
// of the 20 the run's five dwords cover; a run whose dwords would leave the
// frame is a gather.  (k_ingest keeps only run, lo, inside and the
// background bytes: a gather re-reads the indices per frame, ingest_index,
// so no 16-register index array stays live.)
DEV int ingest_locate(const LmConst& K, const int32_t* __restrict__ cal, const uint8_t* __restrict__ bkg, int R, int C0,
                      uint32_t (&bw)[4], int& lo, unsigned& inside) {
  const int r = R - K.pad_pre_rows;
  inside = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) bw[j] = 0u;
  // one pass, no index array: the first inside pixel fixes the candidate
  // runs' virtual idx[0] (up0 for a run, dn0 for a flipped one), the later
  // ones are tested against them
  int up0 = 0, dn0 = 0;
  bool any = false, up = true, down = true;
#pragma unroll
  for (int k = 0; k < LM_INGEST_VEC; ++k) {
    int c = C0 + k - K.pad_pre_cols;
    if (r >= 0 && r < K.n_rows && c >= 0 && c < K.n_cols) {
      if (K.flip) c = K.n_cols - 1 - c;
      const int ix = cal[r * K.n_cols + c];
      bw[k >> 2] |= (uint32_t)bkg[ix] << (8 * (k & 3));
      inside |= 1u << k;
      if (!any) {
        up0 = ix - k;
        dn0 = ix + k;
        any = true;
      } else {
        up = up && ix == up0 + k;
        down = down && ix == dn0 - k;
      }
    }
  }
  if (!any) {  // no pixel inside I_UNPAD: all zeros
    lo = 0;
    return 1;
  }
  int run = up ? 1 : (down ? -1 : 0);
  lo = up ? up0 : dn0 - (LM_INGEST_VEC - 1);
  if (run != 0 && (lo < 0 || (lo & ~3) + 20 > K.video_rows * K.video_cols)) run = 0;  // the dwords would leave the frame
  return run;
}

// 0xFF in byte j of the result for bit j of the 4-bit n (masking a word's
// outside bytes)
DEV uint32_t byte_keep4(uint32_t n) { return ((n * 0x00204081u) & 0x01010101u) * 0xFFu; }

// Source map of one view's crop at a fixed position (cx, cy): per 16-byte
// ext-crop chunk, {first source byte, run code | inside mask} and the 16
// background bytes, so
// k_ingest's batches with their crop there (always, with a provided bounding
// box) skip the calibration and background gathers (frame-invariant data,
// LocoMouse_class.cpp:1337-1406).  key[2 v], key[2 v + 1] = the position.
__global__ __launch_bounds__(256) void k_srcmap(const LmConst* __restrict__ Kp, const int32_t* __restrict__ cal,
                                                const uint8_t* __restrict__ bkg, int v, int cx, int cy,
                                                int2* __restrict__ smap, uint4* __restrict__ sbkg,
                                                int32_t* __restrict__ key) {
  const LmConst& K = *Kp;
  const int64_t e0 = (int64_t)K.ext_h[0] * K.ext_w[0];
  const int64_t nv = (int64_t)K.ext_h[v] * K.ext_w[v];
  const int64_t qq = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * LM_INGEST_VEC;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    key[2 * v] = cx;
    key[2 * v + 1] = cy;
  }
  if (qq >= nv) return;
  const int er = (int)(qq / K.ext_w[v]), ec = (int)(qq % K.ext_w[v]);
  uint32_t w[4];
  int lo;
  unsigned inside;
  const int run = ingest_locate(K, cal, bkg, cy + K.ext_oy[v] + er, cx + K.ext_ox[v] + ec, w, lo, inside);
  const int64_t ci = ((v ? e0 : 0) + qq) / LM_INGEST_VEC;
  // y: run code (1 up, 2 down, 0 a gather) | inside mask << 16
  smap[ci] = make_int2(lo, (run > 0 ? 1 : run < 0 ? 2 : 0) | (int)(inside << 16));
  sbkg[ci] = make_uint4(w[0], w[1], w[2], w[3]);
}

// Bright bytes (> 25: threshold(25.5, BINARY_INV) leaves them unmasked) of a
// packed word, as 0x80 in each such byte.
DEV uint32_t bright_bytes(uint32_t w) {
  return (((w & 0x7F7F7F7Fu) + 0x66666666u) | w) & 0x80808080u;
}
// 0x80 in byte i of the result for bit i of the 4-bit n
DEV uint32_t byte_mask4(uint32_t n) { return ((n * 0x00204081u) & 0x01010101u) << 7; }

// Largest byte | smallest byte << 8 of the eight bytes of a, b: the pixel range
// of an aligned block of LM_TB_BLK columns (lm_tail_bound.h; a 16-byte chunk
// holds two of them: lm_tile_plan.h).
DEV uint32_t block_range(uint32_t a, uint32_t b) {
  uint32_t mx = 0u, mn = 255u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t x = (a >> (8 * j)) & 0xFFu, y = (b >> (8 * j)) & 0xFFu;
    mx = max(mx, max(x, y));
    mn = min(mn, min(x, y));
  }
  return mx | mn << 8;
}

// The five aligned dwords that cover the 16 source bytes [lo, lo + 16) of a
// run: one dwordx4 (gfx950 global loads need only dword alignment) plus one
// dword -- two vector-memory instructions instead of five.
#ifndef LM_INGEST_X4
#define LM_INGEST_X4 1
#endif
typedef uint32_t lm_u4a4 __attribute__((ext_vector_type(4), aligned(4)));
DEV void ingest_run_load(const lm_gu8* F, int lo, uint32_t (&d)[5]) {
  const lm_gu32* w = reinterpret_cast<const lm_gu32*>(F + (lo & ~3));
#if LM_INGEST_X4
  const lm_u4a4 a = *reinterpret_cast<const __attribute__((address_space(1))) lm_u4a4*>(w);
  d[0] = a.x;
  d[1] = a.y;
  d[2] = a.z;
  d[3] = a.w;
  d[4] = w[4];
#else
#pragma unroll
  for (int u = 0; u < 5; ++u) d[u] = w[u];
#endif
}

#ifndef LM_INGEST_PIPE
#define LM_INGEST_PIPE 3  // frames whose run loads are in flight at once
#endif
#ifndef LM_INGEST_WPE
#define LM_INGEST_WPE 5  // amdgpu_waves_per_eu minimum: <= 96 VGPRs, so 5 four-wave groups per CU (one round at C3)
#endif
// MATCH: a matched context (k_match): the grey LUT is the slot's own table, the tables of the slot group in LDS
template <bool MATCH>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(LM_INGEST_WPE, 8))) void k_ingest(const LmConst* __restrict__ Kp, const uint8_t* const* __restrict__ frame_ptr,
                                                 const uint8_t* __restrict__ bkg, const int32_t* __restrict__ cal,
                                                 const uint8_t* __restrict__ luts, const LmSlot* __restrict__ slots,
                                                 int s0, int s_end, uint8_t* __restrict__ ext, int64_t ext_slot_bytes,
                                                 unsigned* __restrict__ tailbm, const int2* __restrict__ smap,
                                                 const uint4* __restrict__ sbkg, const int32_t* __restrict__ skey,
                                                 uint8_t* __restrict__ flags, int32_t* __restrict__ tl_cnt,
                                                 uint32_t* __restrict__ tl_list, uint32_t* __restrict__ rng,
                                                 long long* __restrict__ prof) {
  const LmConst& K = *Kp;
  // LM_KPROF=1: clock64() of thread 0 at the phase ends, wall clock at start / end
  long long* pb = prof ? prof + (int64_t)(blockIdx.y * gridDim.x + blockIdx.x) * 16 : nullptr;
#define ING_PROF(k) \
  if (pb && threadIdx.x == 0) pb[k] = clock64();
  ING_PROF(0)
  if (pb && threadIdx.x == 0) pb[14] = wall_clock64();
  const int sb = s0 + blockIdx.y * LM_INGEST_FB;
  const int nf = min(LM_INGEST_FB, s_end - sb);
  const int T = (int)blockDim.x, tid = (int)threadIdx.x;
  {  // this block's share of the group's tail bitmaps is zeroed (k_corr ORs the tail detectors' bits in)
    const int per = (K.tail_bm_words + (int)gridDim.x - 1) / (int)gridDim.x;
    const int w0 = (int)blockIdx.x * per, w1 = min(K.tail_bm_words, w0 + per);
    for (int f = 0; f < nf; ++f) {
      unsigned* __restrict__ t = tailbm + (int64_t)(sb + f) * K.tail_bm_words;
      for (int w = w0 + tid; w < w1; w += T) t[w] = 0u;
    }
  }
  // this block's view and band
  const int v = (int)blockIdx.x < K.ing_nb[0] ? 0 : 1;
  const int band = K.ing_b0[v] + (int)blockIdx.x - (v ? K.ing_nb[0] : 0);
  const int ew = K.ext_w[v], cw = ew / LM_INGEST_VEC, nch = 8 * cw;
  const int64_t e0 = (int64_t)K.ext_h[0] * K.ext_w[0];
  constexpr int FPB = 8 / LM_FH;  // flag rows per band
  const bool fl_band = flags != nullptr && band >= 0 && band * FPB < K.fl_ty[v];
  const int ftx = K.fl_tx[v];
  // One round of independent loads (the group's LUTs into registers, the
  // slots, the first chunk's source map entry), then the frame loads the map
  // points at, and only then the LUTs into LDS and the barrier: the group
  // costs two load latencies, not four (LUT copy, slots, map, frames one
  // after another).
  __shared__ __attribute__((aligned(16))) uint8_t lut[LM_INGEST_FB][256];
  __shared__ __attribute__((aligned(MATCH ? 8 : 1))) uint8_t glut[MATCH ? LM_INGEST_FB * 256 : 256];
  __shared__ uint8_t s_fl[LM_INGEST_FB][8 / LM_FH][LM_INGEST_MAXTX];  // bright output tiles of the band, per slot
  __shared__ uint32_t s_ent[LM_INGEST_FB * (8 / LM_FH) * LM_INGEST_MAXTX];
  __shared__ int s_n, s_outs, s_base;
  for (int i = tid; i < LM_INGEST_FB * 256 / 8; i += T) {
    const int li = i * 8;
    if (li < nf * 256) *reinterpret_cast<uint2*>(&lut[0][0] + li) = *reinterpret_cast<const uint2*>(luts + (int64_t)sb * 256 + li);
  }
  if constexpr (MATCH) {
    for (int i = tid; i < LM_INGEST_FB * 256 / 8; i += T) {
      const int li = i * 8;
      if (li < nf * 256) *reinterpret_cast<uint2*>(&glut[0] + li) = *reinterpret_cast<const uint2*>(luts + K.match_off + (int64_t)sb * 256 + li);
    }
  } else {
    for (int i = tid; i < 256; i += T) glut[i] = K.gray_lut[i];
  }
  for (int i = tid; i < LM_INGEST_FB * FPB * LM_INGEST_MAXTX; i += T) (&s_fl[0][0][0])[i] = 0;
  if (tid == 0) {
    s_n = 0;
    s_outs = 0;
  }
  // the grey LUT's switch and rectangle, read once (in_gray_rect takes them from gk)
  const bool gray_on = MATCH || K.gray_lut_on != 0;
  GrayRect gk;
  gk.unpad_y[0] = K.unpad_y[0];
  gk.unpad_x[0] = K.unpad_x[0];
  gk.bb_bottom_h = K.bb_bottom_h;
  gk.bb_bottom_w = K.bb_bottom_w;
  const LmSlot sl0 = slots[sb];
  bool same = true;
  for (int f = 1; f < nf; ++f)
    same = same && slots[sb + f].crop_x[v] == sl0.crop_x[v] && slots[sb + f].crop_y[v] == sl0.crop_y[v];
  const bool mapped = same && smap && skey[2 * v] == sl0.crop_x[v] && skey[2 * v + 1] == sl0.crop_y[v];
  // chunk i of the band: ext row er, byte column ec (a multiple of 16)
  auto chunk_pos = [&](int i, int& er, int& ec) {
    const int rr = i / cw;
    er = K.fl_my[v] + 8 * band + rr;
    ec = (i - rr * cw) * LM_INGEST_VEC;
    return i < nch && er >= 0 && er < K.ext_h[v];
  };
  // the run loads of frames f .. f + LM_INGEST_PIPE - 1 in flight at once:
  // frame f's registers take frame f + LM_INGEST_PIPE's loads as soon as they
  // are consumed, so the group needs LM_INGEST_PIPE x 5 registers for them,
  // not LM_INGEST_FB x 5 (five waves per SIMD: the grid is one round)
  constexpr int PIPE = LM_INGEST_PIPE;
  uint32_t d[PIPE][5];
  int2 m = make_int2(0, 0);
  uint4 b4 = make_uint4(0u, 0u, 0u, 0u);
  auto frame_load = [&](int f, int lo_, uint32_t (&dd)[5]) {
    ingest_run_load(as_global(frame_ptr[sb + f]), lo_, dd);
  };
  // the fast path's loads of chunk i (source map entry, then the first frames' run dwords)
  auto fast_loads = [&](int i) {
    int er, ec;
    const bool act = chunk_pos(i, er, ec);
    m = make_int2(0, 0);
    if (act && mapped) {
      const int64_t ci = ((v ? e0 : 0) + (int64_t)er * ew + ec) / LM_INGEST_VEC;
      m = smap[ci];
      b4 = sbkg[ci];
      if ((m.y & 3) != 0) {
#pragma unroll
        for (int f = 0; f < PIPE; ++f)
          if (f < nf) frame_load(f, m.x, d[f]);
      }
    }
  };
  ING_PROF(1)
  fast_loads(tid);
  __syncthreads();
  ING_PROF(2)

  for (int i = tid; i < nch; i += T) {
    if (i != tid) fast_loads(i);
    int er, ec;
    if (!chunk_pos(i, er, ec)) continue;
    const int64_t q = (v ? e0 : 0) + (int64_t)er * ew + ec;  // byte offset in the slot's ext crops
    // dark-tile flags: the bytes of this chunk that are point-detector
    // outputs' I_*_MOUSE pixels (output (y, x) = ext (fl_my + y, fl_mx + x)),
    // split at the LM_FW-column tile boundary: tile ta and ta + 1
    uint32_t ma[4] = {0u, 0u, 0u, 0u}, mb[4] = {0u, 0u, 0u, 0u};
    int ta = 0;
    const int y = er - K.fl_my[v];
    const int fr = (y - 8 * band) / LM_FH;  // the chunk's flag row in the band (when fl_band)
    if (fl_band && y < K.fl_oh[v]) {
      const int x0 = ec - K.fl_mx[v];
      ta = x0 >= 0 ? x0 / LM_FW : -((LM_FW - 1 - x0) / LM_FW);
      const int lo = max(0, -x0), hi = min(LM_INGEST_VEC, K.fl_ow[v] - x0), ks = (ta + 1) * LM_FW - x0;
      auto range = [](int a, int b) -> uint32_t {  // bits [a, b) of 16
        return a < b ? ((b >= 32 ? 0xFFFFFFFFu : (1u << b) - 1u) & ~((1u << a) - 1u)) & 0xFFFFu : 0u;
      };
      const uint32_t bits_a = range(lo, min(hi, ks)), bits_b = range(max(lo, ks), hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ma[j] = byte_mask4((bits_a >> (4 * j)) & 0xFu);
        mb[j] = byte_mask4((bits_b >> (4 * j)) & 0xFu);
      }
    }
    const bool flag_chunk = (ma[0] | ma[1] | ma[2] | ma[3] | mb[0] | mb[1] | mb[2] | mb[3]) != 0u;
    uint32_t bw[4];  // background bytes, packed
    int run = 0;  // 1: idx[k] = idx[0] + k, -1: idx[k] = idx[0] - k, 0: gather
    int lo = 0;   // a run's first source byte
    unsigned inside = 0xFFFFu;  // bit k: pixel k inside I_UNPAD (the others are masked to 0 after the LUT)
    // the 16 source bytes of a run span [lo, lo + 16): five aligned dwords cover them
    // (funnel shifts by the byte offset, then a byte reversal for a flipped run:
    // no register array is indexed with a run-time value, so nothing spills)
    auto run_bytes = [&](const uint32_t (&dd)[5], uint32_t (&w)[4]) {
      const unsigned sh = (unsigned)(lo & 3);
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = __builtin_amdgcn_alignbyte(dd[j + 1], dd[j], sh);
      if (run < 0) {
        const uint32_t r0 = __builtin_bswap32(w[3]), r1 = __builtin_bswap32(w[2]), r2 = __builtin_bswap32(w[1]),
                       r3 = __builtin_bswap32(w[0]);
        w[0] = r0;
        w[1] = r1;
        w[2] = r2;
        w[3] = r3;
      }
    };
    // background subtraction, the slot's LUT, the grey LUT, the 16-byte store
    // and the chunk's bright-tile bits (pixels and background bytes stay
    // packed four to a register)
    // Pixels outside I_UNPAD (inside bit clear: the pad, or the background-
    // and-LUT of a don't-care byte) are zeroed after the LUT, once per word.
    // The grey LUT is a separate instantiation (GRAY, chosen once per
    // kernel): a K field tested per byte made the compiler re-load it per
    // byte and wait for it -- with the LUT read just issued, whose wait
    // counter the scalar load shares -- so every byte's LDS read was waited
    // for on its own.
    auto emit = [&](int f, const uint32_t (&pw)[4], const LmSlot& sl, int R, int C0, unsigned in_mask, auto gray_c) {
      constexpr bool GRAY = decltype(gray_c)::value;
      uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < LM_INGEST_VEC; ++k) {
        const uint32_t pk = (pw[k >> 2] >> (8 * (k & 3))) & 0xFFu, bk = (bw[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        uint32_t o = lut[f][pk > bk ? pk - bk : 0];
        // (the grey LUT's rectangle never reaches the pad: the host rejects that)
        if (GRAY && in_gray_rect(gk, sl, R, C0 + k)) o = glut[(MATCH ? f * 256 : 0) + o];
        word[k >> 2] |= o << (8 * (k & 3));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) word[j] &= byte_keep4((in_mask >> (4 * j)) & 0xFu);
      *reinterpret_cast<uint4*>(ext + (int64_t)(sb + f) * ext_slot_bytes + q) = make_uint4(word[0], word[1], word[2], word[3]);
      // k_tile_bound's block ranges: largest and smallest byte of each aligned
      // half of the chunk as stored (rng: a kernel argument, tested once per chunk)
      if (rng)
        rng[(int64_t)(sb + f) * (ext_slot_bytes / LM_INGEST_VEC) + q / LM_INGEST_VEC] =
            block_range(word[0], word[1]) | block_range(word[2], word[3]) << 16;
      if (flag_chunk) {
        uint32_t ha = 0u, hb = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t br = bright_bytes(word[j]);
          ha |= br & ma[j];
          hb |= br & mb[j];
        }
        if (ha) s_fl[f][fr][ta] = 1;
        if (hb) s_fl[f][fr][ta + 1] = 1;
      }
    };

    const int R = sl0.crop_y[v] + K.ext_oy[v] + er, C0 = sl0.crop_x[v] + K.ext_ox[v] + ec;
    if (mapped && (m.y & 3) != 0) {  // the source map holds this crop position: no calibration / background gathers
      run = (m.y & 3) == 1 ? 1 : -1;
      lo = m.x;
      inside = (unsigned)m.y >> 16;
      bw[0] = b4.x;
      bw[1] = b4.y;
      bw[2] = b4.z;
      bw[3] = b4.w;
#pragma unroll
      for (int f = 0; f < LM_INGEST_FB; ++f)
        if (f < nf) {
          uint32_t pw[4];
          run_bytes(d[f % PIPE], pw);
          if (f + PIPE < nf) frame_load(f + PIPE, lo, d[f % PIPE]);
          if (gray_on) emit(f, pw, slots[sb + f], R, C0, inside, std::true_type{});
          else emit(f, pw, sl0, R, C0, inside, std::false_type{});
        }
      continue;
    }
    run = ingest_locate(K, cal, bkg, R, C0, bw, lo, inside);
    if (same && run != 0) {
      // Every slot of the group has its crop at the same place and the pixels
      // are a run, but the source map does not hold it: the group's frame
      // loads are issued PIPE ahead of their use.
#pragma unroll
      for (int f = 0; f < PIPE; ++f)
        if (f < nf) frame_load(f, lo, d[f]);
#pragma unroll
      for (int f = 0; f < LM_INGEST_FB; ++f)
        if (f < nf) {
          uint32_t pw[4];
          run_bytes(d[f % PIPE], pw);
          if (f + PIPE < nf) frame_load(f + PIPE, lo, d[f % PIPE]);
          if (gray_on) emit(f, pw, slots[sb + f], R, C0, inside, std::true_type{});
          else emit(f, pw, sl0, R, C0, inside, std::false_type{});
        }
      continue;
    }
    // General case: frame by frame, the indices recomputed whenever the crop moves.
    int px = sl0.crop_x[v], py = sl0.crop_y[v];
    for (int f = 0; f < nf; ++f) {
      const int slot = sb + f;
      const LmSlot sl = slots[slot];
      const int Rf = sl.crop_y[v] + K.ext_oy[v] + er;
      const int Cf = sl.crop_x[v] + K.ext_ox[v] + ec;
      if (sl.crop_x[v] != px || sl.crop_y[v] != py) {  // crop moved: recompute the gather indices
        px = sl.crop_x[v];
        py = sl.crop_y[v];
        run = ingest_locate(K, cal, bkg, Rf, Cf, bw, lo, inside);
      }
      const lm_gu8* __restrict__ F = as_global(frame_ptr[slot]);
      uint32_t pw[4] = {0, 0, 0, 0};
      if (run != 0) {
        uint32_t d1[5];
        ingest_run_load(F, lo, d1);
        run_bytes(d1, pw);
      } else {
#pragma unroll
        for (int k = 0; k < LM_INGEST_VEC; ++k)
          if ((inside >> k) & 1u) pw[k >> 2] |= (uint32_t)F[ingest_index(K, cal, Rf, Cf + k)] << (8 * (k & 3));
      }
      if (gray_on) emit(f, pw, sl, Rf, Cf, inside, std::true_type{});
      else emit(f, pw, sl, Rf, Cf, inside, std::false_type{});
    }
  }
  ING_PROF(3)
  if (!fl_band || !tl_list) {
    if (pb && threadIdx.x == 0) {
      pb[4] = clock64();
      pb[15] = wall_clock64();
    }
  }
  if (!fl_band) return;
  // the band's flag bytes (each written by this block only: no zeroing pass)
  // and its bright tiles appended to the view's list (any order: the
  // correlation's waves take them LM_RW_NQ at a time, and the keys they
  // produce are sorted by k_nms)
  __syncthreads();
  for (int i = tid; i < nf * FPB * ftx; i += T) {
    const int f = i / (FPB * ftx), r = (i / ftx) % FPB, tx = i % ftx;
    const int ty = band * FPB + r;
    if (ty >= K.fl_ty[v]) continue;
    const int oh_t = min(LM_FH, K.fl_oh[v] - LM_FH * ty);
    const uint8_t b = s_fl[f][r][tx];
    flags[(int64_t)(sb + f) * K.fl_slot + K.fl_off[v] + ty * ftx + tx] = b;
    if (b && tl_list) {
      s_ent[atomicAdd(&s_n, 1)] = ((uint32_t)(sb + f) << 16) | (uint32_t)(ty * ftx + tx);
      atomicAdd(&s_outs, oh_t * min(LM_FW, K.fl_ow[v] - tx * LM_FW));
    }
  }
  if (!tl_list) return;
  __syncthreads();
  // this workgroup's list segment and its counter (tl_cnt: bright tiles of
  // view v at v LM_TL_NC + c, their outputs at (2 + v) LM_TL_NC + c)
  const int G = (int)gridDim.y, c = (int)blockIdx.y * LM_TL_NC / G;
  if (tid == 0) {
    s_base = s_n ? atomicAdd(&tl_cnt[v * LM_TL_NC + c], s_n) : 0;
    if (s_outs) atomicAdd(&tl_cnt[(2 + v) * LM_TL_NC + c], s_outs);
  }
  __syncthreads();
  uint32_t* __restrict__ out = tl_list + (int64_t)v * K.tl_stride +
                               (int64_t)lm_tl_y0(c, G) * LM_INGEST_FB * K.fl_tx[v] * K.fl_ty[v] + s_base;
  for (int p = tid; p < s_n; p += T) out[p] = s_ent[p];
  if (pb && threadIdx.x == 0) {
    pb[4] = clock64();
    pb[15] = wall_clock64();
  }
#undef ING_PROF
}

// ----------------------------------------------------------------- k_match
// A matched context's table per slot (lm_match_core.h, locomouse_match.h):
// the histogram of the slot's bottom box I_BOTTOM_MOUSE -- the pixels
// ipad_pixel returns, before any grey table -- then, on one lane, the CDF and
// the two loops of the table.  One workgroup of LM_MATCH_THREADS per slot with
// a normalisation table (the unprocessed slot 0 of a carry too: its frame is
// the halo, and the table equals what its own batch computed).
//
// The box is read in the 16-byte chunks of the bottom ext crop that cover it,
// as k_ingest reads them: where the lane's source map holds the slot's crop
// position, a chunk is its map entry, its 16 background bytes and five frame
// dwords (LM_MATCH_PIPE chunks' loads in flight per lane); elsewhere (a moving
// box, a gather chunk) the pixels come one by one through ipad_pixel.  The
// host has checked that the box lies inside I_UNPAD (lm_bp_check_match) and,
// at creation, inside the bottom ext crop (every point detector's centre tap
// reads it), so the chunk columns below are non-negative and inside the map.
//
// Counts: LM_MATCH_SUB sub-histograms in LDS, bin v of sub-histogram s at
// [v][s] (lanes that meet on one value spread over LM_MATCH_SUB banks), a lane
// adds a run of equal bytes of its chunk at once (a crop is mostly the
// background's 0), and the sub-histograms are summed once at the end.
#define LM_MATCH_THREADS 256
#define LM_MATCH_SUB 8
#define LM_MATCH_PIPE 4
__global__ __launch_bounds__(LM_MATCH_THREADS) void k_match(const LmConst* __restrict__ Kp,
                                                            const uint8_t* const* __restrict__ frame_ptr,
                                                            const uint8_t* __restrict__ bkg,
                                                            const int32_t* __restrict__ cal, uint8_t* __restrict__ luts,
                                                            const LmSlot* __restrict__ slots, int s0,
                                                            const int2* __restrict__ smap, const uint4* __restrict__ sbkg,
                                                            const int32_t* __restrict__ skey,
                                                            uint32_t* __restrict__ hist) {
  const LmConst& K = *Kp;
  const int slot = s0 + (int)blockIdx.x, tid = (int)threadIdx.x;
  __shared__ uint32_t s_h[256][LM_MATCH_SUB];
  __shared__ uint32_t s_cnt[256];
  __shared__ float s_c[256], s_ref[256];
  __shared__ uint8_t s_lut[256], s_T[256];
  const uint8_t* lut = luts + (int64_t)slot * 256;
  for (int i = tid; i < 256 * LM_MATCH_SUB; i += LM_MATCH_THREADS) (&s_h[0][0])[i] = 0u;
  for (int i = tid; i < 256; i += LM_MATCH_THREADS) {
    s_lut[i] = lut[i];
    s_ref[i] = K.match_ref[i];
  }
  const LmSlot sl = slots[slot];
  const bool mapped = skey[0] == sl.crop_x[0] && skey[1] == sl.crop_y[0];
  __syncthreads();
  const lm_gu8* __restrict__ F = as_global(frame_ptr[slot]);
  // the box in the bottom ext crop: rows ey0 .., byte columns [ex0, ex0 + bw)
  const int bw = K.bb_bottom_w, bh = K.bb_bottom_h, ew = K.ext_w[0];
  const int ey0 = K.unpad_y[0] - K.ext_oy[0], ex0 = K.unpad_x[0] - K.ext_ox[0];
  const int c_lo = ex0 / LM_INGEST_VEC, ncr = (ex0 + bw - 1) / LM_INGEST_VEC - c_lo + 1;  // chunks per row
  const int nchunk = bh * ncr;
  uint32_t* const my = &s_h[0][tid & (LM_MATCH_SUB - 1)];
  // one byte after another, equal neighbours counted together
  uint32_t run_v = 0u, run_n = 0u;
  auto count = [&](uint32_t v) {
    if (v != run_v && run_n) {
      atomicAdd(my + run_v * LM_MATCH_SUB, run_n);
      run_n = 0u;
    }
    run_v = v;
    ++run_n;
  };
  // chunk i of the box: its ext row and first byte column
  auto chunk_pos = [&](int i, int& er, int& ec) {
    const int rr = i / ncr;
    er = ey0 + rr;
    ec = (c_lo + i - rr * ncr) * LM_INGEST_VEC;
  };
  // the pixels of chunk (er, ec) inside the box, through ipad_pixel
  auto chunk_gather = [&](int er, int ec) {
    const int R = sl.crop_y[0] + K.ext_oy[0] + er, C0 = sl.crop_x[0] + K.ext_ox[0] + ec;
    for (int k = max(0, ex0 - ec); k < min(LM_INGEST_VEC, ex0 + bw - ec); ++k) count(ipad_pixel(F, bkg, cal, s_lut, K, R, C0 + k));
  };
  if (mapped) {
    for (int i0 = tid; i0 < nchunk; i0 += LM_MATCH_PIPE * LM_MATCH_THREADS) {
      int2 m[LM_MATCH_PIPE];
      uint4 b4[LM_MATCH_PIPE];
      uint32_t d[LM_MATCH_PIPE][5];
#pragma unroll
      for (int u = 0; u < LM_MATCH_PIPE; ++u) {  // the map entries ...
        const int i = i0 + u * LM_MATCH_THREADS;
        m[u] = make_int2(0, 0);
        b4[u] = make_uint4(0u, 0u, 0u, 0u);
        if (i < nchunk) {
          int er, ec;
          chunk_pos(i, er, ec);
          const int64_t ci = ((int64_t)er * ew + ec) / LM_INGEST_VEC;
          m[u] = smap[ci];
          b4[u] = sbkg[ci];
        }
      }
#pragma unroll
      for (int u = 0; u < LM_MATCH_PIPE; ++u) {  // ... then the frame dwords they point at
#pragma unroll
        for (int j = 0; j < 5; ++j) d[u][j] = 0u;
        if ((m[u].y & 3) != 0) ingest_run_load(F, m[u].x, d[u]);
      }
#pragma unroll
      for (int u = 0; u < LM_MATCH_PIPE; ++u) {
        const int i = i0 + u * LM_MATCH_THREADS;
        if (i >= nchunk) continue;
        int er, ec;
        chunk_pos(i, er, ec);
        if ((m[u].y & 3) == 0) {  // a gather chunk
          chunk_gather(er, ec);
          continue;
        }
        const unsigned sh = (unsigned)(m[u].x & 3);
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = __builtin_amdgcn_alignbyte(d[u][j + 1], d[u][j], sh);
        if ((m[u].y & 3) == 2) {  // a flipped run
          const uint32_t r0 = __builtin_bswap32(w[3]), r1 = __builtin_bswap32(w[2]), r2 = __builtin_bswap32(w[1]),
                         r3 = __builtin_bswap32(w[0]);
          w[0] = r0;
          w[1] = r1;
          w[2] = r2;
          w[3] = r3;
        }
        const uint32_t bwd[4] = {b4[u].x, b4[u].y, b4[u].z, b4[u].w};
        const int k0 = ex0 - ec, k1 = ex0 + bw - ec;  // the chunk's bytes [k0, k1) lie in the box
#pragma unroll
        for (int k = 0; k < LM_INGEST_VEC; ++k) {
          const uint32_t pk = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu, bk = (bwd[k >> 2] >> (8 * (k & 3))) & 0xFFu;
          if (k >= k0 && k < k1) count(s_lut[pk > bk ? pk - bk : 0u]);
        }
      }
    }
  } else {
    for (int i = tid; i < nchunk; i += LM_MATCH_THREADS) {
      int er, ec;
      chunk_pos(i, er, ec);
      chunk_gather(er, ec);
    }
  }
  if (run_n) atomicAdd(my + run_v * LM_MATCH_SUB, run_n);
  __syncthreads();
  if (tid < 256) {
    uint32_t n = 0u;
#pragma unroll
    for (int s = 0; s < LM_MATCH_SUB; ++s) n += s_h[tid][s];
    s_cnt[tid] = n;
    hist[(int64_t)slot * 256 + tid] = n;
  }
  __syncthreads();
  if (tid == 0) {  // serial by definition: a float sum in index order, cur carried across i
    lm_match_cdf_of(s_cnt, K.match_scale, s_c);
    lm_match_table(s_c, s_ref, s_T);
  }
  __syncthreads();
  if (tid < 256) luts[(int64_t)slot * 256 + K.match_off + tid] = s_T[tid];
}

// lm_debug_match_crop (debug bit 1): the bottom box of every frame f of the
// batch as its steps see it, through ipad_pixel_t: image 2 f the current image
// (slot f + 1), image 2 f + 1 I_PREV_PAD at the same position (slot f, with
// its own table inside its own box; zeros where there is no such slot).
__global__ __launch_bounds__(256) void k_match_crop(const LmConst* __restrict__ Kp,
                                                    const uint8_t* const* __restrict__ frame_ptr,
                                                    const uint8_t* __restrict__ bkg, const int32_t* __restrict__ cal,
                                                    const uint8_t* __restrict__ luts, const LmSlot* __restrict__ slots,
                                                    int s_lut0, uint8_t* __restrict__ out) {
  const LmConst& K = *Kp;
  const int n = K.bb_bottom_w * K.bb_bottom_h;
  const int scur = (int)blockIdx.y + 1, prev = (int)blockIdx.z, sread = scur - prev;
  uint8_t* __restrict__ o = out + (int64_t)(2 * (int)blockIdx.y + prev) * n;
  const LmSlot sc = slots[scur];
  if (sread < s_lut0) {
    for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < n; p += (int)(gridDim.x * blockDim.x)) o[p] = 0;
    return;
  }
  const LmSlot sr = slots[sread];
  const lm_gu8* __restrict__ F = as_global(frame_ptr[sread]);
  for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < n; p += (int)(gridDim.x * blockDim.x)) {
    const int y = p / K.bb_bottom_w, x = p - y * K.bb_bottom_w;
    o[p] = ipad_pixel_t(F, bkg, cal, luts + (int64_t)sread * 256, K, sr, sc.crop_y[0] + K.unpad_y[0] + y,
                        sc.crop_x[0] + K.unpad_x[0] + x);
  }
}

// ------------------------------------------------------------ k_tile_bound
// The tiles of a view's three detectors that the correlation has to compute.
// The pipeline uses only the sign of a tail score (k_ingest has zeroed the
// tail bitmaps) and of a point score only whether it is > 0 under a bright
// mask pixel (corr_epilogue), so a LM_FW x LM_FH tile whose scores are all
// provably < 0 (lm_tail_bound.h: an upper bound from per-row pixel ranges,
// with the fp32 chain's rounding error added) is left out.  One workgroup per
// (slot, view): the view's ext crop is read once and reduced to pixel ranges
// per row and aligned block of 8 columns; from those, per detector (paw,
// snout, tail: each with its own window origin, column spans and constants),
// ranges per window row and tile column, then the bound per tile -- of a
// point detector only for the tiles k_ingest flagged bright; a dark tile
// stays unlisted without evaluation.  The tiles to compute are flagged (one
// byte each, for k_corr_gen) and appended to the detector's own list segments
// (for the ring kernels), in k_ingest's entry format and segment scheme.  A
// detector without a usable bound (tb_skip = 0: rho <= 0, non-finite weights,
// ranges beyond the LDS) lists every tile (a point detector: every bright
// tile).  tt_cnt / pt_cnt null: the tail / point detectors are not handled
// here (LM_CORR_TAILSKIP=0 / LM_CORR_POINTSKIP=0).
// A tile the tile bound fails is tried once more per 8-column output block and
// group of 8 taps (LmConst::tbr_on, lm_tail_bound.h: lm_tbr_*), from the same
// block ranges, and left out when every block of it is proven
// (LM_TILE_REFINE=0: the tile bound alone).
//
// k_tile_bound_ref is the first form of the pre-pass (LM_TILE_BOUND_REF=1):
// it reads the crops themselves and reduces a whole view per workgroup.  It is
// kept as the reference that k_tile_bound (below) is tested against.
// (LM_TB_THREADS, LM_TBW_TILES, LM_TBW_ROW_LOOP: lm_tile_plan.h, which plans both kernels' LDS)
#ifndef LM_TBW_LD
#define LM_TBW_LD 8  // k_tile_bound: a thread's loads of block ranges in flight
#endif
#ifndef LM_TBW_CV
#define LM_TBW_CV 8  // k_tile_bound: words of the pair table a thread forms between two barriers
#endif
#ifndef LM_TBW_CR
#define LM_TBW_CR 2  // k_tile_bound: entries a thread holds while the refined entries close up
#endif
__global__ __launch_bounds__(LM_TB_THREADS) void k_tile_bound_ref(
    const LmConst* __restrict__ Kp, const uint8_t* __restrict__ ext, int64_t ext_slot_bytes, int s0,
    const double* __restrict__ tbc, const uint8_t* __restrict__ bright, uint8_t* __restrict__ tail_flags,
    int32_t* __restrict__ tt_cnt, uint32_t* __restrict__ tt_list, uint8_t* __restrict__ pt_flags,
    int32_t* __restrict__ pt_cnt, uint32_t* __restrict__ pt_list) {
  const LmConst& K = *Kp;
  extern __shared__ uint8_t tb_lds[];
  __shared__ int s_n[3], s_b[3], s_k[3], s_base[3];
  const int v = (int)blockIdx.y, slot = s0 + (int)blockIdx.x;
  const int T = (int)blockDim.x, tid = (int)threadIdx.x;
  const int ew = K.ext_w[v], eh = K.ext_h[v], nbw = ew / LM_TB_BLK;  // (ext rows are multiples of 16 bytes)
  uint8_t* bmax = tb_lds;
  uint8_t* bmin = bmax + eh * nbw;
  if (tid < 3) {
    s_n[tid] = 0;
    s_b[tid] = 0;
    s_k[tid] = 0;
  }
  // the view's detectors (paw, snout, tail: ids 3 v + k): on = its tiles are
  // listed here, use = with the bound; the ext rows and blocks their windows span
  static_assert(DET_PAW_S == 3 && DET_TAIL_B == 2 && DET_TAIL_S == 5, "three detectors per view, the tail last");
  bool on[3], use[3];
  int y_lo = eh, y_hi = 0, b_lo = nbw, b_hi = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const LmDet& D = K.det[3 * v + k];
    on[k] = D.kind != 0 ? tt_cnt != nullptr : pt_cnt != nullptr;
    use[k] = on[k] && K.tb_skip[3 * v + k] != 0;
    if (use[k]) {  // (the host accepts a bound only when the window lies inside the ext crop)
      y_lo = min(y_lo, D.in_y);
      y_hi = max(y_hi, D.in_y + D.oh + D.kh - 1);
      b_lo = min(b_lo, D.in_x / LM_TB_BLK);
      b_hi = max(b_hi, (D.in_x + D.ow + D.kw - 1 + LM_TB_BLK - 1) / LM_TB_BLK);
    }
  }
  y_hi = min(y_hi, eh);
  b_hi = min(b_hi, nbw);
  if (y_lo < y_hi && b_lo < b_hi) {
    const uint8_t* __restrict__ vsrc =
        ext + (int64_t)slot * ext_slot_bytes + (v ? (int64_t)K.ext_h[0] * K.ext_w[0] : 0);
    static_assert(LM_TB_BLK == 8, "one 8-byte load per block");
    // ranges per (ext row, aligned block of 8 columns): every byte of the
    // view read once, for all of its detectors
    // (batching eight of a thread's loads before their use changed nothing for
    // the tail detectors' pass: 175 vs 178 us per launch among eight contexts'
    // kernels, profiles/tailskip/)
    const int nb = b_hi - b_lo, ne = (y_hi - y_lo) * nb;
    for (int e = tid; e < ne; e += T) {
      const int r = y_lo + e / nb, b = b_lo + e % nb;
      const uint2 p = *reinterpret_cast<const uint2*>(vsrc + (int64_t)r * ew + LM_TB_BLK * b);
      unsigned mx = 0u, mn = 255u;
#pragma unroll
      for (int j = 0; j < LM_TB_BLK; ++j) {
        const unsigned q = ((j < 4 ? p.x : p.y) >> (8 * (j & 3))) & 0xFFu;
        mx = max(mx, q);
        mn = min(mn, q);
      }
      bmax[r * nbw + b] = (uint8_t)mx;
      bmin[r * nbw + b] = (uint8_t)mn;
    }
  }
  __syncthreads();
  // ranges per (detector, window row, tile column): the blocks that cover
  // lm_tb_span's columns of the detector's window
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!use[k]) continue;
    const LmDet& D = K.det[3 * v + k];
    const int ftx = D.kind != 0 ? K.tt_tx[v] : K.fl_tx[v], rows = D.oh + D.kh - 1;
    uint8_t* rmax = tb_lds + K.tb_rng[3 * v + k];
    uint8_t* rmin = rmax + rows * ftx;
    for (int e = tid; e < rows * ftx; e += T) {
      const int r = e / ftx, tx = e - r * ftx;
      int c0, c1, b0, b1;
      lm_tb_span(tx, D.kw, D.ow, &c0, &c1);
      lm_tb_blocks(D.in_x, c0, c1, &b0, &b1);
      unsigned mx = 0u, mn = 255u;
      for (int b = b0; b < b1; ++b) {
        mx = max(mx, (unsigned)bmax[(D.in_y + r) * nbw + b]);
        mn = min(mn, (unsigned)bmin[(D.in_y + r) * nbw + b]);
      }
      rmax[e] = (uint8_t)mx;
      rmin[e] = (uint8_t)mn;
    }
  }
  __syncthreads();
  // the flags: a tail tile unless proven, a point tile when k_ingest flagged
  // it bright and it is not proven
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!on[k]) continue;
    const int d = 3 * v + k;
    const LmDet& D = K.det[d];
    const bool tail = D.kind != 0;
    const int ftx = tail ? K.tt_tx[v] : K.fl_tx[v], ntile = ftx * (tail ? K.tt_ty[v] : K.fl_ty[v]);
    uint8_t* __restrict__ fl = tail ? tail_flags + (int64_t)slot * K.tt_slot + K.tt_off[v]
                                    : pt_flags + (D.list & 1) * K.pt_plane + (int64_t)slot * K.fl_slot + K.fl_off[v];
    const uint8_t* __restrict__ br = tail ? nullptr : bright + (int64_t)slot * K.fl_slot + K.fl_off[v];
    const uint8_t* rmax = tb_lds + K.tb_rng[d];
    const uint8_t* rmin = rmax + (D.oh + D.kh - 1) * ftx;
    const double* __restrict__ P = tbc + K.tb_off[d];
    int mine = 0, mbr = 0;
    for (int i = tid; i < ntile; i += T) {
      bool keep = br ? br[i] != 0 : true;
      mbr += br && keep ? 1 : 0;
      if (keep && use[k])
        keep = !lm_tb_tile_skip(rmax, rmin, ftx, D.oh, D.kh, i / ftx, i % ftx, P, P + D.kh, K.tb_bias[d]);
      if (keep && use[k] && K.tbr_on[d] != 0)  // the refinement, block by block at the final height (no shortcut)
        keep = !lm_tbr_tile_skip(bmax, bmin, nbw, D.in_y, D.in_x, D.oh, D.ow, D.kh, D.kw, i / ftx, i % ftx,
                                 tbc + K.tbr_off[d], K.tb_bias[d], LM_TB_RH, false);
      fl[i] = keep ? 1 : 0;
      mine += keep ? 1 : 0;
    }
    if (mine) atomicAdd(&s_n[k], mine);
    if (mbr) atomicAdd(&s_b[k], mbr);
  }
  __syncthreads();
  // this workgroup's list segments and their counters, as in k_ingest (a
  // point detector's bright tiles counted next to its listed ones)
  const int G = ((int)gridDim.x + LM_INGEST_FB - 1) / LM_INGEST_FB;
  const int c = ((int)blockIdx.x / LM_INGEST_FB) * LM_TL_NC / G;
  if (tid < 3 && (K.det[3 * v + tid].kind != 0 ? tt_cnt != nullptr : pt_cnt != nullptr)) {
    const LmDet& D = K.det[3 * v + tid];
    int32_t* __restrict__ cnt = D.kind != 0 ? tt_cnt + v * LM_TL_NC : pt_cnt + D.list * LM_TL_NC;
    s_base[tid] = s_n[tid] ? atomicAdd(&cnt[c], s_n[tid]) : 0;
    if (D.kind == 0 && s_b[tid]) atomicAdd(&pt_cnt[(LM_NLIST + D.list) * LM_TL_NC + c], s_b[tid]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!on[k]) continue;
    const LmDet& D = K.det[3 * v + k];
    const bool tail = D.kind != 0;
    const int ntile = tail ? K.tt_tx[v] * K.tt_ty[v] : K.fl_tx[v] * K.fl_ty[v];
    const uint8_t* __restrict__ fl = tail ? tail_flags + (int64_t)slot * K.tt_slot + K.tt_off[v]
                                          : pt_flags + (D.list & 1) * K.pt_plane + (int64_t)slot * K.fl_slot + K.fl_off[v];
    uint32_t* __restrict__ out =
        (tail ? tt_list + (int64_t)v * K.tt_stride : pt_list + (int64_t)D.list * K.tl_stride) +
        (int64_t)lm_tl_y0(c, G) * LM_INGEST_FB * ntile + s_base[k];
    for (int i = tid; i < ntile; i += T)  // (each thread re-reads the flags it wrote)
      if (fl[i]) out[atomicAdd(&s_k[k], 1)] = ((uint32_t)slot << 16) | (uint32_t)i;
  }
}

// The pre-pass the pipeline runs.  It computes what k_tile_bound_ref computes
// (the same flags, counters and sets of list entries) from k_ingest's block
// ranges (rng: per slot and 16-byte chunk of the ext crops, largest | smallest
// byte of each aligned half, block_range) instead of the crops, a quarter of
// their bytes.  One workgroup per (slot, view, band of LmConst::tbw_br tile
// rows): about a workgroup's threads of tiles over the view's detectors, and a
// few KB of LDS, so that many workgroups share a compute unit.
//   1. The bright point tiles and all tail tiles of the band are compacted
//      into a work list (a dark point tile is flagged 0 and costs nothing
//      more); the band's block ranges are loaded, several loads per thread in
//      flight.
//   2. Their four-row windows: the rows a tile's outputs read at one weight
//      row, the same for all of the view's detectors.
//   3. Per detector the window table of lm_tail_bound.h: entry (window row,
//      tile column) is the range over the column's blocks (lm_tb_span,
//      lm_tb_blocks) of the four-row windows -- of the block ranges themselves
//      for the rows of a last tile row of fewer than four output rows.
//   4. lm_tb_tile_skip_win per listed tile: kh pairs of bytes, the work list
//      handed out densely.  Kept tiles take their place in the band's entries
//      by a ballot and one LDS atomic per wave.
//   4b. The refinement of the kept tiles: one pass over the (tile, output
//      block) items of all three detectors, in wave-sized chunks of one
//      detector each, the terms read from the pair table that the four-row
//      windows are turned into after step 3 (3b: entry b is the range over
//      blocks b and b + 1, which is what a term reads; see there), by a loop
//      without chunk stepping where the detectors' weight rows are one chunk
//      of constants each (at most four tap groups: all of C3's; ROWS below),
//      and there in fp32 first (lm_tbs_*: one packed FMA per term; only a lane
//      whose fp32 sum lies within its proven margin of zero takes the double
//      loop, and tbs_fallback counts those lanes; LM_TILE_SCREEN=0 or a
//      detector the screen's gate refuses: the double loop alone).  An
//      unproven block marks its entry.
//   Without the narrow class (NARROW false):
//   4c. One compaction drops the entries of proven tiles from all three
//      segments.
//   5. One global atomic per (workgroup, detector) on the slot group's segment
//      counter (the segment index comes from the slot and the batch's slot
//      count nslot, so all bands of a slot append to one segment), then the
//      entries are copied out.
//   With it (NARROW true) nothing follows 4b's barrier but
//   5w. one wave per detector of the view (the fourth leaves): it reads the
//      detector's entries and marks where 4b left them, 64 at a time, writes
//      a refined tile's flag, counts the kept entries per class by ballots,
//      takes its places in the wide and the narrow list of the slot group's
//      segment and adds to the listed and bright counters (one lane, the
//      atomics back to back), then writes each kept entry once, straight from
//      LDS to its list.  Nothing is closed up and the existing lists (pt_list,
//      tt_list) are not written: with the class on nothing reads them.
// No index of a loop is divided at run time (lm_div by reciprocals).
DEV uint32_t range_merge(uint32_t a, uint32_t b) { return lm_tb_range_merge(a, b); }  // of two words of block ranges
// The place of each lane with p set in the sequence counted by *ctr (LDS): one
// atomic per wave.  To be called by whole waves.
DEV int wave_append(bool p, int* ctr) {
  const unsigned long long m = __ballot(p);
  if (m == 0ull) return 0;
  const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  int base = 0;
  if (p && rank == 0) base = atomicAdd(ctr, (int)__popcll(m));
  return __shfl(base, __ffsll((long long)m) - 1) + rank;
}
#ifndef LM_TBW_WPE
#define LM_TBW_WPE 8  // amdgpu_waves_per_eu minimum: <= 64 VGPRs, eight workgroups per compute unit
#endif
// ROWS: step 4b sums the detectors of one chunk of constants per weight row
// with lm_tbr_sum_rows_n (the others, and every detector of ROWS false, with
// lm_tbr_sum).  The host launches ROWS true only where a refined detector is
// such a one (lm_ctx::tbw_row_loop: all of C3's); elsewhere (C5) the kernel
// holds the generic loop alone, instruction for instruction as it was compiled
// before the row loops existed (with them next to it C5 lost 1.2 %; DESIGN.md
// section 12).
// TBW_SEL: detector k's member of one of the kernel's per-detector arrays,
// chosen among the three uniform values, not loaded per lane.
#define TBW_SEL(a) (k == 0 ? a[0] : k == 1 ? a[1] : a[2])
// NARROW (LM_CORR_NARROW, lm_corr_narrow.h): step 4b marks an entry with the
// mask of its unproven blocks instead of 0 / 1, and step 5w appends every kept
// entry to one of two lists of its detector, which the ring kernels read in
// place of the existing ones: narrow (the unproven blocks span at most two:
// the entry with the span's first block and length) or wide (every other, as
// in the existing list; all of a detector that is not refined or has
// LmConst::nw_on 0).  The existing flags and counters are written as without
// it; the existing lists are not written (nwo is set: the host launches NARROW
// only with the class's lists).  Within a workgroup a detector's entries of
// one class stand in entry order; every reader takes them in any order.
template <bool ROWS, bool NARROW>
__global__ __launch_bounds__(LM_TB_THREADS) __attribute__((amdgpu_waves_per_eu(LM_TBW_WPE, 8))) void k_tile_bound(
    const LmConst* __restrict__ Kp, const uint32_t* __restrict__ rng, int64_t rng_slot, int s0, int nslot,
    const double* __restrict__ tbc, const uint8_t* __restrict__ bright, uint8_t* __restrict__ tail_flags,
    int32_t* __restrict__ tt_cnt, uint32_t* __restrict__ tt_list, uint8_t* __restrict__ pt_flags,
    int32_t* __restrict__ pt_cnt, uint32_t* __restrict__ pt_list, unsigned long long* __restrict__ tbs_fallback,
    const LmNarrowOut nwo) {
  const LmConst& K = *Kp;
  extern __shared__ __attribute__((aligned(16))) uint8_t tbw_lds[];
  __shared__ int s_n[3], s_b[3], s_m[3], s_base[3], s_nw;  // (s_m, s_base: NARROW false only)
  const int v = (int)blockIdx.y < K.tbw_nband[0] ? 0 : 1;
  const int band = (int)blockIdx.y - (v ? K.tbw_nband[0] : 0);
  const int slot = s0 + (int)blockIdx.x;
  const int T = (int)blockDim.x, tid = (int)threadIdx.x;
  if (tid < 3) {
    s_n[tid] = 0;
    s_b[tid] = 0;
    if (!NARROW) s_m[tid] = 0;
  }
  if (tid == 0) s_nw = 0;
  // the view's detectors (paw, snout, tail: ids 3 v + k) in this band: on =
  // its tiles are listed here, use = with the bound; t0, nt: its first tile
  // row and tile count, ohb: its output rows; y_lo .. y_hi: the ext rows the
  // windows of the detectors with a bound span
  bool on[3], use[3], refine[3], tail[3];
  int t0[3], nt[3], ohb[3], ftx[3], tbase[3];
  uint8_t* fl[3];
  int y_lo = K.ext_h[v], y_hi = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int d = 3 * v + k;
    const LmDet& D = K.det[d];
    tail[k] = D.kind != 0;
    on[k] = tail[k] ? tt_cnt != nullptr : pt_cnt != nullptr;
    use[k] = on[k] && K.tbw_use[d] != 0;
    ftx[k] = tail[k] ? K.tt_tx[v] : K.fl_tx[v];
    int nty;
    ohb[k] = lm_tbw_band(D, tail[k] ? K.tt_ty[v] : K.fl_ty[v], K.tbw_br[v], band, &t0[k], &nty);
    nt[k] = on[k] ? nty * ftx[k] : 0;
    tbase[k] = t0[k] * ftx[k];  // the band's first tile of the detector's grid
    fl[k] = tail[k] ? tail_flags + (int64_t)slot * K.tt_slot + K.tt_off[v]
                    : pt_flags + (D.list & 1) * K.pt_plane + (int64_t)slot * K.fl_slot + K.fl_off[v];
    use[k] = use[k] && nt[k] > 0;
    refine[k] = use[k] && K.tbr_on[d] != 0;
    if (use[k]) {  // (the host accepts a bound only when the window lies inside the ext crop)
      y_lo = min(y_lo, D.in_y + LM_FH * t0[k]);
      y_hi = max(y_hi, D.in_y + LM_FH * t0[k] + ohb[k] + D.kh - 1);
    }
  }
  y_hi = min(y_hi, K.ext_h[v]);
  const int nrow = max(0, min(y_hi - y_lo, K.tbw_rows[v]));
  const int nbk = K.tbw_nbk[v], nw = nbk / 2;  // blocks and words (of two blocks) per row
  uint32_t* B = reinterpret_cast<uint32_t*>(tbw_lds);
  uint32_t* V = reinterpret_cast<uint32_t*>(tbw_lds + K.tbw_v[v]);
  uint32_t* work = reinterpret_cast<uint32_t*>(tbw_lds + K.tbw_work[v]);
  __syncthreads();
  // The band's block ranges: LM_TBW_LD loads per thread in flight, the first
  // round issued before the work list is built (whose loads of the bright
  // flags then wait alongside them), P_i and N_i likewise.
  constexpr int LD = LM_TBW_LD;
  const int ne = nrow * nw, ewq = K.ext_w[v] / LM_INGEST_VEC;
  const uint32_t rc = lm_rcp(max(nw, 1));
  const uint32_t* __restrict__ src = rng + (int64_t)slot * rng_slot +
                                     (v ? (int64_t)K.ext_h[0] * K.ext_w[0] / LM_INGEST_VEC : 0) +
                                     (int64_t)min(y_lo, y_hi) * ewq + K.tbw_blo[v] / 2;
  uint32_t w[LD];
  auto rng_load = [&](int e0) {
#pragma unroll
    for (int u = 0; u < LD; ++u) {
      const int e = e0 + u * T + tid;
      if (e < ne) {
        const int r = lm_div(e, rc);
        w[u] = src[r * ewq + (e - r * nw)];
      }
    }
  };
  auto rng_store = [&](int e0) {
#pragma unroll
    for (int u = 0; u < LD; ++u) {
      const int e = e0 + u * T + tid;
      if (e < ne) B[e] = w[u];
    }
  };
  rng_load(0);
  double pnv[3] = {0.0, 0.0, 0.0};  // (a detector has at most T / 2 rows: the host checks)
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (use[k] && tid < 2 * K.det[3 * v + k].kh) pnv[k] = tbc[K.tb_off[3 * v + k] + tid];
  // 1. the work list: tile j of the band of detector k as k << 28 | j
  const uint8_t* __restrict__ br = bright + (int64_t)slot * K.fl_slot + K.fl_off[v];
  const int ntot = nt[0] + nt[1] + nt[2];
  for (int i0 = 0; i0 < ntot; i0 += T) {
    const int i = i0 + tid;
    const bool act = i < ntot;
    const int k = i < nt[0] ? 0 : i < nt[0] + nt[1] ? 1 : 2;
    const int j = i - (k == 0 ? 0 : k == 1 ? nt[0] : nt[0] + nt[1]);
    const bool tl = k == 0 ? tail[0] : k == 1 ? tail[1] : tail[2];
    const int tb = k == 0 ? tbase[0] : k == 1 ? tbase[1] : tbase[2];
    bool cand = act;
    if (act && !tl) {
      cand = br[tb + j] != 0;
      if (!cand) (k == 0 ? fl[0] : k == 1 ? fl[1] : fl[2])[tb + j] = 0;
    }
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {  // a point detector's bright tiles, counted next to its listed ones
      const unsigned long long m = __ballot(cand && !tl && k == kk);
      if (m != 0ull && (tid & 63) == 0) atomicAdd(&s_b[kk], (int)__popcll(m));
    }
    const int pos = wave_append(cand, &s_nw);
    if (cand) work[pos] = (uint32_t)k << 28 | (uint32_t)j;
  }
  rng_store(0);
  for (int e0 = LD * T; e0 < ne; e0 += LD * T) {
    rng_load(e0);
    rng_store(e0);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (use[k] && tid < 2 * K.det[3 * v + k].kh) reinterpret_cast<double*>(tbw_lds + K.tbw_pn[3 * v + k])[tid] = pnv[k];
  __syncthreads();
  // 2. four-row windows of the block ranges
  for (int e = tid; e < (nrow - (LM_TB_H - 1)) * nw; e += T)
    V[e] = range_merge(range_merge(B[e], B[e + nw]), range_merge(B[e + 2 * nw], B[e + 3 * nw]));
  static_assert(LM_TB_H == 4, "four-row windows");
  __syncthreads();
  // 3. the detectors' window tables
  const uint16_t* B16 = reinterpret_cast<const uint16_t*>(B);
  const uint16_t* V16 = reinterpret_cast<const uint16_t*>(V);
  // (and, for the refinement, per detector the windows' entries at the last
  // block of its window, which a term there reads alone: the windows
  // themselves become their pair table below)
  uint16_t* AL = reinterpret_cast<uint16_t*>(tbw_lds + K.tbw_al[v]);
  const int nvr = max(nrow - (LM_TB_H - 1), 0), als = K.tbw_rows[v];  // window rows; the stride of a detector's entries
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!refine[k]) continue;
    const LmDet& D = K.det[3 * v + k];
    const int bl = lm_tbr_block_end(D.in_x, D.ow, D.kw, K.ext_w[v] / LM_TB_BLK) - K.tbw_blo[v] - 1;
    for (int r = tid; r < nvr; r += T) AL[k * als + r] = V16[r * nbk + bl];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!use[k]) continue;
    const int d = 3 * v + k;
    const LmDet& D = K.det[d];
    uint8_t* wmax = tbw_lds + K.tbw_win[d];
    uint8_t* wmin = wmax + K.tbw_wsz[d];
    const int nent = min(lm_tb_win_rows(ohb[k], D.kh) * ftx[k], K.tbw_wsz[d]);
    const uint32_t rc = K.tbw_inv[d];
    const int yb = D.in_y + LM_FH * t0[k] - y_lo;  // the band's window row 0 among the loaded rows
    for (int e = tid; e < nent; e += T) {
      const int w = lm_div(e, rc), tx = e - w * ftx[k];
      int r0, nr, c0, c1, b0, b1;
      lm_tb_win_src(ohb[k], D.kh, w, &r0, &nr);
      lm_tb_span(tx, D.kw, D.ow, &c0, &c1);
      lm_tb_blocks(D.in_x, c0, c1, &b0, &b1);
      b0 = max(b0 - K.tbw_blo[v], 0);
      b1 = min(b1 - K.tbw_blo[v], nbk);
      const uint16_t* row = (nr == LM_TB_H ? V16 : B16) + (yb + r0) * nbk;
      const int nrr = nr == LM_TB_H ? 1 : nr;
      unsigned mx = 0u, mn = 255u;
      for (int r = 0; r < nrr; ++r, row += nbk)
        for (int b = b0; b < b1; ++b) {
          const unsigned q = row[b];
          mx = max(mx, q & 0xFFu);
          mn = min(mn, q >> 8);
        }
      wmax[e] = (uint8_t)mx;
      wmin[e] = (uint8_t)mn;
    }
  }
  __syncthreads();
  // 3b. the windows become their pair table in place (entry b: the range over
  // blocks b and b + 1, lm_tbr_pair_word: what a term of the refinement
  // reads): a group of words is formed in registers, then written (a word
  // needs its right neighbour as it was; a later group's words are not written
  // before its own barrier).  Nothing reads the windows between here and 4b.
  if (refine[0] || refine[1] || refine[2]) {
    constexpr int CV = LM_TBW_CV;
    const int nv = nvr * nw;
    for (int e0 = 0; e0 < nv; e0 += CV * T) {
      uint32_t pv[CV];
#pragma unroll
      for (int u = 0; u < CV; ++u) {
        const int e = e0 + u * T + tid;
        if (e < nv) {
          const int r = lm_div(e, rc);
          const bool last = e - r * nw == nw - 1;
          pv[u] = lm_tbr_pair_word(V[e], last ? 0u : V[e + 1], last);
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < CV; ++u) {
        const int e = e0 + u * T + tid;
        if (e < nv) V[e] = pv[u];
      }
    }
  }
  // 4. the bound per tile of the work list
  int kh3[3], win3[3], wsz3[3], pn3[3];
  uint32_t inv3[3];
  double bias3[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int d = 3 * v + k;
    kh3[k] = K.det[d].kh;
    win3[k] = K.tbw_win[d];
    wsz3[k] = K.tbw_wsz[d];
    pn3[k] = K.tbw_pn[d];
    inv3[k] = K.tbw_inv[d];
    bias3[k] = K.tb_bias[d];
  }
  const int nwork = s_nw;
  for (int w0 = 0; w0 < nwork; w0 += T) {
    const bool act = w0 + tid < nwork;
    const uint32_t item = act ? work[w0 + tid] : 0u;
    const int k = (int)(item >> 28), j = (int)(item & 0x0FFFFFFFu);
    const int tb = TBW_SEL(tbase);
    bool keep = act;
    if (act && TBW_SEL(use)) {
      const int fx = TBW_SEL(ftx), kh = TBW_SEL(kh3);
      const int ty = lm_div(j, TBW_SEL(inv3)), tx = j - ty * fx;
      const uint8_t* wmax = tbw_lds + TBW_SEL(win3);
      const double* pn = reinterpret_cast<const double*>(tbw_lds + TBW_SEL(pn3));
      keep = !lm_tb_tile_skip_win(wmax, wmax + TBW_SEL(wsz3), fx, kh, lm_tb_win_row0(TBW_SEL(ohb), kh, ty), tx, pn,
                                  pn + kh, TBW_SEL(bias3));
    }
    // (a tile that goes on to the refinement gets its flag there)
    if (act && !(keep && TBW_SEL(refine))) TBW_SEL(fl)[tb + j] = keep ? 1 : 0;
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {
      const bool mine = act && keep && k == kk;
      const int pos = wave_append(mine, &s_n[kk]);
      if (mine) reinterpret_cast<uint32_t*>(tbw_lds + K.tbw_ent[3 * v + kk])[pos] = ((uint32_t)slot << 16) | (uint32_t)(tb + j);
    }
  }
  __syncthreads();
  // 4b. the refinement of the tiles the tile bound failed, which now stand in
  // the band's entries: one pass over the (tile, output block) items of all
  // three detectors.  A detector's items are cut into chunks of a wave's lanes
  // and the chunks of all detectors are handed to the waves in turn, so the
  // lanes are dense and the detector is uniform in a wave: kh, the group count
  // and the constants (scalar loads of tbc, a 64-byte chunk of four groups at
  // a time, the next chunk fetched while this one is summed) stay scalar.  A
  // block is tried over the tile's four rows first: a term reads one entry of
  // the windows' pair table (V since 3b), a chunk's four entries as three words, the
  // next chunk's words fetched before this chunk's terms are summed (after the
  // last chunk: the row below, which the table's spare row covers); at the
  // block the detector's window ends in, the term reads V (that block alone).  Then row by row (B)
  // at LM_TB_RH 1 (or over the rows of a short last tile row), the pairs formed
  // from B.  A tile with a block that stays unproven is marked and keeps its
  // entry, the others get flag 0 and their entries are dropped (NARROW false:
  // the entries of each detector close up; NARROW true: step 5w skips them).
  // With ROWS a detector of one chunk per row takes lm_tbr_sum_rows_n, the same
  // terms in the same order with the group count a constant: no chunk counter,
  // no guard per term, a fixed step of nw words to the next row's entries, and
  // the select of the alone entry only at the row's last term.
  uint32_t* mark = work;  // (the work list is done with; one word per entry, the detectors' one after the other)
  int nr3[3], ent3[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    nr3[k] = refine[k] ? __builtin_amdgcn_readfirstlane(s_n[k]) : 0;
    ent3[k] = K.tbw_ent[3 * v + k];
  }
  const int nref = nr3[0] + nr3[1] + nr3[2];
  if (nref > 0) {
    for (int t = tid; t < nref; t += T) mark[t] = 0u;
    __syncthreads();
    constexpr int WV = 64;  // lanes of a wave
    const int c1 = (nr3[0] * LM_TB_NBX + WV - 1) / WV, c2 = c1 + (nr3[1] * LM_TB_NBX + WV - 1) / WV,
              c3 = c2 + (nr3[2] * LM_TB_NBX + WV - 1) / WV;
    const uint32_t rcx = lm_rcp(LM_TB_NBX);
    for (int ch = __builtin_amdgcn_readfirstlane(tid / WV); ch < c3; ch += T / WV) {
      const int k = ch < c1 ? 0 : ch < c2 ? 1 : 2;  // (uniform)
      const int d = 3 * v + k;
      const LmDet& D = K.det[d];
      const int n = TBW_SEL(nr3), fx = TBW_SEL(ftx), tk0 = TBW_SEL(t0), ohk = TBW_SEL(ohb);
      const int e = (ch - (k == 0 ? 0 : k == 1 ? c1 : c2)) * WV + (tid & (WV - 1));
      const int mb = k == 0 ? 0 : k == 1 ? nr3[0] : nr3[0] + nr3[1];
      const uint32_t* ent = reinterpret_cast<const uint32_t*>(tbw_lds + K.tbw_ent[d]);
      const int kh = D.kh, ng = K.tbr_ng[d], nc = lm_tbr_chunks(ng);
      const double* __restrict__ C = tbc + K.tbr_off[d];
      const double bias = K.tb_bias[d];
      const float* __restrict__ Cf = reinterpret_cast<const float*>(tbc + K.tbs_off[d]);  // (the screen's rows)
      const int yb = D.in_y + LM_FH * tk0 - y_lo;  // the band's window row 0 among the loaded rows
      const int bl0 = lm_tbr_block0(D.in_x, 0) - K.tbw_blo[v];
      const int bendl = lm_tbr_block_end(D.in_x, D.ow, D.kw, K.ext_w[v] / LM_TB_BLK) - K.tbw_blo[v];
      const int nbx = (D.ow + LM_TB_BLK - 1) / LM_TB_BLK;
      if (e >= n * LM_TB_NBX) continue;
      const int t = lm_div(e, rcx);
      const int tile = (int)(ent[t] & 0xFFFFu);
      const int ty = lm_div(tile, K.tbw_inv[d]), tx = tile - ty * fx;
      const int xb = tx * LM_TB_NBX + (e - t * LM_TB_NBX);
      if (xb >= nbx) continue;  // (a last tile column of fewer blocks)
      const int tyb = ty - tk0;
      const int nr = min(LM_TB_H, ohk - LM_TB_H * tyb);
      const int row0 = yb + LM_TB_H * tyb, ba0 = bl0 + xb;
      // the tile's four rows at once from the pair table of their windows
      // (rows > 0: a detector of one chunk per row and `rows` tap groups, lm_tbr_sum_rows_n -- a row's words and
      // alone entry lie a fixed nw words and one entry behind the row's before it, and the row's last term is the
      // detector's last group; rows 0: any detector, lm_tbr_sum)
      auto level_v = [&](auto rows, auto screen) {
        const uint32_t* pw = V + row0 * nw + (ba0 >> 1);
        const uint16_t* alone = AL + k * als + row0;  // the windows' last block of the detector's window, alone:
        const bool clipped = ba0 + ng == bendl;       // what the last group reads when it stands there
        const int jl = (ng - 1) % LM_TBR_GC;
        uint32_t w0, w1, w2, x0 = 0u, x1 = 0u;
        unsigned qn, q = 0u;
        bool lastc = false;
        auto fetch = [&]() {
          w0 = pw[0];
          w1 = pw[1];
          w2 = pw[2];
          qn = *alone;
        };
        fetch();
        if constexpr (decltype(rows)::value > 0) {
          constexpr int NG = decltype(rows)::value;  // (== ng: the row's last term is known where it is read)
          auto term = [&](int i, int g, unsigned& M, unsigned& m) {
            if (g == 0) {  // the row's entries, and the next row's words on their way
              lm_tbr_quad_align(w0, w1, w2, ba0, x0, x1);
              q = qn;
              pw += nw;
              alone += 1;
              fetch();
            }
            lm_tbr_quad_get(x0, x1, g, g == NG - 1 && clipped, q, M, m);
          };
          // the fp32 screen of the same terms (-1 proven, 1 unproven, 0 undecided), or the double sum (-1, 1)
          if constexpr (decltype(screen)::value)
            return lm_tbs_decide(lm_tbs_sum_rows_n<NG>(kh, Cf, K.tbs_bf[d], term), K.tbs_e[d]);
          else
            return lm_tbr_sum_rows_n<NG>(kh, C, bias, term) < 0.0 ? -1 : 1;
        }
        return lm_tbr_sum_negative(kh, ng, C, bias, [&](int i, int g, unsigned& M, unsigned& m) {
          if (g % LM_TBR_GC == 0) {  // a chunk's first term: its entries, and the next chunk's words on their way
            const int c = g / LM_TBR_GC;
            lm_tbr_quad_align(w0, w1, w2, ba0, x0, x1);
            q = qn;
            lastc = c == nc - 1;
            // (after the last chunk the words of the row below, which the tables' spare row covers: no branch)
            pw += lastc ? nw - 2 * (nc - 1) : 2;
            alone += lastc ? 1 : 0;
            fetch();
          }
          lm_tbr_quad_get(x0, x1, g % LM_TBR_GC, lastc && clipped && g % LM_TBR_GC == jl, q, M, m);
        }) ? -1 : 1;
      };
      // rows rs .. rs + nn - 1 from the block ranges B
      auto level_b = [&](int rs, int nn) {
        return lm_tbr_sum_negative(kh, ng, C, bias, [&](int i, int g, unsigned& M, unsigned& m) {
          const uint16_t* row = B16 + (row0 + rs + i) * nbk;
          M = 0u;
          m = 255u;
          for (int r = 0; r < nn; ++r, row += nbk) {
            unsigned a, b;
            lm_tbr_pair_range(nullptr, row, ba0 + g, bendl, a, b);
            M = max(M, a);
            m = min(m, b);
          }
        });
      };
      using std::integral_constant;
      using std::false_type;
      using std::true_type;
      bool proven;
      if constexpr (!ROWS) {
        proven = nr == LM_TB_H && level_v(integral_constant<int, 0>{}, false_type{}) < 0;
      } else {  // (nc, ng and the screen's flag are uniform: a wave takes one of the loops)
        proven = false;
        if (nr != LM_TB_H) {
        } else if (nc != 1) proven = level_v(integral_constant<int, 0>{}, false_type{}) < 0;
        else {
          // the screen first; the lanes it leaves undecided (few: DESIGN.md section 12) take the double sum, as every
          // lane of a detector without the screen does, and a wave that has such lanes counts them
          int dec = 0;
          if (K.tbs_on[d] != 0) {
            if (ng == 4) dec = level_v(integral_constant<int, 4>{}, true_type{});
            else if (ng == 3) dec = level_v(integral_constant<int, 3>{}, true_type{});
            else if (ng == 2) dec = level_v(integral_constant<int, 2>{}, true_type{});
            else dec = level_v(integral_constant<int, 1>{}, true_type{});
            const unsigned long long und = __ballot(dec == 0);
            if (und != 0ull && (tid & (WV - 1)) == __ffsll((long long)und) - 1)
              atomicAdd(tbs_fallback, (unsigned long long)__popcll(und));
          }
          if (dec == 0) {
            if (ng == 4) dec = level_v(integral_constant<int, 4>{}, false_type{});
            else if (ng == 3) dec = level_v(integral_constant<int, 3>{}, false_type{});
            else if (ng == 2) dec = level_v(integral_constant<int, 2>{}, false_type{});
            else dec = level_v(integral_constant<int, 1>{}, false_type{});
          }
          proven = dec < 0;
        }
      }
      if (!proven && !(LM_TB_RH == LM_TB_H && nr == LM_TB_H)) {
        if (LM_TB_RH == LM_TB_H) {
          proven = level_b(0, nr);
        } else {
          proven = true;
          for (int r = 0; r < nr && proven; ++r) proven = level_b(r, 1);
        }
      }
      if constexpr (NARROW) {  // (a short last tile row is not tried per 4-row block: its tiles stay wide)
        if (!proven) atomicOr(&mark[mb + t], 1u << (e - t * LM_TB_NBX) | (nr != LM_TB_H ? LM_NW_UNTRIED : 0u));
      } else {
        if (!proven) mark[mb + t] = 1u;
      }
    }
    __syncthreads();
    // 4c. (NARROW false) the marked entries of each detector close up: a group
    // of entries is read into registers, then written (an entry moves down or
    // stays, and a later group's entries lie above every place written before,
    // so one barrier per group of LM_TBW_CR * T entries, which a band's entries
    // rarely exceed)
    if constexpr (!NARROW) {
      constexpr int CR = LM_TBW_CR;
      for (int g0 = 0; g0 < nref; g0 += CR * T) {
        uint32_t en[CR], mk[CR];
        int kk[CR];
#pragma unroll
        for (int u = 0; u < CR; ++u) {
          const int i = g0 + u * T + tid;
          const bool act = i < nref;
          const int k = i < nr3[0] ? 0 : i < nr3[0] + nr3[1] ? 1 : 2;
          const int t = i - (k == 0 ? 0 : k == 1 ? nr3[0] : nr3[0] + nr3[1]);
          en[u] = act ? reinterpret_cast<const uint32_t*>(tbw_lds + TBW_SEL(ent3))[t] : 0u;
          mk[u] = act ? mark[i] : 0u;
          const bool kp = mk[u] != 0u;

          kk[u] = kp ? k : -1;
          if (act) TBW_SEL(fl)[en[u] & 0xFFFFu] = kp ? 1 : 0;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < CR; ++u)
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const bool mine = kk[u] == k;
            const int pos = wave_append(mine, &s_m[k]);
            if (mine) reinterpret_cast<uint32_t*>(tbw_lds + ent3[k])[pos] = en[u];
          }
      }
      __syncthreads();
      if (tid < 3) {
        const int k = tid;
        if (TBW_SEL(nr3) > 0) s_n[k] = s_m[k];
      }
    }
  }
  // this workgroup's list segment, as in k_ingest
  const int G = (nslot + LM_INGEST_FB - 1) / LM_INGEST_FB;
  const int c = ((int)blockIdx.x / LM_INGEST_FB) * LM_TL_NC / G;
  if constexpr (NARROW) {
    // 5w. the lists by class, a wave per detector.  The entries and their
    // marks stand where steps 4 and 4b left them (4b's barrier, or step 4's
    // when no detector is refined, is the last of the workgroup); a wave
    // without a detector, with a detector that is not listed or with one that
    // has neither an entry nor a bright tile leaves by a scalar branch.
    static_assert(LM_TB_THREADS >= 3 * 64, "a wave per detector of a view");
    const int k = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    if (k >= 3 || !TBW_SEL(on)) return;
    const int d = 3 * v + k;
    const LmDet& D = K.det[d];
    const bool tl = D.kind != 0;
    const int n = __builtin_amdgcn_readfirstlane(s_n[k]);
    const int nb = tl ? 0 : __builtin_amdgcn_readfirstlane(s_b[k]);  // a point detector's bright tiles
    if (n == 0 && nb == 0) return;
    const bool rf = TBW_SEL(refine), sp = rf && K.nw_on[d] != 0;
    const uint32_t* ent = reinterpret_cast<const uint32_t*>(tbw_lds + TBW_SEL(ent3));
    const uint32_t* mk = mark + (k == 0 ? 0 : k == 1 ? nr3[0] : nr3[0] + nr3[1]);  // (a refined detector: nr3[k] == n)
    uint8_t* __restrict__ flk = TBW_SEL(fl);
    // entries p0 .. p0 + 63 of the detector: lane's entry e, its class cls (0 dropped: a refined tile with every
    // block proven, 1 wide, 2 narrow) and a narrow one's span fc (first | count << 4)
    uint32_t e = 0u;
    int cls = 0, fc = 0;
    auto chunk = [&](int p0, bool flags) {
      const int p = p0 + lane;
      cls = 0;
      if (p < n) {
        e = ent[p];
        const uint32_t m = rf ? mk[p] : 0u;
        const bool kept = !rf || m != 0u;
        if (flags && rf) flk[e & 0xFFFFu] = kept ? 1 : 0;
        const LmNwClass cl = sp ? lm_nw_classify(m) : LmNwClass{0, 0, 0};
        cls = !kept ? 0 : cl.narrow != 0 ? 2 : 1;
        fc = cl.first | cl.count << 4;
      }
    };
    // pass A: the flags of a refined detector's tiles and the kept entries per class
    int cn = 0, cw = 0;
    for (int p0 = 0; p0 < n; p0 += 64) {
      chunk(p0, true);
      cn += (int)__popcll(__ballot(cls == 2));
      cw += (int)__popcll(__ballot(cls == 1));
    }
    // the places in the two lists of segment c and the listed and bright counters: one lane, no wait between them
    int32_t* __restrict__ cnt = tl ? tt_cnt + v * LM_TL_NC : pt_cnt + D.list * LM_TL_NC;
    int32_t* __restrict__ wcnt = nwo.cnt + (tl ? LM_NW_CNT_TTW + v * LM_TL_NC : LM_NW_CNT_PTW + D.list * LM_TL_NC);
    int32_t* __restrict__ ncnt = nwo.cnt + LM_NW_CNT_N + d * LM_TL_NC;
    int gn = 0, gw = 0;
    if (lane == 0) {
      if (cn) gn = atomicAdd(&ncnt[c], cn);
      if (cw) gw = atomicAdd(&wcnt[c], cw);
      if (cn + cw) atomicAdd(&cnt[c], cn + cw);
      if (nb) atomicAdd(&pt_cnt[(LM_NLIST + D.list) * LM_TL_NC + c], nb);
    }
    if (cn + cw == 0) return;
    gn = __builtin_amdgcn_readfirstlane(gn);
    gw = __builtin_amdgcn_readfirstlane(gw);
    // pass B: every kept entry to its place (one chunk: it is still in the registers)
    const int ntile = tl ? K.tt_tx[v] * K.tt_ty[v] : K.fl_tx[v] * K.fl_ty[v];
    const int64_t lo = tl ? (int64_t)v * K.tt_stride : (int64_t)D.list * K.tl_stride;  // the detector's lists
    const int64_t so = (int64_t)lm_tl_y0(c, G) * LM_INGEST_FB * ntile;                 // the segment in them
    uint32_t* __restrict__ wout = (tl ? nwo.ttw_list : nwo.ptw_list) + lo + so;
    unsigned long long* __restrict__ nout = nwo.n_list + (tl ? (int64_t)LM_NLIST * K.tl_stride : 0) + lo + so;
    for (int p0 = 0; p0 < n; p0 += 64) {
      if (n > 64) chunk(p0, false);
      const unsigned long long bn = __ballot(cls == 2), bw = __ballot(cls == 1);
      if (cls == 2)
        nout[gn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bn >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bn, 0u))] =
            lm_nw_entry(e, fc & 15, fc >> 4);
      if (cls == 1)
        wout[gw + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bw >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bw, 0u))] = e;
      gn += (int)__popcll(bn);
      gw += (int)__popcll(bw);
    }
  } else {
    __syncthreads();
    // 5. the segments' counters and the entries
    if (tid < 3 && (K.det[3 * v + tid].kind != 0 ? tt_cnt != nullptr : pt_cnt != nullptr)) {
      const LmDet& D = K.det[3 * v + tid];
      int32_t* __restrict__ cnt = D.kind != 0 ? tt_cnt + v * LM_TL_NC : pt_cnt + D.list * LM_TL_NC;
      s_base[tid] = s_n[tid] ? atomicAdd(&cnt[c], s_n[tid]) : 0;
      if (D.kind == 0 && s_b[tid]) atomicAdd(&pt_cnt[(LM_NLIST + D.list) * LM_TL_NC + c], s_b[tid]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (!on[k] || s_n[k] == 0) continue;
      const LmDet& D = K.det[3 * v + k];
      const int ntile = tail[k] ? K.tt_tx[v] * K.tt_ty[v] : K.fl_tx[v] * K.fl_ty[v];
      const uint32_t* ent = reinterpret_cast<const uint32_t*>(tbw_lds + K.tbw_ent[3 * v + k]);
      uint32_t* __restrict__ out =
          (tail[k] ? tt_list + (int64_t)v * K.tt_stride : pt_list + (int64_t)D.list * K.tl_stride) +
          (int64_t)lm_tl_y0(c, G) * LM_INGEST_FB * ntile + s_base[k];
      for (int p = tid; p < s_n[k]; p += T) out[p] = ent[p];
    }
  }
}
#undef TBW_SEL

#include "lm_corr.h"  // the correlation kernels are their own translation unit (lm_corr.hip)

#include "lm_cc.h"

// ------------------------------------------------------------------ k_tail
// keys of positive scores: (~float_bits(score) << 32) | row-major output index
DEV float key_score(unsigned long long k) { return __uint_as_float(~(unsigned)(k >> 32)); }
DEV unsigned key_lo(unsigned long long k) { return (unsigned)(k & 0xFFFFFFFFu); }
// detectTail (:2541-2555) -> detectLineCandidates (:2558-2742), one
// workgroup per frame:
//   bottom: largest component of (tail_b > 0) (selectLargestRegion :2604,
//     lm_cc.h) -> TAIL_MASK (:2611, a bitmap here: 64 columns per word),
//     colmax = reduce(MAX) over rows (:2615), first / last occupied columns
//     (:2642-2670), tail_width = last - first (:2677), 15 segments, the first
//     tail_width % 15 one column wider (:2678-2685), per segment the binary
//     moments m00, m10, m01 (:2702-2725) -> track x, y;
//   side: largest component of (tail_s > 0) & repeat(colmax) (:2623-2626),
//     then at every track x > 0 the moments of that one column (:2728-2737)
//     -> track z.
// cv::moments(binary) walks 32x32 tiles in raster order, accumulates integer
// tile sums (count, sum of x and of y inside the tile), scales them by 1/255
// and adds x0*m00 / y0*m00 of the tile origin; the sums are built here from
// the component's runs (arithmetic series per run and tile) and turned into
// doubles in that same tile order, so the tracks are bit-identical.
// No size limit: run tables beyond the LDS capacity go to global scratch.
#ifndef LM_TAIL_THREADS
#define LM_TAIL_THREADS 256
#endif
#define LM_TAIL_SEGS 15

struct TailLayout {  // byte offsets into k_tail's dynamic LDS
  int rowoff, colc, colm, mask, bm, par, area, key, rs, re, mb, ms, bytes;
};
__host__ __device__ inline TailLayout tail_layout(int TW, int HB, int HS, int cap, int ntc) {
  const int Hm = HB > HS ? HB : HS, nb64 = (TW + 63) / 64;
  const int ntrb = (HB + 31) / 32, ntrs = (HS + 31) / 32;
  TailLayout L;
  int o = 0;
  L.rowoff = o;
  o += 4 * (Hm + 1);
  L.colc = o;
  o += 4 * (TW + 2);
  o = (o + 15) & ~15;
  L.colm = o;
  o += 8 * nb64;
  L.mask = o;
  o += 8 * HB * nb64;
  L.bm = o;
  L.par = o;
  L.area = o + 4 * cap;
  L.key = o + 8 * cap;
  const int bmb = 8 * Hm * (nb64 + 1), ufb = 12 * cap;
  o += bmb > ufb ? bmb : ufb;
  L.rs = o;
  o += 2 * cap;
  L.re = o;
  o += 2 * cap;
  o = (o + 15) & ~15;
  L.mb = o;
  o += 4 * LM_TAIL_SEGS * ntrb * ntc * 3;
  L.ms = o;
  o += 4 * LM_TAIL_SEGS * ntrs * 2;
  L.bytes = o;
  return L;
}

// Segment of column offset rx in [0, tail_width) and its start (:2678-2685).
DEV void tail_segment(int rx, int rem, int reg, int* seg, int* sx) {
  if (rx < rem * (reg + 1)) {
    *seg = rx / (reg + 1);
    *sx = *seg * (reg + 1);
  } else {
    *seg = rem + (rx - rem * (reg + 1)) / reg;
    *sx = rem * (reg + 1) + (*seg - rem) * reg;
  }
}

// Bottom pass 1 over the chosen component's runs: TAIL_MASK bits, the column
// counts (difference array) and the first / last occupied columns.
template <bool G, class IX>
DEV void tail_bottom_runs(const CCRuns<IX> S, int R, const int* rowoff, int H, unsigned broot, int nb64,
                          unsigned long long* mask, int* colc, int* s_first, int* s_last) {
  for (int i = threadIdx.x; i < R; i += blockDim.x) {
    if (rld<G>(&S.par[i]) != broot) continue;
    const int y = cc_row_of(rowoff, H, i);
    const int x0 = (int)rld<G>(&S.rs[i]), x1 = (int)rld<G>(&S.re[i]);
    for (int k = x0 >> 6; k <= (x1 >> 6); ++k) {
      const int a = max(x0, 64 * k) - 64 * k, b = min(x1, 64 * k + 63) - 64 * k;
      const unsigned long long bits = (b == 63 ? ~0ull : ((1ull << (b + 1)) - 1)) & ~((1ull << a) - 1);
      atomicOr(&mask[(int64_t)y * nb64 + k], bits);
    }
    atomicAdd(&colc[x0], 1);
    atomicSub(&colc[x1 + 1], 1);
    atomicMin(s_first, x0);
    atomicMax(s_last, x1);
  }
}

// Bottom pass 2: integer tile sums of every segment's moments from the runs
// inside [first, first + tail_width).
template <bool G, class IX>
DEV void tail_bottom_moments(const CCRuns<IX> S, int R, const int* rowoff, int H, unsigned broot, int first, int tw,
                             int rem, int reg, unsigned* mb, int ntrb, int ntc) {
  for (int i = threadIdx.x; i < R; i += blockDim.x) {
    if (rld<G>(&S.par[i]) != broot) continue;
    const int y = cc_row_of(rowoff, H, i);
    const int a = max((int)rld<G>(&S.rs[i]), first) - first, b = min((int)rld<G>(&S.re[i]), first + tw - 1) - first;
    int rx = a;
    while (rx <= b) {
      int seg, sx;
      tail_segment(rx, rem, reg, &seg, &sx);
      const int wseg = seg < rem ? reg + 1 : reg;
      const int end = min(b, sx + wseg - 1);  // this segment's part of the run
      for (int l0 = rx - sx; l0 <= end - sx;) {  // 32-column tiles inside the segment
        const int tx = l0 >> 5, l1 = min(end - sx, 32 * tx + 31);
        const unsigned cnt = (unsigned)(l1 - l0 + 1);
        const unsigned sumx = (unsigned)((l0 + l1 - 64 * tx) * (int)cnt / 2);  // sum of (l - 32 tx), l in [l0, l1]
        unsigned* t = mb + ((seg * ntrb + (y >> 5)) * ntc + tx) * 3;
        atomicAdd(&t[0], cnt);
        atomicAdd(&t[1], sumx);
        atomicAdd(&t[2], (unsigned)(y & 31) * cnt);
        l0 = l1 + 1;
      }
      rx = end + 1;
    }
  }
}

// Side: every track column x > 0 the chosen component covers in a row adds
// that row to the column's tile sums.
template <bool G, class IX>
DEV void tail_side_moments(const CCRuns<IX> S, int R, const int* rowoff, int H, unsigned broot, const int* s_tx,
                           unsigned* ms, int ntrs) {
  for (int i = threadIdx.x; i < R; i += blockDim.x) {
    if (rld<G>(&S.par[i]) != broot) continue;
    const int y = cc_row_of(rowoff, H, i);
    const int x0 = (int)rld<G>(&S.rs[i]), x1 = (int)rld<G>(&S.re[i]);
    for (int k = 0; k < LM_TAIL_SEGS; ++k)
      if (s_tx[k] > 0 && s_tx[k] >= x0 && s_tx[k] <= x1) {
        atomicAdd(&ms[(k * ntrs + (y >> 5)) * 2], 1u);
        atomicAdd(&ms[(k * ntrs + (y >> 5)) * 2 + 1], (unsigned)(y & 31));
      }
  }
}

// BIG: tail boxes whose bitmaps and tables do not fit the CU's LDS (the
// reference has no size limit, LocoMouse_class.cpp:2604-2626): the same code
// on a per-slot global workspace (`ws`, tail_layout(..., cap 0) bytes per
// slot), every run table in global scratch.
template <bool BIG>
__global__ __launch_bounds__(LM_TAIL_THREADS) void k_tail(const LmConst* __restrict__ Kp, int s0,
                                                          const uint8_t* __restrict__ tailbin, int64_t tailbin_slot_bytes,
                                                          unsigned long long* __restrict__ tailmask,
                                                          unsigned* __restrict__ scratch, LmSlotOut* __restrict__ hdr,
                                                          long long* __restrict__ prof, uint8_t* __restrict__ ws,
                                                          int64_t ws_slot, const unsigned long long* __restrict__ keys,
                                                          const int32_t* __restrict__ n_pos) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smt_lds[];
#define TAIL_PROF(k) \
  if (prof && threadIdx.x == 0) prof[blockIdx.x * 16 + (k)] = clock64();
  TAIL_PROF(0)
  if (prof && threadIdx.x == 0) prof[blockIdx.x * 16 + 14] = wall_clock64();
  const LmConst& K = *Kp;
  const int slot = s0 + blockIdx.x;
  uint8_t* smt = BIG ? ws + (int64_t)slot * ws_slot : smt_lds;
  const int TW = K.tail_w, HB = K.tail_hb, HS = K.tail_hs, nb64 = (TW + 63) / 64;
  const int cap = BIG ? 0 : K.tail_cap, ntc = K.tail_ntc, ntrb = (HB + 31) / 32, ntrs = (HS + 31) / 32;
  const TailLayout L = tail_layout(TW, HB, HS, cap, ntc);
  int* rowoff = reinterpret_cast<int*>(smt + L.rowoff);
  int* colc = reinterpret_cast<int*>(smt + L.colc);
  unsigned long long* colm = reinterpret_cast<unsigned long long*>(smt + L.colm);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(smt + L.mask);
  unsigned long long* bm = reinterpret_cast<unsigned long long*>(smt + L.bm);
  unsigned* mb = reinterpret_cast<unsigned*>(smt + L.mb);
  unsigned* ms = reinterpret_cast<unsigned*>(smt + L.ms);
  const CCRuns<uint16_t> SL{reinterpret_cast<uint16_t*>(smt + L.rs), reinterpret_cast<uint16_t*>(smt + L.re),
                            reinterpret_cast<unsigned*>(smt + L.par), reinterpret_cast<unsigned*>(smt + L.area),
                            reinterpret_cast<unsigned*>(smt + L.key)};
  const int64_t capg = (int64_t)max(HB, HS) * ((TW + 1) / 2);  // at most ceil(TW/2) runs per row
  unsigned* gb = scratch + (int64_t)slot * 5 * capg;
  const CCRuns<unsigned> SG{gb, gb + capg, gb + 2 * capg, gb + 3 * capg, gb + 4 * capg};
  __shared__ unsigned long long s_red[LM_TAIL_THREADS / 64];
  __shared__ unsigned s_best;
  __shared__ int s_total, s_first, s_last;
  __shared__ int s_tx[LM_TAIL_SEGS];
  const int tid = threadIdx.x, nt = blockDim.x;
  const bool c8 = K.connectivity == 8;
  const bool lds_ok = TW <= 65535;
  const unsigned long long* __restrict__ binb =
      reinterpret_cast<const unsigned long long*>(tailbin + (int64_t)slot * tailbin_slot_bytes);
  const unsigned long long* __restrict__ bins = binb + (int64_t)HB * nb64;

  for (int i = tid; i < TW + 2; i += nt) colc[i] = 0;
  for (int i = tid; i < HB * nb64; i += nt) mask[i] = 0;
  for (int i = tid; i < LM_TAIL_SEGS * ntrb * ntc * 3; i += nt) mb[i] = 0;
  for (int i = tid; i < LM_TAIL_SEGS * ntrs * 2; i += nt) ms[i] = 0;
  if (tid == 0) {
    s_first = 0x7FFFFFFF;
    s_last = -1;
  }

  // ---- bottom: largest component, TAIL_MASK, column mask, segment moments
  cc_bitmap_bits(binb, HB, nb64, nullptr, bm, rowoff);
  TAIL_PROF(1)
  cc_wave0_scan(rowoff, HB, &s_total);
  int R = s_total;
  TAIL_PROF(2)
  const bool gb_b = !(lds_ok && R <= cap);
  if (!gb_b) cc_label<false>(SL, bm, nb64, TW, HB, R, rowoff, c8, s_red, &s_best);
  else cc_label<true>(SG, bm, nb64, TW, HB, R, rowoff, c8, s_red, &s_best);
  const unsigned best_b = s_best;
  TAIL_PROF(3)
  const bool have = best_b != 0xFFFFFFFFu;
  if (have) {
    if (!gb_b) tail_bottom_runs<false>(SL, R, rowoff, HB, best_b, nb64, mask, colc, &s_first, &s_last);
    else tail_bottom_runs<true>(SG, R, rowoff, HB, best_b, nb64, mask, colc, &s_first, &s_last);
  }
  __syncthreads();
  const int first = s_first, last = s_last;
  const int tail_width = have ? last - first : 0;  // :2677 (no +1)
  const int rem = tail_width % LM_TAIL_SEGS, reg = (tail_width - rem) / LM_TAIL_SEGS;
  if (have) {
    if (!gb_b) tail_bottom_moments<false>(SL, R, rowoff, HB, best_b, first, tail_width, rem, reg, mb, ntrb, ntc);
    else tail_bottom_moments<true>(SG, R, rowoff, HB, best_b, first, tail_width, rem, reg, mb, ntrb, ntc);
  }
  // column counts -> colmax bitmap (reduce(MAX, dim 0), :2615)
  if (tid < 64) {
    const int lane = tid;
    int carry = 0;
    for (int k = 0; k < nb64; ++k) {
      const int x = 64 * k + lane;
      int inc = x < TW ? colc[x] : 0;
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
      }
      const unsigned long long b = __ballot(x < TW && carry + inc > 0);
      if (lane == 0) colm[k] = b;
      carry += __shfl(inc, 63);
    }
  }
  __syncthreads();
  TAIL_PROF(4)
  unsigned long long* __restrict__ tm = tailmask + (int64_t)slot * HB * nb64;
  for (int i = tid; i < HB * nb64; i += nt) tm[i] = mask[i];
  // detectSideCandidates runs only when the bottom list of the feature is
  // non-empty after the TAIL_MASK filter (:820-833).  Decided here, from the
  // keys before k_nms stages any candidate over them: in k_nms the bottom
  // block of a (slot, feature) overwrites its own keys while the side block
  // would be reading them.
  for (int feat = 0; feat < LM_NFEAT; ++feat) {
    const LmDet& D = K.det[feat == 0 ? DET_PAW_B : DET_SNOUT_B];
    const unsigned long long* __restrict__ src = keys + (int64_t)slot * K.keys_per_slot + K.list_off[feat];
    const int n = n_pos[slot * LM_NLIST + feat];
    int keep = 0;
    for (int k = tid; k < n && !keep; k += nt) {
      const unsigned idx = key_lo(src[k]);
      const int y = idx / D.ow, x = idx - y * D.ow;
      keep = !(x < TW && y < HB && ((mask[y * nb64 + (x >> 6)] >> (x & 63)) & 1));
    }
    keep = __syncthreads_or(keep);
    if (tid == 0) hdr[slot].bottom_kept[feat] = keep != 0;
  }

  // ---- side: (tail_s > 0) & repeat(colmax) -> largest component
  cc_bitmap_bits(bins, HS, nb64, colm, bm, rowoff);
  TAIL_PROF(5)
  cc_wave0_scan(rowoff, HS, &s_total);
  R = s_total;
  const bool gb_s = !(lds_ok && R <= cap);
  if (!gb_s) cc_label<false>(SL, bm, nb64, TW, HS, R, rowoff, c8, s_red, &s_best);
  else cc_label<true>(SG, bm, nb64, TW, HS, R, rowoff, c8, s_red, &s_best);
  const unsigned best_s = s_best;
  TAIL_PROF(6)

  // track x, y per segment (moments of the bottom component, :2702-2725)
  if (tid < LM_TAIL_SEGS) {
    const int i = tid;
    int tx_ = -1, ty_ = -1;
    if (have) {
      const int sx = first + (i < rem ? i * (reg + 1) : rem * (reg + 1) + (i - rem) * reg);
      const int wseg = i < rem ? reg + 1 : reg;
      double m00 = 0, m10 = 0, m01 = 0;
      const double s = 1. / 255;
      const int nc = (wseg + 31) >> 5;
      for (int ty = 0; ty < ntrb; ++ty)
        for (int tx = 0; tx < nc; ++tx) {
          const unsigned* t = mb + ((i * ntrb + ty) * ntc + tx) * 3;
          const double mom0 = (double)(255u * t[0]) * s;
          const double mom1 = (double)(255u * t[1]) * s;
          const double mom2 = (double)(255u * t[2]) * s;
          const double xm = (double)(tx * 32) * mom0, ym = (double)(ty * 32) * mom0;
          m00 += mom0;
          m10 += mom1 + xm;
          m01 += mom2 + ym;
        }
      if (m00 > 0) {
        tx_ = (int)(m10 / m00) + sx;
        ty_ = (int)(m01 / m00) + 0;
      }
    }
    s_tx[i] = tx_;
    hdr[slot].tail[i] = tx_;
    hdr[slot].tail[LM_TAIL_SEGS + i] = ty_;
  }
  __syncthreads();
  TAIL_PROF(7)
  if (best_s != 0xFFFFFFFFu) {
    if (!gb_s) tail_side_moments<false>(SL, R, rowoff, HS, best_s, s_tx, ms, ntrs);
    else tail_side_moments<true>(SG, R, rowoff, HS, best_s, s_tx, ms, ntrs);
  }
  __syncthreads();
  TAIL_PROF(8)
  // track z (:2728-2737): the side moments of column x_i when x_i > 0
  if (tid < LM_TAIL_SEGS) {
    const int i = tid;
    int tz = -1;
    if (s_tx[i] > 0) {
      double m00 = 0, m01 = 0;
      const double s = 1. / 255;
      for (int ty = 0; ty < ntrs; ++ty) {
        const double mom0 = (double)(255u * ms[(i * ntrs + ty) * 2]) * s;
        const double mom2 = (double)(255u * ms[(i * ntrs + ty) * 2 + 1]) * s;
        const double ym = (double)(ty * 32) * mom0;
        m00 += mom0;
        m01 += mom2 + ym;
      }
      if (m00 > 0) tz = (int)(m01 / m00) + 0;
    }
    hdr[slot].tail[2 * LM_TAIL_SEGS + i] = tz;
  }
  if (prof && threadIdx.x == 0) {
    prof[blockIdx.x * 16 + 9] = clock64();
    prof[blockIdx.x * 16 + 13] = R;
    prof[blockIdx.x * 16 + 15] = wall_clock64();
  }
#undef TAIL_PROF
}

// ------------------------------------------------------------------- k_nms
// One 512-thread block per (frame, list).  Positive detections are filtered by
// TAIL_MASK (bottom lists), sorted by (score desc, row-major index asc) —
// equal to std::sort whenever scores are distinct; on an exact tie the list is
// re-sorted from row-major order with the libstdc++ introsort replica
// (lm_introsort.h) — then clustered: nmsMax for the bottom view,
// peakClustering for the side view.
#ifndef LM_NMS_THREADS
#define LM_NMS_THREADS 512
#endif
#define LM_GLOB_BLOCKS 16   // grid of the global-scratch (<true>) k_nms / k_post launches: one scratch region each
// The LDS instantiation at 36 KB and <= 64 VGPRs (8 waves per SIMD): four
// 512-thread blocks per CU, so a batch's 1,024 (slot, list) blocks are one
// round (at 2,048 entries / 48 KB and 75 VGPRs, three per CU): 67 -> 61 us per
// batch alone, +1 % frames/s with four contexts (profiles/r04/nms/)
#ifndef LM_NMS_CAP
#define LM_NMS_CAP 1536     // entries kept in LDS; larger lists use the global-memory path
#endif
#ifndef LM_NMS_RANKSORT
#define LM_NMS_RANKSORT 768  // up to this many entries: O(n^2/T) rank sort instead of bitonic
#endif
#ifndef LM_NMS_WPE
#define LM_NMS_WPE 8  // amdgpu_waves_per_eu minimum of the LDS instantiation
#endif
// nmsMax's "first earlier overlapping point": every (i < j) pair spread over
// the block (LM_NMS_PAIRPAR entries or fewer), or each j scanning its earlier
// points until its first hit.  All pairs balance a block's threads but test
// ~3x the pairs; with four blocks per CU that VALU time is taken from the
// other blocks and the correlation: the early-exit scan is 1-2 % more
// frames/s with four contexts (profiles/r04/nms/sweep.txt), so it is used.
#ifndef LM_NMS_PAIRPAR
#define LM_NMS_PAIRPAR 0
#endif
#ifndef LM_NMS_BRANCHLESS
#define LM_NMS_BRANCHLESS 1   // overlap test without branches (a zero factor when the rects do not intersect)
#endif


// in-place ascending bitonic sort of a[0..np), np a power of two, block-wide
DEV void bitonic_sort(unsigned long long* a, int np) {
  for (int k = 2; k <= np; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < np; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long x = a[i], y = a[ixj];
          const bool up = (i & k) == 0;
          if ((x > y) == up) {
            a[i] = y;
            a[ixj] = x;
          }
        }
      }
      __syncthreads();
    }
  }
}

// ascending sort of n DISTINCT keys by rank counting: every key's position is
// the number of smaller keys.  All lanes of a wave read the same a[i]
// (LDS broadcast), no barrier inside.  tmp holds n keys.
DEV void rank_sort(unsigned long long* a, unsigned long long* tmp, int n) {
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    const unsigned long long key = a[k];
    int r = 0;
    int i = 0;
#pragma unroll 1  // (unrolled further, the loads in flight spill at 64 VGPRs)
    for (; i + 8 <= n; i += 8) {  // 4 x 16 B loads in flight per iteration
      const ulonglong2 q0 = *reinterpret_cast<const ulonglong2*>(a + i);
      const ulonglong2 q1 = *reinterpret_cast<const ulonglong2*>(a + i + 2);
      const ulonglong2 q2 = *reinterpret_cast<const ulonglong2*>(a + i + 4);
      const ulonglong2 q3 = *reinterpret_cast<const ulonglong2*>(a + i + 6);
      r += (q0.x < key) + (q0.y < key) + (q1.x < key) + (q1.y < key) + (q2.x < key) + (q2.y < key) +
           (q3.x < key) + (q3.y < key);
    }
    for (; i < n; ++i) r += a[i] < key;
    tmp[r] = key;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < n; k += blockDim.x) a[k] = tmp[k];
  __syncthreads();
}

// ascending sort of n <= blockDim.x DISTINCT keys (< ~0): every wave sorts
// its 64 keys in registers (bitonic network over lane shuffles), the sorted
// runs go back to a, and each key's position is its index in its run plus,
// for every other run, the count of smaller keys there (binary searches, the
// runs' probes interleaved).  A few shuffle and LDS latencies per step instead
// of rank_sort's n / 8 rounds of loads per key.  tmp holds n keys.
static_assert(LM_NMS_THREADS % 64 == 0 && LM_NMS_THREADS <= 512, "wave_merge_sort: up to 8 runs of 64");
DEV void wave_merge_sort(unsigned long long* a, unsigned long long* tmp, int n) {
  constexpr int NR = LM_NMS_THREADS / 64;  // runs
  const int t = threadIdx.x, lane = t & 63, run = t >> 6, nruns = (n + 63) >> 6;
  unsigned long long v = t < n ? a[t] : ~0ull;
  if (run < nruns) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) {
        const unsigned long long p = __shfl_xor(v, j);
        const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
        v = keep_min ? (v < p ? v : p) : (v < p ? p : v);
      }
  }
  __syncthreads();  // every key of a has been read
  if (run < nruns) a[t] = v;  // sorted runs, padded with ~0 past n
  __syncthreads();
  if (t < n) {
    int lo[NR], rank = lane;
#pragma unroll
    for (int r = 0; r < NR; ++r) lo[r] = 0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < nruns && r != run && a[r * 64 + lo[r] + s - 1] < v) lo[r] += s;
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nruns && r != run) rank += lo[r] + (a[r * 64 + lo[r]] < v ? 1 : 0);
    tmp[rank] = v;
  }
  __syncthreads();
  for (int k = t; k < n; k += blockDim.x) a[k] = tmp[k];
  __syncthreads();
}

struct ReplicaLess {  // compareCandidate on (idx << 32 | score bits) words
  DEV bool operator()(unsigned long long a, unsigned long long b) const {
    return __uint_as_float((unsigned)(a & 0xFFFFFFFFu)) > __uint_as_float((unsigned)(b & 0xFFFFFFFFu));
  }
};

// Rect overlap test of nmsMax / peakClustering (:1698-1709, :1833-1844) on
// packed x | y << 16: inter / (2wh - inter) > 0.5  <=>  3*inter > 2wh.  The two
// are equal for these integers: the margin of the double quotient over 0.5 is
// >= 1/(4wh), far above its rounding error.
DEV bool overlaps_xy(unsigned a, unsigned b, int bw, int bh) {
  const int dx = abs((int)(a & 0xFFFFu) - (int)(b & 0xFFFFu));
  const int dy = abs((int)(a >> 16) - (int)(b >> 16));
  if constexpr (LM_NMS_BRANCHLESS) {
    // no intersection (dx >= bw or dy >= bh) makes a factor 0: 0 > 2wh is false
    return 3 * max(bw - dx, 0) * max(bh - dy, 0) > 2 * bw * bh;
  } else {
    if (dx >= bw || dy >= bh) return false;  // R.area() == 0
    return 3 * (bw - dx) * (bh - dy) > 2 * bw * bh;
  }
}

// std::sort(compareCandidate) replica in level order (lm_introsort.h
// process_range / std_sort_levels; tests/cpp/introsort_check.cpp proves the
// level-order form equal to libstdc++).  Every range of a level is handled
// by one wave:
//  * median-of-3 to the front (lane 0), then libstdc++'s unguarded Hoare
//    partition computed in parallel: with f_k the k-th element from the left
//    that is !(a < pivot) and l_k the k-th from the right that is
//    !(pivot < a) (both in the range as it was before the loop), the loop
//    swaps a[f_k] <-> a[l_k] for k < K, K = first k with f_k >= l_k, and
//    returns min(f_K, l_{K-1}) (f_0 when K = 0);
//  * depth 0: heap sort by lane 0 (libstdc++'s fallback; never seen here);
//  * ranges of <= 64 elements: their whole subtree, leaves' insertion sorts
//    included, in one wave's registers (wave_subtree).  Partitioned level
//    by level down to the 16-element leaves, every level took ~5k cycles,
//    latency-bound (the LDS lists, three wave syncs, the level's two block
//    barriers), and a leaf phase another ~15k: ~64k cycles for a
//    350-element tie list (profiles/r04/nms/kprof_tie_levels.txt).
// q: two queues of qcap (first, last, depth); tf, tr: n ints.
// Lanes of one wave exchanging data through memory.  k_nms reaches its
// arrays through generic pointers (LDS, or global scratch for long lists), so
// the accesses are FLAT instructions, which complete out of order: a
// wavefront-scope fence alone emits no wait, and a lane could read a value
// another lane had stored but whose store had not landed (measured: rare
// wrong leaders in the tie sort and in peakClustering, more often when other
// kernels load the memory system).  Drain both counters, then a workgroup
// fence for the global-scratch case, then the wave barrier.
DEV void wave_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

DEV int wave_partition(unsigned long long* a, int F, int L, int* tf, int* tr) {
  const ReplicaLess comp;
  const int lane = threadIdx.x & 63;
  if (lane == 0) {
    const int mid = F + (L - F) / 2;
    lm_sort::move_median_to_first(a + F, a + F + 1, a + mid, a + L - 1, comp);
  }
  wave_sync();
  const unsigned long long pv = a[F];
  const int lo = F + 1, hi = L;
  // ranks of the stoppers; tf[lo + k] = f_k, tr[lo + k] = k-th R-stopper from the LEFT
  int nl = 0, nr = 0;
  for (int b = lo; b < hi; b += 64) {
    const int i = b + lane;
    bool lf = false, rf = false;
    if (i < hi) {
      const unsigned long long v = a[i];
      lf = !comp(v, pv);
      rf = !comp(pv, v);
    }
    const unsigned long long ml = __ballot(lf), mr = __ballot(rf);
    const unsigned long long below = (1ull << lane) - 1;
    if (lf) tf[lo + nl + __popcll(ml & below)] = i;
    if (rf) tr[lo + nr + __popcll(mr & below)] = i;
    nl += __popcll(ml);
    nr += __popcll(mr);
  }
  wave_sync();
  // K: f_k < l_k holds for a prefix of k
  int K = 0;
  const int kmax = min(nl, nr);
  for (int b = 0; b < kmax; b += 64) {
    const int k = b + lane;
    const bool ok = k < kmax && tf[lo + k] < tr[lo + nr - 1 - k];
    const unsigned long long m = __ballot(ok);
    K += __popcll(m);
    if (m != ~0ull) break;
  }
  int cut;
  if (K == 0) cut = tf[lo];
  else cut = min(K < nl ? tf[lo + K] : 0x7fffffff, tr[lo + nr - K]);
  for (int k = lane; k < K; k += 64) {
    const int i = tf[lo + k], j = tr[lo + nr - 1 - k];
    const unsigned long long x = a[i], y = a[j];
    a[i] = y;
    a[j] = x;
  }
  wave_sync();
  return cut;
}

DEV unsigned long long readlane_u64(unsigned long long v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
DEV unsigned long long bpermute_u64(unsigned long long v, int src) {  // lane src's v
  const unsigned lo = __builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)v);
  const unsigned hi = __builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
DEV unsigned long long permute_u64(unsigned long long v, int dst) {  // v to lane dst (a permutation)
  const unsigned lo = __builtin_amdgcn_ds_permute(dst << 2, (int)(unsigned)v);
  const unsigned hi = __builtin_amdgcn_ds_permute(dst << 2, (int)(unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
// position of the k-th (0-based) set bit of m counting from bit 0 (m must
// have more than k set bits)
DEV int nth_set_bit(unsigned long long m, int k) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const int c = __popcll((m >> pos) & ((1ull << w) - 1));
    if (k >= c) {
      k -= c;
      pos += w;
    }
  }
  return pos;
}

// One range [F, L) of <= 64 elements at depth d0, finished by one wave in
// registers (element F + i in lane i): every partition of its introsort
// subtree, then the final insertion sort of its leaves.  The ranges of the
// subtree are disjoint and what happens to a range depends on its contents
// and depth alone (lm_introsort.h, level-order formulation), so they are
// taken one at a time, lowest first: `bnd` marks where the ranges start,
// `pend` those of > kThreshold elements still to partition, lane s's `dep`
// the depth of the range starting at s.  A partition is wave_partition's
// (median of three to the front, then the k-th !(a < pivot) element from the
// left swapped with the k-th !(pivot < a) from the right while the first is
// left of the second) on ballots instead of LDS lists; a leaf's insertion
// sort is its stable sort (each element's place: the leaf's elements that
// compare before it, and the equal ones left of it).  No LDS round trip and
// no barrier except on the depth-0 heap-sort fallback.
DEV void wave_subtree(unsigned long long* a, int F, int L, int d0) {
  const ReplicaLess comp;
  constexpr int TH = lm_sort::kThreshold;
  const int lane = threadIdx.x & 63;
  const int m = L - F;
  unsigned long long v = lane < m ? a[F + lane] : 0ull;
  unsigned long long bnd = 1ull, pend = m > TH ? 1ull : 0ull;
  int dep = d0;
  const unsigned long long below = (1ull << lane) - 1;
  while (pend) {
    const int s = __builtin_ctzll(pend);  // s + TH < m <= 64
    pend &= pend - 1;
    const unsigned long long after = bnd & ~((2ull << s) - 1);
    const int e = after ? __builtin_ctzll(after) : m;
    const int d = __builtin_amdgcn_readlane(dep, s);
    if (d == 0) {  // depth limit: libstdc++'s heap sort, by lane 0 (never seen here)
      if (lane < m) a[F + lane] = v;
      wave_sync();
      if (lane == 0) lm_sort::partial_sort_full(a + F + s, a + F + e, comp);
      wave_sync();
      v = lane < m ? a[F + lane] : 0ull;
      continue;  // sorted: its leaf sort below leaves it as it is
    }
    // move_median_to_first(s, s + 1, mid, e - 1)
    const int mid = s + (e - s) / 2;
    const unsigned long long x = readlane_u64(v, s + 1), y = readlane_u64(v, mid), z = readlane_u64(v, e - 1);
    int ch;
    if (comp(x, y)) ch = comp(y, z) ? mid : comp(x, z) ? e - 1 : s + 1;
    else ch = comp(x, z) ? s + 1 : comp(y, z) ? e - 1 : mid;
    const unsigned long long vs = readlane_u64(v, s), pv = readlane_u64(v, ch);
    if (lane == s) v = pv;
    if (lane == ch) v = vs;
    const bool in = lane > s && lane < e;
    const bool lf = in && !comp(v, pv), rf = in && !comp(pv, v);
    const unsigned long long ml = __ballot(lf), mr = __ballot(rf);
    const int nl = __popcll(ml), nr = __popcll(mr);
    const int fk = nth_set_bit(ml, lane);           // f_k, k = lane (lane < nl)
    const int lk = nth_set_bit(mr, nr - 1 - lane);  // l_k, k = lane (lane < nr)
    const int K = __popcll(__ballot(lane < nl && lane < nr && fk < lk));
    int cut;
    if (K == 0) {
      cut = __builtin_amdgcn_readlane(fk, 0);
    } else {
      cut = __builtin_amdgcn_readlane(lk, K - 1);
      if (K < nl) cut = min(cut, __builtin_amdgcn_readlane(fk, K));
    }
    // swap a[f_k] <-> a[l_k], k < K (no element is both an f_k and an l_k)
    const int rl = __popcll(ml & below), rr = __popcll(mr >> lane) - 1;
    const int from_l = __shfl(lk, rl), from_r = __shfl(fk, rr & 63);
    const int src = (lf && rl < K) ? from_l : (rf && rr < K) ? from_r : lane;
    v = bpermute_u64(v, src);
    if (lane == s || (lane == cut && cut < e)) dep = d - 1;
    if (cut < e) bnd |= 1ull << cut;
    if (cut - s > TH) pend |= 1ull << s;
    if (e - cut > TH) pend |= 1ull << cut;
  }
  // leaves: stable sort of each (a heap-sorted range keeps its order)
  const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1;
  const int ls = 63 - __builtin_clzll(bnd & upto);
  const unsigned long long aft = bnd & ~upto;
  const int le = aft ? __builtin_ctzll(aft) : m;
  const float sc = __uint_as_float((unsigned)v);
  int rk = 0;
#pragma unroll
  for (int j = 0; j < TH; ++j) {
    const int i = ls + j;
    const float sj = __shfl(sc, i & 63);
    if (i < le) rk += (sj > sc) || (i < lane && !(sc > sj));
  }
  const int dst = lane >= m ? lane : le - ls <= TH ? ls + rk : lane;
  v = permute_u64(v, dst);
  if (lane < m) a[F + lane] = v;
}

// wave_partition by the whole block: the stoppers' ranks come from per-wave
// ballot counts (s_w: 2 nw + 1 ints), the swaps are spread over the block.
DEV int block_partition(unsigned long long* a, int F, int L, int* tf, int* tr, int* s_w) {
  const ReplicaLess comp;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, nw = blockDim.x >> 6;
  if (t == 0) {
    const int mid = F + (L - F) / 2;
    lm_sort::move_median_to_first(a + F, a + F + 1, a + mid, a + L - 1, comp);
    s_w[2 * nw] = 0;
  }
  __syncthreads();
  const unsigned long long pv = a[F];
  const int lo = F + 1, hi = L;
  const unsigned long long below = (1ull << lane) - 1;
  int nl = 0, nr = 0;
  for (int b = lo; b < hi; b += blockDim.x) {
    const int i = b + t;
    bool lf = false, rf = false;
    if (i < hi) {
      const unsigned long long v = a[i];
      lf = !comp(v, pv);
      rf = !comp(pv, v);
    }
    const unsigned long long ml = __ballot(lf), mr = __ballot(rf);
    if (lane == 0) {
      s_w[wid] = __popcll(ml);
      s_w[nw + wid] = __popcll(mr);
    }
    __syncthreads();
    int bl = nl, br = nr, tl = 0, tr_ = 0;
    for (int w = 0; w < nw; ++w) {
      const int cl = s_w[w], cr = s_w[nw + w];
      if (w < wid) {
        bl += cl;
        br += cr;
      }
      tl += cl;
      tr_ += cr;
    }
    if (lf) tf[lo + bl + __popcll(ml & below)] = i;
    if (rf) tr[lo + br + __popcll(mr & below)] = i;
    nl += tl;
    nr += tr_;
    __syncthreads();  // the lists are complete, s_w free again
  }
  const int kmax = min(nl, nr);
  for (int k0 = 0; k0 < kmax; k0 += blockDim.x) {  // K: f_k < l_k holds for a prefix of k
    const int k = k0 + t;
    const unsigned long long m = __ballot(k < kmax && tf[lo + k] < tr[lo + nr - 1 - k]);
    if (lane == 0 && m) atomicAdd(&s_w[2 * nw], __popcll(m));
  }
  __syncthreads();
  const int K = s_w[2 * nw];
  int cut;
  if (K == 0) cut = tf[lo];
  else cut = min(K < nl ? tf[lo + K] : 0x7fffffff, tr[lo + nr - K]);
  for (int k = t; k < K; k += blockDim.x) {
    const int i = tf[lo + k], j = tr[lo + nr - 1 - k];
    const unsigned long long x = a[i], y = a[j];
    a[i] = y;
    a[j] = x;
  }
  __syncthreads();
  return cut;
}

// Ranges of <= 64 elements go to a list (`small`, packed first | size << 11
// | depth << 18) that the waves finish at the end with wave_subtree; the
// others are partitioned level by level, by the whole block when a level
// holds one range (the top levels, and the long chains of uneven partitions
// that exact ties produce), else one wave per range.
// prof (LM_KPROF=1, else null): [0] clock at the end of the levels, [1] the
// number of levels
DEV int small_range(int f, int l, int d) { return f | (l - f) << 11 | d << 18; }
DEV void std_sort_levels_dev(unsigned long long* a, int n, int* q, int qcap, int* small, int* tf, int* tr,
                             int* s_cnt, int* s_w, long long* prof = nullptr) {
  static_assert(LM_NMS_CAP <= 2048, "small_range packs first in 11 bits");
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int* s_small = s_w + 2 * nw + 1;
  const ReplicaLess comp;
  if (threadIdx.x == 0) {
    const int d0 = 2 * lm_sort::lg_(n);
    s_cnt[0] = n > 64 ? 1 : 0;
    s_cnt[1] = 0;
    *s_small = 0;
    if (n > 64) {
      q[0] = 0;
      q[1] = n;
      q[2] = d0;
    } else if (n > 0) {
      small[0] = small_range(0, n, d0);
      *s_small = 1;
    }
  }
  __syncthreads();
  // children of a partitioned range: > 64 elements to the next level, the rest to `small`
  auto push = [&](int* nxt, int sel, int f, int l, int d) {
    if (l - f > 64) {
      const int k = atomicAdd(&s_cnt[1 - sel], 1);
      nxt[3 * k] = f;
      nxt[3 * k + 1] = l;
      nxt[3 * k + 2] = d;
    } else if (l > f) {
      small[atomicAdd(s_small, 1)] = small_range(f, l, d);
    }
  };
  int sel = 0;
  while (true) {
    const int qn = s_cnt[sel];
    if (qn == 0) break;
    const int* cur = q + sel * 3 * qcap;
    int* nxt = q + (1 - sel) * 3 * qcap;
    if (qn == 1 && cur[2] > 0) {
      const int f = cur[0], l = cur[1], d = cur[2];
      const int cut = block_partition(a, f, l, tf, tr, s_w);
      if (threadIdx.x == 0) {
        push(nxt, sel, f, cut, d - 1);
        push(nxt, sel, cut, l, d - 1);
      }
    } else {
      for (int r = wid; r < qn; r += nw) {
        const int f = cur[3 * r], l = cur[3 * r + 1], d = cur[3 * r + 2];
        if (d == 0) {
          if (lane == 0) lm_sort::partial_sort_full(a + f, a + l, comp);  // sorted: a leaf
        } else {
          const int cut = wave_partition(a, f, l, tf, tr);
          if (lane == 0) {
            push(nxt, sel, f, cut, d - 1);
            push(nxt, sel, cut, l, d - 1);
          }
        }
        wave_sync();
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) s_cnt[sel] = 0;
    sel = 1 - sel;
    __syncthreads();
    if (prof && threadIdx.x == 0) ++prof[1];
  }
  if (prof && threadIdx.x == 0) prof[0] = clock64();
  const int ns = *s_small;
  for (int r = wid; r < ns; r += nw) {  // the whole subtree and its leaves' insertion sorts
    const int e = small[r];
    const int f = e & 0x7FF;
    wave_subtree(a, f, f + ((e >> 11) & 0x7F), e >> 18);
  }
  __syncthreads();
}

// Enumerates the j in [0, n) with flag(j) in increasing order: out[r] = j.
// Returns their count.
template <class F>
DEV int block_compact(int n, F flag, int* out, int* s_wsum) {
  const int T = blockDim.x, chunk = (n + T - 1) / T;
  const int j0 = threadIdx.x * chunk, j1 = min(n, j0 + chunk);
  int c = 0;
  for (int j = j0; j < j1; ++j) c += flag(j);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int v = c;  // inclusive wave scan
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  if (lane == 63) s_wsum[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int w = 0; w < (T >> 6); ++w) {
      const int t = s_wsum[w];
      s_wsum[w] = acc;
      acc += t;
    }
    s_wsum[T >> 6] = acc;
  }
  __syncthreads();
  int r = s_wsum[wid] + v - c;
  for (int j = j0; j < j1; ++j)
    if (flag(j)) out[r++] = j;
  const int total = s_wsum[T >> 6];
  __syncthreads();
  return total;
}

DEV double readlane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// The body of k_nms on its working arrays: LDS (GLOB = false, every access a
// ds_* instruction) or per-block global scratch for lists above LM_NMS_CAP.
// Kept as two instantiations so the common case never goes through generic
// (FLAT) pointers, which cost several times the latency of LDS accesses.
// optional phase timestamps (LM_KPROF=1): clock64() of thread 0 per phase
#ifndef LM_NMS_PREHASH
#define LM_NMS_PREHASH 1
#endif
#ifndef LM_NMS_TIE_PRIO
#define LM_NMS_TIE_PRIO 3  // s_setprio of a tie block's waves (0: as every block)
#endif
#define NMS_PROF(k) \
  if (prof && threadIdx.x == 0) prof[(blockIdx.x * 2 + (blockIdx.y & 1)) * 16 + (k)] = clock64();
template <bool GLOB>
DEV auto nms_run(const LmConst& K, const LmDet& D, LmSlotOut* H, int slot, int list, int side, int feat, int n_in,
                 const unsigned long long* __restrict__ src, const unsigned long long* __restrict__ tailmask,
                 unsigned long long* a, int* assign, int* mlist, unsigned* xy, int* s_tmp, unsigned long long* stmp,
                 int qcap, int* s_stk, int* s_wsum,
                 int* s_n_, int* s_flag_, int* s_qcnt, int* s_part, unsigned long long* __restrict__ keys,
                 int32_t* __restrict__ err,
                 long long* __restrict__ prof) -> int {
  int& s_n = *s_n_;
  int& s_flag = *s_flag_;
  constexpr bool glob = GLOB;
  int* s_assign = assign;
  int* s_mlist = mlist;
  unsigned* s_xy = xy;
  if (threadIdx.x == 0) {
    s_n = 0;
    s_flag = 0;
  }
  __syncthreads();
  // load + TAIL_MASK filter (bottom: mask(BB_BOTTOM_TAIL).setTo(255, TAIL_MASK), :783)
  const int tnb = (K.tail_w + 63) / 64;  // TAIL_MASK bitmap words per row
  const unsigned long long* __restrict__ tm = tailmask + (int64_t)slot * K.tail_hb * tnb;
  for (int k = threadIdx.x; k < n_in; k += blockDim.x) {
    const unsigned long long v = src[k];
    bool keep = true;
    if (!side) {
      const unsigned idx = key_lo(v);
      const int y = idx / D.ow, x = idx - y * D.ow;
      if (x < K.tail_w && y < K.tail_hb && ((tm[y * tnb + (x >> 6)] >> (x & 63)) & 1)) keep = false;
    }
    if (keep) a[atomicAdd(&s_n, 1)] = v;
  }
  __syncthreads();
  NMS_PROF(1)
  const int n = s_n;
  if (prof && threadIdx.x == 0) prof[(blockIdx.x * 2 + (blockIdx.y & 1)) * 16 + 13] = n;
  int np = 1;
  while (np < n) np <<= 1;
  // Exact score ties, found before sorting (an LDS hash set of the score
  // bits, linear probing, at most half full): a tie list is re-sorted from
  // row-major order by the std::sort replica below, so its (score, index)
  // sort would be thrown away -- ~20k cycles of the slowest blocks.
  // The table is the next power of two >= 2n and lives in s_tmp
  // (LM_NMS_CAP ints), so it is used only when that power fits: n <= 512 at
  // LM_NMS_CAP = 1536 (2n <= CAP alone would let 513..768 keys write a
  // 2048-entry table past s_tmp).
  int tb = 64, lg = 6;
  while (tb < 2 * n) {
    tb <<= 1;
    ++lg;
  }
  const bool pre = LM_NMS_PREHASH && !glob && tb <= LM_NMS_CAP;
  if (pre) {
    unsigned* tab = reinterpret_cast<unsigned*>(s_tmp);
    for (int k = threadIdx.x; k < tb; k += blockDim.x) tab[k] = ~0u;  // empty: a NaN pattern no score has
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
      const unsigned h = (unsigned)(a[k] >> 32);
      // Fibonacci hashing: the product's HIGH bits, which every bit of the
      // score feeds (scores of a smooth map often share their low mantissa
      // bits, and the low bits of the product only see those)
      unsigned sl = (h * 2654435761u) >> (32 - lg);
      while (true) {
        const unsigned old = atomicCAS(&tab[sl], ~0u, h);
        if (old == ~0u) break;
        if (old == h) {
          s_flag = 1;
          break;
        }
        sl = (sl + 1) & (unsigned)(tb - 1);
      }
    }
    __syncthreads();
  }
  if (!(pre && s_flag)) {
    if (!glob && n <= LM_NMS_THREADS) {
      wave_merge_sort(a, stmp, n);
    } else if (n <= LM_NMS_RANKSORT) {
      rank_sort(a, stmp, n);
    } else {
      for (int k = n + threadIdx.x; k < np; k += blockDim.x) a[k] = ~0ull;
      __syncthreads();
      bitonic_sort(a, np);
    }
  }
  NMS_PROF(2)
  if (!pre) {
    for (int k = threadIdx.x; k + 1 < n; k += blockDim.x)
      if ((a[k] >> 32) == (a[k + 1] >> 32)) s_flag = 1;
    __syncthreads();
  }
  const int tie = s_flag;
  if (tie) {  // (GLOB: the row-major re-sort below is the single-thread replica)
    // A tie block is the launch's slowest (the replica's levels, then the
    // same clustering as every block) and shares its CU with three others
    // that end far earlier: its waves take issue priority for the rest of
    // the block, so the span is more nearly its own length.
    __builtin_amdgcn_s_setprio(LM_NMS_TIE_PRIO);
    // exact score tie: std::sort from the row-major order nmsMax builds (:1638-1648)
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
      const unsigned long long v = a[k];
      a[k] = ((unsigned long long)key_lo(v) << 32) | (unsigned)(~(unsigned)(v >> 32));
    }
    // every key must be re-keyed before any thread ranks them (rank_sort reads
    // all n keys); without this barrier a lagging wave's old-format keys were
    // ranked among new-format ones -- duplicate ranks, unwritten slots, and
    // garbage candidates in rare tie blocks
    __syncthreads();
    NMS_PROF(8)
    if (!glob) {
      if (n <= LM_NMS_THREADS) {  // back to row-major order
        wave_merge_sort(a, stmp, n);
      } else if (n <= LM_NMS_RANKSORT) {
        rank_sort(a, stmp, n);
      } else {
        for (int k = n + threadIdx.x; k < np; k += blockDim.x) a[k] = ~0ull;
        __syncthreads();
        bitonic_sort(a, np);
      }
      NMS_PROF(9)
      std_sort_levels_dev(a, n, s_mlist, qcap, s_assign, reinterpret_cast<int*>(s_xy), s_tmp, s_qcnt, s_part,
                          prof ? prof + (blockIdx.x * 2 + (blockIdx.y & 1)) * 16 + 11 : nullptr);
      NMS_PROF(10)
    } else {  // rare and slow: one thread, explicit stack
      for (int k = n + threadIdx.x; k < np; k += blockDim.x) a[k] = ~0ull;
      __syncthreads();
      if (np > 1) bitonic_sort(a, np);
      if (threadIdx.x == 0) lm_sort::std_sort(a, a + n, ReplicaLess(), s_stk);
      __syncthreads();
    }
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
      const unsigned long long v = a[k];
      a[k] = ((unsigned long long)(~(unsigned)(v & 0xFFFFFFFFu)) << 32) | (unsigned)(v >> 32);
    }
    __syncthreads();
  }
  // row-major index -> packed (x | y << 16), once per detection
  const int ow = D.ow, bw = D.box_w, bh = D.box_h;
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    const unsigned idx = key_lo(a[k]);
    const unsigned y = idx / ow, x = idx - y * ow;
    xy[k] = x | (y << 16);
  }
  for (int k = n + threadIdx.x; k < ((n + 15) & ~15); k += blockDim.x) xy[k] = 0;
  __syncthreads();
  NMS_PROF(3)
  if (!side) {
    // nmsMax: every point, suppressed or not, suppresses the later points it
    // overlaps (:1677-1720) => j belongs to the first i < j overlapping it;
    // maxima by pointer jumping.
    if (n <= LM_NMS_PAIRPAR) {
      // Every (i < j) pair tested once, spread evenly over the block: tile
      // (b, j) holds the pairs i in [16 b, min(16 b + 16, j)), tiles in (b, j)
      // order, a thread takes every blockDim-th one; its first hit goes to
      // assign[j] by an LDS atomicMin.  (Each j scanning its earlier points
      // until its first hit left the block waiting for the last maxima's full
      // scans: ~25k cycles at ~300 points.)
      for (int j = threadIdx.x; j < n; j += blockDim.x) assign[j] = j;
      __syncthreads();
      int b = 0, j = 1 + threadIdx.x;  // tile index threadIdx.x: row b = 0 holds j = 1 .. n - 1
      while (true) {
        while (b * 16 + 1 < n && j >= n) {  // past row b: into row b + 1 (j = 16 (b + 1) + 1 ..)
          const int over = j - n;
          ++b;
          j = 16 * b + 1 + over;
        }
        if (j >= n) break;
        const int i0 = 16 * b;
        unsigned v[16];
        *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(xy + i0);
        *reinterpret_cast<uint4*>(v + 4) = *reinterpret_cast<const uint4*>(xy + i0 + 4);
        *reinterpret_cast<uint4*>(v + 8) = *reinterpret_cast<const uint4*>(xy + i0 + 8);
        *reinterpret_cast<uint4*>(v + 12) = *reinterpret_cast<const uint4*>(xy + i0 + 12);
        const unsigned xj = xy[j];
        unsigned hit = 0;
#pragma unroll
        for (int t = 0; t < 16; ++t) hit |= (unsigned)(i0 + t < j && overlaps_xy(v[t], xj, bw, bh)) << t;
        if (hit) atomicMin(&assign[j], i0 + __ffs(hit) - 1);
        j += blockDim.x;
      }
    } else {
      // long lists: each j scans the earlier points 16 at a time (4 x 16 B
      // loads in flight) and stops at its first hit
      for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const unsigned xj = xy[j];
        int as = j;
        for (int i0 = 0; i0 < j && as == j; i0 += 16) {
          unsigned v[16];
          *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(xy + i0);
          *reinterpret_cast<uint4*>(v + 4) = *reinterpret_cast<const uint4*>(xy + i0 + 4);
          *reinterpret_cast<uint4*>(v + 8) = *reinterpret_cast<const uint4*>(xy + i0 + 8);
          *reinterpret_cast<uint4*>(v + 12) = *reinterpret_cast<const uint4*>(xy + i0 + 12);
          unsigned hit = 0;
#pragma unroll
          for (int t = 0; t < 16; ++t) hit |= (unsigned)(i0 + t < j && overlaps_xy(v[t], xj, bw, bh)) << t;
          if (hit) as = i0 + __ffs(hit) - 1;
        }
        assign[j] = as;
      }
    }
    __syncthreads();
    NMS_PROF(4)
    while (true) {
      if (threadIdx.x == 0) s_flag = 0;
      __syncthreads();
      for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int m = assign[j], mm = assign[m];
        if (mm != m) {
          assign[j] = mm;
          s_flag = 1;
        }
      }
      __syncthreads();
      const int again = s_flag;
      __syncthreads();
      if (!again) break;
    }
  } else if (threadIdx.x < 64) {
    // peakClustering: leaders in sorted order; each claims the undecided
    // points overlapping it (:1815-1850).  One wave, no block barriers:
    // assign[j] = leader, -1 undecided.
    const int lane = threadIdx.x;
    for (int j = lane; j < n; j += 64) assign[j] = -1;
    wave_sync();
    int lead = 0;
    while (lead < n) {
      const unsigned xl = xy[lead];
      if (lane == 0) assign[lead] = lead;
      int next = n;
      for (int b = lead + 1; b < n; b += 64) {
        const int j = b + lane;
        bool und = false;
        if (j < n && assign[j] < 0) {
          if (overlaps_xy(xl, xy[j], bw, bh)) assign[j] = lead;
          else und = true;
        }
        const unsigned long long m = __ballot(und);
        if (m && next == n) next = b + __ffsll((long long)m) - 1;
      }
      wave_sync();  // the next leader's sweep reads assign[] entries other lanes just wrote
      lead = next;
    }
  }
  __syncthreads();
  NMS_PROF(5)
  // maxima (leaders) in sorted order
  const int ncand = block_compact(n, [&](int j) { return assign[j] == j; }, mlist, s_wsum);
  LmCand* __restrict__ out = LM_CAND_STAGE(K, keys, slot, list);
  const bool fits = ncand <= K.list_cap[list] / 2;  // always: maxima are >= w/3 apart
  if (!fits && threadIdx.x == 0) atomicOr(err, 32);
  NMS_PROF(6)
  // weighted mean over each cluster's members in sorted order, in double
  // (:1731-1744 / :1865-1883).  One wave per cluster: members are found 64 at
  // a time with a ballot; the products x*s, y*s are exact in double, so they
  // are formed per lane and only the additions run in member order.
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int r = wid; r < ncand && fits; r += nw) {
    const int m = mlist[r];
    double wx = 0, wy = 0, ss = 0;
    int members = 0;
    for (int b = m; b < n; b += 64) {
      const int j = b + lane;
      bool mem = false;
      double px = 0, py = 0, ps = 0;
      if (j < n && assign[j] == m) {
        mem = true;
        const unsigned q = xy[j];
        ps = (double)key_score(a[j]);
        px = (double)(int)(q & 0xFFFFu) * ps;
        py = (double)(int)(q >> 16) * ps;
      }
      unsigned long long mask = __ballot(mem);
      members += __popcll(mask);
      while (mask) {
        const int sl = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        wx += readlane_f64(px, sl);
        wy += readlane_f64(py, sl);
        ss += readlane_f64(ps, sl);
      }
    }
    if (lane == 0) {
      const unsigned xm = xy[m];
      LmCand c;
      c.s = (double)key_score(a[m]);
      if (!side) {  // Point_<double> / double -> Point_<int>: cvRound (half even)
        c.x = (int)rint(wx / ss);
        c.y = (int)rint(wy / ss);
      } else if (members > 1) {  // std::round (half away from zero)
        c.x = (int)round(wx / ss);
        c.y = (int)round(wy / ss);
      } else {
        c.x = (int)(xm & 0xFFFFu);
        c.y = (int)(xm >> 16);
      }
      out[r] = c;
    }
  }
  NMS_PROF(7)
  if (prof && threadIdx.x == 0) prof[(blockIdx.x * 2 + (blockIdx.y & 1)) * 16 + 15] = wall_clock64();
  if (threadIdx.x == 0) {
    H->n_pos[list] = n;
    H->cand_cnt[list] = fits ? ncand : 0;
    H->ties[list] = tie;
  }
  return fits ? ncand : 0;
}

// One block per (slot, list): nmsMax for the bottom lists, peakClustering
// for the side lists.  detectSideCandidates runs only when the frame's
// bottom candidate list for the feature is non-empty (:820-833); nmsMax makes
// at least one candidate from any non-empty point list, so "is any bottom
// key left after the TAIL_MASK filter" decides it.  k_tail records that per
// (slot, feature) in the slot header (LmSlotOut::bottom_kept) before k_nms
// runs, so a side block neither waits for the bottom block nor reads the
// bottom keys the bottom block overwrites with its staged candidates.
// <false>: lists of at most LM_NMS_CAP positives, in LDS.  <true>: the
// longer lists, in global scratch (for_overflow_pairs, launched after
// <false>).

template <bool GLOB>
DEV void nms_block(int bx, int list, const LmConst* __restrict__ Kp, int s0, unsigned long long* __restrict__ keys,
                   const int32_t* __restrict__ n_pos, const unsigned long long* __restrict__ tailmask,
                   unsigned long long* __restrict__ gscratch, int64_t gscratch_slot, LmSlotOut* __restrict__ hdr,
                   int32_t* __restrict__ err, long long* __restrict__ prof_b, long long* __restrict__ prof_s) {
  constexpr int ACAP = GLOB ? 1 : LM_NMS_CAP;  // LDS array sizes
  const LmConst& K = *Kp;
  const int slot = s0 + bx;
  const int feat = list & 1, side = list >> 1;  // feat: 0 paw, 1 snout
  LmSlotOut* H = hdr + slot;
  // 16-byte aligned: the sorts and the nmsMax sweep read them with ds_read_b128
  __shared__ __attribute__((aligned(16))) unsigned long long s_keys[ACAP];
  __shared__ __attribute__((aligned(16))) int s_assign[ACAP];
  __shared__ int s_mlist[ACAP];
  __shared__ __attribute__((aligned(16))) unsigned s_xy[ACAP + 16];
  __shared__ int s_tmp[LM_NMS_CAP];
  __shared__ int s_stk[GLOB ? lm_sort::kStackInts : 1];
  __shared__ int s_wsum[LM_NMS_THREADS / 64 + 1];
  __shared__ int s_n, s_flag, s_qcnt[2];
  __shared__ int s_part[2 * (LM_NMS_THREADS / 64) + 2];  // block_partition's counts + the small-range count
  static_assert(LM_NMS_RANKSORT * 8 <= LM_NMS_CAP * 4, "s_assign holds the sorts' keys");
  const int64_t npg = gscratch_slot / 3;
  // <true>: the launch's block b works its pairs one after another in scratch region b
  unsigned long long* ga = gscratch + (int64_t)(GLOB ? blockIdx.x : 0) * gscratch_slot;
  int* gassign = reinterpret_cast<int*>(ga + npg);
  int* gmlist = gassign + npg;
  const int n_in = n_pos[slot * LM_NLIST + list];
  if (side && slot < 1) return;  // the previous frame (halo slot): bottom lists only
  if (GLOB != (n_in > LM_NMS_CAP)) return;  // the other instantiation's list
  const int det = side ? (feat == 0 ? DET_PAW_S : DET_SNOUT_S) : (feat == 0 ? DET_PAW_B : DET_SNOUT_B);
  const LmDet D = K.det[det];
  if (side) {
    if (!H->bottom_kept[feat]) {  // set by k_tail from the keys before any block stages candidates over them
      if (threadIdx.x == 0) {  // detectSideCandidates not run: an empty side list
        H->n_pos[list] = 0;
        H->cand_cnt[list] = 0;
        H->ties[list] = 0;
      }
      return;
    }
  }
  long long* prof = side ? prof_s : prof_b;
  NMS_PROF(0)
  if (prof && threadIdx.x == 0) prof[(blockIdx.x * 2 + (blockIdx.y & 1)) * 16 + 14] = wall_clock64();
  const unsigned long long* __restrict__ src = keys + (int64_t)slot * K.keys_per_slot + K.list_off[list];
  if constexpr (!GLOB)
    nms_run<false>(K, D, H, slot, list, side, feat, n_in, src, tailmask, s_keys, s_assign, s_mlist, s_xy, s_tmp,
                   reinterpret_cast<unsigned long long*>(s_assign), LM_NMS_CAP / 6, s_stk, s_wsum, &s_n, &s_flag, s_qcnt, s_part,
                   keys, err, prof);
  else
    nms_run<true>(K, D, H, slot, list, side, feat, n_in, src, tailmask, ga, gassign, gmlist,
                  reinterpret_cast<unsigned*>(gmlist + npg), s_tmp, reinterpret_cast<unsigned long long*>(gassign), 0,
                  s_stk, s_wsum, &s_n, &s_flag, s_qcnt, s_part, keys, err, prof);
}

// For the <true> (global-scratch) instantiations of k_nms / k_post: a small
// grid finds the (slot, feature) pairs that need it — every thread tests one
// pair, so the usual "none" costs one round of header reads — and the blocks
// share them out.  fn(pair) runs block-wide.
template <class Pred, class Fn>
DEV void for_overflow_pairs(int npairs, Pred overflow, Fn fn) {
  // every block must see the same list in the same order (block b takes
  // entries b, b + gridDim.x, ...): an order-preserving compaction, not
  // atomics (whose order differs between blocks: pairs were skipped or run
  // twice when several overflowed)
  __shared__ int s_list[1024], s_wsum[1024 / 64 + 1];
  for (int c0 = 0; c0 < npairs; c0 += 1024) {
    const int cnt = block_compact(min(npairs - c0, 1024), [&](int j) { return overflow(c0 + j) ? 1 : 0; }, s_list,
                                  s_wsum);
    for (int i = blockIdx.x; i < cnt; i += gridDim.x) {
      fn(c0 + s_list[i]);
      __syncthreads();  // the next pair reuses the block's shared variables
    }
    __syncthreads();
  }
}

// <false>: one block per (slot, feature), lists of at most LM_NMS_CAP
// positives in LDS.  <true>: the longer lists, from global scratch, by a
// small grid that walks all npairs (slot, feature) pairs — usually none
// qualifies, so it costs a launch and a few header reads.  One kernel
// holding both paths ran the common one slower (register allocation).
// LM_KPROF=1: clock64() of thread 0 per k_post phase (LDS instantiation),
// 16 per (frame, feature) block; null otherwise
#define POST_PROF(k)                                                                           \
  if (!G && threadIdx.x == 0) {                                                                \
    long long* pp_ = prof;                                                                     \
    if (pp_) pp_[(blockIdx.x * 2 + blockIdx.y) * 16 + (k)] = (k) >= 14 ? wall_clock64() : clock64(); \
  }
template <bool GLOB>
__global__ __launch_bounds__(LM_NMS_THREADS) __attribute__((amdgpu_waves_per_eu(GLOB ? 1 : LM_NMS_WPE, 8))) void k_nms(const LmConst* __restrict__ Kp, int s0, unsigned long long* __restrict__ keys,
                                                       const int32_t* __restrict__ n_pos, const unsigned long long* __restrict__ tailmask,
                                                       unsigned long long* __restrict__ gscratch, int64_t gscratch_slot,
                                                       LmSlotOut* __restrict__ hdr, int32_t* __restrict__ err,
                                                       long long* __restrict__ prof_b, long long* __restrict__ prof_s,
                                                       int npairs) {
  if constexpr (!GLOB)
    nms_block<false>(blockIdx.x, blockIdx.y, Kp, s0, keys, n_pos, tailmask, gscratch, gscratch_slot, hdr, err, prof_b,
                     prof_s);
  else
    for_overflow_pairs(
        npairs,  // (slot, list) pairs
        [&](int p) {
          const int slot = s0 + (p >> 2), list = p & 3;
          return n_pos[slot * LM_NLIST + list] > LM_NMS_CAP && (slot >= 1 || list < 2);
        },
        [&](int p) {
          nms_block<true>(p >> 2, p & 3, Kp, s0, keys, n_pos, tailmask, gscratch, gscratch_slot, hdr, err, nullptr,
                          nullptr);
        });
#undef NMS_PROF
}

// ------------------------------------------------------------------ k_post
#ifndef LM_POST_THREADS
#define LM_POST_THREADS 256
#endif
#define LM_POST_MAXC 512     // candidates per list handled in LDS
#define LM_POST_MAXOFF 2048  // CSC columns (Ni + Nong) + 1

// checkVelCriterion (:1256-1267): sum(sat_u8(I - I_prev) > 25) >= area*alpha,
// by one whole wave (called with every lane active, arguments wave-uniform):
// the rectangle's pixels are shared out over the lanes and counted with a
// ballot per round, so a check costs a few dependent load chains
// (calibration -> frame -> LUT) instead of one per pixel.
template <class FP>
DEV bool vel_criterion_wave(const LmConst& K, FP Fc, FP Fp, const uint8_t* bkg, const int32_t* cal,
                            const uint8_t* lutc, const uint8_t* lutp, const LmSlot& slc, const LmSlot& slp, int crop_x,
                            int crop_y, int crop_w, int crop_h, int bx, int by, int bwid, int bhei, int area,
                            double alpha, int32_t* err, int tag) {
  const int lane = threadIdx.x & 63;
  if (bx < 0 || by < 0 || bwid < 0 || bhei < 0 || bx + bwid > crop_w || by + bhei > crop_h) {
    if (lane == 0) {
      atomicOr(err, 4);  // cv::Mat ROI assertion in the reference
      if (atomicCAS(&err[1], 0, 1) == 0) {  // first offender, for the error message
        err[2] = tag;
        err[3] = bx;
        err[4] = by;
        err[5] = bwid;
        err[6] = bhei;
        err[7] = crop_w;
        err[8] = crop_h;
      }
    }
    return false;
  }
  const int n = bwid * bhei;
  int sum = 0;
  for (int p0 = 0; p0 < n; p0 += 64) {
    const int p = p0 + lane;
    bool hit = false;
    if (p < n) {
      const int r = p / bwid, c = p - r * bwid;
      const int R = crop_y + by + r, C = crop_x + bx + c;
      const int a = ipad_pixel_t(Fc, bkg, cal, lutc, K, slc, R, C);  // I_*_MOUSE_PAD
      const int b = ipad_pixel_t(Fp, bkg, cal, lutp, K, slp, R, C);  // I_*_MOUSE_PAD_PREV
      hit = (a > b ? a - b : 0) > 25;
    }
    sum += __popcll(__ballot(hit));
  }
  return (double)sum >= ((double)area) * alpha;
}

// Bump allocation of `amount` entries of arena k from sub-arena g (one
// thread): the offset, or -1 with the overflow flag set.
DEV int arena_alloc(LmArenaCtl* __restrict__ ctl, int k, int g, int amount) {
  const int part = ctl->cap[k] / ctl->nparts;
  const int b = atomicAdd(&ctl->sub[g][k], amount);
  if (b + amount > part) {
    atomicOr(&ctl->overflow, 1);
    return -1;
  }
  return g * part + b;
}

// The body of k_post on its working arrays: candidate copies and per-list
// state in LDS (G = false), or, for lists beyond the LDS capacity, the staged
// candidate lists themselves and per-block global scratch (G = true; the
// reference has no size limit).  Two instantiations, so the common case stays
// on ds_* instructions.
template <bool G>
DEV void post_run(const LmConst& K, const LmSlot* __restrict__ slots, const uint8_t* const* __restrict__ frame_ptr,
                  const uint8_t* __restrict__ bkg, const int32_t* __restrict__ cal, const uint8_t* __restrict__ luts,
                  LmSlotOut* H, int slot, int feat, int frame, int Nb, int Ns, int Ni, const LmCand* sb,
                  const LmCand* st, const LmCand* sp, int* s_off, int* s_mb, int* s_mt, float* s_bps, float* s_tpb,
                  int cap, int* s_base, int& s_any1, int& s_any0, LmP22D* __restrict__ arena_p22d,
                  int32_t* __restrict__ arena_side_y, double* __restrict__ arena_side_s, double* __restrict__ arena_unary,
                  int32_t* __restrict__ arena_jc, int32_t* __restrict__ arena_ir, double* __restrict__ arena_pr,
                  LmArenaCtl* __restrict__ ctl, int32_t* __restrict__ err, int sub,
                  long long* __restrict__ prof) {
  POST_PROF(14)
  POST_PROF(0)
  // ---------------- unary (unaryCostBox :1909-1952), column-major Nb x nprior
  const int nprior = feat == 0 ? 4 : 1;
  const int p0 = feat == 0 ? 0 : 4;
  if (threadIdx.x == 0) {
    s_base[0] = arena_alloc(ctl, AR_UNARY, sub, Nb * nprior);
  }
  __syncthreads();
  if (s_base[0] >= 0) {
    const double norm_fact = 1 / sqrt(2.0);
    for (int e = threadIdx.x; e < Nb * nprior; e += blockDim.x) {
      const int j = e / Nb, i = e % Nb;  // column-major: values[j*nrows + i]
      const double* pr = K.prior[p0 + j];
      const double cx = (double)sb[i].x / (double)K.bb_bottom_w, cy = (double)sb[i].y / (double)K.bb_bottom_h;
      const double ax = pr[3], aw = pr[4] - pr[3], ay = pr[5], ah = pr[6] - pr[5];
      double v = 0.0;
      if (ax <= cx && cx < ax + aw && ay <= cy && cy < ay + ah) {
        const double dx = cx - pr[0], dy = cy - pr[1];
        const double dd = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        const double val = sqrt(dd) * norm_fact;
        if (val <= pr[2]) v = (1 - val) * sb[i].s;
      }
      arena_unary[s_base[0] + e] = v;
    }
  }
  if (threadIdx.x == 0) {
    H->unary_off[feat] = s_base[0];
    H->unary_cnt[feat] = Nb * nprior;
  }

  POST_PROF(1)
  // ---------------- pairwise (pairwisePotential :1954-2070) when frame > 0
  if (frame > 0) {
    const int Nong = K.ong_nx * K.ong_ny;
    const int ncols = Ni + Nong, nrows = Nb + Nong;
    const double gs = (double)K.ong_spacing_bottom, maxd = (double)K.max_displacement_bottom;
    const double alpha = K.alpha_vel_bottom, occ = K.pairwise_occluded_cost * alpha;
    auto ong_of = [&](const LmCand& c) {
      const int xc = (int)round((K.ong_br_x - (double)c.x) / gs);
      const int yc = (int)round((K.ong_br_y - (double)c.y) / gs);
      const int ox = xc < 0 ? 0 : (xc > K.ong_nx - 1 ? K.ong_nx - 1 : xc);
      const int oy = yc < 0 ? 0 : (yc > K.ong_ny - 1 ? K.ong_ny - 1 : yc);
      return oy * K.ong_nx + ox;
    };
    auto trans = [&](int i, int j) {  // D(j, i) candidate -> candidate
      const double dx = (double)sb[j].x - (double)sp[i].x, dy = (double)sb[j].y - (double)sp[i].y;
      const double dist = sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
      if (!(dist < maxd)) return 0.0;
      double inv = 1 - (dist / maxd);
      return inv * alpha;
    };
    // each bottom candidate's ONG node once (s_mb is free until the matching)
    int* s_ong = s_mb;
    for (int j = threadIdx.x; j < Nb; j += blockDim.x) s_ong[j] = ong_of(sb[j]);
    __syncthreads();
    // column counts -> Jc
    for (int c = threadIdx.x; c < ncols; c += blockDim.x) {
      int cnt = 0;
      if (c < Ni) {
        for (int j = 0; j < Nb; ++j) cnt += trans(c, j) != 0.0;
        cnt += occ != 0.0;
      } else {
        const int q = c - Ni;
        if (Ni > 0 && occ != 0.0)
          for (int j = 0; j < Nb; ++j) cnt += s_ong[j] == q;
        cnt += occ != 0.0;
      }
      s_off[c] = cnt;
    }
    __syncthreads();
    // exclusive scan of the counts by the first wave, 64 columns a round
    if (threadIdx.x < 64) {
      const int lane = threadIdx.x;
      int carry = 0;
      for (int c0 = 0; c0 < ncols; c0 += 64) {
        const int c = c0 + lane;
        const int t = c < ncols ? s_off[c] : 0;
        int v = t;  // inclusive wave scan
        for (int o = 1; o < 64; o <<= 1) {
          const int u = __shfl_up(v, o);
          if (lane >= o) v += u;
        }
        if (c < ncols) s_off[c] = carry + v - t;
        carry += __shfl(v, 63);
      }
      if (lane == 0) s_off[ncols] = carry;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int acc = s_off[ncols];
      const int bj = arena_alloc(ctl, AR_PWJC, sub, ncols + 1);
      const int bn = arena_alloc(ctl, AR_PWNZ, sub, acc);
      s_base[1] = bn < 0 ? -1 : bj;
      s_base[2] = bn;
    }
    __syncthreads();
    POST_PROF(2)
    const int bj = s_base[1], bn = s_base[2];
    if (bj >= 0) {
      for (int c = threadIdx.x; c <= ncols; c += blockDim.x) arena_jc[bj + c] = s_off[c];
      for (int c = threadIdx.x; c < ncols; c += blockDim.x) {
        int o = bn + s_off[c];
        if (c < Ni) {
          for (int j = 0; j < Nb; ++j) {
            const double v = trans(c, j);
            if (v != 0.0) {
              arena_ir[o] = j;
              arena_pr[o] = v;
              ++o;
            }
          }
          if (occ != 0.0) {
            arena_ir[o] = Nb + ong_of(sp[c]);
            arena_pr[o] = occ;
            ++o;
          }
        } else {
          const int q = c - Ni;
          if (Ni > 0 && occ != 0.0)
            for (int j = 0; j < Nb; ++j)
              if (s_ong[j] == q) {
                arena_ir[o] = j;
                arena_pr[o] = occ;
                ++o;
              }
          if (occ != 0.0) {
            arena_ir[o] = Nb + q;
            arena_pr[o] = occ;
            ++o;
          }
        }
      }
    }
    if (threadIdx.x == 0) {
      H->pw_rows[feat] = nrows;
      H->pw_cols[feat] = ncols;
      H->pw_nnz[feat] = s_off[ncols];
      H->pw_jc_off[feat] = bj;
      H->pw_nz_off[feat] = bn;
    }
    __syncthreads();
  } else if (threadIdx.x == 0) {
    H->pw_rows[feat] = -1;
    H->pw_cols[feat] = -1;
    H->pw_nnz[feat] = 0;
    H->pw_jc_off[feat] = 0;
    H->pw_nz_off[feat] = 0;
  }

  POST_PROF(3)
  // ---------------- matching (:1023-1254)
  const int ovlp = (int)(K.size_b[feat][0] * (1 - K.side_bottom_min_overlap));
  const bool vel_check = frame > 0;
  if (threadIdx.x == 0) {
    s_any1 = 0;
    s_any0 = 0;
  }
  for (int k = threadIdx.x; k < cap; k += blockDim.x) {
    s_mb[k] = -1;
    s_mt[k] = -1;
    s_bps[k] = 0.f;
    s_tpb[k] = 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < Nb * Ns; e += blockDim.x) {
    const int i = e / Ns, j = e % Ns;
    if (abs(sb[i].x - st[j].x) <= ovlp) s_any1 = 1;
    else s_any0 = 1;
  }
  __syncthreads();
  const bool mixed = s_any1 && s_any0;  // normalize(NORM_MINMAX) all-equal -> all 0 (:1065)
  auto boolD = [&](int i, int j) { return mixed && abs(sb[i].x - st[j].x) <= ovlp; };
  for (int j = threadIdx.x; j < Ns; j += blockDim.x) {
    float s = 0.f;
    for (int i = 0; i < Nb; ++i) s += boolD(i, j) ? 1.f : 0.f;
    s_bps[j] = s;
  }
  for (int i = threadIdx.x; i < Nb; i += blockDim.x) {
    float s = 0.f;
    for (int j = 0; j < Ns; ++j) s += boolD(i, j) ? 1.f : 0.f;
    s_tpb[i] = s;
  }
  __syncthreads();
  POST_PROF(4)
  // motion status where the reference evaluates it
  const LmSlot sl = slots[slot], slp = slots[slot - 1];
  const lm_gu8* Fc = as_global(frame_ptr[slot]);
  const lm_gu8* Fp = as_global(frame_ptr[slot - 1]);
  const uint8_t* lutc = luts + slot * 256;
  const uint8_t* lutp = luts + (slot - 1) * 256;
  const int* mbox = K.match_b[feat];
  const int* tbox = K.match_s[feat];
  if (vel_check) {
    // which candidates the reference tests (-2: pending), then one wave per test
    for (int i = threadIdx.x; i < Nb; i += blockDim.x) {
      bool need = false;
      for (int j = 0; j < Ns; ++j) need |= boolD(i, j) && s_bps[j] > 1;
      if (need) s_mb[i] = -2;
    }
    for (int j = threadIdx.x; j < Ns; j += blockDim.x) {
      bool need = false;
      if (s_bps[j] > 1)
        for (int i = 0; i < Nb; ++i) need |= boolD(i, j);
      if (need) s_mt[j] = -2;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int k = wid; k < Nb + Ns; k += nw) {
      if (k < Nb) {
        const int i = k;
        if (s_mb[i] != -2) continue;
        const bool m = vel_criterion_wave(K, Fc, Fp, bkg, cal, lutc, lutp, sl, slp, sl.crop_x[0], sl.crop_y[0], K.crop_w[0],
                                          K.crop_h[0], mbox[0] + sb[i].x + K.spre_b_w, mbox[1] + sb[i].y + K.spre_b_h,
                                          mbox[2], mbox[3], K.size_b[feat][0] * K.size_b[feat][1], 0.02, err,
                                          (slot << 16) | (feat << 12) | i);
        if (lane == 0) s_mb[i] = m;
      } else {
        const int j = k - Nb;
        if (s_mt[j] != -2) continue;
        const bool m = vel_criterion_wave(K, Fc, Fp, bkg, cal, lutc, lutp, sl, slp, sl.crop_x[1], sl.crop_y[1], K.crop_w[1],
                                          K.crop_h[1], tbox[0] + st[j].x + K.spre_t_w, tbox[1] + st[j].y + K.spre_t_h,
                                          tbox[2], tbox[3], K.size_s[feat][0] * K.size_s[feat][1], 0.05, err,
                                          (slot << 16) | (feat << 12) | 0x800 | j);
        if (lane == 0) s_mt[j] = m;
      }
    }
  }
  __syncthreads();
  POST_PROF(5)
  const double walpha = -(1. / (double)ovlp);
  auto matches = [&](int i, int j) {
    if (!boolD(i, j)) return false;
    if ((s_bps[j] > 1) & vel_check) return s_mb[i] == s_mt[j];
    return true;
  };
  // side entries per bottom candidate (>= 1: the "no match" entry)
  for (int i = threadIdx.x; i < Nb; i += blockDim.x) {
    int cnt = 0;
    if (Ns > 0 && s_tpb[i] != 0)
      for (int j = 0; j < Ns; ++j) cnt += matches(i, j);
    s_off[i] = cnt > 0 ? cnt : 1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int i = 0; i < Nb; ++i) {
      const int t = s_off[i];
      s_off[i] = acc;
      acc += t;
    }
    s_off[Nb] = acc;
    const int bp = arena_alloc(ctl, AR_P22D, sub, Nb);
    const int bs = arena_alloc(ctl, AR_SIDE, sub, acc);
    s_base[0] = bs < 0 ? -1 : bp;
    s_base[1] = bs;
  }
  __syncthreads();
  const int bp = s_base[0], bs = s_base[1];
  if (bp >= 0) {
    for (int i = threadIdx.x; i < Nb; i += blockDim.x) {
      const int o = bs + s_off[i];
      int cnt = 0;
      double st0 = -1;
      if (Ns > 0 && s_tpb[i] != 0) {
        for (int j = 0; j < Ns; ++j) {
          if (!matches(i, j)) continue;
          const double wgt = __dadd_rn(__dmul_rn((double)abs(sb[i].x - st[j].x), walpha), 1.0);
          const double sv = st[j].s * wgt;
          // P22D(C_b, C_temp) then add_side_candidate (Candidates.cpp:106-115)
          if (cnt == 0) {
            arena_side_y[o] = st[j].y;
            arena_side_s[o] = sv;
            st0 = sv;
            cnt = 1;
          } else if (st0 < 0) {
            arena_side_y[o] = st[j].y;
            arena_side_s[o] = sv;
            st0 = sv;
          } else {
            if (!(sv >= 0)) atomicOr(err, 16);  // CV_Assert(S >= 0)
            arena_side_y[o + cnt] = st[j].y;
            arena_side_s[o + cnt] = sv;
            ++cnt;
          }
        }
      }
      if (cnt == 0) {
        arena_side_y[o] = -1;  // Candidate(-1, -1, -1)
        arena_side_s[o] = -1;
        cnt = 1;
      }
      LmP22D p;
      p.bottom = sb[i];
      p.side_off = o;
      p.side_cnt = cnt;
      arena_p22d[bp + i] = p;
    }
  }
  POST_PROF(6)
  POST_PROF(15)
  if (threadIdx.x == 0) {
    H->p22d_off[feat] = bp;
    H->p22d_cnt[feat] = Nb;
    H->side_off[feat] = bs;
    H->side_cnt[feat] = s_off[Nb];
  }
}


// Two instantiations, launched back to back on the same grid: <false> takes
// the (slot, feature) blocks whose lists fit the LDS arrays, <true> the rest
// (global scratch).  One kernel holding both paths ran the common one 60 %
// slower (register allocation and code layout of the larger body).
#define LM_POST_ARGS                                                                                               \
  const LmConst *__restrict__ Kp, const LmSlot *__restrict__ slots, const uint8_t *const *__restrict__ frame_ptr,  \
      const uint8_t *__restrict__ bkg, const int32_t *__restrict__ cal, const uint8_t *__restrict__ luts,           \
      LmSlotOut *__restrict__ hdr, const unsigned long long *__restrict__ keys, LmP22D *__restrict__ arena_p22d,    \
      int32_t *__restrict__ arena_side_y, double *__restrict__ arena_side_s, double *__restrict__ arena_unary,      \
      int32_t *__restrict__ arena_jc, int32_t *__restrict__ arena_ir, double *__restrict__ arena_pr,                \
      LmArenaCtl *__restrict__ ctl, int32_t *__restrict__ err, unsigned long long *__restrict__ gscratch,          \
      int64_t gscratch_slot, long long *__restrict__ prof
#define LM_POST_PASS                                                                                                \
  Kp, slots, frame_ptr, bkg, cal, luts, hdr, keys, arena_p22d, arena_side_y, arena_side_s, arena_unary, arena_jc,    \
      arena_ir, arena_pr, ctl, err, gscratch, gscratch_slot, prof
template <bool GLOB>
DEV void post_block(int bx, int feat, LM_POST_ARGS) {
  const LmConst& K = *Kp;
  const int slot = 1 + bx;
  LmSlotOut* H = hdr + slot;
  const LmSlotOut* HP = hdr + slot - 1;
  const int frame = slots[slot].frame;
  __shared__ int s_any1, s_any0, s_base[4];
  const int Nb = H->cand_cnt[feat], Ns = H->cand_cnt[2 + feat];
  const int Ni = frame > 0 ? HP->cand_cnt[feat] : 0;
  const int Nong = K.ong_nx * K.ong_ny;
  const LmCand* cb = LM_CAND_STAGE(K, keys, slot, feat);
  const LmCand* ct = LM_CAND_STAGE(K, keys, slot, 2 + feat);
  const LmCand* cp = LM_CAND_STAGE(K, keys, slot - 1, feat);
  const bool fits = Nb <= LM_POST_MAXC && Ns <= LM_POST_MAXC && Ni <= LM_POST_MAXC && Ni + Nong + 1 <= LM_POST_MAXOFF;
  if (fits == GLOB) return;  // the other instantiation's block
  if constexpr (!GLOB) {
    __shared__ LmCand sb[LM_POST_MAXC], st[LM_POST_MAXC], sp[LM_POST_MAXC];
    __shared__ int s_off[LM_POST_MAXOFF];
    __shared__ int s_mb[LM_POST_MAXC], s_mt[LM_POST_MAXC];  // motion status (-1 unknown)
    __shared__ float s_bps[LM_POST_MAXC], s_tpb[LM_POST_MAXC];
    for (int k = threadIdx.x; k < Nb; k += blockDim.x) sb[k] = cb[k];
    for (int k = threadIdx.x; k < Ns; k += blockDim.x) st[k] = ct[k];
    for (int k = threadIdx.x; k < Ni; k += blockDim.x) sp[k] = cp[k];
    __syncthreads();
    post_run<false>(K, slots, frame_ptr, bkg, cal, luts, H, slot, feat, frame, Nb, Ns, Ni, sb, st, sp, s_off, s_mb, s_mt,
                    s_bps, s_tpb, LM_POST_MAXC, s_base, s_any1, s_any0, arena_p22d, arena_side_y, arena_side_s,
                    arena_unary, arena_jc, arena_ir, arena_pr, ctl, err, (2 * bx + feat) % ctl->nparts, prof);
  } else {  // long lists, in the block's global scratch region
    const int big = max(max(Nb, Ns), Ni);
    // the launch's block b works its pairs one after another in scratch region b
    int* g = reinterpret_cast<int*>(gscratch + (int64_t)blockIdx.x * gscratch_slot);
    int* g_off = g;                      // max(Ni + Nong, Nb) + 1
    int* g_mb = g_off + max(Ni + Nong, Nb) + 1;
    int* g_mt = g_mb + big;
    float* g_bps = reinterpret_cast<float*>(g_mt + big);
    float* g_tpb = g_bps + big;
    if ((int64_t)(reinterpret_cast<int*>(g_tpb + big) - g) > 2 * gscratch_slot) {  // the host sizes the scratch for it
      if (threadIdx.x == 0) atomicOr(err, 8);
      return;
    }
    post_run<true>(K, slots, frame_ptr, bkg, cal, luts, H, slot, feat, frame, Nb, Ns, Ni, cb, ct, cp, g_off, g_mb, g_mt,
                   g_bps, g_tpb, big, s_base, s_any1, s_any0, arena_p22d, arena_side_y, arena_side_s, arena_unary,
                   arena_jc, arena_ir, arena_pr, ctl, err, (2 * bx + feat) % ctl->nparts, prof);
  }
}

// <false>: one block per (slot, feature) whose lists fit the LDS arrays;
// <true>: the others, from global scratch, by a small grid walking all npairs
// (slot, feature) pairs (usually none).  Kept apart: one kernel holding both
// paths ran the common one 60 % slower.
template <bool GLOB>
__global__ __launch_bounds__(LM_POST_THREADS) void k_post(LM_POST_ARGS, int npairs) {
  if constexpr (!GLOB)
    post_block<false>(blockIdx.x, blockIdx.y, LM_POST_PASS);
  else
    for_overflow_pairs(
        npairs,
        [&](int p) {
          const int slot = 1 + (p >> 1), feat = p & 1;
          const LmSlotOut* H = hdr + slot;
          const int Nb = H->cand_cnt[feat], Ns = H->cand_cnt[2 + feat];
          const int Ni = slots[slot].frame > 0 ? hdr[slot - 1].cand_cnt[feat] : 0;
          return !(Nb <= LM_POST_MAXC && Ns <= LM_POST_MAXC && Ni <= LM_POST_MAXC &&
                   Ni + Kp->ong_nx * Kp->ong_ny + 1 <= LM_POST_MAXOFF);
        },
        [&](int p) { post_block<true>(p >> 1, p & 1, LM_POST_PASS); });
}

// ----------------------------------------------------------------- k_carry
// Copies the bottom candidate lists of the last slot of the previous batch
// (frame first-1) into slot 0's candidate staging, where k_post reads the
// previous frame's candidates (pairwisePotential, :896-919).  Runs first in a
// batch, before k_corr reuses the key areas of slots >= 1.
// k_carry (block 1 of k_prep's launch when the batch continues the lane's
// last one): the previous batch's last frame's bottom candidates into slot 0.
DEV void carry_block(const LmConst& K, unsigned long long* __restrict__ keys, const LmSlotOut* __restrict__ prev_hdr,
                     int prev_slot, LmSlotOut* __restrict__ hdr) {
  for (int l = 0; l < LM_NFEAT; ++l) {
    const int cnt = prev_hdr[prev_slot].cand_cnt[l];
    const LmCand* src = LM_CAND_STAGE(K, keys, prev_slot, l);
    LmCand* dst = LM_CAND_STAGE(K, keys, 0, l);
    for (int k = threadIdx.x; k < cnt; k += blockDim.x) dst[k] = src[k];
    if (threadIdx.x == 0) hdr[0].cand_cnt[l] = cnt;
  }
}

// ------------------------------------------------------------- k_prep / k_out
// The batch's only transfers between host and device memory are done by these
// two kernels through mapped pinned host memory, so a batch's stream holds
// nothing but kernels: 5 runtime copies/memsets and a second stream sync per
// batch are gone (the header and the packed results land in host memory in
// the same pass, the host reads them after one hipStreamSynchronize).
//
// k_prep: slots, frame pointers and the arena control block from host memory,
// candidate counters and error flags zeroed.  One block.
static_assert(4 * LM_TL_NC == 256 && 2 * LM_NLIST * LM_TL_NC == 512, "k_prep zeroes the tile-list counters with its 256 threads");
__global__ __launch_bounds__(256) void k_prep(const LmSlot* __restrict__ h_slots, const uint8_t* const* __restrict__ h_fptr,
                                              const LmArenaCtl* __restrict__ h_ctl, int ns, LmSlot* __restrict__ slots,
                                              const uint8_t** __restrict__ fptr, LmArenaCtl* __restrict__ ctl,
                                              int32_t* __restrict__ npos, int32_t* __restrict__ err,
                                              const LmConst* __restrict__ Kp, unsigned long long* __restrict__ keys,
                                              const LmSlotOut* __restrict__ prev_hdr, int prev_slot,
                                              LmSlotOut* __restrict__ hdr, int32_t* __restrict__ dark_cnt,
                                              int32_t* __restrict__ tail_cnt, int32_t* __restrict__ pt_cnt,
                                              int32_t* __restrict__ nw_cnt) {
  if (blockIdx.x == 1) {
    carry_block(*Kp, keys, prev_hdr, prev_slot, hdr);
    return;
  }
  if (dark_cnt) dark_cnt[threadIdx.x] = 0;  // k_ingest's bright-tile counters (4 LM_TL_NC = blockDim.x)
  if (tail_cnt && threadIdx.x < 2 * LM_TL_NC) tail_cnt[threadIdx.x] = 0;  // k_tile_bound's tail-tile counters
  if (pt_cnt) {  // and its point-tile counters (listed and bright tiles per detector)
    pt_cnt[threadIdx.x] = 0;
    pt_cnt[256 + threadIdx.x] = 0;
  }
  if (nw_cnt) {  // and the counters of its narrow and wide lists (lm_corr_narrow.h)
    static_assert(LM_NW_CNT_WORDS == 3 * 256, "k_prep zeroes the narrow / wide counters with its 256 threads");
    for (int i = 0; i < 3; ++i) nw_cnt[256 * i + threadIdx.x] = 0;
  }
  for (int i = threadIdx.x; i < ns; i += blockDim.x) {
    slots[i] = h_slots[i];
    fptr[i] = h_fptr[i];
  }
  for (int i = threadIdx.x; i < ns * LM_NLIST; i += blockDim.x) npos[i] = 0;
  if (threadIdx.x < 16) err[threadIdx.x] = 0;
  if (threadIdx.x < AR_COUNT) {
    ctl->used[threadIdx.x] = h_ctl->used[threadIdx.x];
    ctl->cap[threadIdx.x] = h_ctl->cap[threadIdx.x];
  }
  if (threadIdx.x == 0) {
    ctl->overflow = h_ctl->overflow;
    ctl->nparts = h_ctl->nparts;
    ctl->pack_dst = h_ctl->pack_dst;
    ctl->pack_cap = h_ctl->pack_cap;
  }
  for (int i = threadIdx.x; i < LM_SUBARENA * 32; i += blockDim.x) (&ctl->sub[0][0])[i] = 0;
}

// k_out: the pack header always, and when the batch succeeded and its packed
// results fit the host buffer, the results themselves -> mapped pinned host
// memory; then the next batch's previous frame (storePreviousImage,
// LocoMouse_class.cpp:1508-1513) -> the halo buffer.  Packed sizes and frame
// sizes are multiples of 16 bytes.
// h_pack == nullptr: the destination and its size are the batch's, in ctl
// (k_prep copied them from the lane's mapped control block).
__global__ __launch_bounds__(256) void k_out(const LmPackHdr* __restrict__ ph, LmPackHdr* __restrict__ h_ph,
                                             const uint8_t* __restrict__ pack, uint8_t* __restrict__ h_pack, int64_t h_cap,
                                             const LmArenaCtl* __restrict__ ctl,
                                             const uint8_t* __restrict__ halo_arg, const uint8_t* const* __restrict__ fptr,
                                             int fidx, uint8_t* __restrict__ halo_dst, int64_t halo_bytes) {
  if (!h_pack && ctl) {
    h_pack = ctl->pack_dst;
    h_cap = ctl->pack_cap;
  }
  // halo source: halo_arg, else the batch's frame pointer fptr[fidx] (device
  // array written by k_prep, so a captured graph replays with fresh frames)
  const uint8_t* __restrict__ halo_src = halo_arg ? halo_arg : (fptr ? fptr[fidx] : nullptr);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  if (tid == 0) *h_ph = *ph;
  const int64_t bytes = ph->bytes;
  if (ph->overflow || ph->err || bytes > h_cap) return;
  for (int64_t i = tid; i < bytes / 16; i += nth)
    reinterpret_cast<uint4*>(h_pack)[i] = reinterpret_cast<const uint4*>(pack)[i];
  if (halo_src) {
    for (int64_t i = tid; i < halo_bytes / 16; i += nth)
      reinterpret_cast<uint4*>(halo_dst)[i] = reinterpret_cast<const uint4*>(halo_src)[i];
    for (int64_t i = halo_bytes / 16 * 16 + tid; i < halo_bytes; i += nth) halo_dst[i] = halo_src[i];
  }
}

// ------------------------------------------------------------------ k_pack
// Packs the batch's results into lm_batch_result's layout (frame order) in one
// buffer: k_pack_scan computes every offset array (exclusive scans over the
// frames) and the totals, k_pack_copy moves each (frame, feature)'s data.
// Unit = one batch; a few KB per frame, launch-latency bound.
// All six offset arrays in one pass: each thread takes a contiguous run of
// frames, sums its frames' counts per array, one block-wide exclusive scan of
// the six sums (one pair of barriers instead of six), then the thread writes
// its frames' per-list offsets.  (Six scans one after the other cost six
// dependent load + barrier rounds: ~19 us per batch, launch-latency bound.)
__global__ __launch_bounds__(1024) void k_pack_scan(const LmSlotOut* __restrict__ hdr, int n,
                                                    const LmArenaCtl* __restrict__ ctl, const int32_t* __restrict__ err,
                                                    LmPackHdr* __restrict__ ph, uint8_t* __restrict__ pack, int64_t pack_cap,
                                                    int64_t* __restrict__ side_base) {
  constexpr int NA = 6;  // cand, p22d, unary, jc, nz, side
  __shared__ int64_t s_w[1024 / 64 + 1][NA];
  const int64_t zero[PK_COUNT] = {0, 0, 0, 0, 0, 0};
  const LmPackLayout L0 = lm_pack_layout(n, zero);  // offset arrays do not depend on the totals
  const LmSlotOut* H = hdr + 1;
  int64_t* outs[NA] = {reinterpret_cast<int64_t*>(pack + L0.cand_off), reinterpret_cast<int64_t*>(pack + L0.p22d_off),
                       reinterpret_cast<int64_t*>(pack + L0.unary_off), reinterpret_cast<int64_t*>(pack + L0.jc_off),
                       reinterpret_cast<int64_t*>(pack + L0.nz_off), side_base};
  const int per[NA] = {4, 2, 2, 2, 2, 2};  // entries per frame
  // count of array a, entry j of frame f
  auto count = [&](const LmSlotOut& h, int a, int j) -> int64_t {
    switch (a) {
      case 0: return h.cand_cnt[j];
      case 1: return h.p22d_cnt[j];
      case 2: return h.unary_cnt[j];
      case 3: return h.pw_rows[j] >= 0 ? (int64_t)h.pw_cols[j] + 1 : 0;
      case 4: return h.pw_rows[j] >= 0 ? (int64_t)h.pw_nnz[j] : 0;
      default: return h.side_cnt[j];
    }
  };
  const int T = blockDim.x, chunk = (n + T - 1) / T;
  const int f0 = threadIdx.x * chunk, f1 = min(n, f0 + chunk);
  int64_t c[NA] = {0, 0, 0, 0, 0, 0};
  for (int f = f0; f < f1; ++f) {
    const LmSlotOut& h = H[f];
#pragma unroll
    for (int a = 0; a < NA; ++a)
      for (int j = 0; j < per[a]; ++j) c[a] += count(h, a, j);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int64_t v[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    v[a] = c[a];
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t u = __shfl_up(v[a], o);
      if (lane >= o) v[a] += u;
    }
  }
  if (lane == 63)
#pragma unroll
    for (int a = 0; a < NA; ++a) s_w[wid][a] = v[a];
  __syncthreads();
  if (threadIdx.x < NA) {
    const int a = threadIdx.x;
    int64_t acc = 0;
    for (int w = 0; w < (T >> 6); ++w) {
      const int64_t t = s_w[w][a];
      s_w[w][a] = acc;
      acc += t;
    }
    s_w[T >> 6][a] = acc;
  }
  __syncthreads();
  int64_t r[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) r[a] = s_w[wid][a] + v[a] - c[a];
  for (int f = f0; f < f1; ++f) {
    const LmSlotOut& h = H[f];
#pragma unroll
    for (int a = 0; a < NA; ++a)
      for (int j = 0; j < per[a]; ++j) {
        outs[a][per[a] * f + j] = r[a];
        r[a] += count(h, a, j);
      }
  }
  if (threadIdx.x < NA) outs[threadIdx.x][per[threadIdx.x] * n] = s_w[T >> 6][threadIdx.x];
  // the sub-arena counts, one load per thread (a serial loop over them by one
  // thread waited out 6 x 16 dependent L2 round trips)
  __shared__ int s_sub[AR_COUNT][LM_SUBARENA];
  const int nparts = ctl->nparts;
  if (threadIdx.x < AR_COUNT * LM_SUBARENA) {
    const int k = threadIdx.x / LM_SUBARENA, g = threadIdx.x % LM_SUBARENA;
    s_sub[k][g] = g < nparts ? ctl->sub[g][k] : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t tot[PK_COUNT];
    tot[PK_CAND] = s_w[T >> 6][0];
    tot[PK_P22D] = s_w[T >> 6][1];
    tot[PK_UNARY] = s_w[T >> 6][2];
    tot[PK_JC] = s_w[T >> 6][3];
    tot[PK_NZ] = s_w[T >> 6][4];
    tot[PK_SIDE] = s_w[T >> 6][5];
    const LmPackLayout L = lm_pack_layout(n, tot);
    for (int k = 0; k < PK_COUNT; ++k) ph->tot[k] = tot[k];
    ph->bytes = L.bytes;
    ph->overflow = (L.bytes > pack_cap ? 1 : 0) | (ctl->overflow ? 2 : 0);
    ph->err = *err;
    for (int k = 0; k < AR_COUNT; ++k) {
      int m = 0;
      for (int g = 0; g < LM_SUBARENA; ++g) m = max(m, s_sub[k][g]);
      ph->used[k] = m * nparts;
    }
  }
}

__global__ __launch_bounds__(256) void k_pack_copy(const LmConst* __restrict__ Kp, const LmSlotOut* __restrict__ hdr, int n,
                                                   const unsigned long long* __restrict__ keys,
                                                   const LmP22D* __restrict__ arena_p22d, const int32_t* __restrict__ arena_side_y,
                                                   const double* __restrict__ arena_side_s, const double* __restrict__ arena_unary,
                                                   const int32_t* __restrict__ arena_jc, const int32_t* __restrict__ arena_ir,
                                                   const double* __restrict__ arena_pr, const LmPackHdr* __restrict__ ph,
                                                   uint8_t* __restrict__ pack, const int64_t* __restrict__ side_base) {
  const LmConst& K = *Kp;
  if (ph->overflow || ph->err) return;  // the host raises or reruns; offsets may be garbage
  const int f = blockIdx.x, feat = blockIdx.y, slot = 1 + f;
  const LmSlotOut& H = hdr[slot];
  int64_t tot[PK_COUNT];
  for (int k = 0; k < PK_COUNT; ++k) tot[k] = ph->tot[k];
  const LmPackLayout L = lm_pack_layout(n, tot);
  const int64_t* cand_off = reinterpret_cast<const int64_t*>(pack + L.cand_off);
  const int64_t* p22d_off = reinterpret_cast<const int64_t*>(pack + L.p22d_off);
  const int64_t* unary_off = reinterpret_cast<const int64_t*>(pack + L.unary_off);
  const int64_t* jc_off = reinterpret_cast<const int64_t*>(pack + L.jc_off);
  const int64_t* nz_off = reinterpret_cast<const int64_t*>(pack + L.nz_off);
  LmCand* cand = reinterpret_cast<LmCand*>(pack + L.cand);
  for (int l = feat; l < LM_NLIST; l += 2) {
    const LmCand* src = LM_CAND_STAGE(K, keys, slot, l);
    LmCand* dst = cand + cand_off[4 * f + l];
    for (int k = threadIdx.x; k < H.cand_cnt[l]; k += blockDim.x) dst[k] = src[k];
  }
  const int q = 2 * f + feat;
  const int64_t sb = side_base[q];
  LmP22D* p22d = reinterpret_cast<LmP22D*>(pack + L.p22d) + p22d_off[q];
  for (int k = threadIdx.x; k < H.p22d_cnt[feat]; k += blockDim.x) {
    LmP22D v = arena_p22d[H.p22d_off[feat] + k];
    v.side_off = (int32_t)(sb + (v.side_off - H.side_off[feat]));
    p22d[k] = v;
  }
  int32_t* side_y = reinterpret_cast<int32_t*>(pack + L.side_y) + sb;
  double* side_s = reinterpret_cast<double*>(pack + L.side_s) + sb;
  for (int k = threadIdx.x; k < H.side_cnt[feat]; k += blockDim.x) {
    side_y[k] = arena_side_y[H.side_off[feat] + k];
    side_s[k] = arena_side_s[H.side_off[feat] + k];
  }
  double* unary = reinterpret_cast<double*>(pack + L.unary) + unary_off[q];
  for (int k = threadIdx.x; k < H.unary_cnt[feat]; k += blockDim.x) unary[k] = arena_unary[H.unary_off[feat] + k];
  int32_t* dims = reinterpret_cast<int32_t*>(pack + L.pw_dims) + 3 * q;
  if (H.pw_rows[feat] >= 0) {
    int32_t* jc = reinterpret_cast<int32_t*>(pack + L.jc) + jc_off[q];
    int32_t* ir = reinterpret_cast<int32_t*>(pack + L.ir) + nz_off[q];
    double* pr = reinterpret_cast<double*>(pack + L.pr) + nz_off[q];
    for (int k = threadIdx.x; k <= H.pw_cols[feat]; k += blockDim.x) jc[k] = arena_jc[H.pw_jc_off[feat] + k];
    for (int k = threadIdx.x; k < H.pw_nnz[feat]; k += blockDim.x) {
      ir[k] = arena_ir[H.pw_nz_off[feat] + k];
      pr[k] = arena_pr[H.pw_nz_off[feat] + k];
    }
    if (threadIdx.x == 0) {
      dims[0] = H.pw_rows[feat];
      dims[1] = H.pw_cols[feat];
      dims[2] = H.pw_nnz[feat];
    }
  } else if (threadIdx.x == 0) {
    dims[0] = -1;
    dims[1] = -1;
    dims[2] = 0;
  }
  if (feat == 0) {
    int32_t* tail = reinterpret_cast<int32_t*>(pack + L.tail) + 45 * f;
    for (int k = threadIdx.x; k < 45; k += blockDim.x) tail[k] = H.tail[k];
  }
}

