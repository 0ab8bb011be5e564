// lm_dev_common.h — device-side helpers shared by the kernel translation
// units (lm_kernels.hip via lm_runtime.hip, lm_bbox.hip, lm_train.hip).
#ifndef LM_DEV_COMMON_H
#define LM_DEV_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lm_device.h"

#define DEV __device__ __forceinline__

// Frame pointers come from a device array (frame_ptr), so the compiler cannot
// tell that they point to global memory and would access the frames with FLAT
// instructions (longer latency, and they hold the LDS counter too); the casts
// below make those accesses global_load_*.
typedef __attribute__((address_space(1))) const uint8_t lm_gu8;
typedef __attribute__((address_space(1))) const uint32_t lm_gu32;
typedef unsigned lm_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const lm_u32x4 lm_gu4;
DEV const lm_gu8* as_global(const uint8_t* p) { return (const lm_gu8*)p; }

template <class FP>
DEV uint8_t ipad_pixel(FP __restrict__ F, const uint8_t* __restrict__ bkg,
                       const int32_t* __restrict__ cal, const uint8_t* lut, const LmConst& K, int R, int C) {
  // I_PAD(R, C): zero outside I_UNPAD (:684-689); inside, the corrected,
  // normalised, optionally flipped frame.
  const int r = R - K.pad_pre_rows;
  int c = C - K.pad_pre_cols;
  if (r < 0 || r >= K.n_rows || c < 0 || c >= K.n_cols) return 0;
  if (K.flip) c = K.n_cols - 1 - c;
  const int idx = cal[r * K.n_cols + c];
  const int f = F[idx], b = bkg[idx];
  return lut[f > b ? f - b : 0];
}

#endif  // LM_DEV_COMMON_H
