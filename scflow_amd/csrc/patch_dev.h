// What the patch kernels (patch.hip) and the training-patch kernels (train_patch.hip) share: the
// limits both accept from a geometry in device memory, the 3×3 product and cv2's INTER_LINEAR
// source coordinate.  Every fp32 expression is part of the contract, so the files
// that include this keep contraction off.
#pragma once
#include "common.h"

constexpr int PX_THREADS = 256;
constexpr int PX_MAX_CROP = 16384;      // crop sides the extract kernels accept from geom
constexpr int PX_MAX_ORIGIN = 1 << 20;  // |x1|, |y1| they accept (keeps every index in 32 bits)

// c = a·b, row-major 3×3, every element summed over k = 0, 1, 2 in that order
__device__ inline void mat3_mul(const float* a, const float* b, float* c) {
#pragma clang fp contract(off)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      float acc = a[3 * i] * b[j];
      acc = acc + a[3 * i + 1] * b[3 + j];
      acc = acc + a[3 * i + 2] * b[6 + j];
      c[3 * i + j] = acc;
    }
}

// cv2's INTER_LINEAR source coordinate of output index o on an axis of n source and no output
// samples, the exact rational ((2o + 1)·n − no) / (2·no): its floor i0 and fraction f, clamped to
// the first / last sample.  f is the only rounded quantity.
__device__ inline void linear_coord(int o, int n, int no, int& i0, float& f) {
  const int num = (2 * o + 1) * n - no, den = 2 * no;
  if (num < 0) {
    i0 = 0, f = 0.f;
    return;
  }
  i0 = num / den;
  f = (float)(num - i0 * den) / (float)den;
  if (i0 >= n - 1) i0 = n - 1, f = 0.f;
}
