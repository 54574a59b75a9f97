// Segmented fp32 feature rows, shared by the pairwise metric kernels (knn.hip, ksum.hip): a segment's row range out of an offset
// array the kernel cannot trust, and the scalar / 16-byte load of four features of a row with zeros past its end.
#pragma once
#include "common.h"

#define KNN_MAX_D 256
#define KNN_MAX_SEG 1024

// a segment's row range out of an offset array the kernel cannot trust: clamped to [0, n], a decreasing pair is an empty segment
__device__ __forceinline__ void knn_segment(const int32_t* __restrict__ off, int s, int n, int* lo, int* hi) {
  const int a = min(max(off[s], 0), n), b = min(max(off[s + 1], 0), n);
  *lo = a;
  *hi = b < a ? a : b;
}

// elements [c0, c0 + 4) of row `row` (d wide), zeros past d or when the row does not exist
__device__ __forceinline__ float4 knn_load4(const float* __restrict__ x, size_t row, int d, int c0, bool exists, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!exists || c0 >= d) return v;
  const float* p = x + row * (size_t)d + c0;
  if (vec) return *(const float4*)p;           // (d a multiple of 4 and the base 16-byte aligned: c0 < d implies c0 + 3 < d)
  v.x = p[0];
  if (c0 + 1 < d) v.y = p[1];
  if (c0 + 2 < d) v.z = p[2];
  if (c0 + 3 < d) v.w = p[3];
  return v;
}

// may rows of x be read 16 bytes at a time?
static inline int knn_vec(const float* p, int d) { return (d & 3) == 0 && ((uintptr_t)p & 15) == 0; }
