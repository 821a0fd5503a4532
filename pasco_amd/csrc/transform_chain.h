// The `transform` chain of include/pasco_frame.h (transform_coords of data/semantic_kitti.py) as device functions, shared by
// frame.hip (pf_*) and target.hip (pt_*): voxel index -> metres (voxel centre) in fp32 -> T by an fmaf chain over k = 0..3
// from 0 -> voxel index, rintf.  Include inside the translation unit's unnamed namespace, with FP contraction off.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// min_bound of transform_coords: torch.tensor([0, -25.6, -2]) is fp32
constexpr float MINB[3] = {0.0f, -25.6f, -2.0f};

// metres -> T -> voxel index (transform_coords): h = (x, y, z, 1) in fp32
__device__ __forceinline__ void apply_T(const float *T, const float h[3], int64_t out[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float acc = fmaf(T[i * 4 + 0], h[0], 0.0f);
    acc = fmaf(T[i * 4 + 1], h[1], acc);
    acc = fmaf(T[i * 4 + 2], h[2], acc);
    acc = fmaf(T[i * 4 + 3], 1.0f, acc);
    float v = ((acc - MINB[i]) - 0.1f) / 0.2f;
    out[i] = static_cast<int64_t>(static_cast<int32_t>(rintf(v)));
  }
}

__device__ __forceinline__ void metres_f64(const double c[3], float h[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) h[i] = static_cast<float>(static_cast<double>(MINB[i]) + (c[i] * 0.2 + 0.1));
}

__device__ __forceinline__ void metres_i64(const int64_t c[3], float h[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) h[i] = MINB[i] + (static_cast<float>(c[i]) * 0.2f + 0.1f);
}
