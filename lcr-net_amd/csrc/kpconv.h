// kpconv.h — what the two files of the encoder's gather kernels share: kpconv.hip (the forward) and kpconv_grad.hip (the reverse pass).
// The kernel-point table, the query -> workgroup mapping and the influence arithmetic are defined once, here, so the reverse pass
// evaluates w(m,h,k) with the forward's own operations.
#pragma once
#include <algorithm>

#include "common.h"

namespace lcr {

constexpr int KP_K = 15;       // kernel points (cfg.backbone.kernel_size)
constexpr int KP_HMAX = 128;   // neighbour columns supported per query
constexpr int KP_WAVES = 4;

struct KPoints {               // by value in kernel arguments
  float p[KP_K][3];
};
inline KPoints load_kp(const float* kp_host) {
  KPoints k;
  for (int i = 0; i < KP_K; ++i)
    for (int d = 0; d < 3; ++d) k.p[i][d] = kp_host[3 * i + d];
  return k;
}

// a multiple of 8 workgroups for the kernels that walk an xcd_band, enough for every XCD's eighth of the rows
inline int grid_for_xcd(int64_t rows, int per_block) {
  const int64_t per_xcd = ((rows + 7) / 8 + per_block - 1) / per_block;
  return 8 * static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(per_xcd, 256 * 2)));
}

#ifdef __HIPCC__
// Row -> workgroup mapping of the gather kernels.  Workgroups go round-robin to the 8 XCDs (id % 8), each with its own,
// non-coherent L2.  With a plain grid-stride walk all XCDs sweep the (spatially ordered) query list side by side, so every XCD
// pulls the SAME support rows into its own L2 — the gathered table crosses the fabric up to eight times (PMC: max-pool fetched
// 445 MB for a 65 MB table).  Here XCD x walks the x-th CONTIGUOUS eighth of the list: its L2 only ever holds that region's rows.
struct XcdBand {
  int64_t begin, end, stride;   // this wavefront's first row, the end of its band, the step
};
__device__ __forceinline__ XcdBand xcd_band(int64_t M, int wave_in_block, int waves_per_block) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslots = gridDim.x >> 3;      // the grid is a multiple of 8
  const int64_t per = (M + 7) / 8;
  XcdBand b;
  b.begin = xcd * per + static_cast<int64_t>(slot) * waves_per_block + wave_in_block;
  b.end = min(M, (xcd + 1) * per);
  b.stride = static_cast<int64_t>(nslots) * waves_per_block;
  return b;
}

// Declares kx, ky, kz: the kernel point of the lane's MFMA column `col` out of the kernel argument `kp` (column 15 is no kernel point:
// zeros).  A macro, not a function: through a call the 45 argument loads are emitted ahead of the select chain instead of inside it, and
// the kernels around it come out with another instruction order and register assignment.
#define LCR_KP_SELECT(kp, col, kx, ky, kz) \
  float kx = 0.f, ky = 0.f, kz = 0.f;      \
  _Pragma("unroll")                        \
  for (int k = 0; k < KP_K; ++k)           \
    if ((col) == k) {                      \
      kx = (kp).p[k][0];                   \
      ky = (kp).p[k][1];                   \
      kz = (kp).p[k][2];                   \
    }

// One edge against one kernel point: e = d - k with d = s_n - q_m, r = |e| as fma(ez, ez, fma(ey, ey, ex * ex)) under v_sqrt_f32, and
// the linear influence w = max(0, 1 - r / sigma) as fma(-r, 1/sigma, 1) (kpconv.py:96-99).
__device__ __forceinline__ void kp_edge(float dx, float dy, float dz, float kx, float ky, float kz, float inv_sigma, float& ex, float& ey, float& ez,
                                        float& r, float& w) {
  ex = dx - kx, ey = dy - ky, ez = dz - kz;
  r = __builtin_amdgcn_sqrtf(fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
  w = fmaxf(fmaf(-r, inv_sigma, 1.f), 0.f);
}
__device__ __forceinline__ float kp_influence(float dx, float dy, float dz, float kx, float ky, float kz, float inv_sigma) {
  float ex, ey, ez, r, w;
  kp_edge(dx, dy, dz, kx, ky, kz, inv_sigma, ex, ey, ez, r, w);
  return w;
}
#endif  // __HIPCC__

}  // namespace lcr
