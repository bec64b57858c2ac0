// attention.h — what the two files of the 3D-RoFormer attention block share: attention.hip (the forward) and attention_grad.hip (the
// reverse pass).  The tile geometry, the tile load and the accumulator-to-operand step are defined once, here, so the reverse pass walks
// the forward's register layout.
#pragma once
#include "common.h"

namespace lcr {

constexpr int AT_D = 32;            // head dim (d_model 128 / 4 heads)
constexpr int AT_LD = 33;           // LDS row stride: conflict-free ds_read_b32 for both "row = lane" operand patterns
constexpr int AT_TILE = 32 * AT_LD;
constexpr int AT_SPLIT = 4;         // wavefronts per workgroup
constexpr int AT_MAX_P = 64;        // problems per launch

// 32 x 32 tile (rows r0.., columns col0..col0+31) of a row-major matrix -> dst[32][AT_LD]; rows beyond `rows` -> 0.  One wavefront.
__device__ __forceinline__ void load_tile(const float* __restrict__ src, int64_t rows, int64_t r0, int ld_src, int col0, float* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int f = lane + 64 * i;          // 256 float4 pieces
    const int r = f >> 3, c4 = f & 7;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < rows) v = *reinterpret_cast<const float4*>(src + (r0 + r) * ld_src + col0 + c4 * 4);
    float* d = dst + r * AT_LD + c4 * 4;
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  }
}

// A 32x32 MFMA result (this lane: column `col`, rows (r & 3) + 8 (r >> 2) + 4 half) as the B operand of the next product: at step kk this
// lane must supply row 2 kk + half, which sits in half (kk >> 1) & 1 at register 2 (kk & 1) + 4 (kk >> 2) + (row & 1); the partner lane
// (lane ^ 32) holds the other half's rows: one cross-half swap per step.  kk is a compile-time constant.
__device__ __forceinline__ float acc_as_b(const floatx16& s, int kk, int half) {
  const int hp = (kk >> 1) & 1;
  const int rbase = 2 * (kk & 1) + 4 * (kk >> 2);
  const float own = (half == 0) ? s[rbase + 0] : s[rbase + 1];       // value for a requester in my own half
  const float other = (half == 0) ? s[rbase + 1] : s[rbase + 0];     // value my partner (other half) needs
  const float recv = __shfl_xor(other, 32);
  return (half == hp) ? own : recv;
}

}  // namespace lcr
