// sinkhorn.h — what the two files of the log-domain Sinkhorn share: sinkhorn.hip (the forward) and sinkhorn_grad.hip (the reverse pass).
// The register-resident layout of the patch-level problems and its base-2 log-sum-exp are defined once, here, so the reverse pass
// recomputes the forward's duals with the forward's own operations.
#pragma once
#include "common.h"

namespace lcr {

// Four threads share a row (column): each takes every 4th element, partials are folded with two quad shuffles.
__device__ __forceinline__ float quad_max(float x) {      // quad permutes on the DPP path (no LDS crossbar round trip)
  x = fmaxf(x, dpp0<DPP_QUAD_1032>(x));
  return fmaxf(x, dpp0<DPP_QUAD_2301>(x));
}
__device__ __forceinline__ float quad_sum(float x) {
  x += dpp0<DPP_QUAD_1032>(x);
  return x + dpp0<DPP_QUAD_2301>(x);
}

// The register-resident layout, for matrices up to 132 x 132 (the 129 x 129 patch problems): every thread keeps its 33 row entries AND
// its 33 column entries in registers for all iterations — four threads per row / column — so a half-iteration is 33 independent
// exponentials per thread plus two quad folds; LDS only carries the dual vectors.
constexpr int SKR_E = 33;                 // entries per thread
constexpr int SKR_LINES = 4 * SKR_E;      // 132 rows / columns at most
constexpr int SKR_T = 576;                // 9 wavefronts >= 4 * 132 threads
// The iteration runs in base-2 logarithms — scores, marginals and duals scaled by log2(e) once, so that an exponential is the bare
// v_exp_f32 and the logarithm the bare v_log_f32 (no multiply in front of / behind every transcendental) — and on PAIRS of entries
// (element 8k + part and 8k + 4 + part): the adds are packed fp32 (v_pk_add_f32), the maximum a v_max3_f32.  Per element and pass:
// 0.5 + 0.5 + 0.5 + 0.5 full-rate operations + one quarter-rate exponential instead of 5 + one (7.0 -> 4.7 ms per launch of ~3600
// patch problems).  Same algorithm, same stabiliser (the exact maximum), results equal to the natural-log form to fp32 rounding.
typedef float float2v __attribute__((ext_vector_type(2)));
constexpr int SKR_P = (SKR_E + 1) / 2;    // entry pairs per thread
constexpr float SKR_LOG2E = 1.44269504088896341f, SKR_LN2 = 0.693147180559945309f;

__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }     // v_exp_f32
__device__ __forceinline__ float log2_hw(float x) { return __builtin_amdgcn_logf(x); }      // v_log_f32

// log2-sum-exp2 over this thread's entries (pairs in x) folded over the four threads of the line
__device__ __forceinline__ float skr_lse2(const float2v (&x)[SKR_P], bool live) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < SKR_P; ++k) mx = fmaxf(fmaxf(mx, x[k].x), x[k].y);
  mx = quad_max(mx);
  const float m0 = live ? mx : 0.f;
  const float2v neg = {-m0, -m0};
  float2v acc = {0.f, 0.f};
#pragma unroll
  for (int k = 0; k < SKR_P; ++k) {
    const float2v y = x[k] + neg;
    const float2v e = {exp2_hw(y.x), exp2_hw(y.y)};
    acc += e;
  }
  return mx + log2_hw(quad_sum(acc.x + acc.y));
}

}  // namespace lcr
