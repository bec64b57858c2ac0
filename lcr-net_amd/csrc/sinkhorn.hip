// sinkhorn.hip — log-domain Sinkhorn with dustbins for the registration tail (modules/sinkhorn/learnable_sinkhorn.py:5-66): the padded score
// matrix and the iteration in five kernel forms.  Which form a call takes is decided once on the host, in sk_plan at the end of this file.
#include <algorithm>
#include <cmath>

#include "sinkhorn.h"

namespace lcr {

// ---- log-domain Sinkhorn with dustbins ---------------------------------------------------------------------------------------
// S: [B, M+1, N+1] padded score matrices (dustbin row/column = alpha, masked entries = -inf_val), overwritten by the result
// S + u + v - norm.  One workgroup per matrix; u, v live in global scratch (L2 resident).
constexpr int SK_T = 512;

// log-sum-exp over a strided vector with hardware exp/log (v_exp_f32 / v_log_f32 based; ~1e-6 relative) in two branch-free
// passes (max, then sum of exp(x - max)); `add` is the dual vector added on the fly.
__device__ __forceinline__ float fast_exp(float x) { return __expf(x); }
__device__ __forceinline__ float fast_log(float x) { return __logf(x); }

__device__ __forceinline__ void sk_setup(const uint8_t* __restrict__ row_mask, const uint8_t* __restrict__ col_mask, int64_t b, int M, int N,
                                         float inf_val, float* u, float* v, float* log_mu, float* log_nu, float* norm_out) {
  __shared__ int s_nr, s_nc;
  if (threadIdx.x == 0) {
    s_nr = 0;
    s_nc = 0;
  }
  __syncthreads();
  int cr = 0, cc = 0;
  for (int i = threadIdx.x; i < M; i += blockDim.x) cr += row_mask[b * M + i] ? 1 : 0;
  for (int j = threadIdx.x; j < N; j += blockDim.x) cc += col_mask[b * N + j] ? 1 : 0;
  atomicAdd(&s_nr, cr);
  atomicAdd(&s_nc, cc);
  __syncthreads();
  const float nr = static_cast<float>(s_nr), nc = static_cast<float>(s_nc);
  const float norm = -logf(nr + nc);
  for (int i = threadIdx.x; i <= M; i += blockDim.x) {
    const bool masked = i < M && !row_mask[b * M + i];
    log_mu[i] = masked ? -inf_val : (i < M ? norm : logf(nc) + norm);
    u[i] = 0.f;
  }
  for (int j = threadIdx.x; j <= N; j += blockDim.x) {
    const bool masked = j < N && !col_mask[b * N + j];
    log_nu[j] = masked ? -inf_val : (j < N ? norm : logf(nr) + norm);
    v[j] = 0.f;
  }
  if (threadIdx.x == 0) *norm_out = norm;
  __syncthreads();
}

// u[i] = log_mu[i] - LSE_j(s[i][j] + v[j]) for the rows owned by this wavefront (lanes over columns)
__device__ __forceinline__ void sk_row(const float* __restrict__ s, int N1, int i, const float* __restrict__ v, const float* __restrict__ log_mu,
                                       float* __restrict__ u) {
  const int lane = threadIdx.x & 63;
  float mx = -INFINITY;
  for (int j = lane; j < N1; j += 64) mx = fmaxf(mx, s[i * N1 + j] + v[j]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  float sum = 0.f;
  for (int j = lane; j < N1; j += 64) sum += fast_exp(s[i * N1 + j] + v[j] - mx);
  sum = wave_sum(sum);
  if (lane == 0) u[i] = log_mu[i] - (mx + fast_log(sum));
}

// v[j] = log_nu[j] - LSE_i(s[i][j] + u[i]) for one column (one thread; rows coalesced across threads)
__device__ __forceinline__ void sk_col(const float* __restrict__ s, int M1, int N1, int j, const float* __restrict__ u,
                                       const float* __restrict__ log_nu, float* __restrict__ v) {
  float mx = -INFINITY;
  for (int i0 = 0; i0 < M1; i0 += 8) {
    float x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = i0 + q < M1 ? s[(i0 + q) * N1 + j] + u[i0 + q] : -INFINITY;
#pragma unroll
    for (int q = 0; q < 8; ++q) mx = fmaxf(mx, x[q]);
  }
  float sum = 0.f;
  for (int i0 = 0; i0 < M1; i0 += 8) {
    float x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = i0 + q < M1 ? s[(i0 + q) * N1 + j] + u[i0 + q] : -INFINITY;
#pragma unroll
    for (int q = 0; q < 8; ++q) sum += fast_exp(x[q] - mx);
  }
  v[j] = log_nu[j] - (mx + fast_log(sum));
}

// (a') patch level, register resident: sinkhorn.h's layout, element e of part p being column (row) 4e + p.  The LDS-matrix version (a)
//      below spent ~7 us per half-iteration re-reading the matrix twice.
__global__ __launch_bounds__(SKR_T) void k_log_sinkhorn_reg(float* __restrict__ S, const uint8_t* __restrict__ row_mask,
                                                            const uint8_t* __restrict__ col_mask, int M, int N, int iters, float inf_val,
                                                            const unsigned* __restrict__ only) {
  __shared__ float u[SKR_LINES + 8], v[SKR_LINES + 8], log_mu[SKR_LINES + 8], log_nu[SKR_LINES + 8];
  __shared__ float s_norm;
  if (only && !only[blockIdx.x]) return;      // second launch behind k_sinkhorn_scaled: only the problems it handed back
  const int64_t b = blockIdx.x;
  const int M1 = M + 1, N1 = N + 1;
  float* sg = S + b * M1 * N1;
  const int part = threadIdx.x & 3, line = threadIdx.x >> 2;
  const bool row_live = line < M1, col_live = line < N1;
  float2v R[SKR_P], Cc[SKR_P];              // base-2 scores; elements beyond the line are -inf
#pragma unroll
  for (int k = 0; k < SKR_P; ++k) {
    const int j0 = 8 * k + part, j1 = j0 + 4;
    R[k].x = (row_live && j0 < N1) ? sg[line * N1 + j0] * SKR_LOG2E : -INFINITY;
    R[k].y = (row_live && j1 < N1) ? sg[line * N1 + j1] * SKR_LOG2E : -INFINITY;
    Cc[k].x = (col_live && j0 < M1) ? sg[j0 * N1 + line] * SKR_LOG2E : -INFINITY;
    Cc[k].y = (col_live && j1 < M1) ? sg[j1 * N1 + line] * SKR_LOG2E : -INFINITY;
  }
  sk_setup(row_mask, col_mask, b, M, N, inf_val, u, v, log_mu, log_nu, &s_norm);
  for (int t = threadIdx.x; t < SKR_LINES + 8; t += SKR_T) {      // marginals to base 2; neutral duals beyond the lines (pair reads)
    log_mu[t] = t < M1 ? log_mu[t] * SKR_LOG2E : 0.f;
    log_nu[t] = t < N1 ? log_nu[t] * SKR_LOG2E : 0.f;
    if (t >= M1) u[t] = 0.f;
    if (t >= N1) v[t] = 0.f;
  }
  __syncthreads();
  // Exact early exit: when a whole iteration leaves every u AND every v bit-identical, all later iterations repeat it — the result is
  // the one the full `iters` would give, to the bit.  (The patch problems of real pairs reach their fp32 fixed point long before the
  // reference's 100 iterations; a problem that keeps flipping a last bit simply runs them all.)
  for (int it = 0; it < iters; ++it) {
    int changed = 0;
    {
      float2v x[SKR_P];
#pragma unroll
      for (int k = 0; k < SKR_P; ++k) {
        const float2v d = {v[8 * k + part], v[8 * k + part + 4]};
        x[k] = R[k] + d;
      }
      const float lse = skr_lse2(x, row_live);
      if (row_live && part == 0) {
        const float un = log_mu[line] - lse;
        changed |= __float_as_uint(un) != __float_as_uint(u[line]);
        u[line] = un;
      }
    }
    __syncthreads();
    {
      float2v x[SKR_P];
#pragma unroll
      for (int k = 0; k < SKR_P; ++k) {
        const float2v d = {u[8 * k + part], u[8 * k + part + 4]};
        x[k] = Cc[k] + d;
      }
      const float lse = skr_lse2(x, col_live);
      if (col_live && part == 0) {
        const float vn = log_nu[line] - lse;
        changed |= __float_as_uint(vn) != __float_as_uint(v[line]);
        v[line] = vn;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  if (row_live) {
    const float ui = u[line], nrm = s_norm;
#pragma unroll
    for (int k = 0; k < SKR_P; ++k) {
      const int j0 = 8 * k + part, j1 = j0 + 4;
      if (j0 < N1) sg[line * N1 + j0] = fmaf(R[k].x + ui + v[j0], SKR_LN2, -nrm);
      if (j1 < N1) sg[line * N1 + j1] = fmaf(R[k].y + ui + v[j1], SKR_LN2, -nrm);
    }
  }
}

// (a) whole problem in one workgroup, matrix AND dual vectors resident in LDS (patch level: 129 x 129 floats = 66.5 KB; from L2
//     every one of the 200 passes would be a chain of dependent ~1 us loads).  Four threads share a row (column): each takes
//     every 4th element, partials are folded with two quad shuffles.
__global__ __launch_bounds__(SK_T) void k_log_sinkhorn_lds(float* __restrict__ S, const uint8_t* __restrict__ row_mask,
                                                           const uint8_t* __restrict__ col_mask, int M, int N, int iters, float inf_val,
                                                           float* __restrict__ uv_ws) {
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  __shared__ float s_norm;
  const int64_t b = blockIdx.x;
  const int M1 = M + 1, N1 = N + 1;
  float* s_mat = s_dyn;
  float* u = s_dyn + M1 * N1;
  float* v = u + M1;
  float* log_mu = v + N1;
  float* log_nu = log_mu + M1;
  float* sg = S + b * M1 * N1;
  for (int t = threadIdx.x; t < M1 * N1; t += SK_T) s_mat[t] = sg[t];
  sk_setup(row_mask, col_mask, b, M, N, inf_val, u, v, log_mu, log_nu, &s_norm);
  const int part = threadIdx.x & 3, line0 = threadIdx.x >> 2;
  for (int it = 0; it < iters; ++it) {
    for (int i = line0; i < ((M1 + 15) & ~15); i += SK_T / 4) {     // padded so that whole quads stay converged for the shuffles
      const bool live = i < M1;
      const float* row = s_mat + (live ? i : 0) * N1;
      float mx = -INFINITY;
      for (int j = part; j < N1; j += 4) mx = fmaxf(mx, row[j] + v[j]);
      mx = quad_max(mx);
      float sum = 0.f;
      for (int j = part; j < N1; j += 4) sum += fast_exp(row[j] + v[j] - mx);
      sum = quad_sum(sum);
      if (live && part == 0) u[i] = log_mu[i] - (mx + fast_log(sum));
    }
    __syncthreads();
    for (int j = line0; j < ((N1 + 15) & ~15); j += SK_T / 4) {
      const bool live = j < N1;
      const float* colp = s_mat + (live ? j : 0);
      float mx = -INFINITY;
      for (int i = part; i < M1; i += 4) mx = fmaxf(mx, colp[i * N1] + u[i]);
      mx = quad_max(mx);
      float sum = 0.f;
      for (int i = part; i < M1; i += 4) sum += fast_exp(colp[i * N1] + u[i] - mx);
      sum = quad_sum(sum);
      if (live && part == 0) v[j] = log_nu[j] - (mx + fast_log(sum));
    }
    __syncthreads();
  }
  for (int t = threadIdx.x; t < M1 * N1; t += SK_T) {
    const int i = t / N1, j = t - i * N1;
    sg[t] = s_mat[t] + u[i] + v[j] - s_norm;
  }
}

// (b) matrices that do not fit LDS (node level, ~350 x 330): one launch per half-iteration so that every row / column gets its
//     own wavefront / thread across the whole chip instead of one CU grinding through 200 passes
__global__ __launch_bounds__(SK_T) void k_sk_init(const uint8_t* __restrict__ row_mask, const uint8_t* __restrict__ col_mask, int M, int N,
                                                  float inf_val, float* __restrict__ uv_ws, float* __restrict__ norm_ws) {
  const int64_t b = blockIdx.x;
  const int M1 = M + 1, N1 = N + 1;
  float* u = uv_ws + b * (M1 + N1) * 2;
  float* v = u + M1;
  __shared__ float s_norm;
  sk_setup(row_mask, col_mask, b, M, N, inf_val, u, v, v + N1, v + N1 + M1, &s_norm);
  if (threadIdx.x == 0) norm_ws[b] = s_norm;
}
__global__ __launch_bounds__(256) void k_sk_rows(const float* __restrict__ S, int M, int N, float* __restrict__ uv_ws) {
  const int64_t b = blockIdx.y;
  const int M1 = M + 1, N1 = N + 1;
  float* u = uv_ws + b * (M1 + N1) * 2;
  const float* v = u + M1;
  const float* log_mu = v + N1;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i < M1) sk_row(S + b * M1 * N1, N1, i, v, log_mu, u);
}
// 64 columns per workgroup, 16 row-slices x 64 columns = 1024 threads: loads are coalesced along the columns and only
// ceil(M1/16) deep per thread; slices are folded through LDS
__global__ __launch_bounds__(1024) void k_sk_cols(const float* __restrict__ S, int M, int N, float* __restrict__ uv_ws) {
  __shared__ float s_part[16][64];
  const int64_t b = blockIdx.y;
  const int M1 = M + 1, N1 = N + 1;
  float* u = uv_ws + b * (M1 + N1) * 2;
  float* v = u + M1;
  const float* log_nu = v + N1 + M1;
  const float* s = S + b * M1 * N1;
  const int c = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + c;
  const bool live = j < N1;
  float x[24];
  int cnt = 0;
  float mx = -INFINITY;
  for (int i = slice; i < M1 && cnt < 24; i += 16, ++cnt) {
    x[cnt] = live ? s[i * N1 + j] + u[i] : -INFINITY;
    mx = fmaxf(mx, x[cnt]);
  }
  for (int i = slice + 16 * 24; i < M1; i += 16) mx = fmaxf(mx, live ? s[i * N1 + j] + u[i] : -INFINITY);   // very tall matrices
  s_part[slice][c] = mx;
  __syncthreads();
  float m = s_part[0][c];
#pragma unroll
  for (int q = 1; q < 16; ++q) m = fmaxf(m, s_part[q][c]);
  __syncthreads();
  float sum = 0.f;
  for (int q = 0; q < cnt; ++q) sum += fast_exp(x[q] - m);
  for (int i = slice + 16 * 24; i < M1; i += 16) sum += live ? fast_exp(s[i * N1 + j] + u[i] - m) : 0.f;
  s_part[slice][c] = sum;
  __syncthreads();
  if (slice == 0 && live) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += s_part[q][c];
    v[j] = log_nu[j] - (m + fast_log(t));
  }
}
__global__ __launch_bounds__(256) void k_sk_final(float* __restrict__ S, int M, int N, const float* __restrict__ uv_ws, const float* __restrict__ norm_ws) {
  const int64_t b = blockIdx.y;
  const int M1 = M + 1, N1 = N + 1;
  const float* u = uv_ws + b * (M1 + N1) * 2;
  const float* v = u + M1;
  float* s = S + b * M1 * N1;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < M1 * N1; t += gridDim.x * blockDim.x) {
    const int i = t / N1, j = t - i * N1;
    s[t] = s[t] + u[i] + v[j] - norm_ws[b];
  }
}

// (a'') patch level, SCALED form (the default for matrices up to 132 x 132): the same iteration as the log-domain kernels, carried in the
//      exponential domain.  With gauges a, b (base-2 logarithms) and K~_ij = 2^(S2_ij + a_i + b_j), the duals are u_i = a_i + log2 u~_i,
//      v_j = b_j + log2 v~_j and one iteration is  u~_i = mu_i / sum_j K~_ij v~_j,  v~_j = nu_j / sum_i K~_ij u~_i  — one packed FMA per
//      two entries instead of a max, a subtraction and a quarter-rate exponential per entry.  It is the reference's sequence of iterates
//      (optimal_transport's u/v updates) in exact arithmetic for ANY gauge; fp32 range is kept by re-gauging: whenever a scale leaves
//      [2^-40, 2^40] the scales are folded into a, b and K~ is rebuilt from the scores (one exponential pass, a handful of times per
//      problem, all in its first iterations).  Entries below 2^-126 of their row's largest flush to zero — they are below 2^-80 of
//      every sum they enter.  A problem whose sums leave [2^-100, 2^100] anyway (or turn NaN) is handed back untouched through
//      `redo[b]` to the log-domain kernel launched behind this one.  Fully masked lines keep u = 0 / v = 0, as the reference's fp32
//      arithmetic gives them (-1e12 - (-1e12)).  Entry e of part p is column (row) 33 p + e, so a thread's 33 scales are 8 ds_read_b128
//      + one b64 from a 36-float-strided copy of the scale vector.
constexpr int SKS_STRIDE = 36;
constexpr float SKS_BAND_HI = 1.099511627776e12f, SKS_BAND_LO = 1.f / 1.099511627776e12f;      // 2^40
constexpr float SKS_FAIL_HI = 1.2676506e30f, SKS_FAIL_LO = 1.f / 1.2676506e30f;                // 2^100
__device__ __forceinline__ int sks_pos(int idx) { return (idx / SKR_E) * SKS_STRIDE + idx % SKR_E; }

__device__ __forceinline__ void sks_build(const float* __restrict__ sm, int line, int part, bool row_live, bool col_live, int M1, int N1,
                                          const float* ga, const float* gb, float2v (&KR)[SKR_P], float2v (&KC)[SKR_P]) {
  const int pl = sks_pos(min(line, SKR_LINES - 1));
  const float ar = row_live ? ga[pl] : 0.f, bc = col_live ? gb[pl] : 0.f;
  // reads are unconditional from clamped (in-range) LDS addresses and selected afterwards
  const int rl = min(line, M1 - 1), cl = min(line, N1 - 1);
  const float* gpa = ga + part * SKS_STRIDE;
  const float* gpb = gb + part * SKS_STRIDE;
  {
    float t[2 * SKR_P];
#pragma unroll
    for (int e = 0; e < SKR_E; ++e) t[e] = sm[rl * N1 + min(part * SKR_E + e, N1 - 1)];
    t[2 * SKR_P - 1] = 0.f;
#pragma unroll
    for (int e = 0; e < SKR_E; ++e) {
      const float x = exp2_hw(fmaf(t[e], SKR_LOG2E, ar + gpb[e]));
      t[e] = (row_live && part * SKR_E + e < N1) ? x : 0.f;
    }
#pragma unroll
    for (int k = 0; k < SKR_P; ++k) KR[k] = float2v{t[2 * k], t[2 * k + 1]};
  }
  {
    float t[2 * SKR_P];
#pragma unroll
    for (int e = 0; e < SKR_E; ++e) t[e] = sm[min(part * SKR_E + e, M1 - 1) * N1 + cl];
    t[2 * SKR_P - 1] = 0.f;
#pragma unroll
    for (int e = 0; e < SKR_E; ++e) {
      const float x = exp2_hw(fmaf(t[e], SKR_LOG2E, gpa[e] + bc));
      t[e] = (col_live && part * SKR_E + e < M1) ? x : 0.f;
    }
#pragma unroll
    for (int k = 0; k < SKR_P; ++k) KC[k] = float2v{t[2 * k], t[2 * k + 1]};
  }
}

// sum over this thread's 33 entries of K[e] * scale[33 part + e], folded over the four parts of the line
__device__ __forceinline__ float sks_dot(const float2v (&K)[SKR_P], const float* sc, int part) {
  const float4* sp = reinterpret_cast<const float4*>(sc + part * SKS_STRIDE);
  float4 t[SKR_P / 2];
#pragma unroll
  for (int q = 0; q < SKR_P / 2; ++q) t[q] = sp[q];
  const float2 t2 = *reinterpret_cast<const float2*>(sc + part * SKS_STRIDE + 4 * (SKR_P / 2));
  float2v acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
#pragma unroll
  for (int q = 0; q < SKR_P / 2; ++q) {                 // explicit FMAs: the library is built with -ffp-contract=off
    acc0 = __builtin_elementwise_fma(K[2 * q], float2v{t[q].x, t[q].y}, acc0);
    acc1 = __builtin_elementwise_fma(K[2 * q + 1], float2v{t[q].z, t[q].w}, acc1);
  }
  acc0 = __builtin_elementwise_fma(K[SKR_P - 1], float2v{t2.x, t2.y}, acc0);
  acc0 += acc1;
  return quad_sum(acc0.x + acc0.y);
}

// Line 128 (the dustbin row / column of the 129 x 129 patch problems) would cost a ninth, almost empty wavefront the full 80-instruction
// pass and leave one SIMD with three wavefronts against two on the others (the pass is issue bound: 1325 -> ~800 us per launch in a
// timing experiment without it).  That wavefront instead holds line 128 SPREAD over its 64 lanes — entry l + 64 q of the row and of the
// column in lane l — so its pass is three multiply-adds and one wavefront sum.
constexpr int SKS_MAIN = 128;                 // lines with four threads each (wavefronts 0..7)
constexpr int SKS_XQ = 3;                     // spread entries per lane of the extra line: 3 * 64 >= 129
__device__ __forceinline__ void sks_build_x(const float* __restrict__ sm, int lane, bool row_live, bool col_live, int M1, int N1,
                                            const float* ga, const float* gb, float (&KRx)[SKS_XQ], float (&KCx)[SKS_XQ]) {
  const int px = sks_pos(SKS_MAIN);
  const float ar = ga[px], bc = gb[px];
#pragma unroll
  for (int q = 0; q < SKS_XQ; ++q) {
    const int j = lane + 64 * q;
    const float r = exp2_hw(fmaf(sm[min(SKS_MAIN, M1 - 1) * N1 + min(j, N1 - 1)], SKR_LOG2E, ar + gb[sks_pos(min(j, SKR_LINES - 1))]));
    const float c = exp2_hw(fmaf(sm[min(j, M1 - 1) * N1 + min(SKS_MAIN, N1 - 1)], SKR_LOG2E, ga[sks_pos(min(j, SKR_LINES - 1))] + bc));
    KRx[q] = (row_live && j < N1) ? r : 0.f;
    KCx[q] = (col_live && j < M1) ? c : 0.f;
  }
}
__device__ __forceinline__ float sks_dot_x(const float (&K)[SKS_XQ], const float* sc, int lane) {
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < SKS_XQ; ++q) acc = fmaf(K[q], sc[sks_pos(min(lane + 64 * q, SKR_LINES - 1))], acc);
  return wave_sum(acc);
}

// The matrix is staged once through LDS (coalesced read), the two register copies of K~ are built from there, and the result leaves
// from there (coalesced write): the scores cross HBM once in each direction.  Two barriers per iteration: the "anything changed" and
// "out of band" words are plain LDS flags read behind the second one (double-buffered by iteration parity).  M + 1, N + 1 <= 129.
__global__ __launch_bounds__(SKR_T) void k_sinkhorn_scaled(float* __restrict__ S, const uint8_t* __restrict__ row_mask,
                                                           const uint8_t* __restrict__ col_mask, int M, int N, int iters, float inf_val,
                                                           unsigned* __restrict__ redo) {
  extern __shared__ __attribute__((aligned(16))) float sm[];      // [M1][N1] scores
  __shared__ float u[SKR_LINES + 8], v[SKR_LINES + 8], log_mu[SKR_LINES + 8], log_nu[SKR_LINES + 8];
  __shared__ __attribute__((aligned(16))) float ga[4 * SKS_STRIDE], gb[4 * SKS_STRIDE], su[4 * SKS_STRIDE], sv[4 * SKS_STRIDE];
  __shared__ float s_norm;
  __shared__ int s_flag[2], s_chg[2];                    // both double-buffered by iteration parity (see the loop)
  const int64_t b = blockIdx.x;
  const int M1 = M + 1, N1 = N + 1;
  float* sg = S + b * M1 * N1;
  const int lane = threadIdx.x & 63;
  const bool extra = threadIdx.x >= 4 * SKS_MAIN;        // wavefront 8: line 128, spread over the lanes
  const int part = threadIdx.x & 3, line = extra ? SKS_MAIN : threadIdx.x >> 2, pl = sks_pos(line);
  const bool owner = extra ? lane == 0 : part == 0;      // the thread that publishes the line's scale
  const bool row_live = line < M1, col_live = line < N1;
#pragma unroll 8
  for (int t = threadIdx.x; t < M1 * N1; t += SKR_T) sm[t] = sg[t];
  sk_setup(row_mask, col_mask, b, M, N, inf_val, u, v, log_mu, log_nu, &s_norm);
  const bool row_on = row_live && log_mu[line] > -0.5f * inf_val, col_on = col_live && log_nu[line] > -0.5f * inf_val;
  const float mu = row_on ? exp2_hw(log_mu[line] * SKR_LOG2E) : 0.f, nu = col_on ? exp2_hw(log_nu[line] * SKR_LOG2E) : 0.f;
  float mx = -INFINITY;
  {
    const int rl = min(line, M1 - 1);                    // clamped reads: repeats of in-row entries
    if (!extra) {
#pragma unroll
      for (int e = 0; e < SKR_E; ++e) mx = fmaxf(mx, sm[rl * N1 + min(part * SKR_E + e, N1 - 1)]);
      mx = quad_max(mx);
    } else {
#pragma unroll
      for (int q = 0; q < SKS_XQ; ++q) mx = fmaxf(mx, sm[rl * N1 + min(lane + 64 * q, N1 - 1)]);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
    }
  }
  for (int t = threadIdx.x; t < 4 * SKS_STRIDE; t += SKR_T) {
    ga[t] = 0.f;
    gb[t] = 0.f;
    su[t] = 1.f;
    sv[t] = 1.f;
  }
  if (threadIdx.x == 0) {
    s_flag[0] = 0;
    s_chg[0] = 0;
  }
  __syncthreads();
  if (row_on && owner) ga[pl] = -mx * SKR_LOG2E;         // first gauge: every live row's largest entry becomes 1
  __syncthreads();
  float2v KR[SKR_P], KC[SKR_P];
  float KRx[SKS_XQ], KCx[SKS_XQ];
  if (!extra) sks_build(sm, line, part, row_live, col_live, M1, N1, ga, gb, KR, KC);
  else sks_build_x(sm, lane, row_live, col_live, M1, N1, ga, gb, KRx, KCx);
  float uo = 1.f, vo = 1.f;                              // the scale this thread last wrote
  for (int it = 0; it < iters; ++it) {
    int changed = 0;
    {
      const float sum = extra ? sks_dot_x(KRx, sv, lane) : sks_dot(KR, sv, part);
      if (row_on && owner) {
        const float un = mu * __builtin_amdgcn_rcpf(sum);
        changed |= __float_as_uint(un) != __float_as_uint(uo);
        if (!(un >= SKS_BAND_LO && un <= SKS_BAND_HI)) atomicOr(&s_flag[it & 1], (un >= SKS_FAIL_LO && un <= SKS_FAIL_HI) ? 1 : 2);
        su[pl] = uo = un;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {                              // nobody reads or writes the other parity's words between these two barriers:
      s_chg[(it + 1) & 1] = 0;                           // their last readers (the block-uniform reads below, iteration it - 1) are
      s_flag[(it + 1) & 1] = 0;                          // behind the barrier above, their next writers (iteration it + 1) behind the next
    }
    {
      const float sum = extra ? sks_dot_x(KCx, su, lane) : sks_dot(KC, su, part);
      if (col_on && owner) {
        const float vn = nu * __builtin_amdgcn_rcpf(sum);
        changed |= __float_as_uint(vn) != __float_as_uint(vo);
        if (!(vn >= SKS_BAND_LO && vn <= SKS_BAND_HI)) atomicOr(&s_flag[it & 1], (vn >= SKS_FAIL_LO && vn <= SKS_FAIL_HI) ? 1 : 2);
        sv[pl] = vo = vn;
      }
    }
    if (changed) s_chg[it & 1] = 1;
    __syncthreads();
    const int any = s_chg[it & 1], flag = s_flag[it & 1];   // block-uniform: written before the barrier above, not again before two more
    if (flag & 2) {                                      // out of fp32 range: the log-domain kernel redoes this problem from its input
      if (threadIdx.x == 0) redo[b] = 1u;
      return;
    }
    if (!any) break;                                     // exact early exit (see k_log_sinkhorn_reg): a repeated iterate repeats forever
    if (flag) {                                          // fold the scales into the gauges, rebuild K~ from the scores
      if (owner) {
        if (row_on) {
          ga[pl] += log2_hw(uo);
          su[pl] = uo = 1.f;
        }
        if (col_on) {
          gb[pl] += log2_hw(vo);
          sv[pl] = vo = 1.f;
        }
      }
      __syncthreads();
      if (!extra) sks_build(sm, line, part, row_live, col_live, M1, N1, ga, gb, KR, KC);
      else sks_build_x(sm, lane, row_live, col_live, M1, N1, ga, gb, KRx, KCx);
      __syncthreads();
    }
  }
  if (owner) {
    if (row_on) ga[pl] += log2_hw(uo);
    if (col_on) gb[pl] += log2_hw(vo);
  }
  if (threadIdx.x == 0) redo[b] = 0u;
  __syncthreads();
  const float nrm = s_norm;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = w; i < M1; i += SKR_T / 64) {             // a wavefront per row: coalesced stores
    const float ui = ga[sks_pos(i)];
    for (int j = lane; j < N1; j += 64) sg[i * N1 + j] = sm[i * N1 + j] + fmaf(ui + gb[sks_pos(j)], SKR_LN2, -nrm);
  }
}

// (c) round 3: the node-level problems as ONE persistent launch.  A matrix (~350 x 330 floats = 466 KB) is cut into G row slabs
//     that fit LDS (117 KB at G = 4); workgroup g of problem b keeps its slab, its rows' u and a full copy of v in LDS for all
//     iterations.  A row half-iteration is local.  A column half-iteration needs every slab: each workgroup publishes the
//     (max, sum of exp) of its slab per column, the G workgroups of the problem meet at a counter, and every one of them folds the G
//     partials into the full v itself (no second hand-off; the partial buffer alternates between two copies, so the next
//     iteration's writes cannot overtake this one's reads).  One hand-off per iteration (~3 us) instead of two launch floors
//     (~13 us): 2.6 -> 0.7 ms for the six 351 x 332 problems of a 6-pair call.
//     Hand-off (MI355X_MICROARCH "valid forms"): plain payload stores -> __syncthreads -> lane 0: agent-scope release fence,
//     s_waitcnt vmcnt(0), relaxed agent counter add; consumers: lane 0 polls the counter (relaxed, agent), ONE agent-scope acquire
//     fence, __syncthreads, plain loads.  The G workgroups of a problem must be resident together: the launcher only takes this path
//     when B * G workgroups (one CU each: 1 024 threads, > 80 KB LDS) are a fraction of the chip, and every poll loop is bounded — a
//     workgroup that gives up sets a status bit and leaves, so a scheduling surprise costs a wrong result that is reported, not a hang.
constexpr int SKC_T = 1024;
constexpr int SKC_MAX_G = 16;
constexpr unsigned SKC_SPIN_LIMIT = 1u << 24;
struct SkCoop {
  float*    part;      // [2][B][G][N1][2]
  unsigned* counter;   // [B], zero at launch
  unsigned* status;    // bit 0: a hand-off timed out
  int       G, slab;   // row slabs per problem, rows per slab
  int       nsub;      // row parts of a slab in the column pass (threads = nsub x columns <= 1 024)
};
__global__ void k_sk_coop_init(unsigned* counter, unsigned* status, int B) {
  for (int i = threadIdx.x; i < B; i += blockDim.x) counter[i] = 0u;
  if (threadIdx.x == 0) *status = 0u;
}
__global__ __launch_bounds__(SKC_T) void k_log_sinkhorn_coop(float* __restrict__ S, const uint8_t* __restrict__ row_mask,
                                                             const uint8_t* __restrict__ col_mask, int M, int N, int iters, float inf_val, SkCoop c) {
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  __shared__ float s_norm;
  __shared__ int s_ok;
  const int b = blockIdx.x / c.G, g = blockIdx.x % c.G;
  const int M1 = M + 1, N1 = N + 1;
  const int r0 = g * c.slab, r1 = min(M1, r0 + c.slab), nr = max(r1 - r0, 0);
  float* s_mat = s_dyn;                              // [slab][N1]
  float* u = s_mat + static_cast<size_t>(c.slab) * N1;   // [M1] (only [r0, r1) is maintained after the set-up)
  float* v = u + M1;                                 // [N1]
  float* log_mu = v + N1;                            // [M1]
  float* log_nu = log_mu + M1;                       // [N1]
  float* s_red = log_nu + N1;                        // [nsub][N1][2] column partials of the slab's row parts
  float* sg = S + static_cast<int64_t>(b) * M1 * N1;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int t = tid; t < nr * N1; t += SKC_T) s_mat[t] = sg[static_cast<int64_t>(r0) * N1 + t];
  sk_setup(row_mask, col_mask, b, M, N, inf_val, u, v, log_mu, log_nu, &s_norm);
  const int nsub = c.nsub;
  const int sub = tid / N1, jc = tid - sub * N1;     // column pass: thread (row part, column); threads beyond nsub * N1 idle
  const int third = (nr + nsub - 1) / nsub;
  for (int it = 0; it < iters; ++it) {
    // rows of the slab: 16 lanes per row (64 rows at a time), ONE pass with a running (max, sum) per lane, four independent loads per step
    // (the two-pass form was bound by the LDS latency of its dependent loop, not by LDS bandwidth), DPP row permutes for the 16-lane merge
    for (int i = tid >> 4; i < nr; i += SKC_T / 16) {
      const float* row = s_mat + i * N1;
      const int l16 = tid & 15;
      float m = -INFINITY, sum = 0.f;
      int j = l16;
      for (; j + 48 < N1; j += 64) {
        const float x0 = row[j] + v[j], x1 = row[j + 16] + v[j + 16], x2 = row[j + 32] + v[j + 32], x3 = row[j + 48] + v[j + 48];
        const float mn = fmaxf(fmaxf(fmaxf(x0, x1), fmaxf(x2, x3)), m);
        sum = fmaf(sum, fast_exp(m - mn), (fast_exp(x0 - mn) + fast_exp(x1 - mn)) + (fast_exp(x2 - mn) + fast_exp(x3 - mn)));
        m = mn;
      }
      for (; j < N1; j += 16) {
        const float x = row[j] + v[j];
        const float mn = fmaxf(x, m);
        sum = fmaf(sum, fast_exp(m - mn), fast_exp(x - mn));
        m = mn;
      }
      float mx = fmaxf(m, dpp0<DPP_QUAD_1032>(m));
      mx = fmaxf(mx, dpp0<DPP_QUAD_2301>(mx));
      mx = fmaxf(mx, dpp0<DPP_ROW_HALF_MIRROR>(mx));
      mx = fmaxf(mx, dpp0<DPP_ROW_MIRROR>(mx));
      sum = row_sum16(sum * fast_exp(m - mx));            // a lane without columns: 0 * exp(-inf) = 0
      if (l16 == 0) u[r0 + i] = log_mu[r0 + i] - (mx + fast_log(sum));
    }
    __syncthreads();
    // columns: running (max, sum of exp) over this slab's rows, `nsub` row parts per column folded through LDS
    if (sub < nsub) {
      const int ia = min(nr, sub * third), ib = min(nr, ia + third);
      const float* col = s_mat + jc;
      const float* ur = u + r0;
      float m = -INFINITY, sum = 0.f;
      int i = ia;
      for (; i + 4 <= ib; i += 4) {
        const float x0 = col[i * N1] + ur[i], x1 = col[(i + 1) * N1] + ur[i + 1], x2 = col[(i + 2) * N1] + ur[i + 2], x3 = col[(i + 3) * N1] + ur[i + 3];
        const float mn = fmaxf(fmaxf(fmaxf(x0, x1), fmaxf(x2, x3)), m);
        sum = fmaf(sum, fast_exp(m - mn), (fast_exp(x0 - mn) + fast_exp(x1 - mn)) + (fast_exp(x2 - mn) + fast_exp(x3 - mn)));
        m = mn;
      }
      for (; i < ib; ++i) {
        const float x = col[i * N1] + ur[i];
        const float mn = fmaxf(x, m);
        sum = fmaf(sum, fast_exp(m - mn), fast_exp(x - mn));
        m = mn;
      }
      s_red[(sub * N1 + jc) * 2] = m;
      s_red[(sub * N1 + jc) * 2 + 1] = sum;
    }
    __syncthreads();
    float* mine = c.part + ((static_cast<int64_t>(it & 1) * gridDim.x + blockIdx.x) * N1) * 2;
    if (tid < N1) {
      float mx = -INFINITY;
      for (int q = 0; q < nsub; ++q) mx = fmaxf(mx, s_red[(q * N1 + tid) * 2]);
      float sum = 0.f;
      for (int q = 0; q < nsub; ++q) {
        const float m_q = s_red[(q * N1 + tid) * 2];
        sum += m_q == -INFINITY ? 0.f : s_red[(q * N1 + tid) * 2 + 1] * fast_exp(m_q - mx);
      }
      mine[2 * tid] = mx;
      mine[2 * tid + 1] = sum;
    }
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_fetch_add(&c.counter[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned want = static_cast<unsigned>(c.G) * static_cast<unsigned>(it + 1);
      unsigned spins = 0;
      int ok = 1;
      while (__hip_atomic_load(&c.counter[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > SKC_SPIN_LIMIT) {
          ok = 0;
          break;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      s_ok = ok;
    }
    __syncthreads();
    if (!s_ok) {                                       // block-uniform: give up loudly
      if (tid == 0) atomicOr(c.status, 1u);
      return;
    }
    if (tid < N1) {
      const float2* base = reinterpret_cast<const float2*>(c.part + ((static_cast<int64_t>(it & 1) * gridDim.x + static_cast<int64_t>(b) * c.G) * N1) * 2) + tid;
      float2 pv[SKC_MAX_G];                               // all slabs' partials in flight at once (they come from the other XCDs' memory side)
#pragma unroll
      for (int q = 0; q < SKC_MAX_G; ++q) pv[q] = q < c.G ? base[static_cast<int64_t>(q) * N1] : make_float2(-INFINITY, 0.f);
      float mx = -INFINITY;
#pragma unroll
      for (int q = 0; q < SKC_MAX_G; ++q) mx = fmaxf(mx, pv[q].x);
      float sum = 0.f;
#pragma unroll
      for (int q = 0; q < SKC_MAX_G; ++q) sum += pv[q].x == -INFINITY ? 0.f : pv[q].y * fast_exp(pv[q].x - mx);
      v[tid] = log_nu[tid] - (mx + fast_log(sum));
    }
    __syncthreads();
  }
  for (int t = tid; t < nr * N1; t += SKC_T) {
    const int i = t / N1, j = t - i * N1;
    sg[static_cast<int64_t>(r0) * N1 + t] = s_mat[t] + u[r0 + i] + v[j] - s_norm;
  }
}

// padded score matrix from raw products: S[b][i][j] = scale * raw[b][i][j]; dustbin row / col = alpha; masked -> -inf_val.
// One wavefront per (problem, row) of the padded matrix, lanes along the row (no division per value).
__global__ __launch_bounds__(256) void k_build_padded_scores_rows(const float* __restrict__ raw, const uint8_t* __restrict__ row_mask,
                                                                  const uint8_t* __restrict__ col_mask, int64_t B, int M, int N, float scale,
                                                                  const float* __restrict__ alpha, float inf_val, float* __restrict__ S) {
  const int lane = threadIdx.x & 63;
  const int M1 = M + 1, N1 = N + 1;
  const float a = alpha[0];
  const int64_t rows = B * M1;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6), nwaves = static_cast<int64_t>(gridDim.x) * 4;
  for (int64_t r = wave; r < rows; r += nwaves) {
    const int64_t b = r / M1;
    const int i = static_cast<int>(r - b * M1);
    const bool row_in = i < M;
    const bool row_dead = row_in && !row_mask[b * M + i];
    const float* rr = raw + (b * M + (row_in ? i : 0)) * N;
    float* o = S + r * N1;
    for (int j = lane; j < N1; j += 64) {
      const bool col_in = j < N;
      const float val = (row_in && col_in) ? rr[j] * scale : a;
      const bool masked = row_dead || (col_in && !col_mask[b * N + j]);
      o[j] = masked ? -inf_val : val;
    }
  }
}

}  // namespace lcr

using namespace lcr;

extern "C" int lcr_build_padded_scores(const float* raw, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N, float scale,
                                       const float* alpha, float inf_val, float* S, void* stream) {
  if (!raw || !row_mask || !col_mask || !alpha || !S || B < 1 || M < 1 || N < 1) return refuse(LCR_EARG, "lcr_build_padded_scores: null pointer or outside the domain (B, M, N >= 1): B=%lld M=%d N=%d", static_cast<long long>(B), M, N);
  hipLaunchKernelGGL(k_build_padded_scores_rows, dim3(blocks_for(B * (M + 1) * 64, 256, 8192)), dim3(256), 0, ST(stream), raw, row_mask, col_mask, B, M,
                     N, scale, alpha, inf_val, S);
  return check_launch("lcr_build_padded_scores");
}

// Persistent form for matrices beyond LDS (see k_log_sinkhorn_coop): G row slabs of <= 144 KB; feasible when the B * G workgroups (one CU
// each) are at most a quarter of the chip, N + 1 <= 1 024 (one thread per column and row part) and LCR_SINKHORN_COOP != 0.
static bool sk_coop_plan(int64_t B, int M, int N, int* G_out, int* slab_out) {
  static const bool on = !(getenv("LCR_SINKHORN_COOP") && atoi(getenv("LCR_SINKHORN_COOP")) == 0);
  const int M1 = M + 1, N1 = N + 1;
  if (!on || N1 > SKC_T) return false;
  const int nsub = std::min(4, SKC_T / N1);
  const size_t fixed = sizeof(float) * (2 * static_cast<size_t>(M1 + N1) + 2 * static_cast<size_t>(nsub) * N1);
  const size_t room = 144 * 1024;
  if (fixed + sizeof(float) * N1 > room) return false;
  const int slab_max = static_cast<int>((room - fixed) / (sizeof(float) * N1));
  int G = (M1 + slab_max - 1) / slab_max;
  if (G > SKC_MAX_G || B * G > 64) return false;
  const int G64 = (M1 + 63) / 64;                        // slabs of <= 64 rows: one round of the 16-lanes-per-row pass
  if (G64 > G && G64 <= SKC_MAX_G && B * G64 <= 64) G = G64;
  *G_out = G;
  *slab_out = (M1 + G - 1) / G;
  return true;
}

// Which kernels a call takes and what they need.  Every entry below reads this and nothing else decides:
//   form 0  M + 1, N + 1 <= 132: register resident (k_log_sinkhorn_reg), behind k_sinkhorn_scaled when `scaled`
//   form 1  matrix + vectors <= 150 KB: LDS resident (k_log_sinkhorn_lds)
//   form 2  persistent row slabs (k_log_sinkhorn_coop), where feasible AND the caller's workspace holds its hand-off buffers
//   form 3  one launch per half-iteration (k_sk_rows / k_sk_cols)
constexpr size_t SK_LDS_ROOM = 150 * 1024, SK_WS_FULL = ~size_t(0);   // SK_WS_FULL: "a workspace of ws_floats floats" (lcr_log_sinkhorn_form)
struct SkPlan {
  int    form, G, slab, nsub;   // G, slab, nsub: form 2, see SkCoop
  bool   scaled;
  size_t lds;                   // dynamic LDS bytes of the form's kernel
  size_t ws_floats;             // per-problem vectors and norms, or the persistent form's hand-off buffers wherever that form is feasible
};                              // (whatever form the shape takes: callers' sizes do not move), + the status word (last)
static SkPlan sk_plan(int64_t B, int M, int N, size_t uv_floats) {
  static const bool scaled_on = !(getenv("LCR_SINKHORN_SCALED") && atoi(getenv("LCR_SINKHORN_SCALED")) == 0);
  const int M1 = M + 1, N1 = N + 1;
  const size_t mat_bytes = sizeof(float) * (static_cast<size_t>(M1) * N1 + 2 * (M1 + N1));   // matrix + u, v, log_mu, log_nu
  SkPlan p = {3, 0, 0, 0, false, 0, 0};
  const bool coop = sk_coop_plan(B, M, N, &p.G, &p.slab);
  const size_t coop_floats = coop ? static_cast<size_t>(4) * B * p.G * N1 + B + 8 : 0;
  p.ws_floats = std::max(static_cast<size_t>(B) * (2 * (static_cast<size_t>(M) + N + 2) + 1), coop_floats) + 1;
  if (M1 <= SKR_LINES && N1 <= SKR_LINES) {
    p.form = 0;
    p.scaled = scaled_on && M1 <= SKS_MAIN + 1 && N1 <= SKS_MAIN + 1;
    p.lds = p.scaled ? sizeof(float) * static_cast<size_t>(M1) * N1 : 0;
  } else if (mat_bytes <= SK_LDS_ROOM) {
    p.form = 1;
    p.lds = mat_bytes;
  } else if (coop && uv_floats >= coop_floats + 1) {
    p.form = 2;
    p.nsub = std::min(4, SKC_T / N1);
    p.lds = sizeof(float) * (static_cast<size_t>(p.slab) * N1 + 2 * (M1 + N1) + 2 * static_cast<size_t>(p.nsub) * N1);
  }
  return p;
}

extern "C" int lcr_log_sinkhorn_ws_floats(int64_t B, int M, int N, size_t* floats) {
  if (!floats || B < 1 || M < 1 || N < 1) return refuse(LCR_EARG, "lcr_log_sinkhorn_ws_floats: null pointer or outside the domain (B, M, N >= 1): B=%lld M=%d N=%d", static_cast<long long>(B), M, N);
  *floats = sk_plan(B, M, N, SK_WS_FULL).ws_floats;
  return LCR_OK;
}
// the form lcr_log_sinkhorn_ex takes with a workspace of lcr_log_sinkhorn_ws_floats floats
extern "C" int lcr_log_sinkhorn_form(int64_t B, int M, int N, int* form) {
  if (!form || B < 1 || M < 1 || N < 1) return refuse(LCR_EARG, "lcr_log_sinkhorn_form: null pointer or outside the domain (B, M, N >= 1): B=%lld M=%d N=%d", static_cast<long long>(B), M, N);
  *form = sk_plan(B, M, N, SK_WS_FULL).form;
  return LCR_OK;
}
// the body of lcr_log_sinkhorn and lcr_log_sinkhorn_ex; `who` = the one that was called
static int log_sinkhorn(const char* who, float* S, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N, int iters, float inf_val,
                        float* uv_ws, size_t uv_floats, void* stream) {
  if (!S || !row_mask || !col_mask || !uv_ws || B < 1 || M < 1 || N < 1 || iters < 0)
    return refuse(LCR_EARG, "%s: null pointer or outside the domain (B, M, N >= 1, iters >= 0): B=%lld M=%d N=%d iters=%d", who, static_cast<long long>(B), M, N, iters);
  const SkPlan p = sk_plan(B, M, N, uv_floats);
  KernelTimerScope timed(KT_SINKHORN, ST(stream), B, M, N, iters, p.form);      // brackets every launch of the call (bench.py's pair block)
  if (p.form == 0) {
    unsigned* redo = p.scaled ? reinterpret_cast<unsigned*>(uv_ws) : nullptr;    // B words of the workspace: problems handed back
    if (p.scaled) {
      static DynLds opt_in;                              // up to 132 x 132 floats of dynamic LDS beside the static vectors
      if (opt_in.need(reinterpret_cast<const void*>(&k_sinkhorn_scaled), sizeof(float) * SKR_LINES * SKR_LINES) != hipSuccess)
        return refuse(LCR_EHIP, "%s: cannot reserve dynamic LDS for the scaled-domain kernel", who);
      hipLaunchKernelGGL(k_sinkhorn_scaled, dim3(static_cast<int>(B)), dim3(SKR_T), p.lds, ST(stream), S, row_mask, col_mask, M, N, iters, inf_val, redo);
    }
    hipLaunchKernelGGL(k_log_sinkhorn_reg, dim3(static_cast<int>(B)), dim3(SKR_T), 0, ST(stream), S, row_mask, col_mask, M, N, iters, inf_val, redo);
  } else if (p.form == 1) {
    static DynLds opt_in;                                // > 64 KB of dynamic LDS needs an explicit opt-in
    if (opt_in.need(reinterpret_cast<const void*>(&k_log_sinkhorn_lds), SK_LDS_ROOM) != hipSuccess)
      return refuse(LCR_EHIP, "%s: cannot reserve dynamic LDS for the LDS-resident kernel", who);
    hipLaunchKernelGGL(k_log_sinkhorn_lds, dim3(static_cast<int>(B)), dim3(SK_T), p.lds, ST(stream), S, row_mask, col_mask, M, N, iters, inf_val,
                       uv_ws);
  } else if (p.form == 2) {
    SkCoop c;
    c.part = uv_ws;
    c.counter = reinterpret_cast<unsigned*>(uv_ws + static_cast<size_t>(4) * B * p.G * (N + 1));
    c.status = reinterpret_cast<unsigned*>(uv_ws + uv_floats - 1);      // the LAST word of the workspace (the caller reads it)
    c.G = p.G;
    c.slab = p.slab;
    c.nsub = p.nsub;
    static DynLds opt_in;
    if (opt_in.need(reinterpret_cast<const void*>(&k_log_sinkhorn_coop), p.lds) != hipSuccess)
      return refuse(LCR_EHIP, "%s: cannot reserve %zu B of dynamic LDS for the persistent kernel", who, p.lds);
    hipLaunchKernelGGL(k_sk_coop_init, dim3(1), dim3(64), 0, ST(stream), c.counter, c.status, static_cast<int>(B));
    hipLaunchKernelGGL(k_log_sinkhorn_coop, dim3(static_cast<int>(B) * p.G), dim3(SKC_T), p.lds, ST(stream), S, row_mask, col_mask, M, N, iters, inf_val, c);
  } else {
    if (B > 65535) return refuse(LCR_EARG, "%s: more than 65535 problems in the launch-per-half-iteration form (B=%lld)", who, static_cast<long long>(B));
    // the last B floats of uv_ws's per-problem blocks are not spare, so norms live after all of them (caller sizes uv_ws with +B)
    float* norm_ws = uv_ws + B * 2 * (static_cast<int64_t>(M) + N + 2);
    hipLaunchKernelGGL(k_sk_init, dim3(static_cast<int>(B)), dim3(SK_T), 0, ST(stream), row_mask, col_mask, M, N, inf_val, uv_ws, norm_ws);
    const dim3 grow((M + 1 + 3) / 4, static_cast<int>(B)), gcol((N + 1 + 63) / 64, static_cast<int>(B));
    for (int it = 0; it < iters; ++it) {
      hipLaunchKernelGGL(k_sk_rows, grow, dim3(256), 0, ST(stream), S, M, N, uv_ws);
      hipLaunchKernelGGL(k_sk_cols, gcol, dim3(1024), 0, ST(stream), S, M, N, uv_ws);
    }
    hipLaunchKernelGGL(k_sk_final, dim3(64, static_cast<int>(B)), dim3(256), 0, ST(stream), S, M, N, uv_ws, norm_ws);
  }
  return check_launch(who);
}
// the legacy entry: a workspace of B * (2 * (M + N + 2) + 1) floats, too short for the persistent form's buffers wherever they are larger
extern "C" int lcr_log_sinkhorn(float* S, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N, int iters, float inf_val,
                                float* uv_ws, void* stream) {
  return log_sinkhorn("lcr_log_sinkhorn", S, row_mask, col_mask, B, M, N, iters, inf_val, uv_ws,
                      static_cast<size_t>(B) * (2 * (static_cast<size_t>(M) + N + 2) + 1), stream);
}
// in place on S [B, M+1, N+1]; uv_ws: uv_floats floats, lcr_log_sinkhorn_ws_floats(B, M, N) of them for the form lcr_log_sinkhorn_form reports
extern "C" int lcr_log_sinkhorn_ex(float* S, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N, int iters, float inf_val,
                                   float* uv_ws, size_t uv_floats, void* stream) {
  return log_sinkhorn("lcr_log_sinkhorn_ex", S, row_mask, col_mask, B, M, N, iters, inf_val, uv_ws, uv_floats, stream);
}
