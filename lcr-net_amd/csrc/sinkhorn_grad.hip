// sinkhorn_grad.hip — reverse pass of the log-domain Sinkhorn with dustbins (sinkhorn.hip): dL/dS0 of Z = S0 + u_T + v_T - norm for a given
// G = dL/dZ, S0 being the padded score matrix before the transport.  With u_0 = v_0 = 0 and, for t = 1..T,
//   u_t = log_mu - LSE_j(S + v_{t-1}),   v_t = log_nu - LSE_i(S + u_t),
// the reverse recurrences are
//   dS = G;  du = rowsum(G);  dv = colsum(G)
//   for t = T..1:  Pc = exp(S + u_t + v_t - log_nu)      (softmax over i);   dS -= Pc * dv[None, :];  du -= Pc @ dv
//                  Pr = exp(S + v_{t-1} + u_t - log_mu)  (softmax over j);   dS -= Pr * du[:, None];  dv = -(Pr^T @ du);  du = 0
// Masked rows and columns are absent: G, Pc, Pr and dS are zero there and their duals are never read.  A problem without a valid row or
// without a valid column gets dS = 0.  The duals of all iterations are needed in reverse order; both forms recompute them themselves (the
// log-domain iteration of k_log_sinkhorn_reg / k_sk_rows + k_sk_cols without an early exit) and record them.
// No floating-point atomics: every sum has one fixed order, so results repeat to the bit and a problem's dS does not depend on its batch.
// Which form a call takes is decided in skg_plan at the end of this file.
#include <algorithm>
#include <cmath>

#include "sinkhorn.h"

namespace lcr {
namespace skg {

// ---- resident form: M + 1, N + 1 <= 132 (the 129 x 129 patch problems), one workgroup per problem ------------------------------------
// The forward's register layout (sinkhorn.h; the duals are recomputed with its skr_lse2), R for the row and C for the column of a
// thread.  A reverse half-step needs one sum along the line that its softmax is NOT normalised over — du_i -= sum_j Pc_ij dv_j runs along row i, dv_j = -sum_i Pr_ij du_i along column j — so the v-step terms are formed
// and accumulated in the row layout (dSr) and the u-step terms in the column layout (dSc): both sums are quad folds, nothing is transposed
// per step, and the two accumulators meet once at the end (dS = G - dSr - dSc^T, the column part through the output buffer).  Per entry and
// half-step: three LDS reads (the recorded dual, and {log marginal, dv or du} as one 8-byte pair), three adds, one exponential, one
// multiply, two accumulations.
// The recorded duals — u_1..u_T and v_0..v_T, (2T + 1) lines of GR_LS floats — live in LDS when they fit beside the static vectors
// (T <= 140; 109 KB at T = 100): the four accumulator copies already hold the kernel at 3 wavefronts per SIMD, i.e. one workgroup per CU, so
// the LDS costs no occupancy, and every half-step reads 33 duals per thread that would otherwise be dependent L2 loads.  Longer iteration
// counts record into the caller's workspace instead (same code, HIST_LDS = false).
constexpr int GR_LS = 136;                // floats per recorded line: pair reads reach index 8 * 16 + 3 + 4 = 135
constexpr size_t GR_LDS_ROOM = 150 * 1024;

template <bool HIST_LDS>
__global__ __launch_bounds__(SKR_T) void k_sinkhorn_grad_res(const float* __restrict__ S0, const float* G,
                                                            const uint8_t* __restrict__ row_mask, const uint8_t* __restrict__ col_mask, int M,
                                                            int N, int iters, float* dS, float* __restrict__ d_alpha_part, float* hist_ws) {
  extern __shared__ __attribute__((aligned(16))) float s_hist[];
  __shared__ float2 s_mu[GR_LS], s_nu[GR_LS];      // {base-2 log marginal, du} per row, {.., dv} per column
  __shared__ float s_pr[GR_LS], s_pc[GR_LS];       // 0 on a valid line, -inf on a masked one and beyond the matrix
  __shared__ float s_red[SKR_T];
  __shared__ int s_nr, s_nc;
  const int64_t b = blockIdx.x;
  const int M1 = M + 1, N1 = N + 1, tid = threadIdx.x;
  const float* sg = S0 + b * M1 * N1;
  const float* gg = G + b * M1 * N1;
  float* dg = dS + b * M1 * N1;
  const size_t hist_floats = static_cast<size_t>(2 * iters + 1) * GR_LS;
  float* hist = HIST_LDS ? s_hist : hist_ws + static_cast<size_t>(b) * hist_floats;
  float* hu = hist;                                 // u_t at hu + (t - 1) * GR_LS, t = 1..T
  float* hv = hist + static_cast<size_t>(iters) * GR_LS;   // v_t at hv + t * GR_LS, t = 0..T
  if (tid == 0) {
    s_nr = 0;
    s_nc = 0;
  }
  __syncthreads();
  {
    int cr = 0, cc = 0;
    for (int i = tid; i < M; i += SKR_T) cr += row_mask[b * M + i] ? 1 : 0;
    for (int j = tid; j < N; j += SKR_T) cc += col_mask[b * N + j] ? 1 : 0;
    if (cr) atomicAdd(&s_nr, cr);
    if (cc) atomicAdd(&s_nc, cc);
  }
  __syncthreads();
  const int nr = s_nr, nc = s_nc;
  if (nr == 0 || nc == 0) {                         // block-uniform: no transport to differentiate
    for (int t = tid; t < M1 * N1; t += SKR_T) dg[t] = 0.f;
    if (tid == 0) d_alpha_part[b] = 0.f;
    return;
  }
  {
    const float norm = -logf(static_cast<float>(nr + nc));
    for (int t = tid; t < GR_LS; t += SKR_T) {
      const bool rv = t < M ? row_mask[b * M + t] != 0 : t == M;
      const bool cv = t < N ? col_mask[b * N + t] != 0 : t == N;
      s_pr[t] = rv ? 0.f : -INFINITY;
      s_pc[t] = cv ? 0.f : -INFINITY;
      s_mu[t] = make_float2(rv ? (t < M ? norm : logf(static_cast<float>(nc)) + norm) * SKR_LOG2E : 0.f, 0.f);
      s_nu[t] = make_float2(cv ? (t < N ? norm : logf(static_cast<float>(nr)) + norm) * SKR_LOG2E : 0.f, 0.f);
    }
    for (size_t t = tid; t < hist_floats; t += SKR_T) hist[t] = 0.f;      // v_0 = 0; masked lines and the padding of a line stay 0
  }
  __syncthreads();
  const int part = tid & 3, line = tid >> 2, lc = min(line, GR_LS - 1);
  const bool row_live = s_pr[lc] == 0.f, col_live = s_pc[lc] == 0.f;
  float2v R[SKR_P], C[SKR_P];                         // base-2 scores; -inf on masked lines and beyond the matrix
#pragma unroll
  for (int k = 0; k < SKR_P; ++k) {
    const int j0 = 8 * k + part, j1 = j0 + 4;
    R[k].x = ((line < M1 && j0 < N1) ? sg[line * N1 + j0] * SKR_LOG2E : 0.f) + (s_pr[lc] + s_pc[j0]);
    R[k].y = ((line < M1 && j1 < N1) ? sg[line * N1 + j1] * SKR_LOG2E : 0.f) + (s_pr[lc] + s_pc[j1]);
    C[k].x = ((line < N1 && j0 < M1) ? sg[j0 * N1 + line] * SKR_LOG2E : 0.f) + (s_pc[lc] + s_pr[j0]);
    C[k].y = ((line < N1 && j1 < M1) ? sg[j1 * N1 + line] * SKR_LOG2E : 0.f) + (s_pc[lc] + s_pr[j1]);
  }
  // ---- the forward iteration again, every dual recorded ----
  // When a whole iteration leaves every u AND every v bit-identical, all later iterations repeat it (k_log_sinkhorn_reg's exact early exit):
  // the recompute stops there and the reverse pass, which still runs all `iters` steps, reads the last recorded duals for the steps beyond.
  int t_last = iters;
  for (int t = 1; t <= iters; ++t) {
    int changed = 0;
    {
      const float* vp = hv + static_cast<size_t>(t - 1) * GR_LS;
      float2v x[SKR_P];
#pragma unroll
      for (int k = 0; k < SKR_P; ++k) {
        const float2v d = {vp[8 * k + part], vp[8 * k + part + 4]};
        x[k] = R[k] + d;
      }
      const float lse = skr_lse2(x, row_live);
      if (row_live && part == 0) {
        const float un = s_mu[line].x - lse;
        changed |= t == 1 || __float_as_uint(un) != __float_as_uint(hu[static_cast<size_t>(max(t - 2, 0)) * GR_LS + line]);
        hu[static_cast<size_t>(t - 1) * GR_LS + line] = un;
      }
    }
    __syncthreads();
    {
      const float* up = hu + static_cast<size_t>(t - 1) * GR_LS;
      float2v x[SKR_P];
#pragma unroll
      for (int k = 0; k < SKR_P; ++k) {
        const float2v d = {up[8 * k + part], up[8 * k + part + 4]};
        x[k] = C[k] + d;
      }
      const float lse = skr_lse2(x, col_live);
      if (col_live && part == 0) {
        const float vn = s_nu[line].x - lse;
        changed |= __float_as_uint(vn) != __float_as_uint(hv[static_cast<size_t>(t - 1) * GR_LS + line]);
        hv[static_cast<size_t>(t) * GR_LS + line] = vn;
      }
    }
    if (!__syncthreads_or(changed)) {
      t_last = t;
      break;
    }
  }
  // ---- du = rowsum(G), dv = colsum(G) over the valid entries ----
  float du_base;
  {
    float ar = 0.f, ac = 0.f;
#pragma unroll
    for (int k = 0; k < SKR_P; ++k) {
      const int j0 = 8 * k + part, j1 = j0 + 4;
      ar += R[k].x > -INFINITY ? gg[line * N1 + j0] : 0.f;
      ar += R[k].y > -INFINITY ? gg[line * N1 + j1] : 0.f;
      ac += C[k].x > -INFINITY ? gg[j0 * N1 + line] : 0.f;
      ac += C[k].y > -INFINITY ? gg[j1 * N1 + line] : 0.f;
    }
    du_base = quad_sum(ar);
    ac = quad_sum(ac);
    if (col_live && part == 0) s_nu[line].y = ac;
  }
  __syncthreads();
  // ---- the reverse iteration ----
  float2v dSr[SKR_P], dSc[SKR_P];
#pragma unroll
  for (int k = 0; k < SKR_P; ++k) {
    dSr[k] = float2v{0.f, 0.f};
    dSc[k] = float2v{0.f, 0.f};
  }
  for (int t = iters; t >= 1; --t) {
    {                                               // v-step, row layout: Pc = 2^(R + u_t,i + v_t,j - log_nu_j)
      const int tc = min(t, t_last);
      const float ui = hu[static_cast<size_t>(tc - 1) * GR_LS + lc];
      const float* vc = hv + static_cast<size_t>(tc) * GR_LS;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < SKR_P; ++k) {
        const int j0 = 8 * k + part, j1 = j0 + 4;
        const float2 n0 = s_nu[j0], n1 = s_nu[j1];
        const float t0 = exp2_hw((R[k].x + ui) + (vc[j0] - n0.x)) * n0.y;
        const float t1 = exp2_hw((R[k].y + ui) + (vc[j1] - n1.x)) * n1.y;
        dSr[k].x += t0;
        dSr[k].y += t1;
        acc += t0 + t1;
      }
      const float du = du_base - quad_sum(acc);     // the incoming du is rowsum(G) at t = T and 0 afterwards (the u-step consumed it)
      du_base = 0.f;
      if (row_live && part == 0) s_mu[line].y = du;
    }
    __syncthreads();
    {                                               // u-step, column layout: Pr = 2^(C + v_{t-1},j + u_t,i - log_mu_i)
      const float vj = hv[static_cast<size_t>(min(t - 1, t_last)) * GR_LS + lc];
      const float* uc = hu + static_cast<size_t>(min(t, t_last) - 1) * GR_LS;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < SKR_P; ++k) {
        const int i0 = 8 * k + part, i1 = i0 + 4;
        const float2 m0 = s_mu[i0], m1 = s_mu[i1];
        const float t0 = exp2_hw((C[k].x + vj) + (uc[i0] - m0.x)) * m0.y;
        const float t1 = exp2_hw((C[k].y + vj) + (uc[i1] - m1.x)) * m1.y;
        dSc[k].x += t0;
        dSc[k].y += t1;
        acc += t0 + t1;
      }
      const float dv = -quad_sum(acc);
      if (col_live && part == 0) s_nu[line].y = dv;
    }
    __syncthreads();
  }
  // ---- dS = G - dSr - dSc^T: the column part through the output buffer, then one pass in the row layout ----
  if (line < N1) {
#pragma unroll
    for (int k = 0; k < SKR_P; ++k) {
      const int i0 = 8 * k + part, i1 = i0 + 4;
      if (i0 < M1) dg[i0 * N1 + line] = dSc[k].x;
      if (i1 < M1) dg[i1 * N1 + line] = dSc[k].y;
    }
  }
  __syncthreads();
  float da = 0.f;                                   // this thread's share of the dustbin row and column
  if (line < M1) {
#pragma unroll
    for (int k = 0; k < SKR_P; ++k) {
      const int j0 = 8 * k + part, j1 = j0 + 4;
      if (j0 < N1) {
        const float g = R[k].x > -INFINITY ? gg[line * N1 + j0] : 0.f;
        const float val = (g - dSr[k].x) - dg[line * N1 + j0];
        dg[line * N1 + j0] = val;
        if (line == M || j0 == N) da += val;
      }
      if (j1 < N1) {
        const float g = R[k].y > -INFINITY ? gg[line * N1 + j1] : 0.f;
        const float val = (g - dSr[k].y) - dg[line * N1 + j1];
        dg[line * N1 + j1] = val;
        if (line == M || j1 == N) da += val;
      }
    }
  }
  s_red[tid] = da;
  __syncthreads();
  if (tid < 64) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < SKR_T / 64; ++q) s += s_red[tid + 64 * q];
    s = wave_sum(s);
    if (tid == 0) d_alpha_part[b] = s;
  }
}

// ---- general form: anything larger (the ~350 x 330 node level), one launch per half-step over the matrix in global memory / L2 ----------
// like forward form 3: a wavefront per row for everything that sums along a row, 64 columns x 16 row slices per workgroup for everything that
// sums along a column (slices folded through LDS in slice order).  dS itself is the accumulator (G, masked, at the start).  The duals are
// recorded in the workspace: [T][M+1] and [T+1][N+1] floats per problem.
struct GenWs {
  float *hu, *hv, *lmu, *lnu, *du, *dv;     // per problem: T*M1, (T+1)*N1, M1, N1, M1, N1 floats
  int*   ok;                                // per problem: it has a valid row and a valid column
};
enum { GG_INIT = 0, GG_FWD = 1, GG_REV = 2 };

__global__ __launch_bounds__(256) void k_gg_setup(const uint8_t* __restrict__ row_mask, const uint8_t* __restrict__ col_mask, int M, int N,
                                                  int iters, GenWs w) {
  __shared__ int s_nr, s_nc;
  const int64_t b = blockIdx.x;
  const int M1 = M + 1, N1 = N + 1;
  if (threadIdx.x == 0) {
    s_nr = 0;
    s_nc = 0;
  }
  __syncthreads();
  int cr = 0, cc = 0;
  for (int i = threadIdx.x; i < M; i += blockDim.x) cr += row_mask[b * M + i] ? 1 : 0;
  for (int j = threadIdx.x; j < N; j += blockDim.x) cc += col_mask[b * N + j] ? 1 : 0;
  if (cr) atomicAdd(&s_nr, cr);
  if (cc) atomicAdd(&s_nc, cc);
  __syncthreads();
  const int nr = s_nr, nc = s_nc;
  const bool ok = nr > 0 && nc > 0;
  if (threadIdx.x == 0) w.ok[b] = ok ? 1 : 0;
  const float norm = ok ? -logf(static_cast<float>(nr + nc)) : 0.f;
  for (int i = threadIdx.x; i < M1; i += blockDim.x) w.lmu[b * M1 + i] = !ok ? 0.f : (i < M ? norm : logf(static_cast<float>(nc)) + norm);
  for (int j = threadIdx.x; j < N1; j += blockDim.x) {
    w.lnu[b * N1 + j] = !ok ? 0.f : (j < N ? norm : logf(static_cast<float>(nr)) + norm);
    w.hv[b * (iters + 1) * N1 + j] = 0.f;           // v_0
  }
}

// one wavefront per (problem, row)
template <int MODE>
__global__ __launch_bounds__(256) void k_gg_rows(const float* __restrict__ S0, const float* __restrict__ G, const uint8_t* __restrict__ row_mask,
                                                 const uint8_t* __restrict__ col_mask, int M, int N, int iters, int t, int first, float* dS,
                                                 GenWs w) {
  const int64_t b = blockIdx.y;
  const int M1 = M + 1, N1 = N + 1, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M1) return;
  const bool ok = w.ok[b] != 0 && (i == M || row_mask[b * M + i] != 0);
  const uint8_t* cm = col_mask + b * N;
  const float* s = S0 + (b * M1 + i) * N1;
  float* d = dS + (b * M1 + i) * N1;
  if (MODE == GG_INIT) {
    const float* g = G + (b * M1 + i) * N1;
    float acc = 0.f;
    for (int j = lane; j < N1; j += 64) {
      const float x = (ok && (j == N || cm[j])) ? g[j] : 0.f;
      d[j] = x;
      acc += x;
    }
    acc = wave_sum(acc);
    if (lane == 0) w.du[b * M1 + i] = acc;
    return;
  }
  if (!ok) return;
  if (MODE == GG_FWD) {                             // u_t,i = log_mu_i - LSE_j(S_ij + v_{t-1},j)
    const float* vp = w.hv + (b * (iters + 1) + (t - 1)) * N1;
    float mx = -INFINITY;
    for (int j = lane; j < N1; j += 64)
      if (j == N || cm[j]) mx = fmaxf(mx, s[j] + vp[j]);
#pragma unroll
    for (int q = 32; q >= 1; q >>= 1) mx = fmaxf(mx, __shfl_xor(mx, q));
    float sum = 0.f;
    for (int j = lane; j < N1; j += 64)
      if (j == N || cm[j]) sum += __expf(s[j] + vp[j] - mx);
    sum = wave_sum(sum);
    if (lane == 0) w.hu[(b * iters + (t - 1)) * M1 + i] = w.lmu[b * M1 + i] - (mx + __logf(sum));
  } else {                                          // v-step reverse: Pc = exp(S + u_t,i + v_t,j - log_nu_j); dS -= Pc dv; du -= Pc @ dv
    const float ui = w.hu[(b * iters + (t - 1)) * M1 + i];
    const float* vc = w.hv + (b * (iters + 1) + t) * N1;
    const float* lnu = w.lnu + b * N1;
    const float* dv = w.dv + b * N1;
    float acc = 0.f;
    for (int j = lane; j < N1; j += 64)
      if (j == N || cm[j]) {
        const float x = __expf((s[j] + ui) + (vc[j] - lnu[j])) * dv[j];
        d[j] -= x;
        acc += x;
      }
    acc = wave_sum(acc);
    if (lane == 0) w.du[b * M1 + i] = (first ? w.du[b * M1 + i] : 0.f) - acc;
  }
}

// 64 columns x 16 row slices per workgroup
template <int MODE>
__global__ __launch_bounds__(1024) void k_gg_cols(const float* __restrict__ S0, const uint8_t* __restrict__ row_mask,
                                                  const uint8_t* __restrict__ col_mask, int M, int N, int iters, int t, float* dS, GenWs w) {
  __shared__ float s_part[16][64];
  const int64_t b = blockIdx.y;
  if (!w.ok[b]) {                                   // block-uniform
    if (MODE == GG_INIT && threadIdx.x < 64 && blockIdx.x * 64 + threadIdx.x <= N) w.dv[b * (N + 1) + blockIdx.x * 64 + threadIdx.x] = 0.f;
    return;
  }
  const int M1 = M + 1, N1 = N + 1;
  const int c = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + c;
  const bool live = j < N1 && (j == N || col_mask[b * N + j] != 0);
  const uint8_t* rm = row_mask + b * M;
  const float* s = S0 + b * M1 * N1;
  float* d = dS + b * M1 * N1;
  float acc = 0.f, mx = -INFINITY;
  if (MODE == GG_INIT) {                            // dv = colsum of the masked G that k_gg_rows<GG_INIT> left in dS
    if (live)
      for (int i = slice; i < M1; i += 16) acc += d[i * N1 + j];
  } else if (MODE == GG_FWD) {                      // v_t,j = log_nu_j - LSE_i(S_ij + u_t,i)
    const float* up = w.hu + (b * iters + (t - 1)) * M1;
    if (live)
      for (int i = slice; i < M1; i += 16)
        if (i == M || rm[i]) mx = fmaxf(mx, s[i * N1 + j] + up[i]);
    s_part[slice][c] = mx;
    __syncthreads();
    mx = s_part[0][c];
#pragma unroll
    for (int q = 1; q < 16; ++q) mx = fmaxf(mx, s_part[q][c]);
    __syncthreads();
    if (live)
      for (int i = slice; i < M1; i += 16)
        if (i == M || rm[i]) acc += __expf(s[i * N1 + j] + up[i] - mx);
  } else {                                          // u-step reverse: Pr = exp(S + v_{t-1},j + u_t,i - log_mu_i); dS -= Pr du; dv = -(Pr^T @ du)
    const float* uc = w.hu + (b * iters + (t - 1)) * M1;
    const float* lmu = w.lmu + b * M1;
    const float* du = w.du + b * M1;
    if (live) {
      const float vj = w.hv[(b * (iters + 1) + (t - 1)) * N1 + j];
      for (int i = slice; i < M1; i += 16)
        if (i == M || rm[i]) {
          const float x = __expf((s[i * N1 + j] + vj) + (uc[i] - lmu[i])) * du[i];
          d[i * N1 + j] -= x;
          acc += x;
        }
    }
  }
  s_part[slice][c] = acc;
  __syncthreads();
  if (slice == 0 && j < N1) {
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) tot += s_part[q][c];
    if (MODE == GG_INIT) w.dv[b * N1 + j] = live ? tot : 0.f;
    else if (MODE == GG_FWD) {
      if (live) w.hv[(b * (iters + 1) + t) * N1 + j] = w.lnu[b * N1 + j] - (mx + __logf(tot));
    } else w.dv[b * N1 + j] = live ? -tot : 0.f;
  }
}

// d_alpha_part[b] = the dustbin row and column of dS, summed in one fixed order
__global__ __launch_bounds__(256) void k_gg_alpha(const float* __restrict__ dS, int M, int N, const GenWs w, float* __restrict__ d_alpha_part) {
  __shared__ float s_red[256];
  const int64_t b = blockIdx.x;
  const int M1 = M + 1, N1 = N + 1;
  const float* d = dS + b * M1 * N1;
  float acc = 0.f;
  if (w.ok[b]) {
    for (int j = threadIdx.x; j < N1; j += 256) acc += d[M * N1 + j];
    for (int i = threadIdx.x; i < M; i += 256) acc += d[i * N1 + N];
  }
  s_red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < 64) {
    float s = (s_red[threadIdx.x] + s_red[threadIdx.x + 64]) + (s_red[threadIdx.x + 128] + s_red[threadIdx.x + 192]);
    s = wave_sum(s);
    if (threadIdx.x == 0) d_alpha_part[b] = s;
  }
}

// Which kernels a call takes and what they need:
//   form 0  M + 1, N + 1 <= 132: resident (k_sinkhorn_grad_res), the recorded duals in LDS when (2 iters + 1) * GR_LS floats fit
//           GR_LDS_ROOM, in the workspace otherwise
//   form 1  one launch per half-step (k_gg_rows / k_gg_cols), duals, marginals and du / dv in the workspace
struct Plan {
  int    form;
  bool   hist_lds;
  size_t hist_floats;       // form 0: per problem
  size_t ws_bytes;
};
static GenWs gen_carve(void* ws, size_t cap, int64_t B, int M, int N, int iters, size_t* used) {
  const size_t M1 = M + 1, N1 = N + 1, b = static_cast<size_t>(B), T = iters;
  Carver cv(ws, cap);
  GenWs w;
  w.hu = cv.take<float>(b * T * M1);
  w.hv = cv.take<float>(b * (T + 1) * N1);
  w.lmu = cv.take<float>(b * M1);
  w.lnu = cv.take<float>(b * N1);
  w.du = cv.take<float>(b * M1);
  w.dv = cv.take<float>(b * N1);
  w.ok = cv.take<int>(b);
  *used = cv.off;
  return w;
}
static Plan skg_plan(int64_t B, int M, int N, int iters) {
  Plan p = {1, false, 0, 0};
  if (M + 1 <= SKR_LINES && N + 1 <= SKR_LINES) {
    p.form = 0;
    p.hist_floats = (2 * static_cast<size_t>(iters) + 1) * GR_LS;
    p.hist_lds = p.hist_floats * sizeof(float) <= GR_LDS_ROOM;
    p.ws_bytes = p.hist_lds ? 0 : static_cast<size_t>(B) * p.hist_floats * sizeof(float);
  } else {
    gen_carve(nullptr, 0, B, M, N, iters, &p.ws_bytes);
  }
  p.ws_bytes = align_up(std::max<size_t>(p.ws_bytes, 1));
  return p;
}

}  // namespace skg
}  // namespace lcr

using namespace lcr;

extern "C" int lcr_log_sinkhorn_grad_ws_bytes(int64_t B, int M, int N, int iters, size_t* bytes) {
  if (!bytes || B < 0 || M < 1 || N < 1 || iters < 1)
    return refuse(LCR_EARG, "lcr_log_sinkhorn_grad_ws_bytes: null pointer or outside the domain (B >= 0, M, N, iters >= 1): B=%lld M=%d N=%d iters=%d",
                  static_cast<long long>(B), M, N, iters);
  *bytes = skg::skg_plan(B, M, N, iters).ws_bytes;
  return LCR_OK;
}

extern "C" int lcr_log_sinkhorn_grad_form(int64_t B, int M, int N, int* form) {
  if (!form || B < 0 || M < 1 || N < 1)
    return refuse(LCR_EARG, "lcr_log_sinkhorn_grad_form: null pointer or outside the domain (B >= 0, M, N >= 1): B=%lld M=%d N=%d", static_cast<long long>(B), M, N);
  *form = skg::skg_plan(B, M, N, 1).form;
  return LCR_OK;
}

extern "C" int lcr_log_sinkhorn_grad(const float* S0, const float* G, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N,
                                     int iters, float inf_val, float* dS, float* d_alpha_part, void* ws, size_t ws_bytes, void* stream) {
  (void)inf_val;      // masked lines are taken from the masks, whatever S0 holds there
  if (B < 0 || M < 1 || N < 1 || iters < 1)
    return refuse(LCR_EARG, "lcr_log_sinkhorn_grad: outside the domain (B >= 0, M, N, iters >= 1): B=%lld M=%d N=%d iters=%d", static_cast<long long>(B), M, N, iters);
  if (B == 0) return LCR_OK;
  if (!S0 || !G || !row_mask || !col_mask || !dS || !d_alpha_part || !ws) return refuse(LCR_EARG, "lcr_log_sinkhorn_grad: null pointer");
  const skg::Plan p = skg::skg_plan(B, M, N, iters);
  if (ws_bytes < p.ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_log_sinkhorn_grad", ws_bytes, p.ws_bytes);
  hipStream_t st = ST(stream);
  if (p.form == 0) {
    if (B > 0x7fffffff) return refuse(LCR_EARG, "lcr_log_sinkhorn_grad: more than 2^31-1 problems (B=%lld)", static_cast<long long>(B));
    const dim3 grid(static_cast<unsigned>(B));
    if (p.hist_lds) {
      static DynLds opt_in;                                // > 64 KB of dynamic LDS needs an explicit opt-in
      if (opt_in.need(reinterpret_cast<const void*>(&skg::k_sinkhorn_grad_res<true>), skg::GR_LDS_ROOM) != hipSuccess)
        return refuse(LCR_EHIP, "lcr_log_sinkhorn_grad: cannot reserve dynamic LDS for the recorded duals");
      hipLaunchKernelGGL(skg::k_sinkhorn_grad_res<true>, grid, dim3(SKR_T), p.hist_floats * sizeof(float), st, S0, G, row_mask, col_mask, M, N,
                         iters, dS, d_alpha_part, static_cast<float*>(nullptr));
    } else {
      hipLaunchKernelGGL(skg::k_sinkhorn_grad_res<false>, grid, dim3(SKR_T), 0, st, S0, G, row_mask, col_mask, M, N, iters, dS, d_alpha_part,
                         static_cast<float*>(ws));
    }
    return check_launch("lcr_log_sinkhorn_grad");
  }
  if (B > 65535) return refuse(LCR_EARG, "lcr_log_sinkhorn_grad: more than 65535 problems in the launch-per-half-iteration form (B=%lld)", static_cast<long long>(B));
  size_t used = 0;
  const skg::GenWs w = skg::gen_carve(ws, ws_bytes, B, M, N, iters, &used);
  const int nb = static_cast<int>(B);
  const dim3 grow((M + 1 + 3) / 4, nb), gcol((N + 1 + 63) / 64, nb);
  hipLaunchKernelGGL(skg::k_gg_setup, dim3(nb), dim3(256), 0, st, row_mask, col_mask, M, N, iters, w);
  for (int t = 1; t <= iters; ++t) {
    hipLaunchKernelGGL(skg::k_gg_rows<skg::GG_FWD>, grow, dim3(256), 0, st, S0, G, row_mask, col_mask, M, N, iters, t, 0, dS, w);
    hipLaunchKernelGGL(skg::k_gg_cols<skg::GG_FWD>, gcol, dim3(1024), 0, st, S0, row_mask, col_mask, M, N, iters, t, dS, w);
  }
  hipLaunchKernelGGL(skg::k_gg_rows<skg::GG_INIT>, grow, dim3(256), 0, st, S0, G, row_mask, col_mask, M, N, iters, 0, 0, dS, w);
  hipLaunchKernelGGL(skg::k_gg_cols<skg::GG_INIT>, gcol, dim3(1024), 0, st, S0, row_mask, col_mask, M, N, iters, 0, dS, w);
  for (int t = iters; t >= 1; --t) {
    hipLaunchKernelGGL(skg::k_gg_rows<skg::GG_REV>, grow, dim3(256), 0, st, S0, G, row_mask, col_mask, M, N, iters, t, t == iters ? 1 : 0, dS, w);
    hipLaunchKernelGGL(skg::k_gg_cols<skg::GG_REV>, gcol, dim3(1024), 0, st, S0, row_mask, col_mask, M, N, iters, t, dS, w);
  }
  hipLaunchKernelGGL(skg::k_gg_alpha, dim3(nb), dim3(256), 0, st, dS, M, N, w, d_alpha_part);
  return check_launch("lcr_log_sinkhorn_grad");
}
