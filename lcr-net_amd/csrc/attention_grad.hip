// attention_grad.hip — reverse passes of the 3D-RoFormer attention block (attention.hip), fp32.
//
// The forward keeps nothing but its inputs and its output, so the reverse pass of the fused attention recomputes the softmax row statistic:
//   k_ag_stats : per (problem, head, 32-query tile) the forward's key walk once more (S^T = K·Q^T on the matrix cores, running max / sum per
//                lane, four wavefronts merged through LDS) -> L = m + log2 l in the forward's base-2 units, and D = sum_d dO·O as the diagonal
//                of one more 32x32 MFMA product (dO·O^T): the same instruction sequence that forms dP = dO·V^T below, so that with a single
//                key (O == V) dP - D is exactly zero;
//   k_ag_dkdv  : one workgroup per (problem, head, 32-key tile), a lane owns one KEY; its wavefronts take the query tiles round-robin:
//                S = Q·K^T, P = exp2(S - L), dV^T += dO^T·P, dP = dO·V^T, dS = P∘(dP - D), dK^T += Q^T·dS;
//   k_ag_dq    : one workgroup per (problem, head, 32-query tile), a lane owns one QUERY; its wavefronts take the key tiles round-robin:
//                S^T = K·Q^T, P^T, dP^T = V·dO^T, dS^T, dQ^T += K^T·dS^T.
// As in the forward the 32x32 result of one MFMA group feeds the next one as its B operand straight from the accumulator registers
// (attention.h's acc_as_b), and tiles reach LDS through the forward's load_tile.  The four partial sums of a workgroup are added in LDS in wavefront order: no floating-point atomics, a
// problem's bytes do not depend on its batch.
//   k_rotary_grad     : dx = R(-theta)·dy, dtheta = dy0·(-y1) + dy1·y0 from the POST-rotary y (d y / d theta = rot(y));
//   k_ln_grad / k_ln_grad_reduce : LayerNorm(a + b) reverse; mean and rstd recomputed per row as the forward computes them, dgamma / dbeta
//                as per-wavefront partial column sums over 16 rows each, then one wavefront per column over the partials.
#include <algorithm>
#include <cmath>

#include "attention.h"

namespace lcr {

struct AgSeg {
  int P;
  int q_off[AT_MAX_P + 1], k_off[AT_MAX_P + 1];        // row offsets
  int qt_off[AT_MAX_P + 1], kt_off[AT_MAX_P + 1];      // first 32-query tile / first 32-key tile of every problem
};

// row of accumulator register r in this lane's half
__device__ __forceinline__ int ag_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// grid (query tiles of all problems, heads).  Lq / Dq: [heads][total queries]
__global__ __launch_bounds__(64 * AT_SPLIT) void k_ag_stats(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ out,
                                                            const float* __restrict__ d_out, AgSeg seg, int heads, float scale,
                                                            float* __restrict__ Lq, float* __restrict__ Dq) {
  __shared__ __attribute__((aligned(16))) float s_q[AT_TILE], s_k[AT_SPLIT][AT_TILE], s_do[AT_TILE], s_o[AT_TILE];
  __shared__ float s_m[AT_SPLIT][32], s_l[AT_SPLIT][32];
  const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
  const int wsp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = cloud_of(seg.qt_off, seg.P, static_cast<int>(blockIdx.x));
  const int head = blockIdx.y, ld = heads * AT_D;
  const int64_t qo = seg.q_off[p], ko = seg.k_off[p];
  const int64_t Nq = seg.q_off[p + 1] - qo, Nk = seg.k_off[p + 1] - ko, Ntot = seg.q_off[seg.P];
  const int64_t q0 = static_cast<int64_t>(static_cast<int>(blockIdx.x) - seg.qt_off[p]) * 32;
  if (wsp == 0) load_tile(q + qo * ld, Nq, q0, ld, head * AT_D, s_q);
  __syncthreads();
  float qf[16];
  const float scale2 = scale * 1.44269504088896341f;
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) qf[kk] = s_q[col * AT_LD + 2 * kk + half] * scale2;
  float m = -INFINITY, l = 0.f;
  float* sk = s_k[wsp];
  for (int64_t k0 = 32 * static_cast<int64_t>(wsp); k0 < Nk; k0 += 32 * AT_SPLIT) {
    wave_sync();
    load_tile(k + ko * ld, Nk, k0, ld, head * AT_D, sk);
    wave_sync();
    floatx16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x2f32(sk[col * AT_LD + 2 * kk + half], qf[kk], s, 0, 0, 0);
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (k0 + ag_row(r, half) >= Nk) s[r] = -INFINITY;
      tmax = fmaxf(tmax, s[r]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float m_new = fmaxf(m, tmax);                        // finite: every tile holds at least one valid key
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) psum += __builtin_amdgcn_exp2f(s[r] - m_new);
    psum += __shfl_xor(psum, 32);
    l = l * __builtin_amdgcn_exp2f(m - m_new) + psum;
    m = m_new;
  }
  if (half == 0) {
    s_m[wsp][col] = m;
    s_l[wsp][col] = l;
  }
  __syncthreads();
  if (wsp == 0) {
    float mm = -INFINITY;
#pragma unroll
    for (int u = 0; u < AT_SPLIT; ++u) mm = fmaxf(mm, s_m[u][col]);
    float lsum = 0.f;
#pragma unroll
    for (int u = 0; u < AT_SPLIT; ++u) lsum += s_l[u][col] * __builtin_amdgcn_exp2f(s_m[u][col] - mm);
    if (half == 0 && q0 + col < Nq) Lq[head * Ntot + qo + q0 + col] = mm + __builtin_amdgcn_logf(lsum);     // v_log_f32: base 2
  } else if (wsp == 1) {
    load_tile(d_out + qo * ld, Nq, q0, ld, head * AT_D, s_do);
    load_tile(out + qo * ld, Nq, q0, ld, head * AT_D, s_o);
    wave_sync();
    floatx16 acc;      // acc[query i][query j] = sum_d dO[i][d] O[j][d]; wanted: the diagonal
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s_do[col * AT_LD + 2 * kk + half], s_o[col * AT_LD + 2 * kk + half], acc, 0, 0, 0);
    float dsum = 0.f;
    bool mine = false;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (ag_row(r, half) == col) dsum = acc[r], mine = true;
    if (mine && q0 + col < Nq) Dq[head * Ntot + qo + q0 + col] = dsum;
  }
}

// grid (key tiles of all problems, heads)
__global__ __launch_bounds__(64 * AT_SPLIT) void k_ag_dkdv(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                           const float* __restrict__ d_out, const float* __restrict__ Lq, const float* __restrict__ Dq,
                                                           AgSeg seg, int heads, float scale, float* __restrict__ dk, float* __restrict__ dv) {
  __shared__ __attribute__((aligned(16))) float s_k[AT_TILE], s_v[AT_TILE];
  __shared__ __attribute__((aligned(16))) float s_buf[2 * AT_SPLIT * AT_TILE];      // per wavefront a Q and a dO tile; afterwards the merge buffer
  __shared__ float s_L[AT_SPLIT][32], s_D[AT_SPLIT][32];
  static_assert(2 * AT_SPLIT * AT_TILE >= AT_SPLIT * 2 * 16 * 64, "merge buffer");
  const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
  const int wsp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = cloud_of(seg.kt_off, seg.P, static_cast<int>(blockIdx.x));
  const int head = blockIdx.y, ld = heads * AT_D;
  const int64_t qo = seg.q_off[p], ko = seg.k_off[p];
  const int64_t Nq = seg.q_off[p + 1] - qo, Nk = seg.k_off[p + 1] - ko, Ntot = seg.q_off[seg.P];
  const int64_t k0 = static_cast<int64_t>(static_cast<int>(blockIdx.x) - seg.kt_off[p]) * 32;
  if (wsp == 0) load_tile(k + ko * ld, Nk, k0, ld, head * AT_D, s_k);
  if (wsp == 1) load_tile(v + ko * ld, Nk, k0, ld, head * AT_D, s_v);
  __syncthreads();
  float kf[16], vf[16];
  const float scale2 = scale * 1.44269504088896341f;
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    kf[kk] = s_k[col * AT_LD + 2 * kk + half];               // B[kd][j = key] of S = Q·K^T
    vf[kk] = s_v[col * AT_LD + 2 * kk + half];               // B[kd][j = key] of dP = dO·V^T
  }
  const bool key_ok = k0 + col < Nk;
  float* sq = s_buf + (2 * wsp) * AT_TILE;
  float* sdo = s_buf + (2 * wsp + 1) * AT_TILE;
  floatx16 adv, adk;     // dV^T[d][key], dK^T[d][key]
#pragma unroll
  for (int r = 0; r < 16; ++r) adv[r] = 0.f, adk[r] = 0.f;
  for (int64_t q0 = 32 * static_cast<int64_t>(wsp); q0 < Nq; q0 += 32 * AT_SPLIT) {
    wave_sync();
    load_tile(q + qo * ld, Nq, q0, ld, head * AT_D, sq);
    load_tile(d_out + qo * ld, Nq, q0, ld, head * AT_D, sdo);
    if (lane < 32) {
      const bool ok = q0 + lane < Nq;
      s_L[wsp][lane] = ok ? Lq[head * Ntot + qo + q0 + lane] : 0.f;
      s_D[wsp][lane] = ok ? Dq[head * Ntot + qo + q0 + lane] : 0.f;
    }
    wave_sync();
    floatx16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f, dp[r] = 0.f;
    // S[query][key] = sum_d Q[query][d] K[key][d]; q is scaled as in k_ag_stats ((q scale2) k, not q (k scale2)): the products, and with
    // them S - L, carry the bits L was formed from (one key: P = exp2(0) = 1 exactly)
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x2f32(sq[col * AT_LD + 2 * kk + half] * scale2, kf[kk], s, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ag_row(r, half);
      s[r] = (key_ok && q0 + row < Nq) ? __builtin_amdgcn_exp2f(s[r] - s_L[wsp][row]) : 0.f;      // P
    }
    // dV^T[d][key] += sum_query dO[query][d] P[query][key]
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) adv = __builtin_amdgcn_mfma_f32_32x32x2f32(sdo[(2 * kk + half) * AT_LD + col], acc_as_b(s, kk, half), adv, 0, 0, 0);
    // dP[query][key] = sum_d dO[query][d] V[key][d]
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(sdo[col * AT_LD + 2 * kk + half], vf[kk], dp, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = s[r] * (dp[r] - s_D[wsp][ag_row(r, half)]);      // dS
    // dK^T[d][key] += sum_query Q[query][d] dS[query][key]
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) adk = __builtin_amdgcn_mfma_f32_32x32x2f32(sq[(2 * kk + half) * AT_LD + col], acc_as_b(s, kk, half), adk, 0, 0, 0);
  }
  __syncthreads();                                             // every wavefront is done with its tiles: s_buf becomes the merge buffer
  float* mg = s_buf;                                           // [wavefront][dv | dk][16][64]
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    mg[((wsp * 2 + 0) * 16 + r) * 64 + lane] = adv[r];
    mg[((wsp * 2 + 1) * 16 + r) * 64 + lane] = adk[r];
  }
  __syncthreads();
  if (key_ok) {
#pragma unroll
    for (int rr = 0; rr < 16 / AT_SPLIT; ++rr) {
      const int r = wsp * (16 / AT_SPLIT) + rr;
      float sv = 0.f, sk2 = 0.f;
#pragma unroll
      for (int u = 0; u < AT_SPLIT; ++u) {                      // fixed order
        sv += mg[((u * 2 + 0) * 16 + r) * 64 + lane];
        sk2 += mg[((u * 2 + 1) * 16 + r) * 64 + lane];
      }
      const int64_t at = (ko + k0 + col) * ld + head * AT_D + ag_row(r, half);
      dv[at] = sv;
      dk[at] = sk2 * scale;
    }
  }
}

// grid (query tiles of all problems, heads)
__global__ __launch_bounds__(64 * AT_SPLIT) void k_ag_dq(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                         const float* __restrict__ d_out, const float* __restrict__ Lq, const float* __restrict__ Dq,
                                                         AgSeg seg, int heads, float scale, float* __restrict__ dq) {
  __shared__ __attribute__((aligned(16))) float s_q[AT_TILE], s_do[AT_TILE];
  __shared__ __attribute__((aligned(16))) float s_buf[2 * AT_SPLIT * AT_TILE];      // per wavefront a K and a V tile; afterwards the merge buffer
  const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
  const int wsp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = cloud_of(seg.qt_off, seg.P, static_cast<int>(blockIdx.x));
  const int head = blockIdx.y, ld = heads * AT_D;
  const int64_t qo = seg.q_off[p], ko = seg.k_off[p];
  const int64_t Nq = seg.q_off[p + 1] - qo, Nk = seg.k_off[p + 1] - ko, Ntot = seg.q_off[seg.P];
  const int64_t q0 = static_cast<int64_t>(static_cast<int>(blockIdx.x) - seg.qt_off[p]) * 32;
  if (wsp == 0) load_tile(q + qo * ld, Nq, q0, ld, head * AT_D, s_q);
  if (wsp == 1) load_tile(d_out + qo * ld, Nq, q0, ld, head * AT_D, s_do);
  __syncthreads();
  float qf[16], dof[16];
  const float scale2 = scale * 1.44269504088896341f;
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    qf[kk] = s_q[col * AT_LD + 2 * kk + half] * scale2;      // B[kd][j = query] of S^T = K·Q^T
    dof[kk] = s_do[col * AT_LD + 2 * kk + half];             // B[kd][j = query] of dP^T = V·dO^T
  }
  const bool q_ok = q0 + col < Nq;
  const float Lr = q_ok ? Lq[head * Ntot + qo + q0 + col] : 0.f;
  const float Dr = q_ok ? Dq[head * Ntot + qo + q0 + col] : 0.f;
  float* sk = s_buf + (2 * wsp) * AT_TILE;
  float* sv = s_buf + (2 * wsp + 1) * AT_TILE;
  floatx16 adq;     // dQ^T[d][query]
#pragma unroll
  for (int r = 0; r < 16; ++r) adq[r] = 0.f;
  for (int64_t k0 = 32 * static_cast<int64_t>(wsp); k0 < Nk; k0 += 32 * AT_SPLIT) {
    wave_sync();
    load_tile(k + ko * ld, Nk, k0, ld, head * AT_D, sk);
    load_tile(v + ko * ld, Nk, k0, ld, head * AT_D, sv);
    wave_sync();
    floatx16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f, dp[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x2f32(sk[col * AT_LD + 2 * kk + half], qf[kk], s, 0, 0, 0);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(sv[col * AT_LD + 2 * kk + half], dof[kk], dp, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pr = (q_ok && k0 + ag_row(r, half) < Nk) ? __builtin_amdgcn_exp2f(s[r] - Lr) : 0.f;
      s[r] = pr * (dp[r] - Dr);                                                      // dS^T[key][query]
    }
    // dQ^T[d][query] += sum_key K[key][d] dS^T[key][query]
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) adq = __builtin_amdgcn_mfma_f32_32x32x2f32(sk[(2 * kk + half) * AT_LD + col], acc_as_b(s, kk, half), adq, 0, 0, 0);
  }
  __syncthreads();
  float* mg = s_buf;                                           // [wavefront][16][64]
#pragma unroll
  for (int r = 0; r < 16; ++r) mg[(wsp * 16 + r) * 64 + lane] = adq[r];
  __syncthreads();
  if (q_ok) {
#pragma unroll
    for (int rr = 0; rr < 16 / AT_SPLIT; ++rr) {
      const int r = wsp * (16 / AT_SPLIT) + rr;
      float sum = 0.f;
#pragma unroll
      for (int u = 0; u < AT_SPLIT; ++u) sum += mg[(u * 16 + r) * 64 + lane];      // fixed order
      dq[(qo + q0 + col) * ld + head * AT_D + ag_row(r, half)] = sum * scale;
    }
  }
}

// y, dy [N, H*32], theta [N, H*16] -> dx [N, H*32], dtheta [N, H*16]
__global__ __launch_bounds__(256) void k_rotary_grad(const float* __restrict__ y, const float* __restrict__ dy, const float* __restrict__ theta, int64_t N,
                                                     int heads, float* __restrict__ dx, float* __restrict__ dtheta) {
  const int pairs = heads * 16;
  const int64_t total = N * pairs;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < total; t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float s, c;
    sincosf(theta[t], &s, &c);
    const float2 yv = *reinterpret_cast<const float2*>(y + 2 * t);
    const float2 g = *reinterpret_cast<const float2*>(dy + 2 * t);
    *reinterpret_cast<float2*>(dx + 2 * t) = make_float2(g.x * c + g.y * s, g.y * c - g.x * s);
    dtheta[t] = g.y * yv.x - g.x * yv.y;
  }
}

constexpr int LNG_ROWS = 16;   // rows per wavefront = rows per partial column sum

// one wavefront per LNG_ROWS rows; part [wavefronts][2][D]: its sums of dy·xhat and of dy
__global__ __launch_bounds__(256) void k_ln_grad(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ gamma,
                                                 const float* __restrict__ dy, int64_t N, int D, float eps, float* __restrict__ dx,
                                                 float* __restrict__ part) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t g = static_cast<int64_t>(blockIdx.x) * 4 + w;
  if (g * LNG_ROWS >= N) return;                         // whole wavefront; no block-wide barrier below
  float dg[16], db[16], gam[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    dg[i] = 0.f, db[i] = 0.f;
    const int c = lane + 64 * i;
    gam[i] = c < D ? gamma[c] : 0.f;
  }
  const int64_t n_end = (g + 1) * LNG_ROWS < N ? (g + 1) * LNG_ROWS : N;
  for (int64_t n = g * LNG_ROWS; n < n_end; ++n) {
    float vals[16], gy[16];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = lane + 64 * i;
      if (c < D) {
        vals[i] = a[n * D + c] + (b ? b[n * D + c] : 0.f);
        s += vals[i];
      } else {
        vals[i] = 0.f;
      }
    }
    s = wave_sum(s);
    float mean = s / D;
    float sr = 0.f;                                      // k_add_layernorm's correction step of the mean
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (lane + 64 * i < D) sr += vals[i] - mean;
    mean += wave_sum(sr) / D;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (lane + 64 * i < D) {
        const float d = vals[i] - mean;
        ss = fmaf(d, d, ss);
      }
    ss = wave_sum(ss);
    const float rstd = 1.f / sqrtf(ss / D + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = lane + 64 * i;
      if (c < D) {
        const float xh = (vals[i] - mean) * rstd, d = dy[n * D + c];
        vals[i] = xh;
        gy[i] = d * gam[i];
        s1 += gy[i];
        s2 = fmaf(gy[i], xh, s2);
        dg[i] = fmaf(d, xh, dg[i]);
        db[i] += d;
      } else {
        gy[i] = 0.f;
      }
    }
    s1 = wave_sum(s1) / D;
    s2 = wave_sum(s2) / D;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = lane + 64 * i;
      if (c < D) dx[n * D + c] = rstd * ((gy[i] - s1) - vals[i] * s2);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = lane + 64 * i;
    if (c < D) {
      part[(g * 2 + 0) * D + c] = dg[i];
      part[(g * 2 + 1) * D + c] = db[i];
    }
  }
}

// one wavefront per (which, column): the partials in a fixed order (lane l takes l, l + 64, ...; then the fixed tree of wave_sum)
__global__ __launch_bounds__(256) void k_ln_grad_reduce(const float* __restrict__ part, int64_t nparts, int D, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int id = static_cast<int>(blockIdx.x) * 4 + w;
  if (id >= 2 * D) return;
  const int which = id / D, c = id - which * D;
  float s = 0.f;
  for (int64_t g = lane; g < nparts; g += 64) s += part[(g * 2 + which) * D + c];
  s = wave_sum(s);
  if (lane == 0) (which == 0 ? dgamma : dbeta)[c] = s;
}

}  // namespace lcr

using namespace lcr;

extern "C" int lcr_attention_grad_ws_bytes(int64_t n_queries, int heads, size_t* bytes) {
  if (!bytes || n_queries < 0 || heads < 1) return refuse(LCR_EARG, "lcr_attention_grad_ws_bytes: bad argument");
  *bytes = align_up(static_cast<size_t>(2) * static_cast<size_t>(heads) * static_cast<size_t>(n_queries) * sizeof(float));
  return LCR_OK;
}

extern "C" int lcr_attention_seg_grad_f32(const float* q, const float* k, const float* v, const float* out, const float* d_out,
                                          const int64_t* q_len_host, const int64_t* k_len_host, int P, int heads, int head_dim, float* dq, float* dk,
                                          float* dv, void* ws, size_t ws_bytes, void* stream) {
  if (!q || !k || !v || !out || !d_out || !dq || !dk || !dv || !q_len_host || !k_len_host || P < 1 || P > AT_MAX_P || heads < 1 || heads > 65535 ||
      head_dim != AT_D)
    return refuse(LCR_EARG, "lcr_attention_seg_grad_f32: bad argument (head_dim must be %d, 1 <= P <= %d)", AT_D, AT_MAX_P);
  AgSeg seg;
  seg.P = P;
  int64_t qo = 0, ko = 0, qt = 0, kt = 0;
  for (int p = 0; p < P; ++p) {
    if (q_len_host[p] < 0 || k_len_host[p] < 1)
      return refuse(LCR_EARG, "lcr_attention_seg_grad_f32: problem %d has %lld queries / %lld keys (keys >= 1)", p, static_cast<long long>(q_len_host[p]),
                    static_cast<long long>(k_len_host[p]));
    seg.q_off[p] = static_cast<int>(qo);
    seg.k_off[p] = static_cast<int>(ko);
    seg.qt_off[p] = static_cast<int>(qt);
    seg.kt_off[p] = static_cast<int>(kt);
    qo += q_len_host[p];
    ko += k_len_host[p];
    qt += (q_len_host[p] + 31) / 32;
    kt += (k_len_host[p] + 31) / 32;
    if (qo > 2147483647 || ko > 2147483647) return refuse(LCR_EARG, "lcr_attention_seg_grad_f32: more than 2^31-1 stacked rows");
  }
  seg.q_off[P] = static_cast<int>(qo);
  seg.k_off[P] = static_cast<int>(ko);
  seg.qt_off[P] = static_cast<int>(qt);
  seg.kt_off[P] = static_cast<int>(kt);
  size_t need = 0;
  lcr_attention_grad_ws_bytes(qo, heads, &need);
  if (qo > 0 && (!ws || ws_bytes < need)) return refuse_ws(LCR_ESPACE, "lcr_attention_seg_grad_f32", ws_bytes, need);
  const float scale = 1.f / sqrtf(static_cast<float>(head_dim));
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* Lq = static_cast<float*>(ws);
  float* Dq = Lq + static_cast<size_t>(heads) * static_cast<size_t>(qo);
  if (qt > 0) hipLaunchKernelGGL(k_ag_stats, dim3(static_cast<int>(qt), heads), dim3(64 * AT_SPLIT), 0, st, q, k, out, d_out, seg, heads, scale, Lq, Dq);
  hipLaunchKernelGGL(k_ag_dkdv, dim3(static_cast<int>(kt), heads), dim3(64 * AT_SPLIT), 0, st, q, k, v, d_out, Lq, Dq, seg, heads, scale, dk, dv);
  if (qt > 0) hipLaunchKernelGGL(k_ag_dq, dim3(static_cast<int>(qt), heads), dim3(64 * AT_SPLIT), 0, st, q, k, v, d_out, Lq, Dq, seg, heads, scale, dq);
  return check_launch("lcr_attention_seg_grad_f32");
}

extern "C" int lcr_rotary_embed_grad(const float* y, const float* dy, const float* theta, int64_t N, int heads, float* dx, float* dtheta, void* stream) {
  if (!y || !dy || !theta || !dx || !dtheta || N < 0 || heads < 1) return refuse(LCR_EARG, "lcr_rotary_embed_grad: bad argument");
  if (N == 0) return LCR_OK;
  const int64_t total = N * heads * 16;
  hipLaunchKernelGGL(k_rotary_grad, dim3(static_cast<int>(std::min<int64_t>((total + 255) / 256, 4096))), dim3(256), 0, static_cast<hipStream_t>(stream), y,
                     dy, theta, N, heads, dx, dtheta);
  return check_launch("lcr_rotary_embed_grad");
}

extern "C" int lcr_add_layernorm_grad_ws_bytes(int64_t N, int D, size_t* bytes) {
  if (!bytes || N < 0 || D < 1 || D > 1024) return refuse(LCR_EARG, "lcr_add_layernorm_grad_ws_bytes: bad argument (D <= 1024)");
  const size_t parts = static_cast<size_t>((N + LNG_ROWS - 1) / LNG_ROWS);
  *bytes = align_up(parts * 2 * static_cast<size_t>(D) * sizeof(float));
  return LCR_OK;
}

extern "C" int lcr_add_layernorm_grad(const float* a, const float* b, const float* gamma, const float* dy, int64_t N, int D, float eps, float* dx,
                                      float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
  if (!a || !gamma || !dy || !dx || !dgamma || !dbeta || N < 0 || D < 1 || D > 1024) return refuse(LCR_EARG, "lcr_add_layernorm_grad: bad argument (D <= 1024)");
  size_t need = 0;
  lcr_add_layernorm_grad_ws_bytes(N, D, &need);
  if (N > 0 && (!ws || ws_bytes < need)) return refuse_ws(LCR_ESPACE, "lcr_add_layernorm_grad", ws_bytes, need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t parts = (N + LNG_ROWS - 1) / LNG_ROWS;
  if (parts > 4 * static_cast<int64_t>(2147483647)) return refuse(LCR_EARG, "lcr_add_layernorm_grad: too many rows");
  if (N > 0)
    hipLaunchKernelGGL(k_ln_grad, dim3(static_cast<int>((parts + 3) / 4)), dim3(256), 0, st, a, b, gamma, dy, N, D, eps, dx, static_cast<float*>(ws));
  hipLaunchKernelGGL(k_ln_grad_reduce, dim3((2 * D + 3) / 4), dim3(256), 0, st, static_cast<const float*>(ws), parts, D, dgamma, dbeta);   // N == 0: zeros
  return check_launch("lcr_add_layernorm_grad");
}
