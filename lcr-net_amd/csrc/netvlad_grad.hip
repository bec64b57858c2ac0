// netvlad_grad.hip — row p: the reverse pass of the global-descriptor head in training mode (lcr_netvlad_backward), fp32.
//
// The forward it reverses is lcr_netvlad_train_forward (csrc/netvlad.hip, which also says how the reference's cyclic padding becomes the
// row multiplicities c = p + 1).  It reads what that forward saved (nv::Saved in netvlad.h); x^ (4 KB a row) is NOT among it: the rows are
// normalised again here, by the forward's own kernel.  Every sum has one order: wavefront / workgroup trees of fixed shape,
// cross-workgroup partials added in ascending order by one thread per column, batch statistics in fp64.  No floating-point atomics.
#include <algorithm>

#include "netvlad.h"

namespace lcr {
namespace {
using namespace nv;

// dx = dx^/d - [n >= eps] (dx^ . x^) x^ / n with x^ = x/d, d = max(n, 1e-12): F.normalize's backward, a zero row included (dx = dx^/1e-12)
__global__ __launch_bounds__(256) void k_row_unit_grad(const float* __restrict__ x, const float* __restrict__ g, int64_t N, float* __restrict__ dx) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * 4 + w; n < N; n += static_cast<int64_t>(gridDim.x) * 4) {
    float xv[F / 64], gv[F / 64];
    float ss = 0.f;
#pragma unroll
    for (int u = 0; u < F / 64; ++u) {
      xv[u] = x[n * F + lane + 64 * u];
      gv[u] = g[n * F + lane + 64 * u];
      ss = fmaf(xv[u], xv[u], ss);
    }
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss), d = fmaxf(nrm, 1e-12f);
    float dot = 0.f;
#pragma unroll
    for (int u = 0; u < F / 64; ++u) dot = fmaf(gv[u], xv[u] / d, dot);
    dot = wave_sum(dot);
    const float back = nrm >= 1e-12f ? dot / nrm : 0.f;
#pragma unroll
    for (int u = 0; u < F / 64; ++u) dx[n * F + lane + 64 * u] = gv[u] / d - back * (xv[u] / d);
  }
}

// ------------------------------------------------------------------------------------------------ bn1 column sums (fp64, fixed order)
// (sum g, sum g a^) of g[N,64] with a^ = (a - mu) r, partitioned as the forward's k_bn1_moments.   part[g][2][64]
__global__ __launch_bounds__(256) void k_bn1_grad_partial(const float* __restrict__ a, const float* __restrict__ g, const float* __restrict__ mu,
                                                           const float* __restrict__ r, int64_t N, double* __restrict__ part) {
  __shared__ double s_p[4][2][K];
  const int k = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t chunk = (N + gridDim.x - 1) / gridDim.x;
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * chunk, hi = std::min<int64_t>(lo + chunk, N);
  double t0 = 0.0, t1 = 0.0;
  const float m = mu[k], rr = r[k];
  for (int64_t n = lo + q; n < hi; n += 4) {
    const float av = a[n * K + k];
    const float gv = g[n * K + k];
    t0 += gv;
    t1 += static_cast<double>(gv) * ((av - m) * rr);
  }
  s_p[q][0][k] = t0;
  s_p[q][1][k] = t1;
  __syncthreads();
  if (q < 2) part[(static_cast<int64_t>(blockIdx.x) * 2 + q) * K + k] = (s_p[0][q][k] + s_p[1][q][k]) + (s_p[2][q][k] + s_p[3][q][k]);
}

// d gamma1 = sum g a^, d beta1 = sum g; sums[0][k] = gamma sum g, sums[1][k] = gamma sum g a^ (the two means of the bn1 backward, times S Lmax)
__global__ __launch_bounds__(K) void k_bn1_grad_sums(const double* __restrict__ part, int G, const float* __restrict__ gamma, float* __restrict__ dgamma,
                                                      float* __restrict__ dbeta, float* __restrict__ sums) {
  const int k = threadIdx.x;
  double t0 = 0.0, t1 = 0.0;
  for (int g = 0; g < G; ++g) {
    t0 += part[(g * 2 + 0) * K + k];
    t1 += part[(g * 2 + 1) * K + k];
  }
  if (dgamma) dgamma[k] = static_cast<float>(t1);
  if (dbeta) dbeta[k] = static_cast<float>(t0);
  sums[k] = static_cast<float>(t0 * gamma[k]);
  sums[K + k] = static_cast<float>(t1 * gamma[k]);
}

// ------------------------------------------------------------------------------------------------ the tail ([S,256]; thread = column)
// cloud blockIdx.x: through the last normalise, the product and the sigmoid: dhp1 = dt g, dpre = dt h' g (1 - g)
__global__ __launch_bounds__(D) void k_gate_out_grad(const float* __restrict__ d_out, const float* __restrict__ out, const float* __restrict__ tn,
                                                      const float* __restrict__ g, const float* __restrict__ hp, float* __restrict__ dhp1,
                                                      float* __restrict__ dpre) {
  __shared__ float s_red[4];
  const int s = blockIdx.x, j = threadIdx.x;
  const float dy = d_out[s * D + j], o = out[s * D + j];
  const float dot = block_sum<4>(dy * o, s_red);
  const float nrm = tn[s], d = fmaxf(nrm, 1e-12f);
  const float dt = dy / d - (nrm >= 1e-12f ? dot * o / nrm : 0.f);
  const float gv = g[s * D + j];
  dhp1[s * D + j] = dt * gv;
  dpre[s * D + j] = dt * hp[s * D + j] * gv * (1.f - gv);
}

// BatchNorm backward over the S descriptors: dy = dy1 (+ dy2) -> dgamma = sum dy xh, dbeta = sum dy, dx = gamma r (dy - mean(dy) - xh mean(dy xh))
__global__ __launch_bounds__(D) void k_bn_batch_grad(const float* __restrict__ dy1, const float* __restrict__ dy2, const float* __restrict__ xh, int S,
                                                      const float* __restrict__ gamma, const float* __restrict__ r, float* __restrict__ dgamma,
                                                      float* __restrict__ dbeta, float* __restrict__ dx) {
  const int j = threadIdx.x;
  double t0 = 0.0, t1 = 0.0;
  for (int s = 0; s < S; ++s) {
    const float dy = dy1[s * D + j] + (dy2 ? dy2[s * D + j] : 0.f);
    t0 += dy;
    t1 += static_cast<double>(dy) * xh[s * D + j];
  }
  if (dgamma) dgamma[j] = static_cast<float>(t1);
  if (dbeta) dbeta[j] = static_cast<float>(t0);
  const float m0 = static_cast<float>(t0 / S), m1 = static_cast<float>(t1 / S), f = gamma[j] * r[j];
  for (int s = 0; s < S; ++s) {
    const float dy = dy1[s * D + j] + (dy2 ? dy2[s * D + j] : 0.f);
    dx[s * D + j] = f * ((dy - m0) - xh[s * D + j] * m1);
  }
}

// ------------------------------------------------------------------------------------------------ the hidden projection, reverse
// One sweep over the rows of H: dv[s][i] = sum_j dh[s][j] H[i][j] and dH[i][j] = sum_s v[s][i] dh[s][j] (s ascending).  dh[S,256] sits in LDS;
// one wavefront covers a row with one float4 per lane and keeps RB rows in flight, so every LDS read of dh serves RB rows.  The RB
// per-lane dot products of a cloud are summed across the lanes by one transposing tree (lane l ends with the sum of row l & 3).
constexpr int SW_THREADS = 512, SW_ROWS = 256, RB = 4;

__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }

template <bool WANT_DH>
__global__ __launch_bounds__(SW_THREADS) void k_hidden_sweep(const float* __restrict__ H, const float* __restrict__ V, const float* __restrict__ dh, int S,
                                                              float* __restrict__ dV, float* __restrict__ dH) {
  extern __shared__ float4 s_dh[];   // [S][64]
  for (int t = threadIdx.x; t < S * 64; t += SW_THREADS) s_dh[t] = reinterpret_cast<const float4*>(dh)[t];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr int PER_WAVE = SW_ROWS / (SW_THREADS / 64);
  const int row0 = blockIdx.x * SW_ROWS + w * PER_WAVE;
  const bool b0 = lane & 1, b1 = lane & 2;
  const float4* H4 = reinterpret_cast<const float4*>(H);
  float4 h[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) h[r] = H4[static_cast<int64_t>(row0 + r) * 64 + lane];
  for (int it = 0; it < PER_WAVE / RB; ++it) {
    const int i0 = row0 + it * RB;
    float4 hn[RB];                                   // the next four rows, requested before this trip's arithmetic
    const int inext = it + 1 < PER_WAVE / RB ? i0 + RB : i0;
#pragma unroll
    for (int r = 0; r < RB; ++r) hn[r] = H4[static_cast<int64_t>(inext + r) * 64 + lane];
    float4 acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s) {
      const float4 d = s_dh[s * 64 + lane];
      const float4 vv = *reinterpret_cast<const float4*>(V + static_cast<int64_t>(s) * FK + i0);
      const float p0 = dot4(h[0], d), p1 = dot4(h[1], d), p2 = dot4(h[2], d), p3 = dot4(h[3], d);
      if (WANT_DH) {
        const float vr[RB] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          acc[r].x = fmaf(vr[r], d.x, acc[r].x);
          acc[r].y = fmaf(vr[r], d.y, acc[r].y);
          acc[r].z = fmaf(vr[r], d.z, acc[r].z);
          acc[r].w = fmaf(vr[r], d.w, acc[r].w);
        }
      }
      float a0 = (b0 ? p1 : p0) + __shfl_xor(b0 ? p0 : p1, 1);   // pair sums: row 0 on even lanes, row 1 on odd ones
      float a1 = (b0 ? p3 : p2) + __shfl_xor(b0 ? p2 : p3, 1);   // rows 2 / 3
      float c = (b1 ? a1 : a0) + __shfl_xor(b1 ? a0 : a1, 2);    // quad sums of row (lane & 3)
      c += __shfl_xor(c, 4);
      c += __shfl_xor(c, 8);
      c += __shfl_xor(c, 16);
      c += __shfl_xor(c, 32);
      if (lane < RB) dV[static_cast<int64_t>(s) * FK + i0 + lane] = c;
    }
    if (WANT_DH) {
#pragma unroll
      for (int r = 0; r < RB; ++r) reinterpret_cast<float4*>(dH)[static_cast<int64_t>(i0 + r) * 64 + lane] = acc[r];
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) h[r] = hn[r];
  }
}

// ------------------------------------------------------------------------------------------------ both normalisations of V, reverse
// cloud blockIdx.x, in place on g = dv -> dV0:
//   dV1 = dv/n2 - [n2raw >= eps] (dv . v) v / n2raw;  per column: dV0 = dV1/n1 - [n1raw >= eps] (dV1 . V1) V1 / n1raw with V1 = v n2
// and dasum[k] = -sum_c dV0[c][k] W2[c][k]
__global__ __launch_bounds__(1024) void k_vlad_finalize_grad(float* __restrict__ G, const float* __restrict__ V, const float* __restrict__ n1raw,
                                                              const float* __restrict__ n2raw, const float* __restrict__ W2, float* __restrict__ dasum) {
  __shared__ float s_red[16];
  __shared__ float s_col[16][K];
  __shared__ float s_dot[K];
  float* g = G + static_cast<int64_t>(blockIdx.x) * FK;
  const float* v = V + static_cast<int64_t>(blockIdx.x) * FK;
  const int k = threadIdx.x & 63, q = threadIdx.x >> 6;
  float t = 0.f;
  for (int c = q; c < F; c += 16) t = fmaf(g[c * K + k], v[c * K + k], t);
  const float dot2 = block_sum<16>(t, s_red);
  const float r2 = n2raw[blockIdx.x], n2 = fmaxf(r2, 1e-6f);
  const float back2 = r2 >= 1e-6f ? dot2 / r2 : 0.f;
  float dd = 0.f;
  for (int c = q; c < F; c += 16) {
    const float vv = v[c * K + k];
    const float d1 = g[c * K + k] / n2 - back2 * vv;
    g[c * K + k] = d1;
    dd = fmaf(d1, vv * n2, dd);
  }
  s_col[q][k] = dd;
  __syncthreads();
  if (q == 0) {
    float u = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) u += s_col[i][k];
    s_dot[k] = u;
  }
  __syncthreads();
  const float r1 = n1raw[blockIdx.x * K + k], n1 = fmaxf(r1, 1e-6f);
  const float back1 = r1 >= 1e-6f ? s_dot[k] / r1 : 0.f;
  float da = 0.f;
  for (int c = q; c < F; c += 16) {
    const float d0 = g[c * K + k] / n1 - back1 * (v[c * K + k] * n2);
    g[c * K + k] = d0;
    da = fmaf(d0, W2[c * K + k], da);
  }
  __syncthreads();
  s_col[q][k] = da;
  __syncthreads();
  if (q == 0) {
    float u = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) u += s_col[i][k];
    dasum[blockIdx.x * K + k] = -u;
  }
}

// dW2[c][k] = -sum_s asum[s][k] dV0[s][c][k], s ascending
__global__ __launch_bounds__(256) void k_w2_grad(const float* __restrict__ dV0, const float* __restrict__ asum, int S, float* __restrict__ dW2) {
  const int e = blockIdx.x * 256 + threadIdx.x, k = e & 63;
  float t = 0.f;
  for (int s = 0; s < S; ++s) t = fmaf(asum[s * K + k], dV0[static_cast<int64_t>(s) * FK + e], t);
  dW2[e] = -t;
}

// dw[n][k] = sum_d x^[n][d] dV0[cloud of n][d][k], d ascending: every cloud has its own B, so this is S ragged products of [n_s,1024] x [1024,64].
// One workgroup per 64 rows of one cloud (blockIdx.y = cloud; tiles beyond its rows leave), 4 x 4 outputs per thread, x^ and dV0 staged through
// LDS 32 feature columns at a time.  As S separate lcr_gemm_f32 calls each product filled 13 of the 256 CUs and the calls ran one after another.
__global__ __launch_bounds__(256) void k_assign_grad(const float* __restrict__ xn, const float* __restrict__ dV0, Seg seg, float* __restrict__ dw) {
  constexpr int TM = 64, KC = 32;
  __shared__ float s_a[TM][KC + 1];
  __shared__ float4 s_b[KC][K / 4];
  const int s = blockIdx.y;
  const int64_t row0 = seg.off[s] + static_cast<int64_t>(blockIdx.x) * TM;
  const int rows = static_cast<int>(std::min<int64_t>(TM, seg.off[s + 1] - row0));
  if (rows <= 0) return;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const float* b = dV0 + static_cast<int64_t>(s) * FK;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int d0 = 0; d0 < F; d0 += KC) {
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = (threadIdx.x >> 3) + 32 * h, c = (threadIdx.x & 7) * 4;
      const float4 v = r < rows ? *reinterpret_cast<const float4*>(xn + (row0 + r) * F + d0 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      s_a[r][c] = v.x;
      s_a[r][c + 1] = v.y;
      s_a[r][c + 2] = v.z;
      s_a[r][c + 3] = v.w;
      const int d = (threadIdx.x >> 4) + 16 * h;
      s_b[d][tx] = *reinterpret_cast<const float4*>(b + static_cast<int64_t>(d0 + d) * K + tx * 4);
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < KC; ++kk) {
      const float4 bv = s_b[kk][tx];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a = s_a[ty * 4 + i][kk];
        acc[i][0] = fmaf(a, bv.x, acc[i][0]);
        acc[i][1] = fmaf(a, bv.y, acc[i][1]);
        acc[i][2] = fmaf(a, bv.z, acc[i][2]);
        acc[i][3] = fmaf(a, bv.w, acc[i][3]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (ty * 4 + i < rows)
      *reinterpret_cast<float4*>(dw + (row0 + ty * 4 + i) * K + tx * 4) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
}

// dx^[n][d] = sum_k w[n][k] dV0[cloud of n][d][k] + sum_k da[n][k] Wc[d][k] (k ascending, the first sum first): both terms of the unit rows'
// gradient in one ragged launch — workgroup = 64 rows of one cloud (blockIdx.y) x 64 feature columns (blockIdx.z), 4 x 4 outputs per thread,
// the two K = 64 halves staged through the same LDS one after the other (B transposed on the way in: both B operands are stored [d][k]).
__global__ __launch_bounds__(256) void k_unit_grad(const float* __restrict__ wgt, const float* __restrict__ da, const float* __restrict__ dV0,
                                                    const float* __restrict__ Wc, Seg seg, float* __restrict__ dxn) {
  constexpr int TM = 64, TN = 64;
  __shared__ float s_a[TM][K + 1];
  __shared__ float s_b[K][TN + 1];
  const int s = blockIdx.y;
  const int64_t row0 = seg.off[s] + static_cast<int64_t>(blockIdx.x) * TM;
  const int rows = static_cast<int>(std::min<int64_t>(TM, seg.off[s + 1] - row0));
  if (rows <= 0) return;
  const int d0 = blockIdx.z * TN;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int half = 0; half < 2; ++half) {
    const float* A = half ? da : wgt;
    const float* B = (half ? Wc : dV0 + static_cast<int64_t>(s) * FK) + static_cast<int64_t>(d0) * K;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int idx = threadIdx.x + 256 * h, r = idx >> 4, c = (idx & 15) * 4;
      const float4 v = r < rows ? *reinterpret_cast<const float4*>(A + (row0 + r) * K + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      s_a[r][c] = v.x;
      s_a[r][c + 1] = v.y;
      s_a[r][c + 2] = v.z;
      s_a[r][c + 3] = v.w;
      const float4 u = *reinterpret_cast<const float4*>(B + r * K + c);      // r: feature column d0 + r here
      s_b[c][r] = u.x;
      s_b[c + 1][r] = u.y;
      s_b[c + 2][r] = u.z;
      s_b[c + 3][r] = u.w;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < K; ++kk) {
      float bv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = s_b[kk][tx * 4 + j];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a = s_a[ty * 4 + i][kk];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a, bv[j], acc[i][j]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (ty * 4 + i < rows)
      *reinterpret_cast<float4*>(dxn + (row0 + ty * 4 + i) * F + d0 + tx * 4) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
}

// real rows only (padding copies are constants): dw += dasum of the row's cloud; g = sm (dw - sum_k sm dw), in place; w = sm + p/64 again
__global__ __launch_bounds__(256) void k_softmax_grad(float* __restrict__ dw, const float* __restrict__ sm, const float* __restrict__ dasum,
                                                       const int32_t* __restrict__ rseg, const int32_t* __restrict__ cmul, int64_t N,
                                                       float* __restrict__ wgt) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * 4 + w; n < N; n += static_cast<int64_t>(gridDim.x) * 4) {
    const float p = sm[n * K + lane];
    const float d = dw[n * K + lane] + dasum[rseg[n] * K + lane];
    const float dot = wave_sum(p * d);
    dw[n * K + lane] = p * (d - dot);
    wgt[n * K + lane] = p + static_cast<float>(cmul[n] - 1) * (1.f / 64.f);
  }
}

// da = r (gamma g - c/(S Lmax) (s1 + a^ s2)), in place on g
__global__ __launch_bounds__(256) void k_bn1_grad(float* __restrict__ g, const float* __restrict__ a, const int32_t* __restrict__ cmul,
                                                   const float* __restrict__ mu, const float* __restrict__ r, const float* __restrict__ gamma,
                                                   const float* __restrict__ sums, float inv_count, int64_t total) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= total) return;
  const int k = static_cast<int>(e & 63);
  const int64_t n = e >> 6;
  const float ah = (a[e] - mu[k]) * r[k];
  const float c = static_cast<float>(cmul[n]) * inv_count;
  g[e] = r[k] * (gamma[k] * g[e] - c * (sums[k] + ah * sums[K + k]));
}

// out[e] = sum_z part[z][e], z ascending
__global__ __launch_bounds__(256) void k_sum_chunks(const float* __restrict__ part, int count, float* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  float t = part[e];
  for (int z = 1; z < count; ++z) t += part[static_cast<int64_t>(z) * FK + e];
  out[e] = t;
}

}  // namespace
}  // namespace lcr

using namespace lcr;
using namespace lcr::nv;

namespace {

int chunk_count(int64_t n_rows) { return static_cast<int>(std::min<int64_t>(64, std::max<int64_t>(1, (n_rows + 255) / 256))); }

struct BwdWs {
  float *xn, *dxn, *dw, *w, *dv, *dasum, *dhp1, *dpre, *dg0, *dhp2, *dh, *sums, *wc_part;
  double* part;
  size_t bytes;
};
BwdWs bwd_layout(void* p, int64_t n_rows, int S) {
  BwdWs L;
  Carver c(p, ~size_t(0));
  const size_t rows = static_cast<size_t>(std::max<int64_t>(n_rows, 1)), s = static_cast<size_t>(S);
  L.xn = c.take<float>(rows * F);       // x^ again
  L.dxn = c.take<float>(rows * F);      // w.dV0^T + da.Wc^T
  L.dw = c.take<float>(rows * K);
  L.w = c.take<float>(rows * K);
  L.dv = c.take<float>(s * FK);
  L.dasum = c.take<float>(s * K);
  L.dhp1 = c.take<float>(s * D);
  L.dpre = c.take<float>(s * D);
  L.dg0 = c.take<float>(s * D);
  L.dhp2 = c.take<float>(s * D);
  L.dh = c.take<float>(s * D);
  L.sums = c.take<float>(2 * K);
  L.wc_part = c.take<float>(static_cast<size_t>(chunk_count(n_rows)) * FK);
  L.part = c.take<double>(static_cast<size_t>(STAT_G) * 2 * K);
  L.bytes = c.off;
  return L;
}

}  // namespace

extern "C" int lcr_netvlad_backward_ws_bytes(int64_t n_rows, int S, size_t* bytes) {
  if (!bytes || n_rows < 0 || S < 1) return refuse(LCR_EARG, "lcr_netvlad_backward_ws_bytes: null pointer or outside the domain (n_rows >= 0, S >= 1): n_rows=%lld S=%d", static_cast<long long>(n_rows), S);
  *bytes = bwd_layout(nullptr, n_rows, S).bytes;
  return LCR_OK;
}

extern "C" int lcr_netvlad_backward(const float* d_out, const float* feats, const int64_t* seg_len_host, int S, const LcrNetvladWeights* wt,
                                    const void* saved, size_t saved_bytes, float* d_feats, const LcrNetvladGrads* grads, void* ws, size_t ws_bytes,
                                    void* stream) {
  const char* who = "lcr_netvlad_backward";
  if (!d_out || !feats || !wt || !saved || !grads || !ws) return refuse(LCR_EARG, "%s: bad argument", who);
  std::vector<int64_t> off;
  int Lmax = 0;
  int rc = seg_offsets(who, seg_len_host, S, 2, S_MAX, &off, &Lmax);   // the training forward's domain
  if (rc) return rc;
  const Seg seg = seg_window(off, 0, S, Lmax);
  const int64_t N = off[S];
  const Saved sv = saved_layout(const_cast<void*>(saved), N, S);
  const BwdWs L = bwd_layout(ws, N, S);
  if (sv.bytes > saved_bytes || L.bytes > ws_bytes)
    return refuse(LCR_ESPACE, "%s: buffer too small (saved %zu < %zu or workspace %zu < %zu)", who, saved_bytes, sv.bytes, ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  const LcrNetvladGrads& g = *grads;
  // the tail: last normalise, gate, context_gating.bn1, gating product, bn2
  hipLaunchKernelGGL(k_gate_out_grad, dim3(S), dim3(D), 0, st, d_out, sv.out, sv.tn, sv.g, sv.hp, L.dhp1, L.dpre);
  hipLaunchKernelGGL(k_bn_batch_grad, dim3(1), dim3(D), 0, st, L.dpre, static_cast<const float*>(nullptr), sv.gh, S, wt->gbn_w, sv.rg, g.gbn_w, g.gbn_b, L.dg0);
  if (g.gating_weights) {
    rc = lcr_gemm_f32(sv.hp, L.dg0, g.gating_weights, D, D, S, 1, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, stream);
    if (rc) return rc;
  }
  rc = lcr_gemm_f32(L.dg0, wt->gating_weights, L.dhp2, S, D, D, 0, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_bn_batch_grad, dim3(1), dim3(D), 0, st, L.dhp1, L.dhp2, sv.hh, S, wt->bn2_w, sv.r2, g.bn2_w, g.bn2_b, L.dh);
  // the sweep over H
  const bool upstream = d_feats || g.cluster_weights || g.cluster_weights2 || g.bn1_w || g.bn1_b;
  if (upstream || g.hidden1_weights) {
    const size_t lds = static_cast<size_t>(S) * D * sizeof(float);
    static DynLds opt_in_dh, opt_in_dv;
    const void* fn = g.hidden1_weights ? reinterpret_cast<const void*>(&k_hidden_sweep<true>) : reinterpret_cast<const void*>(&k_hidden_sweep<false>);
    if ((g.hidden1_weights ? opt_in_dh : opt_in_dv).need(fn, lds) != hipSuccess)
      return refuse(LCR_EHIP, "%s: cannot reserve %zu B of dynamic LDS for the sweep over hidden1_weights", who, lds);
    if (g.hidden1_weights)
      hipLaunchKernelGGL((k_hidden_sweep<true>), dim3(FK / SW_ROWS), dim3(SW_THREADS), lds, st, wt->hidden1_weights, sv.v, L.dh, S, L.dv, g.hidden1_weights);
    else
      hipLaunchKernelGGL((k_hidden_sweep<false>), dim3(FK / SW_ROWS), dim3(SW_THREADS), lds, st, wt->hidden1_weights, sv.v, L.dh, S, L.dv,
                         static_cast<float*>(nullptr));
  }
  if (!upstream) return check_launch(who);
  hipLaunchKernelGGL(k_vlad_finalize_grad, dim3(S), dim3(1024), 0, st, L.dv, sv.v, sv.n1raw, sv.n2raw, wt->cluster_weights2, L.dasum);
  if (g.cluster_weights2) hipLaunchKernelGGL(k_w2_grad, dim3(FK / 256), dim3(256), 0, st, L.dv, sv.asum, S, g.cluster_weights2);
  if (!(d_feats || g.cluster_weights || g.bn1_w || g.bn1_b)) return check_launch(who);
  // dw = x^ . dV0 per cloud, softmax and bn1 on the real rows
  const int nblk = row_blocks(N);
  launch_row_l2norm(feats, N, L.xn, st);
  hipLaunchKernelGGL(k_assign_grad, dim3(div_up(seg.Lmax, 64), S), dim3(256), 0, st, L.xn, L.dv, seg, L.dw);
  hipLaunchKernelGGL(k_softmax_grad, dim3(nblk), dim3(256), 0, st, L.dw, sv.sm, L.dasum, sv.rseg, sv.cmul, N, L.w);
  const int G = stat_blocks(N);
  hipLaunchKernelGGL(k_bn1_grad_partial, dim3(G), dim3(256), 0, st, sv.a, L.dw, sv.mu1, sv.r1, N, L.part);
  hipLaunchKernelGGL(k_bn1_grad_sums, dim3(1), dim3(K), 0, st, L.part, G, wt->bn1_w, g.bn1_w, g.bn1_b, L.sums);
  if (!(d_feats || g.cluster_weights)) return check_launch(who);
  hipLaunchKernelGGL(k_bn1_grad, dim3(div_up(N * K, 256)), dim3(256), 0, st, L.dw, sv.a, sv.cmul, sv.mu1, sv.r1, wt->bn1_w, L.sums,
                     static_cast<float>(1.0 / (static_cast<double>(S) * seg.Lmax)), N * K);
  if (g.cluster_weights) {
    // dWc = x^T . da over equal row chunks of at most 256 rows (at most 64 chunks), added in chunk order
    const int count = chunk_count(N);
    const int64_t per = (N + count - 1) / count;
    int kk[64], used = 0;
    int64_t ao[64], bo[64], co[64];
    for (int z = 0; z < count && z * per < N; ++z, ++used) {
      kk[z] = static_cast<int>(std::min<int64_t>(per, N - z * per));
      ao[z] = z * per * F;
      bo[z] = z * per * K;
      co[z] = static_cast<int64_t>(z) * FK;
    }
    rc = lcr_gemm_f32_batched_ta(L.xn, L.dw, L.wc_part, F, K, used, kk, ao, bo, co, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sum_chunks, dim3(FK / 256), dim3(256), 0, st, L.wc_part, used, g.cluster_weights);
  }
  if (d_feats) {
    hipLaunchKernelGGL(k_unit_grad, dim3(div_up(seg.Lmax, 64), S, F / 64), dim3(256), 0, st, L.w, L.dw, L.dv, wt->cluster_weights, seg, L.dxn);
    hipLaunchKernelGGL(k_row_unit_grad, dim3(nblk), dim3(256), 0, st, feats, L.dxn, N, d_feats);
  }
  return check_launch(who);
}
