// kpconv_grad.hip — reverse passes of the encoder's gather kernels (kpconv.hip): the inverted neighbour list, the KPConv aggregate's
// gradient to the support features and to the points, the C_in = 1 KPConv's gradient to weights and bias, the max-pool's gradient.
//
// All sums per support row are GATHERS over the inverted list: the support row n owns the flat positions e = m*H + h of the forward list with
// idx[m,h] == n, in ascending order (lcr_neighbor_transpose: a stable radix sort of (support index, flat position)), and one wavefront
// sums what its edges send, in list order.  No floating-point atomics: a row's sum has one order, results repeat to the bit, and a
// cloud's rows get the same bytes alone and inside a stack (its edges keep their relative order).
//
// The influence w(m,h,k) = max(0, 1 - |s_n - q_m - kp_k| / sigma) is kpconv.h's kp_influence / kp_edge, the functions the forward's
// k_kpconv_aggregate_vec, k_kpconv_fused32 and k_kpconv_cin1 call; the rows are walked in the forward's xcd_band.
#include <algorithm>

#include "kpconv.h"
#include "radix_sort.h"

namespace lcr {

// ---- inverted neighbour list ---------------------------------------------------------------------------------------------------
template <typename IdxT>
__global__ __launch_bounds__(256) void k_nt_keys(const IdxT* __restrict__ idx, int64_t E, int64_t Ns, int passes, RadixCtl* __restrict__ ctl,
                                                 uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctl->n = E;
    ctl->num_passes = passes;
  }
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < E; i += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t j = static_cast<int64_t>(idx[i]);
    keys[i] = (j >= 0 && j < Ns) ? static_cast<uint64_t>(j) : static_cast<uint64_t>(Ns);     // padding sorts behind every support
    vals[i] = static_cast<uint32_t>(i);
  }
}

// row_start[n] = the first sorted position whose key is >= n (n = Ns: the number of real entries); edges = the values of the real entries
__global__ __launch_bounds__(256) void k_nt_rows(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t E, int64_t Ns,
                                                 int32_t* __restrict__ row_start, uint32_t* __restrict__ edges) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; n <= Ns; n += stride) {
    int64_t lo = 0, hi = E;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < static_cast<uint64_t>(n)) lo = mid + 1;
      else hi = mid;
    }
    row_start[n] = static_cast<int32_t>(lo);
  }
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < E; i += stride)
    if (keys[i] < static_cast<uint64_t>(Ns)) edges[i] = vals[i];
}

struct NtLayout {
  RadixCtl* ctl;
  uint64_t *kA, *kB;
  uint32_t *vA, *vB;
  int32_t* hist;
  char* scan;
  size_t bytes;
};
static NtLayout nt_layout(void* ws, int64_t E) {
  Carver c(ws, ~size_t(0));
  NtLayout L;
  const size_t n = static_cast<size_t>(std::max<int64_t>(E, 1));
  L.ctl = c.take<RadixCtl>(1);
  L.kA = c.take<uint64_t>(n);
  L.kB = c.take<uint64_t>(n);
  L.vA = c.take<uint32_t>(n);
  L.vB = c.take<uint32_t>(n);
  L.hist = c.take<int32_t>(radix_hist_elems(static_cast<int64_t>(n)));
  L.scan = c.take<char>(scan_ws_bytes(static_cast<int64_t>(radix_hist_elems(static_cast<int64_t>(n)))));
  L.bytes = c.off;
  return L;
}

// ---- d_s_feats of the aggregate -------------------------------------------------------------------------------------------------
// One wavefront per support row, V = C / 64 channels per lane (C = 32: two half-wavefronts take alternate non-zero terms and are added
// once, lower half first).  Per trip the 64 lanes evaluate the influences of 4 edges x 16 kernel-point slots, as the forward does;
// a ballot names the non-zero ones and only their dA blocks are read: up to 4 G block loads are issued before the first is used.  The
// next trip's edge numbers and query points are fetched before this trip's blocks.
template <int C>
__global__ __launch_bounds__(KP_WAVES * 64) void k_kpconv_aggregate_grad(const float* __restrict__ dA, const float* __restrict__ q_pts,
                                                                         const float* __restrict__ s_pts, const int32_t* __restrict__ row_start,
                                                                         const uint32_t* __restrict__ edges, int64_t M, int64_t Ns, int H,
                                                                         KPoints kp, float sigma, float* __restrict__ out) {
  constexpr int V = C >= 64 ? C / 64 : 1;
  constexpr int G = C >= 64 ? 1 : 2;           // terms taken side by side
  constexpr int U = 4;                          // block loads in flight per lane
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane >> 4, col = lane & 15;
  const int grp = G == 1 ? 0 : lane >> 5;
  const int ch = G == 1 ? lane * V : (lane & 31);
  const float inv_sigma = 1.f / sigma;
  LCR_KP_SELECT(kp, col, kx, ky, kz);
  const uint32_t MH = static_cast<uint32_t>(M * H);        // host-checked: M * H < 2^30
  const XcdBand band = xcd_band(Ns, w, KP_WAVES);
  for (int64_t n = band.begin; n < band.end; n += band.stride) {
    int b = row_start[n], e = row_start[n + 1];
    b = max(0, min(b, static_cast<int>(MH)));
    e = max(b, min(e, static_cast<int>(MH)));
    const float sx = s_pts[3 * n], sy = s_pts[3 * n + 1], sz = s_pts[3 * n + 2];
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
    struct Hdr {
      int   m;
      bool  ok;
      float qx, qy, qz;
    };
    auto header = [&](int p, Hdr& h) {
      const int pe = p + sub;
      h.ok = pe < e;
      const uint32_t ed = h.ok ? edges[pe] : 0u;
      h.ok = h.ok && ed < MH;                              // a list entry outside the forward list is skipped, never dereferenced
      h.m = h.ok ? static_cast<int>(ed / static_cast<uint32_t>(H)) : 0;
      h.qx = q_pts[3 * static_cast<int64_t>(h.m)];
      h.qy = q_pts[3 * static_cast<int64_t>(h.m) + 1];
      h.qz = q_pts[3 * static_cast<int64_t>(h.m) + 2];
    };
    Hdr cur{0, false, 0.f, 0.f, 0.f}, nxt = cur;
    if (b < e) header(b, cur);
    for (int p = b; p < e; p += 4) {
      if (p + 4 < e) header(p + 4, nxt);
      float wv = kp_influence(sx - cur.qx, sy - cur.qy, sz - cur.qz, kx, ky, kz, inv_sigma);
      if (!cur.ok || col == 15) wv = 0.f;
      uint64_t mask = wave_ballot(wv > 0.f);
      while (mask) {                                       // wave-uniform
        float wu[U];
        float val[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int bit[2];
#pragma unroll
          for (int g = 0; g < G; ++g) {
            bit[g] = mask ? __builtin_ctzll(mask) : -1;
            if (mask) mask &= mask - 1;
          }
          const int mine = G == 1 ? bit[0] : (grp ? bit[1] : bit[0]);
          const int src = mine < 0 ? 0 : mine;
          float ww;
          int mm;
          if (G == 1) {
            ww = rdlane(wv, src);
            mm = rdlane(cur.m, src);
          } else {
            ww = __shfl(wv, src);
            mm = __shfl(cur.m, src);
          }
          wu[u] = mine < 0 ? 0.f : ww;
          const float* row = dA + (static_cast<int64_t>(mm) * KP_K + (src & 15)) * C + ch;
          if (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(row);
            val[u][0] = t.x, val[u][1 % V] = t.y, val[u][2 % V] = t.z, val[u][3 % V] = t.w;
          } else if (V == 2) {
            const float2 t = *reinterpret_cast<const float2*>(row);
            val[u][0] = t.x, val[u][1 % V] = t.y;
          } else {
            val[u][0] = *row;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (wu[u] > 0.f) {                               // an empty slot adds nothing (not even 0 * Inf)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = fmaf(wu[u], val[u][v], acc[v]);
          }
      }
      cur = nxt;
    }
    if (G == 2) {
      const float other = __shfl(acc[0], (lane & 31) + 32);
      if (lane < 32) out[n * C + ch] = acc[0] + other;
    } else if (V == 4) {
      *reinterpret_cast<float4*>(out + n * C + ch) = make_float4(acc[0], acc[1 % V], acc[2 % V], acc[3 % V]);
    } else if (V == 2) {
      *reinterpret_cast<float2*>(out + n * C + ch) = make_float2(acc[0], acc[1 % V]);
    } else {
      out[n * C + ch] = acc[0];
    }
  }
}

// ---- gradient of the aggregate to the points ----------------------------------------------------------------------------------------
// A[m][k*C + c] = sum_h w(m,h,k) f[idx[m,h]][c] with w = max(0, 1 - r / sigma), r = |e|, e = s_n - q_m - kp_k.  Where 0 < r < sigma,
// dw/dq = e / (sigma r) = -dw/ds, so with t(m,h,k) = sum_c dA[m][k*C + c] f[n][c] the edge (m,h) sends v(m,h) = sum_k t e / (sigma r) to q_m
// and -v to s_n.  r == 0 is defined as no term (the self edge of a cloud convolved with itself: e does not move with the point).
//
// "Store each contribution once, then sum per destination through an inverted index": k_kpconv_points_grad, one wavefront per query row,
// keeps dA[m] in registers (15 V values per lane, V = C / 64 channels), walks the row's columns in order, and per real neighbour reads the
// feature row once (V consecutive channels per lane: 16 bytes at C = 256).  Lane k < 15 evaluates kernel point k with the forward's
// arithmetic; a ballot names the live kernel points and only those are contracted.  A lane folds its partial dots into three sums with
// the (wave-uniform) coefficients e / (sigma r) before the wavefront is reduced: three reductions per edge, not one per kernel point.
// v goes to the [M,H,3] workspace, d_q[m] is the sum of the row's v in column order.  k_kpconv_points_grad_s, one wavefront per support
// row, then sums -v over the row's inverted list: lane l takes the list positions l, l + 64, ... in order and the lanes are folded once.
// C = 32: the upper half of the wavefront holds zeros.
template <int C, typename IdxT>
__global__ __launch_bounds__(KP_WAVES * 64) void k_kpconv_points_grad(const float* __restrict__ dA, const float* __restrict__ s_feats,
                                                                      const float* __restrict__ q_pts, const float* __restrict__ s_pts,
                                                                      const IdxT* __restrict__ idx, int64_t M, int64_t Ns, int H, KPoints kp,
                                                                      float sigma, float* __restrict__ v_ws, float* __restrict__ d_q) {
  constexpr int V = C >= 64 ? C / 64 : 1;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15;
  const bool has = C >= 64 || lane < 32;
  const int ch = C >= 64 ? lane * V : (lane & 31);
  const float inv_sigma = 1.f / sigma;
  LCR_KP_SELECT(kp, col, kx, ky, kz);
  auto load_row = [&](const float* row, float (&dst)[V]) {
    if (V == 4) {
      const float4 t = *reinterpret_cast<const float4*>(row);
      dst[0] = t.x, dst[1 % V] = t.y, dst[2 % V] = t.z, dst[3 % V] = t.w;
    } else if (V == 2) {
      const float2 t = *reinterpret_cast<const float2*>(row);
      dst[0] = t.x, dst[1 % V] = t.y;
    } else {
      dst[0] = *row;
    }
  };
  const XcdBand band = xcd_band(M, w, KP_WAVES);
  for (int64_t m = band.begin; m < band.end; m += band.stride) {
    float g[KP_K][V];
#pragma unroll
    for (int k = 0; k < KP_K; ++k) {
#pragma unroll
      for (int v = 0; v < V; ++v) g[k][v] = 0.f;
      if (has) load_row(dA + (m * KP_K + k) * C + ch, g[k]);
    }
    int jrow[2];                                           // the row's indices, column lane + 64 i; -1 = padding
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int h = lane + 64 * i;
      const int64_t j = h < H ? static_cast<int64_t>(idx[m * H + h]) : -1;
      jrow[i] = (j >= 0 && j < Ns) ? static_cast<int>(j) : -1;
    }
    const float qx = q_pts[3 * m], qy = q_pts[3 * m + 1], qz = q_pts[3 * m + 2];
    float tx = 0.f, ty = 0.f, tz = 0.f;
    for (int h = 0; h < H; ++h) {
      const int j = h < 64 ? rdlane(jrow[0], h) : rdlane(jrow[1], h - 64);      // wave-uniform
      float vx = 0.f, vy = 0.f, vz = 0.f;
      if (j >= 0) {
        const int64_t n = j;
        float ex, ey, ez, r, wv;
        kp_edge(s_pts[3 * n] - qx, s_pts[3 * n + 1] - qy, s_pts[3 * n + 2] - qz, kx, ky, kz, inv_sigma, ex, ey, ez, r, wv);
        const uint64_t mask = wave_ballot(lane < KP_K && wv > 0.f && r > 0.f);
        if (mask) {                                        // wave-uniform
          const float cs = 1.f / (sigma * r);              // lanes outside the mask are never read
          const float cx = ex * cs, cy = ey * cs, cz = ez * cs;
          float f[V];
#pragma unroll
          for (int v = 0; v < V; ++v) f[v] = 0.f;
          if (has) load_row(s_feats + n * C + ch, f);
          float px = 0.f, py = 0.f, pz = 0.f;
#pragma unroll
          for (int k = 0; k < KP_K; ++k)
            if ((mask >> k) & 1) {
              float p = 0.f;
#pragma unroll
              for (int v = 0; v < V; ++v) p = fmaf(g[k][v], f[v], p);
              px = fmaf(p, rdlane(cx, k), px);
              py = fmaf(p, rdlane(cy, k), py);
              pz = fmaf(p, rdlane(cz, k), pz);
            }
          vx = wave_sum(px);
          vy = wave_sum(py);
          vz = wave_sum(pz);
        }
      }
      if (v_ws && lane < 3) v_ws[(m * H + h) * 3 + lane] = lane == 0 ? vx : (lane == 1 ? vy : vz);
      tx += vx;
      ty += vy;
      tz += vz;
    }
    if (d_q && lane < 3) d_q[3 * m + lane] = lane == 0 ? tx : (lane == 1 ? ty : tz);
  }
}

__global__ __launch_bounds__(KP_WAVES * 64) void k_kpconv_points_grad_s(const float* __restrict__ v_ws, const int32_t* __restrict__ row_start,
                                                                        const uint32_t* __restrict__ edges, int64_t M, int64_t Ns, int H,
                                                                        float* __restrict__ d_s) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t MH = static_cast<uint32_t>(M * H);
  const XcdBand band = xcd_band(Ns, w, KP_WAVES);
  for (int64_t n = band.begin; n < band.end; n += band.stride) {
    int b = row_start[n], e = row_start[n + 1];
    b = max(0, min(b, static_cast<int>(MH)));
    e = max(b, min(e, static_cast<int>(MH)));
    float tx = 0.f, ty = 0.f, tz = 0.f;
    for (int p = b + lane; p < e; p += 64) {
      const uint32_t ed = edges[p];
      if (ed >= MH) continue;                              // a list entry outside the forward list is skipped, never dereferenced
      tx += v_ws[3 * static_cast<int64_t>(ed)];
      ty += v_ws[3 * static_cast<int64_t>(ed) + 1];
      tz += v_ws[3 * static_cast<int64_t>(ed) + 2];
    }
    tx = wave_sum(tx);
    ty = wave_sum(ty);
    tz = wave_sum(tz);
    if (lane < 3) d_s[3 * n + lane] = -(lane == 0 ? tx : (lane == 1 ? ty : tz));
  }
}

// ---- C_in = 1 -------------------------------------------------------------------------------------------------------------------
// out[m][o] = (sum_k a[m][k] W[k][o]) / div[m] + bias[o], a[m][k] = sum_h w(m,h,k) f[idx[m,h]], div = max(1, #{h: f > 0}).
// Pass 1: workgroup b owns the queries [b * CG_ROWS, (b + 1) * CG_ROWS); a wavefront computes a[m][:] (lanes = neighbours) and adds
// a[m][k] * dOut[m][o] / div to its lanes' registers (lanes = output channels); the four wavefronts are folded in LDS, wavefront 0 first,
// and the block writes part[b][16][Cout] (row 15: dbias).  Pass 2 adds the blocks in ascending order in fp64.  The chunking depends on M alone.
constexpr int CG_ROWS = 256;

template <typename IdxT, int MAXO>
__global__ __launch_bounds__(KP_WAVES * 64) void k_cin1_grad_partial(const float* __restrict__ d_out, const float* __restrict__ s_feats,
                                                                     const float* __restrict__ q_pts, const float* __restrict__ s_pts,
                                                                     const IdxT* __restrict__ idx, const float* __restrict__ nn_saved, int64_t M, int64_t Ns,
                                                                     int H, KPoints kp, float sigma, const float* __restrict__ W, int Cout,
                                                                     float* __restrict__ part, float* __restrict__ gk) {
  __shared__ float s_fold[16][64 * MAXO];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float inv_sigma = 1.f / sigma;
  float acc[MAXO][16];
#pragma unroll
  for (int q = 0; q < MAXO; ++q)
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[q][k] = 0.f;
  const int64_t m_lo = static_cast<int64_t>(blockIdx.x) * CG_ROWS, m_hi = min(M, m_lo + CG_ROWS);
  for (int64_t m = m_lo + w; m < m_hi; m += KP_WAVES) {
    const float qx = q_pts[3 * m], qy = q_pts[3 * m + 1], qz = q_pts[3 * m + 2];
    float a[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = 0.f;
    for (int h = lane; h < H; h += 64) {
      const int64_t j = static_cast<int64_t>(idx[m * H + h]);
      if (j >= 0 && j < Ns) {
        const float f = s_feats[j];
        a[15] += f > 0.f ? 1.f : 0.f;
        const float dx = s_pts[3 * j] - qx, dy = s_pts[3 * j + 1] - qy, dz = s_pts[3 * j + 2] - qz;
#pragma unroll
        for (int k = 0; k < KP_K; ++k) a[k] = fmaf(kp_influence(dx, dy, dz, kp.p[k][0], kp.p[k][1], kp.p[k][2], inv_sigma), f, a[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = wave_sum(a[k]);
    const float cnt = nn_saved ? nn_saved[m] : a[15];
    const float div = cnt > 1.f ? cnt : 1.f;
    float gsum[KP_K];
#pragma unroll
    for (int k = 0; k < KP_K; ++k) gsum[k] = 0.f;
#pragma unroll
    for (int q = 0; q < MAXO; ++q) {
      const int o = lane + 64 * q;
      const float g = o < Cout ? d_out[m * Cout + o] : 0.f;
      const float gd = g / div;
#pragma unroll
      for (int k = 0; k < KP_K; ++k) acc[q][k] = fmaf(a[k], gd, acc[q][k]);
      acc[q][15] += g;
      if (gk) {
#pragma unroll
        for (int k = 0; k < KP_K; ++k) gsum[k] = fmaf(o < Cout ? W[k * Cout + o] : 0.f, gd, gsum[k]);
      }
    }
    if (gk) {                                            // gk[m][k] = sum_o W[k][o] dOut[m][o] / div: what d_s_feats gathers
#pragma unroll
      for (int k = 0; k < KP_K; ++k) {
        const float t = wave_sum(gsum[k]);
        if (lane == 0) gk[m * 16 + k] = t;
      }
    }
  }
  for (int ww = 0; ww < KP_WAVES; ++ww) {                  // the wavefronts add their sums one after the other, wavefront 0 first
    if (w == ww) {
#pragma unroll
      for (int q = 0; q < MAXO; ++q)
#pragma unroll
        for (int k = 0; k < 16; ++k) s_fold[k][lane + 64 * q] = ww == 0 ? acc[q][k] : s_fold[k][lane + 64 * q] + acc[q][k];
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < 16 * Cout; i += blockDim.x) {
    const int k = i / Cout, o = i - k * Cout;
    part[(static_cast<int64_t>(blockIdx.x) * 16 + k) * Cout + o] = s_fold[k][o];
  }
}

__global__ __launch_bounds__(256) void k_cin1_grad_fold(const float* __restrict__ part, int nblk, int Cout, float* __restrict__ dW,
                                                        float* __restrict__ dbias) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 16 * Cout) return;
  double t = 0.0;
  for (int b = 0; b < nblk; ++b) t += static_cast<double>(part[static_cast<int64_t>(b) * 16 * Cout + i]);
  const int k = i / Cout, o = i - k * Cout;
  if (k < KP_K) dW[k * Cout + o] = static_cast<float>(t);
  else if (dbias) dbias[o] = static_cast<float>(t);
}

// d_s_feats[n] = sum over the edges (m,h) of n, sum_k w(m,h,k) gk[m][k]: one wavefront per support, lanes = edges, folded once per row
__global__ __launch_bounds__(KP_WAVES * 64) void k_cin1_grad_feats(const float* __restrict__ gk, const float* __restrict__ q_pts,
                                                                   const float* __restrict__ s_pts, const int32_t* __restrict__ row_start,
                                                                   const uint32_t* __restrict__ edges, int64_t M, int64_t Ns, int H, KPoints kp,
                                                                   float sigma, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float inv_sigma = 1.f / sigma;
  const uint32_t MH = static_cast<uint32_t>(M * H);
  const XcdBand band = xcd_band(Ns, w, KP_WAVES);
  for (int64_t n = band.begin; n < band.end; n += band.stride) {
    int b = row_start[n], e = row_start[n + 1];
    b = max(0, min(b, static_cast<int>(MH)));
    e = max(b, min(e, static_cast<int>(MH)));
    const float sx = s_pts[3 * n], sy = s_pts[3 * n + 1], sz = s_pts[3 * n + 2];
    float t = 0.f;
    for (int p = b + lane; p < e; p += 64) {
      const uint32_t ed = edges[p];
      if (ed >= MH) continue;
      const int64_t m = ed / static_cast<uint32_t>(H);
      const float dx = sx - q_pts[3 * m], dy = sy - q_pts[3 * m + 1], dz = sz - q_pts[3 * m + 2];
#pragma unroll
      for (int k = 0; k < KP_K; ++k) t = fmaf(kp_influence(dx, dy, dz, kp.p[k][0], kp.p[k][1], kp.p[k][2], inv_sigma), gk[m * 16 + k], t);
    }
    t = wave_sum(t);
    if (lane == 0) out[n] = t;
  }
}

// ---- max-pool -------------------------------------------------------------------------------------------------------------------
// winners[m][c] = the first column h of row m holding a real index with x[idx[m,h]][c] == out[m][c]; 255 when there is none (the zero
// shadow row owns the maximum: its gradient goes nowhere)
template <typename IdxT>
__global__ __launch_bounds__(256) void k_maxpool_winners(const float* __restrict__ x, const IdxT* __restrict__ idx, const float* __restrict__ pooled,
                                                         int64_t M, int64_t Ns, int H, int C, uint8_t* __restrict__ winners) {
  __shared__ int32_t s_idx[4][KP_HMAX];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t m = static_cast<int64_t>(blockIdx.x) * 4 + w; m < M; m += static_cast<int64_t>(gridDim.x) * 4) {
    for (int h = lane; h < H; h += 64) {
      const int64_t j = static_cast<int64_t>(idx[m * H + h]);
      s_idx[w][h] = (j >= 0 && j < Ns) ? static_cast<int32_t>(j) : -1;
    }
    wave_sync();
    for (int c = lane; c < C; c += 64) {
      const float top = pooled[m * C + c];
      int win = 255;
      for (int h = H - 1; h >= 0; --h) {
        const int j = s_idx[w][h];
        if (j >= 0 && x[static_cast<int64_t>(j) * C + c] == top) win = h;
      }
      winners[m * C + c] = static_cast<uint8_t>(win);
    }
    wave_sync();
  }
}

__global__ __launch_bounds__(256) void k_maxpool_grad(const float* __restrict__ d_out, const uint8_t* __restrict__ winners,
                                                      const int32_t* __restrict__ row_start, const uint32_t* __restrict__ edges, int64_t M, int64_t Ns,
                                                      int H, int C, float* __restrict__ dx) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t MH = static_cast<uint32_t>(M * H);
  const XcdBand band = xcd_band(Ns, w, 4);
  for (int64_t n = band.begin; n < band.end; n += band.stride) {
    int b = row_start[n], e = row_start[n + 1];
    b = max(0, min(b, static_cast<int>(MH)));
    e = max(b, min(e, static_cast<int>(MH)));
    for (int c = lane; c < C; c += 64) {
      float t = 0.f;
      for (int p = b; p < e; ++p) {
        const uint32_t ed = edges[p];                      // wave-uniform
        if (ed >= MH) continue;
        const uint32_t m = ed / static_cast<uint32_t>(H), h = ed - m * static_cast<uint32_t>(H);
        if (winners[static_cast<int64_t>(m) * C + c] == h) t += d_out[static_cast<int64_t>(m) * C + c];
      }
      dx[n * C + c] = t;
    }
  }
}

static bool list_args_ok(int64_t M, int64_t Ns, int H) {
  return M >= 0 && Ns >= 0 && Ns < (int64_t(1) << 31) - 1 && H >= 1 && H <= KP_HMAX && M * H < (int64_t(1) << 30);
}

}  // namespace lcr

using namespace lcr;

extern "C" int lcr_neighbor_transpose_ws_bytes(int64_t M, int H, size_t* bytes) {
  if (!bytes || M < 0 || H < 1 || H > KP_HMAX || M * H >= (int64_t(1) << 30))
    return refuse(LCR_EARG, "lcr_neighbor_transpose_ws_bytes: bad argument (H in [1,%d], M * H < 2^30)", KP_HMAX);
  *bytes = nt_layout(nullptr, M * H).bytes;
  return LCR_OK;
}

extern "C" int lcr_neighbor_transpose(const void* idx, int idx_is_64, int64_t M, int64_t Ns, int H, int32_t* row_start, uint32_t* edges,
                                      void* ws, size_t ws_bytes, void* stream) {
  if (!idx || !row_start || !edges || !ws || !list_args_ok(M, Ns, H))
    return refuse(LCR_EARG, "lcr_neighbor_transpose: bad argument (H in [1,%d], M * H < 2^30, Ns < 2^31 - 1)", KP_HMAX);
  const int64_t E = M * H;
  const NtLayout L = nt_layout(ws, E);
  if (ws_bytes < L.bytes) return refuse_ws(LCR_EARG, "lcr_neighbor_transpose", ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  int bits = 0;
  while ((Ns >> bits) != 0) ++bits;                        // the largest key is Ns (padding)
  const int passes = radix_passes(bits);
  if (idx_is_64) hipLaunchKernelGGL((k_nt_keys<int64_t>), dim3(blocks_for(E)), dim3(256), 0, st, static_cast<const int64_t*>(idx), E, Ns, passes, L.ctl, L.kA, L.vA);
  else hipLaunchKernelGGL((k_nt_keys<int32_t>), dim3(blocks_for(E)), dim3(256), 0, st, static_cast<const int32_t*>(idx), E, Ns, passes, L.ctl, L.kA, L.vA);
  if (E > 0) {
    const int rc = radix_sort_pairs("lcr_neighbor_transpose", L.ctl, L.kA, L.kB, L.vA, L.vB, E, passes, L.hist, L.scan, st);
    if (rc) return rc;
  }
  const bool in_b = (passes & 1) != 0;
  hipLaunchKernelGGL(k_nt_rows, dim3(blocks_for(std::max(E, Ns + 1))), dim3(256), 0, st, in_b ? L.kB : L.kA, in_b ? L.vB : L.vA, E, Ns, row_start, edges);
  return check_launch("lcr_neighbor_transpose");
}

extern "C" int lcr_kpconv_aggregate_grad(const float* dA, const float* q_pts, const float* s_pts, const int32_t* row_start, const uint32_t* edges,
                                         int64_t M, int64_t Ns, int H, int C, const float* kernel_points_host, float sigma, float* d_s_feats,
                                         void* stream) {
  if (!dA || !q_pts || !s_pts || !row_start || !edges || !kernel_points_host || !d_s_feats || !list_args_ok(M, Ns, H) || !(sigma > 0.f))
    return refuse(LCR_EARG, "lcr_kpconv_aggregate_grad: bad argument (H in [1,%d], M * H < 2^30)", KP_HMAX);
  if (C != 32 && C != 64 && C != 128 && C != 256) return refuse(LCR_EARG, "lcr_kpconv_aggregate_grad: C must be 32, 64, 128 or 256 (got %d)", C);
  if (Ns == 0) return LCR_OK;
  const KPoints kp = load_kp(kernel_points_host);
  hipStream_t st = ST(stream);
  dim3 grid(grid_for_xcd(Ns, KP_WAVES)), block(KP_WAVES * 64);
#define LCR_AGG_GRAD(CC) \
  hipLaunchKernelGGL((k_kpconv_aggregate_grad<CC>), grid, block, 0, st, dA, q_pts, s_pts, row_start, edges, M, Ns, H, kp, sigma, d_s_feats)
  switch (C) {
    case 32: LCR_AGG_GRAD(32); break;
    case 64: LCR_AGG_GRAD(64); break;
    case 128: LCR_AGG_GRAD(128); break;
    default: LCR_AGG_GRAD(256); break;
  }
#undef LCR_AGG_GRAD
  return check_launch("lcr_kpconv_aggregate_grad");
}

static size_t points_grad_bytes(int64_t M, int H) { return align_up(static_cast<size_t>(std::max<int64_t>(M * H, 1)) * 3 * sizeof(float)); }

extern "C" int lcr_kpconv_points_grad_ws_bytes(int64_t M, int H, size_t* bytes) {
  if (!bytes || M < 0 || H < 1 || H > KP_HMAX || M * H >= (int64_t(1) << 30))
    return refuse(LCR_EARG, "lcr_kpconv_points_grad_ws_bytes: bad argument (H in [1,%d], M * H < 2^30)", KP_HMAX);
  *bytes = points_grad_bytes(M, H);
  return LCR_OK;
}

extern "C" int lcr_kpconv_points_grad(const float* dA, const float* s_feats, const float* q_pts, const float* s_pts, const void* idx, int idx_is_64,
                                      const int32_t* row_start, const uint32_t* edges, int64_t M, int64_t Ns, int H, int C,
                                      const float* kernel_points_host, float sigma, float* d_q, float* d_s, void* ws, size_t ws_bytes, void* stream) {
  if (!list_args_ok(M, Ns, H) || !kernel_points_host || !(sigma > 0.f) || (M > 0 && (!dA || !q_pts || !idx)) || (Ns > 0 && (!s_feats || !s_pts)) ||
      (d_s && (!row_start || !edges || !ws)))
    return refuse(LCR_EARG, "lcr_kpconv_points_grad: bad argument (H in [1,%d], M * H < 2^30; d_s needs the inverted list and the workspace)", KP_HMAX);
  if (C != 32 && C != 64 && C != 128 && C != 256) return refuse(LCR_EARG, "lcr_kpconv_points_grad: C must be 32, 64, 128 or 256 (got %d)", C);
  if (d_s && ws_bytes < points_grad_bytes(M, H)) return refuse_ws(LCR_EARG, "lcr_kpconv_points_grad", ws_bytes, points_grad_bytes(M, H));
  if ((!d_q && !d_s) || (M == 0 && (Ns == 0 || !d_s))) return LCR_OK;
  const KPoints kp = load_kp(kernel_points_host);
  hipStream_t st = ST(stream);
  float* v_ws = d_s ? static_cast<float*>(ws) : nullptr;
  if (M > 0) {
    dim3 grid(grid_for_xcd(M, KP_WAVES)), block(KP_WAVES * 64);
#define LCR_PTS_GRAD(CC)                                                                                                                                   \
  do {                                                                                                                                                     \
    if (idx_is_64) hipLaunchKernelGGL((k_kpconv_points_grad<CC, int64_t>), grid, block, 0, st, dA, s_feats, q_pts, s_pts, static_cast<const int64_t*>(idx), \
                                      M, Ns, H, kp, sigma, v_ws, d_q);                                                                                     \
    else hipLaunchKernelGGL((k_kpconv_points_grad<CC, int32_t>), grid, block, 0, st, dA, s_feats, q_pts, s_pts, static_cast<const int32_t*>(idx), M, Ns, H, \
                            kp, sigma, v_ws, d_q);                                                                                                         \
  } while (0)
    switch (C) {
      case 32: LCR_PTS_GRAD(32); break;
      case 64: LCR_PTS_GRAD(64); break;
      case 128: LCR_PTS_GRAD(128); break;
      default: LCR_PTS_GRAD(256); break;
    }
#undef LCR_PTS_GRAD
  }
  if (d_s && Ns > 0)                                       // M == 0: every list is empty and the rows are zeroed
    hipLaunchKernelGGL(k_kpconv_points_grad_s, dim3(grid_for_xcd(Ns, KP_WAVES)), dim3(KP_WAVES * 64), 0, st, v_ws, row_start, edges, M, Ns, H, d_s);
  return check_launch("lcr_kpconv_points_grad");
}

static size_t cin1_grad_bytes(int64_t M, int Cout, bool feats) {
  const int64_t nblk = std::max<int64_t>(1, (M + CG_ROWS - 1) / CG_ROWS);
  return align_up(static_cast<size_t>(nblk) * 16 * Cout * sizeof(float)) + (feats ? align_up(static_cast<size_t>(std::max<int64_t>(M, 1)) * 16 * sizeof(float)) : 0);
}

extern "C" int lcr_kpconv_cin1_grad_ws_bytes(int64_t M, int Cout, int want_feats, size_t* bytes) {
  if (!bytes || M < 0 || Cout < 1 || Cout > 256) return refuse(LCR_EARG, "lcr_kpconv_cin1_grad_ws_bytes: bad argument");
  *bytes = cin1_grad_bytes(M, Cout, want_feats != 0);
  return LCR_OK;
}

extern "C" int lcr_kpconv_cin1_grad(const float* d_out, const float* s_feats, const float* q_pts, const float* s_pts, const void* idx, int idx_is_64,
                                    const float* nn, const int32_t* row_start, const uint32_t* edges, int64_t M, int64_t Ns, int H,
                                    const float* kernel_points_host, float sigma, const float* W, int Cout, float* dW, float* dbias,
                                    float* d_s_feats, void* ws, size_t ws_bytes, void* stream) {
  if (!d_out || !s_feats || !q_pts || !s_pts || !idx || !kernel_points_host || !W || !dW || !ws || !list_args_ok(M, Ns, H) || Cout < 1 ||
      Cout > 256 || !(sigma > 0.f) || (d_s_feats && (!row_start || !edges)))
    return refuse(LCR_EARG, "lcr_kpconv_cin1_grad: bad argument (Cout in [1,256], H in [1,%d]; d_s_feats needs the inverted list)", KP_HMAX);
  if (ws_bytes < cin1_grad_bytes(M, Cout, d_s_feats != nullptr))
    return refuse_ws(LCR_EARG, "lcr_kpconv_cin1_grad", ws_bytes, cin1_grad_bytes(M, Cout, d_s_feats != nullptr));
  const KPoints kp = load_kp(kernel_points_host);
  hipStream_t st = ST(stream);
  const int nblk = static_cast<int>(std::max<int64_t>(1, (M + CG_ROWS - 1) / CG_ROWS));
  float* part = static_cast<float*>(ws);
  float* gk = d_s_feats ? reinterpret_cast<float*>(static_cast<char*>(ws) + align_up(static_cast<size_t>(nblk) * 16 * Cout * sizeof(float))) : nullptr;
#define LCR_CIN1_GRAD(IDX, MAXO)                                                                                                                  \
  hipLaunchKernelGGL((k_cin1_grad_partial<IDX, MAXO>), dim3(nblk), dim3(KP_WAVES * 64), 0, st, d_out, s_feats, q_pts, s_pts, static_cast<const IDX*>(idx), nn, \
                     M, Ns, H, kp, sigma, W, Cout, part, gk)
  if (idx_is_64) {
    if (Cout <= 64) LCR_CIN1_GRAD(int64_t, 1);
    else LCR_CIN1_GRAD(int64_t, 4);
  } else {
    if (Cout <= 64) LCR_CIN1_GRAD(int32_t, 1);
    else LCR_CIN1_GRAD(int32_t, 4);
  }
#undef LCR_CIN1_GRAD
  hipLaunchKernelGGL(k_cin1_grad_fold, dim3((16 * Cout + 255) / 256), dim3(256), 0, st, part, nblk, Cout, dW, dbias);
  if (d_s_feats && Ns > 0)
    hipLaunchKernelGGL(k_cin1_grad_feats, dim3(grid_for_xcd(Ns, KP_WAVES)), dim3(KP_WAVES * 64), 0, st, gk, q_pts, s_pts, row_start, edges, M, Ns, H, kp, sigma,
                       d_s_feats);
  return check_launch("lcr_kpconv_cin1_grad");
}

extern "C" int lcr_maxpool_grad(const float* d_out, const float* x, const float* pooled, const void* idx, int idx_is_64, const int32_t* row_start,
                                const uint32_t* edges, int64_t M, int64_t Ns, int H, int C, uint8_t* winners, float* d_x, void* stream) {
  if (!d_out || !x || !pooled || !idx || !row_start || !edges || !winners || !d_x || !list_args_ok(M, Ns, H) || C < 1)
    return refuse(LCR_EARG, "lcr_maxpool_grad: bad argument (H in [1,%d], M * H < 2^30)", KP_HMAX);
  hipStream_t st = ST(stream);
  if (M > 0) {
    const int grid = blocks_for(M, 4);
    if (idx_is_64) hipLaunchKernelGGL((k_maxpool_winners<int64_t>), dim3(grid), dim3(256), 0, st, x, static_cast<const int64_t*>(idx), pooled, M, Ns, H, C, winners);
    else hipLaunchKernelGGL((k_maxpool_winners<int32_t>), dim3(grid), dim3(256), 0, st, x, static_cast<const int32_t*>(idx), pooled, M, Ns, H, C, winners);
  }
  if (Ns > 0) hipLaunchKernelGGL(k_maxpool_grad, dim3(grid_for_xcd(Ns, 4)), dim3(256), 0, st, d_out, winners, row_start, edges, M, Ns, H, C, d_x);
  return check_launch("lcr_maxpool_grad");
}
