// pose_tail.hip — a-10: device kernels of the registration tail that are neither Sinkhorn (sinkhorn.hip), matching (matching.hip)
// nor the pose fit (lgr.hip); no host round trips between them.
//
// Reference (all PyTorch op chains, several with .cpu() hops and Python loops):
//   vote offsets + clamp          modules/vote/vote.py:146-182
//   greedy NMS                    modules/vote/vote.py:13-70   (Python loop over ~840 nodes, order dependent)
//   node centres                  backbone4.py:161-175         (mean of the in-radius voted points)
//   point-to-node partition       modules/ops/pointcloud_partition.py:60-107 (dense M x N distances + top-k 128)
//   nearest upsample + concat     modules/kpconv/functional.py:6-22, backbone4.py:355-367
//
// Everything here is small, integer / latency bound work; kernels are sized one workgroup per problem instance
// (cloud, node) so that batches of pairs fill the chip.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace lcr {

// ---- vote: shifted = xyz + off * min(1, max_range / |off|) ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vote_shift(const float* __restrict__ xyz, const float* __restrict__ off, int64_t N, float max_range,
                                                    float* __restrict__ out) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < N; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float ox = off[3 * i], oy = off[3 * i + 1], oz = off[3 * i + 2];
    const float d = sqrtf(ox * ox + oy * oy + oz * oz);
    const float a = d > max_range ? max_range / d : 1.f;
    out[3 * i + 0] = xyz[3 * i + 0] + ox * a;
    out[3 * i + 1] = xyz[3 * i + 1] + oy * a;
    out[3 * i + 2] = xyz[3 * i + 2] + oz * a;
  }
}

// reverse: with a = R / |o| and o^ = o / |o|, d_off = a (g - o^ (o^ . g)) where the forward clipped (the same |o| and the same comparison), else g
__global__ __launch_bounds__(256) void k_vote_shift_grad(const float* __restrict__ off, const float* __restrict__ g, int64_t N, float max_range,
                                                         float* __restrict__ d_off) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < N; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float ox = off[3 * i], oy = off[3 * i + 1], oz = off[3 * i + 2];
    float gx = g[3 * i], gy = g[3 * i + 1], gz = g[3 * i + 2];
    const float d = sqrtf(ox * ox + oy * oy + oz * oz);
    if (d > max_range) {
      const float a = max_range / d, ux = ox / d, uy = oy / d, uz = oz / d;
      const float dot = ux * gx + uy * gy + uz * gz;
      gx = a * (gx - ux * dot);
      gy = a * (gy - uy * dot);
      gz = a * (gz - uz * dot);
    }
    d_off[3 * i + 0] = gx;
    d_off[3 * i + 1] = gy;
    d_off[3 * i + 2] = gz;
  }
}

// ---- greedy NMS: exact parallel replay of the sequential rule ------------------------------------------------------------
// keep[i] <=> no kept j < i with ||p_i - p_j + 1e-6|| <= radius (nn.PairwiseDistance semantics, vote.py:48-54).  Each round,
// an undecided node is dropped if a kept lower node is in range, kept if no lower node in range is still undecided.  Every
// round decides at least the lowest undecided node, so the loop terminates; real clouds need ~10 rounds.
constexpr int NMS_T = 1024;
constexpr int NMS_NB = 24;   // lower-index in-range neighbours cached per node (more -> that node rescans)
__global__ __launch_bounds__(NMS_T) void k_greedy_nms(const float* __restrict__ pts, const int64_t* __restrict__ len, int B, float radius,
                                                      uint8_t* __restrict__ keep, int64_t* __restrict__ out_len, int8_t* __restrict__ state_ws,
                                                      int32_t* __restrict__ nbr_ws) {
  __shared__ int s_undecided, s_cnt;
  const int b = blockIdx.x;
  int64_t o = 0;
  for (int i = 0; i < b; ++i) o += len[i];
  const int n = static_cast<int>(len[b]);
  const float* p = pts + 3 * o;
  int8_t* st = state_ws + o;                       // 0 undecided, 1 kept, 2 dropped
  int32_t* nbr = nbr_ws + o * (NMS_NB + 1);        // [n][1 + NMS_NB]: count (or -1 = overflow), then indices
  auto in_range = [&](int i, int j) {
    const float dx = p[3 * i] - p[3 * j] + 1e-6f, dy = p[3 * i + 1] - p[3 * j + 1] + 1e-6f, dz = p[3 * i + 2] - p[3 * j + 2] + 1e-6f;
    return !(sqrtf(dx * dx + dy * dy + dz * dz) > radius);
  };
  for (int i = threadIdx.x; i < n; i += NMS_T) {
    st[i] = i == 0 ? 1 : 0;
    int c = 0;
    for (int j = 0; j < i; ++j)
      if (in_range(i, j)) {
        if (c < NMS_NB) nbr[i * (NMS_NB + 1) + 1 + c] = j;
        ++c;
      }
    nbr[i * (NMS_NB + 1)] = c <= NMS_NB ? c : -1;
  }
  __syncthreads();
  while (true) {
    if (threadIdx.x == 0) s_undecided = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += NMS_T) {
      if (st[i] != 0) continue;
      bool blocked = false, dropped = false;
      const int c = nbr[i * (NMS_NB + 1)];
      if (c >= 0) {
        for (int q = 0; q < c && !dropped; ++q) {
          const int8_t sj = st[nbr[i * (NMS_NB + 1) + 1 + q]];   // may be one round stale: only delays a decision
          dropped = sj == 1;
          blocked |= sj == 0;
        }
      } else {
        for (int j = 0; j < i && !dropped; ++j) {
          const int8_t sj = st[j];
          if (sj == 2 || !in_range(i, j)) continue;
          dropped = sj == 1;
          blocked |= sj == 0;
        }
      }
      if (dropped) st[i] = 2;
      else if (!blocked) st[i] = 1;
      else s_undecided = 1;
    }
    __syncthreads();
    const bool done = !s_undecided;
    __syncthreads();
    if (done) break;
  }
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  int c = 0;
  for (int i = threadIdx.x; i < n; i += NMS_T) {
    const bool k = st[i] == 1;
    keep[o + i] = k ? 1 : 0;
    c += k;
  }
  atomicAdd(&s_cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) out_len[b] = s_cnt;
}

// ---- mean of the valid neighbours of every row (sequential in row order like the reference's sum) -------------------------
template <typename IdxT>
__global__ __launch_bounds__(256) void k_neighbor_mean(const float* __restrict__ pts, const IdxT* __restrict__ idx, int64_t M, int H, int64_t pad,
                                                       float* __restrict__ out) {
  for (int64_t m = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; m < M; m += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int c = 0;
    for (int h = 0; h < H; ++h) {
      const int64_t j = static_cast<int64_t>(idx[m * H + h]);
      if (j >= 0 && j < pad) {
        sx += pts[3 * j];
        sy += pts[3 * j + 1];
        sz += pts[3 * j + 2];
        ++c;
      }
    }
    const float d = static_cast<float>(c);
    out[3 * m] = sx / d;
    out[3 * m + 1] = sy / d;
    out[3 * m + 2] = sz / d;
  }
}

// reverse: d_pts[j] = sum of d_out[m] / c_m over the edges (m,h) of j.  One wavefront per point; lane l takes the positions l, l + 64, ... of
// the point's inverted list in order, recounts c_m over row m exactly as the forward does, and the lanes are folded once.
template <typename IdxT>
__global__ __launch_bounds__(256) void k_neighbor_mean_grad(const float* __restrict__ d_out, const IdxT* __restrict__ idx, const int32_t* __restrict__ row_start,
                                                            const uint32_t* __restrict__ edges, int64_t M, int H, int64_t pad, float* __restrict__ d_pts) {
  const int lane = threadIdx.x & 63;
  const uint32_t MH = static_cast<uint32_t>(M * H);          // host-checked: M * H < 2^30
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6), nwaves = static_cast<int64_t>(gridDim.x) * 4;
  for (int64_t j = wave; j < pad; j += nwaves) {
    int b = row_start[j], e = row_start[j + 1];
    b = max(0, min(b, static_cast<int>(MH)));
    e = max(b, min(e, static_cast<int>(MH)));
    float tx = 0.f, ty = 0.f, tz = 0.f;
    for (int p = b + lane; p < e; p += 64) {
      const uint32_t ed = edges[p];
      if (ed >= MH) continue;                                // a list entry outside the forward list is skipped, never dereferenced
      const int64_t m = ed / static_cast<uint32_t>(H);
      int c = 0;
      for (int h = 0; h < H; ++h) {
        const int64_t q = static_cast<int64_t>(idx[m * H + h]);
        c += (q >= 0 && q < pad) ? 1 : 0;
      }
      const float d = static_cast<float>(c);
      tx += d_out[3 * m] / d;
      ty += d_out[3 * m + 1] / d;
      tz += d_out[3 * m + 2] / d;
    }
    tx = wave_sum(tx);
    ty = wave_sum(ty);
    tz = wave_sum(tz);
    if (lane < 3) d_pts[3 * j + lane] = lane == 0 ? tx : (lane == 1 ? ty : tz);
  }
}

// ---- point-to-node partition ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float p2n_dist(float nx, float ny, float nz, float n2, float px, float py, float pz, float p2) {
  // pairwise_distance (modules/ops/pairwise_distance.py:18-31): x2 - 2*xy + y2, clamped at 1e-12
  const float xy = nx * px + ny * py + nz * pz;
  return fmaxf((n2 - 2.f * xy) + p2, 1e-12f);
}

constexpr int PT_CAP = 4096;   // own points held in LDS per node

// The partition of a STACK of clouds in one launch sequence (the pair model calls it for the 2P clouds of a group of pairs: 12 x (a fill +
// 3 kernels + a scan) per 6 pairs otherwise; the single-cloud entry is the stack of one).  Offsets are host values passed by value; point /
// node indices in the outputs stay LOCAL to their cloud.
//   k_point_to_node_stack   nearest node of every point (ties: lowest node index); per-node point counts
//   k_p2n_scatter_stack     every point into its node's member list
//   k_node_topk_stack       per node: its K nearest own points, ascending (d2, index); padded with N.  One workgroup per node.
constexpr int P2N_MAX_CLOUDS = 64;
struct P2nStack {
  int64_t po[P2N_MAX_CLOUDS + 1];   // first point row of every cloud
  int32_t mo[P2N_MAX_CLOUDS + 1];   // first node row of every cloud
  int     C;
};
__global__ __launch_bounds__(256) void k_point_to_node_stack(const float* __restrict__ points, const float* __restrict__ nodes, P2nStack sk,
                                                              int32_t* __restrict__ p2n, int32_t* __restrict__ node_cnt) {
  extern __shared__ float s_nodes[];   // [M_c][4] (x,y,z,|n|^2)
  const int c = blockIdx.y;
  const int64_t p0 = sk.po[c], N = sk.po[c + 1] - p0;
  const int m0 = sk.mo[c], M = sk.mo[c + 1] - m0;
  for (int i = threadIdx.x; i < M; i += blockDim.x) {
    const float x = nodes[3 * (m0 + i)], y = nodes[3 * (m0 + i) + 1], z = nodes[3 * (m0 + i) + 2];
    s_nodes[4 * i] = x;
    s_nodes[4 * i + 1] = y;
    s_nodes[4 * i + 2] = z;
    s_nodes[4 * i + 3] = x * x + y * y + z * z;
  }
  __syncthreads();
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < N; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float px = points[3 * (p0 + i)], py = points[3 * (p0 + i) + 1], pz = points[3 * (p0 + i) + 2];
    const float p2 = px * px + py * py + pz * pz;
    float best = INFINITY;
    int bi = 0;
    for (int m = 0; m < M; ++m) {
      const float d = p2n_dist(s_nodes[4 * m], s_nodes[4 * m + 1], s_nodes[4 * m + 2], s_nodes[4 * m + 3], px, py, pz, p2);
      if (d < best) {
        best = d;
        bi = m;
      }
    }
    p2n[p0 + i] = bi;
    if (M > 0) atomicAdd(&node_cnt[m0 + bi], 1);
  }
}
__global__ __launch_bounds__(256) void k_p2n_scatter_stack(const int32_t* __restrict__ p2n, P2nStack sk, const int32_t* __restrict__ node_start,
                                                           int32_t* __restrict__ cursor, int32_t* __restrict__ members) {
  const int c = blockIdx.y;
  const int64_t p0 = sk.po[c], N = sk.po[c + 1] - p0;
  const int m0 = sk.mo[c];
  if (sk.mo[c + 1] == m0) return;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < N; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int m = m0 + p2n[p0 + i];
    members[node_start[m] + atomicAdd(&cursor[m], 1)] = static_cast<int32_t>(i);      // local point index
  }
}
__global__ __launch_bounds__(256) void k_node_topk_stack(const float* __restrict__ points, const float* __restrict__ nodes, P2nStack sk,
                                                         const int32_t* __restrict__ node_start, const int32_t* __restrict__ members, int K,
                                                         int64_t* __restrict__ knn, uint8_t* __restrict__ knn_mask, uint8_t* __restrict__ node_mask,
                                                         uint32_t* __restrict__ status) {
  __shared__ uint64_t s_key[PT_CAP];
  const int m = blockIdx.x;
  const int c = cloud_of(sk.mo, sk.C, m);                   // block-uniform
  const int64_t p0 = sk.po[c], N = sk.po[c + 1] - p0;
  const float* pts = points + 3 * p0;
  const int a = node_start[m], n_all = node_start[m + 1] - a;
  const int n = n_all < PT_CAP ? n_all : PT_CAP;
  if (n_all > PT_CAP && threadIdx.x == 0) atomicOr(status, LCR_STATUS_LEN_MISMATCH);
  const float nx = nodes[3 * m], ny = nodes[3 * m + 1], nz = nodes[3 * m + 2];
  const float n2 = nx * nx + ny * ny + nz * nz;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int32_t pi = members[a + i];
    const float px = pts[3 * pi], py = pts[3 * pi + 1], pz = pts[3 * pi + 2];
    const float d = p2n_dist(nx, ny, nz, n2, px, py, pz, px * px + py * py + pz * pz);
    s_key[i] = (static_cast<uint64_t>(__float_as_uint(d)) << 32) | static_cast<uint32_t>(pi);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    const uint64_t key = s_key[e];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += s_key[j] < key;
    if (rank < K) {
      knn[static_cast<int64_t>(m) * K + rank] = static_cast<int64_t>(static_cast<uint32_t>(key));
      knn_mask[static_cast<int64_t>(m) * K + rank] = 1;
    }
  }
  for (int col = n + threadIdx.x; col < K; col += blockDim.x) {
    knn[static_cast<int64_t>(m) * K + col] = N;
    knn_mask[static_cast<int64_t>(m) * K + col] = 0;
  }
  if (threadIdx.x == 0) node_mask[m] = n_all > 0 ? 1 : 0;
}

// ---- decoder: out[n] = [ x[idx[n][0]] (zeros for the shadow index) , skip[n] ] -------------------------------------------------
template <typename IdxT>
__global__ __launch_bounds__(256) void k_upsample_concat(const float* __restrict__ x, int64_t Nx, int C1, const IdxT* __restrict__ idx, int H,
                                                         const float* __restrict__ skip, int C2, int64_t N, float* __restrict__ out) {
  const int C = C1 + C2;
  const int64_t total = N * C;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < total; t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t n = t / C;
    const int c = static_cast<int>(t - n * C);
    float v;
    if (c < C1) {
      const int64_t j = static_cast<int64_t>(idx[n * H]);
      v = (j >= 0 && j < Nx) ? x[j * C1 + c] : 0.f;
    } else {
      v = skip[n * C2 + (c - C1)];
    }
    out[t] = v;
  }
}

// out[r][:] = src[idx[r]][:] with zeros for idx == pad (index_select on a zero-padded tensor)
__global__ __launch_bounds__(256) void k_gather_rows(const float* __restrict__ src, int64_t pad, int C, const int64_t* __restrict__ idx, int64_t R,
                                                     float* __restrict__ out) {
  const int64_t total = R * C;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < total; t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t r = t / C;
    const int c = static_cast<int>(t - r * C);
    const int64_t j = idx[r];
    out[t] = (j >= 0 && j < pad) ? src[j * C + c] : 0.f;
  }
}

// Row-wise forms of the two gathers above (C1, C2 / C multiples of 4, 16-byte aligned bases — every call of the pair model): one wavefront
// per output row, 16-byte lanes, the row's index read once.  The element-wise forms spend a 64-bit division and a 4-byte access per
// value (PMC: 6 % and 3 % of the pair model's VALU instructions for two copies).
template <typename IdxT>
__global__ __launch_bounds__(256) void k_upsample_concat_rows(const float* __restrict__ x, int64_t Nx, int C1, const IdxT* __restrict__ idx, int H,
                                                              const float* __restrict__ skip, int C2, int64_t N, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int q1 = C1 >> 2, q = (C1 + C2) >> 2;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6), nwaves = static_cast<int64_t>(gridDim.x) * 4;
  for (int64_t n = wave; n < N; n += nwaves) {
    const int64_t j = static_cast<int64_t>(idx[n * H]);
    const bool ok = j >= 0 && j < Nx;
    const float4* xr = reinterpret_cast<const float4*>(x + (ok ? j : 0) * C1);
    const float4* sr = reinterpret_cast<const float4*>(skip + n * C2);
    float4* o = reinterpret_cast<float4*>(out + n * (C1 + C2));
    for (int c = lane; c < q; c += 64) {
      float4 v;
      if (c < q1) {
        v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) v = xr[c];                                   // the shadow index (and an empty x) read nothing
      } else {
        v = sr[c - q1];
      }
      o[c] = v;
    }
  }
}
__global__ __launch_bounds__(256) void k_gather_rows_vec(const float* __restrict__ src, int64_t pad, int C, const int64_t* __restrict__ idx, int64_t R,
                                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int q = C >> 2;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6), nwaves = static_cast<int64_t>(gridDim.x) * 4;
  for (int64_t r = wave; r < R; r += nwaves) {
    const int64_t j = idx[r];
    const bool ok = j >= 0 && j < pad;
    const float4* sr = reinterpret_cast<const float4*>(src + (ok ? j : 0) * C);
    float4* o = reinterpret_cast<float4*>(out + r * C);
    for (int c = lane; c < q; c += 64) o[c] = ok ? sr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// reverse of the decoder's gather: d_x[j][:] = sum of d_out[n][:C1] over the rows n that list j in column 0, in ascending n (the inverted
// form of column 0: an [N,1] list, so an edge IS its row n).  One wavefront per x row, lanes over the channels (T = float4 when the widths
// and bases allow 16-byte accesses, else float); a row nobody lists gets zeros.  q1 / q: C1 / (C1 + C2) in units of T.
__device__ __forceinline__ void acc_zero(float& a) { a = 0.f; }
__device__ __forceinline__ void acc_zero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void acc_add(float& a, float b) { a += b; }
__device__ __forceinline__ void acc_add(float4& a, const float4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}
template <typename T>
__global__ __launch_bounds__(256) void k_upsample_concat_grad_x(const T* __restrict__ d_out, const int32_t* __restrict__ row_start,
                                                                const uint32_t* __restrict__ edges, int64_t N, int64_t Nx, int q1, int q, T* __restrict__ d_x) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6), nwaves = static_cast<int64_t>(gridDim.x) * 4;
  const int n_max = static_cast<int>(N);                     // host-checked: N < 2^30
  for (int64_t j = wave; j < Nx; j += nwaves) {
    int b = row_start[j], e = row_start[j + 1];
    b = max(0, min(b, n_max));
    e = max(b, min(e, n_max));
    for (int c = lane; c < q1; c += 64) {
      T t;
      acc_zero(t);
      for (int p = b; p < e; ++p) {
        const uint32_t n = edges[p];                         // wave-uniform
        if (n >= static_cast<uint32_t>(n_max)) continue;     // a list entry outside the forward list is skipped, never dereferenced
        acc_add(t, d_out[static_cast<int64_t>(n) * q + c]);
      }
      d_x[j * q1 + c] = t;
    }
  }
}
template <typename T>
__global__ __launch_bounds__(256) void k_upsample_concat_grad_skip(const T* __restrict__ d_out, int64_t N, int q1, int q, T* __restrict__ d_skip) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6), nwaves = static_cast<int64_t>(gridDim.x) * 4;
  for (int64_t n = wave; n < N; n += nwaves)
    for (int c = lane; c < q - q1; c += 64) d_skip[n * (q - q1) + c] = d_out[n * q + q1 + c];
}

}  // namespace lcr

using namespace lcr;

extern "C" int lcr_vote_shift_grad(const float* offsets, const float* d_out, int64_t N, float max_range, float* d_off, void* stream) {
  if (N == 0) return LCR_OK;
  if (!offsets || !d_out || !d_off || N < 0) return refuse(LCR_EARG, "lcr_vote_shift_grad: bad argument (null pointer or N < 0)");
  hipLaunchKernelGGL(k_vote_shift_grad, dim3(blocks_for(N)), dim3(256), 0, ST(stream), offsets, d_out, N, max_range, d_off);
  return check_launch("lcr_vote_shift_grad");
}

extern "C" int lcr_neighbor_mean_grad(const float* d_out, const void* idx, int idx_is_64, const int32_t* row_start, const uint32_t* edges, int64_t M,
                                      int H, int64_t pad, float* d_pts, void* stream) {
  if (M < 0 || pad < 0 || pad >= (int64_t(1) << 31) - 1 || H < 1 || H > 128 || M * H >= (int64_t(1) << 30) || (pad > 0 && (!row_start || !edges || !d_pts)) ||
      (M > 0 && (!d_out || !idx)))
    return refuse(LCR_EARG, "lcr_neighbor_mean_grad: bad argument (H in [1,128], M * H < 2^30, pad < 2^31 - 1, no null pointer)");
  if (pad == 0) return LCR_OK;                               // no points: nothing to write
  const int nb = blocks_for(pad, 4, 8192);                   // one wavefront per point
  if (idx_is_64) hipLaunchKernelGGL((k_neighbor_mean_grad<int64_t>), dim3(nb), dim3(256), 0, ST(stream), d_out, static_cast<const int64_t*>(idx), row_start, edges, M, H, pad, d_pts);
  else hipLaunchKernelGGL((k_neighbor_mean_grad<int32_t>), dim3(nb), dim3(256), 0, ST(stream), d_out, static_cast<const int32_t*>(idx), row_start, edges, M, H, pad, d_pts);
  return check_launch("lcr_neighbor_mean_grad");
}

extern "C" int lcr_upsample_concat_grad(const float* d_out, const int32_t* row_start, const uint32_t* edges, int64_t N, int64_t Nx, int C1, int C2,
                                        float* d_x, float* d_skip, void* stream) {
  if (N < 0 || N >= (int64_t(1) << 30) || Nx < 0 || Nx >= (int64_t(1) << 31) - 1 || C1 < 1 || C2 < 1 || (N > 0 && !d_out) ||
      (d_x && Nx > 0 && (!row_start || !edges)))
    return refuse(LCR_EARG, "lcr_upsample_concat_grad: bad argument (N < 2^30, C1, C2 >= 1; d_x needs the inverted list of column 0)");
  hipStream_t st = ST(stream);
  const bool vec = C1 % 4 == 0 && C2 % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_skip)) & 15) == 0;
  if (d_x && Nx > 0) {                                       // N == 0: every list is empty and the rows are zeroed
    const int nb = blocks_for(Nx, 4, 8192);
    if (vec) hipLaunchKernelGGL((k_upsample_concat_grad_x<float4>), dim3(nb), dim3(256), 0, st, reinterpret_cast<const float4*>(d_out), row_start, edges, N, Nx, C1 / 4, (C1 + C2) / 4, reinterpret_cast<float4*>(d_x));
    else hipLaunchKernelGGL((k_upsample_concat_grad_x<float>), dim3(nb), dim3(256), 0, st, d_out, row_start, edges, N, Nx, C1, C1 + C2, d_x);
  }
  if (d_skip && N > 0) {
    const int nb = blocks_for(N, 4, 8192);
    if (vec) hipLaunchKernelGGL((k_upsample_concat_grad_skip<float4>), dim3(nb), dim3(256), 0, st, reinterpret_cast<const float4*>(d_out), N, C1 / 4, (C1 + C2) / 4, reinterpret_cast<float4*>(d_skip));
    else hipLaunchKernelGGL((k_upsample_concat_grad_skip<float>), dim3(nb), dim3(256), 0, st, d_out, N, C1, C1 + C2, d_skip);
  }
  return check_launch("lcr_upsample_concat_grad");
}

extern "C" int lcr_vote_shift(const float* xyz, const float* offsets, int64_t N, float max_range, float* out, void* stream) {
  if (N == 0) return LCR_OK;                               // no points: nothing to read or write, null pointers allowed
  if (!xyz || !offsets || !out || N < 0) return refuse(LCR_EARG, "lcr_vote_shift: null pointer or a negative count: N=%lld", static_cast<long long>(N));
  hipLaunchKernelGGL(k_vote_shift, dim3(blocks_for(N)), dim3(256), 0, ST(stream), xyz, offsets, N, max_range, out);
  return check_launch("lcr_vote_shift");
}

extern "C" int lcr_greedy_nms_ws_bytes(int64_t n_total, size_t* bytes) {
  if (!bytes || n_total < 0) return refuse(LCR_EARG, "lcr_greedy_nms_ws_bytes: null pointer or a negative count: n_total=%lld", static_cast<long long>(n_total));
  *bytes = align_up(static_cast<size_t>(n_total) + 16) + sizeof(int32_t) * static_cast<size_t>(n_total + 1) * (NMS_NB + 1);
  return LCR_OK;
}

extern "C" int lcr_greedy_nms(const float* pts, const int64_t* len, int B, int64_t n_total, float radius, uint8_t* keep, int64_t* out_len,
                              void* ws, void* stream) {
  if (!pts || !len || !keep || !out_len || !ws || B < 1) return refuse(LCR_EARG, "lcr_greedy_nms: null pointer or B < 1: B=%d", B);
  int8_t* st = static_cast<int8_t*>(ws);
  int32_t* nbr = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + align_up(static_cast<size_t>(n_total) + 16));
  hipLaunchKernelGGL(k_greedy_nms, dim3(B), dim3(NMS_T), 0, ST(stream), pts, len, B, radius, keep, out_len, st, nbr);
  return check_launch("lcr_greedy_nms");
}

extern "C" int lcr_neighbor_mean(const float* pts, const void* idx, int idx_is_64, int64_t M, int H, int64_t pad, float* out, void* stream) {
  if (M == 0) return LCR_OK;                               // no rows: nothing to read or write, null pointers allowed
  if (!pts || !idx || !out || M < 0 || H < 1) return refuse(LCR_EARG, "lcr_neighbor_mean: null pointer, M < 0 or H < 1: M=%lld H=%d", static_cast<long long>(M), H);
  if (idx_is_64) hipLaunchKernelGGL((k_neighbor_mean<int64_t>), dim3(blocks_for(M)), dim3(256), 0, ST(stream), pts, static_cast<const int64_t*>(idx), M, H, pad, out);
  else hipLaunchKernelGGL((k_neighbor_mean<int32_t>), dim3(blocks_for(M)), dim3(256), 0, ST(stream), pts, static_cast<const int32_t*>(idx), M, H, pad, out);
  return check_launch("lcr_neighbor_mean");
}

// workspace of the partition of N points (all clouds) over M nodes (all clouds); ws may be null (sizes only)
struct P2nLayout {
  int32_t *p2n, *members;        // [N+1] nearest node of every point; points grouped by node (both local to the cloud)
  int32_t *cnt, *start, *cursor; // [M+2] points per node, their exclusive scan, scatter cursors; ONE fill zeroes cnt .. cursor: keep them adjacent
  void*    scan_ws;
  size_t   bytes;
};
static P2nLayout p2n_layout(void* ws, int64_t N, int M) {
  P2nLayout L;
  Carver c(ws, ~size_t(0));
  L.p2n = c.take<int32_t>(N + 1);
  L.cnt = c.take<int32_t>(M + 2);
  L.start = c.take<int32_t>(M + 2);
  L.cursor = c.take<int32_t>(M + 2);
  L.members = c.take<int32_t>(N + 1);
  L.scan_ws = c.take<char>(scan_ws_bytes(M + 2));
  L.bytes = c.off;
  return L;
}

extern "C" int lcr_point_to_node_ws_bytes(int64_t N, int M, size_t* bytes) {
  if (!bytes || N < 0 || M < 1) return refuse(LCR_EARG, "lcr_point_to_node_ws_bytes: null pointer, N < 0 or M < 1: N=%lld M=%d", static_cast<long long>(N), M);
  *bytes = p2n_layout(nullptr, N, M).bytes;
  return LCR_OK;
}

// the launch sequence of both partition entries (arguments already validated but the workspace size; `entry` names the caller in a refusal)
static int p2n_run(const char* entry, const float* points, const float* nodes, const P2nStack& sk, int64_t n_max, int m_max, int K, int32_t* p2n_out,
                   int64_t* knn, uint8_t* knn_mask, uint8_t* node_mask, uint32_t* status, void* ws, size_t ws_bytes, void* stream) {
  const int C = sk.C;
  const int64_t N = sk.po[C];
  const int M = sk.mo[C];
  const P2nLayout L = p2n_layout(ws, N, M);
  if (L.bytes > ws_bytes) return refuse_ws(LCR_ESPACE, entry, ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  hipMemsetAsync(L.cnt, 0, static_cast<size_t>(reinterpret_cast<char*>(L.cursor + M + 2) - reinterpret_cast<char*>(L.cnt)), st);   // counts .. cursor: one fill
  const int bx = blocks_for(n_max, 256, 2048);
  hipLaunchKernelGGL(k_point_to_node_stack, dim3(bx, C), dim3(256), sizeof(float) * 4 * m_max, st, points, nodes, sk, L.p2n, L.cnt);
  int rc = exclusive_scan_i32(entry, L.cnt, L.start, M + 1, nullptr, L.scan_ws, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_p2n_scatter_stack, dim3(blocks_for(n_max), C), dim3(256), 0, st, L.p2n, sk, L.start, L.cursor, L.members);
  hipLaunchKernelGGL(k_node_topk_stack, dim3(M), dim3(256), 0, st, points, nodes, sk, L.start, L.members, K, knn, knn_mask, node_mask, status);
  if (p2n_out) hipMemcpyAsync(p2n_out, L.p2n, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, st);
  return check_launch(entry);
}

// point_to_node_partition (pointcloud_partition.py:60-107), a stack of one cloud: knn i64[M,K] (pad = N), knn_mask u8[M,K], node_mask u8[M], p2n i32[N]
extern "C" int lcr_point_to_node_partition(const float* points, int64_t N, const float* nodes, int M, int K, int32_t* p2n_out, int64_t* knn,
                                           uint8_t* knn_mask, uint8_t* node_mask, uint32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!points || !nodes || !knn || !knn_mask || !node_mask || !status || !ws || N < 1 || M < 1 || K < 1 || M > 4000)
    return refuse(LCR_EARG, "lcr_point_to_node_partition: bad argument (1 <= M <= 4000)");
  const P2nStack sk = {{0, N}, {0, M}, 1};
  return p2n_run("lcr_point_to_node_partition", points, nodes, sk, N, M, K, p2n_out, knn, knn_mask, node_mask, status, ws, ws_bytes, stream);
}

// point_to_node_partition of C stacked clouds (cloud c: points [point_off[c], point_off[c+1]), nodes [node_off[c], node_off[c+1]); host
// offsets): the per-cloud results stacked — p2n i32[N_total] and knn i64[M_total, K] hold indices LOCAL to the cloud, knn padded with the
// cloud's own point count.  Workspace: lcr_point_to_node_ws_bytes(N_total, M_total).
extern "C" int lcr_point_to_node_partition_stack(const float* points, const int64_t* point_off, const float* nodes, const int64_t* node_off, int C,
                                                 int K, int32_t* p2n_out, int64_t* knn, uint8_t* knn_mask, uint8_t* node_mask, uint32_t* status,
                                                 void* ws, size_t ws_bytes, void* stream) {
  if (!points || !point_off || !nodes || !node_off || !knn || !knn_mask || !node_mask || !status || !ws || C < 1 || C > P2N_MAX_CLOUDS || K < 1)
    return refuse(LCR_EARG, "lcr_point_to_node_partition_stack: bad argument (1 <= clouds <= %d)", P2N_MAX_CLOUDS);
  P2nStack sk;
  sk.C = C;
  int64_t n_max = 0;
  int m_max = 0;
  for (int c = 0; c <= C; ++c) {
    if (c && (point_off[c] < point_off[c - 1] || node_off[c] < node_off[c - 1]))
      return refuse(LCR_EARG, "lcr_point_to_node_partition_stack: offsets must not decrease (cloud %d)", c - 1);
    sk.po[c] = point_off[c] - point_off[0];
    sk.mo[c] = static_cast<int32_t>(node_off[c] - node_off[0]);
    if (c) {
      n_max = std::max(n_max, sk.po[c] - sk.po[c - 1]);
      m_max = std::max(m_max, sk.mo[c] - sk.mo[c - 1]);
    }
  }
  if (sk.po[C] < 1 || sk.mo[C] < 1 || m_max > 4000) return refuse(LCR_EARG, "lcr_point_to_node_partition_stack: empty stack or more than 4000 nodes in a cloud");
  return p2n_run("lcr_point_to_node_partition_stack", points + 3 * point_off[0], nodes + 3 * node_off[0], sk, n_max, m_max, K, p2n_out, knn, knn_mask,
                 node_mask, status, ws, ws_bytes, stream);
}

extern "C" int lcr_upsample_concat(const float* x, int64_t Nx, int C1, const void* idx, int idx_is_64, int H, const float* skip, int C2, int64_t N,
                                   float* out, void* stream) {
  if (N == 0) return LCR_OK;
  if (!x || !idx || !skip || !out || N < 0 || C1 < 1 || C2 < 1 || H < 1)
    return refuse(LCR_EARG, "lcr_upsample_concat: null pointer, N < 0, or C1, C2 or H below 1: N=%lld C1=%d C2=%d H=%d", static_cast<long long>(N), C1, C2, H);
  const bool vec = C1 % 4 == 0 && C2 % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(skip) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  if (vec) {
    const int nbr = blocks_for(N * 64, 256, 8192);         // one wavefront per row
    if (idx_is_64) hipLaunchKernelGGL((k_upsample_concat_rows<int64_t>), dim3(nbr), dim3(256), 0, ST(stream), x, Nx, C1, static_cast<const int64_t*>(idx), H, skip, C2, N, out);
    else hipLaunchKernelGGL((k_upsample_concat_rows<int32_t>), dim3(nbr), dim3(256), 0, ST(stream), x, Nx, C1, static_cast<const int32_t*>(idx), H, skip, C2, N, out);
    return check_launch("lcr_upsample_concat");
  }
  const int nb = blocks_for(N * (C1 + C2), 256, 8192);
  if (idx_is_64) hipLaunchKernelGGL((k_upsample_concat<int64_t>), dim3(nb), dim3(256), 0, ST(stream), x, Nx, C1, static_cast<const int64_t*>(idx), H, skip, C2, N, out);
  else hipLaunchKernelGGL((k_upsample_concat<int32_t>), dim3(nb), dim3(256), 0, ST(stream), x, Nx, C1, static_cast<const int32_t*>(idx), H, skip, C2, N, out);
  return check_launch("lcr_upsample_concat");
}

extern "C" int lcr_gather_rows(const float* src, int64_t pad, int C, const int64_t* idx, int64_t R, float* out, void* stream) {
  if (R == 0) return LCR_OK;                               // an empty selection: nothing to read, null pointers allowed
  if (!src || !idx || !out || R < 0 || C < 1) return refuse(LCR_EARG, "lcr_gather_rows: null pointer, R < 0 or C < 1: R=%lld C=%d", static_cast<long long>(R), C);
  if (C % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
    hipLaunchKernelGGL(k_gather_rows_vec, dim3(blocks_for(R * 64, 256, 8192)), dim3(256), 0, ST(stream), src, pad, C, idx, R, out);
    return check_launch("lcr_gather_rows");
  }
  hipLaunchKernelGGL(k_gather_rows, dim3(blocks_for(R * C, 256, 8192)), dim3(256), 0, ST(stream), src, pad, C, idx, R, out);
  return check_launch("lcr_gather_rows");
}

