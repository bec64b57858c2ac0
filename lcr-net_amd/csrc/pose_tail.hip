// pose_tail.hip — a-10: device kernels of the registration tail (no host round trips between them).
//
// Reference (all PyTorch op chains, several with .cpu() hops and Python loops):
//   vote offsets + clamp          modules/vote/vote.py:146-182
//   greedy NMS                    modules/vote/vote.py:13-70   (Python loop over ~840 nodes, order dependent)
//   node centres                  backbone4.py:161-175         (mean of the in-radius voted points)
//   point-to-node partition       modules/ops/pointcloud_partition.py:60-107 (dense M x N distances + top-k 128)
//   log-domain Sinkhorn           modules/sinkhorn/learnable_sinkhorn.py:5-66 (100 iterations)
//   dustbin top-1 matching        geotransformer/superpoint_matching.py:130-162, local_global_registration.py:49-92
//   nearest upsample + concat     modules/kpconv/functional.py:6-22, backbone4.py:355-367
//   weighted Procrustes           modules/registration/procrustes.py:6-73 (torch.svd on the CPU) + LGR :134-200
//
// Everything here is small, integer / latency bound work; kernels are sized one workgroup per problem instance
// (cloud, score matrix, hypothesis) so that batches of pairs fill the chip.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "rigid3.h"

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

// ---- point-to-node partition ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float p2n_dist(float nx, float ny, float nz, float n2, float px, float py, float pz, float p2) {
  // pairwise_distance (modules/ops/pairwise_distance.py:18-31): x2 - 2*xy + y2, clamped at 1e-12
  const float xy = nx * px + ny * py + nz * pz;
  return fmaxf((n2 - 2.f * xy) + p2, 1e-12f);
}

// nearest node of every point (ties: lowest node index); per-node point counts
__global__ __launch_bounds__(256) void k_point_to_node(const float* __restrict__ points, int64_t N, const float* __restrict__ nodes, int M,
                                                       int32_t* __restrict__ p2n, int32_t* __restrict__ node_cnt) {
  extern __shared__ float s_nodes[];   // [M][4] (x,y,z,|n|^2)
  for (int i = threadIdx.x; i < M; i += blockDim.x) {
    const float x = nodes[3 * i], y = nodes[3 * i + 1], z = nodes[3 * i + 2];
    s_nodes[4 * i] = x;
    s_nodes[4 * i + 1] = y;
    s_nodes[4 * i + 2] = z;
    s_nodes[4 * i + 3] = x * x + y * y + z * z;
  }
  __syncthreads();
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < N; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
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
    p2n[i] = bi;
    atomicAdd(&node_cnt[bi], 1);
  }
}

__global__ __launch_bounds__(256) void k_p2n_scatter(const int32_t* __restrict__ p2n, int64_t N, const int32_t* __restrict__ node_start,
                                                     int32_t* __restrict__ cursor, int32_t* __restrict__ members) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < N; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int m = p2n[i];
    members[node_start[m] + atomicAdd(&cursor[m], 1)] = static_cast<int32_t>(i);
  }
}

// per node: its K nearest own points, ascending (d2, index); padded with N.  One workgroup per node.
constexpr int PT_CAP = 4096;   // own points held in LDS per node
__global__ __launch_bounds__(256) void k_node_topk(const float* __restrict__ points, int64_t N, const float* __restrict__ nodes,
                                                   const int32_t* __restrict__ node_start, const int32_t* __restrict__ members, int K,
                                                   int64_t* __restrict__ knn, uint8_t* __restrict__ knn_mask, uint8_t* __restrict__ node_mask,
                                                   uint32_t* __restrict__ status) {
  __shared__ uint64_t s_key[PT_CAP];
  const int m = blockIdx.x;
  const int a = node_start[m], n_all = node_start[m + 1] - a;
  const int n = n_all < PT_CAP ? n_all : PT_CAP;
  if (n_all > PT_CAP && threadIdx.x == 0) atomicOr(status, LCR_STATUS_LEN_MISMATCH);
  const float nx = nodes[3 * m], ny = nodes[3 * m + 1], nz = nodes[3 * m + 2];
  const float n2 = nx * nx + ny * ny + nz * nz;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int32_t pi = members[a + i];
    const float px = points[3 * pi], py = points[3 * pi + 1], pz = points[3 * pi + 2];
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
  for (int c = n + threadIdx.x; c < K; c += blockDim.x) {
    knn[static_cast<int64_t>(m) * K + c] = N;
    knn_mask[static_cast<int64_t>(m) * K + c] = 0;
  }
  if (threadIdx.x == 0) node_mask[m] = n_all > 0 ? 1 : 0;
}

// The same partition for a STACK of clouds in one launch sequence (the pair model calls it for the 2P clouds of a group of pairs:
// 12 x (2 fills + 3 kernels + a scan) per 6 pairs otherwise).  Offsets are host values passed by value; point / node indices in the
// outputs stay LOCAL to their cloud, as the per-cloud call returns them.
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
  int c = 0;
  while (c + 1 < sk.C && m >= sk.mo[c + 1]) ++c;            // block-uniform
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

// (a) whole problem in one workgroup, matrix AND dual vectors resident in LDS (patch level: 129 x 129 floats = 66.5 KB; from L2
//     every one of the 200 passes would be a chain of dependent ~1 us loads).  Four threads share a row (column): each takes
//     every 4th element, partials are folded with two quad shuffles.
__device__ __forceinline__ float quad_max(float x) {      // quad permutes on the DPP path (no LDS crossbar round trip)
  x = fmaxf(x, dpp0<DPP_QUAD_1032>(x));
  return fmaxf(x, dpp0<DPP_QUAD_2301>(x));
}
__device__ __forceinline__ float quad_sum(float x) {
  x += dpp0<DPP_QUAD_1032>(x);
  return x + dpp0<DPP_QUAD_2301>(x);
}

// (a') patch level, register resident: for matrices up to 132 x 132 (the 129 x 129 patch problems) every thread keeps its 33
//      row entries AND its 33 column entries in registers for all iterations — four threads per row / column, element e of part p
//      is column (row) 4e + p — so a half-iteration is 33 independent exponentials per thread plus two quad folds; LDS only
//      carries the dual vectors.  The LDS-matrix version spent ~7 us per half-iteration re-reading the matrix twice.
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

// logs below this cannot reach the exp value of a line whose largest log is m (see k_top1_stats)
__device__ __forceinline__ float top1_floor(float m) { return m < -80.f ? -INFINITY : m - 1e-5f * fmaxf(1.f, fabsf(m)); }

// ---- dustbin top-1 matching (exp domain): row / column maxima vs the dustbins -------------------------------------------------
// rowarg[b][i] = argmax_j P[i][:], rowbeat = P[i][rowarg] > P[i][N];  colarg[b][j] = argmax_i P[:][j], colbeat = P[colarg][j] > P[M][j].
__global__ __launch_bounds__(256) void k_top1_stats(const float* __restrict__ logS, int M, int N, int32_t* __restrict__ rowarg,
                                                    uint8_t* __restrict__ rowbeat, int32_t* __restrict__ colarg, uint8_t* __restrict__ colbeat) {
  // grid (B, slices): few large problems (the node-level matrix of a pair, B = 1..P) are spread over `slices` workgroups each
  // (one workgroup scanning a 351 x 332 matrix twice took 85-965 us); many small ones (patch matrices) use one workgroup each
  const int b = blockIdx.x, slice = blockIdx.y, nslices = gridDim.y;
  const int M1 = M + 1, N1 = N + 1;
  const float* s = logS + static_cast<int64_t>(b) * M1 * N1;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave index in an SGPR
  // The reference takes exp of the whole matrix and then the arg-max (local_global_registration.py:222, superpoint_matching.py:137): the
  // winner is the largest EXP value, the lowest index among equal ones.  exp is evaluated here for the CANDIDATES only — the entries within
  // top1_floor() of the line's largest log (two logs further apart than 1e-5 relative cannot round to one exp value; below -80, where exp
  // underflows and its values get coarse, every entry is a candidate) — so the decision is taken on the same exp values as before
  // (129 expf per line -> typically 1: the kernel was 0.7 ms of a 16-pair call).
  for (int i = slice * 4 + w; i < M1; i += 4 * nslices) {
    float m = -INFINITY;
    for (int j = lane; j < N1; j += 64) m = fmaxf(m, s[i * N1 + j]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    const float thr = top1_floor(m);
    float best = -INFINITY;
    int bj = 0;
    for (int j = lane; j < N1; j += 64) {
      const float x = s[i * N1 + j];
      if (x >= thr) {
        const float p = expf(x);
        if (p > best) {
          best = p;
          bj = j;
        }
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const float ob = __shfl_xor(best, d);
      const int oj = __shfl_xor(bj, d);
      if (ob > best || (ob == best && oj < bj)) {
        best = ob;
        bj = oj;
      }
    }
    if (lane == 0) {
      rowarg[static_cast<int64_t>(b) * M1 + i] = bj;
      rowbeat[static_cast<int64_t>(b) * M1 + i] = best > expf(s[i * N1 + N]) ? 1 : 0;
    }
  }
  for (int j = slice * 256 + threadIdx.x; j < N1; j += 256 * nslices) {
    float m = -INFINITY;
    for (int i = 0; i < M1; ++i) m = fmaxf(m, s[i * N1 + j]);
    const float thr = top1_floor(m);
    float best = -INFINITY;
    int bi = 0;
    for (int i = 0; i < M1; ++i) {
      const float x = s[i * N1 + j];
      if (x >= thr) {
        const float p = expf(x);
        if (p > best) {
          best = p;
          bi = i;
        }
      }
    }
    colarg[static_cast<int64_t>(b) * N1 + j] = bi;
    colbeat[static_cast<int64_t>(b) * N1 + j] = best > expf(s[M * N1 + j]) ? 1 : 0;
  }
}

// The same for matrices of up to 192 x 192 (the 129 x 129 patch problems: 7 716 of them per 16-pair call), ONE pass over the matrix per
// phase for rows AND columns: wavefront w takes rows w, w + 4, ...; a lane holds three columns (lane, lane + 64, lane + 128) and carries their
// running maxima / candidates down its rows, the four wavefronts' column partials meet in LDS.  The generic kernel reads the matrix four times
// and walks every column serially in one thread (2 x 129 dependent steps): 0.85 ms of a 16-pair call (profiles/r06_pair16_one_worker_kernel_summary.md).
constexpr int T1S_MAX = 192;
__global__ __launch_bounds__(256) void k_top1_stats_small(const float* __restrict__ logS, int M, int N, int32_t* __restrict__ rowarg,
                                                          uint8_t* __restrict__ rowbeat, int32_t* __restrict__ colarg, uint8_t* __restrict__ colbeat) {
  __shared__ float s_rm[T1S_MAX];
  __shared__ float s_cv[4][T1S_MAX];
  __shared__ int s_ci[4][T1S_MAX];
  const int64_t b = blockIdx.x;
  const int M1 = M + 1, N1 = N + 1;
  const float* s = logS + b * M1 * N1;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float cm[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = w; i < M1; i += 4) {
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int j = lane + 64 * c;
      const float x = j < N1 ? s[i * N1 + j] : -INFINITY;
      m = fmaxf(m, x);
      cm[c] = fmaxf(cm[c], x);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if (lane == 0) s_rm[i] = m;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) s_cv[w][lane + 64 * c] = cm[c];
  __syncthreads();
  float cthr[3], cb[3] = {-INFINITY, -INFINITY, -INFINITY};
  int ci[3] = {0, 0, 0};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int j = lane + 64 * c;
    cthr[c] = top1_floor(fmaxf(fmaxf(s_cv[0][j], s_cv[1][j]), fmaxf(s_cv[2][j], s_cv[3][j])));
  }
  __syncthreads();                                       // s_cv is reused for the candidates below
  for (int i = w; i < M1; i += 4) {
    const float rthr = top1_floor(s_rm[i]);
    float best = -INFINITY;
    int bj = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                        // ascending j inside the lane, ascending i down the loop: first index among equal values
      const int j = lane + 64 * c;
      if (j < N1) {
        const float x = s[i * N1 + j];
        const bool rc = x >= rthr, cc = x >= cthr[c];
        if (rc || cc) {
          const float pv = expf(x);
          if (rc && pv > best) {
            best = pv;
            bj = j;
          }
          if (cc && pv > cb[c]) {
            cb[c] = pv;
            ci[c] = i;
          }
        }
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const float ob = __shfl_xor(best, d);
      const int oj = __shfl_xor(bj, d);
      if (ob > best || (ob == best && oj < bj)) {
        best = ob;
        bj = oj;
      }
    }
    if (lane == 0) {
      rowarg[b * M1 + i] = bj;
      rowbeat[b * M1 + i] = best > expf(s[i * N1 + N]) ? 1 : 0;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    s_cv[w][lane + 64 * c] = cb[c];
    s_ci[w][lane + 64 * c] = ci[c];
  }
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int j = lane + 64 * c;
      if (j < N1) {
        float best = s_cv[0][j];
        int bi = s_ci[0][j];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
          const float ob = s_cv[q][j];
          const int oi = s_ci[q][j];
          if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
          }
        }
        colarg[b * N1 + j] = bi;
        colbeat[b * N1 + j] = best > expf(s[M * N1 + j]) ? 1 : 0;
      }
    }
  }
}

// count / emit the (i, j) pairs of every row in row-major order: (rowarg hit) OR — AND with `mutual` — (column hits with colarg == i), i < M, j < N,
// optionally gated by validity masks.  PHASE 0 = count per (b, i); PHASE 1 = write at the scanned offsets.
template <int PHASE>
__global__ __launch_bounds__(256) void k_top1_emit(const float* __restrict__ logS, int64_t B, int M, int N, const int32_t* __restrict__ rowarg,
                                                   const uint8_t* __restrict__ rowbeat, const int32_t* __restrict__ colarg,
                                                   const uint8_t* __restrict__ colbeat, const uint8_t* __restrict__ row_mask,
                                                   const uint8_t* __restrict__ col_mask, int32_t* __restrict__ counts,
                                                   const int32_t* __restrict__ offsets, int32_t* __restrict__ out_bij, float* __restrict__ out_score,
                                                   int mutual) {
  const int M1 = M + 1, N1 = N + 1;
  const int64_t rows = B * M;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < rows; t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t b = t / M;
    const int i = static_cast<int>(t - b * M);
    int c = 0;
    const bool rvalid = !row_mask || row_mask[b * M + i];
    if (rvalid) {
      const int ra = rowarg[b * M1 + i];
      const bool rb = rowbeat[b * M1 + i] != 0;
      const int64_t o = PHASE ? offsets[t] : 0;
      for (int j = 0; j < N; ++j) {
        if (col_mask && !col_mask[b * N + j]) continue;
        const bool from_row = rb && ra == j, from_col = colbeat[b * N1 + j] && colarg[b * N1 + j] == i;
        const bool hit = mutual ? (from_row && from_col) : (from_row || from_col);      // local_global_registration.py:84-87
        if (hit) {
          if (PHASE) {
            out_bij[3 * (o + c) + 0] = static_cast<int32_t>(b);
            out_bij[3 * (o + c) + 1] = i;
            out_bij[3 * (o + c) + 2] = j;
            out_score[o + c] = expf(logS[(b * M1 + i) * N1 + j]);
          }
          ++c;
        }
      }
    }
    if (!PHASE) counts[t] = c;
  }
}

// ---- dustbin top-K matching, K > 1 (LocalGlobalRegistration(k=K), local_global_registration.py:56-82; the shipped configuration has K = 1) ----
// A pair (i, j) is kept from the row side if P[i][j] is among the K largest of row i (over the N + 1 columns, dustbin included) and beats the
// row's dustbin P[i][N]; from the column side likewise.  "Among the K largest" in the order (value descending, index ascending) — torch.topk
// leaves the order of equal values open — so the row keeps the K-th element (value, index) and membership is one comparison.
// dust = 0 (LocalGlobalRegistration(use_dustbin=False), :62-65 / :74-77 / LCRNet.py:256-257): the dustbin row and column are stripped before the
// selection — the K largest are taken over the M x N interior only (Mr = M rows, Nr = N columns take part).
__global__ __launch_bounds__(256) void k_topk_stats(const float* __restrict__ logS, int M, int N, int K, int dust, float* __restrict__ rowv,
                                                    int32_t* __restrict__ rowj, float* __restrict__ colv, int32_t* __restrict__ coli) {
  const int b = blockIdx.x, slice = blockIdx.y, nslices = gridDim.y;
  const int M1 = M + 1, N1 = N + 1;
  const int Mr = dust ? M1 : M, Nr = dust ? N1 : N;
  const float* s = logS + static_cast<int64_t>(b) * M1 * N1;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = slice * 4 + w; i < Mr; i += 4 * nslices) {
    float pv = INFINITY;                                     // the previous pick: everything is "after" (+inf, -1)
    int pj = -1;
    bool exhausted = false;
    for (int t = 0; t < K; ++t) {
      float best = -INFINITY;
      int bj = 0x7fffffff;
      for (int j = lane; j < Nr; j += 64) {
        const float p = expf(s[i * N1 + j]);
        const bool after = p < pv || (p == pv && j > pj);
        if (after && (p > best || (p == best && j < bj))) {
          best = p;
          bj = j;
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const float ob = __shfl_xor(best, d);
        const int oj = __shfl_xor(bj, d);
        if (ob > best || (ob == best && oj < bj)) {
          best = ob;
          bj = oj;
        }
      }
      if (bj == 0x7fffffff) {                                // fewer than K entries: the whole row is in the set
        exhausted = true;
        break;
      }
      pv = best;
      pj = bj;
    }
    if (lane == 0) {
      rowv[static_cast<int64_t>(b) * M1 + i] = exhausted ? -INFINITY : pv;
      rowj[static_cast<int64_t>(b) * M1 + i] = exhausted ? 0x7fffffff : pj;
    }
  }
  for (int j = slice * 256 + threadIdx.x; j < Nr; j += 256 * nslices) {
    float pv = INFINITY;
    int pi = -1;
    bool exhausted = false;
    for (int t = 0; t < K; ++t) {
      float best = -INFINITY;
      int bi = 0x7fffffff;
      for (int i = 0; i < Mr; ++i) {
        const float p = expf(s[i * N1 + j]);
        const bool after = p < pv || (p == pv && i > pi);
        if (after && (p > best || (p == best && i < bi))) {
          best = p;
          bi = i;
        }
      }
      if (bi == 0x7fffffff) {
        exhausted = true;
        break;
      }
      pv = best;
      pi = bi;
    }
    colv[static_cast<int64_t>(b) * N1 + j] = exhausted ? -INFINITY : pv;
    coli[static_cast<int64_t>(b) * N1 + j] = exhausted ? 0x7fffffff : pi;
  }
}

template <int PHASE>
__global__ __launch_bounds__(256) void k_topk_emit(const float* __restrict__ logS, int64_t B, int M, int N, const float* __restrict__ rowv,
                                                   const int32_t* __restrict__ rowj, const float* __restrict__ colv, const int32_t* __restrict__ coli,
                                                   const uint8_t* __restrict__ row_mask, const uint8_t* __restrict__ col_mask, int32_t* __restrict__ counts,
                                                   const int32_t* __restrict__ offsets, int32_t* __restrict__ out_bij, float* __restrict__ out_score,
                                                   int mutual, int dust, float thr, const float* __restrict__ gscore) {
  const int M1 = M + 1, N1 = N + 1;
  const int64_t rows = B * M;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < rows; t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t b = t / M;
    const int i = static_cast<int>(t - b * M);
    int c = 0;
    if (!row_mask || row_mask[b * M + i]) {
      const float* srow = logS + (b * M1 + i) * N1;
      const float rv = rowv[b * M1 + i], rdust = expf(srow[N]);
      const float gs = gscore ? gscore[b] : 1.f;               // use_global_score: the patch pair's node-level score (:236-237)
      const int rj = rowj[b * M1 + i];
      const int64_t o = PHASE ? offsets[t] : 0;
      for (int j = 0; j < N; ++j) {
        if (col_mask && !col_mask[b * N + j]) continue;
        const float p = expf(srow[j]);
        const float cv = colv[b * N1 + j];
        const bool top_row = p > rv || (p == rv && j <= rj), top_col = p > cv || (p == cv && i <= coli[b * N1 + j]);
        // dustbin form: a selected entry must beat its row's / column's dustbin.  Without the dustbin the reference scatters the selected
        // values into a ZERO matrix and compares that with confidence_threshold (:61-65): an unselected entry counts as 0 (> a negative threshold)
        const bool from_row = dust ? (top_row && p > rdust) : ((top_row ? p : 0.f) > thr);
        const bool from_col = dust ? (top_col && p > expf(logS[(b * M1 + M) * N1 + j])) : ((top_col ? p : 0.f) > thr);
        if (mutual ? (from_row && from_col) : (from_row || from_col)) {
          if (PHASE) {
            out_bij[3 * (o + c) + 0] = static_cast<int32_t>(b);
            out_bij[3 * (o + c) + 1] = i;
            out_bij[3 * (o + c) + 2] = j;
            out_score[o + c] = p * gs;
          }
          ++c;
        }
      }
    }
    if (!PHASE) counts[t] = c;
  }
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

// ---- weighted Procrustes (batched): rotation_from_H in rigid3.h ------------------------------------------------------------

// problem p uses correspondences [start[p], start[p+1]) of src/ref/w; one wavefront per problem; T out [P,4,4] row-major
__global__ __launch_bounds__(64) void k_procrustes(const float* __restrict__ src, const float* __restrict__ ref, const float* __restrict__ w,
                                                   const int32_t* __restrict__ start, float eps, float* __restrict__ T) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int a = start[p], b = start[p + 1];
  double ws = 0;
  for (int i = a + lane; i < b; i += 64) ws += fmaxf(w[i], 0.f);
  ws = wave_sum(ws);
  const double inv = 1.0 / (ws + static_cast<double>(eps));
  double sc[3] = {0, 0, 0}, rc[3] = {0, 0, 0};
  for (int i = a + lane; i < b; i += 64) {
    const double wi = fmaxf(w[i], 0.f) * inv;
    for (int d = 0; d < 3; ++d) {
      sc[d] += wi * src[3 * i + d];
      rc[d] += wi * ref[3 * i + d];
    }
  }
  for (int d = 0; d < 3; ++d) {
    sc[d] = wave_sum(sc[d]);
    rc[d] = wave_sum(rc[d]);
  }
  double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int i = a + lane; i < b; i += 64) {
    const double wi = fmaxf(w[i], 0.f) * inv;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) H[r][c] += (src[3 * i + r] - sc[r]) * wi * (ref[3 * i + c] - rc[c]);
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) H[r][c] = wave_sum(H[r][c]);
  if (lane == 0) {
    double R[3][3];
    rotation_from_H(H, R);
    float* t = T + 16 * p;
    for (int r = 0; r < 3; ++r) {
      double tr = rc[r];
      for (int c = 0; c < 3; ++c) {
        t[4 * r + c] = static_cast<float>(R[r][c]);
        tr -= R[r][c] * sc[c];
      }
      t[4 * r + 3] = static_cast<float>(tr);
    }
    t[12] = t[13] = t[14] = 0.f;
    t[15] = 1.f;
  }
}

// inlier counts of every hypothesis over all correspondences; one workgroup per hypothesis
__global__ __launch_bounds__(256) void k_inlier_count(const float* __restrict__ T, const float* __restrict__ src, const float* __restrict__ ref, int n,
                                                      float radius, const int32_t* __restrict__ start, int min_count, int32_t* __restrict__ counts) {
  __shared__ int s_c;
  if (start && start[blockIdx.x + 1] - start[blockIdx.x] < min_count) {   // hypothesis from too few correspondences: never the best
    if (threadIdx.x == 0) counts[blockIdx.x] = -1;
    return;
  }
  const float* t = T + 16 * blockIdx.x;
  if (threadIdx.x == 0) s_c = 0;
  __syncthreads();
  int c = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
    const float dx = ref[3 * i] - (t[0] * x + t[1] * y + t[2] * z + t[3]);
    const float dy = ref[3 * i + 1] - (t[4] * x + t[5] * y + t[6] * z + t[7]);
    const float dz = ref[3 * i + 2] - (t[8] * x + t[9] * y + t[10] * z + t[11]);
    c += sqrtf(dx * dx + dy * dy + dz * dz) < radius ? 1 : 0;
  }
  atomicAdd(&s_c, c);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_c;
}

// w_out = score * [ |ref - T src| < radius ] with T = T_all[sel ? *sel : 0]
__global__ __launch_bounds__(256) void k_inlier_weights(const float* __restrict__ T_all, const int32_t* __restrict__ sel, const float* __restrict__ src,
                                                        const float* __restrict__ ref, const float* __restrict__ score, int n, float radius,
                                                        float* __restrict__ w_out) {
  const float* t = T_all + 16 * (sel ? sel[0] : 0);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
    const float dx = ref[3 * i] - (t[0] * x + t[1] * y + t[2] * z + t[3]);
    const float dy = ref[3 * i + 1] - (t[4] * x + t[5] * y + t[6] * z + t[7]);
    const float dz = ref[3 * i + 2] - (t[8] * x + t[9] * y + t[10] * z + t[11]);
    w_out[i] = sqrtf(dx * dx + dy * dy + dz * dz) < radius ? score[i] : 0.f;
  }
}

// first index of the maximum (torch.argmax on equal values returns the first)
__global__ void k_argmax_i32(const int32_t* __restrict__ v, int n, int32_t* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int best = 0;
    for (int i = 1; i < n; ++i)
      if (v[i] > v[best]) best = i;
    out[0] = best;
  }
}

// ---- local-to-global registration of S pairs in one launch sequence --------------------------------------------------------
// Correspondences of all pairs are stacked pair-major (inside a pair: patch-major, as top-1 matching emits them); hypothesis h is the
// weighted Procrustes fit of chunk [hyp_start[h], hyp_start[h+1]); pair s owns hypotheses [seg_hyp_start[s], seg_hyp_start[s+1]) and
// the rows they cover.  The same arithmetic as the single-pair kernels above, with every "over all correspondences" restricted to
// the hypothesis's own pair.
__global__ void k_lgr_seg_rows(const int32_t* __restrict__ hyp_start, const int32_t* __restrict__ seg_hyp_start, int S, int32_t* __restrict__ seg_row_start) {
  for (int s = threadIdx.x; s <= S; s += blockDim.x) seg_row_start[s] = hyp_start[seg_hyp_start[s]];
}

__global__ __launch_bounds__(256) void k_inlier_count_seg(const float* __restrict__ T, const float* __restrict__ src, const float* __restrict__ ref,
                                                          float radius, const int32_t* __restrict__ hyp_start, const int32_t* __restrict__ seg_hyp_start,
                                                          const int32_t* __restrict__ seg_row_start, int S, int min_count, int32_t* __restrict__ counts,
                                                          const uint8_t* __restrict__ ver_mask) {
  __shared__ int s_c, s_lo, s_hi;
  const int h = blockIdx.x;
  if (hyp_start[h + 1] - hyp_start[h] < min_count) {       // hypothesis from too few correspondences: never the best
    if (threadIdx.x == 0) counts[h] = -1;
    return;
  }
  if (threadIdx.x == 0) {
    int sg = 0;
    while (sg + 1 < S && h >= seg_hyp_start[sg + 1]) ++sg;
    s_lo = seg_row_start[sg];
    s_hi = seg_row_start[sg + 1];
    s_c = 0;
  }
  __syncthreads();
  const float* t = T + 16 * h;
  int c = 0;
  for (int i = s_lo + threadIdx.x; i < s_hi; i += 256) {
    const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
    const float dx = ref[3 * i] - (t[0] * x + t[1] * y + t[2] * z + t[3]);
    const float dy = ref[3 * i + 1] - (t[4] * x + t[5] * y + t[6] * z + t[7]);
    const float dz = ref[3 * i + 2] - (t[8] * x + t[9] * y + t[10] * z + t[11]);
    c += (sqrtf(dx * dx + dy * dy + dz * dz) < radius && (!ver_mask || ver_mask[i])) ? 1 : 0;     // rows of the verification set only
  }
  atomicAdd(&s_c, c);
  __syncthreads();
  if (threadIdx.x == 0) counts[h] = s_c;
}

// correspondence_limit (local_global_registration.py:152-160): the VERIFICATION set of a pair = its `limit` highest-scoring correspondences
// (all of them when it has no more than that); hypotheses still come from all correspondences, inlier counting and the refinement use the
// verification set only.  One workgroup per pair: 4-pass radix select of the limit-th largest score, ties at the threshold admitted in index
// order (torch.topk leaves that open).  Writes ver_mask[i] and score_ver[i] = mask ? score : 0 — a zero weight takes a row out of every
// weighted Procrustes sum exactly, so the set never has to be compacted.
__global__ __launch_bounds__(256) void k_lgr_topl(const float* __restrict__ score, const int32_t* __restrict__ seg_row_start, int limit,
                                                  uint8_t* __restrict__ ver_mask, float* __restrict__ score_ver) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_prefix, s_need, s_base;
  __shared__ uint8_t s_flag[256];
  const int lo = seg_row_start[blockIdx.x], hi = seg_row_start[blockIdx.x + 1];
  const int n = hi - lo, tid = threadIdx.x;
  if (n <= limit) {
    for (int i = lo + tid; i < hi; i += 256) {
      ver_mask[i] = 1;
      score_ver[i] = score[i];
    }
    return;
  }
  auto key_of = [&](int i) {                                  // order-preserving map of a float onto unsigned
    const unsigned u = __float_as_uint(score[i]);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  };
  if (tid == 0) {
    s_prefix = 0;
    s_need = static_cast<unsigned>(limit);
  }
  __syncthreads();
  for (int shift = 24; shift >= 0; shift -= 8) {
    s_hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix, hmask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    for (int i = lo + tid; i < hi; i += 256) {
      const unsigned k = key_of(i);
      if ((k & hmask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned need = s_need, acc = 0;
      int bin = 255;
      for (; bin > 0; --bin) {                                // from the largest digit down: the bin holding the need-th largest key
        if (acc + s_hist[bin] >= need) break;
        acc += s_hist[bin];
      }
      s_need = need - acc;
      s_prefix = prefix | (static_cast<unsigned>(bin) << shift);
    }
    __syncthreads();
  }
  const unsigned thr = s_prefix;                              // the limit-th largest key; s_need of the keys EQUAL to it are admitted
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int c0 = lo; c0 < hi; c0 += 256) {
    const int i = c0 + tid;
    const unsigned k = i < hi ? key_of(i) : 0u;
    const bool eq = i < hi && k == thr;
    s_flag[tid] = eq ? 1 : 0;
    __syncthreads();
    unsigned rank = s_base;
    for (int t = 0; t < tid; ++t) rank += s_flag[t];
    const bool in = i < hi && (k > thr || (eq && rank < s_need));
    if (i < hi) {
      ver_mask[i] = in ? 1 : 0;
      score_ver[i] = in ? score[i] : 0.f;
    }
    __syncthreads();
    if (tid == 255) s_base = rank + s_flag[255];
    __syncthreads();
  }
}

// per pair: the first hypothesis with the most inliers (torch.argmax order), or — when no chunk of the pair reached min_count
// correspondences (local_global_registration.py:186-190) — the fit over all of the pair's correspondences
__global__ void k_lgr_select(const float* __restrict__ hyp, const int32_t* __restrict__ counts, const int32_t* __restrict__ seg_hyp_start,
                             const float* __restrict__ T_all_rows, float* __restrict__ T_sel, int32_t* __restrict__ best_out) {
  const int s = blockIdx.x;
  __shared__ int s_best;
  if (threadIdx.x == 0) {
    int best = -1, bc = -1;
    for (int h = seg_hyp_start[s]; h < seg_hyp_start[s + 1]; ++h)
      if (counts[h] > bc) {
        bc = counts[h];
        best = h;
      }
    s_best = bc >= 0 ? best : -1;
    if (best_out) best_out[s] = s_best;
  }
  __syncthreads();
  const float* from = s_best >= 0 ? hyp + 16 * s_best : T_all_rows + 16 * s;
  if (threadIdx.x < 16) T_sel[16 * s + threadIdx.x] = from[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_inlier_weights_seg(const float* __restrict__ T_seg, const int32_t* __restrict__ seg_row_start, int S,
                                                            const float* __restrict__ src, const float* __restrict__ ref,
                                                            const float* __restrict__ score, int n, float radius, float* __restrict__ w_out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    int sg = 0;
    while (sg + 1 < S && i >= seg_row_start[sg + 1]) ++sg;
    const float* t = T_seg + 16 * sg;
    const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
    const float dx = ref[3 * i] - (t[0] * x + t[1] * y + t[2] * z + t[3]);
    const float dy = ref[3 * i + 1] - (t[4] * x + t[5] * y + t[6] * z + t[7]);
    const float dz = ref[3 * i + 2] - (t[8] * x + t[9] * y + t[10] * z + t[11]);
    w_out[i] = sqrtf(dx * dx + dy * dy + dz * dz) < radius ? score[i] : 0.f;
  }
}

}  // namespace lcr

using namespace lcr;
#define ST(s) static_cast<hipStream_t>(s)
static int blocks_for(int64_t n, int per = 256, int cap = 4096) { return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, cap))); }

extern "C" int lcr_vote_shift(const float* xyz, const float* offsets, int64_t N, float max_range, float* out, void* stream) {
  if (!xyz || !offsets || !out || N < 0) return LCR_EARG;
  if (N) hipLaunchKernelGGL(k_vote_shift, dim3(blocks_for(N)), dim3(256), 0, ST(stream), xyz, offsets, N, max_range, out);
  return check_launch("lcr_vote_shift");
}

extern "C" int lcr_greedy_nms_ws_bytes(int64_t n_total, size_t* bytes) {
  if (!bytes || n_total < 0) return LCR_EARG;
  *bytes = align_up(static_cast<size_t>(n_total) + 16) + sizeof(int32_t) * static_cast<size_t>(n_total + 1) * (NMS_NB + 1);
  return LCR_OK;
}

extern "C" int lcr_greedy_nms(const float* pts, const int64_t* len, int B, int64_t n_total, float radius, uint8_t* keep, int64_t* out_len,
                              void* ws, void* stream) {
  if (!pts || !len || !keep || !out_len || !ws || B < 1) return LCR_EARG;
  int8_t* st = static_cast<int8_t*>(ws);
  int32_t* nbr = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + align_up(static_cast<size_t>(n_total) + 16));
  hipLaunchKernelGGL(k_greedy_nms, dim3(B), dim3(NMS_T), 0, ST(stream), pts, len, B, radius, keep, out_len, st, nbr);
  return check_launch("lcr_greedy_nms");
}

extern "C" int lcr_neighbor_mean(const float* pts, const void* idx, int idx_is_64, int64_t M, int H, int64_t pad, float* out, void* stream) {
  if (!pts || !idx || !out || M < 0 || H < 1) return LCR_EARG;
  if (M == 0) return LCR_OK;
  if (idx_is_64) hipLaunchKernelGGL((k_neighbor_mean<int64_t>), dim3(blocks_for(M)), dim3(256), 0, ST(stream), pts, static_cast<const int64_t*>(idx), M, H, pad, out);
  else hipLaunchKernelGGL((k_neighbor_mean<int32_t>), dim3(blocks_for(M)), dim3(256), 0, ST(stream), pts, static_cast<const int32_t*>(idx), M, H, pad, out);
  return check_launch("lcr_neighbor_mean");
}

extern "C" int lcr_point_to_node_ws_bytes(int64_t N, int M, size_t* bytes) {
  if (!bytes || N < 0 || M < 1) return LCR_EARG;
  Carver c(nullptr, ~size_t(0));
  c.take<int32_t>(N + 1);      // p2n
  c.take<int32_t>(M + 2);      // counts
  c.take<int32_t>(M + 2);      // starts
  c.take<int32_t>(M + 2);      // cursor
  c.take<int32_t>(N + 1);      // members
  c.take<char>(scan_ws_bytes(M + 2));
  *bytes = c.off;
  return LCR_OK;
}

// point_to_node_partition (pointcloud_partition.py:60-107): knn i64[M,K] (pad = N), knn_mask u8[M,K], node_mask u8[M], p2n i32[N]
extern "C" int lcr_point_to_node_partition(const float* points, int64_t N, const float* nodes, int M, int K, int32_t* p2n_out, int64_t* knn,
                                           uint8_t* knn_mask, uint8_t* node_mask, uint32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!points || !nodes || !knn || !knn_mask || !node_mask || !status || !ws || N < 1 || M < 1 || K < 1 || M > 4000) {
    set_error("lcr_point_to_node_partition: bad argument (1 <= M <= 4000)");
    return LCR_EARG;
  }
  size_t need = 0;
  lcr_point_to_node_ws_bytes(N, M, &need);
  if (need > ws_bytes) return LCR_ESPACE;
  Carver c(ws, ws_bytes);
  int32_t* p2n = c.take<int32_t>(N + 1);
  int32_t* cnt = c.take<int32_t>(M + 2);
  int32_t* start = c.take<int32_t>(M + 2);
  int32_t* cursor = c.take<int32_t>(M + 2);
  int32_t* members = c.take<int32_t>(N + 1);
  void* sws = c.take<char>(scan_ws_bytes(M + 2));
  hipStream_t st = ST(stream);
  hipMemsetAsync(cnt, 0, sizeof(int32_t) * (M + 2), st);
  hipMemsetAsync(cursor, 0, sizeof(int32_t) * (M + 2), st);
  hipLaunchKernelGGL(k_point_to_node, dim3(blocks_for(N, 256, 2048)), dim3(256), sizeof(float) * 4 * M, st, points, N, nodes, M, p2n, cnt);
  int rc = exclusive_scan_i32(cnt, start, M + 1, nullptr, sws, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_p2n_scatter, dim3(blocks_for(N)), dim3(256), 0, st, p2n, N, start, cursor, members);
  hipLaunchKernelGGL(k_node_topk, dim3(M), dim3(256), 0, st, points, N, nodes, start, members, K, knn, knn_mask, node_mask, status);
  if (p2n_out) hipMemcpyAsync(p2n_out, p2n, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, st);
  return check_launch("lcr_point_to_node_partition");
}

// point_to_node_partition of C stacked clouds (cloud c: points [point_off[c], point_off[c+1]), nodes [node_off[c], node_off[c+1]); host
// offsets): the per-cloud results stacked — p2n i32[N_total] and knn i64[M_total, K] hold indices LOCAL to the cloud, knn padded with the
// cloud's own point count.  Workspace: lcr_point_to_node_ws_bytes(N_total, M_total).
extern "C" int lcr_point_to_node_partition_stack(const float* points, const int64_t* point_off, const float* nodes, const int64_t* node_off, int C,
                                                 int K, int32_t* p2n_out, int64_t* knn, uint8_t* knn_mask, uint8_t* node_mask, uint32_t* status,
                                                 void* ws, size_t ws_bytes, void* stream) {
  if (!points || !point_off || !nodes || !node_off || !knn || !knn_mask || !node_mask || !status || !ws || C < 1 || C > P2N_MAX_CLOUDS || K < 1) {
    set_error("lcr_point_to_node_partition_stack: bad argument (1 <= clouds <= %d)", P2N_MAX_CLOUDS);
    return LCR_EARG;
  }
  P2nStack sk;
  sk.C = C;
  int64_t n_max = 0;
  int m_max = 0;
  for (int c = 0; c <= C; ++c) {
    if (c && (point_off[c] < point_off[c - 1] || node_off[c] < node_off[c - 1])) return LCR_EARG;
    sk.po[c] = point_off[c] - point_off[0];
    sk.mo[c] = static_cast<int32_t>(node_off[c] - node_off[0]);
    if (c) {
      n_max = std::max(n_max, sk.po[c] - sk.po[c - 1]);
      m_max = std::max(m_max, sk.mo[c] - sk.mo[c - 1]);
    }
  }
  const int64_t N = sk.po[C];
  const int M = sk.mo[C];
  if (N < 1 || M < 1 || m_max > 4000) {
    set_error("lcr_point_to_node_partition_stack: empty stack or more than 4000 nodes in a cloud");
    return LCR_EARG;
  }
  points += 3 * point_off[0];
  nodes += 3 * node_off[0];
  size_t need = 0;
  lcr_point_to_node_ws_bytes(N, M, &need);
  if (need > ws_bytes) return LCR_ESPACE;
  Carver cv(ws, ws_bytes);
  int32_t* p2n = cv.take<int32_t>(N + 1);
  int32_t* cnt = cv.take<int32_t>(M + 2);
  int32_t* start = cv.take<int32_t>(M + 2);
  int32_t* cursor = cv.take<int32_t>(M + 2);
  int32_t* members = cv.take<int32_t>(N + 1);
  void* sws = cv.take<char>(scan_ws_bytes(M + 2));
  hipStream_t st = ST(stream);
  hipMemsetAsync(cnt, 0, static_cast<size_t>(reinterpret_cast<char*>(cursor + M + 2) - reinterpret_cast<char*>(cnt)), st);   // counts .. cursor: one fill
  const int bx = blocks_for(n_max, 256, 2048);
  hipLaunchKernelGGL(k_point_to_node_stack, dim3(bx, C), dim3(256), sizeof(float) * 4 * m_max, st, points, nodes, sk, p2n, cnt);
  int rc = exclusive_scan_i32(cnt, start, M + 1, nullptr, sws, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_p2n_scatter_stack, dim3(blocks_for(n_max), C), dim3(256), 0, st, p2n, sk, start, cursor, members);
  hipLaunchKernelGGL(k_node_topk_stack, dim3(M), dim3(256), 0, st, points, nodes, sk, start, members, K, knn, knn_mask, node_mask, status);
  if (p2n_out) hipMemcpyAsync(p2n_out, p2n, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, st);
  return check_launch("lcr_point_to_node_partition_stack");
}

extern "C" int lcr_build_padded_scores(const float* raw, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N, float scale,
                                       const float* alpha, float inf_val, float* S, void* stream) {
  if (!raw || !row_mask || !col_mask || !alpha || !S || B < 1 || M < 1 || N < 1) return LCR_EARG;
  hipLaunchKernelGGL(k_build_padded_scores_rows, dim3(blocks_for(B * (M + 1) * 64, 256, 8192)), dim3(256), 0, ST(stream), raw, row_mask, col_mask, B, M,
                     N, scale, alpha, inf_val, S);
  return check_launch("lcr_build_padded_scores");
}

// in place on S [B, M+1, N+1]; uv_ws: B * (2 * (M + N + 2) + 1) floats
// Persistent form for matrices beyond LDS (see k_log_sinkhorn_coop): G row slabs of <= 144 KB; taken when the B * G workgroups (one CU
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
  if (G_out) *G_out = G;
  if (slab_out) *slab_out = (M1 + G - 1) / G;
  return true;
}
static size_t sk_coop_floats(int64_t B, int M, int N) {
  int G = 0, slab = 0;
  if (!sk_coop_plan(B, M, N, &G, &slab)) return 0;
  return static_cast<size_t>(4) * B * G * (N + 1) + B + 8;
}
extern "C" int lcr_log_sinkhorn_ws_floats(int64_t B, int M, int N, size_t* floats) {
  if (!floats || B < 1 || M < 1 || N < 1) return LCR_EARG;
  *floats = std::max(static_cast<size_t>(B) * (2 * (static_cast<size_t>(M) + N + 2) + 1), sk_coop_floats(B, M, N)) + 1;   // + the status word (last)
  return LCR_OK;
}
// must mirror the dispatch of lcr_log_sinkhorn_ex below (with a workspace of lcr_log_sinkhorn_ws_floats floats)
extern "C" int lcr_log_sinkhorn_form(int64_t B, int M, int N, int* form) {
  if (!form || B < 1 || M < 1 || N < 1) return LCR_EARG;
  const size_t mat_bytes = sizeof(float) * (static_cast<size_t>(M + 1) * (N + 1) + 2 * (M + N + 2));
  if (M + 1 <= SKR_LINES && N + 1 <= SKR_LINES) *form = 0;
  else if (mat_bytes <= 150 * 1024) *form = 1;
  else if (sk_coop_plan(B, M, N, nullptr, nullptr)) *form = 2;
  else *form = 3;
  return LCR_OK;
}
extern "C" int lcr_log_sinkhorn_ex(float* S, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N, int iters, float inf_val,
                                   float* uv_ws, size_t uv_floats, void* stream);
extern "C" int lcr_log_sinkhorn(float* S, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N, int iters, float inf_val,
                                float* uv_ws, void* stream) {
  return lcr_log_sinkhorn_ex(S, row_mask, col_mask, B, M, N, iters, inf_val, uv_ws, static_cast<size_t>(B) * (2 * (static_cast<size_t>(M) + N + 2) + 1), stream);
}
extern "C" int lcr_log_sinkhorn_ex(float* S, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N, int iters, float inf_val,
                                   float* uv_ws, size_t uv_floats, void* stream) {
  if (!S || !row_mask || !col_mask || !uv_ws || B < 1 || M < 1 || N < 1 || iters < 0) return LCR_EARG;
  const size_t mat_bytes = sizeof(float) * (static_cast<size_t>(M + 1) * (N + 1) + 2 * (M + N + 2));   // matrix + u, v, log_mu, log_nu
  int form_id = 3;
  lcr_log_sinkhorn_form(B, M, N, &form_id);
  KernelTimerScope timed(KT_SINKHORN, ST(stream), B, M, N, iters, form_id);      // brackets every launch of the call (bench.py's pair block)
  if (M + 1 <= SKR_LINES && N + 1 <= SKR_LINES) {
    static const bool scaled_on = !(getenv("LCR_SINKHORN_SCALED") && atoi(getenv("LCR_SINKHORN_SCALED")) == 0);
    const bool scaled = scaled_on && M + 1 <= SKS_MAIN + 1 && N + 1 <= SKS_MAIN + 1;
    unsigned* redo = scaled ? reinterpret_cast<unsigned*>(uv_ws) : nullptr;      // B words of the workspace: problems handed back
    if (scaled) {
      const size_t lds = sizeof(float) * static_cast<size_t>(M + 1) * (N + 1);
      static DynLds opt_in;                              // up to 132 x 132 floats of dynamic LDS beside the static vectors
      if (opt_in.need(reinterpret_cast<const void*>(&k_sinkhorn_scaled), sizeof(float) * SKR_LINES * SKR_LINES) != hipSuccess) {
        set_error("lcr_log_sinkhorn: cannot reserve dynamic LDS for the scaled-domain kernel");
        return LCR_EHIP;
      }
      hipLaunchKernelGGL(k_sinkhorn_scaled, dim3(static_cast<int>(B)), dim3(SKR_T), lds, ST(stream), S, row_mask, col_mask, M, N, iters, inf_val, redo);
    }
    hipLaunchKernelGGL(k_log_sinkhorn_reg, dim3(static_cast<int>(B)), dim3(SKR_T), 0, ST(stream), S, row_mask, col_mask, M, N, iters, inf_val, redo);
  } else if (mat_bytes <= 150 * 1024) {
    static DynLds opt_in;                                // > 64 KB of dynamic LDS needs an explicit opt-in
    if (opt_in.need(reinterpret_cast<const void*>(&k_log_sinkhorn_lds), 150 * 1024) != hipSuccess) {
      set_error("lcr_log_sinkhorn: cannot reserve dynamic LDS for the LDS-resident kernel");
      return LCR_EHIP;
    }
    hipLaunchKernelGGL(k_log_sinkhorn_lds, dim3(static_cast<int>(B)), dim3(SK_T), mat_bytes, ST(stream), S, row_mask, col_mask, M, N, iters, inf_val,
                       uv_ws);
  } else if (sk_coop_plan(B, M, N, nullptr, nullptr) && uv_floats >= sk_coop_floats(B, M, N) + 1) {
    int G = 0, slab = 0;
    sk_coop_plan(B, M, N, &G, &slab);
    const int M1 = M + 1, N1 = N + 1;
    SkCoop c;
    c.part = uv_ws;
    c.counter = reinterpret_cast<unsigned*>(uv_ws + static_cast<size_t>(4) * B * G * N1);
    c.status = reinterpret_cast<unsigned*>(uv_ws + uv_floats - 1);      // the LAST word of the workspace (the caller reads it)
    c.G = G;
    c.slab = slab;
    c.nsub = std::min(4, SKC_T / N1);
    const size_t lds = sizeof(float) * (static_cast<size_t>(slab) * N1 + 2 * (M1 + N1) + 2 * static_cast<size_t>(c.nsub) * N1);
    static DynLds opt_in;
    if (opt_in.need(reinterpret_cast<const void*>(&k_log_sinkhorn_coop), lds) != hipSuccess) {
      set_error("lcr_log_sinkhorn: cannot reserve %zu B of dynamic LDS for the persistent kernel", lds);
      return LCR_EHIP;
    }
    hipLaunchKernelGGL(k_sk_coop_init, dim3(1), dim3(64), 0, ST(stream), c.counter, c.status, static_cast<int>(B));
    hipLaunchKernelGGL(k_log_sinkhorn_coop, dim3(static_cast<int>(B) * G), dim3(SKC_T), lds, ST(stream), S, row_mask, col_mask, M, N, iters, inf_val, c);
  } else {
    if (B > 65535) return LCR_EARG;
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
  return check_launch("lcr_log_sinkhorn");
}

extern "C" int lcr_top1_matching_ws_bytes(int64_t B, int M, int N, size_t* bytes) {
  if (!bytes || B < 1 || M < 1 || N < 1) return LCR_EARG;
  Carver c(nullptr, ~size_t(0));
  c.take<int32_t>(B * (M + 1));
  c.take<uint8_t>(B * (M + 1));
  c.take<int32_t>(B * (N + 1));
  c.take<uint8_t>(B * (N + 1));
  c.take<int32_t>(B * M + 1);
  c.take<int32_t>(B * M + 1);
  c.take<char>(scan_ws_bytes(B * M + 1));
  *bytes = c.off;
  return LCR_OK;
}

// Two-phase: out_bij == NULL -> only *total (device i64) is produced (and the per-row offsets kept in ws);
// then call again with buffers of `total` entries.  (b,i,j) triplets in row-major order; scores in the exp domain.
extern "C" int lcr_top1_matching(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int64_t* total,
                                 int32_t* out_bij, float* out_score, void* ws, size_t ws_bytes, void* stream) {
  return lcr_top1_matching_ex(logS, B, M, N, row_mask, col_mask, 0, total, out_bij, out_score, ws, ws_bytes, stream);
}

// mutual != 0: a pair is kept only if it is BOTH its row's and its column's dustbin-beating maximum (LocalGlobalRegistration(mutual=True),
// local_global_registration.py:84-85); 0: either (the shipped configuration)
extern "C" int lcr_top1_matching_ex(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int mutual,
                                    int64_t* total, int32_t* out_bij, float* out_score, void* ws, size_t ws_bytes, void* stream) {
  if (!logS || !ws || B < 1 || M < 1 || N < 1 || (!out_bij && !total)) return LCR_EARG;
  size_t need = 0;
  lcr_top1_matching_ws_bytes(B, M, N, &need);
  if (need > ws_bytes) return LCR_ESPACE;
  Carver c(ws, ws_bytes);
  int32_t* rowarg = c.take<int32_t>(B * (M + 1));
  uint8_t* rowbeat = c.take<uint8_t>(B * (M + 1));
  int32_t* colarg = c.take<int32_t>(B * (N + 1));
  uint8_t* colbeat = c.take<uint8_t>(B * (N + 1));
  int32_t* counts = c.take<int32_t>(B * M + 1);
  int32_t* offsets = c.take<int32_t>(B * M + 1);
  void* sws = c.take<char>(scan_ws_bytes(B * M + 1));
  hipStream_t st = ST(stream);
  if (!out_bij) {
    const int slices = B >= 64 ? 1 : std::max(1, std::min(32, (M + 1 + 15) / 16));
    if (M + 1 <= T1S_MAX && N + 1 <= T1S_MAX)
      hipLaunchKernelGGL(k_top1_stats_small, dim3(static_cast<int>(B)), dim3(256), 0, st, logS, M, N, rowarg, rowbeat, colarg, colbeat);
    else
      hipLaunchKernelGGL(k_top1_stats, dim3(static_cast<int>(B), slices), dim3(256), 0, st, logS, M, N, rowarg, rowbeat, colarg, colbeat);
    hipLaunchKernelGGL((k_top1_emit<0>), dim3(blocks_for(B * M)), dim3(256), 0, st, logS, B, M, N, rowarg, rowbeat, colarg, colbeat, row_mask, col_mask,
                       counts, offsets, out_bij, out_score, mutual);
    hipMemsetAsync(counts + B * M, 0, sizeof(int32_t), st);
    int rc = exclusive_scan_i32(counts, offsets, B * M + 1, total, sws, st);
    if (rc) return rc;
  } else {
    hipLaunchKernelGGL((k_top1_emit<1>), dim3(blocks_for(B * M)), dim3(256), 0, st, logS, B, M, N, rowarg, rowbeat, colarg, colbeat, row_mask, col_mask,
                       counts, offsets, out_bij, out_score, mutual);
  }
  return check_launch("lcr_top1_matching");
}

extern "C" int lcr_topk_matching_ws_bytes(int64_t B, int M, int N, size_t* bytes) {
  if (!bytes || B < 1 || M < 1 || N < 1) return LCR_EARG;
  Carver c(nullptr, ~size_t(0));
  c.take<float>(B * (M + 1));
  c.take<int32_t>(B * (M + 1));
  c.take<float>(B * (N + 1));
  c.take<int32_t>(B * (N + 1));
  c.take<int32_t>(B * M + 1);
  c.take<int32_t>(B * M + 1);
  c.take<char>(scan_ws_bytes(B * M + 1));
  *bytes = c.off;
  return LCR_OK;
}

// dustbin top-K matching (K >= 1), two-phase like lcr_top1_matching; for K = 1 the rows equal lcr_top1_matching_ex's
extern "C" int lcr_topk_matching(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int K, int mutual,
                                 int64_t* total, int32_t* out_bij, float* out_score, void* ws, size_t ws_bytes, void* stream) {
  return lcr_topk_matching_ex(logS, B, M, N, row_mask, col_mask, K, mutual, 1, 0.f, nullptr, total, out_bij, out_score, ws, ws_bytes, stream);
}

// every switch of LocalGlobalRegistration.compute_correspondence_matrix (local_global_registration.py:48-93) + use_global_score (:236-237):
// use_dustbin = 0 takes the K largest over the M x N interior and keeps what exceeds confidence_threshold; global_scores [B] (or NULL)
// multiplies the emitted scores of patch pair b
extern "C" int lcr_topk_matching_ex(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int K, int mutual,
                                    int use_dustbin, float confidence_threshold, const float* global_scores, int64_t* total, int32_t* out_bij,
                                    float* out_score, void* ws, size_t ws_bytes, void* stream) {
  if (!logS || !ws || B < 1 || M < 1 || N < 1 || K < 1 || (!out_bij && !total)) return LCR_EARG;
  size_t need = 0;
  lcr_topk_matching_ws_bytes(B, M, N, &need);
  if (need > ws_bytes) return LCR_ESPACE;
  Carver c(ws, ws_bytes);
  float* rowv = c.take<float>(B * (M + 1));
  int32_t* rowj = c.take<int32_t>(B * (M + 1));
  float* colv = c.take<float>(B * (N + 1));
  int32_t* coli = c.take<int32_t>(B * (N + 1));
  int32_t* counts = c.take<int32_t>(B * M + 1);
  int32_t* offsets = c.take<int32_t>(B * M + 1);
  void* sws = c.take<char>(scan_ws_bytes(B * M + 1));
  hipStream_t st = ST(stream);
  const int dust = use_dustbin ? 1 : 0;
  if (!out_bij) {
    const int slices = B >= 64 ? 1 : std::max(1, std::min(32, (M + 1 + 15) / 16));
    hipLaunchKernelGGL(k_topk_stats, dim3(static_cast<int>(B), slices), dim3(256), 0, st, logS, M, N, K, dust, rowv, rowj, colv, coli);
    hipLaunchKernelGGL((k_topk_emit<0>), dim3(blocks_for(B * M)), dim3(256), 0, st, logS, B, M, N, rowv, rowj, colv, coli, row_mask, col_mask, counts,
                       offsets, out_bij, out_score, mutual, dust, confidence_threshold, global_scores);
    hipMemsetAsync(counts + B * M, 0, sizeof(int32_t), st);
    int rc = exclusive_scan_i32(counts, offsets, B * M + 1, total, sws, st);
    if (rc) return rc;
  } else {
    hipLaunchKernelGGL((k_topk_emit<1>), dim3(blocks_for(B * M)), dim3(256), 0, st, logS, B, M, N, rowv, rowj, colv, coli, row_mask, col_mask, counts,
                       offsets, out_bij, out_score, mutual, dust, confidence_threshold, global_scores);
  }
  return check_launch("lcr_topk_matching");
}

extern "C" int lcr_upsample_concat(const float* x, int64_t Nx, int C1, const void* idx, int idx_is_64, int H, const float* skip, int C2, int64_t N,
                                   float* out, void* stream) {
  if (N == 0) return LCR_OK;
  if (!x || !idx || !skip || !out || N < 0 || C1 < 1 || C2 < 1 || H < 1) return LCR_EARG;
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
  if (!src || !idx || !out || R < 0 || C < 1) return LCR_EARG;
  if (C % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
    hipLaunchKernelGGL(k_gather_rows_vec, dim3(blocks_for(R * 64, 256, 8192)), dim3(256), 0, ST(stream), src, pad, C, idx, R, out);
    return check_launch("lcr_gather_rows");
  }
  hipLaunchKernelGGL(k_gather_rows, dim3(blocks_for(R * C, 256, 8192)), dim3(256), 0, ST(stream), src, pad, C, idx, R, out);
  return check_launch("lcr_gather_rows");
}

extern "C" int lcr_procrustes_batched(const float* src, const float* ref, const float* w, const int32_t* start, int P, float eps, float* T, void* stream) {
  if (!src || !ref || !w || !start || !T || P < 1) return LCR_EARG;
  hipLaunchKernelGGL(k_procrustes, dim3(P), dim3(64), 0, ST(stream), src, ref, w, start, eps, T);
  return check_launch("lcr_procrustes_batched");
}

extern "C" int lcr_inlier_count(const float* T, int P, const float* src, const float* ref, int n, float radius, const int32_t* start, int min_count,
                                int32_t* counts, int32_t* best, void* stream) {
  if (!T || !src || !ref || !counts || P < 1 || n < 0) return LCR_EARG;
  hipLaunchKernelGGL(k_inlier_count, dim3(P), dim3(256), 0, ST(stream), T, src, ref, n, radius, start, min_count, counts);
  if (best) hipLaunchKernelGGL(k_argmax_i32, dim3(1), dim3(64), 0, ST(stream), counts, P, best);
  return check_launch("lcr_inlier_count");
}

extern "C" int lcr_inlier_weights(const float* T_all, const int32_t* sel, const float* src, const float* ref, const float* score, int n, float radius,
                                  float* w_out, void* stream) {
  if (!T_all || !src || !ref || !score || !w_out || n < 0) return LCR_EARG;
  if (n == 0) return LCR_OK;
  hipLaunchKernelGGL(k_inlier_weights, dim3(blocks_for(n)), dim3(256), 0, ST(stream), T_all, sel, src, ref, score, n, radius, w_out);
  return check_launch("lcr_inlier_weights");
}

// LocalGlobalRegistration.local_to_global_registration (geotransformer/local_global_registration.py:134-201) for S pairs at once:
// per-chunk hypotheses -> per-hypothesis inlier counts over the hypothesis's own pair -> best hypothesis per pair -> `steps`
// re-weighted refits.  ~2*steps + 5 launches whatever S is, no host synchronisation.  ws: lcr_lgr_ws_bytes(n, H, S).
extern "C" int lcr_lgr_ws_bytes(int64_t n, int H, int S, size_t* bytes) {
  if (!bytes || n < 0 || H < 1 || S < 1) return LCR_EARG;
  Carver c(nullptr, ~size_t(0));
  c.take<float>(static_cast<size_t>(H) * 16);      // hypotheses
  c.take<int32_t>(H);                              // inlier counts
  c.take<int32_t>(S + 1);                          // first row of every pair
  c.take<float>(static_cast<size_t>(S) * 16);      // fit over all rows of a pair
  c.take<float>(static_cast<size_t>(S) * 16);      // current transform of a pair
  c.take<float>(static_cast<size_t>(n > 0 ? n : 1));   // current weights
  c.take<float>(static_cast<size_t>(n > 0 ? n : 1));   // scores of the verification set (correspondence_limit)
  c.take<uint8_t>(static_cast<size_t>(n > 0 ? n : 1)); // its membership flags
  *bytes = c.off;
  return LCR_OK;
}
extern "C" int lcr_local_global_registration(const float* src, const float* ref, const float* score, int64_t n, const int32_t* hyp_start, int H,
                                             const int32_t* seg_hyp_start, int S, float radius, int min_count, int steps, float* T_out /*[S,4,4]*/,
                                             float* hyp_out /*[H,4,4] or NULL*/, int32_t* counts_out /*[H] or NULL*/, int32_t* best_out /*[S] or NULL*/,
                                             void* ws, size_t ws_bytes, void* stream) {
  return lcr_local_global_registration_ex(src, ref, score, n, hyp_start, H, seg_hyp_start, S, radius, min_count, steps, 0, T_out, hyp_out, counts_out,
                                          best_out, ws, ws_bytes, stream);
}
// correspondence_limit > 0: the per-pair verification set of local_global_registration.py:152-160 (k_lgr_topl); 0 = every correspondence
extern "C" int lcr_local_global_registration_ex(const float* src, const float* ref, const float* score, int64_t n, const int32_t* hyp_start, int H,
                                                const int32_t* seg_hyp_start, int S, float radius, int min_count, int steps, int correspondence_limit,
                                                float* T_out, float* hyp_out, int32_t* counts_out, int32_t* best_out, void* ws, size_t ws_bytes,
                                                void* stream) {
  if (correspondence_limit < 0) return LCR_EARG;
  if (!src || !ref || !score || !hyp_start || !seg_hyp_start || !T_out || !ws || n < 1 || H < 1 || S < 1 || steps < 1 || n > 2147483647) {
    set_error("lcr_local_global_registration: bad argument");
    return LCR_EARG;
  }
  size_t need = 0;
  lcr_lgr_ws_bytes(n, H, S, &need);
  if (need > ws_bytes) return LCR_ESPACE;
  Carver c(ws, ws_bytes);
  float* hyp = c.take<float>(static_cast<size_t>(H) * 16);
  int32_t* counts = c.take<int32_t>(H);
  int32_t* seg_rows = c.take<int32_t>(S + 1);
  float* T_rows = c.take<float>(static_cast<size_t>(S) * 16);
  float* T_cur = c.take<float>(static_cast<size_t>(S) * 16);
  float* cur = c.take<float>(static_cast<size_t>(n));
  float* score_ver = c.take<float>(static_cast<size_t>(n));
  uint8_t* ver_mask = c.take<uint8_t>(static_cast<size_t>(n));
  hipStream_t st = ST(stream);
  const int ni = static_cast<int>(n);
  hipLaunchKernelGGL(k_lgr_seg_rows, dim3(1), dim3(64), 0, st, hyp_start, seg_hyp_start, S, seg_rows);
  const float* vscore = score;                     // scores of the verification set (zero outside it)
  const uint8_t* vmask = nullptr;
  if (correspondence_limit > 0) {
    hipLaunchKernelGGL(k_lgr_topl, dim3(S), dim3(256), 0, st, score, seg_rows, correspondence_limit, ver_mask, score_ver);
    vscore = score_ver;
    vmask = ver_mask;
  }
  hipLaunchKernelGGL(k_procrustes, dim3(H), dim3(64), 0, st, src, ref, score, hyp_start, 1e-5f, hyp);        // hypotheses: ALL correspondences (:175-178)
  hipLaunchKernelGGL(k_procrustes, dim3(S), dim3(64), 0, st, src, ref, vscore, seg_rows, 1e-5f, T_rows);     // degenerate branch (:186-190)
  hipLaunchKernelGGL(k_inlier_count_seg, dim3(H), dim3(256), 0, st, hyp, src, ref, radius, hyp_start, seg_hyp_start, seg_rows, S, min_count, counts, vmask);
  hipLaunchKernelGGL(k_lgr_select, dim3(S), dim3(64), 0, st, hyp, counts, seg_hyp_start, T_rows, T_cur, best_out);
  for (int it = 0; it < steps; ++it) {
    hipLaunchKernelGGL(k_inlier_weights_seg, dim3(blocks_for(n)), dim3(256), 0, st, T_cur, seg_rows, S, src, ref, vscore, ni, radius, cur);
    hipLaunchKernelGGL(k_procrustes, dim3(S), dim3(64), 0, st, src, ref, cur, seg_rows, 1e-5f, it + 1 == steps ? T_out : T_cur);
  }
  if (hyp_out) hipMemcpyAsync(hyp_out, hyp, sizeof(float) * 16 * H, hipMemcpyDeviceToDevice, st);
  if (counts_out) hipMemcpyAsync(counts_out, counts, sizeof(int32_t) * H, hipMemcpyDeviceToDevice, st);
  return check_launch("lcr_local_global_registration");
}
