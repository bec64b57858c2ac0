// feature_nn.hip — exact nearest neighbour in feature space, batched over pairs, and the correspondence list built from it
// (utils/utils/open3d.py:109-142: Open3D's registration_ransac_based_on_feature_matching does both on the host with a KD-tree over the
// features).  The semantics are stated in include/lcr_hip.h next to the entry points.
//
// lcr_feature_nn: the plain exact form.  d2(i, j) is the channel-by-channel chain of the header for EVERY (i, j), on the vector unit:
//   k_fnn_tiles   the hot path.  One scan over the pair sizes maps workgroup -> (pair, tile of 128 query rows); a workgroup of 256
//                 threads holds a 128 x 64 block of (query, database) accumulators in registers, 8 x 4 per thread, and walks the
//                 channels in chunks of 32 staged channel-major through LDS (the 8 query values of a thread are one broadcast address
//                 per 16 lanes, its 4 database values one conflict-free ds_read_b128).  Per (i, j, c): one subtract, one multiply, one
//                 add, every one rounded — VALU-issue bound: 3 * nq * nd * C operations against the unit's 78.6 T non-fused op/s.  The
//                 accumulation order over c is that of the definition, so no tile shape changes a bit of d2.  After the last channel
//                 every thread folds its 32 distances into a running (d2, j) minimum per query row; at the end of the walk the 16
//                 threads of a row are merged through LDS.  grid.y splits the database tiles (tile t goes to slice t mod Z) so that a
//                 single pair still fills the chip; the slices' minima go to the workspace;
//   k_fnn_merge   one thread per query row: the minimum of its Z partial results in the total order (d2, j).
// The minimum of a total order does not depend on how the candidates were grouped, so tiles, slices and batch position cannot show.
//
// lcr_feature_correspondences: count (one workgroup per pair, decides the mutual fall-back), exclusive scan over the pairs, ordered
// write (wavefront ballot + prefix, no atomics).
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace lcr {

constexpr int FN_TQ = 128;            // query rows per workgroup
constexpr int FN_TD = 64;             // database rows per tile
constexpr int FN_CK = 32;             // channels per LDS chunk
constexpr int FN_QP = FN_TQ + 4;      // LDS row pitch in floats (channel-major; +4 keeps float4 reads aligned and spreads the staging writes)
constexpr int FN_DP = FN_TD + 4;
constexpr int FN_MAX_SPLIT = 16;      // database slices at most
constexpr uint32_t FN_NAN = 0x7fc00000u;

// candidate (d, j) against the running minimum (bd, bj): NaN never wins, ties go to the smaller row
__device__ __forceinline__ bool fn_better(float d, int j, float bd, int bj) {
  return j >= 0 && d == d && (bj < 0 || d < bd || (d == bd && j < bj));
}

// tiles[s] = query tiles of pair s (s < S), tiles[S] = 0: the input of the scan that maps workgroups to (pair, tile)
__global__ __launch_bounds__(256) void k_fnn_count_tiles(const int32_t* __restrict__ q_start, int S, int32_t* __restrict__ tiles) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > S) return;
  tiles[s] = s < S ? (max(q_start[s + 1] - q_start[s], 0) + FN_TQ - 1) / FN_TQ : 0;
}

__global__ __launch_bounds__(256) void k_fnn_tiles(const float* __restrict__ qf, const float* __restrict__ df, const int32_t* __restrict__ q_start,
                                                   const int32_t* __restrict__ d_start, const int32_t* __restrict__ tile_start, int S, int C,
                                                   int64_t nq_total, float* __restrict__ part_d2, int32_t* __restrict__ part_j) {
  __shared__ __attribute__((aligned(16))) float sm[FN_CK * (FN_QP + FN_DP)];
  float* Qs = sm;
  float* Ds = sm + FN_CK * FN_QP;
  const int wg = blockIdx.x, z = blockIdx.y, Z = gridDim.y, tid = threadIdx.x;
  if (wg >= tile_start[S]) return;
  int lo = 0, hi = S - 1;                                 // the pair that owns tile wg: the last s with tile_start[s] <= wg
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_start[mid] <= wg) lo = mid; else hi = mid - 1;
  }
  const int s = lo;
  const int64_t qa = q_start[s], da = d_start[s];
  const int nq = q_start[s + 1] - q_start[s], nd = d_start[s + 1] - d_start[s];
  const int q0 = (wg - tile_start[s]) * FN_TQ;
  const int tx = tid & 15, ty = tid >> 4;
  float bd[8];
  int bj[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    bd[a] = __uint_as_float(FN_NAN);
    bj[a] = -1;
  }
  const int ndt = nd > 0 ? (nd + FN_TD - 1) / FN_TD : 0;
  for (int dt = z; dt < ndt; dt += Z) {
    const int j0 = dt * FN_TD;
    float acc[8][4];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int c0 = 0; c0 < C; c0 += FN_CK) {
      __syncthreads();
      // stage channel-major; rows or channels outside the pair are zeros (t = 0 adds +0 to a non-negative sum: no bit changes)
      for (int e = tid; e < FN_TQ * FN_CK; e += 256) {
        const int c = e & (FN_CK - 1), r = e / FN_CK;
        const bool in = q0 + r < nq && c0 + c < C;
        Qs[c * FN_QP + r] = in ? qf[(qa + q0 + r) * C + c0 + c] : 0.f;
      }
      for (int e = tid; e < FN_TD * FN_CK; e += 256) {
        const int c = e & (FN_CK - 1), r = e / FN_CK;
        const bool in = j0 + r < nd && c0 + c < C;
        Ds[c * FN_DP + r] = in ? df[(da + j0 + r) * C + c0 + c] : 0.f;
      }
      __syncthreads();
#pragma unroll 4
      for (int c = 0; c < FN_CK; ++c) {
        const float4 qa4 = *reinterpret_cast<const float4*>(Qs + c * FN_QP + ty * 8);
        const float4 qb4 = *reinterpret_cast<const float4*>(Qs + c * FN_QP + ty * 8 + 4);
        const float4 d4 = *reinterpret_cast<const float4*>(Ds + c * FN_DP + tx * 4);
        const float q[8] = {qa4.x, qa4.y, qa4.z, qa4.w, qb4.x, qb4.y, qb4.z, qb4.w};
        const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const float t = fsub(q[a], d[b]);
            acc[a][b] = fadd(acc[a][b], fmul(t, t));
          }
      }
    }
    // ascending j inside the thread: a strict "<" keeps the smaller row on ties
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + tx * 4 + b;
      if (j < nd) {
#pragma unroll
        for (int a = 0; a < 8; ++a) {
          const float d = acc[a][b];
          if (d == d && (bj[a] < 0 || d < bd[a])) {
            bd[a] = d;
            bj[a] = j;
          }
        }
      }
    }
  }
  // merge the 16 threads of every query row through LDS (the staging buffer is free now)
  __syncthreads();
  float* rd = sm;
  int32_t* rj = reinterpret_cast<int32_t*>(sm + FN_TQ * 16);
  static_assert(FN_TQ * 16 * 2 <= FN_CK * (FN_QP + FN_DP), "the row merge must fit the staging buffer");
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    rd[(ty * 8 + a) * 16 + tx] = bd[a];
    rj[(ty * 8 + a) * 16 + tx] = bj[a];
  }
  __syncthreads();
  if (tid < FN_TQ && q0 + tid < nq) {
    float d = rd[tid * 16];
    int j = rj[tid * 16];
    for (int k = 1; k < 16; ++k) {
      const float od = rd[tid * 16 + k];
      const int oj = rj[tid * 16 + k];
      if (fn_better(od, oj, d, j)) {
        d = od;
        j = oj;
      }
    }
    const int64_t o = static_cast<int64_t>(z) * nq_total + qa + q0 + tid;
    part_d2[o] = d;
    part_j[o] = j;
  }
}

__global__ __launch_bounds__(256) void k_fnn_merge(const float* __restrict__ part_d2, const int32_t* __restrict__ part_j, int Z, int64_t nq_total,
                                                   int32_t* __restrict__ nn, float* __restrict__ d2) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= nq_total) return;
  float d = part_d2[i];
  int j = part_j[i];
  for (int z = 1; z < Z; ++z) {
    const float od = part_d2[z * nq_total + i];
    const int oj = part_j[z * nq_total + i];
    if (fn_better(od, oj, d, j)) {
      d = od;
      j = oj;
    }
  }
  nn[i] = j;
  d2[i] = j < 0 ? __uint_as_float(FN_NAN) : d;
}

// ---- correspondences from the nearest-neighbour rows ---------------------------------------------------------------------------------

__device__ __forceinline__ bool fc_keep(const int32_t* __restrict__ nn_sr, const int32_t* __restrict__ nn_rs, int64_t sa, int64_t ra, int nr, int i,
                                        bool mutual) {
  const int j = nn_sr[sa + i];
  if (j < 0 || j >= nr) return false;
  return !mutual || nn_rs[ra + j] == i;
}

// one workgroup per pair: rows kept without and with the mutual filter; the filter holds for the pair iff it leaves >= min_rows rows
__global__ __launch_bounds__(256) void k_fc_count(const int32_t* __restrict__ nn_sr, const int32_t* __restrict__ src_start,
                                                  const int32_t* __restrict__ nn_rs, const int32_t* __restrict__ ref_start, int S, int min_rows,
                                                  int32_t* __restrict__ count, int32_t* __restrict__ use_mutual) {
  __shared__ int s_any[4], s_mut[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int64_t sa = src_start[s], ra = ref_start[s];
  const int ns = src_start[s + 1] - src_start[s], nr = ref_start[s + 1] - ref_start[s];
  int any = 0, mut = 0;
  for (int i = tid; i < ns; i += 256) {
    any += fc_keep(nn_sr, nn_rs, sa, ra, nr, i, false) ? 1 : 0;
    if (nn_rs) mut += fc_keep(nn_sr, nn_rs, sa, ra, nr, i, true) ? 1 : 0;
  }
  any = wave_sum(any);
  mut = wave_sum(mut);
  if ((tid & 63) == 0) {
    s_any[tid >> 6] = any;
    s_mut[tid >> 6] = mut;
  }
  __syncthreads();
  if (tid == 0) {
    any = s_any[0] + s_any[1] + s_any[2] + s_any[3];
    mut = s_mut[0] + s_mut[1] + s_mut[2] + s_mut[3];
    const bool use = nn_rs != nullptr && mut >= min_rows;
    count[s] = use ? mut : any;
    use_mutual[s] = use ? 1 : 0;
    if (s == 0) count[S] = 0;
  }
}

// one workgroup per pair: the kept rows (i, nn_sr[i]) in ascending i at start[s] + rank
__global__ __launch_bounds__(256) void k_fc_write(const int32_t* __restrict__ nn_sr, const int32_t* __restrict__ src_start,
                                                  const int32_t* __restrict__ nn_rs, const int32_t* __restrict__ ref_start,
                                                  const int32_t* __restrict__ start, const int32_t* __restrict__ use_mutual,
                                                  int32_t* __restrict__ corr, int32_t* __restrict__ mutual_out) {
  __shared__ int s_w[4];
  const int s = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  const int64_t sa = src_start[s], ra = ref_start[s];
  const int ns = src_start[s + 1] - src_start[s], nr = ref_start[s + 1] - ref_start[s];
  const bool mutual = use_mutual[s] != 0;
  if (tid == 0 && mutual_out) mutual_out[s] = mutual ? 1 : 0;
  int64_t base = start[s];
  for (int i0 = 0; i0 < ns; i0 += 256) {                  // block-uniform trip count
    const int i = i0 + tid;
    const bool keep = i < ns && fc_keep(nn_sr, nn_rs, sa, ra, nr, i, mutual);
    const uint64_t m = wave_ballot(keep);
    __syncthreads();
    if ((tid & 63) == 0) s_w[w] = __popcll(m);
    __syncthreads();
    int off = mbcnt_lt(m);
    for (int k = 0; k < w; ++k) off += s_w[k];
    if (keep) {
      corr[2 * (base + off)] = i;
      corr[2 * (base + off) + 1] = nn_sr[sa + i];
    }
    base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
  }
}

}  // namespace lcr

using namespace lcr;

static int fnn_domain(int S, int C, int64_t nq, int64_t nd, const char* what) {
  if (S < 1 || S > 65535 || C < 1 || C > 1024 || nq < 0 || nd < 0 || nq > INT32_MAX || nd > INT32_MAX)
    return refuse(LCR_EARG, "%s: outside the domain (1 <= S <= 65535, 1 <= C <= 1024, 0 <= nq, nd <= 2^31-1): S=%d C=%d nq=%lld nd=%lld", what, S, C,
                  static_cast<long long>(nq), static_cast<long long>(nd));
  return LCR_OK;
}

// database slices: enough workgroups for ~4 per CU when few query tiles exist, never more slices than database tiles
static int fnn_split(int S, int64_t nq, int64_t nd) {
  const int64_t tiles = (nq + FN_TQ - 1) / FN_TQ + S;
  const int64_t dt = std::max<int64_t>(1, (nd / S + FN_TD - 1) / FN_TD);
  int64_t z = (1024 + tiles - 1) / tiles;
  z = std::min<int64_t>(std::min<int64_t>(z, dt), FN_MAX_SPLIT);
  return static_cast<int>(std::max<int64_t>(z, 1));
}

struct FnnLayout {
  int32_t *tiles, *pj;   // tiles [S+1]: query tiles per pair, scanned in place; pd / pj [Z, nq]: per-slice minima and their rows
  float*   pd;
  void*    scan_ws;
  int      Z;            // database slices (fnn_split)
  size_t   bytes;
};
static FnnLayout fnn_layout(void* ws, int S, int64_t nq, int64_t nd) {
  FnnLayout L;
  Carver c(ws, ~size_t(0));
  L.tiles = c.take<int32_t>(static_cast<size_t>(S) + 1);
  L.scan_ws = c.take<char>(scan_ws_bytes(S + 2));
  L.Z = fnn_split(S, nq, nd);
  L.pd = c.take<float>(static_cast<size_t>(L.Z) * nq);
  L.pj = c.take<int32_t>(static_cast<size_t>(L.Z) * nq);
  L.bytes = c.off;
  return L;
}

extern "C" int lcr_feature_nn_ws_bytes(int S, int64_t nq, int64_t nd, size_t* bytes) {
  if (!bytes) return refuse(LCR_EARG, "lcr_feature_nn_ws_bytes: null pointer");
  if (int rc = fnn_domain(S, 1, nq, nd, "lcr_feature_nn_ws_bytes")) return rc;
  *bytes = fnn_layout(nullptr, S, nq, nd).bytes;
  return LCR_OK;
}

extern "C" int lcr_feature_nn(const float* qf, const float* df, const int32_t* q_start, const int32_t* d_start, int S, int C, int64_t nq,
                              int64_t nd, int32_t* nn, float* d2, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = fnn_domain(S, C, nq, nd, "lcr_feature_nn")) return rc;
  if (!q_start || !d_start || !ws || (nq > 0 && (!qf || !nn || !d2)) || (nd > 0 && !df)) return refuse(LCR_EARG, "lcr_feature_nn: null pointer");
  const FnnLayout L = fnn_layout(ws, S, nq, nd);
  if (L.bytes > ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_feature_nn", ws_bytes, L.bytes);
  if (nq == 0) return LCR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_fnn_count_tiles, dim3(div_up(S + 1, 256)), dim3(256), 0, st, q_start, S, L.tiles);
  int rc = exclusive_scan_i32("lcr_feature_nn", L.tiles, L.tiles, S + 1, nullptr, L.scan_ws, st);
  if (rc != LCR_OK) return rc;
  const int64_t wgs = (nq + FN_TQ - 1) / FN_TQ + S;                   // upper bound of sum ceil(nq_s / 128); the surplus exits at once
  hipLaunchKernelGGL(k_fnn_tiles, dim3(static_cast<unsigned>(wgs), L.Z), dim3(256), 0, st, qf, df, q_start, d_start, L.tiles, S, C, nq, L.pd, L.pj);
  hipLaunchKernelGGL(k_fnn_merge, dim3(div_up(nq, 256)), dim3(256), 0, st, L.pd, L.pj, L.Z, nq, nn, d2);
  return check_launch("lcr_feature_nn");
}

struct FcLayout {
  int32_t *count, *use;   // count [S+1]: correspondences per pair; use [S]: 1 = the pair uses its mutual matches
  void*    scan_ws;
  size_t   bytes;
};
static FcLayout fc_layout(void* ws, int S) {
  FcLayout L;
  Carver c(ws, ~size_t(0));
  L.count = c.take<int32_t>(static_cast<size_t>(S) + 1);
  L.use = c.take<int32_t>(static_cast<size_t>(S));
  L.scan_ws = c.take<char>(scan_ws_bytes(S + 2));
  L.bytes = c.off;
  return L;
}

extern "C" int lcr_feature_correspondences_ws_bytes(int S, size_t* bytes) {
  if (!bytes || S < 1 || S > 65535) return refuse(LCR_EARG, "lcr_feature_correspondences_ws_bytes: null pointer or S outside 1..65535 (S=%d)", S);
  *bytes = fc_layout(nullptr, S).bytes;
  return LCR_OK;
}

extern "C" int lcr_feature_correspondences(const int32_t* nn_sr, const int32_t* src_start, const int32_t* nn_rs, const int32_t* ref_start, int S,
                                           int min_rows, int32_t* corr, int32_t* start, int32_t* mutual_used, void* ws, size_t ws_bytes,
                                           void* stream) {
  if (S < 1 || S > 65535 || min_rows < 0 || !nn_sr || !src_start || !ref_start || !corr || !start || !ws)
    return refuse(LCR_EARG, "lcr_feature_correspondences: null pointer or outside the domain (1 <= S <= 65535, min_rows >= 0): S=%d min_rows=%d", S, min_rows);
  const FcLayout L = fc_layout(ws, S);
  if (L.bytes > ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_feature_correspondences", ws_bytes, L.bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_fc_count, dim3(S), dim3(256), 0, st, nn_sr, src_start, nn_rs, ref_start, S, min_rows, L.count, L.use);
  int rc = exclusive_scan_i32("lcr_feature_correspondences", L.count, start, S + 1, nullptr, L.scan_ws, st);
  if (rc != LCR_OK) return rc;
  hipLaunchKernelGGL(k_fc_write, dim3(S), dim3(256), 0, st, nn_sr, src_start, nn_rs, ref_start, start, L.use, corr, mutual_used);
  return check_launch("lcr_feature_correspondences");
}
