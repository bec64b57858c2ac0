// node_corr.hip — ground-truth patch overlaps (node correspondences) for P pairs in one call: which (ref node, src node) patches share
// a point pair closer than pos_radius under the ground-truth transform, and the overlap of the two patches.  The reference computes these
// labels pair by pair in torch (modules/registration/matching.py:252-349); the semantics here are stated in include/lcr_hip.h next to
// lcr_node_correspondences: direct differences, every operation rounded, so a label is a pure function of the inputs.
//
//   k_nc_transform  every point of the stack into the workspace once: pos clouds copied, anc clouds moved by their pair's transform;
//   k_nc_box        one wavefront per node: the axis-aligned box of its valid finite patch points (an empty box when it has none);
//   k_nc_overlap    the hot path.  One wavefront per (pair, ref node, slice of the src nodes).  The ref patch's valid points are compacted
//                   into LDS once.  64 src nodes at a time are screened against the ref box, one per lane; a survivor's valid points are
//                   compacted into LDS and walked by all lanes at a wave-uniform address (an LDS broadcast) while each lane holds one
//                   ref point in registers: 3 subtracts, 3 multiplies, 2 adds and a compare per point pair.  Row coverage is one bit per
//                   lane and 64-point ref chunk, column coverage one scalar bit per src point (ballot != 0).  The overlap goes into a
//                   dense M_p x N_p table, 0 = none (a correspondence has cr > 0, so its overlap is > 0);
//   k_nc_rowcount   one wavefront per ref row: non-zeros of its table row; a device scan over all rows follows;
//   k_nc_write      one wavefront per ref row: its non-zeros in ascending src node at the row's scanned offset (ballot + prefix);
//   k_nc_start      start[p] = scanned offset of pair p's first row; the status word.
// Every (i, j) of a pair is decided by its own patches alone and lands in the pair's own table, so neither the slice count nor the batch
// shows in a pair's rows.  No atomics anywhere.
//
// The box screen is lossless under the definition's arithmetic: with r' such that fl(r' * r') >= r2, fl(lo_b - hi_a) > r' on an axis
// means every point pair has fl(d) >= fl(lo_b - hi_a) > r' on that axis (rounding is monotone), hence fl(d * d) >= fl(r' * r') >= r2,
// and the other two squares only add non-negative terms: the pair is not near.
#include <climits>
#include <cmath>

#include "common.h"

namespace lcr {

constexpr int NC_MAX_PAIRS = 32;
constexpr int NC_MAX_K = 2048;             // 24 * K bytes of LDS per wavefront (<= 48 KB); row coverage is a 64-bit word of 64-point chunks
constexpr int NC_TARGET_WAVES = 2048;      // src slices are added until the overlap kernel has about this many wavefronts

struct NcPlan {
  int64_t po[2 * NC_MAX_PAIRS + 1];   // first point row of every cloud, relative to the first cloud
  int64_t to[NC_MAX_PAIRS + 1];       // first table entry of every pair
  int32_t mo[2 * NC_MAX_PAIRS + 1];   // first node row of every cloud, relative to the first cloud
  int32_t ro[NC_MAX_PAIRS + 1];       // first ref row of every pair among the stacked ref rows
  int     P;
};

__global__ __launch_bounds__(256) void k_nc_transform(const float* __restrict__ pts, const float* __restrict__ T, NcPlan pl, float* __restrict__ tp) {
  const int c = blockIdx.y;
  const int64_t p0 = pl.po[c], n = pl.po[c + 1] - p0;
  const float* t = T + 16 * (c >> 1);
  const bool move = c & 1;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float x = pts[3 * (p0 + i)], y = pts[3 * (p0 + i) + 1], z = pts[3 * (p0 + i) + 2];
    float ox = x, oy = y, oz = z;
    if (move) {
      ox = fadd(fadd(fadd(fmul(t[0], x), fmul(t[1], y)), fmul(t[2], z)), t[3]);
      oy = fadd(fadd(fadd(fmul(t[4], x), fmul(t[5], y)), fmul(t[6], z)), t[7]);
      oz = fadd(fadd(fadd(fmul(t[8], x), fmul(t[9], y)), fmul(t[10], z)), t[11]);
    }
    tp[3 * (p0 + i)] = ox;
    tp[3 * (p0 + i) + 1] = oy;
    tp[3 * (p0 + i) + 2] = oz;
  }
}

// a patch entry counts iff its node's mask and its own mask are set and its index is a point of the cloud
__device__ __forceinline__ bool nc_valid(const int64_t* __restrict__ knn, const uint8_t* __restrict__ km, int64_t row, int K, int k, bool node_ok,
                                         int64_t n_pts, int64_t* idx) {
  if (!node_ok || k >= K) return false;
  const int64_t e = row * K + k;
  if (!km[e]) return false;
  *idx = knn[e];
  return *idx >= 0 && *idx < n_pts;
}

__global__ __launch_bounds__(256) void k_nc_box(const float* __restrict__ tp, const int64_t* __restrict__ knn, const uint8_t* __restrict__ km,
                                                const uint8_t* __restrict__ nm, NcPlan pl, int K, float* __restrict__ box) {
  const int c = blockIdx.y;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= pl.mo[c + 1] - pl.mo[c]) return;                    // wave-uniform
  const int64_t g = pl.mo[c] + m, p0 = pl.po[c], n_pts = pl.po[c + 1] - p0;
  const bool node_ok = nm[g] != 0;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int k = lane_id(); k < K; k += WAVE) {
    int64_t idx;
    if (!nc_valid(knn, km, g, K, k, node_ok, n_pts, &idx)) continue;
    const float v[3] = {tp[3 * (p0 + idx)], tp[3 * (p0 + idx) + 1], tp[3 * (p0 + idx) + 2]};
    if (!(fabsf(v[0]) < INFINITY && fabsf(v[1]) < INFINITY && fabsf(v[2]) < INFINITY)) continue;      // a non-finite point is never near
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      lo[d] = fminf(lo[d], v[d]);
      hi[d] = fmaxf(hi[d], v[d]);
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      lo[d] = fminf(lo[d], __shfl_xor(lo[d], s));
      hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], s));
    }
  if (lane_id() < 3) {
    box[6 * g + lane_id()] = lane_id() == 0 ? lo[0] : lane_id() == 1 ? lo[1] : lo[2];
    box[6 * g + 3 + lane_id()] = lane_id() == 0 ? hi[0] : lane_id() == 1 ? hi[1] : hi[2];
  }
}

// the valid points of patch `row` compacted into sx / sy / sz in ascending k; returns their number (the whole wavefront calls this)
__device__ __forceinline__ int nc_stage(const float* __restrict__ tp, const int64_t* __restrict__ knn, const uint8_t* __restrict__ km, int64_t row,
                                        int K, bool node_ok, int64_t p0, int64_t n_pts, float* sx, float* sy, float* sz) {
  int n = 0;
  for (int k0 = 0; k0 < K; k0 += WAVE) {                       // wave-uniform trip count
    int64_t idx = 0;
    const bool ok = nc_valid(knn, km, row, K, k0 + lane_id(), node_ok, n_pts, &idx);
    const uint64_t m = wave_ballot(ok);
    if (ok) {
      const int o = n + mbcnt_lt(m);
      sx[o] = tp[3 * (p0 + idx)];
      sy[o] = tp[3 * (p0 + idx) + 1];
      sz[o] = tp[3 * (p0 + idx) + 2];
    }
    n += __popcll(m);
  }
  return n;
}

// one wavefront per workgroup: (ref node blockIdx.x, pair blockIdx.y, src slice blockIdx.z)
__global__ __launch_bounds__(64) void k_nc_overlap(const float* __restrict__ tp, const float* __restrict__ box, const int64_t* __restrict__ knn,
                                                   const uint8_t* __restrict__ km, const uint8_t* __restrict__ nm, NcPlan pl, int K, float r2,
                                                   float rbox, float* __restrict__ table) {
  extern __shared__ float nc_sm[];
  float *rx = nc_sm, *ry = rx + K, *rz = ry + K, *sx = rz + K, *sy = sx + K, *sz = sy + K;
  const int p = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
  const int cr_c = 2 * p, cs_c = 2 * p + 1;
  const int M = pl.mo[cr_c + 1] - pl.mo[cr_c], N = pl.mo[cs_c + 1] - pl.mo[cs_c];
  if (i >= M || N == 0) return;
  const int64_t gi = pl.mo[cr_c] + i, gs0 = pl.mo[cs_c];
  const int nr = nc_stage(tp, knn, km, gi, K, nm[gi] != 0, pl.po[cr_c], pl.po[cr_c + 1] - pl.po[cr_c], rx, ry, rz);
  float bl[3], bh[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    bl[d] = box[6 * gi + d];
    bh[d] = box[6 * gi + 3 + d];
  }
  float* row = table + pl.to[p] + static_cast<int64_t>(i) * N;
  const int64_t sp0 = pl.po[cs_c], sn = pl.po[cs_c + 1] - sp0;
  const int chunks = (N + WAVE - 1) / WAVE;
  __syncthreads();
  for (int c = blockIdx.z; c < chunks; c += gridDim.z) {
    const int j = c * WAVE + lane;
    bool surv = nr > 0 && j < N;
    if (surv) {
      const float* b = box + 6 * (gs0 + j);
#pragma unroll
      for (int d = 0; d < 3; ++d) surv = surv && !(fsub(b[d], bh[d]) > rbox) && !(fsub(bl[d], b[3 + d]) > rbox);
    }
    uint64_t todo = wave_ballot(surv);
    float ov = 0.f;
    while (todo) {                                             // wave-uniform
      const int b = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int64_t gj = gs0 + c * WAVE + b;
      const int ns = nc_stage(tp, knn, km, gj, K, nm[gj] != 0, sp0, sn, sx, sy, sz);
      __syncthreads();
      uint64_t rowbits = 0;                                    // bit t: my ref point of chunk t is near some src point
      int cs = 0;
      for (int g0 = 0; g0 < ns; g0 += WAVE) {
        const int gn = min(WAVE, ns - g0);
        uint64_t colbits = 0;                                  // bit k: src point g0 + k is near some ref point (wave-uniform)
        for (int t = 0; t * WAVE < nr; ++t) {
          const int a = t * WAVE + lane;
          const bool have = a < nr;
          const float px = have ? rx[a] : NAN, py = have ? ry[a] : NAN, pz = have ? rz[a] : NAN;
          bool any = false;
          for (int k = 0; k < gn; ++k) {
            const float dx = fsub(px, sx[g0 + k]), dy = fsub(py, sy[g0 + k]), dz = fsub(pz, sz[g0 + k]);
            const bool near = fadd(fadd(fmul(dx, dx), fmul(dy, dy)), fmul(dz, dz)) < r2;
            any = any || near;
            colbits |= static_cast<uint64_t>(wave_ballot(near) != 0) << k;
          }
          rowbits |= static_cast<uint64_t>(any) << t;
        }
        cs += __popcll(colbits);
      }
      const int cr = wave_sum(static_cast<int>(__popcll(rowbits)));
      if (lane == b && cr > 0)
        ov = fdiv(fadd(fdiv(static_cast<float>(cr), static_cast<float>(nr)), fdiv(static_cast<float>(cs), static_cast<float>(ns))), 2.f);
      __syncthreads();                                         // the next survivor overwrites the src patch
    }
    if (j < N) row[j] = ov;
  }
}

__global__ __launch_bounds__(256) void k_nc_rowcount(const float* __restrict__ table, NcPlan pl, int R, int32_t* __restrict__ count) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r > R) return;
  int n = 0;
  if (r < R) {
    const int p = cloud_of(pl.ro, pl.P, r);
    const int N = pl.mo[2 * p + 2] - pl.mo[2 * p + 1];
    const float* row = table + pl.to[p] + static_cast<int64_t>(r - pl.ro[p]) * N;
    for (int j0 = 0; j0 < N; j0 += WAVE) n += __popcll(wave_ballot(j0 + lane_id() < N && row[j0 + lane_id()] != 0.f));
  }
  if (lane_id() == 0) count[r] = n;                            // count[R] = 0: the scan's last entry becomes the total
}

__global__ __launch_bounds__(256) void k_nc_write(const float* __restrict__ table, NcPlan pl, int R, const int32_t* __restrict__ scan, int64_t cap,
                                                  int32_t* __restrict__ corr, float* __restrict__ overlap) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int p = cloud_of(pl.ro, pl.P, r);
  const int N = pl.mo[2 * p + 2] - pl.mo[2 * p + 1], i = r - pl.ro[p];
  const float* row = table + pl.to[p] + static_cast<int64_t>(i) * N;
  int64_t base = scan[r];
  for (int j0 = 0; j0 < N; j0 += WAVE) {
    const int j = j0 + lane_id();
    const float v = j < N ? row[j] : 0.f;
    const uint64_t m = wave_ballot(v != 0.f);
    const int64_t o = base + mbcnt_lt(m);
    if (v != 0.f && o < cap) {
      corr[2 * o] = i;
      corr[2 * o + 1] = j;
      overlap[o] = v;
    }
    base += __popcll(m);
  }
}

__global__ __launch_bounds__(64) void k_nc_start(NcPlan pl, int R, const int32_t* __restrict__ scan, int64_t cap, int32_t* __restrict__ start,
                                                 uint32_t* __restrict__ status) {
  const int t = threadIdx.x;
  if (t <= pl.P) start[t] = scan[t < pl.P ? pl.ro[t] : R];
  if (t == 0) *status = scan[R] > cap ? LCR_STATUS_CAP_EXCEEDED : 0u;
}

}  // namespace lcr

using namespace lcr;

struct NcLayout {
  float *  tp, *box, *table;   // tp [points,3]: the stack with the anc clouds moved; box [nodes,6]; table: the pairs' M_p x N_p overlaps
  int32_t *count, *scan;       // [R+1] each, R = stacked ref rows
  void*    scan_ws;
  size_t   bytes;
};

// the plan from the host offsets; LCR_EARG (with a message) outside the domain
static int nc_plan(const char* entry, const int64_t* point_off, const int64_t* node_off, int P, int K, NcPlan* pl, int64_t* n_pts, int64_t* n_nodes,
                   int64_t* n_max, int* m_max_cloud, int* m_max_ref, int* n_max_src) {
  if (!point_off || !node_off || P < 1 || P > NC_MAX_PAIRS || K < 1 || K > NC_MAX_K)
    return refuse(LCR_EARG, "%s: null offsets or outside the domain (1 <= P <= %d, 1 <= K <= %d): P=%d K=%d", entry, NC_MAX_PAIRS, NC_MAX_K, P, K);
  *n_max = 0;
  *m_max_cloud = *m_max_ref = *n_max_src = 0;
  for (int c = 0; c <= 2 * P; ++c) {
    if (c && (point_off[c] < point_off[c - 1] || node_off[c] < node_off[c - 1])) return refuse(LCR_EARG, "%s: offsets must not decrease", entry);
    pl->po[c] = point_off[c] - point_off[0];
    const int64_t mo = node_off[c] - node_off[0];
    if (pl->po[c] > INT32_MAX || mo > INT32_MAX) return refuse(LCR_EARG, "%s: more than 2^31-1 points or nodes", entry);
    pl->mo[c] = static_cast<int32_t>(mo);
    if (c) {
      *n_max = std::max(*n_max, pl->po[c] - pl->po[c - 1]);
      const int m = pl->mo[c] - pl->mo[c - 1];
      *m_max_cloud = std::max(*m_max_cloud, m);
      if (c & 1) *m_max_ref = std::max(*m_max_ref, m); else *n_max_src = std::max(*n_max_src, m);
    }
  }
  pl->P = P;
  pl->to[0] = 0;
  pl->ro[0] = 0;
  for (int p = 0; p < P; ++p) {
    const int64_t M = pl->mo[2 * p + 1] - pl->mo[2 * p], N = pl->mo[2 * p + 2] - pl->mo[2 * p + 1];
    pl->to[p + 1] = pl->to[p] + M * N;
    pl->ro[p + 1] = pl->ro[p] + static_cast<int32_t>(M);
    if (pl->to[p + 1] > INT32_MAX) return refuse(LCR_EARG, "%s: more than 2^31-1 node pairs", entry);
  }
  *n_pts = pl->po[2 * P];
  *n_nodes = pl->mo[2 * P];
  return LCR_OK;
}

static NcLayout nc_layout(void* ws, const NcPlan& pl, int64_t n_pts, int64_t n_nodes) {
  NcLayout L;
  Carver c(ws, ~size_t(0));
  const size_t R = static_cast<size_t>(pl.ro[pl.P]);
  L.tp = c.take<float>(3 * static_cast<size_t>(n_pts));
  L.box = c.take<float>(6 * static_cast<size_t>(n_nodes));
  L.table = c.take<float>(static_cast<size_t>(pl.to[pl.P]));
  L.count = c.take<int32_t>(R + 1);
  L.scan = c.take<int32_t>(R + 1);
  L.scan_ws = c.take<char>(scan_ws_bytes(static_cast<int64_t>(R) + 2));
  L.bytes = c.off;
  return L;
}

extern "C" int lcr_node_correspondences_ws_bytes(const int64_t* point_off, const int64_t* node_off, int P, int K, size_t* bytes) {
  NcPlan pl;
  int64_t n_pts, n_nodes, n_max;
  int mc, mr, nsrc;
  if (!bytes) return refuse(LCR_EARG, "lcr_node_correspondences_ws_bytes: null pointer");
  const int rc = nc_plan("lcr_node_correspondences_ws_bytes", point_off, node_off, P, K, &pl, &n_pts, &n_nodes, &n_max, &mc, &mr, &nsrc);
  if (rc != LCR_OK) return rc;
  *bytes = nc_layout(nullptr, pl, n_pts, n_nodes).bytes;
  return LCR_OK;
}

extern "C" int lcr_node_correspondences(const float* points, const int64_t* point_off, const float* nodes, const int64_t* node_off,
                                        const int64_t* knn, const uint8_t* knn_mask, const uint8_t* node_mask, const float* transforms, int P,
                                        int K, double pos_radius, int64_t cap, int32_t* corr, float* overlap, int32_t* start, uint32_t* status,
                                        void* ws, size_t ws_bytes, void* stream) {
  (void)nodes;   // the node centres are part of the partition's output but not of the definition (the reference's sphere screen is not used)
  NcPlan pl;
  int64_t n_pts, n_nodes, n_max;
  int m_cloud, m_ref, n_src;
  const int rc = nc_plan("lcr_node_correspondences", point_off, node_off, P, K, &pl, &n_pts, &n_nodes, &n_max, &m_cloud, &m_ref, &n_src);
  if (rc != LCR_OK) return rc;
  const float r2 = static_cast<float>(pos_radius * pos_radius);
  if (!transforms || !start || !status || !ws || cap < 0 || (cap > 0 && (!corr || !overlap)) || (n_pts > 0 && !points) ||
      (n_nodes > 0 && (!knn || !knn_mask || !node_mask)) || !(pos_radius >= 0) || !(r2 < INFINITY))
    return refuse(LCR_EARG, "lcr_node_correspondences: null pointer, negative cap, or pos_radius negative / not finite when squared");
  const NcLayout L = nc_layout(ws, pl, n_pts, n_nodes);
  if (L.bytes > ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_node_correspondences", ws_bytes, L.bytes);
  // the box screen's radius: the smallest float at or above pos_radius whose rounded square reaches r2
  float rbox = static_cast<float>(pos_radius);
  while (rbox * rbox < r2) rbox = nextafterf(rbox, INFINITY);
  hipStream_t st = ST(stream);
  const int R = pl.ro[P];
  const float* pts = points ? points + 3 * point_off[0] : nullptr;
  if (n_max > 0) hipLaunchKernelGGL(k_nc_transform, dim3(blocks_for(n_max, 256, 1024), 2 * P), dim3(256), 0, st, pts, transforms, pl, L.tp);
  if (m_cloud > 0) hipLaunchKernelGGL(k_nc_box, dim3(div_up(m_cloud, 4), 2 * P), dim3(256), 0, st, L.tp, knn, knn_mask, node_mask, pl, K, L.box);
  if (m_ref > 0 && n_src > 0) {
    const int chunks = div_up(n_src, WAVE);
    const int Z = std::max(1, std::min(chunks, NC_TARGET_WAVES / std::max(1, m_ref * P)));
    hipLaunchKernelGGL(k_nc_overlap, dim3(m_ref, P, Z), dim3(64), sizeof(float) * 6 * K, st, L.tp, L.box, knn, knn_mask, node_mask, pl, K, r2, rbox,
                       L.table);
  }
  hipLaunchKernelGGL(k_nc_rowcount, dim3(div_up(R + 1, 4)), dim3(256), 0, st, L.table, pl, R, L.count);
  const int src = exclusive_scan_i32("lcr_node_correspondences", L.count, L.scan, R + 1, nullptr, L.scan_ws, st);
  if (src != LCR_OK) return src;
  if (R > 0) hipLaunchKernelGGL(k_nc_write, dim3(div_up(R, 4)), dim3(256), 0, st, L.table, pl, R, L.scan, cap, corr, overlap);
  hipLaunchKernelGGL(k_nc_start, dim3(1), dim3(64), 0, st, pl, R, L.scan, cap, start, status);
  return check_launch("lcr_node_correspondences");
}
