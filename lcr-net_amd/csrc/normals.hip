// normals.hip — surface normals (Open3D's EstimateNormals with KDTreeSearchParamHybrid(radius, max_nn), which the reference's helpers
// call: utils/utils/open3d.py:53-58) for B stacked clouds in one call, exact and batch-invariant.  Semantics in include/lcr_hip.h
// (lcr_estimate_normals).
//
// Per call: stack_to_device (cloud lengths to the device), the support grid of radius_search.hip (cell >= r, built once), then
//   k_normals_cov     one wavefront per query row.  Its lanes stride over the candidates of the nine x-runs of the row's 3x3x3 cell
//                     neighbourhood.  Pass 1 counts the hits (d2 < r*r), compacts them into an LDS list while they fit (max_nn slots)
//                     and histograms the top byte of their (d2, row) keys.  A ball of at most max_nn hits is done after pass 1.  A
//                     larger one selects the max_nn-th key by an MSB-first radix select over the 64-bit key (8-bit digits, one LDS
//                     histogram per pass, stopping at the first digit whose bin is taken whole), then compacts the keys below it in
//                     one more pass.  Every pass costs one stride over the candidates for the whole wavefront, so a
//                     ball of thousands of hits costs a few times a small one, never a re-enumeration per hit.  The selected rows are
//                     ranked by row index and summed in that order (lane l takes ranks l and l + 64, then a fixed xor tree): the sum
//                     does not depend on the grid's within-cell order, which the build's atomics leave unspecified.  Writes the fp64
//                     covariance (6 entries) and k per row.
//   k_normals_finish  one thread per row: fp64 Jacobi eigen-solve (rigid3.h), degeneracy, orientation, outputs.
// Why one wavefront per query and not one thread (k_icp_match's form): selecting the max_nn-th key needs a histogram or a sorted list
// per query; per wavefront that is 1 KiB of LDS, per thread a max_nn-row list for each of 256 threads.  Both forms evaluate every
// candidate of a query once per pass.
#include <climits>
#include <cmath>

#include "common.h"
#include "grid.h"
#include "rigid3.h"

namespace lcr {

constexpr int NRM_WAVES = 4;        // wavefronts (= query rows) per k_normals_cov workgroup
constexpr int NRM_MAX_NN = 128;     // largest max_nn: two selected rows per lane

// Visit the candidates of row (qx, qy, qz) of cloud c, the runs of grid_for_each_run (grid.h): fn(valid, p) once per lane and per stride
// of 64, wave-uniform trip counts.
template <typename F>
__device__ __forceinline__ void nrm_candidates(const GridCloud& c, const int32_t* __restrict__ cell_start, const float4* __restrict__ sorted,
                                               float qx, float qy, float qz, F&& fn) {
  const int lane = threadIdx.x & 63;
  grid_for_each_run(c, cell_start, qx, qy, qz, [&](int k0, int e) {
    for (; k0 < e; k0 += 64) {
      const int k = k0 + lane;
      const bool valid = k < e;
      const float4 p = sorted[valid ? k : e - 1];
      fn(valid, p);
    }
  });
}

__device__ __forceinline__ uint64_t nrm_key(float qx, float qy, float qz, const float4& p, float r2, bool valid, bool& hit) {
  const float d2 = grid_d2(qx, qy, qz, p);
  hit = valid && d2 < r2;
  return grid_key(d2, p.w);
}

// one wavefront per row: the row's neighbourhood (max_nn smallest (d2, row) keys with d2 < r2), covariance about the row -> cov[6], cnt
__global__ __launch_bounds__(NRM_WAVES * 64) void k_normals_cov(Stack C, const float* __restrict__ pts, const GridHeader* __restrict__ h,
                                                               const int32_t* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                               float r2, int max_nn, double* __restrict__ cov, int32_t* __restrict__ cnt_out) {
  __shared__ uint32_t s_hist[NRM_WAVES][256];
  __shared__ float4 s_sel[NRM_WAVES][NRM_MAX_NN];
  __shared__ float4 s_ord[NRM_WAVES][NRM_MAX_NN];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * NRM_WAVES + w;
  if (i >= C.off[C.B]) return;                                   // wave-uniform
  const int b = cloud_of(C.off, C.B, i);
  const GridCloud& c = h->cloud[b];
  const float qx = pts[3 * i], qy = pts[3 * i + 1], qz = pts[3 * i + 2];
  uint32_t* hist = s_hist[w];
  float4* sel = s_sel[w];
  float4* ord = s_ord[w];
#pragma unroll
  for (int u = 0; u < 4; ++u) hist[4 * lane + u] = 0u;
  wave_sync();

  // pass 1: count, compact while the hits fit, histogram of key bits 63..56
  int cnt = 0;
  nrm_candidates(c, cell_start, sorted, qx, qy, qz, [&](bool valid, const float4& p) {
    bool hit;
    const uint64_t key = nrm_key(qx, qy, qz, p, r2, valid, hit);
    const uint64_t m = wave_ballot(hit);
    if (hit) {
      const int slot = cnt + mbcnt_lt(m);
      if (slot < max_nn) sel[slot] = p;
      atomicAdd(&hist[static_cast<uint32_t>(key >> 56)], 1u);
    }
    cnt += __popcll(m);
  });
  int k = cnt;
  if (cnt > max_nn) {
    // radix select: the smallest limit such that exactly max_nn hits have key < limit
    uint64_t prefix = 0, limit = 0;
    int need = max_nn;
    for (int shift = 56;; shift -= 8) {
      if (shift < 56) {
        wave_sync();
#pragma unroll
        for (int u = 0; u < 4; ++u) hist[4 * lane + u] = 0u;
        wave_sync();
        nrm_candidates(c, cell_start, sorted, qx, qy, qz, [&](bool valid, const float4& p) {
          bool hit;
          const uint64_t key = nrm_key(qx, qy, qz, p, r2, valid, hit);
          if (hit && (key >> (shift + 8)) == prefix) atomicAdd(&hist[static_cast<uint32_t>(key >> shift) & 255u], 1u);
        });
      }
      wave_sync();
      uint32_t hb[4], local = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        hb[u] = hist[4 * lane + u];
        local += hb[u];
      }
      uint32_t incl = local;                                    // inclusive scan of the per-lane sums
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
      }
      uint32_t before = incl - local;
      int dig = -1;
      uint32_t below = 0, inbin = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (dig < 0 && before < static_cast<uint32_t>(need) && static_cast<uint32_t>(need) <= before + hb[u]) {
          dig = 4 * lane + u;
          below = before;
          inbin = hb[u];
        }
        before += hb[u];
      }
      const int src = __builtin_ctzll(wave_ballot(dig >= 0));
      dig = __shfl(dig, src);
      below = __shfl(below, src);
      inbin = __shfl(inbin, src);
      const uint64_t pd = (prefix << 8) | static_cast<uint64_t>(dig);
      if (inbin == static_cast<uint32_t>(need) - below) {       // the whole bin is taken (always so at shift 0: keys are distinct)
        limit = (pd + 1) << shift;
        break;
      }
      prefix = pd;
      need -= static_cast<int>(below);
    }
    int base = 0;
    nrm_candidates(c, cell_start, sorted, qx, qy, qz, [&](bool valid, const float4& p) {
      bool hit;
      const uint64_t key = nrm_key(qx, qy, qz, p, r2, valid, hit);
      const bool take = hit && key < limit;
      const uint64_t m = wave_ballot(take);
      const int slot = base + mbcnt_lt(m);
      if (take && slot < max_nn) sel[slot] = p;                   // exactly max_nn keys lie below the limit
      base += __popcll(m);
    });
    k = max_nn;
  }
  wave_sync();
  // rank by row and place: lane l then sums ranks l and l + 64, in that order
  const int e1 = lane + 64 < NRM_MAX_NN ? lane + 64 : NRM_MAX_NN - 1;
  const uint32_t row0 = __float_as_uint(sel[lane].w), row1 = __float_as_uint(sel[e1].w);
  int rk0 = 0, rk1 = 0;
  for (int j = 0; j < k; ++j) {
    const uint32_t rj = __float_as_uint(sel[j].w);
    rk0 += rj < row0 ? 1 : 0;
    rk1 += rj < row1 ? 1 : 0;
  }
  if (lane < k) ord[rk0] = sel[lane];
  if (lane + 64 < k) ord[rk1] = sel[e1];
  wave_sync();
  double m[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) m[j] = 0.0;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = lane + 64 * u;
    if (e < k) {
      const float4 p = ord[e];
      const double d[3] = {static_cast<double>(p.x) - static_cast<double>(qx), static_cast<double>(p.y) - static_cast<double>(qy),
                           static_cast<double>(p.z) - static_cast<double>(qz)};
      m[0] = dadd(m[0], d[0]);
      m[1] = dadd(m[1], d[1]);
      m[2] = dadd(m[2], d[2]);
      m[3] = dadd(m[3], dmul(d[0], d[0]));
      m[4] = dadd(m[4], dmul(d[0], d[1]));
      m[5] = dadd(m[5], dmul(d[0], d[2]));
      m[6] = dadd(m[6], dmul(d[1], d[1]));
      m[7] = dadd(m[7], dmul(d[1], d[2]));
      m[8] = dadd(m[8], dmul(d[2], d[2]));
    }
  }
#pragma unroll
  for (int j = 0; j < 9; ++j)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m[j] = dadd(m[j], __shfl_xor(m[j], d));
  if (lane == 0) {
    cnt_out[i] = k;
    double* o = cov + 6 * i;
    if (k > 0) {
      const double kk = static_cast<double>(k);
      const double mu[3] = {m[0] / kk, m[1] / kk, m[2] / kk};
      o[0] = m[3] / kk - dmul(mu[0], mu[0]);
      o[1] = m[4] / kk - dmul(mu[0], mu[1]);
      o[2] = m[5] / kk - dmul(mu[0], mu[2]);
      o[3] = m[6] / kk - dmul(mu[1], mu[1]);
      o[4] = m[7] / kk - dmul(mu[1], mu[2]);
      o[5] = m[8] / kk - dmul(mu[2], mu[2]);
    } else {
      for (int j = 0; j < 6; ++j) o[j] = 0.0;
    }
  }
}

// one thread per row: eigen-solve, degeneracy, orientation toward the viewpoint
__global__ __launch_bounds__(256) void k_normals_finish(Stack C, const float* __restrict__ pts, const float* __restrict__ viewpoint,
                                                        const double* __restrict__ cov, const int32_t* __restrict__ cnt, float* __restrict__ normals,
                                                        float* __restrict__ curvature, int32_t* __restrict__ count) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= C.off[C.B]) return;
  const int k = cnt[i];
  if (count) count[i] = k;
  double n[3] = {0.0, 0.0, 0.0}, curv = 0.0;
  if (k >= 3) {
    const double* o = cov + 6 * i;
    const double A[3][3] = {{o[0], o[1], o[2]}, {o[1], o[3], o[4]}, {o[2], o[4], o[5]}};
    double lam[3], V[3][3];
    sym3_eigen(A, lam, V);
    if (!(lam[2] <= 1e-30 || lam[1] <= 1e-12 * lam[2])) {
      const double nr = sqrt(V[0][0] * V[0][0] + V[1][0] * V[1][0] + V[2][0] * V[2][0]);
      for (int r = 0; r < 3; ++r) n[r] = V[r][0] / nr;
      const int b = cloud_of(C.off, C.B, i);
      double v[3] = {0.0, 0.0, 0.0};
      if (viewpoint)
        for (int r = 0; r < 3; ++r) v[r] = viewpoint[3 * b + r];
      const double w[3] = {v[0] - static_cast<double>(pts[3 * i]), v[1] - static_cast<double>(pts[3 * i + 1]),
                           v[2] - static_cast<double>(pts[3 * i + 2])};
      const double dot = dadd(dadd(dmul(n[0], w[0]), dmul(n[1], w[1])), dmul(n[2], w[2]));
      // dot == 0 (the viewpoint in the tangent plane): the first non-zero component of n is made positive
      const double lead = n[0] != 0.0 ? n[0] : (n[1] != 0.0 ? n[1] : n[2]);
      if (dot < 0.0 || (dot == 0.0 && lead < 0.0))
        for (int r = 0; r < 3; ++r) n[r] = -n[r];
      curv = lam[0] / dadd(dadd(lam[0], lam[1]), lam[2]);
    }
  }
  for (int r = 0; r < 3; ++r) normals[3 * i + r] = static_cast<float>(n[r]);
  if (curvature) curvature[i] = static_cast<float>(curv);
}

}  // namespace lcr

using namespace lcr;

namespace {

size_t normals_layout(void* ws, int B, int64_t n, size_t grid_bytes, double** cov, int32_t** cnt, int64_t** len) {
  Carver c(ws, ~size_t(0));
  c.take<char>(grid_bytes);                                      // the support grid, at the workspace base
  double* cv = c.take<double>(static_cast<size_t>(n > 0 ? n : 1) * 6);
  int32_t* ct = c.take<int32_t>(n > 0 ? n : 1);
  int64_t* ln = c.take<int64_t>(B);
  if (cov) {
    *cov = cv;
    *cnt = ct;
    *len = ln;
  }
  return c.off;
}

}  // namespace

extern "C" int lcr_normals_ws_bytes(int B, int64_t n, size_t* bytes) {
  if (!bytes || B < 1 || B > GRID_MAX_B || n < 0 || n > INT32_MAX)
    return refuse(LCR_EARG, "lcr_normals_ws_bytes: outside the domain (1 <= B <= %d, 0 <= n <= 2^31-1): B=%d n=%lld", GRID_MAX_B, B, static_cast<long long>(n));
  size_t g = 0;
  if (int rc = support_grid_ws_bytes("lcr_normals_ws_bytes", n, B, &g)) return rc;
  *bytes = normals_layout(nullptr, B, n, g, nullptr, nullptr, nullptr);
  return LCR_OK;
}

extern "C" int lcr_estimate_normals(const float* points, const int64_t* lengths, int B, float radius, int max_nn, const float* viewpoint,
                                    float* normals, float* curvature, int32_t* count, void* ws, size_t ws_bytes, void* stream) {
  if (!(radius > 0.f) || !std::isfinite(radius * radius) || max_nn < 1 || max_nn > NRM_MAX_NN)
    return refuse(LCR_EARG, "lcr_estimate_normals: outside the domain (radius > 0 with radius*radius finite, 1 <= max_nn <= %d): radius=%g max_nn=%d",
                  NRM_MAX_NN, static_cast<double>(radius), max_nn);
  Stack C;
  if (int rc = stack_from_lengths("lcr_estimate_normals", lengths, B, &C)) return rc;
  const int64_t n = C.off[B];
  if (!ws || (n > 0 && (!points || !normals)))
    return refuse(LCR_EARG, "lcr_estimate_normals: null workspace, or a null point / normal array (n=%lld)", static_cast<long long>(n));
  size_t need = 0, grid_bytes = 0;
  lcr_normals_ws_bytes(B, n, &need);
  support_grid_ws_bytes("lcr_estimate_normals", n, B, &grid_bytes);
  if (need > ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_estimate_normals", ws_bytes, need);
  if (n == 0) return LCR_OK;
  double* cov;
  int32_t* cnt;
  int64_t* len_dev;
  normals_layout(ws, B, n, grid_bytes, &cov, &cnt, &len_dev);
  const GridLayout L = grid_layout(ws, n, B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = stack_to_device("lcr_estimate_normals", C, len_dev, nullptr, nullptr, st);
  if (rc) return rc;
  rc = support_grid_build("lcr_estimate_normals", points, len_dev, B, n, radius, nullptr, ws, grid_bytes, nullptr, stream);
  if (rc) return rc;
  const float r2 = radius * radius;                              // fp32 product, as lcr_radius_query
  hipLaunchKernelGGL(k_normals_cov, dim3(div_up(n, NRM_WAVES)), dim3(NRM_WAVES * 64), 0, st, C, points, L.hdr, L.cell_start, L.sorted, r2, max_nn,
                     cov, cnt);
  hipLaunchKernelGGL(k_normals_finish, dim3(div_up(n, 256)), dim3(256), 0, st, C, points, viewpoint, cov, cnt, normals, curvature, count);
  return check_launch("lcr_estimate_normals");
}
