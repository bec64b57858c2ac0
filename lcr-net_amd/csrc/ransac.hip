// ransac.hip — correspondence RANSAC (utils/utils/open3d.py:145-173: Open3D's registration_ransac_based_on_correspondence with
// point-to-point estimation without scaling and RANSACConvergenceCriteria(N, N), i.e. every iteration runs), batched over pairs and
// made deterministic.  The semantics (sampler, hypothesis, score, selection) are stated in include/lcr_hip.h next to the entry points.
//
// Three stream-ordered launches per call, no host synchronisation, no allocation:
//   k_ransac_hyp     one thread per (pair, hypothesis): counter-based sample, fp64 Kabsch (rigid3.h), 12 floats + a valid flag;
//   k_ransac_score   the hot path.  One wavefront owns 64 hypotheses of one pair, one per lane, its transform in registers, and streams the
//                    pair's correspondences through LDS; every lane reads the same LDS address (a broadcast, no bank conflict).  Per
//                    (hypothesis, correspondence): 9 FMA for R s + t, 3 subtracts, 1 mul + 2 FMA for d², a compare and two accumulates —
//                    VALU-issue bound, nothing else close (DESIGN.md "Correspondence RANSAC").  Each wavefront writes its best candidate;
//   k_ransac_select  one workgroup per pair reduces the candidates in the total order (count desc, SSE asc, h asc).
// lcr_ransac_correspondences_ex adds Open3D's correspondence checkers (edge length before the fit, distance after it; k_ransac_hyp) and,
// when one of them is on, k_ransac_compact: one workgroup per pair lists the surviving hypotheses in ascending h (ballot + prefix), and
// k_ransac_score gives its lanes to that list, so that a rejected hypothesis never streams a correspondence.  Its index form (corr rows
// into the pairs' point clouds) is a gather kernel of its own in front (k_ransac_gather): everything after it sees today's layout.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"
#include "rigid3.h"

namespace lcr {

constexpr int RS_TILE = 64;       // hypotheses per scoring workgroup (one wavefront, one hypothesis per lane)
constexpr int RS_CHUNK = 128;     // correspondences per LDS chunk (4 KB: two float4 per correspondence; 16 KB would cap a CU at 10 waves)
constexpr int RS_MAX_N = 8;       // largest ransac_n
constexpr int RS_HYP = 16;        // floats per stored hypothesis: R|t row-major [12], valid flag [12], pad

// Draw j of hypothesis h: SplitMix64 of seed + golden * (1 + 8h + j), mapped to [0, n) by multiply-shift on the high 32 bits.
__host__ __device__ inline uint32_t ransac_draw(uint64_t seed, int64_t h, int j, uint32_t n) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * static_cast<uint64_t>(1 + 8 * h + j);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return static_cast<uint32_t>(((z >> 32) * static_cast<uint64_t>(n)) >> 32);
}

// total order of candidates: more inliers, then smaller SSE, then smaller hypothesis index
__device__ __forceinline__ bool rs_better(int c1, float s1, int h1, int c2, float s2, int h2) {
  return c1 > c2 || (c1 == c2 && (s1 < s2 || (s1 == s2 && h1 < h2)));
}

__device__ __forceinline__ void rs_wave_best(int& c, float& s, int& h) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int oc = __shfl_xor(c, d), oh = __shfl_xor(h, d);
    const float os = __shfl_xor(s, d);
    if (rs_better(oc, os, oh, c, s, h)) {
      c = oc;
      s = os;
      h = oh;
    }
  }
}

// one thread per (pair blockIdx.y, hypothesis h): hyp[(s * iters + h) * 16 + 0..11] = R|t, [12] = 1 valid / 0 invalid (R = I, t = 0)
// edge_k2 > 0: the edge-length check (before the fit); check_d2 > 0: the distance check (after it, on the stored fp32 transform); reject
// (nullable): 0 valid, 1 degenerate, 2 edge, 3 distance.  checked: counts_all / sse_all of the invalid hypotheses are written here (-1, 0),
// because the compacted scoring pass never visits them.
__global__ __launch_bounds__(256) void k_ransac_hyp(const float* __restrict__ src, const float* __restrict__ ref, const int32_t* __restrict__ start,
                                                    int iters, int rn, uint64_t seed, float edge_k2, float check_d2, bool checked,
                                                    float* __restrict__ hyp, float* __restrict__ T_all, uint8_t* __restrict__ reject,
                                                    int32_t* __restrict__ counts_all, float* __restrict__ sse_all) {
  const int s = blockIdx.y;
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= iters) return;
  const int a = start[s], n = start[s + 1] - a;
  const int64_t g = static_cast<int64_t>(s) * iters + h;
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, t[3] = {0, 0, 0};
  bool ok = false;
  int code = 1;
  bool edge_ok = true;
  if (n >= rn && edge_k2 > 0.f) {                         // CorrespondenceCheckerBasedOnEdgeLength on the fp32 rows, squared lengths
    float fs[RS_MAX_N][3], fr[RS_MAX_N][3];
#pragma unroll
    for (int j = 0; j < RS_MAX_N; ++j)
      if (j < rn) {
        const int64_t i = a + static_cast<int64_t>(ransac_draw(seed, h, j, static_cast<uint32_t>(n)));
        for (int d = 0; d < 3; ++d) {
          fs[j][d] = src[3 * i + d];
          fr[j][d] = ref[3 * i + d];
        }
      }
#pragma unroll
    for (int j = 0; j < RS_MAX_N; ++j)
#pragma unroll
      for (int k = j + 1; k < RS_MAX_N; ++k)
        if (k < rn) {
          const float sx = fsub(fs[j][0], fs[k][0]), sy = fsub(fs[j][1], fs[k][1]), sz = fsub(fs[j][2], fs[k][2]);
          const float rx = fsub(fr[j][0], fr[k][0]), ry = fsub(fr[j][1], fr[k][1]), rz = fsub(fr[j][2], fr[k][2]);
          const float ls2 = fadd(fadd(fmul(sx, sx), fmul(sy, sy)), fmul(sz, sz));
          const float lr2 = fadd(fadd(fmul(rx, rx), fmul(ry, ry)), fmul(rz, rz));
          edge_ok = edge_ok && ls2 >= fmul(edge_k2, lr2) && lr2 >= fmul(edge_k2, ls2);
        }
    if (!edge_ok) code = 2;
  }
  if (n >= rn && edge_ok) {
    double ps[RS_MAX_N][3], pr[RS_MAX_N][3], cs[3] = {0, 0, 0}, cr[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < RS_MAX_N; ++j) {
      if (j < rn) {
        const int64_t i = a + static_cast<int64_t>(ransac_draw(seed, h, j, static_cast<uint32_t>(n)));
        for (int d = 0; d < 3; ++d) {
          ps[j][d] = src[3 * i + d];
          pr[j][d] = ref[3 * i + d];
          cs[d] += ps[j][d];
          cr[d] += pr[j][d];
        }
      }
    }
    for (int d = 0; d < 3; ++d) {
      cs[d] /= rn;
      cr[d] /= rn;
    }
    double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int j = 0; j < RS_MAX_N; ++j)
      if (j < rn)
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) H[r][c] += (ps[j][r] - cs[r]) * (pr[j][c] - cr[c]);
    double Rf[3][3], sv[3];
    rotation_from_H_sv(H, Rf, sv);
    ok = !(sv[0] <= 1e-30 || sv[1] <= 1e-9 * sv[0]);       // coincident or collinear sample: never selected
    if (ok) {
      for (int r = 0; r < 3; ++r) {
        t[r] = cr[r];
        for (int c = 0; c < 3; ++c) {
          R[r][c] = Rf[r][c];
          t[r] -= Rf[r][c] * cs[c];
        }
      }
      if (check_d2 > 0.f) {                               // CorrespondenceCheckerBasedOnDistance: the scoring rule on the sampled rows
        float m[12];
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c) m[4 * r + c] = static_cast<float>(R[r][c]);
          m[4 * r + 3] = static_cast<float>(t[r]);
        }
#pragma unroll
        for (int j = 0; j < RS_MAX_N; ++j)
          if (j < rn) {
            const float px = static_cast<float>(ps[j][0]), py = static_cast<float>(ps[j][1]), pz = static_cast<float>(ps[j][2]);
            const float dx = fmaf(m[2], pz, fmaf(m[1], py, fmaf(m[0], px, m[3]))) - static_cast<float>(pr[j][0]);
            const float dy = fmaf(m[6], pz, fmaf(m[5], py, fmaf(m[4], px, m[7]))) - static_cast<float>(pr[j][1]);
            const float dz = fmaf(m[10], pz, fmaf(m[9], py, fmaf(m[8], px, m[11]))) - static_cast<float>(pr[j][2]);
            ok = ok && fmaf(dz, dz, fmaf(dy, dy, dx * dx)) < check_d2;
          }
        if (!ok) {
          code = 3;
          for (int r = 0; r < 3; ++r) {
            t[r] = 0;
            for (int c = 0; c < 3; ++c) R[r][c] = r == c ? 1 : 0;
          }
        }
      }
    }
  }
  if (ok) code = 0;
  if (reject) reject[g] = static_cast<uint8_t>(code);
  if (checked && !ok) {
    if (counts_all) counts_all[g] = -1;
    if (sse_all) sse_all[g] = 0.f;
  }
  float* o = hyp + RS_HYP * g;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) o[4 * r + c] = static_cast<float>(R[r][c]);
    o[4 * r + 3] = static_cast<float>(t[r]);
  }
  o[12] = ok ? 1.f : 0.f;
  if (T_all) {
    float* q = T_all + 16 * g;
    for (int k = 0; k < 12; ++k) q[k] = o[k];
    q[12] = q[13] = q[14] = 0.f;
    q[15] = 1.f;
  }
}

// one workgroup per pair: surv[s * iters + k] = the k-th valid hypothesis in ascending h, nsurv[s] = their number
__global__ __launch_bounds__(256) void k_ransac_compact(const float* __restrict__ hyp, int iters, int32_t* __restrict__ surv,
                                                        int32_t* __restrict__ nsurv) {
  __shared__ int s_w[4];
  const int s = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  const int64_t g0 = static_cast<int64_t>(s) * iters;
  int base = 0;
  for (int h0 = 0; h0 < iters; h0 += 256) {               // block-uniform trip count
    const int h = h0 + tid;
    const bool keep = h < iters && hyp[RS_HYP * (g0 + h) + 12] != 0.f;
    const uint64_t m = wave_ballot(keep);
    __syncthreads();
    if ((tid & 63) == 0) s_w[w] = __popcll(m);
    __syncthreads();
    int off = base + mbcnt_lt(m);
    for (int k = 0; k < w; ++k) off += s_w[k];
    if (keep) surv[g0 + off] = h;
    base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
  }
  if (tid == 0) nsurv[s] = base;
}

// index form: row i of pair s (start[s] <= i < start[s+1]) = (cloud_src[src_start[s] + corr[i][0]], cloud_ref[ref_start[s] + corr[i][1]]);
// an index outside its cloud is not read: the row becomes NaN, which is an inlier of no hypothesis and gives a hypothesis no inlier
__global__ __launch_bounds__(256) void k_ransac_gather(const float* __restrict__ csrc, const float* __restrict__ cref, const int32_t* __restrict__ corr,
                                                       const int32_t* __restrict__ start, const int32_t* __restrict__ src_start,
                                                       const int32_t* __restrict__ ref_start, int S, int64_t cap, float* __restrict__ gs,
                                                       float* __restrict__ gr) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= cap || i >= start[S]) return;
  int lo = 0, hi = S - 1;                                 // the last s with start[s] <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const int a = corr[2 * i], b = corr[2 * i + 1];
  const int ns = src_start[lo + 1] - src_start[lo], nr = ref_start[lo + 1] - ref_start[lo];
  const float nan = __uint_as_float(0x7fc00000u);
  for (int d = 0; d < 3; ++d) {
    gs[3 * i + d] = a >= 0 && a < ns ? csrc[3 * (static_cast<int64_t>(src_start[lo]) + a) + d] : nan;
    gr[3 * i + d] = b >= 0 && b < nr ? cref[3 * (static_cast<int64_t>(ref_start[lo]) + b) + d] : nan;
  }
}

// one wavefront per (tile blockIdx.x of 64 hypotheses, pair blockIdx.y); writes the tile's best (count, sse, h) candidate.
// surv != nullptr: the tile's lanes take the pair's surviving hypotheses surv[s * iters + tile * 64 + lane] (all valid) instead of h itself
__global__ __launch_bounds__(RS_TILE) void k_ransac_score(const float* __restrict__ src, const float* __restrict__ ref, const int32_t* __restrict__ start,
                                                          int iters, float thr2, const float* __restrict__ hyp, int32_t* __restrict__ cand_count,
                                                          float* __restrict__ cand_sse, int32_t* __restrict__ cand_h, int32_t* __restrict__ counts_all,
                                                          float* __restrict__ sse_all, const int32_t* __restrict__ surv,
                                                          const int32_t* __restrict__ nsurv) {
  __shared__ float4 sh[2 * RS_CHUNK];
  const int s = blockIdx.y, lane = threadIdx.x;
  int h = blockIdx.x * RS_TILE + lane;
  bool live = h < iters;
  if (surv) {
    live = h < nsurv[s];
    h = live ? surv[static_cast<int64_t>(s) * iters + h] : INT_MAX;
  }
  const int a = start[s], n = start[s + 1] - a;
  const int64_t g = static_cast<int64_t>(s) * iters + (live ? h : 0);
  float m[12];
  const float4* hv = reinterpret_cast<const float4*>(hyp + RS_HYP * g);
  const float4 m0 = hv[0], m1 = hv[1], m2 = hv[2], m3 = hv[3];
  m[0] = m0.x, m[1] = m0.y, m[2] = m0.z, m[3] = m0.w;
  m[4] = m1.x, m[5] = m1.y, m[6] = m1.z, m[7] = m1.w;
  m[8] = m2.x, m[9] = m2.y, m[10] = m2.z, m[11] = m2.w;
  const bool valid = live && m3.x != 0.f;
  int cnt = 0;
  float sse = 0.f;
  if (wave_ballot(valid) != 0) {                         // wave-uniform: pairs without a valid hypothesis skip the stream
    for (int c0 = 0; c0 < n; c0 += RS_CHUNK) {
      const int cn = min(RS_CHUNK, n - c0);
      __syncthreads();
      for (int k = lane; k < cn; k += RS_TILE) {
        const int64_t i = a + static_cast<int64_t>(c0 + k);
        sh[2 * k] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], ref[3 * i]);
        sh[2 * k + 1] = make_float4(ref[3 * i + 1], ref[3 * i + 2], 0.f, 0.f);
      }
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < cn; ++k) {
        const float4 p = sh[2 * k], q = sh[2 * k + 1];
        const float dx = fmaf(m[2], p.z, fmaf(m[1], p.y, fmaf(m[0], p.x, m[3]))) - p.w;
        const float dy = fmaf(m[6], p.z, fmaf(m[5], p.y, fmaf(m[4], p.x, m[7]))) - q.x;
        const float dz = fmaf(m[10], p.z, fmaf(m[9], p.y, fmaf(m[8], p.x, m[11]))) - q.y;
        const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const bool in = d2 < thr2;
        cnt += in ? 1 : 0;
        sse += in ? d2 : 0.f;
      }
    }
  }
  if (!valid) {
    cnt = -1;
    sse = 0.f;
  }
  if (live && counts_all) counts_all[g] = cnt;
  if (live && sse_all) sse_all[g] = sse;
  int bc = live ? cnt : INT_MIN, bh = live ? h : INT_MAX;
  float bs = sse;
  rs_wave_best(bc, bs, bh);
  if (lane == 0) {
    const int64_t o = static_cast<int64_t>(s) * gridDim.x + blockIdx.x;
    cand_count[o] = bc;
    cand_sse[o] = bs;
    cand_h[o] = bh;
  }
}

// one workgroup per pair: best of the pair's `tiles` candidates; a winner needs at least one inlier (else identity, 0 inliers, best_h -1)
__global__ __launch_bounds__(256) void k_ransac_select(const float* __restrict__ hyp, int iters, int tiles, const int32_t* __restrict__ cand_count,
                                                       const float* __restrict__ cand_sse, const int32_t* __restrict__ cand_h, float* __restrict__ T,
                                                       int32_t* __restrict__ inliers, float* __restrict__ rmse, int32_t* __restrict__ best_h) {
  __shared__ int s_c[4], s_h[4];
  __shared__ float s_s[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  int bc = INT_MIN, bh = INT_MAX;
  float bs = 0.f;
  for (int k = tid; k < tiles; k += blockDim.x) {
    const int64_t o = static_cast<int64_t>(s) * tiles + k;
    const int c = cand_count[o], h = cand_h[o];
    const float e = cand_sse[o];
    if (rs_better(c, e, h, bc, bs, bh)) {
      bc = c;
      bs = e;
      bh = h;
    }
  }
  rs_wave_best(bc, bs, bh);
  if ((tid & 63) == 0) {
    s_c[tid >> 6] = bc;
    s_s[tid >> 6] = bs;
    s_h[tid >> 6] = bh;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < static_cast<int>(blockDim.x >> 6); ++w)
    if (rs_better(s_c[w], s_s[w], s_h[w], bc, bs, bh)) {
      bc = s_c[w];
      bs = s_s[w];
      bh = s_h[w];
    }
  float* o = T + 16 * s;
  if (bc >= 1) {
    const float* m = hyp + RS_HYP * (static_cast<int64_t>(s) * iters + bh);
    for (int k = 0; k < 12; ++k) o[k] = m[k];
    inliers[s] = bc;
    rmse[s] = sqrtf(bs / static_cast<float>(bc));
    if (best_h) best_h[s] = bh;
  } else {
    for (int k = 0; k < 12; ++k) o[k] = (k % 5 == 0) ? 1.f : 0.f;
    inliers[s] = 0;
    rmse[s] = 0.f;
    if (best_h) best_h[s] = -1;
  }
  o[12] = o[13] = o[14] = 0.f;
  o[15] = 1.f;
}

}  // namespace lcr

using namespace lcr;

static int ransac_domain(int S, int ransac_n, int iterations, const char* what) {
  if (S < 1 || S > 65535 || ransac_n < 3 || ransac_n > RS_MAX_N || iterations < 1 || iterations > 1000000)
    return refuse(LCR_EARG, "%s: outside the domain (1 <= S <= 65535, 3 <= ransac_n <= 8, 1 <= iterations <= 1e6): S=%d ransac_n=%d iterations=%d", what, S,
                  ransac_n, iterations);
  return LCR_OK;
}

extern "C" int lcr_ransac_sample_host(uint64_t seed, int64_t h0, int64_t count, int ransac_n, int64_t n, int32_t* idx_host) {
  if (!idx_host || h0 < 0 || count < 0 || h0 + count > 1000000 || ransac_n < 1 || ransac_n > RS_MAX_N || n < 1 || n > INT32_MAX)
    return refuse(LCR_EARG, "lcr_ransac_sample_host: bad argument (h0=%lld count=%lld ransac_n=%d n=%lld)", static_cast<long long>(h0),
                  static_cast<long long>(count), ransac_n, static_cast<long long>(n));
  for (int64_t k = 0; k < count; ++k)
    for (int j = 0; j < ransac_n; ++j) idx_host[k * ransac_n + j] = static_cast<int32_t>(ransac_draw(seed, h0 + k, j, static_cast<uint32_t>(n)));
  return LCR_OK;
}

// workspace layout shared by the two entries: the old one has no survivor list and no gathered rows
static size_t ransac_carve(Carver& c, int S, int iterations, bool checked, int64_t n_gather, float** hyp, int32_t** cc, float** cs, int32_t** ch,
                           int32_t** surv, int32_t** nsurv, float** gs, float** gr) {
  const size_t tiles = static_cast<size_t>(div_up(iterations, RS_TILE));
  float* a = c.take<float>(static_cast<size_t>(S) * iterations * RS_HYP);   // hypotheses + valid flags
  int32_t* b = c.take<int32_t>(S * tiles);                                  // per-tile best count
  float* d = c.take<float>(S * tiles);                                      // its SSE
  int32_t* e = c.take<int32_t>(S * tiles);                                  // its hypothesis index
  int32_t* f = checked ? c.take<int32_t>(static_cast<size_t>(S) * iterations) : nullptr;   // surviving hypotheses per pair, ascending h
  int32_t* g = checked ? c.take<int32_t>(static_cast<size_t>(S)) : nullptr;
  float* p = n_gather > 0 ? c.take<float>(3 * static_cast<size_t>(n_gather)) : nullptr;    // index form: the gathered rows
  float* q = n_gather > 0 ? c.take<float>(3 * static_cast<size_t>(n_gather)) : nullptr;
  if (hyp) *hyp = a, *cc = b, *cs = d, *ch = e, *surv = f, *nsurv = g, *gs = p, *gr = q;
  return c.off;
}

extern "C" int lcr_ransac_ws_bytes(int S, int iterations, size_t* bytes) {
  if (!bytes) return refuse(LCR_EARG, "lcr_ransac_ws_bytes: null pointer");
  if (int rc = ransac_domain(S, RS_MAX_N, iterations, "lcr_ransac_ws_bytes")) return rc;
  Carver c(nullptr, ~size_t(0));
  *bytes = ransac_carve(c, S, iterations, false, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  return LCR_OK;
}

extern "C" int lcr_ransac_ex_ws_bytes(int S, int iterations, int64_t n_corr, size_t* bytes) {
  if (!bytes) return refuse(LCR_EARG, "lcr_ransac_ex_ws_bytes: null pointer");
  if (int rc = ransac_domain(S, RS_MAX_N, iterations, "lcr_ransac_ex_ws_bytes")) return rc;
  if (n_corr < 0 || n_corr > INT32_MAX) return refuse(LCR_EARG, "lcr_ransac_ex_ws_bytes: n_corr outside 0..2^31-1 (%lld)", static_cast<long long>(n_corr));
  Carver c(nullptr, ~size_t(0));
  *bytes = ransac_carve(c, S, iterations, true, n_corr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  return LCR_OK;
}

static int ransac_run(const char* what, const float* src, const float* ref, const int32_t* start, int S, const int32_t* corr,
                      const int32_t* src_start, const int32_t* ref_start, int64_t n_corr, float thr, int ransac_n, int iterations, uint64_t seed,
                      float edge_similarity, float checker_distance, float* T, int32_t* inliers, float* rmse, int32_t* best_h, float* T_all,
                      int32_t* counts_all, float* sse_all, uint8_t* reject_all, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = ransac_domain(S, ransac_n, iterations, what)) return rc;
  if (!src || !ref || !start || !T || !inliers || !rmse || !ws || !(thr > 0.f) || !std::isfinite(thr) || !std::isfinite(thr * thr))
    return refuse(LCR_EARG, "%s: null pointer or distance threshold not finite and > 0 (thr=%g)", what, static_cast<double>(thr));
  const float edge_k2 = edge_similarity > 0.f ? edge_similarity * edge_similarity : 0.f;
  const float check_d2 = checker_distance > 0.f ? checker_distance * checker_distance : 0.f;
  if (std::isnan(edge_similarity) || std::isnan(checker_distance) || !std::isfinite(edge_k2) || !std::isfinite(check_d2) ||
      (corr && (!src_start || !ref_start || n_corr < 0 || n_corr > INT32_MAX)))
    return refuse(LCR_EARG, "%s: checker parameter not finite when squared (edge_similarity=%g checker_distance=%g), or the index form without "
                  "src_start / ref_start or with n_corr outside 0..2^31-1", what, static_cast<double>(edge_similarity),
                  static_cast<double>(checker_distance));
  const bool checked = edge_k2 > 0.f || check_d2 > 0.f;
  const int64_t n_gather = corr ? n_corr : 0;
  float *hyp, *cs, *gs, *gr;
  int32_t *cc, *ch, *surv, *nsurv;
  Carver c(ws, ws_bytes);
  const size_t need = ransac_carve(c, S, iterations, checked, n_gather, &hyp, &cc, &cs, &ch, &surv, &nsurv, &gs, &gr);
  if (need > ws_bytes) return refuse_ws(LCR_ESPACE, what, ws_bytes, need);
  const int tiles = div_up(iterations, RS_TILE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_gather > 0) {
    hipLaunchKernelGGL(k_ransac_gather, dim3(div_up(n_gather, 256)), dim3(256), 0, st, src, ref, corr, start, src_start, ref_start, S, n_gather, gs,
                       gr);
    src = gs;
    ref = gr;
  }
  hipLaunchKernelGGL(k_ransac_hyp, dim3(div_up(iterations, 256), S), dim3(256), 0, st, src, ref, start, iterations, ransac_n, seed, edge_k2, check_d2,
                     checked, hyp, T_all, reject_all, counts_all, sse_all);
  if (checked) hipLaunchKernelGGL(k_ransac_compact, dim3(S), dim3(256), 0, st, hyp, iterations, surv, nsurv);
  hipLaunchKernelGGL(k_ransac_score, dim3(tiles, S), dim3(RS_TILE), 0, st, src, ref, start, iterations, thr * thr, hyp, cc, cs, ch, counts_all, sse_all,
                     checked ? surv : nullptr, checked ? nsurv : nullptr);
  hipLaunchKernelGGL(k_ransac_select, dim3(S), dim3(256), 0, st, hyp, iterations, tiles, cc, cs, ch, T, inliers, rmse, best_h);
  return check_launch(what);
}

extern "C" int lcr_ransac_correspondences_ex(const float* src, const float* ref, const int32_t* start, int S, const int32_t* corr,
                                             const int32_t* src_start, const int32_t* ref_start, int64_t n_corr, float thr, int ransac_n,
                                             int iterations, uint64_t seed, float edge_similarity, float checker_distance, float* T,
                                             int32_t* inliers, float* rmse, int32_t* best_h, float* T_all, int32_t* counts_all, float* sse_all,
                                             uint8_t* reject_all, void* ws, size_t ws_bytes, void* stream) {
  return ransac_run("lcr_ransac_correspondences_ex", src, ref, start, S, corr, src_start, ref_start, n_corr, thr, ransac_n, iterations, seed,
                    edge_similarity, checker_distance, T, inliers, rmse, best_h, T_all, counts_all, sse_all, reject_all, ws, ws_bytes, stream);
}

extern "C" int lcr_ransac_correspondences(const float* src, const float* ref, const int32_t* start, int S, float thr, int ransac_n, int iterations,
                                          uint64_t seed, float* T, int32_t* inliers, float* rmse, int32_t* best_h, float* T_all, int32_t* counts_all,
                                          float* sse_all, void* ws, size_t ws_bytes, void* stream) {
  return ransac_run("lcr_ransac_correspondences", src, ref, start, S, nullptr, nullptr, nullptr, 0, thr, ransac_n, iterations, seed, 0.f, 0.f, T,
                    inliers, rmse, best_h, T_all, counts_all, sse_all, nullptr, ws, ws_bytes, stream);
}
