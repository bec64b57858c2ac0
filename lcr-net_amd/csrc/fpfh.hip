// fpfh.hip — FPFH descriptors (Open3D's compute_fpfh_feature with KDTreeSearchParamHybrid(radius, max_nn): the 33-bin hand-crafted feature
// registration_ransac_based_on_feature_matching is documented with) for B stacked clouds in one call, exact in its votes and
// batch-invariant.  Semantics in include/lcr_hip.h (lcr_fpfh).
//
// Per call: stack_to_device (cloud lengths to the device), the support grid and the ordered query of radius_search.hip with limit = max_nn
// into an int32 [N, max_nn] table in the workspace (global rows, padded with N), then
//   k_spfh   one wavefront per row.  Lane l takes ranks l and l + 64 of the row's list, drops the row itself and the padding, computes the
//            Darboux pair features in fp64 (two divisions, two square roots and one atan2 per pair) and votes into a 33-entry LDS integer
//            histogram.  Integer votes: the SPFH row, votes * 100 / m, depends on no order.  Writes SPFH as fp64 into the workspace.
//   k_fpfh   one wavefront per row.  The row's usable neighbours (d2 != 0) are compacted in list order into LDS; lane j < 33 owns bin j and
//            walks the list serially, acc_j += spfh(nb, j) / d2(nb): each step is one coalesced 264-byte read of a neighbour's SPFH row, the
//            order of the sum is the list's own, and no cross-lane reduction is needed at all.  Loads are issued four neighbours ahead of
//            the dependent fp64 division chain.  The three block sums are taken from LDS in ascending bin order.
// d2 is recomputed with grid_d2 (grid.h), so it has the bits the search compared.
#include <climits>
#include <cmath>

#include "common.h"
#include "grid.h"

namespace lcr {

constexpr int FP_WAVES = 4;         // wavefronts (= rows) per workgroup
constexpr int FP_MAX_NN = 128;      // largest max_nn: two list entries per lane
constexpr int FP_BINS = 33;

__device__ __forceinline__ float fp_d2(const float* __restrict__ pts, int64_t i, int64_t j) {
  return grid_d2(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]);
}

__device__ __forceinline__ int fp_bin(double scaled) {
  const double b = floor(scaled);
  return !(b >= 0.0) ? 0 : (b > 10.0 ? 10 : static_cast<int>(b));    // a NaN (non-finite input) lands in bin 0
}

// the three bins of the pair (row i, neighbour j): the header's "Pair features" and "Bins"
__device__ __forceinline__ void fp_pair_bins(const float* __restrict__ pts, const float* __restrict__ nrm, int64_t i, int64_t j, int bins[3]) {
  double n1[3], n2[3], dp[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    n1[r] = static_cast<double>(nrm[3 * i + r]);
    n2[r] = static_cast<double>(nrm[3 * j + r]);
    dp[r] = static_cast<double>(pts[3 * j + r]) - static_cast<double>(pts[3 * i + r]);
  }
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  const double d = sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]);
  if (d != 0.0) {
    const double a1 = (n1[0] * dp[0] + n1[1] * dp[1] + n1[2] * dp[2]) / d;
    const double a2 = (n2[0] * dp[0] + n2[1] * dp[1] + n2[2] * dp[2]) / d;
    if (fabs(a1) < fabs(a2)) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double t = n1[r];
        n1[r] = n2[r];
        n2[r] = t;
        dp[r] = -dp[r];
      }
      f2 = -a2;
    } else {
      f2 = a1;
    }
    double v[3] = {dp[1] * n1[2] - dp[2] * n1[1], dp[2] * n1[0] - dp[0] * n1[2], dp[0] * n1[1] - dp[1] * n1[0]};
    const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (vn == 0.0) {
      f2 = 0.0;
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r) v[r] /= vn;
      const double w[3] = {n1[1] * v[2] - n1[2] * v[1], n1[2] * v[0] - n1[0] * v[2], n1[0] * v[1] - n1[1] * v[0]};
      f1 = v[0] * n2[0] + v[1] * n2[1] + v[2] * n2[2];
      f0 = atan2(w[0] * n2[0] + w[1] * n2[1] + w[2] * n2[2], n1[0] * n2[0] + n1[1] * n2[1] + n1[2] * n2[2]);
    }
  }
  constexpr double PI = 3.14159265358979323846;
  bins[0] = fp_bin(11.0 * (f0 + PI) / (2.0 * PI));
  bins[1] = fp_bin(11.0 * (f1 + 1.0) / 2.0);
  bins[2] = fp_bin(11.0 * (f2 + 1.0) / 2.0);
}

// one wavefront per row: votes of the row's neighbours -> spfh64[i, 33]
__global__ __launch_bounds__(FP_WAVES * 64) void k_spfh(const float* __restrict__ pts, const float* __restrict__ nrm, int64_t n, int max_nn,
                                                        const int32_t* __restrict__ nbr, double* __restrict__ spfh64,
                                                        float* __restrict__ spfh_out, int32_t* __restrict__ count_out) {
  __shared__ int s_hist[FP_WAVES][FP_BINS + 3];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * FP_WAVES + w;
  if (i >= n) return;                                             // wave-uniform
  int* hist = s_hist[w];
  if (lane < FP_BINS) hist[lane] = 0;
  wave_sync();
  int m = 0;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = lane + 64 * u;
    int64_t j = n;
    if (e < max_nn) j = nbr[i * max_nn + e];
    const bool valid = j >= 0 && j < n && j != i;
    if (valid) {
      int bins[3];
      fp_pair_bins(pts, nrm, i, j, bins);
      atomicAdd(&hist[bins[0]], 1);
      atomicAdd(&hist[11 + bins[1]], 1);
      atomicAdd(&hist[22 + bins[2]], 1);
    }
    m += __popcll(wave_ballot(valid));
  }
  wave_sync();
  if (lane < FP_BINS) {
    const double s = m > 0 ? static_cast<double>(hist[lane] * 100) / static_cast<double>(m) : 0.0;
    spfh64[i * FP_BINS + lane] = s;
    if (spfh_out) spfh_out[i * FP_BINS + lane] = static_cast<float>(s);
  }
  if (lane == 0 && count_out) count_out[i] = m;
}

// one wavefront per row: the weighted sum of the neighbours' SPFH rows, normalised per block of 11, plus the row's own SPFH
__global__ __launch_bounds__(FP_WAVES * 64) void k_fpfh(const float* __restrict__ pts, int64_t n, int max_nn, const int32_t* __restrict__ nbr,
                                                        const double* __restrict__ spfh64, float* __restrict__ features) {
  __shared__ int32_t s_nb[FP_WAVES][FP_MAX_NN];
  __shared__ float s_d2[FP_WAVES][FP_MAX_NN];
  __shared__ double s_acc[FP_WAVES][FP_BINS + 3];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * FP_WAVES + w;
  if (i >= n) return;                                             // wave-uniform
  int32_t* nb = s_nb[w];
  float* dd = s_d2[w];
  int k = 0;                                                      // usable neighbours, compacted in list order
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = lane + 64 * u;
    int64_t j = n;
    if (e < max_nn) j = nbr[i * max_nn + e];
    const bool valid = j >= 0 && j < n && j != i;
    float d2 = 0.f;
    if (valid) d2 = fp_d2(pts, i, j);
    const bool use = valid && d2 != 0.f;
    const uint64_t mask = wave_ballot(use);
    if (use) {
      const int slot = k + mbcnt_lt(mask);                        // < FP_MAX_NN: at most max_nn entries are read
      nb[slot] = static_cast<int32_t>(j);
      dd[slot] = d2;
    }
    k += __popcll(mask);
  }
  wave_sync();
  const int bin = lane < FP_BINS ? lane : FP_BINS - 1;            // lanes 33..63 shadow bin 32 and write nothing
  double acc = 0.0;
  for (int e0 = 0; e0 < k; e0 += 4) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u < k ? e0 + u : k - 1;
      v[u] = spfh64[static_cast<int64_t>(nb[e]) * FP_BINS + bin];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e0 + u < k) acc = dadd(acc, v[u] / static_cast<double>(dd[e0 + u]));
  }
  if (lane < FP_BINS) s_acc[w][lane] = acc;
  wave_sync();
  if (lane < FP_BINS) {
    const int blk = lane / 11;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 11; ++r) s = dadd(s, s_acc[w][11 * blk + r]);
    const double scale = s != 0.0 ? 100.0 / s : 0.0;
    features[i * FP_BINS + lane] = static_cast<float>(dadd(dmul(acc, scale), spfh64[i * FP_BINS + lane]));
  }
}

}  // namespace lcr

using namespace lcr;

namespace {

struct FpfhLayout {
  int32_t* nbr;
  double*  spfh;
  int64_t* len;
  size_t   bytes;
};

FpfhLayout fpfh_layout(void* ws, int B, int64_t n, int max_nn, size_t grid_bytes) {
  FpfhLayout L;
  Carver c(ws, ~size_t(0));
  c.take<char>(grid_bytes);                                      // the support grid, at the workspace base
  const size_t rows = static_cast<size_t>(n > 0 ? n : 1);
  L.nbr = c.take<int32_t>(rows * static_cast<size_t>(max_nn));
  L.spfh = c.take<double>(rows * FP_BINS);
  L.len = c.take<int64_t>(B);
  L.bytes = c.off;
  return L;
}

}  // namespace

extern "C" int lcr_fpfh_ws_bytes(int B, int64_t n, int max_nn, size_t* bytes) {
  if (!bytes || B < 1 || B > GRID_MAX_B || n < 0 || n > INT32_MAX || max_nn < 2 || max_nn > FP_MAX_NN)
    return refuse(LCR_EARG, "lcr_fpfh_ws_bytes: outside the domain (1 <= B <= %d, 0 <= n <= 2^31-1, 2 <= max_nn <= %d): B=%d n=%lld max_nn=%d", GRID_MAX_B,
                  FP_MAX_NN, B, static_cast<long long>(n), max_nn);
  size_t g = 0;
  if (int rc = support_grid_ws_bytes("lcr_fpfh_ws_bytes", n, B, &g)) return rc;
  *bytes = fpfh_layout(nullptr, B, n, max_nn, g).bytes;
  return LCR_OK;
}

extern "C" int lcr_fpfh(const float* points, const float* normals, const int64_t* lengths, int B, float radius, int max_nn, float* features,
                        float* spfh, int32_t* count, void* ws, size_t ws_bytes, void* stream) {
  if (!(radius > 0.f) || !std::isfinite(radius * radius) || max_nn < 2 || max_nn > FP_MAX_NN)
    return refuse(LCR_EARG, "lcr_fpfh: outside the domain (radius > 0 with radius*radius finite, 2 <= max_nn <= %d): radius=%g max_nn=%d", FP_MAX_NN,
                  static_cast<double>(radius), max_nn);
  Stack C;
  if (int rc = stack_from_lengths("lcr_fpfh", lengths, B, &C)) return rc;
  const int64_t n = C.off[B];
  if (!ws || (n > 0 && (!points || !normals || !features)))
    return refuse(LCR_EARG, "lcr_fpfh: null workspace, or a null point / normal / feature array (n=%lld)", static_cast<long long>(n));
  size_t grid_bytes = 0;
  support_grid_ws_bytes("lcr_fpfh", n, B, &grid_bytes);
  const FpfhLayout L = fpfh_layout(ws, B, n, max_nn, grid_bytes);
  if (L.bytes > ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_fpfh", ws_bytes, L.bytes);
  if (n == 0) return LCR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = stack_to_device("lcr_fpfh", C, L.len, nullptr, nullptr, st);
  if (rc) return rc;
  rc = support_grid_build("lcr_fpfh", points, L.len, B, n, radius, nullptr, ws, grid_bytes, nullptr, stream);
  if (rc) return rc;
  rc = radius_query("lcr_fpfh", points, L.len, B, n, ws, n, radius, max_nn, nullptr, L.nbr, nullptr, nullptr, stream);
  if (rc) return rc;
  const dim3 grid(div_up(n, FP_WAVES)), block(FP_WAVES * 64);
  hipLaunchKernelGGL(k_spfh, grid, block, 0, st, points, normals, n, max_nn, L.nbr, L.spfh, spfh, count);
  hipLaunchKernelGGL(k_fpfh, grid, block, 0, st, points, n, max_nn, L.nbr, L.spfh, features);
  return check_launch("lcr_fpfh");
}
