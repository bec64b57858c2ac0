// icp.hip — point-to-point ICP (Open3D's RegistrationICP with TransformationEstimationPointToPoint, as the reference's pair generators
// run it: data/Kitti/generate_kitti_pairs.py:145-147) for S pairs of dense clouds in one call, exact and batch-invariant.  The semantics
// (correspondence step, update, loop, outputs) are stated in include/lcr_hip.h next to the entry points.
//
// Per call: k_icp_init (state from `init`, target lengths to the device: stack_store), the support grid of radius_search.hip over the targets
// (cell >= r, built once), then per iteration two stream-ordered launches:
//   k_icp_match   the hot path.  One thread per source row (a block = ICP_BLOCK consecutive rows of one pair): fp64 transform to fp32 q,
//                 arg-min of the (d², target row) key over the nine x-runs of q's 3x3x3 cell neighbourhood (the rule of
//                 lcr_radius_query_ordered's limit == 1 rows), and the row's moments about the pair's anchors reduced over the block in a
//                 fixed tree into a slab of 17 doubles per block.  A block of a finished pair exits at once.
//   k_icp_update  one workgroup per pair: the pair's slab rows summed in a fixed order, fitness / rmse, the convergence test, the fp64
//                 Kabsch (rigid3.h), the history rows, the `done` flag and the count of pairs still running.
// Why one thread per query and not one wavefront (k_radius_query's form): a nearest-only query needs no row, no sort and no LDS.  Here a
// lane spends 18.25 VALU instructions per candidate (ISA, 4 candidates per trip), and a wavefront serves 64 queries at once; the
// cooperative form adds per query a 9-run setup, a prefix scan, an LDS compaction of every in-radius candidate and a 12-shuffle arg-min.
// Source rows are processed in scan order, so neighbouring lanes query neighbouring cells and their trip counts stay close.  Measured on
// raw scans at r = 0.5 m (~1 180 candidates per query): one iteration (both kernels) for 1.36 M queries costs 1.9 ms, while
// lcr_radius_query_ordered(limit = 1) on the same queries takes 8.1 s, because balls of more than 512 rows take its exact
// re-enumeration path (DESIGN.md "Point-to-point ICP").
// Reductions never use float atomics: every sum is a fixed tree over the pair's own row indices, so a pair gives the same bits alone or
// at any position in any batch.
// Point-to-plane (lcr_icp_point_to_plane) runs the same loop with k_icp_match_plane / k_icp_update_plane: the same nearest-partner search
// (icp_nearest), a row block of ICP_PLANE_MOM doubles (count, sum d², usable rows, the 21 entries of A = sum J J^T, g = sum J r), and an
// fp64 LDL^T solve of A x = -g in the update.
// Generalized ICP (lcr_icp_generalized) is the third estimator of the same loop, k_icp_match_gicp / k_icp_update_gicp: per partnered row the
// 3x3 weight W = (C_t + R C_s R^T)^-1 from both normals, a row block of ICP_GICP_MOM doubles (count, sum d², the 21 entries of
// A = sum J^T W J, g = sum J^T W d) and the same solve and composition as point-to-plane (icp_solve_commit).
#include <algorithm>
#include <climits>
#include <cmath>
#include <string>

#include "common.h"
#include "grid.h"
#include "rigid3.h"

namespace lcr {

constexpr int ICP_BLOCK = 256;   // source rows (= threads) per k_icp_match workgroup; also the k_icp_update workgroup size
constexpr int ICP_UNROLL = 4;    // candidate loads in flight per lane
constexpr int ICP_MOM = 17;      // count, sum d², sum dp[3], sum dr[3], sum dp dr^T [9]  (dp = p - anchor_src, dr = r - anchor_tgt)
constexpr int ICP_PLANE_MOM = 30;  // count, sum d², usable rows, A = sum J J^T [21, upper triangle row by row], g = sum J r [6]
constexpr int ICP_GICP_MOM = 29;   // count, sum d², A = sum J^T W J [21, upper triangle row by row], g = sum J^T W d [6]

// pair table, by value in the kernel arguments (S <= GRID_MAX_B): the first k_icp_match block of every pair and the off[] of the two Stacks
struct IcpPairs {
  int     S;
  int     blk_off[GRID_MAX_B + 1];
  int64_t src_off[GRID_MAX_B + 1];
  int64_t tgt_off[GRID_MAX_B + 1];
};

// fp32(((T[4r] * x + T[4r+1] * y) + T[4r+2] * z) + T[4r+3]), no contraction
__device__ __forceinline__ float icp_row(const double* T, int r, double x, double y, double z) {
  return static_cast<float>(dadd(dadd(dadd(dmul(T[4 * r], x), dmul(T[4 * r + 1], y)), dmul(T[4 * r + 2], z)), T[4 * r + 3]));
}

// fixed-order sum of MOM doubles over a workgroup of ICP_BLOCK threads (across the wavefront first); the totals land in thread 0's m[]
template <int MOM>
__device__ __forceinline__ void icp_block_sum(double (&m)[MOM], double (*s_red)[MOM]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < MOM; ++j)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m[j] = dadd(m[j], __shfl_xor(m[j], d));
  if (lane == 0)
#pragma unroll
    for (int j = 0; j < MOM; ++j) s_red[w][j] = m[j];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int j = 0; j < MOM; ++j) {
      double a = s_red[0][j];
      for (int v = 1; v < ICP_BLOCK / 64; ++v) a = dadd(a, s_red[v][j]);
      m[j] = a;
    }
}

// the moments of a pair for its k_icp_update*: the slab rows of its nb row blocks (from b0) summed in a fixed order, totals in thread 0's m[]
template <int MOM>
__device__ __forceinline__ void icp_slab_sum(const double* __restrict__ slab, int b0, int nb, double (&m)[MOM], double (*s_red)[MOM]) {
#pragma unroll
  for (int j = 0; j < MOM; ++j) m[j] = 0.0;
  for (int b = threadIdx.x; b < nb; b += ICP_BLOCK)
#pragma unroll
    for (int j = 0; j < MOM; ++j) m[j] = dadd(m[j], slab[static_cast<int64_t>(b0 + b) * MOM + j]);
  icp_block_sum<MOM>(m, s_red);
}

// the partner key of q: the smallest (d², target row) with d² < r2 over the nine x-runs of q's 3x3x3 cell neighbourhood, ~0 if none
__device__ __forceinline__ uint64_t icp_nearest(const GridCloud& c, const int32_t* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                float r2, float qx, float qy, float qz) {
  uint64_t best = ~0ull;
  // the candidates are the runs of grid_for_each_run (grid.h), the neighbourhood every client of the grid sees; an empty target has none,
  // and asking first spares its rows the cell arithmetic
  if (c.dim[0] > 0) grid_for_each_run(c, cell_start, qx, qy, qz, [&](int k0, int e) {
    // ICP_UNROLL loads in flight per trip; the tail re-reads the run's last candidate, which cannot change an arg-min
    for (int k = k0; k < e; k += ICP_UNROLL) {
      float4 p[ICP_UNROLL];
#pragma unroll
      for (int u = 0; u < ICP_UNROLL; ++u) p[u] = sorted[min(k + u, e - 1)];
#pragma unroll
      for (int u = 0; u < ICP_UNROLL; ++u) {
        const float d2 = grid_d2(qx, qy, qz, p[u]);
        const uint64_t key = grid_key(d2, p[u].w);
        // &, not &&: `best` is captured by reference, and a short circuit over it stays a branch in the compiled loop
        best = ((d2 < r2) & (key < best)) ? key : best;
      }
    }
  });
  return best;
}

// the shared head of k_icp_match*: source row i of pair s under the pair's current T.  Tm = rows 0..2 of T, p = the row in fp64; the partner
// (icp_nearest of fp32(T p)) comes back as its stacked target row j and d² (0 without one); corr[i] gets the pair-local partner (-1: none).  False: no partner.
__device__ __forceinline__ bool icp_match_row(const double* __restrict__ T, int s, const float* __restrict__ src, int64_t i, int64_t tb,
                                              const GridHeader* __restrict__ h, const int32_t* __restrict__ cell_start,
                                              const float4* __restrict__ sorted, float r2, int32_t* __restrict__ corr, double (&Tm)[12],
                                              double (&p)[3], int64_t& j, double& d2) {
#pragma unroll
  for (int k = 0; k < 12; ++k) Tm[k] = T[16 * s + k];
#pragma unroll
  for (int d = 0; d < 3; ++d) p[d] = src[3 * i + d];
  const float qx = icp_row(Tm, 0, p[0], p[1], p[2]), qy = icp_row(Tm, 1, p[0], p[1], p[2]), qz = icp_row(Tm, 2, p[0], p[1], p[2]);
  const uint64_t best = icp_nearest(h->cloud[s], cell_start, sorted, r2, qx, qy, qz);
  const bool found = best != ~0ull;
  j = static_cast<int64_t>(static_cast<uint32_t>(best));
  d2 = found ? static_cast<double>(__uint_as_float(static_cast<uint32_t>(best >> 32))) : 0.0;
  if (corr) corr[i] = found ? static_cast<int32_t>(j - tb) : -1;
  return found;
}

__global__ void k_icp_init(IcpPairs P, const double* __restrict__ init, int hist_rows, double* __restrict__ T, double* __restrict__ fitness,
                           double* __restrict__ rmse, int32_t* __restrict__ iters, int32_t* __restrict__ done, int32_t* __restrict__ running,
                           int64_t* __restrict__ tgt_len, double* __restrict__ T_hist, double* __restrict__ fit_hist, double* __restrict__ rmse_hist) {
  if (threadIdx.x < 2) running[threadIdx.x] = 0;
  stack_store(P.tgt_off, P.S, tgt_len, nullptr);
  for (int s = threadIdx.x; s < P.S; s += blockDim.x) {
    const int64_t ns = P.src_off[s + 1] - P.src_off[s], nt = P.tgt_off[s + 1] - P.tgt_off[s];
    for (int k = 0; k < 16; ++k) T[16 * s + k] = init[16 * s + k];
    fitness[s] = 0.0;
    rmse[s] = 0.0;
    iters[s] = 0;
    done[s] = (ns == 0 || nt == 0) ? 1 : 0;          // empty source or target: init, fitness 0, rmse 0, 0 iterations
    const int64_t h0 = static_cast<int64_t>(s) * hist_rows;
    if (T_hist)
      for (int k = 0; k < 16; ++k) T_hist[16 * h0 + k] = init[16 * s + k];
    if (done[s]) {
      if (fit_hist) fit_hist[h0] = 0.0;
      if (rmse_hist) rmse_hist[h0] = 0.0;
    }
  }
}

// one thread per source row: correspondence at the pair's current T, moments reduced per block into slab[blockIdx.x][ICP_MOM]
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_match(IcpPairs P, const float* __restrict__ src, const float* __restrict__ tgt,
                                                         const GridHeader* __restrict__ h, const int32_t* __restrict__ cell_start,
                                                         const float4* __restrict__ sorted, float r2, const double* __restrict__ T,
                                                         const int32_t* __restrict__ done, double* __restrict__ slab, int32_t* __restrict__ corr) {
  __shared__ double s_red[ICP_BLOCK / 64][ICP_MOM];
  const int blk = blockIdx.x;
  const int s = cloud_of(P.blk_off, P.S, blk);
  if (done[s]) return;                                         // workgroup-uniform
  const int64_t a = P.src_off[s], n = P.src_off[s + 1] - a, tb = P.tgt_off[s];
  const int64_t row = static_cast<int64_t>(blk - P.blk_off[s]) * ICP_BLOCK + threadIdx.x;     // pair-local
  double m[ICP_MOM];
#pragma unroll
  for (int j = 0; j < ICP_MOM; ++j) m[j] = 0.0;
  if (row < n) {
    const int64_t i = a + row;
    double Tm[12], p[3], d2;
    int64_t j;
    if (icp_match_row(T, s, src, i, tb, h, cell_start, sorted, r2, corr, Tm, p, j, d2)) {
      const double x = p[0], y = p[1], z = p[2];
      const double dp[3] = {x - static_cast<double>(src[3 * a]), y - static_cast<double>(src[3 * a + 1]), z - static_cast<double>(src[3 * a + 2])};
      const double dr[3] = {static_cast<double>(tgt[3 * j]) - static_cast<double>(tgt[3 * tb]),
                            static_cast<double>(tgt[3 * j + 1]) - static_cast<double>(tgt[3 * tb + 1]),
                            static_cast<double>(tgt[3 * j + 2]) - static_cast<double>(tgt[3 * tb + 2])};
      m[0] = 1.0;
      m[1] = d2;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        m[2 + r] = dp[r];
        m[5 + r] = dr[r];
#pragma unroll
        for (int q = 0; q < 3; ++q) m[8 + 3 * r + q] = dmul(dp[r], dr[q]);
      }
    }
  }
  icp_block_sum<ICP_MOM>(m, s_red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int j = 0; j < ICP_MOM; ++j) slab[static_cast<int64_t>(blk) * ICP_MOM + j] = m[j];
}

// thread 0 of a pair's k_icp_update*: result_k (fitness, rmse) from the summed count and d², the convergence test against result_{k-1} and
// the history row; false when the pair stops here (done)
__device__ __forceinline__ bool icp_result(const IcpPairs& P, int s, double cnt, double d2sum, int k, int max_iter, double rel_fit, double rel_rmse,
                                           double* __restrict__ fitness, double* __restrict__ rmse, int32_t* __restrict__ done,
                                           double* __restrict__ fit_hist, double* __restrict__ rmse_hist) {
  const int64_t ns = P.src_off[s + 1] - P.src_off[s];
  const int64_t hrow = static_cast<int64_t>(s) * (max_iter + 1);
  const double fit = cnt / static_cast<double>(ns);
  const double rm = cnt > 0.0 ? sqrt(d2sum / cnt) : 0.0;
  const bool conv = k > 0 && fabs(fitness[s] - fit) < rel_fit && fabs(rmse[s] - rm) < rel_rmse;
  fitness[s] = fit;
  rmse[s] = rm;
  if (fit_hist) fit_hist[hrow + k] = fit;
  if (rmse_hist) rmse_hist[hrow + k] = rm;
  if (conv || k >= max_iter) {
    done[s] = 1;
    return false;
  }
  return true;
}

// thread 0 of a pair's k_icp_update*: T_{k+1} = Tn (rows 0..2), the iteration count, its history row, and the pair counted as running
__device__ __forceinline__ void icp_commit(int s, int k, int max_iter, const double (&Tn)[12], double* __restrict__ T, int32_t* __restrict__ iters,
                                           int32_t* __restrict__ running, double* __restrict__ T_hist) {
  const int64_t hrow = static_cast<int64_t>(s) * (max_iter + 1);
  for (int q = 0; q < 12; ++q) T[16 * s + q] = Tn[q];
  T[16 * s + 12] = T[16 * s + 13] = T[16 * s + 14] = 0.0;
  T[16 * s + 15] = 1.0;
  iters[s] = k + 1;
  if (T_hist) {
    double* o = T_hist + 16 * (hrow + k + 1);
    for (int q = 0; q < 12; ++q) o[q] = Tn[q];
    o[12] = o[13] = o[14] = 0.0;
    o[15] = 1.0;
  }
  atomicAdd(&running[k & 1], 1);
}

// one workgroup per pair: result_k from the slab, convergence test against result_{k-1}, then update k (T_{k+1}) unless the pair stops
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_update(IcpPairs P, const float* __restrict__ src, const float* __restrict__ tgt,
                                                          const double* __restrict__ slab, int k, int max_iter, double rel_fit, double rel_rmse,
                                                          double* __restrict__ T, double* __restrict__ fitness, double* __restrict__ rmse,
                                                          int32_t* __restrict__ iters, int32_t* __restrict__ done, int32_t* __restrict__ running,
                                                          double* __restrict__ T_hist, double* __restrict__ fit_hist, double* __restrict__ rmse_hist) {
  __shared__ double s_red[ICP_BLOCK / 64][ICP_MOM];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (s == 0 && tid == 0) running[(k + 1) & 1] = 0;          // the other slot: read by the host after the previous launch, if at all
  if (done[s]) return;
  const int b0 = P.blk_off[s], nb = P.blk_off[s + 1] - b0;
  double m[ICP_MOM];
  icp_slab_sum<ICP_MOM>(slab, b0, nb, m, s_red);
  if (tid != 0) return;

  const int64_t a = P.src_off[s], tb = P.tgt_off[s];
  const double cnt = m[0];
  if (!icp_result(P, s, cnt, m[1], k, max_iter, rel_fit, rel_rmse, fitness, rmse, done, fit_hist, rmse_hist)) return;
  // update k: unit-weight Kabsch on (p_i, r_j) about the anchors; T unchanged when count < 3 or H is degenerate
  double Tn[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) Tn[q] = T[16 * s + q];
  if (cnt >= 3.0) {
    const double ap[3] = {src[3 * a], src[3 * a + 1], src[3 * a + 2]}, ar[3] = {tgt[3 * tb], tgt[3 * tb + 1], tgt[3 * tb + 2]};
    double H[3][3], cp[3], cr[3];
    for (int r = 0; r < 3; ++r) {
      cp[r] = m[2 + r] / cnt;                                  // centroids relative to the anchors
      cr[r] = m[5 + r] / cnt;
    }
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) H[r][q] = m[8 + 3 * r + q] - cnt * cp[r] * cr[q];
    double R[3][3], sv[3];
    rotation_from_H_sv(H, R, sv);
    if (!(sv[0] <= 1e-30 || sv[1] <= 1e-9 * sv[0])) {
      for (int r = 0; r < 3; ++r) {
        const double cpa[3] = {ap[0] + cp[0], ap[1] + cp[1], ap[2] + cp[2]};
        double t = ar[r] + cr[r];
        for (int q = 0; q < 3; ++q) {
          Tn[4 * r + q] = R[r][q];
          t -= R[r][q] * cpa[q];
        }
        Tn[4 * r + 3] = t;
      }
    }
  }
  icp_commit(s, k, max_iter, Tn, T, iters, running, T_hist);
}

// point-to-plane: one thread per source row, the partner of k_icp_match; a usable row (partner with a non-zero normal) adds J J^T and J r
// (s = T p in fp64, J = [s x n, n], r = (s - t) . n) to its row block, reduced into slab[blockIdx.x][ICP_PLANE_MOM].  The row keeps only
// J and r; each of the 30 block sums is formed from them and reduced on its own (the tree of icp_block_sum), so that the 30 moments are
// never live at once: 30 doubles in flight would double the registers of the candidate loop's kernel and halve its occupancy.
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_match_plane(IcpPairs P, const float* __restrict__ src, const float* __restrict__ tgt,
                                                               const float* __restrict__ nrm, const GridHeader* __restrict__ h,
                                                               const int32_t* __restrict__ cell_start, const float4* __restrict__ sorted, float r2,
                                                               const double* __restrict__ T, const int32_t* __restrict__ done,
                                                               double* __restrict__ slab, int32_t* __restrict__ corr) {
  __shared__ double s_red[ICP_BLOCK / 64][ICP_PLANE_MOM];
  const int blk = blockIdx.x;
  const int s = cloud_of(P.blk_off, P.S, blk);
  if (done[s]) return;                                         // workgroup-uniform
  const int64_t a = P.src_off[s], n = P.src_off[s + 1] - a, tb = P.tgt_off[s];
  const int64_t row = static_cast<int64_t>(blk - P.blk_off[s]) * ICP_BLOCK + threadIdx.x;     // pair-local
  double found = 0.0, d2 = 0.0, use = 0.0, res = 0.0, J[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (row < n) {
    const int64_t i = a + row;
    double Tm[12], p[3];
    int64_t j;
    if (icp_match_row(T, s, src, i, tb, h, cell_start, sorted, r2, corr, Tm, p, j, d2)) {
      const double x = p[0], y = p[1], z = p[2];
      found = 1.0;
      const double nv[3] = {nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2]};
      if (nv[0] != 0.0 || nv[1] != 0.0 || nv[2] != 0.0) {
        double sp[3], dv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          sp[r] = dadd(dadd(dadd(dmul(Tm[4 * r], x), dmul(Tm[4 * r + 1], y)), dmul(Tm[4 * r + 2], z)), Tm[4 * r + 3]);
          dv[r] = sp[r] - static_cast<double>(tgt[3 * j + r]);
        }
        use = 1.0;
        res = dadd(dadd(dmul(dv[0], nv[0]), dmul(dv[1], nv[1])), dmul(dv[2], nv[2]));
        J[0] = dmul(sp[1], nv[2]) - dmul(sp[2], nv[1]);
        J[1] = dmul(sp[2], nv[0]) - dmul(sp[0], nv[2]);
        J[2] = dmul(sp[0], nv[1]) - dmul(sp[1], nv[0]);
        J[3] = nv[0];
        J[4] = nv[1];
        J[5] = nv[2];
      }
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  auto wave_sum = [&](double v, int q) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = dadd(v, __shfl_xor(v, d));
    if (lane == 0) s_red[w][q] = v;
  };
  wave_sum(found, 0);
  wave_sum(d2, 1);
  wave_sum(use, 2);
  int q = 3;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) wave_sum(dmul(J[r], J[c]), q++);
#pragma unroll
  for (int r = 0; r < 6; ++r) wave_sum(dmul(J[r], res), 24 + r);
  __syncthreads();
  if (threadIdx.x < ICP_PLANE_MOM) {                              // the cross-wave step of icp_block_sum, one moment per thread
    double v = s_red[0][threadIdx.x];
    for (int u = 1; u < ICP_BLOCK / 64; ++u) v = dadd(v, s_red[u][threadIdx.x]);
    slab[static_cast<int64_t>(blk) * ICP_PLANE_MOM + threadIdx.x] = v;
  }
}

// x = solution of A x = -g by LDL^T without pivoting (A symmetric 6x6 from its upper triangle, row by row); false when a pivot is
// <= 1e-12 times the largest diagonal entry of A
__device__ inline bool icp_solve6(const double* au, const double* g, double x[6]) {
  double A[6][6], L[6][6], D[6];
  int q = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) A[r][c] = A[c][r] = au[q++];
  double amax = 0.0;
  for (int r = 0; r < 6; ++r) amax = fmax(amax, A[r][r]);
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
    if (!(d > 1e-12 * amax)) return false;
    D[j] = d;
    L[j][j] = 1.0;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * D[k];
      L[i][j] = v / d;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {                                  // L y = -g
    double v = -g[i];
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v;
  }
  for (int i = 5; i >= 0; --i) {                                 // D L^T x = y
    double v = y[i] / D[i];
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
    x[i] = v;
  }
  return true;
}

// thread 0 of a pair's k_icp_update_plane / k_icp_update_gicp: update k from the summed normal equations (au = A's upper triangle row by
// row, g), T <- dT(x) T with dT = [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)], then icp_commit.  T is kept when `enough` is false or a pivot of
// icp_solve6 fails.
__device__ __forceinline__ void icp_solve_commit(int s, int k, int max_iter, bool enough, const double* au, const double* g, double* __restrict__ T,
                                                 int32_t* __restrict__ iters, int32_t* __restrict__ running, double* __restrict__ T_hist) {
  double Tn[12];
  for (int q = 0; q < 12; ++q) Tn[q] = T[16 * s + q];
  double x[6];
  if (enough && icp_solve6(au, g, x)) {
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cc = cos(x[2]), sc = sin(x[2]);
    const double R[3][3] = {{cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa},     // Rz(x2) Ry(x1) Rx(x0)
                            {sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa},
                            {-sb, cb * sa, cb * ca}};
    double To[12];
    for (int q = 0; q < 12; ++q) To[q] = Tn[q];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 4; ++c) Tn[4 * r + c] = (R[r][0] * To[c] + R[r][1] * To[4 + c]) + R[r][2] * To[8 + c];
      Tn[4 * r + 3] += x[3 + r];
    }
  }
  icp_commit(s, k, max_iter, Tn, T, iters, running, T_hist);
}

// one workgroup per pair: result_k as k_icp_update, then the point-to-plane update T <- dT(x) T
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_update_plane(IcpPairs P, const double* __restrict__ slab, int k, int max_iter, double rel_fit,
                                                                double rel_rmse, double* __restrict__ T, double* __restrict__ fitness,
                                                                double* __restrict__ rmse, int32_t* __restrict__ iters, int32_t* __restrict__ done,
                                                                int32_t* __restrict__ running, double* __restrict__ T_hist,
                                                                double* __restrict__ fit_hist, double* __restrict__ rmse_hist) {
  __shared__ double s_red[ICP_BLOCK / 64][ICP_PLANE_MOM];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (s == 0 && tid == 0) running[(k + 1) & 1] = 0;          // the other slot: read by the host after the previous launch, if at all
  if (done[s]) return;
  const int b0 = P.blk_off[s], nb = P.blk_off[s + 1] - b0;
  double m[ICP_PLANE_MOM];
  icp_slab_sum<ICP_PLANE_MOM>(slab, b0, nb, m, s_red);
  if (tid != 0) return;
  if (!icp_result(P, s, m[0], m[1], k, max_iter, rel_fit, rel_rmse, fitness, rmse, done, fit_hist, rmse_hist)) return;
  // update k: T unchanged when fewer than 6 rows are usable or A is (numerically) singular
  icp_solve_commit(s, k, max_iter, m[2] >= 6.0, m + 3, m + 24, T, iters, running, T_hist);
}

// generalized ICP: one thread per source row, the partner of k_icp_match; a partnered row weights its residual d = s - t (s = T p in
// fp64) by W = M^-1, M = 2I - (1 - eps)(a a^T + b b^T) with a = Rm n_src and b = n_tgt (zero normals: C = I on that side), and adds
// J^T W J and J^T W d, J = [-[s]x | I], to its row block, reduced into slab[blockIdx.x][ICP_GICP_MOM].  As in k_icp_match_plane the row
// keeps only s, d and the six entries of W (zero without a partner); each of the 29 block sums is formed from them and reduced on its own,
// so that the moments are never live at once and the candidate loop keeps its occupancy.
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_match_gicp(IcpPairs P, const float* __restrict__ src, const float* __restrict__ src_nrm,
                                                              const float* __restrict__ tgt, const float* __restrict__ tgt_nrm,
                                                              const GridHeader* __restrict__ h, const int32_t* __restrict__ cell_start,
                                                              const float4* __restrict__ sorted, float r2, double one_minus_eps,
                                                              const double* __restrict__ T, const int32_t* __restrict__ done,
                                                              double* __restrict__ slab, int32_t* __restrict__ corr) {
  __shared__ double s_red[ICP_BLOCK / 64][ICP_GICP_MOM];
  const int blk = blockIdx.x;
  const int s = cloud_of(P.blk_off, P.S, blk);
  if (done[s]) return;                                         // workgroup-uniform
  const int64_t a = P.src_off[s], n = P.src_off[s + 1] - a, tb = P.tgt_off[s];
  const int64_t row = static_cast<int64_t>(blk - P.blk_off[s]) * ICP_BLOCK + threadIdx.x;     // pair-local
  double found = 0.0, d2 = 0.0, sp[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0};
  double W[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                // xx, xy, xz, yy, yz, zz
  if (row < n) {
    const int64_t i = a + row;
    double Tm[12], p[3];
    int64_t j;
    if (icp_match_row(T, s, src, i, tb, h, cell_start, sorted, r2, corr, Tm, p, j, d2)) {
      const double x = p[0], y = p[1], z = p[2];
      const double nx = src_nrm[3 * i], ny = src_nrm[3 * i + 1], nz = src_nrm[3 * i + 2];
      found = 1.0;
      double av[3], bv[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        sp[r] = dadd(dadd(dadd(dmul(Tm[4 * r], x), dmul(Tm[4 * r + 1], y)), dmul(Tm[4 * r + 2], z)), Tm[4 * r + 3]);
        dv[r] = sp[r] - static_cast<double>(tgt[3 * j + r]);
        av[r] = dadd(dadd(dmul(Tm[4 * r], nx), dmul(Tm[4 * r + 1], ny)), dmul(Tm[4 * r + 2], nz));
        bv[r] = tgt_nrm[3 * j + r];
      }
      auto Mrc = [&](int r, int c) {
        return (r == c ? 2.0 : 0.0) - dmul(one_minus_eps, dadd(dmul(av[r], av[c]), dmul(bv[r], bv[c])));
      };
      const double m00 = Mrc(0, 0), m01 = Mrc(0, 1), m02 = Mrc(0, 2), m11 = Mrc(1, 1), m12 = Mrc(1, 2), m22 = Mrc(2, 2);
      // W = adj(M) / det(M); det > 0 on the domain (eps >= 1e-6, normals unit or zero)
      const double c00 = dmul(m11, m22) - dmul(m12, m12), c01 = dmul(m02, m12) - dmul(m01, m22), c02 = dmul(m01, m12) - dmul(m02, m11);
      const double c11 = dmul(m00, m22) - dmul(m02, m02), c12 = dmul(m01, m02) - dmul(m00, m12), c22 = dmul(m00, m11) - dmul(m01, m01);
      const double det = dadd(dadd(dmul(m00, c00), dmul(m01, c01)), dmul(m02, c02));
      W[0] = c00 / det;
      W[1] = c01 / det;
      W[2] = c02 / det;
      W[3] = c11 / det;
      W[4] = c12 / det;
      W[5] = c22 / det;
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  auto wave_sum = [&](double v, int q) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = dadd(v, __shfl_xor(v, d));
    if (lane == 0) s_red[w][q] = v;
  };
  auto Wrc = [&](int r, int c) { return W[r <= c ? (r == 0 ? c : r + c + 1) : (c == 0 ? r : r + c + 1)]; };      // the symmetric W
  // B = [s]x W = A_rt: column c is s x (column c of W)
  auto Brc = [&](int r, int c) { return dmul(sp[(r + 1) % 3], Wrc((r + 2) % 3, c)) - dmul(sp[(r + 2) % 3], Wrc((r + 1) % 3, c)); };
  // A_rr = -[s]x W [s]x = B [s]x^T: entry (r, c) is row r of B against row c of [s]x
  auto Arr = [&](int r, int c) { return dmul(Brc(r, (c + 2) % 3), sp[(c + 1) % 3]) - dmul(Brc(r, (c + 1) % 3), sp[(c + 2) % 3]); };
  wave_sum(found, 0);
  wave_sum(d2, 1);
  int q = 2;
#pragma unroll
  for (int r = 0; r < 3; ++r) {                                  // rows 0..2 of A: A_rr from the diagonal on, then A_rt
#pragma unroll
    for (int c = r; c < 3; ++c) wave_sum(Arr(r, c), q++);
#pragma unroll
    for (int c = 0; c < 3; ++c) wave_sum(Brc(r, c), q++);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)                                    // rows 3..5: A_tt = W
#pragma unroll
    for (int c = r; c < 3; ++c) wave_sum(Wrc(r, c), q++);
  double u[3];                                                   // u = W d;  g = [s x u ; u]
#pragma unroll
  for (int r = 0; r < 3; ++r) u[r] = dadd(dadd(dmul(Wrc(r, 0), dv[0]), dmul(Wrc(r, 1), dv[1])), dmul(Wrc(r, 2), dv[2]));
#pragma unroll
  for (int r = 0; r < 3; ++r) wave_sum(dmul(sp[(r + 1) % 3], u[(r + 2) % 3]) - dmul(sp[(r + 2) % 3], u[(r + 1) % 3]), 23 + r);
#pragma unroll
  for (int r = 0; r < 3; ++r) wave_sum(u[r], 26 + r);
  __syncthreads();
  if (threadIdx.x < ICP_GICP_MOM) {                                // the cross-wave step of icp_block_sum, one moment per thread
    double v = s_red[0][threadIdx.x];
    for (int u2 = 1; u2 < ICP_BLOCK / 64; ++u2) v = dadd(v, s_red[u2][threadIdx.x]);
    slab[static_cast<int64_t>(blk) * ICP_GICP_MOM + threadIdx.x] = v;
  }
}

// one workgroup per pair: result_k as k_icp_update, then the generalized update T <- dT(x) T (T unchanged when count < 3 or a pivot fails)
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_update_gicp(IcpPairs P, const double* __restrict__ slab, int k, int max_iter, double rel_fit,
                                                               double rel_rmse, double* __restrict__ T, double* __restrict__ fitness,
                                                               double* __restrict__ rmse, int32_t* __restrict__ iters, int32_t* __restrict__ done,
                                                               int32_t* __restrict__ running, double* __restrict__ T_hist,
                                                               double* __restrict__ fit_hist, double* __restrict__ rmse_hist) {
  __shared__ double s_red[ICP_BLOCK / 64][ICP_GICP_MOM];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (s == 0 && tid == 0) running[(k + 1) & 1] = 0;          // the other slot: read by the host after the previous launch, if at all
  if (done[s]) return;
  const int b0 = P.blk_off[s], nb = P.blk_off[s + 1] - b0;
  double m[ICP_GICP_MOM];
  icp_slab_sum<ICP_GICP_MOM>(slab, b0, nb, m, s_red);
  if (tid != 0) return;
  if (!icp_result(P, s, m[0], m[1], k, max_iter, rel_fit, rel_rmse, fitness, rmse, done, fit_hist, rmse_hist)) return;
  icp_solve_commit(s, k, max_iter, m[0] >= 3.0, m + 2, m + 23, T, iters, running, T_hist);
}

}  // namespace lcr

using namespace lcr;

namespace {
constexpr int ICP_MAX_ITER = 100000;

int icp_blocks_bound(int S, int64_t ns) { return div_up(ns, ICP_BLOCK) + S; }

size_t icp_layout(void* ws, int S, int64_t ns, int64_t nt, size_t grid_bytes, int mom, double** slab, int32_t** done, int32_t** running,
                  int64_t** tgt_len) {
  Carver c(ws, ~size_t(0));
  c.take<char>(grid_bytes);                                      // the support grid, at the workspace base
  double* sl = c.take<double>(static_cast<size_t>(icp_blocks_bound(S, ns)) * mom);
  int32_t* dn = c.take<int32_t>(S);
  int32_t* rn = c.take<int32_t>(2);
  int64_t* tl = c.take<int64_t>(S);
  if (slab) {
    *slab = sl;
    *done = dn;
    *running = rn;
    *tgt_len = tl;
  }
  (void)nt;
  return c.off;
}

int icp_ws_bytes(const char* name, int S, int64_t ns, int64_t nt, int mom, size_t* bytes) {
  if (!bytes || S < 1 || S > GRID_MAX_B || ns < 0 || nt < 0 || ns > INT32_MAX || nt > INT32_MAX)
    return refuse(LCR_EARG, "%s: outside the domain (1 <= S <= %d, 0 <= ns, nt <= 2^31-1): S=%d ns=%lld nt=%lld", name, GRID_MAX_B, S,
                  static_cast<long long>(ns), static_cast<long long>(nt));
  size_t g = 0;
  if (int rc = support_grid_ws_bytes(name, nt, S, &g)) return rc;
  *bytes = icp_layout(nullptr, S, ns, nt, g, mom, nullptr, nullptr, nullptr, nullptr);
  return LCR_OK;
}

enum class IcpEst { POINT, PLANE, GICP };
constexpr double ICP_GICP_MIN_EPS = 1e-6;

// the host loop of the three estimators (POINT reads no normals, PLANE tgt_normals, GICP both sides' and epsilon)
template <IcpEst EST>
int icp_run(const char* name, const float* src, const int64_t* src_len, const float* src_normals, const float* tgt, const int64_t* tgt_len,
            const float* tgt_normals, int S, const double* init, float max_correspondence_distance, double epsilon, int max_iteration,
            double relative_fitness, double relative_rmse, double* T, double* fitness, double* inlier_rmse, int32_t* iterations, int32_t* corr,
            double* T_hist, double* fitness_hist, double* rmse_hist, int check_every, void* ws, size_t ws_bytes, void* stream) {
  constexpr bool PLANE = EST == IcpEst::PLANE, GICP = EST == IcpEst::GICP;
  const float r = max_correspondence_distance;
  if (max_iteration < 0 || max_iteration > ICP_MAX_ITER || !(r > 0.f) || !std::isfinite(r * r) || check_every < 0 ||
      !(relative_fitness >= 0.0) || !(relative_rmse >= 0.0))
    return refuse(LCR_EARG, "%s: outside the domain (0 <= max_iteration <= %d, r > 0 with r*r finite, relative criteria >= 0, check_every >= 0): "
                  "max_iteration=%d r=%g check_every=%d", name, ICP_MAX_ITER, max_iteration, static_cast<double>(r), check_every);
  if (GICP && !(epsilon >= ICP_GICP_MIN_EPS && epsilon <= 1.0))
    return refuse(LCR_EARG, "%s: outside the domain (%g <= epsilon <= 1): epsilon=%g", name, ICP_GICP_MIN_EPS, epsilon);
  if (!init || !T || !fitness || !inlier_rmse || !iterations || !ws) return refuse(LCR_EARG, "%s: null pointer", name);
  Stack sources, targets;
  const std::string who(name);                                   // the error text says which of the two tables is at fault
  if (int rc = stack_from_lengths((who + ": source lengths").c_str(), src_len, S, &sources)) return rc;
  if (int rc = stack_from_lengths((who + ": target lengths").c_str(), tgt_len, S, &targets)) return rc;
  IcpPairs P;
  P.S = S;
  std::copy(sources.off, sources.off + S + 1, P.src_off);
  std::copy(targets.off, targets.off + S + 1, P.tgt_off);
  P.blk_off[0] = 0;
  for (int s = 0; s < S; ++s) P.blk_off[s + 1] = P.blk_off[s] + div_up(src_len[s], ICP_BLOCK);
  const int64_t ns = P.src_off[S], nt = P.tgt_off[S];
  if ((ns > 0 && (!src || (GICP && !src_normals))) || (nt > 0 && (!tgt || ((PLANE || GICP) && !tgt_normals))))
    return refuse(LCR_EARG, "%s: null point or normal array (ns=%lld nt=%lld)", name, static_cast<long long>(ns), static_cast<long long>(nt));
  constexpr int mom = GICP ? ICP_GICP_MOM : PLANE ? ICP_PLANE_MOM : ICP_MOM;
  size_t need = 0, grid_bytes = 0;
  icp_ws_bytes(name, S, ns, nt, mom, &need);
  support_grid_ws_bytes(name, nt, S, &grid_bytes);
  if (need > ws_bytes) return refuse_ws(LCR_ESPACE, name, ws_bytes, need);
  double* slab;
  int32_t *done, *running;
  int64_t* tgt_len_dev;
  icp_layout(ws, S, ns, nt, grid_bytes, mom, &slab, &done, &running, &tgt_len_dev);
  const GridLayout L = grid_layout(ws, nt, S);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, st, P, init, max_iteration + 1, T, fitness, inlier_rmse, iterations, done, running, tgt_len_dev,
                     T_hist, fitness_hist, rmse_hist);
  if (corr && ns > 0 && hipMemsetAsync(corr, 0xff, static_cast<size_t>(ns) * sizeof(int32_t), st) != hipSuccess) {   // -1 for pairs that never run
    return refuse(LCR_EHIP, "%s: clearing corr failed", name);
  }
  int rc = check_launch(name);
  if (rc) return rc;
  rc = support_grid_build(name, tgt, tgt_len_dev, S, nt, r, nullptr, ws, grid_bytes, nullptr, stream);
  if (rc) return rc;
  const int nblk = P.blk_off[S];
  const float r2 = r * r;                                        // fp32 product, as lcr_radius_query
  for (int k = 0; k <= max_iteration; ++k) {
    if constexpr (GICP) {
      if (nblk > 0)
        hipLaunchKernelGGL(k_icp_match_gicp, dim3(nblk), dim3(ICP_BLOCK), 0, st, P, src, src_normals, tgt, tgt_normals, L.hdr, L.cell_start,
                           L.sorted, r2, 1.0 - epsilon, T, done, slab, corr);
      hipLaunchKernelGGL(k_icp_update_gicp, dim3(S), dim3(ICP_BLOCK), 0, st, P, slab, k, max_iteration, relative_fitness, relative_rmse, T,
                         fitness, inlier_rmse, iterations, done, running, T_hist, fitness_hist, rmse_hist);
    } else if constexpr (PLANE) {
      if (nblk > 0)
        hipLaunchKernelGGL(k_icp_match_plane, dim3(nblk), dim3(ICP_BLOCK), 0, st, P, src, tgt, tgt_normals, L.hdr, L.cell_start, L.sorted, r2, T,
                           done, slab, corr);
      hipLaunchKernelGGL(k_icp_update_plane, dim3(S), dim3(ICP_BLOCK), 0, st, P, slab, k, max_iteration, relative_fitness, relative_rmse, T,
                         fitness, inlier_rmse, iterations, done, running, T_hist, fitness_hist, rmse_hist);
    } else {
      if (nblk > 0)
        hipLaunchKernelGGL(k_icp_match, dim3(nblk), dim3(ICP_BLOCK), 0, st, P, src, tgt, L.hdr, L.cell_start, L.sorted, r2, T, done, slab, corr);
      hipLaunchKernelGGL(k_icp_update, dim3(S), dim3(ICP_BLOCK), 0, st, P, src, tgt, slab, k, max_iteration, relative_fitness, relative_rmse, T,
                         fitness, inlier_rmse, iterations, done, running, T_hist, fitness_hist, rmse_hist);
    }
    if ((rc = check_launch(name))) return rc;
    if (check_every > 0 && k < max_iteration && (k + 1) % check_every == 0) {
      int32_t still = 0;
      if (hipMemcpyAsync(&still, running + (k & 1), sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        return refuse(LCR_EHIP, "%s: read-back of the running count failed", name);
      if (still == 0) break;
    }
  }
  return LCR_OK;
}
}  // namespace

extern "C" int lcr_icp_ws_bytes(int S, int64_t ns, int64_t nt, size_t* bytes) {
  return icp_ws_bytes("lcr_icp_ws_bytes", S, ns, nt, ICP_MOM, bytes);
}

extern "C" int lcr_icp_plane_ws_bytes(int S, int64_t ns, int64_t nt, size_t* bytes) {
  return icp_ws_bytes("lcr_icp_plane_ws_bytes", S, ns, nt, ICP_PLANE_MOM, bytes);
}

extern "C" int lcr_icp_point_to_point(const float* src, const int64_t* src_len, const float* tgt, const int64_t* tgt_len, int S, const double* init,
                                      float max_correspondence_distance, int max_iteration, double relative_fitness, double relative_rmse,
                                      double* T, double* fitness, double* inlier_rmse, int32_t* iterations, int32_t* corr, double* T_hist,
                                      double* fitness_hist, double* rmse_hist, int check_every, void* ws, size_t ws_bytes, void* stream) {
  return icp_run<IcpEst::POINT>("lcr_icp_point_to_point", src, src_len, nullptr, tgt, tgt_len, nullptr, S, init, max_correspondence_distance, 0.0,
                                max_iteration, relative_fitness, relative_rmse, T, fitness, inlier_rmse, iterations, corr, T_hist, fitness_hist,
                                rmse_hist, check_every, ws, ws_bytes, stream);
}

extern "C" int lcr_icp_point_to_plane(const float* src, const int64_t* src_len, const float* tgt, const int64_t* tgt_len, const float* tgt_normals,
                                      int S, const double* init, float max_correspondence_distance, int max_iteration, double relative_fitness,
                                      double relative_rmse, double* T, double* fitness, double* inlier_rmse, int32_t* iterations, int32_t* corr,
                                      double* T_hist, double* fitness_hist, double* rmse_hist, int check_every, void* ws, size_t ws_bytes,
                                      void* stream) {
  return icp_run<IcpEst::PLANE>("lcr_icp_point_to_plane", src, src_len, nullptr, tgt, tgt_len, tgt_normals, S, init, max_correspondence_distance,
                                0.0, max_iteration, relative_fitness, relative_rmse, T, fitness, inlier_rmse, iterations, corr, T_hist,
                                fitness_hist, rmse_hist, check_every, ws, ws_bytes, stream);
}

extern "C" int lcr_icp_generalized_ws_bytes(int S, int64_t ns, int64_t nt, size_t* bytes) {
  // never less than point-to-plane's answer: a workspace sized here serves all three estimators on the same shapes
  return icp_ws_bytes("lcr_icp_generalized_ws_bytes", S, ns, nt, std::max(ICP_GICP_MOM, ICP_PLANE_MOM), bytes);
}

extern "C" int lcr_icp_generalized(const float* src, const int64_t* src_len, const float* src_normals, const float* tgt, const int64_t* tgt_len,
                                   const float* tgt_normals, int S, const double* init, float max_correspondence_distance, double epsilon,
                                   int max_iteration, double relative_fitness, double relative_rmse, double* T, double* fitness,
                                   double* inlier_rmse, int32_t* iterations, int32_t* corr, double* T_hist, double* fitness_hist,
                                   double* rmse_hist, int check_every, void* ws, size_t ws_bytes, void* stream) {
  return icp_run<IcpEst::GICP>("lcr_icp_generalized", src, src_len, src_normals, tgt, tgt_len, tgt_normals, S, init, max_correspondence_distance,
                               epsilon, max_iteration, relative_fitness, relative_rmse, T, fitness, inlier_rmse, iterations, corr, T_hist,
                               fitness_hist, rmse_hist, check_every, ws, ws_bytes, stream);
}
