// teaser.hip — TEASER-style robust registration from correspondences (experiments/registration/eval.py:197-218 runs TEASER++ with
// GNC-TLS rotation), batched over problems.  The definition (consistency graph, k-core selection, GNC-TLS rotation over all pairs of the
// selected rows, truncated-least-squares voting of the translation) is stated in include/lcr_hip.h next to lcr_teaser_registration.
// All arithmetic is fp64 on the fp32 rows; no floating-point atomic anywhere, every sum has one order that depends on the problem alone.
//
// Stream-ordered launches, no host synchronisation, no allocation:
//   k_tz_graph      (kcore) one workgroup per (row i, problem): lane l of a wavefront tests the pair (i, 64 w + l), the ballot is word w of
//                   row i of the bit adjacency (N^2 / 8 bytes per problem), the popcounts are the degree;
//   k_tz_select     one workgroup per problem.  kcore: peels the graph in LDS — each round removes every live vertex of degree <= k
//                   (k jumps to the smallest live degree when nobody is at or below it) and walks only the removed vertices' adjacency
//                   rows to decrement their live neighbours (integer LDS atomics; at most N rounds) — then lists {core = k_max} in
//                   ascending order.  none: lists every row.  Gathers the selected rows and initialises the problem's GNC state;
//   k_tz_sweep      the hot path, max_iterations + 2 launches.  Workgroup b of a problem owns the measurements (i, j > i) of the rows
//                   i = b and i = K - 2 - b (K of them: the triangle is balanced), recomputed from the selected points every pass.  The
//                   weights are not stored: w at pass t is a function of the residual under the previous rotation and the previous mu,
//                   so a pass holds two rotations and accumulates the cost of this iteration and H of the next together;
//   k_tz_step       one workgroup per problem after every sweep: adds the workgroups' partials in index order, fits the rotation
//                   (rigid3.h), applies the exit test and advances mu.  A stopped problem's later sweeps and steps exit at once;
//   k_tz_vote_prep / k_tz_vote_rank / k_tz_vote_scan   x = ref - R src per axis, the rank of each of the 2K interval endpoints in the
//                   total order (value, position) by counting, then ordered prefix sums of (+-1, +-x, +-x^2) with x centred on the axis's
//                   first value and the arg-min of the TLS cost (earliest endpoint wins ties).
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"
#include "rigid3.h"

namespace lcr {

constexpr int TZ_MAX_ROWS = 4096;    // rows per problem at most (the bit adjacency is then 2 MB per problem, the peel's LDS 49 KB)
constexpr int TZ_SEL_T = 1024;       // threads of k_tz_select and k_tz_vote_scan
constexpr int TZ_PART = 12;          // doubles per sweep partial: H[9], cost, max residual, count of weights >= 0.5 (as int64 bits)

struct TzState {
  double Rp[9], Rc[9];               // rotation of the previous / the current iteration
  double mu_p, mu_c, cost_prev, cost_last;
  long long rot_inl;
  int phase;                         // 0: H of the unit weights, 1: max residual -> mu, 2: the GNC loop, 3: stopped
  int it, K, valid, iters, pad;
};

struct TzParams {
  double beta, rho, c2, gnc_factor, cost_threshold;
  int max_iterations, mode, max_rows, wpr;   // wpr: 64-bit adjacency words per row = ceil(max_rows / 64)
};

__device__ __forceinline__ double tz_len(const float* __restrict__ p, int64_t i, int64_t j) {
  const double dx = static_cast<double>(p[3 * j]) - static_cast<double>(p[3 * i]);
  const double dy = static_cast<double>(p[3 * j + 1]) - static_cast<double>(p[3 * i + 1]);
  const double dz = static_cast<double>(p[3 * j + 2]) - static_cast<double>(p[3 * i + 2]);
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// grid (max_rows, S), 256 threads: row i = blockIdx.x of problem blockIdx.y
__global__ __launch_bounds__(256) void k_tz_graph(const float* __restrict__ src, const float* __restrict__ ref, const int32_t* __restrict__ start,
                                                  TzParams P, uint64_t* __restrict__ adj, int32_t* __restrict__ deg) {
  __shared__ int s_d[4];
  const int s = blockIdx.y, i = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t a0 = start[s];
  const int N = start[s + 1] - start[s];
  if (N > P.max_rows || i >= N) return;                   // block-uniform
  const int W = (N + 63) >> 6;
  uint64_t* row = adj + (static_cast<int64_t>(s) * P.max_rows + i) * P.wpr;
  int d = 0;
  for (int w = wv; w < W; w += 4) {
    const int j = 64 * w + lane;
    bool e = false;
    if (j < N && j != i) e = fabs(tz_len(src, a0 + i, a0 + j) - tz_len(ref, a0 + i, a0 + j)) <= P.beta;
    const uint64_t m = wave_ballot(e);
    if (lane == 0) row[w] = m;
    d += __popcll(m);
  }
  if (lane == 0) s_d[wv] = d;
  __syncthreads();
  if (threadIdx.x == 0) deg[static_cast<int64_t>(s) * P.max_rows + i] = s_d[0] + s_d[1] + s_d[2] + s_d[3];
}

// one workgroup of TZ_SEL_T threads per problem: core numbers, the selected rows in ascending order, their gathered points
// (pts[(s * max_rows + q) * 6] = src xyz, ref xyz of the q-th selected row), the GNC state and the selection outputs
__global__ __launch_bounds__(TZ_SEL_T) void k_tz_select(const float* __restrict__ src, const float* __restrict__ ref, const int32_t* __restrict__ start,
                                                        TzParams P, const uint64_t* __restrict__ adj, const int32_t* __restrict__ deg_in,
                                                        TzState* __restrict__ state, float* __restrict__ pts, int32_t* __restrict__ n_selected,
                                                        uint8_t* __restrict__ selected_mask, int32_t* __restrict__ core_out) {
  __shared__ int s_deg[TZ_MAX_ROWS], s_core[TZ_MAX_ROWS], s_rem[TZ_MAX_ROWS];
  __shared__ unsigned long long s_live[TZ_MAX_ROWS / 64];
  __shared__ int s_red[TZ_SEL_T / 64], s_cnt;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t a0 = start[s];
  const int Nraw = start[s + 1] - start[s];
  const bool fits = Nraw >= 0 && Nraw <= P.max_rows;
  const int N = fits ? Nraw : 0;                          // a problem over the caller's bound is invalid and touches no table
  const int W = (N + 63) >> 6;
  int kmax = 0;
  if (P.mode == 0) {
    for (int v = tid; v < N; v += TZ_SEL_T) {
      s_deg[v] = deg_in[static_cast<int64_t>(s) * P.max_rows + v];
      s_core[v] = 0;
    }
    for (int w = tid; w < W; w += TZ_SEL_T) s_live[w] = (w == W - 1 && (N & 63)) ? ((1ull << (N & 63)) - 1ull) : ~0ull;
    __syncthreads();
    int k = 0, remaining = N;
    for (int round = 0; round < N && remaining > 0; ++round) {       // every round removes at least one vertex
      int m = INT_MAX;
      for (int v = tid; v < N; v += TZ_SEL_T)
        if ((s_live[v >> 6] >> (v & 63)) & 1ull) m = min(m, s_deg[v]);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) m = min(m, __shfl_xor(m, d));
      if (lane == 0) s_red[wv] = m;
      if (tid == 0) s_cnt = 0;
      __syncthreads();
      m = s_red[0];
      for (int q = 1; q < TZ_SEL_T / 64; ++q) m = min(m, s_red[q]);
      k = max(k, m);
      for (int v = tid; v < N; v += TZ_SEL_T)
        if (((s_live[v >> 6] >> (v & 63)) & 1ull) && s_deg[v] <= k) {
          s_rem[atomicAdd(&s_cnt, 1)] = v;
          s_core[v] = k;
        }
      __syncthreads();
      const int nr = s_cnt;
      for (int q = tid; q < nr; q += TZ_SEL_T) atomicAnd(&s_live[s_rem[q] >> 6], ~(1ull << (s_rem[q] & 63)));
      __syncthreads();
      for (int q = wv; q < nr; q += TZ_SEL_T / 64) {      // subtract the removed rows from their live neighbours' degrees
        const uint64_t* row = adj + (static_cast<int64_t>(s) * P.max_rows + s_rem[q]) * P.wpr;
        for (int w = lane; w < W; w += 64) {
          uint64_t bits = row[w] & s_live[w];
          while (bits) {
            atomicSub(&s_deg[64 * w + __builtin_ctzll(bits)], 1);
            bits &= bits - 1;
          }
        }
      }
      __syncthreads();
      remaining -= nr;
    }
    kmax = k;
  }
  // the selected rows in ascending order
  const bool graph_ok = P.mode != 0 || kmax >= 1;
  int base = 0;
  for (int v0 = 0; v0 < N; v0 += TZ_SEL_T) {              // block-uniform trip count
    const int v = v0 + tid;
    const bool keep = v < N && graph_ok && (P.mode != 0 || s_core[v] == kmax);
    const uint64_t bm = wave_ballot(keep);
    __syncthreads();
    if (lane == 0) s_red[wv] = __popcll(bm);
    __syncthreads();
    int off = base + mbcnt_lt(bm);
    for (int q = 0; q < wv; ++q) off += s_red[q];
    if (keep) s_rem[off] = v;
    for (int q = 0; q < TZ_SEL_T / 64; ++q) base += s_red[q];
  }
  __syncthreads();
  const int K = base;
  const bool valid = fits && graph_ok && K >= 3;
  for (int q = tid; q < K; q += TZ_SEL_T) {
    const int64_t g = a0 + s_rem[q];
    float* o = pts + (static_cast<int64_t>(s) * P.max_rows + q) * 6;
    for (int d = 0; d < 3; ++d) {
      o[d] = src[3 * g + d];
      o[3 + d] = ref[3 * g + d];
    }
  }
  if (fits) {
    for (int v = tid; v < N; v += TZ_SEL_T) {
      if (selected_mask) selected_mask[a0 + v] = valid && (P.mode != 0 || s_core[v] == kmax) ? 1 : 0;
      if (core_out) core_out[a0 + v] = P.mode == 0 ? s_core[v] : 0;
    }
  } else if (Nraw > 0) {
    for (int64_t v = tid; v < Nraw; v += TZ_SEL_T) {
      if (selected_mask) selected_mask[a0 + v] = 0;
      if (core_out) core_out[a0 + v] = 0;
    }
  }
  if (tid == 0) {
    TzState* st = state + s;
    for (int q = 0; q < 9; ++q) st->Rp[q] = st->Rc[q] = (q % 4 == 0) ? 1.0 : 0.0;
    st->mu_p = st->mu_c = 0.0;
    st->cost_prev = INFINITY;
    st->cost_last = 0.0;
    st->rot_inl = 0;
    st->phase = valid ? 0 : 3;
    st->it = 0;
    st->K = valid ? K : 0;
    st->valid = valid ? 1 : 0;
    st->iters = 0;
    st->pad = 0;
    n_selected[s] = valid ? K : 0;
  }
}

// the GNC-TLS weight of a residual r at (mu, c2): 0 above th1, 1 below th2, sqrt(c2 mu (mu + 1) / r) - mu between
__device__ __forceinline__ double tz_weight(double r, double mu, double c2, double th1, double th2) {
  if (r >= th1) return 0.0;
  if (r <= th2) return 1.0;
  return sqrt(c2 * mu * (mu + 1.0) / r) - mu;
}

__device__ __forceinline__ double tz_residual(const double* R, const double a[3], const double b[3]) {
  const double ex = b[0] - ((R[0] * a[0] + R[1] * a[1]) + R[2] * a[2]);
  const double ey = b[1] - ((R[3] * a[0] + R[4] * a[1]) + R[5] * a[2]);
  const double ez = b[2] - ((R[6] * a[0] + R[7] * a[1]) + R[8] * a[2]);
  return (ex * ex + ey * ey) + ez * ez;
}

// grid (max(1, max_rows / 2), S), 256 threads.  part[(s * pstride + b) * TZ_PART ..]
__global__ __launch_bounds__(256) void k_tz_sweep(const TzState* __restrict__ state, const float* __restrict__ pts, TzParams P, int pstride,
                                                  double* __restrict__ part) {
  __shared__ double s_p[4][TZ_PART];
  const int s = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const TzState* st = state + s;
  const int phase = st->phase;
  if (phase == 3) return;                                 // stopped (or invalid): nothing to do
  const int K = st->K;
  if (b >= K / 2) return;
  double Rp[9], Rc[9];
  for (int q = 0; q < 9; ++q) {
    Rp[q] = st->Rp[q];
    Rc[q] = st->Rc[q];
  }
  const double mu_p = st->mu_p, mu_c = st->mu_c, c2 = P.c2;
  const bool first = st->it == 0;
  const double th1p = (mu_p + 1.0) / mu_p * c2, th2p = mu_p / (mu_p + 1.0) * c2;
  const double th1c = (mu_c + 1.0) / mu_c * c2, th2c = mu_c / (mu_c + 1.0) * c2;
  const float* p = pts + static_cast<int64_t>(s) * P.max_rows * 6;
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cost = 0.0, rmax = 0.0;
  long long cnt = 0;
  const int i2 = K - 2 - b;
  for (int half = 0; half < 2; ++half) {
    const int i = half == 0 ? b : i2;
    if (half == 1 && i2 == b) break;
    const double si[3] = {p[6 * i], p[6 * i + 1], p[6 * i + 2]}, ri[3] = {p[6 * i + 3], p[6 * i + 4], p[6 * i + 5]};
    for (int j = i + 1 + tid; j < K; j += 256) {
      double a[3], bb[3];
      for (int d = 0; d < 3; ++d) {
        a[d] = static_cast<double>(p[6 * j + d]) - si[d];
        bb[d] = static_cast<double>(p[6 * j + 3 + d]) - ri[d];
      }
      double wn = 1.0;                                    // the weight that enters H
      if (phase != 0) {
        const double r = tz_residual(Rc, a, bb);
        rmax = fmax(rmax, r);
        double wc = 1.0;                                  // the weight that produced Rc
        if (phase == 2 && !first) wc = tz_weight(tz_residual(Rp, a, bb), mu_p, c2, th1p, th2p);
        cost += wc * r;
        if (phase == 2) {
          wn = tz_weight(r, mu_c, c2, th1c, th2c);
          cnt += wn >= 0.5 ? 1 : 0;
        }
      }
      if (phase != 1) {
        const double wa[3] = {wn * a[0], wn * a[1], wn * a[2]};
        for (int r3 = 0; r3 < 3; ++r3)
          for (int c3 = 0; c3 < 3; ++c3) H[3 * r3 + c3] += wa[r3] * bb[c3];
      }
    }
  }
  for (int q = 0; q < 9; ++q) H[q] = wave_sum(H[q]);
  cost = wave_sum(cost);
  cnt = wave_sum(cnt);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, d));
  if (lane == 0) {
    for (int q = 0; q < 9; ++q) s_p[wv][q] = H[q];
    s_p[wv][9] = cost;
    s_p[wv][10] = rmax;
    s_p[wv][11] = __longlong_as_double(cnt);
  }
  __syncthreads();
  if (tid < TZ_PART) {
    double* o = part + (static_cast<int64_t>(s) * pstride + b) * TZ_PART;
    if (tid == 10) {
      o[tid] = fmax(fmax(s_p[0][10], s_p[1][10]), fmax(s_p[2][10], s_p[3][10]));
    } else if (tid == 11) {
      long long c = 0;
      for (int w = 0; w < 4; ++w) c += __double_as_longlong(s_p[w][11]);
      o[tid] = __longlong_as_double(c);
    } else {
      o[tid] = ((s_p[0][tid] + s_p[1][tid]) + s_p[2][tid]) + s_p[3][tid];
    }
  }
}

// grid (S), 256 threads: the K / 2 partials of the sweep in index order (thread t adds b = t, t + 256, ... in order, then a fixed tree),
// then the state machine of the definition
__global__ __launch_bounds__(256) void k_tz_step(TzState* __restrict__ state, TzParams P, int pstride, const double* __restrict__ part) {
  __shared__ double s_p[256][TZ_PART + 1];
  const int s = blockIdx.x, tid = threadIdx.x;
  TzState* st = state + s;
  const int phase = st->phase;
  if (phase == 3) return;
  const int nb = st->K / 2;
  double acc[TZ_PART];
  for (int q = 0; q < TZ_PART; ++q) acc[q] = 0.0;
  long long cnt = 0;
  for (int b = tid; b < nb; b += 256) {
    const double* o = part + (static_cast<int64_t>(s) * pstride + b) * TZ_PART;
    for (int q = 0; q < 10; ++q) acc[q] += o[q];
    acc[10] = fmax(acc[10], o[10]);
    cnt += __double_as_longlong(o[11]);
  }
  for (int q = 0; q < 11; ++q) s_p[tid][q] = acc[q];
  s_p[tid][11] = __longlong_as_double(cnt);
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) {
      for (int q = 0; q < 10; ++q) s_p[tid][q] += s_p[tid + h][q];
      s_p[tid][10] = fmax(s_p[tid][10], s_p[tid + h][10]);
      s_p[tid][11] = __longlong_as_double(__double_as_longlong(s_p[tid][11]) + __double_as_longlong(s_p[tid + h][11]));
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double cost = s_p[0][9], rmax = s_p[0][10];
  const long long inl = __double_as_longlong(s_p[0][11]);
  double H[3][3], R[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) H[r][c] = s_p[0][3 * r + c];
  if (phase == 0) {
    rotation_from_H(H, R);
    for (int q = 0; q < 9; ++q) st->Rc[q] = R[q / 3][q % 3];
    st->phase = 1;
  } else if (phase == 1) {
    const double mu = 1.0 / (2.0 * rmax / P.c2 - 1.0);
    if (!(mu > 0.0)) {                                    // step 3: stop at iteration 0 and keep R; every weight is still 1
      const long long K = st->K;
      st->phase = 3;
      st->iters = 1;
      st->cost_last = cost;
      st->rot_inl = K * (K - 1) / 2;
    } else {
      st->mu_c = mu;
      st->it = 0;
      st->phase = 2;
    }
  } else {
    const int it = st->it;
    const double d = fabs(cost - st->cost_prev);
    st->cost_last = cost;
    st->iters = it + 1;
    st->rot_inl = inl;
    if (d < P.cost_threshold || it + 1 >= P.max_iterations) {
      st->phase = 3;
    } else {
      rotation_from_H(H, R);
      for (int q = 0; q < 9; ++q) {
        st->Rp[q] = st->Rc[q];
        st->Rc[q] = R[q / 3][q % 3];
      }
      st->mu_p = st->mu_c;
      st->mu_c = st->mu_c * P.gnc_factor;
      st->cost_prev = cost;
      st->it = it + 1;
    }
  }
}

// grid (max(1, ceil(max_rows / 256)), S): x[(s * 3 + axis) * max_rows + q] = ref - R src of the q-th selected row; block 0 writes the
// rotation part of T and the per-problem outputs that the GNC state holds
__global__ __launch_bounds__(256) void k_tz_vote_prep(const TzState* __restrict__ state, const float* __restrict__ pts, TzParams P,
                                                      double* __restrict__ x, float* __restrict__ T, int32_t* __restrict__ valid,
                                                      long long* __restrict__ rot_inliers, int32_t* __restrict__ iterations,
                                                      double* __restrict__ cost) {
  const int s = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
  const TzState* st = state + s;
  const int K = st->K;
  if (q < K) {
    const float* p = pts + (static_cast<int64_t>(s) * P.max_rows + q) * 6;
    const double a[3] = {p[0], p[1], p[2]};
    for (int r = 0; r < 3; ++r)
      x[(static_cast<int64_t>(s) * 3 + r) * P.max_rows + q] =
          static_cast<double>(p[3 + r]) - ((st->Rc[3 * r] * a[0] + st->Rc[3 * r + 1] * a[1]) + st->Rc[3 * r + 2] * a[2]);
  }
  if (q == 0) {
    float* o = T + 16 * s;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) o[4 * r + c] = st->valid ? static_cast<float>(st->Rc[3 * r + c]) : (r == c ? 1.f : 0.f);
    o[12] = o[13] = o[14] = 0.f;
    o[15] = 1.f;
    valid[s] = st->valid;
    rot_inliers[s] = st->valid ? st->rot_inl : 0;
    if (iterations) iterations[s] = st->valid ? st->iters : 0;
    if (cost) cost[s] = st->valid ? st->cost_last : 0.0;
  }
}

__device__ __forceinline__ double tz_endpoint(const double* __restrict__ xa, int K, int p, double rho) {
  return p < K ? xa[p] - rho : xa[p - K] + rho;
}

// grid (max(1, ceil(2 max_rows / 256)), 3, S): order[(s * 3 + axis) * 2 max_rows + rank of endpoint p] = p
__global__ __launch_bounds__(256) void k_tz_vote_rank(const TzState* __restrict__ state, TzParams P, const double* __restrict__ x,
                                                      int32_t* __restrict__ order) {
  __shared__ double s_v[256];
  const int s = blockIdx.z, axis = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const int K = state[s].K, E = 2 * K;
  if (blockIdx.x * 256 >= E) return;                      // block-uniform
  const double* xa = x + (static_cast<int64_t>(s) * 3 + axis) * P.max_rows;
  const double v = p < E ? tz_endpoint(xa, K, p, P.rho) : 0.0;
  int rank = 0;
  for (int q0 = 0; q0 < E; q0 += 256) {
    __syncthreads();
    if (q0 + threadIdx.x < E) s_v[threadIdx.x] = tz_endpoint(xa, K, q0 + threadIdx.x, P.rho);
    __syncthreads();
    const int qn = min(256, E - q0);
    for (int q = 0; q < qn; ++q) {
      const double u = s_v[q];
      rank += (u < v || (u == v && q0 + q < p)) ? 1 : 0;
    }
  }
  if (p < E) order[(static_cast<int64_t>(s) * 3 + axis) * 2 * P.max_rows + rank] = p;
}

// grid (3, S), TZ_SEL_T threads: thread t owns the sorted endpoints [t e, (t + 1) e), e = ceil(2K / TZ_SEL_T)
__global__ __launch_bounds__(TZ_SEL_T) void k_tz_vote_scan(const TzState* __restrict__ state, TzParams P, const double* __restrict__ x,
                                                           const int32_t* __restrict__ order, float* __restrict__ T,
                                                           int32_t* __restrict__ t_count) {
  __shared__ double s_1[TZ_SEL_T / 64], s_2[TZ_SEL_T / 64], s_c[TZ_SEL_T / 64];
  __shared__ int s_n[TZ_SEL_T / 64], s_e[TZ_SEL_T / 64], s_m[TZ_SEL_T / 64];
  __shared__ double s_x[TZ_SEL_T / 64];
  const int axis = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int K = state[s].K, E = 2 * K;
  if (K == 0) {                                           // invalid problem: no translation, no count
    if (tid == 0) {
      T[16 * s + 4 * axis + 3] = 0.f;
      t_count[3 * s + axis] = 0;
    }
    return;
  }
  const double* xa = x + (static_cast<int64_t>(s) * 3 + axis) * P.max_rows;
  const int32_t* ord = order + (static_cast<int64_t>(s) * 3 + axis) * 2 * P.max_rows;
  const double x0 = xa[0], rho2 = P.rho * P.rho;
  const int per = (E + TZ_SEL_T - 1) / TZ_SEL_T, e0 = min(E, tid * per), e1 = min(E, e0 + per);
  int n = 0;
  double a1 = 0.0, a2 = 0.0;
  for (int e = e0; e < e1; ++e) {
    int p = ord[e];
    if (static_cast<unsigned>(p) >= static_cast<unsigned>(E)) p = 0;   // a NaN coordinate leaves ranks unwritten: stay inside the tables
    const double xc = xa[p < K ? p : p - K] - x0;
    if (p < K) {
      n += 1, a1 += xc, a2 += xc * xc;
    } else {
      n -= 1, a1 -= xc, a2 -= xc * xc;
    }
  }
  // exclusive prefix over the threads: inside the wavefront, then the wavefronts in order
  const int in_n = wave_incl_scan(n);
  const double in_1 = wave_incl_scan(a1), in_2 = wave_incl_scan(a2);
  if (lane == 63) {
    s_n[wv] = in_n;
    s_1[wv] = in_1;
    s_2[wv] = in_2;
  }
  __syncthreads();
  int pn = in_n - n;
  double p1 = in_1 - a1, p2 = in_2 - a2;
  {
    int bn = 0;
    double b1 = 0.0, b2 = 0.0;
    for (int w = 0; w < wv; ++w) {
      bn += s_n[w];
      b1 += s_1[w];
      b2 += s_2[w];
    }
    pn += bn;
    p1 = b1 + p1;
    p2 = b2 + p2;
  }
  double best = INFINITY, best_x = 0.0;
  int best_e = INT_MAX, best_n = 0;
  for (int e = e0; e < e1; ++e) {
    int p = ord[e];
    if (static_cast<unsigned>(p) >= static_cast<unsigned>(E)) p = 0;
    const double xc = xa[p < K ? p : p - K] - x0;
    if (p < K) {
      pn += 1, p1 += xc, p2 += xc * xc;
    } else {
      pn -= 1, p1 -= xc, p2 -= xc * xc;
    }
    if (pn > 0) {
      const double mean = p1 / pn;
      const double c = (p2 - p1 * mean) + rho2 * static_cast<double>(K - pn);
      if (c < best) {
        best = c;
        best_e = e;
        best_n = pn;
        best_x = x0 + mean;
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double oc = __shfl_xor(best, d), ox = __shfl_xor(best_x, d);
    const int oe = __shfl_xor(best_e, d), on = __shfl_xor(best_n, d);
    if (oc < best || (oc == best && oe < best_e)) {
      best = oc;
      best_x = ox;
      best_e = oe;
      best_n = on;
    }
  }
  __syncthreads();
  if (lane == 0) {
    s_c[wv] = best;
    s_x[wv] = best_x;
    s_e[wv] = best_e;
    s_m[wv] = best_n;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < TZ_SEL_T / 64; ++w)
      if (s_c[w] < best || (s_c[w] == best && s_e[w] < best_e)) {
        best = s_c[w];
        best_x = s_x[w];
        best_e = s_e[w];
        best_n = s_m[w];
      }
    T[16 * s + 4 * axis + 3] = static_cast<float>(best_x);
    t_count[3 * s + axis] = best_n;
  }
}

}  // namespace lcr

using namespace lcr;

static int teaser_shape(const char* what, int S, int64_t n, int max_rows, int mode) {
  if (S < 1 || S > 65535 || n < 0 || max_rows < 0 || max_rows > TZ_MAX_ROWS || n > static_cast<int64_t>(S) * max_rows || mode < 0 || mode > 1)
    return refuse(LCR_EARG, "%s: outside the domain (1 <= S <= 65535, 0 <= max_rows <= %d rows per problem, 0 <= n <= S * max_rows, mode 0 = kcore or "
                  "1 = none): S=%d n=%lld max_rows=%d mode=%d", what, TZ_MAX_ROWS, S, static_cast<long long>(n), max_rows, mode);
  return LCR_OK;
}

struct TzCarve {
  TzState* state;
  float* pts;
  uint64_t* adj;
  int32_t* deg;
  double* part;
  double* x;
  int32_t* order;
  int pstride;
};

static size_t teaser_carve(Carver& c, int S, int max_rows, int mode, TzCarve* o) {
  const size_t rows = static_cast<size_t>(S) * std::max(max_rows, 1), wpr = static_cast<size_t>(div_up(std::max(max_rows, 1), 64));
  TzCarve t;
  t.pstride = std::max(1, max_rows / 2);
  t.state = c.take<TzState>(static_cast<size_t>(S));
  t.pts = c.take<float>(rows * 6);
  t.adj = mode == 0 ? c.take<uint64_t>(rows * wpr) : nullptr;
  t.deg = mode == 0 ? c.take<int32_t>(rows) : nullptr;
  t.part = c.take<double>(static_cast<size_t>(S) * t.pstride * TZ_PART);
  t.x = c.take<double>(rows * 3);
  t.order = c.take<int32_t>(rows * 6);
  if (o) *o = t;
  return c.off;
}

extern "C" int lcr_teaser_ws_bytes(int S, int64_t n, int max_rows, int mode, size_t* bytes) {
  if (!bytes) return refuse(LCR_EARG, "lcr_teaser_ws_bytes: null pointer");
  if (int rc = teaser_shape("lcr_teaser_ws_bytes", S, n, max_rows, mode)) return rc;
  Carver c(nullptr, ~size_t(0));
  *bytes = teaser_carve(c, S, max_rows, mode, nullptr);
  return LCR_OK;
}

extern "C" int lcr_teaser_registration(const float* src, const float* ref, const int32_t* start, int S, int64_t n, int max_rows,
                                       double noise_bound, double cbar2, double gnc_factor, int max_iterations, double cost_threshold, int mode,
                                       float* T, int32_t* valid, int32_t* n_selected, int64_t* rot_inliers, int32_t* t_count,
                                       int32_t* iterations, double* cost, uint8_t* selected_mask, int32_t* core, void* ws, size_t ws_bytes,
                                       void* stream) {
  const char* what = "lcr_teaser_registration";
  if (int rc = teaser_shape(what, S, n, max_rows, mode)) return rc;
  if (!(noise_bound > 0.0) || !(cbar2 > 0.0) || !(gnc_factor > 1.0) || !std::isfinite(noise_bound) || !std::isfinite(cbar2) ||
      !std::isfinite(gnc_factor) || max_iterations < 1 || max_iterations > 1000 || !(cost_threshold >= 0.0) || !std::isfinite(cost_threshold))
    return refuse(LCR_EARG, "%s: outside the domain (noise_bound > 0, cbar2 > 0, gnc_factor > 1, all finite, 1 <= max_iterations <= 1000, "
                  "cost_threshold >= 0): noise_bound=%g cbar2=%g gnc_factor=%g max_iterations=%d cost_threshold=%g", what, noise_bound, cbar2,
                  gnc_factor, max_iterations, cost_threshold);
  if (!start || !T || !valid || !n_selected || !rot_inliers || !t_count || !ws || (n > 0 && (!src || !ref))) return refuse(LCR_EARG, "%s: null pointer", what);
  TzCarve w;
  Carver c(ws, ws_bytes);
  const size_t need = teaser_carve(c, S, max_rows, mode, &w);
  if (need > ws_bytes) return refuse_ws(LCR_ESPACE, what, ws_bytes, need);
  TzParams P;
  P.beta = 2.0 * noise_bound * std::sqrt(cbar2);
  P.rho = noise_bound * std::sqrt(cbar2);
  P.c2 = noise_bound * noise_bound;
  P.gnc_factor = gnc_factor;
  P.cost_threshold = cost_threshold;
  P.max_iterations = max_iterations;
  P.mode = mode;
  P.max_rows = max_rows;
  P.wpr = div_up(std::max(max_rows, 1), 64);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (mode == 0 && max_rows > 0) hipLaunchKernelGGL(k_tz_graph, dim3(max_rows, S), dim3(256), 0, st, src, ref, start, P, w.adj, w.deg);
  hipLaunchKernelGGL(k_tz_select, dim3(S), dim3(TZ_SEL_T), 0, st, src, ref, start, P, w.adj, w.deg, w.state, w.pts, n_selected, selected_mask,
                     core);
  if (max_rows >= 3)
    for (int l = 0; l < max_iterations + 2; ++l) {         // fixed count: a stopped problem's launches exit at once
      hipLaunchKernelGGL(k_tz_sweep, dim3(w.pstride, S), dim3(256), 0, st, w.state, w.pts, P, w.pstride, w.part);
      hipLaunchKernelGGL(k_tz_step, dim3(S), dim3(256), 0, st, w.state, P, w.pstride, w.part);
    }
  hipLaunchKernelGGL(k_tz_vote_prep, dim3(std::max(1, div_up(max_rows, 256)), S), dim3(256), 0, st, w.state, w.pts, P, w.x, T, valid,
                     reinterpret_cast<long long*>(rot_inliers), iterations, cost);
  if (max_rows >= 3)
    hipLaunchKernelGGL(k_tz_vote_rank, dim3(std::max(1, div_up(2 * max_rows, 256)), 3, S), dim3(256), 0, st, w.state, P, w.x, w.order);
  hipLaunchKernelGGL(k_tz_vote_scan, dim3(3, S), dim3(TZ_SEL_T), 0, st, w.state, P, w.x, w.order, T, t_count);
  return check_launch(what);
}
