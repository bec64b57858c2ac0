// matching.hip — dustbin top-1 / top-K matching on the Sinkhorn output: per-line maxima against the dustbins, then the (b, i, j) pairs in
// row-major order by a count / scan / write pass.  Reference: geotransformer/superpoint_matching.py:130-162, local_global_registration.py:49-92.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace lcr {

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

}  // namespace lcr

using namespace lcr;

// Workspace of both matchers: per-line statistics (top-1: arg-max + "beats the dustbin" flag; top-K: the K-th value + its index), the
// per-row pair counts and their scan.  ws may be null (sizes only).
template <typename RowT, typename FlagT>
struct MatchLayout {
  RowT *   rowa, *cola;         // [B, M+1], [B, N+1]
  FlagT *  rowb, *colb;         // [B, M+1], [B, N+1]
  int32_t *counts, *offsets;    // [B*M + 1]
  void*    scan_ws;
  size_t   bytes;
};
template <typename RowT, typename FlagT>
static MatchLayout<RowT, FlagT> match_layout(void* ws, int64_t B, int M, int N) {
  MatchLayout<RowT, FlagT> L;
  Carver c(ws, ~size_t(0));
  L.rowa = c.take<RowT>(B * (M + 1));
  L.rowb = c.take<FlagT>(B * (M + 1));
  L.cola = c.take<RowT>(B * (N + 1));
  L.colb = c.take<FlagT>(B * (N + 1));
  L.counts = c.take<int32_t>(B * M + 1);
  L.offsets = c.take<int32_t>(B * M + 1);
  L.scan_ws = c.take<char>(scan_ws_bytes(B * M + 1));
  L.bytes = c.off;
  return L;
}
static auto top1_layout(void* ws, int64_t B, int M, int N) { return match_layout<int32_t, uint8_t>(ws, B, M, N); }   // rowarg, rowbeat, colarg, colbeat
static auto topk_layout(void* ws, int64_t B, int M, int N) { return match_layout<float, int32_t>(ws, B, M, N); }     // rowv, rowj, colv, coli

extern "C" int lcr_top1_matching_ws_bytes(int64_t B, int M, int N, size_t* bytes) {
  if (!bytes || B < 1 || M < 1 || N < 1)
    return refuse(LCR_EARG, "lcr_top1_matching_ws_bytes: null pointer or outside the domain (B, M, N >= 1): B=%lld M=%d N=%d", static_cast<long long>(B), M, N);
  *bytes = top1_layout(nullptr, B, M, N).bytes;
  return LCR_OK;
}

// The body of lcr_top1_matching and lcr_top1_matching_ex; `who` = the one that was called.
// Two-phase: out_bij == NULL -> only *total (device i64) is produced (and the per-row offsets kept in ws);
// then call again with buffers of `total` entries.  (b,i,j) triplets in row-major order; scores in the exp domain.
// mutual != 0: a pair is kept only if it is BOTH its row's and its column's dustbin-beating maximum (LocalGlobalRegistration(mutual=True),
// local_global_registration.py:84-85); 0: either (the shipped configuration)
static int top1_matching(const char* who, const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int mutual,
                         int64_t* total, int32_t* out_bij, float* out_score, void* ws, size_t ws_bytes, void* stream) {
  if (!logS || !ws || B < 1 || M < 1 || N < 1 || (!out_bij && !total))
    return refuse(LCR_EARG, "%s: null pointer (out_bij or total is needed) or outside the domain (B, M, N >= 1): B=%lld M=%d N=%d", who,
                  static_cast<long long>(B), M, N);
  const auto L = top1_layout(ws, B, M, N);
  if (L.bytes > ws_bytes) return refuse_ws(LCR_ESPACE, who, ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  if (!out_bij) {
    const int slices = B >= 64 ? 1 : std::max(1, std::min(32, (M + 1 + 15) / 16));
    if (M + 1 <= T1S_MAX && N + 1 <= T1S_MAX)
      hipLaunchKernelGGL(k_top1_stats_small, dim3(static_cast<int>(B)), dim3(256), 0, st, logS, M, N, L.rowa, L.rowb, L.cola, L.colb);
    else
      hipLaunchKernelGGL(k_top1_stats, dim3(static_cast<int>(B), slices), dim3(256), 0, st, logS, M, N, L.rowa, L.rowb, L.cola, L.colb);
    hipLaunchKernelGGL((k_top1_emit<0>), dim3(blocks_for(B * M)), dim3(256), 0, st, logS, B, M, N, L.rowa, L.rowb, L.cola, L.colb, row_mask, col_mask,
                       L.counts, L.offsets, out_bij, out_score, mutual);
    hipMemsetAsync(L.counts + B * M, 0, sizeof(int32_t), st);
    int rc = exclusive_scan_i32(who, L.counts, L.offsets, B * M + 1, total, L.scan_ws, st);
    if (rc) return rc;
  } else {
    hipLaunchKernelGGL((k_top1_emit<1>), dim3(blocks_for(B * M)), dim3(256), 0, st, logS, B, M, N, L.rowa, L.rowb, L.cola, L.colb, row_mask, col_mask,
                       L.counts, L.offsets, out_bij, out_score, mutual);
  }
  return check_launch(who);
}

extern "C" int lcr_top1_matching(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int64_t* total,
                                 int32_t* out_bij, float* out_score, void* ws, size_t ws_bytes, void* stream) {
  return top1_matching("lcr_top1_matching", logS, B, M, N, row_mask, col_mask, 0, total, out_bij, out_score, ws, ws_bytes, stream);
}

extern "C" int lcr_top1_matching_ex(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int mutual,
                                    int64_t* total, int32_t* out_bij, float* out_score, void* ws, size_t ws_bytes, void* stream) {
  return top1_matching("lcr_top1_matching_ex", logS, B, M, N, row_mask, col_mask, mutual, total, out_bij, out_score, ws, ws_bytes, stream);
}

extern "C" int lcr_topk_matching_ws_bytes(int64_t B, int M, int N, size_t* bytes) {
  if (!bytes || B < 1 || M < 1 || N < 1)
    return refuse(LCR_EARG, "lcr_topk_matching_ws_bytes: null pointer or outside the domain (B, M, N >= 1): B=%lld M=%d N=%d", static_cast<long long>(B), M, N);
  *bytes = topk_layout(nullptr, B, M, N).bytes;
  return LCR_OK;
}

// The body of lcr_topk_matching and lcr_topk_matching_ex; `who` = the one that was called.
// dustbin top-K matching (K >= 1), two-phase like lcr_top1_matching; for K = 1 the rows equal lcr_top1_matching_ex's;
// every switch of LocalGlobalRegistration.compute_correspondence_matrix (local_global_registration.py:48-93) + use_global_score (:236-237):
// use_dustbin = 0 takes the K largest over the M x N interior and keeps what exceeds confidence_threshold; global_scores [B] (or NULL)
// multiplies the emitted scores of patch pair b
static int topk_matching(const char* who, const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int K,
                         int mutual, int use_dustbin, float confidence_threshold, const float* global_scores, int64_t* total, int32_t* out_bij,
                         float* out_score, void* ws, size_t ws_bytes, void* stream) {
  if (!logS || !ws || B < 1 || M < 1 || N < 1 || K < 1 || (!out_bij && !total))
    return refuse(LCR_EARG, "%s: null pointer (out_bij or total is needed) or outside the domain (B, M, N, K >= 1): B=%lld M=%d N=%d K=%d", who,
                  static_cast<long long>(B), M, N, K);
  const auto L = topk_layout(ws, B, M, N);
  if (L.bytes > ws_bytes) return refuse_ws(LCR_ESPACE, who, ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  const int dust = use_dustbin ? 1 : 0;
  if (!out_bij) {
    const int slices = B >= 64 ? 1 : std::max(1, std::min(32, (M + 1 + 15) / 16));
    hipLaunchKernelGGL(k_topk_stats, dim3(static_cast<int>(B), slices), dim3(256), 0, st, logS, M, N, K, dust, L.rowa, L.rowb, L.cola, L.colb);
    hipLaunchKernelGGL((k_topk_emit<0>), dim3(blocks_for(B * M)), dim3(256), 0, st, logS, B, M, N, L.rowa, L.rowb, L.cola, L.colb, row_mask, col_mask, L.counts,
                       L.offsets, out_bij, out_score, mutual, dust, confidence_threshold, global_scores);
    hipMemsetAsync(L.counts + B * M, 0, sizeof(int32_t), st);
    int rc = exclusive_scan_i32(who, L.counts, L.offsets, B * M + 1, total, L.scan_ws, st);
    if (rc) return rc;
  } else {
    hipLaunchKernelGGL((k_topk_emit<1>), dim3(blocks_for(B * M)), dim3(256), 0, st, logS, B, M, N, L.rowa, L.rowb, L.cola, L.colb, row_mask, col_mask, L.counts,
                       L.offsets, out_bij, out_score, mutual, dust, confidence_threshold, global_scores);
  }
  return check_launch(who);
}

extern "C" int lcr_topk_matching(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int K, int mutual,
                                 int64_t* total, int32_t* out_bij, float* out_score, void* ws, size_t ws_bytes, void* stream) {
  return topk_matching("lcr_topk_matching", logS, B, M, N, row_mask, col_mask, K, mutual, 1, 0.f, nullptr, total, out_bij, out_score, ws, ws_bytes, stream);
}

extern "C" int lcr_topk_matching_ex(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int K, int mutual,
                                    int use_dustbin, float confidence_threshold, const float* global_scores, int64_t* total, int32_t* out_bij,
                                    float* out_score, void* ws, size_t ws_bytes, void* stream) {
  return topk_matching("lcr_topk_matching_ex", logS, B, M, N, row_mask, col_mask, K, mutual, use_dustbin, confidence_threshold, global_scores, total,
                       out_bij, out_score, ws, ws_bytes, stream);
}

