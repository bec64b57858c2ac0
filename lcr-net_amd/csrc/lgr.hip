// lgr.hip — the pose fit of the registration tail: batched weighted Procrustes, inlier counting / re-weighting, local-to-global registration.
// Reference: modules/registration/procrustes.py:6-73 (torch.svd on the CPU) + geotransformer/local_global_registration.py:134-200.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "rigid3.h"

namespace lcr {

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

// |ref_i - T src_i| of correspondence i under the row-major 4 x 4 transform t (the one expression of all four inlier kernels; the library is
// built with -ffp-contract=off, so products and sums round one by one, in this order)
__device__ __forceinline__ float residual(const float* __restrict__ t, const float* __restrict__ src, const float* __restrict__ ref, int i) {
  const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
  const float dx = ref[3 * i] - (t[0] * x + t[1] * y + t[2] * z + t[3]);
  const float dy = ref[3 * i + 1] - (t[4] * x + t[5] * y + t[6] * z + t[7]);
  const float dz = ref[3 * i + 2] - (t[8] * x + t[9] * y + t[10] * z + t[11]);
  return sqrtf(dx * dx + dy * dy + dz * dz);
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
    c += residual(t, src, ref, i) < radius ? 1 : 0;
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
    w_out[i] = residual(t, src, ref, i) < radius ? score[i] : 0.f;
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
    const int sg = cloud_of(seg_hyp_start, S, h);
    s_lo = seg_row_start[sg];
    s_hi = seg_row_start[sg + 1];
    s_c = 0;
  }
  __syncthreads();
  const float* t = T + 16 * h;
  int c = 0;
  for (int i = s_lo + threadIdx.x; i < s_hi; i += 256) {
    c += (residual(t, src, ref, i) < radius && (!ver_mask || ver_mask[i])) ? 1 : 0;     // rows of the verification set only
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
    const int sg = cloud_of(seg_row_start, S, i);
    const float* t = T_seg + 16 * sg;
    w_out[i] = residual(t, src, ref, i) < radius ? score[i] : 0.f;
  }
}

}  // namespace lcr

using namespace lcr;

extern "C" int lcr_procrustes_batched(const float* src, const float* ref, const float* w, const int32_t* start, int P, float eps, float* T, void* stream) {
  if (!src || !ref || !w || !start || !T || P < 1) return refuse(LCR_EARG, "lcr_procrustes_batched: null pointer or P < 1: P=%d", P);
  hipLaunchKernelGGL(k_procrustes, dim3(P), dim3(64), 0, ST(stream), src, ref, w, start, eps, T);
  return check_launch("lcr_procrustes_batched");
}

extern "C" int lcr_inlier_count(const float* T, int P, const float* src, const float* ref, int n, float radius, const int32_t* start, int min_count,
                                int32_t* counts, int32_t* best, void* stream) {
  if (!T || !counts || P < 1 || n < 0 || (n > 0 && (!src || !ref)))                        // no rows: nothing to read, null src / ref allowed
    return refuse(LCR_EARG, "lcr_inlier_count: null pointer, P < 1 or n < 0: P=%d n=%d", P, n);
  hipLaunchKernelGGL(k_inlier_count, dim3(P), dim3(256), 0, ST(stream), T, src, ref, n, radius, start, min_count, counts);
  if (best) hipLaunchKernelGGL(k_argmax_i32, dim3(1), dim3(64), 0, ST(stream), counts, P, best);
  return check_launch("lcr_inlier_count");
}

extern "C" int lcr_inlier_weights(const float* T_all, const int32_t* sel, const float* src, const float* ref, const float* score, int n, float radius,
                                  float* w_out, void* stream) {
  if (n == 0) return LCR_OK;                               // no rows: nothing to read or write, null pointers allowed
  if (!T_all || !src || !ref || !score || !w_out || n < 0) return refuse(LCR_EARG, "lcr_inlier_weights: null pointer or a negative count: n=%d", n);
  hipLaunchKernelGGL(k_inlier_weights, dim3(blocks_for(n)), dim3(256), 0, ST(stream), T_all, sel, src, ref, score, n, radius, w_out);
  return check_launch("lcr_inlier_weights");
}

// LocalGlobalRegistration.local_to_global_registration (geotransformer/local_global_registration.py:134-201) for S pairs at once:
// per-chunk hypotheses -> per-hypothesis inlier counts over the hypothesis's own pair -> best hypothesis per pair -> `steps`
// re-weighted refits.  ~2*steps + 5 launches whatever S is, no host synchronisation.  ws: lcr_lgr_ws_bytes(n, H, S).
struct LgrLayout {
  float *  hyp, *T_rows, *T_cur;   // hypotheses [H, 16]; per pair [S, 16]: the fit over all its rows, its current transform
  int32_t *counts, *seg_rows;      // inlier counts [H]; first row of every pair [S+1]
  float *  cur, *score_ver;        // [n] current weights; scores of the verification set (correspondence_limit)
  uint8_t* ver_mask;               // [n] its membership flags
  size_t   bytes;
};
static LgrLayout lgr_layout(void* ws, int64_t n, int H, int S) {
  LgrLayout L;
  Carver c(ws, ~size_t(0));
  const size_t rows = static_cast<size_t>(n > 0 ? n : 1);
  L.hyp = c.take<float>(static_cast<size_t>(H) * 16);
  L.counts = c.take<int32_t>(H);
  L.seg_rows = c.take<int32_t>(S + 1);
  L.T_rows = c.take<float>(static_cast<size_t>(S) * 16);
  L.T_cur = c.take<float>(static_cast<size_t>(S) * 16);
  L.cur = c.take<float>(rows);
  L.score_ver = c.take<float>(rows);
  L.ver_mask = c.take<uint8_t>(rows);
  L.bytes = c.off;
  return L;
}
extern "C" int lcr_lgr_ws_bytes(int64_t n, int H, int S, size_t* bytes) {
  if (!bytes || n < 0 || H < 1 || S < 1)
    return refuse(LCR_EARG, "lcr_lgr_ws_bytes: null pointer or outside the domain (n >= 0, H >= 1, S >= 1): n=%lld H=%d S=%d", static_cast<long long>(n), H, S);
  *bytes = lgr_layout(nullptr, n, H, S).bytes;
  return LCR_OK;
}
// the body of lcr_local_global_registration and lcr_local_global_registration_ex; `who` = the one that was called
// correspondence_limit > 0: the per-pair verification set of local_global_registration.py:152-160 (k_lgr_topl); 0 = every correspondence
static int local_global_registration(const char* who, const float* src, const float* ref, const float* score, int64_t n, const int32_t* hyp_start,
                                     int H, const int32_t* seg_hyp_start, int S, float radius, int min_count, int steps, int correspondence_limit,
                                     float* T_out, float* hyp_out, int32_t* counts_out, int32_t* best_out, void* ws, size_t ws_bytes, void* stream) {
  if (correspondence_limit < 0) return refuse(LCR_EARG, "%s: correspondence_limit must not be negative (%d)", who, correspondence_limit);
  if (!src || !ref || !score || !hyp_start || !seg_hyp_start || !T_out || !ws || n < 1 || H < 1 || S < 1 || steps < 1 || n > 2147483647)
    return refuse(LCR_EARG, "%s: bad argument", who);
  const LgrLayout L = lgr_layout(ws, n, H, S);
  if (L.bytes > ws_bytes) return refuse_ws(LCR_ESPACE, who, ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  const int ni = static_cast<int>(n);
  hipLaunchKernelGGL(k_lgr_seg_rows, dim3(1), dim3(64), 0, st, hyp_start, seg_hyp_start, S, L.seg_rows);
  const float* vscore = score;                     // scores of the verification set (zero outside it)
  const uint8_t* vmask = nullptr;
  if (correspondence_limit > 0) {
    hipLaunchKernelGGL(k_lgr_topl, dim3(S), dim3(256), 0, st, score, L.seg_rows, correspondence_limit, L.ver_mask, L.score_ver);
    vscore = L.score_ver;
    vmask = L.ver_mask;
  }
  hipLaunchKernelGGL(k_procrustes, dim3(H), dim3(64), 0, st, src, ref, score, hyp_start, 1e-5f, L.hyp);        // hypotheses: ALL correspondences (:175-178)
  hipLaunchKernelGGL(k_procrustes, dim3(S), dim3(64), 0, st, src, ref, vscore, L.seg_rows, 1e-5f, L.T_rows);     // degenerate branch (:186-190)
  hipLaunchKernelGGL(k_inlier_count_seg, dim3(H), dim3(256), 0, st, L.hyp, src, ref, radius, hyp_start, seg_hyp_start, L.seg_rows, S, min_count, L.counts, vmask);
  hipLaunchKernelGGL(k_lgr_select, dim3(S), dim3(64), 0, st, L.hyp, L.counts, seg_hyp_start, L.T_rows, L.T_cur, best_out);
  for (int it = 0; it < steps; ++it) {
    hipLaunchKernelGGL(k_inlier_weights_seg, dim3(blocks_for(n)), dim3(256), 0, st, L.T_cur, L.seg_rows, S, src, ref, vscore, ni, radius, L.cur);
    hipLaunchKernelGGL(k_procrustes, dim3(S), dim3(64), 0, st, src, ref, L.cur, L.seg_rows, 1e-5f, it + 1 == steps ? T_out : L.T_cur);
  }
  if (hyp_out) hipMemcpyAsync(hyp_out, L.hyp, sizeof(float) * 16 * H, hipMemcpyDeviceToDevice, st);
  if (counts_out) hipMemcpyAsync(counts_out, L.counts, sizeof(int32_t) * H, hipMemcpyDeviceToDevice, st);
  return check_launch(who);
}
extern "C" int lcr_local_global_registration(const float* src, const float* ref, const float* score, int64_t n, const int32_t* hyp_start, int H,
                                             const int32_t* seg_hyp_start, int S, float radius, int min_count, int steps, float* T_out /*[S,4,4]*/,
                                             float* hyp_out /*[H,4,4] or NULL*/, int32_t* counts_out /*[H] or NULL*/, int32_t* best_out /*[S] or NULL*/,
                                             void* ws, size_t ws_bytes, void* stream) {
  return local_global_registration("lcr_local_global_registration", src, ref, score, n, hyp_start, H, seg_hyp_start, S, radius, min_count, steps, 0,
                                   T_out, hyp_out, counts_out, best_out, ws, ws_bytes, stream);
}
extern "C" int lcr_local_global_registration_ex(const float* src, const float* ref, const float* score, int64_t n, const int32_t* hyp_start, int H,
                                                const int32_t* seg_hyp_start, int S, float radius, int min_count, int steps, int correspondence_limit,
                                                float* T_out, float* hyp_out, int32_t* counts_out, int32_t* best_out, void* ws, size_t ws_bytes,
                                                void* stream) {
  return local_global_registration("lcr_local_global_registration_ex", src, ref, score, n, hyp_start, H, seg_hyp_start, S, radius, min_count, steps,
                                   correspondence_limit, T_out, hyp_out, counts_out, best_out, ws, ws_bytes, stream);
}
