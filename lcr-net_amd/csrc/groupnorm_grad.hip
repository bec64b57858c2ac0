// groupnorm_grad.hip — the reverse of lcr_groupnorm_apply (groupnorm.hip), including the path through the statistics.
//
// With z = GN(x) [+ residual], y = act(z), dz = dy * (y > 0 ? 1 : slope) (act) or dy, x^ = (x - mean) * rstd and g = dz * gamma:
//     dbeta[c] = sum_n dz,   dgamma[c] = sum_n dz x^,   dx = rstd * (g - mean_sg(g) - x^ * mean_sg(g x^)),
// the means over the elements of one (segment, group).  mean and rstd come from the forward's own fp64 table through gn_mean_rstd, the
// function k_gn_apply finalises them with.
//
// Two passes, no floating-point atomics:
//   1. reduce — a segment is cut into pieces of GG_ROWS rows counted from ITS first row; a workgroup owns one piece and writes, per channel,
//      (sum dz, sum dz x^) of its rows (fp32, one fixed order).  One workgroup per segment then adds the segment's pieces in ascending order
//      in fp64, per channel, and from those the two group means (sum_c gamma_c * ...) and the finalised (mean, rstd) row of the table; a
//      last small kernel adds the segments in order into dgamma / dbeta.
//   2. apply — elementwise from the table.
// The pieces of a segment depend on its own length alone: dx of a segment has the same bytes alone and inside a stack.
#include <algorithm>

#include "common.h"

namespace lcr {

constexpr int GG_ROWS = 128;       // rows per piece
constexpr int GG_MAX_C = 2048;     // channels (the per-segment fold keeps 2 doubles per channel in LDS)

struct GgRow {                     // finalised per (segment, group)
  float mean_hi, mean_lo, rstd, pad;
  float m1, m2;                    // mean(g), mean(g x^)
  float pad2[2];
};

__device__ __forceinline__ float gg_xhat(float x, float mean_hi, float mean_lo, float rstd) { return fmaf(x - mean_hi, rstd, -(mean_lo * rstd)); }
__device__ __forceinline__ float gg_dz(float dy, float y, int act, float slope) { return act ? (y > 0.f ? dy : dy * slope) : dy; }

// piece -> (segment, first row, end row); false beyond the last piece
__device__ __forceinline__ bool gg_piece(const int64_t* __restrict__ seg_len, int S, int64_t N, int64_t piece, int* seg, int64_t* r0, int64_t* r1) {
  int64_t start = 0, first = 0;
  for (int s = 0; s < S; ++s) {
    int64_t len = seg_len[s];
    if (s == S - 1) len = N - start;                 // the last segment absorbs rows beyond the sum, as in the forward
    len = max(int64_t(0), min(len, N - start));
    const int64_t np = (len + GG_ROWS - 1) / GG_ROWS;
    if (piece < first + np) {
      *seg = s;
      *r0 = start + (piece - first) * GG_ROWS;
      *r1 = min(start + len, *r0 + GG_ROWS);
      return true;
    }
    first += np;
    start += len;
  }
  return false;
}

__global__ __launch_bounds__(256) void k_gg_reduce(const float* __restrict__ x, const double* __restrict__ stats, const float* __restrict__ y,
                                                   const float* __restrict__ dy, int64_t N, int C, int groups, const int64_t* __restrict__ seg_len, int S,
                                                   float eps, float slope, int act, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  float* s_mh = s_mem;                   // [groups] mean_hi, mean_lo, rstd
  float* s_ml = s_mem + groups;
  float* s_rs = s_mem + 2 * groups;
  float* s_acc = s_mem + 3 * groups;     // [RS][Cl][2]
  int seg;
  int64_t r0, r1;
  if (!gg_piece(seg_len, S, N, blockIdx.x, &seg, &r0, &r1)) return;      // block-uniform
  const int gs = C / groups;
  int64_t slen = seg_len[seg];
  {
    int64_t start = 0;
    for (int s = 0; s < seg; ++s) start += seg_len[s];
    if (seg == S - 1) slen = N - start;
  }
  const double cnt = static_cast<double>(slen) * gs;
  for (int g = threadIdx.x; g < groups; g += blockDim.x) gn_mean_rstd(stats, S, groups, seg, g, cnt, eps, &s_mh[g], &s_ml[g], &s_rs[g]);
  __syncthreads();
  const int Cl = C < 256 ? C : 256;      // channels per slab
  const int RS = 256 / Cl;               // rows side by side
  const int rsub = threadIdx.x / Cl, cl = threadIdx.x - rsub * Cl;
  for (int c0 = 0; c0 < C; c0 += Cl) {
    const int c = c0 + cl;
    const bool live = rsub < RS && c < C;
    float sb = 0.f, sg = 0.f;
    if (live) {
      const int g = c / gs;
      const float mh = s_mh[g], ml = s_ml[g], rs = s_rs[g];
      for (int64_t n = r0 + rsub; n < r1; n += RS) {
        const int64_t o = n * C + c;
        const float dz = gg_dz(dy[o], y ? y[o] : 1.f, act, slope);
        sb += dz;
        sg = fmaf(dz, gg_xhat(x[o], mh, ml, rs), sg);
      }
      s_acc[(rsub * Cl + cl) * 2] = sb;
      s_acc[(rsub * Cl + cl) * 2 + 1] = sg;
    }
    __syncthreads();
    if (live && rsub == 0) {
      for (int r = 1; r < RS; ++r) {       // row lanes added in order
        sb += s_acc[(r * Cl + cl) * 2];
        sg += s_acc[(r * Cl + cl) * 2 + 1];
      }
      part[(static_cast<int64_t>(blockIdx.x) * C + c) * 2] = sb;
      part[(static_cast<int64_t>(blockIdx.x) * C + c) * 2 + 1] = sg;
    }
    __syncthreads();
  }
}

// one workgroup per segment: pieces -> per-channel fp64 sums (segsum), group means and the finalised table row
__global__ __launch_bounds__(256) void k_gg_fold_seg(const float* __restrict__ part, const double* __restrict__ stats, const float* __restrict__ gamma,
                                                     int64_t N, int C, int groups, const int64_t* __restrict__ seg_len, int S, float eps,
                                                     double* __restrict__ segsum, GgRow* __restrict__ table) {
  extern __shared__ __attribute__((aligned(16))) double s_ch[];       // [C][2]: gamma * sum dz, gamma * sum dz x^
  const int seg = blockIdx.x;
  int64_t start = 0, first = 0;
  for (int s = 0; s < seg; ++s) {
    const int64_t len = max(int64_t(0), min(seg_len[s], N - start));
    first += (len + GG_ROWS - 1) / GG_ROWS;
    start += len;
  }
  int64_t slen = seg == S - 1 ? N - start : seg_len[seg];
  slen = max(int64_t(0), min(slen, N - start));
  const int64_t np = (slen + GG_ROWS - 1) / GG_ROWS;
  const int gs = C / groups;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    double sb = 0.0, sg = 0.0;
    for (int64_t p = 0; p < np; ++p) {
      sb += static_cast<double>(part[((first + p) * C + c) * 2]);
      sg += static_cast<double>(part[((first + p) * C + c) * 2 + 1]);
    }
    segsum[(static_cast<int64_t>(seg) * C + c) * 2] = sb;
    segsum[(static_cast<int64_t>(seg) * C + c) * 2 + 1] = sg;
    const double gm = static_cast<double>(gamma[c]);
    s_ch[2 * c] = gm * sb;
    s_ch[2 * c + 1] = gm * sg;
  }
  __syncthreads();
  const double cnt = static_cast<double>(slen) * gs;
  for (int g = threadIdx.x; g < groups; g += blockDim.x) {
    double a1 = 0.0, a2 = 0.0;
    for (int j = 0; j < gs; ++j) {
      a1 += s_ch[2 * (g * gs + j)];
      a2 += s_ch[2 * (g * gs + j) + 1];
    }
    GgRow r;
    r.pad = 0.f;
    r.pad2[0] = r.pad2[1] = 0.f;
    r.mean_hi = r.mean_lo = 0.f;
    r.rstd = 0.f;
    r.m1 = r.m2 = 0.f;
    if (slen > 0) {
      gn_mean_rstd(stats, S, groups, seg, g, cnt, eps, &r.mean_hi, &r.mean_lo, &r.rstd);
      r.m1 = static_cast<float>(a1 / cnt);
      r.m2 = static_cast<float>(a2 / cnt);
    }
    table[static_cast<int64_t>(seg) * groups + g] = r;
  }
}

__global__ __launch_bounds__(256) void k_gg_fold_chan(const double* __restrict__ segsum, int C, int S, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double sb = 0.0, sg = 0.0;
  for (int s = 0; s < S; ++s) {
    sb += segsum[(static_cast<int64_t>(s) * C + c) * 2];
    sg += segsum[(static_cast<int64_t>(s) * C + c) * 2 + 1];
  }
  if (dbeta) dbeta[c] = static_cast<float>(sb);
  if (dgamma) dgamma[c] = static_cast<float>(sg);
}

__global__ __launch_bounds__(256) void k_gg_apply(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ y,
                                                  const float* __restrict__ dy, int64_t N, int C, int groups, const int64_t* __restrict__ seg_len, int S,
                                                  float slope, int act, const GgRow* __restrict__ table, float* __restrict__ dx, float* __restrict__ dz_out) {
  __shared__ int64_t s_start[GN_MAX_SEG + 1];
  if (threadIdx.x == 0) {
    int64_t o = 0;
    for (int i = 0; i < S; ++i) {
      s_start[i] = o;
      o += seg_len[i];
    }
    s_start[S] = o;
  }
  __syncthreads();
  const int gs = C / groups, c4n = C >> 2;
  const int64_t total = N * c4n;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; t < total; t += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t n = t / c4n;
    const int c0 = static_cast<int>(t - n * c4n) * 4;
    int lo = 0, hi = S - 1;                            // the segment of row n (the last one absorbs rows beyond the sum)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_start[mid] <= n) lo = mid;
      else hi = mid - 1;
    }
    // zero-length segments share their start with the next one: take the last segment that starts at or before n and holds it
    const int64_t o = n * C + c0;
    const float4 xv = *reinterpret_cast<const float4*>(x + o), dv = *reinterpret_cast<const float4*>(dy + o);
    float4 yv = make_float4(1.f, 1.f, 1.f, 1.f);
    if (y) yv = *reinterpret_cast<const float4*>(y + o);
    const float4 gv = *reinterpret_cast<const float4*>(gamma + c0);
    const float xin[4] = {xv.x, xv.y, xv.z, xv.w}, din[4] = {dv.x, dv.y, dv.z, dv.w}, yin[4] = {yv.x, yv.y, yv.z, yv.w}, g4[4] = {gv.x, gv.y, gv.z, gv.w};
    float out[4], dzv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const GgRow r = table[static_cast<int64_t>(lo) * groups + (c0 + u) / gs];
      const float dz = gg_dz(din[u], yin[u], act, slope);
      const float xh = gg_xhat(xin[u], r.mean_hi, r.mean_lo, r.rstd);
      const float g = dz * g4[u];
      out[u] = r.rstd * ((g - r.m1) - xh * r.m2);
      dzv[u] = dz;
    }
    *reinterpret_cast<float4*>(dx + o) = make_float4(out[0], out[1], out[2], out[3]);
    if (dz_out) *reinterpret_cast<float4*>(dz_out + o) = make_float4(dzv[0], dzv[1], dzv[2], dzv[3]);
  }
}

struct GgLayout {
  float*  part;
  double* segsum;
  GgRow*  table;
  size_t  bytes;
  int64_t pieces;
};
static GgLayout gg_layout(void* ws, int64_t N, int C, int groups, int S) {
  Carver c(ws, ~size_t(0));
  GgLayout L;
  L.pieces = (N + GG_ROWS - 1) / GG_ROWS + S;           // sum over segments of ceil(len / GG_ROWS) is at most this
  L.part = c.take<float>(static_cast<size_t>(L.pieces) * C * 2);
  L.segsum = c.take<double>(static_cast<size_t>(S) * C * 2);
  L.table = c.take<GgRow>(static_cast<size_t>(S) * groups);
  L.bytes = c.off;
  return L;
}
static bool gg_domain(int64_t N, int C, int groups, int S) {
  return N >= 0 && C >= 4 && C % 4 == 0 && C <= GG_MAX_C && groups >= 1 && C % groups == 0 && S >= 1 && S <= GN_MAX_SEG && N * (C / 4) < (int64_t(1) << 40);
}

}  // namespace lcr

using namespace lcr;

extern "C" int lcr_groupnorm_apply_grad_ws_bytes(int64_t N, int C, int groups, int S, size_t* bytes) {
  if (!bytes || !gg_domain(N, C, groups, S))
    return refuse(LCR_EARG, "lcr_groupnorm_apply_grad_ws_bytes: C must be a multiple of 4 and of groups, at most %d, and 1 <= S <= %d", GG_MAX_C, GN_MAX_SEG);
  *bytes = gg_layout(nullptr, N, C, groups, S).bytes;
  return LCR_OK;
}

extern "C" int lcr_groupnorm_apply_grad(const float* x, const double* stats, const float* gamma, const float* y, const float* dy, int64_t N, int C,
                                        int groups, const int64_t* seg_len, int S, float eps, float slope, int act, float* dx, float* dgamma,
                                        float* dbeta, float* dz, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !stats || !gamma || !dy || !dx || !seg_len || !ws || (act && !y)) return refuse(LCR_EARG, "lcr_groupnorm_apply_grad: null argument (y is needed with act)");
  if (!gg_domain(N, C, groups, S))
    return refuse(LCR_EARG, "lcr_groupnorm_apply_grad: C must be a multiple of 4 and of groups, at most %d, and 1 <= S <= %d", GG_MAX_C, GN_MAX_SEG);
  const GgLayout L = gg_layout(ws, N, C, groups, S);
  if (ws_bytes < L.bytes) return refuse_ws(LCR_EARG, "lcr_groupnorm_apply_grad", ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  const int Cl = C < 256 ? C : 256;
  const size_t red_lds = (3 * static_cast<size_t>(groups) + static_cast<size_t>(256 / Cl) * Cl * 2) * sizeof(float);
  if (N > 0)
    hipLaunchKernelGGL(k_gg_reduce, dim3(static_cast<unsigned>(L.pieces)), dim3(256), red_lds, st, x, stats, act ? y : nullptr, dy, N, C, groups, seg_len, S, eps,
                       slope, act, L.part);
  hipLaunchKernelGGL(k_gg_fold_seg, dim3(S), dim3(256), static_cast<size_t>(C) * 2 * sizeof(double), st, L.part, stats, gamma, N, C, groups, seg_len, S, eps,
                     L.segsum, L.table);
  if (dgamma || dbeta) hipLaunchKernelGGL(k_gg_fold_chan, dim3((C + 255) / 256), dim3(256), 0, st, L.segsum, C, S, dgamma, dbeta);
  if (N > 0)
    hipLaunchKernelGGL(k_gg_apply, dim3(blocks_for(N * (C / 4), 1024, 2048)), dim3(256), 0, st, x, gamma, act ? y : nullptr, dy, N, C, groups, seg_len, S, slope, act,
                       L.table, dx, dz);
  return check_launch("lcr_groupnorm_apply_grad");
}
