// losses.hip — the registration loss terms of the reference's OverallLoss_new (experiments/lcrnet/loss_reg.py) for P pairs in one call:
// the gap loss of `gap` / `node_gap` with its gradient to the scores, and the one-sided nearest distance behind
// SingleSideChamferLoss_Brute / VoteLoss_new with its gradient to the queries.  The semantics are stated in include/lcr_hip.h next to
// lcr_gap_loss and lcr_min_dist.
//
//   k_gap_labels_pts   one thread per inner (slice, i, j): q' = R q + t, d2 by differences, the 2-bit label (bit 0 positive, bit 1 negative);
//   k_gap_labels_ov    the plane is preset to "negative"; one thread per listed (i, j, overlap) entry rewrites its own byte;
//   k_gap_rows         one wavefront per (slice, row): positives counted and averaged, the dustbin label decided, the hinge summed;
//   k_gap_cols         one thread per (slice, column), rows walked in order (coalesced across the wavefront): the transpose;
//   k_gap_finish       one workgroup per pair: the kept lines' log terms summed in a fixed order, the three loss values, the status word;
//   k_gap_grad         one thread per score: its row part and its column part from the saved line statistics, written once;
//   k_min_dist         16 queries per workgroup, the segment's data tiled through LDS, 16 lanes per query, (d2, index) minimum;
//   k_md_mean          one workgroup per segment: mean distance of the valid queries in a fixed order;
//   k_md_grad          one thread per query.
// Sums run in fp64 in an order that depends on the line or segment alone, so a pair gives the same bytes alone or in any batch.  No atomics.
#include <cmath>

#include "common.h"

namespace lcr {

constexpr int MD_TILE = 1024;   // data points per LDS tile (12 KB)
constexpr int MD_Q = 16;        // queries per workgroup, 16 lanes each

struct GapGeom {
  const int64_t *soff, *roff, *coff;   // [B+1] each: first score, first row, first column of every slice
  int64_t elems, rows, cols;           // totals: the extents of S / labels, of the row tables, of the column tables
  int     n_max, m_max;
};

// slice b's extents; false (and nothing may be touched) when the tables do not fit the declared totals
__device__ __forceinline__ bool gap_slice(const GapGeom& g, int b, int64_t* s0, int64_t* r0, int64_t* c0, int* n, int* m) {
  *s0 = g.soff[b];
  *r0 = g.roff[b];
  *c0 = g.coff[b];
  const int64_t nn = g.roff[b + 1] - *r0, mm = g.coff[b + 1] - *c0;
  if (*s0 < 0 || *r0 < 0 || *c0 < 0 || nn < 0 || mm < 0 || nn > g.n_max || mm > g.m_max) return false;
  if (*r0 + nn > g.rows || *c0 + mm > g.cols || *s0 + (nn + 1) * (mm + 1) > g.elems) return false;
  *n = static_cast<int>(nn);
  *m = static_cast<int>(mm);
  return true;
}

__device__ __forceinline__ int gap_pair_of(const int32_t* __restrict__ seg, int P, int b) {
  int lo = 0, hi = P - 1;                       // the last p with seg[p] <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid] <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_gap_labels_pts(GapGeom g, const int32_t* __restrict__ seg, int P, const float* __restrict__ pp,
                                                        const float* __restrict__ qp, const uint8_t* __restrict__ pm,
                                                        const uint8_t* __restrict__ qm, const float* __restrict__ T, float r2, float r2neg,
                                                        uint8_t* __restrict__ labels) {
  const int b = blockIdx.y;
  int64_t s0, r0, c0;
  int n, m;
  if (!gap_slice(g, b, &s0, &r0, &c0, &n, &m)) return;
  const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (e >= static_cast<int64_t>(n) * m) return;
  const int i = static_cast<int>(e / m), j = static_cast<int>(e % m);
  const float* t = T + 16 * gap_pair_of(seg, P, b);
  const float x = qp[3 * (c0 + j)], y = qp[3 * (c0 + j) + 1], z = qp[3 * (c0 + j) + 2];
  const float qx = fadd(fadd(fadd(fmul(t[0], x), fmul(t[1], y)), fmul(t[2], z)), t[3]);
  const float qy = fadd(fadd(fadd(fmul(t[4], x), fmul(t[5], y)), fmul(t[6], z)), t[7]);
  const float qz = fadd(fadd(fadd(fmul(t[8], x), fmul(t[9], y)), fmul(t[10], z)), t[11]);
  const float dx = fsub(pp[3 * (r0 + i)], qx), dy = fsub(pp[3 * (r0 + i) + 1], qy), dz = fsub(pp[3 * (r0 + i) + 2], qz);
  const float d2 = fadd(fadd(fmul(dx, dx), fmul(dy, dy)), fmul(dz, dz));
  const bool pos = d2 < r2 && pm[r0 + i] && qm[c0 + j];
  labels[s0 + static_cast<int64_t>(i) * (m + 1) + j] = static_cast<uint8_t>((pos ? 1 : 0) | (d2 > r2neg ? 2 : 0));     // negatives are NOT masked
}

// entry c of pair p: (i, j) of the pair's first slice, overlap ov.  Entries of one pair are distinct node pairs (the caller's list).
__global__ __launch_bounds__(256) void k_gap_labels_ov(GapGeom g, const int32_t* __restrict__ seg, const int64_t* __restrict__ corr,
                                                       const float* __restrict__ ov, const int32_t* __restrict__ cstart, int64_t C,
                                                       const uint8_t* __restrict__ pm, const uint8_t* __restrict__ qm, float thr,
                                                       uint8_t* __restrict__ labels, int32_t* __restrict__ flag, int B) {
  const int p = blockIdx.y, b = seg[p];
  int64_t s0, r0, c0;
  int n, m;
  if (b < 0 || b >= B || !gap_slice(g, b, &s0, &r0, &c0, &n, &m)) return;
  const int64_t lo = cstart[p], hi = cstart[p + 1];
  if (lo < 0 || hi > C || lo > hi) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *flag = 1;
    return;
  }
  const int64_t c = lo + blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (c >= hi) return;
  const int64_t i = corr[2 * c], j = corr[2 * c + 1];
  if (i < 0 || i >= n || j < 0 || j >= m) {
    *flag = 1;                                                 // the same value from every writer
    return;
  }
  const float o = ov[c];
  const bool pos = o > thr && pm[r0 + i] && qm[c0 + j];
  labels[s0 + i * (m + 1) + j] = static_cast<uint8_t>((pos ? 1 : 0) | (o == 0.f ? 2 : 0));
}

__device__ __forceinline__ bool gap_dropped(double pos) { return static_cast<float>(pos) == 1e12f; }

__global__ __launch_bounds__(256) void k_gap_rows(GapGeom g, const float* __restrict__ S, double gamma, uint8_t* __restrict__ labels,
                                                  double* __restrict__ lpos, double* __restrict__ lhs, int32_t* __restrict__ lcnt,
                                                  int32_t* __restrict__ lact, double* __restrict__ llog) {
  const int b = blockIdx.y;
  int64_t s0, r0, c0;
  int n, m;
  if (!gap_slice(g, b, &s0, &r0, &c0, &n, &m)) return;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = lane_id();
  if (i > n) return;                                            // wave-uniform
  const int64_t base = s0 + static_cast<int64_t>(i) * (m + 1);
  if (i == n) {
    if (lane == 0) labels[base + m] = 0;                        // the corner belongs to neither direction
    return;
  }
  int cnt = 0;
  double sum = 0.0;
  for (int j = lane; j < m; j += WAVE)
    if (labels[base + j] & 1) {
      ++cnt;
      sum -= static_cast<double>(S[base + j]);
    }
  cnt = wave_sum(cnt);
  sum = wave_sum(sum);
  const uint8_t dust = cnt == 0 ? 1 : 2;                        // the dustbin is the positive of a row without one
  if (cnt == 0) {
    cnt = 1;
    sum = -static_cast<double>(S[base + m]);
  }
  const double pos = sum / cnt;
  int act = 0;
  double hs = 0.0;
  for (int j = lane; j <= m; j += WAVE) {
    const uint8_t lab = j < m ? labels[base + j] : dust;
    if (lab & 2) {
      const double a = pos + static_cast<double>(S[base + j]) + gamma;
      if (a >= 0.0) {
        hs += a;
        ++act;
      }
    }
  }
  act = wave_sum(act);
  hs = wave_sum(hs);
  if (lane == 0) {
    const bool drop = gap_dropped(pos);
    const int64_t l = r0 + i;
    labels[base + m] = dust;
    lpos[l] = pos;
    lcnt[l] = cnt;
    lhs[l] = drop ? 0.0 : hs;
    lact[l] = drop ? -1 : act;
    llog[l] = drop ? 0.0 : log(hs + 1.0);
  }
}

__global__ __launch_bounds__(64) void k_gap_cols(GapGeom g, const float* __restrict__ S, double gamma, uint8_t* __restrict__ labels,
                                                 double* __restrict__ lpos, double* __restrict__ lhs, int32_t* __restrict__ lcnt,
                                                 int32_t* __restrict__ lact, double* __restrict__ llog) {
  const int b = blockIdx.y;
  int64_t s0, r0, c0;
  int n, m;
  if (!gap_slice(g, b, &s0, &r0, &c0, &n, &m)) return;
  const int j = blockIdx.x * WAVE + threadIdx.x;
  if (j >= m) return;
  const int64_t w = m + 1, base = s0 + j;
  int cnt = 0;
  double sum = 0.0;
  for (int i = 0; i < n; ++i)
    if (labels[base + i * w] & 1) {
      ++cnt;
      sum -= static_cast<double>(S[base + i * w]);
    }
  const uint8_t dust = cnt == 0 ? 1 : 2;
  if (cnt == 0) {
    cnt = 1;
    sum = -static_cast<double>(S[base + n * w]);
  }
  const double pos = sum / cnt;
  int act = 0;
  double hs = 0.0;
  for (int i = 0; i <= n; ++i) {
    const uint8_t lab = i < n ? labels[base + i * w] : dust;
    if (lab & 2) {
      const double a = pos + static_cast<double>(S[base + i * w]) + gamma;
      if (a >= 0.0) {
        hs += a;
        ++act;
      }
    }
  }
  const bool drop = gap_dropped(pos);
  const int64_t l = g.rows + c0 + j;
  labels[base + n * w] = dust;
  lpos[l] = pos;
  lcnt[l] = cnt;
  lhs[l] = drop ? 0.0 : hs;
  lact[l] = drop ? -1 : act;
  llog[l] = drop ? 0.0 : log(hs + 1.0);
}

// fixed-order sum of 256 partials (double, int) in LDS; every thread returns the totals
__device__ __forceinline__ void block_sum_256(double* sd, int* si, double* v, int* k) {
  const int t = threadIdx.x;
  sd[t] = *v;
  si[t] = *k;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) {
      sd[t] += sd[t + s];
      si[t] += si[t + s];
    }
    __syncthreads();
  }
  *v = sd[0];
  *k = si[0];
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_gap_finish(GapGeom g, const int32_t* __restrict__ seg, int B, int P, const int32_t* __restrict__ lact,
                                                    const double* __restrict__ llog, const int32_t* __restrict__ flag,
                                                    float* __restrict__ terms, int32_t* __restrict__ kept, uint32_t* __restrict__ status) {
  __shared__ double sd[256];
  __shared__ int si[256];
  const int p = blockIdx.x, t = threadIdx.x;
  const int b0 = seg[p], b1 = seg[p + 1];
  // the pair's lines are those of its slices, back to back in the row and column tables; a segment or slice outside the declared
  // totals contributes nothing and raises the status
  int64_t r0 = 0, r1 = 0, c0 = 0, c1 = 0;
  bool pair_ok = b0 >= 0 && b1 <= B && b0 <= b1;
  if (pair_ok && b0 < b1) {
    int64_t s, ra, ca, rb, cb;
    int n, m;
    pair_ok = gap_slice(g, b0, &s, &ra, &ca, &n, &m) && gap_slice(g, b1 - 1, &s, &rb, &cb, &n, &m) && rb + n >= ra && cb + m >= ca;
    if (pair_ok) {
      r0 = ra;
      c0 = ca;
      r1 = rb + n;
      c1 = cb + m;
    }
  }
  double tv[2];
  for (int dir = 0; dir < 2; ++dir) {
    const int64_t lo = dir ? g.rows + c0 : r0, hi = dir ? g.rows + c1 : r1;
    double v = 0.0;
    int k = 0;
    for (int64_t l = lo + t; l < hi; l += 256)
      if (lact[l] >= 0) {
        v += llog[l];
        ++k;
      }
    block_sum_256(sd, si, &v, &k);
    tv[dir] = v / k;                                            // 0 / 0: NaN when no line is kept, like the reference's mean of nothing
    if (t == 0) {
      terms[3 * p + dir] = static_cast<float>(tv[dir]);
      kept[2 * p + dir] = k;
    }
  }
  if (t == 0) terms[3 * p + 2] = static_cast<float>((tv[0] + tv[1]) / 2.0);
  if (p == 0) {                                                 // the status word: every slice and segment against the declared totals
    int64_t s, r, c;
    int n, m, any = !pair_ok;
    for (int b = t; b < B; b += 256) any |= !gap_slice(g, b, &s, &r, &c, &n, &m);
    for (int q = t; q < P; q += 256) any |= !(seg[q] >= 0 && seg[q] <= seg[q + 1] && seg[q + 1] <= B);
    double none = 0.0;
    block_sum_256(sd, si, &none, &any);
    if (t == 0) *status = (any ? LCR_STATUS_LEN_MISMATCH : 0u) | (*flag ? LCR_STATUS_INDEX_RANGE : 0u);
  }
}

__global__ __launch_bounds__(256) void k_gap_grad(GapGeom g, const int32_t* __restrict__ seg, int P, const float* __restrict__ S,
                                                  const uint8_t* __restrict__ labels, const double* __restrict__ lpos,
                                                  const double* __restrict__ lhs, const int32_t* __restrict__ lcnt,
                                                  const int32_t* __restrict__ lact, const int32_t* __restrict__ kept,
                                                  const float* __restrict__ gup, double gamma, float* __restrict__ dS) {
  const int b = blockIdx.y;
  int64_t s0, r0, c0;
  int n, m;
  if (!gap_slice(g, b, &s0, &r0, &c0, &n, &m)) return;
  const int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (e >= static_cast<int64_t>(n + 1) * (m + 1)) return;
  const int i = static_cast<int>(e / (m + 1)), j = static_cast<int>(e % (m + 1));
  const int p = gap_pair_of(seg, P, b);
  const uint8_t lab = labels[s0 + e];
  const double s = static_cast<double>(S[s0 + e]);
  double v = 0.0;
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    if (dir == 0 ? i >= n : j >= m) continue;                   // the dustbin row has no row term, the dustbin column no column term
    const int64_t l = dir == 0 ? r0 + i : g.rows + c0 + j;
    const int act = lact[l];
    if (act < 0) continue;                                      // a dropped line
    const double w = static_cast<double>(gup[2 * p + dir]) / (static_cast<double>(kept[2 * p + dir]) * (lhs[l] + 1.0));
    if ((lab & 2) && lpos[l] + s + gamma >= 0.0) v += w;
    if (lab & 1) v -= w * act / lcnt[l];
  }
  dS[s0 + e] = static_cast<float>(v);
}

// ---- one-sided nearest distance -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool md_seg(const int32_t* __restrict__ off, int p, int64_t total, int64_t* lo, int64_t* hi) {
  *lo = off[p];
  *hi = off[p + 1];
  return *lo >= 0 && *lo <= *hi && *hi <= total;
}

__global__ __launch_bounds__(256) void k_min_dist(const float* __restrict__ A, const int32_t* __restrict__ aoff, int64_t na,
                                                  const float* __restrict__ D, const int32_t* __restrict__ doff, int64_t nd,
                                                  float* __restrict__ dist, int32_t* __restrict__ arg) {
  __shared__ float sx[MD_TILE], sy[MD_TILE], sz[MD_TILE];
  const int p = blockIdx.y, t = threadIdx.x;
  int64_t a0, a1, d0, d1;
  if (!md_seg(aoff, p, na, &a0, &a1) || !md_seg(doff, p, nd, &d0, &d1)) return;      // block-uniform
  if (a0 + static_cast<int64_t>(blockIdx.x) * MD_Q >= a1) return;
  const int64_t q = a0 + static_cast<int64_t>(blockIdx.x) * MD_Q + (t >> 4);
  const int sub = t & 15;
  const bool have = q < a1;
  const float ax = have ? A[3 * q] : 0.f, ay = have ? A[3 * q + 1] : 0.f, az = have ? A[3 * q + 2] : 0.f;
  float best = INFINITY;
  int64_t bi = -1;
  for (int64_t t0 = d0; t0 < d1; t0 += MD_TILE) {
    const int tn = static_cast<int>(d1 - t0 < MD_TILE ? d1 - t0 : MD_TILE);
    __syncthreads();
    for (int f = t; f < 3 * tn; f += 256) {
      const float v = D[3 * t0 + f];
      const int k = f / 3, c = f - 3 * k;
      (c == 0 ? sx : c == 1 ? sy : sz)[k] = v;
    }
    __syncthreads();
    for (int k = sub; k < tn; k += 16) {
      const float dx = fsub(ax, sx[k]), dy = fsub(ay, sy[k]), dz = fsub(az, sz[k]);
      const float d2 = fadd(fadd(fmul(dx, dx), fmul(dy, dy)), fmul(dz, dz));
      if (d2 < best) {                                           // ascending k: the lower index keeps a tie
        best = d2;
        bi = t0 + k;
      }
    }
  }
#pragma unroll
  for (int s = 8; s >= 1; s >>= 1) {
    const float od = __shfl_xor(best, s);
    const int64_t oi = __shfl_xor(bi, s);
    if (oi >= 0 && (bi < 0 || od < best || (od == best && oi < bi))) {
      best = od;
      bi = oi;
    }
  }
  if (have && sub == 0) {
    dist[q] = sqrtf(fmaxf(best, 1e-12f));
    arg[q] = bi < 0 ? -1 : static_cast<int32_t>(bi - d0);
  }
}

__global__ __launch_bounds__(256) void k_md_mean(const float* __restrict__ dist, const uint8_t* __restrict__ valid,
                                                 const int32_t* __restrict__ aoff, int64_t na, float* __restrict__ mean,
                                                 int32_t* __restrict__ count) {
  __shared__ double sd[256];
  __shared__ int si[256];
  const int p = blockIdx.x, t = threadIdx.x;
  int64_t a0, a1;
  if (!md_seg(aoff, p, na, &a0, &a1)) a0 = a1 = 0;
  double v = 0.0;
  int k = 0;
  for (int64_t q = a0 + t; q < a1; q += 256)
    if (!valid || valid[q]) {
      v += static_cast<double>(dist[q]);
      ++k;
    }
  block_sum_256(sd, si, &v, &k);
  if (t == 0) {
    mean[p] = static_cast<float>(v / k);                         // NaN without a valid query, like the reference's mean of nothing
    count[p] = k;
  }
}

__global__ __launch_bounds__(256) void k_md_grad(const float* __restrict__ A, const int32_t* __restrict__ aoff, int64_t na,
                                                 const float* __restrict__ D, const int32_t* __restrict__ doff, int64_t nd,
                                                 const uint8_t* __restrict__ valid, const int32_t* __restrict__ arg,
                                                 const float* __restrict__ dist, const int32_t* __restrict__ count,
                                                 const float* __restrict__ gup, float* __restrict__ dA) {
  const int p = blockIdx.y;
  int64_t a0, a1, d0, d1;
  if (!md_seg(aoff, p, na, &a0, &a1) || !md_seg(doff, p, nd, &d0, &d1)) return;
  const int64_t q = a0 + blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (q >= a1) return;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  const int32_t a = arg[q];
  if ((!valid || valid[q]) && a >= 0 && d0 + a < d1) {
    const int64_t d = d0 + a;
    const float dx = fsub(A[3 * q], D[3 * d]), dy = fsub(A[3 * q + 1], D[3 * d + 1]), dz = fsub(A[3 * q + 2], D[3 * d + 2]);
    const float d2 = fadd(fadd(fmul(dx, dx), fmul(dy, dy)), fmul(dz, dz));
    if (d2 >= 1e-12f) {                                          // below the clamp the distance is a constant
      const double w = static_cast<double>(gup[p]) / static_cast<double>(dist[q]) / static_cast<double>(count[p]);
      gx = static_cast<float>(w * dx);
      gy = static_cast<float>(w * dy);
      gz = static_cast<float>(w * dz);
    }
  }
  dA[3 * q] = gx;
  dA[3 * q + 1] = gy;
  dA[3 * q + 2] = gz;
}

}  // namespace lcr

using namespace lcr;

struct GapLayout {
  double*  llog;    // [rows + cols]
  int32_t* flag;    // [1]
  size_t   bytes;
};

static GapLayout gap_layout(void* ws, int64_t rows, int64_t cols) {
  GapLayout L;
  Carver c(ws, ~size_t(0));
  L.llog = c.take<double>(static_cast<size_t>(rows + cols));
  L.flag = c.take<int32_t>(1);
  L.bytes = c.off;
  return L;
}

static int gap_domain(const char* entry, int64_t B, int P, int n_max, int m_max, int64_t elems, int64_t rows, int64_t cols) {
  if (B < 1 || B > 65535 || P < 1 || P > 65535 || P > B || n_max < 0 || m_max < 0 || n_max > 32767 || m_max > 32767 || elems < B ||
      rows < 0 || cols < 0 || rows > B * static_cast<int64_t>(n_max) || cols > B * static_cast<int64_t>(m_max) ||
      elems > B * static_cast<int64_t>(n_max + 1) * (m_max + 1))
    return refuse(LCR_EARG, "%s: outside the domain (1 <= P <= B <= 65535, 0 <= n_max, m_max <= 32767, totals within B slices of that size): B=%lld P=%d "
                  "n_max=%d m_max=%d elems=%lld rows=%lld cols=%lld", entry, static_cast<long long>(B), P, n_max, m_max,
                  static_cast<long long>(elems), static_cast<long long>(rows), static_cast<long long>(cols));
  return LCR_OK;
}

extern "C" int lcr_gap_loss_ws_bytes(int64_t rows, int64_t cols, size_t* bytes) {
  if (!bytes || rows < 0 || cols < 0) return refuse(LCR_EARG, "lcr_gap_loss_ws_bytes: null pointer or negative count");
  *bytes = gap_layout(nullptr, rows, cols).bytes;
  return LCR_OK;
}

extern "C" int lcr_gap_loss(const float* S, const int64_t* soff, const int64_t* roff, const int64_t* coff, const int32_t* seg_start, int64_t B,
                            int P, int n_max, int m_max, int64_t elems, int64_t rows, int64_t cols, int source, const float* p_pts,
                            const float* q_pts, const float* transforms, double positive_radius, const int64_t* corr, const float* overlaps,
                            const int32_t* corr_start, int64_t C, int64_t c_max, double positive_overlap, const uint8_t* pmask,
                            const uint8_t* qmask, double gamma, float* terms, int32_t* kept, uint8_t* labels, double* line_pos,
                            double* line_hinge, int32_t* line_count, int32_t* line_active, uint32_t* status, void* ws, size_t ws_bytes,
                            void* stream) {
  const int rc = gap_domain("lcr_gap_loss", B, P, n_max, m_max, elems, rows, cols);
  if (rc != LCR_OK) return rc;
  const bool lines = rows + cols > 0;
  if (!S || !soff || !roff || !coff || !seg_start || !terms || !kept || !labels || !status || !ws ||
      (lines && (!line_pos || !line_hinge || !line_count || !line_active)) || (rows > 0 && !pmask) || (cols > 0 && !qmask) ||
      !(gamma == gamma))
    return refuse(LCR_EARG, "lcr_gap_loss: null pointer or NaN gamma");
  const float r2 = static_cast<float>(positive_radius * positive_radius);
  const float r2neg = static_cast<float>((positive_radius * 2) * (positive_radius * 2));
  if (source == LCR_GAP_LABELS_POINTS) {
    if (!transforms || (rows > 0 && !p_pts) || (cols > 0 && !q_pts) || !(positive_radius >= 0) || !(r2neg < INFINITY))
      return refuse(LCR_EARG, "lcr_gap_loss: the point labels need points, transforms and a radius >= 0 with a finite fp32 square");
  } else if (source == LCR_GAP_LABELS_OVERLAPS) {
    if (C < 0 || c_max < 0 || c_max > C || !corr_start || (C > 0 && (!corr || !overlaps)) || !(positive_overlap >= 0))
      return refuse(LCR_EARG, "lcr_gap_loss: the overlap labels need the correspondence list, its offsets and positive_overlap >= 0");
  } else {
    return refuse(LCR_EARG, "lcr_gap_loss: unknown label source %d", source);
  }
  const GapLayout L = gap_layout(ws, rows, cols);
  if (L.bytes > ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_gap_loss", ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  const GapGeom g{soff, roff, coff, elems, rows, cols, n_max, m_max};
  const int Bi = static_cast<int>(B);
  if (hipMemsetAsync(L.flag, 0, sizeof(int32_t), st) != hipSuccess) return check_launch("lcr_gap_loss");
  if (source == LCR_GAP_LABELS_POINTS) {
    if (n_max > 0 && m_max > 0)
      hipLaunchKernelGGL(k_gap_labels_pts, dim3(div_up(static_cast<int64_t>(n_max) * m_max, 256), Bi), dim3(256), 0, st, g, seg_start, P, p_pts,
                         q_pts, pmask, qmask, transforms, r2, r2neg, labels);
  } else {
    if (hipMemsetAsync(labels, 2, static_cast<size_t>(elems), st) != hipSuccess) return check_launch("lcr_gap_loss");     // not listed: overlap 0
    if (c_max > 0)
      hipLaunchKernelGGL(k_gap_labels_ov, dim3(div_up(c_max, 256), P), dim3(256), 0, st, g, seg_start, corr, overlaps, corr_start, C, pmask,
                         qmask, static_cast<float>(positive_overlap), labels, L.flag, Bi);
  }
  hipLaunchKernelGGL(k_gap_rows, dim3(div_up(n_max + 1, 4), Bi), dim3(256), 0, st, g, S, gamma, labels, line_pos, line_hinge, line_count,
                     line_active, L.llog);
  if (m_max > 0)
    hipLaunchKernelGGL(k_gap_cols, dim3(div_up(m_max, WAVE), Bi), dim3(64), 0, st, g, S, gamma, labels, line_pos, line_hinge, line_count,
                       line_active, L.llog);
  hipLaunchKernelGGL(k_gap_finish, dim3(P), dim3(256), 0, st, g, seg_start, Bi, P, line_active, L.llog, L.flag, terms, kept, status);
  return check_launch("lcr_gap_loss");
}

extern "C" int lcr_gap_loss_grad(const float* S, const int64_t* soff, const int64_t* roff, const int64_t* coff, const int32_t* seg_start,
                                 int64_t B, int P, int n_max, int m_max, int64_t elems, int64_t rows, int64_t cols, double gamma,
                                 const float* upstream, const int32_t* kept, const uint8_t* labels, const double* line_pos,
                                 const double* line_hinge, const int32_t* line_count, const int32_t* line_active, float* dS, void* stream) {
  const int rc = gap_domain("lcr_gap_loss_grad", B, P, n_max, m_max, elems, rows, cols);
  if (rc != LCR_OK) return rc;
  if (!S || !soff || !roff || !coff || !seg_start || !upstream || !kept || !labels || !dS ||
      (rows + cols > 0 && (!line_pos || !line_hinge || !line_count || !line_active)))
    return refuse(LCR_EARG, "lcr_gap_loss_grad: null pointer");
  const GapGeom g{soff, roff, coff, elems, rows, cols, n_max, m_max};
  hipLaunchKernelGGL(k_gap_grad, dim3(div_up(static_cast<int64_t>(n_max + 1) * (m_max + 1), 256), static_cast<int>(B)), dim3(256), 0, ST(stream),
                     g, seg_start, P, S, labels, line_pos, line_hinge, line_count, line_active, kept, upstream, gamma, dS);
  return check_launch("lcr_gap_loss_grad");
}

static int md_domain(const char* entry, int P, int64_t na, int64_t nd, int64_t q_max) {
  if (P < 1 || P > 65535 || na < 0 || nd < 0 || na > INT32_MAX / 3 || nd > INT32_MAX / 3 || q_max < 0 || q_max > na)
    return refuse(LCR_EARG, "%s: outside the domain (1 <= P <= 65535, 0 <= q_max <= na, na and nd at most (2^31-1)/3): P=%d na=%lld nd=%lld q_max=%lld", entry,
                  P, static_cast<long long>(na), static_cast<long long>(nd), static_cast<long long>(q_max));
  return LCR_OK;
}

extern "C" int lcr_min_dist(const float* A, const int32_t* a_start, int64_t na, const float* D, const int32_t* d_start, int64_t nd,
                            const uint8_t* valid, int P, int64_t q_max, float* dist, int32_t* arg, float* mean, int32_t* count, void* stream) {
  const int rc = md_domain("lcr_min_dist", P, na, nd, q_max);
  if (rc != LCR_OK) return rc;
  if (!a_start || !d_start || !mean || !count || (na > 0 && (!A || !dist || !arg)) || (nd > 0 && !D)) return refuse(LCR_EARG, "lcr_min_dist: null pointer");
  hipStream_t st = ST(stream);
  if (q_max > 0)
    hipLaunchKernelGGL(k_min_dist, dim3(div_up(q_max, MD_Q), P), dim3(256), 0, st, A, a_start, na, D, d_start, nd, dist, arg);
  hipLaunchKernelGGL(k_md_mean, dim3(P), dim3(256), 0, st, dist, valid, a_start, na, mean, count);
  return check_launch("lcr_min_dist");
}

extern "C" int lcr_min_dist_grad(const float* A, const int32_t* a_start, int64_t na, const float* D, const int32_t* d_start, int64_t nd,
                                 const uint8_t* valid, int P, int64_t q_max, const int32_t* arg, const float* dist, const int32_t* count,
                                 const float* upstream, float* dA, void* stream) {
  const int rc = md_domain("lcr_min_dist_grad", P, na, nd, q_max);
  if (rc != LCR_OK) return rc;
  if (!a_start || !d_start || !count || !upstream || (na > 0 && (!A || !dist || !arg || !dA)) || (nd > 0 && !D))
    return refuse(LCR_EARG, "lcr_min_dist_grad: null pointer");
  if (q_max > 0)
    hipLaunchKernelGGL(k_md_grad, dim3(div_up(q_max, 256), P), dim3(256), 0, ST(stream), A, a_start, na, D, d_start, nd, valid, arg, dist,
                       count, upstream, dA);
  return check_launch("lcr_min_dist_grad");
}
