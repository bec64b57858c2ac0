// scan_context.hip — Scan Context (Kim & Kim, IROS 2018): the polar max-height image of a scan, its ring key and column-normalised form,
// and the exhaustive distance over all column shifts, for pairs and as a causal top-k search.  Semantics in include/lcr_hip.h
// (lcr_scan_context, lcr_scan_context_distance, lcr_scan_context_topk); restated in tests/scan_context_restatement.py.
//
// Descriptor: workgroups of SC_T threads take chunks of SC_CHUNK points of one cloud, bin each point in fp64 and take an integer maximum
//   on the order-preserving map of the fp32 height (f2ord) in an LDS image, then fold the touched bins into the cloud's image in the
//   workspace with the same integer maximum (order-free: a bin depends on no arrival order).  One workgroup per cloud finalises.
// Distance: one wavefront per pair.  G = unit_a^T unit_b (W x W, padded to 64 x 64, K = R padded to a multiple of 4 with zero rows) on
//   v_mfma_f32_32x32x2_f32 as four 32 x 32 tiles; G goes through the wavefront's 8 KB of LDS in two halves of 32 rows and lane s walks
//   G[j][(j + s) mod W], j ascending.
//   sc_pair() is that routine; both entries call it with the same operands in the same registers, so a pair has one set of bytes.
// Top-k: a workgroup of eight wavefronts holds eight queries' A fragments in registers and streams a chunk of database descriptors through a
//   double-buffered LDS tile that all eight read; distances and shifts go to a [Q, Cw] workspace, and one workgroup per row then selects
//   the k smallest (dist, index) keys with an 8-bit radix select and orders them by an all-pairs rank.
#include <climits>
#include <cmath>

#include "common.h"

namespace lcr {

constexpr int SC_MAX_R = 32, SC_MAX_W = 64, SC_KMAX = 128;
constexpr int SC_T = 256;            // threads of a binning / finalising / selecting workgroup
constexpr int SC_CHUNK = 4096;       // points per binning workgroup
constexpr int SC_QW = 8;             // queries (wavefronts) per search workgroup
constexpr int SC_COLS = 32;          // database descriptors per search workgroup
constexpr int SC_TILE = SC_MAX_R * SC_MAX_W;   // floats of a padded descriptor tile
constexpr int SC_GT = 32 * SC_MAX_W;           // floats of a wavefront's half Gram tile

struct ScBins {
  int    R, W;
  double max_length;
  float  height;
};

// ---- descriptor -----------------------------------------------------------------------------------------------------------
// bins u32[B, R*W]: 0 = empty (f2ord of a finite float is never 0)
__global__ __launch_bounds__(SC_T) void k_sc_bin(const float* __restrict__ points, Stack C, ScBins p, uint32_t* __restrict__ bins) {
  __shared__ uint32_t s_bin[SC_TILE];
  constexpr double TWO_PI = 6.283185307179586476925286766559;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n0 = C.off[b] + static_cast<int64_t>(blockIdx.x) * SC_CHUNK;
  if (n0 >= C.off[b + 1]) return;                                 // block-uniform
  const int64_t n1 = n0 + SC_CHUNK < C.off[b + 1] ? n0 + SC_CHUNK : C.off[b + 1];
  const int nb = p.R * p.W;
  for (int e = tid; e < nb; e += SC_T) s_bin[e] = 0u;
  __syncthreads();
  for (int64_t q = n0 + tid; q < n1; q += SC_T) {
    const float zf = points[3 * q + 2];
    const double x = static_cast<double>(points[3 * q]), y = static_cast<double>(points[3 * q + 1]);
    const double r = sqrt(dadd(dmul(x, x), dmul(y, y)));
    if (!(r < p.max_length) || !(fabsf(zf) < INFINITY)) continue;  // NaN and infinite coordinates end here
    double fr = floor(dmul(r / p.max_length, static_cast<double>(p.R)));
    fr = fr > static_cast<double>(p.R - 1) ? static_cast<double>(p.R - 1) : fr;
    double fs = 0.0;
    if (r > 0.0) {
      double th = atan2(y, x);
      if (th < 0.0) th = dadd(th, TWO_PI);
      fs = floor(dmul(th / TWO_PI, static_cast<double>(p.W)));
      fs = fs > static_cast<double>(p.W - 1) ? static_cast<double>(p.W - 1) : fs;
    }
    atomicMax(&s_bin[static_cast<int>(fr) * p.W + static_cast<int>(fs)], f2ord(fadd(zf, p.height)));
  }
  __syncthreads();
  for (int e = tid; e < nb; e += SC_T) {
    const uint32_t v = s_bin[e];
    if (v) atomicMax(&bins[static_cast<size_t>(b) * nb + e], v);
  }
}

__global__ __launch_bounds__(SC_T) void k_sc_finalise(const uint32_t* __restrict__ bins, int R, int W, float* __restrict__ desc,
                                                      float* __restrict__ ring_key, float* __restrict__ unit, uint64_t* __restrict__ mask) {
  __shared__ float s_d[SC_TILE];
  __shared__ float s_n[SC_MAX_W];
  const int b = blockIdx.x, tid = threadIdx.x, nb = R * W;
  const size_t base = static_cast<size_t>(b) * nb;
  for (int e = tid; e < nb; e += SC_T) {
    const uint32_t v = bins[base + e];
    const float d = v ? ord2f(v) : 0.f;
    s_d[e] = d;
    desc[base + e] = d;
  }
  __syncthreads();
  if (tid < 64) {                                                 // wavefront 0: a column per lane
    float n = 0.f;
    if (tid < W) {
      for (int i = 0; i < R; ++i) n = fadd(n, fmul(s_d[i * W + tid], s_d[i * W + tid]));
      n = sqrtf(n);                                             // correctly rounded (hipcc's default for fp32 sqrt and division)
      s_n[tid] = n;
    }
    const uint64_t m = wave_ballot(tid < W && n > 0.f);
    if (tid == 0) mask[b] = m;
  } else if (tid - 64 < R) {                                      // a ring per thread
    const int i = tid - 64;
    float s = 0.f;
    for (int j = 0; j < W; ++j) s = fadd(s, s_d[i * W + j]);
    ring_key[static_cast<size_t>(b) * R + i] = fdiv(s, static_cast<float>(W));
  }
  __syncthreads();
  for (int e = tid; e < nb; e += SC_T) {
    const float n = s_n[e % W];
    unit[base + e] = n > 0.f ? fdiv(s_d[e], n) : 0.f;
  }
}

// ---- the distance of one pair, by one wavefront ---------------------------------------------------------------------------------
__device__ __forceinline__ int sc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// A / B fragments of a descriptor for v_mfma_f32_32x32x2_f32: f[t][kk] = u[2 kk + half][32 t + col], zero outside R x W.  `ld` is the row
// stride of u: W for a descriptor in global memory, SC_MAX_W for a padded LDS tile (then R = K4, W = 64: nothing is outside).
template <int K2>
__device__ __forceinline__ void sc_fragments(const float* u, int R, int W, int ld, float (&f)[2][K2]) {
  const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int kk = 0; kk < K2; ++kk) {
      const int i = 2 * kk + half, j = 32 * t + col;
      f[t][kk] = (i < R && j < W) ? u[i * ld + j] : 0.f;
    }
}

// (dist, shift) of descriptors a, b from their fragments and masks; s_g: SC_GT floats of LDS owned by this wavefront.  The Gram matrix is
// formed and walked in two halves of 32 rows (j = 0 .. 31, then 32 .. W - 1), so that a wavefront needs 8 KB for it and a SIMD can hold four
// wavefronts, one's walk under another's MFMAs; the walk's order is j ascending all the same.  Every lane returns the same pair.
template <int K2>
__device__ __forceinline__ void sc_pair(const float (&af)[2][K2], const float (&bf)[2][K2], uint64_t ma, uint64_t mb, int W, float* s_g,
                                        float* dist, int* shift) {
  const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
  const int s = lane;
  const uint64_t full = W == 64 ? ~0ull : ((1ull << W) - 1ull);
  const uint64_t rot = s == 0 ? mb : (((mb >> (s & 63)) | (mb << ((W - s) & 63))) & full);      // bit j = mask_b[(j + s) mod W], for s < W
  const uint64_t v = s < W ? (ma & rot) : 0ull;
  float sum = 0.f;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    if (32 * mt >= W) continue;                                   // wave-uniform: rows nobody walks
    wave_sync();                                                  // the previous walk over s_g is over
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      if (32 * nt >= W) continue;                                 // wave-uniform: a tile nobody reads
      floatx16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int kk = 0; kk < K2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt][kk], bf[nt][kk], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) s_g[sc_row(r, half) * SC_MAX_W + 32 * nt + col] = acc[r];
    }
    wave_sync();
    if (s < W) {
      const int j_end = W < 32 * mt + 32 ? W : 32 * mt + 32;
      int jb = 32 * mt + s;                                       // (j + s) mod W: 32 + s < 2 W when the second half exists
      jb = jb >= W ? jb - W : jb;
      for (int j = 32 * mt; j < j_end; ++j) {
        if ((v >> j) & 1ull) sum = fadd(sum, s_g[(j - 32 * mt) * SC_MAX_W + jb]);
        jb = jb + 1 == W ? 0 : jb + 1;
      }
    }
  }
  uint64_t key = ~0ull;
  if (s < W) {
    const int c = __popcll(v);
    const float d = c > 0 ? fsub(1.f, fdiv(sum, static_cast<float>(c))) : 1.f;
    key = (static_cast<uint64_t>(f2ord(d)) << 32) | static_cast<uint32_t>(s);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t other = __shfl_xor(key, o);
    key = other < key ? other : key;
  }
  *dist = ord2f(static_cast<uint32_t>(key >> 32));
  *shift = static_cast<int>(static_cast<uint32_t>(key));
}

template <int K2>
__global__ __launch_bounds__(64) void k_sc_distance(const float* __restrict__ unit, const uint64_t* __restrict__ mask, int64_t B, int R, int W,
                                                    const int32_t* __restrict__ pairs, float* __restrict__ dist, int32_t* __restrict__ shift,
                                                    int32_t* __restrict__ status) {
  __shared__ float s_g[SC_GT];
  const int64_t p = blockIdx.x;
  const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
  if (ia < 0 || ia >= B || ib < 0 || ib >= B) {                   // wave-uniform: nothing of the pair is read
    if (threadIdx.x == 0) {
      dist[p] = __uint_as_float(0x7fc00000u);
      shift[p] = -1;
      atomicMax(status, static_cast<int32_t>(p < INT32_MAX ? p + 1 : INT32_MAX));
    }
    return;
  }
  float af[2][K2], bf[2][K2];
  sc_fragments<K2>(unit + static_cast<size_t>(ia) * R * W, R, W, W, af);
  sc_fragments<K2>(unit + static_cast<size_t>(ib) * R * W, R, W, W, bf);
  float d;
  int s;
  sc_pair<K2>(af, bf, mask[ia], mask[ib], W, s_g, &d, &s);
  if (threadIdx.x == 0) {
    dist[p] = d;
    shift[p] = s;
  }
}

__global__ void k_sc_clear(int32_t* status) { *status = 0; }

// ---- the causal search -----------------------------------------------------------------------------------------------------------
// Workgroup (x, y): query rows SC_QW y .. SC_QW y + SC_QW - 1 (a wavefront each), database frames SC_COLS x .. SC_COLS x + SC_COLS - 1.  Row r is frame
// q0 + r and sees frames j < lim(r) = clamp(q0 + r - exclude, 0, C).  wd / wsft [Q, ld]: the row's distances and shifts, j < lim(r) only.
template <int K2>
__global__ __launch_bounds__(64 * SC_QW) void k_sc_search(const float* __restrict__ unit, const uint64_t* __restrict__ mask, int64_t C, int R, int W,
                                                          int64_t Q, int64_t q0, int exclude, int64_t ld, float* __restrict__ wd,
                                                          int32_t* __restrict__ wsft) {
  extern __shared__ float s_dyn[];
  float* s_tile = s_dyn;                                          // [2][2 K2][64]: the database tile, double-buffered
  constexpr int TILE = 2 * K2 * SC_MAX_W;
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* s_g = s_dyn + 2 * TILE + w * SC_GT;
  const int64_t r_last = min(Q - 1, static_cast<int64_t>(blockIdx.y) * SC_QW + SC_QW - 1);
  const int64_t lim_blk = max(static_cast<int64_t>(0), min(C, q0 + r_last - exclude));
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * SC_COLS;
  if (j0 >= lim_blk) return;                                      // block-uniform
  const int64_t j1 = min(lim_blk, j0 + SC_COLS);
  const int64_t row = static_cast<int64_t>(blockIdx.y) * SC_QW + w;
  const bool have_q = row < Q;
  const int64_t lim = have_q ? max(static_cast<int64_t>(0), min(C, q0 + row - exclude)) : 0;
  float af[2][K2];
  uint64_t ma = 0;
  if (have_q) {                                                   // a query frame is a database frame: q0 + Q <= C
    sc_fragments<K2>(unit + static_cast<size_t>(q0 + row) * R * W, R, W, W, af);
    ma = mask[q0 + row];
  } else {
    sc_fragments<K2>(unit, 0, 0, W, af);
  }
  for (int e = tid; e < 2 * TILE; e += 64 * SC_QW) s_tile[e] = 0.f;    // the padding of both buffers stays zero
  const int nb = R * W;
  constexpr int PER = (TILE + 64 * SC_QW - 1) / (64 * SC_QW);
  float pre[PER];
  auto fetch = [&](int64_t j) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * 64 * SC_QW;
      pre[u] = e < nb ? unit[static_cast<size_t>(j) * nb + e] : 0.f;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * 64 * SC_QW;
      if (e < nb) s_tile[buf * TILE + (e / W) * SC_MAX_W + e % W] = pre[u];
    }
  };
  __syncthreads();
  fetch(j0);
  stage(0);
  __syncthreads();
  for (int64_t j = j0; j < j1; ++j) {
    const int buf = static_cast<int>(j - j0) & 1;
    if (j + 1 < j1) fetch(j + 1);                                 // in flight under the MFMAs
    if (j < lim) {                                                // wave-uniform
      float bf[2][K2];
      sc_fragments<K2>(s_tile + buf * TILE, 2 * K2, SC_MAX_W, SC_MAX_W, bf);
      float d;
      int s;
      sc_pair<K2>(af, bf, ma, mask[j], W, s_g, &d, &s);
      if ((tid & 63) == 0) {
        wd[row * ld + j] = d;
        wsft[row * ld + j] = s;
      }
    }
    if (j + 1 < j1) stage(buf ^ 1);                               // its last readers passed the barrier below one trip ago
    __syncthreads();
  }
}

// k smallest (dist, j) of every row, ascending, with their shifts; short rows padded with (-1, +inf, -1).  Keys are unique.
__global__ __launch_bounds__(SC_T) void k_sc_select(const float* __restrict__ wd, const int32_t* __restrict__ wsft, int64_t ld, int64_t C, int64_t q0,
                                                    int exclude, int k, int32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                    int32_t* __restrict__ out_shift) {
  __shared__ int s_hist[256];
  __shared__ uint64_t s_best[SC_KMAX];
  __shared__ uint64_t s_prefix;
  __shared__ int s_need, s_cnt;
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t lim = max(static_cast<int64_t>(0), min(C, q0 + row - exclude));
  const float* r = wd + row * ld;
  auto key_of = [&](int64_t j) { return (static_cast<uint64_t>(f2ord(r[j])) << 32) | static_cast<uint32_t>(j); };
  uint64_t thr = ~0ull;
  if (lim > k) {                                                  // block-uniform: the k-th smallest key by an MSB-first radix select
    if (tid == 0) {
      s_prefix = 0ull;
      s_need = k;
    }
    __syncthreads();
    for (int pass = 7; pass >= 0; --pass) {
      for (int i = tid; i < 256; i += SC_T) s_hist[i] = 0;
      __syncthreads();
      const uint64_t prefix = s_prefix;
      const uint64_t himask = pass == 7 ? 0ull : (~0ull << (8 * (pass + 1)));
      for (int64_t j = tid; j < lim; j += SC_T) {
        const uint64_t key = key_of(j);
        if ((key & himask) == prefix) atomicAdd(&s_hist[(key >> (8 * pass)) & 255], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int need = s_need, b = 0;
        for (; b < 255; ++b) {
          if (s_hist[b] >= need) break;
          need -= s_hist[b];
        }
        s_need = need;
        s_prefix = prefix | (static_cast<uint64_t>(b) << (8 * pass));
      }
      __syncthreads();
    }
    thr = s_prefix;
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int64_t j = tid; j < lim; j += SC_T) {
    const uint64_t key = key_of(j);
    if (key <= thr) {
      const int at = atomicAdd(&s_cnt, 1);
      if (at < SC_KMAX) s_best[at] = key;
    }
  }
  __syncthreads();
  const int nbest = min(s_cnt, k);
  for (int e = tid; e < k; e += SC_T) {
    if (e < nbest) {
      const uint64_t key = s_best[e];
      int rank = 0;
      for (int j = 0; j < nbest; ++j) rank += s_best[j] < key;
      const int32_t col = static_cast<int32_t>(static_cast<uint32_t>(key));
      out_idx[row * k + rank] = col;
      out_dist[row * k + rank] = ord2f(static_cast<uint32_t>(key >> 32));
      out_shift[row * k + rank] = wsft[row * ld + col];
    } else {
      out_idx[row * k + e] = -1;
      out_dist[row * k + e] = INFINITY;
      out_shift[row * k + e] = -1;
    }
  }
}

}  // namespace lcr

using namespace lcr;

namespace {

int sc_shape(const char* who, int R, int W) {
  if (R < 1 || R > SC_MAX_R || W < 1 || W > SC_MAX_W)
    return refuse(LCR_EARG, "%s: outside the domain (1 <= R <= %d, 1 <= W <= %d): R=%d W=%d", who, SC_MAX_R, SC_MAX_W, R, W);
  return LCR_OK;
}

size_t sc_bins_bytes(int B, int R, int W) { return align_up(sizeof(uint32_t) * static_cast<size_t>(B) * R * W); }

// columns any row of the search can see, and the workspace of [Q, Cw] distances and shifts
int64_t sc_cols(int64_t Q, int64_t q0, int64_t C, int exclude) { return std::max<int64_t>(0, std::min<int64_t>(C, q0 + Q - 1 - exclude)); }
struct ScSearchLayout {
  float*   wd;
  int32_t* wsft;
  int64_t  ld;
  size_t   bytes;
};
ScSearchLayout sc_search_layout(void* ws, int64_t Q, int64_t q0, int64_t C, int exclude) {
  ScSearchLayout L;
  Carver c(ws, ~size_t(0));
  L.ld = std::max<int64_t>(sc_cols(Q, q0, C, exclude), 1);
  const size_t n = static_cast<size_t>(std::max<int64_t>(Q, 1)) * static_cast<size_t>(L.ld);
  L.wd = c.take<float>(n);
  L.wsft = c.take<int32_t>(n);
  L.bytes = c.off;
  return L;
}

int sc_search_domain(const char* who, int64_t Q, int64_t q0, int64_t C, int exclude) {
  if (C < 1 || C > INT32_MAX || Q < 0 || q0 < 0 || Q > C || q0 > C - Q || exclude < 0)
    return refuse(LCR_EARG, "%s: outside the domain (1 <= C <= 2^31-1, 0 <= Q, 0 <= q0, q0 + Q <= C, exclude >= 0): C=%lld Q=%lld q0=%lld exclude=%d", who,
                  static_cast<long long>(C), static_cast<long long>(Q), static_cast<long long>(q0), exclude);
  return LCR_OK;
}

// the kernels are instantiated for K = R padded to a multiple of 4 (zero rows add nothing to a product)
template <int K2>
void sc_launch_distance(int64_t P, hipStream_t st, const float* unit, const uint64_t* mask, int64_t B, int R, int W, const int32_t* pairs, float* dist,
                        int32_t* shift, int32_t* status) {
  hipLaunchKernelGGL(k_sc_distance<K2>, dim3(static_cast<unsigned>(P)), dim3(64), 0, st, unit, mask, B, R, W, pairs, dist, shift, status);
}
template <int K2>
int sc_launch_search(const char* who, dim3 grid, hipStream_t st, const float* unit, const uint64_t* mask, int64_t C, int R, int W, int64_t Q, int64_t q0,
                     int exclude, const ScSearchLayout& L) {
  const size_t lds = sizeof(float) * (2 * 2 * K2 * SC_MAX_W + SC_QW * SC_GT);      // at most 80 KB
  static DynLds opt_in;
  if (opt_in.need(reinterpret_cast<const void*>(&k_sc_search<K2>), lds) != hipSuccess)
    return refuse(LCR_EHIP, "%s: cannot opt in to %zu bytes of LDS", who, lds);
  hipLaunchKernelGGL(k_sc_search<K2>, grid, dim3(64 * SC_QW), lds, st, unit, mask, C, R, W, Q, q0, exclude, L.ld, L.wd, L.wsft);
  return LCR_OK;
}
#define SC_BY_K(R, CALL)                  \
  switch (((R) + 3) / 4) {                \
    case 1: CALL(2); break;               \
    case 2: CALL(4); break;               \
    case 3: CALL(6); break;               \
    case 4: CALL(8); break;               \
    case 5: CALL(10); break;              \
    case 6: CALL(12); break;              \
    case 7: CALL(14); break;              \
    default: CALL(16); break;             \
  }

}  // namespace

extern "C" int lcr_scan_context_ws_bytes(int B, int R, int W, size_t* bytes) {
  if (!bytes || B < 1 || B > GRID_MAX_B)
    return refuse(LCR_EARG, "lcr_scan_context_ws_bytes: outside the domain (1 <= B <= %d, bytes non-null): B=%d", GRID_MAX_B, B);
  const int rc = sc_shape("lcr_scan_context_ws_bytes", R, W);
  if (rc) return rc;
  *bytes = sc_bins_bytes(B, R, W);
  return LCR_OK;
}

extern "C" int lcr_scan_context(const float* points, const int64_t* lengths, int B, int R, int W, double max_length, double lidar_height, float* desc,
                                float* ring_key, float* unit, uint64_t* mask, void* ws, size_t ws_bytes, void* stream) {
  Stack C;
  int rc = stack_from_lengths("lcr_scan_context", lengths, B, &C);
  if (rc) return rc;
  rc = sc_shape("lcr_scan_context", R, W);
  if (rc) return rc;
  if (!(max_length > 0.0) || !std::isfinite(max_length) || !std::isfinite(lidar_height))
    return refuse(LCR_EARG, "lcr_scan_context: outside the domain (0 < max_length finite, lidar_height finite): max_length=%g lidar_height=%g", max_length,
                  lidar_height);
  if (!desc || !ring_key || !unit || !mask || !ws) return refuse(LCR_EARG, "lcr_scan_context: null pointer");
  const int64_t n = C.off[B];
  if (n > 0 && !points) return refuse(LCR_EARG, "lcr_scan_context: null point array (n=%lld)", static_cast<long long>(n));
  const size_t need = sc_bins_bytes(B, R, W);
  if (need > ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_scan_context", ws_bytes, need);
  hipStream_t st = ST(stream);
  uint32_t* bins = static_cast<uint32_t*>(ws);
  if (hipMemsetAsync(bins, 0, sizeof(uint32_t) * static_cast<size_t>(B) * R * W, st) != hipSuccess)
    return refuse(LCR_EHIP, "lcr_scan_context: cannot clear the workspace");
  int64_t longest = 0;
  for (int b = 0; b < B; ++b) longest = std::max<int64_t>(longest, C.off[b + 1] - C.off[b]);
  if (longest > 0) {
    const ScBins p{R, W, max_length, static_cast<float>(lidar_height)};
    hipLaunchKernelGGL(k_sc_bin, dim3(static_cast<unsigned>((longest + SC_CHUNK - 1) / SC_CHUNK), static_cast<unsigned>(B)), dim3(SC_T), 0, st, points, C, p,
                       bins);
  }
  hipLaunchKernelGGL(k_sc_finalise, dim3(static_cast<unsigned>(B)), dim3(SC_T), 0, st, bins, R, W, desc, ring_key, unit, mask);
  return check_launch("lcr_scan_context");
}

extern "C" int lcr_scan_context_distance_ws_bytes(int64_t B, int R, int W, int64_t P, size_t* bytes) {
  if (!bytes || B < 1 || B > INT32_MAX || P < 0 || P > INT32_MAX)
    return refuse(LCR_EARG, "lcr_scan_context_distance_ws_bytes: outside the domain (1 <= B <= 2^31-1, 0 <= P <= 2^31-1, bytes non-null): B=%lld P=%lld",
                  static_cast<long long>(B), static_cast<long long>(P));
  const int rc = sc_shape("lcr_scan_context_distance_ws_bytes", R, W);
  if (rc) return rc;
  *bytes = 0;                                                     // a pair's Gram tile lives in LDS
  return LCR_OK;
}

extern "C" int lcr_scan_context_distance(const float* unit, const uint64_t* mask, int64_t B, int R, int W, const int32_t* pairs, int64_t P, float* dist,
                                         int32_t* shift, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  (void)ws;
  (void)ws_bytes;
  if (B < 1 || B > INT32_MAX || P < 0 || P > INT32_MAX)
    return refuse(LCR_EARG, "lcr_scan_context_distance: outside the domain (1 <= B <= 2^31-1, 0 <= P <= 2^31-1): B=%lld P=%lld", static_cast<long long>(B),
                  static_cast<long long>(P));
  const int rc = sc_shape("lcr_scan_context_distance", R, W);
  if (rc) return rc;
  if (P == 0) return LCR_OK;
  if (!unit || !mask || !pairs || !dist || !shift || !status) return refuse(LCR_EARG, "lcr_scan_context_distance: null pointer");
  hipStream_t st = ST(stream);
  hipLaunchKernelGGL(k_sc_clear, dim3(1), dim3(1), 0, st, status);
#define SC_CALL(K2) sc_launch_distance<K2>(P, st, unit, mask, B, R, W, pairs, dist, shift, status)
  SC_BY_K(R, SC_CALL)
#undef SC_CALL
  return check_launch("lcr_scan_context_distance");
}

extern "C" int lcr_scan_context_topk_ws_bytes(int64_t Q, int64_t q0, int64_t C, int exclude, size_t* bytes) {
  if (!bytes) return refuse(LCR_EARG, "lcr_scan_context_topk_ws_bytes: null pointer");
  const int rc = sc_search_domain("lcr_scan_context_topk_ws_bytes", Q, q0, C, exclude);
  if (rc) return rc;
  *bytes = sc_search_layout(nullptr, Q, q0, C, exclude).bytes;
  return LCR_OK;
}

extern "C" int lcr_scan_context_topk(const float* db_unit, const uint64_t* db_mask, int64_t C, int R, int W, int64_t Q, int64_t q0, int k, int exclude,
                                     int32_t* idx, float* dist, int32_t* shift, void* ws, size_t ws_bytes, void* stream) {
  int rc = sc_search_domain("lcr_scan_context_topk", Q, q0, C, exclude);
  if (rc) return rc;
  rc = sc_shape("lcr_scan_context_topk", R, W);
  if (rc) return rc;
  if (k < 1 || k > SC_KMAX) return refuse(LCR_EARG, "lcr_scan_context_topk: outside the domain (1 <= k <= %d): k=%d", SC_KMAX, k);
  if (Q == 0) return LCR_OK;
  if (!db_unit || !db_mask || !idx || !dist || !shift || !ws) return refuse(LCR_EARG, "lcr_scan_context_topk: null pointer");
  const ScSearchLayout L = sc_search_layout(ws, Q, q0, C, exclude);
  if (L.bytes > ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_scan_context_topk", ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  const int64_t cols = sc_cols(Q, q0, C, exclude);
  if (cols > 0) {
    const int64_t gy = (Q + SC_QW - 1) / SC_QW;
    for (int64_t y0 = 0; y0 < gy; y0 += 65535) {                  // the grid's y extent
      const int64_t ny = std::min<int64_t>(65535, gy - y0);
      // the rows of this slab are frames q0 + SC_QW y0 ..: pass them as a shifted q0 over shifted row pointers
      const int64_t r0 = y0 * SC_QW, rows = std::min<int64_t>(Q - r0, ny * SC_QW);
      const int64_t cmax = sc_cols(rows, q0 + r0, C, exclude);
      if (cmax == 0) continue;
      const dim3 grid(static_cast<unsigned>((cmax + SC_COLS - 1) / SC_COLS), static_cast<unsigned>(ny));
      ScSearchLayout S = L;
      S.wd = L.wd + r0 * L.ld;
      S.wsft = L.wsft + r0 * L.ld;
#define SC_CALL(K2) rc = sc_launch_search<K2>("lcr_scan_context_topk", grid, st, db_unit, db_mask, C, R, W, rows, q0 + r0, exclude, S)
      SC_BY_K(R, SC_CALL)
#undef SC_CALL
      if (rc) return rc;
    }
  }
  hipLaunchKernelGGL(k_sc_select, dim3(static_cast<unsigned>(Q)), dim3(SC_T), 0, st, L.wd, L.wsft, L.ld, C, q0, exclude, k, idx, dist, shift);
  return check_launch("lcr_scan_context_topk");
}
