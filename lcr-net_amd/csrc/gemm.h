// gemm.h — what the fp32 GEMM's kernel families share: the argument structs, the fused epilogue, and the host-side checks.
// The families: gemm_f32.hip (register-staged tiles, light form, stream-K, the dispatcher), gemm_deep.hip (K-deep LDS-direct form),
// gemm_split.hip (split-bf16 form).
#pragma once
#include <cstdlib>

#include "common.h"

namespace lcr {

constexpr int GM_BK = 32;
constexpr int GM_T = 256;

// Optional batching over blockIdx.z: per-entry element offsets into A/B/C and per-entry K (NetVLAD's per-scan x^T·a products).
constexpr int GM_MAX_BATCH = 64;
struct GemmBatch {
  int     count;                 // 0 = plain GEMM
  int     strided;               // 1: entry z uses offsets z * {a,b,c}_off[0] and K = k[0] (uniform batch)
  int     k[GM_MAX_BATCH];
  int64_t a_off[GM_MAX_BATCH], b_off[GM_MAX_BATCH], c_off[GM_MAX_BATCH];
};

struct GemmEpilogue {
  const float*   bias;      // [N] or null
  const float*   rowdiv;    // [M] or null: C[m][:] /= rowdiv[m] (before the bias), KPConv neighbour-count normalisation
  const int64_t* seg_len;   // [S] rows per GroupNorm segment (device) or null
  int            S;
  int            groups;    // GroupNorm groups over N
  double*        stats;     // [GN_REPLICAS, S, groups, 2] (sum, sumsq), accumulated atomically; null = no statistics
};

// Normalise-on-load of the A operand: A holds the RAW output of the producing layer and the GroupNorm + LeakyReLU that the
// reference applies between the two layers (ResidualBlock: norm_conv + leaky_relu in front of unary2, modules.py:215-217) happens
// while the tile goes from registers to LDS — the normalised tensor is never written to memory (one stand-alone GroupNorm pass
// per residual block less).  Rows of A and rows of C share the segment table.
struct ANorm {
  const double* stats;    // [GN_REPLICAS, S, groups, 2] sums of the A producer (its GEMM epilogue)
  const float*  gamma;    // [K]
  const float*  beta;     // [K]
  int           groups;   // GroupNorm groups over K
  float         eps, slope;
};
constexpr int AN_KMAX = 256;   // K of the fused form (the light kernel: K <= 256)

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// The table of the normalise-on-load forms (k_gemm_f32<.., ANORM>, k_gemm_f32_bsplit_p<.., ANORM>), built once per 256-thread workgroup:
// s_an[slot][scale | shift][k] (AN_KMAX floats each) for the one or two segments a 64-row block touches (slot 0 = the segment of the block's
// first row, slot 1 = the next one; the host guarantees that no segment is shorter than the block).  Two calls, so that the loads of the
// first are in flight under the caller's segment scan:
//   anorm_load_affine: this thread's (gamma, beta) of table entries e = tid and tid + 256 (2 K <= 512);
//   anorm_build_table: (mean, rstd) per (slot, group) finalised in fp64 from the producer's statistics replicas by gn_finalise, as
//   lcr_groupnorm_apply does, then scale = rstd * gamma, shift = beta - mean * scale.  Ends with a barrier: the table is readable on return.
__device__ __forceinline__ void anorm_load_affine(const ANorm& an, int K, float (&an_g)[2], float (&an_b)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = threadIdx.x + u * GM_T;
    an_g[u] = an_b[u] = 0.f;
    if (e < 2 * K) {
      const int k = e >= K ? e - K : e;
      an_g[u] = an.gamma[k];
      an_b[u] = an.beta[k];
    }
  }
}

__device__ __forceinline__ void anorm_build_table(const ANorm& an, const GemmEpilogue& ep, int K, int blk_first, const float (&an_g)[2],
                                                  const float (&an_b)[2], float* __restrict__ s_an) {
  const int gs = K / an.groups;
  __shared__ float2 s_mr[2 * 64];                        // (mean, rstd) of [slot][group]
  for (int e = threadIdx.x; e < 2 * an.groups; e += GM_T) {
    const int slot = e >= an.groups ? 1 : 0, g = e - slot * an.groups;
    const int sg = min(blk_first + slot, ep.S - 1);
    const double cnt = static_cast<double>(ep.seg_len[sg]) * gs;
    double sx = 0.0, sxx = 0.0;                          // gn_mean_rstd's fold, written out: through the call one k_gemm_f32 form peels
    for (int rep = 0; rep < GN_REPLICAS; ++rep) {        // the first replica instead of the last
      const int64_t o = ((static_cast<int64_t>(rep) * ep.S + sg) * an.groups + g) * 2;
      sx += an.stats[o];
      sxx += an.stats[o + 1];
    }
    float mean, mean_lo, rstd;                           // mean_lo is not carried: the table is in scale / shift form
    gn_finalise(sx, sxx, cnt, an.eps, &mean, &mean_lo, &rstd);
    s_mr[e] = make_float2(mean, rstd);
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = threadIdx.x + u * GM_T;
    if (e < 2 * K) {
      const int slot = e >= K ? 1 : 0, k = e - slot * K;
      const float2 mr = s_mr[slot * an.groups + k / gs];
      const float sc = mr.y * an_g[u];
      s_an[slot * 2 * AN_KMAX + k] = sc;
      s_an[slot * 2 * AN_KMAX + AN_KMAX + k] = fmaf(-mr.x, sc, an_b[u]);
    }
  }
  __syncthreads();
}

// Epilogue shared by the tile-per-workgroup kernel and the stream-K kernel: C = acc [/ rowdiv] [+ bias], GroupNorm statistics.
template <int BM, int BN, int WM, int WN, int NT>
__device__ __forceinline__ void gemm_epilogue(floatx16 (&acc)[NT], float* __restrict__ C, int64_t M, int N, int64_t m0, int n0, int64_t m_tile,
                                              const GemmEpilogue& ep, const float (&bias_v)[NT], int blk_first, int64_t blk_seg_start,
                                              int64_t blk_seg_end, int wm, int wn, int lane) {
  const bool want_stats = ep.stats != nullptr;
  const int gs = want_stats ? N / ep.groups : 1;   // channels per group
  const int64_t wrow0 = m0 + wm * 32;

  // store (and keep the final values in the accumulators for the statistics pass)
  // Interior tiles (every row and column of the tile inside the matrix — all but the last row / column block; element offsets below 2^30):
  // one 32-bit offset per lane and value, a compile-time multiple of N apart, on the scalar base — 2-3 VALU instructions per stored value.
  // The general form below costs ~16 (64-bit row, bounds, 64-bit address) x 16 values x 4 wavefronts per tile: ~50 M of a step's 600 M VALU
  // instructions (PMC, profiles/r04_pmc_insts*.md).  Same values, same order.
  const bool interior = m0 + BM <= M && n0 + BN <= N && M * static_cast<int64_t>(N) < (int64_t(1) << 30);   // workgroup-uniform
  if (interior) {
    const unsigned row_l = static_cast<unsigned>(wrow0) + 4u * static_cast<unsigned>(lane >> 5);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const unsigned col = static_cast<unsigned>(n0 + wn * (32 * NT) + j * 32 + (lane & 31));
      const float bv = bias_v[j];
      const unsigned off0 = row_l * static_cast<unsigned>(N) + col;
      if (ep.rowdiv) {                                 // uniform: the KPConv contractions
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const unsigned dr = static_cast<unsigned>((r & 3) + 8 * (r >> 2));
          const float v = acc[j][r] / ep.rowdiv[row_l + dr] + bv;
          C[off0 + dr * static_cast<unsigned>(N)] = v;
          acc[j][r] = v;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const unsigned dr = static_cast<unsigned>((r & 3) + 8 * (r >> 2));
          const float v = acc[j][r] + bv;
          C[off0 + dr * static_cast<unsigned>(N)] = v;
          acc[j][r] = v;
        }
      }
    }
  } else
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = n0 + wn * (32 * NT) + j * 32 + (lane & 31);
    const float bv = bias_v[j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = wrow0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      float v = acc[j][r];
      if (row < M) {
        if (ep.rowdiv) v = v / ep.rowdiv[row];
        v += bv;
        if (col < N) C[row * N + col] = v;
      } else {
        v = 0.f;
      }
      acc[j][r] = v;
    }
  }

  // GroupNorm statistics.  Fast path (all BM rows of the workgroup in one segment — all but B-1 workgroups): every lane parks
  // the fp32 sums of its 16 values per column in LDS, one thread per column folds the 2*WM row slices in fp64, the gs lanes of
  // a group are folded with shuffles in the BN/64 wavefronts that hold the columns, and the workgroup issues one pair of
  // global fp64 atomics per group into the statistics replica (row block % GN_REPLICAS).  (A version with fp64 shuffles in
  // every wavefront + LDS fp64 atomics cost 8-9 us per unary GEMM.)  Slow path (a segment boundary inside the tile, or a segment
  // of fewer than GN_EXACT_ROWS rows): per wavefront, per segment present in its 32 rows, straight to global memory.
  // The fp32 partials cost sum x^2 / n - mean^2 a relative 1e-7 (|mean| / std)^2, and fp64 atomics of fp32 values add exactly, so the
  // table does not depend on the order in which the wavefronts arrive.  A group of a few values can have next to no variance, and
  // there the rounding of x^2 to fp32 was all that was left of it: segments of fewer than GN_EXACT_ROWS rows (groups of <= 32
  // columns) are summed in fp64 from the first addition.  Such a segment meets at most two wavefronts per column block, two
  // atomics per table entry, and a + b = b + a: still independent of the order.
  if (want_stats) {
    __shared__ float s_part[2][2 * WM][BN];
    double* rep = ep.stats + static_cast<int64_t>(m_tile % GN_REPLICAS) * ep.S * ep.groups * 2;
    int64_t seg_start = blk_seg_start, seg_end = blk_seg_end;
    const int64_t blk_last_row = min(m0 + BM - 1, M - 1);
    constexpr int GN_EXACT_ROWS = 32;
    auto exact_segment = [&](int64_t rows) { return rows < GN_EXACT_ROWS && gs <= 32; };      // the one rule for "summed in fp64"; wave-uniform
    const bool uniform = blk_last_row < seg_end && !exact_segment(seg_end - seg_start);       // block-uniform
    if (uniform) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        float s = 0.f, ss = 0.f;                      // rows beyond M hold zeros in the accumulators
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s += acc[j][r];
          ss = fmaf(acc[j][r], acc[j][r], ss);
        }
        const int cl = wn * (32 * NT) + j * 32 + (lane & 31);
        s_part[0][2 * wm + (lane >> 5)][cl] = s;
        s_part[1][2 * wm + (lane >> 5)][cl] = ss;
      }
      __syncthreads();
      if (threadIdx.x < BN) {
        const int cl = threadIdx.x;
        double ds = 0.0, dss = 0.0;
#pragma unroll
        for (int r = 0; r < 2 * WM; ++r) {
          ds += static_cast<double>(s_part[0][r][cl]);
          dss += static_cast<double>(s_part[1][r][cl]);
        }
        const int span = gs < 64 ? gs : 64;           // gs is a power of two; groups wider than 64 columns add per wavefront
        for (int d = 1; d < span; d <<= 1) {
          ds += __shfl_xor(ds, d);
          dss += __shfl_xor(dss, d);
        }
        const int col = n0 + cl;
        if ((cl & (span - 1)) == 0 && col < N) {
          double* d = rep + (static_cast<int64_t>(blk_first) * ep.groups + col / gs) * 2;
          atomicAdd(d, ds);
          atomicAdd(d + 1, dss);
        }
      }
    } else if (wrow0 < M) {
      const int64_t wlast = min(wrow0 + 31, M - 1);
      int sg = blk_first;
      while (sg + 1 < ep.S && wrow0 >= seg_end) {
        ++sg;
        seg_start = seg_end;
        seg_end += ep.seg_len[sg];
      }
      while (true) {   // wave-uniform loop over the segments that intersect [wrow0, wlast]
        const bool whole = seg_start <= wrow0 && wlast < seg_end;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int col = n0 + wn * (32 * NT) + j * 32 + (lane & 31);
          double ds, dss;
          if (exact_segment(seg_end - seg_start)) {
            ds = dss = 0.0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int64_t row = wrow0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
              float vf = (row >= seg_start && row < seg_end) ? acc[j][r] : 0.f;
              // converted here, one at a time.  Without the barrier the sixteen conversions are hoisted out of the segment loop and held
              // as doubles: the light-form kernels (cap 80 registers) then spill 8-12 bytes to scratch; with it they need no more than before.
              asm volatile("" : "+v"(vf));
              const double v = vf;
              ds += v;
              dss = fma(v, v, dss);
            }
          } else {
            float s = 0.f, ss = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int64_t row = wrow0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
              const float v = (whole || (row >= seg_start && row < seg_end)) ? acc[j][r] : 0.f;
              s += v;
              ss = fmaf(v, v, ss);
            }
            ds = s, dss = ss;
          }
          // fold the two row-halves, then the lanes of one group (gs consecutive columns, capped at the 32-column tile)
          ds += __shfl_xor(ds, 32);
          dss += __shfl_xor(dss, 32);
          const int span = gs < 32 ? gs : 32;
          for (int d = 1; d < span; d <<= 1) {
            ds += __shfl_xor(ds, d);
            dss += __shfl_xor(dss, d);
          }
          if (lane < 32 && (lane & (span - 1)) == 0 && col < N) {
            double* d = rep + (static_cast<int64_t>(sg) * ep.groups + col / gs) * 2;
            atomicAdd(d, ds);
            atomicAdd(d + 1, dss);
          }
        }
        if (wlast < seg_end || sg + 1 >= ep.S) break;
        ++sg;
        seg_start = seg_end;
        seg_end += ep.seg_len[sg];
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline int env_int(const char* name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; }

// The domain of the epilogue's statistics, for every entry point that takes a `stats` table: LCR_OK, or a refusal in the name of
// entry point `who` outside it.
inline int gemm_stats_domain(const char* who, const double* stats, const int64_t* seg_len, int S, int groups, int N) {
  if (!stats) return LCR_OK;
  if (seg_len && S >= 1 && groups >= 1 && N % groups == 0 && ((N / groups) & (N / groups - 1)) == 0) return LCR_OK;
  return refuse(LCR_EARG, "%s: statistics need seg_len, S >= 1 and groups dividing N into power-of-two sized groups", who);
}

// workgroups of a BM x BN tiling in the XCD-aware tile order: the row-block count is padded to a multiple of 8 (see k_gemm_f32)
inline int gemm_grid(int64_t M, int N, int BM, int BN) { return (div_up(M, BM) + 7) / 8 * 8 * div_up(N, BN); }

// block_k (columns per mask bit) -> log2(block_k / 32), or -1 when the mask cannot describe K
inline int mask_kshift(int K, int block_k) {
  for (int s = 0; s <= 3; ++s)
    if (block_k == (GM_BK << s)) return K <= 16 * block_k ? s : -1;
  return -1;
}

// The K-deep form (gemm_deep.hip) for C = A[M,K] · B[N,K]^T, K % 32 == 0, M*K and N*K < 2^30; amask / kshift: row-masked A or null.
// Owns the tile choice (N <= 32: 128x32, else 64x64).
int gemm_deep_launch(const char* who, const float* A, const float* B, float* C, int64_t M, int N, int K, const GemmEpilogue& ep, hipStream_t st,
                     const uint16_t* amask, int kshift);

}  // namespace lcr
