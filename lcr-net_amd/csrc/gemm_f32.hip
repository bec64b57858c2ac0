// gemm_f32.hip — fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 FMA chain, 157 TFLOP/s peak)
// with the epilogues the KPConv encoder needs fused in:  C = (A·B) [/ rowdiv[m]] [+ bias[n]],  plus per-(segment, group)
// sum / sum-of-squares accumulation for the GroupNorm that always follows (modules/kpconv/modules.py:33-50, 53-84).
//
// Used for: nn.Linear of UnaryBlock (B = weight^T, TB=1), the kernel-point contraction of KPConv
// (kpconv.py:108-110: (M, 15*C) x (15*C, Cout), TB=0), NetVLAD's assignment / aggregation GEMMs (TA=1 for x^T·a).
// fp32 in, fp32 accumulate: bf16 would break the 1e-4 descriptor tolerance.
//
// Tiling: 256 threads = 4 wavefronts arranged WM x WN; block tile BM x BN x 32; every wavefront owns 32 rows x (BN/WN)
// columns = NT accumulators of 16 registers.  Operands are staged through LDS K-major (As[k][m], Bs[k][n]) so an MFMA
// operand fetch is one conflict-free ds_read_b32 per lane.  Because the fp32 MFMA is slow (64 cycles per 4 KFLOP) the
// only thing that matters is never exposing a latency: global loads are branch-free 16-B vectors issued one K-step ahead
// into registers (double-buffered LDS, one barrier per K-step), LDS fragments are prefetched one MFMA group ahead, and the
// tile shape is chosen so that >= ~400 workgroups exist (two per CU) even for the short-M stages.
// Two more forms live in files of their own and share gemm.h (structs, epilogue, host checks) with this one:
// gemm_deep.hip — the K-deep form (LDS-direct loads), which the dispatcher below launches through gemm_deep_launch, and its
// row-masked entry point; gemm_split.hip — the split-bf16 form and its entry points.
#include <cstdio>
#include <map>
#include <mutex>
#include <type_traits>

#include "gemm.h"

namespace lcr {

// R x 32 tile of a row-major [rows_total x K] matrix -> S[k][r]   (transposing loader; src contiguous along k).
// Branch-free: out-of-range pieces read a valid clamped address and are zeroed by a select.
// RM: the LDS tile is kept ROW-major instead (S[r][k], LD = 36): the store is one 16-B write per piece instead of four
// transposing 4-B ones, and an MFMA operand fetch becomes one 16-B read per FOUR MFMAs (see the K pairing in k_gemm_f32).
template <int R, int LD, bool VEC, bool RM = false>
struct LoaderT {
  static constexpr int PIECES = R * 8 / GM_T;   // float4 pieces per thread
  float4 reg[PIECES];
  unsigned okmask;                              // bit j: piece j is inside K (zeroing is deferred to the LDS store, so that
                                                // nothing waits on the load between its issue and its use one K-step later)
  int kb;                                       // k0 of the loaded tile (for the normalising store)
  __device__ __forceinline__ void load(const float* __restrict__ src, int64_t rows_total, int K, int64_t r0, int k0) {
    kb = k0;
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int f = threadIdx.x + GM_T * j;
      const int row = f >> 3, c4 = f & 7;
      int64_t gr = r0 + row;
      gr = gr < rows_total ? gr : rows_total - 1;          // duplicate rows only feed outputs that are never stored
      const int gk = k0 + c4 * 4;
      if (VEC) {
        const bool ok = gk < K;                               // K % 4 == 0: a piece is entirely in or out
        reg[j] = ld4(src + gr * K + (ok ? gk : 0));
        okmask = j == 0 ? (ok ? 1u : 0u) : (okmask | (ok ? (1u << j) : 0u));
      } else {
        const float* p = src + gr * K;
        float4 v;
        v.x = gk + 0 < K ? p[gk + 0] : 0.f;
        v.y = gk + 1 < K ? p[gk + 1] : 0.f;
        v.z = gk + 2 < K ? p[gk + 2] : 0.f;
        v.w = gk + 3 < K ? p[gk + 3] : 0.f;
        reg[j] = v;
        okmask = ~0u;
      }
    }
  }
  __device__ __forceinline__ void store_piece(float* __restrict__ S, int j) const {
    const int f = threadIdx.x + GM_T * j;
    const int row = f >> 3, c4 = f & 7;
    const bool ok = (okmask >> j) & 1u;
    if (RM) {
      *reinterpret_cast<float4*>(&S[row * LD + c4 * 4]) = ok ? reg[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      return;
    }
    S[(c4 * 4 + 0) * LD + row] = ok ? reg[j].x : 0.f;
    S[(c4 * 4 + 1) * LD + row] = ok ? reg[j].y : 0.f;
    S[(c4 * 4 + 2) * LD + row] = ok ? reg[j].z : 0.f;
    S[(c4 * 4 + 3) * LD + row] = ok ? reg[j].w : 0.f;
  }
  __device__ __forceinline__ void store(float* __restrict__ S) const {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) store_piece(S, j);
  }
  // row-major tiles only: y = leaky(x * scale[k] + shift[k]) with the (scale, shift) of the row's segment slot (tab[slot][0|1][k];
  // rows < split are slot 0, the others slot 1), then the same store as above
  __device__ __forceinline__ void store_norm(float* __restrict__ S, const float* __restrict__ tab, int split, float slope) const {
    static_assert(RM, "normalise-on-load is built for the row-major A tile");
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int f = threadIdx.x + GM_T * j;
      const int row = f >> 3, c4 = f & 7;
      const bool ok = (okmask >> j) & 1u;
      const float* t = tab + (row >= split ? 2 * AN_KMAX : 0) + (ok ? kb + c4 * 4 : 0);
      const float4 sc = *reinterpret_cast<const float4*>(t), sh = *reinterpret_cast<const float4*>(t + AN_KMAX);
      float4 v;
      v.x = fmaf(reg[j].x, sc.x, sh.x), v.y = fmaf(reg[j].y, sc.y, sh.y), v.z = fmaf(reg[j].z, sc.z, sh.z), v.w = fmaf(reg[j].w, sc.w, sh.w);
      v.x = v.x > 0.f ? v.x : v.x * slope, v.y = v.y > 0.f ? v.y : v.y * slope;
      v.z = v.z > 0.f ? v.z : v.z * slope, v.w = v.w > 0.f ? v.w : v.w * slope;
      *reinterpret_cast<float4*>(&S[row * LD + c4 * 4]) = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
};

// 32 x W tile of a row-major [K x cols_total] matrix -> S[k][c]   (straight loader; src contiguous along c)
template <int W, int LD, bool VEC>
struct LoaderN {
  static constexpr int PIECES = 8 * W / GM_T;
  float4 reg[PIECES];
  unsigned okmask;
  __device__ __forceinline__ void load(const float* __restrict__ src, int64_t cols_total, int K, int64_t c0, int k0) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int f = threadIdx.x + GM_T * j;
      const int kr = f / (W / 4), c4 = f % (W / 4);
      const int gk = k0 + kr;
      const int64_t gc = c0 + c4 * 4;
      const bool kok = gk < K;
      const float* p = src + static_cast<int64_t>(kok ? gk : 0) * cols_total;
      if (VEC) {
        const bool ok = kok && gc < cols_total;              // cols_total % 4 == 0
        reg[j] = ld4(p + (gc < cols_total ? gc : 0));
        okmask = j == 0 ? (ok ? 1u : 0u) : (okmask | (ok ? (1u << j) : 0u));
      } else {
        float4 v;
        v.x = (kok && gc + 0 < cols_total) ? p[gc + 0] : 0.f;
        v.y = (kok && gc + 1 < cols_total) ? p[gc + 1] : 0.f;
        v.z = (kok && gc + 2 < cols_total) ? p[gc + 2] : 0.f;
        v.w = (kok && gc + 3 < cols_total) ? p[gc + 3] : 0.f;
        reg[j] = v;
        okmask = ~0u;
      }
    }
  }
  __device__ __forceinline__ void store_piece(float* __restrict__ S, int j) const {
    const int f = threadIdx.x + GM_T * j;
    const int kr = f / (W / 4), c4 = f % (W / 4);
    const bool ok = (okmask >> j) & 1u;
    *reinterpret_cast<float4*>(&S[kr * LD + c4 * 4]) = ok ? reg[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __device__ __forceinline__ void store(float* __restrict__ S) const {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) store_piece(S, j);
  }
};

// SHORT = the light form for K <= 128 (the unary Linears of the big stages): such a problem is all prologue — load, one to four
// K-steps, epilogue — so what hides the load latency is the number of workgroups a CU holds, not prefetch depth: one LDS
// buffer (17 KB), one register stage, shallow fragment prefetch, and a register budget that lets 6-8 workgroups share a CU
// instead of 4.
template <int BM, int BN, int WM, int WN, bool TA, bool TB, bool VEC, bool SHORT = false, bool ANORM = false>
__global__ __launch_bounds__(GM_T, SHORT ? 6 : 2) void k_gemm_f32(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C,
                                                       int64_t M, int N, int K, GemmEpilogue ep, GemmBatch batch, ANorm an) {
  static_assert(!ANORM || (SHORT && !TA && VEC && BN / (32 * WN) == 1), "normalise-on-load: light form, row-major A");
  static_assert(WM * WN == 4 && BM == 32 * WM, "one 32-row MFMA tile per wavefront along M");
  if (batch.count) {
    const int z = blockIdx.z;
    if (batch.strided) {
      A += static_cast<int64_t>(z) * batch.a_off[0];
      B += static_cast<int64_t>(z) * batch.b_off[0];
      C += static_cast<int64_t>(z) * batch.c_off[0];
      K = batch.k[0];
    } else {
      A += batch.a_off[z];
      B += batch.b_off[z];
      C += batch.c_off[z];
      K = batch.k[z];
    }
  }
  constexpr int NT = BN / (32 * WN);
  constexpr int NBUF = SHORT ? 1 : 2;
  // K pairing.  A 32x32x2 MFMA consumes two K indices (lanes 0-31 one, lanes 32-63 the other); which two is free as long as A
  // and B agree.  With one accumulator per wavefront (NT == 1: every encoder GEMM) MFMA j of a 32-deep K-step takes (j, j + 16):
  // a lane then needs 16 CONSECUTIVE k of its row, so an operand whose global layout is k-contiguous (A [M,K]; B = nn.Linear
  // weight [N,K]) stays row-major in LDS — stored with one 16-B write per piece, fetched with four 16-B reads per K-step instead
  // of sixteen 4-B ones.  (Before: (2j, 2j+1) on K-major tiles, 48 LDS instructions per wavefront and K-step; now 12 for the
  // unary Linears, 24 for the KPConv contraction whose B [K,N] stays K-major.)  Multi-accumulator tiles keep the old scheme.
  constexpr bool NEWP = NT == 1;
  constexpr bool ARM = NEWP && !TA, BRM = NEWP && TB;
  constexpr int LDR = GM_BK + 4;
  constexpr int LDA = ARM ? LDR : (TA ? BM + 4 : BM + 1);
  constexpr int LDB = BRM ? LDR : (TB ? BN + 1 : BN + 4);
  __shared__ __attribute__((aligned(16))) float As[NBUF][ARM ? BM * LDR : GM_BK * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[NBUF][BRM ? BN * LDR : GM_BK * LDB];

  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave index in an SGPR
  const int wm = w / WN, wn = w % WN;
  // XCD-aware tile order.  Workgroups go round-robin to the 8 XCDs (linear id % 8), each with its own L2; the column tiles
  // of one row block all read the same A rows, so they are given ids that land on ONE XCD back to back: the A tile is then
  // fetched from HBM / Infinity Cache once instead of once per column tile (PMC: GEMM fetch traffic was ~2x algorithmic).
  const int ntn = (N + BN - 1) / BN;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int64_t m_tile = static_cast<int64_t>(slot / ntn) * 8 + xcd;
  const int64_t m0 = m_tile * BM;
  const int n0 = (slot % ntn) * BN;
  if (m0 >= M) return;                     // padding of the row-block count to a multiple of 8

  // two register stages: the tile for K-step t+2 is requested while step t computes and step t+1 already sits in registers,
  // so a global load has two full MFMA phases (~2 x 1024 cycles) to land before it is needed for the LDS store
  LoaderT<BM, LDA, VEC, ARM> la_t[NBUF];
  LoaderN<BM, LDA, VEC> la_n[NBUF];
  LoaderT<BN, LDB, VEC, BRM> lb_t[NBUF];
  LoaderN<BN, LDB, VEC> lb_n[NBUF];

  auto gload = [&](int k0, int r) {
    if (TA) la_n[r].load(A, M, K, m0, k0);
    else la_t[r].load(A, M, K, m0, k0);
    if (TB) lb_t[r].load(B, N, K, n0, k0);
    else lb_n[r].load(B, N, K, n0, k0);
  };
  auto sstore = [&](int buf, int r) {
    if (TA) la_n[r].store(As[buf]);
    else la_t[r].store(As[buf]);
    if (TB) lb_t[r].store(Bs[buf]);
    else lb_n[r].store(Bs[buf]);
  };

  // The 128x32 tile (N = 32: the stage-1 KPConv contraction) chains every MFMA on one accumulator, where any issue bubble
  // costs a full 64-cycle latency: it alternates between two accumulator sets (even / odd K pairs), +10 % measured.  The
  // 64x64 tile measured slower with the extra registers, so it keeps one.
  constexpr int NACC = (NT == 1 && BM == 128) ? 2 : 1;
  floatx16 acc[NT], acc2[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[j][r] = 0.f;
      acc2[j][r] = 0.f;
    }

  const int nk = (K + GM_BK - 1) / GM_BK;                 // K may have been replaced by a per-entry value above
  // Both prologue tiles are requested before anything waits (for nk == 1 the second request re-reads tile 0: its pieces are
  // out of K, so their addresses fall back to column 0 — cache hits, never stored).  The epilogue's per-column bias and the
  // GroupNorm segment of this row block (a chain of dependent scalar loads) are fetched here too, under the same latency.
  gload(0, 0);
  if (!SHORT) gload(GM_BK, NBUF - 1);
  const bool want_stats = ep.stats != nullptr;
  float bias_v[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = n0 + (w % WN) * (32 * NT) + j * 32 + (lane & 31);
    bias_v[j] = (ep.bias && col < N) ? ep.bias[col] : 0.f;
  }
  float an_g[2] = {0.f, 0.f}, an_b[2] = {0.f, 0.f};           // normalise-on-load: this thread's (gamma, beta) of table entries
  if constexpr (ANORM) anorm_load_affine(an, K, an_g, an_b);   // e = tid and tid + 256 (2 K <= 512), requested before the segment scan
  int blk_first = 0;
  int64_t blk_seg_start = 0, blk_seg_end = 0;
  if (want_stats || ANORM) {
    blk_seg_end = ep.seg_len[0];
    while (blk_first + 1 < ep.S && m0 >= blk_seg_end) {
      ++blk_first;
      blk_seg_start = blk_seg_end;
      blk_seg_end += ep.seg_len[blk_first];
    }
  }
  __shared__ __attribute__((aligned(16))) float s_an[ANORM ? 4 * AN_KMAX : 4];   // [slot][scale | shift][k]
  int an_split = BM;
  if constexpr (ANORM) {
    // (scale, shift) per channel for the one or two segments this row block touches (anorm_build_table, gemm.h)
    an_split = static_cast<int>(min(static_cast<int64_t>(BM), blk_seg_end - m0));
    anorm_build_table(an, ep, K, blk_first, an_g, an_b, s_an);
  }
  auto sstore_a0 = [&]() {                                 // the light form's (only) A store
    if constexpr (ANORM) la_t[0].store_norm(As[0], s_an, an_split, an.slope);
  };
  if constexpr (ANORM) {
    sstore_a0();
    lb_t[0].store(Bs[0]);
  } else {
    sstore(0, 0);
  }
  __syncthreads();
  const int half = lane >> 5;
  const int a_off = ARM ? (wm * 32 + (lane & 31)) * LDR + half * 16 : half * (NEWP ? 16 : 1) * LDA + wm * 32 + (lane & 31);
  const int b_off = BRM ? (wn * (32 * NT) + (lane & 31)) * LDR + half * 16 : half * (NEWP ? 16 : 1) * LDB + wn * (32 * NT) + (lane & 31);
  // operands of MFMAs 4q .. 4q+3 of a K-step (NEWP only)
  auto fetch4_a = [&](const float* as, int q, float (&o)[4]) {
    if (ARM) {
      const float4 v = *reinterpret_cast<const float4*>(as + 4 * q);
      o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = as[(4 * q + i) * LDA];
    }
  };
  auto fetch4_b = [&](const float* bs, int q, float (&o)[4]) {
    if (BRM) {
      const float4 v = *reinterpret_cast<const float4*>(bs + 4 * q);
      o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = bs[(4 * q + i) * LDB];
    }
  };
  if constexpr (SHORT) {
    constexpr int KKS = GM_BK / 2, PFS = 4;
    for (int t = 0; t < nk; ++t) {
      if (t > 0) {
        gload(t * GM_BK, 0);
        __syncthreads();                                        // every wavefront has read step t-1's fragments
        if constexpr (ANORM) {
          sstore_a0();
          lb_t[0].store(Bs[0]);
        } else {
          sstore(0, 0);
        }
        __syncthreads();
      }
      const float* as = As[0] + a_off;
      const float* bs = Bs[0] + b_off;
      static_assert(NEWP, "the light form is only instantiated for single-accumulator tiles");
      float af[2][4], bf[2][4];                               // two groups of four MFMAs in flight
      fetch4_a(as, 0, af[0]);
      fetch4_b(bs, 0, bf[0]);
      fetch4_a(as, 1, af[1]);
      fetch4_b(bs, 1, bf[1]);
#pragma unroll
      for (int q = 0; q < KKS / 4; ++q) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q & 1][i], bf[q & 1][i], acc[0], 0, 0, 0);
        if (q + 2 < KKS / 4) {
          fetch4_a(as, q + 2, af[q & 1]);
          fetch4_b(bs, q + 2, bf[q & 1]);
        }
      }
    }
  } else {
  // One K-step: compute LDS buffer BUF while (a) the tile for step t+2 is requested into register set BUF and (b) the tile
  // for step t+1 (register set 1-BUF) is written to LDS buffer 1-BUF — its ds_writes are issued BETWEEN the MFMAs, and the
  // MFMA operand fragments are read PF K-pairs ahead: LDS latency (~100+ cycles) exceeds one 64-cycle MFMA, so a one-deep
  // prefetch exposes a bubble on every MFMA when a SIMD holds a single wavefront (measured: the loop skeleton, the MFMAs and
  // the global-load stalls simply added up).
  constexpr int KK = GM_BK / 2;
  constexpr int PF = NT == 1 ? KK : (NT == 2 ? 8 : 4);           // fragment prefetch depth (registers: PF * (1 + NT))
  constexpr int PA = BM * 8 / GM_T, PB = BN * 8 / GM_T;           // LDS-store pieces per thread for the A / B tile
  constexpr int ST0 = KK - (PA + PB) - 1 > 2 ? (KK - (PA + PB)) / 2 : 1;   // first K-pair that carries a store piece
  // FULL = steps t+1 and t+2 exist: no branches in the body, which keeps the whole K-step one basic block (the waitcnt
  // insertion is only exact inside a block: with the conditional stores it waited for the loads it had just issued).
  auto step = [&](auto buf_c, auto full_c, int t) {
    constexpr int BUF = decltype(buf_c)::value;
    constexpr bool FULL = decltype(full_c)::value;
    if (FULL || t + 2 < nk) gload((t + 2) * GM_BK, BUF);
    const bool do_store = FULL || t + 1 < nk;                     // block-uniform
    const float* as = As[BUF] + a_off;
    const float* bs = Bs[BUF] + b_off;
    float af[PF], bf[PF][NT];
    if constexpr (NEWP) {                                         // PF == KK: the whole K-step's operands, in 16-B reads where row-major
#pragma unroll
      for (int q = 0; q < KK / 4; ++q) {
        float a4[4], b4[4];
        fetch4_a(as, q, a4);
        fetch4_b(bs, q, b4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          af[4 * q + i] = a4[i];
          bf[4 * q + i][0] = b4[i];
        }
      }
    } else {
#pragma unroll
      for (int d = 0; d < PF; ++d) {
        af[d] = as[d * 2 * LDA];
#pragma unroll
        for (int j = 0; j < NT; ++j) bf[d][j] = bs[d * 2 * LDB + j * 32];
      }
    }
    __builtin_amdgcn_sched_barrier(0);                            // keep the fragment reads ahead of the MFMA chain
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int sl = kk % PF;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if (NACC == 2 && (kk & 1)) acc2[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[sl], bf[sl][j], acc2[j], 0, 0, 0);
        else acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[sl], bf[sl][j], acc[j], 0, 0, 0);
      }
      if (kk + PF < KK) {
        af[sl] = as[(kk + PF) * 2 * LDA];
#pragma unroll
        for (int j = 0; j < NT; ++j) bf[sl][j] = bs[(kk + PF) * 2 * LDB + j * 32];
      }
      const int piece = kk - ST0;                                 // compile-time after unrolling
      if (do_store && piece >= 0 && piece < PA + PB) {
        if (piece < PA) {
          if (TA) la_n[1 - BUF].store_piece(As[1 - BUF], piece);
          else la_t[1 - BUF].store_piece(As[1 - BUF], piece);
        } else {
          if (TB) lb_t[1 - BUF].store_piece(Bs[1 - BUF], piece - PA);
          else lb_n[1 - BUF].store_piece(Bs[1 - BUF], piece - PA);
        }
      }
    }
    __syncthreads();
  };
  int t = 0;
  for (; t + 3 < nk; t += 2) {
    step(std::integral_constant<int, 0>{}, std::true_type{}, t);
    step(std::integral_constant<int, 1>{}, std::true_type{}, t + 1);
  }
  for (; t < nk; t += 2) {
    step(std::integral_constant<int, 0>{}, std::false_type{}, t);
    if (t + 1 >= nk) break;
    step(std::integral_constant<int, 1>{}, std::false_type{}, t + 1);
  }

  }

  if (NACC == 2) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] += acc2[j][r];
  }

  gemm_epilogue<BM, BN, WM, WN, NT>(acc, C, M, N, m0, n0, m_tile, ep, bias_v, blk_first, blk_seg_start, blk_seg_end, wm, wn, lane);
}

// ---- stream-K form of the K-deep contractions ---------------------------------------------------------------------------
// With one tile per workgroup, 408 / 596 / 806 tiles of 64x64 on 256 CUs (<= 3 resident workgroups each) leave some CUs with one
// tile more than others: the deepest KPConv contractions lose ~20 % to that quantisation.  Here the grid is a fixed number of
// persistent workgroups (a multiple of the CU count) and every workgroup takes an equal, CONTIGUOUS range of (tile, K-step)
// iterations, so it touches at most two partial tiles.  Nobody waits for anybody: a workgroup parks every partial tile it
// computes (16 KB, device-coherent stores), then bumps the tile's arrival counter; the workgroup that arrives LAST folds all the
// pieces of the tile in ascending workgroup order (its own included, read back like the others: the sum is the same whoever
// folds), runs the epilogue and resets the counter for the next launch.  (Two earlier protocols with an owner waiting for the
// others' flags: in range order the waits chain up — 20x slower; with the shared pieces computed first an owner still idles
// whenever its neighbour's piece is the longer one — erratic, 0.8-1.4x.)  Tiles are dealt to the XCDs as in k_gemm_f32 (row
// block % 8) and the iteration ranges are cut inside one XCD's band, so the column tiles of a row block stay on one L2.
struct GemmStreamK {
  float*    partial;   // [grid][2][NT * 16][GM_T]: slot 0 = the piece a workgroup's range starts with, slot 1 = any later piece
  uint32_t* arrived;   // [tiles] pieces parked so far; zero between launches
  int       U;         // workgroups per XCD band (grid = 8 * U)
};

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(GM_T, 3) void k_gemm_f32_sk(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C,
                                                         int64_t M, int N, int K, GemmEpilogue ep, GemmStreamK sk) {
  static_assert(WM * WN == 4 && BM == 32 * WM, "one 32-row MFMA tile per wavefront along M");
  constexpr int LDA = BM + 1, LDB = BN + 4;
  constexpr int NT = BN / (32 * WN);
  __shared__ __attribute__((aligned(16))) float As[2][GM_BK * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2][GM_BK * LDB];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w / WN, wn = w % WN;
  const int ntn = (N + BN - 1) / BN;
  const int64_t mt = (M + BM - 1) / BM;
  const int xcd = blockIdx.x & 7, u = blockIdx.x >> 3;
  const int64_t mt_x = mt > xcd ? (mt - xcd + 7) / 8 : 0;          // row blocks of this XCD's band: m_tile = 8 * i + xcd
  const int nk = (K + GM_BK - 1) / GM_BK;
  const int64_t I = mt_x * ntn * nk;                                // iterations of the band
  auto first_it = [&](int uu) { return static_cast<int64_t>(uu) * I / sk.U; };
  const int64_t it_begin = first_it(u), it_end = first_it(u + 1);
  LoaderT<BM, LDA, true> la[2];
  LoaderN<BN, LDB, true> lb[2];
  const int a_off = (lane >> 5) * LDA + wm * 32 + (lane & 31);
  const int b_off = (lane >> 5) * LDB + wn * (32 * NT) + (lane & 31);
  constexpr int PIECE = NT * 16 * GM_T;                             // floats of one parked partial tile
  __shared__ unsigned s_arrived;

  int64_t it = it_begin;
  while (it < it_end) {
    const int64_t lt = it / nk;
    const int ks = static_cast<int>(it - lt * nk);
    const int ns = static_cast<int>(min(static_cast<int64_t>(nk - ks), it_end - it));        // K-steps of this segment
    const int64_t m_tile = (lt / ntn) * 8 + xcd;
    const int64_t m0 = m_tile * BM;
    const int n0 = static_cast<int>(lt % ntn) * BN;
    const int k_begin = ks * GM_BK;
    auto gload = [&](int k0, int r) {
      la[r].load(A, M, K, m0, k0);
      lb[r].load(B, N, K, n0, k0);
    };
    floatx16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    gload(k_begin, 0);
    gload(k_begin + GM_BK, 1);
    const bool covers_end = ks + ns == nk, covers_start = ks == 0;
    float bias_v[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = n0 + wn * (32 * NT) + j * 32 + (lane & 31);
      bias_v[j] = (ep.bias && col < N) ? ep.bias[col] : 0.f;
    }
    int blk_first = 0;
    int64_t blk_seg_start = 0, blk_seg_end = 0;
    la[0].store(As[0]);
    lb[0].store(Bs[0]);
    __syncthreads();

    // the K-step of k_gemm_f32 (see there): fragments PF K-pairs ahead, next tile's LDS stores between the MFMAs
    constexpr int KK = GM_BK / 2;
    constexpr int PF = NT == 1 ? KK : (NT == 2 ? 8 : 4);
    constexpr int PA = BM * 8 / GM_T, PB = BN * 8 / GM_T;
    constexpr int ST0 = KK - (PA + PB) - 1 > 2 ? (KK - (PA + PB)) / 2 : 1;
    auto step = [&](auto buf_c, auto full_c, int t) {
      constexpr int BUF = decltype(buf_c)::value;
      constexpr bool FULL = decltype(full_c)::value;
      if (FULL || t + 2 < ns) gload(k_begin + (t + 2) * GM_BK, BUF);
      const bool do_store = FULL || t + 1 < ns;
      const float* as = As[BUF] + a_off;
      const float* bs = Bs[BUF] + b_off;
      float af[PF], bf[PF][NT];
#pragma unroll
      for (int d = 0; d < PF; ++d) {
        af[d] = as[d * 2 * LDA];
#pragma unroll
        for (int j = 0; j < NT; ++j) bf[d][j] = bs[d * 2 * LDB + j * 32];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const int sl = kk % PF;
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[sl], bf[sl][j], acc[j], 0, 0, 0);
        if (kk + PF < KK) {
          af[sl] = as[(kk + PF) * 2 * LDA];
#pragma unroll
          for (int j = 0; j < NT; ++j) bf[sl][j] = bs[(kk + PF) * 2 * LDB + j * 32];
        }
        const int piece = kk - ST0;
        if (do_store && piece >= 0 && piece < PA + PB) {
          if (piece < PA) la[1 - BUF].store_piece(As[1 - BUF], piece);
          else lb[1 - BUF].store_piece(Bs[1 - BUF], piece - PA);
        }
      }
      __syncthreads();
    };
    int t = 0;
    for (; t + 3 < ns; t += 2) {
      step(std::integral_constant<int, 0>{}, std::true_type{}, t);
      step(std::integral_constant<int, 1>{}, std::true_type{}, t + 1);
    }
    for (; t < ns; t += 2) {
      step(std::integral_constant<int, 0>{}, std::false_type{}, t);
      if (t + 1 >= ns) break;
      step(std::integral_constant<int, 1>{}, std::false_type{}, t + 1);
    }

    bool finish = true;
    if (!(covers_start && covers_end)) {
      // park this piece: device-coherent stores (a device-scope release FENCE per workgroup would write back the XCD's whole L2:
      // measured 2x slower overall), then count it in once every lane's stores are acknowledged
      float* mine = sk.partial + (static_cast<int64_t>(blockIdx.x) * 2 + (it == it_begin ? 0 : 1)) * PIECE;
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          __hip_atomic_store(&mine[(j * 16 + r) * GM_T + threadIdx.x], acc[j][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // the workgroups that hold pieces of this tile: uf .. ul of this band (those with a non-empty range)
      const int64_t tile_it0 = lt * nk, tile_it1 = tile_it0 + nk;
      int uf = static_cast<int>(tile_it0 * sk.U / I);
      while (uf > 0 && first_it(uf) > tile_it0) --uf;
      while (first_it(uf + 1) <= tile_it0) ++uf;
      int ul = uf, pieces = 0;
      for (int uu = uf; uu < sk.U && first_it(uu) < tile_it1; ++uu)
        if (first_it(uu + 1) > first_it(uu)) {
          ul = uu;
          ++pieces;
        }
      __builtin_amdgcn_s_waitcnt(0);                                       // THIS wavefront's parked values are acknowledged ...
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();                                                     // ... and so are the other three's, before the count
      uint32_t* cnt = sk.arrived + (m_tile * ntn + lt % ntn);
      if (threadIdx.x == 0) s_arrived = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      finish = s_arrived == static_cast<unsigned>(pieces - 1);           // block-uniform: the last piece to arrive folds the tile
      if (finish) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        for (int uu = uf; uu <= ul; ++uu) {
          if (first_it(uu + 1) <= first_it(uu)) continue;
          const float* pp = sk.partial + (static_cast<int64_t>(uu * 8 + xcd) * 2 + (first_it(uu) >= tile_it0 ? 0 : 1)) * PIECE;
#pragma unroll
          for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              acc[j][r] += __hip_atomic_load(&pp[(j * 16 + r) * GM_T + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (threadIdx.x == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (finish) {
      if (ep.stats != nullptr) {                                           // GroupNorm segment of this row block
        blk_first = 0;
        blk_seg_start = 0;
        blk_seg_end = ep.seg_len[0];
        while (blk_first + 1 < ep.S && m0 >= blk_seg_end) {
          ++blk_first;
          blk_seg_start = blk_seg_end;
          blk_seg_end += ep.seg_len[blk_first];
        }
      }
      gemm_epilogue<BM, BN, WM, WN, NT>(acc, C, M, N, m0, n0, m_tile, ep, bias_v, blk_first, blk_seg_start, blk_seg_end, wm, wn, lane);
    }
    it += ns;
    __syncthreads();                                                       // LDS is reused by the next segment
  }
}

template <int BM, int BN, int WM, int WN, bool VEC, bool SHORT = false>
static int launch_gemm(const char* who, const float* A, const float* B, float* C, int64_t M, int N, int K, int transA, int transB, const GemmEpilogue& ep,
                       hipStream_t st, const GemmBatch* batch = nullptr) {
  static const GemmBatch no_batch = {};
  const GemmBatch& bt = batch ? *batch : no_batch;
  dim3 grid(gemm_grid(M, N, BM, BN), 1, bt.count ? bt.count : 1);     // see the XCD-aware tile order in the kernel
  dim3 block(GM_T);
  if (!transA && !transB) LCR_LAUNCH_TIMED((k_gemm_f32<BM, BN, WM, WN, false, false, VEC, SHORT>), grid, block, 0, st, A, B, C, M, N, K, ep, bt, ANorm{});
  else if (!transA && transB) LCR_LAUNCH_TIMED((k_gemm_f32<BM, BN, WM, WN, false, true, VEC, SHORT>), grid, block, 0, st, A, B, C, M, N, K, ep, bt, ANorm{});
  else if (transA && !transB) LCR_LAUNCH_TIMED((k_gemm_f32<BM, BN, WM, WN, true, false, VEC, SHORT>), grid, block, 0, st, A, B, C, M, N, K, ep, bt, ANorm{});
  else LCR_LAUNCH_TIMED((k_gemm_f32<BM, BN, WM, WN, true, true, VEC, SHORT>), grid, block, 0, st, A, B, C, M, N, K, ep, bt, ANorm{});
  return check_launch(who);
}

// Scratch of the stream-K launches, one per stream (launches on one stream are ordered, so they can share it): the parked
// partial tiles (two per workgroup) and the per-tile arrival counters (left at zero by every launch).
struct SkScratch {
  float*    partial = nullptr;
  uint32_t* arrived = nullptr;
};
static std::mutex g_sk_mu;
static std::map<std::pair<int, hipStream_t>, SkScratch> g_sk_scratch;
constexpr int SK_MAX_GRID = 1024;
constexpr int SK_MAX_TILES = 8192;

static int sk_cu_count() {
  static const int n = [] {
    int dev = 0, cus = 0;
    hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return cus;
  }();
  return n;
}

// Stream-K pays when whole-tile scheduling leaves the busiest CU with >= 10 % more work than the average one.
static bool sk_worth(int64_t M, int N, int K) {
  const int cus = sk_cu_count();
  const int64_t tiles = static_cast<int64_t>(div_up(M, 64)) * div_up(N, 64);
  if (K < 480 || tiles < cus / 2 || tiles > 6 * static_cast<int64_t>(cus) || tiles > SK_MAX_TILES) return false;
  const double avg = static_cast<double>(tiles) / cus;
  const double worst = static_cast<double>((tiles + cus - 1) / cus);
  return worst / avg >= 1.10;
}

static int launch_gemm_sk(const char* who, const float* A, const float* B, float* C, int64_t M, int N, int K, const GemmEpilogue& ep, hipStream_t st) {
  const int cus = sk_cu_count();
  const int64_t iters = static_cast<int64_t>(div_up(M, 64)) * div_up(N, 64) * div_up(K, GM_BK);
  // persistent workgroups: 3, 2 or 1 per CU — as many as still get >= 24 K-steps each
  int per_cu = 3;
  while (per_cu > 1 && iters / (static_cast<int64_t>(cus) * per_cu) < 24) --per_cu;
  per_cu = env_int("LCR_SK_PER_CU", per_cu);
  int U = cus * per_cu / 8;
  if (U < 1) U = 1;
  if (8 * U > SK_MAX_GRID) U = SK_MAX_GRID / 8;
  int dev = 0;
  hipGetDevice(&dev);
  GemmStreamK sk;
  {
    std::lock_guard<std::mutex> lk(g_sk_mu);
    SkScratch& sc = g_sk_scratch[{dev, st}];
    if (!sc.partial) {
      if (hipMalloc(reinterpret_cast<void**>(&sc.partial), sizeof(float) * 2 * 16 * GM_T * SK_MAX_GRID) != hipSuccess ||
          hipMalloc(reinterpret_cast<void**>(&sc.arrived), sizeof(uint32_t) * SK_MAX_TILES) != hipSuccess)
        return refuse(LCR_EHIP, "%s: cannot allocate the stream-K scratch", who);
      hipMemsetAsync(sc.arrived, 0, sizeof(uint32_t) * SK_MAX_TILES, st);     // once: every launch leaves the counters at zero
    }
    sk.partial = sc.partial;
    sk.arrived = sc.arrived;
    sk.U = U;
  }
  LCR_LAUNCH_TIMED((k_gemm_f32_sk<64, 64, 2, 2>), dim3(8 * U), dim3(GM_T), 0, st, A, B, C, M, N, K, ep, sk);
  return check_launch(who);
}

}  // namespace lcr

using namespace lcr;

// tuning hook (tools/gemm_bench.py): 0 = heuristic, 1..5 = force a tile shape
static int g_force_tile = 0;
extern "C" void lcr_gemm_debug_force_tile(int t) { g_force_tile = t; }
// tuning / test hook: -1 = LCR_GEMM_STREAMK (default 0 = never), 0 = never, 1 = heuristic, 2 = whenever the stream-K kernel is legal
static int g_force_streamk = -1;
// tuning / test hook: -1 = LCR_GEMM_DEEP (default on), 0 = never, 1 = wherever legal
static int g_force_deep = -1;
extern "C" void lcr_gemm_debug_deep(int mode) { g_force_deep = mode; }
extern "C" void lcr_gemm_debug_streamk(int mode) { g_force_streamk = mode; }

// Which form lcr_gemm_f32 takes for a shape (vec: both leading dimensions multiples of 4 floats and 16-byte aligned bases).  lcr_gemm_f32
// dispatches on it and lcr_kpconv_mask_ok asks it; every switch is read here, once.
// LCR_GEMM_NO_SHORT set: no light form; LCR_GEMM_SHORT_K: its largest K (256); LCR_GEMM_DEEP 0: off, 1: K beyond the light form (default),
// 2: every legal K; LCR_GEMM_STREAMK 0: off (default), 1: heuristic, 2: whenever legal.
enum GemmForm { GF_SCALAR, GF_FORCED_TILE, GF_SHORT, GF_DEEP, GF_STREAMK, GF_TILE };
static GemmForm gemm_form(int64_t M, int N, int K, int transA, int transB, bool vec) {
  static const bool no_short = getenv("LCR_GEMM_NO_SHORT") != nullptr;   // A/B switch while the light form is being evaluated
  static const int short_k = env_int("LCR_GEMM_SHORT_K", 256);
  static const int deep_env = env_int("LCR_GEMM_DEEP", 1);
  static const int sk_env = env_int("LCR_GEMM_STREAMK", 0);
  if (!vec) return GF_SCALAR;
  if (g_force_tile >= 1 && g_force_tile <= 5) return GF_FORCED_TILE;
  // K-deep form (LDS-direct loads + cross-step fragment prefetch) wherever both operands are k-contiguous and K is a multiple of the K-step
  const int deep_mode = g_force_deep >= 0 ? g_force_deep : deep_env;
  const bool deep_ok = !transA && transB && K % GM_BK == 0 && !g_force_tile && M * K < (int64_t(1) << 30) && static_cast<int64_t>(N) * K < (int64_t(1) << 30);
  if (deep_mode == 2 && deep_ok) return GF_DEEP;
  if (!no_short && K <= short_k && !transA) return GF_SHORT;
  if (deep_mode && deep_ok) return GF_DEEP;
  if (N <= 32) return GF_TILE;
  // Stream-K is opt-in: measured +3 / +5 / +7 % on the three deepest KPConv contractions alone (93.6 vs 96, 121 vs 128, 153 vs
  // 164 us) — far from the 20 % a CU-count model predicts, because one or two workgroups per CU already reach 40 / 60 % of the
  // matrix-pipe rate that three reach (65 %), so an unevenly loaded CU is slower per tile but not idle pro rata.
  const int sk_mode = g_force_streamk >= 0 ? g_force_streamk : sk_env;
  const bool sk_legal = !transA && !transB && K >= 64 && static_cast<int64_t>(div_up(M, 64)) * div_up(N, 64) <= SK_MAX_TILES;
  if (sk_mode && sk_legal && (sk_mode == 2 || sk_worth(M, N, K))) return GF_STREAMK;
  return GF_TILE;
}

// Which Linears C[M,N] = A[M,K] · W[N,K]^T run on the split-bf16 form (gemm_split.hip) instead of the form gemm_form picks: the ONE rule, a
// function of (N, K) alone, that the encoder driver (encoder.hip: unary1, unary2 with or without normalise-on-load, shortcut), the module tree
// (functional.gemm_split_ok mirrors it; tests/test_gemm_split_light_gpu.py holds the two together) and bench.py's launch classification
// share.  K >= 288: the K-deep shapes, since round 5.  K <= 256 (the light fp32 form's range): the (N, K) classes where the split kernel
// measured >= 1.10x the light fp32 kernel in one job (tools/gemm_split_bench.py --light, profiles/r12_light_split.md); the others stay.
// LCR_GEMM_SPLIT_LIGHT=0: K >= 288 only (A/B).  N < 64 never: those launches stream A at the HBM rate on the fp32 form already.
// Measured classes (fp32 light us / split us, in the form the encoder launches): (512, 128) 1.21-1.25, (1024, 256) 1.40, (256, 128) 1.29,
// (512, 256) 1.39, (64, 128) 1.19, (64, 256) 1.30, (128, 256) 1.32 move; (128, 32) 1.05-1.15 and (256, 64) 1.04-1.14 miss the margin on their
// smaller-M members and stay.  A class that was not measured stays as well.
static bool gemm_split_light(int N, int K) {
  switch (K) {
    case 128: return N == 64 || N == 256 || N == 512;
    case 256: return N == 64 || N == 128 || N == 512 || N == 1024;
    default: return false;
  }
}
extern "C" int lcr_gemm_split_ok(int N, int K) {
  static const bool light = env_int("LCR_GEMM_SPLIT_LIGHT", 1) != 0;
  if (N < 64 || K < GM_BK || K % GM_BK != 0) return 0;
  return K >= 288 || (light && K <= AN_KMAX && gemm_split_light(N, K));
}

// C = leaky(GroupNorm(A)) · B^T (+ bias, + statistics of C): the light GEMM with normalise-on-load (ANorm above).  The caller
// guarantees that every segment holds at least 64 rows (a row block then touches at most two segments); shapes outside the
// light form are an argument error — the caller normalises with lcr_groupnorm_apply and calls lcr_gemm_f32 instead.
extern "C" int lcr_gemm_f32_anorm(const float* A, const float* B, float* C, int64_t M, int N, int K, const float* bias,
                                  const double* a_stats, const float* a_gamma, const float* a_beta, int a_groups, float a_eps,
                                  float a_slope, const int64_t* seg_len, int S, int groups, double* stats, void* stream) {
  if (!A || !B || !C || M < 0 || N <= 32 || K <= 0 || K > AN_KMAX || K % 4 != 0 || !a_stats || !a_gamma || !a_beta || a_groups < 1 ||
      K % a_groups != 0 || a_groups > 64 || !seg_len || S < 1 || reinterpret_cast<uintptr_t>(A) % 16 != 0 || reinterpret_cast<uintptr_t>(B) % 16 != 0)
    return refuse(LCR_EARG, "lcr_gemm_f32_anorm: needs 32 < N, K <= 256, K %% 4 == 0, a_groups dividing K, a segment table and 16-byte aligned operands");
  if (int rc = gemm_stats_domain("lcr_gemm_f32_anorm", stats, seg_len, S, groups, N)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimerScope timed(KT_GEMM, st, M, N, K);
  if (M == 0) return LCR_OK;
  GemmEpilogue ep{bias, nullptr, seg_len, S, groups, stats};
  ANorm an{a_stats, a_gamma, a_beta, a_groups, a_eps, a_slope};
  LCR_LAUNCH_TIMED((k_gemm_f32<64, 64, 2, 2, false, true, true, true, true>), dim3(gemm_grid(M, N, 64, 64)), dim3(GM_T), 0, st, A, B, C, M,
                     N, K, ep, GemmBatch{}, an);
  return check_launch("lcr_gemm_f32_anorm");
}

extern "C" int lcr_gemm_f32(const float* A, const float* B, float* C, int64_t M, int N, int K, int transA, int transB, const float* bias,
                            const float* rowdiv, const int64_t* seg_len, int S, int groups, double* stats, void* stream) {
  if (!A || !B || !C || M < 0 || N <= 0 || K <= 0) return refuse(LCR_EARG, "lcr_gemm_f32: bad argument");
  if (int rc = gemm_stats_domain("lcr_gemm_f32", stats, seg_len, S, groups, N)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimerScope timed(KT_GEMM, st, M, N, K);
  // `stats` ACCUMULATES: the caller passes a zeroed table (one fill per forward pass for all layers, instead of a fill
  // launch in front of every GEMM)
  if (M == 0) return LCR_OK;
  GemmEpilogue ep{bias, rowdiv, seg_len, S, groups, stats};
  // 16-byte vector loads need leading dimensions that are multiples of 4 floats (bases: torch allocations are >= 256-B aligned,
  // row offsets inside them are multiples of the leading dimension)
  const int64_t lda = transA ? M : K, ldb = transB ? K : N;
  const bool vec = (lda % 4 == 0) && (ldb % 4 == 0) && (reinterpret_cast<uintptr_t>(A) % 16 == 0) && (reinterpret_cast<uintptr_t>(B) % 16 == 0);
  switch (gemm_form(M, N, K, transA, transB, vec)) {
    case GF_SCALAR: return launch_gemm<128, 64, 4, 1, false>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
    case GF_FORCED_TILE:
      switch (g_force_tile) {
        case 1: return launch_gemm<128, 128, 4, 1, true>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
        case 2: return launch_gemm<128, 64, 4, 1, true>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
        case 3: return launch_gemm<128, 32, 4, 1, true>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
        case 4: return launch_gemm<64, 64, 2, 2, true>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
        default: return launch_gemm<64, 128, 2, 2, true>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
      }
    case GF_SHORT:
      if (N <= 32) return launch_gemm<128, 32, 4, 1, true, true>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
      return launch_gemm<64, 64, 2, 2, true, true>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
    case GF_DEEP: return gemm_deep_launch("lcr_gemm_f32", A, B, C, M, N, K, ep, st, nullptr, 0);
    case GF_STREAMK: return launch_gemm_sk("lcr_gemm_f32", A, B, C, M, N, K, ep, st);
    case GF_TILE: break;
  }
  // Tile choice from tools/gemm_bench.py --tiles on MI355X: 64x64 (2x2 wavefronts) wins or ties on every encoder shape with
  // N >= 64 (enough workgroups for two per CU matters more than per-tile reuse at these M); N = 32 wants the 128-row tile;
  // only large, deep problems (>= 512 tiles of 128x128 and K >= 512) pay for the big tile.
  if (N <= 32) return launch_gemm<128, 32, 4, 1, true>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
  const int64_t b128 = (M + 127) / 128, nb128 = (N + 127) / 128;
  if (K >= 512 && b128 * nb128 >= 512) return launch_gemm<128, 128, 4, 1, true>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
  return launch_gemm<64, 64, 2, 2, true>("lcr_gemm_f32", A, B, C, M, N, K, transA, transB, ep, st);
}

// Whether the contraction C[M,N] = A[M,K] . B[N,K]^T of a KPConv with C_in = K / 15 can read a row-masked aggregate and still compute what
// lcr_gemm_f32 (split = 0) / lcr_gemm_f32_bsplit (split = 1) compute on the full one: the split form always can within its offset range; the
// fp32 form only where lcr_gemm_f32 itself takes the K-deep kernel.  Environment LCR_KP_MASK=0: never (A/B).
extern "C" int lcr_kpconv_mask_ok(int64_t M, int N, int K, int split) {
  static const bool off = env_int("LCR_KP_MASK", 1) == 0;
  if (off || M <= 0 || N <= 0 || K % 15 != 0 || mask_kshift(K, K / 15) < 0) return 0;
  if (split) return M * static_cast<int64_t>(K) < (int64_t(1) << 29);
  return gemm_form(M, N, K, 0, 1, true) == GF_DEEP;      // A [M,K] and B [N,K] row-major with K % 32 == 0 (mask_kshift): the vector forms
}

// Batched C_z = A_z^T·B_z (transA) with per-entry K — NetVLAD's per-scan aggregation (NetVlad.py:68): one launch for S scans.
extern "C" int lcr_gemm_f32_batched_ta(const float* A, const float* B, float* C, int64_t M, int N, int count, const int* k_host,
                                       const int64_t* a_off_host, const int64_t* b_off_host, const int64_t* c_off_host, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || count < 1 || count > GM_MAX_BATCH || !k_host || !a_off_host || !b_off_host || !c_off_host)
    return refuse(LCR_EARG, "lcr_gemm_f32_batched_ta: bad argument (count <= %d)", GM_MAX_BATCH);
  GemmBatch bt = {};
  bt.count = count;
  for (int i = 0; i < count; ++i) {
    bt.k[i] = k_host[i];
    bt.a_off[i] = a_off_host[i];
    bt.b_off[i] = b_off_host[i];
    bt.c_off[i] = c_off_host[i];
    if (a_off_host[i] % 4 || b_off_host[i] % 4 || k_host[i] < 1) return refuse(LCR_EARG, "lcr_gemm_f32_batched_ta: offsets must be multiples of 4 floats and K >= 1");
  }
  if ((M % 4) || (N % 4)) return refuse(LCR_EARG, "lcr_gemm_f32_batched_ta: M and N must be multiples of 4");
  GemmEpilogue ep{nullptr, nullptr, nullptr, 0, 0, nullptr};
  return launch_gemm<64, 64, 2, 2, true>("lcr_gemm_f32_batched_ta", A, B, C, M, N, /*K (per entry)*/ 1, 1, 0, ep, static_cast<hipStream_t>(stream), &bt);
}

// Uniform batch: C_z[M,N] = op(A_z)·op(B_z), z < count (<= 65535), constant strides (in floats, multiples of 4) — the per-patch
// feature products of the dense matching stage (LCRNet.py:237-238: einsum('bnd,bmd->bnm')).
extern "C" int lcr_gemm_f32_strided_batched(const float* A, const float* B, float* C, int64_t M, int N, int K, int transA, int transB,
                                            int64_t strideA, int64_t strideB, int64_t strideC, int count, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || count < 1 || count > 65535 || (strideA % 4) || (strideB % 4))
    return refuse(LCR_EARG, "lcr_gemm_f32_strided_batched: bad argument");
  const int64_t lda = transA ? M : K, ldb = transB ? K : N;
  if ((lda % 4) || (ldb % 4)) return refuse(LCR_EARG, "lcr_gemm_f32_strided_batched: leading dimensions must be multiples of 4");
  GemmBatch bt = {};
  bt.count = count;
  bt.strided = 1;
  bt.k[0] = K;
  bt.a_off[0] = strideA;
  bt.b_off[0] = strideB;
  bt.c_off[0] = strideC;
  GemmEpilogue ep{nullptr, nullptr, nullptr, 0, 0, nullptr};
  // K <= 256 (the 128 x 128 x 256 patch products: thousands of two-by-two-tile problems of eight K-steps each): the light form — one
  // register stage, six to eight workgroups per CU — like the un-batched Linears of that depth (LCR_GEMM_BATCH_SHORT=0: the deep-pipeline form)
  // LCR_GEMM_BATCH_TILE=128: ONE 128 x 128 tile per problem instead of four 64 x 64 ones for the 128 x 128 x 256 patch products.  Looked like
  // +4 % pairs/s across two gpurun sessions (590 -> 616), is -3 % in a same-session A/B (648 / 644 vs 632 / 623 pairs/s at 16 pairs per call) and
  // 1.29 vs 0.96 ms per call alone: off by default, kept as the switch that measured it
  static const int batch_tile = env_int("LCR_GEMM_BATCH_TILE", 64);
  if (batch_tile == 128 && M >= 128 && N >= 128) return launch_gemm<128, 128, 4, 1, true>("lcr_gemm_f32_strided_batched", A, B, C, M, N, K, transA, transB, ep, static_cast<hipStream_t>(stream), &bt);
  static const bool batch_short = env_int("LCR_GEMM_BATCH_SHORT", 1) != 0;
  if (batch_short && K <= 256 && !transA) return launch_gemm<64, 64, 2, 2, true, true>("lcr_gemm_f32_strided_batched", A, B, C, M, N, K, transA, transB, ep, static_cast<hipStream_t>(stream), &bt);
  return launch_gemm<64, 64, 2, 2, true>("lcr_gemm_f32_strided_batched", A, B, C, M, N, K, transA, transB, ep, static_cast<hipStream_t>(stream), &bt);
}
