// gemm_split.hip — the split-bf16 form of the K-deep fp32 GEMM: the operand splitters, the kernel and their entry points.
#include <type_traits>

#include "gemm.h"

namespace lcr {

// ---- split-bf16 form of the K-deep contractions: fp32 operands as three bf16 terms, six cross products on the bf16 matrix cores ----
// The K-deep fp32 form above is bound by the matrix pipe (mfma_busy 0.82) on an instruction that runs at 1/16 of the bf16 rate
// (v_mfma_f32_32x32x2_f32: 64 cycles for 4 096 flop; v_mfma_f32_32x32x16_bf16: 32 cycles for 32 768).  An fp32 number is EXACTLY the sum
// of three bf16 numbers (8 + 8 + 8 significand bits: h1 = rn(x), h2 = rn(x - h1), h3 = rn(x - h1 - h2); both subtractions are exact in
// fp32), so a·b = Σ_{i,j} a_i b_j over nine exact bf16 x bf16 products.  Kept: the six with i + j <= 4 (a1b1; a1b2, a2b1; a1b3, a2b2,
// a3b1); dropped: a2b3, a3b2 (each <= 2^-24 |ab|) and a3b3 (2^-32): a product is carried to <= 2^-23 relative, accumulation in fp32 inside the
// MFMA — six K=16 instructions (192 cycles) replace eight fp32 ones (512) per 32 x 32 x 16 block.
//   * B (weights, constant) arrives pre-split, once per weight, in the order the MFMA reads it (lcr_split_bf16x3_tiles) and goes from
//     global memory straight into the MFMA's registers: it never crosses LDS;
//   * A (activations) is split ONCE PER WORKGROUP on its way from registers to LDS (8 values per thread and K-step: 44 VALU), not per
//     wavefront at the fragment read; planes are row-major bf16 tiles, 64-B rows with XOR-ed 16-B chunks (k_gemm_f32_bsplit_p);
//   * A's LDS double-buffered, loads two tiles ahead in registers: one barrier per K-step.
// Results are NOT bit-identical to the fp32 form (different rounding points); tests/test_gemm_split_gpu.py holds both against fp64.
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));     // plain vector type: arrays of HIP's uint4 struct did not leave scratch memory

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {           // v_cvt_pk_bf16_f32 (round to nearest even): a -> low half
  f32x2_t v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
// two fp32 values -> their three bf16 terms (packed pairs)
__device__ __forceinline__ void split2(float x0, float x1, uint32_t& h1, uint32_t& h2, uint32_t& h3) {
  h1 = pk_bf16(x0, x1);
  const float r0 = fsub(x0, __uint_as_float(h1 << 16)), r1 = fsub(x1, __uint_as_float(h1 & 0xffff0000u));     // exact
  h2 = pk_bf16(r0, r1);
  const float s0 = fsub(r0, __uint_as_float(h2 << 16)), s1 = fsub(r1, __uint_as_float(h2 & 0xffff0000u));     // exact
  h3 = pk_bf16(s0, s1);
}

__global__ __launch_bounds__(256) void k_split_bf16x3(const float* __restrict__ w, int64_t n, uint16_t* __restrict__ planes) {
  for (int64_t i = (blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x) * 2; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x * 2) {
    const float x0 = w[i], x1 = i + 1 < n ? w[i + 1] : 0.f;
    uint32_t h1, h2, h3;
    split2(x0, x1, h1, h2, h3);
    planes[i] = static_cast<uint16_t>(h1), planes[n + i] = static_cast<uint16_t>(h2), planes[2 * n + i] = static_cast<uint16_t>(h3);
    if (i + 1 < n) planes[i + 1] = static_cast<uint16_t>(h1 >> 16), planes[n + i + 1] = static_cast<uint16_t>(h2 >> 16), planes[2 * n + i + 1] = static_cast<uint16_t>(h3 >> 16);
  }
}

// The planes of a constant operand in the layout the GEMM stages them in: for every (64-column tile ct, K-step ks of 32) one contiguous
// 12 KB block, its 16-B chunks (8 bf16 of one plane, column and 8-k group) in the order the MFMA's B operand is read:
// [column quarter wn 0..3][plane 0..2][lane 0..63], lane l holding column 64 ct + 16 wn + (l & 15), k 32 ks + 8 (l >> 4) .. + 7 (v_mfma_f32_16x16x32_bf16).
// A wavefront's B fragment is then ONE 16-B load per lane, 1 KB contiguous per instruction (full 128-B lines), straight into the MFMA's registers.
// Rows beyond N are zero.  One thread per chunk of a plane (thread q = 64 wn + lane: every wavefront stores contiguous KBs).
__global__ __launch_bounds__(256) void k_split_bf16x3_tiles(const float* __restrict__ w, int N, int K, uint16_t* __restrict__ tiles) {
  const int KS = K / GM_BK;
  const int64_t blk = blockIdx.x;                               // ct * KS + ks
  const int ct = static_cast<int>(blk / KS), ks = static_cast<int>(blk % KS);
  const int fl = threadIdx.x & 63, wn = threadIdx.x >> 6;
  const int row = wn * 16 + (fl & 15), kc = fl >> 4;
  const int n = ct * 64 + row;
  u32x4_t p1 = {0u, 0u, 0u, 0u}, p2 = p1, p3 = p1;
  if (n < N) {
    const float* src = w + static_cast<int64_t>(n) * K + ks * GM_BK + kc * 8;
    const float4 x0 = ld4(src), x1 = ld4(src + 4);
    uint32_t h1, h2, h3;
    split2(x0.x, x0.y, h1, h2, h3), p1.x = h1, p2.x = h2, p3.x = h3;
    split2(x0.z, x0.w, h1, h2, h3), p1.y = h1, p2.y = h2, p3.y = h3;
    split2(x1.x, x1.y, h1, h2, h3), p1.z = h1, p2.z = h2, p3.z = h3;
    split2(x1.z, x1.w, h1, h2, h3), p1.w = h1, p2.w = h2, p3.w = h3;
  }
  char* dst = reinterpret_cast<char*>(tiles) + blk * 12288 + wn * 3072 + fl * 16;
  *reinterpret_cast<u32x4_t*>(dst) = p1;
  *reinterpret_cast<u32x4_t*>(dst + 1024) = p2;
  *reinterpret_cast<u32x4_t*>(dst + 2048) = p3;
}

// 64 x 64 tile, FOUR wavefronts of 64 rows x 16 columns on v_mfma_f32_16x16x32_bf16 (the stage-3/4 contractions are 200-600 such tiles on 256
// CUs).  Only A's planes are in LDS, DOUBLE-buffered: the split + plane writes of tile t+1 run under the MFMAs of tile t and a K-step has ONE
// barrier; A's tiles t+1 and t+2 in flight / parked in two register stages; B's fragments of tiles t and t+1 in registers, each 16-B chunk
// fetched once per workgroup; every load instruction fetches full 128-B lines (A: 8 lanes per row; B: 1 KB contiguous per instruction).
// LDS cycles per 64 x 64 x 32 step of a workgroup (MI355X: ds_read_b128 4, ds_write_b64 ~6, ds_write_b128 ~13; derived, not measured):
//   2 x 2 wavefronts of 32 x 32, both operands through LDS (the form before): 48 reads + 24 A stores + 12 B stores = 192 + 144 + 156 = 492;
//   this form: 48 reads + 24 A stores = 192 + 144 = 336; the matrix pipe needs 384 per SIMD either way (24 x 16 against 12 x 32).
// LDS per workgroup 48.5 -> 26 KB, 114 VGPRs (118 masked): four workgroups per CU instead of three.  Measured (tools/gemm_split_bench.py
// --table, both forms in one run on one GPU, profiles/r08_split_gemm_fragments.md): 646 -> 583 us over the 13 bench shapes (-10 %), every
// encoder shape faster: 2_2 54.6 -> 48.5, 3_1 29.0 -> 26.6, 3_2 74.7 -> 67.9, 4_2 99.3 -> 87.6, 4_x unary1 31.6 -> 28.9, 4_2 short 53.5 -> 48.2,
// square 120.2 -> 107.0 (161 TFLOP/s-equivalent); 4_1 (204 tiles) unchanged at 34.  The K = 32 instruction adds the products of a K-step in
// another order than two K = 16 ones: results differ from the earlier form's in the last bits (same error against fp64).
// The form tried first — TWO wavefronts of 64 x 32 on the 32 x 32 x 16 instruction (bit-identical sums, LDS path 240 cycles, 24 MFMAs per 12
// fragment reads): 168 VGPRs with one A register stage at three wavefronts per SIMD, or 194 with two stages at two — 705 / 689 us against 628
// in its run: faster only where the grid fills the chip several times (2_2 53.4 -> 50.4, 4_2 short 52.3 -> 50.1, square 114.8 -> 104.4 at
// two per SIMD), much slower on the few-tile shapes (3_1 28.1 -> 40.3, 4_1 33.1 -> 48.5, 4_2 96.1 -> 127.6): 200-400 workgroups of two
// wavefronts leave half of a CU's four SIMDs without a wavefront, and each wavefront's step is twice as long.  Tile COUNT is not the
// invariant to keep on these shapes; wavefronts per CU is.
// What was measured on the way to the earlier form (LABNOTES.md §4.4), each against the fp32 K-deep kernel over the 13 bench shapes:
// single-buffered LDS with two barriers per step 1.00x; larger tiles (128 x 64, 128 x 128 on 4 wavefronts; 128 x 64 on 8) lose on the encoder's
// shapes (too few tiles) and win on 8192 x 1024 x 1024 (1.45x); A straight from global memory into fragment registers 0.92x; four register
// stages: no change; 80-byte padded LDS rows: a third of the LDS cycles were bank conflicts of the 16-B WRITES (SQ_LDS_BANK_CONFLICT) — the XOR
// layout: 1.07x -> 1.17x; two alternating accumulators: same speed, half the error; producer / consumer wavefronts (512 threads): same time;
// ablations (LCR_SPLIT_ABL): loads alone 75 us and MFMAs alone 47 us of 4_2's 98 — the loads were bound by LINE REQUESTS (every A line asked
// for twice, B rows half lines): full-line loads + tiled planes: loads alone 53 us — and the whole kernel still 100: every ablation removed
// its own 10-25 %, i.e. the K-step is a latency chain (arrival -> split -> park -> barrier -> fragment reads -> MFMAs); matrix pipe 38 % busy.
// Raising the wavefront's priority over its MFMA section (s_setprio) 0.98x, parking the next tile before the MFMAs instead of between them 1.00x;
// B planes global -> LDS directly (global_load_lds_dwordx4, three B stages): 0.89x (60 KB of LDS: two workgroups per CU).  A 64 x 128 form
// (wavefront = 32 x 64): 160 TFLOP/s-equivalent on 8192 x 1024 x 1024 against 146 but 0.93x over the 13 shapes (4_2 is 204 such tiles) — removed.
// ABL: timing ablations (LCR_SPLIT_ABL): 1 no MFMAs, 2 no split arithmetic, 4 no A plane stores, 8 no global loads in the loop, 16 no A
// fragment reads, 32 no B fragment loads in the loop.  0 = the product; any other value computes garbage.
// MASK: row-masked A as in k_gemm_f32_deep.  The A pieces are then buffer loads whose offset is pushed out of the buffer's range for a
// block that was never stored: the range check returns zeros without a memory access (and without a branch in the K-step).
// ANORM: normalise-on-load as in k_gemm_f32 (ANorm, gemm.h), for the K <= AN_KMAX Linears that follow a KPConv (unary2): a piece of A becomes
// y = leaky(fmaf(x, scale[k], shift[k])) with the (scale, shift) of its row's segment slot BEFORE it is split, on its way from registers to
// LDS — the same operations in the same order as LoaderT::store_norm, so both GEMM forms see bit-equal normalised operands, and the table
// is the one anorm_build_table (gemm.h) makes for both.  Per thread and K-step: 4 more LDS reads (16 B) and 16 more VALU under the MFMAs;
// +5 KB of LDS (table + (mean, rstd)): 31 KB.  Left to itself the form takes 132 VGPRs (three workgroups per CU); bounded to four per SIMD it
// takes 128 and spills five registers (20 bytes) that live only outside the K loop — stored before it, reloaded after it.  Measured
// (tools/gemm_split_bench.py --light, profiles/r12_light_split.md): 1.21-1.40x lcr_gemm_f32_anorm at K = 128 / 256.  The prologue (tiles 0
// and 1 requested, tile 0 parked, tile 2 requested) clamps every tile index to nk - 1, so nk = 1 and 2 (K = 32, 64) re-request the last tile
// (cache hits, parked into the idle LDS stage, never read): correct for every nk >= 1, and the table index is clamped the same way.
template <int ABL, bool MASK = false, bool ANORM = false>
__global__ __launch_bounds__(256, ANORM ? 4 : 3) void k_gemm_f32_bsplit_p(const float* __restrict__ A, const uint16_t* __restrict__ Bs, float* __restrict__ C,
                                                           int64_t M, int N, int K, GemmEpilogue ep, const uint16_t* __restrict__ amask,
                                                           int kshift, ANorm an) {
  static_assert(!(ANORM && MASK), "normalise-on-load reads a dense A");
  // LDS plane tile of A: 64 rows x 64 B (32 bf16), no padding; the four 16-B chunks of row r are XOR-ed with (r >> 2) & 3.  A ds_read_b128 is
  // serviced in groups of 16 lanes over 64 banks (16 different rows, one logical chunk: rows r, r+4, r+8, r+12 share a 64-B bank quadrant
  // and get four different chunks).
  // (The 80-byte padded rows of the first version were conflict-free for the reads only: SQ_LDS_BANK_CONFLICT = a third of SQ_LDS_IDX_ACTIVE.)
  constexpr int BM = 64, BN = 64, RS = 64, T = 256, PLA = BM * RS, STGA = 3 * PLA, D = 2;
  __shared__ __attribute__((aligned(16))) char sA[2 * STGA];
  const int lane = threadIdx.x & 63, wn = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // the wavefront: 64 rows x columns [16 wn, + 16)
  const int ntn = (N + BN - 1) / BN;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int64_t m_tile = static_cast<int64_t>(slot / ntn) * 8 + xcd;
  const int64_t m0 = m_tile * BM;
  const int n0 = (slot % ntn) * BN;
  if (m0 >= M) return;
  // A staging: the tile is 64 rows x eight 16-B pieces; thread t takes pieces t and t + T, i.e. (row t >> 3 (+ 32), piece t & 7): the 8 lanes
  // of a row fetch one full 128-B line per load instruction (with 4 lanes x two strided 16-B pieces per row, every line was requested twice,
  // and the kernel was bound by line requests: see the ablations).  A piece = 4 floats -> 8 bytes per plane (ds_write_b64).
  const int srow = threadIdx.x >> 3, spc = threadIdx.x & 7;
  const float* ap[2];
  int soff[2];
  uint32_t aoff[2], rmask[2];                                  // MASK: byte offset of the piece in A (the launcher guarantees M*K*4 < 2^31), row mask
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = srow + j * (T / 8);
    int64_t ga = m0 + r;
    ga = ga < M ? ga : M - 1;                                  // duplicate rows only feed outputs that are never stored
    ap[j] = A + ga * K + spc * 4;
    if constexpr (MASK) {
      aoff[j] = static_cast<uint32_t>((ga * K + spc * 4) * 4);
      rmask[j] = amask[ga];
    } else {
      aoff[j] = rmask[j] = 0;
    }
    soff[j] = r * RS + (((spc >> 1) ^ ((r >> 2) & 3)) << 4) + (spc & 1) * 8;
  }
  // B: the wavefront's quarter (wn) of the step's 12 KB block of the fragment-ordered planes: plane p is the 1 KB at 1024 p, lane l its bytes
  // [16 l, + 16).  Nothing is staged: the registers the load fills are the MFMA's B operand, and every B byte is fetched once per workgroup.
  const char* bp = reinterpret_cast<const char*>(Bs) + static_cast<int64_t>(n0 / 64) * (K / GM_BK) * 12288 + wn * 3072 + lane * 16;
  // A fragment of row block b (16 rows): lane l reads row 16 b + (l & 15), logical chunk l >> 4 (k 8 (l >> 4) .. + 7); 16 rows on have the same swizzle
  const int fa = (lane & 15) * RS + (((lane >> 4) ^ (((lane & 15) >> 2) & 3)) << 4);
  f32x4_t acc[4], acc2[4];                                     // per 16-row block two accumulators, alternating: half the error of one
#pragma unroll
  for (int b = 0; b < 4; ++b) acc[b] = acc2[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nk = K / GM_BK;
  f32x4_t ra[D][2];                                            // A: tiles t+1, t+2 in flight / parked (two pieces each)
  u32x4_t rb[2][3];                                            // B: the three planes' fragments of tile t (stage t & 1) and of tile t+1
  __amdgpu_buffer_rsrc_t arsrc;
  if constexpr (MASK) arsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A), 0, static_cast<int>(M * K * 4), 0x00020000);
  auto fetch_a = [&](auto st_c, int t) {
    constexpr int st = decltype(st_c)::value;
    const int tt = t < nk ? t : nk - 1;                         // the tail re-reads the last tile
    if constexpr (MASK) {
      const int kb = tt >> kshift;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint32_t o = ((rmask[j] >> kb) & 1u) ? aoff[j] + static_cast<uint32_t>(tt * GM_BK * 4) : 0x80000000u;
        ra[st][j] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(arsrc, static_cast<int>(o), 0, 0));
      }
    } else {
      ra[st][0] = *reinterpret_cast<const f32x4_t*>(ap[0] + tt * GM_BK), ra[st][1] = *reinterpret_cast<const f32x4_t*>(ap[1] + tt * GM_BK);
    }
  };
  auto fetch_b = [&](auto st_c, int t) {
    constexpr int st = decltype(st_c)::value;
    const int tt = t < nk ? t : nk - 1;
#pragma unroll
    for (int p = 0; p < 3; ++p) rb[st][p] = *reinterpret_cast<const u32x4_t*>(bp + static_cast<int64_t>(tt) * 12288 + p * 1024);
  };
  __shared__ __attribute__((aligned(16))) float s_an[ANORM ? 4 * AN_KMAX : 4];   // [slot][scale | shift][k]
  int toff[2] = {0, 0};                                        // ANORM: this thread's piece j in the table of its row's slot, at k = 0
  auto park = [&](auto st_c, int lds_stage, int t) {           // A register stage (tile t) -> [normalise] -> split -> LDS stage
    constexpr int st = decltype(st_c)::value;
    char* da = sA + lds_stage * STGA;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      uint32_t h1, h2, h3, g1, g2, g3;
      if constexpr (ANORM) {
        const float* tb = s_an + toff[j] + (t < nk ? t : nk - 1) * GM_BK;        // the tile fetch_a loaded
        const float4 sc = *reinterpret_cast<const float4*>(tb), sh = *reinterpret_cast<const float4*>(tb + AN_KMAX);
        f32x4_t v = ra[st][j];
        v.x = fmaf(v.x, sc.x, sh.x), v.y = fmaf(v.y, sc.y, sh.y), v.z = fmaf(v.z, sc.z, sh.z), v.w = fmaf(v.w, sc.w, sh.w);
        v.x = v.x > 0.f ? v.x : v.x * an.slope, v.y = v.y > 0.f ? v.y : v.y * an.slope;
        v.z = v.z > 0.f ? v.z : v.z * an.slope, v.w = v.w > 0.f ? v.w : v.w * an.slope;
        ra[st][j] = v;
      }
      if constexpr (ABL & 2) {
        h1 = __float_as_uint(ra[st][j].x), h2 = __float_as_uint(ra[st][j].y), h3 = h1, g1 = __float_as_uint(ra[st][j].z), g2 = __float_as_uint(ra[st][j].w), g3 = g1;
      } else {
        split2(ra[st][j].x, ra[st][j].y, h1, h2, h3);
        split2(ra[st][j].z, ra[st][j].w, g1, g2, g3);
      }
      if constexpr (ABL & 4) {
        asm volatile("" ::"v"(h1), "v"(h2), "v"(h3), "v"(g1), "v"(g2), "v"(g3));
      } else {
        *reinterpret_cast<uint2*>(da + soff[j]) = make_uint2(h1, g1);
        *reinterpret_cast<uint2*>(da + PLA + soff[j]) = make_uint2(h2, g2);
        *reinterpret_cast<uint2*>(da + 2 * PLA + soff[j]) = make_uint2(h3, g3);
      }
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  // A register stage of tile t is t & 1, as are its LDS stage and the B register stage.  The prologue issues its loads in the order the steps
  // do (A two tiles ahead, then B one tile ahead): the s_waitcnt counts at the loop's head are the minimum over both ways into it.
  float bias_v[1];
  {
    const int col = n0 + (wn & 1) * 32 + (lane & 31);           // the epilogue's 2 x 2 arrangement of 32 x 32 blocks (below)
    bias_v[0] = (ep.bias && col < N) ? ep.bias[col] : 0.f;
  }
  fetch_a(I0{}, 0);
  fetch_a(I1{}, 1);
  fetch_b(I0{}, 0);
  float an_g[2], an_b[2];
  if constexpr (ANORM) anorm_load_affine(an, K, an_g, an_b);
  int blk_first = 0;
  int64_t blk_seg_start = 0, blk_seg_end = 0;
  if (ep.stats != nullptr || ANORM) {
    blk_seg_end = ep.seg_len[0];
    while (blk_first + 1 < ep.S && m0 >= blk_seg_end) {
      ++blk_first;
      blk_seg_start = blk_seg_end;
      blk_seg_end += ep.seg_len[blk_first];
    }
  }
  if constexpr (ANORM) {
    const int an_split = static_cast<int>(min(static_cast<int64_t>(BM), blk_seg_end - m0));   // rows >= an_split: the next segment (slot 1)
#pragma unroll
    for (int j = 0; j < 2; ++j) toff[j] = (srow + j * (T / 8) >= an_split ? 2 * AN_KMAX : 0) + spc * 4;
    anorm_build_table(an, ep, K, blk_first, an_g, an_b, s_an);
  }
  park(I0{}, 0, 0);
  fetch_a(I0{}, 2);
  fetch_b(I1{}, 1);
  __syncthreads();
  // step t: LDS stage t & 1 holds A's tile t and B register stage t & 1 its B fragments; A's tile t+1 (register stage (t+1) & 1) is split into
  // the other LDS stage under this step's MFMAs, its registers then take tile t+3; the B registers take tile t+2 after the step's last MFMA
  auto step = [&](auto lds_c, int t) {
    constexpr int P = decltype(lds_c)::value;                  // t & 1
    using NX = std::integral_constant<int, P ^ 1>;
    const char* la = sA + P * STGA + fa;
    bf16x8_t a[4][3];                                           // [16-row block][plane]
    auto mm = [&](const bf16x8_t& x, const u32x4_t& y, f32x4_t& c) {
      if constexpr (ABL & 1) {
        asm volatile("" ::"v"(x), "v"(y));                        // operands stay live (their loads are not dead), no matrix instruction
      } else {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, __builtin_bit_cast(bf16x8_t, y), c, 0, 0, 0);
      }
    };
    if constexpr (ABL & 16) {
      u32x4_t z = {static_cast<uint32_t>(t), 0u, 0u, 0u};
      asm volatile("" : "+v"(z));
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int p = 0; p < 3; ++p) a[b][p] = __builtin_bit_cast(bf16x8_t, z);
      (void)la;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int p = 0; p < 3; ++p) a[b][p] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(la + p * PLA + b * (16 * RS)));
    }
    const u32x4_t &b0 = rb[P][0], &b1 = rb[P][1], &b2 = rb[P][2];
    auto six = [&](int b) {                                    // the six kept products of one 16-row block, small terms first
      mm(a[b][2], b0, acc[b]);
      mm(a[b][0], b2, acc2[b]);
      mm(a[b][1], b1, acc[b]);
      mm(a[b][1], b0, acc2[b]);
      mm(a[b][0], b1, acc[b]);
      mm(a[b][0], b0, acc2[b]);
    };
    six(0), six(1);
    park(NX{}, P ^ 1, t + 1);                                       // tile t+1 -> the other LDS stage (its last readers passed the barrier of step t-1)
    six(2), six(3);
    if constexpr (!(ABL & 8)) fetch_a(NX{}, t + 3);
    if constexpr (!(ABL & (8 | 32))) fetch_b(lds_c, t + 2);
    __syncthreads();
  };
  int t = 0;
  for (; t + 2 <= nk; t += 2) {
    step(I0{}, t);
    step(I1{}, t + 1);
  }
  if (t < nk) step(I0{}, t);
  // The epilogue is written for 2 x 2 wavefronts of 32 x 32 blocks: hand the tile over through LDS (the A stages are free after the last
  // step's barrier; 65-float rows).  Once per workgroup: 16 + 16 LDS accesses per lane against 36 per K-step.
  float* sC = reinterpret_cast<float*>(sA);
  static_assert(64 * 65 * 4 <= 2 * STGA, "the output tile fits the A stages");
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) sC[(16 * b + 4 * (lane >> 4) + r) * 65 + 16 * wn + (lane & 15)] = acc[b][r] + acc2[b][r];
  __syncthreads();
  const int wm2 = wn >> 1, wn2 = wn & 1;
  floatx16 accs[1];
#pragma unroll
  for (int r = 0; r < 16; ++r) accs[0][r] = sC[(32 * wm2 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 65 + 32 * wn2 + (lane & 31)];
  gemm_epilogue<BM, BN, 2, 2, 1>(accs, C, M, N, m0, n0, m_tile, ep, bias_v, blk_first, blk_seg_start, blk_seg_end, wm2, wn2, lane);
}

}  // namespace lcr

using namespace lcr;

// fp32 array -> its three bf16 terms, planes [3][n] (bf16 bit patterns); once per constant operand (weights)
extern "C" int lcr_split_bf16x3(const float* w, int64_t n, uint16_t* planes, void* stream) {
  if (!w || !planes || n < 0) return refuse(LCR_EARG, "lcr_split_bf16x3: bad argument");
  if (n == 0) return LCR_OK;
  hipLaunchKernelGGL(k_split_bf16x3, dim3(min(div_up(n, 512), 2048)), dim3(256), 0, static_cast<hipStream_t>(stream), w, n, planes);
  return check_launch("lcr_split_bf16x3");
}

// weights [N,K] (K % 32 == 0) -> the tiled planes lcr_gemm_f32_bsplit takes: u16[ceil(N/64)][K/32][3][64][32] (12 KB per block)
extern "C" int lcr_split_bf16x3_tiles(const float* w, int N, int K, uint16_t* tiles, void* stream) {
  if (!w || !tiles || N < 1 || K < GM_BK || K % GM_BK != 0 || reinterpret_cast<uintptr_t>(w) % 16 != 0 || reinterpret_cast<uintptr_t>(tiles) % 16 != 0)
    return refuse(LCR_EARG, "lcr_split_bf16x3_tiles: needs K %% 32 == 0 and 16-byte aligned buffers");
  hipLaunchKernelGGL(k_split_bf16x3_tiles, dim3(div_up(N, 64) * (K / GM_BK)), dim3(256), 0, static_cast<hipStream_t>(stream), w, N, K, tiles);
  return check_launch("lcr_split_bf16x3_tiles");
}

// C = A[M,K] · B[N,K]^T with B given as the TILED bf16 planes of lcr_split_bf16x3_tiles; epilogue as lcr_gemm_f32.
// The body of lcr_gemm_f32_bsplit and lcr_gemm_f32_bsplit_masked; `who` = the one that was called.
static int bsplit_impl(const char* who, const float* A, const uint16_t* Bs, float* C, int64_t M, int N, int K, const float* bias, const float* rowdiv,
                       const int64_t* seg_len, int S, int groups, double* stats, const uint16_t* amask, int kshift, void* stream) {
  if (!A || !Bs || !C || M < 0 || N <= 0 || K <= 0 || K % GM_BK != 0 || reinterpret_cast<uintptr_t>(A) % 16 != 0 || reinterpret_cast<uintptr_t>(Bs) % 16 != 0 ||
      K < GM_BK)
    return refuse(LCR_EARG, "%s: needs K %% 32 == 0 and 16-byte aligned operands", who);
  if (int rc = gemm_stats_domain(who, stats, seg_len, S, groups, N)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimerScope timed(KT_GEMM, st, M, N, K);
  if (M == 0) return LCR_OK;
  GemmEpilogue ep{bias, rowdiv, seg_len, S, groups, stats};
  static const int abl = env_int("LCR_SPLIT_ABL", 0);      // timing ablations only (garbage results)
  const dim3 grid(gemm_grid(M, N, 64, 64)), block(256);
  if (amask) {
    LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<0, true>), grid, block, 0, st, A, Bs, C, M, N, K, ep, amask, kshift, ANorm{});
    return check_launch(who);
  }
  switch (abl) {
    case 1: LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<1>), grid, block, 0, st, A, Bs, C, M, N, K, ep, amask, kshift, ANorm{}); break;
    case 2: LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<2>), grid, block, 0, st, A, Bs, C, M, N, K, ep, amask, kshift, ANorm{}); break;
    case 4: LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<4>), grid, block, 0, st, A, Bs, C, M, N, K, ep, amask, kshift, ANorm{}); break;
    case 8: LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<8>), grid, block, 0, st, A, Bs, C, M, N, K, ep, amask, kshift, ANorm{}); break;
    case 16: LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<16>), grid, block, 0, st, A, Bs, C, M, N, K, ep, amask, kshift, ANorm{}); break;
    case 23: LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<23>), grid, block, 0, st, A, Bs, C, M, N, K, ep, amask, kshift, ANorm{}); break;
    case 30: LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<30>), grid, block, 0, st, A, Bs, C, M, N, K, ep, amask, kshift, ANorm{}); break;
    case 32: LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<32>), grid, block, 0, st, A, Bs, C, M, N, K, ep, amask, kshift, ANorm{}); break;
    default: LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<0>), grid, block, 0, st, A, Bs, C, M, N, K, ep, amask, kshift, ANorm{}); break;
  }
  return check_launch(who);
}

extern "C" int lcr_gemm_f32_bsplit(const float* A, const uint16_t* Bs, float* C, int64_t M, int N, int K, const float* bias, const float* rowdiv,
                                   const int64_t* seg_len, int S, int groups, double* stats, void* stream) {
  return bsplit_impl("lcr_gemm_f32_bsplit", A, Bs, C, M, N, K, bias, rowdiv, seg_len, S, groups, stats, nullptr, 0, stream);
}

// C = leaky(GroupNorm(A)) · B^T (+ bias, + statistics of C) on the split form: lcr_gemm_f32_anorm's arguments with the tiled planes in place of
// the weight, and its domain (K <= 256, every segment >= 64 rows by the caller's guarantee) narrowed to the split kernel's K % 32 == 0, N >= 64.
extern "C" int lcr_gemm_f32_bsplit_anorm(const float* A, const uint16_t* Bs, float* C, int64_t M, int N, int K, const float* bias,
                                         const double* a_stats, const float* a_gamma, const float* a_beta, int a_groups, float a_eps,
                                         float a_slope, const int64_t* seg_len, int S, int groups, double* stats, void* stream) {
  if (!A || !Bs || !C || M < 0 || N < 64 || K < GM_BK || K > AN_KMAX || K % GM_BK != 0 || !a_stats || !a_gamma || !a_beta || a_groups < 1 ||
      K % a_groups != 0 || a_groups > 64 || !seg_len || S < 1 || reinterpret_cast<uintptr_t>(A) % 16 != 0 || reinterpret_cast<uintptr_t>(Bs) % 16 != 0)
    return refuse(LCR_EARG, "lcr_gemm_f32_bsplit_anorm: needs N >= 64, K <= 256, K %% 32 == 0, a_groups (<= 64) dividing K, a segment table and 16-byte aligned operands");
  if (int rc = gemm_stats_domain("lcr_gemm_f32_bsplit_anorm", stats, seg_len, S, groups, N)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  KernelTimerScope timed(KT_GEMM, st, M, N, K);
  if (M == 0) return LCR_OK;
  GemmEpilogue ep{bias, nullptr, seg_len, S, groups, stats};
  ANorm an{a_stats, a_gamma, a_beta, a_groups, a_eps, a_slope};
  LCR_LAUNCH_TIMED((k_gemm_f32_bsplit_p<0, false, true>), dim3(gemm_grid(M, N, 64, 64)), dim3(256), 0, st, A, Bs, C, M, N, K, ep,
                   static_cast<const uint16_t*>(nullptr), 0, an);
  return check_launch("lcr_gemm_f32_bsplit_anorm");
}

extern "C" int lcr_gemm_f32_bsplit_masked(const float* A, const uint16_t* Bs, float* C, int64_t M, int N, int K, const float* bias,
                                          const float* rowdiv, const int64_t* seg_len, int S, int groups, double* stats, const uint16_t* row_mask,
                                          int block_k, void* stream) {
  const int ks = mask_kshift(K, block_k);
  if (!row_mask || ks < 0 || M * static_cast<int64_t>(K) >= (int64_t(1) << 29))
    return refuse(LCR_EARG, "lcr_gemm_f32_bsplit_masked: needs a row mask, block_k = 32 << s (s <= 3) with K <= 16 block_k, and M*K < 2^29");
  return bsplit_impl("lcr_gemm_f32_bsplit_masked", A, Bs, C, M, N, K, bias, rowdiv, seg_len, S, groups, stats, row_mask, ks, stream);
}
