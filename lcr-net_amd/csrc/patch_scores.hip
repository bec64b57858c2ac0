// patch_scores.hip — a-10, dense point matching: the patch score matrices of DenseMatchingHEAD (model_family/LCRNet.py:236-250) in ONE kernel.
//
// The reference gathers the K = 128 point features of every matched patch on both sides (index_select on the zero-padded feature
// tensor, :236-239), multiplies them (einsum 'bnd,bmd->bnm', :247), scales by 1/sqrt(C) (:248) and hands the (P,128,128) products to
// LearnableLogOptimalTransport, which pads them with the dustbin row / column alpha and masks invalid rows / columns to -inf
// (learnable_sinkhorn.py:38-49).  As separate launches that is two gathers writing 2 x P x 128 x C floats (1 GB each for a 16-pair call),
// a batched product reading them back, and a pass over the (P,129,129) scores.  Here one workgroup per patch pair gathers the rows
// straight from the point-feature tensor into LDS (a patch's 128 rows are re-used by neighbouring patches: L2 hits), multiplies on
// v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate, k ascending: the arithmetic of lcr_gemm_f32) and writes the PADDED, MASKED, SCALED
// score matrix the transport kernel starts from.  The gathered feature copies never exist.
//
//   tile: 128 x 128 outputs per workgroup, 4 wavefronts x (64 x 64 = 2 x 2 MFMA tiles), K-steps of 32 channels, k-major LDS tiles
//   (stride 130 floats: the transposing 4-B stores of a wavefront — 8 rows x 8 channel quads — hit 64 different banks), double-buffered,
//   the next step's 16-B gathers in flight under the 64 MFMAs of the current one; 8 consecutive lanes fetch one row's full 128-B line.
//
// Second half of the file: the reverse pass to the two feature tensors (lcr_patch_scores_grad), on the constants and the line fetch above.
#include "common.h"

namespace lcr {

typedef float ps_floatx16 __attribute__((ext_vector_type(16)));
constexpr int PS_K = 128;      // points per patch (cfg.model.num_points_in_patch)
constexpr int PS_BK = 32;      // channels per K-step
constexpr int PS_LD = 130;     // LDS row stride of the k-major tiles (floats)
constexpr int PS_T = 256;

__global__ __launch_bounds__(PS_T, 2) void k_patch_scores(const float* __restrict__ fa, int64_t Na, const float* __restrict__ fb, int64_t Nb, int C,
                                                          const int64_t* __restrict__ idx_a, const int64_t* __restrict__ idx_b,
                                                          const uint8_t* __restrict__ mask_a, const uint8_t* __restrict__ mask_b, float scale,
                                                          const float* __restrict__ alpha, float inf_val, float* __restrict__ S) {
  extern __shared__ __attribute__((aligned(16))) float ps_lds[];      // 4 tiles of 32 x 130 floats = 66 560 B: dynamic (above the 64 KB static limit)
  constexpr int TILE = PS_BK * PS_LD;
  auto sA = [&](int buf) { return ps_lds + buf * TILE; };
  auto sB = [&](int buf) { return ps_lds + (2 + buf) * TILE; };
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  // staging: piece q = tid + 256 i (i = 0..3) is (row q >> 3, channel quad q & 7): the 8 lanes of a row fetch one full line per K-step
  const int k4 = tid & 7;
  const float* pa[4];
  const float* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (tid + PS_T * i) >> 3;
    const int64_t ja = idx_a[p * PS_K + row], jb = idx_b[p * PS_K + row];
    pa[i] = (ja >= 0 && ja < Na) ? fa + ja * C + k4 * 4 : nullptr;       // the shadow index (== N): a zero row (index_select on the padded tensor)
    pb[i] = (jb >= 0 && jb < Nb) ? fb + jb * C + k4 * 4 : nullptr;
  }
  float4 ra[4], rb[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = pa[i] ? *reinterpret_cast<const float4*>(pa[i] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
      rb[i] = pb[i] ? *reinterpret_cast<const float4*>(pb[i] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto park = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (tid + PS_T * i) >> 3;
      float* da = sA(buf) + (k4 * 4) * PS_LD + row;
      float* db = sB(buf) + (k4 * 4) * PS_LD + row;
      da[0] = ra[i].x, da[PS_LD] = ra[i].y, da[2 * PS_LD] = ra[i].z, da[3 * PS_LD] = ra[i].w;
      db[0] = rb[i].x, db[PS_LD] = rb[i].y, db[2 * PS_LD] = rb[i].z, db[3 * PS_LD] = rb[i].w;
    }
  };
  ps_floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int nk = C / PS_BK;
  gload(0);
  park(0);
  __syncthreads();
  const int a_off = (lane >> 5) * PS_LD + wm * 64 + (lane & 31);
  const int b_off = (lane >> 5) * PS_LD + wn * 64 + (lane & 31);
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    if (t + 1 < nk) gload((t + 1) * PS_BK);
    const float* as = sA(buf) + a_off;
    const float* bs = sB(buf) + b_off;
#pragma unroll
    for (int kk = 0; kk < PS_BK / 2; ++kk) {
      const float a0 = as[kk * 2 * PS_LD], a1 = as[kk * 2 * PS_LD + 32];
      const float b0 = bs[kk * 2 * PS_LD], b1 = bs[kk * 2 * PS_LD + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (t + 1 < nk) park(buf ^ 1);                       // its last readers passed the barrier of step t - 1
    __syncthreads();
  }
  // ---- the padded score matrix (learnable_sinkhorn.py:38-49): scaled products, dustbin row / column = alpha, masked entries = -inf
  const float al = alpha[0];
  float* Sp = S + p * (PS_K + 1) * (PS_K + 1);
  const uint8_t* ma = mask_a + p * PS_K;
  const uint8_t* mb = mask_b + p * PS_K;
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const int col = wn * 64 + tj * 32 + (lane & 31);
    const bool col_ok = mb[col] != 0;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const bool ok = col_ok && ma[row] != 0;
        Sp[row * (PS_K + 1) + col] = ok ? acc[ti][tj][r] * scale : -inf_val;
      }
    }
  }
  if (tid <= PS_K) {
    const bool in = tid < PS_K;
    Sp[PS_K * (PS_K + 1) + tid] = (in && !mb[tid]) ? -inf_val : al;          // dustbin row: masked columns stay masked
    Sp[tid * (PS_K + 1) + PS_K] = (in && !ma[tid]) ? -inf_val : al;          // dustbin column (the corner is written twice with alpha)
  }
}

// ---- reverse pass (lcr_patch_scores_grad): the gradient of the products with respect to the two feature tensors -------------------------------
// With G[p] = scale * dS[p][:K,:K] (an entry of a masked row or column SELECTED to zero, so whatever dS holds there, NaN included, never enters
// a product; the dustbin row and column are never read): dA_g[p] = G[p] . gather(feats_b, idx_b[p]), dB_g[p] = G[p]^T . gather(feats_a, idx_a[p]),
// and d_feats_a[n] = the sum of dA_g[p][i] over the slots (p, i) that list n, in ascending p K + i (d_feats_b likewise).
//
//   phase 1 (k_patch_scores_grad): one workgroup per (patch pair, side).  G[p] is staged through LDS once (row stride 129 floats: 4-byte
//   loads — the rows of dS are not 16-byte aligned — and conflict-free 4-byte LDS reads along rows AND along columns, which is what lets the
//   same image serve G and G^T); every wavefront keeps the A fragments of its 32 output rows over all 128 contraction steps in 64 registers,
//   so the MFMA loop reads ONE LDS value per v_mfma_f32_32x32x2_f32.  The other side's rows are gathered straight from the feature tensor
//   in steps of 32 channels with the forward's line fetch (8 consecutive lanes = one row's 128-byte line), double-buffered in the LDS the
//   G image no longer needs, the next step's loads in flight under the 64 MFMAs of the current one.  fp32 accumulate, contraction index
//   ascending.  The products go to a workspace of 2 P K C floats (side a first).  In training P <= num_targets x pairs = 128 per pair
//   and C = 128: 8 MB per pair and side, so the workspace is not chunked.
//   phase 2 (k_patch_scores_grad_gather): one wavefront per feature row sums the workspace rows of its slots over the inverted list of
//   idx viewed as [P,K] over N rows (lcr_neighbor_transpose: positions ascending), float4 per lane.  No floating-point atomics, every output
//   element is written exactly once, and nothing depends on the launch order.
constexpr int PSG_LD = PS_K + 1;          // LDS row stride of the staged G (floats)

__global__ __launch_bounds__(PS_T, 2) void k_patch_scores_grad(const float* __restrict__ dS, const float* __restrict__ fa, int64_t Na,
                                                               const float* __restrict__ fb, int64_t Nb, int C, const int64_t* __restrict__ idx_a,
                                                               const int64_t* __restrict__ idx_b, const uint8_t* __restrict__ mask_a,
                                                               const uint8_t* __restrict__ mask_b, float scale, int64_t P, int side0,
                                                               float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) float psg_lds[];     // 128 x 129 floats (G), then two 128 x 32 tiles of the gathered rows
  const int64_t p = blockIdx.x;
  const int side = side0 + static_cast<int>(blockIdx.y);              // 0: dA_g = G . gather(fb, idx_b);  1: dB_g = G^T . gather(fa, idx_a)
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l32 = lane & 31;
  const float* fo = side ? fa : fb;
  const int64_t No = side ? Na : Nb;
  const int64_t* io = (side ? idx_a : idx_b) + p * PS_K;
  auto sB = [&](int buf) { return psg_lds + buf * (PS_K * PS_BK); };
  // the forward's staging: piece q = tid + 256 i is (row q >> 3, channel quad q & 7)
  const int k4 = tid & 7;
  const float* po[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t j = io[(tid + PS_T * i) >> 3];
    po[i] = (j >= 0 && j < No) ? fo + j * C + k4 * 4 : nullptr;       // the shadow index: a zero row
  }
  float4 rb[4];
  auto gload = [&](int c0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) rb[i] = po[i] ? *reinterpret_cast<const float4*>(po[i] + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto park = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(sB(buf) + ((tid + PS_T * i) >> 3) * PS_BK + k4 * 4) = rb[i];
  };
  gload(0);
  // ---- G[p] into LDS: thread = (column tid & 127, rows (tid >> 7) + 2 it)
  {
    const float* dSp = dS + p * (PS_K + 1) * (PS_K + 1);
    const uint8_t* ma = mask_a + p * PS_K;
    const int j = tid & (PS_K - 1);
    const bool col_ok = mask_b[p * PS_K + j] != 0;
#pragma unroll 8
    for (int it = 0; it < PS_K / 2; ++it) {
      const int i = (tid >> 7) + 2 * it;
      const float v = dSp[i * (PS_K + 1) + j];
      psg_lds[i * PSG_LD + j] = (col_ok && ma[i] != 0) ? v * scale : 0.f;
    }
  }
  __syncthreads();
  // ---- A fragments: lane (row l32, half h) holds op(G)[32 w + l32][2 kk + h], kk = 0..63
  float areg[PS_K / 2];
  if (side == 0) {
#pragma unroll
    for (int kk = 0; kk < PS_K / 2; ++kk) areg[kk] = psg_lds[(32 * w + l32) * PSG_LD + 2 * kk + h];
  } else {
#pragma unroll
    for (int kk = 0; kk < PS_K / 2; ++kk) areg[kk] = psg_lds[(2 * kk + h) * PSG_LD + 32 * w + l32];
  }
  __syncthreads();                                                     // the G image is dead: its LDS becomes the row tiles
  park(0);
  __syncthreads();
  float* out = ws + ((static_cast<int64_t>(side) * P + p) * PS_K + 32 * w) * C + l32;
  const int nk = C / PS_BK;
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    if (t + 1 < nk) gload((t + 1) * PS_BK);
    const float* bs = sB(buf) + h * PS_BK + l32;
    ps_floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < PS_K / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[kk], bs[kk * 2 * PS_BK], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) out[static_cast<int64_t>((r & 3) + 8 * (r >> 2) + 4 * h) * C + t * PS_BK] = acc[r];
    if (t + 1 < nk) park(buf ^ 1);                                     // its last readers passed the barrier of step t - 1
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_patch_scores_grad_gather(const float4* __restrict__ prod, const int32_t* __restrict__ row_start,
                                                                  const uint32_t* __restrict__ edges, int64_t N, int n_slots, int q,
                                                                  float4* __restrict__ d_feats) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6), nwaves = static_cast<int64_t>(gridDim.x) * 4;
  for (int64_t n = wave; n < N; n += nwaves) {
    int b = row_start[n], e = row_start[n + 1];
    b = max(0, min(b, n_slots));
    e = max(b, min(e, n_slots));
    for (int c = lane; c < q; c += 64) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int s = b; s < e; ++s) {
        const uint32_t slot = edges[s];                                // wave-uniform
        if (slot >= static_cast<uint32_t>(n_slots)) continue;          // an entry outside the forward's list is skipped, never dereferenced
        const float4 v = prod[static_cast<int64_t>(slot) * q + c];
        t.x += v.x, t.y += v.y, t.z += v.z, t.w += v.w;
      }
      d_feats[n * q + c] = t;
    }
  }
}

}  // namespace lcr

using namespace lcr;

extern "C" int lcr_patch_scores(const float* feats_a, int64_t Na, const float* feats_b, int64_t Nb, int C, const int64_t* idx_a, const int64_t* idx_b,
                                const uint8_t* mask_a, const uint8_t* mask_b, int64_t P, int K, float scale, const float* alpha, float inf_val,
                                float* S, void* stream) {
  if (!feats_a || !feats_b || !idx_a || !idx_b || !mask_a || !mask_b || !alpha || !S || P < 0 || Na < 0 || Nb < 0 || K != PS_K || C < PS_BK ||
      C % PS_BK != 0 || (reinterpret_cast<uintptr_t>(feats_a) | reinterpret_cast<uintptr_t>(feats_b)) % 16 != 0 || P > 2147483647)
    return refuse(LCR_EARG, "lcr_patch_scores: bad argument (patches of %d points, C a multiple of %d, 16-byte aligned features)", PS_K, PS_BK);
  if (P == 0) return LCR_OK;
  constexpr size_t lds = sizeof(float) * 4 * PS_BK * PS_LD;
  static DynLds opt_in;
  if (opt_in.need(reinterpret_cast<const void*>(&k_patch_scores), lds) != hipSuccess)
    return refuse(LCR_EHIP, "lcr_patch_scores: cannot reserve %zu B of dynamic LDS", lds);
  hipLaunchKernelGGL(k_patch_scores, dim3(static_cast<unsigned>(P)), dim3(PS_T), lds, static_cast<hipStream_t>(stream), feats_a, Na, feats_b, Nb, C, idx_a,
                     idx_b, mask_a, mask_b, scale, alpha, inf_val, S);
  return check_launch("lcr_patch_scores");
}

static bool psg_domain(int64_t P, int K, int C) { return P >= 0 && K == PS_K && C >= PS_BK && C % PS_BK == 0 && P * PS_K < (int64_t(1) << 30); }

extern "C" int lcr_patch_scores_grad_ws_bytes(int64_t P, int K, int C, size_t* bytes) {
  if (!bytes || !psg_domain(P, K, C))
    return refuse(LCR_EARG, "lcr_patch_scores_grad_ws_bytes: bad argument (patches of %d points, C a multiple of %d, P * K < 2^30)", PS_K, PS_BK);
  *bytes = sizeof(float) * 2 * static_cast<size_t>(P) * PS_K * C;
  return LCR_OK;
}

extern "C" int lcr_patch_scores_grad(const float* dS, const float* feats_a, int64_t Na, const float* feats_b, int64_t Nb, int C, const int64_t* idx_a,
                                     const int64_t* idx_b, const uint8_t* mask_a, const uint8_t* mask_b, int64_t P, int K, float scale,
                                     const int32_t* row_start_a, const uint32_t* edges_a, const int32_t* row_start_b, const uint32_t* edges_b,
                                     float* d_feats_a, float* d_feats_b, void* ws, size_t ws_bytes, void* stream) {
  const int64_t n_lim = (int64_t(1) << 31) - 1;
  if (!psg_domain(P, K, C) || Na < 0 || Nb < 0 || Na >= n_lim || Nb >= n_lim ||
      (reinterpret_cast<uintptr_t>(d_feats_a) | reinterpret_cast<uintptr_t>(d_feats_b)) % 16 != 0)
    return refuse(LCR_EARG, "lcr_patch_scores_grad: bad argument (patches of %d points, C a multiple of %d, P * K < 2^30, 16-byte aligned gradients)", PS_K, PS_BK);
  hipStream_t st = ST(stream);
  if (P == 0) {                                                        // no patch lists any row: zeros
    if ((d_feats_a && Na > 0 && hipMemsetAsync(d_feats_a, 0, sizeof(float) * Na * C, st) != hipSuccess) ||
        (d_feats_b && Nb > 0 && hipMemsetAsync(d_feats_b, 0, sizeof(float) * Nb * C, st) != hipSuccess))
      return refuse(LCR_EHIP, "lcr_patch_scores_grad: cannot zero the gradients");
    return LCR_OK;
  }
  const bool want_a = d_feats_a != nullptr, want_b = d_feats_b != nullptr;
  if (!want_a && !want_b) return LCR_OK;
  const size_t side_bytes = sizeof(float) * static_cast<size_t>(P) * PS_K * C;
  if (!dS || (Na > 0 && !feats_a) || (Nb > 0 && !feats_b) || !idx_a || !idx_b || !mask_a || !mask_b || !ws || (want_a && Na > 0 && (!row_start_a || !edges_a)) ||
      (want_b && Nb > 0 && (!row_start_b || !edges_b)) ||
      (reinterpret_cast<uintptr_t>(feats_a) | reinterpret_cast<uintptr_t>(feats_b) | reinterpret_cast<uintptr_t>(ws)) % 16 != 0)
    return refuse(LCR_EARG, "lcr_patch_scores_grad: null pointer, or features / workspace not 16-byte aligned (each gradient needs the inverted list of its idx)");
  if (ws_bytes < 2 * side_bytes) return refuse_ws(LCR_EARG, "lcr_patch_scores_grad", ws_bytes, 2 * side_bytes);
  constexpr size_t lds = sizeof(float) * PS_K * PSG_LD;
  static_assert(2 * PS_K * PS_BK <= PS_K * PSG_LD, "the row tiles live in the LDS of the G image");
  static DynLds opt_in;
  if (opt_in.need(reinterpret_cast<const void*>(&k_patch_scores_grad), lds) != hipSuccess)
    return refuse(LCR_EHIP, "lcr_patch_scores_grad: cannot reserve %zu B of dynamic LDS", lds);
  float* prod = static_cast<float*>(ws);
  hipLaunchKernelGGL(k_patch_scores_grad, dim3(static_cast<unsigned>(P), want_a && want_b ? 2 : 1), dim3(PS_T), lds, st, dS, feats_a, Na, feats_b, Nb, C,
                     idx_a, idx_b, mask_a, mask_b, scale, P, want_a ? 0 : 1, prod);
  const int n_slots = static_cast<int>(P * PS_K);
  if (want_a && Na > 0)
    hipLaunchKernelGGL(k_patch_scores_grad_gather, dim3(blocks_for(Na, 4, 8192)), dim3(256), 0, st, reinterpret_cast<const float4*>(prod), row_start_a,
                       edges_a, Na, n_slots, C / 4, reinterpret_cast<float4*>(d_feats_a));
  if (want_b && Nb > 0)
    hipLaunchKernelGGL(k_patch_scores_grad_gather, dim3(blocks_for(Nb, 4, 8192)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(prod + static_cast<size_t>(P) * PS_K * C), row_start_b, edges_b, Nb, n_slots, C / 4,
                       reinterpret_cast<float4*>(d_feats_b));
  return check_launch("lcr_patch_scores_grad");
}
