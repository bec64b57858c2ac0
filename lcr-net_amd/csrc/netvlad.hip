// netvlad.hip — a-7 / row p: the forward of the global-descriptor head (NetVLAD + context gating) for a batch of scans, fp32, in eval mode
// (lcr_netvlad_forward, running statistics) and in training mode (lcr_netvlad_train_forward, batch statistics).  The reverse pass is
// netvlad_grad.hip; what the two files share is in netvlad.h.
//
// Reference: GlobalDescritionHEAD (model_family/LCRNet_GlobalDescrition.py:34-57, LCRNet.py:115-122) =
//   F.normalize(feats_c, dim=2) -> NetVLADLoupe2.forward (modules/netvlad/NetVlad.py:49-87) -> GatingContext (:165-201) -> F.normalize(dim=1).
// The reference runs eval with batch 1 (one scan per stack); here S scans of a batch are stacked (seg_len rows each) and every
// step is segment-aware, so the 67 MB hidden1_weights matrix — the only HBM-significant operand — is streamed ONCE per group of scans
// by a split-K kernel (256 K-slices x the scans of the group), instead of once per scan.
//
// Steps, both modes: row L2-normalise (wave per row) -> assignment GEMM (lcr_gemm_f32, K=1024, N=64) -> BN + softmax over the 64 clusters
// (lane = cluster) -> per-segment x^T·a GEMM (TA) and column sums -> residual / intra-normalise / global normalise ->
// split-K hidden projection -> BN2, gating GEMV, sigmoid, final L2 normalise.  Only the three BatchNorms and what they feed differ.
//
// Training: the reference pads every cloud to Lmax rows by repeating its rows cyclically, takes bn1's statistics over all S*Lmax rows and
// gives the padding rows the uniform assignment 1/64.  No padded tensor exists here: local row i of a cloud of L rows stands for
// c = (Lmax-1-i)/L + 1 padded rows, one real and p = c-1 padding copies, so
//     bn1 statistics  = sums weighted by c over the real rows, divided by S*Lmax
//     assignment      w = softmax(bn1(a)) + p/64
// and everything behind w is the eval arithmetic up to bn2.  Saved for the reverse pass (nv::Saved): a = x^.Wc and softmax [N,64], the
// multiplicity and cloud of every row, v [S,65536] with both raw norms, the column sums of w, and the [S,256] tensors of the tail.
// x^ (4 KB a row) is NOT kept: the reverse pass normalises the rows again.  Every sum has one order: wavefront / workgroup trees of fixed
// shape, cross-workgroup partials added in ascending order by one thread per column, batch statistics in fp64.  No floating-point atomics.
#include <algorithm>
#include <vector>

#include "netvlad.h"

namespace lcr {
using namespace nv;

struct BnParams {
  const float *w, *b, *mean, *var;
};

// ------------------------------------------------------------------------------------------------ rows
// y[n] = x[n] / max(|x[n]|, 1e-12), wave per row.  The width is the constant F, not an argument: the compiler then keeps a row's 16 loads
// in flight; with the width as an argument the 78-cloud training forward and backward were 1 % and 0.5 % slower
// (profiles/r15_netvlad_shared.md).
__global__ __launch_bounds__(256) void k_row_l2norm(const float* __restrict__ x, int64_t N, float* __restrict__ y) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave index in an SGPR
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * 4 + w; n < N; n += static_cast<int64_t>(gridDim.x) * 4) {
    float ss = 0.f;
    for (int c = lane; c < F; c += 64) {
      const float v = x[n * F + c];
      ss = fmaf(v, v, ss);
    }
    ss = wave_sum(ss);
    const float d = fmaxf(sqrtf(ss), 1e-12f);
    for (int c = lane; c < F; c += 64) y[n * F + c] = x[n * F + c] / d;
  }
}

// training: the multiplicity c and the cloud of every row
__global__ __launch_bounds__(256) void k_rows_of(Seg seg, int64_t N, int32_t* __restrict__ cmul, int32_t* __restrict__ rseg) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (n >= N) return;
  const int s = cloud_of(seg.off, seg.S, n);
  const int64_t i = n - seg.off[s], L = seg.off[s + 1] - seg.off[s];
  cmul[n] = static_cast<int32_t>((seg.Lmax - 1 - i) / L + 1);
  rseg[n] = s;
}

// ------------------------------------------------------------------------------------------------ bn1 and the soft assignment
// eval: act[n][k] <- softmax_k( BN_eval(act[n][k]) ), lane = cluster (64 clusters = one wavefront)
__global__ __launch_bounds__(256) void k_bn_softmax64(float* __restrict__ act, int64_t N, BnParams bn, float eps) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave index in an SGPR
  const float scale = bn.w[lane] / sqrtf(bn.var[lane] + eps);
  const float mean = bn.mean[lane], beta = bn.b[lane];
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * 4 + w; n < N; n += static_cast<int64_t>(gridDim.x) * 4) {
    const float v = (act[n * K + lane] - mean) * scale + beta;
    float mx = v;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
    const float e = expf(v - mx);
    const float s = wave_sum(e);
    act[n * K + lane] = e / s;
  }
}

// training: (sum c a, sum c a^2) of a[N,64] in fp64, fixed order: part[g][2][64] per workgroup g, then one thread per column
__global__ __launch_bounds__(256) void k_bn1_moments(const float* __restrict__ a, const int32_t* __restrict__ cmul, int64_t N, double* __restrict__ part) {
  __shared__ double s_p[4][2][K];
  const int k = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t chunk = (N + gridDim.x - 1) / gridDim.x;
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * chunk, hi = std::min<int64_t>(lo + chunk, N);
  double t0 = 0.0, t1 = 0.0;
  for (int64_t n = lo + q; n < hi; n += 4) {
    const float av = a[n * K + k];
    const double c = static_cast<double>(cmul[n]);
    t0 += c * av;
    t1 += c * (static_cast<double>(av) * av);
  }
  s_p[q][0][k] = t0;
  s_p[q][1][k] = t1;
  __syncthreads();
  if (q < 2) part[(static_cast<int64_t>(blockIdx.x) * 2 + q) * K + k] = (s_p[0][q][k] + s_p[1][q][k]) + (s_p[2][q][k] + s_p[3][q][k]);
}

__global__ __launch_bounds__(K) void k_bn1_stats(const double* __restrict__ part, int G, double count, float* __restrict__ stat_mean,
                                                  float* __restrict__ stat_var, float* __restrict__ mu, float* __restrict__ r) {
  const int k = threadIdx.x;
  double t0 = 0.0, t1 = 0.0;
  for (int g = 0; g < G; ++g) {
    t0 += part[(g * 2 + 0) * K + k];
    t1 += part[(g * 2 + 1) * K + k];
  }
  const double mean = t0 / count, var = fmax(t1 / count - mean * mean, 0.0);
  stat_mean[k] = static_cast<float>(mean);
  stat_var[k] = static_cast<float>(var);
  mu[k] = static_cast<float>(mean);
  r[k] = static_cast<float>(1.0 / sqrt(var + static_cast<double>(BN_EPS)));
}

// training: sm = softmax_k(gamma (a - mu) r + beta) kept; w = sm + p/64 (the real copy and its p padding copies, which the reference sets
// to -1e12 before the softmax: uniform 1/64 each)
__global__ __launch_bounds__(256) void k_bn_softmax_train(const float* __restrict__ a, const int32_t* __restrict__ cmul, const float* __restrict__ mu,
                                                           const float* __restrict__ r, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           int64_t N, float* __restrict__ sm, float* __restrict__ wgt) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float m = mu[lane], rr = r[lane], ga = gamma[lane], be = beta[lane];
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * 4 + w; n < N; n += static_cast<int64_t>(gridDim.x) * 4) {
    const float v = (a[n * K + lane] - m) * rr * ga + be;
    float mx = v;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
    const float e = expf(v - mx);
    const float p = e / wave_sum(e);
    sm[n * K + lane] = p;
    if (wgt) wgt[n * K + lane] = p + static_cast<float>(cmul[n] - 1) * (1.f / 64.f);
  }
}

// ------------------------------------------------------------------------------------------------ VLAD
// out[s][k] = sum of w over the rows of cloud s = blockIdx.x of the window (deterministic: fixed 16-way row partition, fixed combine order)
__global__ __launch_bounds__(1024) void k_colsum64(const float* __restrict__ w, Seg seg, float* __restrict__ out) {
  __shared__ float part[16][K];
  const int k = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t row0 = seg.off[blockIdx.x], rows = seg.off[blockIdx.x + 1] - row0;
  float s = 0.f;
  for (int64_t n = q; n < rows; n += 16) s += w[(row0 + n) * K + k];
  part[q][k] = s;
  __syncthreads();
  if (q == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += part[i][k];
    out[blockIdx.x * K + k] = t;
  }
}

// V_s (1024 x 64) = xn_s^T (1024 x n_s) · w_s (n_s x 64) and asum[s] = the column sums of w_s for all S clouds of off[0..S], 64 clouds per
// launch: A is stored K-major -> transA
static int vlad_accumulate(const float* xn, const float* w, const std::vector<int64_t>& off, int S, float* V, float* asum, void* stream) {
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int cnt = std::min(64, S - s0);
    int kk[64];
    int64_t ao[64], bo[64], co[64];
    for (int i = 0; i < cnt; ++i) {
      kk[i] = static_cast<int>(off[s0 + i + 1] - off[s0 + i]);
      ao[i] = off[s0 + i] * F;
      bo[i] = off[s0 + i] * K;
      co[i] = static_cast<int64_t>(s0 + i) * FK;
    }
    const int rc = lcr_gemm_f32_batched_ta(xn, w, V, F, K, cnt, kk, ao, bo, co, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_colsum64, dim3(cnt), dim3(1024), 0, ST(stream), w, seg_window(off, s0, cnt, 0), asum + s0 * K);
  }
  return LCR_OK;
}

// V[c][k] (1024 x 64 per segment): subtract a_sum * Wc2, normalise each cluster column over c (eps 1e-6), then the whole
// 65536-vector (eps 1e-6); output flattened c-major (index c*64 + k) = vlad.view(-1, 65536) of NetVlad.py:73-75.  KEEP_NORMS: the two raw
// norms go to n1raw [S,64] and n2raw [S] for the reverse pass.
template <bool KEEP_NORMS>
__global__ __launch_bounds__(1024) void k_vlad_finalize(float* __restrict__ V, const float* __restrict__ a_sum, const float* __restrict__ Wc2,
                                                         float* __restrict__ n1raw, float* __restrict__ n2raw) {
  __shared__ float s_col[16][K];
  __shared__ float s_inv[K];
  __shared__ float s_tot;
  float* v = V + static_cast<int64_t>(blockIdx.x) * FK;
  const float* as = a_sum + blockIdx.x * K;
  const int k = threadIdx.x & 63, q = threadIdx.x >> 6;   // 16 row-groups x 64 clusters
  const float ak = as[k];
  float ss = 0.f;
  constexpr int FB = 8;                           // rows requested per trip: one workgroup per scan, latency is all there is to hide
  static_assert((F / 16) % FB == 0, "row batches");
  for (int c0 = q; c0 < F; c0 += 16 * FB) {
    float vv[FB], ww[FB];
#pragma unroll
    for (int u = 0; u < FB; ++u) {
      vv[u] = v[(c0 + 16 * u) * K + k];
      ww[u] = Wc2[(c0 + 16 * u) * K + k];
    }
#pragma unroll
    for (int u = 0; u < FB; ++u) {
      const float t = vv[u] - ak * ww[u];
      v[(c0 + 16 * u) * K + k] = t;
      ss = fmaf(t, t, ss);
    }
  }
  s_col[q][k] = ss;
  __syncthreads();
  if (q == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += s_col[i][k];
    const float nrm = sqrtf(t);
    const float inv = 1.f / fmaxf(nrm, 1e-6f);
    s_inv[k] = inv;
    if constexpr (KEEP_NORMS) n1raw[blockIdx.x * K + k] = nrm;
    const float u = nrm * inv;   // norm of the normalised column
    float tot = u * u;
    tot = wave_sum(tot);
    if (k == 0) s_tot = tot;
  }
  __syncthreads();
  const float n2 = sqrtf(s_tot);
  if constexpr (KEEP_NORMS)
    if (threadIdx.x == 0) n2raw[blockIdx.x] = n2;
  const float g = 1.f / fmaxf(n2, 1e-6f);
  const float f = s_inv[k] * g;
  for (int c0 = q; c0 < F; c0 += 16 * FB) {
    float vv[FB];
#pragma unroll
    for (int u = 0; u < FB; ++u) vv[u] = v[(c0 + 16 * u) * K + k];
#pragma unroll
    for (int u = 0; u < FB; ++u) v[(c0 + 16 * u) * K + k] = vv[u] * f;
  }
}

// ------------------------------------------------------------------------------------------------ the hidden projection
// partial[slice][s][j] = sum_{i in slice} v[s][i] * H[i][j] for up to SMAX clouds from s0; one workgroup per K-slice, thread = output
// column j, so the 67 MB weight matrix is streamed once per SMAX clouds.  The slice of v goes through LDS CH rows at a time (clouds past
// the last are zero-filled: staging only the live ones spills at SMAX = 64), HB rows of H are requested per trip (one wavefront per SIMD
// has nothing else to hide the latency with); the additions keep the row order whatever CH and HB are.
template <int SMAX, int CH, int HB>
__global__ __launch_bounds__(D) void k_hidden_splitk(const float* __restrict__ V, const float* __restrict__ H, int S, int s0,
                                                      float* __restrict__ partial) {
  constexpr int ROWS = FK / SPLIT;   // 256
  static_assert(ROWS % CH == 0 && CH % HB == 0 && (SMAX * CH) % D == 0, "chunks and row batches");
  __shared__ float s_v[SMAX][CH];
  const int j = threadIdx.x;
  const int i0 = blockIdx.x * ROWS;
  const int ns = min(SMAX, S - s0);
  float acc[SMAX];
#pragma unroll
  for (int s = 0; s < SMAX; ++s) acc[s] = 0.f;
  for (int c0 = 0; c0 < ROWS; c0 += CH) {
    __syncthreads();
    for (int t = j; t < SMAX * CH; t += D) {
      const int s = t / CH, i = t % CH;
      s_v[s][i] = s < ns ? V[static_cast<int64_t>(s0 + s) * FK + i0 + c0 + i] : 0.f;
    }
    __syncthreads();
    const float* hp = H + static_cast<int64_t>(i0 + c0) * D + j;
    for (int i = 0; i < CH; i += HB) {
      float h[HB];
#pragma unroll
      for (int u = 0; u < HB; ++u) h[u] = hp[static_cast<int64_t>(i + u) * D];
#pragma unroll
      for (int u = 0; u < HB; ++u)
#pragma unroll
        for (int s = 0; s < SMAX; ++s) acc[s] = fmaf(s_v[s][i + u], h[u], acc[s]);
    }
  }
#pragma unroll
  for (int s = 0; s < SMAX; ++s)
    if (s < ns) partial[(static_cast<int64_t>(blockIdx.x) * S + s0 + s) * D + j] = acc[s];
}

template <int SMAX, int CH, int HB>
static void launch_hidden(const float* V, const float* H, int S, float* partial, hipStream_t st) {
  for (int s0 = 0; s0 < S; s0 += SMAX) hipLaunchKernelGGL((k_hidden_splitk<SMAX, CH, HB>), dim3(SPLIT), dim3(D), 0, st, V, H, S, s0, partial);
}

// column j of cloud s: the SPLIT K-slices added in ascending order, 16 loads requested per trip (a few workgroups: nothing else hides
// the latency)
__device__ __forceinline__ float hidden_slice_sum(const float* __restrict__ partial, int S, int s, int j) {
  constexpr int TB = 16;
  static_assert(SPLIT % TB == 0, "load batches");
  float o = 0.f;
  for (int b = 0; b < SPLIT; b += TB) {
    float p[TB];
#pragma unroll
    for (int u = 0; u < TB; ++u) p[u] = partial[(static_cast<int64_t>(b + u) * S + s) * D + j];
#pragma unroll
    for (int u = 0; u < TB; ++u) o += p[u];
  }
  return o;
}

__global__ __launch_bounds__(D) void k_hidden_reduce(const float* __restrict__ partial, int S, float* __restrict__ h) {
  const int s = blockIdx.x, j = threadIdx.x;
  h[s * D + j] = hidden_slice_sum(partial, S, s, j);
}

// ------------------------------------------------------------------------------------------------ the tail ([S,256]; thread = column)
// eval, one workgroup per scan: reduce the K-slices, BN2, context gating (NetVlad.py:187-199), final F.normalize(dim=1)
__global__ __launch_bounds__(D) void k_netvlad_tail(const float* __restrict__ partial, int S, BnParams bn2, const float* __restrict__ Wg,
                                                     BnParams bng, float eps, float* __restrict__ out) {
  __shared__ float s_o[D];
  __shared__ float s_red[4];
  const int s = blockIdx.x, j = threadIdx.x;
  float o = hidden_slice_sum(partial, S, s, j);
  constexpr int TB = 16;                          // rows of Wg requested per trip (8 workgroups: nothing else hides the latency)
  static_assert(D % TB == 0, "load batches");
  o = (o - bn2.mean[j]) / sqrtf(bn2.var[j] + eps) * bn2.w[j] + bn2.b[j];
  s_o[j] = o;
  __syncthreads();
  float g = 0.f;
  for (int i = 0; i < D; i += TB) {
    float wv[TB];
#pragma unroll
    for (int u = 0; u < TB; ++u) wv[u] = Wg[(i + u) * D + j];
#pragma unroll
    for (int u = 0; u < TB; ++u) g = fmaf(s_o[i + u], wv[u], g);
  }
  g = (g - bng.mean[j]) / sqrtf(bng.var[j] + eps) * bng.w[j] + bng.b[j];
  g = 1.f / (1.f + expf(-g));
  const float a = o * g;
  const float tot = block_sum<4>(a * a, s_red);
  out[s * D + j] = a / fmaxf(sqrtf(tot), 1e-12f);
}

// training: BatchNorm over the S descriptors of x[S,256] on batch statistics (fp64 sums in ascending s): xh = (x - mean) r, y = gamma xh + beta
__global__ __launch_bounds__(D) void k_bn_batch(const float* __restrict__ x, int S, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                 float* __restrict__ stat_mean, float* __restrict__ stat_var, float* __restrict__ r_out,
                                                 float* __restrict__ xh, float* __restrict__ y) {
  const int j = threadIdx.x;
  double t = 0.0;
  for (int s = 0; s < S; ++s) t += x[s * D + j];
  const double mean = t / S;
  double q = 0.0;
  for (int s = 0; s < S; ++s) {
    const double d = x[s * D + j] - mean;
    q += d * d;
  }
  const double var = q / S;
  const float r = static_cast<float>(1.0 / sqrt(var + static_cast<double>(BN_EPS)));
  stat_mean[j] = static_cast<float>(mean);
  stat_var[j] = static_cast<float>(var);
  r_out[j] = r;
  const float mf = static_cast<float>(mean), ga = gamma[j], be = beta[j];
  for (int s = 0; s < S; ++s) {
    const float n = (x[s * D + j] - mf) * r;
    xh[s * D + j] = n;
    if (y) y[s * D + j] = n * ga + be;
  }
}

// training, cloud blockIdx.x: g = sigmoid(gamma gh + beta), t = h' g, out = t / max(|t|, 1e-12)
__global__ __launch_bounds__(D) void k_gate_out(const float* __restrict__ hp, const float* __restrict__ gh, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float* __restrict__ g, float* __restrict__ tn, float* __restrict__ out_keep,
                                                 float* __restrict__ out) {
  __shared__ float s_red[4];
  const int s = blockIdx.x, j = threadIdx.x;
  const float pre = gh[s * D + j] * gamma[j] + beta[j];
  const float gv = 1.f / (1.f + expf(-pre));
  const float t = hp[s * D + j] * gv;
  const float nrm = sqrtf(block_sum<4>(t * t, s_red));
  const float o = t / fmaxf(nrm, 1e-12f);
  g[s * D + j] = gv;
  out[s * D + j] = o;
  out_keep[s * D + j] = o;
  if (j == 0) tn[s] = nrm;
}

// ------------------------------------------------------------------------------------------------ what netvlad.h declares
namespace nv {

int seg_offsets(const char* who, const int64_t* seg_len_host, int S, int s_min, int s_max, std::vector<int64_t>* off, int* Lmax) {
  if (!seg_len_host || S < s_min || (s_max && S > s_max))
    return s_max ? refuse(LCR_EARG, "%s: S = %d outside %d .. %d, or no segment lengths", who, S, s_min, s_max)
                 : refuse(LCR_EARG, "%s: S = %d below %d, or no segment lengths", who, S, s_min);
  off->resize(static_cast<size_t>(S) + 1);
  int64_t N = 0, longest = 0;
  for (int s = 0; s < S; ++s) {
    if (seg_len_host[s] < 1 || seg_len_host[s] > 2147483647LL - N)
      return refuse(LCR_EARG, "%s: segment %d has length %lld (each at least 1, %lld rows before it, 2^31-1 in all)", who, s,
                    static_cast<long long>(seg_len_host[s]), static_cast<long long>(N));
    (*off)[s] = N;
    N += seg_len_host[s];
    longest = std::max(longest, seg_len_host[s]);
  }
  (*off)[S] = N;
  *Lmax = static_cast<int>(longest);
  return LCR_OK;
}

void launch_row_l2norm(const float* x, int64_t N, float* y, hipStream_t st) {
  hipLaunchKernelGGL(k_row_l2norm, dim3(row_blocks(N)), dim3(256), 0, st, x, N, y);
}

}  // namespace nv
}  // namespace lcr

using namespace lcr;

// ------------------------------------------------------------------------------------------------ eval
struct NetvladLayout {   // xn [n_rows, F] unit-norm rows, act [n_rows, K] soft assignments, V [S, F, K], asum [S, K],
  float *xn, *act, *V, *asum, *partial;   // partial [SPLIT, S, D] split-K partials of the hidden projection
  size_t bytes;
};
static NetvladLayout netvlad_layout(void* ws, int64_t n_rows, int S) {
  NetvladLayout L;
  Carver c(ws, ~size_t(0));
  const size_t rows = static_cast<size_t>(n_rows > 0 ? n_rows : 1);
  L.xn = c.take<float>(rows * F);
  L.act = c.take<float>(rows * K);
  L.V = c.take<float>(static_cast<size_t>(S) * FK);
  L.asum = c.take<float>(static_cast<size_t>(S) * K);
  L.partial = c.take<float>(static_cast<size_t>(SPLIT) * S * D);
  L.bytes = c.off;
  return L;
}

extern "C" int lcr_netvlad_ws_bytes(int64_t n_rows, int S, size_t* bytes) {
  if (!bytes || n_rows < 0 || S < 1) return refuse(LCR_EARG, "lcr_netvlad_ws_bytes: null pointer or outside the domain (n_rows >= 0, S >= 1): n_rows=%lld S=%d", static_cast<long long>(n_rows), S);
  *bytes = netvlad_layout(nullptr, n_rows, S).bytes;
  return LCR_OK;
}

// feats [sum(seg_len), 1024] (coarse node features, stacked) -> out [S, 256] unit-norm descriptors.  Any S >= 1.
extern "C" int lcr_netvlad_forward(const float* feats, const int64_t* seg_len_host, int S, const LcrNetvladWeights* wt, float* out,
                                   void* ws, size_t ws_bytes, void* stream) {
  const char* who = "lcr_netvlad_forward";
  if (!feats || !wt || !out || !ws) return refuse(LCR_EARG, "%s: bad argument", who);
  std::vector<int64_t> off;
  int Lmax = 0;
  int rc = seg_offsets(who, seg_len_host, S, 1, 0, &off, &Lmax);
  if (rc) return rc;
  const int64_t N = off[S];
  const NetvladLayout L = netvlad_layout(ws, N, S);
  if (L.bytes > ws_bytes) return refuse(LCR_ESPACE, "%s: workspace too small (%zu < %zu)", who, ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  launch_row_l2norm(feats, N, L.xn, st);
  rc = lcr_gemm_f32(L.xn, wt->cluster_weights, L.act, N, K, F, 0, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_bn_softmax64, dim3(row_blocks(N)), dim3(256), 0, st, L.act, N, BnParams{wt->bn1_w, wt->bn1_b, wt->bn1_mean, wt->bn1_var},
                     BN_EPS);
  rc = vlad_accumulate(L.xn, L.act, off, S, L.V, L.asum, stream);
  if (rc) return rc;
  hipLaunchKernelGGL((k_vlad_finalize<false>), dim3(S), dim3(1024), 0, st, L.V, L.asum, wt->cluster_weights2, static_cast<float*>(nullptr),
                     static_cast<float*>(nullptr));
  launch_hidden<8, 256, 16>(L.V, wt->hidden1_weights, S, L.partial, st);   // the whole 256-row slice of 8 scans in LDS
  hipLaunchKernelGGL(k_netvlad_tail, dim3(S), dim3(D), 0, st, L.partial, S, BnParams{wt->bn2_w, wt->bn2_b, wt->bn2_mean, wt->bn2_var},
                     wt->gating_weights, BnParams{wt->gbn_w, wt->gbn_b, wt->gbn_mean, wt->gbn_var}, BN_EPS, out);
  return check_launch(who);
}

// ------------------------------------------------------------------------------------------------ training
struct FwdWs {
  float *xn, *w, *partial, *h, *g0;
  double* part;
  size_t bytes;
};
static FwdWs fwd_layout(void* p, int64_t n_rows, int S) {
  FwdWs L;
  Carver c(p, ~size_t(0));
  const size_t rows = static_cast<size_t>(std::max<int64_t>(n_rows, 1)), s = static_cast<size_t>(S);
  L.xn = c.take<float>(rows * F);
  L.w = c.take<float>(rows * K);
  L.partial = c.take<float>(static_cast<size_t>(SPLIT) * s * D);
  L.h = c.take<float>(s * D);
  L.g0 = c.take<float>(s * D);
  L.part = c.take<double>(static_cast<size_t>(STAT_G) * 2 * K);
  L.bytes = c.off;
  return L;
}

extern "C" int lcr_netvlad_train_saved_bytes(int64_t n_rows, int S, size_t* bytes) {
  if (!bytes || n_rows < 0 || S < 1) return refuse(LCR_EARG, "lcr_netvlad_train_saved_bytes: null pointer or outside the domain (n_rows >= 0, S >= 1): n_rows=%lld S=%d", static_cast<long long>(n_rows), S);
  *bytes = saved_layout(nullptr, n_rows, S).bytes;
  return LCR_OK;
}

extern "C" int lcr_netvlad_train_ws_bytes(int64_t n_rows, int S, size_t* bytes) {
  if (!bytes || n_rows < 0 || S < 1) return refuse(LCR_EARG, "lcr_netvlad_train_ws_bytes: null pointer or outside the domain (n_rows >= 0, S >= 1): n_rows=%lld S=%d", static_cast<long long>(n_rows), S);
  *bytes = fwd_layout(nullptr, n_rows, S).bytes;
  return LCR_OK;
}

// 2 <= S <= 128 (batch statistics need more than one cloud).  batch_stats: mean, biased variance of bn1 [64], bn2 [256],
// context_gating.bn1 [256]
extern "C" int lcr_netvlad_train_forward(const float* feats, const int64_t* seg_len_host, int S, const LcrNetvladWeights* wt, float* out,
                                         float* batch_stats, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "lcr_netvlad_train_forward";
  if (!feats || !wt || !out || !batch_stats || !saved || !ws) return refuse(LCR_EARG, "%s: bad argument", who);
  std::vector<int64_t> off;
  int Lmax = 0;
  int rc = seg_offsets(who, seg_len_host, S, 2, S_MAX, &off, &Lmax);
  if (rc) return rc;
  const int64_t N = off[S];
  const Saved sv = saved_layout(saved, N, S);
  const FwdWs L = fwd_layout(ws, N, S);
  if (sv.bytes > saved_bytes || L.bytes > ws_bytes)
    return refuse(LCR_ESPACE, "%s: buffer too small (saved %zu < %zu or workspace %zu < %zu)", who, saved_bytes, sv.bytes, ws_bytes, L.bytes);
  hipStream_t st = ST(stream);
  float* st_mean1 = batch_stats;
  float* st_var1 = batch_stats + K;
  float* st_mean2 = batch_stats + 2 * K;
  float* st_var2 = st_mean2 + D;
  float* st_meang = st_var2 + D;
  float* st_varg = st_meang + D;
  const int nblk = row_blocks(N);
  hipLaunchKernelGGL(k_rows_of, dim3(div_up(N, 256)), dim3(256), 0, st, seg_window(off, 0, S, Lmax), N, sv.cmul, sv.rseg);
  launch_row_l2norm(feats, N, L.xn, st);
  rc = lcr_gemm_f32(L.xn, wt->cluster_weights, sv.a, N, K, F, 0, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, stream);
  if (rc) return rc;
  const int G = stat_blocks(N);
  hipLaunchKernelGGL(k_bn1_moments, dim3(G), dim3(256), 0, st, sv.a, sv.cmul, N, L.part);
  hipLaunchKernelGGL(k_bn1_stats, dim3(1), dim3(K), 0, st, L.part, G, static_cast<double>(S) * Lmax, st_mean1, st_var1, sv.mu1, sv.r1);
  hipLaunchKernelGGL(k_bn_softmax_train, dim3(nblk), dim3(256), 0, st, sv.a, sv.cmul, sv.mu1, sv.r1, wt->bn1_w, wt->bn1_b, N, sv.sm, L.w);
  rc = vlad_accumulate(L.xn, L.w, off, S, sv.v, sv.asum, stream);
  if (rc) return rc;
  hipLaunchKernelGGL((k_vlad_finalize<true>), dim3(S), dim3(1024), 0, st, sv.v, sv.asum, wt->cluster_weights2, sv.n1raw, sv.n2raw);
  // H is streamed once up to 64 clouds, twice up to 128
  if (S <= 8) launch_hidden<8, 128, 8>(sv.v, wt->hidden1_weights, S, L.partial, st);
  else if (S <= 32) launch_hidden<32, 128, 8>(sv.v, wt->hidden1_weights, S, L.partial, st);
  else launch_hidden<64, 128, 8>(sv.v, wt->hidden1_weights, S, L.partial, st);
  hipLaunchKernelGGL(k_hidden_reduce, dim3(S), dim3(D), 0, st, L.partial, S, L.h);
  hipLaunchKernelGGL(k_bn_batch, dim3(1), dim3(D), 0, st, L.h, S, wt->bn2_w, wt->bn2_b, st_mean2, st_var2, sv.r2, sv.hh, sv.hp);
  rc = lcr_gemm_f32(sv.hp, wt->gating_weights, L.g0, S, D, D, 0, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_bn_batch, dim3(1), dim3(D), 0, st, L.g0, S, wt->gbn_w, wt->gbn_b, st_meang, st_varg, sv.rg, sv.gh, static_cast<float*>(nullptr));
  hipLaunchKernelGGL(k_gate_out, dim3(S), dim3(D), 0, st, sv.hp, sv.gh, wt->gbn_w, wt->gbn_b, sv.g, sv.tn, sv.out, out);
  return check_launch(who);
}
