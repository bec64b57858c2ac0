// adan.hip — the Adan optimiser step over a list of tensors in one pass, and the global gradient norm it clips by (include/lcr_hip.h).
//
// Multi-tensor apply: the HOST tensor table is packed into kernel arguments, ADAN_STEP_TENSORS (step) or ADAN_NORM_TENSORS (norm) tensors
// per launch together with the prefix table of their chunk counts; workgroup b of a launch finds its (tensor, chunk) by a search of that
// table (wave-uniform: scalar loads from the kernel-argument segment).  Nothing lives on the device between calls, nothing is copied and
// the host never waits.  A chunk is ADAN_CHUNK = 4096 elements: 256 threads x 4 quads of 4 consecutive floats; thread t of a chunk owns
// the quads t, t + 256, t + 512, t + 768.  A quad moves as one 16-byte access when it lies inside the tensor and every array of the
// tensor is 16-byte aligned, element by element otherwise (the tail quad, and all of a tensor that is a view at an odd offset).
#include "common.h"

namespace lcr {

constexpr int ADAN_BLOCK = 256;
constexpr int ADAN_QUADS = 4;                                    // quads per thread
constexpr int64_t ADAN_CHUNK = ADAN_BLOCK * ADAN_QUADS * 4;      // 4096 elements
constexpr int ADAN_STEP_TENSORS = 48;                            // 6 x 48 pointers + sizes + prefix: 2.9 KB of the 4 KB of kernel arguments
constexpr int ADAN_NORM_TENSORS = 160;                           // 1 x 160 pointers + sizes + prefix: 3.2 KB
constexpr int64_t ADAN_MAX_GRID = int64_t(1) << 23;                  // workgroups per launch: 2^31 threads, 2^35 elements

struct AdanHyperF {                                              // the host's doubles, rounded to fp32 once
  float beta1, beta2, beta3, omb1, omb2, omb3, bias1, bias2, bias3_sqrt, lr, eps, decay;      // decay = 1 - lr*wd (no_prox) or 1 + lr*wd
  int32_t no_prox;
};

struct AdanStepArgs {
  float* p[ADAN_STEP_TENSORS];
  float* g[ADAN_STEP_TENSORS];
  float* m[ADAN_STEP_TENSORS];
  float* n[ADAN_STEP_TENSORS];
  float* d[ADAN_STEP_TENSORS];
  float* pg[ADAN_STEP_TENSORS];
  int64_t numel[ADAN_STEP_TENSORS];
  int32_t first[ADAN_STEP_TENSORS + 1];                          // first[i] = the launch's first workgroup of tensor i; first[count] = grid
  int32_t count;
  uint64_t fresh;                                                // bit i: tensor i has no previous gradient
  const float* clip;
  AdanHyperF h;
};
static_assert(sizeof(AdanStepArgs) <= 4096, "kernel arguments are limited to 4 KB");

struct AdanNormArgs {
  const float* g[ADAN_NORM_TENSORS];
  int64_t numel[ADAN_NORM_TENSORS];
  int32_t first[ADAN_NORM_TENSORS + 1];
  int32_t count;
  int64_t base;                                                  // global index of the launch's first workgroup
  double* partial;
};
static_assert(sizeof(AdanNormArgs) <= 4096, "kernel arguments are limited to 4 KB");

// the tensor that owns workgroup b: the last i with first[i] <= b (tensors without elements own no workgroup and are skipped by <=)
__device__ __forceinline__ int adan_owner(const int32_t* first, int count, int b) {
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ float4 load_quad(const float* __restrict__ x, int64_t e, int64_t numel, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(x + e);
  float4 v;
  v.x = e < numel ? x[e] : 0.f;
  v.y = e + 1 < numel ? x[e + 1] : 0.f;
  v.z = e + 2 < numel ? x[e + 2] : 0.f;
  v.w = e + 3 < numel ? x[e + 3] : 0.f;
  return v;
}

__device__ __forceinline__ void store_quad(float* __restrict__ x, int64_t e, int64_t numel, bool vec, float4 v) {
  if (vec) {
    *reinterpret_cast<float4*>(x + e) = v;
    return;
  }
  if (e < numel) x[e] = v.x;
  if (e + 1 < numel) x[e + 1] = v.y;
  if (e + 2 < numel) x[e + 2] = v.z;
  if (e + 3 < numel) x[e + 3] = v.w;
}

// One element of the step (the definition in include/lcr_hip.h): fp32, every operation rounded.
__device__ __forceinline__ void adan_element(const AdanHyperF& h, float c, bool fresh, float& p, float& g, float& m, float& n, float& d,
                                             float& pg) {
#pragma clang fp contract(off)
  const float gc = c < 1.0f ? g * c : g;
  const float diff = fresh ? 0.0f : gc - pg;
  const float u = gc + h.beta2 * diff;
  m = m * h.beta1 + h.omb1 * gc;
  d = d * h.beta2 + h.omb2 * diff;
  n = n * h.beta3 + h.omb3 * u * u;
  const float den = __fdiv_rn(__fsqrt_rn(n), h.bias3_sqrt) + h.eps;
  const float upd = __fdiv_rn(__fdiv_rn(m, h.bias1) + __fdiv_rn(h.beta2 * d, h.bias2), den);
  p = h.no_prox ? p * h.decay - h.lr * upd : __fdiv_rn(p - h.lr * upd, h.decay);
  g = gc;
  pg = gc;
}

__global__ __launch_bounds__(ADAN_BLOCK) void k_adan_step(const AdanStepArgs a) {
  const int b = blockIdx.x;
  const int i = __builtin_amdgcn_readfirstlane(adan_owner(a.first, a.count, b));
  const int64_t numel = a.numel[i];
  const int64_t chunk0 = static_cast<int64_t>(b - a.first[i]) * ADAN_CHUNK;
  float* __restrict__ P = a.p[i];
  float* __restrict__ G = a.g[i];
  float* __restrict__ M = a.m[i];
  float* __restrict__ N = a.n[i];
  float* __restrict__ D = a.d[i];
  float* __restrict__ PG = a.pg[i];
  const bool fresh = (a.fresh >> i) & 1u;
  const bool all16 = aligned16(P) && aligned16(G) && aligned16(M) && aligned16(N) && aligned16(D) && aligned16(PG);
  const float c = a.clip ? *a.clip : 1.0f;
  const bool clips = c < 1.0f;
#pragma unroll 1
  for (int q = 0; q < ADAN_QUADS; ++q) {
    const int64_t e = chunk0 + (static_cast<int64_t>(q) * ADAN_BLOCK + threadIdx.x) * 4;
    if (e >= numel) break;
    const bool vec = all16 && e + 4 <= numel;
    float4 p = load_quad(P, e, numel, vec), g = load_quad(G, e, numel, vec), m = load_quad(M, e, numel, vec);
    float4 n = load_quad(N, e, numel, vec), d = load_quad(D, e, numel, vec);
    float4 pg = fresh ? make_float4(0.f, 0.f, 0.f, 0.f) : load_quad(PG, e, numel, vec);
    adan_element(a.h, c, fresh, p.x, g.x, m.x, n.x, d.x, pg.x);
    adan_element(a.h, c, fresh, p.y, g.y, m.y, n.y, d.y, pg.y);
    adan_element(a.h, c, fresh, p.z, g.z, m.z, n.z, d.z, pg.z);
    adan_element(a.h, c, fresh, p.w, g.w, m.w, n.w, d.w, pg.w);
    store_quad(P, e, numel, vec, p);
    store_quad(M, e, numel, vec, m);
    store_quad(N, e, numel, vec, n);
    store_quad(D, e, numel, vec, d);
    store_quad(PG, e, numel, vec, pg);
    if (clips) store_quad(G, e, numel, vec, g);
  }
}

// fixed-order sum of a workgroup's 256 doubles: the wavefront's xor tree, then the four wavefronts in order
__device__ __forceinline__ double adan_block_sum(double v, double* s_w) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = dadd(v, __shfl_xor(v, s));
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return dadd(dadd(dadd(s_w[0], s_w[1]), s_w[2]), s_w[3]);
}

__global__ __launch_bounds__(ADAN_BLOCK) void k_adan_sumsq(const AdanNormArgs a) {
  __shared__ double s_w[ADAN_BLOCK / WAVE];
  const int b = blockIdx.x;
  const int i = __builtin_amdgcn_readfirstlane(adan_owner(a.first, a.count, b));
  const int64_t numel = a.numel[i];
  const int64_t chunk0 = static_cast<int64_t>(b - a.first[i]) * ADAN_CHUNK;
  const float* __restrict__ G = a.g[i];
  const bool all16 = aligned16(G);
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < ADAN_QUADS; ++q) {
    const int64_t e = chunk0 + (static_cast<int64_t>(q) * ADAN_BLOCK + threadIdx.x) * 4;
    if (e < numel) {                                             // elements past the end load as 0 and add +0.0
      const float4 g = load_quad(G, e, numel, all16 && e + 4 <= numel);
      acc = dadd(acc, dmul(g.x, g.x));
      acc = dadd(acc, dmul(g.y, g.y));
      acc = dadd(acc, dmul(g.z, g.z));
      acc = dadd(acc, dmul(g.w, g.w));
    }
  }
  const double total = adan_block_sum(acc, s_w);
  if (threadIdx.x == 0) a.partial[a.base + b] = total;
}

__global__ __launch_bounds__(ADAN_BLOCK) void k_adan_norm_finish(const double* __restrict__ partial, int64_t count, float max_grad_norm,
                                                                 float eps, float* __restrict__ norm_clip) {
  __shared__ double s_w[ADAN_BLOCK / WAVE];
  double acc = 0.0;
  for (int64_t k = threadIdx.x; k < count; k += ADAN_BLOCK) acc = dadd(acc, partial[k]);
  const double total = adan_block_sum(acc, s_w);
  if (threadIdx.x == 0) {
    const float norm = static_cast<float>(sqrt(total));
    norm_clip[0] = norm;
    norm_clip[1] = max_grad_norm > 0.0f ? fminf(fdiv(max_grad_norm, fadd(norm, eps)), 1.0f) : 1.0f;
  }
}

}  // namespace lcr

using namespace lcr;

// Validates the table; *chunks = the workgroups the whole list needs.
static int adan_check(const char* entry, const LcrAdanTensor* t, int T, bool grads_only, int64_t* chunks) {
  if (T < 0 || (T > 0 && !t)) return refuse(LCR_EARG, "%s: T = %d tensors with %s table", entry, T, t ? "a" : "no");
  int64_t total = 0;
  for (int i = 0; i < T; ++i) {
    const float* ptrs[6] = {t[i].g, t[i].p, t[i].m, t[i].n, t[i].d, t[i].pg};
    const int np = grads_only ? 1 : 6;
    if (t[i].numel < 0) return refuse(LCR_EARG, "%s: tensor %d has numel %lld", entry, i, static_cast<long long>(t[i].numel));
    for (int k = 0; k < np; ++k) {
      if (t[i].numel > 0 && !ptrs[k]) return refuse(LCR_EARG, "%s: tensor %d has a null pointer", entry, i);
      if (reinterpret_cast<uintptr_t>(ptrs[k]) & 3u) return refuse(LCR_EARG, "%s: tensor %d has a pointer that is not 4-byte aligned", entry, i);
    }
    const int64_t c = (t[i].numel + ADAN_CHUNK - 1) / ADAN_CHUNK;
    if (c > ADAN_MAX_GRID) return refuse(LCR_EARG, "%s: tensor %d has more than 2^35 elements", entry, i);
    total += c;
  }
  *chunks = total;
  return LCR_OK;
}

extern "C" int lcr_adan_ws_bytes(const LcrAdanTensor* t, int T, size_t* bytes) {
  int64_t chunks = 0;
  if (!bytes) return refuse(LCR_EARG, "lcr_adan_ws_bytes: null pointer");
  const int rc = adan_check("lcr_adan_ws_bytes", t, T, true, &chunks);
  if (rc != LCR_OK) return rc;
  *bytes = align_up(static_cast<size_t>(std::max<int64_t>(chunks, 1)) * sizeof(double));
  return LCR_OK;
}

extern "C" int lcr_adan_grad_norm(const LcrAdanTensor* t, int T, double max_grad_norm, double eps, float* norm_clip, void* ws,
                                  size_t ws_bytes, void* stream) {
  int64_t chunks = 0;
  const int rc = adan_check("lcr_adan_grad_norm", t, T, true, &chunks);
  if (rc != LCR_OK) return rc;
  if (!norm_clip || !ws || !(max_grad_norm >= 0) || !(eps >= 0)) return refuse(LCR_EARG, "lcr_adan_grad_norm: null pointer, or max_grad_norm / eps negative or NaN");
  if (static_cast<size_t>(chunks) * sizeof(double) > ws_bytes)
    return refuse_ws(LCR_ESPACE, "lcr_adan_grad_norm", ws_bytes, static_cast<size_t>(chunks) * sizeof(double));
  hipStream_t st = ST(stream);
  AdanNormArgs a;
  a.partial = static_cast<double*>(ws);
  a.base = 0;
  int cnt = 0;
  int64_t grid = 0;
  auto flush = [&]() {
    if (grid > 0) {
      a.count = cnt;
      a.first[cnt] = static_cast<int32_t>(grid);
      hipLaunchKernelGGL(k_adan_sumsq, dim3(static_cast<unsigned>(grid)), dim3(ADAN_BLOCK), 0, st, a);
    }
    a.base += grid;
    cnt = 0;
    grid = 0;
  };
  for (int i = 0; i < T; ++i) {
    if (t[i].numel == 0) continue;
    const int64_t c = (t[i].numel + ADAN_CHUNK - 1) / ADAN_CHUNK;
    if (cnt == ADAN_NORM_TENSORS || grid + c > ADAN_MAX_GRID) flush();
    a.g[cnt] = t[i].g;
    a.numel[cnt] = t[i].numel;
    a.first[cnt] = static_cast<int32_t>(grid);
    ++cnt;
    grid += c;
  }
  flush();
  hipLaunchKernelGGL(k_adan_norm_finish, dim3(1), dim3(ADAN_BLOCK), 0, st, static_cast<const double*>(ws), chunks,
                     static_cast<float>(max_grad_norm), static_cast<float>(eps), norm_clip);
  return check_launch("lcr_adan_grad_norm");
}

extern "C" int lcr_adan_step(const LcrAdanTensor* t, int T, const LcrAdanHyper* h, const float* clip, void* stream) {
  int64_t chunks = 0;
  const int rc = adan_check("lcr_adan_step", t, T, false, &chunks);
  if (rc != LCR_OK) return rc;
  if (!h || (reinterpret_cast<uintptr_t>(clip) & 3u)) return refuse(LCR_EARG, "lcr_adan_step: no hyper-parameters, or a clip pointer that is not 4-byte aligned");
  hipStream_t st = ST(stream);
  AdanStepArgs a;
  a.clip = clip;
  a.h.beta1 = static_cast<float>(h->beta1);
  a.h.beta2 = static_cast<float>(h->beta2);
  a.h.beta3 = static_cast<float>(h->beta3);
  a.h.omb1 = static_cast<float>(1.0 - h->beta1);
  a.h.omb2 = static_cast<float>(1.0 - h->beta2);
  a.h.omb3 = static_cast<float>(1.0 - h->beta3);
  a.h.bias1 = static_cast<float>(h->bias1);
  a.h.bias2 = static_cast<float>(h->bias2);
  a.h.bias3_sqrt = static_cast<float>(h->bias3_sqrt);
  a.h.lr = static_cast<float>(h->lr);
  a.h.eps = static_cast<float>(h->eps);
  a.h.no_prox = h->no_prox ? 1 : 0;
  a.h.decay = static_cast<float>(h->no_prox ? 1.0 - h->lr * h->weight_decay : 1.0 + h->lr * h->weight_decay);
  a.fresh = 0;
  int cnt = 0;
  int64_t grid = 0;
  auto flush = [&]() {
    if (grid > 0) {
      a.count = cnt;
      a.first[cnt] = static_cast<int32_t>(grid);
      hipLaunchKernelGGL(k_adan_step, dim3(static_cast<unsigned>(grid)), dim3(ADAN_BLOCK), 0, st, a);
    }
    a.fresh = 0;
    cnt = 0;
    grid = 0;
  };
  for (int i = 0; i < T; ++i) {
    if (t[i].numel == 0) continue;
    const int64_t c = (t[i].numel + ADAN_CHUNK - 1) / ADAN_CHUNK;
    if (cnt == ADAN_STEP_TENSORS || grid + c > ADAN_MAX_GRID) flush();
    a.p[cnt] = t[i].p;
    a.g[cnt] = t[i].g;
    a.m[cnt] = t[i].m;
    a.n[cnt] = t[i].n;
    a.d[cnt] = t[i].d;
    a.pg[cnt] = t[i].pg;
    a.numel[cnt] = t[i].numel;
    a.first[cnt] = static_cast<int32_t>(grid);
    if (t[i].fresh) a.fresh |= uint64_t(1) << cnt;
    ++cnt;
    grid += c;
  }
  flush();
  return check_launch("lcr_adan_step");
}
