// augment.hip — training-time augmentation and point-limit sampling of stacked clouds (include/lcr_hip.h, lcr_augment_clouds): what the
// reference's dataset classes do per cloud in NumPy (datasets/registration/kitti/dataset.py:73-115 `_augment_point_cloud` /
// `_load_point_cloud`, datasets/loop_detection/kitti/dataset_overlap_online.py:123-153), for up to 128 clouds in one call.
//
//   header  (1 workgroup)   offsets of the input and output stacks from the device-side lengths, out_len = min(L, limit)
//   keys    (limit > 0)     key = cloud << 32 | (Philox word 0 of stream 1 & mask), value = stacked row
//   sort    (limit > 0)     ONE stable radix sort (radix_sort.h): inside a cloud the rows end up in ascending (word, original index)
//   apply                   one lane per OUTPUT row: picks its source row (identity for a cloud within the limit, else the sorted
//                           value), draws the noise from the SOURCE index and writes the augmented point — no stacked intermediate
//
// Every random word is a pure function of (seed, sample_id, original index, stream), so a cloud gives the same bytes alone and in any
// stack, and a point's augmented value does not depend on the limit.  No atomics on data, no floating-point atomics at all.
#include "radix_sort.h"

namespace lcr {

constexpr int AUG_MAX_B = 128;   // clouds per call: the training head's own cap (S <= 128 segments)

struct AugHeader {
  RadixCtl rx;                   // n, num_passes (first: the radix kernels read it)
  int      B;
  int64_t  in_off[AUG_MAX_B + 1];
  int64_t  out_off[AUG_MAX_B + 1];
  int32_t  cut[AUG_MAX_B];       // 1: the cloud is longer than the limit and takes its rows from the sort
};

struct AugLayout {
  AugHeader* hdr;
  uint64_t * keyA, *keyB;
  uint32_t * valA, *valB;
  int32_t*   hist;
  void*      scan_ws;
  size_t     bytes;
};

static AugLayout aug_layout(void* ws, int64_t n_cap, bool select) {
  AugLayout L{};
  Carver c(ws, ~size_t(0));
  L.hdr = c.take<AugHeader>(1);
  if (select) {
    const size_t n = static_cast<size_t>(n_cap > 0 ? n_cap : 1);
    L.keyA = c.take<uint64_t>(n);
    L.keyB = c.take<uint64_t>(n);
    L.valA = c.take<uint32_t>(n);
    L.valB = c.take<uint32_t>(n);
    L.hist = c.take<int32_t>(radix_hist_elems(n_cap));
    L.scan_ws = c.take<char>(scan_ws_bytes(static_cast<int64_t>(radix_hist_elems(n_cap))));
  }
  L.bytes = c.off;
  return L;
}

static std::atomic<uint32_t> g_aug_select_mask{0xFFFFFFFFu};

// ---- Philox4x32-10 (Salmon et al., SC'11): the standard multipliers and Weyl key increments -----------------------------------------
struct Philox4 {
  uint32_t w[4];
};
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

constexpr uint32_t AUG_STREAM_NOISE = 0, AUG_STREAM_SELECT = 1;

__device__ __forceinline__ float aug_uniform(uint32_t word) { return static_cast<float>(word >> 8) * 5.9604644775390625e-8f; }   // 24 bits, exact

// one workgroup; the lengths are few (<= 128): a serial walk by one lane, as k_gs_init does
__global__ void k_aug_header(AugHeader* h, const int64_t* __restrict__ len, int B, int64_t n_cap, int64_t out_cap, int64_t limit, int cbits,
                             int64_t* __restrict__ out_len, uint32_t* status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t o = 0, q = 0;
  bool cut = false, bad = false;
  for (int b = 0; b < B; ++b) {
    int64_t l = len[b];
    if (l < 0) {
      l = 0;
      bad = true;
    }
    if (l > n_cap - o) {                       // lengths that overrun the capacity are reported and clamped
      l = n_cap - o;
      bad = true;
    }
    int64_t m = limit > 0 && l > limit ? limit : l;
    h->cut[b] = m < l;
    cut |= m < l;
    if (m > out_cap - q) {                     // so are output rows beyond what the caller allocated
      m = out_cap - q;
      bad = true;
    }
    h->in_off[b] = o;
    h->out_off[b] = q;
    out_len[b] = m;
    o += l;
    q += m;
  }
  h->in_off[B] = o;
  h->out_off[B] = q;
  h->B = B;
  h->rx.n = o;
  h->rx.num_passes = cut ? radix_passes(32 + cbits) : 0;    // nothing to select: every sort launch exits at once
  if (bad) atomicOr(status, LCR_STATUS_LEN_MISMATCH);
}

// offsets of the stack to LDS, then the cloud of a row by bisection (128 clouds: a linear walk per lane would dominate the kernel)
__device__ __forceinline__ void aug_load_offsets(const int64_t* __restrict__ off, int B, int64_t* s_off) {
  for (int b = threadIdx.x; b <= B; b += blockDim.x) s_off[b] = off[b];
  __syncthreads();
}
__device__ __forceinline__ int aug_cloud_of(const int64_t* s_off, int B, int64_t i) {
  int lo = 0, hi = B - 1;                      // last b with s_off[b] <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (s_off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_aug_keys(const AugHeader* __restrict__ h, const uint32_t* __restrict__ sample_id, uint32_t k0, uint32_t k1,
                                                  uint32_t mask, uint64_t* __restrict__ keyA, uint32_t* __restrict__ valA) {
  __shared__ int64_t s_off[AUG_MAX_B + 1];
  const int B = h->B;
  aug_load_offsets(h->in_off, B, s_off);
  if (h->rx.num_passes == 0) return;           // no cloud is cut: the apply kernel never reads the sort buffers
  const int64_t n = h->rx.n;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int b = aug_cloud_of(s_off, B, i);
    const uint32_t idx = static_cast<uint32_t>(i - s_off[b]);
    const Philox4 r = philox4x32_10(idx, 0u, sample_id[b], AUG_STREAM_SELECT, k0, k1);
    keyA[i] = (static_cast<uint64_t>(b) << 32) | (r.w[0] & mask);
    valA[i] = static_cast<uint32_t>(i);
  }
}

__global__ __launch_bounds__(256) void k_aug_apply(const AugHeader* __restrict__ h, const float* __restrict__ rows, int rs,
                                                   const uint32_t* __restrict__ sample_id, const float* __restrict__ rotation,
                                                   const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ noise,
                                                   uint32_t k0, uint32_t k1, const uint32_t* __restrict__ vA, const uint32_t* __restrict__ vB,
                                                   float* __restrict__ out) {
  __shared__ int64_t s_in[AUG_MAX_B + 1], s_out[AUG_MAX_B + 1];
  __shared__ int32_t s_cut[AUG_MAX_B];
  const int B = h->B;
  for (int b = threadIdx.x; b <= B; b += blockDim.x) {
    s_in[b] = h->in_off[b];
    s_out[b] = h->out_off[b];
    if (b < B) s_cut[b] = h->cut[b];
  }
  __syncthreads();
  const int64_t m = s_out[B];
  const uint32_t* sorted = (h->rx.num_passes & 1) ? vB : vA;
  for (int64_t j = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; j < m; j += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int b = aug_cloud_of(s_out, B, j);
    const int64_t k = j - s_out[b];                                   // position inside the output cloud
    // a cloud within the limit passes through in order; a cut one takes the k-th smallest (word, index) of its slice of the sort
    // (the flag, not the lengths: rows clamped to the caller's output capacity are a prefix, and no sort ran for them)
    const int64_t src = s_cut[b] ? static_cast<int64_t>(sorted[s_in[b] + k]) : s_in[b] + k;
    const float* p = rows + static_cast<int64_t>(rs) * src;           // columns 3 .. rs-1 are never read
    const Philox4 u = philox4x32_10(static_cast<uint32_t>(src - s_in[b]), 0u, sample_id[b], AUG_STREAM_NOISE, k0, k1);
    const float amp = noise[b], sc = scale[b];
    const float* R = rotation + 9 * b;
    const float* t = shift + 3 * b;
    float q[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) q[d] = fadd(p[d], fmul(fsub(aug_uniform(u.w[d]), 0.5f), amp));
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float r = fadd(fadd(fmul(R[3 * d + 0], q[0]), fmul(R[3 * d + 1], q[1])), fmul(R[3 * d + 2], q[2]));
      out[3 * j + d] = fadd(fmul(r, sc), t[d]);
    }
  }
}

}  // namespace lcr

using namespace lcr;

extern "C" void lcr_augment_debug_select_mask(uint32_t mask) { g_aug_select_mask.store(mask, std::memory_order_relaxed); }

static int aug_check_shape(const char* who, int B, int64_t n_cap) {
  if (B < 1 || B > AUG_MAX_B) return refuse(LCR_EARG, "%s: %d clouds (1 .. %d per call)", who, B, AUG_MAX_B);
  if (n_cap < 0 || n_cap > (int64_t(1) << 31) - 2) return refuse(LCR_EARG, "%s: capacity of %lld rows (0 .. 2^31-2)", who, static_cast<long long>(n_cap));
  return LCR_OK;
}

extern "C" int lcr_augment_clouds_ws_bytes(int64_t n_cap, int B, int64_t limit, size_t* bytes) {
  if (!bytes) return refuse(LCR_EARG, "lcr_augment_clouds_ws_bytes: null size pointer");
  const int rc = aug_check_shape("lcr_augment_clouds_ws_bytes", B, n_cap);
  if (rc) return rc;
  *bytes = aug_layout(nullptr, n_cap, limit > 0).bytes;
  return LCR_OK;
}

extern "C" int lcr_augment_clouds(const float* rows, int row_floats, const int64_t* len, int B, int64_t n_cap, const uint32_t* sample_id,
                                  const float* rotation, const float* scale, const float* shift, const float* noise, uint64_t seed,
                                  int64_t limit, float* out_xyz, int64_t out_cap, int64_t* out_len, uint32_t* status, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (row_floats < 3 || row_floats > 64) return refuse(LCR_EARG, "lcr_augment_clouds: rows of %d floats (3 .. 64: x, y, z first)", row_floats);
  const int rc = aug_check_shape("lcr_augment_clouds", B, n_cap);
  if (rc) return rc;
  if (out_cap < 0 || out_cap > n_cap)
    return refuse(LCR_EARG, "lcr_augment_clouds: output capacity of %lld rows (0 .. n_cap = %lld)", static_cast<long long>(out_cap), static_cast<long long>(n_cap));
  if (!len || !sample_id || !rotation || !scale || !shift || !noise || !out_len || !status || !ws || (n_cap > 0 && !rows) || (out_cap > 0 && !out_xyz))
    return refuse(LCR_EARG, "lcr_augment_clouds: null argument");
  const bool select = limit > 0;
  const AugLayout L = aug_layout(ws, n_cap, select);
  if (L.bytes > ws_bytes) {                    // refused like every other argument of this entry: nothing is launched
    return refuse(LCR_EARG, "lcr_augment_clouds: workspace too small (%zu < %zu)", ws_bytes, L.bytes);
  }
  hipStream_t st = ST(stream);
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  int cbits = 0;
  while ((1 << cbits) < B) ++cbits;
  hipLaunchKernelGGL(k_aug_header, dim3(1), dim3(64), 0, st, L.hdr, len, B, n_cap, out_cap, limit, cbits, out_len, status);
  if (n_cap == 0 || out_cap == 0) return check_launch("lcr_augment_clouds");
  if (select) {
    hipLaunchKernelGGL(k_aug_keys, dim3(blocks_for(n_cap, 256, 2048)), dim3(256), 0, st, L.hdr, sample_id, k0, k1,
                       g_aug_select_mask.load(std::memory_order_relaxed), L.keyA, L.valA);
    const int src = radix_sort_pairs("lcr_augment_clouds", &L.hdr->rx, L.keyA, L.keyB, L.valA, L.valB, n_cap, radix_passes(32 + cbits), L.hist, L.scan_ws, st);
    if (src) return src;
  }
  hipLaunchKernelGGL(k_aug_apply, dim3(blocks_for(out_cap, 256, 2048)), dim3(256), 0, st, L.hdr, rows, row_floats, sample_id, rotation, scale, shift,
                     noise, k0, k1, L.valA, L.valB, out_xyz);
  return check_launch("lcr_augment_clouds");
}
