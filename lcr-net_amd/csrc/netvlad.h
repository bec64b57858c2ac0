// netvlad.h — what the two files of the global-descriptor head share: netvlad.hip (the forward, eval and training) and
// netvlad_grad.hip (the reverse pass).  Every kernel both need is defined once, in netvlad.hip, behind a host launcher declared here.
#pragma once
#include <vector>

#include "common.h"

extern "C" int lcr_gemm_f32(const float* A, const float* B, float* C, int64_t M, int N, int K, int transA, int transB, const float* bias,
                            const float* rowdiv, const int64_t* seg_len, int S, int groups, double* stats, void* stream);
extern "C" int lcr_gemm_f32_batched_ta(const float* A, const float* B, float* C, int64_t M, int N, int count, const int* k_host,
                                       const int64_t* a_off_host, const int64_t* b_off_host, const int64_t* c_off_host, void* stream);

namespace lcr {
namespace nv {

constexpr int F = 1024;          // feature size
constexpr int K = 64;            // clusters
constexpr int D = 256;           // output dim
constexpr int FK = F * K;        // 65536 rows of hidden1_weights
constexpr int SPLIT = 256;       // K-slices of the forward hidden projection (FK / SPLIT = 256 rows each)
constexpr int S_MAX = 128;       // clouds per offset window, and per training call
constexpr int STAT_G = 128;      // workgroups of the bn1 column sums
constexpr float BN_EPS = 1e-5f;

struct Seg {                     // row offsets of a window of S clouds (+ its end), by value in kernel arguments
  int S, Lmax;                   // Lmax: the longest cloud of the whole call
  int64_t off[S_MAX + 1];
};

// seg_len_host[S] -> off[0..S], exclusive row offsets with off[S] = total rows, and the longest length.  The domain is checked before
// anything is launched: s_min <= S (<= s_max unless s_max is 0), every length >= 1, total <= 2^31-1.  LCR_OK, or the error text in the
// name of entry point `who` and LCR_EARG.  No HIP call.
int seg_offsets(const char* who, const int64_t* seg_len_host, int S, int s_min, int s_max, std::vector<int64_t>* off, int* Lmax);

inline Seg seg_window(const std::vector<int64_t>& off, int s0, int count, int Lmax) {   // clouds s0 .. s0 + count - 1, count <= S_MAX
  Seg seg;
  seg.S = count;
  seg.Lmax = Lmax;
  std::copy(off.begin() + s0, off.begin() + s0 + count + 1, seg.off);
  return seg;
}

// What the training forward keeps for the reverse pass.  Opaque to callers, but its size is part of the ABI.
struct Saved {
  float *a, *sm, *v, *n1raw, *n2raw, *asum, *hh, *hp, *gh, *g, *out, *tn, *mu1, *r1, *r2, *rg;
  int32_t *cmul, *rseg;
  size_t bytes;
};
inline Saved saved_layout(void* p, int64_t n_rows, int S) {
  Saved L;
  Carver c(p, ~size_t(0));
  const size_t rows = static_cast<size_t>(std::max<int64_t>(n_rows, 1)), s = static_cast<size_t>(S);
  L.a = c.take<float>(rows * K);
  L.sm = c.take<float>(rows * K);
  L.cmul = c.take<int32_t>(rows);
  L.rseg = c.take<int32_t>(rows);
  L.v = c.take<float>(s * FK);
  L.n1raw = c.take<float>(s * K);
  L.n2raw = c.take<float>(s);
  L.asum = c.take<float>(s * K);
  L.hh = c.take<float>(s * D);
  L.hp = c.take<float>(s * D);
  L.gh = c.take<float>(s * D);
  L.g = c.take<float>(s * D);
  L.out = c.take<float>(s * D);
  L.tn = c.take<float>(s);
  L.mu1 = c.take<float>(K);
  L.r1 = c.take<float>(K);
  L.r2 = c.take<float>(D);
  L.rg = c.take<float>(D);
  L.bytes = c.off;
  return L;
}

inline int row_blocks(int64_t N) { return static_cast<int>(std::min<int64_t>((N + 3) / 4, 256 * 16)); }      // wavefront-per-row kernels
inline int stat_blocks(int64_t N) { return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(STAT_G, (N + 63) / 64))); }

// y[n] = x[n] / max(|x[n]|, 1e-12) for the N rows of x [N, F]
void launch_row_l2norm(const float* x, int64_t N, float* y, hipStream_t st);

}  // namespace nv
}  // namespace lcr
