// scan_overlap.hip — spherical range images of B stacked scans and the range-image overlap of P scan pairs: the labels behind "frame j
// overlaps frame i by more than 0.3" of the loop-detection evaluation.  Semantics in include/lcr_hip.h (lcr_range_images, lcr_scan_overlap).
//
// One workgroup of 1024 threads per image (a cloud, or a pair's projected cloud), the image held in LDS:
//   a 64 x 900 fp32 image is 230 KB and does not fit the 160 KiB of a CU, so the workgroup walks the image in bands of as many rows as fit
//   (43 at W = 900: two bands); per band it grid-strides over the cloud's points, transforms and projects each in fp64 and takes an
//   integer minimum on the fp32 bit pattern of the depth in LDS (ds_min_u32: order-free, so a pixel depends on no arrival order), then
//   sweeps the band: lcr_range_images stores it, lcr_scan_overlap compares it with the stored image of the pair's other scan and counts.
//   The row needs asin alone; atan2 (the column) is evaluated for the points of the current band only, so every point pays the transform,
//   the square root and asin once per band and atan2 once.  A pair therefore writes nothing but its three integers: no scratch image in
//   HBM, no global atomics (the status word aside), and the counts are plain stores after a fixed tree over the workgroup.
// The workspace holds the clouds' prefix offsets, written by stack_to_device (common.h), which also clears the status word.
#include <climits>
#include <cmath>

#include "common.h"
#include "grid.h"

namespace lcr {

constexpr int SO_THREADS = 1024;
constexpr int SO_MAX_H = 128, SO_MAX_W = 4096;
constexpr size_t SO_LDS_BYTES = 152 * 1024;      // band image; the rest of the 160 KiB is left to the static reduction arrays
constexpr uint32_t SO_EMPTY = 0xffffffffu;       // above the bit pattern of every non-negative float

struct SoProj {
  int    H, W;
  double afd, fov, max_range, eps;               // |fov_down| and |fov_up| + |fov_down| in radians
};

// One point through M (row-major 3x4) onto the H x W grid, as the header states it.  Returns false for a dropped point.  The row comes
// first; the column (atan2) only where the caller wants the row: rows r0 .. r0 + nr - 1.
__device__ __forceinline__ bool so_project(const float* __restrict__ p, const double* M, const SoProj& pr, int r0, int nr, int* pix, uint32_t* bits) {
  constexpr double PI = 3.14159265358979323846;
  const double x = static_cast<double>(p[0]), y = static_cast<double>(p[1]), z = static_cast<double>(p[2]);
  const double xt = dadd(dadd(dadd(dmul(M[0], x), dmul(M[1], y)), dmul(M[2], z)), M[3]);
  const double yt = dadd(dadd(dadd(dmul(M[4], x), dmul(M[5], y)), dmul(M[6], z)), M[7]);
  const double zt = dadd(dadd(dadd(dmul(M[8], x), dmul(M[9], y)), dmul(M[10], z)), M[11]);
  const double d = sqrt(dadd(dadd(dmul(xt, xt), dmul(yt, yt)), dmul(zt, zt)));
  if (!(d > 0.0 && d < pr.max_range)) return false;            // NaN and infinite coordinates end here
  double s = zt / d;
  s = s < -1.0 ? -1.0 : (s > 1.0 ? 1.0 : s);
  const double pitch = asin(s);
  const double v = dmul(1.0 - dadd(pitch, pr.afd) / pr.fov, static_cast<double>(pr.H));
  double fr = floor(v);
  fr = !(fr >= 0.0) ? 0.0 : (fr > static_cast<double>(pr.H - 1) ? static_cast<double>(pr.H - 1) : fr);
  const int row = static_cast<int>(fr);
  if (row < r0 || row >= r0 + nr) return false;
  const double yaw = -atan2(yt, xt);
  const double u = dmul(dmul(0.5, dadd(yaw / PI, 1.0)), static_cast<double>(pr.W));
  double fc = floor(u);
  fc = !(fc >= 0.0) ? 0.0 : (fc > static_cast<double>(pr.W - 1) ? static_cast<double>(pr.W - 1) : fc);
  *pix = (row - r0) * pr.W + static_cast<int>(fc);
  *bits = __float_as_uint(static_cast<float>(d));
  return true;
}

// sum of a and of b over the workgroup, valid in thread 0 (a fixed tree: wavefront sums, then the 16 wavefronts in order)
__device__ __forceinline__ void so_block_sum2(int& a, int& b) {
  __shared__ int s_red[SO_THREADS / 64][2];
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane_id() == 0) {
    s_red[threadIdx.x >> 6][0] = a;
    s_red[threadIdx.x >> 6][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = 0;
    b = 0;
    for (int w = 0; w < SO_THREADS / 64; ++w) {
      a += s_red[w][0];
      b += s_red[w][1];
    }
  }
}

// PAIR = false: workgroup b projects cloud b through the identity and stores images[b], valid[b].
// PAIR = true:  workgroup p projects cloud j = pairs[p][1] through rel[p], compares with images[i = pairs[p][0]] and stores counts[p].
template <bool PAIR>
__global__ __launch_bounds__(SO_THREADS) void k_so_image(const float* __restrict__ points, const int64_t* __restrict__ off, int B, SoProj pr,
                                                         int band_rows, float* __restrict__ images_out, int32_t* __restrict__ valid_out,
                                                         const float* __restrict__ images, const int32_t* __restrict__ valid,
                                                         const int32_t* __restrict__ pairs, const double* __restrict__ rel,
                                                         int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  extern __shared__ uint32_t s_img[];
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x;
  int ci = 0, cj = static_cast<int>(p);
  double M[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  if (PAIR) {
    ci = pairs[2 * p];
    cj = pairs[2 * p + 1];
    if (ci < 0 || ci >= B || cj < 0 || cj >= B) {               // block-uniform: nothing of the pair is read
      if (tid == 0) {
        counts[3 * p] = counts[3 * p + 1] = counts[3 * p + 2] = -1;
        atomicMax(status, static_cast<int32_t>(p < INT32_MAX ? p + 1 : INT32_MAX));
      }
      return;
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) M[e] = rel[12 * p + e];
  }
  const int64_t n0 = off[cj], n1 = off[cj + 1];
  const size_t image = static_cast<size_t>(pr.H) * pr.W;
  int n_valid = 0, n_match = 0;
  for (int r0 = 0; r0 < pr.H; r0 += band_rows) {
    const int nr = pr.H - r0 < band_rows ? pr.H - r0 : band_rows;
    const int npix = nr * pr.W;
    for (int k = tid; k < npix; k += SO_THREADS) s_img[k] = SO_EMPTY;
    __syncthreads();
    for (int64_t q = n0 + tid; q < n1; q += SO_THREADS) {
      int pix;
      uint32_t bits;
      if (so_project(points + 3 * q, M, pr, r0, nr, &pix, &bits)) atomicMin(&s_img[pix], bits);
    }
    __syncthreads();
    const size_t base = static_cast<size_t>(r0) * pr.W;
    for (int k = tid; k < npix; k += SO_THREADS) {
      const uint32_t a = s_img[k];
      const bool have = a != SO_EMPTY;
      n_valid += have ? 1 : 0;
      if (PAIR) {
        const float b = images[static_cast<size_t>(ci) * image + base + k];
        if (have && b >= 0.f && fabs(static_cast<double>(__uint_as_float(a)) - static_cast<double>(b)) < pr.eps) ++n_match;
      } else {
        images_out[static_cast<size_t>(cj) * image + base + k] = have ? __uint_as_float(a) : -1.f;
      }
    }
    __syncthreads();                                             // the band is re-initialised next
  }
  so_block_sum2(n_valid, n_match);
  if (tid == 0) {
    if (PAIR) {
      counts[3 * p] = n_match;
      counts[3 * p + 1] = valid[ci];
      counts[3 * p + 2] = n_valid;
    } else {
      valid_out[cj] = n_valid;
    }
  }
}

}  // namespace lcr

using namespace lcr;

namespace {

constexpr double SO_PI = 3.14159265358979323846;

// the shared domain checks; fills pr and the band height
int so_params(const char* who, int H, int W, double fov_up, double fov_down, double max_range, double eps, SoProj* pr, int* band_rows) {
  const double fu = fov_up * SO_PI / 180.0, fd = fov_down * SO_PI / 180.0;
  const double fov = std::fabs(fu) + std::fabs(fd);
  if (H < 1 || H > SO_MAX_H || W < 1 || W > SO_MAX_W || !(max_range > 0.0) || !(eps > 0.0) || !(fov > 0.0) ||
      !std::isfinite(fov))
    return refuse(LCR_EARG, "%s: outside the domain (1 <= H <= %d, 1 <= W <= %d, max_range > 0, eps > 0, |fov_up| + |fov_down| > 0 and finite): H=%d W=%d "
                  "fov_up=%g fov_down=%g max_range=%g eps=%g", who, SO_MAX_H, SO_MAX_W, H, W, fov_up, fov_down, max_range, eps);
  pr->H = H;
  pr->W = W;
  pr->afd = std::fabs(fd);
  pr->fov = fov;
  pr->max_range = max_range;
  pr->eps = eps;
  const int fit = static_cast<int>(SO_LDS_BYTES / (sizeof(uint32_t) * static_cast<size_t>(W)));      // >= 9 at W = 4096
  *band_rows = fit < H ? fit : H;
  return LCR_OK;
}

size_t so_ws_bytes(int B) { return align_up(sizeof(int64_t) * static_cast<size_t>(B + 1)); }

template <bool PAIR>
int so_launch(const char* who, int64_t blocks, const float* points, const int64_t* off, int B, const SoProj& pr, int band_rows, float* images_out,
              int32_t* valid_out, const float* images, const int32_t* valid, const int32_t* pairs, const double* rel, int32_t* counts,
              int32_t* status, hipStream_t st) {
  const size_t lds = sizeof(uint32_t) * static_cast<size_t>(band_rows) * pr.W;
  static DynLds opt_in;                                          // > 64 KB of dynamic LDS needs an explicit opt-in
  if (lds > 48 * 1024 && opt_in.need(reinterpret_cast<const void*>(&k_so_image<PAIR>), SO_LDS_BYTES) != hipSuccess)
    return refuse(LCR_EHIP, "%s: cannot opt in to %zu bytes of LDS", who, SO_LDS_BYTES);
  hipLaunchKernelGGL(k_so_image<PAIR>, dim3(static_cast<unsigned>(blocks)), dim3(SO_THREADS), lds, st, points, off, B, pr, band_rows, images_out,
                     valid_out, images, valid, pairs, rel, counts, status);
  return check_launch(who);
}

}  // namespace

extern "C" int lcr_range_images_ws_bytes(int B, size_t* bytes) {
  if (!bytes || B < 1 || B > GRID_MAX_B) return refuse(LCR_EARG, "lcr_range_images_ws_bytes: outside the domain (1 <= B <= %d, bytes non-null): B=%d", GRID_MAX_B, B);
  *bytes = so_ws_bytes(B);
  return LCR_OK;
}

extern "C" int lcr_range_images(const float* points, const int64_t* lengths, int B, int H, int W, double fov_up, double fov_down, double max_range,
                                float* images, int32_t* valid, void* ws, size_t ws_bytes, void* stream) {
  SoProj pr;
  int band_rows = 0;
  int rc = so_params("lcr_range_images", H, W, fov_up, fov_down, max_range, 1.0, &pr, &band_rows);
  if (rc) return rc;
  if (!images || !valid || !ws) return refuse(LCR_EARG, "lcr_range_images: null pointer");
  Stack C;
  rc = stack_from_lengths("lcr_range_images", lengths, B, &C);
  if (rc) return rc;
  const int64_t n = C.off[B];
  if (n > 0 && !points) return refuse(LCR_EARG, "lcr_range_images: null point array (n=%lld)", static_cast<long long>(n));
  if (so_ws_bytes(B) > ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_range_images", ws_bytes, so_ws_bytes(B));
  hipStream_t st = static_cast<hipStream_t>(stream);
  int64_t* off = static_cast<int64_t*>(ws);
  rc = stack_to_device("lcr_range_images", C, nullptr, off, nullptr, st);
  if (rc) return rc;
  return so_launch<false>("lcr_range_images", B, points, off, B, pr, band_rows, images, valid, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          st);
}

extern "C" int lcr_scan_overlap_ws_bytes(int B, int64_t P, size_t* bytes) {
  if (!bytes || B < 1 || B > GRID_MAX_B || P < 0 || P > INT32_MAX)
    return refuse(LCR_EARG, "lcr_scan_overlap_ws_bytes: outside the domain (1 <= B <= %d, 0 <= P <= 2^31-1, bytes non-null): B=%d P=%lld", GRID_MAX_B, B,
                  static_cast<long long>(P));
  *bytes = so_ws_bytes(B);
  return LCR_OK;
}

extern "C" int lcr_scan_overlap(const float* points, const int64_t* lengths, int B, const float* images, const int32_t* valid, const int32_t* pairs,
                                const double* rel, int64_t P, int H, int W, double fov_up, double fov_down, double max_range, double eps,
                                int32_t* counts, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (P < 0 || P > INT32_MAX) return refuse(LCR_EARG, "lcr_scan_overlap: outside the domain (0 <= P <= 2^31-1): P=%lld", static_cast<long long>(P));
  if (P == 0) return LCR_OK;
  SoProj pr;
  int band_rows = 0;
  int rc = so_params("lcr_scan_overlap", H, W, fov_up, fov_down, max_range, eps, &pr, &band_rows);
  if (rc) return rc;
  if (!images || !valid || !pairs || !rel || !counts || !status || !ws) return refuse(LCR_EARG, "lcr_scan_overlap: null pointer");
  Stack C;
  rc = stack_from_lengths("lcr_scan_overlap", lengths, B, &C);
  if (rc) return rc;
  const int64_t n = C.off[B];
  if (n > 0 && !points) return refuse(LCR_EARG, "lcr_scan_overlap: null point array (n=%lld)", static_cast<long long>(n));
  if (so_ws_bytes(B) > ws_bytes) return refuse_ws(LCR_ESPACE, "lcr_scan_overlap", ws_bytes, so_ws_bytes(B));
  hipStream_t st = static_cast<hipStream_t>(stream);
  int64_t* off = static_cast<int64_t*>(ws);
  rc = stack_to_device("lcr_scan_overlap", C, nullptr, off, status, st);
  if (rc) return rc;
  return so_launch<true>("lcr_scan_overlap", P, points, off, B, pr, band_rows, nullptr, nullptr, images, valid, pairs, rel, counts, status, st);
}
