// grid.h — the uniform support grid of radius_search.hip (lcr_support_grid_build), shared with the kernels that query it directly:
// icp.hip (nearest partner) and normals.hip (hybrid neighbourhood) walk its cells through grid_for_each_run; fpfh.hip queries it
// through lcr_radius_query_ordered.  All of them take d² and the (d², row) key from grid_d2 / grid_key below.
// Layout: per cloud a box of dim[0] x dim[1] x dim[2] cells (cell >= radius), cell-sorted supports as float4
// (x, y, z, bits(global row)), cell_start[] the exclusive prefix of the per-cell counts.
#pragma once
#include "common.h"

namespace lcr {

// The bodies of lcr_support_grid_ws_bytes, lcr_support_grid_build{,_ex} and lcr_radius_query{,_ordered} (radius_search.hip), for the
// entry points that build or query a grid of their own: a refusal carries the name `who` of the entry point that was called.
int support_grid_ws_bytes(const char* who, int64_t ns_cap, int B, size_t* bytes);
int support_grid_build(const char* who, const float* s, const int64_t* slen, int B, int64_t ns_cap, float radius, uint32_t* status, void* grid_ws,
                       size_t grid_ws_bytes, int32_t* order, void* stream);
int radius_query(const char* who, const float* q, const int64_t* qlen, int B, int64_t nq_cap, const void* grid_ws, int64_t ns_cap, float radius,
                 int limit, int64_t* out_idx64, int32_t* out_idx32, int32_t* out_cnt, const int32_t* q_order, void* stream);

constexpr int CELL_PER_PT = 32;  // cell budget = CELL_PER_PT * ns_cap + CELL_MIN * B
constexpr int CELL_MIN = 4096;

struct GridCloud {
  double  org[3];
  double  inv_cell;
  int     dim[3];
  int     cell_base;   // first cell of this cloud in the global cell arrays
  int64_t s_start;     // first support row of this cloud
};

struct GridHeader {
  int       B;
  int       n_cells;     // cells in use (<= cell_cap)
  int64_t   ns_total;    // sum(slen)
  int64_t   ns_cap;
  int64_t   cell_cap;
  GridCloud cloud[GRID_MAX_B];
  uint32_t  bb_min[GRID_MAX_B][3];   // order-preserving encodings
  uint32_t  bb_max[GRID_MAX_B][3];
  int64_t   s_off[GRID_MAX_B + 1];
};

struct GridLayout {
  GridHeader* hdr;
  int32_t*    cell_cnt;     // [cell_cap]   (zero before and after build)
  int32_t*    cell_start;   // [cell_cap+1]
  int32_t*    pt_cell;      // [ns_cap]
  float4*     sorted;       // [ns_cap]  x,y,z,bits(idx global)
  void*       scan_ws;
  size_t      bytes;
};

static GridLayout grid_layout(void* ws, int64_t ns_cap, int B) {
  GridLayout L;
  Carver c(ws, ~size_t(0));
  const int64_t cell_cap = CELL_PER_PT * ns_cap + static_cast<int64_t>(CELL_MIN) * B;
  L.hdr = c.take<GridHeader>(1);
  L.cell_cnt = c.take<int32_t>(cell_cap);
  L.cell_start = c.take<int32_t>(cell_cap + 1);
  L.pt_cell = c.take<int32_t>(ns_cap > 0 ? ns_cap : 1);
  L.sorted = c.take<float4>(ns_cap > 0 ? ns_cap : 1);
  L.scan_ws = c.take<char>(scan_ws_bytes(cell_cap + 1));
  L.bytes = c.off;
  return L;
}

__device__ __forceinline__ int cell_coord(double p, double org, double inv_cell, int dim) {
  // clamp in floating point first: queries may lie far outside the support box
  double c = floor((p - org) * inv_cell);
  c = fmin(fmax(c, -2.0), static_cast<double>(dim) + 1.0);
  return static_cast<int>(c);
}

// The supports that query q of cloud c sees: the cells of cell_coord() (clamped to [-2, dim+1]) and their 3x3x3 neighbourhood inside
// the box, as up to nine x-runs of consecutive sorted rows, zz outer and yy inner.  k_radius_query's setup starts from the same cells
// (it then drops runs that lie out of the ball's reach, which hold no hit); a change of the layout has to reach both.
// fn(k_begin, k_end) once per run; nothing for a query whose x range misses the box, which covers an empty cloud (dim[0] == 0: x1 = -1).
template <typename F>
__device__ __forceinline__ void grid_for_each_run(const GridCloud& c, const int32_t* cell_start, float qx, float qy, float qz, F&& fn) {
  const int cx = cell_coord(qx, c.org[0], c.inv_cell, c.dim[0]);
  const int cy = cell_coord(qy, c.org[1], c.inv_cell, c.dim[1]);
  const int cz = cell_coord(qz, c.org[2], c.inv_cell, c.dim[2]);
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, c.dim[0] - 1);
  if (x0 <= x1) {
    for (int zz = max(cz - 1, 0); zz <= min(cz + 1, c.dim[2] - 1); ++zz)
      for (int yy = max(cy - 1, 0); yy <= min(cy + 1, c.dim[1] - 1); ++yy) {
        const int crow = c.cell_base + (zz * c.dim[1] + yy) * c.dim[0];
        const int k_end = cell_start[crow + x1 + 1];
        fn(cell_start[crow + x0], k_end);
      }
  }
}

// d² = ((dx*dx + dy*dy) + dz*dz) of query q and support p with every operation rounded (never contracted), and the (d², row) key the
// searches order by: the bits every consumer of the grid must agree on
__device__ __forceinline__ float grid_d2(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = fsub(qx, px), dy = fsub(qy, py), dz = fsub(qz, pz);
  return fadd(fadd(fmul(dx, dx), fmul(dy, dy)), fmul(dz, dz));
}
__device__ __forceinline__ float grid_d2(float qx, float qy, float qz, const float4& p) { return grid_d2(qx, qy, qz, p.x, p.y, p.z); }
__device__ __forceinline__ uint64_t grid_key(float d2, float row_bits) {
  return (static_cast<uint64_t>(__float_as_uint(d2)) << 32) | __float_as_uint(row_bits);
}

}  // namespace lcr
