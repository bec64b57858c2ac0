// grid.h — the uniform support grid of radius_search.hip (lcr_support_grid_build), shared with the kernels that query it directly
// (icp.hip).  Layout: per cloud a box of dim[0] x dim[1] x dim[2] cells (cell >= radius), cell-sorted supports as float4
// (x, y, z, bits(global row)), cell_start[] the exclusive prefix of the per-cell counts.
#pragma once
#include "common.h"

namespace lcr {

constexpr int GRID_MAX_B = 64;   // clouds per call
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

}  // namespace lcr
