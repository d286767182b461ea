// The DSM lattice (SnerfDsmGrid, include/snerf_hip.h) as csrc/dsm.hip and csrc/ortho.hip share it: which cells a point offers
// itself to, and the host-side checks of a grid and of a quantisation (z0, q).  Every splat on this lattice goes through
// cell_window(); nothing here depends on what a kernel does with the cells.
#pragma once
#include "common.h"
#include "../../include/snerf_hip.h"

#include <math.h>

namespace snerf {

// The cells a point offers itself to: the (2r+1)^2 window round its own cell, clipped to the lattice extent and to the output
// window BEFORE any conversion to an integer (a NaN or infinite coordinate fails the comparisons and offers nothing).
struct CellWindow {
  long long i0, i1, j0, j1;      // lattice cells [i0, i1) x [j0, j1); empty when i0 >= i1 or j0 >= j1
};

__device__ __forceinline__ CellWindow cell_window(double x, double y, const SnerfDsmGrid& g, int r) {
  CellWindow w = {0, 0, 0, 0};
  const double fi = floor((x - g.xoff) / g.res), fj = floor((g.yoff - y) / g.res);
  const double lo_i = fmax((double)g.ioff, 0.0), hi_i = fmin((double)g.ioff + g.out_w, (double)g.xsize);
  const double lo_j = fmax((double)g.joff, 0.0), hi_j = fmin((double)g.joff + g.out_h, (double)g.ysize);
  if (!(fi + r >= lo_i && fi - r < hi_i && fj + r >= lo_j && fj - r < hi_j)) return w;
  // fi, fj now lie within r of [0, 2^31): exact as 64-bit integers
  const long long ci = (long long)fi, cj = (long long)fj;
  const long long li = (long long)lo_i, hi = (long long)hi_i, lj = (long long)lo_j, hj = (long long)hi_j;
  w.i0 = ci - r > li ? ci - r : li;
  w.i1 = ci + r + 1 < hi ? ci + r + 1 : hi;
  w.j0 = cj - r > lj ? cj - r : lj;
  w.j1 = cj + r + 1 < hj ? cj + r + 1 : hj;
  return w;
}

// The 64-bit key of a point on this lattice, as snerf_ortho_top (csrc/ortho.hip) and the fuse entries (csrc/fuse.hip) share it:
// (quantised altitude + 2^31) << 32 | (2^32 - 1 - global index), the quantised altitude rint((z - z0) / q) in [-2^31, 2^31).
// false (and no key) for an altitude whose quantised value is not finite or out of range.  Ascending keys are ascending
// altitudes and, at one altitude, descending indices; no key is 0.
constexpr long long LATTICE_MAX_CELLS = 1LL << 31;       // a raster or a window has FEWER cells: a cell index is an int32
constexpr long long LATTICE_MAX_POINTS = LATTICE_MAX_CELLS;   // a call takes AT MOST as many points or segments (n in [0, 2^31])
constexpr long long ORTHO_MAX_INDEX = 4294967295LL;      // 2^32 - 1: index0 + n may not exceed it

__device__ __forceinline__ bool lattice_key(double z, double z0, double q, unsigned long long index, unsigned long long* key) {
  const double kq = rint((z - z0) / q);
  if (!(kq >= -2147483648.0 && kq < 2147483648.0)) return false;
  *key = ((unsigned long long)((long long)kq + 2147483648LL) << 32) | (0xFFFFFFFFull - index);
  return true;
}

// the grid of an accumulating entry: res > 0, finite offsets, positive sizes
static inline bool lattice_grid_ok(const char* who, const SnerfDsmGrid* g) {
  if (g->res > 0.0 && isfinite(g->res) && isfinite(g->xoff) && isfinite(g->yoff) && g->xsize > 0 && g->ysize > 0 && g->out_w > 0 &&
      g->out_h > 0)
    return true;
  set_error("%s: grid needs res > 0 and positive sizes", who);
  return false;
}

// a window whose cells are int32 indices (the ortho entries refuse any other; snerf_dsm_accumulate does not)
static inline bool lattice_window_fits_int32(const char* who, const SnerfDsmGrid* g) {
  if ((long long)g->ioff + g->out_w <= 2147483647LL && (long long)g->joff + g->out_h <= 2147483647LL) return true;
  set_error("%s: the output window reaches beyond int32 cell indices", who);
  return false;
}

// a window whose cells are counted in an int32
static inline bool lattice_window_cells_ok(const char* who, const SnerfDsmGrid* g) {
  if ((long long)g->out_h * g->out_w < LATTICE_MAX_CELLS) return true;
  set_error("%s: a window of %d x %d cells: out_h * out_w < 2^31 required", who, g->out_h, g->out_w);
  return false;
}

// a raster of h x w cells that are counted in an int32
static inline bool lattice_cells_ok(const char* who, int h, int w) {
  if (h < 1 || w < 1) { set_error("%s: h and w must be >= 1 (h = %d, w = %d)", who, h, w); return false; }
  if ((long long)h * w >= LATTICE_MAX_CELLS) { set_error("%s: h * w must be below 2^31 (h = %d, w = %d)", who, h, w); return false; }
  return true;
}

// Row k of a host table (`what` names a row: "sun", "direction"): its n values are finite, and the dim (2 or 3) of them from
// row[at] on form a unit vector to 1e-9.  The other fields of a row have rules of their own, checked by the entry.
static inline bool unit_row_ok(const char* who, const char* what, int k, const double* row, int n, int at, int dim) {
  for (int c = 0; c < n; ++c)
    if (!isfinite(row[c])) { set_error("%s: %s %d is not finite", who, what, k); return false; }
  const double* u = row + at;
  if (dim == 2) {
    if (fabs(u[0] * u[0] + u[1] * u[1] - 1.0) <= 1e-9) return true;
    set_error("%s: %s %d: (ux, uy) = (%.17g, %.17g) is not a unit vector", who, what, k, u[0], u[1]);
  } else {
    if (fabs(u[0] * u[0] + u[1] * u[1] + u[2] * u[2] - 1.0) <= 1e-9) return true;
    set_error("%s: %s %d: (east, north, up) = (%.17g, %.17g, %.17g) is not a unit vector", who, what, k, u[0], u[1], u[2]);
  }
  return false;
}

// q > 0 and finite, z0 finite; `what` is the entry's own wording of the rule
static inline bool quant_ok(const char* who, double z0, double q, const char* what = "q > 0 and finite, z0 finite required") {
  if (q > 0.0 && isfinite(q) && isfinite(z0)) return true;
  set_error("%s: %s", who, what);
  return false;
}

}  // namespace snerf
