// The one Amanatides-Woo march over a height field: from the centre of a cell along a horizontal unit direction (ux, uy), cell by
// cell, in units of the cell size.  shadow_cast_kernel (shadow.hip) and solar_horizon_kernel (solar.hip) are this walk with a loop
// body each; tests/shadow_numpy.py and tests/solar_numpy.py restate it independently and are compared with it bit for bit.
//   - fp64, evaluated operation by operation: only + - * /, comparisons and integer work, and NO fused multiply-add.  Each of
//     1.0 / fabs(ux), 0.5 * tdx and tmx + tdx is its own rounding, which is what the numpy restatements evaluate;
//   - plain operators under `fp contract(off)`, NOT __dadd_rn / __dmul_rn: those are header inlines compiled under the build's
//     default contraction, their operations keep that licence when inlined into a caller, and `h0 + rise * t` written with them
//     came out as one v_fma_f64.  For the same reason this header sets the pragma itself, and so does every file that uses it;
//   - a workgroup is one TX x TY tile of cells under ONE direction (a plane of the output): the direction is wave-uniform and
//     comes from the kernel arguments, and the parallel marches of a tile read neighbouring cells of the height field;
//   - the walk is a stepper, `while (m.next()) { ... }`, not a function that takes a visitor: a kernel's exits stay `break`s of
//     its own loop.  With a visitor whose bool return ends the walk the compiler merged the exits through mask registers and
//     shadow_cast_kernel took 30 % longer.
// The walk of raycast.hip is a different algorithm (it recomputes each crossing from the integer boundary and clips a segment),
// not a copy of this one.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace snerf {

// the tiles of n_planes rasters of h x w cells (h * w < 2^31), TX x TY cells each
struct MarchTiles {
  int tiles_x;
  long long tiles_per_plane, n_tiles;
};

static inline MarchTiles march_tiles(int h, int w, int TX, int TY, int n_planes) {
  MarchTiles m;
  m.tiles_x = (int)(((long long)w + TX - 1) / TX);
  m.tiles_per_plane = m.tiles_x * (((long long)h + TY - 1) / TY);
  m.n_tiles = m.tiles_per_plane * n_planes;
  return m;
}

// The plane k and the cell (i0, j0) of this thread in tile `tile` (TX is a power of two, a workgroup is TX * TY threads); false
// for a thread of an edge tile that lies outside the raster.
template <int TX, int TY>
__device__ __forceinline__ bool march_tile_cell(long long tile, int tiles_x, long long tiles_per_plane, int h, int w, int* k, int* i0,
                                                int* j0) {
  const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x / TX;
  *k = (int)(tile / tiles_per_plane);
  const long long r = tile - *k * tiles_per_plane;
  const long long i = (r % tiles_x) * TX + tx, j = (r / tiles_x) * TY + ty;
  if (i >= w || j >= h) return false;
  *i0 = (int)i;
  *j0 = (int)j;
  return true;
}

// The walk from the centre of cell (i0, j0) of an h x w raster: each next() enters one more cell (i, j), at distance t along the
// ray, and is false once the ray has left the raster.  An exact tie of the two crossings steps in x first.
struct DsmMarch {
  int i, j;
  double t;

  __device__ __forceinline__ DsmMarch(int h, int w, int i0, int j0, double ux, double uy)
      : i(i0), j(j0), h_(h), w_(w), steps_(h + w + 2),                        // h * w < 2^31: no overflow
        stepx_(ux > 0.0 ? 1 : -1), stepy_(uy > 0.0 ? 1 : -1),
        tdx_(ux == 0.0 ? __builtin_inf() : 1.0 / fabs(ux)), tdy_(uy == 0.0 ? __builtin_inf() : 1.0 / fabs(uy)),
        tmx_(0.5 * tdx_), tmy_(0.5 * tdy_) {}

  __device__ __forceinline__ bool next() {
    if (steps_-- <= 0) return false;
    if (tmx_ <= tmy_) {
      t = tmx_;
      i += stepx_;
      tmx_ = tmx_ + tdx_;
    } else {
      t = tmy_;
      j += stepy_;
      tmy_ = tmy_ + tdy_;
    }
    return !(i < 0 || i >= w_ || j < 0 || j >= h_);
  }

 private:
  int h_, w_, steps_, stepx_, stepy_;
  double tdx_, tdy_, tmx_, tmy_;
};

}  // namespace snerf
