// What the per-facet folds (roofs.hip) and the facet growth (rooflines.hip) share: when a key is valid, and the misfit of a cell from
// a facet's plane in residual steps.  The fp64 tail is restated operation by operation in numpy: no fused multiply-add.
#pragma once
#include "common.h"

#include <limits.h>

#pragma clang fp contract(off)

namespace snerf {

constexpr long long ROOF_RQ_LIMIT = 1LL << 18;

__device__ __forceinline__ bool roof_valid(int k) { return k != INT_MIN && k != INT_MAX; }

// A cell at (di, dj, dk) from the root of a facet with the plane (gamma, alpha, beta), all in key units: e = dk - plane, and rq = e in
// steps of `unit`, rounded to nearest even and clamped at +-2^18 (a NaN counts as clamped high).
struct RoofMisfit {
  double e;
  long long rq;
  unsigned clamped;
};
__device__ __forceinline__ RoofMisfit roof_misfit(double gamma, double alpha, double beta, int di, int dj, long long dk, double unit) {
  RoofMisfit m;
  const double pred = (gamma + (alpha * (double)di)) + (beta * (double)dj);
  m.e = (double)dk - pred;
  m.clamped = 0;
  const double t = rint(m.e / unit);
  if (!(t < 262144.0)) { m.rq = ROOF_RQ_LIMIT; m.clamped = 1; }
  else if (t < -262144.0) { m.rq = -ROOF_RQ_LIMIT; m.clamped = 1; }
  else m.rq = (long long)t;
  return m;
}

}  // namespace snerf
