// Geodetic conversions of the custom ECEF system on the device (the reference's framework/util/conversions.py), shared by the
// ray builder (satrays.hip) and the world-cloud kernels (geo.hip: ecef_to_latlon on the way to the world, latlon_to_ecef on the way
// back into the scene).  fp64, evaluated operation by operation as numpy does.
#pragma once
#include "common.h"

// numpy evaluates every expression below operation by operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace snerf {

// framework/util/conversions.py latlon_to_ecef_custom
__device__ __forceinline__ void latlon_to_ecef(double lat, double lon, double alt, double* x, double* y, double* z) {
  const double rad_lat = lat * (M_PI / 180.0);
  const double rad_lon = lon * (M_PI / 180.0);
  const double a = 6378137.0;
  const double finv = 298.257223563;
  const double f = 1.0 / finv;
  const double e2 = 1.0 - (1.0 - f) * (1.0 - f);
  const double sl = sin(rad_lat), cl = cos(rad_lat);
  const double v = a / sqrt(1.0 - e2 * sl * sl);
  *x = (v + alt) * cl * cos(rad_lon);
  *y = (v + alt) * cl * sin(rad_lon);
  *z = (v * (1.0 - e2) + alt) * sl;
}

// framework/util/conversions.py ecef_to_latlon_custom
__device__ __forceinline__ void ecef_to_latlon(double x, double y, double z, double* lat_out, double* lon_out, double* alt_out) {
  const double a = 6378137.0;
  const double e = 8.1819190842622e-2;
  const double asq = a * a;
  const double esq = e * e;
  const double b = sqrt(asq * (1.0 - esq));
  const double bsq = b * b;
  const double ep = sqrt((asq - bsq) / bsq);
  const double p = sqrt(x * x + y * y);
  const double th = atan2(a * z, b * p);
  const double lon = atan2(y, x);
  const double st = sin(th), ct = cos(th);
  const double lat = atan2(z + (ep * ep) * b * (st * st * st), p - esq * a * (ct * ct * ct));
  const double sl = sin(lat);
  const double N = a / sqrt(1.0 - esq * (sl * sl));
  *alt_out = p / cos(lat) - N;
  *lon_out = lon * 180.0 / M_PI;
  *lat_out = lat * 180.0 / M_PI;
}

}  // namespace snerf
