// Geodetic conversions on the device, shared by the ray builder (satrays.hip), the world-cloud kernels (geo.hip: ecef_to_latlon
// on the way to the world, latlon_to_ecef on the way back into the scene) and the orthorectifier (orthorect.hip: utm_to_latlon per
// map cell): the custom ECEF system (the reference's framework/util/conversions.py) and the `utm` package's two series.  fp64,
// evaluated operation by operation as numpy does.
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

// the utm package's constants (utm/conversion.py), evaluated in its order
constexpr double UTM_K0 = 0.9996;
constexpr double UTM_E = 0.00669438;
constexpr double UTM_E2 = UTM_E * UTM_E;
constexpr double UTM_E3 = UTM_E2 * UTM_E;
constexpr double UTM_E_P2 = UTM_E / (1.0 - UTM_E);
constexpr double UTM_R = 6378137.0;
constexpr double UTM_M1 = 1.0 - UTM_E / 4.0 - 3.0 * UTM_E2 / 64.0 - 5.0 * UTM_E3 / 256.0;
constexpr double UTM_M2 = 3.0 * UTM_E / 8.0 + 3.0 * UTM_E2 / 32.0 + 45.0 * UTM_E3 / 1024.0;
constexpr double UTM_M3 = 15.0 * UTM_E2 / 256.0 + 45.0 * UTM_E3 / 1024.0;
constexpr double UTM_M4 = 35.0 * UTM_E3 / 3072.0;

// utm's mod_angle: (v + pi) % (2 pi) - pi with Python's sign rule for %, into [-pi, pi)
__device__ __forceinline__ double utm_wrap(double v) {
  const double two_pi = 2.0 * M_PI;
  double r = fmod(v + M_PI, two_pi);
  if (r != 0.0 && r < 0.0) r += two_pi;
  return r - M_PI;
}

// utm.from_latlon's series for a point at (lat, lon) in degrees in the zone of central meridian lon0 (radians)
__device__ __forceinline__ void latlon_to_utm(double lat, double lon, double lon0, int south, double* east, double* north) {
  const double lat_rad = lat * (M_PI / 180.0);
  const double lon_rad = lon * (M_PI / 180.0);
  const double ls = sin(lat_rad), lc = cos(lat_rad);
  const double t = ls / lc;
  const double t2 = t * t;
  const double t4 = t2 * t2;
  const double n = UTM_R / sqrt(1.0 - UTM_E * (ls * ls));
  const double c = UTM_E_P2 * (lc * lc);
  const double a = lc * utm_wrap(lon_rad - lon0);
  const double a2 = a * a;
  const double a3 = a2 * a;
  const double a4 = a3 * a;
  const double a5 = a4 * a;
  const double a6 = a5 * a;
  const double m = UTM_R * (UTM_M1 * lat_rad - UTM_M2 * sin(2.0 * lat_rad) + UTM_M3 * sin(4.0 * lat_rad) - UTM_M4 * sin(6.0 * lat_rad));
  *east = UTM_K0 * n * (a + a3 / 6.0 * (1.0 - t2 + c) + a5 / 120.0 * (5.0 - 18.0 * t2 + t4 + 72.0 * c - 58.0 * UTM_E_P2)) + 500000.0;
  double nn = UTM_K0 * (m + n * t * (a2 / 2.0 + a4 / 24.0 * (5.0 - t2 + 9.0 * c + 4.0 * (c * c)) +
                                     a6 / 720.0 * (61.0 - 58.0 * t2 + t4 + 600.0 * c - 330.0 * UTM_E_P2)));
  if (south) nn += 10000000.0;
  *north = nn;
}

// utm.to_latlon's constants: _E = (1 - sqrt(1 - E)) / (1 + sqrt(1 - E)) and the footpoint-latitude coefficients P2 .. P5.
// UTM_SQRT_1ME is the double nearest sqrt(1 - E) (sqrt is not a constant expression); the rest is evaluated in the package's order
constexpr double UTM_SQRT_1ME = 0.9966471893303066;
static_assert(UTM_SQRT_1ME * UTM_SQRT_1ME > (1.0 - UTM_E) * (1.0 - 1e-15) && UTM_SQRT_1ME * UTM_SQRT_1ME < (1.0 - UTM_E) * (1.0 + 1e-15),
              "UTM_SQRT_1ME is sqrt(1 - UTM_E)");
constexpr double UTM_E1 = (1.0 - UTM_SQRT_1ME) / (1.0 + UTM_SQRT_1ME);
constexpr double UTM_E1_2 = UTM_E1 * UTM_E1;
constexpr double UTM_E1_3 = UTM_E1_2 * UTM_E1;
constexpr double UTM_E1_4 = UTM_E1_3 * UTM_E1;
constexpr double UTM_E1_5 = UTM_E1_4 * UTM_E1;
constexpr double UTM_P2 = 3.0 / 2.0 * UTM_E1 - 27.0 / 32.0 * UTM_E1_3 + 269.0 / 512.0 * UTM_E1_5;
constexpr double UTM_P3 = 21.0 / 16.0 * UTM_E1_2 - 55.0 / 32.0 * UTM_E1_4;
constexpr double UTM_P4 = 151.0 / 96.0 * UTM_E1_3 - 417.0 / 128.0 * UTM_E1_5;
constexpr double UTM_P5 = 1097.0 / 512.0 * UTM_E1_4;

// utm.to_latlon's series for a point at (east, north) metres in the zone of central meridian lon0 (radians) -> degrees
__device__ __forceinline__ void utm_to_latlon(double east, double north, double lon0, int south, double* lat, double* lon) {
  const double x = east - 500000.0;
  double y = north;
  if (south) y -= 10000000.0;
  const double m = y / UTM_K0;
  const double mu = m / (UTM_R * UTM_M1);
  const double p = mu + UTM_P2 * sin(2.0 * mu) + UTM_P3 * sin(4.0 * mu) + UTM_P4 * sin(6.0 * mu) + UTM_P5 * sin(8.0 * mu);
  const double ps = sin(p), pc = cos(p);
  const double pt = ps / pc;
  const double pt2 = pt * pt;
  const double pt4 = pt2 * pt2;
  const double eps = 1.0 - UTM_E * (ps * ps);
  const double n = UTM_R / sqrt(eps);
  const double r = (1.0 - UTM_E) / eps;
  const double c = UTM_E_P2 * (pc * pc);
  const double c2 = c * c;
  const double d = x / (n * UTM_K0);
  const double d2 = d * d;
  const double d3 = d2 * d;
  const double d4 = d3 * d;
  const double d5 = d4 * d;
  const double d6 = d5 * d;
  // the d^6 term stands outside the bracket that pt / r multiplies, as in the package
  const double lat_rad = p - (pt / r) * (d2 / 2.0 - d4 / 24.0 * (5.0 + 3.0 * pt2 + 10.0 * c - 4.0 * c2 - 9.0 * UTM_E_P2)) +
                         d6 / 720.0 * (61.0 + 90.0 * pt2 + 298.0 * c + 45.0 * pt4 - 252.0 * UTM_E_P2 - 3.0 * c2);
  const double lon_rad = (d - d3 / 6.0 * (1.0 + 2.0 * pt2 + c) +
                          d5 / 120.0 * (5.0 - 2.0 * c + 28.0 * pt2 - 3.0 * c2 + 8.0 * UTM_E_P2 + 24.0 * pt4)) / pc;
  *lat = lat_rad * (180.0 / M_PI);
  *lon = utm_wrap(lon_rad + lon0) * (180.0 / M_PI);
}

}  // namespace snerf
