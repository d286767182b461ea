// rpcm's RPCModel forward model on the device (rpcm/rpc_model.py apply_poly, apply_rfm, projection) and the host-side check of a
// SnerfRpc, shared by the ray builder (satrays.hip) and the orthorectifier (orthorect.hip).  fp64, evaluated in numpy's order.
#pragma once
#include "common.h"
#include "../../include/snerf_hip.h"

// numpy evaluates every expression below operation by operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace snerf {

// rpcm.rpc_model.apply_poly(poly, x, y, z) with x = lat, y = lon, z = alt (RPC00B term order), evaluated in numpy's order
__device__ __forceinline__ double rpc_poly(const double* c, double x, double y, double z) {
  double out = 0.0;
  out += c[0];
  out += c[1] * y + c[2] * x + c[3] * z;
  out += c[4] * y * x + c[5] * y * z + c[6] * x * z;
  out += c[7] * y * y + c[8] * x * x + c[9] * z * z;
  out += c[10] * x * y * z;
  out += c[11] * y * y * y;
  out += c[12] * y * x * x + c[13] * y * z * z + c[14] * y * y * x;
  out += c[15] * x * x * x;
  out += c[16] * x * z * z + c[17] * y * y * z + c[18] * x * x * z;
  out += c[19] * z * z * z;
  return out;
}

__device__ __forceinline__ double rpc_rfm(const double* num, const double* den, double x, double y, double z) {
  return rpc_poly(num, x, y, z) / rpc_poly(den, x, y, z);
}

// rpcm RPCModel.projection: (lon, lat, alt) -> (col, row)
__device__ __forceinline__ void rpc_project(const SnerfRpc& r, double lon, double lat, double alt, double* col, double* row) {
  const double nlon = (lon - r.lon_offset) / r.lon_scale;
  const double nlat = (lat - r.lat_offset) / r.lat_scale;
  const double nalt = (alt - r.alt_offset) / r.alt_scale;
  const double c = rpc_rfm(r.col_num, r.col_den, nlat, nlon, nalt);
  const double w = rpc_rfm(r.row_num, r.row_den, nlat, nlon, nalt);
  *col = c * r.col_scale + r.col_offset;
  *row = w * r.row_scale + r.row_offset;
}

// a table entry as every entry that takes one checks it: no zero or non-finite scale, has_inverse 0 or 1
static inline int check_rpc(const SnerfRpc& r, const char* who, int idx) {
  const double s[5] = {r.row_scale, r.col_scale, r.lat_scale, r.lon_scale, r.alt_scale};
  for (double v : s)
    if (!(v != 0.0) || !__builtin_isfinite(v)) { set_error("%s: RPC %d has a zero or non-finite scale", who, idx); return SNERF_ERR_BAD_DESC; }
  if (r.has_inverse != 0 && r.has_inverse != 1) { set_error("%s: RPC %d has_inverse = %d", who, idx, r.has_inverse); return SNERF_ERR_BAD_DESC; }
  return SNERF_OK;
}

}  // namespace snerf
