/* xgcm_hip_gm.h -- the Gent-McWilliams side of the C ABI of libxgcm_hip.so: operators on the results of xg_redi_tensor
 * (include/xgcm_hip.h) whose fields all sit at the faces of Z.  Same library, same conventions: element types, boundary
 * codes and status codes are xgcm_hip.h's; strides are in elements, 0 = broadcast; `stream` is a hipStream_t or NULL.
 *
 *   xg_bolus_velocity   -d/dz of the Gent-McWilliams streamfunction (interp(kwx, X), interp(kwy, Y)) and its horizontal
 *                      divergence: the eddy-induced (u*, v*, w*), one pass (float64 and float32 through one entry: the
 *                      element type is an argument)
 */
#ifndef XGCM_HIP_GM_H
#define XGCM_HIP_GM_H

#include "xgcm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The Gent-McWilliams eddy-induced (bolus) velocity from xg_redi_tensor's kwx and kwy, one pass.  `shape` (.., nz, ny, nx) is
 * the LEVELS' shape; kwx, kwy and out_w are contiguous at the faces of Z, nz of them (`outer` = 1: nz + 1); out_u and out_v
 * have `shape`.
 *   px[i] = (kwx[i-1] + kwx[i]) * 0.5    py[j] = (kwy[j-1] + kwy[j]) * 0.5      the streamfunction at u's / v's columns
 *   closed = 1: px = py = +0.0 at face 0 and, `outer`, at face nz; kwx and kwy are never read there
 *   out_u[k] = -1 * ((px[k+1] - px[k]) [/ mzu[k]])    out_v[k] = -1 * ((py[k+1] - py[k]) [/ mzv[k]])
 *   tx = px [* dyG]    ty = py [* dxG]    out_w = ((tx[i+1] - tx[i]) + (ty[j+1] - ty[j])) [/ rA]
 * no fused multiply-add, IEEE quotients.  Pads: kwx left of column 0 and kwy below row 0 (periodic: the far one, extend:
 * itself, fill: the fill value); the TRANSPORTS tx right of the last column and ty above the last row (periodic: the one at
 * index 0, extend: at n-1, fill: the fill value itself, not multiplied by a metric); `outer` = 0: px and py beyond face nz-1
 * (periodic: face 0's -- closed: +0.0 --, extend: face nz-1's, fill: fill_z itself).  A closed face of out_w is formed from
 * +0.0 through the same products, differences and quotient.  mzu and mzv broadcast against `shape`; dyG, dxG and rA against
 * `shape` with the faces along Z; strides in elements, 0 = broadcast; NULL: absent, each on its own.  The fills are cast to
 * the element type (-0.0 and NaN keep their bits).  XG_ERR_UNSUPPORTED: ndim < 3.  XG_ERR_INVALID: an element type other than
 * XG_T_F64 / XG_T_F32, a NULL kwx, kwy, result or shape, a metric without strides, outer or closed not 0 or 1, an unknown
 * boundary code, nz < 1; the results are untouched then.  An empty result is XG_OK without a launch. */
int xg_bolus_velocity(int dtype, const void* kwx, const void* kwy, const void* mzu, const int64_t* mzu_strides, const void* mzv,
                      const int64_t* mzv_strides, const void* dyG, const int64_t* dyG_strides, const void* dxG,
                      const int64_t* dxG_strides, const void* rA, const int64_t* rA_strides, void* out_u, void* out_v,
                      void* out_w, const int64_t* shape, int ndim, int outer, int closed, int bc_x, double fill_x, int bc_y,
                      double fill_y, int bc_z, double fill_z, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XGCM_HIP_GM_H */
