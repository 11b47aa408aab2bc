/* xgcm_hip_ext.h -- the open-ended extension of the C ABI of libxgcm_hip.so: the fused entry points added after
 * include/xgcm_hip.h and include/xgcm_hip_gm.h were closed to new prototypes (their export lists are held to fixed sets).
 * A new fused entry point goes HERE, its row into `_hip.FUSED_EXT`.  Same library, same conventions: element types,
 * boundary codes and status codes are xgcm_hip.h's; strides are in elements, 0 = broadcast; `stream` is a hipStream_t or NULL.
 *
 *   xg_redi_horizontal_tensor   the tapered off-diagonal components of the Redi / Gent-McWilliams tensor at u's and at v's
 *                      points, kappa * taper * sx and kappa * taper * sy there, from b alone: one pass (float64 and float32
 *                      through one entry: the element type is an argument)
 */
#ifndef XGCM_HIP_EXT_H
#define XGCM_HIP_EXT_H

#include "xgcm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The U- and V-point components of the tapered Redi / Gent-McWilliams tensor of a field b of `shape` (.., nz, ny, nx), one
 * pass; out_u (at u's points: left of the cell along X) and out_v (at v's: below it along Y) have `shape`.
 *   gx[i] = (b[i] - b[i-1]) [/ mx]     gy[j] = (b[j] - b[j-1]) [/ my]        f[k] = (b[k] - b[k-1]) [/ mz[k]]   (faces of Z)
 *   bzc[k] = (f[k] + f[k+1]) * 0.5     bzu[i] = (bzc[i-1] + bzc[i]) * 0.5    bzv[j] = (bzc[j-1] + bzc[j]) * 0.5
 *   gyc[j] = (gy[j] + gy[j+1]) * 0.5   gyu[i] = (gyc[i-1] + gyc[i]) * 0.5     gxc[i] = (gx[i] + gx[i+1]) * 0.5   gxv[j] = (gxc[j-1] + gxc[j]) * 0.5
 *   at u's points sx = -1 * (gx / bzu), sy = -1 * (gyu / bzu);  at v's points sx = -1 * (gxv / bzv), sy = -1 * (gy / bzv)
 *   s2 = sx * sx + sy * sy     kt = kappa * (m2 / (m2 + ((s2 - m2) + |s2 - m2|) * 0.5))     (`taper` = 0: kt = kappa)
 *   out_u = kt * sx at u's points     out_v = kt * sy at v's points
 * no fused multiply-add, IEEE quotients, no guard on a zero bzu or bzv.  `outer` = 0: nz faces, f[nz] is the pad of f
 * (periodic: f[0], extend: f[nz-1], fill: fill_z itself); `outer` = 1: nz + 1 faces, b padded above level 0 and below level
 * nz-1 and no pad of f.  Every stage pads its own input: b left of column 0, below row 0 and along Z (periodic: the far one,
 * extend: its own, fill: the fill value); gx right of the last column and gy above the last row; bzc and gyc left of column 0,
 * bzc and gxc below row 0 (fill: the fill value ITSELF, never formed from padded b).  mx and my broadcast against `shape`, mz
 * against `shape` with the faces along Z; NULL: absent, each on its own.  kappa, slope_max2 (= m2) and the fills are cast to
 * the element type once (-0.0 and NaN fills keep their bits).  XG_ERR_UNSUPPORTED: ndim < 3.  XG_ERR_INVALID: an element type
 * other than XG_T_F64 / XG_T_F32, a NULL b, result or shape, a metric without strides, outer or taper not 0 or 1, an unknown
 * boundary code, nz < 1, results that overlap; the results are untouched then.  An empty result is XG_OK without a launch. */
int xg_redi_horizontal_tensor(int dtype, const void* b, const void* mx, const int64_t* mx_strides, const void* my,
                              const int64_t* my_strides, const void* mz, const int64_t* mz_strides, double kappa,
                              double slope_max2, int taper, void* out_u, void* out_v, const int64_t* shape, int ndim, int outer,
                              int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XGCM_HIP_EXT_H */
