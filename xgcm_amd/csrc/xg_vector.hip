// xg_vector.hip -- fused two-component operators (vorticity K7, divergence K7b, gradient / flux K7c) and the broadcasting binary op
// Part of libxgcm_hip.so; compiled twice (real = double / -DXG_F32), see xg_common.hpp.

#include <initializer_list>

#include "xg_common.hpp"

// rows of Y per wave-task of the fused two-component kernels (see STENCIL_SEG in xg_stencil.hip): A/B on one GPU
// (XG_HIP_LIB), 4320 x 4320 x 90: vorticity 70.0 / 71.7 / 71.3 % with 4 / 2 / 1 rows, gradient 73.9 / 75.7 / 75.6 %,
// flux 71.4 / 74.3 / 74.5 %; the two-axis kernel K8 78.3 / 78.6 / 75.1 %  =>  2
#ifndef XG_FUSED_SEG
#define XG_FUSED_SEG 2
#endif

namespace {

// ------------------------------------------------------------------------------------------
// broadcasting binary op (out C-contiguous, a/b addressed through strides; dims pre-coalesced)
// ------------------------------------------------------------------------------------------
struct BinGeo {
  int ndim;
  int64_t total;  // number of V-wide items
  int64_t shape[XG_MAX_NDIM];  // shape[ndim-1] counts V-wide items
  int64_t sa[XG_MAX_NDIM], sb[XG_MAX_NDIM];
  int idx32;                 // total < 2^32: the item index is peeled with multiply-shift divisions (FastDiv)
  FastDiv fs[XG_MAX_NDIM];   // divisors shape[d]
};

template <int BOP> __device__ __forceinline__ real bin2(real a, real b) {
  if (BOP == XG_BIN_MUL) return a * b;
#ifndef XG_INT
  if (BOP == XG_BIN_DIV) return a / b;
#endif
  if (BOP == XG_BIN_ADD) return a + b;
  return a - b;
}

// `nta` / `ntb`: the operand is streamed exactly once (no broadcast dim) => non-temporal loads; together with the
// XCD-banded block order that is worth 4 points on a three-stream kernel (tools/probes/streambench.hip SB_TRIAD: 75.4 %
// plain, 77.8 % with non-temporal loads, 79.1 % banded as well)
template <int BOP, int V, bool NTS>
__global__ __launch_bounds__(BLOCK) void k_binary(const real* __restrict__ a, const real* __restrict__ b,
                                                  real* __restrict__ out, BinGeo g, ZBand zb, u32 nblk, int nta, int ntb) {
  typedef typename VecT<V>::type T;
  const u32 pb = (nblk + 7) >> 3;
  const u32 lb = (blockIdx.x & 7) * pb + (blockIdx.x >> 3);
  if (lb >= nblk) return;
  int64_t gid = (int64_t)lb * BLOCK + threadIdx.x;
  if (zb.on) {
    // (Z, P) items with one operand broadcast along Z (da / dx(Y,X)): band-major order keeps the
    // band of the small operand in L2 while all Z levels of the band stream by (as in K1 / K2S)
    u32 z, pin;
    if (gid >= (int64_t)zb.per_band.d * ((zb.Y + zb.B - 1) / zb.B)) return;
    if (!zband_map(zb, (u32)gid, z, pin)) return;
    gid = (int64_t)z * zb.Y + pin;
  }
  if (gid >= g.total) return;
  int64_t oa = 0, ob = 0;
  if (g.idx32) {  // (a 64-bit division per dim and thread cost this kernel 5 points: 0.74 -> 0.79 for da / dx(Y,X))
    u32 r = (u32)gid;
#pragma unroll
    for (int d = XG_MAX_NDIM - 1; d >= 0; --d) {
      if (d < g.ndim) {
        const u32 q = (d == 0) ? 0u : fdiv(r, g.fs[d]);  // (the slowest dim needs no division: r < shape[0] there)
        int64_t c = (int64_t)(r - q * g.fs[d].d);
        if (d == g.ndim - 1) c *= V;
        oa += c * g.sa[d];
        ob += c * g.sb[d];
        r = q;
      }
    }
  } else {
    int64_t r = gid;
#pragma unroll
    for (int d = XG_MAX_NDIM - 1; d >= 0; --d) {
      if (d < g.ndim) {
        int64_t s = g.shape[d];
        int64_t q = r / s;
        int64_t c = r - q * s;
        if (d == g.ndim - 1) c *= V;
        oa += c * g.sa[d];
        ob += c * g.sb[d];
        r = q;
      }
    }
  }
  const int64_t sa_in = g.sa[g.ndim - 1], sb_in = g.sb[g.ndim - 1];
  if (V > 1) {
    dv av, bv, o;
    if (sa_in == 1) av = nta ? __builtin_nontemporal_load(reinterpret_cast<const dv*>(a + oa)) : *reinterpret_cast<const dv*>(a + oa);
    else {
#pragma unroll
      for (int k = 0; k < NV; ++k) av[k] = a[oa + k * sa_in];
    }
    if (sb_in == 1) bv = ntb ? __builtin_nontemporal_load(reinterpret_cast<const dv*>(b + ob)) : *reinterpret_cast<const dv*>(b + ob);
    else {
#pragma unroll
      for (int k = 0; k < NV; ++k) bv[k] = b[ob + k * sb_in];
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) o[k] = bin2<BOP>(av[k], bv[k]);
    stg_s<dv, NTS>(out + gid * NV, o);  // (`sc1 nt`, DESIGN rule 16: da / dx +2.8, a * b +2.2 points on one box, +-0 on another)
  } else {
    stg<real, NTS>(out + gid, bin2<BOP>(a[oa], b[ob]));
  }
}

#ifndef XG_INT  // the fused two-component operators divide by / multiply with float metrics: float builds only
// ------------------------------------------------------------------------------------------
// K7: fused relative vorticity ((v[j,i]-v[j,i-1]) - (u[j,i]-u[j-1,i])) / area, view (outer,Y,X).
// Same shape as K2S: lanes along X (V=2 when nx even), XCD-banded waves, each wave register-marches
// SEG rows of Y: SEG+1 rows of u (the j-1 halo row is an L2 hit), SEG rows of v plus the 8-byte
// left neighbour (same cache lines), SEG rows of area.  24 B/cell instead of 56 B unfused.
// ------------------------------------------------------------------------------------------
// offset of the (Y, X) plane of `area` that belongs to outer index o: the leading dims of the field
// that the area does not have broadcast (stride 0), the others advance it (e.g. a field (Z, face, j, i)
// with rAz(face, j, i)); dims are peeled innermost-first with multiply-shift division on the scalar unit
struct AreaIdx {
  int n;
  FastDiv fd[XG_MAX_NDIM];
  int64_t stride[XG_MAX_NDIM];
};
__device__ __forceinline__ int64_t area_outer_off(const AreaIdx& ai, int64_t o) {
  int64_t off = 0;
  u32 rem = (u32)o;
#pragma unroll
  for (int d = XG_MAX_NDIM - 1; d >= 0; --d) {
    if (d < ai.n) {
      const u32 q = fdiv(rem, ai.fd[d]);
      off += (int64_t)(rem - q * ai.fd[d].d) * ai.stride[d];
      rem = q;
    }
  }
  return off;
}

// ZK > 1 (z-banded launches only): the wave carries the same rows of ZK consecutive levels and loads the area
// rows once for all of them -- L2-resident metric rows still compete with the field loads for the CU's
// outstanding requests (measured on the 1-D kernels: derivative along X 74.8 -> 77.3 % with shared rows).
// SEG rows of a metric / area plane for a V-wide lane, row r at m[off + r * sy] (short tails repeat the last row), elements
// `sx` apart.  The FORM of the load -- one aligned vector, or element by element -- is the HOST's decision (`vec`: unit step,
// base, row step and every outer stride keep the vector's alignment -- `plane_vec_ok`), one scalar branch per plane: `ldm`'s
// own test is a lane-divergent branch per load, a row loop with such loads in it issues them one by one, each after the wait
// for the one before (the gradient: four round trips to the L2 in a row after the field had arrived), and a test made in the
// kernel joins its paths in front of the loads, where the wave then waits for everything in flight.
template <typename T, int SEG>
__device__ __forceinline__ void load_rows(T (&dst)[SEG], const real* __restrict__ m, int64_t off, int64_t sy, int64_t sx, int64_t nrow, bool vec) {
  if (sizeof(T) > sizeof(real) && vec) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) dst[s_] = *reinterpret_cast<const T*>(m + off + ((s_ < nrow) ? s_ : nrow - 1) * sy);
  } else {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) dst[s_] = ldm<T>(m, off + ((s_ < nrow) ? s_ : nrow - 1) * sy, sx);
  }
}

__device__ __forceinline__ real vec_last(dv v) { return v[NV - 1]; }
__device__ __forceinline__ real vec_last(real v) { return v; }
__device__ __forceinline__ real vec_first(dv v) { return v[0]; }
__device__ __forceinline__ real vec_first(real v) { return v; }

// The wave-task every fused kernel starts from: blocks in XCD-banded order, WPB waves per block, the wave id (on the scalar
// unit: readfirstlane) peeled into (x-tile, outer index of this launch, Y segment) -- segment-major inside an outer index, or
// band-major (`BANDED`; a literal false where the kernel has no bands, and the branch is gone): a band of segments stays in
// the XCD's L2 for all outer indices.  Declares `oo` (outer index inside the launch; ZK levels per task: K7 / K7b), `sg`,
// `o` = o0 + oo, and the lane's V columns from `i0` in SEG rows from `j0` (`nrow` of them exist); returns from the kernel,
// before its first load, for a wave or a lane without work.  Reads the kernel's parameters nblk, ntile, nseg, nouter, o0,
// ny, nx by name.  A macro and not a function: to a function the FastDiv / ZBand kernel arguments go as copies made at the
// call, which moves their loads in front of the first return and changed the registers of K7d, K7e, K7f and K7h (up to +2
// VGPRs, one K7e instance from 3 to 2 waves per SIMD); expanded in place, every kernel compiles to the code it had.
#define XG_WAVE_TASK(V_, SEG_, BANDED, ZB, ZK_)                                          \
  const u32 pb_ = (nblk + 7) >> 3;                                                       \
  const u32 lb_ = (blockIdx.x & 7) * pb_ + (blockIdx.x >> 3);                            \
  if (lb_ >= nblk) return;                                                               \
  const u32 w_ = __builtin_amdgcn_readfirstlane(lb_ * WPB + (threadIdx.x >> 6));         \
  const u32 r_ = fdiv(w_, ntile);                                                        \
  const u32 tile_ = w_ - r_ * ntile.d;                                                   \
  u32 oo, sg;                                                                            \
  if (BANDED) {                                                                          \
    if (!zband_map(ZB, r_, oo, sg)) return;                                              \
    oo *= ZK_;                                                                           \
  } else {                                                                               \
    oo = fdiv(r_, nseg);                                                                 \
    if (oo >= nouter) return;                                                            \
    sg = r_ - oo * nseg.d;                                                               \
  }                                                                                      \
  const int64_t o = o0 + oo;                                                             \
  const int64_t i0 = ((int64_t)tile_ * WAVE + (threadIdx.x & 63)) * V_;                  \
  if (i0 >= nx) return;                                                                  \
  const int64_t j0 = (int64_t)sg * SEG_;                                                 \
  const int64_t nrow = (ny - j0 < SEG_) ? ny - j0 : SEG_

// The X neighbours of a lane's vector where they come from the lanes beside it (`ntl` bit 0 with vector lanes: DPP after the
// loads, K7c's scheme): `lidx` / `ridx` are the columns left / right of the vector, wrapped at a periodic edge and clamped
// (0, nx - 1) at any other, so both are always inside the row; `own_l` / `own_r`: the lane loads that neighbour itself (no
// shuffle, the tile's first / last lane, the row's edge); `form_r`: it also forms the staggered value right of it itself --
// not at an extend / fill right edge, where the pad replaces that value.  K7e reads column `ridx` under `form_r` only, so the
// clamped form that K7g needs (it reads it under `own_r`: the extend pad) serves both.  K7d, K7f and K7h keep these lines
// written out (K7d's and K7f's with 0 for the unread clamped `ridx`): through this helper some of their instances came out
// with other VGPR counts (K7d -1, K7f -2, K7h -2 .. +3; occupancy as before), whichever `ridx` form it had.
struct LaneEdges {
  bool edge_l, edge_r, shl, own_l, own_r, form_r;
  int64_t lidx, ridx;
};
template <int V>
__device__ __forceinline__ LaneEdges lane_edges(int64_t i0, int64_t nx, int bc_x, int ntl) {
  LaneEdges e;
  const bool per = bc_x == XG_BC_PERIODIC;
  e.edge_l = (i0 == 0);
  e.edge_r = (i0 + V >= nx);
  e.lidx = e.edge_l ? (per ? nx - 1 : 0) : i0 - 1;
  e.ridx = e.edge_r ? (per ? 0 : nx - 1) : i0 + V;
  e.shl = V > 1 && (ntl & 1);
  e.own_l = !e.shl || (threadIdx.x & 63) == 0 || e.edge_l;
  e.own_r = !e.shl || (threadIdx.x & 63) == 63 || e.edge_r;
  e.form_r = e.own_r && !(e.edge_r && !per);
  return e;
}

template <int V, bool HAS_AREA, bool NTS, int SEG, int ZK = 1>
__global__ __launch_bounds__(BLOCK) void k_vorticity(
    const real* __restrict__ u, const real* __restrict__ v, const real* __restrict__ area,
    real* __restrict__ out, int64_t o0, u32 nouter, u32 nblk, int64_t ny, int64_t nx, FastDiv ntile,
    FastDiv nseg, ZBand zb, int bc_x, real fill_x, int bc_y, real fill_y, AreaIdx ai, int64_t a_sy,
    int64_t a_sx, const real* __restrict__ halo_x, const real* __restrict__ halo_y, int ntl) {
  typedef typename VecT<V>::type T;
  XG_WAVE_TASK(V, SEG, HAS_AREA && zb.on, zb, ZK);  // (band-major: a (Y,X) area band stays in the XCD's L2 for all levels)
  const int nk = (ZK > 1 && (int64_t)nouter - (int64_t)oo < ZK) ? (int)(nouter - oo) : ZK;
  const int64_t a_base = HAS_AREA ? area_outer_off(ai, o) : 0;
  const bool edge = (i0 == 0);
  const int64_t nidx = edge ? ((bc_x == XG_BC_PERIODIC) ? nx - 1 : 0) : i0 - 1;
  const bool fill_edge = edge && (bc_x == XG_BC_FILL);

  T uu[ZK][SEG + 1], vv[ZK][SEG], ar[SEG];
  real vl[ZK][SEG];
  bool f0 = false;
#pragma unroll
  for (int kz = 0; kz < ZK; ++kz) {
    const int64_t ok = o + ((kz < nk) ? kz : nk - 1);  // a short last group repeats its last level (not stored)
    const real* pu = u + ok * ny * nx + i0;
    const real* pv = v + (ok * ny + j0) * nx;
    {
      int64_t q = j0 - 1;
      const real* src = pu + q * nx;
      if (q < 0) {
        f0 = (bc_y == XG_BC_FILL);
        src = pu + ((bc_y == XG_BC_PERIODIC) ? ny - 1 : 0) * nx;
        if (bc_y == XG_BC_HALO) src = halo_y + ok * nx + i0;  // pre-gathered row below the first one: (outer, 1, X)
      }
      uu[kz][0] = *reinterpret_cast<const T*>(src);  // the previous segment's last row: an L2 hit
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      const int64_t jr = (s_ < nrow) ? s_ : nrow - 1;  // clamp inside the array for short tails
      // rows nobody reads again stream past the caches (non-temporal); the segment's LAST u row is the next
      // segment's halo row and the v row carries the 8-byte neighbour loads, so those stay ordinary loads
      if ((ntl & 2) && s_ + 1 < SEG) uu[kz][s_ + 1] = __builtin_nontemporal_load(reinterpret_cast<const T*>(pu + (j0 + jr) * nx));
      else uu[kz][s_ + 1] = *reinterpret_cast<const T*>(pu + (j0 + jr) * nx);
      if (V > 1 && (ntl & 1)) {
        // the v row is read by this wave only: non-temporal, and the value left of a lane's vector comes from
        // the lane before it (lanes that left at the row's end are the highest ones); lane 0 loads its own.  The
        // shuffles come AFTER every load of the task has been issued (below): taken here, each one made the wave wait for
        // its row before the next row's loads went out -- four round trips to the memory one after the other
        vv[kz][s_] = __builtin_nontemporal_load(reinterpret_cast<const T*>(pv + jr * nx + i0));
        vl[kz][s_] = real(0);
        if ((threadIdx.x & 63) == 0 || edge)
          vl[kz][s_] = (edge && bc_x == XG_BC_HALO) ? halo_x[ok * ny + j0 + jr] : pv[jr * nx + nidx];
      } else {
        vv[kz][s_] = *reinterpret_cast<const T*>(pv + jr * nx + i0);
        vl[kz][s_] = (edge && bc_x == XG_BC_HALO) ? halo_x[ok * ny + j0 + jr]  // pre-gathered column left of the first: (outer, Y, 1)
                                                  : pv[jr * nx + nidx];
      }
    }
  }
  if (HAS_AREA) load_rows<T, SEG>(ar, area, a_base + j0 * a_sy + i0 * a_sx, a_sy, a_sx, nrow, (ntl & 4) != 0);
  if (V > 1 && (ntl & 1)) {
    const bool own = (threadIdx.x & 63) == 0 || edge;
#pragma unroll
    for (int kz = 0; kz < ZK; ++kz) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const real left = from_lane_below(vec_last(vv[kz][s_]));  // DPP wave_shr:1 (lane 0 reads 0 and is `own`)
        if (!own) vl[kz][s_] = left;
      }
    }
  }
#pragma unroll
  for (int kz = 0; kz < ZK; ++kz) {
    if (kz >= nk) break;
    real* po = out + ((o + kz) * ny + j0) * nx + i0;
    const T u0 = f0 ? splat<T>(fill_y) : uu[kz][0];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        const real left = fill_edge ? fill_x : vl[kz][s_];
        T z = dvdx_of(vv[kz][s_], left) - (uu[kz][s_ + 1] - (s_ == 0 ? u0 : uu[kz][s_]));
        if (HAS_AREA) z = z / ar[s_];
        stg_s<T, NTS>(po + s_ * nx, z);  // (`sc1 nt`, rule 16: vorticity +4.5, divergence +2.9 points; the two-output kernels keep `nt`)
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7b: fused horizontal divergence (delta_x u + delta_y v) / area of docs/ufunc_examples.md
// ("Divergence": u on (Y:center, X:left), v on (Y:left, X:center), both left -> center, i.e.
// padding_width (0,1) on both axes).  Mirror image of K7: SEG rows of u with their right
// neighbour, SEG+1 rows of v (the last one is the upper halo row of the segment).
// ------------------------------------------------------------------------------------------
template <int V, bool HAS_AREA, bool NTS, int SEG, int ZK = 1>
__global__ __launch_bounds__(BLOCK) void k_divergence(
    const real* __restrict__ u, const real* __restrict__ v, const real* __restrict__ area,
    real* __restrict__ out, int64_t o0, u32 nouter, u32 nblk, int64_t ny, int64_t nx, FastDiv ntile,
    FastDiv nseg, ZBand zb, int bc_x, real fill_x, int bc_y, real fill_y, AreaIdx ai, int64_t a_sy,
    int64_t a_sx, const real* __restrict__ halo_x, const real* __restrict__ halo_y, int ntl) {
  typedef typename VecT<V>::type T;
  XG_WAVE_TASK(V, SEG, HAS_AREA && zb.on, zb, ZK);
  const int nk = (ZK > 1 && (int64_t)nouter - (int64_t)oo < ZK) ? (int)(nouter - oo) : ZK;
  const int64_t a_base = HAS_AREA ? area_outer_off(ai, o) : 0;
  const bool edge = (i0 + V >= nx);
  const int64_t ridx = edge ? ((bc_x == XG_BC_PERIODIC) ? 0 : nx - 1) : i0 + V;
  const bool fill_edge = edge && (bc_x == XG_BC_FILL);

  T uu[ZK][SEG], vv[ZK][SEG + 1], ar[SEG];
  real ur[ZK][SEG];
  bool ftop = false;
#pragma unroll
  for (int kz = 0; kz < ZK; ++kz) {
    const int64_t ok = o + ((kz < nk) ? kz : nk - 1);
    const real* pu = u + (ok * ny + j0) * nx;
    const real* pv = v + ok * ny * nx + i0;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      const int64_t jr = (s_ < nrow) ? s_ : nrow - 1;
      uu[kz][s_] = *reinterpret_cast<const T*>(pu + jr * nx + i0);
      ur[kz][s_] = (edge && bc_x == XG_BC_HALO) ? halo_x[ok * ny + j0 + jr]  // pre-gathered column right of the last: (outer, Y, 1)
                                                : pu[jr * nx + ridx];
      vv[kz][s_] = *reinterpret_cast<const T*>(pv + (j0 + jr) * nx);
    }
    {
      int64_t q = j0 + nrow;  // the row above the segment's last row
      const real* src = pv + q * nx;
      if (q >= ny) {
        ftop = (bc_y == XG_BC_FILL);
        src = pv + ((bc_y == XG_BC_PERIODIC) ? 0 : ny - 1) * nx;
        if (bc_y == XG_BC_HALO) src = halo_y + ok * nx + i0;  // pre-gathered row above the last one: (outer, 1, X)
      }
      vv[kz][SEG] = *reinterpret_cast<const T*>(src);
    }
  }
  if (HAS_AREA) load_rows<T, SEG>(ar, area, a_base + j0 * a_sy + i0 * a_sx, a_sy, a_sx, nrow, (ntl & 4) != 0);
#pragma unroll
  for (int kz = 0; kz < ZK; ++kz) {
    if (kz >= nk) break;
    real* po = out + ((o + kz) * ny + j0) * nx + i0;
    const T top = ftop ? splat<T>(fill_y) : vv[kz][SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        const real right = fill_edge ? fill_x : ur[kz][s_];
        const T up = (s_ + 1 < nrow) ? vv[kz][s_ + 1] : top;
        T z = dudx_fwd(uu[kz][s_], right) + (up - vv[kz][s_]);
        if (HAS_AREA) z = z / ar[s_];
        stg_s<T, NTS>(po + s_ * nx, z);  // (`sc1 nt`, rule 16: vorticity +4.5, divergence +2.9 points; the two-output kernels keep `nt`)
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7c: the two remaining fused grid ufuncs of docs/ufunc_examples.md, one field in, TWO fields out:
//   gradient: gx = (a - a[x-1]) / mx,  gy = (a - a[y-1]) / my      ("Gradient": center -> left on X, Y)
//   flux:     fx = u * interp(T, X),   fy = v * interp(T, Y)       ("Advection": center -> left on X, Y)
// Load pattern of K7/K8 (SEG+1 rows of the centre field + the 8-B left neighbour); the field is read
// once for both outputs: 24 B/cell instead of 32 (gradient), 40 instead of 80 (flux chain).
// ------------------------------------------------------------------------------------------
template <int V, int MODE, bool NTS, int SEG>   // MODE 0: gradient (optional metrics), 1: flux
__global__ __launch_bounds__(BLOCK) void k_pair2d(
    const real* __restrict__ a, const real* __restrict__ u, const real* __restrict__ v, real* __restrict__ out_x,
    real* __restrict__ out_y, int64_t o0, u32 nouter, u32 nblk, int64_t ny, int64_t nx, FastDiv ntile, FastDiv nseg,
    int bc_x, real fill_x, int bc_y, real fill_y, const real* __restrict__ mx, AreaIdx aix, int64_t mx_sy,
    int64_t mx_sx, const real* __restrict__ my, AreaIdx aiy, int64_t my_sy, int64_t my_sx,
    const real* __restrict__ halo_x, const real* __restrict__ halo_y, ZBand zb, int ntl) {
  typedef typename VecT<V>::type T;
  XG_WAVE_TASK(V, SEG, zb.on, zb, 1);  // (band-major: the metric rows of a band of segments stay in the XCD's L2 for all outer indices, rule 4)
  const int64_t base = o * ny * nx;
  const real* pa = a + base + i0;
  const bool edge = (i0 == 0);
  const int64_t nidx = edge ? ((bc_x == XG_BC_PERIODIC) ? nx - 1 : 0) : i0 - 1;
  const bool fill_edge = edge && (bc_x == XG_BC_FILL);
  T aa[SEG + 1];
  real al[SEG];
  {
    int64_t q = j0 - 1;
    bool f = false;
    const real* src = pa + q * nx;
    if (q < 0) {
      f = (bc_y == XG_BC_FILL);
      src = pa + ((bc_y == XG_BC_PERIODIC) ? ny - 1 : 0) * nx;
      if (bc_y == XG_BC_HALO) src = halo_y + o * nx + i0;  // pre-gathered row below the first one: (outer, 1, X)
    }
    const T t = *reinterpret_cast<const T*>(src);
    aa[0] = f ? splat<T>(fill_y) : t;
  }
  // `ntl` bit 0 (vector lanes): rows the next segment does not need again are loaded non-temporally and the value left of a
  // lane's vector comes from the lane before it (DPP, after the loads) instead of an 8-byte load over the same cache lines --
  // K7's scheme.  Gradient without metrics 2.505 -> 2.401 ms (0.776 -> 0.810 of 8 TB/s), with one / two metric planes +1 %
  // (profiles/r06_kernels/r06be_ab_pair_nt.log).  What the metrics cost is their DIVISIONS, not their planes: none 0.805, one
  // 0.749, two 0.675 -- and the same plane passed twice 0.681, a second plane at shifted addresses 0.681 (r06bf_ab_grad_planes.log)
  const bool shl = V > 1 && (ntl & 1);
  const bool own = (threadIdx.x & 63) == 0 || edge;
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    const int64_t jr = j0 + ((s_ < nrow) ? s_ : nrow - 1);
    if (shl && s_ + 1 < SEG) aa[s_ + 1] = __builtin_nontemporal_load(reinterpret_cast<const T*>(pa + jr * nx));
    else aa[s_ + 1] = *reinterpret_cast<const T*>(pa + jr * nx);
    if (shl) {
      al[s_] = real(0);
      if (own) al[s_] = (edge && bc_x == XG_BC_HALO) ? halo_x[o * ny + jr] : a[base + jr * nx + nidx];
    } else {
      al[s_] = (edge && bc_x == XG_BC_HALO) ? halo_x[o * ny + jr]  // pre-gathered column left of the first: (outer, Y, 1)
                                            : a[base + jr * nx + nidx];
    }
  }
  if (shl) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      const real left = from_lane_below(vec_last(aa[s_ + 1]));
      if (!own) al[s_] = left;
    }
  }
  const int64_t mxb = (MODE == 0 && mx) ? area_outer_off(aix, o) : 0;
  const int64_t myb = (MODE == 0 && my) ? area_outer_off(aiy, o) : 0;
  // (round 6: the metric rows / the u and v rows of all SEG rows loaded HERE, behind the field's loads and before anything
  // waits, in a host-decided vector form -- in the loop below each of them goes out only after the row before has been
  // stored, four round trips to the L2 one after the other -- made the gradient 9 % SLOWER (2.74 -> 3.00 ms, two process
  // pairs on one box) and left the flux where it was: what the row-by-row order has is stores leaving while later loads
  // arrive, the lesson of the scans' batch form.  profiles/r06_kernels/r06bb_ab_loads_first_vector_kernels.log)
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    if (s_ < nrow) {
      const int64_t j = j0 + s_;
      const real left = fill_edge ? fill_x : al[s_];
      T rx, ry;
      if (MODE == 0) {
        rx = dvdx_of(aa[s_ + 1], left);
        ry = aa[s_ + 1] - aa[s_];
        if (mx) rx = rx / ldm<T>(mx, mxb + j * mx_sy + i0 * mx_sx, mx_sx);
        if (my) ry = ry / ldm<T>(my, myb + j * my_sy + i0 * my_sx, my_sx);
      } else {
        // (u and v are read once; loading them non-temporally changed nothing: 4.234 / 4.262 ms, r06be_ab_pair_nt.log)
        const T uu = *reinterpret_cast<const T*>(u + base + j * nx + i0);
        const T vv = *reinterpret_cast<const T*>(v + base + j * nx + i0);
        rx = uu * interp_left_of(aa[s_ + 1], left);
        ry = vv * op2<XG_OP_INTERP>(aa[s_], aa[s_ + 1]);
      }
      // (rule 16: the flux runs at 0.77 with `sc1 nt` in every round, with `nt` at 0.77 or 0.70 from process to process; the
      // gradient -- one input stream, two metric planes to keep in the L2 -- loses 2 points with `sc1 nt` on either output or on
      // both (three rounds each, profiles/history/r03bl_ab_grad_drop.jsonl; r03ba_*; +2 once in r03be_*) and keeps `nt`)
      if (MODE == 1) {
        stg_s<T, NTS>(out_x + base + j * nx + i0, rx);
        stg_s<T, NTS>(out_y + base + j * nx + i0, ry);
      } else {
        stg<T, NTS>(out_x + base + j * nx + i0, rx);
        stg<T, NTS>(out_y + base + j * nx + i0, ry);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7d: the two second-order chains of K7c + K7b in ONE pass, the staggered intermediate kept in registers:
//   MODE 1 flux divergence: Fx = u * interp(T, X),  Fy = v * interp(T, Y)               (divergence(flux(u, v, T)))
//   MODE 0 laplacian:       Fx = (delta_x T / dxC) * dyG,  Fy = (delta_y T / dyC) * dxG  (metrics NULL: the differences)
//   out = ((Fx[i+1] - Fx[i]) + (Fy[j+1] - Fy[j])) [/ area]
// with K7c's / K7b's own arithmetic helpers in the chain's order (-ffp-contract=off).  The chain pads twice: T below / left
// of the first row / column (bc of K7c), the INTERMEDIATE above / right of the last one (bc of K7b): periodic -> the
// intermediate at index 0 (formed from T's own periodic halo), extend -> at n-1, fill -> the fill value itself.
// Per wave-task (SEG rows): SEG+2 rows of T, SEG rows of u, SEG+1 of v; the T value left of a lane's vector and the Fx
// right of it come from the neighbouring lanes (DPP); lane 0 / lane 63 / the edge lanes load or form their own.
// 32 B/cell (flux divergence) and 16 B/cell (laplacian: the five metric planes are 2-D and stay in the L2) instead of
// 64 / ~100 B/cell for the chains.
// ------------------------------------------------------------------------------------------
struct Div2dMet {           // MODE 0 metric planes (all four, or none) at the chain's positions, broadcast strides
  const real* p[4];         // dxC (Y:c, X:l), dyG (Y:c, X:l), dyC (Y:l, X:c), dxG (Y:l, X:c)
  AreaIdx ai[4];
  int64_t sy[4], sx[4];
};

template <int V, int MODE, bool HAS_AREA, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_div2d(
    const real* __restrict__ t, const real* __restrict__ u, const real* __restrict__ v, const real* __restrict__ area,
    real* __restrict__ out, int64_t o0, u32 nouter, u32 nblk, int64_t ny, int64_t nx, FastDiv ntile, FastDiv nseg,
    ZBand zb, int bc_x, real fill_x, int bc_y, real fill_y, AreaIdx ai, int64_t a_sy, int64_t a_sx, Div2dMet mt, int ntl) {
  typedef typename VecT<V>::type T;
  XG_WAVE_TASK(V, SEG, zb.on, zb, 1);  // (band-major: the area / metric rows of a band stay in the XCD's L2 for all outer indices)
  const int64_t base = o * ny * nx;
  const real* pt = t + base;
  const bool met = MODE == 0 && mt.p[0] != nullptr;
  // X: T left of the lane (first stage, K7c's rule) and the column whose Fx lies right of it (second stage, K7b's rule)
  const bool edge_l = (i0 == 0), edge_r = (i0 + V >= nx);
  const int64_t lidx = edge_l ? ((bc_x == XG_BC_PERIODIC) ? nx - 1 : 0) : i0 - 1;
  const int64_t ridx = edge_r ? 0 : i0 + V;  // (periodic; extend and fill take no value from there)
  const bool shl = V > 1 && (ntl & 1);
  const bool own_l = !shl || (threadIdx.x & 63) == 0 || edge_l;
  const bool own_r = !shl || (threadIdx.x & 63) == 63 || edge_r;
  const bool form_r = own_r && !(edge_r && bc_x != XG_BC_PERIODIC);  // lanes that form the Fx right of them themselves
  // Y: the row above the segment's last one (T, v / metrics there) -- row 0 at a periodic top
  const int64_t q = j0 + nrow;
  const bool top_edge = q >= ny;
  const int64_t qr = top_edge ? 0 : q;
  const bool top_own = !top_edge || bc_y == XG_BC_PERIODIC;  // else: extend (Fy of the last row) or fill (fill_y)

  T tt[SEG + 1], ttop;  // tt[0]: the row below the segment; tt[1 + s]: row j0 + s (short tails repeat the last row)
  real tl[SEG], tr[SEG];
  {
    const int64_t qb = j0 - 1;
    bool f = false;
    const real* src = pt + qb * nx + i0;
    if (qb < 0) {
      f = (bc_y == XG_BC_FILL);
      src = pt + ((bc_y == XG_BC_PERIODIC) ? ny - 1 : 0) * nx + i0;
    }
    const T b = *reinterpret_cast<const T*>(src);
    tt[0] = f ? splat<T>(fill_y) : b;
  }
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    const int64_t jr = j0 + ((s_ < nrow) ? s_ : nrow - 1);
    // rows the next segment does not read again stream past the caches (K7c)
    if (shl && s_ + 1 < SEG) tt[s_ + 1] = __builtin_nontemporal_load(reinterpret_cast<const T*>(pt + jr * nx + i0));
    else tt[s_ + 1] = *reinterpret_cast<const T*>(pt + jr * nx + i0);
    tl[s_] = real(0);
    tr[s_] = real(0);
    if (own_l) tl[s_] = pt[jr * nx + lidx];
    if (form_r) tr[s_] = pt[jr * nx + ridx];
  }
  ttop = *reinterpret_cast<const T*>(pt + qr * nx + i0);
  T uu[SEG], vv[SEG], vtop;
  real urt[SEG];
  if (MODE == 1) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      const int64_t jr = j0 + ((s_ < nrow) ? s_ : nrow - 1);
      uu[s_] = *reinterpret_cast<const T*>(u + base + jr * nx + i0);
      vv[s_] = *reinterpret_cast<const T*>(v + base + jr * nx + i0);
      urt[s_] = form_r ? u[base + jr * nx + ridx] : real(0);
    }
    vtop = *reinterpret_cast<const T*>(v + base + qr * nx + i0);
  }
  T ar[SEG];
  if (HAS_AREA) load_rows<T, SEG>(ar, area, area_outer_off(ai, o) + j0 * a_sy + i0 * a_sx, a_sy, a_sx, nrow, (ntl & 4) != 0);
  if (shl) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      const real left = from_lane_below(vec_last(tt[s_ + 1]));  // DPP wave_shr:1 (lane 0 reads 0 and is `own_l`)
      if (!own_l) tl[s_] = left;
    }
  }
  int64_t mb[4] = {0, 0, 0, 0};
  if (met) {
#pragma unroll
    for (int k = 0; k < 4; ++k) mb[k] = area_outer_off(mt.ai[k], o);
  }
  // the metric rows of the segment up front, in the host-decided form (`ntl` bit 3: every plane an aligned vector): with `ldm`
  // inside the row loop below the laplacian ran 6 % slower (profiles/EXPERIMENTS.md, K7d)
  T mr[4][SEG];
  if (met) {
#pragma unroll
    for (int k = 0; k < 4; ++k) load_rows<T, SEG>(mr[k], mt.p[k], mb[k] + j0 * mt.sy[k] + i0 * mt.sx[k], mt.sy[k], mt.sx[k], nrow, (ntl & 8) != 0);
  }
  // the intermediates, each formed once: Fx at the lane's cells, Fy at its cells and at the row above the segment
  T fx[SEG], fy[SEG], fytop;
  real fxr[SEG];
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    const int64_t j = j0 + ((s_ < nrow) ? s_ : nrow - 1);
    const real left = (edge_l && bc_x == XG_BC_FILL) ? fill_x : tl[s_];
    const real last = vec_last(tt[s_ + 1]);
    if (MODE == 1) {
      fx[s_] = uu[s_] * interp_left_of(tt[s_ + 1], left);
      fy[s_] = vv[s_] * op2<XG_OP_INTERP>(tt[s_], tt[s_ + 1]);
      fxr[s_] = urt[s_] * interp_left_of(tr[s_], last);
    } else {
      fx[s_] = dvdx_of(tt[s_ + 1], left);
      fy[s_] = tt[s_ + 1] - tt[s_];
      fxr[s_] = tr[s_] - last;
      if (met) {
        fx[s_] = fx[s_] / mr[0][s_];
        fx[s_] = fx[s_] * mr[1][s_];
        fy[s_] = fy[s_] / mr[2][s_];
        fy[s_] = fy[s_] * mr[3][s_];
        if (form_r) {
          fxr[s_] = fxr[s_] / mt.p[0][mb[0] + j * mt.sy[0] + ridx * mt.sx[0]];
          fxr[s_] = fxr[s_] * mt.p[1][mb[1] + j * mt.sy[1] + ridx * mt.sx[1]];
        }
      }
    }
  }
  if (MODE == 1) {
    fytop = vtop * op2<XG_OP_INTERP>(tt[SEG], ttop);
  } else {
    fytop = ttop - tt[SEG];
    if (met) {
      fytop = fytop / ldm<T>(mt.p[2], mb[2] + qr * mt.sy[2] + i0 * mt.sx[2], mt.sx[2]);
      fytop = fytop * ldm<T>(mt.p[3], mb[3] + qr * mt.sy[3] + i0 * mt.sx[3], mt.sx[3]);
    }
  }
  if (shl) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      const real right = from_lane_above(vec_first(fx[s_]));  // DPP wave_shl:1 (lane 63 reads 0 and is `own_r`)
      if (!own_r) fxr[s_] = right;
    }
  }
  real* po = out + base + j0 * nx + i0;
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    if (s_ < nrow) {
      real right = fxr[s_];
      if (edge_r && bc_x == XG_BC_FILL) right = fill_x;
      else if (edge_r && bc_x == XG_BC_EXTEND) right = vec_last(fx[s_]);
      T up = (s_ + 1 < nrow) ? fy[s_ + 1] : fytop;
      if (s_ + 1 >= nrow && !top_own) up = (bc_y == XG_BC_FILL) ? splat<T>(fill_y) : fy[s_];
      T z = dudx_fwd(fx[s_], right) + (up - fy[s_]);
      if (HAS_AREA) z = z / ar[s_];
      stg_s<T, NTS>(po + s_ * nx, z);
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7e: the 3-D tracer flux divergence (MITgcm's advection term) in ONE pass over (lead, Z, Y, X):
//   out = ((Fx[i+1] - Fx[i]) + (Fy[j+1] - Fy[j])) + (Fz[k+1] - Fz[k])  [/ vol]
// Fx, Fy per level exactly as K7d MODE 1 (same helpers, same order, same X / Y boundaries); Fz[k] = w[k] * interp(T[k-1], T[k]).
// Z pads twice, as the chain does: T above level 0 (periodic: T[nz-1], extend: T[0], fill: fill_z), then Fz below level nz-1
// (periodic: Fz[0], extend: Fz[nz-1], fill: fill_z itself).  Each wave owns one (lead, Y segment, X tile) column and marches
// k = 0 .. nz-1: the rows of T[k+1] and w[k+1] are read at level k (they form Fz[k+1]) and carry over in registers with
// Fz[k+1] to level k+1, so u, v, w and T are each read once and out written once: 40 B/cell in float64.  The volume is one
// broadcast array (`va`) or the product va * vb formed in registers in get_metric's order (area * thickness); rows that do
// not vary along Z are loaded once per wave.
// ------------------------------------------------------------------------------------------
struct VolIdx {  // one volume factor: the lead dims as in AreaIdx, then (Z, Y, X) element strides (0 = broadcast)
  const real* p;
  AreaIdx ai;
  int64_t sz, sy, sx;
};

template <int V, int NVOL, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_div3d(
    const real* __restrict__ t, const real* __restrict__ u, const real* __restrict__ v, const real* __restrict__ w,
    real* __restrict__ out, int64_t o0, u32 nouter, u32 nblk, int64_t nz, int64_t ny, int64_t nx, FastDiv ntile,
    FastDiv nseg, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z, real fill_z, VolIdx va, VolIdx vb, int ntl) {
  typedef typename VecT<V>::type T;
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const int64_t plane = ny * nx;
  const int64_t col = o * nz * plane;  // level 0 of this lead index (int64: a 4320^2 x 90 field has more than 2^32 cells)
  // X and Y exactly as K7d: T left of the lane, the column whose Fx lies right of it, the rows below / above the segment
  const LaneEdges e = lane_edges<V>(i0, nx, bc_x, ntl);
  const int64_t q = j0 + nrow;
  const bool top_edge = q >= ny;
  const int64_t rq = (top_edge ? 0 : q) * nx;
  const bool top_own = !top_edge || bc_y == XG_BC_PERIODIC;
  const bool fill_b = j0 == 0 && bc_y == XG_BC_FILL;
  const int64_t rb = (j0 > 0 ? j0 - 1 : ((bc_y == XG_BC_PERIODIC) ? ny - 1 : 0)) * nx;
  int64_t ro[SEG];  // the segment's rows in a plane (short tails repeat the last row)
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) ro[s_] = (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * nx;

  T fa[SEG], fb[SEG];
  int64_t vao = 0, vbo = 0;
  if (NVOL >= 1) {
    vao = area_outer_off(va.ai, o) + j0 * va.sy + i0 * va.sx;
    load_rows<T, SEG>(fa, va.p, vao, va.sy, va.sx, nrow, (ntl & 4) != 0);
  }
  if (NVOL >= 2) {
    vbo = area_outer_off(vb.ai, o) + j0 * vb.sy + i0 * vb.sx;
    load_rows<T, SEG>(fb, vb.p, vbo, vb.sy, vb.sx, nrow, (ntl & 8) != 0);
  }
  // level 0: Fz[0] from T padded above it; periodic Z keeps Fz[0] for the pad below the last level
  T tc[SEG], fzc[SEG], fz0[SEG];
  {
    const int64_t ka = (bc_z == XG_BC_PERIODIC) ? nz - 1 : 0;
    T ta[SEG], w0[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      tc[s_] = *reinterpret_cast<const T*>(t + col + ro[s_] + i0);
      w0[s_] = *reinterpret_cast<const T*>(w + col + ro[s_] + i0);
      ta[s_] = (bc_z == XG_BC_FILL) ? splat<T>(fill_z) : *reinterpret_cast<const T*>(t + col + ka * plane + ro[s_] + i0);
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      fzc[s_] = w0[s_] * op2<XG_OP_INTERP>(ta[s_], tc[s_]);
      fz0[s_] = fzc[s_];
    }
  }
  for (int64_t k = 0; k < nz; ++k) {
    const int64_t lv = col + k * plane;
    const real* pt = t + lv;
    const bool more = k + 1 < nz;
    // the next level's T and w rows first (Fz[k+1]), then this level's u, v and T halo
    T tn[SEG], wn[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (more) {
        tn[s_] = *reinterpret_cast<const T*>(pt + plane + ro[s_] + i0);
        wn[s_] = *reinterpret_cast<const T*>(w + lv + plane + ro[s_] + i0);
      } else {
        tn[s_] = tc[s_];
        wn[s_] = splat<T>(real(0));
      }
    }
    T tb = *reinterpret_cast<const T*>(pt + rb + i0);
    if (fill_b) tb = splat<T>(fill_y);
    const T ttop = *reinterpret_cast<const T*>(pt + rq + i0);
    T uu[SEG], vv[SEG];
    real tl[SEG], tr[SEG], urt[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      uu[s_] = *reinterpret_cast<const T*>(u + lv + ro[s_] + i0);
      vv[s_] = *reinterpret_cast<const T*>(v + lv + ro[s_] + i0);
      tl[s_] = e.own_l ? pt[ro[s_] + e.lidx] : real(0);
      tr[s_] = e.form_r ? pt[ro[s_] + e.ridx] : real(0);
      urt[s_] = e.form_r ? u[lv + ro[s_] + e.ridx] : real(0);
    }
    const T vtop = *reinterpret_cast<const T*>(v + lv + rq + i0);
    if (NVOL >= 1 && k > 0 && va.sz != 0)
      load_rows<T, SEG>(fa, va.p, vao + k * va.sz, va.sy, va.sx, nrow, (ntl & 4) != 0);
    if (NVOL >= 2 && k > 0 && vb.sz != 0)
      load_rows<T, SEG>(fb, vb.p, vbo + k * vb.sz, vb.sy, vb.sx, nrow, (ntl & 8) != 0);
    if (e.shl) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const real left = from_lane_below(vec_last(tc[s_]));  // DPP wave_shr:1 (lane 0 reads 0 and is `own_l`)
        if (!e.own_l) tl[s_] = left;
      }
    }
    T fx[SEG], fy[SEG];
    real fxr[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      const real left = (e.edge_l && bc_x == XG_BC_FILL) ? fill_x : tl[s_];
      fx[s_] = uu[s_] * interp_left_of(tc[s_], left);
      fy[s_] = vv[s_] * op2<XG_OP_INTERP>(s_ == 0 ? tb : tc[s_ - 1], tc[s_]);
      fxr[s_] = urt[s_] * interp_left_of(tr[s_], vec_last(tc[s_]));
    }
    const T fytop = vtop * op2<XG_OP_INTERP>(tc[SEG - 1], ttop);
    if (e.shl) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const real right = from_lane_above(vec_first(fx[s_]));  // DPP wave_shl:1 (lane 63 reads 0 and is `own_r`)
        if (!e.own_r) fxr[s_] = right;
      }
    }
    T fzn[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (more) fzn[s_] = wn[s_] * op2<XG_OP_INTERP>(tc[s_], tn[s_]);
      else fzn[s_] = (bc_z == XG_BC_PERIODIC) ? fz0[s_] : ((bc_z == XG_BC_EXTEND) ? fzc[s_] : splat<T>(fill_z));
    }
    real* po = out + lv + j0 * nx + i0;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        real right = fxr[s_];
        if (e.edge_r && bc_x == XG_BC_FILL) right = fill_x;
        else if (e.edge_r && bc_x == XG_BC_EXTEND) right = vec_last(fx[s_]);
        T up = (s_ + 1 < nrow) ? fy[s_ + 1] : fytop;
        if (s_ + 1 >= nrow && !top_own) up = (bc_y == XG_BC_FILL) ? splat<T>(fill_y) : fy[s_];
        const T h = dudx_fwd(fx[s_], right) + (up - fy[s_]);
        T z = h + (fzn[s_] - fzc[s_]);
        if (NVOL == 1) z = z / fa[s_];
        if (NVOL == 2) z = z / (fa[s_] * fb[s_]);
        stg_s<T, NTS>(po + s_ * nx, z);
      }
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      tc[s_] = tn[s_];
      fzc[s_] = fzn[s_];
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7f: the vertical transport from continuity in ONE pass over (lead, Z, Y, X):
//   d[k] = (U[i+1] - U[i]) + (V[j+1] - V[j])     K7b's arithmetic and X / Y boundaries, U = u [* face area], V = v [* face area]
//   forward:  w[0] = Z pad (fill: fill_z, extend: d[0]),  w[k] = d[0] + .. + d[k-1]
//   reverse:  w[k] = d[nz-1] + .. + d[k]
//   out = (-1 * w) [/ area]
// i.e. divergence -> nancumsum along Z (center -> left) -> negation -> division, the levels of a column added IN SEQUENCE as
// k_cumsum_strided adds them (a NaN divergence counts as 0; the first sum is d itself, not 0 + d).  The decomposition is
// K7e's: a wave owns one (lead, Y segment, X tile) column and marches Z, upward or downward (`reverse`, wave-uniform); the
// running sum stays in registers, so u and v are read once and w written once: 24 B/cell in float64 against 72 for the chain.
// The loads form a rolling window of U levels ahead of the sum (k_cumsum_strided's PIPE): a march whose loads wait behind
// its own stores loses the memory system (K5c).  Face weights: factor `a` of a field is any broadcast array (its rows stay
// in registers when it does not vary along Z), factor `b` varies along Z only and is one wave-uniform load per level.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ real nan0(real x) { return (x != x) ? real(0) : x; }  // as the scans' (xg_scan.hip)
__device__ __forceinline__ dv nan0(dv x) {
  dv o;
#pragma unroll
  for (int k = 0; k < NV; ++k) o[k] = nan0(x[k]);
  return o;
}

template <typename T, int SEG>
struct WcLevel {  // what one level of a column brings: SEG rows of u with the element right of the lane, SEG + 1 rows of v
  T uu[SEG], vv[SEG], vtop;
  real urt[SEG];
};

template <int V, bool FW, bool AR, bool NTS, int SEG, int U>
__global__ __launch_bounds__(BLOCK) void k_wcont(
    const real* __restrict__ u, const real* __restrict__ v, real* __restrict__ out, int64_t o0, u32 nouter, u32 nblk,
    int64_t nz, int64_t ny, int64_t nx, FastDiv ntile, FastDiv nseg, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z,
    real fill_z, int reverse, VolIdx ua, VolIdx ub, VolIdx va, VolIdx vb, VolIdx ar, int ntl) {
  typedef typename VecT<V>::type T;
  typedef WcLevel<T, SEG> L;
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const int64_t plane = ny * nx;
  const int64_t col = o * nz * plane;  // level 0 of this lead index (int64: a 4320^2 x 90 field has more than 2^32 cells)
  // X as K7e: the element right of the lane's vector comes from the lane above (DPP) or, for the tile's last lane and the
  // row's last vector, from memory (periodic: column 0); fill / extend at the row's end need no load
  const bool edge_r = (i0 + V >= nx);
  const int64_t ridx = edge_r ? 0 : i0 + V;
  const bool shl = V > 1 && (ntl & 1);
  const bool own_r = !shl || (threadIdx.x & 63) == 63 || edge_r;
  const bool form_r = own_r && !(edge_r && bc_x != XG_BC_PERIODIC);
  // Y as K7b: the row above the segment (periodic: row 0; fill / extend at the top need no row, row 0 is loaded and unused)
  const int64_t q = j0 + nrow;
  const bool top_edge = q >= ny;
  const int64_t rq = (top_edge ? 0 : q) * nx;
  const bool top_own = !top_edge || bc_y == XG_BC_PERIODIC;
  int64_t ro[SEG];  // the segment's rows in a plane (short tails repeat the last row)
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) ro[s_] = (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * nx;
  const real* pu = u + col + i0;
  const real* pv = v + col + i0;
  const real* pur = u + col + ridx;

  // the marched levels in scan order: forward drops the last level (center -> left trims it), except that `extend` pads
  // with the first partial sum, which exists for nz == 1 too
  const bool fwd = !reverse;
  const int64_t n = fwd ? ((nz > 1) ? nz - 1 : ((bc_z == XG_BC_EXTEND) ? 1 : 0)) : nz;
  auto level = [&](int64_t t) -> int64_t { return fwd ? t : nz - 1 - t; };
  auto fetch = [&](int64_t k) -> L {
    L x;
    const int64_t lv = k * plane;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      x.uu[s_] = *reinterpret_cast<const T*>(pu + lv + ro[s_]);
      x.vv[s_] = *reinterpret_cast<const T*>(pv + lv + ro[s_]);
      x.urt[s_] = form_r ? pur[lv + ro[s_]] : real(0);
    }
    x.vtop = *reinterpret_cast<const T*>(pv + lv + rq);
    return x;
  };

  // face weights: factor a's rows (u: SEG rows and the element at `ridx`; v: SEG + 1 rows) stay in registers and are
  // loaded again per level only when the factor varies along Z
  T fu[SEG], fv[SEG], fvt = splat<T>(real(1));
  real fur[SEG];
  int64_t uao = 0, vao = 0, ubo = 0, vbo = 0;
  auto weights = [&](int64_t k) {
    const int64_t ou = uao + k * ua.sz, ov = vao + k * va.sz;
    load_rows<T, SEG>(fu, ua.p, ou + j0 * ua.sy + i0 * ua.sx, ua.sy, ua.sx, nrow, (ntl & 4) != 0);
    load_rows<T, SEG>(fv, va.p, ov + j0 * va.sy + i0 * va.sx, va.sy, va.sx, nrow, (ntl & 8) != 0);
    T top[1];
    load_rows<T, 1>(top, va.p, ov + (top_edge ? 0 : q) * va.sy + i0 * va.sx, va.sy, va.sx, 1, (ntl & 8) != 0);
    fvt = top[0];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_)
      fur[s_] = form_r ? ua.p[ou + (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * ua.sy + ridx * ua.sx] : real(0);
  };
  if (FW) {
    uao = area_outer_off(ua.ai, o);
    vao = area_outer_off(va.ai, o);
    if (ub.p) ubo = area_outer_off(ub.ai, o);
    if (vb.p) vbo = area_outer_off(vb.ai, o);
    if (n > 0) weights(level(0));
  }
  T aa[SEG];
  int64_t aro = 0;
  if (AR) {
    aro = area_outer_off(ar.ai, o) + j0 * ar.sy + i0 * ar.sx;
    load_rows<T, SEG>(aa, ar.p, aro, ar.sy, ar.sx, nrow, (ntl & 16) != 0);
  }
  real* po = out + col + j0 * nx + i0;
  auto put = [&](int64_t k, const T (&a)[SEG]) {  // output level k: negation, division, SEG rows in linear order
    if (AR && ar.sz != 0) load_rows<T, SEG>(aa, ar.p, aro + k * ar.sz, ar.sy, ar.sx, nrow, (ntl & 16) != 0);
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        T z = splat<T>(real(-1)) * a[s_];
        if (AR) z = z / aa[s_];
        stg_s<T, NTS>(po + k * plane + s_ * nx, z);
      }
    }
  };

  T acc[SEG];
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) acc[s_] = splat<T>(fill_z);
  if (fwd && bc_z == XG_BC_FILL) put(0, acc);
  bool started = false;
  auto step = [&](int64_t t, const L& x) {
    const int64_t k = level(t);
    T uc[SEG], vc[SEG], vt = x.vtop;
    real right[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      uc[s_] = x.uu[s_];
      vc[s_] = x.vv[s_];
      right[s_] = x.urt[s_];
    }
    if (FW) {
      if (t > 0 && (ua.sz != 0 || va.sz != 0)) weights(k);
      // (products commute bit for bit: a * b is get_metric's product whichever of its two factors varies along Z)
      const bool ubz = ub.p != nullptr, vbz = vb.p != nullptr;
      const real zu = ubz ? ub.p[ubo + k * ub.sz] : real(1), zv = vbz ? vb.p[vbo + k * vb.sz] : real(1);
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        uc[s_] = uc[s_] * (ubz ? fu[s_] * splat<T>(zu) : fu[s_]);
        right[s_] = right[s_] * (ubz ? fur[s_] * zu : fur[s_]);
        vc[s_] = vc[s_] * (vbz ? fv[s_] * splat<T>(zv) : fv[s_]);
      }
      vt = vt * (vbz ? fvt * splat<T>(zv) : fvt);
    }
    if (shl) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const real above = from_lane_above(vec_first(uc[s_]));  // DPP wave_shl:1 (lane 63 reads 0 and is `own_r`)
        if (!own_r) right[s_] = above;
      }
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      real rt = right[s_];
      if (edge_r && bc_x == XG_BC_FILL) rt = fill_x;
      else if (edge_r && bc_x == XG_BC_EXTEND) rt = vec_last(uc[s_]);
      T up = (s_ + 1 < nrow) ? vc[(s_ + 1 < SEG) ? s_ + 1 : s_] : vt;
      if (s_ + 1 >= nrow && !top_own) up = (bc_y == XG_BC_FILL) ? splat<T>(fill_y) : vc[s_];
      const T d = nan0(dudx_fwd(uc[s_], rt) + (up - vc[s_]));
      acc[s_] = started ? acc[s_] + d : d;
    }
    started = true;
    if (fwd) {  // center -> left: the sum through level k is w[k + 1]; `extend` pads with the first one
      if (t == 0 && bc_z == XG_BC_EXTEND) put(0, acc);
      if (k + 1 < nz) put(k + 1, acc);
    } else {
      put(k, acc);
    }
  };

  // the rolling window: every consumed level is replaced by the load of the level U steps ahead
  L win[U];
#pragma unroll
  for (int p = 0; p < U; ++p)
    if (p < n) win[p] = fetch(level(p));
  int64_t t = 0;
  for (; t + 2 * U <= n; t += U) {
#pragma unroll
    for (int p = 0; p < U; ++p) {
      const L x = win[p];
      win[p] = fetch(level(t + U + p));
      step(t + p, x);
    }
  }
  for (; t < n; t += U) {  // the last one or two windows: refills and consumes guarded (wave-uniform tests)
#pragma unroll
    for (int p = 0; p < U; ++p) {
      const L x = win[p];
      if (t + U + p < n) win[p] = fetch(level(t + U + p));
      if (t + p < n) step(t + p, x);
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7g: kinetic energy at the cell centre, 0.5 * (interp(u * u, X) + interp(v * v, Y)), both interpolations left -> center.
// K7b's shape: SEG rows of u with the value right of the lane's vector (DPP; lane 63 and the edge lane load their own), SEG+1
// rows of v.  The SQUARES are padded above / right of the last row / column, as the chain pads them: periodic -> the square
// at index 0, extend -> at n-1, fill -> the fill value itself.  24 B/cell instead of the chain's ~120 (six launches).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ dv interp_right_of(dv c, real r) {
  dv o;
#pragma unroll
  for (int k = 0; k < NV - 1; ++k) o[k] = (c[k] + c[k + 1]) * real(0.5);
  o[NV - 1] = (c[NV - 1] + r) * real(0.5);
  return o;
}
__device__ __forceinline__ real interp_right_of(real c, real r) { return (c + r) * real(0.5); }

template <int V, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_kinetic(
    const real* __restrict__ u, const real* __restrict__ v, real* __restrict__ out, int64_t o0, u32 nouter, u32 nblk,
    int64_t ny, int64_t nx, FastDiv ntile, FastDiv nseg, int bc_x, real fill_x, int bc_y, real fill_y, int ntl) {
  typedef typename VecT<V>::type T;
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const LaneEdges e = lane_edges<V>(i0, nx, bc_x, ntl);  // (the right side only)
  const bool fill_edge = e.edge_r && (bc_x == XG_BC_FILL);
  const real* pu = u + (o * ny + j0) * nx;
  const real* pv = v + o * ny * nx + i0;
  T uu[SEG], vv[SEG + 1];
  real ur[SEG];
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    const int64_t jr = (s_ < nrow) ? s_ : nrow - 1;
    uu[s_] = *reinterpret_cast<const T*>(pu + jr * nx + i0);
    ur[s_] = e.own_r ? pu[jr * nx + e.ridx] : real(0);
    vv[s_] = *reinterpret_cast<const T*>(pv + (j0 + jr) * nx);
  }
  bool ftop = false;
  {
    const int64_t q = j0 + nrow;  // the row above the segment's last row
    const real* src = pv + q * nx;
    if (q >= ny) {
      ftop = (bc_y == XG_BC_FILL);
      src = pv + ((bc_y == XG_BC_PERIODIC) ? 0 : ny - 1) * nx;
    }
    vv[SEG] = *reinterpret_cast<const T*>(src);
  }
  if (e.shl) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      const real right = from_lane_above(vec_first(uu[s_]));  // DPP wave_shl:1 (lane 63 reads 0 and is `own_r`)
      if (!e.own_r) ur[s_] = right;
    }
  }
  real* po = out + (o * ny + j0) * nx + i0;
  const T top = ftop ? splat<T>(fill_y) : vv[SEG] * vv[SEG];
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    if (s_ < nrow) {
      const real sr = fill_edge ? fill_x : ur[s_] * ur[s_];
      const T ix = interp_right_of(uu[s_] * uu[s_], sr);
      const T up = (s_ + 1 < nrow) ? vv[s_ + 1] * vv[s_ + 1] : top;
      const T iy = op2<XG_OP_INTERP>(vv[s_] * vv[s_], up);
      stg_s<T, NTS>(po + s_ * nx, splat<T>(real(0.5)) * (ix + iy));
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7h: the vector-invariant momentum advection (+ Coriolis) tendencies in ONE pass, two fields in, two out:
//   zeta = ((v[j,i] - v[j,i-1]) - (u[j,i] - u[j-1,i])) [/ rAz] [+ f]              (Y:left, X:left)    K7
//   ke   = 0.5 * (interp(u * u, X) + interp(v * v, Y))                             centre              K7g
//   gu   = interp(zeta, Y) * interp(interp(v, X), Y) - (ke[j,i] - ke[j,i-1]) [/ dxC]         at u's points
//   gv   = -(interp(zeta, X) * interp(interp(u, Y), X)) - (ke[j,i] - ke[j-1,i]) [/ dyC]      at v's points
// in the chain's operation order (-ffp-contract=off, the compiler's IEEE quotients).
// WHAT THIS IS: zeta is the curl of the RAW u, v in index space over the area -- not the relative vorticity, whose differences
// are of the circulations u * dxC, v * dyC -- while the same u, v serve as velocities in ke and in the two means.  With the
// metrics the result is (zeta v - d/dx KE, -zeta u - d/dy KE) only on a grid of unit spacing (dxC = dyC = 1, rAz = 1); on a
// uniform grid of spacing h it is (zeta / h) v - d/dx KE, and without the metrics h times the term.  Measured against the
// analytic term in tests/test_convergence.py (a strict expected failure there until the kernel takes circulations).
// Per wave-task (SEG rows, one x-tile) a
// lane holds the patch of u and v it needs: rows j0-1 .. j0+SEG, columns i0-1 .. i0+V -- the columns left and right of its
// vector from the neighbouring lanes (DPP), lane 0 / lane 63 / the edge lanes load their own.  A periodic axis wraps the
// patch's indices: every stage's periodic pad is then the stage's own value at the wrapped index.  At an extend / fill
// boundary the raw patch carries the pads of the FIRST stages (u below row 0, v left of column 0: the clamped index or the
// fill value) and every later stage overrides its own pad: zeta, the X-mean of v above the last row; zeta, the Y-mean of u
// right of the last column; u * u right, v * v above; ke below and left -- extend: the stage's value at the clamped index,
// fill: the fill value itself.  Every intermediate is formed once per lane; the two outputs of a cell share them.
// 32 B/cell in float64 (coriolis and the three metric planes are 2-D and stay in the L2) instead of ~400 for the 20 launches.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ real vec_at(dv v, int k) { return v[k]; }
__device__ __forceinline__ real vec_at(real v, int) { return v; }
__device__ __forceinline__ void vec_set(dv& v, int k, real x) { v[k] = x; }
__device__ __forceinline__ void vec_set(real& v, int, real x) { v = x; }

template <int V, bool MET, bool COR, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_momadv(
    const real* __restrict__ u, const real* __restrict__ v, real* __restrict__ out_u, real* __restrict__ out_v, int64_t o0,
    u32 nouter, u32 nblk, int64_t ny, int64_t nx, FastDiv ntile, FastDiv nseg, ZBand zb, int bc_x, real fill_x, int bc_y,
    real fill_y, Div2dMet mt, int ntl) {  // mt: rAz, coriolis (Y:l, X:l), dxC (Y:c, X:l), dyC (Y:l, X:c)
  typedef typename VecT<V>::type T;
  XG_WAVE_TASK(V, SEG, zb.on, zb, 1);  // (band-major: the metric rows of a band stay in the XCD's L2 for all outer indices)
  const int64_t base = o * ny * nx;
  const bool per_x = bc_x == XG_BC_PERIODIC, per_y = bc_y == XG_BC_PERIODIC;
  const bool edge_l = (i0 == 0), edge_r = (i0 + V >= nx);
  const bool bot = (j0 == 0);  // patch row -1 lies below the array
  const int64_t lidx = edge_l ? (per_x ? nx - 1 : 0) : i0 - 1;
  const int64_t ridx = edge_r ? (per_x ? 0 : nx - 1) : i0 + V;
  const bool shl = V > 1 && (ntl & 1);
  const bool own_l = !shl || (threadIdx.x & 63) == 0 || edge_l;
  const bool own_r = !shl || (threadIdx.x & 63) == 63 || edge_r;
  // patch row p (0 .. SEG+1) is array row j0 + p - 1, wrapped (periodic) or clamped; rows beyond ny (short tails) repeat
  // row ny-1 and feed nothing that is stored
  int64_t rw[SEG + 2];
#pragma unroll
  for (int p = 0; p < SEG + 2; ++p) {
    const int64_t g = j0 + p - 1;
    rw[p] = g < 0 ? (per_y ? ny - 1 : 0) : (g >= ny ? ((per_y && g == ny) ? 0 : ny - 1) : g);
  }
  // U[p][1 + k] / W[p][1 + k]: u / v at patch row p, column i0 + k; [0]: column i0 - 1, [V + 1]: column i0 + V
  real U[SEG + 2][V + 2], W[SEG + 2][V + 2];
  {
    const real* pu = u + base;
    const real* pv = v + base;
#pragma unroll
    for (int p = 0; p < SEG + 2; ++p) {
      const T tu = *reinterpret_cast<const T*>(pu + rw[p] * nx + i0);
      const T tv = *reinterpret_cast<const T*>(pv + rw[p] * nx + i0);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        U[p][1 + k] = vec_at(tu, k);
        W[p][1 + k] = vec_at(tv, k);
      }
      U[p][0] = own_l ? pu[rw[p] * nx + lidx] : real(0);
      W[p][0] = own_l ? pv[rw[p] * nx + lidx] : real(0);
      U[p][V + 1] = own_r ? pu[rw[p] * nx + ridx] : real(0);
      W[p][V + 1] = own_r ? pv[rw[p] * nx + ridx] : real(0);
    }
  }
  // the metric planes at the patch's points (wrapped / clamped like the fields: what a clamped index reads is overridden)
  real RZ[SEG + 1][V + 1], CF[SEG + 1][V + 1];
  T DX[SEG], DY[SEG];
  if (MET || COR) {
    int64_t mb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) mb[k] = mt.p[k] ? area_outer_off(mt.ai[k], o) : 0;
    const bool vec = (ntl & 8) != 0;
    auto plane = [&](real (&dst)[SEG + 1][V + 1], const real* m, int64_t mbase, int64_t sy, int64_t sx) {
#pragma unroll
      for (int p = 0; p < SEG + 1; ++p) {
        const int64_t off = mbase + rw[p + 1] * sy;
        const T row = vec ? *reinterpret_cast<const T*>(m + off + i0) : ldm<T>(m, off + i0 * sx, sx);
#pragma unroll
        for (int c = 0; c < V; ++c) dst[p][c] = vec_at(row, c);
        dst[p][V] = m[off + ridx * sx];
      }
    };
    if (MET) plane(RZ, mt.p[0], mb[0], mt.sy[0], mt.sx[0]);
    if (COR) plane(CF, mt.p[1], mb[1], mt.sy[1], mt.sx[1]);
    if (MET) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const int64_t ox = mb[2] + rw[s_ + 1] * mt.sy[2], oy = mb[3] + rw[s_ + 1] * mt.sy[3];
        DX[s_] = vec ? *reinterpret_cast<const T*>(mt.p[2] + ox + i0) : ldm<T>(mt.p[2], ox + i0 * mt.sx[2], mt.sx[2]);
        DY[s_] = vec ? *reinterpret_cast<const T*>(mt.p[3] + oy + i0) : ldm<T>(mt.p[3], oy + i0 * mt.sx[3], mt.sx[3]);
      }
    }
  }
  if (shl) {
#pragma unroll
    for (int p = 0; p < SEG + 2; ++p) {
      const real ul = from_lane_below(U[p][V]), wl = from_lane_below(W[p][V]);   // DPP wave_shr:1 (lane 0 is `own_l`)
      const real ur = from_lane_above(U[p][1]), wr = from_lane_above(W[p][1]);   // DPP wave_shl:1 (lane 63 is `own_r`)
      if (!own_l) { U[p][0] = ul; W[p][0] = wl; }
      if (!own_r) { U[p][V + 1] = ur; W[p][V + 1] = wr; }
    }
  }
  // the pads of the first stages at a fill boundary: u below row 0, v left of column 0
  if (bot && bc_y == XG_BC_FILL) {
#pragma unroll
    for (int c = 0; c < V + 2; ++c) U[0][c] = fill_y;
  }
  if (edge_l && bc_x == XG_BC_FILL) {
#pragma unroll
    for (int p = 0; p < SEG + 2; ++p) W[p][0] = fill_x;
  }
  const bool ovr_x_hi = edge_r && !per_x, ovr_x_lo = edge_l && !per_x, ovr_y_lo = bot && !per_y;
  const bool ext_x = bc_x == XG_BC_EXTEND, ext_y = bc_y == XG_BC_EXTEND;
  // zeta at rows j0 .. j0+SEG, columns i0 .. i0+V; the X-mean of v at the same rows; the Y-mean of u at the same columns
  real Z[SEG + 1][V + 1], VX[SEG + 1][V], UY[SEG][V + 1];
#pragma unroll
  for (int p = 0; p < SEG + 1; ++p) {
#pragma unroll
    for (int c = 0; c < V + 1; ++c) {
      real z = (W[p + 1][c + 1] - W[p + 1][c]) - (U[p + 1][c + 1] - U[p][c + 1]);
      if (MET) z = z / RZ[p][c];
      if (COR) z = z + CF[p][c];
      Z[p][c] = z;
      if (c < V) VX[p][c] = (W[p + 1][c] + W[p + 1][c + 1]) * real(0.5);
      if (p < SEG) UY[p][c] = (U[p][c + 1] + U[p + 1][c + 1]) * real(0.5);
    }
    if (ovr_x_hi) {
      Z[p][V] = ext_x ? Z[p][V - 1] : fill_x;
      if (p < SEG) UY[p][V] = ext_x ? UY[p][V - 1] : fill_x;
    }
    if (p > 0 && j0 + p == ny && !per_y) {  // the row above the last one (wave-uniform)
#pragma unroll
      for (int c = 0; c < V + 1; ++c) {
        Z[p][c] = ext_y ? Z[p - 1][c] : fill_y;
        if (c < V) VX[p][c] = ext_y ? VX[p - 1][c] : fill_y;
      }
    }
  }
  // ke at rows j0-1 .. j0+SEG-1, columns i0-1 .. i0+V-1: KE[p][c] is row j0 + p - 1, column i0 + c - 1
  real KE[SEG + 1][V + 1];
  {
    real UU[SEG + 1][V + 2], VV[SEG + 2][V + 1];
#pragma unroll
    for (int p = 0; p < SEG + 2; ++p) {
#pragma unroll
      for (int c = 0; c < V + 2; ++c) {
        if (p < SEG + 1) UU[p][c] = U[p][c] * U[p][c];
        if (c < V + 1) VV[p][c] = W[p][c] * W[p][c];
      }
      if (p < SEG + 1 && ovr_x_hi && !ext_x) UU[p][V + 1] = fill_x;
      if (p > 0 && j0 + p - 1 == ny && bc_y == XG_BC_FILL) {
#pragma unroll
        for (int c = 0; c < V + 1; ++c) VV[p][c] = fill_y;
      }
    }
#pragma unroll
    for (int p = 0; p < SEG + 1; ++p) {
#pragma unroll
      for (int c = 0; c < V + 1; ++c)
        KE[p][c] = real(0.5) * ((UU[p][c] + UU[p][c + 1]) * real(0.5) + (VV[p][c] + VV[p + 1][c]) * real(0.5));
    }
  }
#pragma unroll
  for (int p = 1; p < SEG + 1; ++p)
    if (ovr_x_lo) KE[p][0] = ext_x ? KE[p][1] : fill_x;
  if (ovr_y_lo) {
#pragma unroll
    for (int c = 1; c < V + 1; ++c) KE[0][c] = ext_y ? KE[1][c] : fill_y;
  }
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    if (s_ < nrow) {
      T gu, gv;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const real zy = (Z[s_][c] + Z[s_ + 1][c]) * real(0.5);
        const real vbar = (VX[s_][c] + VX[s_ + 1][c]) * real(0.5);
        real gx = KE[s_ + 1][c + 1] - KE[s_ + 1][c];
        if (MET) gx = gx / vec_at(DX[s_], c);
        vec_set(gu, c, zy * vbar - gx);
        const real zx = (Z[s_][c] + Z[s_][c + 1]) * real(0.5);
        const real ubar = (UY[s_][c] + UY[s_][c + 1]) * real(0.5);
        real gy = KE[s_ + 1][c + 1] - KE[s_][c + 1];
        if (MET) gy = gy / vec_at(DY[s_], c);
        vec_set(gv, c, real(-1) * (zx * ubar) - gy);
      }
      const int64_t off = base + (j0 + s_) * nx + i0;
      stg<T, NTS>(out_u + off, gu);  // (two outputs: plain `nt`, as K7c's gradient)
      stg<T, NTS>(out_v + off, gv);
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7k: the vector-invariant harmonic viscosity in the FORM of MITgcm's mom_vi_hdissip (harmonic part) in ONE pass, two fields
// in, two out.  WHAT THIS IS: D and zeta are the divergence and the curl of the RAW u, v in index space over the area -- not
// of the transports u * dyG, v * dxG and the circulations u * dxC, v * dyC, as mom_vi_hdissip's are.  With the metrics the
// result is the named term only on a grid of unit spacing; on a uniform grid of spacing h it is the term over h, and without
// the metrics h^2 times the term.  Measured against the analytic term in tests/test_convergence.py (a strict expected failure
// there until the kernel takes transports and circulations).
//   D    = ((u[j,i+1] - u[j,i]) + (v[j+1,i] - v[j,i])) [/ rA]  [* nu_d]              centre                K7b
//   zeta = ((v[j,i] - v[j,i-1]) - (u[j,i] - u[j-1,i])) [/ rAz] [* nu_z]              (Y:left, X:left)      K7
//   gu   = (D[j,i] - D[j,i-1]) [/ dxC] - (zeta[j+1,i] - zeta[j,i]) [/ dyG]           at u's points
//   gv   = (D[j,i] - D[j-1,i]) [/ dyC] + (zeta[j,i+1] - zeta[j,i]) [/ dxG]           at v's points
// in the chain's operation order (-ffp-contract=off, the compiler's IEEE quotients).  K7h's patch: per wave-task (SEG rows,
// one x-tile) a lane holds u and v at rows j0-1 .. j0+SEG, columns i0-1 .. i0+V -- the columns left and right of its vector
// from the neighbouring lanes (DPP), lane 0 / lane 63 / the edge lanes load their own.  A periodic axis wraps the patch's
// indices: every stage's periodic pad is then the stage's own value at the wrapped index.  At an extend / fill boundary the
// raw patch carries the pads of the FIRST stages, here on both sides (u below row 0 and right of the last column, v left of
// column 0 and above the last row: the clamped index or the fill value), and the two products override their own pads: D
// below and left, zeta above and right -- extend: the product at the clamped index, fill: the fill value itself.  The pads
// of zeta's products take their own fill pair (`zfill_x`, `zfill_y`): the chain's one-axis differences keep the sign of a
// -0.0 fill, its two-axis operators do not.  Every intermediate is formed once per lane; the two outputs of a cell share
// them.  32 B/cell in float64 (the six metric planes and 2-D coefficients stay in the L2) instead of ~150-200 for the chain.
// ------------------------------------------------------------------------------------------
struct HviscPlanes {        // the six metrics (all or none) and the two coefficients (both or none), broadcast strides
  const real* p[8];         // rA (centre), rAz (Y:l, X:l), dxC (Y:c, X:l), dyC (Y:l, X:c), dyG (Y:c, X:l), dxG (Y:l, X:c),
  AreaIdx ai[8];            // nu_d (centre), nu_z (Y:l, X:l)
  int64_t sy[8], sx[8];
};

template <int V, bool MET, bool VIS, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_hvisc(
    const real* __restrict__ u, const real* __restrict__ v, real* __restrict__ out_u, real* __restrict__ out_v, int64_t o0,
    u32 nouter, u32 nblk, int64_t ny, int64_t nx, FastDiv ntile, FastDiv nseg, ZBand zb, int bc_x, real fill_x, real zfill_x,
    int bc_y, real fill_y, real zfill_y, HviscPlanes mt, int ntl) {
  typedef typename VecT<V>::type T;
  XG_WAVE_TASK(V, SEG, zb.on, zb, 1);  // (band-major: the plane rows of a band stay in the XCD's L2 for all outer indices)
  const int64_t base = o * ny * nx;
  const bool per_x = bc_x == XG_BC_PERIODIC, per_y = bc_y == XG_BC_PERIODIC;
  const bool edge_l = (i0 == 0), edge_r = (i0 + V >= nx);
  const bool bot = (j0 == 0);  // patch row -1 lies below the array
  const int64_t lidx = edge_l ? (per_x ? nx - 1 : 0) : i0 - 1;
  const int64_t ridx = edge_r ? (per_x ? 0 : nx - 1) : i0 + V;
  const bool shl = V > 1 && (ntl & 1);
  const bool own_l = !shl || (threadIdx.x & 63) == 0 || edge_l;
  const bool own_r = !shl || (threadIdx.x & 63) == 63 || edge_r;
  // patch row p (0 .. SEG+1) is array row j0 + p - 1, wrapped (periodic) or clamped; rows beyond ny (short tails) repeat
  // row ny-1 and feed nothing that is stored
  int64_t rw[SEG + 2];
#pragma unroll
  for (int p = 0; p < SEG + 2; ++p) {
    const int64_t g = j0 + p - 1;
    rw[p] = g < 0 ? (per_y ? ny - 1 : 0) : (g >= ny ? ((per_y && g == ny) ? 0 : ny - 1) : g);
  }
  // U[p][1 + k] / W[p][1 + k]: u / v at patch row p, column i0 + k; [0]: column i0 - 1, [V + 1]: column i0 + V
  real U[SEG + 2][V + 2], W[SEG + 2][V + 2];
  {
    const real* pu = u + base;
    const real* pv = v + base;
#pragma unroll
    for (int p = 0; p < SEG + 2; ++p) {
      const T tu = *reinterpret_cast<const T*>(pu + rw[p] * nx + i0);
      const T tv = *reinterpret_cast<const T*>(pv + rw[p] * nx + i0);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        U[p][1 + k] = vec_at(tu, k);
        W[p][1 + k] = vec_at(tv, k);
      }
      U[p][0] = own_l ? pu[rw[p] * nx + lidx] : real(0);
      W[p][0] = own_l ? pv[rw[p] * nx + lidx] : real(0);
      U[p][V + 1] = own_r ? pu[rw[p] * nx + ridx] : real(0);
      W[p][V + 1] = own_r ? pv[rw[p] * nx + ridx] : real(0);
    }
  }
  // the planes at the patch's points (wrapped / clamped like the fields: what a clamped index reads is overridden).
  // At the centre, [p][c]: row j0 + p - 1, column i0 + c - 1; at the vorticity point, [p][c]: row j0 + p, column i0 + c
  real RA[SEG + 1][V + 1], ND[SEG + 1][V + 1], RZ[SEG + 1][V + 1], NZ[SEG + 1][V + 1];
  T DXC[SEG], DYC[SEG], DYG[SEG], DXG[SEG];
  if (MET || VIS) {
    int64_t mb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) mb[k] = mt.p[k] ? area_outer_off(mt.ai[k], o) : 0;
    const bool vec = (ntl & 8) != 0;
    // `r0`: the patch row of dst[0]; `left`: the extra column is the one left of the vector (else the one right of it)
    auto plane = [&](real (&dst)[SEG + 1][V + 1], int k, int r0, bool left) {
      const real* m = mt.p[k];
      const int64_t sy = mt.sy[k], sx = mt.sx[k];
#pragma unroll
      for (int p = 0; p < SEG + 1; ++p) {
        const int64_t off = mb[k] + rw[p + r0] * sy;
        const T row = vec ? *reinterpret_cast<const T*>(m + off + i0) : ldm<T>(m, off + i0 * sx, sx);
#pragma unroll
        for (int c = 0; c < V; ++c) dst[p][c + (left ? 1 : 0)] = vec_at(row, c);
        dst[p][left ? 0 : V] = m[off + (left ? lidx : ridx) * sx];
      }
    };
    auto rows = [&](T (&dst)[SEG], int k) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const int64_t off = mb[k] + rw[s_ + 1] * mt.sy[k];
        dst[s_] = vec ? *reinterpret_cast<const T*>(mt.p[k] + off + i0) : ldm<T>(mt.p[k], off + i0 * mt.sx[k], mt.sx[k]);
      }
    };
    if (MET) {
      plane(RA, 0, 0, true);
      plane(RZ, 1, 1, false);
    }
    if (VIS) {
      plane(ND, 6, 0, true);
      plane(NZ, 7, 1, false);
    }
    if (MET) {
      rows(DXC, 2);
      rows(DYC, 3);
      rows(DYG, 4);
      rows(DXG, 5);
    }
  }
  if (shl) {
#pragma unroll
    for (int p = 0; p < SEG + 2; ++p) {
      const real ul = from_lane_below(U[p][V]), wl = from_lane_below(W[p][V]);   // DPP wave_shr:1 (lane 0 is `own_l`)
      const real ur = from_lane_above(U[p][1]), wr = from_lane_above(W[p][1]);   // DPP wave_shl:1 (lane 63 is `own_r`)
      if (!own_l) { U[p][0] = ul; W[p][0] = wl; }
      if (!own_r) { U[p][V + 1] = ur; W[p][V + 1] = wr; }
    }
  }
  // the pads of the first stages at a fill boundary: u below row 0 and right of the last column, v left of column 0 and
  // above the last row (where two of them meet, the value feeds only products that are pads themselves)
  if (bot && bc_y == XG_BC_FILL) {
#pragma unroll
    for (int c = 0; c < V + 2; ++c) U[0][c] = fill_y;
  }
  if (bc_y == XG_BC_FILL) {
#pragma unroll
    for (int p = 1; p < SEG + 2; ++p) {
      if (j0 + p - 1 == ny) {  // the row above the last one (wave-uniform)
#pragma unroll
        for (int c = 0; c < V + 2; ++c) W[p][c] = fill_y;
      }
    }
  }
  if (bc_x == XG_BC_FILL) {
#pragma unroll
    for (int p = 0; p < SEG + 2; ++p) {
      if (edge_l) W[p][0] = fill_x;
      if (edge_r) U[p][V + 1] = fill_x;
    }
  }
  const bool ovr_x_hi = edge_r && !per_x, ovr_x_lo = edge_l && !per_x, ovr_y_lo = bot && !per_y;
  const bool ext_x = bc_x == XG_BC_EXTEND, ext_y = bc_y == XG_BC_EXTEND;
  // P = D [* nu_d] at rows j0-1 .. j0+SEG-1, columns i0-1 .. i0+V-1; Q = zeta [* nu_z] at rows j0 .. j0+SEG, columns
  // i0 .. i0+V
  real P[SEG + 1][V + 1], Q[SEG + 1][V + 1];
#pragma unroll
  for (int p = 0; p < SEG + 1; ++p) {
#pragma unroll
    for (int c = 0; c < V + 1; ++c) {
      real d = (U[p][c + 1] - U[p][c]) + (W[p + 1][c] - W[p][c]);
      if (MET) d = d / RA[p][c];
      if (VIS) d = d * ND[p][c];
      P[p][c] = d;
      real z = (W[p + 1][c + 1] - W[p + 1][c]) - (U[p + 1][c + 1] - U[p][c + 1]);
      if (MET) z = z / RZ[p][c];
      if (VIS) z = z * NZ[p][c];
      Q[p][c] = z;
    }
  }
#pragma unroll
  for (int p = 0; p < SEG + 1; ++p) {
    if (p > 0 && ovr_x_lo) P[p][0] = ext_x ? P[p][1] : fill_x;
    if (ovr_x_hi) Q[p][V] = ext_x ? Q[p][V - 1] : zfill_x;
    if (p > 0 && j0 + p == ny && !per_y) {  // the row above the last one (wave-uniform)
#pragma unroll
      for (int c = 0; c < V; ++c) Q[p][c] = ext_y ? Q[p - 1][c] : zfill_y;
    }
  }
  if (ovr_y_lo) {
#pragma unroll
    for (int c = 1; c < V + 1; ++c) P[0][c] = ext_y ? P[1][c] : fill_y;
  }
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    if (s_ < nrow) {
      T gu, gv;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        real dx = P[s_ + 1][c + 1] - P[s_ + 1][c];
        real zy = Q[s_ + 1][c] - Q[s_][c];
        real dy = P[s_ + 1][c + 1] - P[s_][c + 1];
        real zx = Q[s_][c + 1] - Q[s_][c];
        if (MET) {
          dx = dx / vec_at(DXC[s_], c);
          zy = zy / vec_at(DYG[s_], c);
          dy = dy / vec_at(DYC[s_], c);
          zx = zx / vec_at(DXG[s_], c);
        }
        vec_set(gu, c, dx - zy);
        vec_set(gv, c, dy + zx);
      }
      const int64_t off = base + (j0 + s_) * nx + i0;
      stg<T, NTS>(out_u + off, gu);  // (two outputs: plain `nt`, as K7h)
      stg<T, NTS>(out_v + off, gv);
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7i: the horizontal gradient of the hydrostatic pressure in ONE pass over (lead, Z, Y, X), one field in, two out:
//   t[k]  = nan0(b[k] * w[k])                     the weighted buoyancy, a NaN product counts as 0 (the scans' nancumsum)
//   p[0]  = Z pad (fill: fill_z, extend: p[1]),   p[k+1] = t[0] + .. + t[k], added in sequence (the first sum is t[0] itself)
//   pc[k] = (p[k] + p[k+1]) / 2                   outer -> center, no pad
//   gx = (pc[i] - pc[i-1]) [/ dxC],  gy = (pc[j] - pc[j-1]) [/ dyC]      K7c's gradient, its X / Y boundaries
// i.e. cumint (center -> outer) -> interp -> gradient.  K7f's decomposition: a wave owns one (lead, Y segment, X tile) column
// and marches Z forward with the running sums in registers, so b is read once and gx, gy written once: 24 B/cell in float64
// against about 56 for the chain.  pc of the row below the segment comes from that row's own running sum, marched in the same
// wave (1 + 1/SEG reads of b, the extra row an L2 hit: it is the segment before's last row); pc left of the lane's vector
// comes from the lane before it, which formed it with the same arithmetic (DPP, K7c's move) -- only the tile's first lane
// (and every lane of the narrow form) marches that column's sum itself.  Fill / extend at row 0 / column 0 need neither.
// The loads form K7f's rolling window of levels ahead of the sums.  The Z weight is one wave-uniform load per level when it
// varies along Z (and leading dims) only, else its rows are read with the level; the dxC / dyC rows stay in registers
// unless they vary along Z.
// ------------------------------------------------------------------------------------------
template <typename T, int SEG>
struct PgLevel {  // what one level of a column brings: SEG rows of b with the element left of the lane, the row below them
  T bb[SEG], bel;
  real bl[SEG];
};

// one cell's step: the product, the next running sum (kept in `acc`), the mean of the two sums around the level
template <typename A>
__device__ __forceinline__ A pg_cell(A& acc, A prod, bool started, bool zfill, real fill_z) {
  const A t = nan0(prod);
  const A nxt = started ? acc + t : t;
  const A prv = started ? acc : (zfill ? splat<A>(fill_z) : nxt);
  acc = nxt;
  return op2<XG_OP_INTERP>(prv, nxt);
}

template <int V, bool MET, bool NTS, int SEG, int U>
__global__ __launch_bounds__(BLOCK) void k_pgrad(
    const real* __restrict__ b, real* __restrict__ out_x, real* __restrict__ out_y, int64_t o0, u32 nouter, u32 nblk,
    int64_t nz, int64_t ny, int64_t nx, FastDiv ntile, FastDiv nseg, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z,
    real fill_z, VolIdx wz, VolIdx mx, VolIdx my, int ntl) {
  typedef typename VecT<V>::type T;
  typedef PgLevel<T, SEG> L;
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const int64_t plane = ny * nx;
  const int64_t col = o * nz * plane;  // level 0 of this lead index (int64: a 4320^2 x 90 field has more than 2^32 cells)
  // X as K7c: the column left of the lane's vector (periodic: column nx - 1 left of column 0); `march_l`: this lane forms
  // that column's pc itself -- not at a fill / extend edge, where the pad replaces it
  const bool edge_l = (i0 == 0);
  const bool per_x = bc_x == XG_BC_PERIODIC;
  const int64_t lidx = edge_l ? (per_x ? nx - 1 : 0) : i0 - 1;
  const bool shl = V > 1 && (ntl & 1);
  const bool own_l = !shl || (threadIdx.x & 63) == 0 || edge_l;
  const bool march_l = own_l && !(edge_l && !per_x);
  // Y: the row below the segment (periodic: row ny - 1 below row 0); wave-uniform
  const bool edge_b = (j0 == 0);
  const bool march_b = !(edge_b && bc_y != XG_BC_PERIODIC);
  const int64_t jb = edge_b ? (march_b ? ny - 1 : 0) : j0 - 1;
  int64_t ro[SEG];  // the segment's rows in a plane (short tails repeat the last row)
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) ro[s_] = (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * nx;
  const real* pb = b + col;

  auto fetch = [&](int64_t k) -> L {
    L x;
    const real* pk = pb + k * plane;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      x.bb[s_] = *reinterpret_cast<const T*>(pk + ro[s_] + i0);
      x.bl[s_] = march_l ? pk[ro[s_] + lidx] : real(0);
    }
    x.bel = march_b ? *reinterpret_cast<const T*>(pk + jb * nx + i0) : splat<T>(real(0));
    return x;
  };

  // the Z weight: `wflat` (it varies along Z and leading dims only) is one wave-uniform load per level
  const bool wflat = wz.sy == 0 && wz.sx == 0;
  const int64_t wzo = wz.p ? area_outer_off(wz.ai, o) : 0;
  // dxC / dyC rows: in registers, loaded again per level only when the plane varies along Z
  T dxr[SEG], dyr[SEG];
  int64_t mxo = 0, myo = 0;
  if (MET) {
    if (mx.p) {
      mxo = area_outer_off(mx.ai, o) + j0 * mx.sy + i0 * mx.sx;
      load_rows<T, SEG>(dxr, mx.p, mxo, mx.sy, mx.sx, nrow, (ntl & 8) != 0);
    }
    if (my.p) {
      myo = area_outer_off(my.ai, o) + j0 * my.sy + i0 * my.sx;
      load_rows<T, SEG>(dyr, my.p, myo, my.sy, my.sx, nrow, (ntl & 16) != 0);
    }
  }

  T p[SEG], pbel = splat<T>(real(0));  // the running sums p[k]: the segment's rows, the row below, the column to the left
  real pl[SEG];
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    p[s_] = splat<T>(real(0));
    pl[s_] = real(0);
  }
  const bool zfill = bc_z == XG_BC_FILL;
  bool started = false;
  real* px = out_x + col + j0 * nx + i0;
  real* py = out_y + col + j0 * nx + i0;

  auto step = [&](int64_t k, const L& x) {
    T tc[SEG], tb = x.bel;
    real tl[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      tc[s_] = x.bb[s_];
      tl[s_] = x.bl[s_];
    }
    if (wz.p) {
      const int64_t wk = wzo + k * wz.sz;
      if (wflat) {
        const real zw = wz.p[wk];
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) {
          tc[s_] = tc[s_] * splat<T>(zw);
          tl[s_] = tl[s_] * zw;
        }
        tb = tb * splat<T>(zw);
      } else {
        T wr[SEG], wb[1];
        real wl[SEG];
        load_rows<T, SEG>(wr, wz.p, wk + j0 * wz.sy + i0 * wz.sx, wz.sy, wz.sx, nrow, (ntl & 4) != 0);
        load_rows<T, 1>(wb, wz.p, wk + jb * wz.sy + i0 * wz.sx, wz.sy, wz.sx, 1, (ntl & 4) != 0);
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_)
          wl[s_] = march_l ? wz.p[wk + (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * wz.sy + lidx * wz.sx] : real(0);
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) {
          tc[s_] = tc[s_] * wr[s_];
          tl[s_] = tl[s_] * wl[s_];
        }
        tb = tb * wb[0];
      }
    }
    if (MET && k > 0) {
      if (mx.p && mx.sz != 0) load_rows<T, SEG>(dxr, mx.p, mxo + k * mx.sz, mx.sy, mx.sx, nrow, (ntl & 8) != 0);
      if (my.p && my.sz != 0) load_rows<T, SEG>(dyr, my.p, myo + k * my.sz, my.sy, my.sx, nrow, (ntl & 16) != 0);
    }
    T pc[SEG];
    real pcl[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      pc[s_] = pg_cell(p[s_], tc[s_], started, zfill, fill_z);
      pcl[s_] = pg_cell(pl[s_], tl[s_], started, zfill, fill_z);
    }
    const T pcb = pg_cell(pbel, tb, started, zfill, fill_z);
    started = true;
    if (shl) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const real left = from_lane_below(vec_last(pc[s_]));  // DPP wave_shr:1 (lane 0 reads 0 and is `own_l`)
        if (!own_l) pcl[s_] = left;
      }
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        real left = pcl[s_];
        if (edge_l && !per_x) left = (bc_x == XG_BC_FILL) ? fill_x : vec_first(pc[s_]);
        T below = (s_ == 0) ? pcb : pc[(s_ > 0) ? s_ - 1 : 0];
        if (s_ == 0 && !march_b) below = (bc_y == XG_BC_FILL) ? splat<T>(fill_y) : pc[0];
        T gx = dvdx_of(pc[s_], left);
        T gy = pc[s_] - below;
        if (MET) {
          if (mx.p) gx = gx / dxr[s_];
          if (my.p) gy = gy / dyr[s_];
        }
        stg_s<T, NTS>(px + k * plane + s_ * nx, gx);
        stg_s<T, NTS>(py + k * plane + s_ * nx, gy);
      }
    }
  };

  // the rolling window (K7f's): every consumed level is replaced by the load of the level U steps ahead
  L win[U];
#pragma unroll
  for (int q = 0; q < U; ++q)
    if (q < nz) win[q] = fetch(q);
  int64_t k = 0;
  for (; k + 2 * U <= nz; k += U) {
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const L x = win[q];
      win[q] = fetch(k + U + q);
      step(k + q, x);
    }
  }
  for (; k < nz; k += U) {  // the last one or two windows: refills and consumes guarded (wave-uniform tests)
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const L x = win[q];
      if (k + U + q < nz) win[q] = fetch(k + U + q);
      if (k + q < nz) step(k + q, x);
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7j: the vertical advection of horizontal momentum in ONE pass over (lead, Z, Y, X), three fields in, two out:
//   pu[k] = interp_x(w[k]) * (u[k] - u[k-1]),   pv[k] = interp_y(w[k]) * (v[k] - v[k-1])      at (Z:left), over u's / v's column
//   gu[k] = -((pu[k] + pu[k+1]) / 2) [/ mu],    gv[k] = -((pv[k] + pv[k+1]) / 2) [/ mv]
// i.e. interp (X / Y, center -> left) and diff (Z, center -> left), their product, interp (Z, left -> center), the negation,
// the division.  Every stage pads where the chain pads: w left of the first column and below the first row, u and v above
// level 0 (periodic: level nz-1, extend: level 0, fill: fill_z), the PRODUCTS beyond level nz-1 (periodic: pu[0], extend:
// pu[nz-1], fill: fill_z itself).  K7e's decomposition: a wave owns one (lead, Y segment, X tile) column and marches
// k = 0 .. nz-1 with u[k], v[k], pu[k] and pv[k] in registers; the rows of level k+1 are read at level k and form pu[k+1].
// u, v and w are read once and gu, gv written once: 40 B/cell in float64.  w of the row below the segment is one more row per level (an L2 hit:
// the segment before's last row); w left of the lane's vector comes from the lane before it by DPP, the tile's first lane
// and the row's edge load or pad their own.  No running sum: all three Z boundaries are served.  The metrics (the Z metric
// at u's / v's points) are one broadcast array per output; rows that do not vary along Z are loaded once per wave.
// ------------------------------------------------------------------------------------------
template <typename T, int SEG>
struct VmLevel {  // what one level of a column brings: SEG rows of u, v and w, the w row below them, w left of the lane
  T uu[SEG], vv[SEG], ww[SEG], wb;
  real wl[SEG];
};

template <int V, bool MET, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_vmomadv(
    const real* __restrict__ u, const real* __restrict__ v, const real* __restrict__ w, real* __restrict__ out_u,
    real* __restrict__ out_v, int64_t o0, u32 nouter, u32 nblk, int64_t nz, int64_t ny, int64_t nx, FastDiv ntile,
    FastDiv nseg, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z, real fill_z, VolIdx mu, VolIdx mv, int ntl) {
  typedef typename VecT<V>::type T;
  typedef VmLevel<T, SEG> L;
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const int64_t plane = ny * nx;
  const int64_t col = o * nz * plane;  // level 0 of this lead index (int64: a 4320^2 x 90 field has more than 2^32 cells)
  // X as K7e's T: w left of the lane's vector (periodic: column nx - 1, extend: column 0 itself); Y: the row below the
  // segment (periodic: row ny - 1 below row 0, extend: row 0 itself); a fill edge loads the clamped cell and replaces it
  const LaneEdges e = lane_edges<V>(i0, nx, bc_x, ntl);
  const bool fill_l = e.edge_l && bc_x == XG_BC_FILL;
  const bool fill_b = j0 == 0 && bc_y == XG_BC_FILL;
  const int64_t rb = (j0 > 0 ? j0 - 1 : ((bc_y == XG_BC_PERIODIC) ? ny - 1 : 0)) * nx;
  int64_t ro[SEG];  // the segment's rows in a plane (short tails repeat the last row)
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) ro[s_] = (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * nx;

  auto fetch = [&](int64_t k) -> L {
    L x;
    const int64_t lv = col + k * plane;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      x.uu[s_] = *reinterpret_cast<const T*>(u + lv + ro[s_] + i0);
      x.vv[s_] = *reinterpret_cast<const T*>(v + lv + ro[s_] + i0);
      x.ww[s_] = *reinterpret_cast<const T*>(w + lv + ro[s_] + i0);
      x.wl[s_] = e.own_l ? w[lv + ro[s_] + e.lidx] : real(0);
    }
    x.wb = *reinterpret_cast<const T*>(w + lv + rb + i0);
    return x;
  };
  // the two products of a level from its rows and the level above's u and v
  auto products = [&](const L& x, const T (&up)[SEG], const T (&vp)[SEG], T (&pu)[SEG], T (&pv)[SEG]) {
    real wl[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) wl[s_] = x.wl[s_];
    if (e.shl) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const real left = from_lane_below(vec_last(x.ww[s_]));  // DPP wave_shr:1 (lane 0 reads 0 and is `own_l`)
        if (!e.own_l) wl[s_] = left;
      }
    }
    const T wb = fill_b ? splat<T>(fill_y) : x.wb;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      const real left = fill_l ? fill_x : wl[s_];
      pu[s_] = interp_left_of(x.ww[s_], left) * op2<XG_OP_DIFF>(up[s_], x.uu[s_]);
      pv[s_] = op2<XG_OP_INTERP>(s_ == 0 ? wb : x.ww[(s_ > 0) ? s_ - 1 : 0], x.ww[s_]) * op2<XG_OP_DIFF>(vp[s_], x.vv[s_]);
    }
  };

  // the metric rows: in registers, loaded again per level only when the array varies along Z
  T mur[SEG], mvr[SEG];
  int64_t muo = 0, mvo = 0;
  if (MET) {
    if (mu.p) {
      muo = area_outer_off(mu.ai, o) + j0 * mu.sy + i0 * mu.sx;
      load_rows<T, SEG>(mur, mu.p, muo, mu.sy, mu.sx, nrow, (ntl & 4) != 0);
    }
    if (mv.p) {
      mvo = area_outer_off(mv.ai, o) + j0 * mv.sy + i0 * mv.sx;
      load_rows<T, SEG>(mvr, mv.p, mvo, mv.sy, mv.sx, nrow, (ntl & 8) != 0);
    }
  }

  // level 0: pu[0], pv[0] from u and v padded above it; periodic Z keeps them for the pad beyond the last level
  T uc[SEG], vc[SEG], puc[SEG], pvc[SEG], pu0[SEG], pv0[SEG];
  {
    const L x = fetch(0);
    const int64_t ka = col + ((bc_z == XG_BC_PERIODIC) ? nz - 1 : 0) * plane;
    T ua[SEG], va[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      ua[s_] = (bc_z == XG_BC_FILL) ? splat<T>(fill_z) : *reinterpret_cast<const T*>(u + ka + ro[s_] + i0);
      va[s_] = (bc_z == XG_BC_FILL) ? splat<T>(fill_z) : *reinterpret_cast<const T*>(v + ka + ro[s_] + i0);
    }
    products(x, ua, va, puc, pvc);
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      uc[s_] = x.uu[s_];
      vc[s_] = x.vv[s_];
      pu0[s_] = puc[s_];
      pv0[s_] = pvc[s_];
    }
  }
  real* pgu = out_u + col + j0 * nx + i0;
  real* pgv = out_v + col + j0 * nx + i0;
  for (int64_t k = 0; k < nz; ++k) {
    T pun[SEG], pvn[SEG];
    if (k + 1 < nz) {
      const L x = fetch(k + 1);
      products(x, uc, vc, pun, pvn);
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        uc[s_] = x.uu[s_];
        vc[s_] = x.vv[s_];
      }
    } else {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        pun[s_] = (bc_z == XG_BC_PERIODIC) ? pu0[s_] : ((bc_z == XG_BC_EXTEND) ? puc[s_] : splat<T>(fill_z));
        pvn[s_] = (bc_z == XG_BC_PERIODIC) ? pv0[s_] : ((bc_z == XG_BC_EXTEND) ? pvc[s_] : splat<T>(fill_z));
      }
    }
    if (MET && k > 0) {
      if (mu.p && mu.sz != 0) load_rows<T, SEG>(mur, mu.p, muo + k * mu.sz, mu.sy, mu.sx, nrow, (ntl & 4) != 0);
      if (mv.p && mv.sz != 0) load_rows<T, SEG>(mvr, mv.p, mvo + k * mv.sz, mv.sy, mv.sx, nrow, (ntl & 8) != 0);
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        T gu = -op2<XG_OP_INTERP>(puc[s_], pun[s_]);
        T gv = -op2<XG_OP_INTERP>(pvc[s_], pvn[s_]);
        if (MET) {
          if (mu.p) gu = gu / mur[s_];
          if (mv.p) gv = gv / mvr[s_];
        }
        stg_s<T, NTS>(pgu + k * plane + s_ * nx, gu);
        stg_s<T, NTS>(pgv + k * plane + s_ * nx, gv);
      }
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      puc[s_] = pun[s_];
      pvc[s_] = pvn[s_];
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7l: vertical diffusion d/dz(kappa da/dz) in ONE pass over (lead, Z, Y, X), one field in, one out:
//   f[k]   = ((a[k] - a[k-1]) [/ mf[k]]) [* kappa[k]]        the diffusive flux between level k-1 and level k
//   out[k] = (f[k+1] - f[k]) [/ mc[k]]
// i.e. derivative (Z, center -> left | outer), the product with kappa, derivative (Z, left | outer -> center).  Pads as the
// chain's.  `left` (nz flux levels): a above level 0 (periodic: a[nz-1], extend: a[0], fill: fill_z), then the FLUX beyond
// level nz-1 (periodic: f[0], extend: f[nz-1], fill: fill_z itself).  `outer` (nz+1 flux levels; kappa and mf have nz+1
// levels): a on both sides (periodic: a[nz-1] above, a[0] below; extend: a[0], a[nz-1]; fill: fill_z), the flux needs none.
// K7e's decomposition without its X and Y neighbours: a wave owns one (lead, Y segment, X tile) column and marches
// k = 0 .. nz-1 with a[k] and f[k] in registers; the rows of a[k+1], kappa[k+1] and mf[k+1] are read at level k and form
// f[k+1].  a and kappa are read once and out written once: 24 B/cell in float64 (16 with a profile kappa(Z) or none).
// kappa and the two metrics are one broadcast array each; rows that do not vary along Z are loaded once per wave.  Periodic
// Z costs one more row read before the march (and, `outer`, one after it).
// ------------------------------------------------------------------------------------------
template <int V, bool KAP, bool MET, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_vdiff(
    const real* __restrict__ a, real* __restrict__ out, int64_t o0, u32 nouter, u32 nblk, int64_t nz, int64_t ny,
    int64_t nx, FastDiv ntile, FastDiv nseg, int outer, int bc_z, real fill_z, VolIdx kp, VolIdx mf, VolIdx mc, int ntl) {
  typedef typename VecT<V>::type T;
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const int64_t plane = ny * nx;
  const int64_t col = o * nz * plane;  // level 0 of this lead index (int64: a 4320^2 x 90 field has more than 2^32 cells)
  int64_t ro[SEG];  // the segment's rows in a plane (short tails repeat the last row)
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) ro[s_] = (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * nx;
  auto rows = [&](T (&x)[SEG], int64_t k) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) x[s_] = *reinterpret_cast<const T*>(a + col + k * plane + ro[s_] + i0);
  };

  // the rows of kappa and of the two metrics: in registers, loaded again per level only when the array varies along Z
  T kr[SEG], mfr[SEG], mcr[SEG];
  int64_t kpo = 0, mfo = 0, mco = 0;
  if (KAP) {
    kpo = area_outer_off(kp.ai, o) + j0 * kp.sy + i0 * kp.sx;
    load_rows<T, SEG>(kr, kp.p, kpo, kp.sy, kp.sx, nrow, (ntl & 4) != 0);
  }
  if (MET) {
    if (mf.p) {
      mfo = area_outer_off(mf.ai, o) + j0 * mf.sy + i0 * mf.sx;
      load_rows<T, SEG>(mfr, mf.p, mfo, mf.sy, mf.sx, nrow, (ntl & 8) != 0);
    }
    if (mc.p) {
      mco = area_outer_off(mc.ai, o) + j0 * mc.sy + i0 * mc.sx;
      load_rows<T, SEG>(mcr, mc.p, mco, mc.sy, mc.sx, nrow, (ntl & 16) != 0);
    }
  }
  // the flux between two levels from the rows of kappa and mf that are in registers
  auto flux = [&](const T (&lo)[SEG], const T (&hi)[SEG], T (&f)[SEG]) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      T d = op2<XG_OP_DIFF>(lo[s_], hi[s_]);
      if (MET) {
        if (mf.p) d = d / mfr[s_];
      }
      if (KAP) d = d * kr[s_];
      f[s_] = d;
    }
  };

  // level 0: f[0] from a padded above it; `left` with periodic Z keeps it for the pad beyond the last level
  T ac[SEG], fc[SEG], f0[SEG];
  {
    T aa[SEG];
    rows(ac, 0);
    if (bc_z == XG_BC_PERIODIC) rows(aa, nz - 1);
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (bc_z == XG_BC_FILL) aa[s_] = splat<T>(fill_z);
      else if (bc_z == XG_BC_EXTEND) aa[s_] = ac[s_];
    }
    flux(aa, ac, fc);
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) f0[s_] = fc[s_];
  }
  real* po = out + col + j0 * nx + i0;
  for (int64_t k = 0; k < nz; ++k) {
    const bool more = k + 1 < nz;
    T fn[SEG];
    if (more || outer) {
      // flux level k+1 exists: a[k+1] (`outer`, last level: the pad of a), then the rows of kappa and mf at k+1
      T an[SEG];
      if (more || bc_z == XG_BC_PERIODIC) rows(an, more ? k + 1 : 0);
      if (!more) {
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) {
          if (bc_z == XG_BC_FILL) an[s_] = splat<T>(fill_z);
          else if (bc_z == XG_BC_EXTEND) an[s_] = ac[s_];
        }
      }
      if (KAP && kp.sz != 0) load_rows<T, SEG>(kr, kp.p, kpo + (k + 1) * kp.sz, kp.sy, kp.sx, nrow, (ntl & 4) != 0);
      if (MET) {
        if (mf.p && mf.sz != 0) load_rows<T, SEG>(mfr, mf.p, mfo + (k + 1) * mf.sz, mf.sy, mf.sx, nrow, (ntl & 8) != 0);
      }
      flux(ac, an, fn);
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) ac[s_] = an[s_];
    } else {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_)
        fn[s_] = (bc_z == XG_BC_PERIODIC) ? f0[s_] : ((bc_z == XG_BC_EXTEND) ? fc[s_] : splat<T>(fill_z));
    }
    if (MET && k > 0) {
      if (mc.p && mc.sz != 0) load_rows<T, SEG>(mcr, mc.p, mco + k * mc.sz, mc.sy, mc.sx, nrow, (ntl & 16) != 0);
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        T z = op2<XG_OP_DIFF>(fc[s_], fn[s_]);
        if (MET) {
          if (mc.p) z = z / mcr[s_];
        }
        stg_s<T, NTS>(po + k * plane + s_ * nx, z);
      }
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) fc[s_] = fn[s_];
  }
}

// ------------------------------------------------------------------------------------------
// K7m / K7o, the implicit sweeps: ONE kernel.  K7m: implicit (backward-Euler) vertical diffusion, (I - dt D) x = a with
// D = d/dz(kappa d/dz) under the no-flux condition at the top and at the bottom, over (lead, Z, Y, X) in ONE launch: the
// Thomas algorithm per column, a forward and a backward sweep over the same column.  Faces k = 1 .. nz-1 (face k between
// level k-1 and level k), in the field's type, no FMA:
//   w[k]  = dt * (kappa[k] [/ mf[k]])                  (kappa absent: 1)
//   lo[k] = w[k] [/ mc[k]],  up[k-1] = w[k] [/ mc[k-1]]
//   b     = 1 [+ lo[k], k > 0] [+ up[k], k < nz-1]
//   m     = b [- lo[k] * c[k-1]],  r = 1 / m,  c[k] = up[k] * r,  d[k] = (a[k] [+ lo[k] * d[k-1]]) * r       forward
//   x[nz-1] = d[nz-1],  x[k] = d[k] + c[k] * x[k+1]                                                          backward
// kappa and mf are indexed by face (nz or nz + 1 of them: faces 0 and nz are never read), mc by level; no pivoting (for
// kappa, dt >= 0 and positive metrics m >= 1 and 0 <= c < 1).  K7l's geometry: a wave owns one (lead, Y segment, X tile)
// column set.  The forward sweep marches k = 0 .. nz-1 with c[k-1], d[k-1] and w[k] in registers, stores d[k] into `out` and
// c[k] into the workspace `cw` (the field's shape); the backward sweep marches k = nz-2 .. 0, reads both back and overwrites
// out[k] with x[k].  The coefficients lo, up, b do not depend on the recurrence: those of level k+1 (and the loads behind
// them) are formed BEFORE level k's dependent chain (a reciprocal, two products, a sum), as K7l reads level k+1 at level k;
// the backward sweep reads level k-1 before it forms level k.
// NO barrier, LDS exchange or atomic: every lane reads back exactly the elements it stored itself -- same lane, same level,
// same rows, same columns -- and no other lane or wave touches them.  A store followed by a load of the same address in one
// thread is a dependence of plain program order: the compiler keeps the order of the two accesses, and the hardware performs
// one wave's vector memory accesses to one address in the order they were issued (the vector L1 writes through).  For the
// same reason the stores of c and d are always plain (they are read again by the same wave); only the final store of x
// obeys `nt_store`.
// float64 with a 3-D kappa: a 8 + kappa 8 + d out and back 16 + c out and back 16 + x 8 = 56 B/cell (48 with a profile
// kappa(Z) or none); the read-backs may come from the L2 / the Infinity Cache.
// K7o, implicit vertical viscosity of a C-grid velocity, is this kernel for u and for v with ONE viscosity nu at the centre
// points: SRC says, at compile time, where the coefficient stage of face k takes kappa[k] from --
//   VI_ONE:   1                                    VI_KAPPA: the array kappa, as above
//   VI_NU_U (u, at X:left):   kappa[k] = (nu[k, j, i-1] + nu[k, j, i]) * 0.5       interp_left_of, K7j's neighbour
//   VI_NU_V (v, at Y:left):   kappa[k] = (nu[k, j-1, i] + nu[k, j, i]) * 0.5       op2<XG_OP_INTERP>, K7j's row below
// -- and everything after it is the one recurrence in the one order.  nu (as `kp`, required, loaded per face: it is a field
// of the faces) is padded by `bc` / `fill` left of column 0 / below row 0 (periodic: column nx-1 / row ny-1, extend: column
// 0 / row 0, fill: the fill value in place of the loaded value); there is no pad along Z and faces 0 and nz are never read.
// A wave owns a column set of ONE component and the launcher starts the kernel once per component (both components in one
// wave would keep two sets of the pipelined coefficients live).  u: nu left of the lane's vector comes from the lane below
// by DPP where `ntl` bit 0 allows, the tile's first lane and the row's edge load their own; v: the row below the segment is
// one more row per face (the segment before's last row: an L2 hit).  float64 per component: a 8 + nu 8 + d out and back 16 +
// c out and back 16 + x 8 = 56 B/cell, 112 for both (nu read by each).
// `bc` and `fill` stand LAST among the arguments: in front of `kp` they move the argument offsets of the VI_ONE / VI_KAPPA
// instances, and the float64 V=2 instance with kappa and metrics came out with its blocks laid out otherwise and 0.07 ms
// slower at 14.8 ms on 4320 x 4320 x 90 (EXPERIMENTS.md "Z-march families").
// ------------------------------------------------------------------------------------------
enum { VI_ONE = 0, VI_KAPPA = 1, VI_NU_U = 2, VI_NU_V = 3 };  // k_vimpl's SRC

template <int V, int SRC, bool MET, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_vimpl(
    const real* __restrict__ a, real* __restrict__ cw, real* __restrict__ out, int64_t o0, u32 nouter, u32 nblk, int64_t nz,
    int64_t ny, int64_t nx, FastDiv ntile, FastDiv nseg, real dt, VolIdx kp, VolIdx mf, VolIdx mc, int ntl, int bc, real fill) {
  typedef typename VecT<V>::type T;
  constexpr bool NU = SRC == VI_NU_U || SRC == VI_NU_V;
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const int64_t plane = ny * nx;
  const int64_t col = o * nz * plane;  // level 0 of this lead index (int64: a 4320^2 x 90 field has more than 2^32 cells)
  int64_t ro[SEG];  // the segment's rows in a plane (short tails repeat the last row, which this lane owns too)
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) ro[s_] = col + (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * nx + i0;
  const T one = splat<T>(real(1)), tdt = splat<T>(dt);
  // nu, u: left of the lane's vector (periodic: column nx - 1, extend: column 0 itself); v: the row below the segment
  // (periodic: row ny - 1 below row 0, extend: row 0 itself); a fill edge loads the clamped cell and replaces it
  const LaneEdges e = lane_edges<V>(i0, nx, bc, ntl);
  const bool fill_e = (SRC == VI_NU_U ? e.edge_l : j0 == 0) && bc == XG_BC_FILL;
  const int64_t rb = j0 > 0 ? j0 - 1 : ((bc == XG_BC_PERIODIC) ? ny - 1 : 0);

  // the rows of kappa and of the two metrics: loaded per face / level only when the array varies along Z, else once (and
  // not at all for a column of one level, which has no face); nu per face
  T kr[SEG], mfr[SEG], mcr[SEG];
  int64_t kpb = 0, kpo = 0, mfo = 0, mco = 0;
  if (SRC != VI_ONE) {
    kpb = area_outer_off(kp.ai, o);  // kappa's / nu's (Z, Y, X) volume of this lead index
    kpo = kpb + j0 * kp.sy + i0 * kp.sx;
  }
  if (SRC == VI_KAPPA) {
    if (kp.sz == 0 && nz > 1) load_rows<T, SEG>(kr, kp.p, kpo, kp.sy, kp.sx, nrow, (ntl & 4) != 0);
  }
  if (MET) {
    if (mf.p) {
      mfo = area_outer_off(mf.ai, o) + j0 * mf.sy + i0 * mf.sx;
      if (mf.sz == 0 && nz > 1) load_rows<T, SEG>(mfr, mf.p, mfo, mf.sy, mf.sx, nrow, (ntl & 8) != 0);
    }
    if (mc.p) {
      mco = area_outer_off(mc.ai, o) + j0 * mc.sy + i0 * mc.sx;
      if (mc.sz == 0 && nz > 1) load_rows<T, SEG>(mcr, mc.p, mco, mc.sy, mc.sx, nrow, (ntl & 16) != 0);
    }
  }
  // w = w[k + 1] on return from coef(k) (k < nz-1), which needs w = w[k] on entry (k > 0): the coefficients of level k
  T w[SEG];
  auto coef = [&](int64_t k, T (&a_)[SEG], T (&lo_)[SEG], T (&up_)[SEG], T (&b_)[SEG]) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) a_[s_] = *reinterpret_cast<const T*>(a + ro[s_] + k * plane);
    if (MET && nz > 1) {
      if (mc.p && mc.sz != 0) load_rows<T, SEG>(mcr, mc.p, mco + k * mc.sz, mc.sy, mc.sx, nrow, (ntl & 16) != 0);
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) b_[s_] = one;
    if (k > 0) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        T l = w[s_];
        if (MET) {
          if (mc.p) l = l / mcr[s_];
        }
        lo_[s_] = l;
        b_[s_] = b_[s_] + l;
      }
    }
    if (k + 1 < nz) {
      // face k + 1; nu: its rows and its neighbour, every load before the first shuffle
      const int64_t fz = (k + 1) * kp.sz;
      if (NU || (SRC == VI_KAPPA && kp.sz != 0)) load_rows<T, SEG>(kr, kp.p, kpo + fz, kp.sy, kp.sx, nrow, (ntl & 4) != 0);
      T kap[SEG];
      if (SRC == VI_NU_U) {
        real kl[SEG];
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_)
          kl[s_] = e.own_l ? kp.p[kpb + fz + (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * kp.sy + e.lidx * kp.sx] : real(0);
        if (e.shl) {
#pragma unroll
          for (int s_ = 0; s_ < SEG; ++s_) {
            const real left = from_lane_below(vec_last(kr[s_]));  // DPP wave_shr:1 (lane 0 reads 0 and is `own_l`)
            if (!e.own_l) kl[s_] = left;
          }
        }
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) kap[s_] = interp_left_of(kr[s_], fill_e ? fill : kl[s_]);
      } else if (SRC == VI_NU_V) {
        T kb[1];
        load_rows<T, 1>(kb, kp.p, kpb + fz + rb * kp.sy + i0 * kp.sx, kp.sy, kp.sx, 1, (ntl & 4) != 0);
        if (fill_e) kb[0] = splat<T>(fill);
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) kap[s_] = op2<XG_OP_INTERP>(s_ == 0 ? kb[0] : kr[(s_ > 0) ? s_ - 1 : 0], kr[s_]);
      } else {
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) kap[s_] = (SRC == VI_KAPPA) ? kr[s_] : one;
      }
      if (MET) {
        if (mf.p && mf.sz != 0) load_rows<T, SEG>(mfr, mf.p, mfo + (k + 1) * mf.sz, mf.sy, mf.sx, nrow, (ntl & 8) != 0);
      }
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        T g = kap[s_];
        if (MET) {
          if (mf.p) g = g / mfr[s_];
        }
        w[s_] = tdt * g;
        T u = w[s_];
        if (MET) {
          if (mc.p) u = u / mcr[s_];
        }
        up_[s_] = u;
        b_[s_] = b_[s_] + u;
      }
    }
  };

  // ---- forward: d into out, c into cw; the last level's d is x itself ----
  T ac[SEG], lo[SEG], up[SEG], b[SEG], cp[SEG], dp[SEG];
  coef(0, ac, lo, up, b);
  for (int64_t k = 0; k < nz; ++k) {
    const bool more = k + 1 < nz;
    T an[SEG], lon[SEG], upn[SEG], bn[SEG];
    if (more) coef(k + 1, an, lon, upn, bn);
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      T m = b[s_], d = ac[s_];
      if (k > 0) {
        m = m - lo[s_] * cp[s_];
        d = d + lo[s_] * dp[s_];
      }
      const T r = one / m;
      d = d * r;
      dp[s_] = d;
      if (more) {
        cp[s_] = up[s_] * r;
        if (s_ < nrow) {
          stg<T, false>(out + ro[s_] + k * plane, d);
          stg<T, false>(cw + ro[s_] + k * plane, cp[s_]);
        }
      } else if (s_ < nrow) {
        stg_s<T, NTS>(out + ro[s_] + k * plane, d);
      }
    }
    if (more) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        ac[s_] = an[s_];
        lo[s_] = lon[s_];
        up[s_] = upn[s_];
        b[s_] = bn[s_];
      }
    }
  }
  if (nz < 2) return;

  // ---- backward: x[k] = d[k] + c[k] * x[k+1], what this lane stored read back one level ahead of its use ----
  T dk[SEG], ck[SEG];
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) {
    dk[s_] = *reinterpret_cast<const T*>(out + ro[s_] + (nz - 2) * plane);
    ck[s_] = *reinterpret_cast<const T*>(cw + ro[s_] + (nz - 2) * plane);
  }
  for (int64_t k = nz - 2; k >= 0; --k) {
    T dn[SEG], cn[SEG];
    if (k > 0) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        dn[s_] = *reinterpret_cast<const T*>(out + ro[s_] + (k - 1) * plane);
        cn[s_] = *reinterpret_cast<const T*>(cw + ro[s_] + (k - 1) * plane);
      }
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      dp[s_] = dk[s_] + ck[s_] * dp[s_];
      if (s_ < nrow) stg_s<T, NTS>(out + ro[s_] + k * plane, dp[s_]);
    }
    if (k > 0) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        dk[s_] = dn[s_];
        ck[s_] = cn[s_];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7n / K7p, the Richardson family: the squared vertical shear, the gradient Richardson number or the Pacanowski-Philander
// (1981) mixing coefficients at the flux faces of Z in ONE pass over (lead, Z, Y, X), two or three fields in, one or two
// out (nz faces at Z:left, nz + 1 at Z:outer).  ONE kernel; MODE chooses the epilogue of a face, at compile time:
//   du[k] = (u[k] - u[k-1]) [/ mu[k]]    at u's points,     dv[k] = (v[k] - v[k-1]) [/ mv[k]]    at v's points
//   S2[k] = uz * uz + vz * vz,   uz = (du[j,i] + du[j,i+1]) * 0.5,   vz = (dv[j,i] + dv[j+1,i]) * 0.5      (no FMA)
//   N2[k] = (b[k] - b[k-1]) [/ mb[k]]                                          (RI_S2: S2 is the result, b is not read)
//   Ri[k] = N2[k] / S2[k]                                                                         (RI_RI: the result)
//   ri = N2 / (S2 + shear_floor)      rp = (ri + |ri|) * 0.5      den = 1 + alpha * rp                      (RI_MIX)
//   nu = nu0 / (den * den) + nu_b     kappa = nu / den + kappa_b                      (no FMA, IEEE quotients; K7p)
// i.e. diff | derivative (Z, center -> left | outer) of u, v and b, interp (X / Y, left -> center) of the first two, the
// squares, their sum, the quotient: MITgcm's form, the shear averaged to the centre first and squared then; the closure one
// operation per line of the chain and two stores.  rp is max(ri, 0) for every finite ri (+0.0 for -0.0); a NaN stays one,
// -inf gives NaN.  The second result and the closure's five scalars (in `real`) are arguments of every instance and are
// read by RI_MIX alone; `bb`, the rows of mb and their offset are never formed under RI_S2.  Pads as the
// chain's: u, v and b above level 0 and (`outer`) below level nz-1 (periodic: the far level, extend: the level itself,
// fill: fill_z), then the DERIVATIVES right of the last column / above the last row (periodic: the derivative at index 0,
// extend: at n-1, fill: the fill value itself).  No guard on S2 == 0: the quotient is IEEE's.
// K7j's march with K7g's neighbours: a wave owns one (lead, Y segment, X tile) column and marches the faces with the rows
// of the level above in registers -- SEG rows of u with the element right of the lane's vector where the lane forms that
// derivative itself (the tile's last lane, the row's edge; every other lane takes the finished derivative from the lane
// above by DPP), SEG + 1 rows of v (the row above the segment: an L2 hit, the next segment's first row), SEG rows of b.
// u, v and b are read once and each result written once: 32 B/cell in float64 (S2: 24, K7p: 40).  The three metrics (the
// Z metric at u's points, at v's points, at the centre, all at the faces) are one broadcast array each, each may be absent; rows that
// do not vary along Z are loaded once per wave.  Periodic Z costs one more level read before the march (and, `outer`, one
// after it).
// ------------------------------------------------------------------------------------------
enum { RI_S2 = 0, RI_RI = 1, RI_MIX = 2 };  // k_richardson's MODE: out = S2 | out = Ri | out = nu and out2 = kappa

template <typename T, int SEG>
struct RiLevel {  // what one level of a column brings: SEG rows of u and b, SEG + 1 rows of v, u right of the lane
  T uu[SEG], vv[SEG + 1], bb[SEG];
  real ur[SEG];
};
struct RimixScalars {
  real nu0, alpha, nu_b, kappa_b, floor;
};

template <int V, int MODE, bool MET, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_richardson(
    const real* __restrict__ b, const real* __restrict__ u, const real* __restrict__ v, real* __restrict__ out,
    real* __restrict__ out2, int64_t o0, u32 nouter, u32 nblk, int64_t nz, int64_t ny, int64_t nx, FastDiv ntile,
    FastDiv nseg, int outer, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z, real fill_z, VolIdx mu, VolIdx mv,
    VolIdx mb, int ntl, RimixScalars c) {
  typedef typename VecT<V>::type T;
  typedef RiLevel<T, SEG> L;
  constexpr bool RI = MODE != RI_S2;  // b and its metric are read
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const int64_t plane = ny * nx;
  const int64_t col = o * nz * plane;  // level 0 of this lead index (int64: a 4320^2 x 90 field has more than 2^32 cells)
  const int64_t nf = nz + outer;       // faces
  // X as K7g's u: the column right of the lane's vector (periodic: column 0, extend: column nx - 1 itself); Y as K7g's v:
  // the row above the segment (periodic: row 0 above row ny - 1, extend: row ny - 1 itself); a fill edge replaces the value
  const LaneEdges e = lane_edges<V>(i0, nx, bc_x, ntl);  // (the right side only)
  const bool fill_r = e.edge_r && bc_x == XG_BC_FILL;
  const int64_t q = j0 + nrow;
  const bool fill_t = q >= ny && bc_y == XG_BC_FILL;
  const int64_t jt = (q < ny) ? q : ((bc_y == XG_BC_PERIODIC) ? 0 : ny - 1);  // the row the top derivative is formed at
  int64_t ro[SEG];  // the segment's rows in a plane (short tails repeat the last row)
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) ro[s_] = (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * nx;

  auto fetch = [&](int64_t k) -> L {
    L x;
    const int64_t lv = col + k * plane;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      x.uu[s_] = *reinterpret_cast<const T*>(u + lv + ro[s_] + i0);
      x.ur[s_] = e.own_r ? u[lv + ro[s_] + e.ridx] : real(0);
      x.vv[s_] = *reinterpret_cast<const T*>(v + lv + ro[s_] + i0);
      if (RI) x.bb[s_] = *reinterpret_cast<const T*>(b + lv + ro[s_] + i0);
    }
    x.vv[SEG] = *reinterpret_cast<const T*>(v + lv + jt * nx + i0);
    return x;
  };
  auto padded = [&]() -> L {  // a level of the fill value
    L x;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      x.uu[s_] = x.vv[s_] = splat<T>(fill_z);
      if (RI) x.bb[s_] = splat<T>(fill_z);
      x.ur[s_] = fill_z;
    }
    x.vv[SEG] = splat<T>(fill_z);
    return x;
  };

  // the metric rows of a face: in registers, loaded again per face only when the array varies along Z; the metric of u also
  // at the column right of the lane's vector, for the lanes that form that derivative themselves
  T mur[SEG], mvr[SEG + 1], mbr[SEG];
  real mrr[SEG];
  int64_t muo = 0, mro = 0, mvo = 0, mto = 0, mbo = 0;
  auto metrics = [&](int64_t k, bool first) {
    if (mu.p && (first || mu.sz != 0)) {
      load_rows<T, SEG>(mur, mu.p, muo + k * mu.sz, mu.sy, mu.sx, nrow, (ntl & 4) != 0);
      if (e.own_r) {
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) mrr[s_] = mu.p[mro + k * mu.sz + ((s_ < nrow) ? s_ : nrow - 1) * mu.sy];
      }
    }
    if (mv.p && (first || mv.sz != 0)) {
      T rows[SEG];
      load_rows<T, SEG>(rows, mv.p, mvo + k * mv.sz, mv.sy, mv.sx, nrow, (ntl & 8) != 0);
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) mvr[s_] = rows[s_];
      T top[1];
      load_rows<T, 1>(top, mv.p, mto + k * mv.sz, mv.sy, mv.sx, 1, (ntl & 8) != 0);
      mvr[SEG] = top[0];
    }
    if (RI) {
      if (mb.p && (first || mb.sz != 0)) load_rows<T, SEG>(mbr, mb.p, mbo + k * mb.sz, mb.sy, mb.sx, nrow, (ntl & 16) != 0);
    }
  };
  if (MET) {
    const int64_t uo = mu.p ? area_outer_off(mu.ai, o) : 0, vo = mv.p ? area_outer_off(mv.ai, o) : 0;
    muo = uo + j0 * mu.sy + i0 * mu.sx;
    mro = uo + j0 * mu.sy + e.ridx * mu.sx;
    mvo = vo + j0 * mv.sy + i0 * mv.sx;
    mto = vo + jt * mv.sy + i0 * mv.sx;
    if (RI) {
      if (mb.p) mbo = area_outer_off(mb.ai, o) + j0 * mb.sy + i0 * mb.sx;
    }
    metrics(0, true);
  }

  // one face from the level above it (`lo`) and the level below it (`hi`)
  const int64_t po = o * nf * plane + j0 * nx + i0;
  const T one = splat<T>(real(1)), half = splat<T>(real(0.5));
  auto face = [&](int64_t k, const L& lo, const L& hi) {
    T du[SEG], dv[SEG + 1];
    real dr[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      du[s_] = op2<XG_OP_DIFF>(lo.uu[s_], hi.uu[s_]);
      dr[s_] = hi.ur[s_] - lo.ur[s_];
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG + 1; ++s_) dv[s_] = op2<XG_OP_DIFF>(lo.vv[s_], hi.vv[s_]);
    if (MET) {
      if (mu.p) {
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) du[s_] = du[s_] / mur[s_];
        if (e.own_r) {
#pragma unroll
          for (int s_ = 0; s_ < SEG; ++s_) dr[s_] = dr[s_] / mrr[s_];
        }
      }
      if (mv.p) {
#pragma unroll
        for (int s_ = 0; s_ < SEG + 1; ++s_) dv[s_] = dv[s_] / mvr[s_];
      }
    }
    if (e.shl) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const real right = from_lane_above(vec_first(du[s_]));  // DPP wave_shl:1 (lane 63 reads 0 and is `own_r`)
        if (!e.own_r) dr[s_] = right;
      }
    }
    const T top = fill_t ? splat<T>(fill_y) : dv[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        const T uz = interp_right_of(du[s_], fill_r ? fill_x : dr[s_]);
        const T vz = op2<XG_OP_INTERP>(dv[s_], (s_ + 1 < nrow) ? dv[s_ + 1] : top);
        const T s2 = uz * uz + vz * vz;
        T db;
        if (RI) {
          db = op2<XG_OP_DIFF>(lo.bb[s_], hi.bb[s_]);
          if (MET) {
            if (mb.p) db = db / mbr[s_];
          }
        }
        const int64_t at = po + k * plane + s_ * nx;
        if (MODE == RI_MIX) {  // the closure, one operation per line of the chain
          const T ri = db / (s2 + splat<T>(c.floor));
          const T rp = (ri + __builtin_elementwise_abs(ri)) * half;
          const T den = one + splat<T>(c.alpha) * rp;
          const T nu = splat<T>(c.nu0) / (den * den) + splat<T>(c.nu_b);
          const T ka = nu / den + splat<T>(c.kappa_b);
          stg_s<T, NTS>(out + at, nu);
          stg_s<T, NTS>(out2 + at, ka);
        } else if (MODE == RI_RI) {
          stg_s<T, NTS>(out + at, db / s2);
        } else {
          stg_s<T, NTS>(out + at, s2);
        }
      }
    }
  };

  // face 0 lies between the pad above level 0 and level 0; the march keeps the level above the face
  L cur = fetch(0), prev;
  if (bc_z == XG_BC_PERIODIC) prev = fetch(nz - 1);
  else if (bc_z == XG_BC_EXTEND) prev = cur;
  else prev = padded();
  for (int64_t k = 0;;) {
    face(k, prev, cur);
    if (++k >= nf) break;
    prev = cur;
    if (k < nz) cur = fetch(k);                           // (`outer`, the last face: the pad below level nz-1 --
    else if (bc_z == XG_BC_PERIODIC) cur = fetch(0);      //  extend: the level itself, which `cur` still holds)
    else if (bc_z == XG_BC_FILL) cur = padded();
    if (MET) metrics(k, false);
  }
}

// ------------------------------------------------------------------------------------------
// K7q / K7r / K7s, the isopycnal family: ONE kernel, one pass over (lead, Z, Y, X), around one column stage.  Per level of
// the field b
//   g[i] = (b[i] - b[i-1]) [/ mx[i]]      G_x[i] = (g[i] + g[i+1]) * 0.5        and the same along Y with my: G_y
// per face (nz of them at Z:left, nz + 1 at Z:outer)
//   gx = (G_x[k-1] + G_x[k]) * 0.5    gy = (G_y[k-1] + G_y[k]) * 0.5
// i.e. diff | derivative (X / Y, center -> left), interp back (left -> center), interp (Z, center -> left | outer).  Pads as
// the chain's: b left of column 0 / below row 0, then the DERIVATIVE right of the last column / above the last row (periodic:
// the derivative at index 0, extend: at n-1, fill: the fill value itself), then the LEVEL MEANS G above level 0 and (`outer`)
// below level nz-1 (periodic: the far level's, extend: the level's own, fill: fill_z itself).  MODE chooses, at compile
// time, what a face does with gx and gy:
// IS_SLOPE (K7q), the isopycnal slopes, one field in, two out at the faces:
//   bz = (b[k] - b[k-1]) [/ mz[k]]    sx = -1 * (gx / bz)    sy = -1 * (gy / bz)           (no FMA, IEEE quotients)
// diff | derivative (Z) of b, b along Z padded as K7n's; the two quotients, negated.  No guard on bz == 0.  24 B/cell in
// float64.
// IS_TENSOR (K7r), the tapered Redi / Gent-McWilliams tensor column, three out at the faces: sx and sy, then
//   s2 = sx * sx + sy * sy
//   ex = s2 - m2      den = m2 + (ex + |ex|) * 0.5      kt = kappa * (m2 / den)       (`taper`; else kt = kappa)
//   Kwx = kt * sx     Kwy = kt * sy     Kwz = kt * s2                                   (no FMA, IEEE quotients)
// as the epilogue of every face, and three stores.  den is max(s2, m2) (Gerdes, Koeberle and Willebrand 1991: the taper is
// min(1, m2 / s2), no square root): where s2 <= m2, ex + |ex| is +0.0, den is m2 and the taper exactly 1; an infinite slope
// gives taper 0 and 0 * inf = NaN; a NaN stays one.  32 B/cell in float64.  kappa and m2 arrive in `real`; `taper` is
// wave-uniform.
// IS_FLUX (K7s), the divergence of the off-diagonal vertical isoneutral flux of a tracer, d/dz(Kwx <da/dx> + Kwy <da/dy>):
// the tracer (as `b`) and the two tensor components of K7r in (kwx and kwy, at the faces), one field out at the levels:
//   f[k] = kwx[k] * gx + kwy[k] * gy                        out[k] = (f[k+1] - f[k]) [/ mc[k]]                (no FMA)
// K7l's flux march with f[k] in registers; the level carries no b, and the third metric is mc at the LEVELS, held by K7l's
// rule.  `closed` (wave-uniform): no flux through the top and the bottom -- face 0 and, `outer`, face nz are +0.0; their kwx
// and kwy rows are not loaded and no pad level is formed for them, so nothing there reaches the result.  Otherwise the level
// means are padded as above.  `left`: the FLUX beyond level nz-1 is padded as K7l's (periodic: f[0] -- closed: that +0.0 --,
// extend: f[nz-1], fill: fill_z itself).  32 B/cell in float64.
// K7n's wave-task and march: a wave owns one (lead, Y segment, X tile) column and keeps the level above the face in
// registers -- not its rows but what the faces need of it, G_x, G_y and (but IS_FLUX) b of the segment.  A level brings
// SEG + 2 rows of b (the row below and the row above the segment: L2 hits, the neighbouring segments' rows) and, for the
// segment's rows, the element left of and right of the lane's vector: b left of it from the lane below by DPP, the finished
// derivative right of it from the lane above by DPP; the tile's first / last lane and the row's edges load their own.  WHEN
// the rows of the level below the next face are asked for differs by MODE, for the registers: see the marches.  Every field
// is read once and each result written once.  mx at b's levels and u's columns, my at b's levels and v's rows, mz at the
// faces (IS_FLUX: mc at the levels): one broadcast array each, each may be absent; rows that do not vary along Z are loaded
// once per wave, mx also at the column right of the lane, my also at the row above the segment.  Periodic Z costs one more
// level before the march (and, `outer`, one after it).  The arguments are the union of the three: kwx, kwy and `closed` are
// read by IS_FLUX alone, out_y not by it, out_z and `c` by IS_TENSOR alone.
// ------------------------------------------------------------------------------------------
enum { IS_SLOPE = 0, IS_TENSOR = 1, IS_FLUX = 2 };  // k_islope's MODE

template <typename T, int SEG>
struct IsRows {  // what one level of a column brings: the row below, SEG rows with b left and right of the lane, the row above
  T bb[SEG], below, above;
  real bl[SEG], br[SEG];
};
template <typename T, int SEG>
struct IsLevel {  // what a face needs of a level (IS_FLUX: `bb` is never formed)
  T gx[SEG], gy[SEG], bb[SEG];
};
struct RediScalars {
  real kappa, m2;
  int taper;
};

template <int V, int MODE, bool MET, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_islope(
    const real* __restrict__ b, const real* __restrict__ kwx, const real* __restrict__ kwy, real* __restrict__ out_x,
    real* __restrict__ out_y, real* __restrict__ out_z, int64_t o0, u32 nouter, u32 nblk, int64_t nz, int64_t ny, int64_t nx,
    FastDiv ntile, FastDiv nseg, int outer, int closed, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z, real fill_z,
    VolIdx mx, VolIdx my, VolIdx mz, int ntl, RediScalars c) {
  typedef typename VecT<V>::type T;
  typedef IsRows<T, SEG> Rows;
  typedef IsLevel<T, SEG> L;
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const int64_t plane = ny * nx;
  const int64_t col = o * nz * plane;  // level 0 of this lead index (int64: a 4320^2 x 90 field has more than 2^32 cells)
  const int64_t nf = nz + outer;       // faces
  // X: the columns left and right of the lane's vector, always inside the row (wrapped at a periodic edge, clamped at any
  // other: the clamped left column IS the extend pad of b); a fill edge replaces b on the left, a fill or extend edge the
  // derivative on the right
  const LaneEdges e = lane_edges<V>(i0, nx, bc_x, ntl);
  const bool per_x = bc_x == XG_BC_PERIODIC, per_z = bc_z == XG_BC_PERIODIC;
  const bool fill_l = e.edge_l && bc_x == XG_BC_FILL;
  const bool pad_r = e.edge_r && !per_x;
  // Y: the row below the segment (periodic: row ny - 1 below row 0, extend: row 0 itself) and the row above it, where the
  // top derivative is formed (periodic: row 0 above row ny - 1); wave-uniform
  const bool fill_b = j0 == 0 && bc_y == XG_BC_FILL;
  const int64_t jb = (j0 > 0) ? j0 - 1 : ((bc_y == XG_BC_PERIODIC) ? ny - 1 : 0);
  const int64_t q = j0 + nrow;
  const bool pad_t = q >= ny && bc_y != XG_BC_PERIODIC;
  const int64_t jt = (q < ny) ? q : ((bc_y == XG_BC_PERIODIC) ? 0 : ny - 1);
  int64_t ro[SEG];  // the segment's rows in a plane (short tails repeat the last row)
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) ro[s_] = (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * nx;

  // the rows of mx and my of a level: in registers, loaded again per level only when the array varies along Z; the rows of
  // the third metric likewise, of a face (IS_FLUX: of a level, as K7l holds them)
  T mxr[SEG], myr[SEG], myt, mzc[SEG];
  real mxrr[SEG];
  int64_t mxo = 0, mro = 0, myo = 0, mto = 0, mzo = 0;
  auto zmetric = [&](T (&dst)[SEG], int64_t k, bool first) {
    if (mz.p && (first || mz.sz != 0)) load_rows<T, SEG>(dst, mz.p, mzo + k * mz.sz, mz.sy, mz.sx, nrow, (ntl & 16) != 0);
  };
  auto hmetrics = [&](int64_t k, bool first) {
    if (mx.p && (first || mx.sz != 0)) {
      load_rows<T, SEG>(mxr, mx.p, mxo + k * mx.sz, mx.sy, mx.sx, nrow, (ntl & 4) != 0);
      if (e.own_r) {
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) mxrr[s_] = mx.p[mro + k * mx.sz + ((s_ < nrow) ? s_ : nrow - 1) * mx.sy];
      }
    }
    if (my.p && (first || my.sz != 0)) {
      load_rows<T, SEG>(myr, my.p, myo + k * my.sz, my.sy, my.sx, nrow, (ntl & 8) != 0);
      T top[1];
      load_rows<T, 1>(top, my.p, mto + k * my.sz, my.sy, my.sx, 1, (ntl & 8) != 0);
      myt = top[0];
    }
  };
  if (MET) {
    const int64_t xo = mx.p ? area_outer_off(mx.ai, o) : 0, yo = my.p ? area_outer_off(my.ai, o) : 0;
    mxo = xo + j0 * mx.sy + i0 * mx.sx;
    mro = xo + j0 * mx.sy + e.ridx * mx.sx;
    myo = yo + j0 * my.sy + i0 * my.sx;
    mto = yo + jt * my.sy + i0 * my.sx;
    if (mz.p) mzo = area_outer_off(mz.ai, o) + j0 * mz.sy + i0 * mz.sx;
    if (MODE == IS_FLUX) zmetric(mzc, 0, true);
    hmetrics(0, true);
  }

  auto fetch = [&](int64_t k) -> Rows {  // (with the level's own mx and my rows: `level` is the only reader of both)
    Rows x;
    const int64_t lv = col + k * plane;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      x.bb[s_] = *reinterpret_cast<const T*>(b + lv + ro[s_] + i0);
      x.bl[s_] = e.own_l ? b[lv + ro[s_] + e.lidx] : real(0);
      x.br[s_] = e.own_r ? b[lv + ro[s_] + e.ridx] : real(0);
    }
    x.below = *reinterpret_cast<const T*>(b + lv + jb * nx + i0);
    x.above = *reinterpret_cast<const T*>(b + lv + jt * nx + i0);
    if (MET) hmetrics(k, false);
    return x;
  };
  // G_x, G_y and b of the segment from the rows of a level
  auto level = [&](const Rows& x) -> L {
    L r;
    T g[SEG], h[SEG];
    real gr[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      real left = x.bl[s_];
      if (e.shl) {
        const real dpp = from_lane_below(vec_last(x.bb[s_]));  // DPP wave_shr:1 (lane 0 reads 0 and is `own_l`)
        if (!e.own_l) left = dpp;
      }
      if (fill_l) left = fill_x;
      g[s_] = dvdx_of(x.bb[s_], left);
      gr[s_] = x.br[s_] - vec_last(x.bb[s_]);
      const T lower = (s_ == 0) ? (fill_b ? splat<T>(fill_y) : x.below) : x.bb[(s_ > 0) ? s_ - 1 : 0];
      h[s_] = x.bb[s_] - lower;
    }
    T top = x.above - x.bb[SEG - 1];  // (short tails repeat the last row: bb[SEG - 1] is row nrow - 1)
    if (MET) {
      if (mx.p) {
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) g[s_] = g[s_] / mxr[s_];
        if (e.own_r) {
#pragma unroll
          for (int s_ = 0; s_ < SEG; ++s_) gr[s_] = gr[s_] / mxrr[s_];
        }
      }
      if (my.p) {
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) h[s_] = h[s_] / myr[s_];
        top = top / myt;
      }
    }
    if (e.shl) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const real right = from_lane_above(vec_first(g[s_]));  // DPP wave_shl:1 (lane 63 reads 0 and is `own_r`)
        if (!e.own_r) gr[s_] = right;
      }
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (pad_r) gr[s_] = (bc_x == XG_BC_FILL) ? fill_x : vec_last(g[s_]);
      r.gx[s_] = interp_right_of(g[s_], gr[s_]);
      T up = (s_ + 1 < nrow) ? h[(s_ + 1 < SEG) ? s_ + 1 : s_] : top;
      if (s_ + 1 >= nrow && pad_t) up = (bc_y == XG_BC_FILL) ? splat<T>(fill_y) : h[s_];
      r.gy[s_] = op2<XG_OP_INTERP>(h[s_], up);
      if (MODE != IS_FLUX) r.bb[s_] = x.bb[s_];
    }
    return r;
  };
  auto padded = [&]() -> L {  // a level of the fill value: the pad of the level means and of b
    L r;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      r.gx[s_] = r.gy[s_] = splat<T>(fill_z);
      if (MODE != IS_FLUX) r.bb[s_] = splat<T>(fill_z);
    }
    return r;
  };

  // IS_SLOPE, IS_TENSOR: one face from the level above it (`lo`) and the level below it (`hi`): the slopes, then (IS_TENSOR)
  // the tensor column, one operation per line of the chain
  const int64_t po = o * nf * plane + j0 * nx + i0;
  const T minus = splat<T>(real(-1)), half = splat<T>(real(0.5)), m2 = splat<T>(c.m2), kappa = splat<T>(c.kappa);
  const bool taper = c.taper != 0;
  auto face = [&](int64_t k, const L& lo, const L& hi, const T (&mzr)[SEG]) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        const T gx = op2<XG_OP_INTERP>(lo.gx[s_], hi.gx[s_]);
        const T gy = op2<XG_OP_INTERP>(lo.gy[s_], hi.gy[s_]);
        T bz = op2<XG_OP_DIFF>(lo.bb[s_], hi.bb[s_]);
        if (MET) {
          if (mz.p) bz = bz / mzr[s_];
        }
        const T sx = minus * (gx / bz);
        const T sy = minus * (gy / bz);
        const int64_t at = po + k * plane + s_ * nx;
        if (MODE == IS_TENSOR) {
          const T s2 = sx * sx + sy * sy;
          T kt = kappa;
          if (taper) {
            const T ex = s2 - m2;
            const T den = m2 + (ex + __builtin_elementwise_abs(ex)) * half;
            kt = kappa * (m2 / den);
          }
          stg_s<T, NTS>(out_x + at, kt * sx);
          stg_s<T, NTS>(out_y + at, kt * sy);
          stg_s<T, NTS>(out_z + at, kt * s2);
        } else {
          stg_s<T, NTS>(out_x + at, sx);
          stg_s<T, NTS>(out_y + at, sy);
        }
      }
    }
  };

  if (MODE != IS_FLUX) {
    // face 0 lies between the pad above level 0 and level 0; the march keeps the level above the face.  IS_SLOPE has the
    // rows of the level below the NEXT face on their way while a face's quotients run.  The next face's mz rows are asked
    // for after the face: a second set of them in flight beside the rows costs the float64 metric instance its third wave
    // per SIMD (175 VGPRs against 167; 11.7 against 10.4 ms on 4320 x 4320 x 90 -- EXPERIMENTS.md "K7q").
    // IS_TENSOR asks for the rows of the level below the next face AFTER the face, not before it: with a third product, a
    // third quotient and s2 alive through the epilogue, rows in flight beside it cost the float64 metric instance its third
    // wave per SIMD (171 VGPRs, 14.7 ms on 4320 x 4320 x 90); the rows ahead without the two edge elements keep it (162) at
    // 13.0 - 13.2 ms, nothing ahead (144) runs in 11.5 ms (EXPERIMENTS.md "K7r")
    L prev;
    if (per_z) prev = level(fetch(nz - 1));
    L cur = level(fetch(0));
    if (bc_z == XG_BC_EXTEND) prev = cur;
    else if (bc_z == XG_BC_FILL) prev = padded();
    if (MET) zmetric(mzc, 0, true);
    for (int64_t k = 0;;) {
      const int64_t kn = k + 1;
      const bool more = kn < nf, read = kn < nz || (more && per_z);  // (`outer`, the last face: the pad below level nz-1)
      Rows nxt;
      if (MODE == IS_SLOPE && read) nxt = fetch(kn < nz ? kn : 0);
      face(k, prev, cur, mzc);
      if (!more) break;
      if (MET) zmetric(mzc, kn, false);
      prev = cur;
      if (read) {                                      // (extend: the level itself, which `cur` still holds)
        if (MODE == IS_TENSOR) nxt = fetch(kn < nz ? kn : 0);
        cur = level(nxt);
      } else if (bc_z == XG_BC_FILL) cur = padded();
      k = kn;
    }
    return;
  }

  // IS_FLUX: a level's rows are asked for after the store of the level above, IS_TENSOR's order, at ONE place in the march,
  // and the two tensor rows of the face after the level's means are formed.  The flux at face k from the level above it
  // (`lo`) and the level below it (`hi`): the face's rows of kwx and kwy, 16-byte loads, once; two products, then the sum
  const int64_t fo = o * nf * plane + i0;
  auto flux = [&](int64_t k, const L& lo, const L& hi, T (&f)[SEG]) {
    T kx[SEG], ky[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      kx[s_] = *reinterpret_cast<const T*>(kwx + fo + k * plane + ro[s_]);
      ky[s_] = *reinterpret_cast<const T*>(kwy + fo + k * plane + ro[s_]);
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      const T gx = op2<XG_OP_INTERP>(lo.gx[s_], hi.gx[s_]);
      const T gy = op2<XG_OP_INTERP>(lo.gy[s_], hi.gy[s_]);
      const T px = kx[s_] * gx;
      const T py = ky[s_] * gy;
      f[s_] = px + py;
    }
  };

  // face 0: closed, or from the pad above level 0
  const bool shut = closed != 0;
  T fc[SEG];
  L prev;
  if (!shut && per_z) prev = level(fetch(nz - 1));
  L cur = level(fetch(0));
  if (shut) {
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) fc[s_] = splat<T>(real(0));
  } else {
    if (bc_z == XG_BC_EXTEND) prev = cur;
    else if (bc_z == XG_BC_FILL) prev = padded();
    flux(0, prev, cur, fc);
  }
  real* pc = out_x + col + j0 * nx + i0;
  for (int64_t k = 0; k < nz; ++k) {
    const bool more = k + 1 < nz;
    // the flux below level k is formed from two levels: an interior face; the open last face of `outer` (the pad below
    // level nz-1 -- extend: the level itself, which `cur` still holds); or, `left`, periodic and open, the pad beyond level
    // nz-1, which is f[0]: formed AGAIN from level nz-1 and level 0, one more level read per column in that mode, instead of
    // held through the march as K7l holds its f0 -- 8 VGPRs that the float64 metric instance does not have
    // (EXPERIMENTS.md "K7s")
    const bool form = more || (!shut && (outer || per_z));
    T fn[SEG];
    if (form) {
      prev = cur;
      if (more || per_z) cur = level(fetch(more ? k + 1 : 0));
      else if (bc_z == XG_BC_FILL) cur = padded();
      flux((more || outer) ? k + 1 : 0, prev, cur, fn);
    } else {
      // the closed bottom of `outer` and the closed f[0] of a periodic `left`: +0.0; else `left`'s pad of the flux
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_)
        fn[s_] = (outer || per_z) ? splat<T>(real(0)) : ((bc_z == XG_BC_EXTEND) ? fc[s_] : splat<T>(fill_z));
    }
    if (MET && k > 0) zmetric(mzc, k, false);  // (the rows of mc of level k)
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        T z = op2<XG_OP_DIFF>(fc[s_], fn[s_]);
        if (MET) {
          if (mz.p) z = z / mzc[s_];
        }
        stg_s<T, NTS>(pc + k * plane + s_ * nx, z);
      }
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) fc[s_] = fn[s_];
  }
}

// ------------------------------------------------------------------------------------------
// K7t: the Gent-McWilliams eddy-induced (bolus) velocity from the two tensor components of K7r in ONE pass over
// (lead, Z, Y, X), two fields in at the faces of Z (nz of them at Z:left, nz + 1 at Z:outer), three out:
//   px[i] = (kwx[i-1] + kwx[i]) * 0.5      py[j] = (kwy[j-1] + kwy[j]) * 0.5       the streamfunction at u's / v's columns
//   closed: px = py = +0.0 at face 0 and, `outer`, at face nz -- their rows of kwx and kwy are never loaded
//   ub[k] = -1 * ((px[k+1] - px[k]) [/ mzu[k]])      vb[k] = -1 * ((py[k+1] - py[k]) [/ mzv[k]])         at the levels
//   tx = px [* dyg]    ty = py [* dxg]    wb = ((tx[i+1] - tx[i]) + (ty[j+1] - ty[j])) [/ ra]            at the faces
// i.e. interp (X / Y, center -> left), the closing copy, -diff | -derivative (Z, faces -> center), the two metric products
// and K7b's divergence; no FMA, IEEE quotients.  Pads as the chain's: kwx left of column 0 / kwy below row 0, the TRANSPORTS
// right of the last column / above the last row (periodic: the transport at index 0, extend: at n-1, fill: the fill value
// itself), and, at Z:left, the streamfunction beyond face nz-1 (periodic: face 0's -- closed: that +0.0 --, extend: face
// nz-1's, fill: fill_z itself).  A closed face of wb goes through the same products, differences and quotient with +0.0.
// K7q's wave-task: a wave owns one (lead, Y segment, X tile) column and marches the faces.  A face brings SEG rows of kwx
// with the element left of the lane's vector from the lane below by DPP (the tile's first lane and the row's edge load their
// own) and SEG + 2 rows of kwy (the row below and the row above the segment: L2 hits); the finished transport right of the
// vector comes from the lane above by DPP (the tile's last lane and a periodic edge form their own from the column right of
// it), the transport of the row above is formed from the extra row.  px and py of the face above stay in registers for the
// level between the two faces; at Z:left, periodic and open, face 0's are formed AGAIN after the march, as K7s forms its f[0]
// (one more face read per column in that mode): held through the march they cost the float64 metric instance 16 VGPRs and
// with them its second wave per SIMD (EXPERIMENTS.md "K7t").  Otherwise every input cell is read once; every result cell
// is written once.  Five broadcast metrics, each may be absent: mzu and
// mzv at the levels, dyg, dxg and ra at the faces; rows that do not vary along Z are loaded once per wave, dyg also at the
// column right of the lane, dxg also at the row above the segment.
// ------------------------------------------------------------------------------------------
template <typename T, int SEG>
struct BolusPsi {  // the streamfunction of the segment at one face
  T x[SEG], y[SEG];
};

template <int V, bool MET, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_bolus(
    const real* __restrict__ kwx, const real* __restrict__ kwy, real* __restrict__ out_u, real* __restrict__ out_v,
    real* __restrict__ out_w, int64_t o0, u32 nouter, u32 nblk, int64_t nz, int64_t ny, int64_t nx, FastDiv ntile,
    FastDiv nseg, int outer, int closed, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z, real fill_z, VolIdx mzu,
    VolIdx mzv, VolIdx dyg, VolIdx dxg, VolIdx ra, int ntl) {
  typedef typename VecT<V>::type T;
  typedef BolusPsi<T, SEG> Psi;
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const int64_t plane = ny * nx;
  const int64_t nf = nz + outer;                                    // faces
  const int64_t fcol = o * nf * plane, lcol = o * nz * plane;       // face 0 / level 0 of this lead index (int64)
  // X: the columns left and right of the lane's vector, always inside the row (the clamped left column IS the extend pad of
  // kwx); a fill edge replaces kwx on the left, a fill or extend edge the transport on the right
  const LaneEdges e = lane_edges<V>(i0, nx, bc_x, ntl);
  const bool per_x = bc_x == XG_BC_PERIODIC, per_z = bc_z == XG_BC_PERIODIC;
  const bool fill_l = e.edge_l && bc_x == XG_BC_FILL;
  const bool pad_r = e.edge_r && !per_x;
  // Y: the row below the segment and the row above it, where the top transport is formed; wave-uniform
  const bool fill_b = j0 == 0 && bc_y == XG_BC_FILL;
  const int64_t jb = (j0 > 0) ? j0 - 1 : ((bc_y == XG_BC_PERIODIC) ? ny - 1 : 0);
  const int64_t q = j0 + nrow;
  const bool pad_t = q >= ny && bc_y != XG_BC_PERIODIC;
  const int64_t jt = (q < ny) ? q : ((bc_y == XG_BC_PERIODIC) ? 0 : ny - 1);
  int64_t ro[SEG];  // the segment's rows in a plane (short tails repeat the last row)
#pragma unroll
  for (int s_ = 0; s_ < SEG; ++s_) ro[s_] = (j0 + ((s_ < nrow) ? s_ : nrow - 1)) * nx;

  // the metric rows of a face (dyg with the column right of the lane, dxg with the row above the segment, ra) and of a level
  // (mzu, mzv): in registers, loaded again only when the array varies along Z
  T dyr[SEG], dxr[SEG], dxt, rar[SEG], mur[SEG], mvr[SEG];
  real dyrr[SEG];
  int64_t dyo = 0, dro = 0, dxo = 0, dto = 0, rao = 0, muo = 0, mvo = 0;
  auto fmetrics = [&](int64_t k, bool first) {
    if (dyg.p && (first || dyg.sz != 0)) {
      load_rows<T, SEG>(dyr, dyg.p, dyo + k * dyg.sz, dyg.sy, dyg.sx, nrow, (ntl & 4) != 0);
      if (e.own_r) {
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) dyrr[s_] = dyg.p[dro + k * dyg.sz + ((s_ < nrow) ? s_ : nrow - 1) * dyg.sy];
      }
    }
    if (dxg.p && (first || dxg.sz != 0)) {
      load_rows<T, SEG>(dxr, dxg.p, dxo + k * dxg.sz, dxg.sy, dxg.sx, nrow, (ntl & 8) != 0);
      T top[1];
      load_rows<T, 1>(top, dxg.p, dto + k * dxg.sz, dxg.sy, dxg.sx, 1, (ntl & 8) != 0);
      dxt = top[0];
    }
    if (ra.p && (first || ra.sz != 0)) load_rows<T, SEG>(rar, ra.p, rao + k * ra.sz, ra.sy, ra.sx, nrow, (ntl & 16) != 0);
  };
  auto lmetrics = [&](int64_t k, bool first) {
    if (mzu.p && (first || mzu.sz != 0)) load_rows<T, SEG>(mur, mzu.p, muo + k * mzu.sz, mzu.sy, mzu.sx, nrow, (ntl & 32) != 0);
    if (mzv.p && (first || mzv.sz != 0)) load_rows<T, SEG>(mvr, mzv.p, mvo + k * mzv.sz, mzv.sy, mzv.sx, nrow, (ntl & 64) != 0);
  };
  if (MET) {
    const int64_t yo = dyg.p ? area_outer_off(dyg.ai, o) : 0, xo = dxg.p ? area_outer_off(dxg.ai, o) : 0;
    dyo = yo + j0 * dyg.sy + i0 * dyg.sx;
    dro = yo + j0 * dyg.sy + e.ridx * dyg.sx;
    dxo = xo + j0 * dxg.sy + i0 * dxg.sx;
    dto = xo + jt * dxg.sy + i0 * dxg.sx;
    if (ra.p) rao = area_outer_off(ra.ai, o) + j0 * ra.sy + i0 * ra.sx;
    if (mzu.p) muo = area_outer_off(mzu.ai, o) + j0 * mzu.sy + i0 * mzu.sx;
    if (mzv.p) mvo = area_outer_off(mzv.ai, o) + j0 * mzv.sy + i0 * mzv.sx;
    fmetrics(0, true);
    lmetrics(0, true);
  }

  // one face: its rows (none where it is `shut`), the streamfunction into `ps`, and -- `store` -- the transports and wb
  auto face = [&](int64_t k, bool shut, Psi& ps, bool store) {
    const int64_t fl = fcol + k * plane;
    T pyt;          // py of the row above the segment
    real pxr[SEG];  // px of the column right of the lane's vector
    if (shut) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        ps.x[s_] = ps.y[s_] = splat<T>(real(0));
        pxr[s_] = real(0);
      }
      pyt = splat<T>(real(0));
    } else {
      T kx[SEG], ky[SEG];
      real kl[SEG], kr[SEG];
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        kx[s_] = *reinterpret_cast<const T*>(kwx + fl + ro[s_] + i0);
        kl[s_] = e.own_l ? kwx[fl + ro[s_] + e.lidx] : real(0);
        kr[s_] = e.form_r ? kwx[fl + ro[s_] + e.ridx] : real(0);
        ky[s_] = *reinterpret_cast<const T*>(kwy + fl + ro[s_] + i0);
      }
      const T below = *reinterpret_cast<const T*>(kwy + fl + jb * nx + i0);
      const T above = *reinterpret_cast<const T*>(kwy + fl + jt * nx + i0);
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        real left = kl[s_];
        if (e.shl) {
          const real dpp = from_lane_below(vec_last(kx[s_]));  // DPP wave_shr:1 (lane 0 reads 0 and is `own_l`)
          if (!e.own_l) left = dpp;
        }
        if (fill_l) left = fill_x;
        ps.x[s_] = interp_left_of(kx[s_], left);
        pxr[s_] = (vec_last(kx[s_]) + kr[s_]) * real(0.5);  // (a periodic edge: kwx[nx-1] is the pad left of column 0)
        const T lower = (s_ == 0) ? (fill_b ? splat<T>(fill_y) : below) : ky[(s_ > 0) ? s_ - 1 : 0];
        ps.y[s_] = op2<XG_OP_INTERP>(lower, ky[s_]);
      }
      pyt = op2<XG_OP_INTERP>(ky[SEG - 1], above);  // (short tails repeat the last row: ky[SEG - 1] is row nrow - 1)
    }
    if (!store) return;
    if (MET && k > 0) fmetrics(k, false);
    T tx[SEG], ty[SEG], tyt = pyt;
    real txr[SEG];
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      tx[s_] = ps.x[s_];
      ty[s_] = ps.y[s_];
      txr[s_] = pxr[s_];
    }
    if (MET) {
      if (dyg.p) {
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) tx[s_] = ps.x[s_] * dyr[s_];
        if (e.own_r) {
#pragma unroll
          for (int s_ = 0; s_ < SEG; ++s_) txr[s_] = pxr[s_] * dyrr[s_];
        }
      }
      if (dxg.p) {
#pragma unroll
        for (int s_ = 0; s_ < SEG; ++s_) ty[s_] = ps.y[s_] * dxr[s_];
        tyt = pyt * dxt;
      }
    }
    if (e.shl) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) {
        const real right = from_lane_above(vec_first(tx[s_]));  // DPP wave_shl:1 (lane 63 reads 0 and is `own_r`)
        if (!e.own_r) txr[s_] = right;
      }
    }
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (pad_r) txr[s_] = (bc_x == XG_BC_FILL) ? fill_x : vec_last(tx[s_]);
      T up = (s_ + 1 < nrow) ? ty[(s_ + 1 < SEG) ? s_ + 1 : s_] : tyt;
      if (s_ + 1 >= nrow && pad_t) up = (bc_y == XG_BC_FILL) ? splat<T>(fill_y) : ty[s_];
      if (s_ < nrow) {
        T z = dudx_fwd(tx[s_], txr[s_]) + (up - ty[s_]);  // (K7b's add order)
        if (MET) {
          if (ra.p) z = z / rar[s_];
        }
        stg_s<T, NTS>(out_w + fl + ro[s_] + i0, z);
      }
    }
  };

  const bool shut = closed != 0;
  const T minus = splat<T>(real(-1));
  Psi prev, cur;
  face(0, shut, prev, true);
  for (int64_t k = 0; k < nz; ++k) {
    const int64_t kn = k + 1;
    if (kn < nf) {
      face(kn, shut && kn == nz, cur, true);  // (face nz exists at Z:outer alone: the closed bottom)
    } else if (per_z) {
      face(0, shut, cur, false);  // (Z:left: the pad beyond face nz-1 is face 0's, formed again -- open: its rows read again)
    } else if (bc_z == XG_BC_FILL) {
#pragma unroll
      for (int s_ = 0; s_ < SEG; ++s_) cur.x[s_] = cur.y[s_] = splat<T>(fill_z);
    } else {
      cur = prev;
    }
    if (MET && k > 0) lmetrics(k, false);
    const int64_t lv = lcol + k * plane + i0;
#pragma unroll
    for (int s_ = 0; s_ < SEG; ++s_) {
      if (s_ < nrow) {
        T du = op2<XG_OP_DIFF>(prev.x[s_], cur.x[s_]);
        T dv_ = op2<XG_OP_DIFF>(prev.y[s_], cur.y[s_]);
        if (MET) {
          if (mzu.p) du = du / mur[s_];
          if (mzv.p) dv_ = dv_ / mvr[s_];
        }
        stg_s<T, NTS>(out_u + lv + ro[s_], minus * du);
        stg_s<T, NTS>(out_v + lv + ro[s_], minus * dv_);
      }
    }
    prev = cur;
  }
}

// ------------------------------------------------------------------------------------------
// K7u: the tapered off-diagonal components of the Redi / Gent-McWilliams tensor at u's and v's points in ONE pass over
// (lead, Z, Y, X), one field in, two out at the levels (include/xgcm_hip.h):
//   gx[i] = (b[i] - b[i-1]) [/ mx]    gy[j] = (b[j] - b[j-1]) [/ my]    f[k] = (b[k] - b[k-1]) [/ mz[k]]     bzc[k] = (f[k] + f[k+1]) * 0.5
//   bzu[i] = (bzc[i-1] + bzc[i]) * 0.5          bzv[j] = (bzc[j-1] + bzc[j]) * 0.5
//   gyu[i] = (gyc[i-1] + gyc[i]) * 0.5, gyc[j] = (gy[j] + gy[j+1]) * 0.5        gxv[j] = (gxc[j-1] + gxc[j]) * 0.5, gxc[i] = (gx[i] + gx[i+1]) * 0.5
//   u's points: sx = -1 * (gx / bzu), sy = -1 * (gyu / bzu)        v's points: sx = -1 * (gxv / bzv), sy = -1 * (gy / bzv)
//   K7r's epilogue at each point, kt = kappa * (m2 / (m2 + (ex + |ex|) * 0.5)), ex = sx * sx + sy * sy - m2;  out_u = kt * sx, out_v = kt * sy
// K7q's wave-task: a wave owns one (lead, Y segment, X tile) column and marches the levels one level ahead of its stores
// (bzc[k] needs the faces above and below level k, hence b of level k + 1); it carries the level's patch of b and the face
// derivative f[k].  A level brings SEG + 2 rows of b (the row below and the row above the segment) with the elements left
// and right of the lane's vector (from the lanes beside it by DPP; the tile's first / last lane and the row's edges load
// their own), as K7q's IsRows with the two outer rows' neighbours as well: the patch has rows 0 (below), 1 .. SEG (the
// segment), SEG + 1 (above) and columns 0 (left), 1 .. V (the lane's), V + 1 (right).  More of the halo than K7q: gx on the
// row below (for gxv) and right of the lane (for gxc), gy above the segment (for gyc) and left of the lane (for gyu), f and
// bzc left of the lane and on the row below -- each lane forms the derived values of its halo itself, from the patch.
// Where a chain stage pads a DERIVED quantity -- bzc and gyc left of column 0, bzc and gxc below row 0, gx right of the last
// column, gy above the last row, f beyond the last face of `left` -- the stage's pad is substituted (periodic: the far one,
// which the wrapped patch row / column gives; extend: its own; fill: the fill value itself), never formed from padded b.
// mx at rows 0 .. SEG, columns 1 .. V + 1; my at rows 1 .. SEG + 1, columns 0 .. V; mz (at the faces) at rows 0 .. SEG, columns
// 0 .. V: element loads through the broadcast strides, those that do not vary along Z once per wave.  24 B/cell in float64.
// ------------------------------------------------------------------------------------------
template <int R, int C>
struct UvPatch {  // b of one level around the lane: rows below, the segment's, above; columns left, the lane's, right
  real v[R][C];
};

template <int V, bool MET, bool NTS, int SEG>
__global__ __launch_bounds__(BLOCK) void k_rediuv(
    const real* __restrict__ b, real* __restrict__ out_u, real* __restrict__ out_v, int64_t o0, u32 nouter, u32 nblk,
    int64_t nz, int64_t ny, int64_t nx, FastDiv ntile, FastDiv nseg, int outer, int bc_x, real fill_x, int bc_y, real fill_y,
    int bc_z, real fill_z, VolIdx mx, VolIdx my, VolIdx mz, int ntl, RediScalars c) {
  typedef typename VecT<V>::type T;
  constexpr int R = SEG + 2, C = V + 2;
  typedef UvPatch<R, C> P;
  XG_WAVE_TASK(V, SEG, false, ZBand{}, 1);
  const int64_t plane = ny * nx;
  const int64_t col = o * nz * plane;  // level 0 of this lead index (int64)
  const LaneEdges e = lane_edges<V>(i0, nx, bc_x, ntl);
  const bool per_x = bc_x == XG_BC_PERIODIC, per_y = bc_y == XG_BC_PERIODIC, per_z = bc_z == XG_BC_PERIODIC;
  const bool fill_l = e.edge_l && bc_x == XG_BC_FILL;  // b, bzc and gyc left of column 0 are the fill value
  const bool pad_r = e.edge_r && !per_x;               // gx right of the last column is its pad
  const bool fill_b = j0 == 0 && bc_y == XG_BC_FILL;   // b, bzc and gxc below row 0 are the fill value
  const int64_t jb = (j0 > 0) ? j0 - 1 : (per_y ? ny - 1 : 0);
  const int64_t q = j0 + nrow;
  const bool pad_t = q >= ny && !per_y;                // gy above the last row is its pad
  const int64_t jt = (q < ny) ? q : (per_y ? 0 : ny - 1);
  int64_t rj[R];  // the patch's rows in a plane (short tails repeat the last row of the segment)
  rj[0] = jb;
#pragma unroll
  for (int r = 1; r <= SEG; ++r) rj[r] = j0 + ((r <= nrow) ? r - 1 : nrow - 1);
  rj[R - 1] = jt;
  int64_t ci[C];  // ... and its columns in a row
  ci[0] = e.lidx;
#pragma unroll
  for (int k = 1; k <= V; ++k) ci[k] = i0 + k - 1;
  ci[C - 1] = e.ridx;

  // the metrics of a level (mx, my) and of a face (mz), element by element through the broadcast strides; loaded again per
  // level / face only when the array varies along Z
  real mxv[SEG + 1][V + 1], myv[SEG + 1][V + 1], mzv[SEG + 1][V + 1];
  int64_t mxo = 0, myo = 0, mzo = 0;
  auto hmetrics = [&](int64_t k, bool first) {
    if (mx.p && (first || mx.sz != 0)) {
#pragma unroll
      for (int r = 0; r <= SEG; ++r)
#pragma unroll
        for (int k_ = 1; k_ <= V + 1; ++k_) mxv[r][k_ - 1] = mx.p[mxo + k * mx.sz + rj[r] * mx.sy + ci[k_] * mx.sx];
    }
    if (my.p && (first || my.sz != 0)) {
#pragma unroll
      for (int r = 1; r <= SEG + 1; ++r)
#pragma unroll
        for (int k_ = 0; k_ <= V; ++k_) myv[r - 1][k_] = my.p[myo + k * my.sz + rj[r] * my.sy + ci[k_] * my.sx];
    }
  };
  auto zmetric = [&](int64_t kf, bool first) {
    if (mz.p && (first || mz.sz != 0)) {
#pragma unroll
      for (int r = 0; r <= SEG; ++r)
#pragma unroll
        for (int k_ = 0; k_ <= V; ++k_) mzv[r][k_] = mz.p[mzo + kf * mz.sz + rj[r] * mz.sy + ci[k_] * mz.sx];
    }
  };
  if (MET) {
    if (mx.p) mxo = area_outer_off(mx.ai, o);
    if (my.p) myo = area_outer_off(my.ai, o);
    if (mz.p) mzo = area_outer_off(mz.ai, o);
    hmetrics(0, true);
  }

  auto fetch = [&](int64_t k) -> P {
    P x;
    const int64_t lv = col + k * plane;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = lv + rj[r] * nx;
      const T own = *reinterpret_cast<const T*>(b + row + i0);
      real left = e.own_l ? b[row + e.lidx] : real(0);
      real right = e.own_r ? b[row + e.ridx] : real(0);
      if (e.shl) {
        const real lo = from_lane_below(vec_last(own));   // DPP wave_shr:1 (lane 0 reads 0 and is `own_l`)
        const real hi = from_lane_above(vec_first(own));  // DPP wave_shl:1 (lane 63 reads 0 and is `own_r`)
        if (!e.own_l) left = lo;
        if (!e.own_r) right = hi;
      }
      x.v[r][0] = fill_l ? fill_x : left;
#pragma unroll
      for (int k_ = 0; k_ < V; ++k_) x.v[r][k_ + 1] = vec_at(own, k_);
      x.v[r][C - 1] = right;
    }
    if (fill_b) {
#pragma unroll
      for (int k_ = 0; k_ < C; ++k_) x.v[0][k_] = fill_y;
    }
    return x;
  };
  auto padded = [&]() -> P {  // a level of the fill value: the pad of b along Z
    P x;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k_ = 0; k_ < C; ++k_) x.v[r][k_] = fill_z;
    return x;
  };
  // the face derivative at face kf between the level above it (`lo`) and the level below it (`hi`): rows 0 .. SEG, columns 0 .. V
  auto zface = [&](const P& lo, const P& hi, int64_t kf, bool first, real (&f)[SEG + 1][V + 1]) {
    if (MET) zmetric(kf, first);
#pragma unroll
    for (int r = 0; r <= SEG; ++r)
#pragma unroll
      for (int k_ = 0; k_ <= V; ++k_) {
        real d = hi.v[r][k_] - lo.v[r][k_];
        if (MET) {
          if (mz.p) d = d / mzv[r][k_];
        }
        f[r][k_] = d;
      }
  };

  const real minus = real(-1), half = real(0.5);
  const bool taper = c.taper != 0;
  auto tensor = [&](real sx, real sy, real pick) -> real {  // K7r's epilogue, one operation per line of the chain
    const real s2 = sx * sx + sy * sy;
    real kt = c.kappa;
    if (taper) {
      const real ex = s2 - c.m2;
      const real den = c.m2 + (ex + __builtin_elementwise_abs(ex)) * half;
      kt = c.kappa * (c.m2 / den);
    }
    return kt * pick;
  };
  // level k from its patch and the face derivatives above (`fa`) and below (`fb`) it: both results, one 16-byte store each per row
  auto emit = [&](int64_t k, const P& x, const real (&fa)[SEG + 1][V + 1], const real (&fb)[SEG + 1][V + 1]) {
    if (MET) hmetrics(k, false);
    // gx on rows 0 .. SEG at columns 1 .. V + 1, its mean back to the centre at columns 1 .. V
    real gx[SEG + 1][V + 1], gxc[SEG + 1][V];
#pragma unroll
    for (int r = 0; r <= SEG; ++r) {
#pragma unroll
      for (int k_ = 1; k_ <= V + 1; ++k_) {
        real d = x.v[r][k_] - x.v[r][k_ - 1];
        if (MET) {
          if (mx.p) d = d / mxv[r][k_ - 1];
        }
        gx[r][k_ - 1] = d;
      }
      if (pad_r) gx[r][V] = (bc_x == XG_BC_FILL) ? fill_x : gx[r][V - 1];
#pragma unroll
      for (int k_ = 0; k_ < V; ++k_) gxc[r][k_] = (gx[r][k_] + gx[r][k_ + 1]) * half;
    }
    if (fill_b) {
#pragma unroll
      for (int k_ = 0; k_ < V; ++k_) gxc[0][k_] = fill_y;
    }
    // gy on rows 1 .. SEG + 1 at columns 0 .. V (row SEG + 1, above: against the segment's last row, which row SEG repeats)
    real gy[SEG + 1][V + 1], gyc[SEG][V + 1];
#pragma unroll
    for (int r = 1; r <= SEG + 1; ++r)
#pragma unroll
      for (int k_ = 0; k_ <= V; ++k_) {
        real d = x.v[r][k_] - x.v[r - 1][k_];
        if (MET) {
          if (my.p) d = d / myv[r - 1][k_];
        }
        gy[r - 1][k_] = d;
      }
#pragma unroll
    for (int r = 1; r <= SEG; ++r)
#pragma unroll
      for (int k_ = 0; k_ <= V; ++k_) {
        real up = (r < nrow) ? gy[(r < SEG) ? r : r - 1][k_] : gy[SEG][k_];
        if (r >= nrow && pad_t) up = (bc_y == XG_BC_FILL) ? fill_y : gy[r - 1][k_];
        real m = (gy[r - 1][k_] + up) * half;
        if (k_ == 0 && fill_l) m = fill_x;
        gyc[r - 1][k_] = m;
      }
    // db/dz back at the levels: rows 0 .. SEG, columns 0 .. V
    real bzc[SEG + 1][V + 1];
#pragma unroll
    for (int r = 0; r <= SEG; ++r)
#pragma unroll
      for (int k_ = 0; k_ <= V; ++k_) {
        real m = (fa[r][k_] + fb[r][k_]) * half;
        if (k_ == 0 && fill_l) m = fill_x;
        if (r == 0 && fill_b) m = fill_y;
        bzc[r][k_] = m;
      }
    const int64_t lv = col + k * plane + i0;
#pragma unroll
    for (int r = 1; r <= SEG; ++r) {
      if (r <= nrow) {
        T ku, kv;
#pragma unroll
        for (int k_ = 1; k_ <= V; ++k_) {
          const real bzu = (bzc[r][k_ - 1] + bzc[r][k_]) * half;
          const real bzv = (bzc[r - 1][k_] + bzc[r][k_]) * half;
          const real gyu = (gyc[r - 1][k_ - 1] + gyc[r - 1][k_]) * half;
          const real gxv = (gxc[r - 1][k_ - 1] + gxc[r][k_ - 1]) * half;
          const real sxu = minus * (gx[r][k_ - 1] / bzu);
          const real syu = minus * (gyu / bzu);
          const real sxv = minus * (gxv / bzv);
          const real syv = minus * (gy[r - 1][k_] / bzv);
          vec_set(ku, k_ - 1, tensor(sxu, syu, sxu));
          vec_set(kv, k_ - 1, tensor(sxv, syv, syv));
        }
        stg_s<T, NTS>(out_u + lv + rj[r] * nx, ku);
        stg_s<T, NTS>(out_v + lv + rj[r] * nx, kv);
      }
    }
  };

  // face 0 lies between the pad of b above level 0 and level 0; then level k is stored once the face below it is formed
  real fa[SEG + 1][V + 1], fb[SEG + 1][V + 1];
  P cur = fetch(0);
  {
    P prev;
    if (per_z) prev = fetch(nz - 1);
    else if (bc_z == XG_BC_FILL) prev = padded();
    else prev = cur;
    zface(prev, cur, 0, true, fa);
  }
  for (int64_t k = 0; k < nz; ++k) {
    const bool more = k + 1 < nz;
    P nxt = cur;  // (extend: the pad of b below level nz-1 is the level itself)
    if (more || outer || per_z) {
      // an interior face; `outer`: the last face, from the pad of b below level nz-1; `left` and periodic: the pad of the
      // derivative beyond the last face is f[0], formed again from level nz-1 and level 0 over mz[0]
      if (more || per_z) nxt = fetch(more ? k + 1 : 0);
      else if (bc_z == XG_BC_FILL) nxt = padded();
      zface(cur, nxt, (more || outer) ? k + 1 : 0, false, fb);
    } else {
      // `left`: the pad of the derivative beyond the last face -- extend: its own, fill: the fill value itself
#pragma unroll
      for (int r = 0; r <= SEG; ++r)
#pragma unroll
        for (int k_ = 0; k_ <= V; ++k_) fb[r][k_] = (bc_z == XG_BC_EXTEND) ? fa[r][k_] : fill_z;
    }
    emit(k, cur, fa, fb);
    cur = nxt;
#pragma unroll
    for (int r = 0; r <= SEG; ++r)
#pragma unroll
      for (int k_ = 0; k_ <= V; ++k_) fa[r][k_] = fb[r][k_];
  }
}

// ------------------------------------------------------------------------------------------
// host side of the fused kernels
// ------------------------------------------------------------------------------------------
// may every lane of a V-wide kernel load its piece of a metric / area plane as ONE aligned vector in every row and at
// every outer index?  (lanes start at multiples of NV along X)
bool plane_vec_ok(const real* m, const AreaIdx& ai, int64_t sy, int64_t sx) {
  if (!m || sx != 1 || sy % NV != 0 || !aligned16(m)) return false;
  for (int d = 0; d < ai.n; ++d)
    if (ai.stride[d] % NV != 0) return false;
  return true;
}

// a metric / area plane with broadcast strides: its (Y, X) strides + one stride per leading dim (0 = broadcast); adjacent
// leading dims are merged.  `core`: the trailing dims that are not leading dims (2: (Y, X); K7e's volume: 3, (Z, Y, X))
int area_index(const real* m, const int64_t* strides, const int64_t* shape, int ndim, AreaIdx* ai, int64_t* sy,
                      int64_t* sx, int core = 2) {
  memset(ai, 0, sizeof(*ai));
  for (int d = 0; d < XG_MAX_NDIM; ++d) ai->fd[d] = make_fastdiv(1);
  *sy = *sx = 0;
  if (!m) return 0;
  if (!strides) return fail(XG_ERR_INVALID, "metric without strides");
  *sy = strides[ndim - 2];
  *sx = strides[ndim - 1];
  for (int d = 0; d < ndim - core; ++d) {
    if (shape[d] == 1) continue;
    const int64_t st = strides[d];
    if (ai->n > 0 && ai->stride[ai->n - 1] == st * shape[d]) {  // merges with the previous (slower) dim
      ai->fd[ai->n - 1] = make_fastdiv((u64)ai->fd[ai->n - 1].d * (u64)shape[d]);
      ai->stride[ai->n - 1] = st;
      continue;
    }
    ai->fd[ai->n] = make_fastdiv((u64)shape[d]);
    ai->stride[ai->n] = st;
    ++ai->n;
  }
  return 0;
}

// one factor of a 3-D metric (K7e's volume, K7f's face weights and area): area_index + its stride along Z
int vol_index(VolIdx* vi, const real* m, const int64_t* strides, const int64_t* shape, int ndim) {
  memset(vi, 0, sizeof(*vi));
  vi->p = m;
  const int rc = area_index(m, strides, shape, ndim, &vi->ai, &vi->sy, &vi->sx, 3);
  if (rc) return rc;
  vi->sz = m ? strides[ndim - 3] : 0;
  return 0;
}

// absent, or broadcast along every leading dim: every outer index reads the same plane
bool planes_shared(const real* m, const AreaIdx& ai) {
  for (int d = 0; m && d < ai.n; ++d)
    if (ai.stride[d] != 0) return false;
  return true;
}

// the `ntl` bits that the `vec_nt` tunable governs (bit 0: the neighbours by lane shuffle; K7 also bit 1)
int vec_nt_bits(int mask) { return tune().nt_load ? (tune().vec_nt & mask) : 0; }
// rows of a band at its full height (the `vec_zb_rows` tunable; the launchers halve or double it, see there)
u32 band_rows() { return (u32)(tune().vec_zb_rows > 1 ? tune().vec_zb_rows : 16); }

// ------------------------------------------------------------------------------------------
// What the launchers of the fused kernels share: the view (outer, [Z,] Y, X) of the fields, the decomposition into
// wave-tasks (x-tiles of WAVE * V columns, segments of FSEG rows), the band-major order and the launches.
// ------------------------------------------------------------------------------------------
constexpr int FSEG = XG_FUSED_SEG;  // (K7d with 4 rows: the laplacian 12 % slower, the flux divergence 0.7 % faster -- EXPERIMENTS.md)

struct FusedPlan {
  const char* name;
  bool empty;                   // an extent is 0: nothing to do
  int64_t ny, nx, nz, outer;    // nz = 1 for the 2-D operators
  int V;
  u64 ntile, nseg, per_outer;   // x-tiles, Y segments, wave-tasks per outer index
  FastDiv fnt, fns;
  ZBand zb;                     // band-major order (fused_band), off by default
  u64 band_waves;               // wave-tasks of the one banded launch (tail bands padded)
  u64 outer_step;               // outer indices per launch
  bool nts;
  hipStream_t st;
};

// the argument checks every fused operator makes first: ndim, and each boundary mode in [periodic, bc_max].  The operator's
// own argument checks follow it and precede fused_plan, as they always did, so a bad call keeps its error code.
int fused_dims(const char* name, int ndim, int core, std::initializer_list<int> bcs, int bc_max) {
  if (ndim < core || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "%s: ndim %d not in [%d,%d]", name, ndim, core, XG_MAX_NDIM);
  for (int b : bcs)
    if (b < XG_BC_PERIODIC || b > bc_max) return fail(XG_ERR_INVALID, "%s: boundary mode %d not in [%d,%d]", name, b, XG_BC_PERIODIC, bc_max);
  return 0;
}

// extents (`core` = 2: (Y, X), 3: (Z, Y, X); the leading dims flattened into `outer`), the lane width -- `aligned`: every
// field pointer is 16-byte aligned -- and the task geometry.  `planes_by_outer`: a kernel argument is indexed by the 32-bit
// outer index.  An empty array is XG_OK with `empty` set.
int fused_plan(FusedPlan* p, const char* name, const int64_t* shape, int ndim, int core, bool aligned,
                      bool planes_by_outer, void* stream) {
  memset(p, 0, sizeof(*p));
  p->name = name;
  p->nz = (core == 3) ? shape[ndim - 3] : 1;
  p->ny = shape[ndim - 2];
  p->nx = shape[ndim - 1];
  p->outer = 1;
  for (int d = 0; d < ndim - core; ++d) p->outer *= shape[d];
  p->empty = p->outer == 0 || p->nz == 0 || p->ny == 0 || p->nx == 0;
  if (p->empty) return XG_OK;
  if (planes_by_outer && p->outer > 0xffffffffll)
    return fail(XG_ERR_UNSUPPORTED, "%s: more than 2^32 %s", name, core == 3 ? "(Z,Y,X) volumes" : "(Y,X) planes");
  p->V = (aligned && p->nx % NV == 0) ? NV : 1;
  p->ntile = (u64)((p->nx + (int64_t)WAVE * p->V - 1) / ((int64_t)WAVE * p->V));
  p->nseg = (u64)((p->ny + FSEG - 1) / FSEG);
  p->per_outer = p->ntile * p->nseg;
  p->fnt = make_fastdiv(p->ntile);
  p->fns = make_fastdiv(p->nseg);
  p->zb = make_zband(false, 0, 0, 1);
  p->outer_step = MAX_ITEMS / p->per_outer;  // (0 for an extent that fused_launch refuses)
  p->nts = tune().nt_store;
  p->st = (hipStream_t)stream;
  return XG_OK;
}

// band-major order when the planes are `shared` by every outer index (2-D metrics under a (Z, Y, X) field) -- level-major
// they come from the fabric again for every level (the gradient: 0.56 of 8 TB/s): bands of `rows` rows, all `zgroups` level
// groups (the outer indices; K7 / K7b: groups of ZK levels) of a band in ONE launch
void fused_band(FusedPlan* p, bool shared, u32 rows, u64 zgroups) {
  if (!shared || !tune().zband || p->outer < 2) return;
  const u32 segs = (rows + FSEG - 1) / FSEG;
  const u64 padded = ((p->nseg + segs - 1) / segs) * segs * zgroups * p->ntile;
  if (padded > MAX_ITEMS) return;
  p->zb = make_zband(true, zgroups, p->nseg, segs);
  if (!p->zb.on) return;
  p->band_waves = padded;
  p->outer_step = (u64)p->outer;  // one launch over all levels
}

// the launches: `go(o0, nouter, nblk, grid)` starts the kernel for outer indices o0 .. o0 + nouter - 1 with nblk blocks of
// work on a grid rounded up to the 8 XCD bands.  (More than one launch takes more than 2^31 wave-tasks.)
template <class Go>
int fused_launch(const FusedPlan& p, Go&& go) {
  if (p.per_outer > MAX_ITEMS) return fail(XG_ERR_UNSUPPORTED, "extent too large for the %s kernel", p.name);
  for (int64_t o0 = 0; o0 < p.outer; o0 += (int64_t)p.outer_step) {
    const u32 nouter = (u32)((p.outer - o0 < (int64_t)p.outer_step) ? p.outer - o0 : (int64_t)p.outer_step);
    const u64 waves = p.zb.on ? p.band_waves : (u64)nouter * p.per_outer;
    const u32 nblk = (u32)((waves + WPB - 1) / WPB);
    const int rc = check_grid((u64)nblk + 8);
    if (rc) return rc;
    go(o0, nouter, nblk, ((nblk + 7) / 8) * 8);
  }
  XG_LAUNCH_CHECK();
  return XG_OK;
}

#endif  // !XG_INT

}  // namespace

// ==========================================================================================
// C ABI
// ==========================================================================================
extern "C" {

int XG_FN(xg_binary)(int op, const real* a, const int64_t* a_strides, const real* b, const int64_t* b_strides,
                  real* out, const int64_t* shape, int ndim, void* stream) {
  if (!a || !b || !out || (ndim > 0 && (!shape || !a_strides || !b_strides))) return fail(XG_ERR_INVALID, "NULL argument");
  if (op < XG_BIN_MUL || op > XG_BIN_SUB) return fail(XG_ERR_INVALID, "unknown binary op %d", op);
#ifdef XG_INT
  if (op == XG_BIN_DIV) return fail(XG_ERR_UNSUPPORTED, "true division leaves the integer domain: convert to float64 first");
#endif
  if (ndim < 0 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [0,%d]", ndim, XG_MAX_NDIM);
  BinGeo g;
  memset(&g, 0, sizeof(g));
  // drop size-1 dims, coalesce neighbours compatible for BOTH operands
  int n = 0;
  int64_t total = 1;
  for (int d = 0; d < ndim; ++d) {
    if (shape[d] < 0) return fail(XG_ERR_INVALID, "negative extent");
    total *= shape[d];
    if (shape[d] == 1) continue;
    if (n > 0 && g.sa[n - 1] == a_strides[d] * shape[d] && g.sb[n - 1] == b_strides[d] * shape[d]) {
      g.shape[n - 1] *= shape[d];
      g.sa[n - 1] = a_strides[d];
      g.sb[n - 1] = b_strides[d];
    } else {
      g.shape[n] = shape[d];
      g.sa[n] = a_strides[d];
      g.sb[n] = b_strides[d];
      ++n;
    }
  }
  if (total == 0) return XG_OK;
  if (n == 0) { g.shape[0] = 1; g.sa[0] = 0; g.sb[0] = 0; n = 1; }
  g.ndim = n;
  const int64_t last = g.shape[n - 1];
  const int64_t sa = g.sa[n - 1], sb = g.sb[n - 1];
  bool v2 = (last % NV == 0) && aligned16(out) && (sa == 0 || sa == 1) && (sb == 0 || sb == 1);
  if (v2 && sa == 1) {
    if (!aligned16(a)) v2 = false;
    for (int d = 0; d < n - 1; ++d) if (g.sa[d] % NV) v2 = false;
  }
  if (v2 && sb == 1) {
    if (!aligned16(b)) v2 = false;
    for (int d = 0; d < n - 1; ++d) if (g.sb[d] % NV) v2 = false;
  }
  const int V = v2 ? NV : 1;
  g.shape[n - 1] = last / V;
  g.total = total / V;
  g.idx32 = (tune().bin_idx32 && (u64)g.total < 0xffffffffull) ? 1 : 0;
  for (int d = 0; d < XG_MAX_NDIM; ++d) g.fs[d] = make_fastdiv(d < n ? (u64)g.shape[d] : 1);
  u64 nitems = (u64)g.total;
  ZBand zb = make_zband(false, 0, 0, 1);
  if (tune().zband && n == 2 && (g.sa[0] == 0) != (g.sb[0] == 0) && g.shape[0] >= 2) {
    // exactly one operand is broadcast along the slow dim and re-read once per level: band it
    const u64 Z = (u64)g.shape[0], P = (u64)g.shape[1];
    const u32 B = 16384;  // items per band: 256 KiB of the broadcast operand at 16 B per item
    const u64 padded = ((P + B - 1) / B) * B * Z;
    if (P > 2 * (u64)B && padded < 0x7fffffffull) {
      zb = make_zband(true, Z, P, B);
      if (zb.on) nitems = padded;
    }
  }
  const u64 nblocks = (nitems + BLOCK - 1) / BLOCK;
  int rc;
  if ((rc = check_grid(nblocks + 8))) return rc;
  const u32 grid = (u32)(((nblocks + 7) / 8) * 8);  // XCD-banded block order
  // an operand without a broadcast dim is read exactly once: stream it past the caches
  auto streamed_once = [&](const int64_t* st_) { for (int d = 0; d < n; ++d) if (st_[d] == 0 && g.shape[d] > 1) return 0; return 1; };
  const int nta = tune().nt_load && streamed_once(g.sa), ntb = tune().nt_load && streamed_once(g.sb);
  hipStream_t st = (hipStream_t)stream;
  const bool nts = tune().nt_store;
#define XG_GO(O, V_, NTS) hipLaunchKernelGGL((k_binary<O, V_, NTS>), dim3(grid), dim3(BLOCK), 0, st, a, b, out, g, zb, (u32)nblocks, nta, ntb)
#define XG_O(O) do { if (V > 1) { if (nts) XG_GO(O, NV, true); else XG_GO(O, NV, false); } else { if (nts) XG_GO(O, 1, true); else XG_GO(O, 1, false); } } while (0)
  switch (op) { case XG_BIN_MUL: XG_O(XG_BIN_MUL); break; case XG_BIN_DIV: XG_O(XG_BIN_DIV); break; case XG_BIN_ADD: XG_O(XG_BIN_ADD); break; default: XG_O(XG_BIN_SUB); }
#undef XG_O
#undef XG_GO
  XG_LAUNCH_CHECK();
  return XG_OK;
}

#ifndef XG_INT
static int curl_div_impl(bool div, const real* u, const real* v, const real* area, const int64_t* area_strides,
                         real* out, const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y,
                         void* stream, const real* halo_x = nullptr, const real* halo_y = nullptr) {
  const char* name = div ? "divergence" : "vorticity";
  if (!u || !v || !out || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 2, {bc_x, bc_y}, XG_BC_HALO))) return rc;
  if (area && !area_strides) return fail(XG_ERR_INVALID, "area without strides");
  if ((bc_x == XG_BC_HALO && !halo_x) || (bc_y == XG_BC_HALO && !halo_y))
    return fail(XG_ERR_INVALID, "XG_BC_HALO without the halo buffer of that axis");
  FusedPlan p;
  const bool al = aligned16(u) && aligned16(v) && aligned16(out) && (bc_y != XG_BC_HALO || aligned16(halo_y));
  if ((rc = fused_plan(&p, name, shape, ndim, 2, al, area != nullptr, stream)) || p.empty) return rc;
  AreaIdx ai;
  int64_t a_sy, a_sx;
  if ((rc = area_index(area, area_strides, shape, ndim, &ai, &a_sy, &a_sx))) return rc;
  // bit 0: v rows non-temporal (neighbour by lane shuffle), bit 1: inner u rows, bit 2: the area rows are aligned vectors
  const int vnt = vec_nt_bits(3) | ((p.V > 1 && plane_vec_ok(area, ai, a_sy, a_sx)) ? 4 : 0);
  // levels per wave-task sharing the area rows: z-banded launches with the default vector lanes and stores only
  int zk = (p.V > 1 && p.nts) ? tune().vec_zk : 1;
  zk = zk >= 4 ? 4 : (zk >= 2 ? 2 : 1);
  // band height: the area rows of a band must survive in the XCD's 4 MB L2 while TWO fields and the output of all its
  // levels stream by.  16 rows: PMC reads 1.06x the algorithmic bytes (the halo u row of every band and level is the
  // 6 %); 24 rows 1.17x, 32 rows 1.26x -- the area is then re-read from the fabric once per level group -- at the same
  // speed within 1 % on an otherwise idle device (profiles/history/r03g_*, r03h_*)
  fused_band(&p, area && planes_shared(area, ai), band_rows(), ((u64)p.outer + zk - 1) / zk);
  if (!p.zb.on) zk = 1;
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GZ(V_, A_, NTS, ZK_) do { if (div) hipLaunchKernelGGL((k_divergence<V_, A_, NTS, FSEG, ZK_>), dim3(grid), dim3(BLOCK), 0, p.st, u, v, area, out, o0, nouter, nblk, p.ny, p.nx, p.fnt, p.fns, p.zb, bc_x, fill_x, bc_y, fill_y, ai, a_sy, a_sx, halo_x, halo_y, vnt); \
                                else hipLaunchKernelGGL((k_vorticity<V_, A_, NTS, FSEG, ZK_>), dim3(grid), dim3(BLOCK), 0, p.st, u, v, area, out, o0, nouter, nblk, p.ny, p.nx, p.fnt, p.fns, p.zb, bc_x, fill_x, bc_y, fill_y, ai, a_sy, a_sx, halo_x, halo_y, vnt); } while (0)
#define XG_GO(V_, A_, NTS) XG_GZ(V_, A_, NTS, 1)
#define XG_A(V_, A_) do { if (p.nts) XG_GO(V_, A_, true); else XG_GO(V_, A_, false); } while (0)
    if (zk == 4) XG_GZ(NV, true, true, 4);
    else if (zk == 2) XG_GZ(NV, true, true, 2);
    else if (p.V > 1) { if (area) XG_A(NV, true); else XG_A(NV, false); }
    else { if (area) XG_A(1, true); else XG_A(1, false); }
#undef XG_A
#undef XG_GO
#undef XG_GZ
  });
}

int XG_FN(xg_vorticity)(const real* u, const real* v, const real* area, const int64_t* area_strides, real* out,
                     const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y, void* stream) {
  if (bc_x == XG_BC_HALO || bc_y == XG_BC_HALO) return fail(XG_ERR_INVALID, "XG_BC_HALO needs xg_vorticity_halo");
  return curl_div_impl(false, u, v, area, area_strides, out, shape, ndim, bc_x, fill_x, bc_y, fill_y, stream);
}

int XG_FN(xg_divergence)(const real* u, const real* v, const real* area, const int64_t* area_strides, real* out,
                      const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y, void* stream) {
  if (bc_x == XG_BC_HALO || bc_y == XG_BC_HALO) return fail(XG_ERR_INVALID, "XG_BC_HALO needs xg_divergence_halo");
  return curl_div_impl(true, u, v, area, area_strides, out, shape, ndim, bc_x, fill_x, bc_y, fill_y, stream);
}

int XG_FN(xg_vorticity_halo)(const real* u, const real* v, const real* halo_x, const real* halo_y, const real* area,
                          const int64_t* area_strides, real* out, const int64_t* shape, int ndim, int bc_x,
                          real fill_x, int bc_y, real fill_y, void* stream) {
  return curl_div_impl(false, u, v, area, area_strides, out, shape, ndim, bc_x, fill_x, bc_y, fill_y, stream, halo_x, halo_y);
}

int XG_FN(xg_divergence_halo)(const real* u, const real* v, const real* halo_x, const real* halo_y, const real* area,
                           const int64_t* area_strides, real* out, const int64_t* shape, int ndim, int bc_x,
                           real fill_x, int bc_y, real fill_y, void* stream) {
  return curl_div_impl(true, u, v, area, area_strides, out, shape, ndim, bc_x, fill_x, bc_y, fill_y, stream, halo_x, halo_y);
}

static int pair2d_impl(int mode, const real* a, const real* u, const real* v, real* out_x, real* out_y,
                       const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y, const real* mx,
                       const int64_t* mx_strides, const real* my, const int64_t* my_strides, void* stream,
                       const real* halo_x = nullptr, const real* halo_y = nullptr) {
  const char* name = mode ? "flux" : "gradient";
  if (!a || !out_x || !out_y || !shape || (mode == 1 && (!u || !v))) return fail(XG_ERR_INVALID, "NULL array argument");
  if ((bc_x == XG_BC_HALO && !halo_x) || (bc_y == XG_BC_HALO && !halo_y)) return fail(XG_ERR_INVALID, "halo mode without a halo array");
  int rc;
  if ((rc = fused_dims(name, ndim, 2, {bc_x, bc_y}, (halo_x || halo_y) ? XG_BC_HALO : XG_BC_EXTEND))) return rc;
  bool al = aligned16(a) && aligned16(out_x) && aligned16(out_y);
  if (mode == 1) al = al && aligned16(u) && aligned16(v);
  if (bc_y == XG_BC_HALO) al = al && aligned16(halo_y);
  FusedPlan p;
  if ((rc = fused_plan(&p, name, shape, ndim, 2, al, true, stream)) || p.empty) return rc;
  AreaIdx aix, aiy;
  int64_t mx_sy, mx_sx, my_sy, my_sx;
  if ((rc = area_index(mx, mx_strides, shape, ndim, &aix, &mx_sy, &mx_sx))) return rc;
  if ((rc = area_index(my, my_strides, shape, ndim, &aiy, &my_sy, &my_sx))) return rc;
  const int vnt = vec_nt_bits(1);  // bit 0: field rows non-temporal + the left neighbour by DPP
  // gradient with metrics that every outer index shares (dxC(Y,X), dyC(Y,X) under a (Z,Y,X) field).  Rows per band: twice
  // `vec_zb_rows` (32) with one metric plane, `vec_zb_rows` (16) with two -- round 4, PMC per band height
  // (profiles/history/r04b_ab_bands_grad.log): two metrics 8 -> 16 rows reads 5.97 -> 5.65 GB (traffic 1.041 -> 1.021x), 32
  // rows 5.61 GB, all at the same speed; the two `nt`-stored outputs leave the L2 room the one-output kernels do not have
  // (their cliff sits between 8 and 16 rows for two metrics, r04b_ab_bands_met.log)
  fused_band(&p, mode == 0 && (mx || my) && planes_shared(mx, aix) && planes_shared(my, aiy),
             (mx && my) ? band_rows() : 2 * band_rows(), (u64)p.outer);
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, M_, NTS) hipLaunchKernelGGL((k_pair2d<V_, M_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, a, u, v, out_x, out_y, o0, nouter, nblk, p.ny, p.nx, p.fnt, p.fns, bc_x, fill_x, bc_y, fill_y, mx, aix, mx_sy, mx_sx, my, aiy, my_sy, my_sx, halo_x, halo_y, p.zb, vnt)
#define XG_M(V_, M_) do { if (p.nts) XG_GO(V_, M_, true); else XG_GO(V_, M_, false); } while (0)
    if (p.V > 1) { if (mode) XG_M(NV, 1); else XG_M(NV, 0); }
    else { if (mode) XG_M(1, 1); else XG_M(1, 0); }
#undef XG_M
#undef XG_GO
  });
}

int XG_FN(xg_gradient)(const real* a, real* out_x, real* out_y, const int64_t* shape, int ndim, int bc_x, real fill_x,
                    int bc_y, real fill_y, const real* mx, const int64_t* mx_strides, const real* my,
                    const int64_t* my_strides, void* stream) {
  return pair2d_impl(0, a, nullptr, nullptr, out_x, out_y, shape, ndim, bc_x, fill_x, bc_y, fill_y, mx, mx_strides, my,
                     my_strides, stream);
}

int XG_FN(xg_flux)(const real* u, const real* v, const real* t, real* out_x, real* out_y, const int64_t* shape, int ndim,
                int bc_x, real fill_x, int bc_y, real fill_y, void* stream) {
  return pair2d_impl(1, t, u, v, out_x, out_y, shape, ndim, bc_x, fill_x, bc_y, fill_y, nullptr, nullptr, nullptr, nullptr,
                     stream);
}

int XG_FN(xg_gradient_halo)(const real* a, const real* halo_x, const real* halo_y, real* out_x, real* out_y,
                         const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y, const real* mx,
                         const int64_t* mx_strides, const real* my, const int64_t* my_strides, void* stream) {
  return pair2d_impl(0, a, nullptr, nullptr, out_x, out_y, shape, ndim, bc_x, fill_x, bc_y, fill_y, mx, mx_strides, my,
                     my_strides, stream, halo_x, halo_y);
}

int XG_FN(xg_flux_halo)(const real* u, const real* v, const real* t, const real* halo_x, const real* halo_y, real* out_x,
                     real* out_y, const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y,
                     void* stream) {
  return pair2d_impl(1, t, u, v, out_x, out_y, shape, ndim, bc_x, fill_x, bc_y, fill_y, nullptr, nullptr, nullptr, nullptr,
                     stream, halo_x, halo_y);
}

// K7d's launcher: flux divergence (mode 1: u, v, t) or laplacian (mode 0: a = t, the four metrics all or none)
static int div2d_impl(int mode, const real* t, const real* u, const real* v, const real* const met[4],
                      const int64_t* const met_strides[4], const real* area, const int64_t* area_strides, real* out,
                      const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y, void* stream) {
  const char* name = mode ? "flux divergence" : "laplacian";
  if (!t || !out || !shape || (mode == 1 && (!u || !v))) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 2, {bc_x, bc_y}, XG_BC_EXTEND))) return rc;
  const int nmet = met ? (met[0] != nullptr) + (met[1] != nullptr) + (met[2] != nullptr) + (met[3] != nullptr) : 0;
  if (nmet != 0 && nmet != 4) return fail(XG_ERR_INVALID, "laplacian: the four metrics dxC, dyC, dyG, dxG, or none");
  bool al = aligned16(t) && aligned16(out);
  if (mode == 1) al = al && aligned16(u) && aligned16(v);
  FusedPlan p;
  if ((rc = fused_plan(&p, name, shape, ndim, 2, al, true, stream)) || p.empty) return rc;
  AreaIdx ai;
  int64_t a_sy, a_sx;
  if ((rc = area_index(area, area_strides, shape, ndim, &ai, &a_sy, &a_sx))) return rc;
  Div2dMet mt;
  memset(&mt, 0, sizeof(mt));
  for (int k = 0; k < 4; ++k) {
    mt.p[k] = nmet ? met[k] : nullptr;
    if ((rc = area_index(mt.p[k], nmet ? met_strides[k] : nullptr, shape, ndim, &mt.ai[k], &mt.sy[k], &mt.sx[k]))) return rc;
  }
  // bit 0: inner T rows non-temporal + the neighbours by DPP (K7c's scheme), bit 2: the area rows are aligned vectors
  int vnt = vec_nt_bits(1) | ((p.V > 1 && plane_vec_ok(area, ai, a_sy, a_sx)) ? 4 : 0);
  if (nmet) {  // bit 3: the four metric planes are aligned vectors as well
    bool mv = p.V > 1;
    for (int k = 0; k < 4; ++k) mv = mv && plane_vec_ok(mt.p[k], mt.ai[k], mt.sy[k], mt.sx[k]);
    vnt |= mv ? 8 : 0;
  }
  // K7b's 16 rows per band for the area alone, 8 with the five planes of the weighted laplacian (K7c: the more planes, the
  // lower the band)
  bool all_shared = (area || nmet) && planes_shared(area, ai);
  for (int k = 0; k < 4; ++k) all_shared = all_shared && planes_shared(mt.p[k], mt.ai[k]);
  fused_band(&p, all_shared, nmet ? (band_rows() + 1) / 2 : band_rows(), (u64)p.outer);
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, M_, A_, NTS) do { hipLaunchKernelGGL((k_div2d<V_, M_, A_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, t, u, v, area, out, o0, nouter, nblk, p.ny, p.nx, p.fnt, p.fns, p.zb, bc_x, fill_x, bc_y, fill_y, ai, a_sy, a_sx, mt, vnt); } while (0)
#define XG_A(V_, M_) do { if (area) { if (p.nts) XG_GO(V_, M_, true, true); else XG_GO(V_, M_, true, false); } \
                          else { if (p.nts) XG_GO(V_, M_, false, true); else XG_GO(V_, M_, false, false); } } while (0)
    if (p.V > 1) { if (mode) XG_A(NV, 1); else XG_A(NV, 0); }
    else { if (mode) XG_A(1, 1); else XG_A(1, 0); }
#undef XG_A
#undef XG_GO
  });
}

int XG_FN(xg_flux_divergence)(const real* u, const real* v, const real* t, const real* area, const int64_t* area_strides,
                              real* out, const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y,
                              void* stream) {
  return div2d_impl(1, t, u, v, nullptr, nullptr, area, area_strides, out, shape, ndim, bc_x, fill_x, bc_y, fill_y, stream);
}

int XG_FN(xg_laplacian)(const real* a, const real* dxC, const int64_t* dxC_strides, const real* dyC,
                        const int64_t* dyC_strides, const real* dyG, const int64_t* dyG_strides, const real* dxG,
                        const int64_t* dxG_strides, const real* area, const int64_t* area_strides, real* out,
                        const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y, void* stream) {
  const real* const met[4] = {dxC, dyG, dyC, dxG};  // K7d's order: the Fx pair, then the Fy pair
  const int64_t* const ms[4] = {dxC_strides, dyG_strides, dyC_strides, dxG_strides};
  return div2d_impl(0, a, nullptr, nullptr, met, ms, area, area_strides, out, shape, ndim, bc_x, fill_x, bc_y, fill_y,
                    stream);
}

// K7e's launcher: (lead, Z, Y, X) fields, the volume `vol` (* `vol2`) with broadcast strides, one wave per column
int XG_FN(xg_flux_divergence3d)(const real* u, const real* v, const real* w, const real* t, const real* vol,
                                const int64_t* vol_strides, const real* vol2, const int64_t* vol2_strides, real* out,
                                const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z,
                                real fill_z, void* stream) {
  const char* name = "3-D flux divergence";
  if (!u || !v || !w || !t || !out || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {bc_x, bc_y, bc_z}, XG_BC_EXTEND))) return rc;
  if (vol2 && !vol) return fail(XG_ERR_INVALID, "3-D flux divergence: a second volume factor without the first");
  if ((vol && !vol_strides) || (vol2 && !vol2_strides)) return fail(XG_ERR_INVALID, "metric without strides");
  FusedPlan p;
  const bool al = aligned16(t) && aligned16(u) && aligned16(v) && aligned16(w) && aligned16(out);
  if ((rc = fused_plan(&p, name, shape, ndim, 3, al, true, stream)) || p.empty) return rc;
  VolIdx vi[2];
  if ((rc = vol_index(&vi[0], vol, vol_strides, shape, ndim))) return rc;
  if ((rc = vol_index(&vi[1], vol2, vol2_strides, shape, ndim))) return rc;
  // bit 0: the lane neighbours by DPP (K7d), bits 2 / 3: the rows of volume factor 0 / 1 are aligned vectors
  int vnt = vec_nt_bits(1);
  for (int k = 0; k < 2; ++k)
    if (p.V > 1 && vi[k].sz % NV == 0 && plane_vec_ok(vi[k].p, vi[k].ai, vi[k].sy, vi[k].sx)) vnt |= 4 << k;
  const int nvol = (vol != nullptr) + (vol2 != nullptr);
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, N_, NTS) do { hipLaunchKernelGGL((k_div3d<V_, N_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, t, u, v, w, out, o0, nouter, nblk, p.nz, p.ny, p.nx, p.fnt, p.fns, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, vi[0], vi[1], vnt); } while (0)
#define XG_N(V_, N_) do { if (p.nts) XG_GO(V_, N_, true); else XG_GO(V_, N_, false); } while (0)
#define XG_V(V_) do { if (nvol == 2) XG_N(V_, 2); else if (nvol == 1) XG_N(V_, 1); else XG_N(V_, 0); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_N
#undef XG_GO
  });
}

// K7f's launcher: (lead, Z, Y, X) fields, five optional broadcast metrics (face weights of u and of v, two factors each,
// and the area of the result), one wave per column
#ifndef XG_WCONT_WINDOW
#define XG_WCONT_WINDOW 3  // levels in flight ahead of the running sum
#endif
int XG_FN(xg_vertical_velocity)(const real* u, const real* v, const real* mu, const int64_t* mu_strides, const real* mu2,
                                const int64_t* mu2_strides, const real* mv, const int64_t* mv_strides, const real* mv2,
                                const int64_t* mv2_strides, const real* area, const int64_t* area_strides, real* out,
                                const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z,
                                real fill_z, int reverse, void* stream) {
  const char* name = "vertical velocity";
  if (!u || !v || !out || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {bc_x, bc_y}, XG_BC_EXTEND))) return rc;
  if (!reverse && bc_z != XG_BC_FILL && bc_z != XG_BC_EXTEND)
    return fail(XG_ERR_UNSUPPORTED, "vertical velocity summed upward pads Z with fill or extend (periodic needs the column total first)");
  if ((mu != nullptr) != (mv != nullptr)) return fail(XG_ERR_INVALID, "vertical velocity: face weights for both u and v, or for neither");
  if ((mu2 && !mu) || (mv2 && !mv)) return fail(XG_ERR_INVALID, "vertical velocity: a second face-weight factor without the first");
  FusedPlan p;
  if ((rc = fused_plan(&p, name, shape, ndim, 3, aligned16(u) && aligned16(v) && aligned16(out), true, stream)) || p.empty) return rc;
  VolIdx mi[5];  // u: a, b; v: a, b; area
  const real* mp[5] = {mu, mu2, mv, mv2, area};
  const int64_t* ms[5] = {mu_strides, mu2_strides, mv_strides, mv2_strides, area_strides};
  for (int k = 0; k < 5; ++k)
    if ((rc = vol_index(&mi[k], mp[k], ms[k], shape, ndim))) return rc;
  for (int k : {1, 3})
    if (mp[k] && (mi[k].sy != 0 || mi[k].sx != 0))
      return fail(XG_ERR_UNSUPPORTED, "vertical velocity: the second face-weight factor varies along Z (and leading dims) only");
  constexpr int U = XG_WCONT_WINDOW;
  // bit 0: the lane neighbour by DPP (K7d), bits 2 / 3 / 4: the rows of u's factor a / v's factor a / the area are aligned vectors
  int vnt = vec_nt_bits(1);
  const int vec_of[3] = {0, 2, 4};
  for (int k = 0; k < 3; ++k) {
    const VolIdx& m = mi[vec_of[k]];
    if (p.V > 1 && m.p && m.sz % NV == 0 && plane_vec_ok(m.p, m.ai, m.sy, m.sx)) vnt |= 4 << k;
  }
  const bool fw = mu != nullptr, ar = area != nullptr;
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, F_, A_, NTS) do { hipLaunchKernelGGL((k_wcont<V_, F_, A_, NTS, FSEG, U>), dim3(grid), dim3(BLOCK), 0, p.st, u, v, out, o0, nouter, nblk, p.nz, p.ny, p.nx, p.fnt, p.fns, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, reverse ? 1 : 0, mi[0], mi[1], mi[2], mi[3], mi[4], vnt); } while (0)
#define XG_N(V_, F_, A_) do { if (p.nts) XG_GO(V_, F_, A_, true); else XG_GO(V_, F_, A_, false); } while (0)
#define XG_A(V_, F_) do { if (ar) XG_N(V_, F_, true); else XG_N(V_, F_, false); } while (0)
#define XG_V(V_) do { if (fw) XG_A(V_, true); else XG_A(V_, false); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_A
#undef XG_N
#undef XG_GO
  });
}

// K7g's launcher
int XG_FN(xg_kinetic_energy)(const real* u, const real* v, real* out, const int64_t* shape, int ndim, int bc_x, real fill_x,
                             int bc_y, real fill_y, void* stream) {
  const char* name = "kinetic energy";
  if (!u || !v || !out || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 2, {bc_x, bc_y}, XG_BC_EXTEND))) return rc;
  FusedPlan p;
  if ((rc = fused_plan(&p, name, shape, ndim, 2, aligned16(u) && aligned16(v) && aligned16(out), true, stream)) || p.empty) return rc;
  const int vnt = vec_nt_bits(1);  // bit 0: the right neighbour by DPP (K7d)
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, NTS) do { hipLaunchKernelGGL((k_kinetic<V_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, u, v, out, o0, nouter, nblk, p.ny, p.nx, p.fnt, p.fns, bc_x, fill_x, bc_y, fill_y, vnt); } while (0)
    if (p.V > 1) { if (p.nts) XG_GO(NV, true); else XG_GO(NV, false); }
    else { if (p.nts) XG_GO(1, true); else XG_GO(1, false); }
#undef XG_GO
  });
}

// K7h's launcher: the three metrics all or none; the coriolis plane on its own
int XG_FN(xg_momentum_advection)(const real* u, const real* v, const real* coriolis, const int64_t* coriolis_strides,
                                 const real* rAz, const int64_t* rAz_strides, const real* dxC, const int64_t* dxC_strides,
                                 const real* dyC, const int64_t* dyC_strides, real* out_u, real* out_v,
                                 const int64_t* shape, int ndim, int bc_x, real fill_x, int bc_y, real fill_y, void* stream) {
  const char* name = "momentum advection";
  if (!u || !v || !out_u || !out_v || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 2, {bc_x, bc_y}, XG_BC_EXTEND))) return rc;
  const int nmet = (rAz != nullptr) + (dxC != nullptr) + (dyC != nullptr);
  if (nmet != 0 && nmet != 3) return fail(XG_ERR_INVALID, "momentum advection: the three metrics rAz, dxC, dyC, or none");
  FusedPlan p;
  const bool al = aligned16(u) && aligned16(v) && aligned16(out_u) && aligned16(out_v);
  if ((rc = fused_plan(&p, name, shape, ndim, 2, al, true, stream)) || p.empty) return rc;
  Div2dMet mt;
  memset(&mt, 0, sizeof(mt));
  const real* mp[4] = {rAz, coriolis, dxC, dyC};
  const int64_t* ms[4] = {rAz_strides, coriolis_strides, dxC_strides, dyC_strides};
  for (int k = 0; k < 4; ++k) {
    mt.p[k] = mp[k];
    if ((rc = area_index(mp[k], ms[k], shape, ndim, &mt.ai[k], &mt.sy[k], &mt.sx[k]))) return rc;
  }
  // bit 0: the lane neighbours by DPP (K7d), bit 3: every plane that is there is an aligned vector in every row
  int vnt = vec_nt_bits(1);
  const bool met = nmet != 0, cor = coriolis != nullptr;
  bool all_shared = met || cor;
  if (met || cor) {
    bool mv = p.V > 1;
    for (int k = 0; k < 4; ++k) {
      if (mt.p[k]) mv = mv && plane_vec_ok(mt.p[k], mt.ai[k], mt.sy[k], mt.sx[k]);
      all_shared = all_shared && planes_shared(mt.p[k], mt.ai[k]);
    }
    vnt |= mv ? 8 : 0;
  }
  // 8-row bands as the weighted laplacian's five planes (K7d)
  fused_band(&p, all_shared, (band_rows() + 1) / 2, (u64)p.outer);
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, M_, C_, NTS) do { hipLaunchKernelGGL((k_momadv<V_, M_, C_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, u, v, out_u, out_v, o0, nouter, nblk, p.ny, p.nx, p.fnt, p.fns, p.zb, bc_x, fill_x, bc_y, fill_y, mt, vnt); } while (0)
#define XG_N(V_, M_, C_) do { if (p.nts) XG_GO(V_, M_, C_, true); else XG_GO(V_, M_, C_, false); } while (0)
#define XG_C(V_, M_) do { if (cor) XG_N(V_, M_, true); else XG_N(V_, M_, false); } while (0)
#define XG_V(V_) do { if (met) XG_C(V_, true); else XG_C(V_, false); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_C
#undef XG_N
#undef XG_GO
  });
}

// K7k's launcher: the six metrics all or none, the two coefficient planes both or none
static int hvisc_impl(const real* u, const real* v, const real* const planes[8], const int64_t* const strides[8],
                      real* out_u, real* out_v, const int64_t* shape, int ndim, int bc_x, real fill_x, real zfill_x,
                      int bc_y, real fill_y, real zfill_y, void* stream) {
  const char* name = "horizontal viscosity";
  if (!u || !v || !out_u || !out_v || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 2, {bc_x, bc_y}, XG_BC_EXTEND))) return rc;
  int nmet = 0, nvis = 0;
  for (int k = 0; k < 8; ++k) (k < 6 ? nmet : nvis) += planes[k] != nullptr;
  if (nmet != 0 && nmet != 6) return fail(XG_ERR_INVALID, "horizontal viscosity: the six metrics rA, rAz, dxC, dyC, dyG, dxG, or none");
  if (nvis != 0 && nvis != 2) return fail(XG_ERR_INVALID, "horizontal viscosity: both coefficients nu_d, nu_z, or none");
  FusedPlan p;
  const bool al = aligned16(u) && aligned16(v) && aligned16(out_u) && aligned16(out_v);
  if ((rc = fused_plan(&p, name, shape, ndim, 2, al, true, stream)) || p.empty) return rc;
  HviscPlanes mt;
  memset(&mt, 0, sizeof(mt));
  for (int k = 0; k < 8; ++k) {
    mt.p[k] = planes[k];
    if ((rc = area_index(planes[k], strides[k], shape, ndim, &mt.ai[k], &mt.sy[k], &mt.sx[k]))) return rc;
  }
  // bit 0: the lane neighbours by DPP (K7d), bit 3: every plane that is there is an aligned vector in every row
  int vnt = vec_nt_bits(1);
  const bool met = nmet != 0, vis = nvis != 0;
  bool all_shared = met || vis;
  if (met || vis) {
    bool mv = p.V > 1;
    for (int k = 0; k < 8; ++k) {
      if (mt.p[k]) mv = mv && plane_vec_ok(mt.p[k], mt.ai[k], mt.sy[k], mt.sx[k]);
      all_shared = all_shared && planes_shared(mt.p[k], mt.ai[k]);
    }
    vnt |= mv ? 8 : 0;
  }
  // 8-row bands as K7h's four planes; 4 with all eight (K7c: the more planes, the lower the band)
  fused_band(&p, all_shared, (met && vis) ? (band_rows() + 3) / 4 : (band_rows() + 1) / 2, (u64)p.outer);
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, M_, C_, NTS) do { hipLaunchKernelGGL((k_hvisc<V_, M_, C_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, u, v, out_u, out_v, o0, nouter, nblk, p.ny, p.nx, p.fnt, p.fns, p.zb, bc_x, fill_x, zfill_x, bc_y, fill_y, zfill_y, mt, vnt); } while (0)
#define XG_N(V_, M_, C_) do { if (p.nts) XG_GO(V_, M_, C_, true); else XG_GO(V_, M_, C_, false); } while (0)
#define XG_C(V_, M_) do { if (vis) XG_N(V_, M_, true); else XG_N(V_, M_, false); } while (0)
#define XG_V(V_) do { if (met) XG_C(V_, true); else XG_C(V_, false); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_C
#undef XG_N
#undef XG_GO
  });
}

int XG_FN(xg_horizontal_viscosity)(const real* u, const real* v, const real* rA, const int64_t* rA_strides, const real* rAz,
                                   const int64_t* rAz_strides, const real* dxC, const int64_t* dxC_strides, const real* dyC,
                                   const int64_t* dyC_strides, const real* dyG, const int64_t* dyG_strides, const real* dxG,
                                   const int64_t* dxG_strides, const real* nu_d, const int64_t* nu_d_strides,
                                   const real* nu_z, const int64_t* nu_z_strides, real* out_u, real* out_v,
                                   const int64_t* shape, int ndim, int bc_x, real fill_x, real zfill_x, int bc_y,
                                   real fill_y, real zfill_y, void* stream) {
  const real* const planes[8] = {rA, rAz, dxC, dyC, dyG, dxG, nu_d, nu_z};
  const int64_t* const strides[8] = {rA_strides, rAz_strides, dxC_strides, dyC_strides, dyG_strides, dxG_strides,
                                     nu_d_strides, nu_z_strides};
  return hvisc_impl(u, v, planes, strides, out_u, out_v, shape, ndim, bc_x, fill_x, zfill_x, bc_y, fill_y, zfill_y, stream);
}

// K7i's launcher: (lead, Z, Y, X) fields, three optional broadcast metrics (the Z weight, dxC, dyC), one wave per column
#ifndef XG_PGRAD_WINDOW
#define XG_PGRAD_WINDOW XG_WCONT_WINDOW  // levels in flight ahead of the running sums
#endif
int XG_FN(xg_hydrostatic_pressure_gradient)(const real* b, const real* w, const int64_t* w_strides, const real* dxC,
                                            const int64_t* dxC_strides, const real* dyC, const int64_t* dyC_strides,
                                            real* out_x, real* out_y, const int64_t* shape, int ndim, int bc_x, real fill_x,
                                            int bc_y, real fill_y, int bc_z, real fill_z, void* stream) {
  const char* name = "hydrostatic pressure gradient";
  if (!b || !out_x || !out_y || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {bc_x, bc_y, bc_z}, XG_BC_EXTEND))) return rc;
  if (bc_z != XG_BC_FILL && bc_z != XG_BC_EXTEND)
    return fail(XG_ERR_UNSUPPORTED, "hydrostatic pressure gradient pads Z with fill or extend (periodic needs the column total first)");
  FusedPlan p;
  if ((rc = fused_plan(&p, name, shape, ndim, 3, aligned16(b) && aligned16(out_x) && aligned16(out_y), true, stream)) || p.empty) return rc;
  VolIdx mi[3];  // the Z weight, dxC, dyC
  const real* mp[3] = {w, dxC, dyC};
  const int64_t* ms[3] = {w_strides, dxC_strides, dyC_strides};
  for (int k = 0; k < 3; ++k)
    if ((rc = vol_index(&mi[k], mp[k], ms[k], shape, ndim))) return rc;
  constexpr int U = XG_PGRAD_WINDOW;
  // bit 0: the lane neighbour by DPP (K7c), bits 2 / 3 / 4: the rows of the Z weight / dxC / dyC are aligned vectors
  int vnt = vec_nt_bits(1);
  for (int k = 0; k < 3; ++k)
    if (p.V > 1 && mi[k].p && mi[k].sz % NV == 0 && plane_vec_ok(mi[k].p, mi[k].ai, mi[k].sy, mi[k].sx)) vnt |= 4 << k;
  const bool met = dxC != nullptr || dyC != nullptr;
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, M_, NTS) do { hipLaunchKernelGGL((k_pgrad<V_, M_, NTS, FSEG, U>), dim3(grid), dim3(BLOCK), 0, p.st, b, out_x, out_y, o0, nouter, nblk, p.nz, p.ny, p.nx, p.fnt, p.fns, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, mi[0], mi[1], mi[2], vnt); } while (0)
#define XG_N(V_, M_) do { if (p.nts) XG_GO(V_, M_, true); else XG_GO(V_, M_, false); } while (0)
#define XG_V(V_) do { if (met) XG_N(V_, true); else XG_N(V_, false); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_N
#undef XG_GO
  });
}

// K7j's launcher: (lead, Z, Y, X) fields, two optional broadcast metrics (the Z metric at u's and at v's points), one wave
// per column
int XG_FN(xg_vertical_momentum_advection)(const real* u, const real* v, const real* w, const real* mu,
                                          const int64_t* mu_strides, const real* mv, const int64_t* mv_strides,
                                          real* out_u, real* out_v, const int64_t* shape, int ndim, int bc_x, real fill_x,
                                          int bc_y, real fill_y, int bc_z, real fill_z, void* stream) {
  const char* name = "vertical momentum advection";
  if (!u || !v || !w || !out_u || !out_v || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {bc_x, bc_y, bc_z}, XG_BC_EXTEND))) return rc;
  FusedPlan p;
  const bool al = aligned16(u) && aligned16(v) && aligned16(w) && aligned16(out_u) && aligned16(out_v);
  if ((rc = fused_plan(&p, name, shape, ndim, 3, al, true, stream)) || p.empty) return rc;
  VolIdx mi[2];  // the metric of gu, of gv
  const real* mp[2] = {mu, mv};
  const int64_t* ms[2] = {mu_strides, mv_strides};
  for (int k = 0; k < 2; ++k)
    if ((rc = vol_index(&mi[k], mp[k], ms[k], shape, ndim))) return rc;
  // bit 0: the lane neighbour by DPP (K7e), bits 2 / 3: the rows of the metric of gu / gv are aligned vectors
  int vnt = vec_nt_bits(1);
  for (int k = 0; k < 2; ++k)
    if (p.V > 1 && mi[k].p && mi[k].sz % NV == 0 && plane_vec_ok(mi[k].p, mi[k].ai, mi[k].sy, mi[k].sx)) vnt |= 4 << k;
  const bool met = mu != nullptr || mv != nullptr;
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, M_, NTS) do { hipLaunchKernelGGL((k_vmomadv<V_, M_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, u, v, w, out_u, out_v, o0, nouter, nblk, p.nz, p.ny, p.nx, p.fnt, p.fns, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, mi[0], mi[1], vnt); } while (0)
#define XG_N(V_, M_) do { if (p.nts) XG_GO(V_, M_, true); else XG_GO(V_, M_, false); } while (0)
#define XG_V(V_) do { if (met) XG_N(V_, true); else XG_N(V_, false); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_N
#undef XG_GO
  });
}

// K7l's launcher: one (lead, Z, Y, X) field, kappa and the metric of the flux (both at the flux levels: nz of them, `outer`
// nz + 1) and the metric of the result, each optional and with broadcast strides, one wave per column.  The ABI has ONE
// entry for both element types (xg_vertical_diffusion, below); each float build defines its own implementation, hidden.
__attribute__((visibility("hidden"))) int xg_internal_vdiff_f64(
    const double* a, const double* kappa, const int64_t* kappa_strides, const double* mf, const int64_t* mf_strides,
    const double* mc, const int64_t* mc_strides, double* out, const int64_t* shape, int ndim, int outer, int bc_z,
    double fill_z, void* stream);
__attribute__((visibility("hidden"))) int xg_internal_vdiff_f32(
    const float* a, const float* kappa, const int64_t* kappa_strides, const float* mf, const int64_t* mf_strides,
    const float* mc, const int64_t* mc_strides, float* out, const int64_t* shape, int ndim, int outer, int bc_z,
    float fill_z, void* stream);

int XG_FN(xg_internal_vdiff)(const real* a, const real* kappa, const int64_t* kappa_strides, const real* mf,
                             const int64_t* mf_strides, const real* mc, const int64_t* mc_strides, real* out,
                             const int64_t* shape, int ndim, int outer, int bc_z, real fill_z, void* stream) {
  const char* name = "vertical diffusion";
  if (!a || !out || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {bc_z}, XG_BC_EXTEND))) return rc;
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  FusedPlan p;
  if ((rc = fused_plan(&p, name, shape, ndim, 3, aligned16(a) && aligned16(out), true, stream)) || p.empty) return rc;
  VolIdx mi[3];  // kappa, the metric of the flux, the metric of the result
  const real* mp[3] = {kappa, mf, mc};
  const int64_t* ms[3] = {kappa_strides, mf_strides, mc_strides};
  for (int k = 0; k < 3; ++k)
    if ((rc = vol_index(&mi[k], mp[k], ms[k], shape, ndim))) return rc;
  // bits 2 / 3 / 4: the rows of kappa / the flux metric / the result's metric are aligned vectors (no X neighbour: no bit 0)
  int vnt = 0;
  for (int k = 0; k < 3; ++k)
    if (p.V > 1 && mi[k].p && mi[k].sz % NV == 0 && plane_vec_ok(mi[k].p, mi[k].ai, mi[k].sy, mi[k].sx)) vnt |= 4 << k;
  const bool kap = kappa != nullptr, met = mf != nullptr || mc != nullptr;
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, K_, M_, NTS) do { hipLaunchKernelGGL((k_vdiff<V_, K_, M_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, a, out, o0, nouter, nblk, p.nz, p.ny, p.nx, p.fnt, p.fns, outer, bc_z, fill_z, mi[0], mi[1], mi[2], vnt); } while (0)
#define XG_N(V_, K_, M_) do { if (p.nts) XG_GO(V_, K_, M_, true); else XG_GO(V_, K_, M_, false); } while (0)
#define XG_M(V_, K_) do { if (met) XG_N(V_, K_, true); else XG_N(V_, K_, false); } while (0)
#define XG_V(V_) do { if (kap) XG_M(V_, true); else XG_M(V_, false); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_M
#undef XG_N
#undef XG_GO
  });
}

#ifdef XG_PRIMARY
// the exported entry (defined once, in the float64 build): the element type is an argument, the fill is cast to it here
int xg_vertical_diffusion(int dtype, const void* a, const void* kappa, const int64_t* kappa_strides, const void* mf,
                          const int64_t* mf_strides, const void* mc, const int64_t* mc_strides, void* out,
                          const int64_t* shape, int ndim, int outer, int bc_z, double fill_z, void* stream) {
  if (dtype == XG_T_F64)
    return xg_internal_vdiff_f64((const double*)a, (const double*)kappa, kappa_strides, (const double*)mf, mf_strides,
                                 (const double*)mc, mc_strides, (double*)out, shape, ndim, outer, bc_z, fill_z, stream);
  if (dtype == XG_T_F32)
    return xg_internal_vdiff_f32((const float*)a, (const float*)kappa, kappa_strides, (const float*)mf, mf_strides,
                                 (const float*)mc, mc_strides, (float*)out, shape, ndim, outer, bc_z, (float)fill_z, stream);
  return fail(XG_ERR_INVALID, "vertical diffusion: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
#endif

// The launches of K7m / K7o, the implicit sweeps: one field, its workspace and its result, the coefficient's source `src`
// (k_vimpl's SRC) with its array `kp` (kappa or nu; `bc` and `fill` pad nu), the metric of the flux and of the result.
static int vimpl_launch(const FusedPlan& p, int src, const real* a, real* work, real* out, real dt, int bc, real fill,
                        const VolIdx& kp, const VolIdx& mf, const VolIdx& mc, int vnt) {
  const bool met = mf.p != nullptr || mc.p != nullptr;
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, K_, M_, NTS) do { hipLaunchKernelGGL((k_vimpl<V_, K_, M_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, a, work, out, o0, nouter, nblk, p.nz, p.ny, p.nx, p.fnt, p.fns, dt, kp, mf, mc, vnt, bc, fill); } while (0)
#define XG_N(V_, K_, M_) do { if (p.nts) XG_GO(V_, K_, M_, true); else XG_GO(V_, K_, M_, false); } while (0)
#define XG_M(V_, K_) do { if (met) XG_N(V_, K_, true); else XG_N(V_, K_, false); } while (0)
#define XG_V(V_) do { if (src == VI_NU_V) XG_M(V_, VI_NU_V); else if (src == VI_NU_U) XG_M(V_, VI_NU_U); else if (src == VI_KAPPA) XG_M(V_, VI_KAPPA); else XG_M(V_, VI_ONE); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_M
#undef XG_N
#undef XG_GO
  });
}

// K7m's launcher: K7l's arguments without a boundary (the solve is the no-flux one) and with a workspace of the field's shape
// for the forward sweep's c.  `outer` only says how many faces kappa and mf have (nz or nz + 1): faces 1 .. nz-1 are read
// either way, at the same strides.  One ABI entry for both element types (xg_implicit_vertical_diffusion, below).
__attribute__((visibility("hidden"))) int xg_internal_vimpl_f64(
    const double* a, const double* kappa, const int64_t* kappa_strides, const double* mf, const int64_t* mf_strides,
    const double* mc, const int64_t* mc_strides, double* work, double* out, const int64_t* shape, int ndim, int outer,
    double dt, void* stream);
__attribute__((visibility("hidden"))) int xg_internal_vimpl_f32(
    const float* a, const float* kappa, const int64_t* kappa_strides, const float* mf, const int64_t* mf_strides,
    const float* mc, const int64_t* mc_strides, float* work, float* out, const int64_t* shape, int ndim, int outer,
    float dt, void* stream);

int XG_FN(xg_internal_vimpl)(const real* a, const real* kappa, const int64_t* kappa_strides, const real* mf,
                             const int64_t* mf_strides, const real* mc, const int64_t* mc_strides, real* work, real* out,
                             const int64_t* shape, int ndim, int outer, real dt, void* stream) {
  const char* name = "implicit vertical diffusion";
  if (!a || !out || !work || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {}, XG_BC_EXTEND))) return rc;
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  const real* mp[3] = {kappa, mf, mc};  // kappa, the metric of the flux, the metric of the result
  const int64_t* ms[3] = {kappa_strides, mf_strides, mc_strides};
  for (int k = 0; k < 3; ++k)
    if (mp[k] && !ms[k]) return fail(XG_ERR_INVALID, "%s: a plane without strides", name);
  FusedPlan p;
  if ((rc = fused_plan(&p, name, shape, ndim, 3, aligned16(a) && aligned16(out) && aligned16(work), true, stream)) || p.empty)
    return rc;
  VolIdx mi[3];
  for (int k = 0; k < 3; ++k)
    if ((rc = vol_index(&mi[k], mp[k], ms[k], shape, ndim))) return rc;
  // bits 2 / 3 / 4: the rows of kappa / the flux metric / the result's metric are aligned vectors (no X neighbour: no bit 0)
  int vnt = 0;
  for (int k = 0; k < 3; ++k)
    if (p.V > 1 && mi[k].p && mi[k].sz % NV == 0 && plane_vec_ok(mi[k].p, mi[k].ai, mi[k].sy, mi[k].sx)) vnt |= 4 << k;
  return vimpl_launch(p, kappa ? VI_KAPPA : VI_ONE, a, work, out, dt, XG_BC_EXTEND, real(0), mi[0], mi[1], mi[2], vnt);
}

#ifdef XG_PRIMARY
// the exported entry (defined once, in the float64 build): the element type is an argument, dt is cast to it here, once
int xg_implicit_vertical_diffusion(int dtype, const void* a, const void* kappa, const int64_t* kappa_strides, const void* mf,
                                   const int64_t* mf_strides, const void* mc, const int64_t* mc_strides, void* work, void* out,
                                   const int64_t* shape, int ndim, int outer, double dt, void* stream) {
  if (!(dt >= 0.0) || !__builtin_isfinite(dt))
    return fail(XG_ERR_INVALID, "implicit vertical diffusion: dt %g is negative or not finite", dt);
  if (dtype == XG_T_F64)
    return xg_internal_vimpl_f64((const double*)a, (const double*)kappa, kappa_strides, (const double*)mf, mf_strides,
                                 (const double*)mc, mc_strides, (double*)work, (double*)out, shape, ndim, outer, dt, stream);
  if (dtype == XG_T_F32)
    return xg_internal_vimpl_f32((const float*)a, (const float*)kappa, kappa_strides, (const float*)mf, mf_strides,
                                 (const float*)mc, mc_strides, (float*)work, (float*)out, shape, ndim, outer, (float)dt, stream);
  return fail(XG_ERR_INVALID, "implicit vertical diffusion: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
#endif

// K7o's launcher: K7m's arguments twice -- u and v, a workspace and a result each, the metric of the flux and of the result at
// u's and at v's points -- with ONE nu at the centre points of the faces and the boundaries that pad it along X and Y.  One
// plan for both components (same shape; the lane width is NV only when all six field pointers are 16-byte aligned), one launch
// of k_vimpl per component (SRC VI_NU_U, then VI_NU_V).  One ABI entry for both element types
// (xg_implicit_vertical_viscosity, below).
__attribute__((visibility("hidden"))) int xg_internal_vvisc_f64(
    const double* u, const double* v, const double* nu, const int64_t* nu_strides, const double* const met[4],
    const int64_t* const met_strides[4], double* work_u, double* work_v, double* out_u, double* out_v, const int64_t* shape,
    int ndim, int outer, int bc_x, double fill_x, int bc_y, double fill_y, double dt, void* stream);
__attribute__((visibility("hidden"))) int xg_internal_vvisc_f32(
    const float* u, const float* v, const float* nu, const int64_t* nu_strides, const float* const met[4],
    const int64_t* const met_strides[4], float* work_u, float* work_v, float* out_u, float* out_v, const int64_t* shape,
    int ndim, int outer, int bc_x, float fill_x, int bc_y, float fill_y, float dt, void* stream);

int XG_FN(xg_internal_vvisc)(const real* u, const real* v, const real* nu, const int64_t* nu_strides, const real* const met[4],
                             const int64_t* const met_strides[4], real* work_u, real* work_v, real* out_u, real* out_v,
                             const int64_t* shape, int ndim, int outer, int bc_x, real fill_x, int bc_y, real fill_y, real dt,
                             void* stream) {
  const char* name = "implicit vertical viscosity";
  if (!u || !v || !nu || !out_u || !out_v || !work_u || !work_v || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {bc_x, bc_y}, XG_BC_EXTEND))) return rc;
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  if (!nu_strides) return fail(XG_ERR_INVALID, "%s: a plane without strides", name);
  for (int k = 0; k < 4; ++k)
    if (met[k] && !met_strides[k]) return fail(XG_ERR_INVALID, "%s: a plane without strides", name);
  FusedPlan p;
  const bool al = aligned16(u) && aligned16(v) && aligned16(out_u) && aligned16(out_v) && aligned16(work_u) && aligned16(work_v);
  if ((rc = fused_plan(&p, name, shape, ndim, 3, al, true, stream)) || p.empty) return rc;
  VolIdx ni, mi[4];  // nu; the metric of the flux and of the result at u's points, then at v's
  if ((rc = vol_index(&ni, nu, nu_strides, shape, ndim))) return rc;
  for (int k = 0; k < 4; ++k)
    if ((rc = vol_index(&mi[k], met[k], met_strides[k], shape, ndim))) return rc;
  auto vec = [&](const VolIdx& x) { return p.V > 1 && x.p && x.sz % NV == 0 && plane_vec_ok(x.p, x.ai, x.sy, x.sx); };
  const real* fa[2] = {u, v};
  real* fw[2] = {work_u, work_v};
  real* fo[2] = {out_u, out_v};
  const int fbc[2] = {bc_x, bc_y};
  const real ffill[2] = {fill_x, fill_y};
  for (int c = 0; c < 2; ++c) {
    const VolIdx &mf = mi[2 * c], &mc = mi[2 * c + 1];
    // bit 0: the lane neighbour by DPP (K7j; u only), bits 2 / 3 / 4: the rows of nu / the flux metric / the result's metric
    // are aligned vectors
    const int vnt = (c == 0 ? vec_nt_bits(1) : 0) | (vec(ni) ? 4 : 0) | (vec(mf) ? 8 : 0) | (vec(mc) ? 16 : 0);
    rc = vimpl_launch(p, c == 0 ? VI_NU_U : VI_NU_V, fa[c], fw[c], fo[c], dt, fbc[c], ffill[c], ni, mf, mc, vnt);
    if (rc) return rc;
  }
  return XG_OK;
}

#ifdef XG_PRIMARY
// the exported entry (defined once, in the float64 build): the element type is an argument, dt and the fills are cast to it
// here, once
int xg_implicit_vertical_viscosity(int dtype, const void* u, const void* v, const void* nu, const int64_t* nu_strides,
                                   const void* mfu, const int64_t* mfu_strides, const void* mcu, const int64_t* mcu_strides,
                                   const void* mfv, const int64_t* mfv_strides, const void* mcv, const int64_t* mcv_strides,
                                   void* work_u, void* work_v, void* out_u, void* out_v, const int64_t* shape, int ndim,
                                   int outer, int bc_x, double fill_x, int bc_y, double fill_y, double dt, void* stream) {
  if (!(dt >= 0.0) || !__builtin_isfinite(dt))
    return fail(XG_ERR_INVALID, "implicit vertical viscosity: dt %g is negative or not finite", dt);
  const int64_t* const ms[4] = {mfu_strides, mcu_strides, mfv_strides, mcv_strides};
  if (dtype == XG_T_F64) {
    const double* const mp[4] = {(const double*)mfu, (const double*)mcu, (const double*)mfv, (const double*)mcv};
    return xg_internal_vvisc_f64((const double*)u, (const double*)v, (const double*)nu, nu_strides, mp, ms, (double*)work_u,
                                 (double*)work_v, (double*)out_u, (double*)out_v, shape, ndim, outer, bc_x, fill_x, bc_y,
                                 fill_y, dt, stream);
  }
  if (dtype == XG_T_F32) {
    const float* const mp[4] = {(const float*)mfu, (const float*)mcu, (const float*)mfv, (const float*)mcv};
    return xg_internal_vvisc_f32((const float*)u, (const float*)v, (const float*)nu, nu_strides, mp, ms, (float*)work_u,
                                 (float*)work_v, (float*)out_u, (float*)out_v, shape, ndim, outer, bc_x, (float)fill_x, bc_y,
                                 (float)fill_y, (float)dt, stream);
  }
  return fail(XG_ERR_INVALID, "implicit vertical viscosity: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
#endif

// The Richardson family's launcher, K7n and K7p: (lead, Z, Y, X) fields of `shape`, the results with nz (`outer`: nz + 1)
// faces, three optional broadcast metrics at the faces (the Z metric at u's points, at v's points, at the centre), one wave
// per column.  `mode` RI_MIX: b and both results required, `c` the closure's scalars.  Otherwise one result, and b NULL
// gives the squared shear alone (`mb` is not looked at).
static int richardson_family(int mode, const char* name, const real* b, const real* u, const real* v, const real* mu,
                             const int64_t* mu_strides, const real* mv, const int64_t* mv_strides, const real* mb,
                             const int64_t* mb_strides, const RimixScalars& c, real* out, real* out2, const int64_t* shape,
                             int ndim, int outer, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z, real fill_z,
                             void* stream) {
  if (!u || !v || !out || !shape || (mode == RI_MIX && (!b || !out2))) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {bc_x, bc_y, bc_z}, XG_BC_EXTEND))) return rc;
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  if (shape[ndim - 3] == 0) return fail(XG_ERR_INVALID, "%s: no level along Z", name);
  if (!b) mb = nullptr;
  if (mode != RI_MIX) mode = b ? RI_RI : RI_S2;
  FusedPlan p;
  const bool al = aligned16(u) && aligned16(v) && aligned16(b) && aligned16(out) && aligned16(out2);
  if ((rc = fused_plan(&p, name, shape, ndim, 3, al, true, stream)) || p.empty) return rc;
  VolIdx mi[3];  // the Z metric at u's points, at v's points, at the centre
  const real* mp[3] = {mu, mv, mb};
  const int64_t* ms[3] = {mu_strides, mv_strides, mb_strides};
  for (int k = 0; k < 3; ++k)
    if ((rc = vol_index(&mi[k], mp[k], ms[k], shape, ndim))) return rc;
  // bit 0: the lane neighbour by DPP (K7g), bits 2 / 3 / 4: the rows of the three metrics are aligned vectors
  int vnt = vec_nt_bits(1);
  for (int k = 0; k < 3; ++k)
    if (p.V > 1 && mi[k].p && mi[k].sz % NV == 0 && plane_vec_ok(mi[k].p, mi[k].ai, mi[k].sy, mi[k].sx)) vnt |= 4 << k;
  const bool met = mu != nullptr || mv != nullptr || mb != nullptr;
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, R_, M_, NTS) do { hipLaunchKernelGGL((k_richardson<V_, R_, M_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, b, u, v, out, out2, o0, nouter, nblk, p.nz, p.ny, p.nx, p.fnt, p.fns, outer, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, mi[0], mi[1], mi[2], vnt, c); } while (0)
#define XG_N(V_, R_, M_) do { if (p.nts) XG_GO(V_, R_, M_, true); else XG_GO(V_, R_, M_, false); } while (0)
#define XG_M(V_, R_) do { if (met) XG_N(V_, R_, true); else XG_N(V_, R_, false); } while (0)
#define XG_V(V_) do { if (mode == RI_MIX) XG_M(V_, RI_MIX); else if (mode == RI_RI) XG_M(V_, RI_RI); else XG_M(V_, RI_S2); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_M
#undef XG_N
#undef XG_GO
  });
}

// One ABI entry for both element types each (xg_richardson_number, xg_richardson_mixing, below).
__attribute__((visibility("hidden"))) int xg_internal_richardson_f64(
    const double* b, const double* u, const double* v, const double* mu, const int64_t* mu_strides, const double* mv,
    const int64_t* mv_strides, const double* mb, const int64_t* mb_strides, double* out, const int64_t* shape, int ndim,
    int outer, int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void* stream);
__attribute__((visibility("hidden"))) int xg_internal_richardson_f32(
    const float* b, const float* u, const float* v, const float* mu, const int64_t* mu_strides, const float* mv,
    const int64_t* mv_strides, const float* mb, const int64_t* mb_strides, float* out, const int64_t* shape, int ndim,
    int outer, int bc_x, float fill_x, int bc_y, float fill_y, int bc_z, float fill_z, void* stream);

int XG_FN(xg_internal_richardson)(const real* b, const real* u, const real* v, const real* mu, const int64_t* mu_strides,
                                  const real* mv, const int64_t* mv_strides, const real* mb, const int64_t* mb_strides,
                                  real* out, const int64_t* shape, int ndim, int outer, int bc_x, real fill_x, int bc_y,
                                  real fill_y, int bc_z, real fill_z, void* stream) {
  return richardson_family(RI_RI, "richardson number", b, u, v, mu, mu_strides, mv, mv_strides, mb, mb_strides,
                           RimixScalars{}, out, nullptr, shape, ndim, outer, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, stream);
}

#ifdef XG_PRIMARY
// the exported entry (defined once, in the float64 build): the element type is an argument, the fills are cast to it here
int xg_richardson_number(int dtype, const void* b, const void* u, const void* v, const void* mu, const int64_t* mu_strides,
                         const void* mv, const int64_t* mv_strides, const void* mb, const int64_t* mb_strides, void* out,
                         const int64_t* shape, int ndim, int outer, int bc_x, double fill_x, int bc_y, double fill_y, int bc_z,
                         double fill_z, void* stream) {
  if (dtype == XG_T_F64)
    return xg_internal_richardson_f64((const double*)b, (const double*)u, (const double*)v, (const double*)mu, mu_strides,
                                      (const double*)mv, mv_strides, (const double*)mb, mb_strides, (double*)out, shape, ndim,
                                      outer, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, stream);
  if (dtype == XG_T_F32)
    return xg_internal_richardson_f32((const float*)b, (const float*)u, (const float*)v, (const float*)mu, mu_strides,
                                      (const float*)mv, mv_strides, (const float*)mb, mb_strides, (float*)out, shape, ndim,
                                      outer, bc_x, (float)fill_x, bc_y, (float)fill_y, bc_z, (float)fill_z, stream);
  return fail(XG_ERR_INVALID, "richardson number: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
#endif

__attribute__((visibility("hidden"))) int xg_internal_rimix_f64(
    const double* b, const double* u, const double* v, const double* mu, const int64_t* mu_strides, const double* mv,
    const int64_t* mv_strides, const double* mb, const int64_t* mb_strides, double nu0, double alpha, double nu_b,
    double kappa_b, double shear_floor, double* out_nu, double* out_kappa, const int64_t* shape, int ndim, int outer,
    int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void* stream);
__attribute__((visibility("hidden"))) int xg_internal_rimix_f32(
    const float* b, const float* u, const float* v, const float* mu, const int64_t* mu_strides, const float* mv,
    const int64_t* mv_strides, const float* mb, const int64_t* mb_strides, float nu0, float alpha, float nu_b, float kappa_b,
    float shear_floor, float* out_nu, float* out_kappa, const int64_t* shape, int ndim, int outer, int bc_x, float fill_x,
    int bc_y, float fill_y, int bc_z, float fill_z, void* stream);

int XG_FN(xg_internal_rimix)(const real* b, const real* u, const real* v, const real* mu, const int64_t* mu_strides,
                             const real* mv, const int64_t* mv_strides, const real* mb, const int64_t* mb_strides, real nu0,
                             real alpha, real nu_b, real kappa_b, real shear_floor, real* out_nu, real* out_kappa,
                             const int64_t* shape, int ndim, int outer, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z,
                             real fill_z, void* stream) {
  return richardson_family(RI_MIX, "richardson mixing", b, u, v, mu, mu_strides, mv, mv_strides, mb, mb_strides,
                           RimixScalars{nu0, alpha, nu_b, kappa_b, shear_floor}, out_nu, out_kappa, shape, ndim, outer, bc_x,
                           fill_x, bc_y, fill_y, bc_z, fill_z, stream);
}

#ifdef XG_PRIMARY
// the exported entry (defined once, in the float64 build): the element type is an argument, the fills and the closure's
// scalars are cast to it here
int xg_richardson_mixing(int dtype, const void* b, const void* u, const void* v, const void* mu, const int64_t* mu_strides,
                         const void* mv, const int64_t* mv_strides, const void* mb, const int64_t* mb_strides, double nu0,
                         double alpha, double nu_b, double kappa_b, double shear_floor, void* out_nu, void* out_kappa,
                         const int64_t* shape, int ndim, int outer, int bc_x, double fill_x, int bc_y, double fill_y, int bc_z,
                         double fill_z, void* stream) {
  if (dtype == XG_T_F64)
    return xg_internal_rimix_f64((const double*)b, (const double*)u, (const double*)v, (const double*)mu, mu_strides,
                                 (const double*)mv, mv_strides, (const double*)mb, mb_strides, nu0, alpha, nu_b, kappa_b,
                                 shear_floor, (double*)out_nu, (double*)out_kappa, shape, ndim, outer, bc_x, fill_x, bc_y,
                                 fill_y, bc_z, fill_z, stream);
  if (dtype == XG_T_F32)
    return xg_internal_rimix_f32((const float*)b, (const float*)u, (const float*)v, (const float*)mu, mu_strides,
                                 (const float*)mv, mv_strides, (const float*)mb, mb_strides, (float)nu0, (float)alpha,
                                 (float)nu_b, (float)kappa_b, (float)shear_floor, (float*)out_nu, (float*)out_kappa, shape,
                                 ndim, outer, bc_x, (float)fill_x, bc_y, (float)fill_y, bc_z, (float)fill_z, stream);
  return fail(XG_ERR_INVALID, "richardson mixing: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
#endif

// The isopycnal family's launcher, K7q, K7r and K7s: a (lead, Z, Y, X) field of `shape`, three optional broadcast metrics
// (mx and my at the field's levels; the third at the faces, IS_FLUX: mc at the levels), one wave per column.  IS_SLOPE:
// out_x and out_y with nz (`outer`: nz + 1) faces.  IS_TENSOR: out_z too, and the tensor's scalars in `c` (already in
// `real`).  IS_FLUX: kwx and kwy at the faces, `closed`, and out_x, the one result, of `shape`.
static int isopycnal_family(int mode, const char* name, const real* b, const real* kwx, const real* kwy, const real* mx,
                            const int64_t* mx_strides, const real* my, const int64_t* my_strides, const real* mz,
                            const int64_t* mz_strides, const RediScalars& c, real* out_x, real* out_y, real* out_z,
                            const int64_t* shape, int ndim, int outer, int closed, int bc_x, real fill_x, int bc_y,
                            real fill_y, int bc_z, real fill_z, void* stream) {
  if (!b || !out_x || !shape || (mode == IS_FLUX ? (!kwx || !kwy) : !out_y) || (mode == IS_TENSOR && !out_z))
    return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {bc_x, bc_y, bc_z}, XG_BC_EXTEND))) return rc;
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  if (c.taper != 0 && c.taper != 1) return fail(XG_ERR_INVALID, "%s: taper %d is neither 0 nor 1", name, c.taper);
  if (closed != 0 && closed != 1) return fail(XG_ERR_INVALID, "%s: closed %d is neither 0 nor 1", name, closed);
  if (shape[ndim - 3] == 0) return fail(XG_ERR_INVALID, "%s: no level along Z", name);
  if (mode == IS_TENSOR) {  // the three results, (lead, nz + outer, ny, nx) each, may not overlap
    int64_t n = shape[ndim - 3] + outer;
    for (int d = 0; d < ndim; ++d)
      if (d != ndim - 3) n *= shape[d];
    const real* r[3] = {out_x, out_y, out_z};
    for (int i = 0; i < 3; ++i)
      for (int j = i + 1; j < 3; ++j)
        if (n > 0 && (uintptr_t)r[i] < (uintptr_t)(r[j] + n) && (uintptr_t)r[j] < (uintptr_t)(r[i] + n))
          return fail(XG_ERR_INVALID, "%s: the results overlap", name);
  }
  VolIdx mi[3];
  const real* mp[3] = {mx, my, mz};
  const int64_t* ms[3] = {mx_strides, my_strides, mz_strides};
  for (int k = 0; k < 3; ++k)
    if ((rc = vol_index(&mi[k], mp[k], ms[k], shape, ndim))) return rc;
  FusedPlan p;
  const bool al = aligned16(b) && aligned16(kwx) && aligned16(kwy) && aligned16(out_x) && aligned16(out_y) && aligned16(out_z);
  if ((rc = fused_plan(&p, name, shape, ndim, 3, al, true, stream)) || p.empty) return rc;
  // bit 0: the lane neighbours by DPP (K7c, K7g), bits 2 / 3 / 4: the rows of the three metrics are aligned vectors
  int vnt = vec_nt_bits(1);
  for (int k = 0; k < 3; ++k)
    if (p.V > 1 && mi[k].p && mi[k].sz % NV == 0 && plane_vec_ok(mi[k].p, mi[k].ai, mi[k].sy, mi[k].sx)) vnt |= 4 << k;
  const bool met = mx != nullptr || my != nullptr || mz != nullptr;
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, O_, M_, NTS) do { hipLaunchKernelGGL((k_islope<V_, O_, M_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, b, kwx, kwy, out_x, out_y, out_z, o0, nouter, nblk, p.nz, p.ny, p.nx, p.fnt, p.fns, outer, closed, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, mi[0], mi[1], mi[2], vnt, c); } while (0)
#define XG_N(V_, O_, M_) do { if (p.nts) XG_GO(V_, O_, M_, true); else XG_GO(V_, O_, M_, false); } while (0)
#define XG_M(V_, O_) do { if (met) XG_N(V_, O_, true); else XG_N(V_, O_, false); } while (0)
#define XG_V(V_) do { if (mode == IS_FLUX) XG_M(V_, IS_FLUX); else if (mode == IS_TENSOR) XG_M(V_, IS_TENSOR); else XG_M(V_, IS_SLOPE); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_M
#undef XG_N
#undef XG_GO
  });
}

// One ABI entry for both element types each (xg_isopycnal_slope, xg_redi_tensor, xg_redi_vertical_flux_divergence, below).
__attribute__((visibility("hidden"))) int xg_internal_islope_f64(
    const double* b, const double* mx, const int64_t* mx_strides, const double* my, const int64_t* my_strides,
    const double* mz, const int64_t* mz_strides, double* out_x, double* out_y, const int64_t* shape, int ndim, int outer,
    int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void* stream);
__attribute__((visibility("hidden"))) int xg_internal_islope_f32(
    const float* b, const float* mx, const int64_t* mx_strides, const float* my, const int64_t* my_strides, const float* mz,
    const int64_t* mz_strides, float* out_x, float* out_y, const int64_t* shape, int ndim, int outer, int bc_x, float fill_x,
    int bc_y, float fill_y, int bc_z, float fill_z, void* stream);

int XG_FN(xg_internal_islope)(const real* b, const real* mx, const int64_t* mx_strides, const real* my,
                              const int64_t* my_strides, const real* mz, const int64_t* mz_strides, real* out_x, real* out_y,
                              const int64_t* shape, int ndim, int outer, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z,
                              real fill_z, void* stream) {
  return isopycnal_family(IS_SLOPE, "isopycnal slope", b, nullptr, nullptr, mx, mx_strides, my, my_strides, mz, mz_strides,
                          RediScalars{}, out_x, out_y, nullptr, shape, ndim, outer, 0, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z,
                          stream);
}

#ifdef XG_PRIMARY
// the exported entry (defined once, in the float64 build): the element type is an argument, the fills are cast to it here
int xg_isopycnal_slope(int dtype, const void* b, const void* mx, const int64_t* mx_strides, const void* my,
                       const int64_t* my_strides, const void* mz, const int64_t* mz_strides, void* out_x, void* out_y,
                       const int64_t* shape, int ndim, int outer, int bc_x, double fill_x, int bc_y, double fill_y, int bc_z,
                       double fill_z, void* stream) {
  if (dtype == XG_T_F64)
    return xg_internal_islope_f64((const double*)b, (const double*)mx, mx_strides, (const double*)my, my_strides,
                                  (const double*)mz, mz_strides, (double*)out_x, (double*)out_y, shape, ndim, outer, bc_x,
                                  fill_x, bc_y, fill_y, bc_z, fill_z, stream);
  if (dtype == XG_T_F32)
    return xg_internal_islope_f32((const float*)b, (const float*)mx, mx_strides, (const float*)my, my_strides,
                                  (const float*)mz, mz_strides, (float*)out_x, (float*)out_y, shape, ndim, outer, bc_x,
                                  (float)fill_x, bc_y, (float)fill_y, bc_z, (float)fill_z, stream);
  return fail(XG_ERR_INVALID, "isopycnal slope: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
#endif

__attribute__((visibility("hidden"))) int xg_internal_reditensor_f64(
    const double* b, const double* mx, const int64_t* mx_strides, const double* my, const int64_t* my_strides,
    const double* mz, const int64_t* mz_strides, double kappa, double slope_max2, int taper, double* out_x, double* out_y,
    double* out_z, const int64_t* shape, int ndim, int outer, int bc_x, double fill_x, int bc_y, double fill_y, int bc_z,
    double fill_z, void* stream);
__attribute__((visibility("hidden"))) int xg_internal_reditensor_f32(
    const float* b, const float* mx, const int64_t* mx_strides, const float* my, const int64_t* my_strides, const float* mz,
    const int64_t* mz_strides, float kappa, float slope_max2, int taper, float* out_x, float* out_y, float* out_z,
    const int64_t* shape, int ndim, int outer, int bc_x, float fill_x, int bc_y, float fill_y, int bc_z, float fill_z,
    void* stream);

int XG_FN(xg_internal_reditensor)(const real* b, const real* mx, const int64_t* mx_strides, const real* my,
                                  const int64_t* my_strides, const real* mz, const int64_t* mz_strides, real kappa,
                                  real slope_max2, int taper, real* out_x, real* out_y, real* out_z, const int64_t* shape,
                                  int ndim, int outer, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z, real fill_z,
                                  void* stream) {
  return isopycnal_family(IS_TENSOR, "redi tensor", b, nullptr, nullptr, mx, mx_strides, my, my_strides, mz, mz_strides,
                          RediScalars{kappa, slope_max2, taper}, out_x, out_y, out_z, shape, ndim, outer, 0, bc_x, fill_x, bc_y,
                          fill_y, bc_z, fill_z, stream);
}

#ifdef XG_PRIMARY
// the exported entry (defined once, in the float64 build): the element type is an argument; the fills, kappa and
// slope_max2 are cast to it here, once
int xg_redi_tensor(int dtype, const void* b, const void* mx, const int64_t* mx_strides, const void* my,
                   const int64_t* my_strides, const void* mz, const int64_t* mz_strides, double kappa, double slope_max2,
                   int taper, void* out_x, void* out_y, void* out_z, const int64_t* shape, int ndim, int outer, int bc_x,
                   double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void* stream) {
  if (dtype == XG_T_F64)
    return xg_internal_reditensor_f64((const double*)b, (const double*)mx, mx_strides, (const double*)my, my_strides,
                                      (const double*)mz, mz_strides, kappa, slope_max2, taper, (double*)out_x, (double*)out_y,
                                      (double*)out_z, shape, ndim, outer, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, stream);
  if (dtype == XG_T_F32)
    return xg_internal_reditensor_f32((const float*)b, (const float*)mx, mx_strides, (const float*)my, my_strides,
                                      (const float*)mz, mz_strides, (float)kappa, (float)slope_max2, taper, (float*)out_x,
                                      (float*)out_y, (float*)out_z, shape, ndim, outer, bc_x, (float)fill_x, bc_y,
                                      (float)fill_y, bc_z, (float)fill_z, stream);
  return fail(XG_ERR_INVALID, "redi tensor: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
#endif

__attribute__((visibility("hidden"))) int xg_internal_rediflux_f64(
    const double* a, const double* kwx, const double* kwy, const double* mx, const int64_t* mx_strides, const double* my,
    const int64_t* my_strides, const double* mc, const int64_t* mc_strides, double* out, const int64_t* shape, int ndim,
    int outer, int closed, int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void* stream);
__attribute__((visibility("hidden"))) int xg_internal_rediflux_f32(
    const float* a, const float* kwx, const float* kwy, const float* mx, const int64_t* mx_strides, const float* my,
    const int64_t* my_strides, const float* mc, const int64_t* mc_strides, float* out, const int64_t* shape, int ndim, int outer,
    int closed, int bc_x, float fill_x, int bc_y, float fill_y, int bc_z, float fill_z, void* stream);

int XG_FN(xg_internal_rediflux)(const real* a, const real* kwx, const real* kwy, const real* mx, const int64_t* mx_strides,
                                const real* my, const int64_t* my_strides, const real* mc, const int64_t* mc_strides, real* out,
                                const int64_t* shape, int ndim, int outer, int closed, int bc_x, real fill_x, int bc_y,
                                real fill_y, int bc_z, real fill_z, void* stream) {
  return isopycnal_family(IS_FLUX, "redi vertical flux divergence", a, kwx, kwy, mx, mx_strides, my, my_strides, mc,
                          mc_strides, RediScalars{}, out, nullptr, nullptr, shape, ndim, outer, closed, bc_x, fill_x, bc_y,
                          fill_y, bc_z, fill_z, stream);
}

#ifdef XG_PRIMARY
// the exported entry (defined once, in the float64 build): the element type is an argument, the fills are cast to it here
int xg_redi_vertical_flux_divergence(int dtype, const void* a, const void* kwx, const void* kwy, const void* mx,
                                     const int64_t* mx_strides, const void* my, const int64_t* my_strides, const void* mc,
                                     const int64_t* mc_strides, void* out, const int64_t* shape, int ndim, int outer, int closed,
                                     int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void* stream) {
  if (dtype == XG_T_F64)
    return xg_internal_rediflux_f64((const double*)a, (const double*)kwx, (const double*)kwy, (const double*)mx, mx_strides,
                                    (const double*)my, my_strides, (const double*)mc, mc_strides, (double*)out, shape, ndim,
                                    outer, closed, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, stream);
  if (dtype == XG_T_F32)
    return xg_internal_rediflux_f32((const float*)a, (const float*)kwx, (const float*)kwy, (const float*)mx, mx_strides,
                                    (const float*)my, my_strides, (const float*)mc, mc_strides, (float*)out, shape, ndim, outer,
                                    closed, bc_x, (float)fill_x, bc_y, (float)fill_y, bc_z, (float)fill_z, stream);
  return fail(XG_ERR_INVALID, "redi vertical flux divergence: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
#endif

// K7t's launcher: kwx and kwy at the faces of `shape`'s levels (nz faces, `outer`: nz + 1), five optional broadcast metrics
// (met[]: mzu and mzv at the levels, dyG, dxG and rA at the faces), out_u and out_v of `shape`, out_w at the faces; one wave
// per column, the isopycnal family's plan
static int bolus_impl(const real* kwx, const real* kwy, const real* const met[5], const int64_t* const ms[5], real* out_u,
                      real* out_v, real* out_w, const int64_t* shape, int ndim, int outer, int closed, int bc_x, real fill_x,
                      int bc_y, real fill_y, int bc_z, real fill_z, void* stream) {
  const char* name = "bolus velocity";
  if (!kwx || !kwy || !out_u || !out_v || !out_w || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {bc_x, bc_y, bc_z}, XG_BC_EXTEND))) return rc;
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  if (closed != 0 && closed != 1) return fail(XG_ERR_INVALID, "%s: closed %d is neither 0 nor 1", name, closed);
  if (shape[ndim - 3] < 1) return fail(XG_ERR_INVALID, "%s: no level along Z", name);
  VolIdx mi[5];
  for (int k = 0; k < 5; ++k)
    if ((rc = vol_index(&mi[k], met[k], ms[k], shape, ndim))) return rc;
  FusedPlan p;
  const bool al = aligned16(kwx) && aligned16(kwy) && aligned16(out_u) && aligned16(out_v) && aligned16(out_w);
  if ((rc = fused_plan(&p, name, shape, ndim, 3, al, true, stream)) || p.empty) return rc;
  // bit 0: the lane neighbours by DPP, bits 2 .. 6: the rows of dyG, dxG, rA, mzu, mzv are aligned vectors
  static const int bit_of[5] = {32, 64, 4, 8, 16};
  int vnt = vec_nt_bits(1);
  bool any = false;
  for (int k = 0; k < 5; ++k) {
    any = any || mi[k].p != nullptr;
    if (p.V > 1 && mi[k].p && mi[k].sz % NV == 0 && plane_vec_ok(mi[k].p, mi[k].ai, mi[k].sy, mi[k].sx)) vnt |= bit_of[k];
  }
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, M_, NTS) do { hipLaunchKernelGGL((k_bolus<V_, M_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, kwx, kwy, out_u, out_v, out_w, o0, nouter, nblk, p.nz, p.ny, p.nx, p.fnt, p.fns, outer, closed, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, mi[0], mi[1], mi[2], mi[3], mi[4], vnt); } while (0)
#define XG_N(V_, M_) do { if (p.nts) XG_GO(V_, M_, true); else XG_GO(V_, M_, false); } while (0)
#define XG_V(V_) do { if (any) XG_N(V_, true); else XG_N(V_, false); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_N
#undef XG_GO
  });
}

// One ABI entry for both element types (xg_bolus_velocity, below).
__attribute__((visibility("hidden"))) int xg_internal_bolus_f64(
    const double* kwx, const double* kwy, const double* const met[5], const int64_t* const ms[5], double* out_u, double* out_v,
    double* out_w, const int64_t* shape, int ndim, int outer, int closed, int bc_x, double fill_x, int bc_y, double fill_y,
    int bc_z, double fill_z, void* stream);
__attribute__((visibility("hidden"))) int xg_internal_bolus_f32(
    const float* kwx, const float* kwy, const float* const met[5], const int64_t* const ms[5], float* out_u, float* out_v,
    float* out_w, const int64_t* shape, int ndim, int outer, int closed, int bc_x, float fill_x, int bc_y, float fill_y, int bc_z,
    float fill_z, void* stream);

int XG_FN(xg_internal_bolus)(const real* kwx, const real* kwy, const real* const met[5], const int64_t* const ms[5], real* out_u,
                             real* out_v, real* out_w, const int64_t* shape, int ndim, int outer, int closed, int bc_x,
                             real fill_x, int bc_y, real fill_y, int bc_z, real fill_z, void* stream) {
  return bolus_impl(kwx, kwy, met, ms, out_u, out_v, out_w, shape, ndim, outer, closed, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z,
                    stream);
}

#ifdef XG_PRIMARY
// the exported entry (defined once, in the float64 build): the element type is an argument, the fills are cast to it here
int xg_bolus_velocity(int dtype, const void* kwx, const void* kwy, const void* mzu, const int64_t* mzu_strides, const void* mzv,
                      const int64_t* mzv_strides, const void* dyG, const int64_t* dyG_strides, const void* dxG,
                      const int64_t* dxG_strides, const void* rA, const int64_t* rA_strides, void* out_u, void* out_v,
                      void* out_w, const int64_t* shape, int ndim, int outer, int closed, int bc_x, double fill_x, int bc_y,
                      double fill_y, int bc_z, double fill_z, void* stream) {
  const int64_t* const ms[5] = {mzu_strides, mzv_strides, dyG_strides, dxG_strides, rA_strides};
  if (dtype == XG_T_F64) {
    const double* const met[5] = {(const double*)mzu, (const double*)mzv, (const double*)dyG, (const double*)dxG, (const double*)rA};
    return xg_internal_bolus_f64((const double*)kwx, (const double*)kwy, met, ms, (double*)out_u, (double*)out_v, (double*)out_w,
                                 shape, ndim, outer, closed, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, stream);
  }
  if (dtype == XG_T_F32) {
    const float* const met[5] = {(const float*)mzu, (const float*)mzv, (const float*)dyG, (const float*)dxG, (const float*)rA};
    return xg_internal_bolus_f32((const float*)kwx, (const float*)kwy, met, ms, (float*)out_u, (float*)out_v, (float*)out_w, shape,
                                 ndim, outer, closed, bc_x, (float)fill_x, bc_y, (float)fill_y, bc_z, (float)fill_z, stream);
  }
  return fail(XG_ERR_INVALID, "bolus velocity: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
#endif

// K7u's launcher: a (lead, Z, Y, X) field of `shape`, xg_redi_tensor's three optional broadcast metrics (mx and my at the
// field's levels, mz at the faces) and scalars (already in `real`), out_u and out_v of `shape`; one wave per column, the
// isopycnal family's plan.  The refusals are xg_redi_tensor's.
static int rediuv_impl(const real* b, const real* mx, const int64_t* mx_strides, const real* my, const int64_t* my_strides,
                       const real* mz, const int64_t* mz_strides, const RediScalars& c, real* out_u, real* out_v,
                       const int64_t* shape, int ndim, int outer, int bc_x, real fill_x, int bc_y, real fill_y, int bc_z,
                       real fill_z, void* stream) {
  const char* name = "redi horizontal tensor";
  if (!b || !out_u || !out_v || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  int rc;
  if ((rc = fused_dims(name, ndim, 3, {bc_x, bc_y, bc_z}, XG_BC_EXTEND))) return rc;
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  if (c.taper != 0 && c.taper != 1) return fail(XG_ERR_INVALID, "%s: taper %d is neither 0 nor 1", name, c.taper);
  if (shape[ndim - 3] == 0) return fail(XG_ERR_INVALID, "%s: no level along Z", name);
  int64_t n = 1;  // the two results, `shape` each, may not overlap
  for (int d = 0; d < ndim; ++d) n *= shape[d];
  if (n > 0 && (uintptr_t)out_u < (uintptr_t)(out_v + n) && (uintptr_t)out_v < (uintptr_t)(out_u + n))
    return fail(XG_ERR_INVALID, "%s: the results overlap", name);
  VolIdx mi[3];
  const real* mp[3] = {mx, my, mz};
  const int64_t* ms[3] = {mx_strides, my_strides, mz_strides};
  for (int k = 0; k < 3; ++k)
    if ((rc = vol_index(&mi[k], mp[k], ms[k], shape, ndim))) return rc;
  FusedPlan p;
  const bool al = aligned16(b) && aligned16(out_u) && aligned16(out_v);
  if ((rc = fused_plan(&p, name, shape, ndim, 3, al, true, stream)) || p.empty) return rc;
  const int vnt = vec_nt_bits(1);  // bit 0: the lane neighbours by DPP (the metrics are read element by element)
  const bool met = mx != nullptr || my != nullptr || mz != nullptr;
  return fused_launch(p, [&](int64_t o0, u32 nouter, u32 nblk, u32 grid) {
#define XG_GO(V_, M_, NTS) do { hipLaunchKernelGGL((k_rediuv<V_, M_, NTS, FSEG>), dim3(grid), dim3(BLOCK), 0, p.st, b, out_u, out_v, o0, nouter, nblk, p.nz, p.ny, p.nx, p.fnt, p.fns, outer, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, mi[0], mi[1], mi[2], vnt, c); } while (0)
#define XG_N(V_, M_) do { if (p.nts) XG_GO(V_, M_, true); else XG_GO(V_, M_, false); } while (0)
#define XG_V(V_) do { if (met) XG_N(V_, true); else XG_N(V_, false); } while (0)
    if (p.V > 1) XG_V(NV);
    else XG_V(1);
#undef XG_V
#undef XG_N
#undef XG_GO
  });
}

// One ABI entry for both element types (xg_redi_horizontal_tensor, below).
__attribute__((visibility("hidden"))) int xg_internal_rediuv_f64(
    const double* b, const double* mx, const int64_t* mx_strides, const double* my, const int64_t* my_strides,
    const double* mz, const int64_t* mz_strides, double kappa, double slope_max2, int taper, double* out_u, double* out_v,
    const int64_t* shape, int ndim, int outer, int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z,
    void* stream);
__attribute__((visibility("hidden"))) int xg_internal_rediuv_f32(
    const float* b, const float* mx, const int64_t* mx_strides, const float* my, const int64_t* my_strides, const float* mz,
    const int64_t* mz_strides, float kappa, float slope_max2, int taper, float* out_u, float* out_v, const int64_t* shape,
    int ndim, int outer, int bc_x, float fill_x, int bc_y, float fill_y, int bc_z, float fill_z, void* stream);

int XG_FN(xg_internal_rediuv)(const real* b, const real* mx, const int64_t* mx_strides, const real* my,
                              const int64_t* my_strides, const real* mz, const int64_t* mz_strides, real kappa,
                              real slope_max2, int taper, real* out_u, real* out_v, const int64_t* shape, int ndim, int outer,
                              int bc_x, real fill_x, int bc_y, real fill_y, int bc_z, real fill_z, void* stream) {
  return rediuv_impl(b, mx, mx_strides, my, my_strides, mz, mz_strides, RediScalars{kappa, slope_max2, taper}, out_u, out_v,
                     shape, ndim, outer, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, stream);
}

#ifdef XG_PRIMARY
// the exported entry (defined once, in the float64 build): the element type is an argument; the fills, kappa and
// slope_max2 are cast to it here, once
int xg_redi_horizontal_tensor(int dtype, const void* b, const void* mx, const int64_t* mx_strides, const void* my,
                              const int64_t* my_strides, const void* mz, const int64_t* mz_strides, double kappa,
                              double slope_max2, int taper, void* out_u, void* out_v, const int64_t* shape, int ndim, int outer,
                              int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void* stream) {
  if (dtype == XG_T_F64)
    return xg_internal_rediuv_f64((const double*)b, (const double*)mx, mx_strides, (const double*)my, my_strides,
                                  (const double*)mz, mz_strides, kappa, slope_max2, taper, (double*)out_u, (double*)out_v,
                                  shape, ndim, outer, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, stream);
  if (dtype == XG_T_F32)
    return xg_internal_rediuv_f32((const float*)b, (const float*)mx, mx_strides, (const float*)my, my_strides,
                                  (const float*)mz, mz_strides, (float)kappa, (float)slope_max2, taper, (float*)out_u,
                                  (float*)out_v, shape, ndim, outer, bc_x, (float)fill_x, bc_y, (float)fill_y, bc_z,
                                  (float)fill_z, stream);
  return fail(XG_ERR_INVALID, "redi horizontal tensor: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
#endif

#endif  // !XG_INT

}  // extern "C"
