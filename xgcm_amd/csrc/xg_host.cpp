// xg_host.cpp -- HOST build of the C ABI of include/xgcm_hip.h: the same `extern "C"` symbols over HOST pointers,
// compiled with g++ into libxgcm_host.so ("CPU build of the ABI" for BASELINE
// config 1, "plumbing, no GPU").
//
// What it is for: an integrator without a GPU can load a library with the exact symbol table of libxgcm_hip.so and
// exercise a binding end to end (argument marshalling, shapes, strides, error paths) on small arrays.  What it is
// NOT: a fallback.  xgcm_amd never loads it -- `xgcm_amd._hip.load()` opens libxgcm_hip.so only and the device
// layer raises without a GPU; the only users are tests/ (tests/host_abi_device.py) and examples/.  It has its own
// straightforward loops (one output cell at a time, index arithmetic in the open), written against the header's
// semantics, not against the kernels or the oracle.  It serves the 1-D operators of SURVEY.md section 8(a):
// stencil (+ pre-gathered halos), cumsum, reduce, pad, the broadcasting binary op and the synthetic generator, plus the
// fused divergence / vorticity / flux divergence (2-D and 3-D) / vertical velocity / laplacian / kinetic energy / momentum
// advection / horizontal viscosity; the other fused / topology / transform entry points exist
// and return XG_ERR_UNSUPPORTED.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off  (no FMA contraction: same bit contract as the kernels)

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/xgcm_hip.h"

namespace {

thread_local char g_err[512] = {0};

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int unsupported(const char* what) {
  return fail(XG_ERR_UNSUPPORTED, "%s: not part of the host build of the ABI (1-D operators only)", what);
}

// a C-contiguous N-D array seen as (outer, n, inner) around `axis`
struct View {
  int64_t outer = 1, n = 1, inner = 1;
};
int make_view(const int64_t* shape, int ndim, int axis, View* v) {
  if (!shape) return fail(XG_ERR_INVALID, "NULL shape");
  if (ndim < 1 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [1,%d]", ndim, XG_MAX_NDIM);
  if (axis < 0 || axis >= ndim) return fail(XG_ERR_INVALID, "axis %d out of range for ndim %d", axis, ndim);
  for (int d = 0; d < ndim; ++d)
    if (shape[d] < 0) return fail(XG_ERR_INVALID, "negative extent");
  v->n = shape[axis];
  for (int d = 0; d < axis; ++d) v->outer *= shape[d];
  for (int d = axis + 1; d < ndim; ++d) v->inner *= shape[d];
  return XG_OK;
}

// offset of the cell (o, k, x) of the (outer, n', inner) view in an array addressed by per-dim element strides
// (0 = broadcast) -- the metric convention of the header
int64_t strided_offset(const int64_t* shape, const int64_t* strides, int ndim, int axis, int64_t o, int64_t k, int64_t x) {
  int64_t off = k * strides[axis];
  for (int d = ndim - 1; d > axis; --d) {
    off += (x % shape[d]) * strides[d];
    x /= shape[d];
  }
  for (int d = axis - 1; d >= 0; --d) {
    off += (o % shape[d]) * strides[d];
    o /= shape[d];
  }
  return off;
}

template <typename R>
R op2(int op, R l, R r) {
  switch (op) {
    case XG_OP_DIFF: return r - l;
    case XG_OP_INTERP:
      if constexpr (std::is_integral_v<R>) return l + r;  // _i64: the wrapped sum, halved by the caller in float64
      else return (l + r) / R(2);
    case XG_OP_MIN: return (l != l || r != r) ? (l != l ? l : r) : (l < r ? l : r);  // NaN-propagating like np.min
    case XG_OP_MINU:  // integer entry points: the lanes hold an unsigned array
      if constexpr (std::is_integral_v<R>) return std::make_unsigned_t<R>(l) < std::make_unsigned_t<R>(r) ? l : r;
      else return l;
    case XG_OP_MAXU:
      if constexpr (std::is_integral_v<R>) return std::make_unsigned_t<R>(l) > std::make_unsigned_t<R>(r) ? l : r;
      else return l;
    default: return (l != l || r != r) ? (l != l ? l : r) : (l > r ? l : r);
  }
}

// P[q] of the header: the padded, m_in-weighted input at padded index q along the axis (halo: pre-gathered values)
template <typename R>
int stencil1d(int op, const R* in, const R* halo, R* out, const int64_t* shape, int ndim, int axis, int64_t n_out,
              int pad_lo, int pad_hi, int bc, R fill, const R* m_in, const int64_t* mis, const R* m_out,
              const int64_t* mos) {
  if (!in || !out) return fail(XG_ERR_INVALID, "NULL array argument");
  if (op < XG_OP_DIFF || op > (std::is_integral_v<R> ? XG_OP_MAXU : XG_OP_MAX)) return fail(XG_ERR_INVALID, "unknown op %d", op);
  if ((pad_lo | pad_hi) & ~1) return fail(XG_ERR_INVALID, "pad widths must be 0 or 1, got (%d,%d)", pad_lo, pad_hi);
  if (bc < XG_BC_NONE || bc > XG_BC_HALO) return fail(XG_ERR_INVALID, "unknown boundary mode %d", bc);
  if ((m_in && !mis) || (m_out && !mos)) return fail(XG_ERR_INVALID, "metric without strides");
  if (std::is_integral_v<R> && (m_in || m_out)) return fail(XG_ERR_UNSUPPORTED, "integer stencils take no metrics: convert to float64 first");
  View v;
  if (int rc = make_view(shape, ndim, axis, &v)) return rc;
  if (n_out != v.n + pad_lo + pad_hi - 1)
    return fail(XG_ERR_INVALID, "n_out %lld != n_in %lld + %d + %d - 1", (long long)n_out, (long long)v.n, pad_lo, pad_hi);
  if ((pad_lo || pad_hi) && bc == XG_BC_NONE) return fail(XG_ERR_INVALID, "halo cells requested but no boundary mode given");
  if (v.n < 1) return fail(XG_ERR_INVALID, "empty stencil axis");
  std::vector<int64_t> oshape(shape, shape + ndim);
  oshape[axis] = n_out;
  const int nhalo = pad_lo + pad_hi;
  for (int64_t o = 0; o < v.outer; ++o)
    for (int64_t j = 0; j < n_out; ++j)
      for (int64_t x = 0; x < v.inner; ++x) {
        R side[2];
        for (int s = 0; s < 2; ++s) {
          int64_t q = j + s - pad_lo;  // index into the unpadded input
          if (q >= 0 && q < v.n) {
            R val = in[(o * v.n + q) * v.inner + x];
            if (m_in) val = val * m_in[strided_offset(shape, mis, ndim, axis, o, q, x)];
            side[s] = val;
          } else if (bc == XG_BC_FILL) {
            side[s] = fill;  // the fill halo is not weighted: the reference pads after the product
          } else if (bc == XG_BC_HALO) {
            side[s] = halo[(o * nhalo + (q < 0 ? 0 : pad_lo)) * v.inner + x];
          } else {
            const int64_t src = (bc == XG_BC_PERIODIC) ? (q < 0 ? v.n - 1 : 0) : (q < 0 ? 0 : v.n - 1);
            R val = in[(o * v.n + src) * v.inner + x];
            if (m_in) val = val * m_in[strided_offset(shape, mis, ndim, axis, o, src, x)];
            side[s] = val;
          }
        }
        R res = op2<R>(op, side[0], side[1]);
        if (m_out) res = res / m_out[strided_offset(oshape.data(), mos, ndim, axis, o, j, x)];
        out[(o * n_out + j) * v.inner + x] = res;
      }
  return XG_OK;
}

template <typename R>
int cumsum1d(const R* in, R* out, const int64_t* shape, int ndim, int axis, int reverse, int skipna, int trim_lo,
             int trim_hi, int pad_lo, int pad_hi, int bc, R fill, const R* m_in, const int64_t* mis, const R* m_out,
             const int64_t* mos) {
  if (!in || !out) return fail(XG_ERR_INVALID, "NULL array argument");
  if ((trim_lo | trim_hi | pad_lo | pad_hi) & ~1) return fail(XG_ERR_INVALID, "trim/pad widths must be 0 or 1");
  if (bc < XG_BC_NONE || bc > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "unknown boundary mode %d", bc);
  if ((pad_lo || pad_hi) && bc == XG_BC_NONE) return fail(XG_ERR_INVALID, "halo cells requested but no boundary mode given");
  if ((m_in && !mis) || (m_out && !mos)) return fail(XG_ERR_INVALID, "metric without strides");
  if (std::is_integral_v<R> && (m_in || m_out)) return fail(XG_ERR_UNSUPPORTED, "integer scans take no metrics: convert to float64 first");
  View v;
  if (int rc = make_view(shape, ndim, axis, &v)) return rc;
  const int64_t kept = v.n - trim_lo - trim_hi;
  if (kept < 1) return fail(XG_ERR_INVALID, "nothing left after trimming (n=%lld)", (long long)v.n);
  const int64_t n_out = kept + pad_lo + pad_hi;
  std::vector<int64_t> oshape(shape, shape + ndim);
  oshape[axis] = n_out;
  std::vector<R> c(v.n);
  for (int64_t o = 0; o < v.outer; ++o)
    for (int64_t x = 0; x < v.inner; ++x) {
      R acc = 0;
      for (int64_t t = 0; t < v.n; ++t) {  // sequential in scan order, like numpy.cumsum / nancumsum
        const int64_t k = reverse ? v.n - 1 - t : t;
        R val = in[(o * v.n + k) * v.inner + x];
        if (m_in) val = val * m_in[strided_offset(shape, mis, ndim, axis, o, k, x)];
        if (skipna && val != val) val = 0;
        acc = (t == 0) ? val : acc + val;
        c[k] = acc;
      }
      for (int64_t j = 0; j < n_out; ++j) {  // pad acts on the trimmed CUMULATIVE values
        const int64_t t = j - pad_lo;        // index into the trimmed result
        R val;
        if (t >= 0 && t < kept) val = c[trim_lo + t];
        else if (bc == XG_BC_FILL) val = fill;
        else if (bc == XG_BC_PERIODIC) val = c[trim_lo + (t < 0 ? kept - 1 : 0)];
        else val = c[trim_lo + (t < 0 ? 0 : kept - 1)];
        if (m_out) val = val / m_out[strided_offset(oshape.data(), mos, ndim, axis, o, j, x)];
        out[(o * n_out + j) * v.inner + x] = val;
      }
    }
  return XG_OK;
}

template <typename R>
int reduce1d(const R* in, R* out, const int64_t* shape, int ndim, int axis, int skipna, const R* w, const int64_t* ws) {
  if (!in || !out) return fail(XG_ERR_INVALID, "NULL array argument");
  if (w && !ws) return fail(XG_ERR_INVALID, "weight without strides");
  if (skipna < 0 || skipna > 7) return fail(XG_ERR_INVALID, "skipna / count / mean mode %d not in [0,7]", skipna);
  if (std::is_integral_v<R> && (w || skipna > 1)) return fail(XG_ERR_UNSUPPORTED, "integer reductions are plain sums: weights and means are float");
  View v;
  if (int rc = make_view(shape, ndim, axis, &v)) return rc;
  // one sequential sum per output cell in the given mode (k = 0 .. n-1 in order: numpy's order over a non-last axis)
  auto sum_in_mode = [&](int64_t o, int64_t x, int mode) -> R {
    R acc = 0;
    for (int64_t k = 0; k < v.n; ++k) {
      R val = in[(o * v.n + k) * v.inner + x];
      if (mode >= 2) val = (mode == 3 || val == val) ? R(1) : R(0);
      if (w) val = val * w[strided_offset(shape, ws, ndim, axis, o, k, x)];
      if (mode && val != val) val = 0;
      acc = (k == 0) ? val : acc + val;
    }
    return acc;
  };
  for (int64_t o = 0; o < v.outer; ++o)
    for (int64_t x = 0; x < v.inner; ++x) {
      R res;
      if (skipna == 4) res = sum_in_mode(o, x, 1) / sum_in_mode(o, x, 2);       // NaN-skipping weighted mean
      else if (skipna == 5) res = sum_in_mode(o, x, 0) / sum_in_mode(o, x, 3);  // weighted mean, NaN propagates
      else if (skipna >= 6) {  // numerator and denominator sums side by side
        res = sum_in_mode(o, x, skipna == 6 ? 1 : 0);
        out[(v.outer + o) * v.inner + x] = sum_in_mode(o, x, skipna == 6 ? 2 : 3);
      } else res = sum_in_mode(o, x, skipna);
      out[o * v.inner + x] = res;
    }
  return XG_OK;
}

template <typename R>
int pad_nd(const R* in, R* out, const int64_t* shape, int ndim, const int64_t* lo, const int64_t* hi, const int* bc,
           const R* fill, const int* order) {
  if (!in || !out || !shape || !lo || !hi || !bc) return fail(XG_ERR_INVALID, "NULL argument");
  if (ndim < 1 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [1,%d]", ndim, XG_MAX_NDIM);
  // one axis at a time in application order, each step a fresh array (numpy.pad chain semantics)
  std::vector<int64_t> cur(shape, shape + ndim);
  int64_t total = 1;
  for (int d = 0; d < ndim; ++d) total *= cur[d];
  std::vector<R> a(in, in + total), b;
  for (int step = 0; step < ndim; ++step) {
    const int ax = order ? order[step] : step;
    if (ax < 0 || ax >= ndim) return fail(XG_ERR_INVALID, "bad axis %d in order", ax);
    if (lo[ax] == 0 && hi[ax] == 0) continue;
    if (lo[ax] < 0 || hi[ax] < 0) return fail(XG_ERR_INVALID, "negative pad width");
    if (bc[ax] < XG_BC_PERIODIC || bc[ax] > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "axis %d is padded but has no boundary mode", ax);
    View v;
    if (int rc = make_view(cur.data(), ndim, ax, &v)) return rc;
    if (v.n == 0 && bc[ax] != XG_BC_FILL) return fail(XG_ERR_INVALID, "can't extend empty axis %d using modes other than 'constant'", ax);
    const int64_t n2 = v.n + lo[ax] + hi[ax];
    b.assign((size_t)(v.outer * n2 * v.inner), R(0));
    for (int64_t o = 0; o < v.outer; ++o)
      for (int64_t j = 0; j < n2; ++j) {
        int64_t q = j - lo[ax];
        bool constant = false;
        if (q < 0 || q >= v.n) {
          if (bc[ax] == XG_BC_FILL) constant = true;
          else if (bc[ax] == XG_BC_PERIODIC) q = ((q % v.n) + v.n) % v.n;  // numpy 'wrap'
          else q = q < 0 ? 0 : v.n - 1;                                    // numpy 'edge'
        }
        for (int64_t x = 0; x < v.inner; ++x)
          b[(size_t)((o * n2 + j) * v.inner + x)] = constant ? (fill ? fill[ax] : R(0)) : a[(size_t)((o * v.n + q) * v.inner + x)];
      }
    a.swap(b);
    cur[ax] = n2;
  }
  int64_t n_out = 1;
  for (int d = 0; d < ndim; ++d) n_out *= cur[d];
  if (n_out) memcpy(out, a.data(), sizeof(R) * (size_t)n_out);
  return XG_OK;
}

template <typename R>
int binary(int op, const R* a, const int64_t* sa, const R* b, const int64_t* sb, R* out, const int64_t* shape, int ndim) {
  if (!a || !b || !out || !shape || !sa || !sb) return fail(XG_ERR_INVALID, "NULL argument");
  if (op < XG_BIN_MUL || op > XG_BIN_SUB) return fail(XG_ERR_INVALID, "unknown binary op %d", op);
  if (std::is_integral_v<R> && op == XG_BIN_DIV) return fail(XG_ERR_UNSUPPORTED, "true division leaves the integer domain: convert to float64 first");
  if (ndim < 1 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [1,%d]", ndim, XG_MAX_NDIM);
  int64_t total = 1;
  for (int d = 0; d < ndim; ++d) total *= shape[d];
  for (int64_t i = 0; i < total; ++i) {
    int64_t r = i, oa = 0, ob = 0;
    for (int d = ndim - 1; d >= 0; --d) {
      const int64_t c = r % shape[d];
      r /= shape[d];
      oa += c * sa[d];
      ob += c * sb[d];
    }
    const R x = a[oa], y = b[ob];
    if constexpr (std::is_integral_v<R>) out[i] = op == XG_BIN_MUL ? x * y : op == XG_BIN_ADD ? x + y : x - y;
    else out[i] = op == XG_BIN_MUL ? x * y : op == XG_BIN_DIV ? x / y : op == XG_BIN_ADD ? x + y : x - y;
  }
  return XG_OK;
}

template <typename R>
int fill_synthetic(R* out, int64_t n, uint64_t seed, uint64_t offset, double scale, double shift) {
  if (!out && n > 0) return fail(XG_ERR_INVALID, "NULL output");
  for (int64_t i = 0; i < n; ++i) {
    uint64_t z = (uint64_t)i + offset + seed * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    const double u = (double)(z >> 11) * 0x1.0p-53;
    out[i] = (R)(u * scale + shift);
  }
  return XG_OK;
}

// tunables: the names of the device library (xg_runtime.hip::TUNABLES), accepted and remembered so that bindings
// can be exercised; they have no effect on the host loops
const char* const KNOWN_TUNABLES[] = {"seg", "nt_store", "nt_load", "seg_max_tiles", "scan_narrow_below", "pad_rows", "pad_nt", "transform_lds_kb", "transform_win", "transform_fast", "transform_stage", "transform_ring", "transform_cwin", "transform_lean", "zchunk", "zband", "zb_rows", "scan_block", "strided_gen", "march_band", "scan_vec", "scan_dpp", "contig_gen", "deep_waves", "contig_rw", "rw_zshare", "met_zk", "met_zk1", "vec_zk", "vec_nt", "vec_zb_rows", "nb_dpp", "met_zk2", "met_ys", "met_ys1", "met_ys2", "seg_ys", "contig_rw_mi", "met_seg", "met_seg1", "met_scalar", "scan_pipe", "scan_u", "scan_pace", "scan_chain", "scan_chain_w", "scan_chain_spin", "scan_chain_tmaj", "reduce_zl", "pad_tpw", "bin_idx32", "reduce_ldsw_u", "march_ofast", "reduce_sk", "reduce_ru", "reduce_wfast", "reduce_wg", "scan_sh1", "reduce_ldsw", "reduce_zmarch", "dbg", "march_lds_kb"};
struct Knob { const char* name; int value; bool set; };
std::vector<Knob>& knobs() {
  static std::vector<Knob> k;
  if (k.empty())
    for (const char* n : KNOWN_TUNABLES) k.push_back({n, 0, false});
  return k;
}

// fused vorticity / divergence of the header (docs/ufunc_examples.md): the operator chain's arithmetic cell by cell --
// (dx - dy) / area resp. (dx + dy) / area with the two one-cell halos from bc_x / bc_y -- so that the host build serves the
// config-5 workload of bench.py's CPU dry run (tests/test_bench_dryrun.py); shapes (.., Y, X), area through broadcast strides
template <typename R>
int curl_or_div(bool curl, const R* u, const R* v, const R* area, const int64_t* as, R* out, const int64_t* shape, int ndim,
                int bc_x, R fill_x, int bc_y, R fill_y) {
  if (!u || !v || !out || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 2 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [2,%d]", ndim, XG_MAX_NDIM);
  if (area && !as) return fail(XG_ERR_INVALID, "metric without strides");
  for (int b : {bc_x, bc_y})
    if (b < XG_BC_PERIODIC || b > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "boundary mode %d: periodic, fill or extend", b);
  const int64_t ny = shape[ndim - 2], nx = shape[ndim - 1];
  int64_t outer = 1;
  for (int d = 0; d < ndim - 2; ++d) outer *= shape[d];
  if (outer == 0 || ny == 0 || nx == 0) return XG_OK;
  // neighbour along one axis: index k + s (s = -1 for the curl's center->left, +1 for the divergence's left->center)
  auto nb = [](const R* row, int64_t k, int64_t n, int64_t stride, int s, int bc, R fill) -> R {
    const int64_t q = k + s;
    if (q >= 0 && q < n) return row[q * stride];
    if (bc == XG_BC_FILL) return fill;
    if (bc == XG_BC_PERIODIC) return row[((q % n + n) % n) * stride];
    return row[(q < 0 ? 0 : n - 1) * stride];
  };
  for (int64_t o = 0; o < outer; ++o) {
    int64_t rem = o, aoff = 0;  // the outer index decomposed for the area's broadcast strides
    for (int d = ndim - 3; d >= 0; --d) { const int64_t i = rem % shape[d]; rem /= shape[d]; if (area) aoff += i * as[d]; }
    const R *pu = u + o * ny * nx, *pv = v + o * ny * nx;
    R* po = out + o * ny * nx;
    for (int64_t j = 0; j < ny; ++j)
      for (int64_t i = 0; i < nx; ++i) {
        R r;
        if (curl) {
          const R dvdx = pv[j * nx + i] - nb(pv + j * nx, i, nx, 1, -1, bc_x, fill_x);
          const R dudy = pu[j * nx + i] - nb(pu + i, j, ny, nx, -1, bc_y, fill_y);
          r = dvdx - dudy;
        } else {
          const R dudx = nb(pu + j * nx, i, nx, 1, +1, bc_x, fill_x) - pu[j * nx + i];
          const R dvdy = nb(pv + i, j, ny, nx, +1, bc_y, fill_y) - pv[j * nx + i];
          r = dudx + dvdy;
        }
        po[j * nx + i] = area ? r / area[aoff + j * as[ndim - 2] + i * as[ndim - 1]] : r;
      }
  }
  return XG_OK;
}


// fused second-order operators of the header: the two stages of the chain one after the other, plane by plane -- the
// staggered intermediate Fx / Fy formed with T's halo (center -> left), then the divergence with the intermediate's own halo
// (left -> center); mode 1: Fx = u * (T[i-1] + T[i]) / 2 (and along Y), mode 0: Fx = (T[i] - T[i-1]) / dxC * dyG,
// Fy = (T[j] - T[j-1]) / dyC * dxG (met[] = {dxC, dyG, dyC, dxG}, all four or none)
template <typename R>
int div2d(int mode, const R* t, const R* u, const R* v, const R* const met[4], const int64_t* const ms[4], const R* area,
          const int64_t* as, R* out, const int64_t* shape, int ndim, int bc_x, R fill_x, int bc_y, R fill_y) {
  if (!t || !out || !shape || (mode == 1 && (!u || !v))) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 2 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [2,%d]", ndim, XG_MAX_NDIM);
  if (area && !as) return fail(XG_ERR_INVALID, "metric without strides");
  for (int b : {bc_x, bc_y})
    if (b < XG_BC_PERIODIC || b > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "boundary mode %d: periodic, fill or extend", b);
  int nmet = 0;
  for (int k = 0; met && k < 4; ++k) {
    if (!met[k]) continue;
    if (!ms[k]) return fail(XG_ERR_INVALID, "metric without strides");
    ++nmet;
  }
  if (nmet != 0 && nmet != 4) return fail(XG_ERR_INVALID, "laplacian: the four metrics dxC, dyC, dyG, dxG, or none");
  const int64_t ny = shape[ndim - 2], nx = shape[ndim - 1];
  int64_t outer = 1;
  for (int d = 0; d < ndim - 2; ++d) outer *= shape[d];
  if (outer == 0 || ny == 0 || nx == 0) return XG_OK;
  auto wrap = [](int64_t q, int64_t n, int bc) { return bc == XG_BC_PERIODIC ? ((q % n + n) % n) : (q < 0 ? 0 : n - 1); };
  std::vector<R> fx((size_t)(ny * nx)), fy((size_t)(ny * nx));
  for (int64_t o = 0; o < outer; ++o) {
    int64_t rem = o, aoff = 0, moff[4] = {0, 0, 0, 0};  // the outer index decomposed for the broadcast strides
    for (int d = ndim - 3; d >= 0; --d) {
      const int64_t i = rem % shape[d];
      rem /= shape[d];
      if (area) aoff += i * as[d];
      for (int k = 0; k < 4; ++k)
        if (nmet) moff[k] += i * ms[k][d];
    }
    auto m = [&](int k, int64_t j, int64_t i) { return met[k][moff[k] + j * ms[k][ndim - 2] + i * ms[k][ndim - 1]]; };
    const R* pt = t + o * ny * nx;
    for (int64_t j = 0; j < ny; ++j)
      for (int64_t i = 0; i < nx; ++i) {
        const R c = pt[j * nx + i];
        const R l = i > 0 ? pt[j * nx + i - 1] : (bc_x == XG_BC_FILL ? fill_x : pt[j * nx + wrap(-1, nx, bc_x)]);
        const R b = j > 0 ? pt[(j - 1) * nx + i] : (bc_y == XG_BC_FILL ? fill_y : pt[wrap(-1, ny, bc_y) * nx + i]);
        const int64_t k = o * ny * nx + j * nx + i;
        if (mode == 1) {
          fx[j * nx + i] = u[k] * ((l + c) / R(2));
          fy[j * nx + i] = v[k] * ((b + c) / R(2));
        } else if (nmet) {
          R gx = (c - l) / m(0, j, i), gy = (c - b) / m(2, j, i);
          fx[j * nx + i] = gx * m(1, j, i);
          fy[j * nx + i] = gy * m(3, j, i);
        } else {
          fx[j * nx + i] = c - l;
          fy[j * nx + i] = c - b;
        }
      }
    R* po = out + o * ny * nx;
    for (int64_t j = 0; j < ny; ++j)
      for (int64_t i = 0; i < nx; ++i) {
        const R fr = i + 1 < nx ? fx[j * nx + i + 1] : (bc_x == XG_BC_FILL ? fill_x : fx[j * nx + wrap(nx, nx, bc_x)]);
        const R fu = j + 1 < ny ? fy[(j + 1) * nx + i] : (bc_y == XG_BC_FILL ? fill_y : fy[wrap(ny, ny, bc_y) * nx + i]);
        const R r = (fr - fx[j * nx + i]) + (fu - fy[j * nx + i]);
        po[j * nx + i] = area ? r / area[aoff + j * as[ndim - 2] + i * as[ndim - 1]] : r;
      }
  }
  return XG_OK;
}

// the 3-D flux divergence of the header: the horizontal part per level as div2d (mode 1, no area), then the vertical flux
// Fz[k] = w[k] * (T[k-1] + T[k]) / 2 with T's halo above level 0, its difference Fz[k+1] - Fz[k] with Fz's own halo below
// the last level, added to it, then the division by vol (* vol2)
template <typename R>
int div3d(const R* u, const R* v, const R* w, const R* t, const R* vol, const int64_t* vs, const R* vol2,
          const int64_t* vs2, R* out, const int64_t* shape, int ndim, int bc_x, R fill_x, int bc_y, R fill_y, int bc_z,
          R fill_z) {
  if (!u || !v || !w || !t || !out || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [3,%d]", ndim, XG_MAX_NDIM);
  if (bc_z < XG_BC_PERIODIC || bc_z > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "boundary mode %d: periodic, fill or extend", bc_z);
  if (vol2 && !vol) return fail(XG_ERR_INVALID, "a second volume factor without the first");
  if ((vol && !vs) || (vol2 && !vs2)) return fail(XG_ERR_INVALID, "metric without strides");
  int rc = div2d<R>(1, t, u, v, nullptr, nullptr, nullptr, nullptr, out, shape, ndim, bc_x, fill_x, bc_y, fill_y);
  if (rc) return rc;
  const int64_t nz = shape[ndim - 3], plane = shape[ndim - 2] * shape[ndim - 1];
  int64_t outer = 1;
  for (int d = 0; d < ndim - 3; ++d) outer *= shape[d];
  if (outer == 0 || nz == 0 || plane == 0) return XG_OK;
  std::vector<R> fz((size_t)(nz * plane));
  for (int64_t o = 0; o < outer; ++o) {
    const int64_t col = o * nz * plane;
    for (int64_t k = 0; k < nz; ++k)
      for (int64_t p = 0; p < plane; ++p) {
        const R c = t[col + k * plane + p];
        const R a = k > 0 ? t[col + (k - 1) * plane + p]
                          : (bc_z == XG_BC_FILL ? fill_z : t[col + (bc_z == XG_BC_PERIODIC ? nz - 1 : 0) * plane + p]);
        fz[k * plane + p] = w[col + k * plane + p] * ((a + c) / R(2));
      }
    for (int64_t k = 0; k < nz; ++k)
      for (int64_t p = 0; p < plane; ++p) {
        const R below = k + 1 < nz ? fz[(k + 1) * plane + p]
                                   : (bc_z == XG_BC_FILL ? fill_z : fz[(bc_z == XG_BC_PERIODIC ? 0 : nz - 1) * plane + p]);
        R& r = out[col + k * plane + p];
        r = r + (below - fz[k * plane + p]);
        if (vol) {
          // the cell's multi-index, for the broadcast strides of the volume factor(s)
          int64_t rem = col + k * plane + p, off = 0, off2 = 0;
          for (int d = ndim - 1; d >= 0; --d) {
            const int64_t i = rem % shape[d];
            rem /= shape[d];
            off += i * vs[d];
            if (vol2) off2 += i * vs2[d];
          }
          r = r / (vol2 ? vol[off] * vol2[off2] : vol[off]);
        }
      }
  }
  return XG_OK;
}


// the vertical velocity of the header: per lead index, the weighted transports of a level, their divergence, the running
// nan-sum along Z (upward with the pad at level 0, or downward), then the negation and the division by the area
template <typename R>
int wcont(const R* u, const R* v, const R* const met[5], const int64_t* const ms[5], R* out, const int64_t* shape, int ndim,
          int bc_x, R fill_x, int bc_y, R fill_y, int bc_z, R fill_z, int reverse) {
  if (!u || !v || !out || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [3,%d]", ndim, XG_MAX_NDIM);
  for (int b : {bc_x, bc_y})
    if (b < XG_BC_PERIODIC || b > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "boundary mode %d: periodic, fill or extend", b);
  if (!reverse && bc_z != XG_BC_FILL && bc_z != XG_BC_EXTEND)
    return fail(XG_ERR_UNSUPPORTED, "vertical velocity summed upward pads Z with fill or extend");
  if ((met[0] != nullptr) != (met[2] != nullptr)) return fail(XG_ERR_INVALID, "face weights for both u and v, or for neither");
  if ((met[1] && !met[0]) || (met[3] && !met[2])) return fail(XG_ERR_INVALID, "a second face-weight factor without the first");
  for (int k = 0; k < 5; ++k)
    if (met[k] && !ms[k]) return fail(XG_ERR_INVALID, "metric without strides");
  for (int k : {1, 3})
    if (met[k] && (ms[k][ndim - 2] != 0 || ms[k][ndim - 1] != 0))
      return fail(XG_ERR_UNSUPPORTED, "the second face-weight factor varies along Z (and leading dims) only");
  const int64_t nz = shape[ndim - 3], ny = shape[ndim - 2], nx = shape[ndim - 1], plane = ny * nx;
  int64_t outer = 1;
  for (int d = 0; d < ndim - 3; ++d) outer *= shape[d];
  if (outer == 0 || nz == 0 || plane == 0) return XG_OK;
  auto wrap = [](int64_t q, int64_t n, int bc) { return bc == XG_BC_PERIODIC ? ((q % n + n) % n) : (q < 0 ? 0 : n - 1); };
  std::vector<R> tu((size_t)plane), tv((size_t)plane), acc((size_t)plane);
  for (int64_t o = 0; o < outer; ++o) {
    int64_t rem = o, moff[5] = {0, 0, 0, 0, 0};  // the lead index decomposed for the broadcast strides
    for (int d = ndim - 4; d >= 0; --d) {
      const int64_t i = rem % shape[d];
      rem /= shape[d];
      for (int k = 0; k < 5; ++k)
        if (met[k]) moff[k] += i * ms[k][d];
    }
    auto m = [&](int k, int64_t z, int64_t j, int64_t i) {
      return met[k][moff[k] + z * ms[k][ndim - 3] + j * ms[k][ndim - 2] + i * ms[k][ndim - 1]];
    };
    auto put = [&](int64_t z, int64_t p, R c) {
      const R neg = R(-1) * c;
      out[(o * nz + z) * plane + p] = met[4] ? neg / m(4, z, p / nx, p % nx) : neg;
    };
    if (!reverse && bc_z == XG_BC_FILL)
      for (int64_t p = 0; p < plane; ++p) put(0, p, fill_z);
    const int64_t n = reverse ? nz : (nz > 1 ? nz - 1 : (bc_z == XG_BC_EXTEND ? 1 : 0));  // the last level is trimmed
    for (int64_t t = 0; t < n; ++t) {
      const int64_t z = reverse ? nz - 1 - t : t;
      const R* pu = u + (o * nz + z) * plane;
      const R* pv = v + (o * nz + z) * plane;
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          R a = pu[j * nx + i], b = pv[j * nx + i];
          if (met[0]) a = a * (met[1] ? m(0, z, j, i) * m(1, z, j, i) : m(0, z, j, i));
          if (met[2]) b = b * (met[3] ? m(2, z, j, i) * m(3, z, j, i) : m(2, z, j, i));
          tu[j * nx + i] = a;
          tv[j * nx + i] = b;
        }
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t p = j * nx + i;
          const R ur = i + 1 < nx ? tu[p + 1] : (bc_x == XG_BC_FILL ? fill_x : tu[j * nx + wrap(nx, nx, bc_x)]);
          const R vu = j + 1 < ny ? tv[p + nx] : (bc_y == XG_BC_FILL ? fill_y : tv[wrap(ny, ny, bc_y) * nx + i]);
          R d = (ur - tu[p]) + (vu - tv[p]);
          if (d != d) d = R(0);
          acc[p] = t == 0 ? d : acc[p] + d;
          if (reverse) {
            put(z, p, acc[p]);
          } else {
            if (t == 0 && bc_z == XG_BC_EXTEND) put(0, p, acc[p]);
            if (z + 1 < nz) put(z + 1, p, acc[p]);
          }
        }
    }
  }
  return XG_OK;
}

// the hydrostatic pressure gradient of the header, stage by stage over one (Z, Y, X) volume at a time: the pressure at the
// nz + 1 interfaces, its mean at the cell centres, then the two differences of that field with their own pads.
// met[] = {Z weight, dxC, dyC}
template <typename R>
int pgrad(const R* b, const R* const met[3], const int64_t* const ms[3], R* out_x, R* out_y, const int64_t* shape, int ndim,
          int bc_x, R fill_x, int bc_y, R fill_y, int bc_z, R fill_z) {
  if (!b || !out_x || !out_y || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [3,%d]", ndim, XG_MAX_NDIM);
  for (int c : {bc_x, bc_y, bc_z})
    if (c < XG_BC_PERIODIC || c > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "boundary mode %d: periodic, fill or extend", c);
  if (bc_z != XG_BC_FILL && bc_z != XG_BC_EXTEND)
    return fail(XG_ERR_UNSUPPORTED, "hydrostatic pressure gradient pads Z with fill or extend");
  for (int k = 0; k < 3; ++k)
    if (met[k] && !ms[k]) return fail(XG_ERR_INVALID, "metric without strides");
  const int64_t nz = shape[ndim - 3], ny = shape[ndim - 2], nx = shape[ndim - 1], plane = ny * nx;
  int64_t outer = 1;
  for (int d = 0; d < ndim - 3; ++d) outer *= shape[d];
  if (outer == 0 || nz == 0 || plane == 0) return XG_OK;
  std::vector<R> p((size_t)((nz + 1) * plane)), pc((size_t)(nz * plane));
  for (int64_t o = 0; o < outer; ++o) {
    int64_t rem = o, moff[3] = {0, 0, 0};  // the lead index decomposed for the broadcast strides
    for (int d = ndim - 4; d >= 0; --d) {
      const int64_t i = rem % shape[d];
      rem /= shape[d];
      for (int k = 0; k < 3; ++k)
        if (met[k]) moff[k] += i * ms[k][d];
    }
    auto m = [&](int k, int64_t z, int64_t j, int64_t i) {
      return met[k][moff[k] + z * ms[k][ndim - 3] + j * ms[k][ndim - 2] + i * ms[k][ndim - 1]];
    };
    const R* pb = b + o * nz * plane;
    // (1) the interfaces: p[z + 1] = the nan-sum of b * w through level z, p[0] the pad
    for (int64_t z = 0; z < nz; ++z)
      for (int64_t c = 0; c < plane; ++c) {
        R t = met[0] ? pb[z * plane + c] * m(0, z, c / nx, c % nx) : pb[z * plane + c];
        if (t != t) t = R(0);
        p[(z + 1) * plane + c] = z == 0 ? t : p[z * plane + c] + t;
      }
    for (int64_t c = 0; c < plane; ++c) p[c] = bc_z == XG_BC_FILL ? fill_z : p[plane + c];
    // (2) the centres
    for (int64_t z = 0; z < nz; ++z)
      for (int64_t c = 0; c < plane; ++c) pc[z * plane + c] = (p[z * plane + c] + p[(z + 1) * plane + c]) / R(2);
    // (3) the differences towards the left points
    for (int64_t z = 0; z < nz; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const R* q = pc.data() + z * plane;
          const R here = q[j * nx + i];
          const R left = i > 0 ? q[j * nx + i - 1]
                               : (bc_x == XG_BC_FILL ? fill_x : q[j * nx + (bc_x == XG_BC_PERIODIC ? nx - 1 : 0)]);
          const R below = j > 0 ? q[(j - 1) * nx + i]
                                : (bc_y == XG_BC_FILL ? fill_y : q[(bc_y == XG_BC_PERIODIC ? ny - 1 : 0) * nx + i]);
          R gx = here - left, gy = here - below;
          if (met[1]) gx = gx / m(1, z, j, i);
          if (met[2]) gy = gy / m(2, z, j, i);
          out_x[(o * nz + z) * plane + j * nx + i] = gx;
          out_y[(o * nz + z) * plane + j * nx + i] = gy;
        }
  }
  return XG_OK;
}

// the vertical advection of horizontal momentum of the header as five plain passes over one (Z, Y, X) volume at a time:
// w at u's and v's columns, the Z differences of u and v, the products, their means at the centre, the sign and the metrics.
// Each pass pads its own axis by one cell through `padded`.
// met[] = {the metric of out_u, of out_v}
template <typename R>
int vmomadv(const R* u, const R* v, const R* w, const R* const met[2], const int64_t* const ms[2], R* out_u, R* out_v,
            const int64_t* shape, int ndim, int bc_x, R fill_x, int bc_y, R fill_y, int bc_z, R fill_z) {
  if (!u || !v || !w || !out_u || !out_v || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [3,%d]", ndim, XG_MAX_NDIM);
  for (int c : {bc_x, bc_y, bc_z})
    if (c < XG_BC_PERIODIC || c > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "boundary mode %d: periodic, fill or extend", c);
  for (int k = 0; k < 2; ++k)
    if (met[k] && !ms[k]) return fail(XG_ERR_INVALID, "metric without strides");
  const int64_t nz = shape[ndim - 3], ny = shape[ndim - 2], nx = shape[ndim - 1], plane = ny * nx, vol = nz * plane;
  int64_t outer = 1;
  for (int d = 0; d < ndim - 3; ++d) outer *= shape[d];
  if (outer == 0 || vol == 0) return XG_OK;
  // the padded index of a one-axis read: a cell of the axis, or -1 for "the fill value"
  auto padded = [](int64_t i, int64_t n, int bc) -> int64_t {
    if (i >= 0 && i < n) return i;
    if (bc == XG_BC_FILL) return -1;
    if (bc == XG_BC_PERIODIC) return i < 0 ? n - 1 : 0;
    return i < 0 ? 0 : n - 1;
  };
  std::vector<R> wu((size_t)vol), wv((size_t)vol), du((size_t)vol), dv((size_t)vol);
  R* const out[2] = {out_u, out_v};
  for (int64_t o = 0; o < outer; ++o) {
    int64_t rem = o, moff[2] = {0, 0};  // the lead index decomposed for the broadcast strides
    for (int d = ndim - 4; d >= 0; --d) {
      const int64_t i = rem % shape[d];
      rem /= shape[d];
      for (int k = 0; k < 2; ++k)
        if (met[k]) moff[k] += i * ms[k][d];
    }
    const R *pu = u + o * vol, *pv = v + o * vol, *pw = w + o * vol;
    // (1) w between a cell and the one left of it / below it: (w[i-1] + w[i]) / 2, (w[j-1] + w[j]) / 2
    for (int64_t z = 0; z < nz; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t c = z * plane + j * nx + i, il = padded(i - 1, nx, bc_x), jb = padded(j - 1, ny, bc_y);
          const R left = il < 0 ? fill_x : pw[z * plane + j * nx + il];
          const R below = jb < 0 ? fill_y : pw[z * plane + jb * nx + i];
          wu[c] = (left + pw[c]) / R(2);
          wv[c] = (below + pw[c]) / R(2);
        }
    // (2) u and v minus the level above them
    for (int64_t z = 0; z < nz; ++z) {
      const int64_t za = padded(z - 1, nz, bc_z);
      for (int64_t c = 0; c < plane; ++c) {
        du[z * plane + c] = pu[z * plane + c] - (za < 0 ? fill_z : pu[za * plane + c]);
        dv[z * plane + c] = pv[z * plane + c] - (za < 0 ? fill_z : pv[za * plane + c]);
      }
    }
    // (3) the products, in place
    for (int64_t c = 0; c < vol; ++c) {
      wu[c] = wu[c] * du[c];
      wv[c] = wv[c] * dv[c];
    }
    // (4) their means at the centre: level z and the level after it, (5) the sign and the metric
    for (int which = 0; which < 2; ++which) {
      const std::vector<R>& p = which ? wv : wu;
      for (int64_t z = 0; z < nz; ++z) {
        const int64_t zn = padded(z + 1, nz, bc_z);
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = j * nx + i;
            R g = -((p[z * plane + c] + (zn < 0 ? fill_z : p[zn * plane + c])) / R(2));
            if (met[which])
              g = g / met[which][moff[which] + z * ms[which][ndim - 3] + j * ms[which][ndim - 2] + i * ms[which][ndim - 1]];
            out[which][o * vol + z * plane + c] = g;
          }
      }
    }
  }
  return XG_OK;
}

// the vertical diffusion of the header as the three passes of its chain over one (Z, Y, X) volume at a time, each into a
// temporary: the difference of `a` to the level above at the flux levels (nz of them, `outer`: nz + 1) over the flux'
// metric, the product with kappa, the difference of the flux to the next level's over the result's metric.
// arr[] = {kappa, the metric of the flux, the metric of the result}
template <typename R>
int vdiff(const R* a, const R* const arr[3], const int64_t* const st[3], R* out, const int64_t* shape, int ndim, int outer,
          int bc_z, R fill_z) {
  if (!a || !out || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [3,%d]", ndim, XG_MAX_NDIM);
  if (bc_z < XG_BC_PERIODIC || bc_z > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "boundary mode %d: periodic, fill or extend", bc_z);
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "outer %d is neither 0 (left) nor 1", outer);
  for (int k = 0; k < 3; ++k)
    if (arr[k] && !st[k]) return fail(XG_ERR_INVALID, "metric without strides");
  const int64_t nz = shape[ndim - 3], ny = shape[ndim - 2], nx = shape[ndim - 1], plane = ny * nx, vol = nz * plane;
  const int64_t nf = nz + outer;  // flux levels
  int64_t lead = 1;
  for (int d = 0; d < ndim - 3; ++d) lead *= shape[d];
  if (lead == 0 || vol == 0) return XG_OK;
  std::vector<R> g((size_t)(nf * plane)), f((size_t)(nf * plane));
  for (int64_t o = 0; o < lead; ++o) {
    int64_t rem = o, off[3] = {0, 0, 0};  // the lead index decomposed for the broadcast strides
    for (int d = ndim - 4; d >= 0; --d) {
      const int64_t i = rem % shape[d];
      rem /= shape[d];
      for (int k = 0; k < 3; ++k)
        if (arr[k]) off[k] += i * st[k][d];
    }
    auto at = [&](int k, int64_t z, int64_t j, int64_t i) -> R {
      return arr[k][off[k] + z * st[k][ndim - 3] + j * st[k][ndim - 2] + i * st[k][ndim - 1]];
    };
    const R* pa = a + o * vol;
    // level z of the padded field: a level of `a`, or its pad above level 0 / below level nz - 1
    auto level = [&](int64_t z, int64_t c) -> R {
      if (z >= 0 && z < nz) return pa[z * plane + c];
      if (bc_z == XG_BC_FILL) return fill_z;
      if (bc_z == XG_BC_PERIODIC) return pa[(z < 0 ? nz - 1 : 0) * plane + c];
      return pa[(z < 0 ? 0 : nz - 1) * plane + c];
    };
    // (1) the gradient at the flux levels
    for (int64_t z = 0; z < nf; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t c = j * nx + i;
          R d = level(z, c) - level(z - 1, c);
          if (arr[1]) d = d / at(1, z, j, i);
          g[z * plane + c] = d;
        }
    // (2) the flux
    for (int64_t z = 0; z < nf; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t c = z * plane + j * nx + i;
          f[c] = arr[0] ? g[c] * at(0, z, j, i) : g[c];
        }
    // (3) its difference to the next level's; `left` pads the flux beyond its last level
    for (int64_t z = 0; z < nz; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t c = j * nx + i;
          R next;
          if (z + 1 < nf) next = f[(z + 1) * plane + c];
          else if (bc_z == XG_BC_FILL) next = fill_z;
          else next = f[((bc_z == XG_BC_PERIODIC) ? 0 : nz - 1) * plane + c];
          R d = next - f[z * plane + c];
          if (arr[2]) d = d / at(2, z, j, i);
          out[o * vol + z * plane + c] = d;
        }
  }
  return XG_OK;
}

// the implicit vertical diffusion of the header, level by level over one (Z, Y, X) volume at a time: the Thomas algorithm with
// every cell of a level advanced before the next level is touched.  c goes into `work`, d into `out`; the backward loop
// turns d into x.  arr[] = {kappa, the metric of the flux, the metric of the result}; faces 0 and nz are never read.
// `nb_axis` 0 (X) / 1 (Y): the implicit vertical viscosity of the header for one component -- kappa is the mean of arr[0] and
// its neighbour left of / below the cell, (neighbour + value) * 0.5, the neighbour of column / row 0 padded by `bc` / `fill`.
template <typename R>
int vimpl(const R* a, const R* const arr[3], const int64_t* const st[3], R* work, R* out, const int64_t* shape, int ndim,
          int outer, R dt, int nb_axis = -1, int bc = XG_BC_EXTEND, R fill = 0) {
  if (!a || !out || !work || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [3,%d]", ndim, XG_MAX_NDIM);
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "outer %d is neither 0 (left) nor 1", outer);
  for (int k = 0; k < 3; ++k)
    if (arr[k] && !st[k]) return fail(XG_ERR_INVALID, "a plane without strides");
  const int64_t nz = shape[ndim - 3], ny = shape[ndim - 2], nx = shape[ndim - 1], plane = ny * nx, vol = nz * plane;
  int64_t lead = 1;
  for (int d = 0; d < ndim - 3; ++d) lead *= shape[d];
  if (lead == 0 || vol == 0) return XG_OK;
  const R one = R(1);
  for (int64_t o = 0; o < lead; ++o) {
    int64_t rem = o, off[3] = {0, 0, 0};  // the lead index decomposed for the broadcast strides
    for (int d = ndim - 4; d >= 0; --d) {
      const int64_t i = rem % shape[d];
      rem /= shape[d];
      for (int k = 0; k < 3; ++k)
        if (arr[k]) off[k] += i * st[k][d];
    }
    auto at = [&](int k, int64_t z, int64_t j, int64_t i) -> R {
      return arr[k][off[k] + z * st[k][ndim - 3] + j * st[k][ndim - 2] + i * st[k][ndim - 1]];
    };
    // dt * kappa / mf at face z (1 .. nz-1)
    auto weight = [&](int64_t z, int64_t j, int64_t i) -> R {
      R g = arr[0] ? at(0, z, j, i) : one;
      if (nb_axis >= 0) {
        const int64_t q = nb_axis == 0 ? i : j, n = nb_axis == 0 ? nx : ny;
        const int64_t src = q > 0 ? q - 1 : (bc == XG_BC_PERIODIC ? n - 1 : 0);
        const R nb = (q == 0 && bc == XG_BC_FILL) ? fill : (nb_axis == 0 ? at(0, z, j, src) : at(0, z, src, i));
        g = (nb + g) * R(0.5);
      }
      if (arr[1]) g = g / at(1, z, j, i);
      return dt * g;
    };
    const R* pa = a + o * vol;
    R* pc = work + o * vol;
    R* pd = out + o * vol;
    for (int64_t z = 0; z < nz; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t c = z * plane + j * nx + i;
          R b = one, lo = 0, up = 0;
          if (z > 0) {
            lo = weight(z, j, i);
            if (arr[2]) lo = lo / at(2, z, j, i);
            b = b + lo;
          }
          if (z + 1 < nz) {
            up = weight(z + 1, j, i);
            if (arr[2]) up = up / at(2, z, j, i);
            b = b + up;
          }
          R m = b, d = pa[c];
          if (z > 0) {
            m = m - lo * pc[c - plane];
            d = d + lo * pd[c - plane];
          }
          const R r = one / m;
          if (z + 1 < nz) pc[c] = up * r;
          pd[c] = d * r;
        }
    for (int64_t z = nz - 2; z >= 0; --z)
      for (int64_t c = z * plane; c < (z + 1) * plane; ++c) pd[c] = pd[c] + pc[c] * pd[c + plane];
  }
  return XG_OK;
}

// the implicit vertical viscosity of the header: `vimpl` for u with nu averaged along X and for v with nu averaged along Y
template <typename R>
int vvisc(const R* u, const R* v, const R* nu, const int64_t* nus, const void* const met[4], const int64_t* const ms[4], R* work_u,
          R* work_v, R* out_u, R* out_v, const int64_t* shape, int ndim, int outer, int bc_x, R fill_x, int bc_y, R fill_y, R dt) {
  if (!u || !v || !nu || !out_u || !out_v || !work_u || !work_v || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [3,%d]", ndim, XG_MAX_NDIM);
  for (int b : {bc_x, bc_y})
    if (b < XG_BC_PERIODIC || b > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "boundary mode %d: periodic, fill or extend", b);
  const R* const au[3] = {nu, (const R*)met[0], (const R*)met[1]};
  const R* const av[3] = {nu, (const R*)met[2], (const R*)met[3]};
  const int64_t* const su[3] = {nus, ms[0], ms[1]};
  const int64_t* const sv[3] = {nus, ms[2], ms[3]};
  for (int k = 0; k < 3; ++k)
    if ((au[k] && !su[k]) || (av[k] && !sv[k])) return fail(XG_ERR_INVALID, "a plane without strides");
  const int rc = vimpl<R>(u, au, su, work_u, out_u, shape, ndim, outer, dt, 0, bc_x, fill_x);
  return rc ? rc : vimpl<R>(v, av, sv, work_v, out_v, shape, ndim, outer, dt, 1, bc_y, fill_y);
}

// the squared shear / the Richardson number of the header as the stages of its chain over one (Z, Y, X) volume at a time,
// each into a temporary: the three differences along Z at the faces (nz of them, `outer`: nz + 1) over their metrics, the
// two means to the centre with the pad of the DIFFERENCES right of the last column / above the last row, the squares,
// their sum, the quotient.  arr[] = {the metric at u's points, at v's points, at the centre}; b NULL: the squared shear.
// `clo` = {nu0, alpha, nu_b, kappa_b, shear_floor}: the Pacanowski-Philander closure on that quotient as its own stages, nu
// into `out` and kappa into `out_kappa` (xg_richardson_mixing)
template <typename R>
int richardson(const R* b, const R* u, const R* v, const R* const arr_in[3], const int64_t* const st[3], R* out,
               const int64_t* shape, int ndim, int outer, const int bc[3], const R fill[3],  // bc, fill: X, Y, Z
               const R* clo = nullptr, R* out_kappa = nullptr) {
  const char* name = clo ? "richardson mixing" : "richardson number";
  if (!u || !v || !out || !shape || (clo && (!b || !out_kappa))) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "%s: ndim %d not in [3,%d]", name, ndim, XG_MAX_NDIM);
  for (int k = 0; k < 3; ++k)
    if (bc[k] < XG_BC_PERIODIC || bc[k] > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "%s: boundary mode %d: periodic, fill or extend", name, bc[k]);
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  const R* arr[3] = {arr_in[0], arr_in[1], b ? arr_in[2] : nullptr};
  for (int k = 0; k < 3; ++k)
    if (arr[k] && !st[k]) return fail(XG_ERR_INVALID, "%s: metric without strides", name);
  const int64_t nz = shape[ndim - 3], ny = shape[ndim - 2], nx = shape[ndim - 1], plane = ny * nx, vol = nz * plane;
  if (nz == 0) return fail(XG_ERR_INVALID, "%s: no level along Z", name);
  const int64_t nf = nz + outer;  // faces
  int64_t lead = 1;
  for (int d = 0; d < ndim - 3; ++d) lead *= shape[d];
  if (lead == 0 || vol == 0) return XG_OK;
  std::vector<R> d[3];  // the differences of u, v, b at the faces
  for (int k = 0; k < (b ? 3 : 2); ++k) d[k].resize((size_t)(nf * plane));
  std::vector<R> uz((size_t)(nf * plane)), vz((size_t)(nf * plane));
  for (int64_t o = 0; o < lead; ++o) {
    int64_t rem = o, off[3] = {0, 0, 0};  // the lead index decomposed for the broadcast strides
    for (int dd = ndim - 4; dd >= 0; --dd) {
      const int64_t i = rem % shape[dd];
      rem /= shape[dd];
      for (int k = 0; k < 3; ++k)
        if (arr[k]) off[k] += i * st[k][dd];
    }
    const R* src[3] = {u + o * vol, v + o * vol, b ? b + o * vol : nullptr};
    // (1) the differences along Z: level z of a padded field is a level of it, or its pad above level 0 / below level nz-1
    for (int k = 0; k < 3; ++k) {
      if (!src[k]) continue;
      const R* p = src[k];
      auto level = [&](int64_t z, int64_t c) -> R {
        if (z >= 0 && z < nz) return p[z * plane + c];
        if (bc[2] == XG_BC_FILL) return fill[2];
        if (bc[2] == XG_BC_PERIODIC) return p[(z < 0 ? nz - 1 : 0) * plane + c];
        return p[(z < 0 ? 0 : nz - 1) * plane + c];
      };
      for (int64_t z = 0; z < nf; ++z)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = j * nx + i;
            R x = level(z, c) - level(z - 1, c);
            if (arr[k]) x = x / arr[k][off[k] + z * st[k][ndim - 3] + j * st[k][ndim - 2] + i * st[k][ndim - 1]];
            d[k][z * plane + c] = x;
          }
    }
    // (2) the means at the centre: du with its right neighbour, dv with the one above
    for (int64_t z = 0; z < nf; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t c = z * plane + j * nx + i;
          R right, above;
          if (i + 1 < nx) right = d[0][c + 1];
          else if (bc[0] == XG_BC_FILL) right = fill[0];
          else right = d[0][z * plane + j * nx + (bc[0] == XG_BC_PERIODIC ? 0 : nx - 1)];
          if (j + 1 < ny) above = d[1][c + nx];
          else if (bc[1] == XG_BC_FILL) above = fill[1];
          else above = d[1][z * plane + (bc[1] == XG_BC_PERIODIC ? 0 : ny - 1) * nx + i];
          uz[c] = (d[0][c] + right) * R(0.5);
          vz[c] = (d[1][c] + above) * R(0.5);
        }
    // (3) the squares, their sum, the quotient
    R* po = out + o * nf * plane;
    for (int64_t c = 0; c < nf * plane; ++c) {
      const R a2 = uz[c] * uz[c], b2 = vz[c] * vz[c];
      const R s2 = a2 + b2;
      if (!clo) {
        po[c] = b ? d[2][c] / s2 : s2;
        continue;
      }
      const R ri = d[2][c] / (s2 + clo[4]);
      const R rp = (ri + std::fabs(ri)) * R(0.5);
      const R den = R(1) + clo[1] * rp;
      const R nu = clo[0] / (den * den) + clo[2];
      po[c] = nu;
      out_kappa[o * nf * plane + c] = nu / den + clo[3];
    }
  }
  return XG_OK;
}

// the isopycnal slopes of the header as the stages of their chain over one (Z, Y, X) volume at a time, each into a temporary:
// the difference along X (Y) over its metric, its mean back to the centre, the mean of that along Z to the faces -- each
// stage padding its own input -- the difference of b along Z over its metric, the two quotients, their negation.
// arr[] = {mx, my, mz}: mx and my at the field's levels, mz at the faces
template <typename R>
int islope(const R* b, const R* const arr[3], const int64_t* const st[3], R* out_x, R* out_y, const int64_t* shape, int ndim,
           int outer, const int bc[3], const R fill[3]) {  // bc, fill: X, Y, Z
  const char* name = "isopycnal slope";
  if (!b || !out_x || !out_y || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "%s: ndim %d not in [3,%d]", name, ndim, XG_MAX_NDIM);
  for (int k = 0; k < 3; ++k)
    if (bc[k] < XG_BC_PERIODIC || bc[k] > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "%s: boundary mode %d: periodic, fill or extend", name, bc[k]);
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  for (int k = 0; k < 3; ++k)
    if (arr[k] && !st[k]) return fail(XG_ERR_INVALID, "%s: metric without strides", name);
  const int64_t nz = shape[ndim - 3], ny = shape[ndim - 2], nx = shape[ndim - 1], plane = ny * nx, vol = nz * plane;
  if (nz == 0) return fail(XG_ERR_INVALID, "%s: no level along Z", name);
  const int64_t nf = nz + outer;  // faces
  int64_t lead = 1;
  for (int d = 0; d < ndim - 3; ++d) lead *= shape[d];
  if (lead == 0 || vol == 0) return XG_OK;
  const int64_t n[3] = {nx, ny, nz}, step[3] = {1, nx, plane};
  std::vector<R> g((size_t)vol), G[2], bz((size_t)(nf * plane)), gf((size_t)(nf * plane));
  G[0].resize((size_t)vol);
  G[1].resize((size_t)vol);
  for (int64_t o = 0; o < lead; ++o) {
    int64_t rem = o, off[3] = {0, 0, 0};  // the lead index decomposed for the broadcast strides
    for (int dd = ndim - 4; dd >= 0; --dd) {
      const int64_t i = rem % shape[dd];
      rem /= shape[dd];
      for (int k = 0; k < 3; ++k)
        if (arr[k]) off[k] += i * st[k][dd];
    }
    auto met = [&](int k, int64_t z, int64_t j, int64_t i) -> R {
      return arr[k][off[k] + z * st[k][ndim - 3] + j * st[k][ndim - 2] + i * st[k][ndim - 1]];
    };
    const R* p = b + o * vol;
    // element q of `a` along axis `ax` (0: X, 1: Y, 2: Z) from the cell at `c` whose index there is `at`; beyond either end:
    // the pad of that axis
    auto get = [&](const R* a, int ax, int64_t c, int64_t at, int64_t q) -> R {
      if (q < 0 || q >= n[ax]) {
        if (bc[ax] == XG_BC_FILL) return fill[ax];
        q = bc[ax] == XG_BC_PERIODIC ? (q < 0 ? n[ax] - 1 : 0) : (q < 0 ? 0 : n[ax] - 1);
      }
      return a[c + (q - at) * step[ax]];
    };
    for (int ax = 0; ax < 2; ++ax) {
      // (1) the difference to the cell before, over the metric; (2) the mean with the difference after
      for (int64_t z = 0; z < nz; ++z)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = z * plane + j * nx + i, at = ax == 0 ? i : j;
            R d = p[c] - get(p, ax, c, at, at - 1);
            if (arr[ax]) d = d / met(ax, z, j, i);
            g[c] = d;
          }
      for (int64_t z = 0; z < nz; ++z)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = z * plane + j * nx + i, at = ax == 0 ? i : j;
            G[ax][c] = (g[c] + get(g.data(), ax, c, at, at + 1)) * R(0.5);
          }
    }
    // (3) b's difference along Z at the faces over its metric: level z of the padded field is a level of it or its pad
    for (int64_t z = 0; z < nf; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t c = j * nx + i;
          R d = get(p, 2, c, 0, z) - get(p, 2, c, 0, z - 1);
          if (arr[2]) d = d / met(2, z, j, i);
          bz[z * plane + c] = d;
        }
    // (4) the level means at the faces, the quotient, the negation
    for (int ax = 0; ax < 2; ++ax) {
      R* po = (ax == 0 ? out_x : out_y) + o * nf * plane;
      for (int64_t z = 0; z < nf; ++z)
        for (int64_t c = 0; c < plane; ++c)
          gf[z * plane + c] = (get(G[ax].data(), 2, c, 0, z - 1) + get(G[ax].data(), 2, c, 0, z)) * R(0.5);
      for (int64_t c = 0; c < nf * plane; ++c) {
        const R quot = gf[c] / bz[c];
        po[c] = R(-1) * quot;
      }
    }
  }
  return XG_OK;
}

// the tensor column of the header: the slopes of `islope` into two temporaries, then the stages of the chain after them, one
// operation each
template <typename R>
int reditensor(const R* b, const R* const arr[3], const int64_t* const st[3], R kappa, R m2, int taper, R* out_x, R* out_y,
               R* out_z, const int64_t* shape, int ndim, int outer, const int bc[3], const R fill[3]) {
  const char* name = "redi tensor";
  if (!b || !out_x || !out_y || !out_z || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (taper != 0 && taper != 1) return fail(XG_ERR_INVALID, "%s: taper %d is neither 0 nor 1", name, taper);
  int64_t n = 0;
  if (ndim >= 3 && ndim <= XG_MAX_NDIM && (outer == 0 || outer == 1) && shape[ndim - 3] > 0) {
    n = shape[ndim - 3] + outer;
    for (int d = 0; d < ndim; ++d)
      if (d != ndim - 3) n *= shape[d];
    const R* r[3] = {out_x, out_y, out_z};
    for (int i = 0; i < 3; ++i)
      for (int j = i + 1; j < 3; ++j)
        if (n > 0 && (uintptr_t)r[i] < (uintptr_t)(r[j] + n) && (uintptr_t)r[j] < (uintptr_t)(r[i] + n))
          return fail(XG_ERR_INVALID, "%s: the results overlap", name);
  }
  std::vector<R> sx((size_t)n), sy((size_t)n);
  // (every other condition is `islope`'s, which writes nothing when it refuses; the temporaries are never NULL to it)
  R dummy[1];
  const int rc = islope<R>(b, arr, st, n ? sx.data() : dummy, n ? sy.data() : dummy, shape, ndim, outer, bc, fill);
  if (rc != XG_OK) return rc;
  for (int64_t c = 0; c < n; ++c) {
    const R s2 = sx[c] * sx[c] + sy[c] * sy[c];
    R kt = kappa;
    if (taper) {
      const R ex = s2 - m2;
      const R den = m2 + (ex + std::fabs(ex)) * R(0.5);
      kt = kappa * (m2 / den);
    }
    out_x[c] = kt * sx[c];
    out_y[c] = kt * sy[c];
    out_z[c] = kt * s2;
  }
  return XG_OK;
}

// the divergence of the off-diagonal vertical isoneutral flux of the header as the stages of its chain over one (Z, Y, X)
// volume at a time, each into a temporary: stages (1) and (2) of `islope` on `a`, the level means at the faces, the two
// products, their sum, the closed faces, the difference of the flux to the next face's over the result's metric.
// arr[] = {mx, my, mc}, all at the field's levels
template <typename R>
int rediflux(const R* a, const R* kwx, const R* kwy, const R* const arr[3], const int64_t* const st[3], R* out,
             const int64_t* shape, int ndim, int outer, int closed, const int bc[3], const R fill[3]) {  // bc, fill: X, Y, Z
  const char* name = "redi vertical flux divergence";
  if (!a || !kwx || !kwy || !out || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "%s: ndim %d not in [3,%d]", name, ndim, XG_MAX_NDIM);
  for (int k = 0; k < 3; ++k)
    if (bc[k] < XG_BC_PERIODIC || bc[k] > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "%s: boundary mode %d: periodic, fill or extend", name, bc[k]);
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  if (closed != 0 && closed != 1) return fail(XG_ERR_INVALID, "%s: closed %d is neither 0 nor 1", name, closed);
  for (int k = 0; k < 3; ++k)
    if (arr[k] && !st[k]) return fail(XG_ERR_INVALID, "%s: metric without strides", name);
  const int64_t nz = shape[ndim - 3], ny = shape[ndim - 2], nx = shape[ndim - 1], plane = ny * nx, vol = nz * plane;
  if (nz == 0) return fail(XG_ERR_INVALID, "%s: no level along Z", name);
  const int64_t nf = nz + outer;  // faces
  int64_t lead = 1;
  for (int d = 0; d < ndim - 3; ++d) lead *= shape[d];
  if (lead == 0 || vol == 0) return XG_OK;
  const int64_t n[3] = {nx, ny, nz}, step[3] = {1, nx, plane};
  std::vector<R> g((size_t)vol), G[2], gf((size_t)(nf * plane)), f((size_t)(nf * plane));
  G[0].resize((size_t)vol);
  G[1].resize((size_t)vol);
  for (int64_t o = 0; o < lead; ++o) {
    int64_t rem = o, off[3] = {0, 0, 0};  // the lead index decomposed for the broadcast strides
    for (int dd = ndim - 4; dd >= 0; --dd) {
      const int64_t i = rem % shape[dd];
      rem /= shape[dd];
      for (int k = 0; k < 3; ++k)
        if (arr[k]) off[k] += i * st[k][dd];
    }
    auto met = [&](int k, int64_t z, int64_t j, int64_t i) -> R {
      return arr[k][off[k] + z * st[k][ndim - 3] + j * st[k][ndim - 2] + i * st[k][ndim - 1]];
    };
    const R* p = a + o * vol;
    // element q of `x` along axis `ax` (0: X, 1: Y, 2: Z) from the cell at `c` whose index there is `at`; beyond either end:
    // the pad of that axis
    auto get = [&](const R* x, int ax, int64_t c, int64_t at, int64_t q) -> R {
      if (q < 0 || q >= n[ax]) {
        if (bc[ax] == XG_BC_FILL) return fill[ax];
        q = bc[ax] == XG_BC_PERIODIC ? (q < 0 ? n[ax] - 1 : 0) : (q < 0 ? 0 : n[ax] - 1);
      }
      return x[c + (q - at) * step[ax]];
    };
    for (int ax = 0; ax < 2; ++ax) {
      // (1) the difference to the cell before, over the metric; (2) the mean with the difference after
      for (int64_t z = 0; z < nz; ++z)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = z * plane + j * nx + i, at = ax == 0 ? i : j;
            R d = p[c] - get(p, ax, c, at, at - 1);
            if (arr[ax]) d = d / met(ax, z, j, i);
            g[c] = d;
          }
      for (int64_t z = 0; z < nz; ++z)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = z * plane + j * nx + i, at = ax == 0 ? i : j;
            G[ax][c] = (g[c] + get(g.data(), ax, c, at, at + 1)) * R(0.5);
          }
    }
    // (3) the level means at the faces, the product with the tensor component; the second product is added to the first
    for (int ax = 0; ax < 2; ++ax) {
      const R* kw = (ax == 0 ? kwx : kwy) + o * nf * plane;
      for (int64_t z = 0; z < nf; ++z) {
        if (closed && (z == 0 || z == nz)) continue;  // (neither the pad level nor the tensor is read there)
        for (int64_t c = 0; c < plane; ++c) {
          gf[z * plane + c] = (get(G[ax].data(), 2, c, 0, z - 1) + get(G[ax].data(), 2, c, 0, z)) * R(0.5);
          const R prod = kw[z * plane + c] * gf[z * plane + c];
          f[z * plane + c] = ax == 0 ? prod : f[z * plane + c] + prod;
        }
      }
    }
    // (4) no flux through the top and the bottom
    if (closed)
      for (int64_t c = 0; c < plane; ++c) {
        f[c] = R(0);
        if (outer) f[nz * plane + c] = R(0);
      }
    // (5) the difference to the next face's; `left` pads the flux beyond its last face
    for (int64_t z = 0; z < nz; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t c = j * nx + i;
          R next;
          if (z + 1 < nf) next = f[(z + 1) * plane + c];
          else if (bc[2] == XG_BC_FILL) next = fill[2];
          else next = f[((bc[2] == XG_BC_PERIODIC) ? 0 : nz - 1) * plane + c];
          R d = next - f[z * plane + c];
          if (arr[2]) d = d / met(2, z, j, i);
          out[o * vol + z * plane + c] = d;
        }
  }
  return XG_OK;
}

// the U- and V-point components of the tapered tensor of the header as the stages of their chain over one
// (Z, Y, X) volume at a time, each into a temporary: the differences along X and Y over their metrics; b's difference along Z
// at the faces over its metric and its mean back to the levels; the means of that towards u's and v's points; the centre
// means of the two differences and their means towards the other point; the four quotients, negated; the taper at each
// point -- each stage padding its own input.  arr[] = {mx, my, mz}: mx and my at the field's levels, mz at the faces
template <typename R>
int rediuv(const R* b, const R* const arr[3], const int64_t* const st[3], R kappa, R m2, int taper, R* out_u, R* out_v,
           const int64_t* shape, int ndim, int outer, const int bc[3], const R fill[3]) {  // bc, fill: X, Y, Z
  const char* name = "redi horizontal tensor";
  if (!b || !out_u || !out_v || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "%s: ndim %d not in [3,%d]", name, ndim, XG_MAX_NDIM);
  for (int k = 0; k < 3; ++k)
    if (bc[k] < XG_BC_PERIODIC || bc[k] > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "%s: boundary mode %d: periodic, fill or extend", name, bc[k]);
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  if (taper != 0 && taper != 1) return fail(XG_ERR_INVALID, "%s: taper %d is neither 0 nor 1", name, taper);
  const int64_t nz = shape[ndim - 3], ny = shape[ndim - 2], nx = shape[ndim - 1], plane = ny * nx, vol = nz * plane;
  if (nz == 0) return fail(XG_ERR_INVALID, "%s: no level along Z", name);
  int64_t lead = 1;
  for (int d = 0; d < ndim - 3; ++d) lead *= shape[d];
  if (lead * vol > 0 && (uintptr_t)out_u < (uintptr_t)(out_v + lead * vol) && (uintptr_t)out_v < (uintptr_t)(out_u + lead * vol))
    return fail(XG_ERR_INVALID, "%s: the results overlap", name);
  for (int k = 0; k < 3; ++k)
    if (arr[k] && !st[k]) return fail(XG_ERR_INVALID, "%s: metric without strides", name);
  const int64_t nf = nz + outer;  // faces
  if (lead == 0 || vol == 0) return XG_OK;
  const int64_t n[3] = {nx, ny, nz}, step[3] = {1, nx, plane};
  std::vector<R> g[2], gc((size_t)vol), bzf((size_t)(nf * plane)), bzc((size_t)vol), bzp((size_t)vol), cross((size_t)vol);
  g[0].resize((size_t)vol);
  g[1].resize((size_t)vol);
  for (int64_t o = 0; o < lead; ++o) {
    int64_t rem = o, off[3] = {0, 0, 0};  // the lead index decomposed for the broadcast strides
    for (int dd = ndim - 4; dd >= 0; --dd) {
      const int64_t i = rem % shape[dd];
      rem /= shape[dd];
      for (int k = 0; k < 3; ++k)
        if (arr[k]) off[k] += i * st[k][dd];
    }
    auto met = [&](int k, int64_t z, int64_t j, int64_t i) -> R {
      return arr[k][off[k] + z * st[k][ndim - 3] + j * st[k][ndim - 2] + i * st[k][ndim - 1]];
    };
    const R* p = b + o * vol;
    // element q of `a` along axis `ax` (0: X, 1: Y, 2: Z) from the cell at `c` whose index there is `at`; beyond either end:
    // the pad of that axis
    auto get = [&](const R* a, int ax, int64_t c, int64_t at, int64_t q) -> R {
      if (q < 0 || q >= n[ax]) {
        if (bc[ax] == XG_BC_FILL) return fill[ax];
        q = bc[ax] == XG_BC_PERIODIC ? (q < 0 ? n[ax] - 1 : 0) : (q < 0 ? 0 : n[ax] - 1);
      }
      return a[c + (q - at) * step[ax]];
    };
    // (1) the differences to the cell before along X and along Y, over their metrics: at u's and at v's points
    for (int ax = 0; ax < 2; ++ax)
      for (int64_t z = 0; z < nz; ++z)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = z * plane + j * nx + i, at = ax == 0 ? i : j;
            R d = p[c] - get(p, ax, c, at, at - 1);
            if (arr[ax]) d = d / met(ax, z, j, i);
            g[ax][c] = d;
          }
    // (2) b's difference along Z at the faces over its metric: level z of the padded field is a level of it or its pad
    for (int64_t z = 0; z < nf; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t c = j * nx + i;
          R d = get(p, 2, c, 0, z) - get(p, 2, c, 0, z - 1);
          if (arr[2]) d = d / met(2, z, j, i);
          bzf[z * plane + c] = d;
        }
    // (3) its mean back to the levels; `left` pads the derivative beyond its last face
    for (int64_t z = 0; z < nz; ++z)
      for (int64_t c = 0; c < plane; ++c) {
        R next;
        if (z + 1 < nf) next = bzf[(z + 1) * plane + c];
        else if (bc[2] == XG_BC_FILL) next = fill[2];
        else next = bzf[((bc[2] == XG_BC_PERIODIC) ? 0 : nz - 1) * plane + c];
        bzc[z * plane + c] = (bzf[z * plane + c] + next) * R(0.5);
      }
    for (int ax = 0; ax < 2; ++ax) {  // 0: u's points, kuz;  1: v's points, kvz
      const int ot = 1 - ax;          // the other horizontal axis
      // (4) db/dz at the point: the mean with the cell before along `ax`
      // (5) the other derivative there: its centre mean along its own axis, then the mean with the cell before along `ax`
      for (int64_t z = 0; z < nz; ++z)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = z * plane + j * nx + i, at = ot == 0 ? i : j;
            gc[c] = (g[ot][c] + get(g[ot].data(), ot, c, at, at + 1)) * R(0.5);
          }
      for (int64_t z = 0; z < nz; ++z)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = z * plane + j * nx + i, at = ax == 0 ? i : j;
            bzp[c] = (get(bzc.data(), ax, c, at, at - 1) + bzc[c]) * R(0.5);
            cross[c] = (get(gc.data(), ax, c, at, at - 1) + gc[c]) * R(0.5);
          }
      // (6) the two slopes, the taper, the component along `ax`
      R* po = (ax == 0 ? out_u : out_v) + o * vol;
      for (int64_t c = 0; c < vol; ++c) {
        const R q_own = g[ax][c] / bzp[c], q_other = cross[c] / bzp[c];
        const R s_own = R(-1) * q_own, s_other = R(-1) * q_other;
        const R sx = ax == 0 ? s_own : s_other, sy = ax == 0 ? s_other : s_own;
        const R s2 = sx * sx + sy * sy;
        R kt = kappa;
        if (taper) {
          const R ex = s2 - m2;
          const R den = m2 + (ex + std::fabs(ex)) * R(0.5);
          kt = kappa * (m2 / den);
        }
        po[c] = kt * s_own;
      }
    }
  }
  return XG_OK;
}

// the bolus velocity of the header as the stages of its chain over one lead index at a time, each into a temporary: the two
// means towards the left points, the closed faces, the differences to the next face's over their metrics, negated; the
// two transports, their differences to the next column's / row's, the sum over the area.
// arr[] = {mzu, mzv, dyG, dxG, rA}: the first two at the levels, the others at the faces
template <typename R>
int bolus(const R* kwx, const R* kwy, const R* const arr[5], const int64_t* const st[5], R* out_u, R* out_v, R* out_w,
          const int64_t* shape, int ndim, int outer, int closed, const int bc[3], const R fill[3]) {  // bc, fill: X, Y, Z
  const char* name = "bolus velocity";
  if (!kwx || !kwy || !out_u || !out_v || !out_w || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 3 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "%s: ndim %d not in [3,%d]", name, ndim, XG_MAX_NDIM);
  for (int k = 0; k < 3; ++k)
    if (bc[k] < XG_BC_PERIODIC || bc[k] > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "%s: boundary mode %d: periodic, fill or extend", name, bc[k]);
  if (outer != 0 && outer != 1) return fail(XG_ERR_INVALID, "%s: outer %d is neither 0 (left) nor 1", name, outer);
  if (closed != 0 && closed != 1) return fail(XG_ERR_INVALID, "%s: closed %d is neither 0 nor 1", name, closed);
  const int64_t nz = shape[ndim - 3], ny = shape[ndim - 2], nx = shape[ndim - 1], plane = ny * nx;
  if (nz < 1) return fail(XG_ERR_INVALID, "%s: no level along Z", name);
  for (int k = 0; k < 5; ++k)
    if (arr[k] && !st[k]) return fail(XG_ERR_INVALID, "%s: metric without strides", name);
  const int64_t nf = nz + outer;  // faces
  int64_t lead = 1;
  for (int d = 0; d < ndim - 3; ++d) lead *= shape[d];
  if (lead == 0 || plane == 0) return XG_OK;
  std::vector<R> psi[2], t[2];
  for (int ax = 0; ax < 2; ++ax) {
    psi[ax].resize((size_t)(nf * plane));
    t[ax].resize((size_t)(nf * plane));
  }
  for (int64_t o = 0; o < lead; ++o) {
    int64_t rem = o, off[5] = {0, 0, 0, 0, 0};  // the lead index decomposed for the broadcast strides
    for (int dd = ndim - 4; dd >= 0; --dd) {
      const int64_t i = rem % shape[dd];
      rem /= shape[dd];
      for (int k = 0; k < 5; ++k)
        if (arr[k]) off[k] += i * st[k][dd];
    }
    auto met = [&](int k, int64_t z, int64_t j, int64_t i) -> R {
      return arr[k][off[k] + z * st[k][ndim - 3] + j * st[k][ndim - 2] + i * st[k][ndim - 1]];
    };
    for (int ax = 0; ax < 2; ++ax) {  // 0: X, kwx, ub;  1: Y, kwy, vb
      const R* kw = (ax == 0 ? kwx : kwy) + o * nf * plane;
      const int64_t n = ax == 0 ? nx : ny, step = ax == 0 ? 1 : nx;
      // (1) the mean with the cell before, (2) the closed faces, (3) the transport
      for (int64_t z = 0; z < nf; ++z) {
        const bool shut = closed && (z == 0 || z == nz);  // (kw is not read there)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = z * plane + j * nx + i, at = ax == 0 ? i : j;
            R p = R(0);
            if (!shut) {
              R before;
              if (at > 0) before = kw[c - step];
              else if (bc[ax] == XG_BC_FILL) before = fill[ax];
              else before = kw[c + ((bc[ax] == XG_BC_PERIODIC) ? n - 1 : 0) * step];
              p = (before + kw[c]) * R(0.5);
            }
            psi[ax][c] = p;
            t[ax][c] = arr[2 + ax] ? p * met(2 + ax, z, j, i) : p;
          }
      }
      // (4) the difference to the next face's over the metric, negated; `left` pads the streamfunction beyond its last face
      R* po = (ax == 0 ? out_u : out_v) + o * nz * plane;
      for (int64_t z = 0; z < nz; ++z)
        for (int64_t j = 0; j < ny; ++j)
          for (int64_t i = 0; i < nx; ++i) {
            const int64_t c = j * nx + i;
            R next;
            if (z + 1 < nf) next = psi[ax][(z + 1) * plane + c];
            else if (bc[2] == XG_BC_FILL) next = fill[2];
            else next = psi[ax][((bc[2] == XG_BC_PERIODIC) ? 0 : nz - 1) * plane + c];
            R d = next - psi[ax][z * plane + c];
            if (arr[ax]) d = d / met(ax, z, j, i);
            po[z * plane + c] = R(-1) * d;
          }
    }
    // (5) the divergence of the transports, each padded beyond its last column / row, over the area
    R* pw = out_w + o * nf * plane;
    for (int64_t z = 0; z < nf; ++z)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          const int64_t c = z * plane + j * nx + i;
          R right, up;
          if (i + 1 < nx) right = t[0][c + 1];
          else if (bc[0] == XG_BC_FILL) right = fill[0];
          else right = t[0][c - i + ((bc[0] == XG_BC_PERIODIC) ? 0 : nx - 1)];
          if (j + 1 < ny) up = t[1][c + nx];
          else if (bc[1] == XG_BC_FILL) up = fill[1];
          else up = t[1][c - j * nx + ((bc[1] == XG_BC_PERIODIC) ? 0 : ny - 1) * nx];
          R d = (right - t[0][c]) + (up - t[1][c]);
          if (arr[4]) d = d / met(4, z, j, i);
          pw[c] = d;
        }
  }
  return XG_OK;
}

// kinetic energy (ke_only) and the vector-invariant momentum advection of the header: the stages of the chain one after
// the other over whole planes, each read through `get`, which pads a plane by one cell on one axis at a time (periodic:
// the plane's own value at the wrapped index, extend: at the clamped index, fill: the fill value of that axis).
// met[] = {rAz, coriolis, dxC, dyC}: the three metrics all or none, coriolis on its own
template <typename R>
int momentum(bool ke_only, const R* u, const R* v, const R* const met[4], const int64_t* const ms[4], R* out_u, R* out_v,
             const int64_t* shape, int ndim, int bc_x, R fill_x, int bc_y, R fill_y) {
  if (!u || !v || !out_u || (!ke_only && !out_v) || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 2 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [2,%d]", ndim, XG_MAX_NDIM);
  for (int b : {bc_x, bc_y})
    if (b < XG_BC_PERIODIC || b > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "boundary mode %d: periodic, fill or extend", b);
  for (int k = 0; k < 4; ++k)
    if (met[k] && !ms[k]) return fail(XG_ERR_INVALID, "metric without strides");
  const int nmet = (met[0] != nullptr) + (met[2] != nullptr) + (met[3] != nullptr);
  if (nmet != 0 && nmet != 3) return fail(XG_ERR_INVALID, "momentum advection: the three metrics rAz, dxC, dyC, or none");
  const int64_t ny = shape[ndim - 2], nx = shape[ndim - 1];
  int64_t outer = 1;
  for (int d = 0; d < ndim - 2; ++d) outer *= shape[d];
  if (outer == 0 || ny == 0 || nx == 0) return XG_OK;
  const size_t n = (size_t)(ny * nx);
  std::vector<R> zeta(n), uu(n), vv(n), ke(n), vx(n), uy(n);
  auto get = [&](const R* a, int64_t j, int64_t i) -> R {
    if (i < 0 || i >= nx) {
      if (bc_x == XG_BC_FILL) return fill_x;
      i = bc_x == XG_BC_PERIODIC ? (i + nx) % nx : (i < 0 ? 0 : nx - 1);
    }
    if (j < 0 || j >= ny) {
      if (bc_y == XG_BC_FILL) return fill_y;
      j = bc_y == XG_BC_PERIODIC ? (j + ny) % ny : (j < 0 ? 0 : ny - 1);
    }
    return a[j * nx + i];
  };
  for (int64_t o = 0; o < outer; ++o) {
    int64_t rem = o, moff[4] = {0, 0, 0, 0};  // the outer index decomposed for the broadcast strides
    for (int d = ndim - 3; d >= 0; --d) {
      const int64_t i = rem % shape[d];
      rem /= shape[d];
      for (int k = 0; k < 4; ++k)
        if (met[k]) moff[k] += i * ms[k][d];
    }
    auto m = [&](int k, int64_t j, int64_t i) { return met[k][moff[k] + j * ms[k][ndim - 2] + i * ms[k][ndim - 1]]; };
    const R* pu = u + o * ny * nx;
    const R* pv = v + o * ny * nx;
    auto each = [&](auto&& body) {
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) body(j, i, j * nx + i);
    };
    each([&](int64_t, int64_t, int64_t c) { uu[c] = pu[c] * pu[c]; vv[c] = pv[c] * pv[c]; });
    each([&](int64_t j, int64_t i, int64_t c) {
      ke[c] = R(0.5) * ((uu[c] + get(uu.data(), j, i + 1)) / R(2) + (vv[c] + get(vv.data(), j + 1, i)) / R(2));
    });
    if (ke_only) {
      each([&](int64_t, int64_t, int64_t c) { out_u[o * ny * nx + c] = ke[c]; });
      continue;
    }
    each([&](int64_t j, int64_t i, int64_t c) {
      R z = (pv[c] - get(pv, j, i - 1)) - (pu[c] - get(pu, j - 1, i));
      if (nmet) z = z / m(0, j, i);
      if (met[1]) z = z + m(1, j, i);
      zeta[c] = z;
      vx[c] = (get(pv, j, i - 1) + pv[c]) / R(2);
      uy[c] = (get(pu, j - 1, i) + pu[c]) / R(2);
    });
    each([&](int64_t j, int64_t i, int64_t c) {
      const R zy = (zeta[c] + get(zeta.data(), j + 1, i)) / R(2), vbar = (vx[c] + get(vx.data(), j + 1, i)) / R(2);
      const R zx = (zeta[c] + get(zeta.data(), j, i + 1)) / R(2), ubar = (uy[c] + get(uy.data(), j, i + 1)) / R(2);
      R gx = ke[c] - get(ke.data(), j, i - 1), gy = ke[c] - get(ke.data(), j - 1, i);
      if (nmet) {
        gx = gx / m(2, j, i);
        gy = gy / m(3, j, i);
      }
      const R pu_ = zy * vbar, pv_ = zx * ubar;
      out_u[o * ny * nx + c] = pu_ - gx;
      out_v[o * ny * nx + c] = R(-1) * pv_ - gy;
    });
  }
  return XG_OK;
}

// the harmonic viscosity of the header as five plain passes over one (Y, X) plane at a time, each into its own temporary:
// D and zeta from the padded fields, their products with the coefficients, the four differences of the padded products,
// the combination.  Each read beyond the plane goes through `pad1`, which pads ONE axis by one cell.
// pl[] = {rA, rAz, dxC, dyC, dyG, dxG, nu_d, nu_z}: the six metrics all or none, the two coefficients both or none
template <typename R>
int hvisc(const R* u, const R* v, const R* const pl[8], const int64_t* const ps[8], R* out_u, R* out_v, const int64_t* shape,
          int ndim, int bc_x, R fill_x, R zfill_x, int bc_y, R fill_y, R zfill_y) {
  if (!u || !v || !out_u || !out_v || !shape) return fail(XG_ERR_INVALID, "NULL array argument");
  if (ndim < 2 || ndim > XG_MAX_NDIM) return fail(XG_ERR_UNSUPPORTED, "ndim %d not in [2,%d]", ndim, XG_MAX_NDIM);
  for (int b : {bc_x, bc_y})
    if (b < XG_BC_PERIODIC || b > XG_BC_EXTEND) return fail(XG_ERR_INVALID, "boundary mode %d: periodic, fill or extend", b);
  int nmet = 0, nvis = 0;
  for (int k = 0; k < 8; ++k) {
    if (pl[k] && !ps[k]) return fail(XG_ERR_INVALID, "metric without strides");
    (k < 6 ? nmet : nvis) += pl[k] != nullptr;
  }
  if (nmet != 0 && nmet != 6) return fail(XG_ERR_INVALID, "horizontal viscosity: the six metrics rA, rAz, dxC, dyC, dyG, dxG, or none");
  if (nvis != 0 && nvis != 2) return fail(XG_ERR_INVALID, "horizontal viscosity: both coefficients nu_d, nu_z, or none");
  const int64_t ny = shape[ndim - 2], nx = shape[ndim - 1];
  int64_t outer = 1;
  for (int d = 0; d < ndim - 2; ++d) outer *= shape[d];
  if (outer == 0 || ny == 0 || nx == 0) return XG_OK;
  const size_t n = (size_t)(ny * nx);
  std::vector<R> div(n), zeta(n), dx(n), dy(n), zy(n), zx(n);
  // cell k of an axis of n cells padded by one on each side: the cell itself, the wrapped / clamped one, or -1 = the fill
  auto pad1 = [](int64_t k, int64_t n, int bc) -> int64_t {
    if (k >= 0 && k < n) return k;
    if (bc == XG_BC_FILL) return -1;
    if (bc == XG_BC_PERIODIC) return k < 0 ? n - 1 : 0;
    return k < 0 ? 0 : n - 1;
  };
  for (int64_t o = 0; o < outer; ++o) {
    int64_t rem = o, moff[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the outer index decomposed for the broadcast strides
    for (int d = ndim - 3; d >= 0; --d) {
      const int64_t i = rem % shape[d];
      rem /= shape[d];
      for (int k = 0; k < 8; ++k)
        if (pl[k]) moff[k] += i * ps[k][d];
    }
    auto m = [&](int k, int64_t j, int64_t i) { return pl[k][moff[k] + j * ps[k][ndim - 2] + i * ps[k][ndim - 1]]; };
    const R* pu = u + o * ny * nx;
    const R* pv = v + o * ny * nx;
    auto along_x = [&](const R* a, int64_t j, int64_t i, R fill) { const int64_t q = pad1(i, nx, bc_x); return q < 0 ? fill : a[j * nx + q]; };
    auto along_y = [&](const R* a, int64_t j, int64_t i, R fill) { const int64_t q = pad1(j, ny, bc_y); return q < 0 ? fill : a[q * nx + i]; };
    // (1) the divergence at the centre, the vorticity at the corner
    for (int64_t j = 0; j < ny; ++j)
      for (int64_t i = 0; i < nx; ++i) {
        const int64_t c = j * nx + i;
        R d = (along_x(pu, j, i + 1, fill_x) - pu[c]) + (along_y(pv, j + 1, i, fill_y) - pv[c]);
        R z = (pv[c] - along_x(pv, j, i - 1, fill_x)) - (pu[c] - along_y(pu, j - 1, i, fill_y));
        if (nmet) {
          d = d / m(0, j, i);
          z = z / m(1, j, i);
        }
        div[c] = d;
        zeta[c] = z;
      }
    // (2) times the coefficients, in place
    if (nvis)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          div[j * nx + i] = div[j * nx + i] * m(6, j, i);
          zeta[j * nx + i] = zeta[j * nx + i] * m(7, j, i);
        }
    // (3) the gradient of the first product (towards the cell left of / below it), (4) the differences of the second one
    // (towards the corner above / right of it)
    for (int64_t j = 0; j < ny; ++j)
      for (int64_t i = 0; i < nx; ++i) {
        const int64_t c = j * nx + i;
        dx[c] = div[c] - along_x(div.data(), j, i - 1, fill_x);
        dy[c] = div[c] - along_y(div.data(), j - 1, i, fill_y);
        zy[c] = along_y(zeta.data(), j + 1, i, zfill_y) - zeta[c];
        zx[c] = along_x(zeta.data(), j, i + 1, zfill_x) - zeta[c];
        if (nmet) {
          dx[c] = dx[c] / m(2, j, i);
          dy[c] = dy[c] / m(3, j, i);
          zy[c] = zy[c] / m(4, j, i);
          zx[c] = zx[c] / m(5, j, i);
        }
      }
    // (5) the two tendencies
    for (size_t c = 0; c < n; ++c) {
      out_u[(size_t)(o * ny * nx) + c] = dx[c] - zy[c];
      out_v[(size_t)(o * ny * nx) + c] = dy[c] + zx[c];
    }
  }
  return XG_OK;
}

// xg_stencil_multi: up to four plain two-point results of one (outer, ny, nx) field, one cell at a time; what is declined is
// what the header lists (the kernel's conditions: the device layer then behaves alike over both builds)
template <typename R>
int stencil_multi(const R* in, const int64_t* shape, int ndim, int n, const xg_multi_desc* desc) {
  if (!in || !shape || !desc) return fail(XG_ERR_INVALID, "NULL array argument");
  if (n < 1 || n > 4) return fail(XG_ERR_INVALID, "%d results asked of one pass (1 to 4)", n);
  for (int i = 0; i < n; ++i) {
    if (!desc[i].out) return fail(XG_ERR_INVALID, "NULL array argument");
    if (desc[i].op < XG_OP_DIFF || desc[i].op > XG_OP_MAX) return fail(XG_ERR_INVALID, "unknown op %d", desc[i].op);
  }
  if (ndim != 2 && ndim != 3) return fail(XG_DECLINED, "declined: %d dims", ndim);
  const int64_t nx = shape[ndim - 1], ny = shape[ndim - 2], outer = (ndim == 3) ? shape[0] : 1;
  if (nx < 1 || ny < 1 || outer < 1) return fail(XG_DECLINED, "declined: an empty array");
  const int64_t nv = 16 / (int64_t)sizeof(R);
  auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  if (nx % nv || !aligned(in)) return fail(XG_DECLINED, "declined: rows are not whole 16-byte lane vectors");
  const int64_t lim = 0x7fffffffll;
  if (nx > lim || ny > lim || outer > lim || nx * ny > lim || nx * ny * outer > lim) return fail(XG_DECLINED, "declined: 2^31 cells or more");
  const uint64_t bytes = (uint64_t)(nx * ny * outer) * sizeof(R);
  auto overlap = [bytes](const void* a, const void* b) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return p < q + bytes && q < p + bytes;
  };
  for (int i = 0; i < n; ++i) {
    const xg_multi_desc& d = desc[i];
    if (d.axis != ndim - 1 && d.axis != ndim - 2) return fail(XG_DECLINED, "declined: axis %d", d.axis);
    if (!((d.pad_lo == 1 && d.pad_hi == 0) || (d.pad_lo == 0 && d.pad_hi == 1))) return fail(XG_DECLINED, "declined: pads (%d,%d)", d.pad_lo, d.pad_hi);
    if (d.bc != XG_BC_PERIODIC && d.bc != XG_BC_FILL && d.bc != XG_BC_EXTEND) return fail(XG_DECLINED, "declined: boundary mode %d", d.bc);
    if (!aligned(d.out)) return fail(XG_DECLINED, "declined: a result is not 16-byte aligned");
    if (overlap(d.out, in)) return fail(XG_DECLINED, "declined: a result overlaps the input");
    for (int k = 0; k < i; ++k)
      if (overlap(d.out, desc[k].out)) return fail(XG_DECLINED, "declined: two results overlap");
  }
  for (int64_t o = 0; o < outer; ++o)
    for (int64_t j = 0; j < ny; ++j)
      for (int64_t x = 0; x < nx; ++x)  // the cell is read here, every result of it formed below
        for (int i = 0; i < n; ++i) {
          const xg_multi_desc& d = desc[i];
          const bool along_y = d.axis == ndim - 2;
          const int64_t len = along_y ? ny : nx, at = along_y ? j : x;
          R side[2];
          for (int s = 0; s < 2; ++s) {
            int64_t q = at + s - d.pad_lo;
            bool filled = false;
            if (q < 0 || q >= len) {
              filled = d.bc == XG_BC_FILL;
              q = (d.bc == XG_BC_PERIODIC) ? (q < 0 ? len - 1 : 0) : (q < 0 ? 0 : len - 1);
            }
            side[s] = filled ? (R)d.fill : in[(o * ny + (along_y ? q : j)) * nx + (along_y ? x : q)];
          }
          ((R*)d.out)[(o * ny + j) * nx + x] = op2<R>(d.op, side[0], side[1]);
        }
  return XG_OK;
}

}  // namespace

extern "C" {

int xg_version(void) { return XG_ABI_VERSION; }
int xg_last_error(char* buf, int n) {
  const int len = (int)strlen(g_err);
  if (buf && n > 0) {
    const int c = len < n - 1 ? len : n - 1;
    memcpy(buf, g_err, c);
    buf[c] = 0;
  }
  return len;
}
int xg_set_tunable(const char* name, int value) {
  if (!name) return fail(XG_ERR_INVALID, "NULL tunable name");
  for (auto& k : knobs())
    if (!strcmp(k.name, name)) { k.value = value; k.set = true; return XG_OK; }
  return fail(XG_ERR_INVALID, "unknown tunable '%s'", name);
}
int xg_get_tunable(const char* name, int* value) {
  if (!name || !value) return fail(XG_ERR_INVALID, "NULL argument");
  for (auto& k : knobs())
    if (!strcmp(k.name, name)) { *value = k.value; return XG_OK; }
  return fail(XG_ERR_INVALID, "unknown tunable '%s'", name);
}
int xg_device_count(void) { return 0; }  // the host build drives no device
int xg_set_device(int) { return fail(XG_ERR_UNSUPPORTED, "host build of the ABI: no device"); }
int xg_malloc(void** ptr, uint64_t bytes) {
  if (!ptr) return fail(XG_ERR_INVALID, "NULL argument");
  *ptr = malloc(bytes ? bytes : 1);
  return *ptr ? XG_OK : fail(XG_ERR_HIP, "out of host memory");
}
int xg_free(void* ptr) { free(ptr); return XG_OK; }
int xg_memcpy_h2d(void* dst, const void* src, uint64_t bytes, void*) { if (bytes) memcpy(dst, src, bytes); return XG_OK; }
int xg_memcpy_d2h(void* dst, const void* src, uint64_t bytes, void*) { if (bytes) memcpy(dst, src, bytes); return XG_OK; }
int xg_stream_sync(void*) { return XG_OK; }
int xg_pin_host(void* ptr, uint64_t bytes) { return (ptr && bytes) ? XG_OK : fail(XG_ERR_INVALID, "empty host range"); }  // nothing to lock
int xg_unpin_host(void*) { return XG_OK; }
int xg_stream_create(void** stream) {
  if (!stream) return fail(XG_ERR_INVALID, "NULL argument");
  *stream = nullptr;  // the host build runs everything on the calling thread
  return XG_OK;
}
int xg_stream_destroy(void*) { return XG_OK; }
// (no chained kernels on the host: nothing ever gives up)
int xg_chain_status(int* gave_up, int* redone) {
  if (gave_up) *gave_up = 0;
  if (redone) *redone = 0;
  return XG_OK;
}
int xg_chain_rearm(void) { return XG_OK; }
int xg_scatter_alloc(void** ptr, uint64_t bytes, uint64_t, int, uint64_t) {  // host build: plain memory (placement is an HBM matter)
  if (!ptr || !bytes) return fail(XG_ERR_INVALID, "NULL / empty request");
  *ptr = malloc(bytes);
  return *ptr ? XG_OK : fail(XG_ERR_HIP, "out of host memory");
}
int xg_scatter_free(void* ptr) { free(ptr); return XG_OK; }
int xg_scatter_stats(uint64_t* a, uint64_t* b, uint64_t* c) { if (a) *a = 0; if (b) *b = 0; if (c) *c = 0; return XG_OK; }
int xg_scatter_grade(void* p, uint64_t, double* ratio) { if (!p || !ratio) return fail(XG_ERR_INVALID, "NULL argument"); *ratio = 1.0; return XG_OK; }  // host memory: nothing to grade
int xg_scatter_grade_stats(uint64_t* a, uint64_t* b) { if (a) *a = 0; if (b) *b = 0; return XG_OK; }
void* xg_pool_alloc(ssize_t size, int, void*) { return size > 0 ? malloc((size_t)size) : nullptr; }
void xg_pool_free(void* ptr, ssize_t, int, void*) { free(ptr); }
int xg_bswap(void* data, uint64_t nelem, int elem_bytes, void*) {
  if (elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) return fail(XG_ERR_INVALID, "byte swap of %d-byte elements (2, 4 or 8)", elem_bytes);
  if (nelem && !data) return fail(XG_ERR_INVALID, "NULL buffer");
  unsigned char* p = (unsigned char*)data;
  for (uint64_t e = 0; e < nelem; ++e, p += elem_bytes)
    for (int b = 0; b < elem_bytes / 2; ++b) { unsigned char t = p[b]; p[b] = p[elem_bytes - 1 - b]; p[elem_bytes - 1 - b] = t; }
  return XG_OK;
}
int xg_mask_value(void* data, uint64_t nelem, int elem_bytes, double value, void*) {
  if (elem_bytes != 4 && elem_bytes != 8) return fail(XG_ERR_INVALID, "masking of %d-byte elements (float32 / float64 only)", elem_bytes);
  if (nelem && !data) return fail(XG_ERR_INVALID, "NULL buffer");
  if (elem_bytes == 4) { float* p = (float*)data; for (uint64_t i = 0; i < nelem; ++i) if (p[i] == (float)value) p[i] = NAN; }
  else { double* p = (double*)data; for (uint64_t i = 0; i < nelem; ++i) if (p[i] == value) p[i] = NAN; }
  return XG_OK;
}
int xg_event_create(void** ev) {
  if (!ev) return fail(XG_ERR_INVALID, "NULL argument");
  *ev = calloc(1, sizeof(double));
  return *ev ? XG_OK : fail(XG_ERR_HIP, "out of host memory");
}
int xg_event_record(void* ev, void*) {
  if (!ev) return fail(XG_ERR_INVALID, "NULL event");
  *(double*)ev = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  return XG_OK;
}
int xg_event_elapsed_ms(void* start, void* stop, float* ms) {
  if (!start || !stop || !ms) return fail(XG_ERR_INVALID, "NULL argument");
  *ms = (float)(*(double*)stop - *(double*)start);
  return XG_OK;
}
int xg_event_destroy(void* ev) { free(ev); return XG_OK; }

// the entry points whose results keep the lanes' width (every build: f64, f32, i64, i32)
#define XG_HOST_LANES(SFX, R)                                                                                         \
  int xg_stencil1d_##SFX(int op, const R* in, R* out, const int64_t* shape, int ndim, int axis, int64_t n_out,        \
                         int pad_lo, int pad_hi, int bc, R fill, const R* m_in, const int64_t* mis, const R* m_out,   \
                         const int64_t* mos, void*) {                                                                 \
    if (bc == XG_BC_HALO) return fail(XG_ERR_INVALID, "XG_BC_HALO needs xg_stencil1d_halo");                          \
    return stencil1d<R>(op, in, nullptr, out, shape, ndim, axis, n_out, pad_lo, pad_hi, bc, fill, m_in, mis, m_out,   \
                        mos);                                                                                         \
  }                                                                                                                   \
  int xg_stencil1d_halo_##SFX(int op, const R* in, const R* halo, R* out, const int64_t* shape, int ndim, int axis,   \
                              int64_t n_out, int pad_lo, int pad_hi, const R* m_out, const int64_t* mos, void*) {     \
    if (!halo && (pad_lo || pad_hi)) return fail(XG_ERR_INVALID, "NULL halo buffer");                                 \
    return stencil1d<R>(op, in, halo, out, shape, ndim, axis, n_out, pad_lo, pad_hi,                                  \
                        (pad_lo || pad_hi) ? XG_BC_HALO : XG_BC_NONE, R(0), nullptr, nullptr, m_out, mos);            \
  }                                                                                                                   \
  int xg_pad_##SFX(const R* in, R* out, const int64_t* shape, int ndim, const int64_t* lo, const int64_t* hi,         \
                   const int* bc, const R* fill, const int* order, void*) {                                           \
    return pad_nd<R>(in, out, shape, ndim, lo, hi, bc, fill, order);                                                  \
  }                                                                                                                   \
  int xg_binary_##SFX(int op, const R* a, const int64_t* sa, const R* b, const int64_t* sb, R* out,                   \
                      const int64_t* shape, int ndim, void*) {                                                        \
    return binary<R>(op, a, sa, b, sb, out, shape, ndim);                                                             \
  }                                                                                                                   \
  int xg_halo_put_##SFX(const R* halo, R* out, const int64_t* shape, int ndim, int axis, int pad_lo, int pad_hi, void*) { \
    View v;                                                                                                           \
    if (int rc = make_view(shape, ndim, axis, &v)) return rc;                                                         \
    const int64_t nh = (int64_t)pad_lo + pad_hi;                                                                      \
    if (pad_lo < 0 || pad_hi < 0 || v.n < nh) return fail(XG_ERR_INVALID, "bad halo widths");                         \
    if (v.outer * nh * v.inner == 0) return XG_OK;                                                                    \
    if (!halo || !out) return fail(XG_ERR_INVALID, "NULL array argument");                                            \
    for (int64_t o = 0; o < v.outer; ++o)                                                                             \
      for (int64_t h = 0; h < nh; ++h)                                                                                \
        for (int64_t x = 0; x < v.inner; ++x)                                                                         \
          out[(o * v.n + (h < pad_lo ? h : v.n - nh + h)) * v.inner + x] = halo[(o * nh + h) * v.inner + x];          \
    return XG_OK;                                                                                                     \
  }                                                                                                                   \
  int xg_gather_##SFX(const R*, const R*, R*, const int64_t*, const int64_t*, const int64_t*, int, const int*,        \
                      const int*, const int64_t*, const int64_t*, int64_t, const R*, int, void*) {                    \
    return unsupported("xg_gather");                                                                                  \
  }

// scans and sums (numpy accumulates integers in 64 bits: no i32 build)
#define XG_HOST_SUMS(SFX, R)                                                                                          \
  int xg_cumsum1d_##SFX(const R* in, R* out, const int64_t* shape, int ndim, int axis, int reverse, int skipna,       \
                        int trim_lo, int trim_hi, int pad_lo, int pad_hi, int bc, R fill, const R* m_in,              \
                        const int64_t* mis, const R* m_out, const int64_t* mos, void*) {                              \
    return cumsum1d<R>(in, out, shape, ndim, axis, reverse, skipna, trim_lo, trim_hi, pad_lo, pad_hi, bc, fill,       \
                       m_in, mis, m_out, mos);                                                                        \
  }                                                                                                                   \
  int xg_reduce1d_##SFX(const R* in, R* out, const int64_t* shape, int ndim, int axis, int skipna, const R* w,        \
                        const int64_t* ws, void*) {                                                                   \
    return reduce1d<R>(in, out, shape, ndim, axis, skipna, w, ws);                                                    \
  }

// the float-only entry points (synthetic generator; fused / transform stubs)
#define XG_HOST_FLOAT(SFX, R)                                                                                         \
  int xg_stencil1d_halo_w_##SFX(int op, const R* in, const R* halo, R* out, const int64_t* shape, int ndim, int axis, \
                                int64_t n_out, int pad_lo, int pad_hi, const R* m_in, const int64_t* mis,             \
                                const R* m_out, const int64_t* mos, void*) {                                          \
    if (!halo && (pad_lo || pad_hi)) return fail(XG_ERR_INVALID, "NULL halo buffer");                                 \
    return stencil1d<R>(op, in, halo, out, shape, ndim, axis, n_out, pad_lo, pad_hi,                                  \
                        (pad_lo || pad_hi) ? XG_BC_HALO : XG_BC_NONE, R(0), m_in, mis, m_out, mos);                   \
  }                                                                                                                   \
  int xg_fill_synthetic_##SFX(R* out, int64_t n, uint64_t seed, uint64_t offset, double scale, double shift, void*) { \
    return fill_synthetic<R>(out, n, seed, offset, scale, shift);                                                     \
  }                                                                                                                   \
  int xg_transform_linear_##SFX(const R*, const R*, const int64_t*, const R*, const int64_t*, int64_t, R*,            \
                                const int64_t*, int, int, int, int, int, void*) {                                     \
    return unsupported("xg_transform_linear");                                                                        \
  }                                                                                                                   \
  int xg_transform_conservative_##SFX(const R*, const R*, const int64_t*, const R*, int64_t, R*, const int64_t*, int, \
                                      int, void*) {                                                                   \
    return unsupported("xg_transform_conservative");                                                                  \
  }                                                                                                                   \
  int xg_vorticity_##SFX(const R* u, const R* v, const R* area, const int64_t* as, R* out, const int64_t* shape,      \
                         int ndim, int bc_x, R fill_x, int bc_y, R fill_y, void*) {                                   \
    return curl_or_div<R>(true, u, v, area, as, out, shape, ndim, bc_x, fill_x, bc_y, fill_y);                        \
  }                                                                                                                   \
  int xg_divergence_##SFX(const R* u, const R* v, const R* area, const int64_t* as, R* out, const int64_t* shape,     \
                          int ndim, int bc_x, R fill_x, int bc_y, R fill_y, void*) {                                  \
    return curl_or_div<R>(false, u, v, area, as, out, shape, ndim, bc_x, fill_x, bc_y, fill_y);                       \
  }                                                                                                                   \
  int xg_gradient_##SFX(const R*, R*, R*, const int64_t*, int, int, R, int, R, const R*, const int64_t*, const R*,    \
                        const int64_t*, void*) {                                                                      \
    return unsupported("xg_gradient");                                                                                \
  }                                                                                                                   \
  int xg_flux_##SFX(const R*, const R*, const R*, R*, R*, const int64_t*, int, int, R, int, R, void*) {               \
    return unsupported("xg_flux");                                                                                    \
  }                                                                                                                   \
  int xg_gradient_halo_##SFX(const R*, const R*, const R*, R*, R*, const int64_t*, int, int, R, int, R, const R*,     \
                             const int64_t*, const R*, const int64_t*, void*) {                                       \
    return unsupported("xg_gradient_halo");                                                                           \
  }                                                                                                                   \
  int xg_flux_halo_##SFX(const R*, const R*, const R*, const R*, const R*, R*, R*, const int64_t*, int, int, R, int,  \
                         R, void*) {                                                                                  \
    return unsupported("xg_flux_halo");                                                                               \
  }                                                                                                                   \
  int xg_vorticity_halo_##SFX(const R*, const R*, const R*, const R*, const R*, const int64_t*, R*, const int64_t*,   \
                              int, int, R, int, R, void*) {                                                           \
    return unsupported("xg_vorticity_halo");                                                                          \
  }                                                                                                                   \
  int xg_divergence_halo_##SFX(const R*, const R*, const R*, const R*, const R*, const int64_t*, R*, const int64_t*,  \
                               int, int, R, int, R, void*) {                                                          \
    return unsupported("xg_divergence_halo");                                                                         \
  }                                                                                                                   \
  int xg_flux_divergence_##SFX(const R* u, const R* v, const R* t, const R* area, const int64_t* as, R* out,            \
                               const int64_t* shape, int ndim, int bc_x, R fill_x, int bc_y, R fill_y, void*) {         \
    return div2d<R>(1, t, u, v, nullptr, nullptr, area, as, out, shape, ndim, bc_x, fill_x, bc_y, fill_y);              \
  }                                                                                                                   \
  int xg_flux_divergence3d_##SFX(const R* u, const R* v, const R* w, const R* t, const R* vol, const int64_t* vs,       \
                                 const R* vol2, const int64_t* vs2, R* out, const int64_t* shape, int ndim, int bc_x,  \
                                 R fill_x, int bc_y, R fill_y, int bc_z, R fill_z, void*) {                            \
    return div3d<R>(u, v, w, t, vol, vs, vol2, vs2, out, shape, ndim, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z);     \
  }                                                                                                                   \
  int xg_vertical_velocity_##SFX(const R* u, const R* v, const R* mu, const int64_t* mus, const R* mu2,               \
                                 const int64_t* mu2s, const R* mv, const int64_t* mvs, const R* mv2,                   \
                                 const int64_t* mv2s, const R* area, const int64_t* as, R* out, const int64_t* shape,  \
                                 int ndim, int bc_x, R fill_x, int bc_y, R fill_y, int bc_z, R fill_z, int reverse,    \
                                 void*) {                                                                              \
    const R* const met[5] = {mu, mu2, mv, mv2, area};                                                                 \
    const int64_t* const ms[5] = {mus, mu2s, mvs, mv2s, as};                                                          \
    return wcont<R>(u, v, met, ms, out, shape, ndim, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z, reverse);             \
  }                                                                                                                   \
  int xg_hydrostatic_pressure_gradient_##SFX(const R* b, const R* w, const int64_t* ws, const R* dxC,                 \
                                             const int64_t* dxCs, const R* dyC, const int64_t* dyCs, R* out_x,         \
                                             R* out_y, const int64_t* shape, int ndim, int bc_x, R fill_x, int bc_y,   \
                                             R fill_y, int bc_z, R fill_z, void*) {                                    \
    const R* const met[3] = {w, dxC, dyC};                                                                            \
    const int64_t* const ms[3] = {ws, dxCs, dyCs};                                                                    \
    return pgrad<R>(b, met, ms, out_x, out_y, shape, ndim, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z);                \
  }                                                                                                                   \
  int xg_vertical_momentum_advection_##SFX(const R* u, const R* v, const R* w, const R* mu, const int64_t* mus,       \
                                           const R* mv, const int64_t* mvs, R* out_u, R* out_v, const int64_t* shape, \
                                           int ndim, int bc_x, R fill_x, int bc_y, R fill_y, int bc_z, R fill_z,      \
                                           void*) {                                                                    \
    const R* const met[2] = {mu, mv};                                                                                 \
    const int64_t* const ms[2] = {mus, mvs};                                                                          \
    return vmomadv<R>(u, v, w, met, ms, out_u, out_v, shape, ndim, bc_x, fill_x, bc_y, fill_y, bc_z, fill_z);        \
  }                                                                                                                   \
  int xg_kinetic_energy_##SFX(const R* u, const R* v, R* out, const int64_t* shape, int ndim, int bc_x, R fill_x,     \
                              int bc_y, R fill_y, void*) {                                                            \
    const R* const met[4] = {nullptr, nullptr, nullptr, nullptr};                                                     \
    const int64_t* const ms[4] = {nullptr, nullptr, nullptr, nullptr};                                                \
    return momentum<R>(true, u, v, met, ms, out, nullptr, shape, ndim, bc_x, fill_x, bc_y, fill_y);                   \
  }                                                                                                                   \
  int xg_momentum_advection_##SFX(const R* u, const R* v, const R* cor, const int64_t* cors, const R* rAz,            \
                                  const int64_t* rAzs, const R* dxC, const int64_t* dxCs, const R* dyC,               \
                                  const int64_t* dyCs, R* out_u, R* out_v, const int64_t* shape, int ndim, int bc_x,  \
                                  R fill_x, int bc_y, R fill_y, void*) {                                              \
    const R* const met[4] = {rAz, cor, dxC, dyC};                                                                     \
    const int64_t* const ms[4] = {rAzs, cors, dxCs, dyCs};                                                            \
    return momentum<R>(false, u, v, met, ms, out_u, out_v, shape, ndim, bc_x, fill_x, bc_y, fill_y);                  \
  }                                                                                                                   \
  int xg_horizontal_viscosity_##SFX(const R* u, const R* v, const R* rA, const int64_t* rAs, const R* rAz,             \
                                    const int64_t* rAzs, const R* dxC, const int64_t* dxCs, const R* dyC,              \
                                    const int64_t* dyCs, const R* dyG, const int64_t* dyGs, const R* dxG,              \
                                    const int64_t* dxGs, const R* nud, const int64_t* nuds, const R* nuz,              \
                                    const int64_t* nuzs, R* out_u, R* out_v, const int64_t* shape, int ndim, int bc_x, \
                                    R fill_x, R zfill_x, int bc_y, R fill_y, R zfill_y, void*) {                       \
    const R* const pl[8] = {rA, rAz, dxC, dyC, dyG, dxG, nud, nuz};                                                   \
    const int64_t* const ps[8] = {rAs, rAzs, dxCs, dyCs, dyGs, dxGs, nuds, nuzs};                                     \
    return hvisc<R>(u, v, pl, ps, out_u, out_v, shape, ndim, bc_x, fill_x, zfill_x, bc_y, fill_y, zfill_y);           \
  }                                                                                                                   \
  int xg_laplacian_##SFX(const R* a, const R* dxC, const int64_t* dxCs, const R* dyC, const int64_t* dyCs, const R* dyG, \
                         const int64_t* dyGs, const R* dxG, const int64_t* dxGs, const R* area, const int64_t* as,     \
                         R* out, const int64_t* shape, int ndim, int bc_x, R fill_x, int bc_y, R fill_y, void*) {       \
    const R* const met[4] = {dxC, dyG, dyC, dxG};                                                                     \
    const int64_t* const ms[4] = {dxCs, dyGs, dyCs, dxGs};                                                            \
    return div2d<R>(0, a, nullptr, nullptr, met, ms, area, as, out, shape, ndim, bc_x, fill_x, bc_y, fill_y);         \
  }                                                                                                                   \
  int xg_stencil2d_##SFX(int, const R*, R*, const int64_t*, int, int, int, int, int, R, int, int, int, R, void*) {    \
    return unsupported("xg_stencil2d");                                                                               \
  }                                                                                                                   \
  int xg_stencil2d_metric_##SFX(int, const R*, R*, const int64_t*, int, int, int, int, int, R, int, int, int, R,      \
                                const R*, const R*, const R*, void*) {                                                \
    return unsupported("xg_stencil2d_metric");                                                                        \
  }

XG_HOST_LANES(f64, double)
XG_HOST_LANES(f32, float)
XG_HOST_LANES(i64, int64_t)  // built with -fwrapv: overflow wraps like numpy's integer arithmetic
XG_HOST_LANES(i32, int32_t)
XG_HOST_SUMS(f64, double)
XG_HOST_SUMS(f32, float)
XG_HOST_SUMS(i64, int64_t)
XG_HOST_FLOAT(f64, double)
XG_HOST_FLOAT(f32, float)

// strided N-d copy (see the header): an odometer over the index space, bytes moved with memcpy
int xg_copy_nd(const void* src, const int64_t* ss, void* dst, const int64_t* ds, const int64_t* shape, int ndim, int eb, void*) {
  if (!shape || !ss || !ds) return fail(XG_ERR_INVALID, "NULL shape / stride argument");
  if (ndim < 0 || ndim > XG_MAX_NDIM) return fail(XG_ERR_INVALID, "ndim %d not in [0,%d]", ndim, XG_MAX_NDIM);
  if (eb != 1 && eb != 2 && eb != 4 && eb != 8) return fail(XG_ERR_INVALID, "element size %d not 1, 2, 4 or 8", eb);
  int64_t total = 1;
  for (int d = 0; d < ndim; ++d) {
    if (shape[d] < 0) return fail(XG_ERR_INVALID, "negative extent");
    if (shape[d] > 1 && ds[d] < 0) return fail(XG_ERR_INVALID, "destination strides must be positive");
    if (shape[d] > 1 && ds[d] == 0) return fail(XG_ERR_INVALID, "destination stride 0 on a dim of extent %lld (cells written more than once)", (long long)shape[d]);
    total *= shape[d];
  }
  if (total == 0) return XG_OK;
  if (!src || !dst) return fail(XG_ERR_INVALID, "NULL array argument");
  int64_t idx[XG_MAX_NDIM] = {0};
  const char* s = static_cast<const char*>(src);
  char* o = static_cast<char*>(dst);
  for (int64_t i = 0; i < total; ++i) {
    int64_t so = 0, dof = 0;
    for (int d = 0; d < ndim; ++d) { so += idx[d] * ss[d]; dof += idx[d] * ds[d]; }
    memcpy(o + dof * eb, s + so * eb, (size_t)eb);
    for (int d = ndim - 1; d >= 0; --d) {
      if (++idx[d] < shape[d]) break;
      idx[d] = 0;
    }
  }
  return XG_OK;
}

// numpy `astype` between the storage dtype and the compute dtype (see the header); one element at a time
// IEEE binary16 <-> double without compiler support (gcc 11 has no _Float16): one round-to-nearest-even from the double
static uint16_t half_from_double(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  const uint16_t sign = (uint16_t)((b >> 48) & 0x8000u);
  int64_t e = (int64_t)((b >> 52) & 0x7ff);
  uint64_t m = b & 0xfffffffffffffull;
  if (e == 0x7ff) return (uint16_t)(sign | 0x7c00u | (m ? (0x200u | (uint16_t)(m >> 42)) : 0u));  // inf / quiet NaN
  e = e - 1023 + 15;
  if (e >= 31) return (uint16_t)(sign | 0x7c00u);
  int shift = 42;
  if (e <= 0) {  // subnormal half (or zero): the implicit one joins the mantissa, the shift grows
    if (e < -10) return sign;
    m |= 1ull << 52;
    shift = 42 + (int)(1 - e);
    e = 0;
  }
  uint64_t q = m >> shift;
  const uint64_t rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
  if (rem > half || (rem == half && (q & 1))) ++q;  // a carry out of the mantissa bumps the exponent (up to inf): correct
  return (uint16_t)(sign | (uint16_t)(((uint64_t)e << 10) + q));
}
static double half_to_double(uint16_t h) {
  const int e = (h >> 10) & 31, m = h & 0x3ff;
  double v;
  if (e == 0) v = std::ldexp((double)m, -24);
  else if (e == 31) v = m ? NAN : INFINITY;
  else v = std::ldexp((double)(m | 0x400), e - 25);
  return (h & 0x8000) ? -v : v;
}
int xg_stencil_multi(int dtype, const void* in, const int64_t* shape, int ndim, int n, const xg_multi_desc* desc, void*) {
  if (dtype == XG_T_F64) return stencil_multi<double>((const double*)in, shape, ndim, n, desc);
  if (dtype == XG_T_F32) return stencil_multi<float>((const float*)in, shape, ndim, n, desc);
  return fail(XG_ERR_INVALID, "stencil multi: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}
int xg_vertical_diffusion(int dtype, const void* a, const void* kappa, const int64_t* ks, const void* mf, const int64_t* mfs,
                          const void* mc, const int64_t* mcs, void* out, const int64_t* shape, int ndim, int outer, int bc_z,
                          double fill_z, void*) {
  const int64_t* const st[3] = {ks, mfs, mcs};
  if (dtype == XG_T_F64) {
    const double* const arr[3] = {(const double*)kappa, (const double*)mf, (const double*)mc};
    return vdiff<double>((const double*)a, arr, st, (double*)out, shape, ndim, outer, bc_z, fill_z);
  }
  if (dtype == XG_T_F32) {
    const float* const arr[3] = {(const float*)kappa, (const float*)mf, (const float*)mc};
    return vdiff<float>((const float*)a, arr, st, (float*)out, shape, ndim, outer, bc_z, (float)fill_z);
  }
  return fail(XG_ERR_INVALID, "vertical diffusion: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}

int xg_implicit_vertical_diffusion(int dtype, const void* a, const void* kappa, const int64_t* ks, const void* mf,
                                   const int64_t* mfs, const void* mc, const int64_t* mcs, void* work, void* out,
                                   const int64_t* shape, int ndim, int outer, double dt, void*) {
  if (!(dt >= 0.0) || !std::isfinite(dt)) return fail(XG_ERR_INVALID, "implicit vertical diffusion: dt %g is negative or not finite", dt);
  const int64_t* const st[3] = {ks, mfs, mcs};
  if (dtype == XG_T_F64) {
    const double* const arr[3] = {(const double*)kappa, (const double*)mf, (const double*)mc};
    return vimpl<double>((const double*)a, arr, st, (double*)work, (double*)out, shape, ndim, outer, dt);
  }
  if (dtype == XG_T_F32) {
    const float* const arr[3] = {(const float*)kappa, (const float*)mf, (const float*)mc};
    return vimpl<float>((const float*)a, arr, st, (float*)work, (float*)out, shape, ndim, outer, (float)dt);
  }
  return fail(XG_ERR_INVALID, "implicit vertical diffusion: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}

int xg_richardson_number(int dtype, const void* b, const void* u, const void* v, const void* mu, const int64_t* mus,
                         const void* mv, const int64_t* mvs, const void* mb, const int64_t* mbs, void* out,
                         const int64_t* shape, int ndim, int outer, int bc_x, double fill_x, int bc_y, double fill_y, int bc_z,
                         double fill_z, void*) {
  const int64_t* const st[3] = {mus, mvs, mbs};
  const int bc[3] = {bc_x, bc_y, bc_z};
  if (dtype == XG_T_F64) {
    const double* const arr[3] = {(const double*)mu, (const double*)mv, (const double*)mb};
    const double fill[3] = {fill_x, fill_y, fill_z};
    return richardson<double>((const double*)b, (const double*)u, (const double*)v, arr, st, (double*)out, shape, ndim, outer,
                              bc, fill);
  }
  if (dtype == XG_T_F32) {
    const float* const arr[3] = {(const float*)mu, (const float*)mv, (const float*)mb};
    const float fill[3] = {(float)fill_x, (float)fill_y, (float)fill_z};
    return richardson<float>((const float*)b, (const float*)u, (const float*)v, arr, st, (float*)out, shape, ndim, outer, bc,
                             fill);
  }
  return fail(XG_ERR_INVALID, "richardson number: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}

int xg_implicit_vertical_viscosity(int dtype, const void* u, const void* v, const void* nu, const int64_t* nus, const void* mfu,
                                   const int64_t* mfus, const void* mcu, const int64_t* mcus, const void* mfv, const int64_t* mfvs,
                                   const void* mcv, const int64_t* mcvs, void* work_u, void* work_v, void* out_u, void* out_v,
                                   const int64_t* shape, int ndim, int outer, int bc_x, double fill_x, int bc_y, double fill_y,
                                   double dt, void*) {
  if (!(dt >= 0.0) || !std::isfinite(dt)) return fail(XG_ERR_INVALID, "implicit vertical viscosity: dt %g is negative or not finite", dt);
  const void* const met[4] = {mfu, mcu, mfv, mcv};
  const int64_t* const ms[4] = {mfus, mcus, mfvs, mcvs};
  if (dtype == XG_T_F64)
    return vvisc<double>((const double*)u, (const double*)v, (const double*)nu, nus, met, ms, (double*)work_u, (double*)work_v,
                         (double*)out_u, (double*)out_v, shape, ndim, outer, bc_x, fill_x, bc_y, fill_y, dt);
  if (dtype == XG_T_F32)
    return vvisc<float>((const float*)u, (const float*)v, (const float*)nu, nus, met, ms, (float*)work_u, (float*)work_v,
                        (float*)out_u, (float*)out_v, shape, ndim, outer, bc_x, (float)fill_x, bc_y, (float)fill_y, (float)dt);
  return fail(XG_ERR_INVALID, "implicit vertical viscosity: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}

int xg_richardson_mixing(int dtype, const void* b, const void* u, const void* v, const void* mu, const int64_t* mus,
                         const void* mv, const int64_t* mvs, const void* mb, const int64_t* mbs, double nu0, double alpha,
                         double nu_b, double kappa_b, double shear_floor, void* out_nu, void* out_kappa, const int64_t* shape,
                         int ndim, int outer, int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void*) {
  const int64_t* const st[3] = {mus, mvs, mbs};
  const int bc[3] = {bc_x, bc_y, bc_z};
  if (!b || !out_nu || !out_kappa) return fail(XG_ERR_INVALID, "NULL array argument");
  if (dtype == XG_T_F64) {
    const double* const arr[3] = {(const double*)mu, (const double*)mv, (const double*)mb};
    const double fill[3] = {fill_x, fill_y, fill_z}, clo[5] = {nu0, alpha, nu_b, kappa_b, shear_floor};
    return richardson<double>((const double*)b, (const double*)u, (const double*)v, arr, st, (double*)out_nu, shape, ndim,
                              outer, bc, fill, clo, (double*)out_kappa);
  }
  if (dtype == XG_T_F32) {
    const float* const arr[3] = {(const float*)mu, (const float*)mv, (const float*)mb};
    const float fill[3] = {(float)fill_x, (float)fill_y, (float)fill_z};
    const float clo[5] = {(float)nu0, (float)alpha, (float)nu_b, (float)kappa_b, (float)shear_floor};
    return richardson<float>((const float*)b, (const float*)u, (const float*)v, arr, st, (float*)out_nu, shape, ndim, outer, bc,
                             fill, clo, (float*)out_kappa);
  }
  return fail(XG_ERR_INVALID, "richardson mixing: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}

int xg_isopycnal_slope(int dtype, const void* b, const void* mx, const int64_t* mxs, const void* my, const int64_t* mys,
                       const void* mz, const int64_t* mzs, void* out_x, void* out_y, const int64_t* shape, int ndim, int outer,
                       int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void*) {
  const int64_t* const st[3] = {mxs, mys, mzs};
  const int bc[3] = {bc_x, bc_y, bc_z};
  if (dtype == XG_T_F64) {
    const double* const arr[3] = {(const double*)mx, (const double*)my, (const double*)mz};
    const double fill[3] = {fill_x, fill_y, fill_z};
    return islope<double>((const double*)b, arr, st, (double*)out_x, (double*)out_y, shape, ndim, outer, bc, fill);
  }
  if (dtype == XG_T_F32) {
    const float* const arr[3] = {(const float*)mx, (const float*)my, (const float*)mz};
    const float fill[3] = {(float)fill_x, (float)fill_y, (float)fill_z};
    return islope<float>((const float*)b, arr, st, (float*)out_x, (float*)out_y, shape, ndim, outer, bc, fill);
  }
  return fail(XG_ERR_INVALID, "isopycnal slope: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}

int xg_redi_tensor(int dtype, const void* b, const void* mx, const int64_t* mxs, const void* my, const int64_t* mys,
                   const void* mz, const int64_t* mzs, double kappa, double slope_max2, int taper, void* out_x, void* out_y,
                   void* out_z, const int64_t* shape, int ndim, int outer, int bc_x, double fill_x, int bc_y, double fill_y,
                   int bc_z, double fill_z, void*) {
  const int64_t* const st[3] = {mxs, mys, mzs};
  const int bc[3] = {bc_x, bc_y, bc_z};
  if (dtype == XG_T_F64) {
    const double* const arr[3] = {(const double*)mx, (const double*)my, (const double*)mz};
    const double fill[3] = {fill_x, fill_y, fill_z};
    return reditensor<double>((const double*)b, arr, st, kappa, slope_max2, taper, (double*)out_x, (double*)out_y,
                              (double*)out_z, shape, ndim, outer, bc, fill);
  }
  if (dtype == XG_T_F32) {
    const float* const arr[3] = {(const float*)mx, (const float*)my, (const float*)mz};
    const float fill[3] = {(float)fill_x, (float)fill_y, (float)fill_z};
    return reditensor<float>((const float*)b, arr, st, (float)kappa, (float)slope_max2, taper, (float*)out_x, (float*)out_y,
                             (float*)out_z, shape, ndim, outer, bc, fill);
  }
  return fail(XG_ERR_INVALID, "redi tensor: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}

int xg_redi_vertical_flux_divergence(int dtype, const void* a, const void* kwx, const void* kwy, const void* mx,
                                     const int64_t* mxs, const void* my, const int64_t* mys, const void* mc, const int64_t* mcs,
                                     void* out, const int64_t* shape, int ndim, int outer, int closed, int bc_x, double fill_x,
                                     int bc_y, double fill_y, int bc_z, double fill_z, void*) {
  const int64_t* const st[3] = {mxs, mys, mcs};
  const int bc[3] = {bc_x, bc_y, bc_z};
  if (dtype == XG_T_F64) {
    const double* const arr[3] = {(const double*)mx, (const double*)my, (const double*)mc};
    const double fill[3] = {fill_x, fill_y, fill_z};
    return rediflux<double>((const double*)a, (const double*)kwx, (const double*)kwy, arr, st, (double*)out, shape, ndim, outer,
                            closed, bc, fill);
  }
  if (dtype == XG_T_F32) {
    const float* const arr[3] = {(const float*)mx, (const float*)my, (const float*)mc};
    const float fill[3] = {(float)fill_x, (float)fill_y, (float)fill_z};
    return rediflux<float>((const float*)a, (const float*)kwx, (const float*)kwy, arr, st, (float*)out, shape, ndim, outer,
                           closed, bc, fill);
  }
  return fail(XG_ERR_INVALID, "redi vertical flux divergence: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}

int xg_bolus_velocity(int dtype, const void* kwx, const void* kwy, const void* mzu, const int64_t* mzus, const void* mzv,
                      const int64_t* mzvs, const void* dyG, const int64_t* dyGs, const void* dxG, const int64_t* dxGs,
                      const void* rA, const int64_t* rAs, void* out_u, void* out_v, void* out_w, const int64_t* shape, int ndim,
                      int outer, int closed, int bc_x, double fill_x, int bc_y, double fill_y, int bc_z, double fill_z, void*) {
  const int64_t* const st[5] = {mzus, mzvs, dyGs, dxGs, rAs};
  const int bc[3] = {bc_x, bc_y, bc_z};
  if (dtype == XG_T_F64) {
    const double* const arr[5] = {(const double*)mzu, (const double*)mzv, (const double*)dyG, (const double*)dxG, (const double*)rA};
    const double fill[3] = {fill_x, fill_y, fill_z};
    return bolus<double>((const double*)kwx, (const double*)kwy, arr, st, (double*)out_u, (double*)out_v, (double*)out_w, shape,
                         ndim, outer, closed, bc, fill);
  }
  if (dtype == XG_T_F32) {
    const float* const arr[5] = {(const float*)mzu, (const float*)mzv, (const float*)dyG, (const float*)dxG, (const float*)rA};
    const float fill[3] = {(float)fill_x, (float)fill_y, (float)fill_z};
    return bolus<float>((const float*)kwx, (const float*)kwy, arr, st, (float*)out_u, (float*)out_v, (float*)out_w, shape, ndim,
                        outer, closed, bc, fill);
  }
  return fail(XG_ERR_INVALID, "bolus velocity: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}

int xg_redi_horizontal_tensor(int dtype, const void* b, const void* mx, const int64_t* mxs, const void* my, const int64_t* mys,
                              const void* mz, const int64_t* mzs, double kappa, double slope_max2, int taper, void* out_u,
                              void* out_v, const int64_t* shape, int ndim, int outer, int bc_x, double fill_x, int bc_y,
                              double fill_y, int bc_z, double fill_z, void*) {
  const int64_t* const st[3] = {mxs, mys, mzs};
  const int bc[3] = {bc_x, bc_y, bc_z};
  if (dtype == XG_T_F64) {
    const double* const arr[3] = {(const double*)mx, (const double*)my, (const double*)mz};
    const double fill[3] = {fill_x, fill_y, fill_z};
    return rediuv<double>((const double*)b, arr, st, kappa, slope_max2, taper, (double*)out_u, (double*)out_v, shape, ndim, outer,
                          bc, fill);
  }
  if (dtype == XG_T_F32) {
    const float* const arr[3] = {(const float*)mx, (const float*)my, (const float*)mz};
    const float fill[3] = {(float)fill_x, (float)fill_y, (float)fill_z};
    return rediuv<float>((const float*)b, arr, st, (float)kappa, (float)slope_max2, taper, (float*)out_u, (float*)out_v, shape,
                         ndim, outer, bc, fill);
  }
  return fail(XG_ERR_INVALID, "redi horizontal tensor: element type %d is neither XG_T_F64 nor XG_T_F32", dtype);
}

int xg_convert(const void* src, int st, void* dst, int dt, uint64_t n, int via, double scale, int flags, void*) {
  if (st < XG_T_BOOL || st > XG_T_F16 || dt < XG_T_BOOL || dt > XG_T_F16) return fail(XG_ERR_INVALID, "unknown element type (%d -> %d)", st, dt);
  if (via < -1 || via > XG_T_U64) return fail(XG_ERR_INVALID, "via_type %d is not an integer type", via);
  if (flags & ~1) return fail(XG_ERR_INVALID, "unknown flags %d", flags);
  if (n == 0) return XG_OK;
  if (!src || !dst) return fail(XG_ERR_INVALID, "NULL array argument");
  const bool sf = st >= XG_T_F32, df = dt >= XG_T_F32;
  if (sf && via != -1) return fail(XG_ERR_INVALID, "via_type applies to integer sources only");
  auto bytes = [](int t) { return (t == XG_T_BOOL || t == XG_T_I8 || t == XG_T_U8) ? 1 : (t == XG_T_I16 || t == XG_T_U16 || t == XG_T_F16) ? 2 : (t == XG_T_I32 || t == XG_T_U32 || t == XG_T_F32) ? 4 : 8; };
  if ((flags & 1) && (bytes(st) != 8 || bytes(dt) != 8 || sf || df)) return fail(XG_ERR_INVALID, "the sign-bit flip needs 64-bit integer types on both sides");
  auto wrap = [](int64_t w, int t) -> int64_t {
    switch (t) {
      case XG_T_BOOL: return w != 0;
      case XG_T_I8: return (int8_t)w;   case XG_T_I16: return (int16_t)w;  case XG_T_I32: return (int32_t)w;
      case XG_T_U8: return (uint8_t)w;  case XG_T_U16: return (uint16_t)w; case XG_T_U32: return (uint32_t)w;
      default: return w;
    }
  };
  const int logical = via != -1 ? via : st;
  for (uint64_t i = 0; i < n; ++i) {
    int64_t w = 0;
    double f = 0.0;
    switch (st) {  // load
      case XG_T_BOOL: w = ((const uint8_t*)src)[i] != 0; break;
      case XG_T_I8: w = ((const int8_t*)src)[i]; break;     case XG_T_I16: w = ((const int16_t*)src)[i]; break;
      case XG_T_I32: w = ((const int32_t*)src)[i]; break;   case XG_T_I64: w = ((const int64_t*)src)[i]; break;
      case XG_T_U8: w = ((const uint8_t*)src)[i]; break;    case XG_T_U16: w = ((const uint16_t*)src)[i]; break;
      case XG_T_U32: w = ((const uint32_t*)src)[i]; break;  case XG_T_U64: w = (int64_t)((const uint64_t*)src)[i]; break;
      case XG_T_F32: f = ((const float*)src)[i]; break;     case XG_T_F16: f = half_to_double(((const uint16_t*)src)[i]); break;
      default: f = ((const double*)src)[i]; break;
    }
    if (!sf) w = wrap(w, via);
    if (df) {  // float destination
      if (dt == XG_T_F16) {  // one rounding into binary16, then the scale in binary16 (a power of two: exact unless subnormal)
        const double v = sf ? f : (logical == XG_T_U64 ? (double)(uint64_t)w : (double)w);
        const uint16_t h = half_from_double(v);
        ((uint16_t*)dst)[i] = scale == 1.0 ? h : half_from_double(half_to_double(h) * half_to_double(half_from_double(scale)));
      } else if (dt == XG_T_F32) {
        const float v = sf ? (float)f : (logical == XG_T_U64 ? (float)(uint64_t)w : (float)w);
        ((float*)dst)[i] = v * (float)scale;
      } else {
        const double v = sf ? f : (logical == XG_T_U64 ? (double)(uint64_t)w : (double)w);
        ((double*)dst)[i] = v * scale;
      }
      continue;
    }
    if (sf) w = (dt == XG_T_U64) ? (int64_t)(uint64_t)f : (int64_t)f;
    if (dt == XG_T_BOOL) { ((uint8_t*)dst)[i] = sf ? (f != 0.0) : (w != 0); continue; }
    if (flags & 1) w ^= (int64_t)0x8000000000000000ull;
    switch (dt) {
      case XG_T_I8: ((int8_t*)dst)[i] = (int8_t)w; break;     case XG_T_I16: ((int16_t*)dst)[i] = (int16_t)w; break;
      case XG_T_I32: ((int32_t*)dst)[i] = (int32_t)w; break;  case XG_T_I64: ((int64_t*)dst)[i] = w; break;
      case XG_T_U8: ((uint8_t*)dst)[i] = (uint8_t)w; break;   case XG_T_U16: ((uint16_t*)dst)[i] = (uint16_t)w; break;
      case XG_T_U32: ((uint32_t*)dst)[i] = (uint32_t)w; break; default: ((uint64_t*)dst)[i] = (uint64_t)w; break;
    }
  }
  return XG_OK;
}

}  // extern "C"
