"""A C-grid built from a smooth analytic map, and fields that carry their exact derivatives.  A HELPER, not a test.

Every metric of `tests/test_convergence.py` is geometry, none is random: the map is separable,

    x = xi + ex sin(xi),  y = eta + ey sin(eta)   on [0, 2 pi), periodic,        z = s + cz s (1 - s)   on [0, 1], closed,

cell i of an axis spans xi in [i, i + 1) * 2 pi / n, the `left` point XG[i] is x(i d), the centre XC[i] is x((i + 1/2) d); along
Z the faces are s = k / nz, ZL the first nz of them, ZO all nz + 1, ZC the map of the half indices.  The metrics are MITgcm's
set, each a difference (or a product of differences) of MAP VALUES at the points it lies between:

    dxC(YC, XG)[i] = x(XC[i]) - x(XC[i-1])    the distance between centres, at the u point     (+ 2 pi at the wrap)
    dxG(YG, XC)[i] = x(XG[i+1]) - x(XG[i])    the length of the cell's southern edge, at the v point
    dyC(YG, XC), dyG(YC, XG)                  the same along Y
    rA (YC, XC) = dxG dyG   rAz(YG, XG) = dxC dyC   rAw(YC, XG) = dxC dyG   rAs(YG, XC) = dxG dyC
    drF(ZC)[k]  = z(ZO[k+1]) - z(ZO[k])       the thickness of level k
    drC(ZL | ZO)[k] = z(ZC[k]) - z(ZC[k-1])   the distance between levels; the outermost ones are the half cells

and all are registered with `Grid(..., metrics=...)` the way a user registers them: an operator finds its metric through
`Grid.get_metric`, no test hands it an array.  The map is separable, so dxC and dxG hold the same function of xi sampled half
a cell apart: registering one in the other's place (`swap`) is a first-order error in the metric, which is what the liveness
cases of the convergence tests rely on.

Fields are sums of products X(x) Y(y) Z(z) of one-variable functions (`Trig`, `Poly`) that know their own derivatives and
their integral from 0, so that no derivative of a field is written by hand; `check_derivatives` still compares each with a
fourth-order central difference of the field itself."""

import numpy as np

from xgcm_amd import DataArray, Dataset, Grid

TWO_PI = 2.0 * np.pi
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
        "Z": {"center": "ZC", "left": "ZL", "outer": "ZO"}}
# name -> (axes it is registered under, dims)
METRIC_DIMS = {"dxC": (("X",), ("YC", "XG")), "dxG": (("X",), ("YG", "XC")), "dyC": (("Y",), ("YG", "XC")),
               "dyG": (("Y",), ("YC", "XG")), "rA": (("X", "Y"), ("YC", "XC")), "rAz": (("X", "Y"), ("YG", "XG")),
               "rAw": (("X", "Y"), ("YC", "XG")), "rAs": (("X", "Y"), ("YG", "XC")), "drF": (("Z",), ("ZC",)),
               "drCl": (("Z",), ("ZL",)), "drCo": (("Z",), ("ZO",))}
Z_FIXED = 0.37   # where a field is evaluated for an array without a Z dim


# ---- one-variable functions --------------------------------------------------------------------------------------------
class Trig:
    """amp sin(k s + phase); n-th derivative for n >= 0, the integral from 0 for n = -1"""

    def __init__(self, k, phase=0.0, amp=1.0):
        self.k, self.phase, self.amp = float(k), float(phase), float(amp)

    def __call__(self, s, n=0):
        s = np.asarray(s, np.float64)
        if n == -1:
            return -(self.amp / self.k) * (np.cos(self.k * s + self.phase) - np.cos(self.phase))
        return self.amp * self.k ** n * np.sin(self.k * s + self.phase + n * (np.pi / 2))


def Sin(k, amp=1.0):
    return Trig(k, 0.0, amp)


def Cos(k, amp=1.0):
    return Trig(k, np.pi / 2, amp)


class Poly:
    """c[0] + c[1] s + c[2] s^2 ...; n-th derivative for n >= 0, the integral from 0 for n = -1"""

    def __init__(self, *c):
        self.p = np.polynomial.Polynomial(np.asarray(c, np.float64))

    def __call__(self, s, n=0):
        s = np.asarray(s, np.float64)
        p = self.p.integ() if n == -1 else (self.p.deriv(n) if n > 0 else self.p)
        return p(s) + np.zeros_like(s)


ONE = Poly(1.0)


class Field:
    """sum of Z(z) Y(y) X(x); `terms`: (fz, fy, fx) triples.  `f(z, y, x, d=(dz, dy, dx))` is the mixed derivative of those
    orders (-1: the integral from 0 along that coordinate) on the tensor grid of the three 1-D coordinate arrays"""

    def __init__(self, *terms):
        self.terms = terms

    def __call__(self, z, y, x, d=(0, 0, 0)):
        z, y, x = (np.asarray(c, np.float64) for c in (z, y, x))
        out = 0.0
        for fz, fy, fx in self.terms:
            out = out + fz(z, d[0])[:, None, None] * fy(y, d[1])[None, :, None] * fx(x, d[2])[None, None, :]
        return out

    def __add__(self, other):
        return Field(*(self.terms + other.terms))


def check_derivatives(field, orders=((1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, 2), (0, 1, 1), (1, 0, 1),
                                     (1, 1, 0)), step=1e-3, npoints=4, seed=7):
    """the largest difference, relative to the derivative's own max-norm over the sample, between each stated derivative and
    a fourth-order central difference (step 1e-3) of the derivative one order lower, at npoints^3 interior points; the
    difference formula's own error is about step^4 |f^(5)| / 30 ~ 1e-12 |f| k^5 and its rounding about 1e-16 |f| / step"""
    rng = np.random.default_rng(seed)
    z = 0.1 + 0.8 * rng.random(npoints)
    y, x = TWO_PI * rng.random(npoints), TWO_PI * rng.random(npoints)
    worst = 0.0
    for d in orders:
        ax = max(range(3), key=lambda a: d[a])
        lower = tuple(n - (a == ax) for a, n in enumerate(d))
        pts = [z, y, x]

        def at(shift):
            p = list(pts)
            p[ax] = p[ax] + shift
            return field(*p, d=lower)

        fd = (-at(2 * step) + 8 * at(step) - 8 * at(-step) + at(-2 * step)) / (12 * step)
        want = field(z, y, x, d=d)
        worst = max(worst, float(np.abs(fd - want).max() / max(np.abs(want).max(), 1.0)))
    return worst


# ---- the grid ----------------------------------------------------------------------------------------------------------
class AnalyticGrid:
    """`n`: points per axis, or (nz, ny, nx).  `ex`, `ey`, `cz`: the stretching (0: uniform).  `swap` {name: other}: the
    variant builder -- metric `name` is registered, under its own name and dims, with the VALUES of `other` (a metric of
    another position; a Z metric of another length is cut or continued with its last value); the product is not touched.
    `omit`: metric names not to register at all (no `rA`: `get_metric` forms an area from dx * dy)."""

    def __init__(self, n, ex=0.3, ey=0.25, cz=0.5, dtype=np.float64, swap=None, omit=(), padding=None):
        self.nz, self.ny, self.nx = (n, n, n) if np.isscalar(n) else n
        self.ex, self.ey, self.cz, self.dtype = ex, ey, cz, np.dtype(dtype)
        self.swap, self.omit = dict(swap or {}), tuple(omit)
        nz, ny, nx = self.nz, self.ny, self.nx
        self.xmap = lambda xi: xi + ex * np.sin(xi)            # noqa: E731
        self.ymap = lambda eta: eta + ey * np.sin(eta)         # noqa: E731
        self.zmap = lambda s: s + cz * s * (1.0 - s)           # noqa: E731
        dxi, deta = TWO_PI / nx, TWO_PI / ny
        self.pts = {"XG": self.xmap(np.arange(nx) * dxi), "XC": self.xmap((np.arange(nx) + 0.5) * dxi),
                    "YG": self.ymap(np.arange(ny) * deta), "YC": self.ymap((np.arange(ny) + 0.5) * deta),
                    "ZO": self.zmap(np.arange(nz + 1) / nz), "ZC": self.zmap((np.arange(nz) + 0.5) / nz)}
        self.pts["ZL"] = self.pts["ZO"][:nz]
        p = self.pts
        # one-dimensional factors: distances between centres (at the left points) and between left points (at the centres)
        dxc = p["XC"] - np.roll(p["XC"], 1)
        dxc[0] += TWO_PI
        dxg = np.roll(p["XG"], -1) - p["XG"]
        dxg[-1] += TWO_PI
        dyc = p["YC"] - np.roll(p["YC"], 1)
        dyc[0] += TWO_PI
        dyg = np.roll(p["YG"], -1) - p["YG"]
        dyg[-1] += TWO_PI
        row, col = (lambda a: np.broadcast_to(a[None, :], (ny, nx)).copy()), (lambda a: np.broadcast_to(a[:, None], (ny, nx)).copy())
        drc = np.diff(np.concatenate([p["ZO"][:1], p["ZC"], p["ZO"][-1:]]))   # nz + 1: half cells at both ends
        self.exact = {"dxC": row(dxc), "dxG": row(dxg), "dyC": col(dyc), "dyG": col(dyg),
                      "rA": np.outer(dyg, dxg), "rAz": np.outer(dyc, dxc), "rAw": np.outer(dyg, dxc), "rAs": np.outer(dyc, dxg),
                      "drF": np.diff(p["ZO"]), "drCl": drc[:nz].copy(), "drCo": drc}
        self.h = (dxi, deta)    # the index-space spacings: the grid's own dx, dy when ex = ey = 0
        data = {}
        for name, (_, dims) in METRIC_DIMS.items():
            if name in self.omit:
                continue
            vals = self.exact[self.swap.get(name, name)]
            if vals.shape != self.exact[name].shape:
                assert vals.ndim == 1 and self.exact[name].ndim == 1, (name, self.swap[name])
                m = len(self.exact[name])
                vals = np.concatenate([vals, np.full(max(m - len(vals), 0), vals[-1])])[:m]
            data[name] = (dims, np.ascontiguousarray(vals).astype(self.dtype))
        coords = {k: (k, v.copy()) for k, v in p.items()}
        self.ds = Dataset(data, coords)
        metrics = {}
        for name, (axes, _) in METRIC_DIMS.items():
            if name in data:
                metrics.setdefault(axes, []).append(name)
        self.padding = padding or {"X": "periodic", "Y": "periodic", "Z": "extend"}
        self.grid = Grid(self.ds, coords=AXES, metrics=metrics, padding=self.padding, autoparse_metadata=False)

    def points(self, dims):
        """(z, y, x) coordinate arrays of an array with `dims` (two or three of them, (Z,) Y, X order)"""
        z = np.array([Z_FIXED]) if len(dims) == 2 else self.pts[dims[0]]
        return z, self.pts[dims[-2]], self.pts[dims[-1]]

    def value(self, field, dims, d=(0, 0, 0)):
        """the field (or its derivative `d`) at the points of `dims`, float64"""
        out = field(*self.points(dims), d=d)
        return out[0] if len(dims) == 2 else out

    def array(self, field, dims, name=None, d=(0, 0, 0), times=None):
        """a labelled input in the grid's dtype; `times`: a float64 array it is multiplied by first (a metric)"""
        v = self.value(field, dims, d)
        if times is not None:
            v = v * times
        return DataArray(np.ascontiguousarray(v).astype(self.dtype), tuple(dims), name=name)

    def wrap(self, values, dims, name=None):
        return DataArray(np.ascontiguousarray(values).astype(self.dtype), tuple(dims), name=name)
