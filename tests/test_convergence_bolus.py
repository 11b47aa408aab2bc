"""`Grid.bolus_velocity` against its continuous meaning on the stretched analytic grid of tests/analytic_grid.py, with the
machinery of tests/test_convergence.py (by import; nothing is registered in its tables):

    ub -> -dKWX/dz at (ZC, YC, XG)      vb -> -dKWY/dz at (ZC, YG, XC)      wb -> dKWX/dx + dKWY/dy at (ZO, YC, XC)

KWX and KWY vanish at z = 0 and z = 1, so the closed and the open form approximate the same terms.  Observed order
p = log2(E(32) / E(64)) >= 1.75, the project's bar; E(n) as measured on the host build is recorded and held within a factor of
two, on the GPU to 1e-12.  float32 runs n = 32 only.  Each of the metrics the operator reads -- drF (at ub's and at vb's
points: one registered array serves both), dyG, dxG, rA -- is swapped for the registered metric of another position in turn:
the results that read it must fall below p = 1.5 -- the project's assertion, for all four -- and the others keep every bit.  A
wrong dyG or dxG shows in E only from n = 128 on, so those two are held at p(128 -> 256); the reason is next to `SWAPPED`."""

import types

import numpy as np
import pytest

import test_convergence as TC
from test_convergence import DX, DY, DZ, KWX, KWY, O3, U3, V3, ZEXTEND, cbackend  # noqa: F401  (the fixture)

BAR, LIVE_BAR = TC.BAR, TC.LIVE_BAR


def _bolus(closed):
    def fn(ag):
        ub, vb, wb = ag.grid.bolus_velocity(ag.array(KWX, O3, "kwx"), ag.array(KWY, O3, "kwy"), closed=closed, **ZEXTEND)
        assert tuple(ub.dims) == U3 and tuple(vb.dims) == V3 and tuple(wb.dims) == O3
        ten = ag.dtype.type(10)     # (~0.1: scaled to O(1) for the triviality floor)
        return [("ub", ub.values * ten, -10 * ag.value(KWX, U3, DZ), None), ("vb", vb.values * ten, -10 * ag.value(KWY, V3, DZ), None),
                ("wb", wb.values * ten, 10 * (ag.value(KWX, O3, DX) + ag.value(KWY, O3, DY)), None)]
    return types.SimpleNamespace(name=f"bolus_velocity/{'closed' if closed else 'open'}", fn=fn, entry="bolus_velocity", calls=1,
                                 ns=(16, 32, 64), f32_n=32, xfail=None, interpolated=False, cpu_double=(), reassociated=False)


CASES = {c.name: c for c in (_bolus(True), _bolus(False))}
# "case:label" -> E(16), E(32), E(64), float64, host build.  The fields vanish at the end faces: closed and open record equal errors
_E = {"ub": (0.18276726659748688, 0.052365136177981775, 0.013245834035104487),   # p = 1.80, 1.98
      "vb": (0.12484874803832269, 0.03677504547338595, 0.009281875397205042),    # p = 1.76, 1.99
      "wb": (0.23917229574030374, 0.07263026265118455, 0.01904989889177644)}     # p = 1.72, 1.93
MEASURED = {f"{name}:{label}": e for name in CASES for label, e in _E.items()}
F32_RATIO = {key: 1.0000 for key in MEASURED}
# (metric registered wrongly, the metric whose values it gets) -> ((n, 2n) at which the order is held, {label that reads it:
# p(n -> 2n) of E as observed}).  On this separable map a wrong drF is a wrong divisor of the whole of ub and vb, and a wrong rA
# of the whole of wb: their E stops converging at once.  A wrong dyG (dxG) reaches wb only as the factor (1 + eps) of its X (Y)
# part, eps = O(h) a function of y (x) alone: a first-order term eps * dKWX/dx that is a third of the second-order error at
# n = 64 (p(32 -> 64) = 1.92 / 1.93, p(64 -> 128) = 1.74 / 1.77) and the larger part from n = 128 on, where the order is lost.
SWAPPED = {("drF", "drCl"): ((32, 64), {"ub": -0.04, "vb": -0.03}), ("rA", "rAz"): ((32, 64), {"wb": 1.47}),
           ("dyG", "dyC"): ((128, 256), {"wb": 1.21}), ("dxG", "dxC"): ((128, 256), {"wb": 1.17})}


@pytest.mark.parametrize("name", sorted(CASES))
def test_second_order(cbackend, monkeypatch, name):
    c = CASES[name]
    calls = TC.counted(monkeypatch, c, cbackend)
    errs = [TC.evaluate(c, n, counter=calls) for n in c.ns]
    for label in errs[0]:
        e = [x[label] for x in errs]
        p = TC.order(e[1], e[2])
        print(f"{name}:{label} E = {e[0]!r} {e[1]!r} {e[2]!r}  p = {TC.order(e[0], e[1]):.2f} {p:.2f}")
        assert p >= BAR, (name, label, e, p)
        rec = MEASURED[f"{name}:{label}"]
        assert rec[2] / 2 <= e[2] <= rec[2] * 2, (name, label, e, rec)
        if cbackend == "hip":
            assert np.allclose(e, rec, rtol=1e-12, atol=0), (name, label, e, rec)


def test_closed_and_open_give_equal_errors(host_abi):
    """KWX and KWY vanish at the end faces, so closing them changes nothing the errors see: E of the two forms as computed"""
    closed, opened = (TC.evaluate(CASES[f"bolus_velocity/{form}"], 32) for form in ("closed", "open"))
    assert set(closed) == {"ub", "vb", "wb"} and closed == opened, (closed, opened)


@pytest.mark.parametrize("name", sorted(CASES))
def test_float32_error_ratio(cbackend, monkeypatch, name):
    c = CASES[name]
    calls = TC.counted(monkeypatch, c, cbackend)
    e32, e64 = TC.evaluate(c, c.f32_n, np.float32, counter=calls), TC.evaluate(c, c.f32_n, counter=calls)
    for label in e32:
        ratio = e32[label] / e64[label]
        print(f"{name}:{label} n = {c.f32_n} E32 / E64 = {ratio:.4f}")
        assert ratio <= F32_RATIO[f"{name}:{label}"] * 1.5, (name, label, ratio)


def _results(c, n, swap=None):
    return {label: np.asarray(got, np.float64) for label, got, _, _ in c.fn(TC.AnalyticGrid(n, swap=swap))}


@pytest.mark.parametrize("key", sorted(SWAPPED), ids=lambda k: "-".join(k))
def test_a_metric_of_another_position_costs_an_order(host_abi, monkeypatch, key):
    """the project's assertion (tests/test_convergence.py): the results that read the swapped metric fall below LIVE_BAR, at
    the resolutions `SWAPPED` names.  Next to it, at n = 32 and 64: the change the swap makes to those results is itself first
    order, and the results that do not read the metric keep every bit and the bar"""
    metric, other = key
    (lo, hi), recorded = SWAPPED[key]
    c = CASES["bolus_velocity/closed"]
    e = {n: TC.evaluate(c, n, swap={metric: other}) for n in sorted({32, 64, lo, hi})}
    ps = {label: TC.order(e[lo][label], e[hi][label]) for label in e[lo]}
    change = {n: {label: float(np.abs(got - _results(c, n)[label]).max()) for label, got in _results(c, n, {metric: other}).items()}
              for n in (32, 64)}
    print(f"bolus_velocity with {other} registered as {metric}: p({lo} -> {hi}) = {ps}  change = {change}")
    for label, p in ps.items():
        if label in recorded:
            assert p < LIVE_BAR, (key, label, ps)
            assert abs(p - recorded[label]) < 0.05, (key, label, ps)
            assert change[64][label] > 0 and TC.order(change[32][label], change[64][label]) < LIVE_BAR, (key, label, change)
        else:
            assert change[32][label] == change[64][label] == 0.0, (key, label, change)
            assert TC.order(e[32][label], e[64][label]) >= BAR, (key, label, e)
