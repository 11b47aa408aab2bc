"""Vertical mixing on the GPU: `Grid.vertical_diffusion` (K7l, one launch) against the chain of three launches it replaces --
the derivative to the flux levels, the product with kappa, the derivative back to the centre -- both through libxgcm_hip.so,
bit for bit.  The last test runs the entry under every value of every launch-shape tunable: the battery of
tests/test_gpu_tunables.py looks for `_f64` / `_f32` entries and this one takes its element type as an argument."""

import numpy as np
import pytest
import torch

import test_gpu_tunables as TT
import test_vertical_diffusion as TD
from oracle import refimpl as R
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx", TD.NXS)
def test_small_shapes(monkeypatch, nx):
    calls = TD._counted(monkeypatch)
    cases = TD.shape_cases(nx)
    for grid, f, kw in cases:
        TD._same_labelled(grid.vertical_diffusion(*f, **kw), TD._chain(grid, *f, **kw))
    assert len(calls) == len(cases) == len(TD.NZS) * len(TD.NYS)


@pytest.mark.parametrize("pz", TD.BCS)
@pytest.mark.parametrize("to", TD.TOS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_equals_the_chain(monkeypatch, pz, to, dtype):
    calls = TD._counted(monkeypatch)
    cases = TD.matrix_cases(pz, to, dtype)
    for grid, f, kw, _ in cases:
        TD._same_labelled(grid.vertical_diffusion(*f, **kw), TD._chain(grid, *f, **kw))
    assert len(calls) == len(cases)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_signed_zeros_and_negative_zero_fills_keep_their_sign(monkeypatch, dtype):
    """bit patterns, not values: -0.0 fills and exact zeros of both signs, kernel against chain against numpy"""
    calls = TD._counted(monkeypatch)
    cases = TD.signed_zero_cases(dtype)
    for grid, f, kw, ds, pz in cases:
        got = grid.vertical_diffusion(*f, **kw)
        TD._same_bits(got.values, TD._chain(grid, *f, **kw).values)
        TD._same_bits(got.values, TD._want_of(grid, ds, *f, kw["to"], pz, kw["fill_value"], kw["metric_weighted"]))
    assert len(calls) == len(cases)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TD.abi_layout_cases(dtype)


def test_abi_refuses_bad_calls():
    TD.abi_bad_calls()


def test_seeded_fuzz(monkeypatch):
    """240 cases over the small shapes, the boundaries, both flux positions, the fills, the NaN density, the dtype, where `a`
    sits and the forms of kappa and of the metrics"""
    calls = TD._counted(monkeypatch)
    rng = np.random.default_rng(20240613)
    for case in range(240):
        nz, ny, nx = (int(rng.choice(v)) for v in (TD.NZS, TD.NYS, TD.NXS))
        lead = [(), (2,), (2, 2)][int(rng.integers(3))] if nx < 100 else ()
        pz, to = TD.PADS2[case % 6] if case < 6 else (str(rng.choice(TD.BCS)), str(rng.choice(TD.TOS)))
        dtype = (np.float64, np.float32)[int(rng.integers(2))]
        hpos = "cuv"[int(rng.integers(3))]
        metric = ("1d", "full", "lead")[int(rng.integers(3 if lead else 2))]
        kform = (None, "1d", "3d", "lead")[int(rng.integers(4))]
        grid, ds, dims = TD._grid(lead, nz, ny, nx, dtype, pz, metric=metric, hpos=hpos)
        density = (0.0, 0.05, 0.5)[int(rng.integers(3))]
        a = R.synthetic_field(tuple(lead) + (nz, ny, nx), 500 + 2 * case).astype(dtype)
        a[rng.random(a.shape) < density] = np.nan
        a = DataArray(a, dims + ("ZC",) + TD.HPOS[hpos], name="T")
        kappa = TD._kappa(kform, lead, nz, ny, nx, dtype, dims, to, hpos, seed=501 + 2 * case)
        kw = dict(to=to, fill_value=TD.FILLS[int(rng.integers(3))], metric_weighted=bool(rng.integers(2)))
        try:
            TD._same_labelled(grid.vertical_diffusion(a, kappa, **kw), TD._chain(grid, a, kappa, **kw))
        except AssertionError as err:
            raise AssertionError(f"fuzz case {case}: {lead} {nz}x{ny}x{nx} {pz} {to} {np.dtype(dtype)} a at {hpos}, metric "
                                 f"{metric}, kappa {kform}, NaN density {density} {kw}") from err
    assert len(calls) == 240


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    """several XCD bands, ragged tiles and a ragged last segment together; nx = 515 takes the narrow form, 516 the vector form"""
    calls = TD._counted(monkeypatch)
    lead, nz, ny = (2,), 7, 67
    for pz, to, metric, kform in (("periodic", "left", "full", "lead"), ("extend", "outer", "1d", "3d")):
        grid, ds, dims = TD._grid(lead, nz, ny, nx, dtype, pz, metric=metric)
        a = TD._field(lead, nz, ny, nx, dtype, dims, nan=True)
        kappa = TD._kappa(kform, lead, nz, ny, nx, dtype, dims, to)
        kw = dict(to=to, fill_value=0.375)
        TD._same_labelled(grid.vertical_diffusion(a, kappa, **kw), TD._chain(grid, a, kappa, **kw))
    assert len(calls) == 2


def _resident(x):
    return DataArray(torch.from_numpy(x.values).cuda(), x.dims, name=x.name)


def test_hbm_in_hbm_out(monkeypatch):
    calls = TD._counted(monkeypatch)
    grid, ds, dims = TD._grid((2,), 5, 9, 136, np.float64, "extend")
    host = (TD._field((2,), 5, 9, 136, np.float64, dims, nan=True), TD._kappa("3d", (2,), 5, 9, 136, np.float64, dims, "outer"))
    f = tuple(_resident(x) for x in host)
    got = grid.vertical_diffusion(*f, fill_value=0.375)
    assert len(calls) == 1
    want = TD._chain(grid, *f, fill_value=0.375)
    ref = grid.vertical_diffusion(*host, fill_value=0.375)
    assert isinstance(got.data, torch.Tensor) and got.data.is_cuda and got.is_device
    assert tuple(got.dims) == tuple(want.dims) and got.name == want.name
    assert isinstance(want.data, torch.Tensor) and want.data.is_cuda
    assert np.array_equal(got.data.cpu().numpy(), want.data.cpu().numpy(), equal_nan=True)
    assert isinstance(ref.data, np.ndarray) and np.array_equal(ref.values, got.data.cpu().numpy(), equal_nan=True)


def test_under_graph_capture(monkeypatch):
    """the operator captured once and replayed on new values in the same storage; kappa and the metrics have the field's own
    shape and are HBM-resident (the grid uploads the metrics once, in the capture's warm-up)"""
    from xgcm_amd import graphs

    calls = TD._counted(monkeypatch)
    lead, nz, ny, nx = (2,), 5, 40, 256
    grid, ds, dims = TD._grid(lead, nz, ny, nx, np.float64, "extend", metric="lead")
    a, a2 = (_resident(TD._field(lead, nz, ny, nx, np.float64, dims, seed=s)) for s in (71, 111))
    kappa, kappa2 = (_resident(TD._kappa("lead", lead, nz, ny, nx, np.float64, dims, "outer", seed=s)) for s in (75, 115))
    step = graphs.capture(lambda: grid.vertical_diffusion(a, kappa, fill_value=0.375))
    a.data.copy_(a2.data)
    kappa.data.copy_(kappa2.data)
    out = step()
    torch.cuda.synchronize()
    assert len(calls) == 3   # two warm-up runs and the capture itself: the one-pass entry, not the chain, is in the graph
    got = out.data.clone()
    want = TD._chain(grid, a2, kappa2, fill_value=0.375)
    assert got.shape == (2, nz, ny, nx) and torch.equal(got.view(torch.int64), want.data.view(torch.int64))


def tunable_calls(D, dtype):
    """(calls, references) of the K7l tunable sweep: name -> thunk that calls `D` on inputs uploaded once, name -> thunk
    that gives numpy's result of the same call; tests/test_gpu_guarded_memory.py runs the same table between guard bands"""
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    calls, references = {}, {}
    for n, shape in enumerate(((5, 300, 264), (3, 65, 131))):
        nz, ny, nx = shape
        a = f(shape, 150 + n)
        a[1, 7, 9] = a[0, 0, 0] = a[nz - 1, ny - 1, nx - 1] = np.nan
        da = D.asdevice(a)
        for k, (to, pz) in enumerate((("left", "periodic"), ("outer", "extend"), ("left", "fill"), ("outer", "periodic"))):
            nf = nz + (to == "outer")
            kappa = f((nf, ny, nx), 160 + 4 * n + k)
            mf, mc = (m((nf, 1, 1), 170), m((nz, 1, 1), 171)) if k % 2 else (m((nf, ny, nx), 172), m((nz, ny, nx), 173))
            d = tuple(D.asdevice(x) for x in (kappa, mf, mc))
            key = f"{nx}{to}{pz}"
            calls[key] = lambda da=da, d=d, to=to, pz=pz: D.vertical_diffusion(da, *d, to == "outer", pz, 0.375)
            references[key] = lambda a=a, h=(kappa, mf, mc), to=to, pz=pz: TD._want(a, *h, to, pz, dtype(0.375))
    return calls, references


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_tunable_value_computes_the_same(dtype):
    """`device.vertical_diffusion` under every value of every tunable of the battery's table, on the battery's own shapes, both
    flux positions, a 3-D kappa and both forms of the metrics: bit for bit what the defaults give, and that is numpy's"""
    import warnings

    from xgcm_amd import _hip
    from xgcm_amd import device as D

    calls, references = tunable_calls(D, dtype)
    run = lambda: {k: D.tohost(fn()) for k, fn in calls.items()}  # noqa: E731
    want = run()
    for k, reference in references.items():
        assert TT._same_bits(want[k], reference()), f"{k}: the default result is not numpy's"
    bad = []
    for name, values in TT.ALTERNATIVES.items():
        before = _hip.get_tunable(name)
        try:
            for val in values:
                _hip.set_tunable(name, val)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    got = run()
                bad += [(name, val, k) for k in calls if not TT._same_bits(got[k], want[k])]
        finally:
            _hip.set_tunable(name, before)
    torch.cuda.synchronize()
    assert not bad, bad[:20]
