"""Implicit vertical mixing on the GPU: `Grid.implicit_vertical_diffusion` (K7m, a forward and a backward sweep in one launch)
through libxgcm_hip.so against the numpy statement of tests/test_implicit_vertical_diffusion.py, bit for bit.  The last test
runs the entry under every value of every launch-shape tunable: the battery of tests/test_gpu_tunables.py looks for `_f64` /
`_f32` entries and this one takes its element type as an argument."""

import numpy as np
import pytest
import torch

import test_gpu_tunables as TT
import test_implicit_vertical_diffusion as TI
import test_vertical_diffusion as TD
from oracle import refimpl as R
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu
DT = TI.DT


@pytest.mark.parametrize("nx", TI.NXS)
def test_small_shapes(monkeypatch, nx):
    cases = TI.shape_cases(nx)
    assert len(cases) == len(TI.NZS) * len(TI.NYS)
    TI.run_cases(monkeypatch, cases)


def test_one_long_column(monkeypatch):
    TI.run_cases(monkeypatch, TI.long_column_cases())


@pytest.mark.parametrize("dtype", TI.DTYPES, ids=["f64", "f32"])
def test_a_nan_poisons_exactly_its_column(dtype):
    assert TI.nan_cases(dtype) == 16


@pytest.mark.parametrize("dtype", TI.DTYPES, ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TI.abi_layout_cases(dtype)


def test_abi_refuses_bad_calls():
    TI.abi_bad_calls()


def test_seeded_fuzz(monkeypatch):
    """240 cases over the small shapes, both flux positions, the NaN density, the dtype, dt, where `a` sits and the forms of
    kappa and of the metrics"""
    calls = TI._counted(monkeypatch)
    rng = np.random.default_rng(20241019)
    for case in range(240):
        nz, ny, nx = (int(rng.choice(v)) for v in (TI.NZS, TI.NYS, TI.NXS))
        lead = TI.LEADS[int(rng.integers(3))] if nx < 100 else ()
        to = TI.TOS[case % 2] if case < 2 else str(rng.choice(TI.TOS))
        dtype = TI.DTYPES[int(rng.integers(2))]
        hpos = "cuv"[int(rng.integers(3))]
        mform = TI.MFORMS[int(rng.integers(4))]
        kform = TI.KFORMS[int(rng.integers(4))]
        if not lead:
            mform, kform = ("full" if mform == "lead" else mform), ("3d" if kform == "lead" else kform)
        grid, ds, dims = TI._grid(lead, nz, ny, nx, dtype, metric=mform or "1d", hpos=hpos)
        density = (0.0, 0.05, 0.5)[int(rng.integers(3))]
        a = R.synthetic_field(tuple(lead) + (nz, ny, nx), 500 + 2 * case).astype(dtype)
        a[rng.random(a.shape) < density] = np.nan
        a = DataArray(a, dims + ("ZC",) + TD.HPOS[hpos], name="T")
        kappa = TI._kappa(kform, lead, nz, ny, nx, dtype, dims, to, hpos, seed=501 + 2 * case)
        kw = dict(dt=(0.0, 60.0, DT)[int(rng.integers(3))] * (1.0 if mform else 1e-6), to=to, metric_weighted=mform is not None)
        try:
            got = grid.implicit_vertical_diffusion(a, kappa, **kw)
            assert got.dims == a.dims and got.name == "T"
            TI._same_bits(got.values, TI._want_of(ds, a, kappa, to, kw["metric_weighted"], kw["dt"]))
        except AssertionError as err:
            raise AssertionError(f"fuzz case {case}: {lead} {nz}x{ny}x{nx} {to} {np.dtype(dtype)} a at {hpos}, metric {mform}, "
                                 f"kappa {kform}, NaN density {density} {kw}") from err
    assert len(calls) == 240


@pytest.mark.parametrize("dtype", TI.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    """several XCD bands, ragged tiles and a ragged last segment together; nx = 515 takes the narrow form, 516 the vector form"""
    cases = []
    lead, nz, ny = (2,), 7, 67
    for to, metric, kform in (("left", "full", "lead"), ("outer", "1d", "3d")):
        grid, ds, dims = TI._grid(lead, nz, ny, nx, dtype, metric=metric)
        a = TD._field(lead, nz, ny, nx, dtype, dims, nan=True)
        cases.append((grid, (a, TI._kappa(kform, lead, nz, ny, nx, dtype, dims, to)), dict(dt=DT, to=to, metric_weighted=True), ds))
    TI.run_cases(monkeypatch, cases)


def _resident(x):
    return DataArray(torch.from_numpy(x.values).cuda(), x.dims, name=x.name)


def test_hbm_in_hbm_out(monkeypatch):
    calls = TI._counted(monkeypatch)
    grid, ds, dims = TI._grid((2,), 5, 9, 136, np.float64)
    host = (TD._field((2,), 5, 9, 136, np.float64, dims, nan=True), TI._kappa("3d", (2,), 5, 9, 136, np.float64, dims, "outer"))
    got = grid.implicit_vertical_diffusion(*(_resident(x) for x in host), dt=DT)
    ref = grid.implicit_vertical_diffusion(*host, dt=DT)
    assert len(calls) == 2
    assert isinstance(got.data, torch.Tensor) and got.data.is_cuda and got.is_device
    assert tuple(got.dims) == host[0].dims and got.name == "T"
    assert isinstance(ref.data, np.ndarray)
    TI._same_bits(got.data.cpu().numpy(), ref.values)
    TI._same_bits(ref.values, TI._want_of(ds, *host, "outer", True))


@pytest.mark.parametrize("dtype", TI.DTYPES, ids=["f64", "f32"])
def test_the_explicit_operator_undoes_it_on_resident_tensors(dtype):
    """x - dt * vertical_diffusion(x, kappa, to="outer", padding="extend") is `a` again, within the bound measured on CPU"""
    grid, ds, a, kappa = TI._property_case(dtype)
    a, kappa = _resident(a), _resident(kappa)
    x = grid.implicit_vertical_diffusion(a, kappa, dt=DT)
    back = x.data - DT * grid.vertical_diffusion(x, kappa, to="outer", padding="extend").data
    assert back.is_cuda and back.dtype == a.data.dtype
    err = TI._rel(back.cpu().numpy(), a.values)
    print(f"{np.dtype(dtype)}: residual {err:.3e}")
    assert err <= 16 * TI.PROPERTY_MEASURED[dtype]["residual"]


def test_under_graph_capture(monkeypatch):
    """the operator captured once and replayed on new values in the same storage; kappa and the metrics have the field's own
    shape and are HBM-resident (the grid uploads the metrics once, in the capture's warm-up)"""
    from xgcm_amd import graphs

    calls = TI._counted(monkeypatch)
    lead, nz, ny, nx = (2,), 5, 40, 256
    grid, ds, dims = TI._grid(lead, nz, ny, nx, np.float64, metric="lead")
    h1, h2 = (TD._field(lead, nz, ny, nx, np.float64, dims, seed=s) for s in (71, 111))
    k1, k2 = (TI._kappa("lead", lead, nz, ny, nx, np.float64, dims, "outer", seed=s) for s in (75, 115))
    a, kappa = _resident(h1), _resident(k1)
    step = graphs.capture(lambda: grid.implicit_vertical_diffusion(a, kappa, dt=DT))
    a.data.copy_(torch.from_numpy(h2.values))
    kappa.data.copy_(torch.from_numpy(k2.values))
    out = step()
    torch.cuda.synchronize()
    assert len(calls) == 3   # two warm-up runs and the capture itself
    assert not np.array_equal(h1.values, h2.values)
    TI._same_bits(out.data.cpu().numpy(), TI._want_of(ds, h2, k2, "outer", True))


def tunable_calls(D, dtype):
    """(calls, references) of the K7m tunable sweep: name -> thunk that calls `D` on inputs uploaded once, name -> thunk
    that gives numpy's result of the same call; tests/test_gpu_guarded_memory.py runs the same table between guard bands"""
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    calls, references = {}, {}
    for n, shape in enumerate(((5, 300, 264), (3, 65, 131))):
        nz, ny, nx = shape
        a = f(shape, 150 + n)
        a[1, 7, 9] = a[0, 0, 0] = a[nz - 1, ny - 1, nx - 1] = np.nan
        da = D.asdevice(a)
        for k, to in enumerate(("left", "outer", "left", "outer")):
            nf = nz + (to == "outer")
            kappa = np.abs(f((nf, ny, nx), 160 + 4 * n + k)) * dtype(2e4)
            # 3-D metrics, profiles, the flux' metric alone, none
            mf, mc = [(m((nf, ny, nx), 172), m((nz, ny, nx), 173)), (m((nf, 1, 1), 170), m((nz, 1, 1), 171)),
                      (m((nf, ny, nx), 174), None), (None, None)][k]
            d = tuple(None if x is None else D.asdevice(x) for x in (kappa, mf, mc))
            key = f"{nx}{to}{k}"
            dt = TI.abi_dt({"mf": mf, "mc": mc})
            calls[key] = lambda da=da, d=d, to=to, dt=dt: D.implicit_vertical_diffusion(da, *d, to == "outer", dt)
            references[key] = lambda a=a, h=(kappa, mf, mc), dt=dt: TI.statement(a, *h, dt)
    return calls, references


@pytest.mark.parametrize("dtype", TI.DTYPES, ids=["f64", "f32"])
def test_every_tunable_value_computes_the_same(dtype):
    """`device.implicit_vertical_diffusion` under every value of every tunable of the battery's table, on the battery's own
    shapes, both flux positions, a 3-D kappa and both forms of the metrics: bit for bit what the defaults give, and that is
    the numpy statement's"""
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
