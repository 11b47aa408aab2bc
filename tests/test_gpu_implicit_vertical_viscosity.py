"""Implicit vertical viscosity on the GPU: `Grid.implicit_vertical_viscosity` (K7o, the two averages of nu inside the coefficient
stage of K7m's solve, one launch per component) through libxgcm_hip.so against the numpy statement of
tests/test_implicit_vertical_viscosity.py, bit for bit.  The entry takes its element type as an argument, so the batteries of
tests/test_gpu_tunables.py and tests/test_gpu_guarded_memory.py, which look for `_f64` / `_f32` entries, do not find it: the
last two tests here run its table under every value of every launch-shape tunable and between guard bands."""

import warnings

import numpy as np
import pytest
import torch

import test_gpu_tunables as TT
import test_implicit_vertical_viscosity as TV
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu
DT = TV.DT


@pytest.mark.parametrize("nx", TV.NXS)
def test_small_shapes(monkeypatch, nx):
    cases = TV.shape_cases(nx)
    assert len(cases) == len(TV.NZS) * len(TV.NYS)
    TV.run_cases(monkeypatch, cases)


@pytest.mark.parametrize("dtype", TV.DTYPES, ids=["f64", "f32"])
def test_a_nan_in_nu_poisons_exactly_the_columns_it_reaches(dtype):
    assert TV.nan_cases(dtype) == 27


@pytest.mark.parametrize("dtype", TV.DTYPES, ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TV.abi_layout_cases(dtype)


def test_abi_refuses_bad_calls():
    TV.abi_bad_calls()


def test_seeded_fuzz(monkeypatch):
    """240 cases over the small shapes, both flux positions, the pads and fills of either axis, the NaN density of the fields
    and of nu, the dtype, dt and the forms of nu and of the metrics"""
    calls = TV._counted(monkeypatch)
    rng = np.random.default_rng(20241020)
    for case in range(240):
        nz, ny, nx = (int(rng.choice(v)) for v in (TV.NZS, TV.NYS, TV.NXS))
        lead = TV.LEADS[int(rng.integers(3))] if nx < 100 else ()
        to = TV.TOS[case % 2] if case < 2 else str(rng.choice(TV.TOS))
        dtype = TV.DTYPES[int(rng.integers(2))]
        mform = TV.MFORMS[int(rng.integers(4))]
        nuform = ("3d", "lead")[int(rng.integers(2))]
        pads = TV.PAIRS[int(rng.integers(9))]
        fills = tuple(TV.FILLS[int(rng.integers(3))] for _ in range(2))
        density = (0.0, 0.05, 0.5)[int(rng.integers(3))]
        dt = (0.0, 60.0, DT)[int(rng.integers(3))] * (1.0 if mform else 1e-6)
        grid, (u, v, nu), kw, ds = TV.case_of(lead, nz, ny, nx, to, dtype, mform, nuform, pads, fills, dt=dt, seed=500 + 2 * case)
        u, v, nu = (x._replace(data=np.where(rng.random(x.shape) < density, np.nan, x.values).astype(dtype)) for x in (u, v, nu))
        try:
            xu, xv = grid.implicit_vertical_viscosity(u, v, nu, **kw)
            for got, want in zip((xu, xv), TV._want_of(grid, ds, u, v, nu, kw)):
                TV._same_bits(got.values, want)
        except AssertionError as err:
            raise AssertionError(f"fuzz case {case}: {lead} {nz}x{ny}x{nx} {to} {np.dtype(dtype)} metric {mform}, nu {nuform}, pads "
                                 f"{pads}, NaN density {density} {kw}") from err
    assert len(calls) == 240


@pytest.mark.parametrize("dtype", TV.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    """several XCD bands, ragged tiles and a ragged last segment together; nx = 515 takes the narrow form, 516 the vector form"""
    lead, nz, ny = (2,), 7, 67
    cases = [TV.case_of(lead, nz, ny, nx, to, dtype, mform, nuform, pads, (0.375, float("nan")), nan=True)
             for to, mform, nuform, pads in (("left", "full", "lead", ("fill", "periodic")), ("outer", "1d", "3d", ("periodic", "extend")))]
    TV.run_cases(monkeypatch, cases)


def _resident(x):
    return DataArray(torch.from_numpy(x.values).cuda(), x.dims, name=x.name)


def test_hbm_in_hbm_out(monkeypatch):
    calls = TV._counted(monkeypatch)
    grid, (u, v, nu), kw, ds = TV.case_of((2,), 5, 9, 136, "outer", np.float64, "1d", "3d", ("extend", "periodic"), (0.0, 0.0), nan=True)
    ref = grid.implicit_vertical_viscosity(u, v, nu, **kw)
    for k in range(3):   # a tensor among u, v, nu gives HBM out
        got = grid.implicit_vertical_viscosity(*(_resident(x) if j == k else x for j, x in enumerate((u, v, nu))), **kw)
        for g, r, f in zip(got, ref, (u, v)):
            assert isinstance(g.data, torch.Tensor) and g.data.is_cuda and g.is_device and tuple(g.dims) == f.dims and g.name == f.name
            assert isinstance(r.data, np.ndarray)
            TV._same_bits(g.data.cpu().numpy(), r.values)
    assert len(calls) == 4
    for r, want in zip(ref, TV._want_of(grid, ds, u, v, nu, kw)):
        TV._same_bits(r.values, want)


@pytest.mark.parametrize("dtype", TV.DTYPES, ids=["f64", "f32"])
def test_the_explicit_operator_undoes_it_on_resident_tensors(dtype):
    """xu - dt * vertical_diffusion(xu, interp(nu, X), to="outer", padding="extend") is u again and likewise for v, within the
    bound measured on CPU"""
    grid, ds, u, v, nu = TV.property_case(dtype)
    ru, rv, rn = _resident(u), _resident(v), _resident(nu)
    xu, xv = grid.implicit_vertical_viscosity(ru, rv, rn, dt=DT)
    assert xu.data.is_cuda and xv.data.is_cuda
    got = TV.residuals(grid, ru, rv, rn, xu, xv, values=lambda x: x.data.cpu().numpy())
    print(f"{np.dtype(dtype)}: residual u {got['u']:.3e}, v {got['v']:.3e}")
    for c in "uv":
        assert got[c] <= 16 * TV.RESIDUAL_MEASURED[dtype][c], (c, got[c])


def test_under_graph_capture(monkeypatch):
    """the operator captured once and replayed on new values in the same storage (the two workspaces are allocated per call, so
    the capture holds its own)"""
    from xgcm_amd import graphs

    calls = TV._counted(monkeypatch)
    row = ((2,), 5, 40, 256, "outer", np.float64, "lead", "lead", ("periodic", "fill"), (0.0, -0.0))
    grid, h1, kw, ds = TV.case_of(*row, seed=71)
    _, h2, _, _ = TV.case_of(*row, seed=111)
    res = [_resident(x) for x in h1]
    step = graphs.capture(lambda: grid.implicit_vertical_viscosity(*res, **kw))
    for r, h in zip(res, h2):
        r.data.copy_(torch.from_numpy(h.values))
    out = step()
    torch.cuda.synchronize()
    assert len(calls) == 3   # two warm-up runs and the capture itself
    assert not np.array_equal(h1[0].values, h2[0].values)
    for got, want in zip(out, TV._want_of(grid, ds, *h2, kw)):
        TV._same_bits(got.data.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", TV.DTYPES, ids=["f64", "f32"])
def test_every_tunable_value_computes_the_same(dtype):
    """`device.implicit_vertical_viscosity` under every value of every tunable of the battery's table, on the battery's own
    shapes: bit for bit what the defaults give, and that is the numpy statement's"""
    from xgcm_amd import _hip
    from xgcm_amd import device as D

    calls, references = TV.tunable_calls(D, dtype)
    run = lambda: {k: [D.tohost(x) for x in fn()] for k, fn in calls.items()}  # noqa: E731
    want = run()
    for k, reference in references.items():
        assert all(TT._same_bits(g, w) for g, w in zip(want[k], reference())), f"{k}: the default result is not numpy's"
    bad = []
    for name, values in TT.ALTERNATIVES.items():
        before = _hip.get_tunable(name)
        try:
            for val in values:
                _hip.set_tunable(name, val)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    got = run()
                bad += [(name, val, k) for k in calls if not all(TT._same_bits(g, w) for g, w in zip(got[k], want[k]))]
        finally:
            _hip.set_tunable(name, before)
    torch.cuda.synchronize()
    assert not bad, bad[:20]


@pytest.mark.parametrize("dtype", TV.DTYPES, ids=["f64", "f32"])
def test_between_guard_bands_on_the_device(monkeypatch, dtype):
    """the same table with every result, workspace and uploaded input between guard bands, the payload 512-byte aligned, 16
    bytes and one element off"""
    from xgcm_amd import device as D

    for offset in (0, 16, np.dtype(dtype).itemsize):
        assert TV.guarded_table(D, monkeypatch, dtype, offset, TT._same_bits) == 16
    torch.cuda.synchronize()
