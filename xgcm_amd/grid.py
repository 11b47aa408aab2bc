"""`Grid`: the public operator surface (diff / interp / min / max / cumsum / derivative / integrate /
cumint / average / get_metric ...) of the reference's `xgcm.Grid`, with every array pass executed
by one fused HIP kernel.

Reference call stacks and what replaces them here:

* `Grid.diff/interp/min/max` -> `_1d_grid_ufunc_dispatch` (xgcm/grid.py:728-836): per axis
  `array*metric` -> pad copy -> apply_ufunc -> `array/metric`  (5+ memory passes).  Here: per axis ONE
  launch of `xg_stencil1d_f64` with halo, metric multiply and metric divide fused.
* `Grid.derivative` (grid.py:1576-1578): diff then `/ dx`  ->  same launch with `m_out = dx`.
* `Grid.integrate` (grid.py:1598-1605): `(da*w).sum(dim)`  ->  `xg_reduce1d_f64` (first axis fused with
  the weight multiply).
* `Grid.cumsum` (grid.py:1183-1418): flip/cumsum/flip/trim/pad/`/metric`  ->  one `xg_cumsum1d_f64`.

Metadata logic (axis lookup, default shifts, per-axis kwargs, metric search, coordinate
re-attachment, error types and messages) is restated from the reference so that the parity tests
read like the reference's own.  Grids with face connections or a north fold take the generic
pad-then-apply route (halo gather `xg_gather_f64`, then the un-padded stencil kernel).  Out of scope
(dask-style chunked inputs are walked block by block: xgcm_amd.chunked).
"""

from __future__ import annotations

import contextlib
import functools
import inspect
import itertools
import operator
import threading
import warnings
from collections import OrderedDict
from typing import Any, Dict, Iterable, List, Mapping, NamedTuple, Optional, Tuple

import numpy as np

from . import device as _dev
from . import dtypes as _dt
from . import gridops
from .axis import Axis
from .grid_ufunc import (
    GridUFunc,
    _check_data_input,
    _GridUFuncSignature,
    _maybe_unpack_vector_component,
    _reattach_coords,
    apply_as_grid_ufunc,
)
from . import lazy as _lazy
from .labeled import (CHUNKED_INPUT_MESSAGE, DataArray, Dataset, _aligned_view, _binary_coords, _is_chunked, _is_tensor,
                      _result_name,
                      from_xarray, is_xarray, to_xarray)
from .metrics import iterate_axis_combinations
from .padding import FoldSpec, InteriorOf, fill_of, halo_cells, no_boundary_error, pad


def _maybe_promote_str_to_list(a):
    return [a] if isinstance(a, str) else a


def _name_after(name, *metrics):
    """name of `array OP metric ...` by xarray's rule (kept only while every operand carries it): the fused kernels
    take the metrics into the operator's launch, the NAME still follows the reference's explicit products / quotients"""
    for m in metrics:
        if m is not None and getattr(m, "name", None) != name:
            return None
    return name


def named(g, m):
    """`g`, named after its quotient or product with the metric `m` (None: `g` as it is)"""
    return g if m is None else g._replace(name=_name_after(g.name, m))


class _ColumnPoints(NamedTuple):
    """the dims of the column operators' points (`Grid._column_points`) and `held`, every dim the three axes hold"""

    tz: str
    zf: str
    yc: str
    yl: str
    xc: str
    xl: str
    held: set


class _DimsOnly:
    """Stand-in carrying only `.dims`/`.name`: all `get_metric` needs of its `array` argument."""

    def __init__(self, dims, name=None):
        self.dims = tuple(dims)
        self.name = name


def _refuse_chunked_core_dim_with_changing_length(grid, da, ax_name, sig):
    """The reference maps a ufunc over the chunks of a chunked CORE dim with `dask.array.map_overlap` and refuses signatures
    whose positions change the dim's length (`xgcm/grid_ufunc.py:1136-1159`, reached from `xgcm/grid.py:810-816`; `cumsum` is
    exempt there).  Chunks along the operator's axis are read together here, so nothing would go wrong -- but the same call
    raises the same error, so that code written against this backend also runs on the reference."""
    chunks = getattr(da, "chunks", None)
    if chunks is None:
        return
    _, dim = grid.axes[ax_name]._get_position_name(da)
    if len(chunks[da.dims.index(dim)]) <= 1:
        return
    positions = {p for ps in list(sig.in_ax_positions) + list(sig.out_ax_positions) for p in ps}
    if positions & {"inner", "outer"}:
        raise NotImplementedError(
            "Cannot chunk along a core dimension for a grid ufunc which has a signature which "
            "includes one of the axis positions ['inner', 'outer']."
            "Consider rechunking to a single chunk along this dimension if possible."
        )


class Grid:
    """Multiple :class:`Axis` objects describing the staggered topology of a dataset."""

    def __init__(self, ds, coords: Optional[Mapping[str, Mapping[str, str]]] = None, fill_value=None,
                 default_shifts=None, padding=None, face_connections=None, metrics=None,
                 autoparse_metadata: bool = True, fuse: bool = False, **kwargs):
        if "boundary" in kwargs:
            raise ValueError("Argument 'boundary' has been renamed to 'padding'. Please use 'padding' instead.")
        given = ds
        if is_xarray(ds):
            ds = from_xarray(ds)
        if not isinstance(ds, Dataset):
            raise TypeError(f"ds argument to `xgcm.Grid` must be of type xarray.Dataset, but is of type {type(ds)}")
        # `_ds` is the dataset AS GIVEN (an xarray.Dataset stays one: code written against the reference reads
        # `grid._ds.<coord>`, its tests 69 times); the operators work on `_own_ds`, the library's view of it
        self._ds = given
        self._own_ds = ds
        # `fuse=True` (or `with grid.fused():`): diff / interp / min / max / derivative return deferred results whose
        # chains -- `(grid.diff(v, "X") - grid.diff(u, "Y")) / area` -- run as ONE fused kernel when the value is used
        # (xgcm_amd.lazy; the reference's own TODO, xgcm/grid.py:797-799).  Off by default: results are computed at the call.
        self._fuse = bool(fuse)
        self._fuse_local = threading.local()
        if autoparse_metadata:
            # COMODO attributes / SGRID topology of the dataset supply what the caller left out; what BOTH supply is a
            # conflict, never a silent choice (xgcm/grid.py:151-195 -- `coords` is always among the parsed kwargs, so
            # explicit `coords` need `autoparse_metadata=False` exactly as there)
            from .metadata import parse_metadata

            _, parsed = parse_metadata(ds)
            given = {"coords": coords, "fill_value": fill_value, "default_shifts": default_shifts, "padding": padding,
                     "face_connections": face_connections, "metrics": metrics}
            duplicates = [k for k in given if k in parsed and given[k] is not None]
            if duplicates:
                raise ValueError(
                    f"Autoparsed Grid kwargs: '{', '.join(duplicates)}' conflict with "
                    f"user-supplied kwargs. Run with 'autoparse_metadata=False', or "
                    f"autoparse and amend kwargs before calling Grid constructer."
                )
            coords = parsed.get("coords", coords)
        if "periodic" in kwargs:
            raise ValueError(
                "The `periodic` argument has been removed. Use "
                "`padding='periodic'` (per axis if needed, e.g. "
                "`padding={'X': 'periodic', 'Y': 'fill'}`) instead. "
                "Previously `periodic=False` corresponded to `padding='fill'`."
            )
        if kwargs:
            raise TypeError(
                f"Grid.__init__() got unexpected keyword argument(s): {', '.join(repr(k) for k in kwargs)}"
            )
        if fill_value:
            warnings.warn(
                "The default fill_value will be changed to nan (from 0.0 previously) "
                "in future versions. Provide `fill_value=0.0` to preserve previous behavior.",
                category=DeprecationWarning,
            )
        if coords is None:  # (a dataset whose metadata names no axis parses to {}: an empty Grid, as in the reference)
            raise ValueError(
                "Could not determine Axis names - please provide them in the coords kwarg "
                "or provide a dataset from which they can be parsed"
            )
        names = list(coords.keys())
        per_axis_padding = self._map_kwargs_over_axes(padding, axes=names)
        per_axis_shifts = self._map_kwargs_over_axes(default_shifts, axes=names)
        per_axis_fill = self._map_kwargs_over_axes(fill_value, axes=names)
        # only an axis the user marked periodic can be the seam of a north fold (grid.py:241-249)
        self._explicitly_periodic_axes = {ax for ax, p in per_axis_padding.items() if p == "periodic"}
        if face_connections:
            self._facedim = list(face_connections.keys())[0]
            self._face_connections = face_connections
        else:
            self._facedim = None
            self._face_connections = None
        self._connected_axes: set = set()
        self.axes: "OrderedDict[str, Axis]" = OrderedDict()
        for ax in names:
            self.axes[ax] = Axis(
                ds,
                ax,
                coords=coords[ax],
                default_shifts=per_axis_shifts.get(ax, None),
                padding=per_axis_padding.get(ax, None),
                fill_value=per_axis_fill.get(ax, None),
            )

        if face_connections is not None:
            self._assign_face_connections(face_connections)
        self._validate_folds()

        self._own_metrics: Dict[frozenset, List[DataArray]] = {}
        self._device_cache: Dict[int, Any] = {}
        self._metric_ids: set = set()
        if metrics is not None:
            for key, value in metrics.items():
                self.set_metrics(key, value)

    # ---- complex topologies (reference grid.py:334-470) --------------------------------------
    def _assign_face_connections(self, fc) -> None:
        """Check that every face link is mirrored by its neighbour and hand each axis its links."""
        if len(fc) > 1:
            raise ValueError("Only one face dimension is supported for now. Instead found %r" % repr(fc.keys()))
        facedim = list(fc.keys())[0]
        if facedim not in self._own_ds.dims:
            raise ValueError(
                f"Face dimension {facedim} does not exist in the dataset. Found {list(self._own_ds.dims)} instead"
            )
        face_links = fc[facedim]
        if facedim in self._own_ds.coords:
            valid_faces = set(np.asarray(self._own_ds[facedim].values).tolist())
        else:
            valid_faces = set(range(self._own_ds.dims[facedim]))
        per_axis: Dict[str, Dict[Any, Tuple]] = {}
        for fidx, axis_links_of_face in face_links.items():
            for axis, (link_left, link_right) in axis_links_of_face.items():
                checked = []
                # a link seen from its left end must come back from the neighbour's right end,
                # unless the connection is reversed
                for link, position in ((link_left, 1), (link_right, 0)):
                    if link is None:
                        checked.append(None)
                        continue
                    idx, ax, rev = link
                    back_position = int(not position) if rev else position
                    try:
                        neighbor_link = face_links[idx][ax][back_position]
                    except (KeyError, IndexError):
                        raise KeyError(
                            "Couldn't find a face link for face %r"
                            "in axis %r at position %r" % (idx, ax, back_position)
                        )
                    idx_n, ax_n, rev_n = neighbor_link
                    for name in (ax, ax_n):
                        if name not in self.axes:
                            raise KeyError("axis %r is not a valid axis" % name)
                    for face in (idx, idx_n):
                        if face not in valid_faces:
                            raise IndexError("%r is not a valid index for facedimension %r" % (face, facedim))
                    if (idx_n != fidx) or (ax_n != axis) or (rev_n != rev):
                        raise ValueError(
                            "Face link mismatch: neighbor doesn't"
                            " correctly link back to this face. "
                            "face: %r, axis: %r, position: %r, "
                            "rev: %r, link: %r, neighbor_link: %r"
                            % (fidx, axis, position, rev, link, neighbor_link)
                        )
                    checked.append((idx, self.axes[ax], rev))
                per_axis.setdefault(axis, {})[fidx] = tuple(checked)
        for axis, links in per_axis.items():
            self.axes[axis]._facedim = facedim
            self.axes[axis]._face_connections = links
        # axes that any link touches, as the linked edge or as the neighbour's axis
        self._connected_axes = set(per_axis)
        for links in face_links.values():
            for pair in links.values():
                self._connected_axes.update(link[1] for link in pair if link is not None)

    def _links_swap_axes(self, ax_name: str, first_face: bool = False):
        """does any face link on `ax_name` lead to ANOTHER axis of the neighbour (or any link of another axis lead here)?
        `first_face`: the lowest face number that has such a link (None if none) instead of a bool"""
        if self._face_connections is None:
            return None if first_face else False
        hits = []
        for faces in self._face_connections.values():
            for face, links in faces.items():
                for axis, pair in links.items():
                    for link in pair:
                        if link is not None and (axis == ax_name or link[1] == ax_name) and link[1] != axis:
                            hits.append(face)
        if first_face:
            return min(hits) if hits else None
        return bool(hits)

    def _validate_folds(self) -> None:
        """Resolve north-fold paddings: the seam is the one explicitly periodic other axis."""
        self._folds = {}
        for axname, axis in self.axes.items():
            spec = axis._padding
            if not FoldSpec.looks_like(spec):
                continue
            candidates = [o for o in self.axes if o != axname and o in self._explicitly_periodic_axes]
            if not candidates:
                raise ValueError(
                    f"A fold padding on axis {axname!r} requires an explicitly "
                    "periodic seam axis (the zonal wrap), but no other axis was "
                    "explicitly marked periodic. Set e.g. "
                    "padding={'X': 'periodic', '" + str(axname) + "': {'fold': ...}}."
                )
            if len(candidates) > 1:
                raise ValueError(
                    f"A fold padding on axis {axname!r} is ambiguous: more than one "
                    f"explicitly periodic axis could be the seam ({candidates}). "
                    "Multiple candidate seam axes are not supported."
                )
            self._folds[axname] = {"seam_axis": candidates[0], "pivot": spec["fold"], "south": spec["south"]}
        if self._folds and self._face_connections is not None:
            raise NotImplementedError(
                "Combining a north-fold boundary with face_connections is not "
                f"supported (fold axes: {sorted(self._folds)}). Use one or the "
                "other."
            )
        if self._folds:
            warnings.warn(
                "The north-fold (tripolar) boundary condition is experimental. "
                "Its API and numerical behavior may change in future releases, "
                "and it has not yet been validated across the full range of grid "
                "configurations. Please review results carefully and report any "
                "issues at https://github.com/xgcm/xgcm/issues.",
                category=UserWarning,
            )

    # ---- kwarg plumbing (reference grid.py:291-332) -----------------------------------------
    def _map_kwargs_over_axes(self, kwargs, axes: Optional[Iterable[str]] = None) -> Dict[str, Any]:
        if isinstance(kwargs, dict):
            return kwargs
        return {ax: kwargs for ax in (self.axes if axes is None else axes)}

    def _complete_user_kwargs_using_axis_defaults(self, user_kwargs, property: str) -> Dict[str, Any]:
        defaults = {ax: getattr(self.axes[ax], property) for ax in self.axes}
        if user_kwargs is None:
            return defaults
        return {**defaults, **self._map_kwargs_over_axes(user_kwargs)}

    def __repr__(self) -> str:
        lines = ["<xgcm.Grid>"]
        for name, axis in self.axes.items():
            lines.append("%s Axis (%s, padding=%r):" % (name, "periodic" if axis.periodic else "not periodic", axis.padding))
            lines += axis._coord_desc()
        return "\n".join(lines)

    # ---- deferred results (xgcm_amd.lazy) -----------------------------------------------------
    @contextlib.contextmanager
    def fused(self):
        """Inside the block the built-in 1-D operators return deferred results (`xgcm_amd.lazy.LazyArray`): chains of
        them and `+ - * /` are matched against the fused kernels when a value is first used -- bit-identical to the
        eager chain, one launch instead of three or four.  Per thread; nests."""
        depth = getattr(self._fuse_local, "depth", 0)
        self._fuse_local.depth = depth + 1
        _lazy.enter()
        try:
            yield self
        finally:
            _lazy.leave()
            self._fuse_local.depth = depth

    @property
    def _fusing(self) -> bool:
        return self._fuse or getattr(self._fuse_local, "depth", 0) > 0

    # ---- residency helpers ------------------------------------------------------------------
    def _resident(self, da: DataArray, like) -> DataArray:
        """Metric arrays of grid._own_ds are uploaded once and kept in HBM while HBM data is processed."""
        if _is_tensor(da.data) or not _is_tensor(like):
            return da
        key = id(da.data)
        if key not in self._metric_ids:  # temporaries (e.g. dx*dy products) are uploaded, not cached
            return da._replace(data=_dev.asdevice(da.data))
        hit = self._device_cache.get(key)
        if hit is None or hit[0] is not da.data:
            hit = (da.data, _dev.asdevice(da.data))
            self._device_cache[key] = hit
        return da._replace(data=hit[1])

    @staticmethod
    def _wrap_in(obj):
        """xarray objects -> xgcm_amd labelled objects; returns (obj, was_xarray)."""
        if isinstance(obj, dict):
            conv = {k: Grid._wrap_in(v) for k, v in obj.items()}
            return {k: v[0] for k, v in conv.items()}, any(v[1] for v in conv.values())
        if is_xarray(obj):
            return from_xarray(obj), True
        return obj, False

    # ---- metrics (reference grid.py:472-657) ------------------------------------------------
    @property
    def _metrics(self):
        """{frozenset(axes): [metric, ...]} in the container type of the dataset the grid was given (the reference keeps
        `ds[name].reset_coords(drop=True)` there and its tests read it); the operators use `_own_metrics`"""
        if isinstance(self._ds, Dataset):
            return self._own_metrics
        return {k: [to_xarray(m) for m in ms] for k, ms in self._own_metrics.items()}

    def set_metrics(self, key, value, overwrite: bool = False) -> None:
        metric_axes = frozenset(_maybe_promote_str_to_list(key))
        missing = [ma for ma in metric_axes if ma not in self.axes]
        if missing:
            raise KeyError(f"Metric axes {missing!r} not compatible with grid axes {tuple(self.axes)!r}")
        varnames = _maybe_promote_str_to_list(value)
        for v in varnames:
            if v not in self._own_ds:  # (membership only: a converted xarray.Dataset loads a variable when it is indexed)
                raise KeyError(f"Metric variable {v} not found in dataset.")
        if metric_axes in self._own_metrics:
            # NB the reference only considers the LAST name of `value` here (grid.py:488-512)
            new = self._own_ds[varnames[-1]].reset_coords(drop=True)
            replaced = False
            for i, old in enumerate(self._own_metrics[metric_axes]):
                if set(new.dims) == set(old.dims):
                    if not overwrite:
                        raise ValueError(
                            f"Metric variable {old.name} with dimensions {old.dims} already assigned in metrics."
                            f" Overwrite {old.name} with {varnames[-1]} by setting overwrite=True."
                        )
                    self._own_metrics[metric_axes][i] = new
                    replaced = True
            if not replaced:
                self._own_metrics[metric_axes].append(new)
        else:
            self._own_metrics[metric_axes] = [self._own_ds[v].reset_coords(drop=True) for v in varnames]
        self._metric_ids = {id(m.data) for ms in self._own_metrics.values() for m in ms}

    def _get_dims_from_axis(self, da, axis) -> List[str]:
        da = _maybe_unpack_vector_component(da)
        dims = []
        for ax in _maybe_promote_str_to_list(axis):
            if ax not in self.axes:
                raise KeyError(f"Did not find axis {ax} from data array {da.name}")
            found = [d for d in self.axes[ax].coords.values() if d in da.dims]
            if len(found) != 1:
                raise ValueError(
                    f"Did not find single matching dimension {da.dims} from {da.name} corresponding to axis {ax}, got {found}."
                )
            dims.append(found[0])
        return dims

    def get_metric(self, array, axes, _layout=None, _factors=False):
        """Metric that broadcasts against `array` for the given axes (conditions 1-4 of the reference).

        Condition 4, the reference's rule kept for parity: when no product of registered metrics sits at the array's
        position, the LAST product of the first candidate combination is interpolated there with `extend`, whatever else is
        registered.  With MITgcm's set (dxC, dxG, drF, drC at ZL and ZO; no dxF) the (X, Z) metric of a cell-centre field is
        dxG * drC(ZO) averaged to the levels -- about 3/4 of drF at the two end levels, the half cells -- not dxG * drF.

        `_layout` (internal, the operators pass the dims of the array they weight): a metric that has to be formed
        as a PRODUCT of registered metrics (a volume = area(Y,X) * thickness(Z)) is laid out with its dims in that
        order.  xarray's order -- first factor's dims, then the new ones: (Y, X, Z) -- made every use a transposed
        5 GB copy: `integrate(T, [X, Y, Z])` took 16 ms.  Same factors in the same order, same values."""
        if is_xarray(array):  # xarray in -> xarray out, like every other method (the reference hands back `grid._ds`'s own)
            return to_xarray(self.get_metric(from_xarray(array), axes))

        def product(parts):
            if _factors:  # internal: the factors themselves (separable weights are applied stage by stage)
                return tuple(parts)
            if _layout is None:
                return functools.reduce(operator.mul, parts[1:], parts[0])
            acc = parts[0]
            for p in parts[1:]:
                acc = acc._binary(p, "mul", dims_order=tuple(_layout))
            return acc

        array_dims = set(array.dims)
        self._get_dims_from_axis(array, frozenset(axes))
        registered = set(tuple(k) for k in self._own_metrics.keys())
        wanted = set(itertools.permutations(tuple(axes)))
        exact = registered.intersection(wanted)
        found = None
        if exact:
            candidates = self._own_metrics[frozenset(*exact)]
            for mv in candidates:  # (1) registered under these axes at this position
                if set(mv.dims).issubset(array_dims):
                    found = mv
                    break
            if found is None:  # (2) registered under these axes elsewhere: interpolate it
                mv = candidates[-1]
                warnings.warn(
                    f"Metric at {array.dims} being interpolated from metrics at dimensions {mv.dims}. Boundary value set to 'extend'."
                )
                found = self.interp_like(mv, array, "extend", None)
        else:
            fallback = None
            fallback_locked = False
            for combo in iterate_axis_combinations(axes):
                try:
                    pools = [self._own_metrics[ac] for ac in combo]
                except KeyError:
                    continue
                for pick in itertools.product(*pools):
                    if set(d for mv in pick for d in mv.dims).issubset(array_dims):
                        found = product(pick)  # (3) product of sub-axis metrics
                        break
                    if not fallback_locked:
                        fallback = pick
                if found is not None:
                    break
                fallback_locked = True
            if found is None and fallback is not None:  # (4) interpolate the fallback combination
                warnings.warn(
                    f"Metric at {array.dims} being interpolated from metrics at dimensions {[pc.dims for pc in fallback]}. Boundary value set to 'extend'."
                )
                parts = [self.interp_like(pc, array, "extend", None) for pc in fallback]
                found = product(parts)
        if found is None:
            raise KeyError(f"Unable to find any combinations of metrics for array dims {array_dims!r} and axes {axes!r}")
        if _factors and not isinstance(found, tuple):
            found = (found,)
        return found

    def interp_like(self, array, like, padding=None, fill_value=None, **kwargs):
        """Interpolate `array` onto the positions of `like` wherever they differ (grid.py:659-716)."""
        if "boundary" in kwargs:
            raise ValueError("Argument 'boundary' has been renamed to 'padding'. Please use 'padding' instead.")
        shifted = []
        for name, axis in self.axes.items():
            try:
                here, _ = axis._get_position_name(array)
                there, _ = axis._get_position_name(like)
            except KeyError:
                continue
            if here != there:
                shifted.append(name)
        # like the reference (grid.py:710-715) the target position is NOT passed on: each axis moves by
        # its default shift, which is `like`'s position on the usual two-position (center + one edge) axes
        out = self._1d_grid_ufunc_dispatch("interp", array, shifted, fill_value=fill_value, padding=padding)
        if is_xarray(like) and isinstance(out, DataArray):  # (a registered metric of ours interpolated like an xarray field)
            out = to_xarray(out)
        return out

    # ---- the hot path: 1-D operators ---------------------------------------------------------
    def _create_1d_grid_ufunc_signatures(self, da, axis, to) -> List[_GridUFuncSignature]:
        sigs = []
        for ax_name in axis:
            ax = self.axes[ax_name]
            from_pos, _ = ax._get_position_name(da)
            to_pos = to[ax_name]
            if to_pos is None:
                to_pos = ax._default_shifts[from_pos]
            sigs.append(_GridUFuncSignature.from_string(f"({ax_name}:{from_pos})->({ax_name}:{to_pos})"))
        return sigs

    def _1d_grid_ufunc_dispatch(self, funcname, data, axis, to=None, metric_weighted=None, other_component=None,
                                _divide_by=None, **kwargs):
        """Apply the matching built-in 1-D grid ufunc along each axis in turn (grid.py:728-836).

        `_divide_by` (internal, used by `derivative`): axes tuple whose metric at the OUTPUT position
        divides the result of the (single) axis inside the same kernel launch."""
        if "keep_coords" in kwargs:
            raise ValueError(
                "The 'keep_coords' argument has been removed. Coordinates compatible with the output are now always preserved."
            )
        data, was_xr = self._wrap_in(data)
        if isinstance(axis, str):
            axis = [axis]
        data = _check_data_input(data, self)
        first = _maybe_unpack_vector_component(data)
        chunked = getattr(first, "chunks", None) is not None
        if chunked and (isinstance(data, dict) or other_component is not None or any(gridops.complex_topology(self, a) for a in axis)):
            raise NotImplementedError(CHUNKED_INPUT_MESSAGE)  # (halos from other faces / partner components: whole arrays)
        to = self._map_kwargs_over_axes(to)
        if isinstance(metric_weighted, str):
            metric_weighted = (metric_weighted,)
        metric_weighted = self._map_kwargs_over_axes(metric_weighted)
        signatures = self._create_1d_grid_ufunc_signatures(first, axis=axis, to=to)

        array = first
        vector_key = next(iter(data)) if isinstance(data, dict) else None
        steps = list(zip(signatures, axis))
        i = 0
        while i < len(steps):
            sig, ax_name = steps[i]
            if (i + 1 < len(steps) and vector_key is None and other_component is None and _divide_by is None
                    and not (self._fusing and isinstance(array, _lazy.LazyArray))):
                w_a = metric_weighted.get(ax_name) if isinstance(metric_weighted, dict) else None
                w_b = metric_weighted.get(steps[i + 1][1]) if isinstance(metric_weighted, dict) else None
                fused = None
                if not w_a and not w_b:
                    fused = self._two_axes_in_one_pass(funcname, array, steps[i], steps[i + 1], kwargs)
                elif w_a and w_b and tuple(w_a) == tuple(w_b):  # metric_weighted=("X", "Y") on both axes: three metric planes
                    fused = self._two_axes_in_one_pass(funcname, array, steps[i], steps[i + 1], kwargs, weighted=tuple(w_a))
                if fused is not None:
                    array = fused
                    i += 2
                    continue
            i += 1
            ufunc, remaining = _select_grid_ufunc(funcname, sig, module=gridops, **kwargs)
            if chunked and funcname != "cumsum":
                _refuse_chunked_core_dim_with_changing_length(self, first, ax_name, sig)
            weighted = metric_weighted.get(ax_name) if isinstance(metric_weighted, dict) else None
            out_dims = _shifted_dims(self, array, ax_name, sig.out_ax_positions[0][0], sig.in_ax_positions[0][0])
            m_in = m_out = None
            post_divide = late_error = None
            if weighted:
                m_in = self._resident(self.get_metric(array, weighted, _layout=array.dims), _lazy.like(array))
                if any(d not in array.dims for d in m_in.dims):
                    # the metric found (interpolated by default shifts, so not always onto the array's points) carries a
                    # dim the array lacks: the reference's `array * metric` broadcasts by name into an outer product
                    # BEFORE the operator (xgcm/grid.py:804-808) -- the explicit product does the same
                    array = _lazy.plain(array) * m_in
                    m_in = None
                    out_dims = _shifted_dims(self, array, ax_name, sig.out_ax_positions[0][0], sig.in_ax_positions[0][0])
                try:
                    m_out = self._resident(self.get_metric(_DimsOnly(out_dims, array.name), weighted, _layout=out_dims), _lazy.like(array))
                except (KeyError, ValueError) as exc:
                    late_error = exc  # the reference looks this metric up AFTER the operator ran (:829-831): its errors first
                if m_out is not None and any(d not in out_dims for d in m_out.dims):
                    post_divide, m_out = m_out, None  # ... and `array / metric` AFTER it, likewise by name
            if _divide_by is not None and late_error is None:
                try:
                    dx = self._resident(self.get_metric(_DimsOnly(out_dims, array.name), _divide_by, _layout=out_dims), _lazy.like(array))
                except (KeyError, ValueError) as exc:
                    late_error, dx = exc, None  # `grid.diff(...)` first, then the metric (xgcm/grid.py:1576-1578)
                if dx is None:
                    pass
                elif any(d not in out_dims for d in dx.dims):
                    # the metric found for the result does not live on the result's points (drC on Zp1 interpolated to Z
                    # for a difference that went to Zl ...): the reference's `diff / dx` then BROADCASTS by name into an
                    # outer product (xgcm/grid.py:1576-1578) -- the explicit quotient does the same
                    post_divide = dx
                elif m_out is None:
                    m_out = dx
                else:
                    post_divide = dx  # two successive divisions cannot be merged bit-exactly
            if sum(d in array.dims for d in self.axes[ax_name].coords.values()) > 1 and any(
                    any(w) for w in (getattr(ufunc, "padding_width", None) or {}).values()):
                # a metric product (this step's or an earlier one's) gave the array a second dim of this axis: the
                # reference's pad looks the axis' dim up again and refuses (xgcm/padding.py:595); an operator that pads
                # nothing goes on with the dim its signature names
                self.axes[ax_name]._get_position_name(array)
            arg = {vector_key: array} if vector_key is not None else array
            if isinstance(ufunc, gridops.HipGridUFunc):
                if m_in is not None and gridops.complex_topology(self, ax_name) and (vector_key is not None or other_component is not None):
                    # halos come from other faces / the folded row and must be halos of the PRODUCT (the reference
                    # multiplies first, grid.py:804-808).  A scalar field takes them as the product of two halo slabs and
                    # stays in ONE pass (gridops._fused); a vector component's halos mix components: explicit product
                    # pass, then the halo-fused kernel with the output metric
                    array = array * m_in
                    arg = {vector_key: array} if vector_key is not None else array
                    m_in = None
                if self._fusing and post_divide is None and late_error is None:
                    deferred = _lazy.defer_stencil(self, funcname, ufunc, sig, arg, ax_name, other_component, m_in, m_out,
                                                   remaining, out_dims)
                    if deferred is not None:
                        array = deferred
                        continue
                array = ufunc(self, _lazy.plain(arg), axis=[(ax_name,)], other_component=_lazy.plain(other_component),
                              metric_in=m_in, metric_out=m_out, **remaining)
            else:  # a plain GridUFunc registered in gridops (none of the built-ins): unfused sequence
                if m_in is not None:
                    array = array * m_in
                    arg = {vector_key: array} if vector_key is not None else array
                array = ufunc(self, arg, axis=[(ax_name,)], other_component=other_component, **remaining)
                if m_out is not None:
                    array = array / m_out
            if late_error is not None:
                raise late_error
            if (m_in is not None or m_out is not None) and array.name is not None:
                array = array._replace(name=_name_after(array.name, m_in, m_out))
            if post_divide is not None:
                array = array / post_divide
        if was_xr and isinstance(array, _lazy.LazyArray) and array.is_deferred:
            # deferred: converting now would evaluate it.  The result stays a LazyArray -- it combines with xarray objects
            # through `+ - * /` like the arrays it came from -- and `.compute()` / `.to_xarray()` hand over the
            # xarray.DataArray, as `.compute()` of a dask-backed result does there
            array._xr = True
            return array
        return to_xarray(array) if was_xr else array

    def _two_axes_in_one_pass(self, funcname, array, step_a, step_b, kwargs, weighted=None):
        """`op` along two axes that are the LAST TWO dims of `array` in one kernel launch
        (xg_stencil2d_f64): same bits as the two sequential passes of the reference loop
        (xgcm/grid.py:800-832, whose TODO at :798-800 asks for exactly this), half the traffic.
        Returns None when the pair does not qualify; the caller then runs the axes one by one."""
        if funcname not in ("diff", "interp", "min", "max") or set(kwargs) - {"padding", "fill_value"}:
            return None
        if array.ndim < 2 or getattr(array, "chunks", None) is not None:
            return None
        if gridops.is_integer_data(array.data):
            return None  # integers: one axis at a time on int64 lanes (interp leaves the integer domain between the axes)
        if _dt.np_dtype(array.data) == np.float16:
            return None  # float16 is a storage type: numpy rounds to it BETWEEN the axes -- one axis at a time (found by the GPU sweep)
        (sig_a, ax_a), (sig_b, ax_b) = step_a, step_b
        if ax_a == ax_b or gridops.complex_topology(self, ax_a) or gridops.complex_topology(self, ax_b):
            return None  # halos from other faces / the folded row: one axis at a time (xg_stencil1d_halo)
        try:
            ufa, _ = _select_grid_ufunc(funcname, sig_a, module=gridops)
            ufb, _ = _select_grid_ufunc(funcname, sig_b, module=gridops)
        except NotImplementedError:
            return None  # (one axis at a time, so that the error -- if any -- is the one of the FIRST bad axis, as there)
        if not (isinstance(ufa, gridops.HipGridUFunc) and isinstance(ufb, gridops.HipGridUFunc)):
            return None
        try:
            dim_a = self.axes[ax_a].coords[ufa.from_pos]
            dim_b = self.axes[ax_b].coords[ufb.from_pos]
            out_a = self.axes[ax_a].coords[ufa.to_pos]
            out_b = self.axes[ax_b].coords[ufb.to_pos]
        except KeyError:
            return None
        if {dim_a, dim_b} != set(array.dims[-2:]):
            return None
        pad_a = tuple(next(iter(ufa.padding_width.values())))
        pad_b = tuple(next(iter(ufb.padding_width.values())))
        bc = self._complete_user_kwargs_using_axis_defaults(kwargs.get("padding"), "padding")
        fv = self._complete_user_kwargs_using_axis_defaults(kwargs.get("fill_value"), "fill_value")
        if any(not isinstance(bc[a], str) for a in (ax_a, ax_b)):
            return None  # missing boundary condition / fold spec: the sequential path raises the right error
        x_is_a = array.dims[-1] == dim_a
        padx, pady = (pad_a, pad_b) if x_is_a else (pad_b, pad_a)
        ax_x, ax_y = (ax_a, ax_b) if x_is_a else (ax_b, ax_a)
        if not _dev.stencil2d_supported(array.data, padx, pady):
            return None
        host = not _is_tensor(array.data)
        planes = None
        named = array.name
        if weighted is not None:
            # the metric at the input positions, between the two axes and at the output positions (xgcm/grid.py:804-828
            # multiplies before and divides after EACH axis); each must be a plain (Y, X) plane over the last two dims
            dims_mid = tuple(out_a if d == dim_a else d for d in array.dims)
            dims_out = tuple(out_b if d == dim_b else d for d in dims_mid)
            planes = []
            for dims in (array.dims, dims_mid, dims_out):
                try:
                    m = self.get_metric(_DimsOnly(dims, array.name), weighted, _layout=dims)
                except (KeyError, ValueError):
                    return None
                if tuple(m.dims) != tuple(dims[-2:]) or tuple(m.shape) != tuple(array.shape[-2:]):
                    return None  # broadcast / extra dims: the per-axis kernels take any metric pattern
                if _dt.np_dtype(m.data) != _dt.np_dtype(array.data):
                    return None  # mixed precision (a float32 field, float64 metrics): numpy's steps, one axis at a time
                planes.append(self._resident(m, array.data).data)
                named = _name_after(named, m)
        out = _dev.stencil2d(funcname, array.data, 0 if x_is_a else 1, padx, bc[ax_x], fill_of(fv[ax_x]), pady,
                             bc[ax_y], fill_of(fv[ax_y]), **({"metrics": planes} if planes is not None else {}))
        rename = {dim_a: out_a, dim_b: out_b}
        res = DataArray(_dev.tohost(out) if host else out, tuple(rename.get(d, d) for d in array.dims), name=named)
        return _reattach_coords([res], self, None, {out_a, out_b}, [array])[0]

    def interp(self, da, axis, **kwargs):
        """Interpolate neighboring points to the intermediate grid point along this axis."""
        return self._1d_grid_ufunc_dispatch("interp", da, axis, **kwargs)

    def diff(self, da, axis, **kwargs):
        """Difference neighboring points to the intermediate grid point."""
        return self._1d_grid_ufunc_dispatch("diff", da, axis, **kwargs)

    def min(self, da, axis, **kwargs):
        """Minimum of neighboring points on the intermediate grid point."""
        return self._1d_grid_ufunc_dispatch("min", da, axis, **kwargs)

    def max(self, da, axis, **kwargs):
        """Maximum of neighboring points on the intermediate grid point."""
        return self._1d_grid_ufunc_dispatch("max", da, axis, **kwargs)

    def _apply_vector_function(self, function, vector, **kwargs):
        """Each component of a C-grid vector moved to the cell centre with the other one as its
        `other_component` (reference grid.py:1420-1471; deprecated there, kept for its tests)."""
        if not (isinstance(vector, dict) and len(vector) == 2):
            raise ValueError(
                "Input is expected to be a dictionary with two key/value pairs which map grid axis to the vector component parallel to that axis"
            )
        warnings.warn(
            "`interp_2d_vector` and `diff_2d_vector` will be removed from future releases."
            "The same functionality will be accessible under the `xgcm.Grid.diff` and `xgcm.Grid.interp` methods, please see those docstrings for details.",
            category=DeprecationWarning,
        )
        to = kwargs.get("to", "center")
        if to != "center":
            raise NotImplementedError("Only vector interpolation to cell center is implemented, but got to=%r" % to)
        for axis_name, component in vector.items():
            position, _ = self.axes[axis_name]._get_position_name(self._wrap_in(component)[0])
            if position == "center":
                raise NotImplementedError(
                    "Only vector interpolation to cell "
                    "center is implemented, but vector "
                    "%s component is defined at center "
                    "(dims: %r)" % (axis_name, tuple(component.dims))
                )
        x_name, y_name = list(vector)
        x_component = function({x_name: vector[x_name]}, x_name, other_component={y_name: vector[y_name]}, **kwargs)
        y_component = function({y_name: vector[y_name]}, y_name, other_component={x_name: vector[x_name]}, **kwargs)
        return {x_name: x_component, y_name: y_component}

    def diff_2d_vector(self, vector, **kwargs):
        """Difference a 2D vector to the intermediate grid point (complex topologies)."""
        return self._apply_vector_function(self.diff, vector, **kwargs)

    def interp_2d_vector(self, vector, **kwargs):
        """Interpolate a 2D vector to the intermediate grid point (complex topologies)."""
        return self._apply_vector_function(self.interp, vector, **kwargs)

    def derivative(self, da, axis, **kwargs):
        """Centered-difference derivative: `diff(da, axis) / get_metric(diff, (axis,))` (grid.py:1576-1578)."""
        return self._1d_grid_ufunc_dispatch("diff", da, axis, _divide_by=(axis,), **kwargs)

    def cumsum(self, da, axis, to=None, padding=None, fill_value=None, metric_weighted=None, reverse=False, **kwargs):
        """Cumulative sum along `axis`, shifted to the neighbouring position (grid.py:1183-1418)."""
        if "boundary" in kwargs:
            raise ValueError("Argument 'boundary' has been renamed to 'padding'. Please use 'padding' instead.")
        if "keep_coords" in kwargs:
            raise ValueError(
                "The 'keep_coords' argument has been removed. Coordinates compatible with the output are now always preserved."
            )
        pre_weight = kwargs.pop("_pre_weight", None)  # cumint: `da * metric` folded into the first scan's load
        if kwargs:
            raise TypeError(f"cumsum() got unexpected keyword argument(s): {list(kwargs)}")
        da, was_xr = self._wrap_in(da)
        if isinstance(axis, str):
            axis = [axis]
        to = self._map_kwargs_over_axes(to)
        if isinstance(reverse, dict):
            extra = [a for a in reverse if a not in axis]
            if extra:
                raise ValueError(
                    f"`reverse` was given for axes {extra} which are not being "
                    f"cumulatively summed (axis={axis}). Only pass `reverse` for "
                    f"the axes in `axis`."
                )
        reverse = self._map_kwargs_over_axes(reverse)
        if isinstance(metric_weighted, str):
            metric_weighted = (metric_weighted,)
        metric_weighted = self._map_kwargs_over_axes(metric_weighted)
        all_padding = self._complete_user_kwargs_using_axis_defaults(padding, "padding")
        all_fill = self._complete_user_kwargs_using_axis_defaults(fill_value, "fill_value")

        data = da
        for ax in [self.axes[name] for name in axis]:
            pos, dim = ax._get_position_name(da)
            rev = bool(reverse.get(ax.name, False))
            weighted = metric_weighted.get(ax.name) if isinstance(metric_weighted, dict) else None
            # (the steps below come in the reference's order, xgcm/grid.py:1303-1413, so that a call with several things
            # wrong raises the error the reference raises: input metric, trim table, pad, target dim, output metric)
            m_in = m_out = None
            weight_names = []  # the DataArrays whose products / quotients decide the result's name (xarray's rule)
            generic_pad = gridops.complex_topology(self, ax.name)
            if pre_weight is not None:
                if weighted or generic_pad:  # two input factors / pad-after route: explicit product first
                    data = data * pre_weight
                else:
                    m_in = _aligned_view(pre_weight, data.dims)
                    weight_names.append(pre_weight)
                pre_weight = None
            two_axis_dims = False
            if weighted:
                w_in = self.get_metric(data, weighted, _layout=data.dims)
                if any(d not in data.dims for d in w_in.dims):
                    # a metric that does not live on the field's points (found by default-shift interpolation): the
                    # reference's `data * metric` is an outer product by name (:1311-1313); its pad then looks the axis'
                    # dim up again and refuses an array that now has two of them (xgcm/padding.py:595)
                    data = data * self._resident(w_in, data.data)
                    two_axis_dims = True
                else:
                    weight_names.append(w_in)
                    m_in = _aligned_view(self._resident(w_in, data.data), data.dims)
            ax_to = to.get(ax.name) if isinstance(to, dict) else None
            if ax_to is None:
                ax_to = ax._default_shifts[pos]
            trim_lo, trim_hi, pad_lo, pad_hi = _cumsum_trim_pad(pos, ax_to, rev, ax)
            bc = all_padding[ax.name]
            if pad_lo or pad_hi:
                if two_axis_dims or sum(d in data.dims for d in ax.coords.values()) > 1:  # (this step's product or an earlier one's)
                    ax._get_position_name(data)
                if bc is None and not generic_pad:
                    raise no_boundary_error(ax.name)
                if not generic_pad and self._face_connections is not None and self._facedim in data.dims:
                    # (an axis no link touches: the reference's pad still walks the faces, xgcm/padding.py:394-396)
                    for i in range(data.sizes[self._facedim]):
                        if i not in self._face_connections[self._facedim]:
                            raise KeyError(i)
                if generic_pad:
                    # the topology's own refusals (a face the connections leave out, an open edge without a boundary
                    # condition) come from the reference's pad, i.e. BEFORE the target dim is looked up: run the checks now
                    swapping = self._links_swap_axes(ax.name, first_face=True) if (trim_lo or trim_hi) else None
                    trimmed_faces_do_not_fit = ValueError(
                        # the reference pads the TRIMMED cumulative field through the topology (xgcm/grid.py:1385-1395): across
                        # a link that swaps axes the trimmed faces (n x (n - 1)) no longer fit each other and its concat fails
                        f"cumsum along {ax.name!r} from {pos!r} to {ax_to!r} trims the field along an axis whose face "
                        "connections swap axes: the trimmed faces are no longer square and cannot exchange halos")
                    try:
                        pad(data, self, {ax.name: (pad_lo, pad_hi)}, padding=padding, fill_value=fill_value, _dry=True)
                    except KeyError as missing_face:
                        # (it walks the faces by number: the concat of a lower face fails before a missing one is looked up)
                        if swapping is not None and missing_face.args and isinstance(missing_face.args[0], int) \
                                and swapping < missing_face.args[0]:
                            raise trimmed_faces_do_not_fit from None
                        raise
                    if swapping is not None:
                        raise trimmed_faces_do_not_fit
            fv = all_fill[ax.name]
            new_dim = ax.coords[ax_to]
            out_dims = tuple(new_dim if d == dim else d for d in data.dims)
            post_divide = None
            if weighted:
                w_out = self.get_metric(_DimsOnly(out_dims, data.name), weighted, _layout=out_dims)
                if any(d not in out_dims for d in w_out.dims):
                    post_divide = w_out  # `reattached / metric` (:1411-1413), by name as well
                else:
                    weight_names.append(w_out)
                    m_out = _aligned_view(self._resident(w_out, data.data), out_dims)
            num = data.get_axis_num(dim)
            host = not _is_tensor(data.data)
            # xarray's DataArray.cumsum skips NaN for floats (numpy.nancumsum); see DESIGN.md "unpinned"
            if generic_pad:
                # complex topology: the reference pads the TRIMMED cumulative field through the topology (grid.py:1389-1395),
                # i.e. its halo cells are the neighbouring faces' (the folded row's) cumulative edge values
                if pad_lo or pad_hi:
                    # one pass: the scan writes the padded layout (halo cells hold a placeholder), the halo cells are
                    # gathered from that very buffer -- a (pad_lo + pad_hi)-wide slab -- and put in place: no padded copy
                    src = data.data
                    if host and getattr(src, "nbytes", 0) >= getattr(_dev, "HOST_STREAM_MIN_BYTES", float("inf")):
                        src = _dev.asdevice(src)  # (the block-streamed host route hands back host blocks: keep this one in HBM)
                    out = _dev.cumsum1d(src, num, trim_lo, trim_hi, pad_lo, pad_hi, "fill", 0, rev, True, m_in, None)
                    buf = DataArray(out, data.dims, name=data.name)
                    halo = halo_cells(InteriorOf(buf, dim, pad_lo, pad_hi), self, ax.name, (pad_lo, pad_hi), padding=padding,
                                      fill_value=fill_value)
                    if tuple(halo.shape) != tuple(n if i != num else pad_lo + pad_hi for i, n in enumerate(out.shape)):
                        # links that swap axes need square faces, and trimming the cumulative field along one of them
                        # (center -> left ...) breaks that: the reference's pad of the trimmed field is ill-defined too
                        raise ValueError(
                            f"cumsum along {ax.name!r} from {pos!r} to {ax_to!r} trims the field along an axis whose face "
                            "connections swap axes: the trimmed faces are no longer square and cannot exchange halos")
                    out = _dev.put_halo(out, halo.data, num, pad_lo, pad_hi)
                else:
                    out = _dev.cumsum1d(data.data, num, trim_lo, trim_hi, 0, 0, None, 0.0, rev, True, m_in, None)
                res = DataArray(_dev.tohost(out) if host else out, out_dims, name=data.name)
                if weighted:
                    res = res / self._resident(self.get_metric(res, weighted, _layout=res.dims), res.data)

            else:
                # integer data: numpy.cumsum's int64 / uint64 accumulator and numpy.pad's cast of the fill value, both in
                # the device layer (xgcm_amd.dtypes)
                out = _dev.cumsum1d(data.data, num, trim_lo, trim_hi, pad_lo, pad_hi,
                                    bc if (pad_lo or pad_hi) else None, 0.0 if fv is None else fv, rev, True, m_in, m_out)
                res = DataArray(_dev.tohost(out) if host else out, out_dims, name=data.name)
            if (m_in is not None or m_out is not None) and res.name is not None:
                res = res._replace(name=_name_after(res.name, *weight_names))
            if (pad_lo or pad_hi) and self._facedim is not None and self._facedim in res.dims and res.dims[0] != self._facedim:
                # on a grid with face connections the reference pads EVERY axis through `_pad_face_connections`, which
                # rebuilds the array with `xr.concat(faces, dim=facedim)` -- the face dim comes out FIRST -- and `Grid.cumsum`
                # (unlike diff / interp) does not restore the input's order (xgcm/padding.py:540-572, xgcm/grid.py:1385-1395):
                # the same dims order here, as a view (no copy)
                res = res.transpose(self._facedim, *[d for d in res.dims if d != self._facedim])
            data = _reattach_coords([res], self, {ax.name: (pad_lo, pad_hi)}, {new_dim}, [data])[0]
            if post_divide is not None:
                data = data / self._resident(post_divide, data.data)
        return to_xarray(data) if was_xr else data

    def integrate(self, da, axis, **kwargs):
        """Finite-volume integral `(da * metric).sum(dims)` along one or more axes (grid.py:1580-1605).

        The metric is `get_metric(da, axis)`'s.  Over several axes at a position where no product of registered metrics
        sits (the cell centre along X with MITgcm's set, which has no dxF) that is its condition 4: an interpolated
        product, dxG * drC(ZO) for (X, Z), first-order accurate on a closed column; integrate one axis at a time there."""
        da, was_xr = self._wrap_in(da)
        skipna = kwargs.pop("skipna", None)
        keep_attrs = kwargs.pop("keep_attrs", False)
        if kwargs:
            raise TypeError(f"sum() got unexpected keyword argument(s): {list(kwargs)}")
        dims = self._get_dims_from_axis(da, axis)
        skip = True if skipna is None else bool(skipna)
        factors = self._weight_factors(da, axis, dims)
        if factors is None:  # the weight adds dims to `da`: the explicit product (broadcast result)
            weight = self._resident(self.get_metric(da, axis, _layout=da.dims), da.data)
            out = (da * weight).sum(dims, skipna=skip, keep_attrs=keep_attrs)
        else:
            # (`keep_attrs` keeps the attrs of what is summed -- the PRODUCT `da * metric`, which has none: xarray's binary
            # operators drop them; the reference's results carry no attrs either way)
            out = self._weighted_reduce(da, factors, dims, skip, False)
            # `da * weight` of the reference: nameless unless the weight carries the field's name (xarray's rule); a weight
            # that is itself a product of several metrics has no name
            weight_name = factors[0].name if len(factors) == 1 else None
            out = out._replace(name=da.name if weight_name == da.name else None)
        return to_xarray(out) if was_xr else out

    def _weight_factors(self, da, axis, dims):
        """The metric of `axis` for `da` as a list of FACTORS whose product it is (one factor unless the grid has
        to combine metrics, e.g. a volume = area(Y, X) * thickness(Z)); None when it has dims `da` lacks.
        Integrals over several axes apply each factor at the reduction that removes its first dim instead of
        materialising the product: `integrate(T, [X, Y, Z])` reads T once (8 B/cell), the product form moved a 3-D
        weight array as large as T as well.  The factor order of the reference is kept inside each stage; across
        stages the products associate differently -- multi-axis sums are tolerance results (1e-12) either way."""
        parts = [self._resident(f, da.data) for f in self.get_metric(da, axis, _factors=True)]
        if any(d not in da.dims for f in parts for d in f.dims):
            return None
        if any(not (set(f.dims) & set(dims)) for f in parts):  # a factor that none of the reductions removes
            parts = [functools.reduce(lambda a, b: a._binary(b, "mul", dims_order=tuple(da.dims)), parts[1:], parts[0])]
        return parts

    def _weighted_reduce(self, da, weight, dims, mode, keep_attrs=False):
        """sum over `dims` of da * weight, one `xg_reduce1d` launch per dim; `weight`: a DataArray or a list of factors,
        each riding in the launch that removes its first dim.  `mode`: skipna True / False; "valid" / "all" = the
        weights of the valid / of all cells of `da`; "mean_valid" / "mean_all" = the weighted mean (one dim: divided
        inside the kernel; several dims: numerator and denominator sums side by side, divided at the end)."""
        host = not _is_tensor(da.data)
        cur_dims = list(da.dims)
        data = da.data
        factors = list(weight) if isinstance(weight, (list, tuple)) else [weight]
        mean = mode in ("mean_valid", "mean_all")
        pair = mean and len(dims) > 1
        lead = []  # the leading pair dim once numerator / denominator travel together
        # a factor that has NONE of the summed dims (a metric registered under an axis it does not run along) still weights
        # every cell: it rides in the first launch, broadcast along the summed dim -- `(da * w).sum(d)`, not `w * da.sum(d)`
        loose = [f for f in factors if not any(d in f.dims for d in dims)]
        if factors and not loose and not any(dims[0] in f.dims for f in factors):
            # mixed precision with an unweighted first stage (a float32 field, float64 metrics that lack the first summed
            # dim): numpy has promoted the PRODUCT before it sums anything -- the field is widened first (x * 1.0 is exact)
            wide = np.result_type(_dt.np_dtype(data), *[_dt.np_dtype(f.data) for f in factors])
            if wide != _dt.np_dtype(data) and wide.kind == "f" and _dt.np_dtype(data).kind == "f":
                data = (da * wide.type(1.0)).data
        for i, d in enumerate(dims):
            now = [f for f in factors if d in f.dims] + (loose if i == 0 else [])
            factors = [f for f in factors if d not in f.dims and not any(f is x for x in loose)]
            w = None
            if now:
                wf = functools.reduce(lambda a, b: a._binary(b, "mul", dims_order=tuple(cur_dims)), now[1:], now[0])
                w = _aligned_view(wf, cur_dims)
                if lead:
                    w = w[None]
            num = len(lead) + cur_dims.index(d)
            if i == 0:
                step_mode = ({"mean_valid": "pair_valid", "mean_all": "pair_all"}[mode] if pair else mode)
            else:
                step_mode = mode if isinstance(mode, bool) else (mode == "mean_valid" if mean else False)
            data = _dev.reduce1d(data, num, w, step_mode)
            cur_dims.remove(d)
            if i == 0 and pair:
                lead = ["__pair__"]
        if pair:
            data = _dev.binary("div", data[0], data[1])
        coords = OrderedDict((k, c) for k, c in da.coords.items() if all(cd in cur_dims for cd in c.dims))
        return DataArray(_dev.tohost(data) if host else data, cur_dims, coords=coords, name=da.name,
                         attrs=da.attrs if keep_attrs else None)

    def cumint(self, da, axis, **kwargs):
        """Cumulative integral `cumsum(da * metric, axis)` (grid.py:1607-1660)."""
        da, was_xr = self._wrap_in(da)
        weight = self._resident(self.get_metric(da, axis, _layout=da.dims), da.data)
        if [d for d in weight.dims if d not in da.dims] or gridops.is_integer_data(da.data):
            res = self.cumsum(da * weight, axis, **kwargs)  # the product has more dims than `da` / integer data
        else:
            res = self.cumsum(da, axis, _pre_weight=weight, **kwargs)  # same products, formed inside the scan
        return to_xarray(res) if was_xr else res

    def average(self, da, axis, **kwargs):
        """Metric-weighted mean `sum(da*w) / sum(w where da valid)` (grid.py:1662-1685)."""
        da, was_xr = self._wrap_in(da)
        kwargs.pop("keep_attrs", None)
        skipna = kwargs.pop("skipna", None)
        if kwargs:
            raise TypeError(f"mean() got unexpected keyword argument(s): {list(kwargs)}")
        dims = self._get_dims_from_axis(da, axis)
        skip = True if skipna is None else bool(skipna)
        factors = self._weight_factors(da, axis, dims)
        if factors is None:  # weight adds dims: explicit broadcast products
            weight = self._resident(self.get_metric(da, axis, _layout=da.dims), da.data)
            num = (da * weight).sum(dims, skipna=skip)
            ones = _valid_mask(da) if skip else da._replace(data=_ones_like(da.data), coords=OrderedDict())
            den = (ones * weight).sum(dims, skipna=False)
            out = (num / den)._replace(name=da.name)  # (`da.weighted(w).mean(...)` keeps the array's name)
        else:
            # ONE pass over `da` (8 B/cell): sum(da * w) and sum(w over the valid cells) march together inside the
            # reduction kernel -- divided there for one dim, carried side by side through the remaining (small)
            # reductions for several (reference: product, mask, two sum arrays and a quotient array)
            out = self._weighted_reduce(da, factors, dims, "mean_valid" if skip else "mean_all")
        return to_xarray(out) if was_xr else out

    def apply_as_grid_ufunc(self, func, *args, axis=None, signature="", padding_width=None, padding=None,
                            fill_value=None, dask="forbidden", map_overlap=False, pad_before_func=True, **kwargs):
        """Apply a user function on unlabelled arrays in a grid-aware manner (generic path)."""
        return apply_as_grid_ufunc(func, *args, axis=axis, grid=self, signature=signature, padding_width=padding_width,
                                   padding=padding, fill_value=fill_value, dask=dask, map_overlap=map_overlap,
                                   pad_before_func=pad_before_func, **kwargs)

    def vorticity(self, u, v, x_axis: str = "X", y_axis: str = "Y", padding=None, fill_value=None,
                  metric_weighted: bool = True):
        """Fused relative vorticity `(diff(v, X) - diff(u, Y)) / area` in one kernel launch.

        Equivalent (bit for bit) to the chain of three reference operators
        `(grid.diff(v, X) - grid.diff(u, Y)) / grid.get_metric(zeta, (X, Y))` with both diffs
        center->left; the reference's own docs motivate fusing it (docs/grid_ufuncs.md:27).
        On grids with face connections or a north fold `u`, `v` are the X / Y components of a
        vector: the chain is then `(grid.diff({Y: v}, X, other_component={X: u}) -
        grid.diff({X: u}, Y, other_component={Y: v})) / area`, and the two one-cell halos are
        gathered through the topology's token map before the same single launch."""
        (u, xr1), (v, xr2) = self._wrap_in(u), self._wrap_in(v)
        xa, ya = self.axes[x_axis], self.axes[y_axis]
        vx_pos, vx_dim = xa._get_position_name(v)
        uy_pos, uy_dim = ya._get_position_name(u)
        if (vx_pos, uy_pos) != ("center", "center") or "left" not in xa.coords or "left" not in ya.coords:
            raise NotImplementedError("fused vorticity needs v at X:center, u at Y:center and left points on both axes")
        out_x, out_y = xa.coords["left"], ya.coords["left"]
        if u.dims[-2:] != (uy_dim, out_x) or v.dims[-2:] != (out_y, vx_dim) or u.dims[:-2] != v.dims[:-2]:
            raise NotImplementedError("fused vorticity needs u(..., YC, XG) and v(..., YG, XC) with (Y, X) last")
        out_dims = u.dims[:-2] + (out_y, out_x)
        if gridops.is_integer_data(u.data) or gridops.is_integer_data(v.data):
            # integer components: the operator chain itself, each step in numpy's dtype (the fused kernel is float-only)
            kw = dict(padding=padding, fill_value=fill_value)
            res = (self.diff({y_axis: v}, x_axis, other_component={x_axis: u}, **kw)
                   - self.diff({x_axis: u}, y_axis, other_component={y_axis: v}, **kw))
            if metric_weighted:
                res = res / self._resident(self.get_metric(res, (x_axis, y_axis)), res.data)
            return to_xarray(res) if (xr1 or xr2) else res
        area = None
        if metric_weighted:
            area = _aligned_view(self._resident(self.get_metric(_DimsOnly(out_dims), (x_axis, y_axis)), u.data), out_dims)
        bcx, bcy, fx, fy, hx, hy = self._two_component_halos(u, v, x_axis, y_axis, (1, 0), padding, fill_value,
                                                             x_of="v", y_of="u")
        host = not (_is_tensor(u.data) or _is_tensor(v.data))
        out = _dev.vorticity(u.data, v.data, area, bcx, bcy, fx, fy, hx, hy)
        res = DataArray(_dev.tohost(out) if host else out, out_dims)
        res = _reattach_coords([res], self, None, {out_x, out_y}, [u, v])[0]
        return to_xarray(res) if (xr1 or xr2) else res

    def _scalar_halos(self, a, x_axis, y_axis, widths, padding, fill_value):
        """Boundary modes, fill values and (on complex topologies) the pre-gathered one-cell halos of a
        scalar field along both axes, for the fused one-in / two-out operators."""
        bc = self._complete_user_kwargs_using_axis_defaults(padding, "padding")
        fv = self._complete_user_kwargs_using_axis_defaults(fill_value, "fill_value")
        modes, halos = {}, {}
        for ax in (x_axis, y_axis):
            if gridops.complex_topology(self, ax):
                halos[ax] = halo_cells(a, self, ax, widths, padding=padding, fill_value=fill_value).data
                modes[ax] = "halo"
            else:
                if bc[ax] is None:
                    raise no_boundary_error(ax)
                halos[ax] = None
                modes[ax] = bc[ax]
        return (modes[x_axis], modes[y_axis], fill_of(fv[x_axis]), fill_of(fv[y_axis]), halos[x_axis],
                halos[y_axis])

    def _two_component_halos(self, u, v, x_axis, y_axis, widths, padding, fill_value, x_of: str, y_of: str):
        """Boundary modes, fill values and (on complex topologies) the pre-gathered one-cell halos of the
        fused two-component operators: along X the halo of component `x_of`, along Y of `y_of`; `u` is
        the X-component, `v` the Y-component of the vector (rotation / sign rules of `padding.pad`)."""
        bc = self._complete_user_kwargs_using_axis_defaults(padding, "padding")
        fv = self._complete_user_kwargs_using_axis_defaults(fill_value, "fill_value")
        comp = {"u": ({x_axis: u}, {y_axis: v}), "v": ({y_axis: v}, {x_axis: u})}
        modes, halos = {}, {}
        for ax, which in ((x_axis, x_of), (y_axis, y_of)):
            if gridops.complex_topology(self, ax):
                arg, other = comp[which]
                halos[ax] = halo_cells(arg, self, ax, widths, padding=padding, fill_value=fill_value,
                                       other_component=dict(other)).data
                modes[ax] = "halo"
            else:
                if bc[ax] is None:
                    raise no_boundary_error(ax)
                halos[ax] = None
                modes[ax] = bc[ax]
        return (modes[x_axis], modes[y_axis], fill_of(fv[x_axis]), fill_of(fv[y_axis]), halos[x_axis],
                halos[y_axis])

    def divergence(self, u, v, x_axis: str = "X", y_axis: str = "Y", padding=None, fill_value=None,
                   metric_weighted: bool = True):
        """Fused horizontal divergence `(diff(u, X) + diff(v, Y)) / area` in one kernel launch.

        `u` lives on (Y:center, X:left), `v` on (Y:left, X:center); both differences go left -> center
        (the "Divergence" grid ufunc of the reference's docs/ufunc_examples.md, padding_width (0,1)),
        so the result sits at the cell centre and -- with `metric_weighted` -- is divided by the
        (X, Y) metric there.  Bit-identical to the chain of reference operators
        `(grid.diff(u, X) + grid.diff(v, Y)) / grid.get_metric(div, (X, Y))`; pass transports
        (u*dy, v*dx) for the finite-volume form."""
        (u, xr1), (v, xr2) = self._wrap_in(u), self._wrap_in(v)
        xa, ya = self.axes[x_axis], self.axes[y_axis]
        ux_pos, ux_dim = xa._get_position_name(u)
        uy_pos, uy_dim = ya._get_position_name(u)
        vx_pos, vx_dim = xa._get_position_name(v)
        vy_pos, vy_dim = ya._get_position_name(v)
        if (ux_pos, uy_pos, vx_pos, vy_pos) != ("left", "center", "center", "left"):
            raise NotImplementedError("fused divergence needs u at (Y:center, X:left) and v at (Y:left, X:center)")
        out_x, out_y = xa.coords["center"], ya.coords["center"]
        if u.dims[-2:] != (uy_dim, ux_dim) or v.dims[-2:] != (vy_dim, vx_dim) or u.dims[:-2] != v.dims[:-2]:
            raise NotImplementedError("fused divergence needs u(..., YC, XG) and v(..., YG, XC) with (Y, X) last")
        out_dims = u.dims[:-2] + (out_y, out_x)
        if gridops.is_integer_data(u.data) or gridops.is_integer_data(v.data):
            # integer components: the operator chain itself, each step in numpy's dtype (the fused kernel is float-only)
            kw = dict(padding=padding, fill_value=fill_value)
            res = (self.diff({x_axis: u}, x_axis, other_component={y_axis: v}, **kw)
                   + self.diff({y_axis: v}, y_axis, other_component={x_axis: u}, **kw))
            if metric_weighted:
                res = res / self._resident(self.get_metric(res, (x_axis, y_axis)), res.data)
            return to_xarray(res) if (xr1 or xr2) else res
        area = None
        if metric_weighted:
            area = _aligned_view(self._resident(self.get_metric(_DimsOnly(out_dims), (x_axis, y_axis)), u.data), out_dims)
        bcx, bcy, fx, fy, hx, hy = self._two_component_halos(u, v, x_axis, y_axis, (0, 1), padding, fill_value,
                                                             x_of="u", y_of="v")
        host = not (_is_tensor(u.data) or _is_tensor(v.data))
        out = _dev.divergence(u.data, v.data, area, bcx, bcy, fx, fy, hx, hy)
        res = DataArray(_dev.tohost(out) if host else out, out_dims)
        res = _reattach_coords([res], self, None, {out_x, out_y}, [u, v])[0]
        return to_xarray(res) if (xr1 or xr2) else res

    def gradient(self, a, x_axis: str = "X", y_axis: str = "Y", padding=None, fill_value=None,
                 metric_weighted: bool = False):
        """Fused horizontal gradient of a cell-centre field: `(diff(a, X), diff(a, Y))` -- with
        `metric_weighted` `(derivative(a, X), derivative(a, Y))` -- in ONE kernel launch that reads the
        field once (the "Gradient" grid ufunc of the reference's docs/ufunc_examples.md, center -> left,
        padding_width (1, 0) on both axes).  Bit-identical to the two operator calls; on a complex
        topology (face connections / fold) the two one-cell halos of the field are gathered through the
        token map first, then the same single launch runs."""
        a, was_xr = self._wrap_in(a)
        xa, ya = self.axes[x_axis], self.axes[y_axis]
        x_pos, x_dim = xa._get_position_name(a)
        y_pos, y_dim = ya._get_position_name(a)
        if (x_pos, y_pos) != ("center", "center") or "left" not in xa.coords or "left" not in ya.coords:
            raise NotImplementedError("fused gradient needs a field at (Y:center, X:center) and left points on both axes")
        op = self.derivative if metric_weighted else self.diff
        if a.dims[-2:] != (y_dim, x_dim) or gridops.is_integer_data(a.data):  # (integers: the float-only fused kernel is not theirs)
            kw = dict(padding=padding, fill_value=fill_value)
            res = op(a, x_axis, **kw), op(a, y_axis, **kw)
            return tuple(to_xarray(r) for r in res) if was_xr else res
        bcx, bcy, fx, fy, hx, hy = self._scalar_halos(a, x_axis, y_axis, (1, 0), padding, fill_value)
        dims_x = a.dims[:-1] + (xa.coords["left"],)
        dims_y = a.dims[:-2] + (ya.coords["left"], x_dim)
        mx = my = None
        if metric_weighted:
            mx = _aligned_view(self._resident(self.get_metric(_DimsOnly(dims_x), (x_axis,)), a.data), dims_x)
            my = _aligned_view(self._resident(self.get_metric(_DimsOnly(dims_y), (y_axis,)), a.data), dims_y)
        host = not _is_tensor(a.data)
        gx, gy = _dev.gradient(a.data, bcx, bcy, fx, fy, mx, my, hx, hy)
        rx = DataArray(_dev.tohost(gx) if host else gx, dims_x, name=a.name)
        ry = DataArray(_dev.tohost(gy) if host else gy, dims_y, name=a.name)
        rx = _reattach_coords([rx], self, None, {xa.coords["left"]}, [a])[0]
        ry = _reattach_coords([ry], self, None, {ya.coords["left"]}, [a])[0]
        return (to_xarray(rx), to_xarray(ry)) if was_xr else (rx, ry)

    def flux(self, u, v, tracer, x_axis: str = "X", y_axis: str = "Y", padding=None, fill_value=None):
        """Fused first-order advective flux of a cell-centre tracer: `(u * interp(T, X), v * interp(T, Y))`
        in one launch (the "Advection" flux of docs/ufunc_examples.md; u at (Y:center, X:left), v at
        (Y:left, X:center)).  Bit-identical to the chain of reference operators; `padding` /
        `fill_value` pad the tracer (on complex topologies: its pre-gathered halos)."""
        (u, xr1), (v, xr2), (t, xr3) = self._wrap_in(u), self._wrap_in(v), self._wrap_in(tracer)
        xa, ya = self.axes[x_axis], self.axes[y_axis]
        tx_pos, tx_dim = xa._get_position_name(t)
        ty_pos, ty_dim = ya._get_position_name(t)
        if (tx_pos, ty_pos) != ("center", "center") or "left" not in xa.coords or "left" not in ya.coords:
            raise NotImplementedError("fused flux needs the tracer at (Y:center, X:center) and left points on both axes")
        dims_x = t.dims[:-2] + (ty_dim, xa.coords["left"])
        dims_y = t.dims[:-2] + (ya.coords["left"], tx_dim)
        was_xr = xr1 or xr2 or xr3
        if (t.dims[-2:] != (ty_dim, tx_dim) or u.dims != dims_x or v.dims != dims_y
                or any(gridops.is_integer_data(q.data) for q in (u, v, t))):  # integers: each step in numpy's dtype
            kw = dict(padding=padding, fill_value=fill_value)
            res = u * self.interp(t, x_axis, **kw), v * self.interp(t, y_axis, **kw)
            return tuple(to_xarray(r) for r in res) if was_xr else res
        bcx, bcy, fvx, fvy, hx, hy = self._scalar_halos(t, x_axis, y_axis, (1, 0), padding, fill_value)
        host = not (_is_tensor(u.data) or _is_tensor(v.data) or _is_tensor(t.data))
        fx, fy = _dev.flux(u.data, v.data, t.data, bcx, bcy, fvx, fvy, hx, hy)
        rx = DataArray(_dev.tohost(fx) if host else fx, dims_x)
        ry = DataArray(_dev.tohost(fy) if host else fy, dims_y)
        rx = _reattach_coords([rx], self, None, {xa.coords["left"]}, [u, t])[0]
        ry = _reattach_coords([ry], self, None, {ya.coords["left"]}, [v, t])[0]
        return (to_xarray(rx), to_xarray(ry)) if was_xr else (rx, ry)

    # ---- fused second-order operators: the staggered intermediate of a two-step chain never reaches memory ----------
    def _second_order_plan(self, fields, x_axis, y_axis, padding, fill_value, metrics=()):
        """(bc_x, bc_y, fill_x, fill_y) when the one-pass kernel may serve a chain over `fields` (all at the same shape and
        float dtype, `metrics` in that dtype too, ordinary boundaries on both axes), else None: the chain itself runs"""
        if any(gridops.complex_topology(self, ax) for ax in (x_axis, y_axis)):
            return None  # the intermediate's own halo would have to be gathered across faces / the fold
        dtype = _dt.np_dtype(fields[0].data)
        if dtype not in (_dt.FLOAT32, _dt.FLOAT64) or any(_is_chunked(f.data) for f in fields):
            return None
        if any(tuple(f.shape) != tuple(fields[0].shape) or _dt.np_dtype(f.data) != dtype for f in fields):
            return None
        if any(_dt.np_dtype(m.data) != dtype for m in metrics):
            return None
        bc = self._complete_user_kwargs_using_axis_defaults(padding, "padding")
        fv = self._complete_user_kwargs_using_axis_defaults(fill_value, "fill_value")
        if bc[x_axis] is None or bc[y_axis] is None:
            return None  # (the chain raises the missing-boundary error)
        return bc[x_axis], bc[y_axis], fill_of(fv[x_axis]), fill_of(fv[y_axis])

    def _xyz_plan(self, fields, x_axis, y_axis, z_axis, padding, fill_value, metrics, z_modes=None):
        """`_second_order_plan`'s four extended by (bc_z, fill_z), else None: also where Z has no boundary (the chain raises)
        or one outside `z_modes`.  The one-axis operators of a chain hand their fill value on as it is (None: 0.0), so a
        -0.0 or a NaN keeps its bits on all three axes"""
        plan = self._second_order_plan(fields, x_axis, y_axis, padding, fill_value, metrics)
        if plan is None:
            return None
        bcz = self._complete_user_kwargs_using_axis_defaults(padding, "padding")[z_axis]
        if bcz is None or (z_modes is not None and bcz not in z_modes):
            return None
        return plan + (bcz, fill_of(self._complete_user_kwargs_using_axis_defaults(fill_value, "fill_value")[z_axis]))

    def _stage_metrics(self, stages, like, metric_weighted):
        """the metrics of the `stages` (dims, axes, name) of a one-pass operator, resident where `like` is; None each when
        not `metric_weighted`.  None, not served: a lookup raises (the chain raises it where the chain looks the metric
        up), a metric has a dim outside its stage, or one is chunked"""
        if not metric_weighted:
            return [None] * len(stages)
        try:
            mets = [self._resident(self.get_metric(_DimsOnly(dims, name), axes, _layout=dims), like) for dims, axes, name in stages]
        except (KeyError, ValueError):
            return None
        fits = all(set(m.dims) <= set(dims) and not _is_chunked(m.data) for m, (dims, _, _) in zip(mets, stages))
        return mets if fits else None

    def _column_points(self, x_axis, y_axis, z_axis, to):
        """(`to`, the points) of an operator over (lead, Z, Y, X) columns with faces at Z:`to` (None: `outer` where the Z axis
        has it, else `left`).  The points are None unless `to` is `left` or `outer` and a position of Z, all three axes
        have `center`, X and Y have `left`, and Z has no face connection or fold"""
        zax, yax, xax = self.axes[z_axis], self.axes[y_axis], self.axes[x_axis]
        if to is None:
            to = "outer" if "outer" in zax.coords else "left"
        if not (to in ("left", "outer") and to in zax.coords and all("center" in ax.coords for ax in (zax, yax, xax))
                and "left" in yax.coords and "left" in xax.coords and not gridops.complex_topology(self, z_axis)):
            return to, None
        held = set(zax.coords.values()) | set(yax.coords.values()) | set(xax.coords.values())
        return to, _ColumnPoints(zax.coords["center"], zax.coords[to], yax.coords["center"], yax.coords["left"],
                                 xax.coords["center"], xax.coords["left"], held)

    def flux_divergence(self, u, v, tracer, x_axis: str = "X", y_axis: str = "Y", padding=None, fill_value=None,
                        metric_weighted: bool = True):
        """Flux-form advection tendency `divergence(flux(u, v, tracer))` in ONE pass: u, v and the tracer are read once,
        the result written once (32 B/cell in float64 instead of the chain's 64); the flux stays in registers.

        u at (Y:center, X:left), v at (Y:left, X:center), the tracer and the result at the centre.  Bit-identical to
        `grid.divergence(*grid.flux(u, v, tracer, x_axis, y_axis, padding=padding, fill_value=fill_value), x_axis, y_axis,
        padding=padding, fill_value=fill_value, metric_weighted=metric_weighted)`, which pads twice: the tracer below /
        left of the first cell, then the FLUX above / right of the last one -- periodic: the flux at index 0, extend: at
        n-1, fill: `fill_value` itself.  That chain itself runs (the same calls in the same order) for integer, float16 or
        mixed dtypes (their promotions are the chain's), for (Y, X) not last or fields of different shapes, for chunked
        host arrays, and on grids with face connections or a fold along either axis."""
        args = (u, v, tracer)
        (u, xr1), (v, xr2), (t, xr3) = self._wrap_in(u), self._wrap_in(v), self._wrap_in(tracer)
        was_xr = xr1 or xr2 or xr3
        xa, ya = self.axes[x_axis], self.axes[y_axis]
        tx_pos, tx_dim = xa._get_position_name(t)
        ty_pos, ty_dim = ya._get_position_name(t)
        ux_pos, ux_dim = xa._get_position_name(u)
        uy_pos, uy_dim = ya._get_position_name(u)
        vx_pos, vx_dim = xa._get_position_name(v)
        vy_pos, vy_dim = ya._get_position_name(v)
        if ((tx_pos, ty_pos, ux_pos, uy_pos, vx_pos, vy_pos) != ("center", "center", "left", "center", "center", "left")
                or "left" not in xa.coords or "left" not in ya.coords):
            raise NotImplementedError("fused flux divergence needs the tracer at (Y:center, X:center), u at (Y:center, "
                                      "X:left) and v at (Y:left, X:center)")
        out_x, out_y = xa.coords["center"], ya.coords["center"]
        dims_x = t.dims[:-2] + (ty_dim, xa.coords["left"])
        dims_y = t.dims[:-2] + (ya.coords["left"], tx_dim)
        out_dims = t.dims[:-2] + (out_y, out_x)
        plan = None
        area = None
        if t.dims[-2:] == (ty_dim, tx_dim) and u.dims == dims_x and v.dims == dims_y:
            if metric_weighted:
                area = self._resident(self.get_metric(_DimsOnly(out_dims), (x_axis, y_axis)), t.data)
            plan = self._second_order_plan([u, v, t], x_axis, y_axis, padding, fill_value, [area] if area is not None else [])
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            fx, fy = self.flux(*args, x_axis, y_axis, **kw)
            return self.divergence(fx, fy, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
        bcx, bcy, fvx, fvy = plan
        host = not (_is_tensor(u.data) or _is_tensor(v.data) or _is_tensor(t.data))
        out = _dev.flux_divergence(u.data, v.data, t.data, None if area is None else _aligned_view(area, out_dims),
                                   bcx, bcy, fvx, fvy)
        # coords as the chain's: the flux's (from u / v and the tracer), then the divergence's from the two fluxes
        rx = _reattach_coords([DataArray(_placeholder(u.shape), dims_x)], self, None, {xa.coords["left"]}, [u, t])[0]
        ry = _reattach_coords([DataArray(_placeholder(v.shape), dims_y)], self, None, {ya.coords["left"]}, [v, t])[0]
        res = DataArray(_dev.tohost(out) if host else out, out_dims)
        res = _reattach_coords([res], self, None, {out_x, out_y}, [rx, ry])[0]
        return to_xarray(res) if was_xr else res

    def laplacian(self, a, x_axis: str = "X", y_axis: str = "Y", padding=None, fill_value=None,
                  metric_weighted: bool = True):
        """Finite-volume Laplacian `(delta_x(dyG * delta_x(a) / dxC) + delta_y(dxG * delta_y(a) / dyC)) / rA` of a
        cell-centre field in ONE pass (16 B/cell in float64: the field read once, the result written once; the metric
        planes are read through the cache).  Bit-identical to the chain

            gx, gy = grid.gradient(a, x_axis, y_axis, padding=padding, fill_value=fill_value, metric_weighted=metric_weighted)
            if metric_weighted: gx = gx * grid.get_metric(gx, (y_axis,)); gy = gy * grid.get_metric(gy, (x_axis,))
            grid.divergence(gx, gy, x_axis, y_axis, padding=padding, fill_value=fill_value, metric_weighted=metric_weighted)

        which pads twice: the field below / left of the first cell, then the fluxes gx, gy above / right of the last one
        (periodic: at index 0, extend: at n-1, fill: `fill_value` itself).  That chain itself runs for integer, float16
        or mixed dtypes (the field's and the metrics'), for (Y, X) not last, metrics with dims the field lacks, chunked
        host arrays, and on grids with face connections or a fold along either axis."""
        arg = a
        a, was_xr = self._wrap_in(a)
        xa, ya = self.axes[x_axis], self.axes[y_axis]
        x_pos, x_dim = xa._get_position_name(a)
        y_pos, y_dim = ya._get_position_name(a)
        if (x_pos, y_pos) != ("center", "center") or "left" not in xa.coords or "left" not in ya.coords:
            raise NotImplementedError("fused laplacian needs a field at (Y:center, X:center) and left points on both axes")
        out_dims = a.dims
        dims_x = a.dims[:-1] + (xa.coords["left"],)
        dims_y = a.dims[:-2] + (ya.coords["left"], x_dim)
        plan = None
        mets = {}
        if a.dims[-2:] == (y_dim, x_dim):
            if metric_weighted:
                like = _DimsOnly(dims_x, a.name), _DimsOnly(dims_y, a.name)
                for key, where, axes in (("dxC", 0, (x_axis,)), ("dyC", 1, (y_axis,)), ("dyG", 0, (y_axis,)),
                                         ("dxG", 1, (x_axis,)), ("area", None, (x_axis, y_axis))):
                    m = self.get_metric(_DimsOnly(out_dims) if where is None else like[where], axes)
                    mets[key] = (self._resident(m, a.data), out_dims if where is None else like[where].dims)
            if all(set(m.dims) <= set(dims) for m, dims in mets.values()):
                plan = self._second_order_plan([a], x_axis, y_axis, padding, fill_value, [m for m, _ in mets.values()])
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            gx, gy = self.gradient(arg, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
            if metric_weighted:
                gx = gx * self.get_metric(gx, (y_axis,))
                gy = gy * self.get_metric(gy, (x_axis,))
            return self.divergence(gx, gy, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
        bcx, bcy, fvx, fvy = plan
        host = not _is_tensor(a.data)
        views = {k: _aligned_view(m, dims) for k, (m, dims) in mets.items()}
        out = _dev.laplacian(a.data, bcx, bcy, fvx, fvy, **views)
        # coords as the chain's: the gradient's (from the field), times the face lengths, then the divergence's
        gx = _reattach_coords([DataArray(_placeholder(a.shape), dims_x, name=a.name)], self, None, {xa.coords["left"]}, [a])[0]
        gy = _reattach_coords([DataArray(_placeholder(a.shape), dims_y, name=a.name)], self, None, {ya.coords["left"]}, [a])[0]
        if metric_weighted:
            gx = gx._replace(coords=_binary_coords(gx, mets["dyG"][0], dims_x))
            gy = gy._replace(coords=_binary_coords(gy, mets["dxG"][0], dims_y))
        res = DataArray(_dev.tohost(out) if host else out, out_dims)
        res = _reattach_coords([res], self, None, {xa.coords["center"], ya.coords["center"]}, [gx, gy])[0]
        return to_xarray(res) if was_xr else res

    def flux_divergence_3d(self, u, v, w, tracer, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", padding=None,
                           fill_value=None, metric_weighted: bool = True):
        """3-D flux-form advection tendency of a tracer in ONE pass -- MITgcm's (di Fx + dj Fy + dk Fr) / (rA drF hFacC):
        u, v, w and the tracer are read once, the result written once (40 B/cell in float64); the fluxes stay in registers.

        u at (Z:center, Y:center, X:left), v at (Z:center, Y:left, X:center), w at (Z:left, Y:center, X:center), the tracer
        and the result at the centre.  Bit-identical to the chain

            kw = dict(padding=padding, fill_value=fill_value)
            fx, fy = grid.flux(u, v, tracer, x_axis, y_axis, **kw)
            fz = w * grid.interp(tracer, z_axis, **kw)
            h = grid.divergence(fx, fy, x_axis, y_axis, metric_weighted=False, **kw)
            out = h + grid.diff(fz, z_axis, **kw)
            if metric_weighted:
                out = out / grid.get_metric(out, (x_axis, y_axis, z_axis))

        which pads twice on every axis: the tracer below / left of / above the first cell (center -> left), then the fluxes
        beyond the last one (left -> center; periodic: the flux at index 0, extend: at n-1, fill: `fill_value` itself).
        This is the divergence in INDEX space: the vertical term is fz[k+1] - fz[k].  For a model whose Z index grows
        downward and whose w is positive upward (MITgcm's WVEL), pass -w (exact: negation commutes with *, + and -).

        The volume is what `get_metric(out, (X, Y, Z))` returns: a registered (Z, Y, X) volume, or the product of an area and
        a thickness, whose two factors the kernel multiplies per cell in the same order.  The chain itself runs (the same
        calls in the same order) for integer, float16 or mixed dtypes, for (Z, Y, X) not last or fields of different
        shapes, for chunked host arrays, for a volume with dims the result lacks, and on grids with face connections or a
        fold."""
        args = (u, v, w, tracer)
        (u, xr1), (v, xr2), (w, xr3), (t, xr4) = (self._wrap_in(a) for a in args)
        was_xr = xr1 or xr2 or xr3 or xr4
        axes = (self.axes[z_axis], self.axes[y_axis], self.axes[x_axis])
        za, ya, xa = axes
        want = {"t": ("center", "center", "center"), "u": ("center", "center", "left"), "v": ("center", "left", "center"),
                "w": ("left", "center", "center")}
        got = {k: tuple(ax._get_position_name(f) for ax in axes) for k, f in (("t", t), ("u", u), ("v", v), ("w", w))}
        if any(tuple(p for p, _ in got[k]) != want[k] for k in want) or any("left" not in ax.coords for ax in axes):
            raise NotImplementedError("fused 3-D flux divergence needs the tracer at the centre, u at (Z:center, Y:center, "
                                      "X:left), v at (Z:center, Y:left, X:center) and w at (Z:left, Y:center, X:center)")
        (_, tz), (_, ty), (_, tx) = got["t"]
        zl, yl, xl = (ax.coords["left"] for ax in axes)
        lead = t.dims[:-3]
        out_dims = lead + (tz, ty, tx)
        plan = None
        factors = ()
        if t.dims == out_dims and u.dims == lead + (tz, ty, xl) and v.dims == lead + (tz, yl, tx) and w.dims == lead + (zl, ty, tx):
            if metric_weighted:
                factors = self.get_metric(_DimsOnly(out_dims), (x_axis, y_axis, z_axis), _factors=True)
                if len(factors) > 2:  # (formed as get_metric forms it; the kernel multiplies two factors at most)
                    factors = (functools.reduce(operator.mul, factors[1:], factors[0]),)
                factors = tuple(self._resident(f, t.data) for f in factors)
            if all(set(f.dims) <= set(out_dims) for f in factors) and not gridops.complex_topology(self, z_axis):
                plan = self._xyz_plan([u, v, w, t], x_axis, y_axis, z_axis, padding, fill_value, list(factors))
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            fx, fy = self.flux(args[0], args[1], args[3], x_axis, y_axis, **kw)
            fz = args[2] * self.interp(args[3], z_axis, **kw)
            h = self.divergence(fx, fy, x_axis, y_axis, metric_weighted=False, **kw)
            out = h + self.diff(fz, z_axis, **kw)
            if metric_weighted:
                out = out / self.get_metric(out, (x_axis, y_axis, z_axis))
            return out
        bcx, bcy, fvx, fvy, bcz, fvz = plan
        host = not any(_is_tensor(f.data) for f in (u, v, w, t))
        views = [_aligned_view(f, out_dims) for f in factors] + [None, None]
        out = _dev.flux_divergence_3d(u.data, v.data, w.data, t.data, views[0], views[1], bcx, bcy, bcz, fvx, fvy, fvz)
        # coords and name as the chain's, step by step over placeholders: the fluxes, their divergence; the tracer along Z,
        # its product with w, that product's difference; the sum; the quotient by the volume
        rx = _reattach_coords([DataArray(_placeholder(u.shape), u.dims)], self, None, {xl}, [u, t])[0]
        ry = _reattach_coords([DataArray(_placeholder(v.shape), v.dims)], self, None, {yl}, [v, t])[0]
        h = _reattach_coords([DataArray(_placeholder(t.shape), out_dims)], self, None, {tx, ty}, [rx, ry])[0]
        tz_l = _reattach_coords([DataArray(_placeholder(t.shape), w.dims, name=t.name)], self, None, {zl}, [t])[0]
        fz = DataArray(_placeholder(w.shape), w.dims, coords=_binary_coords(w, tz_l, w.dims), name=_result_name(w, tz_l))
        dz = _reattach_coords([DataArray(_placeholder(t.shape), out_dims, name=fz.name)], self, None, {tz}, [fz])[0]
        res = DataArray(_placeholder(t.shape), out_dims, coords=_binary_coords(h, dz, out_dims), name=_result_name(h, dz))
        if factors:
            vol = factors[0]
            if len(factors) == 2:
                vdims = vol.dims + tuple(d for d in factors[1].dims if d not in vol.dims)
                vshape = tuple(res.sizes[d] for d in vdims)
                vol = DataArray(_placeholder(vshape), vdims, coords=_binary_coords(vol, factors[1], vdims),
                                name=_result_name(vol, factors[1]))
            res = res._replace(coords=_binary_coords(res, vol, out_dims), name=_result_name(res, vol))
        res = res._replace(data=_dev.tohost(out) if host else out)
        return to_xarray(res) if was_xr else res

    def vertical_velocity(self, u, v, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", padding=None,
                          fill_value=None, reverse: bool = False, face_weighted: bool = False,
                          metric_weighted: bool = True):
        """Vertical velocity (or transport) diagnosed from continuity in ONE pass: the horizontal divergence of the
        transports summed along Z.  u and v are read once and w written once (24 B/cell in float64, against 72 for the
        chain); the running sum of a column stays in registers.

        u at (Z:center, Y:center, X:left), v at (Z:center, Y:left, X:center); the result at (Z:left, Y:center, X:center),
        where `flux_divergence_3d` wants its w.  Bit-identical, coords and name included, to the chain

            kw = dict(padding=padding, fill_value=fill_value)
            if face_weighted:                      # velocities -> transports
                u = u * grid.get_metric(u, (y_axis, z_axis))
                v = v * grid.get_metric(v, (x_axis, z_axis))
            d = grid.divergence(u, v, x_axis, y_axis, metric_weighted=False, **kw)
            w = -grid.cumsum(d, z_axis, to="left", reverse=reverse, **kw)
            if metric_weighted:
                w = w / grid.get_metric(w, (x_axis, y_axis))

        Forward (`reverse=False`): w[0] is the Z pad (`fill`: -fill_value, `extend`: w[1]) and w[k] = -(d[0] + .. + d[k-1]),
        added in that order; the last level of d is not used.  This is `flux_divergence_3d`'s index-space convention:
        d[k] + (w[k+1] - w[k]) vanishes to rounding, so this w is passed to it as it is.  Reverse: w[k] = -(d[nz-1] + .. +
        d[k]), summed from the last level upward with no pad -- the form for a model with w = 0 at the sea floor and a Z
        index that grows downward (MITgcm).  That w is positive upward in the model's sense and satisfies
        d[k] - (w[k+1] - w[k]) = 0 in index space, so pass -w to `flux_divergence_3d` (as for MITgcm's own WVEL).

        The sum is `Grid.cumsum`'s nancumsum: a NaN divergence counts as 0.  With `face_weighted` the kernel multiplies the
        factors `get_metric` returns (a face length and a thickness, or one registered face area) per cell and then the
        velocity by their product.  The chain itself runs (the same calls in the same order) for integer, float16 or mixed
        dtypes, for (Z, Y, X) not last or u, v of different shapes, for chunked host arrays, for periodic Z summed forward
        (the pad is the column total), for a single column (ny * nx == 1), for a metric with dims the field lacks, and on
        grids with face connections or a fold."""
        args = (u, v)
        (u, xr1), (v, xr2) = (self._wrap_in(a) for a in args)
        was_xr = xr1 or xr2
        axes = (self.axes[z_axis], self.axes[y_axis], self.axes[x_axis])
        want = {"u": ("center", "center", "left"), "v": ("center", "left", "center")}
        got = {k: tuple(ax._get_position_name(f) for ax in axes) for k, f in (("u", u), ("v", v))}
        if any(tuple(p for p, _ in got[k]) != want[k] for k in want) or any("left" not in ax.coords for ax in axes):
            raise NotImplementedError("fused vertical velocity needs u at (Z:center, Y:center, X:left) and v at "
                                      "(Z:center, Y:left, X:center); the result is at (Z:left, Y:center, X:center)")
        (_, tz), (_, ty), (_, xl) = got["u"]
        (_, _), (_, yl), (_, tx) = got["v"]
        zl = axes[0].coords["left"]
        lead = u.dims[:-3]
        d_dims, out_dims = lead + (tz, ty, tx), lead + (zl, ty, tx)
        plan = None
        fu = fv = fa = ()
        raw = {}
        if u.dims == lead + (tz, ty, xl) and v.dims == lead + (tz, yl, tx):
            if face_weighted:
                raw["u"] = self.get_metric(_DimsOnly(u.dims, u.name), (y_axis, z_axis), _factors=True)
                raw["v"] = self.get_metric(_DimsOnly(v.dims, v.name), (x_axis, z_axis), _factors=True)
            if metric_weighted:
                raw["a"] = self.get_metric(_DimsOnly(out_dims), (x_axis, y_axis), _factors=True)

            def kernel_factors(fs, dims, n):
                # one general factor, then (n == 2) one that varies along Z and leading dims only; anything else is
                # reduced first, formed as get_metric forms it
                fs = tuple(fs)
                if len(fs) == 2 and n == 2:
                    flat = [not (set(f.dims) & set(dims[-2:])) for f in fs]
                    if flat[1]:
                        return fs
                    if flat[0]:
                        return fs[::-1]  # (a product of two factors commutes bit for bit)
                if len(fs) > 1:
                    fs = (functools.reduce(operator.mul, fs[1:], fs[0]),)
                return fs

            fu = tuple(self._resident(f, u.data) for f in kernel_factors(raw.get("u", ()), u.dims, 2))
            fv = tuple(self._resident(f, u.data) for f in kernel_factors(raw.get("v", ()), v.dims, 2))
            fa = tuple(self._resident(f, u.data) for f in kernel_factors(raw.get("a", ()), out_dims, 1))
            fits = (all(set(f.dims) <= set(u.dims) for f in fu) and all(set(f.dims) <= set(v.dims) for f in fv)
                    and all(set(f.dims) <= set(out_dims) for f in fa))
            # (a single column, ny * nx == 1: Z is the contiguous axis there and Grid.cumsum takes its scan for that layout,
            # which does not add in the march's order -- the chain itself keeps its bits)
            if fits and not gridops.complex_topology(self, z_axis) and u.shape[-2] * u.shape[-1] != 1:
                plan = self._second_order_plan([u, v], x_axis, y_axis, padding, fill_value, list(fu + fv + fa))
            if plan is not None:
                bc = self._complete_user_kwargs_using_axis_defaults(padding, "padding")
                fval = self._complete_user_kwargs_using_axis_defaults(fill_value, "fill_value")
                bcz = bc[z_axis]
                if reverse:
                    bcz = bcz or "fill"  # (no pad: the boundary is not looked at)
                elif bcz not in ("fill", "extend") or (bcz == "extend" and u.shape[-3] == 1):
                    # periodic: the pad is the column total; no boundary, or one level to extend from an empty cumulative
                    # field: the chain raises
                    plan = None
                if plan is not None:
                    plan = plan + (bcz, 0.0 if fval[z_axis] is None else float(fval[z_axis]))  # (as cumsum: -0.0 stays)
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            u, v = args
            if face_weighted:
                u = u * self.get_metric(u, (y_axis, z_axis))
                v = v * self.get_metric(v, (x_axis, z_axis))
            d = self.divergence(u, v, x_axis, y_axis, metric_weighted=False, **kw)
            w = -self.cumsum(d, z_axis, to="left", reverse=reverse, **kw)
            if metric_weighted:
                w = w / self.get_metric(w, (x_axis, y_axis))
            return w
        bcx, bcy, fvx, fvy, bcz, fvz = plan
        host = not any(_is_tensor(f.data) for f in (u, v))
        mu = [_aligned_view(f, u.dims) for f in fu] + [None, None]
        mv = [_aligned_view(f, v.dims) for f in fv] + [None, None]
        area = _aligned_view(fa[0], out_dims) if fa else None
        out = _dev.vertical_velocity(u.data, v.data, mu[0], mu[1], mv[0], mv[1], area, bcx, bcy, bcz, fvx, fvy, fvz,
                                     bool(reverse))

        # coords and name as the chain's, step by step over placeholders: the products with the face weights, the
        # divergence, the cumulative sum, the negation (a scalar: nothing changes), the quotient by the area
        def product_of(fs, like):
            acc = fs[0]
            for f in fs[1:]:
                dims = acc.dims + tuple(d for d in f.dims if d not in acc.dims)
                acc = DataArray(_placeholder(tuple(like.sizes[d] for d in dims)), dims,
                                coords=_binary_coords(acc, f, dims), name=_result_name(acc, f))
            return acc

        def times(f, fs):
            m = product_of(fs, f)
            return DataArray(_placeholder(f.shape), f.dims, coords=_binary_coords(f, m, f.dims), name=_result_name(f, m))

        pu, pv = (times(u, raw["u"]), times(v, raw["v"])) if face_weighted else (u, v)
        d = _reattach_coords([DataArray(_placeholder(u.shape), d_dims)], self, None, {tx, ty}, [pu, pv])[0]
        pads = (0, 0) if reverse else (1, 0)
        res = _reattach_coords([DataArray(_placeholder(u.shape), out_dims, name=d.name)], self, {z_axis: pads}, {zl}, [d])[0]
        if metric_weighted:
            m = product_of(raw["a"], res)
            res = res._replace(coords=_binary_coords(res, m, out_dims), name=_result_name(res, m))
        res = res._replace(data=_dev.tohost(out) if host else out)
        return to_xarray(res) if was_xr else res

    def hydrostatic_pressure_gradient(self, b, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", padding=None,
                                      fill_value=None, metric_weighted: bool = True):
        """Horizontal gradient of the hydrostatic pressure (the pressure-gradient force of the hydrostatic momentum
        equations, and what geostrophic and thermal-wind velocities are formed from) in ONE pass: the buoyancy `b` (or
        g * rho / rho0) is read once and the two components written once (24 B/cell in float64, against about 56 for the
        chain); the running sum of a column stays in registers.  Returns `(gx, gy)`.

        b at (Z:center, Y:center, X:center); gx at (Z:center, Y:center, X:left), gy at (Z:center, Y:left, X:center), where
        `momentum_advection` puts its tendencies.  The Z axis needs an `outer` position (MITgcm's Zp1).  Bit-identical,
        dims, coords and names included, to the chain

            kw = dict(padding=padding, fill_value=fill_value)
            p = grid.cumint(b, z_axis, to="outer", **kw)      # (Z:outer, Y, X): p[0] = Z pad, p[k] = sum_{m<k} b[m] * w[m]
            pc = grid.interp(p, z_axis, **kw)                 # outer -> center, no pad: (p[k] + p[k+1]) / 2
            gx, gy = grid.gradient(pc, x_axis, y_axis, metric_weighted=metric_weighted, **kw)

        The sum runs forward from index 0 -- the form for a model whose Z index grows downward from the surface -- and
        p[0] is the Z pad: `fill_value` under `fill`, p[1] under `extend`.  It is `Grid.cumsum`'s nancumsum taken in
        sequence: a NaN product b * w counts as 0, and the first sum is the product itself.  The vertical weight (what
        `get_metric(b, (z_axis,))` returns: drF(Z), or a registered (Z, Y, X) thickness) is always applied;
        `metric_weighted` goes to the gradient only.  The gradient pads pc below and left of the first cell -- periodic:
        pc at the wrapped index, extend: at the clamped index, fill: `fill_value` itself.

        The chain itself runs (the same calls in the same order) for integer, float16 or mixed dtypes, for (Z, Y, X) not
        last, for chunked host arrays, for periodic Z (the pad is the column total) or a missing boundary (the chain
        raises), for a single column (ny * nx == 1), for a metric with dims the field lacks, and on grids with face
        connections or a fold along any of the three axes."""
        arg = b
        b, was_xr = self._wrap_in(b)
        axes = (self.axes[z_axis], self.axes[y_axis], self.axes[x_axis])
        got = tuple(ax._get_position_name(b) for ax in axes)
        if (tuple(p for p, _ in got) != ("center", "center", "center") or "outer" not in axes[0].coords
                or "left" not in axes[1].coords or "left" not in axes[2].coords):
            raise NotImplementedError("fused hydrostatic pressure gradient needs b at (Z:center, Y:center, X:center), left "
                                      "points on X and Y and an outer position on Z")
        (_, tz), (_, ty), (_, tx) = got
        zo, yl, xl = axes[0].coords["outer"], axes[1].coords["left"], axes[2].coords["left"]
        lead = b.dims[:-3]
        p_dims, dims_x, dims_y = lead + (zo, ty, tx), lead + (tz, ty, xl), lead + (tz, yl, tx)
        plan = None
        weight = mx = my = None
        if b.dims == lead + (tz, ty, tx) and not gridops.complex_topology(self, z_axis) and b.shape[-2] * b.shape[-1] != 1:
            try:
                weight = self._resident(self.get_metric(b, (z_axis,), _layout=b.dims), b.data)
                if metric_weighted:
                    mx = self._resident(self.get_metric(_DimsOnly(dims_x), (x_axis,)), b.data)
                    my = self._resident(self.get_metric(_DimsOnly(dims_y), (y_axis,)), b.data)
            except (KeyError, ValueError):
                weight = None  # (the chain raises it where the chain looks the metric up)
            if weight is not None and all(m is None or (set(m.dims) <= set(dims) and not _is_chunked(m.data))
                                          for m, dims in ((weight, b.dims), (mx, dims_x), (my, dims_y))):
                # periodic Z: the pad is the column total
                plan = self._xyz_plan([b], x_axis, y_axis, z_axis, padding, fill_value,
                                      [m for m in (weight, mx, my) if m is not None], z_modes=("fill", "extend"))
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            p = self.cumint(arg, z_axis, to="outer", **kw)
            pc = self.interp(p, z_axis, **kw)
            return self.gradient(pc, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
        bcx, bcy, fvx, fvy, bcz, fvz = plan
        host = not _is_tensor(b.data)
        ox, oy = _dev.hydrostatic_pressure_gradient(b.data, _aligned_view(weight, b.dims),
                                                    None if mx is None else _aligned_view(mx, dims_x),
                                                    None if my is None else _aligned_view(my, dims_y),
                                                    bcx, bcy, bcz, fvx, fvy, fvz)
        # dims, coords and names as the chain's, step by step over placeholders: the cumulative integral (named after the
        # product with the weight, padded by one level), its mean at the centre, the two differences
        p_shape = tuple(b.shape[:-3]) + (b.shape[-3] + 1,) + tuple(b.shape[-2:])
        p = _reattach_coords([DataArray(_placeholder(p_shape), p_dims, name=_name_after(b.name, weight))], self,
                             {z_axis: (1, 0)}, {zo}, [b])[0]
        pc = _reattach_coords([DataArray(_placeholder(b.shape), b.dims, name=p.name)], self, None, {tz}, [p])[0]
        gx, gy = self._labels_of_step(pc, dims_x, xl), self._labels_of_step(pc, dims_y, yl)
        gx = gx._replace(data=_dev.tohost(ox) if host else ox)
        gy = gy._replace(data=_dev.tohost(oy) if host else oy)
        return (to_xarray(gx), to_xarray(gy)) if was_xr else (gx, gy)

    def vertical_momentum_advection(self, u, v, w, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", padding=None,
                                    fill_value=None, metric_weighted: bool = True):
        """Vertical advection of horizontal momentum, -w du/dz and -w dv/dz (MITgcm's mom_vi_u_vertshear and
        mom_vi_v_vertshear), in ONE pass: u, v and w are read once and the two tendencies written once (40 B/cell in
        float64, against about 200 for the twelve launches of the chain).  Returns `(gu, gv)`, gu at u's points, gv at v's.
        With `momentum_advection` and `hydrostatic_pressure_gradient` it completes the inviscid tendency in three launches.

        u at (Z:center, Y:center, X:left), v at (Z:center, Y:left, X:center), w at (Z:left, Y:center, X:center) -- what
        `vertical_velocity` returns and `flux_divergence_3d` takes.  Bit-identical, dims, coords and names included, to
        the chain

            kw = dict(padding=padding, fill_value=fill_value)
            wu = grid.interp(w, x_axis, **kw)          # center -> left: w over u's column, (Z:left, Y:center, X:left)
            wv = grid.interp(w, y_axis, **kw)          # (Z:left, Y:left, X:center)
            du = grid.diff(u, z_axis, **kw)            # center -> left: u[k] - u[k-1]
            dv = grid.diff(v, z_axis, **kw)
            gu = -grid.interp(wu * du, z_axis, **kw)   # left -> center: (p[k] + p[k+1]) / 2
            gv = -grid.interp(wv * dv, z_axis, **kw)
            if metric_weighted:
                gu = gu / grid.get_metric(gu, (z_axis,))
                gv = gv / grid.get_metric(gv, (z_axis,))

        Pads: every stage pads where the chain pads it -- w left of the first column and below the first row, u and v
        above level 0, the PRODUCTS beyond level nz-1.  Periodic: the stage's own value at the wrapped index; extend: at
        the clamped index; fill: `fill_value` itself, not a product formed from it.

        Periodic Z: all three Z boundaries (`periodic`, `fill`, `extend`) go through the kernel -- there is no running sum
        here, a periodic Z costs one more row read before the march.  Only a Z axis with no boundary falls back, because
        there the chain raises.

        Sign convention: the index-space form, as in `flux_divergence_3d`.  For a model whose Z index grows downward and
        whose w is positive upward (MITgcm's WVEL), pass -w (exact: negation commutes with the means and the products).

        Metric: whatever `get_metric` returns at each output's dims -- drF(Z), or a thickness registered at u's / v's
        points -- one broadcast array per output; the negation comes before the division, as in the chain.

        The chain itself runs (the same calls in the same order) for integer, float16 or mixed dtypes, for (Z, Y, X) not
        last or fields of different shapes, for chunked inputs, for a metric with dims the output lacks or a chunked
        metric, for a metric lookup that raises (the chain raises it), for a Z axis without a boundary, on grids with face
        connections or a fold along any of the three axes, and for anything else `_second_order_plan` declines."""
        args = (u, v, w)
        (u, xr1), (v, xr2), (w, xr3) = (self._wrap_in(a) for a in args)
        was_xr = xr1 or xr2 or xr3
        axes = (self.axes[z_axis], self.axes[y_axis], self.axes[x_axis])
        want = {"u": ("center", "center", "left"), "v": ("center", "left", "center"), "w": ("left", "center", "center")}
        got = {k: tuple(ax._get_position_name(f) for ax in axes) for k, f in (("u", u), ("v", v), ("w", w))}
        if any(tuple(p for p, _ in got[k]) != want[k] for k in want) or any("left" not in ax.coords for ax in axes):
            raise NotImplementedError("fused vertical momentum advection needs u at (Z:center, Y:center, X:left), v at "
                                      "(Z:center, Y:left, X:center) and w at (Z:left, Y:center, X:center)")
        (_, tz), (_, ty), (_, xl) = got["u"]
        (_, _), (_, yl), (_, tx) = got["v"]
        zl = axes[0].coords["left"]
        lead = u.dims[:-3]
        u_dims, v_dims, w_dims = lead + (tz, ty, xl), lead + (tz, yl, tx), lead + (zl, ty, tx)
        wu_dims, wv_dims = lead + (zl, ty, xl), lead + (zl, yl, tx)
        plan = None
        mu = mv = None
        if u.dims == u_dims and v.dims == v_dims and w.dims == w_dims and not gridops.complex_topology(self, z_axis):
            try:
                if metric_weighted:
                    mu = self._resident(self.get_metric(_DimsOnly(u_dims), (z_axis,)), u.data)
                    mv = self._resident(self.get_metric(_DimsOnly(v_dims), (z_axis,)), u.data)
                fits = all(m is None or (set(m.dims) <= set(dims) and not _is_chunked(m.data))
                           for m, dims in ((mu, u_dims), (mv, v_dims)))
            except (KeyError, ValueError):
                fits = False  # (the chain raises it where the chain looks the metric up)
            if fits:
                plan = self._xyz_plan([u, v, w], x_axis, y_axis, z_axis, padding, fill_value, [m for m in (mu, mv) if m is not None])
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            u, v, w = args
            wu = self.interp(w, x_axis, **kw)
            wv = self.interp(w, y_axis, **kw)
            du = self.diff(u, z_axis, **kw)
            dv = self.diff(v, z_axis, **kw)
            gu = -self.interp(wu * du, z_axis, **kw)
            gv = -self.interp(wv * dv, z_axis, **kw)
            if metric_weighted:
                gu = gu / self.get_metric(gu, (z_axis,))
                gv = gv / self.get_metric(gv, (z_axis,))
            return gu, gv
        bcx, bcy, fvx, fvy, bcz, fvz = plan
        host = not any(_is_tensor(f.data) for f in (u, v, w))
        ou, ov = _dev.vertical_momentum_advection(u.data, v.data, w.data,
                                                  None if mu is None else _aligned_view(mu, u_dims),
                                                  None if mv is None else _aligned_view(mv, v_dims),
                                                  bcx, bcy, bcz, fvx, fvy, fvz)
        # dims, coords and names as the chain's, step by step over placeholders: w over u's / v's column, the differences
        # along Z, the products, their means at the centre (the negation changes neither coords nor name), the quotients
        wu, wv = self._labels_of_step(w, wu_dims, xl), self._labels_of_step(w, wv_dims, yl)
        du, dv = self._labels_of_step(u, wu_dims, zl), self._labels_of_step(v, wv_dims, zl)
        gu = self._labels_of_step(self._labels_of_binary(wu, du), u_dims, tz)
        gv = self._labels_of_step(self._labels_of_binary(wv, dv), v_dims, tz)
        if mu is not None:
            gu = gu._replace(coords=_binary_coords(gu, mu, u_dims), name=_result_name(gu, mu))
        if mv is not None:
            gv = gv._replace(coords=_binary_coords(gv, mv, v_dims), name=_result_name(gv, mv))
        gu = gu._replace(data=_dev.tohost(ou) if host else ou)
        gv = gv._replace(data=_dev.tohost(ov) if host else ov)
        return (to_xarray(gu), to_xarray(gv)) if was_xr else (gu, gv)

    def vertical_diffusion(self, a, kappa=None, z_axis: str = "Z", to=None, padding=None, fill_value=None,
                           metric_weighted: bool = True):
        """Vertical mixing d/dz(kappa da/dz) -- the vertical diffusion of a tracer, the vertical viscosity of u or v -- in
        ONE pass: `a` and `kappa` are read once and the result written once (24 B/cell in float64, 16 with a profile
        kappa(Z) or none, against 56 for the three launches of the chain); the flux stays in registers.

        `a` at Z:center with its Z dim third from last; the two dims after it are only rows and columns, so `a` may sit
        at the centre, at u's or at v's points.  `kappa` at the flux position on Z, with dims among those of the flux (a
        profile kappa(Z), a (Z, Y, X) field, a field with leading dims): it is read through broadcast strides, never
        materialised.  `to`: the flux position, "left" or "outer" (None: "outer" when the Z axis has one, else "left").
        Bit-identical, dims, coords and name included, to the chain

            kw = dict(padding=padding, fill_value=fill_value)
            g = grid.derivative(a, z_axis, to=to, **kw)    # center -> left | outer: (a[k] - a[k-1]) / drC
            f = g * kappa                                  # the diffusive flux (kappa=None: f = g)
            out = grid.derivative(f, z_axis, **kw)         # left | outer -> center: (f[k+1] - f[k]) / drF

        (`metric_weighted=False`: `diff` in both places).  Pads where the chain pads.  "left": `a` above level 0
        (periodic: a[nz-1], extend: a[0], fill: `fill_value`), then the FLUX beyond level nz-1 (periodic: f[0], extend:
        f[nz-1], fill: `fill_value` itself, not a flux formed from it).  "outer": `a` on both sides; the flux has nz+1
        levels and needs no pad -- with `extend` it is exactly zero at the top and at the bottom, the no-flux condition.

        The metrics are whatever `get_metric` returns at the flux' and at `a`'s dims (drC / drF, or registered 3-D
        thicknesses), one broadcast array each.

        The chain itself runs (the same calls in the same order) for integer, float16 or mixed dtypes (a `kappa` of another
        dtype included), for fewer than three dims or Z not third from last, for another `to` or a position the axis
        lacks, for a `kappa` that is not at the flux position, has dims `a` lacks or is chunked, for chunked `a`, for a
        metric that is chunked or has dims its stage lacks, for a metric lookup that raises (the chain raises it), for a Z
        axis without a boundary, and with face connections or a fold along Z."""
        args = (a, kappa)
        (a, xr1), (kappa, xr2) = self._wrap_in(a), self._wrap_in(kappa)
        was_xr = xr1 or xr2
        zax = self.axes[z_axis]
        if to is None:
            to = "outer" if "outer" in zax.coords else "left"
        plan = None
        mf = mc = None
        served = (isinstance(a, DataArray) and a.ndim >= 3 and to in ("left", "outer") and to in zax.coords
                  and "center" in zax.coords and a.dims[-3] == zax.coords["center"]
                  and sum(d in a.dims for d in zax.coords.values()) == 1
                  and (kappa is None or isinstance(kappa, DataArray)) and not gridops.complex_topology(self, z_axis))
        if served:
            tz, zf = zax.coords["center"], zax.coords[to]
            f_dims = a.dims[:-3] + (zf,) + a.dims[-2:]
            f_shape = tuple(a.shape[:-3]) + (a.shape[-3] + (1 if to == "outer" else 0),) + tuple(a.shape[-2:])
            dtype = _dt.np_dtype(a.data)
            served = dtype in (_dt.FLOAT32, _dt.FLOAT64) and not _is_chunked(a.data)
            if served and kappa is not None:
                served = (set(kappa.dims) <= set(f_dims) and not _is_chunked(kappa.data) and _dt.np_dtype(kappa.data) == dtype
                          and all(kappa.sizes[d] == f_shape[f_dims.index(d)] for d in kappa.dims))
        if served:
            try:
                if metric_weighted:
                    mf = self._resident(self.get_metric(_DimsOnly(f_dims, a.name), (z_axis,), _layout=f_dims), a.data)
                    mc = self._resident(self.get_metric(_DimsOnly(a.dims, a.name), (z_axis,), _layout=a.dims), a.data)
                served = all(m is None or (set(m.dims) <= set(dims) and not _is_chunked(m.data) and _dt.np_dtype(m.data) == dtype)
                             for m, dims in ((mf, f_dims), (mc, a.dims)))
            except (KeyError, ValueError):
                served = False  # (the chain raises it where the chain looks the metric up)
        if served:
            bc = self._complete_user_kwargs_using_axis_defaults(padding, "padding")[z_axis]
            fval = self._complete_user_kwargs_using_axis_defaults(fill_value, "fill_value")[z_axis]
            # (no boundary along Z: the chain raises)  The one-axis operators of the chain hand their fill value on as it is
            # (None: 0.0), so a -0.0 or a NaN keeps its bits
            plan = None if bc is None else (bc, 0.0 if fval is None else float(fval))
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            a, kappa = args
            step = self.derivative if metric_weighted else self.diff
            g = step(a, z_axis, to=to, **kw)
            f = g if kappa is None else g * kappa
            return step(f, z_axis, **kw)
        bcz, fvz = plan
        host = not (_is_tensor(a.data) or (kappa is not None and _is_tensor(kappa.data)))
        out = _dev.vertical_diffusion(a.data, None if kappa is None else _aligned_view(kappa, f_dims),
                                      None if mf is None else _aligned_view(mf, f_dims),
                                      None if mc is None else _aligned_view(mc, a.dims), to == "outer", bcz, fvz)
        # dims, coords and name as the chain's, step by step over placeholders: the gradient at the flux levels (named
        # after its quotient with the metric), the product with kappa, the difference back at the centre, its quotient
        g = _reattach_coords([DataArray(_placeholder(f_shape), f_dims, name=a.name)], self, None, {zf}, [a])[0]
        if mf is not None:
            g = g._replace(name=_name_after(g.name, mf))
        f = g if kappa is None else DataArray(_placeholder(f_shape), f_dims, coords=_binary_coords(g, kappa, f_dims),
                                              name=_result_name(g, kappa))
        res = _reattach_coords([DataArray(_placeholder(a.shape), a.dims, name=f.name)], self, None, {tz}, [f])[0]
        if mc is not None:
            res = res._replace(name=_name_after(res.name, mc))
        res = res._replace(data=_dev.tohost(out) if host else out)
        return to_xarray(res) if was_xr else res

    def implicit_vertical_diffusion(self, a, kappa=None, dt=None, z_axis: str = "Z", to=None, metric_weighted: bool = True):
        """Implicit (backward-Euler) vertical mixing: solves (I - dt D) x = a column by column, where D a is
        d/dz(kappa da/dz) with no flux through the top and the bottom -- a tridiagonal (Thomas) solve along Z in ONE pass,
        a forward and a backward sweep in one launch.  With `kappa` at Z:outer it is the inverse of

            a -> a - dt * grid.vertical_diffusion(a, kappa, to="outer", padding="extend")

        up to rounding; with `kappa` at Z:left (one face fewer: there is none below the last level) it is the same solve,
        only the extent of `kappa` and of the flux' metric differs.  The top and the bottom are insulated, so there is no
        `padding` and no `fill_value`: the face values of `kappa` and of the metric there are never read, and a surface
        flux is added to `a` by the caller.

        `a` at Z:center.  `kappa` at the flux position on Z (`to`: "left" or "outer"; None: "outer" when the Z axis has
        one, else "left"), with dims among those of the flux -- a profile kappa(Z), a (Z, Y, X) field, a field with leading
        dims, in any order: it is read through broadcast strides, never materialised; None: 1.  The metrics are whatever
        `get_metric` returns at the flux' and at `a`'s dims (drC / drF, or registered 3-D thicknesses);
        `metric_weighted=False` drops both divisions.  Per column, levels k = 0 .. n-1, faces k = 1 .. n-1, every operation
        in `a`'s dtype, `dt` cast to it once, no fused multiply-add:

            w[k] = dt * (kappa[k] / mf[k]);  lo[k] = w[k] / mc[k];  up[k-1] = w[k] / mc[k-1]
            b = 1 (+ lo[k], k > 0) (+ up[k], k < n-1)
            m = b - lo[k] * c[k-1];  r = 1 / m;  c[k] = up[k] * r;  d[k] = (a[k] + lo[k] * d[k-1]) * r
            x[n-1] = d[n-1];  x[k] = d[k] + c[k] * x[k+1]

        No pivoting: for kappa >= 0, dt >= 0 and positive metrics the matrix is an M-matrix and max|x| <= max|a| per
        column.  The result carries `a`'s dims, coords and name; xarray in gives xarray out, host in host out, HBM in HBM
        out.

        The kernel serves `a` with Z third from last (the two dims after it are only rows and columns: the centre, u's
        or v's points).  A level loop over whole planes with the array's own arithmetic, the same recurrence in the same
        order and so bit-identical where both apply, serves the rest: fewer than three dims, Z elsewhere, a `kappa` or a
        metric with a dim `a` lacks (the result then has that dim in front).

        Raises ValueError for `dt` negative, NaN or infinite, for an `a` not at Z:center, a `to` that is not "left" or
        "outer" or that the axis lacks, a `kappa` that is not at the flux position or does not fit; TypeError for integer,
        bool or float16 fields and for mixed dtypes (a solve has no exact integer form; nothing is promoted silently);
        NotImplementedError for chunked inputs and for face connections or a fold along Z; the metric lookup's own error
        when `metric_weighted` and the axis has no metric."""
        what = "implicit_vertical_diffusion"
        (a, xr1), (kappa, xr2) = self._wrap_in(a), self._wrap_in(kappa)
        was_xr = xr1 or xr2
        if dt is None:
            raise TypeError(f"{what}: dt, the time step, is required")
        dt = float(dt)
        if not (dt >= 0.0 and np.isfinite(dt)):
            raise ValueError(f"{what}: dt must be finite and not negative, got {dt}")
        if not isinstance(a, DataArray) or not (kappa is None or isinstance(kappa, DataArray)):
            raise TypeError(f"{what}: `a` and `kappa` must be labelled arrays (`kappa` may be None)")
        zax = self.axes[z_axis]
        if to is None:
            to = "outer" if "outer" in zax.coords else "left"
        if to not in ("left", "outer") or to not in zax.coords or "center" not in zax.coords:
            raise ValueError(f"{what}: the flux position must be 'left' or 'outer' and exist on axis {z_axis!r}, got {to!r}")
        if gridops.complex_topology(self, z_axis):
            raise NotImplementedError(f"{what}: face connections or a fold along {z_axis!r} make the columns a coupled system")
        tz, zf = zax.coords["center"], zax.coords[to]
        if tz not in a.dims or sum(d in a.dims for d in zax.coords.values()) != 1:
            raise ValueError(f"{what}: `a` must sit at {z_axis}:center (dim {tz!r}), its dims are {a.dims}")
        if _is_chunked(a.data) or (kappa is not None and _is_chunked(kappa.data)):
            raise NotImplementedError(f"{what}: chunked inputs are not served; compute the array first")
        dtype = _dt.np_dtype(a.data)
        if dtype not in (_dt.FLOAT32, _dt.FLOAT64):
            raise TypeError(f"{what}: a {dtype} field has no exact solve; convert it to float32 or float64 first")
        z = a.dims.index(tz)
        nf = a.shape[z] + (1 if to == "outer" else 0)
        f_dims = tuple(zf if d == tz else d for d in a.dims)
        if kappa is not None:
            if _dt.np_dtype(kappa.data) != dtype:
                raise TypeError(f"{what}: mixed dtypes, `a` is {dtype} and `kappa` {_dt.np_dtype(kappa.data)}; nothing is promoted")
            if any(d in kappa.dims for d in zax.coords.values() if d != zf):
                raise ValueError(f"{what}: `kappa` must sit at the flux position {z_axis}:{to} (dim {zf!r}), its dims are {kappa.dims}")
            for d in kappa.dims:
                n = nf if d == zf else (a.sizes[d] if d in a.dims else None)
                if n is not None and kappa.sizes[d] != n:
                    raise ValueError(f"{what}: `kappa` has {kappa.sizes[d]} entries along {d!r}, the flux has {n}")
        mf = mc = None
        if metric_weighted:
            mf = self._resident(self.get_metric(_DimsOnly(f_dims, a.name), (z_axis,), _layout=f_dims), a.data)
            mc = self._resident(self.get_metric(_DimsOnly(a.dims, a.name), (z_axis,), _layout=a.dims), a.data)
            for m in (mf, mc):
                if _is_chunked(m.data):
                    raise NotImplementedError(f"{what}: chunked metrics are not served; compute them first")
                if _dt.np_dtype(m.data) != dtype:
                    raise TypeError(f"{what}: mixed dtypes, `a` is {dtype} and the metric {m.name!r} {_dt.np_dtype(m.data)}; "
                                    "nothing is promoted")
        host = not (_is_tensor(a.data) or (kappa is not None and _is_tensor(kappa.data)))
        planes = ((kappa, f_dims), (mf, f_dims), (mc, a.dims))
        extra = tuple(dict.fromkeys(d for m, dims in planes if m is not None for d in m.dims if d not in dims))
        if a.ndim >= 3 and z == a.ndim - 3 and not extra:
            out = _dev.implicit_vertical_diffusion(a.data, *(None if m is None else _aligned_view(m, dims) for m, dims in planes),
                                                   to == "outer", dt)
            res = a._replace(data=_dev.tohost(out) if host else out)
        else:
            # the level loop: every operand with the dims (extra.., a's..), Z named alike in all of them
            dims = extra + a.dims
            arrays = [None if m is None else _aligned_view(m, extra + d) for m, d in ((a, a.dims),) + planes]
            if not host:
                arrays = [None if m is None else _dev.asdevice(m) for m in arrays]
            out = _implicit_vertical_diffusion_levels(*arrays, len(extra) + z, dt)
            res = DataArray(out, dims, coords={k: v for k, v in a.coords.items()}, name=a.name, attrs=a.attrs)
        return to_xarray(res) if was_xr else res

    def implicit_vertical_viscosity(self, u, v, nu, dt=None, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", to=None,
                                    padding=None, fill_value=None, metric_weighted: bool = True):
        """Implicit (backward-Euler) vertical viscosity of a C-grid velocity with ONE viscosity `nu` at the centre points of
        the faces of Z -- where `richardson_number` puts Ri and a closure its nu -- in ONE pass: the two averages of nu to
        u's and to v's column are formed inside the coefficient stage of the two solves (MITgcm's implicit momentum mixing).
        Returns `(xu, xv)`.  Bit-identical, dims, coords, name and attrs included, to the chain

            kw   = dict(padding=padding, fill_value=fill_value)
            nu_u = grid.interp(nu, x_axis, **kw)          # (Zf, YC, XC) -> (Zf, YC, XG): (nu[i-1] + nu[i]) * 0.5
            nu_v = grid.interp(nu, y_axis, **kw)          # (Zf, YC, XC) -> (Zf, YG, XC): (nu[j-1] + nu[j]) * 0.5
            xu   = grid.implicit_vertical_diffusion(u, nu_u, dt, z_axis=z_axis, to=to, metric_weighted=metric_weighted)
            xv   = grid.implicit_vertical_diffusion(v, nu_v, dt, z_axis=z_axis, to=to, metric_weighted=metric_weighted)

        which is four launches and two face-sized temporaries.  See `implicit_vertical_diffusion` for the solve: the
        recurrence, its order, the insulated top and bottom (no pad along Z; faces 0 and n of `nu` are never read).

        u at (lead, Z:center, Y:center, X:left), v at (lead, Z:center, Y:left, X:center), the same shape and the same
        float32 or float64 dtype, Z third from last.  `nu` in that dtype at (Zf, Y:center, X:center), Zf the flux position
        `to` ("left" or "outer"; None: "outer" when the Z axis has one, else "left"), with any subset of the leading dims
        in any order: it is read through broadcast strides, never materialised.  `padding` and `fill_value` pad `nu` only,
        left of column 0 and below row 0 (periodic: column nx-1 / row ny-1, extend: column 0 / row 0, fill: the fill value
        cast to the dtype, a -0.0 or a NaN keeping its bits); X and Y may differ.  The metrics are whatever `get_metric`
        returns along Z at u's flux dims, u's dims, v's flux dims and v's dims, one broadcast array each;
        `metric_weighted=False` drops all four.  `xu` carries u's dims, coords, name and attrs, `xv` v's; xarray in gives
        xarray out, host in host out, a tensor among u, v, nu HBM out.

        The chain itself runs (the same calls in the same order, raising what it raises) for `nu` None, for another dtype or
        mixed dtypes, for u or v elsewhere or of different shapes, for a `nu` not at (Zf, Y:center, X:center), lacking one
        of the three dims or with a dim the fields lack, for Z not third from last, for chunked inputs or chunked metrics,
        for a metric with dims its stage lacks, for a metric lookup that raises, for a missing X or Y boundary, and with
        face connections or a fold along any of the three axes.

        Raises, before any work, TypeError for a missing `dt` and ValueError for a `dt` negative, NaN or infinite, as
        `implicit_vertical_diffusion` does."""
        what = "implicit_vertical_viscosity"
        args, to_arg = (u, v, nu), to
        (u, xr1), (v, xr2), (nu, xr3) = (self._wrap_in(a) for a in args)
        if dt is None:
            raise TypeError(f"{what}: dt, the time step, is required")
        dt = float(dt)
        if not (dt >= 0.0 and np.isfinite(dt)):
            raise ValueError(f"{what}: dt must be finite and not negative, got {dt}")
        to, pts = self._column_points(x_axis, y_axis, z_axis, to)
        plan = mets = None
        served = all(isinstance(f, DataArray) for f in (u, v, nu)) and u.ndim >= 3 and pts is not None and not _is_chunked(nu.data)
        if served:
            tz, zf, yc, yl, xc, xl, held = pts
            lead = u.dims[:-3]
            nu_dims = lead + (zf, yc, xc)   # the dims nu is read at: those of `lead` it lacks are broadcast
            f_shape = tuple(u.shape[:-3]) + (u.shape[-3] + (1 if to == "outer" else 0),) + tuple(u.shape[-2:])
            served = (u.dims == lead + (tz, yc, xl) and v.dims == lead + (tz, yl, xc) and not held & set(lead)
                      and {zf, yc, xc} <= set(nu.dims) <= set(nu_dims) and len(set(nu.dims)) == nu.ndim
                      and all(nu.sizes[d] == n for d, n in zip(nu_dims, f_shape) if d in nu.dims))
        if served:
            # the stages of the two solves: u's flux, u's result, v's flux, v's result
            m_dims = [lead + (zf, yc, xl), u.dims, lead + (zf, yl, xc), v.dims]
            mets = self._stage_metrics([(dims, (z_axis,), f.name) for dims, f in zip(m_dims, (u, u, v, v))], u.data, metric_weighted)
        if mets is not None:
            plan = self._second_order_plan([u, v], x_axis, y_axis, padding, fill_value, [nu] + [m for m in mets if m is not None])
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            u, v, nu = args
            nu_u = self.interp(nu, x_axis, **kw)
            nu_v = self.interp(nu, y_axis, **kw)
            xu = self.implicit_vertical_diffusion(u, nu_u, dt, z_axis=z_axis, to=to_arg, metric_weighted=metric_weighted)
            xv = self.implicit_vertical_diffusion(v, nu_v, dt, z_axis=z_axis, to=to_arg, metric_weighted=metric_weighted)
            return xu, xv
        bcx, bcy, fvx, fvy = plan  # (the fills as the chain's one-axis operators hand them on: a -0.0 or a NaN keeps its bits)
        host = not any(_is_tensor(f.data) for f in (u, v, nu))
        ou, ov = _dev.implicit_vertical_viscosity(u.data, v.data, _aligned_view(nu, nu_dims),
                                                  *(None if m is None else _aligned_view(m, dims) for m, dims in zip(mets, m_dims)),
                                                  to == "outer", bcx, bcy, dt, fvx, fvy)
        xu = u._replace(data=_dev.tohost(ou) if host else ou)
        xv = v._replace(data=_dev.tohost(ov) if host else ov)
        # (the chain's nu_u / nu_v are xarray objects when nu is one, and so is each result whose field or nu is one)
        return (to_xarray(xu) if xr1 or xr3 else xu), (to_xarray(xv) if xr2 or xr3 else xv)

    def vertical_shear_squared(self, u, v, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", to=None, padding=None,
                               fill_value=None, metric_weighted: bool = True):
        """Squared vertical shear of a C-grid velocity, S2 = (du/dz)^2 + (dv/dz)^2, at the cell centre on the flux faces of
        Z in ONE pass: u and v are read once and the result written once (24 B/cell in float64).  `richardson_number`
        without its numerator: see there for positions, pads, metrics and the cases the chain itself serves.  Bit-identical,
        dims, coords and name included, to the chain

            kw = dict(padding=padding, fill_value=fill_value)
            step = grid.derivative if metric_weighted else grid.diff
            uz = grid.interp(step(u, z_axis, to=to, **kw), x_axis, **kw)
            vz = grid.interp(step(v, z_axis, to=to, **kw), y_axis, **kw)
            s2 = uz * uz + vz * vz"""
        return self._richardson(None, u, v, x_axis, y_axis, z_axis, to, padding, fill_value, metric_weighted)

    def richardson_number(self, b, u, v, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", to=None, padding=None,
                          fill_value=None, metric_weighted: bool = True):
        """Gradient Richardson number Ri = N2 / S2 -- what every Richardson-number mixing closure (Pacanowski-Philander, the
        interior part of KPP) computes `kappa` from, at the faces where `vertical_diffusion` takes it -- in ONE pass: b, u
        and v are read once and the result written once (32 B/cell in float64, against about 170 for the nine launches of
        the chain); every intermediate stays in registers.

        b at (Z:center, Y:center, X:center), u at (Z:center, Y:center, X:left), v at (Z:center, Y:left, X:center), any
        leading dims, Z third from last; the result has dims (lead, Z face, Y:center, X:center).  `to`: the flux position
        on Z, "left" (nz faces) or "outer" (nz + 1); None: "outer" when the Z axis has one, else "left", as in
        `vertical_diffusion`.  Bit-identical, dims, coords and name included, to the chain

            kw = dict(padding=padding, fill_value=fill_value)
            step = grid.derivative if metric_weighted else grid.diff
            uz = grid.interp(step(u, z_axis, to=to, **kw), x_axis, **kw)   # (Zf, YC, XG) -> (Zf, YC, XC)
            vz = grid.interp(step(v, z_axis, to=to, **kw), y_axis, **kw)   # (Zf, YG, XC) -> (Zf, YC, XC)
            s2 = uz * uz + vz * vz                                         # vertical_shear_squared
            ri = step(b, z_axis, to=to, **kw) / s2

        MITgcm's form: the shear is averaged to the centre first and squared then.  Pads where the chain pads.  Along Z, u,
        v and b above level 0 and, "outer", below level nz-1 (periodic: the far level; extend: the level itself, so the
        difference is exactly 0; fill: `fill_value`).  Along X and Y the Z-DERIVATIVES right of the last column / above the
        last row (periodic: the derivative at index 0, extend: at n-1, fill: `fill_value` itself, not a derivative formed
        from it).  No fused multiply-add, IEEE quotients.

        No guard on S2 == 0: the quotient is IEEE's, inf, or NaN for 0 / 0 (both differences vanish at the outermost faces
        under `extend` with "outer").  A floor on the shear belongs to the closure.

        The metrics are whatever `get_metric` returns at the three derivatives' dims (drC, or registered 3-D thicknesses at
        u's points, at v's points and at the centre), one broadcast array each, read through strides.

        The chain itself runs (the same calls in the same order) for integer, float16 or mixed dtypes, for fewer than three
        dims or Z not third from last, for u or v not on the C-grid positions above or fields of different shapes, for
        another `to` or a position the axis lacks, for chunked inputs or chunked metrics, for a metric with dims its stage
        lacks, for a metric lookup that raises (the chain raises it), for an axis without a boundary, for fields without a
        level along Z, and with face connections or a fold along any of the three axes."""
        return self._richardson(b, u, v, x_axis, y_axis, z_axis, to, padding, fill_value, metric_weighted)

    def richardson_mixing(self, b, u, v, nu0=5e-3, alpha=5.0, nu_b=1e-4, kappa_b=1e-5, shear_floor=0.0, x_axis: str = "X",
                          y_axis: str = "Y", z_axis: str = "Z", to=None, padding=None, fill_value=None,
                          metric_weighted: bool = True):
        """Vertical viscosity `nu` and diffusivity `kappa` of the Pacanowski-Philander (1981) closure -- the middle link of
        the Ri -> nu -> mixing loop, at the faces where `implicit_vertical_viscosity` takes nu and `vertical_diffusion` /
        `implicit_vertical_diffusion` take kappa -- in ONE pass: b, u and v are read once and both results written once
        (40 B/cell in float64, against about 250 for the chain's launches); Ri and every other intermediate stay in registers.

        Positions, `to`, pads, metrics and leading dims are `richardson_number`'s: b at the centre, u at (Y:center, X:left),
        v at (Y:left, X:center), Z third from last; both results have dims (lead, Z face, Y:center, X:center).  Returns
        (nu, kappa), bit-identical, dims, coords and names included, to the chain

            kw   = dict(padding=padding, fill_value=fill_value)
            step = grid.derivative if metric_weighted else grid.diff
            s2   = grid.vertical_shear_squared(u, v, x_axis, y_axis, z_axis, to=to, metric_weighted=metric_weighted, **kw)
            n2   = step(b, z_axis, to=to, **kw)
            ri   = n2 / (s2 + shear_floor)          # an additive floor on the shear
            rp   = (ri + abs(ri)) * 0.5             # max(ri, 0)
            den  = 1.0 + alpha * rp
            nu   = nu0 / (den * den) + nu_b         # exponent 2, as a product
            kappa = nu / den + kappa_b

        Every operation is in the fields' dtype, each scalar cast to it once; no fused multiply-add, IEEE quotients.  The
        defaults are PP81's constants in SI units (m2/s; `shear_floor` in 1/s2): an interface choice, nothing measured.

        `rp` is max(ri, 0) for every finite ri and +0.0 for -0.0, so where the column is statically unstable (Ri < 0) the
        results are the closure's maximum, exactly `nu0 + nu_b` and `(nu0 + nu_b) + kappa_b`; elsewhere
        nu_b <= nu <= nu0 + nu_b.  Ri = +inf (N2 > 0 over no shear) gives the background values nu_b and kappa_b (alpha > 0); a NaN
        stays NaN in both results; Ri = -inf gives NaN (inf - inf), as the chain does.  With `shear_floor=0.0` the
        outermost faces under `extend` with "outer" are 0 / 0 = NaN (both differences vanish there); the implicit solves
        never read those faces (no flux through the top and the bottom), and a positive `shear_floor` makes them finite.

        Out of scope: convective adjustment (a larger kappa where N2 < 0), an exponent other than 2, clipping of nu.

        The one pass serves the call when each of the five scalars is a Python int or float, or a numpy floating scalar that
        does not promote the fields' dtype.  For anything else (a labelled or plain array, a numpy scalar of a wider type)
        and in every case `richardson_number` hands to its chain (the list in its docstring), the chain above itself runs,
        the same calls in the same order, raising what it raises."""
        return self._richardson(b, u, v, x_axis, y_axis, z_axis, to, padding, fill_value, metric_weighted,
                                closure=(nu0, alpha, nu_b, kappa_b, shear_floor))

    def _richardson(self, b, u, v, x_axis, y_axis, z_axis, to, padding, fill_value, metric_weighted, closure=None):
        """`richardson_number`, or with b None `vertical_shear_squared`: one launch of K7n, or their chain.  `closure`
        (nu0, alpha, nu_b, kappa_b, shear_floor): `richardson_mixing`, one launch of K7p, or its chain"""
        ri = b is not None
        args = (b, u, v)
        (b, xr0), (u, xr1), (v, xr2) = (self._wrap_in(a) for a in args)
        was_xr = xr0 or xr1 or xr2
        to, pts = self._column_points(x_axis, y_axis, z_axis, to)
        plan = mets = None
        fields = [f for f in (u, v, b) if f is not None]
        served = all(isinstance(f, DataArray) and f.ndim >= 3 for f in fields) and pts is not None and u.shape[-3] > 0
        if served:
            tz, zf, yc, yl, xc, xl, held = pts
            lead = u.dims[:-3]
            served = (u.dims == lead + (tz, yc, xl) and v.dims == lead + (tz, yl, xc) and (not ri or b.dims == lead + (tz, yc, xc))
                      and not held & set(lead))
        if served:
            f_shape = tuple(u.shape[:-3]) + (u.shape[-3] + (1 if to == "outer" else 0),) + tuple(u.shape[-2:])
            f_dims = [lead + (zf, yc, xl), lead + (zf, yl, xc), lead + (zf, yc, xc)]   # the derivatives of u, v, b; the result
            mets = self._stage_metrics([(dims, (z_axis,), f.name) for dims, f in zip(f_dims, fields)], u.data, metric_weighted)
        if mets is not None:
            mets += [None] * (3 - len(mets))   # (no b: no third stage)
            plan = self._xyz_plan(fields, x_axis, y_axis, z_axis, padding, fill_value, [m for m in mets if m is not None])
        if plan is not None and closure is not None and not all(_weak_scalar(s, u.data) for s in closure):
            plan = None   # (an array, a wider numpy scalar: the chain's own promotion)
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            b, u, v = args
            step = self.derivative if metric_weighted else self.diff
            if closure is not None:
                nu0, alpha, nu_b, kappa_b, shear_floor = closure
                s2 = self.vertical_shear_squared(u, v, x_axis, y_axis, z_axis, to=to, metric_weighted=metric_weighted, **kw)
                n2 = step(b, z_axis, to=to, **kw)
                r = n2 / (s2 + shear_floor)
                rp = (r + abs(r)) * 0.5
                den = 1.0 + alpha * rp
                nu = nu0 / (den * den) + nu_b
                return nu, nu / den + kappa_b
            uz = self.interp(step(u, z_axis, to=to, **kw), x_axis, **kw)
            vz = self.interp(step(v, z_axis, to=to, **kw), y_axis, **kw)
            s2 = uz * uz + vz * vz
            return step(b, z_axis, to=to, **kw) / s2 if ri else s2
        bcx, bcy, fvx, fvy, bcz, fvz = plan
        host = not any(_is_tensor(f.data) for f in fields)
        mu, mv, mb = (None if m is None else _aligned_view(m, dims) for m, dims in zip(mets, f_dims))
        if closure is not None:
            outs = _dev.richardson_mixing(b.data, u.data, v.data, mu, mv, mb, *(float(s) for s in closure), to == "outer",
                                          bcx, bcy, bcz, fvx, fvy, fvz)
        else:
            outs = (_dev.richardson_number(b.data if ri else None, u.data, v.data, mu, mv, mb, to == "outer", bcx, bcy, bcz,
                                           fvx, fvy, fvz),)

        # dims, coords and name as the chain's, step by step over placeholders: the derivatives at the faces (named after
        # their quotients with the metric), the two means at the centre, the squares, their sum, the quotient
        def faces(f, k):
            g = self._labels_of_step(f, f_dims[k], zf, f_shape)
            return g if mets[k] is None else g._replace(name=_name_after(g.name, mets[k]))

        uz, vz = self._labels_of_step(faces(u, 0), f_dims[2], xc), self._labels_of_step(faces(v, 1), f_dims[2], yc)
        res = self._labels_of_binary(self._labels_of_binary(uz, uz), self._labels_of_binary(vz, vz))
        if ri:
            res = self._labels_of_binary(faces(b, 2), res)
        # (the closure's steps pair an array with itself or with a scalar: coords and name stay the quotient's)
        outs = tuple(res._replace(data=_dev.tohost(out) if host else out) for out in outs)
        outs = tuple(to_xarray(r) for r in outs) if was_xr else outs
        return outs if closure is not None else outs[0]

    def isopycnal_slope(self, b, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", to=None, padding=None,
                        fill_value=None, metric_weighted: bool = True):
        """Slopes of the surfaces of constant b (buoyancy, density, any tracer), Sx = -(db/dx) / (db/dz) and
        Sy = -(db/dy) / (db/dz) -- what Gent-McWilliams eddy transport, Redi diffusion and every isoneutral diagnostic
        start from, at the centre points of the faces of Z, where MITgcm's gmredi forms them and `richardson_number`,
        `richardson_mixing` and `vertical_diffusion` put their face fields -- in ONE pass: b is read once and both results
        written once (24 B/cell in float64, against about 190 for the eleven launches of the chain); every intermediate
        stays in registers.

        b at (Z:center, Y:center, X:center), any leading dims, Z third from last; both results have dims (lead, Z face,
        Y:center, X:center).  `to`: the face position on Z, "left" (nz faces) or "outer" (nz + 1); None: "outer" when the Z
        axis has one, else "left", as in `richardson_number`.  Returns (sx, sy), bit-identical, dims, coords and names
        included, to the chain

            kw   = dict(padding=padding, fill_value=fill_value)
            step = grid.derivative if metric_weighted else grid.diff
            gx = grid.interp(grid.interp(step(b, x_axis, **kw), x_axis, **kw), z_axis, to=to, **kw)
            gy = grid.interp(grid.interp(step(b, y_axis, **kw), y_axis, **kw), z_axis, to=to, **kw)
            bz = step(b, z_axis, to=to, **kw)
            sx, sy = -(gx / bz), -(gy / bz)

        Sign convention: all three derivatives run along increasing index, so the result is the slope of the b-surfaces in
        the grid's own Z coordinate, d(Z of the surface) / dx and / dy.  For a Z index that grows downward with positive
        `drC` (MITgcm) that is the slope of their DEPTH: positive where the surface deepens towards larger x.

        Pads where the chain pads, every stage its own input.  b left of column 0 / below row 0 (periodic: b[n-1], extend:
        b[0], fill: `fill_value`); the DERIVATIVE right of the last column / above the last row (periodic: the derivative
        at index 0, extend: at n-1, fill: `fill_value` itself); the LEVEL MEANS above level 0 and, "outer", below level
        nz-1 (periodic: the far level's, extend: the level's own, fill: `fill_value` itself); b along Z as
        `richardson_number` pads it.  No fused multiply-add, IEEE quotients, no guard on db/dz == 0: under `extend` the
        outermost faces are x / 0.

        Out of scope: slope clipping and tapering (GM's `clipping`, `gkw91`, `dm95`, `ldd97`), the natural follow-up.

        The metrics are whatever `get_metric` returns for X at dims (lead, Z:center, Y:center, X:left), for Y at (lead,
        Z:center, Y:left, X:center) and for Z at (lead, Z face, Y:center, X:center) (dxC, dyC, drC, or registered 3-D
        arrays), one broadcast array each, read through strides; each may be absent on its own terms.

        The chain itself runs (the same calls in the same order) for integer, float16 or mixed dtypes, for fewer than three
        dims or Z not third from last, for b elsewhere than the centre, for another `to` or a position the axis lacks, for
        a chunked input or chunked metrics, for a metric with dims its stage lacks, for a metric lookup that raises (the
        chain raises it), for an axis without a boundary, for a field without a level along Z, and with face connections
        or a fold along any of the three axes."""
        return self._isopycnal(b, x_axis, y_axis, z_axis, to, padding, fill_value, metric_weighted)

    def redi_tensor(self, b, kappa=1000.0, slope_max=1e-2, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", to=None,
                    padding=None, fill_value=None, metric_weighted: bool = True):
        """The tapered tensor column Kwx, Kwy, Kwz of Redi isoneutral diffusion and the Gent-McWilliams skew flux at the W
        points, as MITgcm's `gmredi_calc_tensor` forms it -- Kwx = kappa taper Sx, Kwy = kappa taper Sy,
        Kwz = kappa taper (Sx^2 + Sy^2), the last the diffusivity `implicit_vertical_diffusion` takes as its 3-D `kappa`, at
        its position -- in ONE pass: b is read once and the three results written once (32 B/cell in float64, against about
        300 for `isopycnal_slope` and the thirteen launches after it); the slopes and every other intermediate stay in
        registers.

        Positions, `to`, pads, metrics and leading dims are `isopycnal_slope`'s: b at the centre, Z third from last; all
        three results have dims (lead, Z face, Y:center, X:center).  Returns (kwx, kwy, kwz), bit-identical, dims, coords
        and names included, to the chain

            kw = dict(padding=padding, fill_value=fill_value)
            sx, sy = grid.isopycnal_slope(b, x_axis, y_axis, z_axis, to=to, metric_weighted=metric_weighted, **kw)
            s2 = sx * sx + sy * sy
            if slope_max is None:                    # untapered
                kt = kappa
            else:                                    # Gerdes-Koeberle-Willebrand 1991: taper = min(1, (Smax/|S|)^2), no sqrt
                m2  = float(slope_max) * float(slope_max)   # one Python product, cast to the fields' dtype once
                ex  = s2 - m2
                den = m2 + (ex + abs(ex)) * 0.5      # max(s2, m2)
                kt  = kappa * (m2 / den)
            kwx, kwy, kwz = kt * sx, kt * sy, kt * s2

        Every operation is in the fields' dtype; no fused multiply-add, IEEE quotients.  The defaults are MITgcm's usual GM
        background diffusivity (m2/s) and `GM_maxSlope`: an interface choice, nothing measured.

        Exact identity below the limit: where s2 <= m2, `ex + abs(ex)` is exactly +0.0, `den` is exactly m2 and the taper
        exactly 1, so the results carry the bits of kappa * sx, kappa * sy and kappa * s2 -- those of `slope_max=None`.
        Bound above the limit: where s2 > m2 the taper is at most 1 and kwz stays near kappa m2 for every finite s2,
        kwz <= kappa m2 (1 + 4 eps): `den` is m2 + (s2 - m2), two roundings from s2, the quotient adds one and each of the
        two products one.  No guard on db/dz == 0, as in `isopycnal_slope`: an infinite slope gives taper 0 and
        0 * inf = NaN in all three results, so the outermost faces under `extend` with "outer" are NaN; the implicit solves
        never read those faces.  A NaN stays NaN.  float32 range: sx * sx overflows above about 1.8e19; the operator does
        what the chain does.

        Out of scope: other tapers (`clipping`, `dm95`, `ldd97`: tanh cannot be held to numpy bit for bit) and the U- and
        V-point tensor components.  kwx and kwy are what `redi_vertical_flux_divergence` takes, as they are.

        The one pass serves the call when `isopycnal_slope`'s would (the list in its docstring) and `kappa` and `slope_max`
        are each a Python int or float, or a numpy floating scalar that does not promote the fields' dtype (`slope_max` may
        be None).  For anything else (an array-valued kappa, a numpy scalar of a wider type) the chain above itself runs,
        the same calls in the same order, raising what it raises; neither scalar is validated beyond that."""
        return self._isopycnal(b, x_axis, y_axis, z_axis, to, padding, fill_value, metric_weighted, tensor=(kappa, slope_max))

    def redi_horizontal_tensor(self, b, kappa=1000.0, slope_max=1e-2, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z",
                               to=None, padding=None, fill_value=None, metric_weighted: bool = True):
        """The tapered off-diagonal components of the Redi / Gent-McWilliams tensor at the U and the V points, Kuz = kappa
        taper Sx at u's points and Kvz = kappa taper Sy at v's points -- what the horizontal isoneutral flux
        Kux da/dx + Kuz <da/dz> needs beside `redi_tensor`'s W-point column -- from b alone in ONE pass: b is read once and
        the two results written once (24 B/cell in float64, against about 720 for the forty launches of the chain).  The
        diagonal stays the scalar `kappa` (MITgcm's default unit diagonal); the operator that applies (kappa, Kuz, Kvz) to
        a tracer is not part of this method.

        b at (lead, Z:center, Y:center, X:center), Z third from last.  Returns (kuz, kvz): `kuz` with dims (lead, Z:center,
        Y:center, X:left), `kvz` with (lead, Z:center, Y:left, X:center), bit-identical, dims, coords and names included, to
        the chain

            kw   = dict(padding=padding, fill_value=fill_value)
            step = grid.derivative if metric_weighted else grid.diff
            gx   = step(b, x_axis, **kw)                                   # u points
            gy   = step(b, y_axis, **kw)                                   # v points
            bzc  = grid.interp(step(b, z_axis, to=to, **kw), z_axis, to="center", **kw)   # db/dz: faces, then back to the levels
            bzu  = grid.interp(bzc, x_axis, to="left", **kw);   bzv = grid.interp(bzc, y_axis, to="left", **kw)
            gyu  = grid.interp(grid.interp(gy, y_axis, to="center", **kw), x_axis, to="left", **kw)   # db/dy at u points
            gxv  = grid.interp(grid.interp(gx, x_axis, to="center", **kw), y_axis, to="left", **kw)   # db/dx at v points
            sxu, syu = -(gx / bzu),  -(gyu / bzu)
            sxv, syv = -(gxv / bzv), -(gy / bzv)
            for (sa, sb, pick) in ((sxu, syu, sxu), (sxv, syv, syv)):      # redi_tensor's taper, at each point with both slopes there
                s2 = sa * sa + sb * sb
                if slope_max is None:
                    kt = kappa
                else:
                    m2  = float(slope_max) * float(slope_max)              # as in redi_tensor
                    ex  = s2 - m2
                    kt  = kappa * (m2 / (m2 + (ex + abs(ex)) * 0.5))
                result = kt * pick                                         # kuz = kt_u * sxu,  kvz = kt_v * syv

        every operation in the fields' dtype, no fused multiply-add, IEEE quotients, the negation a product with -1, no
        guard on a zero db/dz.  `to` is the face position at which db/dz is formed, "left" or "outer"; None resolves as in
        `isopycnal_slope`.  Every stage pads its own input, as the chain does: with "left" the mean back to the levels
        pads the derivative beyond the last face; with "outer" no pad along Z is used after b's own.  The pads of bzc, of
        the centre mean of gy left of column 0 and of the centre mean of gx below row 0 are those stages' own (periodic:
        the far one, extend: its own, fill: `fill_value` itself).

        `kappa=1.0, slope_max=None` gives the bare slopes at the U and V points exactly, Sx at u's and Sy at v's: the
        results are 1.0 * s, which carries the bits of s.

        Under `extend` the first and the last level see half the stratification: the outermost face derivative is
        b - b = 0, so the mean back to the level is half the inner face's and the slopes there are doubled before the
        taper.  MITgcm's tensor has the same property; nothing is built around it.

        The results are exactly 0 / 0 where the 4-point mean of db/dz cancels: for one level with "outer" under any
        boundary, for one level with "left" unless Z is `fill`, and for two levels with periodic Z.

        Bound where tapered (s2 > m2): |kuz| and |kvz| <= kappa slope_max (1 + 7 eps), see
        `tests/test_redi_horizontal_tensor.py` for the count.  The metrics are `isopycnal_slope`'s: X at (lead, Z:center,
        Y:center, X:left), Y at (lead, Z:center, Y:left, X:center), Z at (lead, Z face, Y:center, X:center), one broadcast
        array each, each may be absent on its own.

        Out of scope: the tracer operator on (kappa, Kuz, Kvz), a non-unit diagonal, other tapers, land masks and partial
        cells.

        The one pass serves exactly the calls that `isopycnal_slope`'s one pass serves (the list in its docstring) with
        `kappa` and `slope_max` each a Python int or float, or a numpy floating scalar that does not promote the fields'
        dtype (`slope_max` may be None).  For everything else the chain above itself runs, the same calls in the same
        order, raising what it raises."""
        return self._isopycnal(b, x_axis, y_axis, z_axis, to, padding, fill_value, metric_weighted, tensor=(kappa, slope_max),
                               horizontal=True)

    def _redi_horizontal_chain(self, b, kappa, slope_max, x_axis, y_axis, z_axis, to, padding, fill_value, metric_weighted):
        """the chain of `redi_horizontal_tensor`'s docstring, call by call (`to` already resolved): every fallback of the one pass"""
        kw = dict(padding=padding, fill_value=fill_value)
        step = self.derivative if metric_weighted else self.diff
        gx = step(b, x_axis, **kw)
        gy = step(b, y_axis, **kw)
        bzc = self.interp(step(b, z_axis, to=to, **kw), z_axis, to="center", **kw)
        bzu = self.interp(bzc, x_axis, to="left", **kw)
        bzv = self.interp(bzc, y_axis, to="left", **kw)
        gyu = self.interp(self.interp(gy, y_axis, to="center", **kw), x_axis, to="left", **kw)
        gxv = self.interp(self.interp(gx, x_axis, to="center", **kw), y_axis, to="left", **kw)
        sxu, syu = -(gx / bzu), -(gyu / bzu)
        sxv, syv = -(gxv / bzv), -(gy / bzv)
        outs = []
        for sa, sb, pick in ((sxu, syu, sxu), (sxv, syv, syv)):
            s2 = sa * sa + sb * sb
            if slope_max is None:
                kt = kappa
            else:
                m2 = float(slope_max) * float(slope_max)
                ex = s2 - m2
                den = m2 + (ex + abs(ex)) * 0.5
                kt = kappa * (m2 / den)
            outs.append(kt * pick)
        return tuple(outs)

    def _isopycnal(self, b, x_axis, y_axis, z_axis, to, padding, fill_value, metric_weighted, tensor=None, horizontal=False):
        """`isopycnal_slope`: one launch of K7q, or its chain.  `tensor` (kappa, slope_max): `redi_tensor`, one launch of
        K7r, or its chain; with `horizontal`: `redi_horizontal_tensor`, one launch of K7u, or its chain"""
        arg, to_arg = b, to
        b, was_xr = self._wrap_in(b)
        to, pts = self._column_points(x_axis, y_axis, z_axis, to)
        plan = mets = None
        served = isinstance(b, DataArray) and b.ndim >= 3 and pts is not None and b.shape[-3] > 0
        if served:
            tz, zf, yc, yl, xc, xl, held = pts
            lead = b.dims[:-3]
            served = b.dims == lead + (tz, yc, xc) and not held & set(lead)
        if served:
            f_shape = tuple(b.shape[:-3]) + (b.shape[-3] + (1 if to == "outer" else 0),) + tuple(b.shape[-2:])
            c_dims = lead + (tz, yc, xc)
            m_dims = [lead + (tz, yc, xl), lead + (tz, yl, xc), lead + (zf, yc, xc)]   # the three derivatives' dims
            mets = self._stage_metrics([(dims, (ax,), b.name) for dims, ax in zip(m_dims, (x_axis, y_axis, z_axis))], b.data,
                                       metric_weighted)
        if mets is not None:
            plan = self._xyz_plan([b], x_axis, y_axis, z_axis, padding, fill_value, [m for m in mets if m is not None])
        if plan is not None and tensor is not None and not (_weak_scalar(tensor[0], b.data)
                                                            and (tensor[1] is None or _weak_scalar(tensor[1], b.data))):
            plan = None   # (an array, a wider numpy scalar: the chain's own promotion)
        if plan is None and horizontal:
            return self._redi_horizontal_chain(arg, tensor[0], tensor[1], x_axis, y_axis, z_axis, to, padding, fill_value, metric_weighted)
        if plan is None and tensor is not None:
            kappa, slope_max = tensor
            kw = dict(padding=padding, fill_value=fill_value)
            sx, sy = self.isopycnal_slope(arg, x_axis, y_axis, z_axis, to=to_arg, metric_weighted=metric_weighted, **kw)
            s2 = sx * sx + sy * sy
            if slope_max is None:
                kt = kappa
            else:
                m2 = float(slope_max) * float(slope_max)
                ex = s2 - m2
                den = m2 + (ex + abs(ex)) * 0.5
                kt = kappa * (m2 / den)
            return kt * sx, kt * sy, kt * s2
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            step = self.derivative if metric_weighted else self.diff
            gx = self.interp(self.interp(step(arg, x_axis, **kw), x_axis, **kw), z_axis, to=to, **kw)
            gy = self.interp(self.interp(step(arg, y_axis, **kw), y_axis, **kw), z_axis, to=to, **kw)
            bz = step(arg, z_axis, to=to, **kw)
            return -(gx / bz), -(gy / bz)
        bcx, bcy, fvx, fvy, bcz, fvz = plan
        host = not _is_tensor(b.data)
        mx, my, mz = (None if m is None else _aligned_view(m, dims) for m, dims in zip(mets, m_dims))
        if horizontal:
            m2 = None if tensor[1] is None else float(tensor[1]) * float(tensor[1])
            outs = _dev.redi_horizontal_tensor(b.data, mx, my, mz, float(tensor[0]), m2, to == "outer", bcx, bcy, bcz, fvx, fvy, fvz)
        elif tensor is not None:
            m2 = None if tensor[1] is None else float(tensor[1]) * float(tensor[1])
            outs = _dev.redi_tensor(b.data, mx, my, mz, float(tensor[0]), m2, to == "outer", bcx, bcy, bcz, fvx, fvy, fvz)
        else:
            outs = _dev.isopycnal_slope(b.data, mx, my, mz, to == "outer", bcx, bcy, bcz, fvx, fvy, fvz)

        # dims, coords and names as the chain's, step by step over placeholders: each derivative (named after its quotient
        # with the metric), the mean back to the centre, the mean at the faces, the quotient (the negation changes neither)
        bz = named(self._labels_of_step(b, m_dims[2], zf, f_shape), mets[2])
        if horizontal:
            # the two derivatives, db/dz back at the levels and at the two points, the cross means, the four quotients; then
            # the taper's steps as below
            step, both = self._labels_of_step, self._labels_of_binary
            gx, gy = named(step(b, m_dims[0], xl), mets[0]), named(step(b, m_dims[1], yl), mets[1])
            bzc = step(bz, c_dims, tz, b.shape)
            bzu, bzv = step(bzc, m_dims[0], xl), step(bzc, m_dims[1], yl)
            gyu = step(step(gy, c_dims, yc), m_dims[0], xl)
            gxv = step(step(gx, c_dims, xc), m_dims[1], yl)
            res = []
            for sa, sb, own in ((both(gx, bzu), both(gyu, bzu), 0), (both(gxv, bzv), both(gy, bzv), 1)):
                pick = (sa, sb)[own]
                res.append(pick if tensor[1] is None else both(both(both(sa, sa), both(sb, sb)), pick))
            outs = tuple(r._replace(data=_dev.tohost(out) if host else out) for r, out in zip(res, outs))
            return tuple(to_xarray(r) for r in outs) if was_xr else outs
        res = []
        for k, (dim_l, dim_c) in enumerate(((xl, xc), (yl, yc))):
            g = named(self._labels_of_step(b, m_dims[k], dim_l), mets[k])
            g = self._labels_of_step(self._labels_of_step(g, c_dims, dim_c), m_dims[2], zf, f_shape)
            res.append(self._labels_of_binary(g, bz))
        if tensor is not None:
            # sx * sx + sy * sy; every step with a scalar keeps coords and name, so kt (tapered) carries those of s2 and
            # kappa (untapered) none of its own
            lx, ly = res
            s2 = self._labels_of_binary(self._labels_of_binary(lx, lx), self._labels_of_binary(ly, ly))
            both = self._labels_of_binary
            res = [lx, ly, s2] if tensor[1] is None else [both(s2, lx), both(s2, ly), both(s2, s2)]
        outs = tuple(r._replace(data=_dev.tohost(out) if host else out) for r, out in zip(res, outs))
        return tuple(to_xarray(r) for r in outs) if was_xr else outs

    def redi_vertical_flux_divergence(self, a, kwx, kwy, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", to=None,
                                      closed: bool = True, padding=None, fill_value=None, metric_weighted: bool = True):
        """The explicit part of Redi isoneutral diffusion (and of the Gent-McWilliams skew flux) of a tracer along Z: the
        divergence of the off-diagonal vertical flux, d/dz(Kwx <da/dx> + Kwy <da/dy>) -- what MITgcm's `gmredi_rtransport`
        adds next to the implicit solve with Kwz -- in ONE pass: `a`, `kwx` and `kwy` are read once and the result written
        once (32 B/cell in float64, against about 200 for the chain); the gradients and the flux stay in registers.  With it
        the tracer side is `redi_tensor(b)` once per step, this operator once per tracer, and
        `implicit_vertical_diffusion(a, kwz, dt)` once per tracer.

        `a` at (Z:center, Y:center, X:center), any leading dims, Z third from last.  `kwx` and `kwy` at (lead, Z face,
        Y:center, X:center): the dims and the position of `redi_tensor`'s results.  `to`: the face position, "left" or
        "outer"; None: "outer" when the Z axis has one, else "left".  The result has `a`'s dims.  Bit-identical, dims,
        coords and name included, to the chain

            kw   = dict(padding=padding, fill_value=fill_value)
            step = grid.derivative if metric_weighted else grid.diff
            gx = grid.interp(grid.interp(step(a, x_axis, **kw), x_axis, **kw), z_axis, to=to, **kw)
            gy = grid.interp(grid.interp(step(a, y_axis, **kw), y_axis, **kw), z_axis, to=to, **kw)
            f  = kwx * gx + kwy * gy            # two products, one sum, in the fields' dtype, no fused multiply-add
            if closed:                          # no flux through the top and the bottom
                f = a copy of f with face 0 -- and with to="outer" also face nz -- set to +0.0
            out = step(f, z_axis, **kw)         # faces -> centre: (f[k+1] - f[k]) [/ drF]

        gx and gy are `isopycnal_slope`'s, formed of `a`; the copy keeps f's dims, coords and name.

        `closed=True`, the default, is MITgcm's condition and makes the operator usable on `redi_tensor`'s results as they
        are (their outermost faces are NaN under `extend` with "outer").  The closed faces are exactly +0.0: no value of
        `kwx`, of `kwy` or of a pad of the level means there reaches the result, a NaN included.  With "outer" no pad along
        Z is used at all.  With "left" face 0 is closed and the flux beyond level nz-1 is the chain's pad of f (periodic:
        f[0], the closed +0.0; extend: f[nz-1]; fill: `fill_value` itself).  `closed=False` is the plain chain with every
        pad along Z: the level means above level 0 and, "outer", below level nz-1 as in `isopycnal_slope`, the flux beyond
        nz-1 ("left") as in `vertical_diffusion`.  The X and Y pads are `isopycnal_slope`'s in both modes.

        Sign convention: `isopycnal_slope`'s, all derivatives run along increasing index.  With `a = b` the explicit flux
        here and `kwz * db/dz` cancel up to rounding: there is no isoneutral flux of the field that defines the surfaces.
        Under the skew-flux form with equal GM and Redi diffusivities the caller passes `2 * kwx, 2 * kwy`, an exact
        scaling; nothing is built for it.  Out of scope: the U- and V-point components of the tensor (the horizontal
        fluxes), other closures of the boundary, and `maskC`-style land masks.

        The metrics are whatever `get_metric` returns for X at (lead, Z:center, Y:center, X:left), for Y at (lead,
        Z:center, Y:left, X:center) and for Z at `a`'s dims (dxC, dyC, drF, or registered 3-D arrays), one broadcast array
        each; each may be absent on its own terms.

        The one pass serves the call exactly when `isopycnal_slope`'s would for `a` (the list in its docstring; float32 /
        float64 only), `kwx` and `kwy` are unchunked labelled arrays of `a`'s dtype with exactly the flux' dims and shape,
        and the Z metric at `a`'s dims passes the tests of the other two.  For everything else the chain above itself
        runs, the same calls in the same order, raising what it raises.  Its closing step needs a materialised flux: a
        chunked flux and one deferred under `grid.fused()` are computed first (a host array, or wherever the deferred
        value lives), then copied and closed; a flux without the face dim is handed on as it is."""
        args, to_arg = (a, kwx, kwy), to
        (a, xr1), (kwx, xr2), (kwy, xr3) = self._wrap_in(a), self._wrap_in(kwx), self._wrap_in(kwy)
        was_xr = xr1 or xr2 or xr3
        to, pts = self._column_points(x_axis, y_axis, z_axis, to)
        plan = mets = None
        served = (isinstance(a, DataArray) and isinstance(kwx, DataArray) and isinstance(kwy, DataArray) and a.ndim >= 3
                  and pts is not None and a.shape[-3] > 0)
        if served:
            tz, zf, yc, yl, xc, xl, held = pts
            lead = a.dims[:-3]
            served = a.dims == lead + (tz, yc, xc) and not held & set(lead)
        if served:
            f_shape = tuple(a.shape[:-3]) + (a.shape[-3] + (1 if to == "outer" else 0),) + tuple(a.shape[-2:])
            c_dims, f_dims = lead + (tz, yc, xc), lead + (zf, yc, xc)
            m_dims = [lead + (tz, yc, xl), lead + (tz, yl, xc), c_dims]   # the two derivatives' dims and the result's
            served = all(k.dims == f_dims and tuple(k.shape) == f_shape for k in (kwx, kwy))
        if served:
            mets = self._stage_metrics([(dims, (ax,), a.name) for dims, ax in zip(m_dims, (x_axis, y_axis, z_axis))], a.data,
                                       metric_weighted)
        if mets is not None and not any(_is_chunked(k.data) for k in (kwx, kwy)):
            dtype = _dt.np_dtype(a.data)
            if all(_dt.np_dtype(k.data) == dtype for k in (kwx, kwy)):
                plan = self._xyz_plan([a], x_axis, y_axis, z_axis, padding, fill_value, [m for m in mets if m is not None])
        if plan is None:
            a, kwx, kwy = args
            kw = dict(padding=padding, fill_value=fill_value)
            step = self.derivative if metric_weighted else self.diff
            gx = self.interp(self.interp(step(a, x_axis, **kw), x_axis, **kw), z_axis, to=to, **kw)
            gy = self.interp(self.interp(step(a, y_axis, **kw), y_axis, **kw), z_axis, to=to, **kw)
            f = kwx * gx + kwy * gy
            if closed:
                f = self._closed_flux(f, self.axes[z_axis].coords.get(to), to == "outer")
            return step(f, z_axis, **kw)
        bcx, bcy, fvx, fvy, bcz, fvz = plan
        host = not any(_is_tensor(x.data) for x in (a, kwx, kwy))
        mx, my, mc = (None if m is None else _aligned_view(m, dims) for m, dims in zip(mets, m_dims))
        out = _dev.redi_vertical_flux_divergence(a.data, kwx.data, kwy.data, mx, my, mc, to == "outer", bool(closed), bcx, bcy,
                                                 bcz, fvx, fvy, fvz)

        # dims, coords and name as the chain's, step by step over placeholders: each derivative (named after its quotient
        # with the metric), the mean back to the centre, the mean at the faces, the product with the tensor component; the
        # sum (closing it changes neither coords nor name); the step back to the centre, named after its metric quotient
        prods = []
        for k, (dim_l, dim_c, kwk) in enumerate(((xl, xc, kwx), (yl, yc, kwy))):
            g = named(self._labels_of_step(a, m_dims[k], dim_l), mets[k])
            g = self._labels_of_step(self._labels_of_step(g, c_dims, dim_c), f_dims, zf, f_shape)
            prods.append(self._labels_of_binary(kwk, g))
        f = self._labels_of_binary(*prods)
        res = named(self._labels_of_step(f, c_dims, tz, a.shape), mets[2])
        res = res._replace(data=_dev.tohost(out) if host else out)
        return to_xarray(res) if was_xr else res

    def bolus_velocity(self, kwx, kwy, x_axis: str = "X", y_axis: str = "Y", z_axis: str = "Z", closed: bool = True,
                       padding=None, fill_value=None, metric_weighted: bool = True):
        """The Gent-McWilliams eddy-induced (bolus) velocity `(ub, vb, wb)` from the two off-diagonal components of
        `redi_tensor`, `kwx = kappa * taper * Sx` and `kwy = kappa * taper * Sy` -- the GM streamfunction at the W points
        -- in ONE pass: `kwx` and `kwy` are read once and the three results written once (about 40 B/cell in float64,
        against about 184 for the eleven launches of the chain).  It is what MITgcm's `gmredi_calc_psi_b` and
        `gmredi_residual_flow` form of the same tensor column:

            u* = -d/dz(kappa Sx)      v* = -d/dz(kappa Sy)      w* = d/dx(kappa Sx) + d/dy(kappa Sy)

        `flux_divergence_3d(ub, vb, wb, T)` is the advective form of the GM tendency.  With different GM and Redi
        diffusivities the caller scales `kwx` and `kwy` first; nothing is built for it.

        `kwx` and `kwy` at (lead, Z face, Y:center, X:center), Z third from last: the dims and the position of
        `redi_tensor`'s results.  The face position, Z:outer (nz + 1 faces) or Z:left (nz), is read from the inputs' own Z
        dim.  `ub` at (lead, Z:center, Y:center, X:left), `vb` at (lead, Z:center, Y:left, X:center), `wb` at the inputs'
        dims.  Bit-identical, dims, coords and names included, to the chain

            kw   = dict(padding=padding, fill_value=fill_value)
            step = grid.derivative if metric_weighted else grid.diff
            px = grid.interp(kwx, x_axis, **kw)          # psi_x at (Z face, Y:center, X:left): (kwx[i-1] + kwx[i]) * 0.5
            py = grid.interp(kwy, y_axis, **kw)          # psi_y at (Z face, Y:left, X:center)
            if closed:                                   # psi = 0 at the top and the bottom
                px, py = copies with face 0 -- and at Z:outer also face nz -- set to +0.0
            ub = -step(px, z_axis, **kw)                 # -(px[k+1] - px[k]) [/ drF at u's points]
            vb = -step(py, z_axis, **kw)
            tx, ty = px, py
            if metric_weighted:
                tx = px * grid.get_metric(px, (y_axis,))         # dyG: the transport through the west face
                ty = py * grid.get_metric(py, (x_axis,))         # dxG
            wb = grid.divergence(tx, ty, x_axis, y_axis, metric_weighted=metric_weighted, **kw)

        every operation in the fields' dtype, no fused multiply-add, IEEE quotients; the negation is a sign change, so
        `-(+0.0)` is `-0.0`.  The pads are the chain's own: `kwx` left of column 0 and `kwy` below row 0; the TRANSPORTS
        right of the last column and above the last row (fill: `fill_value` itself, not multiplied by a metric); at Z:left
        only, psi beyond face nz-1 (periodic: psi[0], +0.0 when closed; extend: psi[nz-1]; fill: `fill_value`).

        `closed=True`, the default, is MITgcm's condition -- no eddy transport through the top and the bottom -- and makes
        the operator usable on `redi_tensor`'s results as they are: the closed faces' rows of `kwx` and `kwy` are never
        read, so their NaN outermost faces under `extend` reach none of the three results.  The closed faces of `wb` are
        still formed from psi = +0.0 through the same products, differences and quotient; with a non-zero `fill` pad on X
        or Y the chain gives a non-zero `wb` in the last column or row of a closed face, and so does the operator.
        `closed=False` is the plain chain.

        Sign convention: `isopycnal_slope`'s, all derivatives run along increasing index, so d/dx u* + d/dy v* + d/dz w* = 0
        holds in index space.  Discretely `divergence(ub * dyG, vb * dxG) * drF + (wb[k+1] - wb[k]) * rA` is zero to
        rounding when drF is a profile: the eddy-induced flow is non-divergent cell by cell.  Out of scope: partial cells
        (hFac), land masks, the U- and V-point components of the tensor, and the bolus streamfunction integrated along X.

        The one pass serves the call when both inputs are unchunked labelled arrays of the same float32 or float64 dtype,
        dims and shape, the dims are lead + (Z:left | Z:outer, Y:center, X:center) with no grid dim in lead and a level
        along Z, both horizontal axes have `left` and `center` and the Z axis `center`, no axis has a face connection or a
        fold, all three have a boundary, and -- `metric_weighted` -- the five metrics (Z at ub's and at vb's dims, Y at
        px's, X at py's, (X, Y) at wb's) resolve to unchunked arrays whose dims are a subset of their stage's.  For
        everything else the chain above itself runs, the same calls in the same order, raising what it raises; a deferred
        or chunked psi is computed first by the closing step."""
        args = (kwx, kwy)
        (kwx, xr1), (kwy, xr2) = self._wrap_in(kwx), self._wrap_in(kwy)
        was_xr = xr1 or xr2
        zax = self.axes[z_axis]
        to = next((pos for pos in ("outer", "left") if zax.coords.get(pos) in getattr(kwx, "dims", ())), None)
        pts = self._column_points(x_axis, y_axis, z_axis, to)[1]   # (`to` stays the input's own: None, no face dim, runs the chain)
        plan = mets = None
        served = isinstance(kwx, DataArray) and isinstance(kwy, DataArray) and kwx.ndim >= 3 and to is not None and pts is not None
        if served:
            tz, zf, yc, yl, xc, xl, held = pts
            lead = kwx.dims[:-3]
            nz = kwx.shape[-3] - (1 if to == "outer" else 0)
            served = (kwx.dims == lead + (zf, yc, xc) and kwy.dims == kwx.dims and tuple(kwy.shape) == tuple(kwx.shape)
                      and not held & set(lead) and nz > 0)
        if served:
            l_shape = tuple(kwx.shape[:-3]) + (nz,) + tuple(kwx.shape[-2:])
            w_dims = kwx.dims
            # the five metrics' stages: ub's and vb's dims, px's and py's, wb's
            m_dims = [lead + (tz, yc, xl), lead + (tz, yl, xc), lead + (zf, yc, xl), lead + (zf, yl, xc), w_dims]
            m_axes = [(z_axis,), (z_axis,), (y_axis,), (x_axis,), (x_axis, y_axis)]
            mets = self._stage_metrics([(dims, axes, kwx.name) for dims, axes in zip(m_dims, m_axes)], kwx.data, metric_weighted)
        if mets is not None:
            plan = self._xyz_plan([kwx, kwy], x_axis, y_axis, z_axis, padding, fill_value, [m for m in mets if m is not None])
        if plan is None:
            kwx, kwy = args
            kw = dict(padding=padding, fill_value=fill_value)
            step = self.derivative if metric_weighted else self.diff
            px = self.interp(kwx, x_axis, **kw)
            py = self.interp(kwy, y_axis, **kw)
            if closed:
                px = self._closed_flux(px, zax.coords.get(to), to == "outer")
                py = self._closed_flux(py, zax.coords.get(to), to == "outer")
            ub = -step(px, z_axis, **kw)
            vb = -step(py, z_axis, **kw)
            tx, ty = px, py
            if metric_weighted:
                tx = px * self.get_metric(px, (y_axis,))
                ty = py * self.get_metric(py, (x_axis,))
            wb = self.divergence(tx, ty, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
            return ub, vb, wb
        bcx, bcy, fvx, fvy, bcz, fvz = plan
        host = not any(_is_tensor(x.data) for x in (kwx, kwy))
        mzu, mzv, dyg, dxg, ra = (None if m is None else _aligned_view(m, dims) for m, dims in zip(mets, m_dims))
        outs = _dev.bolus_velocity(kwx.data, kwy.data, mzu, mzv, dyg, dxg, ra, to == "outer", bool(closed), bcx, bcy, bcz,
                                   fvx, fvy, fvz)

        # dims, coords and names as the chain's, step by step over placeholders: the two means (closing them changes neither
        # coords nor name), the step to the centre named after its metric quotient (the negation changes neither), the
        # transports named after their products, the divergence nameless with the coords of its two components
        px = self._labels_of_step(kwx, m_dims[2], xl)
        py = self._labels_of_step(kwy, m_dims[3], yl)
        ub = named(self._labels_of_step(px, m_dims[0], tz, l_shape), mets[0])
        vb = named(self._labels_of_step(py, m_dims[1], tz, l_shape), mets[1])
        tx = px if mets[2] is None else self._labels_of_binary(px, mets[2])
        ty = py if mets[3] is None else self._labels_of_binary(py, mets[3])
        wb = _reattach_coords([DataArray(_placeholder(kwx.shape), w_dims)], self, None, {xc, yc}, [tx, ty])[0]
        res = tuple(r._replace(data=_dev.tohost(out) if host else out) for r, out in zip((ub, vb, wb), outs))
        return tuple(to_xarray(r) for r in res) if was_xr else res

    def _closed_flux(self, f, face_dim, outer):
        """a copy of the flux `f` with face 0 and (`outer`) its last face along `face_dim` set to +0.0; dims, coords and name
        stay f's.  A deferred or chunked flux is computed first; a flux without that dim passes as it is"""
        f, was_xr = self._wrap_in(f)
        was_xr = was_xr or bool(getattr(f, "_xr", False))   # (a deferred result of xarray inputs)
        with _lazy.suspended():  # (inside a `fused()` block the products behind a deferred flux must not defer themselves again)
            f = _lazy.plain(f)
        if not isinstance(f, DataArray) or face_dim not in f.dims:
            return to_xarray(f) if was_xr else f
        data = f.data
        if _is_chunked(data):
            data = np.asarray(data)
        data = data.clone() if _is_tensor(data) else np.array(data, copy=True)
        at = [slice(None)] * data.ndim
        for face in (0, -1) if outer else (0,):
            at[f.dims.index(face_dim)] = face
            data[tuple(at)] = 0.0
        f = f._replace(data=data)
        return to_xarray(f) if was_xr else f

    # ---- the momentum side: kinetic energy and the vector-invariant advection term, one pass each ---------------------
    def _c_grid_vector(self, u, v, x_axis, y_axis, what):
        """dims of a C-grid vector's points: (lead, at u, at v, centre, vorticity point); raises when u / v sit elsewhere"""
        xa, ya = self.axes[x_axis], self.axes[y_axis]
        (ux_pos, ux_dim), (uy_pos, uy_dim) = xa._get_position_name(u), ya._get_position_name(u)
        (vx_pos, vx_dim), (vy_pos, vy_dim) = xa._get_position_name(v), ya._get_position_name(v)
        if ((ux_pos, uy_pos, vx_pos, vy_pos) != ("left", "center", "center", "left")
                or "left" not in xa.coords or "left" not in ya.coords):
            raise NotImplementedError(f"fused {what} needs u at (Y:center, X:left) and v at (Y:left, X:center)")
        lead = u.dims[:-2]
        return lead, lead + (uy_dim, ux_dim), lead + (vy_dim, vx_dim), lead + (uy_dim, vx_dim), lead + (vy_dim, ux_dim)

    def _labels_of_step(self, src, dims, out_dim, shape=None):
        """placeholder with the dims, coords and name a one-axis operator gives its result (gridops.HipGridUFunc); `shape`:
        the result's, where the step changes the length of its axis"""
        return _reattach_coords([DataArray(_placeholder(src.shape if shape is None else shape), dims, name=src.name)], self, None,
                                {out_dim}, [src])[0]

    @staticmethod
    def _labels_of_binary(a, b):
        """placeholder with the coords and name of `a OP b` for two arrays of the same dims"""
        return DataArray(_placeholder(a.shape), a.dims, coords=_binary_coords(a, b, a.dims), name=_result_name(a, b))

    def _labels_of_ke(self, u, v, c_dims):
        """dims, coords and name of 0.5 * (interp(u * u, X) + interp(v * v, Y)), step by step over placeholders"""
        ix = self._labels_of_step(self._labels_of_binary(u, u), c_dims, c_dims[-1])
        iy = self._labels_of_step(self._labels_of_binary(v, v), c_dims, c_dims[-2])
        return self._labels_of_binary(ix, iy)  # (the scaling by 0.5 changes neither coords nor name)

    def kinetic_energy(self, u, v, x_axis: str = "X", y_axis: str = "Y", padding=None, fill_value=None):
        """Kinetic energy of a C-grid velocity at the cell centre in ONE pass: u and v are read once, the result written
        once (24 B/cell in float64 instead of about 120 for the six launches of the chain).

        u at (Y:center, X:left), v at (Y:left, X:center).  Bit-identical, coords and name included, to the chain

            kw = dict(padding=padding, fill_value=fill_value)
            ke = 0.5 * (grid.interp(u * u, x_axis, **kw) + grid.interp(v * v, y_axis, **kw))

        Both interpolations go left -> center, so each SQUARE is padded right of / above the last cell (periodic: the
        square at index 0, extend: at n-1, fill: `fill_value` itself, not its square).  That chain itself runs (the same
        calls in the same order) for integer, float16 or mixed dtypes, for (Y, X) not last or fields of different shapes,
        for chunked host arrays, and on grids with face connections or a fold along either axis."""
        args = (u, v)
        (u, xr1), (v, xr2) = self._wrap_in(u), self._wrap_in(v)
        was_xr = xr1 or xr2
        lead, u_dims, v_dims, c_dims, z_dims = self._c_grid_vector(u, v, x_axis, y_axis, "kinetic energy")
        plan = None
        if u.dims == u_dims and v.dims == v_dims:
            plan = self._second_order_plan([u, v], x_axis, y_axis, padding, fill_value)
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            return 0.5 * (self.interp(args[0] * args[0], x_axis, **kw) + self.interp(args[1] * args[1], y_axis, **kw))
        bcx, bcy, fvx, fvy = plan
        host = not (_is_tensor(u.data) or _is_tensor(v.data))
        out = _dev.kinetic_energy(u.data, v.data, bcx, bcy, fvx, fvy)
        res = self._labels_of_ke(u, v, c_dims)._replace(data=_dev.tohost(out) if host else out)
        return to_xarray(res) if was_xr else res

    def momentum_advection(self, u, v, coriolis=None, x_axis: str = "X", y_axis: str = "Y", padding=None, fill_value=None,
                           metric_weighted: bool = True):
        """Vector-invariant horizontal momentum advection, plus the Coriolis term when `coriolis` (f at the vorticity
        point, (Y:left, X:left)) is given, in ONE pass: u and v are read once and the two tendencies written once (32 B/cell
        in float64 instead of about 400 for the twenty launches of the chain).  Returns `(gu, gv)`, gu at u's points,
        gv at v's.

        What is computed: the chain below, in which `zeta` is `grid.vorticity` of the RAW u and v -- their curl in index
        space over the area, (delta_x v - delta_y u) / rAz -- not the relative vorticity, which by `vorticity`'s own
        convention needs the circulations u * dxC, v * dyC; the same u and v serve as velocities in ke, ubar and vbar.
        With `metric_weighted` the result is the continuous term ((zeta + f) v - d/dx KE, -(zeta + f) u - d/dy KE) only on
        a grid of unit spacing (dxC = dyC = 1, rAz = 1).  On a uniform grid of spacing h it is (zeta / h + f) v - d/dx KE;
        with `metric_weighted=False` and no `coriolis` it is h times the term.  On a stretched grid it is neither.
        `tests/test_convergence.py` measures this (a strict expected failure against the continuous term).

        u at (Y:center, X:left), v at (Y:left, X:center).  Bit-identical, coords and names included, to the chain

            kw = dict(padding=padding, fill_value=fill_value)
            zeta = grid.vorticity(u, v, x_axis, y_axis, metric_weighted=metric_weighted, **kw)   # (Y:left, X:left)
            if coriolis is not None:
                zeta = zeta + coriolis
            ke = 0.5 * (grid.interp(u * u, x_axis, **kw) + grid.interp(v * v, y_axis, **kw))     # centre
            vbar = grid.interp(grid.interp(v, x_axis, **kw), y_axis, **kw)                       # v at u's points
            ubar = grid.interp(grid.interp(u, y_axis, **kw), x_axis, **kw)                       # u at v's points
            gx, gy = grid.gradient(ke, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
            gu = grid.interp(zeta, y_axis, **kw) * vbar - gx
            gv = -(grid.interp(zeta, x_axis, **kw) * ubar) - gy

        Every stage pads with its axis's own boundary and fill value on the side the chain pads it: u below and v left of
        the first cell (vorticity and the first means), zeta and those means above / right of the last one, the squares
        above / right, ke below / left -- periodic: the stage's own value at the wrapped index, extend: at the clamped
        index, fill: `fill_value` itself (a filled zeta is `fill_value`, not `fill_value + coriolis`).  With
        `metric_weighted` zeta is divided by the (X, Y) metric at the vorticity point and the gradient by the X / Y
        metrics at u's / v's points.  That chain itself runs (the same calls in the same order) for integer, float16 or
        mixed dtypes (`coriolis` and the metrics included), for (Y, X) not last or fields of different shapes, for a
        `coriolis` or a metric with dims the result lacks, for chunked host arrays, and on grids with face connections or
        a fold along either axis."""
        args = (u, v, coriolis)
        (u, xr1), (v, xr2), (cor, xr3) = self._wrap_in(u), self._wrap_in(v), self._wrap_in(coriolis)
        was_xr = xr1 or xr2 or xr3
        lead, u_dims, v_dims, c_dims, z_dims = self._c_grid_vector(u, v, x_axis, y_axis, "momentum advection")
        plan = None
        mets = {}
        if u.dims == u_dims and v.dims == v_dims and (cor is None or isinstance(cor, DataArray)):
            try:
                if metric_weighted:
                    for key, dims, axes in (("rAz", z_dims, (x_axis, y_axis)), ("dxC", u_dims, (x_axis,)),
                                            ("dyC", v_dims, (y_axis,))):
                        mets[key] = (self._resident(self.get_metric(_DimsOnly(dims), axes), u.data), dims)
            except (KeyError, ValueError):
                mets = None  # (the chain raises it where the chain looks the metric up)
            if mets is not None:
                if cor is not None:
                    mets["coriolis"] = (self._resident(cor, u.data), z_dims)
                if all(set(m.dims) <= set(dims) and not _is_chunked(m.data) for m, dims in mets.values()):
                    plan = self._second_order_plan([u, v], x_axis, y_axis, padding, fill_value, [m for m, _ in mets.values()])
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            u, v, coriolis = args
            zeta = self.vorticity(u, v, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
            if coriolis is not None:
                zeta = zeta + coriolis
            ke = 0.5 * (self.interp(u * u, x_axis, **kw) + self.interp(v * v, y_axis, **kw))
            vbar = self.interp(self.interp(v, x_axis, **kw), y_axis, **kw)
            ubar = self.interp(self.interp(u, y_axis, **kw), x_axis, **kw)
            gx, gy = self.gradient(ke, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
            gu = self.interp(zeta, y_axis, **kw) * vbar - gx
            gv = -(self.interp(zeta, x_axis, **kw) * ubar) - gy
            return gu, gv
        bcx, bcy, fvx, fvy = plan
        host = not (_is_tensor(u.data) or _is_tensor(v.data))
        views = {k: _aligned_view(m, dims) for k, (m, dims) in mets.items()}
        ou, ov = _dev.momentum_advection(u.data, v.data, views.get("coriolis"), views.get("rAz"), views.get("dxC"),
                                         views.get("dyC"), bcx, bcy, fvx, fvy)
        # dims, coords and names as the chain's, step by step over placeholders
        xl, yl, xc, yc = u_dims[-1], v_dims[-2], v_dims[-1], u_dims[-2]
        zeta = _reattach_coords([DataArray(_placeholder(u.shape), z_dims)], self, None, {xl, yl}, [u, v])[0]
        if cor is not None:
            zeta = self._labels_of_binary(zeta, mets["coriolis"][0])
        ke = self._labels_of_ke(u, v, c_dims)
        vbar = self._labels_of_step(self._labels_of_step(v, z_dims, xl), u_dims, yc)
        ubar = self._labels_of_step(self._labels_of_step(u, z_dims, yl), v_dims, xc)
        gx, gy = self._labels_of_step(ke, u_dims, xl), self._labels_of_step(ke, v_dims, yl)
        gu = self._labels_of_binary(self._labels_of_binary(self._labels_of_step(zeta, u_dims, yc), vbar), gx)
        gv = self._labels_of_binary(self._labels_of_binary(self._labels_of_step(zeta, v_dims, xc), ubar), gy)
        gu = gu._replace(data=_dev.tohost(ou) if host else ou)
        gv = gv._replace(data=_dev.tohost(ov) if host else ov)
        return (to_xarray(gu), to_xarray(gv)) if was_xr else (gu, gv)

    def horizontal_viscosity(self, u, v, viscosity_d=None, viscosity_z=None, x_axis: str = "X", y_axis: str = "Y",
                             padding=None, fill_value=None, metric_weighted: bool = True):
        """Vector-invariant harmonic viscosity in the form of MITgcm's mom_vi_hdissip (harmonic part), d/dx(D) - d/dy(zeta)
        at u's points and d/dy(D) + d/dx(zeta) at v's, in ONE pass: u and v are read once and the two tendencies written
        once (32 B/cell in float64, against about 150-200 for the seven to nine launches of the chain).  Returns
        `(gu, gv)`, gu at u's points, gv at v's.

        What is computed: the chain below, in which D and zeta are `grid.divergence` and `grid.vorticity` of the RAW u and
        v -- their divergence and curl in index space over the area, (delta_x u + delta_y v) / rA and
        (delta_x v - delta_y u) / rAz -- not the horizontal divergence and the relative vorticity, which by those
        operators' own convention need the transports u * dyG, v * dxG and the circulations u * dxC, v * dyC.  With
        `metric_weighted` the result is the continuous term (del2 u, del2 v for constant coefficients) only on a grid of
        unit spacing; on a uniform grid of spacing h it is the term over h, and with `metric_weighted=False` h^2 times the
        term.  On a stretched grid it is neither.  `tests/test_convergence.py` measures this (a strict expected failure
        against the continuous term).

        u at (Y:center, X:left), v at (Y:left, X:center).  `viscosity_d` is a coefficient at the cell centre, where D
        lives, `viscosity_z` one at the vorticity point (Y:left, X:left) -- the Smagorinsky / Leith form; each may have any
        subset of its stage's dims (a full (lead, Y, X) field included).  A scalar viscosity is the caller's product of the
        result, and `grid.horizontal_viscosity(*grid.horizontal_viscosity(u, v))` is the biharmonic operator.
        Bit-identical, dims, coords and names included, to the chain

            kw = dict(padding=padding, fill_value=fill_value)
            div  = grid.divergence(u, v, x_axis, y_axis, metric_weighted=metric_weighted, **kw)   # centre
            zeta = grid.vorticity(u, v, x_axis, y_axis, metric_weighted=metric_weighted, **kw)    # (Y:left, X:left)
            if viscosity_d is not None: div  = div * viscosity_d
            if viscosity_z is not None: zeta = zeta * viscosity_z
            dx, dy = grid.gradient(div, x_axis, y_axis, metric_weighted=metric_weighted, **kw)    # centre -> left, at u's / v's points
            op = grid.derivative if metric_weighted else grid.diff
            zy = op(zeta, y_axis, **kw)                                                           # left -> centre along Y: at u's points
            zx = op(zeta, x_axis, **kw)                                                           # left -> centre along X: at v's points
            gu = dx - zy
            gv = dy + zx

        Pads: every stage pads with its axis's own boundary on the side the chain pads it -- u right of the last column
        and v above the last row (D), v left of the first column and u below the first row (zeta), the PRODUCT D * nu_d
        left of the first column and below the first row, the PRODUCT zeta * nu_z above the last row and right of the last
        column.  Periodic: the stage's own value at the wrapped index; extend: at the clamped index; fill: `fill_value`
        itself, never a quotient or a product formed from it.

        Signed zeros: every operator of the chain hands a -0.0 fill value on as it is, and so does the one pass (the
        kernel takes a fill pair of its own for the pads of zeta * nu_z: the same values), which leaves the chain's bit
        patterns.

        Metrics: with `metric_weighted`, whatever `get_metric` returns at each stage's dims -- the (X, Y) metric at the
        centre and at the vorticity point, the X metric at u's and the Y metric at v's points (the gradient), the Y metric
        at u's and the X metric at v's points (the differences of zeta); the kernel takes all six or none.

        The chain itself runs (the same calls in the same order) for integer, float16 or mixed dtypes (coefficients and
        metrics included), for (Y, X) not last or fields of different shapes, for chunked inputs, coefficients or metrics,
        for a coefficient or metric with dims its stage lacks, for exactly one of the two coefficients, for a metric
        lookup that raises (the chain raises it), for a missing boundary on either axis (the chain raises), on grids with
        face connections or a fold along either axis, and for anything else `_second_order_plan` declines."""
        args = (u, v, viscosity_d, viscosity_z)
        (u, xr1), (v, xr2), (nud, xr3), (nuz, xr4) = (self._wrap_in(a) for a in args)
        was_xr = xr1 or xr2 or xr3 or xr4
        lead, u_dims, v_dims, c_dims, z_dims = self._c_grid_vector(u, v, x_axis, y_axis, "horizontal viscosity")
        plan = None
        mets = {}
        if (u.dims == u_dims and v.dims == v_dims and (nud is None) == (nuz is None)
                and (nud is None or (isinstance(nud, DataArray) and isinstance(nuz, DataArray)))):
            try:
                if metric_weighted:
                    for key, dims, axes, layout in (("rA", c_dims, (x_axis, y_axis), None), ("rAz", z_dims, (x_axis, y_axis), None),
                                                    ("dxC", u_dims, (x_axis,), None), ("dyC", v_dims, (y_axis,), None),
                                                    ("dyG", u_dims, (y_axis,), u_dims), ("dxG", v_dims, (x_axis,), v_dims)):
                        mets[key] = (self._resident(self.get_metric(_DimsOnly(dims), axes, _layout=layout), u.data), dims)
            except (KeyError, ValueError):
                mets = None  # (the chain raises it where the chain looks the metric up)
            if mets is not None:
                if nud is not None:
                    mets["nu_d"] = (self._resident(nud, u.data), c_dims)
                    mets["nu_z"] = (self._resident(nuz, u.data), z_dims)
                if all(set(m.dims) <= set(dims) and not _is_chunked(m.data) for m, dims in mets.values()):
                    plan = self._second_order_plan([u, v], x_axis, y_axis, padding, fill_value, [m for m, _ in mets.values()])
        if plan is None:
            kw = dict(padding=padding, fill_value=fill_value)
            u, v, viscosity_d, viscosity_z = args
            div = self.divergence(u, v, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
            zeta = self.vorticity(u, v, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
            if viscosity_d is not None:
                div = div * viscosity_d
            if viscosity_z is not None:
                zeta = zeta * viscosity_z
            dx, dy = self.gradient(div, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
            op = self.derivative if metric_weighted else self.diff
            zy = op(zeta, y_axis, **kw)
            zx = op(zeta, x_axis, **kw)
            gu = dx - zy
            gv = dy + zx
            return gu, gv
        bcx, bcy, fvx, fvy = plan
        # the fill of the last stage's one-axis operators (None: 0.0); the same values as the plan's, a -0.0 included
        fval = self._complete_user_kwargs_using_axis_defaults(fill_value, "fill_value")
        zfx, zfy = (0.0 if fval[ax] is None else float(fval[ax]) for ax in (x_axis, y_axis))
        host = not (_is_tensor(u.data) or _is_tensor(v.data))
        views = {k: _aligned_view(m, dims) for k, (m, dims) in mets.items()}
        ou, ov = _dev.horizontal_viscosity(u.data, v.data, *(views.get(k) for k in ("rA", "rAz", "dxC", "dyC", "dyG", "dxG",
                                                                                     "nu_d", "nu_z")),
                                           bcx, bcy, fvx, fvy, zfx, zfy)
        # dims, coords and names as the chain's, step by step over placeholders
        xl, yl, xc, yc = u_dims[-1], v_dims[-2], v_dims[-1], u_dims[-2]
        div = _reattach_coords([DataArray(_placeholder(u.shape), c_dims)], self, None, {xc, yc}, [u, v])[0]
        zeta = _reattach_coords([DataArray(_placeholder(u.shape), z_dims)], self, None, {xl, yl}, [u, v])[0]
        if nud is not None:
            div = self._labels_of_binary(div, mets["nu_d"][0])
            zeta = self._labels_of_binary(zeta, mets["nu_z"][0])
        dx, dy = self._labels_of_step(div, u_dims, xl), self._labels_of_step(div, v_dims, yl)
        zy, zx = self._labels_of_step(zeta, u_dims, yc), self._labels_of_step(zeta, v_dims, xc)
        if metric_weighted and zeta.name is not None:  # (`derivative` names its quotient, `gradient` does not)
            zy = zy._replace(name=_name_after(zeta.name, mets["dyG"][0]))
            zx = zx._replace(name=_name_after(zeta.name, mets["dxG"][0]))
        gu = self._labels_of_binary(dx, zy)._replace(data=_dev.tohost(ou) if host else ou)
        gv = self._labels_of_binary(dy, zx)._replace(data=_dev.tohost(ov) if host else ov)
        return (to_xarray(gu), to_xarray(gv)) if was_xr else (gu, gv)

    def transform(self, da, axis, target, **kwargs):
        """Convert `da` to new 1-D coordinates along `axis` (linear / log / conservative; reference
        grid.py:1687-1777 -> transform.py:284-514), one HIP kernel launch per call."""
        from .transform import transform as _transform

        return _transform(self, axis, da, target, **kwargs)


# ----------------------------------------------------------------------------------------------
def _implicit_vertical_diffusion_levels(a, kappa, mf, mc, z: int, dt: float):
    """`Grid.implicit_vertical_diffusion` as a loop over levels: every operation on whole planes, in the arrays' own
    arithmetic (numpy arrays or tensors, all of one dtype), in the order of the docstring there -- so bit for bit what the
    one-pass kernel computes.  The operands have the same number of dims and broadcast against each other, Z is dim `z` in
    all of them; `kappa` and `mf` are indexed by face (an extent of 1 along Z: the same plane at every face), `mc` by level.
    Some twelve plane-sized operations per level in the forward loop and two in the backward one."""
    present = [m for m in (a, kappa, mf, mc) if m is not None]
    n = a.shape[z]
    shape = list(np.broadcast_shapes(*[tuple(m.shape[:z]) + (1,) + tuple(m.shape[z + 1:]) for m in present]))
    shape[z] = n
    if _is_tensor(a):
        out, c = (a.new_empty(shape) for _ in range(2))
        one, tdt = a.new_tensor(1.0), a.new_tensor(dt)   # dt is cast to the dtype once
    else:
        out, c = (np.empty(shape, a.dtype) for _ in range(2))
        one, tdt = a.dtype.type(1.0), a.dtype.type(dt)
    ix = lambda m, k: (slice(None),) * z + (k if m.shape[z] > 1 else 0,)  # noqa: E731
    at = lambda m, k: m[ix(m, k)]  # noqa: E731

    def weight(k):   # dt * kappa / mf at face k
        g = one if kappa is None else at(kappa, k)
        if mf is not None:
            g = g / at(mf, k)
        return tdt * g

    w = cp = dp = None
    for k in range(n):
        b = one
        if k > 0:
            lo = w if mc is None else w / at(mc, k)
            b = b + lo
        if k < n - 1:
            w = weight(k + 1)
            up = w if mc is None else w / at(mc, k)
            b = b + up
        m = b if k == 0 else b - lo * cp
        r = one / m
        if k < n - 1:
            cp = up * r
            c[ix(c, k)] = cp
        dp = (at(a, k) if k == 0 else at(a, k) + lo * dp) * r
        out[ix(out, k)] = dp
    for k in range(n - 2, -1, -1):
        out[ix(out, k)] = at(out, k) + at(c, k) * at(out, k + 1)
    return out


def _weak_scalar(s, data) -> bool:
    """is `s` a scalar that `DataArray._binary` casts to the dtype of `data` -- a Python int or float, or a numpy floating
    scalar that does not promote it -- and whose cast through a C double is that cast?"""
    if isinstance(s, np.floating):   # (np.float64 is a Python float too, and strong)
        return np.result_type(_dt.np_dtype(data), s) == _dt.np_dtype(data)
    if isinstance(s, bool) or not isinstance(s, (int, float)):
        return False
    return isinstance(s, float) or abs(s) <= 2 ** 53   # (a larger int: double rounding on the way to float32)


def _placeholder(shape):
    """read-only stand-in of an intermediate the fused operators never form: carries a shape (for its coords), no memory"""
    return np.broadcast_to(np.zeros((), dtype=np.int8), tuple(int(n) for n in shape))

# ----------------------------------------------------------------------------------------------
def _shifted_dims(grid: Grid, array, ax_name: str, to_pos: str, from_pos: Optional[str] = None) -> Tuple[str, ...]:
    """dims of the result of moving `array` to `to_pos` along `ax_name` (input order kept).  `from_pos`: the position
    the step's signature names -- fixed from the ORIGINAL array before the first axis (xgcm/grid.py:790-794), so a later
    axis is not looked up again on an array a metric product may have given a second dim of that axis"""
    dim = grid.axes[ax_name].coords.get(from_pos) if from_pos is not None else None
    if dim is None or dim not in array.dims:
        _, dim = grid.axes[ax_name]._get_position_name(array)
    new = grid.axes[ax_name].coords.get(to_pos, dim)
    return tuple(new if d == dim else d for d in array.dims)


def _cumsum_trim_pad(pos: str, to: str, reverse: bool, ax) -> Tuple[int, int, int, int]:
    """(trim_lo, trim_hi, pad_lo, pad_hi) of the reference's table (grid.py:1326-1383)."""
    pair = (pos, to)
    natural = (("center", "right"), ("left", "center"))
    shifted = (("center", "left"), ("right", "center"))
    shrink = (("center", "inner"), ("outer", "center"))
    grow = (("center", "outer"), ("inner", "center"))
    if not reverse:
        table = {natural: (0, 0, 0, 0), shifted: (0, 1, 1, 0), shrink: (0, 1, 0, 0), grow: (0, 0, 1, 0)}
    else:
        table = {shifted: (0, 0, 0, 0), natural: (1, 0, 0, 1), shrink: (1, 0, 0, 0), grow: (0, 0, 0, 1)}
    for pairs, widths in table.items():
        if pair in pairs:
            return widths
    raise ValueError(f"From `{pos}` to `{to}` is not a valid position shift for cumsum operation along axis {ax}.")


def _ones_like(data):
    if _is_tensor(data):
        return _dev.synthetic(tuple(data.shape), 0, 0, 0.0, 1.0)
    return np.ones(data.shape)


def _valid_mask(da: DataArray) -> DataArray:
    """1.0 where `da` is not NaN else 0.0, computed on the GPU as (da - da) == 0 -> via min/max-free arithmetic."""
    # x - x is 0 for finite x and NaN for NaN/inf; nan-skipping sum of (x - x + 1) over a length-1 axis gives the mask
    if gridops.is_integer_data(da.data):  # integers and bool hold no NaN (and numpy refuses `bool - bool`)
        return da._replace(data=_ones_like(da.data), coords=OrderedDict(), name=None)
    z = da - da
    one = z + 1.0
    host = not _is_tensor(one.data)
    data = _dev.asdevice(one.data)
    mask = _dev.reduce1d(data[None], 0, None, True)
    return DataArray(_dev.tohost(mask) if host else mask, da.dims)


_SELECT_CACHE: Dict[Tuple[str, Tuple], Any] = {}


def _select_grid_ufunc(funcname, signature: _GridUFuncSignature, module, **kwargs):
    """The one GridUFunc of `module` whose name starts with `funcname` and whose signature is
    equivalent to `signature` (reference grid.py:1779-1824).  Lookups in the built-in `gridops`
    namespace (fixed at import) are memoised: the scan costs ~65 us, a kernel on a small array less."""
    builtin = module is gridops
    key = (funcname, signature._canonical())
    if builtin and key in _SELECT_CACHE:
        return _SELECT_CACHE[key], kwargs
    # (members through getattr, so that a class used as a namespace -- staticmethods -- works like a module)
    named = [f for name, f in inspect.getmembers(module, lambda o: isinstance(o, GridUFunc)) if name.startswith(funcname)]
    if not named:
        raise NotImplementedError(f"Could not find any pre-defined {funcname} grid ufuncs")
    matching = [f for f in named if f.signature.equivalent(signature)]
    if not matching:
        raise NotImplementedError(f"Could not find any pre-defined {funcname} grid ufuncs with signature {signature}")
    if len(matching) > 1:
        raise ValueError(
            f"Function {funcname} with signature='{signature}' and kwargs={kwargs.copy()} is an ambiguous selection"
        )
    if builtin:
        _SELECT_CACHE[key] = matching[0]
    return matching[0], kwargs
