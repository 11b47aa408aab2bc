"""The learned sibling plan of `xgcm_amd.device`: repeated rounds of plain two-point operators on one kind
of field are served from ONE pass over it (xg_stencil_multi).  On the host build of the ABI, with `device.SIBLING_STATS`; the
same scenarios once on the GPU at 3 x 9 x 130."""

import gc
import threading

import numpy as np
import pytest

import stencil_multi_cases as MC

torch = pytest.importorskip("torch")

A, B, C, E = (("interp", 2, 1, 0, "periodic", 0.0), ("diff", 2, 1, 0, "periodic", 0.0), ("interp", 1, 1, 0, "extend", 0.0),
              ("diff", 1, 1, 0, "extend", 0.0))
ROUND = (A, B, C, E)
OTHER = ("min", 2, 1, 0, "periodic", 0.0)
SHAPE = (3, 9, 130)


def _call(D, x, req):
    return D.stencil1d(req[0], x, *req[1:])


def _single(D, x, req):
    with D.sibling_plans_off():
        return D.tohost(_call(D, x, req))


def _fresh(D):
    D.drop_sibling_plans()
    D.SIBLING_STATS.reset()
    return D.SIBLING_STATS


def _field(D, k=0, dtype=np.float64):
    a = MC.field(SHAPE, dtype, seed=5 + k)
    return a, D.asdevice(a.copy())  # (on the host build a tensor shares its array's memory)


def _live(D, x, rounds=2, reqs=ROUND):
    """`rounds` equal rounds on x: the plan is live afterwards (the next first request is served by one pass)"""
    for _ in range(rounds):
        for r in reqs:
            _call(D, x, r)


def scenario_third_round_is_one_launch(D):
    st = _fresh(D)
    a, x = _field(D)
    want = {r: _single(D, x, r) for r in ROUND}
    got = [[D.tohost(_call(D, x, r)) for r in ROUND] for _ in range(3)]
    assert st.as_dict() == {"launches": 1, "served": 3, "dropped": 0, "retired": 0}
    for rnd in got:
        for r, g in zip(ROUND, rnd):
            assert MC.same_bits(g, want[r]) and MC.same_bits(g, MC.oracle(a, r)), r
    # ... and in any order after the round's first request
    outs = {r: D.tohost(_call(D, x, r)) for r in (A, E, C, B)}
    assert st.as_dict() == {"launches": 2, "served": 6, "dropped": 0, "retired": 0}
    assert all(MC.same_bits(outs[r], want[r]) for r in ROUND)


def scenario_new_tensor_every_round(D):
    st = _fresh(D)
    for k in range(5):
        a, x = _field(D, k)
        for r in ROUND:
            assert MC.same_bits(D.tohost(_call(D, x, r)), MC.oracle(a, r)), (k, r)
        del x
    assert st.as_dict() == {"launches": 3, "served": 9, "dropped": 0, "retired": 0}


def scenario_new_values_in_mid_round(D):
    st = _fresh(D)
    a, x = _field(D)
    _live(D, x)
    first = D.tohost(_call(D, x, A))
    assert st["launches"] == 1 and MC.same_bits(first, MC.oracle(a, A))
    x.add_(1)
    got = D.tohost(_call(D, x, B))
    assert MC.same_bits(got, MC.oracle(a + 1, B))
    assert st.as_dict() == {"launches": 1, "served": 0, "dropped": 3, "retired": 1}
    _call(D, x, C), _call(D, x, E)
    # learning starts over, from the request that met the change: rounds now run B C E A, and the third B is one pass again
    _live(D, x)
    assert MC.same_bits(D.tohost(_call(D, x, A)), MC.oracle(a + 1, A))
    assert st.as_dict() == {"launches": 2, "served": 3, "dropped": 3, "retired": 1}


def scenario_another_tensor_in_mid_round(D):
    st = _fresh(D)
    a, x = _field(D)
    b, y = _field(D, 1)
    _live(D, x)
    _call(D, x, A)
    assert st["launches"] == 1
    got = D.tohost(_call(D, y, B))
    assert MC.same_bits(got, MC.oracle(b, B)) and not MC.same_bits(got, MC.oracle(a, B))
    assert st.as_dict() == {"launches": 1, "served": 0, "dropped": 3, "retired": 1}


def scenario_request_outside_the_set(D):
    st = _fresh(D)
    a, x = _field(D)
    _live(D, x)
    _call(D, x, A)
    assert MC.same_bits(D.tohost(_call(D, x, OTHER)), MC.oracle(a, OTHER))
    assert st.as_dict() == {"launches": 1, "served": 0, "dropped": 3, "retired": 1}
    # with nothing held (the round was served completely) an outsider retires the plan too
    st = _fresh(D)
    _live(D, x, 3)
    assert st.as_dict() == {"launches": 1, "served": 3, "dropped": 0, "retired": 0}
    _call(D, x, OTHER)
    assert st["retired"] == 1
    _call(D, x, A)
    assert st["launches"] == 1


def scenario_one_operator_twice(D):
    st = _fresh(D)
    a, x = _field(D)
    for _ in range(5):
        for r in (A, B, B):
            assert MC.same_bits(D.tohost(_call(D, x, r)), MC.oracle(a, r))
    _live(D, x, 5, reqs=(A,))  # a single request is never a plan either
    assert st.as_dict() == {"launches": 0, "served": 0, "dropped": 0, "retired": 0}


def scenario_two_fields_taking_turns(D):
    """(diff(v, X) - diff(u, Y)) step after step: one kind of input, two tensors -- a round is what is asked of ONE tensor"""
    st = _fresh(D)
    a, u = _field(D)
    b, v = _field(D, 1)
    for _ in range(6):
        assert MC.same_bits(D.tohost(_call(D, v, B)), MC.oracle(b, B))
        assert MC.same_bits(D.tohost(_call(D, u, E)), MC.oracle(a, E))
    for _ in range(6):  # ... nor do whole rounds whose requests change tensor half way
        _call(D, v, A), _call(D, v, B), _call(D, u, C), _call(D, u, E)
    assert st.as_dict() == {"launches": 0, "served": 0, "dropped": 0, "retired": 0}


def scenario_input_dies(D):
    st = _fresh(D)
    a, x = _field(D)
    _live(D, x)
    _call(D, x, A)
    held = [s for s in D._sib_table().values() if s.held]
    assert len(held) == 1 and len(held[0].held) == 3 and st["launches"] == 1
    del x
    gc.collect()
    assert not any(s.held for s in D._sib_table().values()) and st["dropped"] == 3
    b, y = _field(D, 1)  # (may land at the same address)
    assert MC.same_bits(D.tohost(_call(D, y, B)), MC.oracle(b, B)) and st["served"] == 0


def scenario_byte_bound(D, monkeypatch):
    st = _fresh(D)
    a, x = _field(D)
    each = x.numel() * x.element_size()
    monkeypatch.setattr(D, "_free_bytes", lambda: 4 * 3 * each)  # a quarter of it: exactly what would be held -- not under it
    _live(D, x, 3)
    assert st["launches"] == 0 and not any(s.held for s in D._sib_table().values())
    monkeypatch.setattr(D, "_free_bytes", lambda: 4 * 3 * each + 4)
    assert MC.same_bits(D.tohost(_call(D, x, A)), MC.oracle(a, A)) and st["launches"] == 1
    assert sum(s.held_bytes() for s in D._sib_table().values()) == 3 * each < D._free_bytes() // 4


def scenario_written_through_the_library(D):
    """`_version` does not see a write through the address; the library's own in-place writers drop what is held"""
    st = _fresh(D)
    a, x = _field(D)
    _live(D, x)
    _call(D, x, A)
    assert st["launches"] == 1 and any(s.held for s in D._sib_table().values())
    version = x._version
    D.synthetic(SHAPE, 9, out=x)
    assert x._version == version and not any(s.held for s in D._sib_table().values())
    assert MC.same_bits(D.tohost(_call(D, x, B)), MC.oracle(D.tohost(x), B))
    assert st.as_dict() == {"launches": 1, "served": 0, "dropped": 3, "retired": 1}
    _call(D, x, C), _call(D, x, E)
    _live(D, x)
    assert st["launches"] == 2 and any(s.held for s in D._sib_table().values())
    b, y = _field(D, 1)
    D.copy_into(x, y)
    assert not any(s.held for s in D._sib_table().values())
    assert st.as_dict() == {"launches": 2, "served": 2, "dropped": 4, "retired": 2}  # (rounds now run B C E A: A was still held)


def scenario_the_input_is_freed_by_another_thread(D):
    """the weak-reference callback runs on the thread that frees the input: it counts on the OWNER's counters"""
    st = _fresh(D)
    box = [_field(D)[1]]
    _live(D, box[0])
    _call(D, box[0], A)
    seen = {}

    def other():
        box.pop()
        gc.collect()
        seen["stats"] = D.SIBLING_STATS.as_dict()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["stats"] == {"launches": 0, "served": 0, "dropped": 0, "retired": 0}
    assert st.as_dict() == {"launches": 1, "served": 0, "dropped": 3, "retired": 0} and not any(s.held for s in D._sib_table().values())


SCENARIOS = [scenario_third_round_is_one_launch, scenario_new_tensor_every_round, scenario_new_values_in_mid_round,
             scenario_another_tensor_in_mid_round, scenario_request_outside_the_set, scenario_one_operator_twice,
             scenario_two_fields_taking_turns, scenario_input_dies, scenario_written_through_the_library,
             scenario_the_input_is_freed_by_another_thread]


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[9:])
def test_plan(host_abi, scenario):
    from xgcm_amd import device as D

    try:
        scenario(D)
    finally:
        D.drop_sibling_plans()


def test_byte_bound(host_abi, monkeypatch):
    from xgcm_amd import device as D

    try:
        scenario_byte_bound(D, monkeypatch)
    finally:
        D.drop_sibling_plans()


def test_a_decline_of_the_native_entry_is_served_singly(host_abi, monkeypatch):
    from xgcm_amd import device as D

    st = _fresh(D)
    try:
        a, x = _field(D)
        asked = []
        monkeypatch.setattr(D, "_multi_launch", lambda t, reqs: asked.append(len(reqs)))  # (returns None: declined)
        got = [[D.tohost(_call(D, x, r)) for r in ROUND] for _ in range(5)]
        assert asked == [4] and st.as_dict() == {"launches": 0, "served": 0, "dropped": 0, "retired": 0}  # asked once, not again
        assert all(MC.same_bits(g, MC.oracle(a, r)) for rnd in got for r, g in zip(ROUND, rnd))
    finally:
        D.drop_sibling_plans()


class _Claimed:
    """what `_sibling_form` looks at, of a tensor too large to make"""

    def __init__(self, shape, itemsize=8, ptr=4096):
        self.shape, self._item, self._ptr = tuple(shape), itemsize, ptr

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for v in self.shape:
            n *= v
        return n

    def element_size(self):
        return self._item

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self._ptr


def test_only_forms_the_native_entry_takes_are_requests():
    from xgcm_amd import device as D

    ok = lambda shape, axis=2, pads=(1, 0), bc="periodic", **kw: D._sibling_form(_Claimed(shape, **kw), axis, *pads, bc)  # noqa: E731
    assert ok((3, 9, 130)) and ok((3, 9, 130), axis=1) and ok((9, 130), axis=0) and ok((9, 130), axis=1)
    assert ok((1, 65536, 32768 - 2)) and ok((1, 1, 2 ** 31 - 2)) and D.SIBLING_MAX_CELLS == 2 ** 31 - 1
    assert not ok((1, 65536, 32768)) and not ok((1, 1, 2 ** 31)) and not ok((3, 46341, 46344)) and not ok((2 ** 31, 8), axis=1)
    assert not ok((3, 9, 130), axis=0) and not ok((2, 3, 9, 130), axis=3) and not ok((130,), axis=0) and not ok((0, 9, 130))
    assert not ok((3, 9, 130), pads=(1, 1)) and not ok((3, 9, 130), pads=(0, 0)) and not ok((3, 9, 130), bc=None)
    assert not ok((3, 9, 131)) and not ok((3, 9, 130), itemsize=4) and ok((3, 9, 132), itemsize=4) and not ok((3, 9, 130), ptr=4104)


def test_float32_and_key_eviction(host_abi):
    from xgcm_amd import device as D

    st = _fresh(D)
    try:
        a = MC.field((3, 9, 132), np.float32)
        x = D.asdevice(a)
        got = [[D.tohost(_call(D, x, r)) for r in ROUND] for _ in range(3)]
        assert st.as_dict() == {"launches": 1, "served": 3, "dropped": 0, "retired": 0}
        assert all(MC.same_bits(g, MC.oracle(a, r)) for r, g in zip(ROUND, got[2]))
        # rows the native entry would decline are no requests at all: nothing is learnt from them
        odd = D.asdevice(MC.field((3, 9, 130), np.float32))
        _live(D, odd, 4)
        assert st["launches"] == 1 and len(D._sib_table()) == 1
        # the ninth kind of input evicts the least recently used one, and what it held
        _call(D, x, A)
        assert st["launches"] == 2 and any(s.held for s in D._sib_table().values())
        for k in range(D.SIBLING_MAX_KEYS):
            _call(D, D.asdevice(np.zeros((2, 4 + k, 8), np.float32)), A)
        assert len(D._sib_table()) == D.SIBLING_MAX_KEYS and not any(s.held for s in D._sib_table().values())
        assert st["dropped"] == 3 and st["retired"] == 1
    finally:
        D.drop_sibling_plans()


def _grid(D, fuse=False):
    from xgcm_amd import DataArray, Dataset, Grid

    nz, ny, nx = SHAPE
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0), "YC": ("YC", np.arange(ny) + 0.5),
              "YG": ("YG", np.arange(ny) * 1.0), "Z": ("Z", np.arange(nz) * 1.0)}
    grid = Grid(Dataset(coords=coords), coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}, "Z": {"center": "Z"}},
                padding={"X": "periodic", "Y": "extend"}, autoparse_metadata=False, fuse=fuse)
    a, x = _field(D)
    return grid, DataArray(x, ("Z", "YC", "XC"), name="T"), a


def _grid_round(D, grid, T):
    return [D.tohost(getattr(grid, fn)(T, ax).data) for fn, ax in (("interp", "X"), ("diff", "X"), ("interp", "Y"), ("diff", "Y"))]


def test_off_switches(host_abi, monkeypatch):
    from xgcm_amd import device as D

    try:
        # through the Grid, eagerly: the plan serves the third round
        st = _fresh(D)
        grid, T, a = _grid(D)
        for _ in range(3):
            got = _grid_round(D, grid, T)
        assert st.as_dict() == {"launches": 1, "served": 3, "dropped": 0, "retired": 0}
        assert all(MC.same_bits(g, MC.oracle(a, r)) for r, g in zip(ROUND, got))
        # XG_SIBLING_PLAN=0
        st = _fresh(D)
        monkeypatch.setenv("XG_SIBLING_PLAN", "0")
        for _ in range(4):
            got = _grid_round(D, grid, T)
        assert st.as_dict() == {"launches": 0, "served": 0, "dropped": 0, "retired": 0} and not D._sib_table()
        assert all(MC.same_bits(g, MC.oracle(a, r)) for r, g in zip(ROUND, got))
        monkeypatch.delenv("XG_SIBLING_PLAN")
        # inside grid.fused(), and on a fuse=True grid: deferred results have exact knowledge
        with grid.fused():
            for _ in range(4):
                got = _grid_round(D, grid, T)
        fgrid, FT, _ = _grid(D, fuse=True)
        for _ in range(4):
            fgot = _grid_round(D, fgrid, FT)
        assert st.as_dict() == {"launches": 0, "served": 0, "dropped": 0, "retired": 0} and not D._sib_table()
        assert all(MC.same_bits(g, MC.oracle(a, r)) and MC.same_bits(f, MC.oracle(a, r)) for r, g, f in zip(ROUND, got, fgot))
        # entering a fused block drops what an eager round left held
        _live(D, T.data)
        _call(D, T.data, A)
        assert st["launches"] == 1 and any(s.held for s in D._sib_table().values())
        with grid.fused():
            _call(D, T.data, B)
        assert st["dropped"] == 3 and not D._sib_table()
    finally:
        D.drop_sibling_plans()


def test_a_second_thread_has_its_own_table(host_abi):
    from xgcm_amd import device as D

    st = _fresh(D)
    try:
        a, x = _field(D)
        _live(D, x)
        seen = {}

        def other():
            try:
                seen["table"] = len(D._sib_table())
                seen["got"] = [D.tohost(_call(D, x, r)) for r in ROUND]
                seen["stats"] = D.SIBLING_STATS.as_dict()
                seen["keys"] = len(D._sib_table())
            finally:
                D.drop_sibling_plans()

        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert seen["table"] == 0 and seen["keys"] == 1
        assert seen["stats"] == {"launches": 0, "served": 0, "dropped": 0, "retired": 0}
        assert all(MC.same_bits(g, MC.oracle(a, r)) for r, g in zip(ROUND, seen["got"]))
        # this thread's plan did not notice
        got = [D.tohost(_call(D, x, r)) for r in ROUND]
        assert st.as_dict() == {"launches": 1, "served": 3, "dropped": 0, "retired": 0}
        assert all(MC.same_bits(g, MC.oracle(a, r)) for r, g in zip(ROUND, got))
    finally:
        D.drop_sibling_plans()


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", SCENARIOS + [scenario_byte_bound], ids=lambda f: f.__name__[9:])
def test_plan_on_the_gpu(monkeypatch, scenario):
    from xgcm_amd import device as D

    try:
        scenario(D, monkeypatch) if scenario is scenario_byte_bound else scenario(D)
        torch.cuda.synchronize()
    finally:
        D.drop_sibling_plans()


@pytest.mark.gpu
def test_nothing_is_held_across_the_start_of_a_capture():
    from xgcm_amd import device as D

    st = _fresh(D)
    try:
        a, x = _field(D)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _live(D, x)
            _call(D, x, A)
            assert st["launches"] == 1 and any(s.held for s in D._sib_table().values())
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = [_call(D, x, r) for r in ROUND]
        assert st.as_dict() == {"launches": 1, "served": 0, "dropped": 3, "retired": 1} and not D._sib_table()
        x.add_(1)
        graph.replay()
        torch.cuda.synchronize()
        assert all(MC.same_bits(D.tohost(o), MC.oracle(a + 1, r)) for r, o in zip(ROUND, outs))  # every kernel was recorded
    finally:
        D.drop_sibling_plans()
