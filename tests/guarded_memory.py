"""Results and inputs of `xgcm_amd.device` between guard bands: a store outside a result and a read outside an input show.

Every comparison of the suite looks at the cells INSIDE a result.  `guarded(D, monkeypatch, offset)` patches the two points
through which `xgcm_amd.device` gets its memory, for as long as the `with` block lasts:

`D._empty`        every result (and intermediate, and the workspace of the tridiagonal solve) is a contiguous tensor cut from
                  the middle of a byte arena of its own, `[guard | payload | guard]`.  The guards hold `PATTERN`, tiled from
                  the start of the arena; the payload is pre-filled with 0xFF bytes -- a NaN in float64 and in float32 -- so a
                  cell the kernel never writes differs from the reference.  `check()` compares both guards with the pattern,
                  in the memory they live in.
`D._MEM.place`    the copy of a host array is put in the middle of such an arena whose guards hold 0xFF bytes: a float read
                  from outside the input is a NaN and, unless the kernel discards it, reaches the result.

Guard size on each side: `max(64 KiB, 2 planes, 32 rows)` of the array's trailing (Y, X) plane, rounded up to 512 bytes --
a padded tail band of 32 rows or a whole plane written past (or before) the array stays inside memory the test owns.  The 32
rows only matter for arrays of fewer than 16 rows and more than 64 KiB per 32 rows; `_guard_bytes` asserts the condition.

`PATTERN` is eight bytes that read as a NaN at every 4- and 8-byte aligned position and hold no 0xFF byte, so a read outside
an INTERMEDIATE result (a guarded result handed to the next call as its input) is a NaN too.

`offset`: the payload begins `G + offset` bytes into the arena.  0 keeps the 512-byte alignment of torch's allocator, so the
launchers choose what they choose in production; 16 is aligned to 16 bytes and not to 32; the element size makes a 16-byte
alignment test fail and drives the one-element store forms.

What this method does not see: a read outside an input whose value is discarded (a lane that is loaded and masked off, a
NaN that a NaN-skipping sum counts as 0);
memory the library allocates by itself (the chained scans' hand-off words, LDS, the scatter pool); host tensors that are not
contiguous and arrays that are in the target memory already (a tensor the test made with `.cuda()`), which `place` never sees;
stores further than the guard size from the result."""

import contextlib

import numpy as np
import torch

PATTERN = (0xA5, 0x5A, 0xC0, 0x7F, 0xA5, 0x5A, 0xF8, 0x7F)
POISON = 0xFF
MIN_GUARD = 64 << 10
TAIL_ROWS = 32
ALIGN = 512


def _round_up(n, to):
    return -(-int(n) // to) * to


def _guard_bytes(shape, itemsize):
    shape = tuple(int(v) for v in shape)
    row = (shape[-1] if shape else 1) * itemsize
    plane = row * (shape[-2] if len(shape) > 1 else 1)
    G = _round_up(max(MIN_GUARD, 2 * plane, TAIL_ROWS * row), ALIGN)
    assert G % ALIGN == 0 and G >= MIN_GUARD and G >= 2 * plane and G >= TAIL_ROWS * row
    return G


class GuardTouched(AssertionError):
    """a guard byte changed: `side` ("before" / "after") and `at`, the byte offset relative to the payload's start"""

    def __init__(self, text, side, at):
        super().__init__(text)
        self.side, self.at = side, at


class Guards:
    def __init__(self, device, offset):
        self.device, self.offset = torch.device(device), int(offset)
        self.results = []          # (arena, G, nbytes) of every result handed out since the last check
        self.handed_out = 0        # results handed out in all
        self.placed = 0            # inputs placed in all
        self._tile = torch.tensor(PATTERN, dtype=torch.uint8, device=self.device)
        self._pattern = self._tile.repeat(MIN_GUARD // len(PATTERN))

    def pattern(self, start, length):
        """`length` bytes of the tiled pattern as it stands `start` bytes into an arena"""
        phase = start % len(PATTERN)
        if self._pattern.numel() < phase + length:
            self._pattern = self._tile.repeat(-(-(phase + length) // len(PATTERN)) + 1)
        return self._pattern[phase:phase + length]

    def _arena(self, shape, dtype, fill_guards):
        """(arena, G, nbytes, payload): the payload is a contiguous view of `shape` / `dtype`, `G + offset` bytes in"""
        itemsize = torch.empty((), dtype=dtype).element_size()
        assert self.offset % itemsize == 0, "the payload has to stay aligned to its element size"
        n = 1
        for v in shape:
            n *= int(v)
        nbytes = n * itemsize
        G = _guard_bytes(shape, itemsize)
        total = 2 * G + _round_up(self.offset + nbytes, ALIGN)
        if fill_guards is None:
            arena = self.pattern(0, total).clone()
        else:
            arena = torch.full((total,), fill_guards, dtype=torch.uint8, device=self.device)
        at = G + self.offset
        assert arena.data_ptr() % 16 == 0
        payload = arena[at:at + nbytes]
        return arena, G, nbytes, payload

    def empty(self, shape, dtype, device=None):
        shape = tuple(int(v) for v in shape)
        if 0 in shape:
            return torch.empty(shape, dtype=dtype, device=self.device)
        arena, G, nbytes, payload = self._arena(shape, dtype, None)
        payload.fill_(POISON)
        self.results.append((arena, G, nbytes))
        self.handed_out += 1
        return payload.view(dtype).view(shape)

    def place(self, original, t, private=False):
        if t.numel() == 0 or not t.is_contiguous() or t.dtype == torch.bfloat16:
            return original(t, private)
        arena, G, nbytes, payload = self._arena(tuple(t.shape), t.dtype, POISON)
        out = payload.view(t.dtype).view(tuple(t.shape))
        out.copy_(t)
        self.placed += 1
        return out

    def first_touched(self):
        """(index of the result among those handed out since the last check, side, byte offset relative to the payload) of
        the first changed guard byte, or None; the comparison runs where the arenas live"""
        for k, (arena, G, nbytes) in enumerate(self.results):
            at = G + self.offset
            lo, hi = arena[:at], arena[at + nbytes:]
            assert hi.numel() >= G
            same = torch.equal(lo, self.pattern(0, at)) and torch.equal(hi, self.pattern(at + nbytes, hi.numel()))
            if same:
                continue
            bad = (lo != self.pattern(0, at)).nonzero()
            if bad.numel():
                return k, "before", int(bad[0]) - at
            bad = (hi != self.pattern(at + nbytes, hi.numel())).nonzero()
            return k, "after", nbytes + int(bad[0])
        return None

    def check(self, name="call"):
        """both guards of every result handed out since the last check still hold the pattern, and there was a result"""
        results, found = self.results, self.first_touched()
        self.results = []
        if found is not None:
            k, side, at = found
            raise GuardTouched(f"{name}: result {k} of {len(results)} (payload of {results[k][2]} bytes): guard {side} the payload "
                               f"changed, first at byte {at} relative to the payload's start", side, at)
        assert results, f"{name}: no result came from `_empty`: a wrapper bypasses it"


@contextlib.contextmanager
def guarded(D, monkeypatch, offset=0):
    """`xgcm_amd.device as D` with guarded results and inputs; yields the `Guards` whose `check(name)` is called after every
    call under test"""
    mem = D._MEM
    g = Guards(mem.device, offset)
    original = mem.place
    with monkeypatch.context() as mp:
        mp.setattr(D, "_empty", g.empty)
        mp.setattr(mem, "place", lambda t, private=False: g.place(original, t, private), raising=True)
        yield g


def arena_of(t):
    """(base uint8 arena, byte offset of the tensor's first element in it) of a guarded result or placed input"""
    base = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    at = t.data_ptr() - base.data_ptr()
    assert base.dim() == 1 and MIN_GUARD <= at and at + t.numel() * t.element_size() + MIN_GUARD <= base.numel()
    return base, at


def numpy_of(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ---- planted operators: what the harness has to report -------------------------------------------------------------------
# One small "operator" written with torch indexing, out[i] = x[i] + x[min(i + 1, n - 1)] over the flattened array, in a correct
# form and in five forms that misuse the result or the placed input THROUGH THE ARENA'S BASE TENSOR: every access is inside the
# arena, so nothing can fault, on the host or on the device.
def planted_want(x):
    flat = x.reshape(-1)
    return (flat + np.concatenate([flat[1:], flat[-1:]])).reshape(x.shape)


def _planted(D, x, plant):
    t = D.asdevice(x)
    out = D._empty(t.shape, t.dtype, t.device)
    n, item = t.numel(), t.element_size()
    flat = t.reshape(-1)
    nxt = torch.cat([flat[1:], flat[-1:]])
    if plant == "read one element after the input":
        base, at = arena_of(t)
        nxt = base[at + item:at + (n + 1) * item].view(t.dtype)
    res = flat + nxt
    if plant == "a cell left unwritten":
        out.view(-1)[:n // 2] = res[:n // 2]
        out.view(-1)[n // 2 + 1:] = res[n // 2 + 1:]
    else:
        out.view(-1).copy_(res)
    base, at = arena_of(out)
    if plant == "store one element before the result":
        base[at - item:at].view(t.dtype)[0] = 1.0
    elif plant == "store one element after the result":
        base[at + n * item:at + (n + 1) * item].view(t.dtype)[0] = 1.0
    elif plant == "store in the last byte of the far guard":
        base[-1] = 0
    return out


PLANTS = ("store one element before the result", "store one element after the result", "store in the last byte of the far guard",
          "a cell left unwritten", "read one element after the input")


def planted_verdict(D, monkeypatch, x, plant, offset, same_bits):
    """what the harness says about one planted operator (None: the correct one): ("guard", side, byte offset), ("differs",
    number of cells) or ("clean",)"""
    with guarded(D, monkeypatch, offset) as g:
        out = _planted(D, x, plant)
        try:
            g.check(str(plant))
        except GuardTouched as err:
            assert str(plant) in str(err)
            return ("guard", err.side, err.at)
        got, want = numpy_of(out), planted_want(x)
        if not same_bits(got, want):
            return ("differs", int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()))
        return ("clean",)


def planted_expectation(x, plant, offset):
    G, nbytes = _guard_bytes(x.shape, x.itemsize), x.nbytes
    far = 2 * G + _round_up(offset + nbytes, ALIGN) - (G + offset) - 1
    return {None: ("clean",), PLANTS[0]: ("guard", "before", -x.itemsize), PLANTS[1]: ("guard", "after", nbytes),
            PLANTS[2]: ("guard", "after", far), PLANTS[3]: ("differs", 1), PLANTS[4]: ("differs", 1)}[plant]


# ---- the call matrix of tests/test_integer_exact.py::test_integer_kernels_at_kernel_sizes --------------------------------
KERNEL_SHAPES = ((5, 260, 512), (3, 67, 131), (2, 300, 64))
MATRIX_FILL = 3.7


def kernel_size_matrix(D, R, x, a, integer=False, no_diff=False, axes=(0, 1, 2)):
    """(name, thunk, reference) of every call that test makes on one array: `x` the resident array, `a` its host twin.  With
    `integer` the references are the ones that test uses (numpy's integer cumsum and sum); the float twins take the
    statements of `oracle.refimpl`.  `axes`: the part of the matrix along these axes (the pad comes with axis 0)"""
    fill = MATRIX_FILL
    for ax in axes:
        for (lo, hi) in ((1, 0), (0, 1), (1, 1), (0, 0)):
            for bc in ("periodic", "fill", "extend"):
                for op in ("diff", "interp", "min", "max"):
                    if no_diff and op == "diff":
                        continue
                    yield (f"{op} axis {ax} pads {lo},{hi} {bc}",
                           lambda op=op, ax=ax, lo=lo, hi=hi, bc=bc: D.stencil1d(op, x, ax, lo, hi, bc if (lo or hi) else None, fill),
                           lambda op=op, ax=ax, lo=lo, hi=hi, bc=bc: R.stencil1d(op, a, ax, lo, hi, bc, fill))
        for rev in (False, True):
            for trims in ((0, 0, 0, 0), (0, 1, 1, 0), (1, 0, 0, 1), (0, 0, 1, 0)):
                for bc in ("periodic", "fill", "extend"):
                    yield (f"cumsum axis {ax} {trims} {bc}{' reversed' if rev else ''}",
                           lambda ax=ax, rev=rev, trims=trims, bc=bc: D.cumsum1d(x, ax, *trims, bc if (trims[2] or trims[3]) else None,
                                                                                 fill, rev, True),
                           lambda ax=ax, rev=rev, trims=trims, bc=bc: R.cumsum1d(a, ax, *trims, bc, fill, rev, False))
        yield (f"sum axis {ax}", lambda ax=ax: D.reduce1d(x, ax, None, True),
               (lambda ax=ax: np.sum(a, axis=ax)) if integer else (lambda ax=ax: R.integrate(a, ax, None, True)))
        if not integer:   # a NaN counts as 0 in the sums above: the forms that let a NaN read from outside the input through
            for rev in (False, True):
                yield (f"cumsum axis {ax} keeping NaN{' reversed' if rev else ''}",
                       lambda ax=ax, rev=rev: D.cumsum1d(x, ax, 0, 0, 0, 0, None, fill, rev, False),
                       lambda ax=ax, rev=rev: R.cumsum1d(a, ax, 0, 0, 0, 0, None, fill, rev, False))
            yield (f"sum axis {ax} keeping NaN", lambda ax=ax: D.reduce1d(x, ax, None, False), lambda ax=ax: R.integrate(a, ax, None, False))
    if 0 not in axes:
        return
    pad = ({0: (2, 1), 2: (1, 3)}, {0: "periodic", 2: "fill"}, {2: 5.5})
    yield ("pad", lambda: D.pad_nd(x, *pad), lambda: R.pad_nd(a, *pad))
