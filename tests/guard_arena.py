"""Guard bands around every tensor a kernel writes (tests/test_gpu_memory_contract.py, tests/test_guard_arena_host.py).

The value tests compare what a launch computed; nothing in them sees WHERE it wrote.  Here every output and workspace is carved out of
one byte arena with an untouched band of a known pattern on either side, so a store past the end (or before the start) of a tensor
changes a band and `check()` names the tensor and the distance.

    arena = GuardArena(nbytes, device)                     # one per test, never reset: views of it may outlive the call
    y = arena.take((bs, m), torch.float32, name="y")       # every byte 0xFF: NaN / 255 / -1 -- an element nobody wrote shows
    with installed(monkeypatch, arena, ops, quant):        # the wrappers' own torch.empty / zeros / full come from the arena too
        ops.dequant_gemm(..., out=y)
    torch.cuda.synchronize()
    assert arena.check() == []

A plain module (no fixtures, no pytest settings); it works on CPU tensors as well, which is how the helper itself is tested.
"""
import contextlib
import sys

import torch

PATTERN = 0xA5             # what a band holds
UNINIT = 0xFF              # what an "uninitialised" carved tensor holds: NaN in fp16 / bf16 / fp32 / fp64, 255 in uint8, -1 in int32 / int64
ALIGN = 256                # carved addresses, in absolute terms (what torch's device allocator gives; include/quip_amd.h asks for 16)
MIN_BAND = 64 * 1024
BAND_ROWS = 16             # the row tile of every MFMA kernel here: a whole stray tile behind the last row lands inside the band
BIG = 64 << 20             # freeze(): tensors above this are fingerprinted by a checksum instead of a copy

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def band_bytes(shape, dtype):
    """the band-width rule: at least 64 KiB and at least 16 leading-dimension slices of the carved tensor, in whole alignment units"""
    shape = tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    row = item
    for s in shape[1:]:
        row *= s
    need = max(MIN_BAND, BAND_ROWS * row)
    return (need + ALIGN - 1) // ALIGN * ALIGN


def bits(t):
    """t reinterpreted as integers of its element size: comparisons on it are bit for bit (NaN == NaN, -0 != +0)"""
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t if not (t.is_floating_point() or t.is_complex()) else t.view(_INT_VIEW[t.element_size()])


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def count_fill(t, byte=UNINIT):
    """how many elements of t still hold the fill (every byte == `byte`)"""
    b = bits(t)
    if b.numel() == 0:
        return 0
    if b.dtype == torch.uint8:
        return int((b == byte).sum())
    word = int.from_bytes(bytes([byte]) * b.element_size(), "little", signed=True)
    return int((b == word).sum())


class Violation:
    """bytes [first, last] (1 = the byte next to the tensor) `side` ('before' the start | 'after' the end) of a carved tensor changed"""

    def __init__(self, region, side, first, last, nbytes):
        self.name, self.shape, self.dtype = region["name"], region["shape"], region["dtype"]
        self.side, self.first, self.last, self.nbytes = side, first, last, nbytes

    def __repr__(self):
        where = "after the end" if self.side == "after" else "before the start"
        return (f"{self.nbytes} byte(s) changed {self.first}..{self.last} bytes {where} of {self.name} "
                f"(shape {tuple(self.shape)}, {self.dtype})")


class GuardArena:
    def __init__(self, nbytes, device, uninit=UNINIT):
        assert 0 < nbytes <= 4 << 30, "one arena per test, sized to the case, never above 4 GiB"
        self.device = torch.device(device)
        self.uninit = int(uninit)
        self.buf = torch.full((int(nbytes) + ALIGN,), PATTERN, dtype=torch.uint8, device=self.device)
        self._cursor = (-self.buf.data_ptr()) % ALIGN           # bumps forward only; never reset (views may be kept by caches)
        self.regions = []

    # ---------------------------------------------------------------------------------------------------------------- carving
    def _carve(self, nbytes, shape, dtype, name):
        band = band_bytes(shape, dtype)
        start = self._cursor + band
        end = start + nbytes
        after_end = end + band
        if after_end > self.buf.numel():
            raise MemoryError(f"guard arena of {self.buf.numel()} bytes is full: {name} needs {nbytes} + 2 x {band} at offset {self._cursor}")
        self._cursor = after_end + (-(self.buf.data_ptr() + after_end)) % ALIGN
        self.regions.append(dict(name=name, shape=tuple(shape), dtype=dtype, start=start, end=end, band=band))
        return self.buf[start:end]

    def take(self, shape, dtype, fill=None, name=None, stride=None):
        """a view of `shape` / `dtype` (contiguous, or with `stride` in elements) at a 256-byte aligned address with a band before and
        behind it.  fill None: every byte `uninit` (0xFF); a number: filled with it (zeros / full requests)."""
        if isinstance(shape, int):
            shape = (shape,)
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        if stride is None:
            n = 1
            for s in shape:
                n *= s
        else:
            stride = tuple(int(s) for s in stride)
            n = 0 if any(s == 0 for s in shape) else 1 + sum((s - 1) * st for s, st in zip(shape, stride))
        name = name or f"tensor#{len(self.regions)}"
        raw = self._carve(n * item, shape, dtype, name)
        raw.fill_(self.uninit)
        flat = raw.view(dtype)
        out = flat.view(shape) if stride is None else flat.as_strided(shape, stride)
        if fill is not None:
            out.fill_(fill)
        return out

    def copy_of(self, t, name=None):
        """a carved tensor with t's shape, strides (dense tensors) and bits"""
        out = self.take(t.shape, t.dtype, name=name, stride=None if t.is_contiguous() else _like_strides(t))
        out.copy_(t)
        return out

    # ---------------------------------------------------------------------------------------------------------------- checking
    def check(self):
        """compare the bands (only the bands) with the pattern, on the arena's device; returns a list of Violation, empty when clean"""
        if not self.regions:
            return []
        spans = []
        for r in self.regions:
            spans.append((r["start"] - r["band"], r["start"], r, "before"))
            spans.append((r["end"], r["end"] + r["band"], r, "after"))
        allb = torch.cat([self.buf[a:b] for a, b, _, _ in spans])
        bad = (allb != PATTERN).nonzero().reshape(-1).cpu().tolist()
        if not bad:
            return []
        out, base, k = [], 0, 0
        for a, b, r, side in spans:
            mine = []
            while k < len(bad) and bad[k] < base + (b - a):
                mine.append(bad[k] - base)
                k += 1
            base += b - a
            if mine:
                dist = [o + 1 for o in mine] if side == "after" else [(b - a) - o for o in mine]
                out.append(Violation(r, side, min(dist), max(dist), len(mine)))
        return out

    def live_bytes(self):
        return sum(r["end"] - r["start"] for r in self.regions)


def _like_strides(t):
    """the strides torch.empty_like(t) would pick (dense layouts are preserved, anything else becomes contiguous)"""
    return torch.empty_like(t, device="meta").stride()


# -------------------------------------------------------------------------------------------------------------------- torch proxy
def _caller(depth=2):
    f = sys._getframe(depth)
    return f"{f.f_code.co_filename.rsplit('/', 1)[-1]}:{f.f_lineno} {f.f_code.co_name}"


def _size(args):
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


class TorchProxy:
    """stands in for the `torch` global of a module: everything is torch's, except that empty / empty_like / zeros / zeros_like / full /
    ones / empty_strided for a GPU device carve from the arena (CPU requests pass through)"""

    def __init__(self, arena, carve_cpu=False):
        self._arena = arena
        self._carve_cpu = carve_cpu            # the host tests of the helper: a CPU arena serves CPU requests

    def __getattr__(self, name):
        return getattr(torch, name)

    def _mine(self, device):
        if device is None:
            return False
        kind = torch.device(device).type
        return kind == self._arena.device.type and (kind != "cpu" or self._carve_cpu)

    def _new(self, size, dtype, fill, kw, stride=None):
        for k in ("layout", "requires_grad", "pin_memory", "memory_format", "out"):
            v = kw.pop(k, None)
            assert v in (None, False, torch.strided, torch.contiguous_format, torch.preserve_format), f"guard arena: {k}={v} is not supported"
        assert not kw, f"guard arena: unexpected arguments {sorted(kw)}"
        return self._arena.take(size, dtype or torch.get_default_dtype(), fill=fill, name=_caller(3), stride=stride)

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._new(_size(size), dtype, None, kw)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._new(_size(size), dtype, 0, kw)

    def ones(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.ones(*size, dtype=dtype, device=device, **kw)
        return self._new(_size(size), dtype, 1, kw)

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:
            dtype = torch.bool if isinstance(fill_value, bool) else torch.int64 if isinstance(fill_value, int) else torch.get_default_dtype()
        return self._new(_size((size,)), dtype, fill_value, kw)

    def empty_strided(self, size, stride, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.empty_strided(size, stride, dtype=dtype, device=device, **kw)
        return self._new(tuple(size), dtype, None, kw, stride=tuple(stride))

    def _like(self, t, fill, dtype, device, kw):
        st = None if t.is_contiguous() else _like_strides(t)
        return self._new(tuple(t.shape), dtype or t.dtype, fill, kw, stride=st)

    def empty_like(self, t, dtype=None, device=None, **kw):
        if not self._mine(device if device is not None else t.device):
            return torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._like(t, None, dtype, device, kw)

    def zeros_like(self, t, dtype=None, device=None, **kw):
        if not self._mine(device if device is not None else t.device):
            return torch.zeros_like(t, dtype=dtype, device=device, **kw)
        return self._like(t, 0, dtype, device, kw)


# -------------------------------------------------------------------------------------------------------------------- call ledger
LEDGER = set()             # C ABI entry points that ran while an arena was installed (the completeness test reads it)


@contextlib.contextmanager
def installed(monkeypatch, arena, *modules, ledger=LEDGER, carve_cpu=False):
    """for the `with` body: the `torch` global of every module in `modules` is a TorchProxy on `arena`, and every call through
    quip_amd._lib.call is entered in the ledger.  Everything is put back on exit."""
    from quip_amd import _lib
    proxy = TorchProxy(arena, carve_cpu=carve_cpu)
    real_call = _lib.call

    def call(name, *args):
        ledger.add(name)
        return real_call(name, *args)

    with monkeypatch.context() as mp:
        for mod in modules:
            assert getattr(mod, "torch") is torch, f"{mod.__name__}.torch is not the torch module (an arena is installed already?)"
            mp.setattr(mod, "torch", proxy)
        mp.setattr(_lib, "call", call)
        yield proxy


# -------------------------------------------------------------------------------------------------------------------- fingerprints
def checksum64(t):
    """a 64-bit position-weighted checksum of t's bytes, in integer arithmetic on t's device"""
    flat = t.contiguous().view(-1)
    b = bits(flat)
    total = torch.zeros((), dtype=torch.int64, device=t.device)
    step = 1 << 24
    for lo in range(0, b.numel(), step):
        c = b[lo:lo + step].to(torch.int64)
        w = (torch.arange(lo, lo + c.numel(), device=t.device, dtype=torch.int64) % 2147483629) * 2654435761 + 0x9E3779B97F4A7C15 % (1 << 62)
        total = total + (c * w).sum() + (c ^ (w >> 7)).sum()
    return int(total)


class Frozen:
    """bit-exact fingerprints of tensors a call must not change"""

    def __init__(self):
        self.items = []

    def add(self, *tensors, **named):
        for i, t in enumerate(tensors):
            named[f"input#{len(self.items) + i}"] = t
        for name, t in named.items():
            if t is None:
                continue
            nbytes = t.numel() * t.element_size()
            self.items.append((name, t, checksum64(t) if nbytes > BIG else t.clone()))
        return self

    def changed(self):
        out = []
        for name, t, fp in self.items:
            same = (checksum64(t) == fp) if isinstance(fp, int) else bit_equal(t, fp)
            if not same:
                out.append(name)
        return out

    def assert_frozen(self):
        bad = self.changed()
        assert not bad, f"inputs changed by the call: {bad}"


def freeze(*tensors, **named):
    return Frozen().add(*tensors, **named)
