"""
What every operator family shares below its own module, written once: the path switch (``pick_path``, ``choose``), the
line geometry (``lines``), the native handle (``Handle``) and two backends, ``Host`` (NumPy, the ``*_host`` entry points)
and ``Device`` (torch CUDA tensors, the kernels on the current stream), on which a launch is written once.

A launch is a function of a backend: it allocates with ``be.empty`` and hands ``be.code(a)`` and ``be.ptr(a)`` to
``be.call(name, ...)``.  The cell families' drivers (bspy_amd/_cells.py) add the few array operations below; the
line-operator families (refinement, sums, product, reduction, fitting) need the launch alone.  This module imports
``_native`` only, so every other module may use its names at import time.
"""
import ctypes

import numpy as np

from . import _native as nv

FLOATS = (np.float32, np.float64)          # by BSK_F32, BSK_F64: the type of a result that has its operand's type


def is_torch(a):
    return type(a).__module__.startswith("torch")


def pick_path(path, forced):
    """``_path`` of a call, else the module's ``FORCE_PATH``."""
    path = path if path is not None else forced
    if path not in (None, "device", "host"):
        raise ValueError("_path must be None, 'device' or 'host'")
    return path


def choose(path, covered, large, why):
    """The path a call takes: the pinned ``path``, else the device when the kernels cover the call and it is large.
    A device path that is pinned and not covered: ValueError(why)."""
    if path is None:
        return "device" if covered and large else "host"
    if path == "device" and not covered:
        raise ValueError(why)
    return path


def lines(shape, axis, n):
    """(outer, inner) of the lines along ``axis`` (not negative) of a tensor of this shape, which must hold n entries."""
    if shape[axis] != n:
        raise ValueError(f"axis {axis} has {shape[axis]} entries, the map takes {n}")
    return int(np.prod(shape[:axis], dtype=np.int64)), int(np.prod(shape[axis + 1:], dtype=np.int64))


class Handle:
    """A native object made by ``prefix`` + ``_create`` and freed by ``_destroy``.  ``close`` may be called twice, ``with``
    closes; a call on a closed handle hands NULL to the library, which refuses it (``BskError``)."""
    prefix = None
    _handle = None

    def _open(self, *create_args):
        handle = ctypes.c_void_p()
        nv.check(getattr(nv.lib(), self.prefix + "_create")(*create_args, ctypes.byref(handle)))
        self._handle = handle

    def close(self):
        if self._handle is not None:
            getattr(nv.lib(), self.prefix + "_destroy")(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def last_kernel(self):
        return getattr(nv.lib(), self.prefix + "_last_kernel")(self._handle).decode()


class Host:
    """NumPy arrays and the ``*_host`` entry points."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def empty(self, shape, dtype):
        return np.empty(shape, dtype)

    def zeros(self, shape, dtype):
        return np.zeros(shape, dtype)

    def put(self, a, dtype):
        return np.ascontiguousarray(a, dtype)

    def get(self, a):
        return a

    def ptr(self, a):
        return None if a is None else a.ctypes.data

    def code(self, a):
        return nv.dtype_code(a.dtype)

    def cast(self, a, dtype):
        return a.astype(dtype)

    def nonzero(self, a):
        return np.flatnonzero(a).astype(np.int64)

    def cumsum(self, a):
        return np.cumsum(a, dtype=np.int64)

    def isnan(self, a):
        return np.isnan(a)

    def amax(self, a, axes):
        return a.max(axis=axes)

    def sum(self, a, axis):
        return a.sum(axis=axis)

    def repeat(self, a, n):
        return np.repeat(a, n)

    def lexsort(self, columns):
        return np.lexsort(columns)

    def searchsorted(self, a, n):
        return np.searchsorted(a, np.arange(n)).astype(np.int64)

    def arange(self, n):
        return np.arange(n, dtype=np.int64)

    def sort(self, a):
        return np.sort(a)

    def unique(self, a):
        values, inverse = np.unique(a, return_inverse=True)
        return values, inverse.reshape(-1).astype(np.int64)

    def cat(self, arrays):
        return np.concatenate(arrays)

    def call(self, name, *args):
        nv.check(getattr(nv.lib(), name + "_host")(*args))


class Device:
    """The same on contiguous torch CUDA tensors of ``dev``, the kernels on the stream that is current on entry."""

    def __init__(self, dev):
        import torch
        self.torch, self.dev = torch, dev

    @classmethod
    def current(cls):
        """On the current CUDA device, named with its index once: where a NumPy-to-NumPy call computes."""
        import torch
        return cls(torch.device("cuda", torch.cuda.current_device()))

    def __enter__(self):
        self._guard = self.torch.cuda.device(self.dev)
        self._guard.__enter__()
        self.stream = ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        return self

    def __exit__(self, *exc):
        return self._guard.__exit__(*exc)

    def _dtype(self, dtype):
        return getattr(self.torch, np.dtype(dtype).name)

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=self._dtype(dtype), device=self.dev)

    def zeros(self, shape, dtype):
        return self.torch.zeros(shape, dtype=self._dtype(dtype), device=self.dev)

    def put(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.dev)

    def get(self, a):
        return a.cpu().numpy()

    def ptr(self, a):
        return None if a is None else a.data_ptr()

    def code(self, a):
        return nv.BSK_F32 if a.dtype == self.torch.float32 else nv.BSK_F64

    def cast(self, a, dtype):
        return a.to(self._dtype(dtype)).contiguous()

    def nonzero(self, a):
        return self.torch.nonzero(a.reshape(-1)).reshape(-1)             # int64, in index order

    def cumsum(self, a):
        return self.torch.cumsum(a, 0, dtype=self.torch.int64)

    def isnan(self, a):
        return self.torch.isnan(a)

    def amax(self, a, axes):
        return a.amax(dim=axes)

    def sum(self, a, axis):
        return a.sum(dim=axis)

    def repeat(self, a, n):
        return self.torch.repeat_interleave(a, n) if is_torch(n) else a[:, None].expand(-1, n).reshape(-1)

    def lexsort(self, columns):
        order = self.torch.argsort(columns[0], stable=True)
        for column in columns[1:]:
            order = order[self.torch.argsort(column[order], stable=True)]
        return order

    def searchsorted(self, a, n):
        return self.torch.searchsorted(a.contiguous(), self.torch.arange(n, device=self.dev))

    def arange(self, n):
        return self.torch.arange(n, dtype=self.torch.int64, device=self.dev)

    def sort(self, a):
        return self.torch.sort(a).values.contiguous()

    def unique(self, a):
        values, inverse = self.torch.unique(a, sorted=True, return_inverse=True)      # ascending, as np.unique
        return values.contiguous(), inverse.reshape(-1)

    def cat(self, arrays):
        return self.torch.cat(list(arrays))

    def call(self, name, *args):
        nv.check(getattr(nv.lib(), name)(*args, self.stream))
