"""
What tests/test_gpu_side_stream.py and tests/test_poisoned_scratch_host.py share ("The stream contract as
tested"): a side stream, a gate that keeps the null stream busy, poisoned scratch memory and the gated ``Device.call``.

The null stream orders everything, so a launch on the wrong stream, a workspace cleared on the null stream or a readback
that is not ordered behind the call's stream cannot show there.  On a side stream (PyTorch's are non-blocking) with the null
stream held busy by the gate, whatever the library puts on the null stream lands behind the gate, while a correct consumer on
the side stream does not wait for it: it reads what the misplaced work has not written yet, and that is poison.
"""
import contextlib

import numpy as np

from bspy_amd._backend import Device, Host

# The gate: GATE_CHAIN products of two GATE_N x GATE_N float32 matrices on the null stream.  Sized on the MI355X from the
# slowest family call of tests/test_gpu_side_stream.py (DESIGN.md holds the measurement): one gate lasts at least four
# times that call.
GATE_N = 4096
GATE_CHAIN = 96


def side_stream():
    """A fresh non-blocking stream.  The caller makes it wait for the default stream before use and synchronises before a
    handle changes stream: one handle is used from one stream at a time (include/bspy_amd.h)."""
    import torch
    assert torch.cuda.default_stream().cuda_stream == 0, "the default stream is not the null stream: the gate would order nothing"
    return torch.cuda.Stream()


class Gate:
    """Ordinary torch work on the default (null) stream with an event behind it: ``pending()`` while it runs."""

    def __init__(self, n=GATE_N, chain=GATE_CHAIN):
        import torch
        self.torch, self.chain, self.armed = torch, chain, 0
        self.null = torch.cuda.default_stream()
        with torch.cuda.stream(self.null):
            self.a = torch.full((n, n), 1.0 / n, dtype=torch.float32, device="cuda")      # a @ a == a: the chain stays finite
            self.b = torch.empty_like(self.a)
        self.event = torch.cuda.Event()
        self.null.synchronize()

    def arm(self):
        torch = self.torch
        with torch.cuda.stream(self.null):
            for _ in range(self.chain // 2):
                torch.mm(self.a, self.a, out=self.b)
                torch.mm(self.b, self.b, out=self.a)
            self.event.record(self.null)
        self.armed += 1

    def pending(self):
        return not self.event.query()

    def ensure(self):
        if not self.pending():
            self.arm()

    def drain(self):
        self.event.synchronize()


def fill(a, pattern):
    """Every byte of the backend's array ``a`` set to ``pattern`` (a CUDA tensor: on the current stream)."""
    if isinstance(a, np.ndarray):
        if a.size:
            a.reshape(-1).view(np.uint8).fill(pattern)
    elif a.numel():
        import torch
        a.view(-1).view(torch.uint8).fill_(pattern)
    return a


def poison_tensor(shape, dtype, pattern):
    """A fresh CUDA tensor of bytes ``pattern``: the ``out=`` of a DeviceSpline device method."""
    import torch
    return fill(torch.empty(shape, dtype=dtype, device="cuda"), pattern)


@contextlib.contextmanager
def poisoned(pattern):
    """``Device.empty`` and ``Host.empty`` hand out buffers whose every byte is ``pattern`` (0 .. 255); ``zeros`` keeps its
    meaning.  ``torch.empty`` and ``np.empty`` themselves are left alone: the sites that call them directly are listed in
    DESIGN.md."""
    assert 0 <= pattern <= 255
    device_empty, host_empty = Device.empty, Host.empty

    def device(self, shape, dtype):
        return fill(device_empty(self, shape, dtype), pattern)

    def host(self, shape, dtype):
        return fill(host_empty(self, shape, dtype), pattern)

    Device.empty, Host.empty = device, host
    try:
        yield
    finally:
        Device.empty, Host.empty = device_empty, host_empty


def _key(x):
    if isinstance(x, (list, tuple)):
        return tuple(_key(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, _key(v)) for k, v in sorted(x.items()))
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return repr(x)


@contextlib.contextmanager
def kept_handles():
    """The line-operator handles (``BandMap``, ``ScanMap``, ``Plan``, ``ProductMap``) that a call makes for itself are made
    once per set of arguments and stay open until the context ends.  A public call makes its maps anew every time, and the
    first device call on a map uploads its tables with a blocking copy on the null stream (include/bspy_amd.h permits
    that): without this every such call of step (d) would wait for the gate, and the gate would prove nothing about the
    launch behind the upload.  With it the uploads belong to the warm-up of step (b).  The steps synchronise in between,
    so a handle is used from one stream at a time."""
    from bspy_amd import _native as nv
    from bspy_amd._backend import Handle
    from bspy_amd.fitting import Plan
    from bspy_amd.product import ProductMap
    from bspy_amd.refinement import BandMap
    from bspy_amd.sums import ScanMap
    cache, inits, close = {}, {}, Handle.close

    def keeping(cls, init):
        def __init__(self, *args, **kwargs):
            key = (cls, _key(args), _key(kwargs))
            if key not in cache:
                init(self, *args, **kwargs)
                cache[key] = dict(self.__dict__)
            self.__dict__.update(cache[key])
        return __init__

    for cls in (BandMap, ScanMap, Plan, ProductMap):
        inits[cls] = cls.__init__
        cls.__init__ = keeping(cls, cls.__init__)
    Handle.close = lambda self: None
    try:
        yield
    finally:
        Handle.close = close
        for cls, init in inits.items():
            cls.__init__ = init
        for (cls, _, _), attributes in cache.items():
            handle = attributes.get("_handle")
            if handle is not None and handle.value:
                getattr(nv.lib(), cls.prefix + "_destroy")(handle)
                handle.value = None                      # every object that shares it now hands NULL to _destroy, which ignores it


class GateLog:
    """What the gated calls saw: (entry point, gate still pending on return) per call."""

    def __init__(self, gate):
        self.gate, self.calls = gate, []

    def run(self, name, call):
        """``call()`` behind an armed gate; notes whether the gate was still pending when it returned."""
        self.gate.ensure()
        result = call()
        self.calls.append((name, self.gate.pending()))
        return result

    def check(self, allowed):
        """Step (e): every call outside ``allowed`` returned in front of a pending gate, and at least one call did: a run in
        which the gate proved nothing does not pass.  -> the allowed entry points that did return behind a finished gate."""
        late = sorted({name for name, pending in self.calls if not pending and name not in allowed})
        assert not late, (f"{', '.join(late)} returned behind a finished gate: the gate was too short, or the call blocked on "
                          f"the null stream (calls: {self.calls})")
        assert any(pending for _, pending in self.calls), f"no gated call returned in front of a pending gate: the gate proved nothing ({self.calls})"
        return sorted({name for name, pending in self.calls if not pending})


@contextlib.contextmanager
def gated(device, gate):
    """``device.call`` (``Device.call``) arms the gate again where it is no longer pending, and notes after the call
    whether it still was.  -> the ``GateLog``."""
    log = GateLog(gate)
    call = device.call

    def gated_call(self, name, *args):
        return log.run(name, lambda: call(self, name, *args))

    device.call = gated_call
    try:
        yield log
    finally:
        device.call = call
