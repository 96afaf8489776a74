"""What every call into `libgem_hip.so` shares on the Python side: the pointer and stream arguments, the check of a tensor argument, and
the staged call of the features that upload a host table and need scratch memory.  torch is imported where it is used, so that the
modules that lean on this one still import without it."""
import contextlib
import ctypes as C

import numpy as np


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call_stream(device, stream=None):
    """The torch stream a call runs on: `stream`, or the current stream of `device`."""
    import torch
    return torch.cuda.current_stream(device) if stream is None else stream


def check_tensor(x, dtype, shape=None, *, numel=None, at_least=None, rows=None, what=None, error=None, shape_error=None):
    """`x` must be a contiguous device tensor of `dtype` (else `error`: an exception in the entry point's own words; default: a
    TypeError naming `what`) that fits what is given of (else `shape_error`; default: `error`, or a ValueError naming `what`)
      shape     its shape, a None entry standing for any size: (None, 15, 3) is [F,15,3] with any F;
      numel     its number of elements;
      at_least  the fewest elements it may hold (an `out` buffer may be larger than what is written);
      rows      (n, width): [n, >= width] with unit stride along a row and any stride between rows (not contiguous, then).
    None is not a tensor."""
    import torch
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == dtype and (rows is not None or x.is_contiguous())):
        raise error or TypeError("%s wants contiguous device tensors of the documented dtypes" % what)
    if not ((shape is None or (x.dim() == len(shape) and all(s is None or s == g for s, g in zip(shape, x.shape))))
            and (numel is None or x.numel() == numel) and (at_least is None or x.numel() >= at_least)
            and (rows is None or (x.dim() == 2 and x.shape[0] == rows[0] and x.shape[1] >= rows[1] and x.stride(1) == 1))):
        raise shape_error or error or ValueError("%s: a tensor of shape %s where %s is expected" % (what, tuple(x.shape), tuple(shape)))


def check_tensors(what, *specs):
    """Every (tensor, dtype, shape) of `specs` through `check_tensor` in the name of `what`; a tensor that is None is an optional
    argument that was not given and is skipped."""
    for x, dtype, shape in specs:
        if x is not None:
            check_tensor(x, dtype, shape, what=what)


class _Staged:
    """One staged call in progress (`staged_call`): `device`, `stream`, and what it handed out."""

    def __init__(self, lib, device, stream):
        self.lib, self.device, self.stream, self._handed = lib, device, stream, []

    def upload(self, *arrays):
        """ONE host-to-device copy of the arrays' bytes, one behind the other without padding -> a device view per array, of its
        dtype and shape.  The caller orders the arrays so that every view starts at a multiple of its element size."""
        import torch
        host = [np.ascontiguousarray(a) for a in arrays]
        flat = np.concatenate([a.reshape(-1).view(np.uint8) for a in host])
        up = torch.empty(len(flat), dtype=torch.uint8, device=self.device).copy_(torch.from_numpy(flat))
        self._handed.append(up)
        parts = up.split([a.nbytes for a in host])
        return [p.view(torch.from_numpy(np.empty(0, a.dtype)).dtype).reshape(a.shape) for a, p in zip(host, parts)]

    def work(self, nbytes):
        """Scratch memory of at least `nbytes` bytes (and never empty), as a float64 device tensor."""
        import torch
        t = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self.device)
        self._handed.append(t)
        return t

    def run(self, fn, *args):
        """fn(*args, stream) -> (return code, the library's message for it: "" for 0)."""
        rc = fn(*(args + (C.c_void_p(self.stream.cuda_stream),)))
        return rc, ((self.lib.gem_last_error() or b"").decode() if rc else "")


@contextlib.contextmanager
def staged_call(lib, device, stream=None):
    """The frame of a library call that takes a host table and scratch memory: inside, `device` and `stream` (default: the device's
    current stream) are torch's current ones, and the `_Staged` given has `upload`, `work` and `run`; on the way out the stream is
    recorded on what those handed out, so that the caller may drop the tensors while the work is only enqueued.  Nothing waits."""
    import torch
    device = torch.device(device)
    st = call_stream(device, stream)
    with torch.cuda.device(device), torch.cuda.stream(st):
        call = _Staged(lib, device, st)
        try:
            yield call
        finally:
            for t in call._handed:
                t.record_stream(st)
