"""What the output plans (diag, clim, ens) share: the life of a plan handle, the check of a GPU tensor, and the call of a
_dev entry point on torch's current stream."""
from __future__ import annotations

import ctypes as C


class Handle:
    """A plan handle of the library in self.h: made by the create function, destroyed by close() or with the object."""
    _destroy = ""  # the library's destroy function

    def _create(self, create: str, *args):
        """self.h = create(*args, &h); an error is a GrebError with the library's message (_reword may edit it)."""
        from . import engine
        self.h = C.c_void_p()
        rc = getattr(engine.lib(), create)(*args, C.byref(self.h))
        if rc != 0:
            self.h = None
            raise engine.GrebError(rc, self._reword(engine.lib().greb_engine_last_error(None).decode()))

    def _reword(self, msg: str) -> str:
        return msg

    def close(self):
        if getattr(self, "h", None):
            from . import engine
            getattr(engine.lib(), self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gpu_tensor_check(x, shape_ok: bool, who: str, expected: str) -> int:
    """The device index of x, a contiguous float32 GPU tensor whose shape the caller found right; else GrebError(-1)."""
    import torch
    from . import engine
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and shape_ok):
        raise engine.GrebError(-1, f"{who}: a contiguous float32 GPU tensor {expected} expected")
    return x.device.index if x.device.index is not None else torch.cuda.current_device()


def ptr(t):
    """The device pointer of a tensor as an argument (None stays None: a product that was not selected)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def call_on_current_stream(dev: int, fn, *args) -> None:
    """fn(*args, stream) with device `dev` current and torch's current stream there, without synchronising."""
    import torch
    from . import engine
    with torch.cuda.device(dev):
        engine._check(fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
