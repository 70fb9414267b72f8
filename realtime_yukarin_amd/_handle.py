"""What the handles over the audio units of libry355.so share (`world_synth.Synthesizer`, `world_analysis.Analyzer`, `crepe.CrepeModel`):
one rule for the life of a device handle, and the float64 pointer helpers of their calls."""
import ctypes
import os
from typing import Optional

_DP = ctypes.POINTER(ctypes.c_double)


def _dptr(a):
    return a.ctypes.data_as(_DP) if a is not None else ctypes.cast(ctypes.c_void_p(0), _DP)


class EngineForTests(object):
    """tests: `ctx`, a context over another build of the library (the emulator), for the handles a module's own factories create.  Every
    module keeps an instance of its own (`engine_for_tests`): setting one leaves the others alone."""

    def __init__(self):
        self.ctx = None


class DeviceHandle(object):
    """A handle of the C ABI that is created lazily in the process that first uses it, dropped when the object is pickled and destroyed only
    by the process that owns it -- picklable and fork-safe.  `ctx` (tests) is a context over another build of the library -- the emulator --
    used instead of the product's context of `device` while the object stays in the process that made that context.
    Subclasses: `_destroy`, the name of the symbol that frees the handle, and `_create(lib, ctx) -> c_void_p`."""
    _destroy = None

    def __init__(self, ctx=None, device: Optional[int] = None):
        self.device = int(os.environ.get('RY_DEVICE', '0')) if device is None else int(device)
        self._given_ctx = ctx
        self._ctx = None
        self._handle = None
        self._pid = None

    def __getstate__(self):
        d = dict(self.__dict__)
        d.update(_handle=None, _pid=None, _ctx=None, _given_ctx=None)
        return d

    def _create(self, lib, ctx):
        raise NotImplementedError

    def _get(self):
        """-> (library, handle) of this process."""
        if self._handle is None or self._pid != os.getpid():
            from . import engine
            given = self._given_ctx is not None and self._given_ctx.pid == os.getpid()
            self._ctx = self._given_ctx if given else engine.get_context(self.device)
            self._handle, self._pid = self._create(self._ctx.lib, self._ctx), os.getpid()
        return self._ctx.lib, self._handle

    def close(self):
        if self._handle is not None and self._pid == os.getpid() and self._ctx is not None and self._ctx.handle is not None:
            getattr(self._ctx.lib.dll, self._destroy)(self._handle)
        self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
