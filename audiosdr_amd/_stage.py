"""What the ctypes mirrors of every handle but the receiver batch (gate.py, resample.py, codec.py, spectrogram.py, fm.py, tone.py, dcs.py, packet.py, tuner.py,
front.py) share: the typing of a handle's entry points, the life of a handle, and the channel list of write_state."""
import ctypes as C

import numpy as np

from .binding import AsdrError, load_library

vp, i, lg, ll, ip = C.c_void_p, C.c_int, C.c_long, C.c_longlong, C.POINTER(C.c_int)

_typed = set()


def typed_library(prefix, table):
    """The library, with table = {name: (argtypes, restype)} set on its functions prefix + name the first time a prefix is seen."""
    L = load_library()
    if prefix not in _typed:
        for name, (argtypes, restype) in table.items():
            f = getattr(L, prefix + name)
            f.argtypes, f.restype = argtypes, restype
        _typed.add(prefix)
    return L


def _channel_ptr(channels, n_records):
    """write_state's channel list as an int pointer (None without a list); one channel per record."""
    if channels is None:
        return None
    ch = np.ascontiguousarray(channels, dtype=np.int32).reshape(-1)
    if ch.size != n_records:
        raise AsdrError("write_state: %d records for %d channels" % (n_records, ch.size))
    return ch.ctypes.data_as(ip)


class Stage:
    """A handle of the library: self._L the typed library, self._h the handle, _prefix the stage's "asdr_<stage>_"."""
    _prefix = None

    def _create(self, what, handle):
        self._h = handle
        if not handle:
            raise AsdrError("%s failed: %s" % (what, self._L.asdr_last_error().decode()))

    def _call(self, name):
        return self._chk(getattr(self._L, self._prefix + name)(self._h))

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._prefix + "destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise AsdrError(self._L.asdr_last_error().decode())
        return rc

    def synchronize(self):
        self._call("synchronize")


class ResetStage(Stage):
    """A handle whose C API has <prefix>reset (every one but the front end's three)."""

    def reset(self):
        self._call("reset")
