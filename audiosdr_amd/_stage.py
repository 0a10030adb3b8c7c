"""What the ctypes mirrors of every handle but the receiver batch (gate.py, resample.py, codec.py, spectrogram.py, fm.py, tone.py, dcs.py, packet.py, cw.py, tuner.py,
front.py) share: the typing of a handle's entry points, the life of a handle, the state records of an audio stage (RecordStage), and the small
conversions of their arguments (_c_int, _stride)."""
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


def _c_int(v, what):
    """v as a C int; `what` is the refusal of a value that does not fit one (the library's own text for the argument)."""
    v = int(v)
    if not -2**31 <= v < 2**31:
        raise AsdrError(what)
    return v


def _stride(stride, n):
    """A row stride that defaults to the call's length n (n_blocks, n_samples)."""
    return int(n) if stride is None else int(stride)


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


class RecordStage(ResetStage):
    """An audio stage: one state record a channel, of _state_dtype (the stage's *_STATE_DTYPE).  The records of the resampler and the
    spectrogram are rows of int16 samples instead; they give the row's shape in _record_shape()."""
    _state_dtype = None

    def _record_shape(self):
        return ()

    def read_state(self):
        """Array [n_channels] of the stage's state records (its *_STATE_DTYPE; int16 [n_channels, samples] for the resampler and
        the spectrogram: every channel's last input samples, oldest first); waits for the handle's work."""
        st = np.zeros((self.n_channels,) + self._record_shape(), dtype=self._state_dtype)
        self._chk(getattr(self._L, self._prefix + "read_state")(self._h, st.ctypes.data_as(C.c_void_p)))
        return st

    def write_state(self, records, channels=None):
        """Writes records (as read_state gives them) into `channels` (default 0 .. len - 1); checked as a whole before one is
        written."""
        rec = np.ascontiguousarray(records, dtype=self._state_dtype).reshape((-1,) + self._record_shape())
        self._chk(getattr(self._L, self._prefix + "write_state")(self._h, _channel_ptr(channels, rec.shape[0]), int(rec.shape[0]),
                                                                 rec.ctypes.data_as(C.c_void_p)))

    # the stages that count blocks (every one but the resampler, the codec and the spectrogram)
    def clear(self):
        self._call("clear")

    def blocks(self):
        return int(getattr(self._L, self._prefix + "blocks")(self._h))
