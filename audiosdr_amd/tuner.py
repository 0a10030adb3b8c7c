"""ctypes mirror of include/asdr_tuner.h: the digital tuner bank (per-receiver digital LO + decimating low-pass) that feeds
the chain's I/Q rows from shared wideband CS16 sources.  Same rules as binding.py: the work happens in libasdr_hip.so on the GPU;
there is no CPU fallback (tests/tuner_ref.py is the independent numpy statement the tests compare with)."""
import ctypes as C

import numpy as np

from .binding import ALL, BLOCK, AsdrError, load_library

TUNER_EXPORTS = ["asdr_tuner_create", "asdr_tuner_destroy", "asdr_tuner_reset", "asdr_tuner_position", "asdr_tuner_n_channels",
                 "asdr_tuner_n_sources", "asdr_tuner_decimation", "asdr_tuner_set_source", "asdr_tuner_set_frequency",
                 "asdr_tuner_set_frequency_word", "asdr_tuner_set_phase", "asdr_tuner_set_filter", "asdr_tuner_get_filter",
                 "asdr_tuner_read_state", "asdr_tuner_update_device", "asdr_tuner_update", "asdr_tuner_synchronize",
                 "asdr_tuner_last_kernel_ms"]

TUNER_STATE_DTYPE = np.dtype([("src", "<i4"), ("fw", "<u4"), ("pos_a", "<i8"), ("ph_a", "<u4"), ("reserved", "<u4")])
assert TUNER_STATE_DTYPE.itemsize == 24

_typed = False


def _lib():
    global _typed
    L = load_library()
    if _typed:
        return L
    vp, i, u32, lg, i16p = C.c_void_p, C.c_int, C.c_uint32, C.c_long, C.POINTER(C.c_int16)
    L.asdr_tuner_create.argtypes = [i, i, i, i]; L.asdr_tuner_create.restype = vp
    L.asdr_tuner_destroy.argtypes = [vp]; L.asdr_tuner_destroy.restype = None
    for n in ("reset", "n_channels", "n_sources", "decimation", "synchronize"):
        getattr(L, "asdr_tuner_" + n).argtypes = [vp]; getattr(L, "asdr_tuner_" + n).restype = i
    L.asdr_tuner_position.argtypes = [vp]; L.asdr_tuner_position.restype = C.c_longlong
    L.asdr_tuner_set_source.argtypes = [vp, i, i]; L.asdr_tuner_set_source.restype = i
    L.asdr_tuner_set_frequency.argtypes = [vp, i, C.c_double]; L.asdr_tuner_set_frequency.restype = i
    L.asdr_tuner_set_frequency_word.argtypes = [vp, i, u32]; L.asdr_tuner_set_frequency_word.restype = i
    L.asdr_tuner_set_phase.argtypes = [vp, i, u32]; L.asdr_tuner_set_phase.restype = i
    L.asdr_tuner_set_filter.argtypes = [vp, i16p, i, i]; L.asdr_tuner_set_filter.restype = i
    L.asdr_tuner_get_filter.argtypes = [vp, i16p, i, C.POINTER(C.c_int)]; L.asdr_tuner_get_filter.restype = i
    L.asdr_tuner_read_state.argtypes = [vp, vp]; L.asdr_tuner_read_state.restype = i
    L.asdr_tuner_update_device.argtypes = [vp, vp, lg, vp, vp, i, lg, vp]; L.asdr_tuner_update_device.restype = i
    L.asdr_tuner_update.argtypes = [vp, i16p, i16p, i16p, i]; L.asdr_tuner_update.restype = i
    L.asdr_tuner_last_kernel_ms.argtypes = [vp]; L.asdr_tuner_last_kernel_ms.restype = C.c_float
    _typed = True
    return L


def _p16(a):
    return a.ctypes.data_as(C.POINTER(C.c_int16))


class TunerBank:
    """n_channels digital tuners over n_sources shared CS16 rows at decimation D (include/asdr_tuner.h).  device = NO_DEVICE (-1)
    gives the control plane only."""

    def __init__(self, n_channels, n_sources=1, decimation=1, device=0):
        self._L = _lib()
        self._h = self._L.asdr_tuner_create(int(n_channels), int(n_sources), int(decimation), int(device))
        if not self._h:
            raise AsdrError("asdr_tuner_create failed: %s" % self._L.asdr_last_error().decode())
        self.n_channels, self.n_sources, self.decimation = int(n_channels), int(n_sources), int(decimation)

    def close(self):
        if getattr(self, "_h", None):
            self._L.asdr_tuner_destroy(self._h)
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

    def reset(self):
        self._chk(self._L.asdr_tuner_reset(self._h))

    def position(self):
        return int(self._L.asdr_tuner_position(self._h))

    def set_source(self, source, ch=ALL):
        self._chk(self._L.asdr_tuner_set_source(self._h, int(ch), int(source)))

    def set_frequency(self, hz, ch=ALL):
        self._chk(self._L.asdr_tuner_set_frequency(self._h, int(ch), float(hz)))

    def set_frequency_word(self, fw, ch=ALL):
        self._chk(self._L.asdr_tuner_set_frequency_word(self._h, int(ch), int(fw) & 0xFFFFFFFF))

    def set_phase(self, phase, ch=ALL):
        self._chk(self._L.asdr_tuner_set_phase(self._h, int(ch), int(phase) & 0xFFFFFFFF))

    def set_filter(self, h, gain_shift=0):
        h = np.ascontiguousarray(h, dtype=np.int16)
        self._chk(self._L.asdr_tuner_set_filter(self._h, _p16(h), int(h.size), int(gain_shift)))

    def get_filter(self):
        """(h int16 [L], gain_shift)."""
        n = self._chk(self._L.asdr_tuner_get_filter(self._h, None, 0, None))
        h, g = np.zeros(n, dtype=np.int16), C.c_int()
        self._chk(self._L.asdr_tuner_get_filter(self._h, _p16(h), n, C.byref(g)))
        return h, int(g.value)

    def read_state(self):
        """numpy structured array [n_channels] of asdr_tuner_state_t (src, fw, pos_a, ph_a)."""
        st = np.zeros(self.n_channels, dtype=TUNER_STATE_DTYPE)
        self._chk(self._L.asdr_tuner_read_state(self._h, st.ctypes.data_as(C.c_void_p)))
        return st

    def update(self, iq):
        """iq: int16 [n_sources][n_blocks * 128 * D][2] (re, im) on the host.  Returns (I, Q), int16 [n_channels][n_blocks][128]."""
        iq = np.ascontiguousarray(iq, dtype=np.int16)
        per = BLOCK * self.decimation
        assert iq.shape[0] == self.n_sources and iq.shape[-1] == 2 and iq.shape[1] % per == 0, iq.shape
        nb = iq.shape[1] // per
        I = np.empty((self.n_channels, nb, BLOCK), dtype=np.int16)
        Q = np.empty_like(I)
        self._chk(self._L.asdr_tuner_update(self._h, _p16(iq), _p16(I), _p16(Q), nb))
        return I, Q

    def update_device(self, dIQ, dI, dQ, n_blocks, in_stride_samples=None, out_stride_blocks=None, stream=0):
        """Device pointers (ints); asynchronous on `stream`.  Strides default to contiguous rows."""
        ins = in_stride_samples or n_blocks * BLOCK * self.decimation
        self._chk(self._L.asdr_tuner_update_device(self._h, C.c_void_p(dIQ), int(ins), C.c_void_p(dI), C.c_void_p(dQ), int(n_blocks),
                                                   int(out_stride_blocks or n_blocks), C.c_void_p(stream)))

    def synchronize(self):
        self._chk(self._L.asdr_tuner_synchronize(self._h))

    def last_kernel_ms(self):
        return float(self._L.asdr_tuner_last_kernel_ms(self._h))
