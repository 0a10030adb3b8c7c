"""ctypes mirror of include/asdr_fm.h: the FM demodulator (narrow-band FM audio from a tuner bank's int16 I/Q rows: an integer CORDIC
discriminator, DC removal, de-emphasis and a noise squelch that mutes closed channels in the rows it writes).  Same rules as
binding.py: the work happens in libasdr_hip.so on the GPU; there is no CPU fallback (tests/fm_ref.py is the independent numpy
statement the tests compare with)."""
import ctypes as C

import numpy as np

from ._stage import RecordStage, _c_int, _stride, i, ip, lg, typed_library, vp
from .binding import ALL, AsdrError

FM_EXPORTS = ["asdr_fm_create", "asdr_fm_destroy", "asdr_fm_n_channels", "asdr_fm_set_gain", "asdr_fm_get_gain", "asdr_fm_set_deemphasis",
              "asdr_fm_get_deemphasis", "asdr_fm_set_dc_shift", "asdr_fm_get_dc_shift", "asdr_fm_set_squelch", "asdr_fm_get_squelch",
              "asdr_fm_gain_from_deviation", "asdr_fm_deemphasis_from_tau_us", "asdr_fm_update_device", "asdr_fm_read_state",
              "asdr_fm_write_state", "asdr_fm_clear", "asdr_fm_reset", "asdr_fm_blocks", "asdr_fm_synchronize"]

FM_STATE_DTYPE = np.dtype([("prev_i", "<i2"), ("prev_q", "<i2"), ("v1", "<i2"), ("v2", "<i2"), ("s", "<i4"), ("m", "<i4"),
                           ("last_noise", "<u8"), ("last_power", "<u8"), ("openings", "<u4"), ("open_blocks", "<u4"),
                           ("hang_left", "<u2"), ("open", "u1"), ("reserved", "u1"), ("reserved2", "<u4")])
assert FM_STATE_DTYPE.itemsize == 48
FM_ROWS = 64             # channels per workgroup (ASDR_FM_ROWS) ...
FM_NARROW_ROWS = 16      # ... and in a bank below FM_WIDE_CHANNELS channels (ASDR_FM_NARROW_ROWS, ASDR_FM_WIDE_CHANNELS)
FM_WIDE_CHANNELS = 32768
FM_CHUNK_BLOCKS = 1      # blocks of a row staged in LDS at a time (ASDR_FM_CHUNK_BLOCKS)
FM_MAX_NOISE = 1 << 41

_u32, _u64, _u32p, _u64p = C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_API = {"create": ([i, i], vp), "destroy": ([vp], None), "n_channels": ([vp], i), "clear": ([vp], i), "reset": ([vp], i),
        "synchronize": ([vp], i), "set_gain": ([vp, i, _u32], i), "get_gain": ([vp, i, _u32p], i),
        "set_deemphasis": ([vp, i, _u32], i), "get_deemphasis": ([vp, i, _u32p], i), "set_dc_shift": ([vp, i, i], i),
        "get_dc_shift": ([vp, i, ip], i), "set_squelch": ([vp, i, _u64, _u64, i], i), "get_squelch": ([vp, i, _u64p, _u64p, ip], i),
        "gain_from_deviation": ([C.c_double], _u32), "deemphasis_from_tau_us": ([C.c_double], _u32),
        "update_device": ([vp, vp, vp, lg, vp, lg, i, vp], i), "read_state": ([vp, vp], i), "write_state": ([vp, ip, i, vp], i),
        "blocks": ([vp], C.c_longlong)}


def _lib():
    return typed_library("asdr_fm_", _API)


def _helper(name, x):
    L = _lib()
    v = int(getattr(L, "asdr_fm_" + name)(float(x)))
    if v == 0:
        raise AsdrError(L.asdr_last_error().decode())
    return v


def fm_gain_from_deviation(hz):
    """asdr_fm_gain_from_deviation: floor(32767 * 44100 / (2 hz) + 0.5), the gain at which a deviation of hz is full scale."""
    return _helper("gain_from_deviation", hz)


def fm_deemphasis_from_tau_us(tau_us):
    """asdr_fm_deemphasis_from_tau_us: floor(32768 * (1 - exp(-1e6 / (44100 tau_us))) + 0.5), the Q15 coefficient."""
    return _helper("deemphasis_from_tau_us", tau_us)


class FmDemodulator(RecordStage):
    """FM demodulators of n_channels tuner channels (include/asdr_fm.h).  device = NO_DEVICE (-1) gives the control plane and the
    state records only."""
    _prefix = "asdr_fm_"
    _state_dtype = FM_STATE_DTYPE

    def __init__(self, n_channels, device=0):
        self._L = _lib()
        self._create("asdr_fm_create", self._L.asdr_fm_create(int(n_channels), int(device)))
        self.n_channels = int(n_channels)

    # settings: of a channel, or of every channel; from the next call
    def set_gain(self, gain, ch=ALL):
        """G in 1 .. 2^24: v = theta * G >> 31."""
        g = int(gain)
        if not 0 <= g < 2**32:
            raise AsdrError("gain must be in 1..2^24")
        self._chk(self._L.asdr_fm_set_gain(self._h, int(ch), g))

    def get_gain(self, ch=0):
        g = C.c_uint32()
        self._chk(self._L.asdr_fm_get_gain(self._h, int(ch), C.byref(g)))
        return int(g.value)

    def set_deviation(self, hz, ch=ALL):
        """The gain at which a deviation of hz is full scale (fm_gain_from_deviation)."""
        self.set_gain(fm_gain_from_deviation(hz), ch=ch)

    def set_deemphasis(self, a=None, ch=ALL, tau_us=None):
        """The Q15 coefficient a in 1 .. 32768 (32768: bypass), or tau_us = the time constant in microseconds."""
        if (a is None) == (tau_us is None):
            raise AsdrError("set_deemphasis: give a or tau_us")
        a = fm_deemphasis_from_tau_us(tau_us) if a is None else int(a)
        if not 0 <= a < 2**32:
            raise AsdrError("de-emphasis coefficient must be in 1..32768")
        self._chk(self._L.asdr_fm_set_deemphasis(self._h, int(ch), a))

    def get_deemphasis(self, ch=0):
        a = C.c_uint32()
        self._chk(self._L.asdr_fm_get_deemphasis(self._h, int(ch), C.byref(a)))
        return int(a.value)

    def set_dc_shift(self, hp_shift, ch=ALL):
        """hp_shift in 0 .. 15: the DC remover's time constant is 2^hp_shift samples; 0 turns it off."""
        self._chk(self._L.asdr_fm_set_dc_shift(self._h, int(ch), _c_int(hp_shift, "hp_shift must be in 0..15")))

    def get_dc_shift(self, ch=0):
        k = C.c_int()
        self._chk(self._L.asdr_fm_get_dc_shift(self._h, int(ch), C.byref(k)))
        return int(k.value)

    def set_squelch(self, open_noise=FM_MAX_NOISE, close_noise=None, hang_blocks=0, ch=ALL):
        """The noise squelch: a block with N <= open_noise opens, an open channel holds up to close_noise (default: open_noise) and
        for hang_blocks blocks above it.  The defaults are the creation values: always open."""
        o = int(open_noise)
        c = o if close_noise is None else int(close_noise)
        if not (0 <= o < 2**64 and 0 <= c < 2**64):
            raise AsdrError("the noise thresholds must not exceed 2^41")
        self._chk(self._L.asdr_fm_set_squelch(self._h, int(ch), o, c, _c_int(hang_blocks, "hang_blocks must be in 0..65535")))

    def get_squelch(self, ch=0):
        """(open_noise, close_noise, hang_blocks) of a channel."""
        o, c, h = C.c_uint64(), C.c_uint64(), C.c_int()
        self._chk(self._L.asdr_fm_get_squelch(self._h, int(ch), C.byref(o), C.byref(c), C.byref(h)))
        return int(o.value), int(c.value), int(h.value)

    # the pass
    def update_device(self, i_ptr, q_ptr, out_ptr, n_blocks, in_stride_blocks=None, out_stride_blocks=None, stream=0):
        """Raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle as int).  i_ptr, q_ptr: int16 rows
        [n_channels][in_stride_blocks][128]; out_ptr: int16 rows [n_channels][out_stride_blocks][128]; the strides default to
        n_blocks."""
        si = _stride(in_stride_blocks, n_blocks)
        so = _stride(out_stride_blocks, n_blocks)
        self._chk(self._L.asdr_fm_update_device(self._h, C.c_void_p(i_ptr), C.c_void_p(q_ptr), si, C.c_void_p(out_ptr), so, int(n_blocks),
                                                C.c_void_p(stream or None)))

    # state (read_state, write_state, clear, blocks: RecordStage)
    def offset_hz(self, deviation_hz):
        """The tuning offset of every channel in Hz, float64 [n_channels], from the DC meter m (hp_shift > 0): m / 2^15 is the mean
        of v, and v = 32767 at deviation_hz, the deviation the channel's gain was set for."""
        return self.read_state()["m"].astype(np.float64) / 32768.0 / 32767.0 * float(deviation_hz)
