"""ctypes mirror of include/asdr_tone.h: the tone squelch (CTCSS decode, tone squelch and a sub-audible high-pass on the int16 audio
rows the FM demodulator writes: a decimating CIC, a correlator bank over a table of up to 64 tones, a biquad cascade, and a
per-window verdict that mutes the channels whose tone is not the wanted one).  Same rules as binding.py: the work happens in
libasdr_hip.so on the GPU; there is no CPU fallback (tests/tone_ref.py is the independent numpy statement the tests compare
with)."""
import ctypes as C

import numpy as np

from ._stage import RecordStage, _c_int, _stride, i, ip, lg, typed_library, vp
from .binding import ALL, AsdrError

TONE_EXPORTS = ["asdr_tone_create", "asdr_tone_destroy", "asdr_tone_n_channels", "asdr_tone_set_tones", "asdr_tone_get_tones",
                "asdr_tone_set_window", "asdr_tone_get_window", "asdr_tone_set_dominance", "asdr_tone_get_dominance",
                "asdr_tone_set_highpass", "asdr_tone_get_highpass", "asdr_tone_highpass_design", "asdr_tone_min_power",
                "asdr_tone_set_want", "asdr_tone_get_want", "asdr_tone_set_min_power", "asdr_tone_get_min_power", "asdr_tone_set_hang",
                "asdr_tone_get_hang", "asdr_tone_update_device", "asdr_tone_read_state", "asdr_tone_write_state", "asdr_tone_clear",
                "asdr_tone_reset", "asdr_tone_blocks", "asdr_tone_synchronize"]

TONE_STATE_DTYPE = np.dtype([("hist", "<i2", (48,)), ("hp", "<i4", (3, 4)), ("last_power", "<u8"), ("last_other", "<u8"),
                             ("windows", "<u4"), ("matches", "<u4"), ("openings", "<u4"), ("open_blocks", "<u4"), ("detected", "<i2"),
                             ("last_best", "<i2"), ("window_block", "<u2"), ("hang_left", "u1"), ("open", "u1"), ("reserved", "<u4", (2,)),
                             ("acc", "<i4", (64, 2))])
assert TONE_STATE_DTYPE.itemsize == 704
# the 50 standard CTCSS tones in Hz (ASDR_CTCSS_TONES): the creation table
CTCSS_TONES = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0,
               127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2,
               189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1)
TONE_PASS, TONE_ANY = -2, -1   # ASDR_TONE_PASS, ASDR_TONE_ANY
TONE_ROWS = 16                 # channels per workgroup (ASDR_TONE_ROWS) ...
TONE_WAVE_ROWS = 4             # ... and per wave in the correlation (ASDR_TONE_WAVE_ROWS)
TONE_MAX_TONES = 64

_u32p, _u64, _u64p, _dp, _i32p = C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_int32)
_API = {"create": ([i, i], vp), "destroy": ([vp], None), "n_channels": ([vp], i), "clear": ([vp], i), "reset": ([vp], i),
        "synchronize": ([vp], i), "set_tones": ([vp, _dp, i], i), "get_tones": ([vp, _dp, _u32p], i), "set_window": ([vp, i], i),
        "get_window": ([vp], i), "set_dominance": ([vp, i], i), "get_dominance": ([vp], i), "set_highpass": ([vp, _i32p, i], i),
        "get_highpass": ([vp, _i32p], i), "highpass_design": ([C.c_double, i, _i32p], i), "min_power": ([C.c_double, i], _u64),
        "set_want": ([vp, i, i], i), "get_want": ([vp, i, ip], i), "set_min_power": ([vp, i, _u64], i),
        "get_min_power": ([vp, i, _u64p], i), "set_hang": ([vp, i, i], i), "get_hang": ([vp, i, ip], i),
        "update_device": ([vp, vp, lg, vp, lg, i, vp], i), "read_state": ([vp, vp], i), "write_state": ([vp, ip, i, vp], i),
        "blocks": ([vp], C.c_longlong)}


def _lib():
    return typed_library("asdr_tone_", _API)


def tone_highpass_design(fc_hz, sections):
    """asdr_tone_highpass_design: the Q28 coefficients (b0, b1, b2, a1, a2) of the bilinear Butterworth high-pass of order
    2 sections at 44.1 kHz, int32 [sections][5]."""
    L = _lib()
    n = _c_int(sections, "sections must be in 0..3")
    out = np.zeros((max(min(n, 3), 0), 5), dtype=np.int32)
    if L.asdr_tone_highpass_design(float(fc_hz), n, out.ctypes.data_as(_i32p)) < 0:
        raise AsdrError(L.asdr_last_error().decode())
    return out


def tone_min_power(amplitude, window_blocks):
    """asdr_tone_min_power: floor((128 amplitude W)^2 / 4), a quarter of the power a tone of that amplitude gives over W blocks."""
    L = _lib()
    a, w = float(amplitude), _c_int(window_blocks, "window must be in 16..128")
    v = int(L.asdr_tone_min_power(a, w))
    if v == 0 and not (16 <= w <= 128 and 0.0 <= a <= 32768.0):       # 0 is also the answer for a tiny amplitude
        raise AsdrError(L.asdr_last_error().decode())
    return v


class ToneSquelch(RecordStage):
    """Tone squelches of n_channels audio rows (include/asdr_tone.h).  device = NO_DEVICE (-1) gives the control plane and the state
    records only."""
    _prefix = "asdr_tone_"
    _state_dtype = TONE_STATE_DTYPE

    def __init__(self, n_channels, device=0):
        self._L = _lib()
        self._create("asdr_tone_create", self._L.asdr_tone_create(int(n_channels), int(device)))
        self.n_channels = int(n_channels)

    # bank-wide settings: from the next call
    def set_tones(self, hz):
        """The tone table: 1 .. 64 frequencies in Hz, strictly ascending, below 1378.  Starts every channel's window again."""
        f = np.ascontiguousarray(hz, dtype=np.float64).reshape(-1)
        self._chk(self._L.asdr_tone_set_tones(self._h, f.ctypes.data_as(_dp), int(f.size)))

    def get_tones(self):
        """(hz float64 [n_tones], steps uint32 [n_tones])."""
        f, s = np.zeros(TONE_MAX_TONES, dtype=np.float64), np.zeros(TONE_MAX_TONES, dtype=np.uint32)
        n = self._chk(self._L.asdr_tone_get_tones(self._h, f.ctypes.data_as(_dp), s.ctypes.data_as(_u32p)))
        return f[:n], s[:n]

    def set_window(self, window_blocks):
        """W in 16 .. 128 blocks.  Starts every channel's window again."""
        self._chk(self._L.asdr_tone_set_window(self._h, _c_int(window_blocks, "window must be in 16..128")))

    def get_window(self):
        return self._chk(self._L.asdr_tone_get_window(self._h))

    def set_dominance(self, dominance_q4):
        """Q4, 16 .. 1024: the best tone must carry dominance / 16 times the power of the strongest tone that is not its neighbour."""
        self._chk(self._L.asdr_tone_set_dominance(self._h, _c_int(dominance_q4, "dominance must be in 16..1024")))

    def get_dominance(self):
        return self._chk(self._L.asdr_tone_get_dominance(self._h))

    def set_highpass(self, coefficients=None, fc_hz=None, sections=None):
        """int32 Q28 coefficients [sections][5] (none, or an empty list: an exact pass), or fc_hz and sections for
        tone_highpass_design."""
        if fc_hz is not None:
            coefficients = tone_highpass_design(fc_hz, 3 if sections is None else sections)
        c = np.zeros((0, 5), dtype=np.int32) if coefficients is None else np.asarray(coefficients)
        if c.size and (c.ndim != 2 or c.shape[1] != 5 or np.any(c != c.astype(np.int32))):
            raise AsdrError("set_highpass: coefficients must be int32 [sections][5]")
        c = np.ascontiguousarray(c, dtype=np.int32).reshape(-1, 5)
        self._chk(self._L.asdr_tone_set_highpass(self._h, c.ctypes.data_as(_i32p), int(c.shape[0])))

    def get_highpass(self):
        """int32 [sections][5]."""
        c = np.zeros((3, 5), dtype=np.int32)
        n = self._chk(self._L.asdr_tone_get_highpass(self._h, c.ctypes.data_as(_i32p)))
        return c[:n]

    # per-channel settings: of a channel, or of every channel; from the next call
    def set_want(self, want, ch=ALL):
        """TONE_PASS (-2): never muted; TONE_ANY (-1): any detected tone opens; 0 .. n_tones - 1: only that tone opens."""
        self._chk(self._L.asdr_tone_set_want(self._h, int(ch), _c_int(want, "want must be ASDR_TONE_PASS, ASDR_TONE_ANY or a tone of the table")))

    def get_want(self, ch=0):
        w = C.c_int()
        self._chk(self._L.asdr_tone_get_want(self._h, int(ch), C.byref(w)))
        return int(w.value)

    def set_min_power(self, min_power, ch=ALL):
        p = int(min_power)
        if not 0 <= p < 2**64:
            raise AsdrError("min_power must be in 0..2^64-1")
        self._chk(self._L.asdr_tone_set_min_power(self._h, int(ch), p))

    def get_min_power(self, ch=0):
        p = C.c_uint64()
        self._chk(self._L.asdr_tone_get_min_power(self._h, int(ch), C.byref(p)))
        return int(p.value)

    def set_hang(self, hang_windows, ch=ALL):
        self._chk(self._L.asdr_tone_set_hang(self._h, int(ch), _c_int(hang_windows, "hang_windows must be in 0..255")))

    def get_hang(self, ch=0):
        h = C.c_int()
        self._chk(self._L.asdr_tone_get_hang(self._h, int(ch), C.byref(h)))
        return int(h.value)

    # the pass
    def update_device(self, in_ptr, out_ptr, n_blocks, in_stride_blocks=None, out_stride_blocks=None, stream=0):
        """Raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle as int).  in_ptr: int16 rows
        [n_channels][in_stride_blocks][128]; out_ptr: int16 rows [n_channels][out_stride_blocks][128]; the strides default to
        n_blocks."""
        si = _stride(in_stride_blocks, n_blocks)
        so = _stride(out_stride_blocks, n_blocks)
        self._chk(self._L.asdr_tone_update_device(self._h, C.c_void_p(in_ptr), si, C.c_void_p(out_ptr), so, int(n_blocks),
                                                  C.c_void_p(stream or None)))

    # state (read_state, write_state, clear, blocks: RecordStage)
    def decoded_hz(self):
        """The table frequency of every channel's `detected`, float64 [n_channels]; NaN where no tone is detected."""
        hz, _ = self.get_tones()
        d = self.read_state()["detected"].astype(np.int64)
        ok = (d >= 0) & (d < hz.size)
        return np.where(ok, hz[np.clip(d, 0, hz.size - 1)], np.nan)
