"""ctypes mirror of include/asdr_dcs.h: the DCS squelch (digital coded squelch on the int16 audio rows the FM demodulator writes: a
decimating CIC, a bit filter, a slicer with a bit clock at 134.4 bit/s, a 23-bit register scanned against a table of up to 128 Golay
words, and a verdict that mutes the channels whose code is not the wanted one).  Same rules as binding.py: the work happens in
libasdr_hip.so on the GPU; there is no CPU fallback (tests/dcs_ref.py is the independent numpy statement the tests compare with)."""
import ctypes as C

import numpy as np

from ._stage import RecordStage, _c_int, _stride, i, ip, lg, typed_library, vp
from .binding import ALL, AsdrError

DCS_EXPORTS = ["asdr_dcs_create", "asdr_dcs_destroy", "asdr_dcs_n_channels", "asdr_dcs_word", "asdr_dcs_find", "asdr_dcs_set_codes",
               "asdr_dcs_get_codes", "asdr_dcs_set_max_errors", "asdr_dcs_get_max_errors", "asdr_dcs_set_confirm", "asdr_dcs_get_confirm",
               "asdr_dcs_set_hold_bits", "asdr_dcs_get_hold_bits", "asdr_dcs_set_want", "asdr_dcs_get_want", "asdr_dcs_set_hysteresis",
               "asdr_dcs_get_hysteresis", "asdr_dcs_update_device", "asdr_dcs_read_state", "asdr_dcs_write_state", "asdr_dcs_clear",
               "asdr_dcs_reset", "asdr_dcs_blocks", "asdr_dcs_synchronize"]

DCS_STATE_DTYPE = np.dtype([("hist", "<i2", (48,)), ("dhist", "<i2", (24,)), ("sr", "<u4"), ("bits", "<u4"), ("hits", "<u4"),
                            ("detections", "<u4"), ("openings", "<u4"), ("open_blocks", "<u4"), ("edges", "<u4"), ("detected", "<i2"),
                            ("cand", "<i2"), ("clk", "<u2"), ("quiet", "<u2"), ("age", "u1"), ("run", "u1"), ("b", "u1"), ("open", "u1"),
                            ("reserved", "<u4", (2,))])
assert DCS_STATE_DTYPE.itemsize == 192
# the 104 standard DCS codes (ASDR_DCS_CODES): the creation table
DCS_CODES = (0o023, 0o025, 0o026, 0o031, 0o032, 0o036, 0o043, 0o047, 0o051, 0o053, 0o054, 0o065, 0o071, 0o072, 0o073, 0o074, 0o114, 0o115,
             0o116, 0o122, 0o125, 0o131, 0o132, 0o134, 0o143, 0o145, 0o152, 0o155, 0o156, 0o162, 0o165, 0o172, 0o174, 0o205, 0o212, 0o223,
             0o225, 0o226, 0o243, 0o244, 0o245, 0o246, 0o251, 0o252, 0o255, 0o261, 0o263, 0o265, 0o266, 0o271, 0o274, 0o306, 0o311, 0o315,
             0o325, 0o331, 0o332, 0o343, 0o346, 0o351, 0o356, 0o364, 0o365, 0o371, 0o411, 0o412, 0o413, 0o423, 0o431, 0o432, 0o445, 0o446,
             0o452, 0o454, 0o455, 0o462, 0o464, 0o465, 0o466, 0o503, 0o506, 0o516, 0o523, 0o526, 0o532, 0o546, 0o565, 0o606, 0o612, 0o624,
             0o627, 0o631, 0o632, 0o654, 0o662, 0o664, 0o703, 0o712, 0o723, 0o731, 0o732, 0o734, 0o743, 0o754)
DCS_PASS, DCS_ANY = -2, -1     # ASDR_DCS_PASS, ASDR_DCS_ANY
DCS_ROWS = 64                  # channels per workgroup in a bank of DCS_WIDE_CHANNELS channels or more (ASDR_DCS_ROWS) ...
DCS_NARROW_ROWS = 16           # ... and in a smaller bank (ASDR_DCS_NARROW_ROWS, ASDR_DCS_WIDE_CHANNELS)
DCS_WIDE_CHANNELS = 32768
DCS_MAX_CODES = 128

_u32, _u32p = C.c_uint32, C.POINTER(C.c_uint32)
_API = {"create": ([i, i], vp), "destroy": ([vp], None), "n_channels": ([vp], i), "clear": ([vp], i), "reset": ([vp], i),
        "synchronize": ([vp], i), "word": ([i], _u32), "find": ([vp, i, i], i), "set_codes": ([vp, ip, i], i),
        "get_codes": ([vp, ip, _u32p], i), "set_max_errors": ([vp, i], i), "get_max_errors": ([vp], i), "set_confirm": ([vp, i], i),
        "get_confirm": ([vp], i), "set_hold_bits": ([vp, i], i), "get_hold_bits": ([vp], i), "set_want": ([vp, i, i], i),
        "get_want": ([vp, i, ip], i), "set_hysteresis": ([vp, i, _u32], i), "get_hysteresis": ([vp, i, _u32p], i),
        "update_device": ([vp, vp, lg, vp, lg, i, vp], i), "read_state": ([vp, vp], i), "write_state": ([vp, ip, i, vp], i),
        "blocks": ([vp], C.c_longlong)}


def _lib():
    return typed_library("asdr_dcs_", _API)


def dcs_word(code):
    """asdr_dcs_word: the 23-bit word of a code (three octal digits, as an int: 0o023), parity << 12 | 0x800 | code."""
    L = _lib()
    c = _c_int(code, "code must be in 0..0777")
    w = int(L.asdr_dcs_word(c))
    if w == 0:                                                 # no code's word is 0: the data bits hold 0x800
        raise AsdrError(L.asdr_last_error().decode())
    return w


class DcsSquelch(RecordStage):
    """DCS squelches of n_channels audio rows (include/asdr_dcs.h).  device = NO_DEVICE (-1) gives the control plane and the state
    records only."""
    _prefix = "asdr_dcs_"
    _state_dtype = DCS_STATE_DTYPE

    def __init__(self, n_channels, device=0):
        self._L = _lib()
        self._create("asdr_dcs_create", self._L.asdr_dcs_create(int(n_channels), int(device)))
        self.n_channels = int(n_channels)

    def find(self, code, inverted=False):
        """The table index whose word is a rotation of the code's word, or of its complement if `inverted`; -1 if none is.  With the
        creation table find(0o023, True) == find(0o047)."""
        c = _c_int(code, "code must be in 0..0777")
        if not 0 <= c <= 0o777:
            raise AsdrError("code must be in 0..0777")
        return int(self._L.asdr_dcs_find(self._h, c, 1 if inverted else 0))

    # bank-wide settings: from the next call
    def set_codes(self, codes):
        """The code table: 1 .. 128 codes whose words differ pairwise in at least 2 max_errors + 1 bits.  Restarts every channel's
        decode; open and the counters stay."""
        try:
            c = np.asarray([_c_int(v, "code must be in 0..0777") for v in np.asarray(codes).reshape(-1).tolist()], dtype=np.int32)
        except (TypeError, ValueError):
            raise AsdrError("set_codes: codes must be integers")
        self._chk(self._L.asdr_dcs_set_codes(self._h, c.ctypes.data_as(ip), int(c.size)))

    def get_codes(self):
        """(codes int32 [n_codes], words uint32 [n_codes])."""
        c, w = np.zeros(DCS_MAX_CODES, dtype=np.int32), np.zeros(DCS_MAX_CODES, dtype=np.uint32)
        n = self._chk(self._L.asdr_dcs_get_codes(self._h, c.ctypes.data_as(ip), w.ctypes.data_as(_u32p)))
        return c[:n], w[:n]

    def set_max_errors(self, max_errors):
        """0 .. 3 bits of a word that may be wrong; refused if the table's words do not differ in 2 max_errors + 1 bits."""
        self._chk(self._L.asdr_dcs_set_max_errors(self._h, _c_int(max_errors, "max_errors must be in 0..3")))

    def get_max_errors(self):
        return self._chk(self._L.asdr_dcs_get_max_errors(self._h))

    def set_confirm(self, confirm):
        """1 .. 8 words in a row, 23 bits apart, that make a detection."""
        self._chk(self._L.asdr_dcs_set_confirm(self._h, _c_int(confirm, "confirm must be in 1..8")))

    def get_confirm(self):
        return self._chk(self._L.asdr_dcs_get_confirm(self._h))

    def set_hold_bits(self, hold_bits):
        """23 .. 1023 bits without a confirmed word after which a detection lapses."""
        self._chk(self._L.asdr_dcs_set_hold_bits(self._h, _c_int(hold_bits, "hold_bits must be in 23..1023")))

    def get_hold_bits(self):
        return self._chk(self._L.asdr_dcs_get_hold_bits(self._h))

    # per-channel settings: of a channel, or of every channel; from the next call
    def set_want(self, want, ch=ALL):
        """DCS_PASS (-2): never muted; DCS_ANY (-1): any detected code opens; 0 .. n_codes - 1: only that table entry opens."""
        self._chk(self._L.asdr_dcs_set_want(self._h, int(ch), _c_int(want, "want must be ASDR_DCS_PASS, ASDR_DCS_ANY or an entry of the table")))

    def get_want(self, ch=0):
        w = C.c_int()
        self._chk(self._L.asdr_dcs_get_want(self._h, int(ch), C.byref(w)))
        return int(w.value)

    def set_hysteresis(self, hysteresis, ch=ALL):
        h = int(hysteresis)
        if not 0 <= h < 2**32:
            raise AsdrError("hysteresis must be in 0..2^32-1")
        self._chk(self._L.asdr_dcs_set_hysteresis(self._h, int(ch), h))

    def get_hysteresis(self, ch=0):
        h = C.c_uint32()
        self._chk(self._L.asdr_dcs_get_hysteresis(self._h, int(ch), C.byref(h)))
        return int(h.value)

    # the pass
    def update_device(self, in_ptr, out_ptr, n_blocks, in_stride_blocks=None, out_stride_blocks=None, stream=0):
        """Raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle as int).  in_ptr: int16 rows
        [n_channels][in_stride_blocks][128]; out_ptr: int16 rows [n_channels][out_stride_blocks][128]; the strides default to
        n_blocks."""
        si = _stride(in_stride_blocks, n_blocks)
        so = _stride(out_stride_blocks, n_blocks)
        self._chk(self._L.asdr_dcs_update_device(self._h, C.c_void_p(in_ptr), si, C.c_void_p(out_ptr), so, int(n_blocks),
                                                 C.c_void_p(stream or None)))

    # state (read_state, write_state, clear, blocks: RecordStage)
    def decoded_codes(self):
        """The table code of every channel's `detected`, int32 [n_channels]; -1 where no code is detected."""
        codes, _ = self.get_codes()
        d = self.read_state()["detected"].astype(np.int64)
        ok = (d >= 0) & (d < codes.size)
        return np.where(ok, codes[np.clip(d, 0, codes.size - 1)], -1).astype(np.int32)
