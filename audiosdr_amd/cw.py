"""ctypes mirror of include/asdr_cw.h: the CW decoder (Morse text from a CW receiver's int16 audio rows: a mixer to the pitch, a
128-sample envelope at 1378.125 Hz, two level trackers and a key with a glitch filter, the dot / dash decision with a speed tracker,
the gaps, the Morse table, a ring of character events per channel and their ascending compact delivery).  Same rules as binding.py:
the work happens in libasdr_hip.so on the GPU; there is no CPU fallback (tests/cw_ref.py is the independent numpy statement the
tests compare with)."""
import ctypes as C

import numpy as np

from ._stage import RecordStage, _stride, i, ip, lg, typed_library, vp
from .binding import ALL, AsdrError

CW_EXPORTS = ["asdr_cw_create", "asdr_cw_destroy", "asdr_cw_n_channels", "asdr_cw_pitch_step", "asdr_cw_cos", "asdr_cw_set_pitch_step",
              "asdr_cw_set_min_power", "asdr_cw_set_glitch", "asdr_cw_set_track", "asdr_cw_get_settings", "asdr_cw_set_speed",
              "asdr_cw_update_device", "asdr_cw_collect_device", "asdr_cw_deliver", "asdr_cw_ring_state", "asdr_cw_read_state",
              "asdr_cw_write_state", "asdr_cw_clear", "asdr_cw_reset", "asdr_cw_blocks", "asdr_cw_synchronize"]

CW_STATE_DTYPE = np.dtype([("ph", "<u4"), ("prev_i", "<i4", (3,)), ("prev_q", "<i4", (3,)), ("hi", "<u4"), ("lo", "<u4"), ("D", "<u4"),
                           ("run", "<u4"), ("marks", "<u4"), ("chars", "<u4"), ("unknown", "<u4"), ("glitches", "<u4"), ("cnt", "u1"),
                           ("key", "u1"), ("sym", "u1"), ("gap", "u1"), ("reserved", "<u4", (4,))])
assert CW_STATE_DTYPE.itemsize == 80
CW_EVENT_DTYPE = np.dtype([("channel", "<u4"), ("seq", "<u4"), ("block", "<u4"), ("ch", "u1"), ("wpm", "u1"), ("sym", "u1"), ("flags", "u1")])
assert CW_EVENT_DTYPE.itemsize == 16
CW_ROWS = 64                   # channels per workgroup in a bank of CW_WIDE_CHANNELS channels or more (ASDR_CW_ROWS) ...
CW_NARROW_ROWS = 16            # ... and in a smaller bank (ASDR_CW_NARROW_ROWS, ASDR_CW_WIDE_CHANNELS)
CW_WIDE_CHANNELS = 32768
CW_MAX_RING = 64
CW_FLAG_UNKNOWN = 1

_u32, _u32p = C.c_uint32, C.POINTER(C.c_uint32)
_API = {"create": ([i, i, i], vp), "destroy": ([vp], None), "n_channels": ([vp], i), "clear": ([vp], i), "reset": ([vp], i),
        "synchronize": ([vp], i), "pitch_step": ([C.c_double], _u32), "cos": ([i], i), "set_pitch_step": ([vp, i, _u32], i),
        "set_min_power": ([vp, i, _u32], i), "set_glitch": ([vp, i, i], i), "set_track": ([vp, i, i], i),
        "get_settings": ([vp, i, _u32p, _u32p, ip, ip], i), "set_speed": ([vp, i, i], i), "update_device": ([vp, vp, lg, i, vp], i),
        "collect_device": ([vp, vp, vp, i, vp], i), "deliver": ([vp, _u32p, vp, i], i), "ring_state": ([vp, vp, vp], i),
        "read_state": ([vp, vp], i), "write_state": ([vp, ip, i, vp], i), "blocks": ([vp], C.c_longlong)}


def _lib():
    return typed_library("asdr_cw_", _API)


def cw_pitch_step(hz):
    """asdr_cw_pitch_step: the mixer's phase step per sample for a pitch of hz (100 .. 3000), floor(hz 2^32 / 44100 + 0.5)."""
    L = _lib()
    step = int(L.asdr_cw_pitch_step(float(hz)))
    if step == 0:
        raise AsdrError(L.asdr_last_error().decode())
    return step


def _u32_arg(v, what):
    v = int(v)
    if not 0 <= v < 2**32:
        raise AsdrError("%s must be in 0..4294967295" % what)
    return v


class CwDecoder(RecordStage):
    """CW decoders of n_channels audio rows with `ring` event slots a channel (include/asdr_cw.h).  device = NO_DEVICE (-1) gives
    the control plane and the state records only."""
    _prefix = "asdr_cw_"
    _state_dtype = CW_STATE_DTYPE

    def __init__(self, n_channels, ring=16, device=0):
        self._L = _lib()
        self._create("asdr_cw_create", self._L.asdr_cw_create(int(n_channels), int(ring), int(device)))
        self.n_channels, self.ring = int(n_channels), int(ring)

    # per-channel settings: of a channel, or of every channel; from the next call
    def set_pitch_step(self, pitch_step, ch=ALL):
        """The mixer's phase step per sample (cw_pitch_step(hz))."""
        self._chk(self._L.asdr_cw_set_pitch_step(self._h, int(ch), _u32_arg(pitch_step, "pitch_step")))

    def set_pitch(self, hz, ch=ALL):
        self.set_pitch_step(cw_pitch_step(hz), ch=ch)

    def set_min_power(self, min_power, ch=ALL):
        """The key can be down only when P >= min_power (P ~ A^2 / 4 for a tone of amplitude A)."""
        self._chk(self._L.asdr_cw_set_min_power(self._h, int(ch), _u32_arg(min_power, "min_power")))

    def set_glitch(self, glitch, ch=ALL):
        """1 .. 16: the envelope samples (of 1378.125 Hz) a key change must last."""
        self._chk(self._L.asdr_cw_set_glitch(self._h, int(ch), int(glitch)))

    def set_track(self, track, ch=ALL):
        """Whether the dit length D follows the marks."""
        self._chk(self._L.asdr_cw_set_track(self._h, int(ch), int(track)))

    def get_settings(self, ch=0):
        """(pitch_step, min_power, glitch, track)."""
        s, p, g, t = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int()
        self._chk(self._L.asdr_cw_get_settings(self._h, int(ch), C.byref(s), C.byref(p), C.byref(g), C.byref(t)))
        return int(s.value), int(p.value), int(g.value), int(t.value)

    def set_speed(self, wpm, ch=ALL):
        """5 .. 60 WPM into the record's D; waits for the handle's work."""
        self._chk(self._L.asdr_cw_set_speed(self._h, int(ch), int(wpm)))

    # the pass
    def update_device(self, in_ptr, n_blocks, in_stride_blocks=None, stream=0):
        """A raw device pointer (int), asynchronous on `stream` (a hipStream_t handle as int).  in_ptr: int16 rows
        [n_channels][in_stride_blocks][128]; the stride defaults to n_blocks."""
        si = _stride(in_stride_blocks, n_blocks)
        self._chk(self._L.asdr_cw_update_device(self._h, C.c_void_p(in_ptr), si, int(n_blocks), C.c_void_p(stream or None)))

    # delivery
    def collect_device(self, count_ptr, events_ptr, max_events, stream=0):
        """Raw device pointers (ints), asynchronous on `stream`: a uint32 count to count_ptr and that many 16-byte events
        (CW_EVENT_DTYPE) to events_ptr, ascending by (channel, seq); at most max_events, the rest stay for the next collect."""
        self._chk(self._L.asdr_cw_collect_device(self._h, C.c_void_p(count_ptr), C.c_void_p(events_ptr or None), int(max_events),
                                                 C.c_void_p(stream or None)))

    def deliver(self, max_events=None):
        """The waiting events, at most max_events (default: every ring full), as a structured array of CW_EVENT_DTYPE; waits."""
        m = self.n_channels * self.ring if max_events is None else int(max_events)
        out = np.zeros(max(0, min(m, self.n_channels * self.ring)), dtype=CW_EVENT_DTYPE)
        n = C.c_uint32()
        self._chk(self._L.asdr_cw_deliver(self._h, C.byref(n), out.ctypes.data_as(C.c_void_p) if out.size else None, m))
        return out[:int(n.value)]

    def ring_state(self):
        """(pending uint32 [n_channels], lost uint32 [n_channels]): the events waiting and the events lost to overruns."""
        p, l = np.zeros(self.n_channels, dtype=np.uint32), np.zeros(self.n_channels, dtype=np.uint32)
        self._chk(self._L.asdr_cw_ring_state(self._h, p.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p)))
        return p, l

    @staticmethod
    def text(events, channel=None):
        """The characters of the events (of one channel, if given), joined: a host helper."""
        ev = np.asarray(events)
        if channel is not None:
            ev = ev[ev["channel"] == channel]
        return ev["ch"].astype(np.uint8).tobytes().decode("ascii")
