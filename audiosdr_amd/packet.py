"""ctypes mirror of include/asdr_packet.h: the packet decoder (1200-baud Bell-202 AFSK carrying AX.25 frames on the int16 audio rows
the FM demodulator writes: a decimator by 4, 1200 / 2200 Hz correlators over one bit, a slicer with a bit clock, NRZI, HDLC framing
with the FCS, a ring of decoded frames per channel and their ascending compact delivery).  Same rules as binding.py: the work happens
in libasdr_hip.so on the GPU; there is no CPU fallback (tests/packet_ref.py is the independent numpy statement the tests compare
with)."""
import ctypes as C

import numpy as np

from ._stage import RecordStage, _stride, i, ip, lg, typed_library, vp
from .binding import ALL, AsdrError

PACKET_EXPORTS = ["asdr_packet_create", "asdr_packet_destroy", "asdr_packet_n_channels", "asdr_packet_fcs", "asdr_packet_format_address",
                  "asdr_packet_set_space_boost", "asdr_packet_get_space_boost", "asdr_packet_update_device", "asdr_packet_collect_device",
                  "asdr_packet_deliver", "asdr_packet_ring_state", "asdr_packet_read_state", "asdr_packet_write_state", "asdr_packet_clear",
                  "asdr_packet_reset", "asdr_packet_blocks", "asdr_packet_synchronize"]

PACKET_STATE_DTYPE = np.dtype([("hist", "<i2", (8,)), ("dhist", "<i2", (8,)), ("bits", "<u4"), ("edges", "<u4"), ("flags", "<u4"),
                               ("frames", "<u4"), ("crc_errors", "<u4"), ("aborts", "<u4"), ("clk", "<u2"), ("len", "<u2"), ("crc", "<u2"),
                               ("b", "u1"), ("prev", "u1"), ("sr", "u1"), ("cur", "u1"), ("nb", "u1"), ("in_frame", "u1"),
                               ("reserved", "<u4", (11,)), ("buf", "u1", (336,))])
assert PACKET_STATE_DTYPE.itemsize == 448
PACKET_FRAME_DTYPE = np.dtype([("channel", "<u4"), ("seq", "<u4"), ("block", "<u4"), ("length", "<u2"), ("flags", "<u2"),
                               ("data", "u1", (336,))])
assert PACKET_FRAME_DTYPE.itemsize == 352
PACKET_ROWS = 64               # channels per workgroup in a bank of PACKET_WIDE_CHANNELS channels or more (ASDR_PACKET_ROWS) ...
PACKET_NARROW_ROWS = 16        # ... and in a smaller bank (ASDR_PACKET_NARROW_ROWS, ASDR_PACKET_WIDE_CHANNELS)
PACKET_WIDE_CHANNELS = 32768
PACKET_MAX_RING = 16
PACKET_MAX_PAYLOAD = 330

_u32, _u32p = C.c_uint32, C.POINTER(C.c_uint32)
_API = {"create": ([i, i, i], vp), "destroy": ([vp], None), "n_channels": ([vp], i), "clear": ([vp], i), "reset": ([vp], i),
        "synchronize": ([vp], i), "fcs": ([vp, C.c_size_t], C.c_uint16), "format_address": ([vp, i, C.c_char_p, i], i),
        "set_space_boost": ([vp, i, _u32], i), "get_space_boost": ([vp, i, _u32p], i), "update_device": ([vp, vp, lg, i, vp], i),
        "collect_device": ([vp, vp, vp, i, vp], i), "deliver": ([vp, _u32p, vp, i], i), "ring_state": ([vp, vp, vp], i),
        "read_state": ([vp, vp], i), "write_state": ([vp, ip, i, vp], i), "blocks": ([vp], C.c_longlong)}


def _lib():
    return typed_library("asdr_packet_", _API)


def packet_fcs(data):
    """asdr_packet_fcs: the AX.25 frame check sequence of bytes (0x906E for b"123456789")."""
    b = bytes(data)
    return int(_lib().asdr_packet_fcs(C.c_char_p(b) if b else None, len(b)))


def packet_format_address(frame):
    """asdr_packet_format_address: "SRC>DST,PATH" of a payload's address field (bytes, or a row of PACKET_FRAME_DTYPE)."""
    L = _lib()
    if isinstance(frame, np.void) and frame.dtype == PACKET_FRAME_DTYPE:
        frame = frame["data"][:int(frame["length"])].tobytes()
    b = bytes(frame)
    out = C.create_string_buffer(128)
    if L.asdr_packet_format_address(C.c_char_p(b), len(b), out, len(out)) < 0:
        raise AsdrError(L.asdr_last_error().decode())
    return out.value.decode()


class PacketDecoder(RecordStage):
    """Packet decoders of n_channels audio rows with `ring` frame slots a channel (include/asdr_packet.h).  device = NO_DEVICE (-1)
    gives the control plane and the state records only."""
    _prefix = "asdr_packet_"
    _state_dtype = PACKET_STATE_DTYPE

    def __init__(self, n_channels, ring=4, device=0):
        self._L = _lib()
        self._create("asdr_packet_create", self._L.asdr_packet_create(int(n_channels), int(ring), int(device)))
        self.n_channels, self.ring = int(n_channels), int(ring)

    # per-channel setting: of a channel, or of every channel; from the next call
    def set_space_boost(self, space_boost, ch=ALL):
        """64 .. 4096: the weight of the 2200 Hz energy against 256 for the 1200 Hz energy."""
        b = int(space_boost)
        if not 0 <= b < 2**32:
            raise AsdrError("space_boost must be in 64..4096")
        self._chk(self._L.asdr_packet_set_space_boost(self._h, int(ch), b))

    def get_space_boost(self, ch=0):
        b = C.c_uint32()
        self._chk(self._L.asdr_packet_get_space_boost(self._h, int(ch), C.byref(b)))
        return int(b.value)

    # the pass
    def update_device(self, in_ptr, n_blocks, in_stride_blocks=None, stream=0):
        """A raw device pointer (int), asynchronous on `stream` (a hipStream_t handle as int).  in_ptr: int16 rows
        [n_channels][in_stride_blocks][128]; the stride defaults to n_blocks."""
        si = _stride(in_stride_blocks, n_blocks)
        self._chk(self._L.asdr_packet_update_device(self._h, C.c_void_p(in_ptr), si, int(n_blocks), C.c_void_p(stream or None)))

    # delivery
    def collect_device(self, count_ptr, frames_ptr, max_frames, stream=0):
        """Raw device pointers (ints), asynchronous on `stream`: a uint32 count to count_ptr and that many 352-byte slots
        (PACKET_FRAME_DTYPE) to frames_ptr, ascending by (channel, seq); at most max_frames, the rest stay for the next collect."""
        self._chk(self._L.asdr_packet_collect_device(self._h, C.c_void_p(count_ptr), C.c_void_p(frames_ptr or None), int(max_frames),
                                                     C.c_void_p(stream or None)))

    def deliver(self, max_frames=None):
        """The waiting frames, at most max_frames (default: every ring full), as a structured array of PACKET_FRAME_DTYPE; waits."""
        m = self.n_channels * self.ring if max_frames is None else int(max_frames)
        out = np.zeros(max(0, min(m, self.n_channels * self.ring)), dtype=PACKET_FRAME_DTYPE)
        n = C.c_uint32()
        self._chk(self._L.asdr_packet_deliver(self._h, C.byref(n), out.ctypes.data_as(C.c_void_p) if out.size else None, m))
        return out[:int(n.value)]

    def ring_state(self):
        """(pending uint32 [n_channels], lost uint32 [n_channels]): the frames waiting and the frames lost to overruns."""
        p, l = np.zeros(self.n_channels, dtype=np.uint32), np.zeros(self.n_channels, dtype=np.uint32)
        self._chk(self._L.asdr_packet_ring_state(self._h, p.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p)))
        return p, l
