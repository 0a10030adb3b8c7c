"""ctypes mirror of include/asdr_resample.h: the audio resampler (the receivers' 44.1 kHz int16 audio rows at a decoder's rate such
as 12 kHz, for every channel or for the channels a gate delivered).  Same rules as binding.py: the work happens in libasdr_hip.so
on the GPU; there is no CPU fallback (tests/resample_ref.py is the independent numpy statement the tests compare with)."""
import ctypes as C

import numpy as np

from ._stage import RecordStage, _stride, i, ip, lg, ll, typed_library, vp
from .binding import AsdrError

RESAMPLE_EXPORTS = ["asdr_resampler_create", "asdr_resampler_create_custom", "asdr_resampler_destroy", "asdr_resampler_n_channels",
                    "asdr_resampler_up", "asdr_resampler_down", "asdr_resampler_taps_per_phase", "asdr_resampler_get_taps",
                    "asdr_resampler_delay", "asdr_resampler_set_filter", "asdr_resampler_position", "asdr_resampler_output_position",
                    "asdr_resampler_out_samples", "asdr_resampler_set_position", "asdr_resampler_update_device",
                    "asdr_resampler_read_state", "asdr_resampler_write_state", "asdr_resampler_reset", "asdr_resampler_synchronize"]

RESAMPLE_FS_IN = 44100
RESAMPLE_STATE_SAMPLES = 256     # int16 per channel record (ASDR_RESAMPLE_STATE_SAMPLES)
RESAMPLE_DEFAULT_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000)   # the rates of the header's table

_API = {"create": ([i, i, i], vp), "create_custom": ([i, i, i, i, vp, i, i], vp), "destroy": ([vp], None), "n_channels": ([vp], i),
        "up": ([vp], i), "down": ([vp], i), "taps_per_phase": ([vp], i), "reset": ([vp], i), "synchronize": ([vp], i),
        "get_taps": ([vp, vp, ip], i), "delay": ([vp], C.c_double), "set_filter": ([vp, i, vp, i], i), "position": ([vp], ll),
        "output_position": ([vp], ll), "out_samples": ([vp, i], lg), "set_position": ([vp, ll], i),
        "update_device": ([vp, vp, lg, i, vp, lg, vp, vp, i, vp], lg), "read_state": ([vp, vp], i), "write_state": ([vp, ip, i, vp], i)}


def _lib():
    return typed_library("asdr_resampler_", _API)


def _taps_array(taps, up):
    t = np.ascontiguousarray(taps, dtype=np.int64).reshape(-1)
    if t.size == 0 or (int(up) >= 1 and t.size % int(up)) or t.min() < -32768 or t.max() > 32767:
        raise AsdrError("the taps must be int16, up * taps_per_phase of them")
    return t.astype(np.int16)


class AudioResampler(RecordStage):
    """Resampler of n_channels receivers' audio rows from 44.1 kHz to fs_out (include/asdr_resample.h).  Either fs_out (the default
    filter of that rate) or up, down, taps [up * K] as h[k * up + phi] and shift (a custom filter).  device = NO_DEVICE (-1) gives
    the control plane and the state records only."""
    _prefix = "asdr_resampler_"
    _state_dtype = np.int16

    def _record_shape(self):           # a record: the channel's last 256 input samples, oldest first
        return (RESAMPLE_STATE_SAMPLES,)

    def __init__(self, n_channels, fs_out=12000, device=0, up=None, down=None, taps=None, shift=15):
        self._L = _lib()
        if taps is None:
            if up is not None or down is not None:
                raise AsdrError("AudioResampler: up / down come with custom taps")
            self._create("asdr_resampler_create", self._L.asdr_resampler_create(int(n_channels), int(fs_out), int(device)))
        else:
            t = _taps_array(taps, up)
            self._create("asdr_resampler_create_custom",
                         self._L.asdr_resampler_create_custom(int(n_channels), int(up), int(down), t.size // max(int(up), 1),
                                                              t.ctypes.data_as(C.c_void_p), int(shift), int(device)))
        self.n_channels = int(n_channels)
        self.up, self.down = int(self._L.asdr_resampler_up(self._h)), int(self._L.asdr_resampler_down(self._h))

    # the rate and the filter
    @property
    def fs_out(self):
        """44100 up / down, as a float (exact for the default rates)."""
        return RESAMPLE_FS_IN * self.up / self.down

    def taps_per_phase(self):
        return int(self._chk(self._L.asdr_resampler_taps_per_phase(self._h)))

    def get_taps(self):
        """(taps int16 [up * K] as h[k * up + phi], shift)."""
        t = np.zeros(self.up * self.taps_per_phase(), dtype=np.int16)
        s = C.c_int(0)
        self._chk(self._L.asdr_resampler_get_taps(self._h, t.ctypes.data_as(C.c_void_p), C.byref(s)))
        return t, int(s.value)

    def delay(self):
        """The causal filter's delay in input samples, (up * K - 1) / (2 up)."""
        return float(self._L.asdr_resampler_delay(self._h))

    def set_filter(self, taps, shift=15):
        """Swaps the filter (same up and down); the records and the position stay."""
        t = _taps_array(taps, self.up)
        self._chk(self._L.asdr_resampler_set_filter(self._h, t.size // self.up, t.ctypes.data_as(C.c_void_p), int(shift)))

    # position
    def position(self):
        return int(self._L.asdr_resampler_position(self._h))

    def output_position(self):
        return int(self._L.asdr_resampler_output_position(self._h))

    def out_samples(self, n_blocks):
        """What the next update_device of n_blocks blocks returns."""
        return int(self._chk(self._L.asdr_resampler_out_samples(self._h, int(n_blocks))))

    def set_position(self, n):
        if not -2**63 <= int(n) < 2**63:
            raise AsdrError("resampler: position must be in 0..2^50")
        self._chk(self._L.asdr_resampler_set_position(self._h, int(n)))

    # the pass
    def update_device(self, ptr, n_blocks, out_ptr, out_stride, stride_blocks=None, index_ptr=0, count_ptr=0, capacity_rows=0, stream=0):
        """Raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle as int).  ptr: int16 rows
        [n_channels][stride_blocks][128] (stride_blocks defaults to n_blocks); out_ptr: int16 rows [..][out_stride].  With index_ptr /
        count_ptr (device int32 [..] and int32, e.g. a gate's index_tensor().data_ptr() / count_tensor().data_ptr()) row i is channel
        index[i] for i < min(count, capacity_rows); otherwise row c is channel c.  Returns the per-row output count."""
        stride = _stride(stride_blocks, n_blocks)
        return int(self._chk(self._L.asdr_resampler_update_device(self._h, C.c_void_p(ptr or None), stride, int(n_blocks), C.c_void_p(out_ptr or None),
                                                                  int(out_stride), C.c_void_p(index_ptr or None), C.c_void_p(count_ptr or None),
                                                                  int(capacity_rows), C.c_void_p(stream or None))))
