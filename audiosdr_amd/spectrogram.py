"""ctypes mirror of include/asdr_spectrogram.h: the audio spectrogram (per-receiver STFT rows, a band of bins per frame, of int16 audio
rows on the device -- what a WSPR / FT8 decoder, a CW skimmer or an audio waterfall begins with).  Same rules as binding.py: the work
happens in libasdr_hip.so on the GPU; there is no CPU fallback (tests/spectrogram_ref.py is the independent numpy statement the
tests compare with)."""
import ctypes as C

import numpy as np

from ._stage import RecordStage, _stride, i, ip, lg, ll, typed_library, vp
from .binding import AsdrError

SPECTROGRAM_EXPORTS = ["asdr_spectrogram_create", "asdr_spectrogram_destroy", "asdr_spectrogram_n_channels", "asdr_spectrogram_n_fft",
                       "asdr_spectrogram_hop", "asdr_spectrogram_first_bin", "asdr_spectrogram_n_bins", "asdr_spectrogram_window_kind",
                       "asdr_spectrogram_output_kind", "asdr_spectrogram_get_window", "asdr_spectrogram_set_window",
                       "asdr_spectrogram_position", "asdr_spectrogram_frame_position", "asdr_spectrogram_out_frames",
                       "asdr_spectrogram_set_position", "asdr_spectrogram_update_device", "asdr_spectrogram_read_state",
                       "asdr_spectrogram_write_state", "asdr_spectrogram_reset", "asdr_spectrogram_synchronize"]

SPECTROGRAM_SIZES = (128, 256, 512, 1024, 2048, 4096, 8192)
SPECTROGRAM_WINDOWS = ("rect", "hann", "custom")      # ASDR_SPECTROGRAM_RECT / _HANN / _CUSTOM
SPECTROGRAM_KINDS = ("power", "complex")              # ASDR_SPECTROGRAM_POWER / _COMPLEX
SPECTROGRAM_MAX_SAMPLES = 1 << 24                     # per call

_API = {"create": ([i] * 8, vp), "destroy": ([vp], None), "n_channels": ([vp], i), "n_fft": ([vp], i), "hop": ([vp], i),
        "first_bin": ([vp], i), "n_bins": ([vp], i), "window_kind": ([vp], i), "output_kind": ([vp], i), "reset": ([vp], i),
        "synchronize": ([vp], i), "get_window": ([vp, vp], i), "set_window": ([vp, vp], i), "position": ([vp], ll),
        "frame_position": ([vp], ll), "out_frames": ([vp, lg], lg), "set_position": ([vp, ll], i),
        "update_device": ([vp, vp, lg, lg, vp, lg, vp, vp, i, vp], lg), "read_state": ([vp, vp], i), "write_state": ([vp, ip, i, vp], i)}


def _lib():
    return typed_library("asdr_spectrogram_", _API)


class AudioSpectrogram(RecordStage):
    """Spectrogram of n_channels receivers' int16 audio rows (include/asdr_spectrogram.h): frames of n_fft samples (a power of two in
    128 .. 8192) every hop samples (n_fft / 16 .. n_fft, default n_fft / 2), of which the bins first_bin .. first_bin + n_bins - 1
    (default: all n_fft / 2 + 1) are written per frame, as |X|^2 (kind "power") or (re, im) (kind "complex"), float32, scaled by
    1 / n_fft and not window-corrected.  window: "rect", "hann" or a float32 array [n_fft].  device = NO_DEVICE (-1) gives the control
    plane and the state records only."""
    _prefix = "asdr_spectrogram_"
    _state_dtype = np.int16

    def _record_shape(self):           # a record: the channel's last n_fft input samples, oldest first
        return (self.n_fft,)

    def __init__(self, n_channels, n_fft=8192, hop=None, first_bin=0, n_bins=None, window="hann", kind="power", device=0):
        self._L = _lib()
        custom = None
        if not isinstance(window, str):
            custom, window = window, "rect"
        if window not in SPECTROGRAM_WINDOWS[:2]:
            raise AsdrError("AudioSpectrogram: the window must be 'rect', 'hann' or an array")
        if kind not in SPECTROGRAM_KINDS:
            raise AsdrError("AudioSpectrogram: the output kind must be 'power' or 'complex'")
        n_fft = int(n_fft)
        hop = n_fft // 2 if hop is None else int(hop)
        n_bins = n_fft // 2 + 1 - int(first_bin) if n_bins is None else int(n_bins)
        if max(abs(int(n_channels)), abs(n_fft), abs(hop), abs(int(first_bin)), abs(n_bins)) >= 2**31:
            raise AsdrError("AudioSpectrogram: a parameter does not fit an int")
        self._create("asdr_spectrogram_create",
                     self._L.asdr_spectrogram_create(int(n_channels), n_fft, hop, int(first_bin), n_bins, SPECTROGRAM_WINDOWS.index(window),
                                                     SPECTROGRAM_KINDS.index(kind), int(device)))
        self.n_channels = int(n_channels)
        self.n_fft, self.hop = int(self._L.asdr_spectrogram_n_fft(self._h)), int(self._L.asdr_spectrogram_hop(self._h))
        self.first_bin, self.n_bins = int(self._L.asdr_spectrogram_first_bin(self._h)), int(self._L.asdr_spectrogram_n_bins(self._h))
        self.kind = SPECTROGRAM_KINDS[self._L.asdr_spectrogram_output_kind(self._h)]
        if custom is not None:
            try:
                self.set_window(custom)
            except AsdrError:
                self.close()
                raise

    # the parameters
    @property
    def window_kind(self):
        """'rect', 'hann', or 'custom' after set_window."""
        return SPECTROGRAM_WINDOWS[self._chk(self._L.asdr_spectrogram_window_kind(self._h))]

    @property
    def frame_floats(self):
        """float32 values per frame of an output row: n_bins, or 2 n_bins for kind 'complex'."""
        return self.n_bins * (2 if self.kind == "complex" else 1)

    def get_window(self):
        w = np.zeros(self.n_fft, dtype=np.float32)
        self._chk(self._L.asdr_spectrogram_get_window(self._h, w.ctypes.data_as(C.c_void_p)))
        return w

    def set_window(self, window):
        """A custom window, float32 [n_fft], finite values only; the records and the position stay."""
        w = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
        if w.size != self.n_fft:
            raise AsdrError("set_window: %d values for n_fft = %d" % (w.size, self.n_fft))
        self._chk(self._L.asdr_spectrogram_set_window(self._h, w.ctypes.data_as(C.c_void_p)))

    def bin_hz(self, fs):
        """The centre frequencies of the band's bins at sample rate fs, float64 [n_bins]."""
        return (self.first_bin + np.arange(self.n_bins)) * (float(fs) / self.n_fft)

    # position
    def position(self):
        return int(self._L.asdr_spectrogram_position(self._h))

    def frame_position(self):
        return int(self._L.asdr_spectrogram_frame_position(self._h))

    def out_frames(self, n_samples):
        """What the next update_device of n_samples samples returns."""
        if not 0 <= int(n_samples) < 2**62:
            raise AsdrError("n_samples must be in 0..2^24")
        return int(self._chk(self._L.asdr_spectrogram_out_frames(self._h, int(n_samples))))

    def set_position(self, t):
        if not -2**63 <= int(t) < 2**63:
            raise AsdrError("spectrogram: position must be in 0..2^50")
        self._chk(self._L.asdr_spectrogram_set_position(self._h, int(t)))

    # the pass
    def out_tensor(self, n_frames, rows=None, fill=None):
        """A torch float32 tensor on the device for update_device: [rows][n_frames][n_bins], or [..][n_bins][2] for kind 'complex'
        (rows defaults to n_channels); pass its data_ptr() and out_stride = n_frames."""
        import torch
        shape = (self.n_channels if rows is None else int(rows), int(n_frames), self.n_bins) + ((2,) if self.kind == "complex" else ())
        if fill is None:
            return torch.empty(shape, dtype=torch.float32, device="cuda")
        return torch.full(shape, float(fill), dtype=torch.float32, device="cuda")

    def update_device(self, ptr, n_samples, out_ptr, out_stride, stride_samples=None, index_ptr=0, count_ptr=0, capacity_rows=0, stream=0):
        """Raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle as int).  ptr: int16 rows
        [n_channels][stride_samples] (stride_samples defaults to n_samples); out_ptr: float32 rows [..][out_stride][frame_floats].
        With index_ptr / count_ptr (device int32 [..] and int32, e.g. a gate's index_tensor().data_ptr() / count_tensor().data_ptr())
        row i is channel index[i] for i < min(count, capacity_rows); otherwise row c is channel c.  Returns the per-row frame count."""
        stride = _stride(stride_samples, n_samples)
        return int(self._chk(self._L.asdr_spectrogram_update_device(self._h, C.c_void_p(ptr or None), stride, int(n_samples), C.c_void_p(out_ptr or None),
                                                                    int(out_stride), C.c_void_p(index_ptr or None), C.c_void_p(count_ptr or None),
                                                                    int(capacity_rows), C.c_void_p(stream or None))))
