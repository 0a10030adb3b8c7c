"""ctypes mirror of include/asdr_tuner.h: the digital tuner bank (per-receiver digital LO + decimating low-pass) that feeds
the chain's I/Q rows from shared wideband sources (CS16 by default; CU8, CS8, CF32 and real int16 by set_input_format).  Same rules as binding.py: the work happens in libasdr_hip.so on the GPU;
there is no CPU fallback (tests/tuner_ref.py is the independent numpy statement the tests compare with)."""
import ctypes as C

import numpy as np

from ._stage import ResetStage, i, ip, lg, ll, typed_library, vp
from .binding import ALL, BLOCK, AsdrError

TUNER_EXPORTS = ["asdr_tuner_create", "asdr_tuner_destroy", "asdr_tuner_reset", "asdr_tuner_position", "asdr_tuner_n_channels",
                 "asdr_tuner_n_sources", "asdr_tuner_decimation", "asdr_tuner_set_source", "asdr_tuner_set_frequency",
                 "asdr_tuner_set_frequency_word", "asdr_tuner_set_phase", "asdr_tuner_set_filter", "asdr_tuner_get_filter",
                 "asdr_tuner_read_state", "asdr_tuner_update_device", "asdr_tuner_update", "asdr_tuner_synchronize",
                 "asdr_tuner_last_kernel_ms", "asdr_tuner_create_rate", "asdr_tuner_rate", "asdr_tuner_ratio",
                 "asdr_tuner_output_position", "asdr_tuner_set_resampler", "asdr_tuner_get_resampler", "asdr_tuner_out_blocks",
                 "asdr_tuner_update_rate_device", "asdr_tuner_update_rate", "asdr_tuner_create_fastconv", "asdr_tuner_fft_size",
                 "asdr_tuner_set_channel_filter", "asdr_tuner_get_channel_filter", "asdr_tuner_set_input_format",
                 "asdr_tuner_input_format", "asdr_tuner_update_samples_device", "asdr_tuner_update_samples",
                 "asdr_tuner_spectrum_enable", "asdr_tuner_spectrum_bins", "asdr_tuner_spectrum_window", "asdr_tuner_spectrum_mode",
                 "asdr_tuner_spectrum_read", "asdr_tuner_spectrum_device", "asdr_tuner_spectrum_frames", "asdr_tuner_spectrum_clear",
                 "asdr_tuner_levels_enable", "asdr_tuner_levels_enabled", "asdr_tuner_levels_read", "asdr_tuner_levels_device",
                 "asdr_tuner_levels_frames", "asdr_tuner_levels_clear", "asdr_tuner_palette_set", "asdr_tuner_palette_get",
                 "asdr_tuner_palette_clear", "asdr_tuner_set_channel_slot", "asdr_tuner_read_slots", "asdr_tuner_set_channel_gain",
                 "asdr_tuner_read_gains", "asdr_tuner_set_iq_correction", "asdr_tuner_get_iq_correction",
                 "asdr_tuner_iq_stats_enable", "asdr_tuner_iq_stats_enabled", "asdr_tuner_iq_stats_read", "asdr_tuner_iq_stats_clear",
                 "asdr_tuner_iq_estimate", "asdr_tuner_iq_track", "asdr_tuner_condition_launches",
                 "asdr_tuner_channel_record_bytes", "asdr_tuner_channel_record_field", "asdr_tuner_export_channels",
                 "asdr_tuner_import_channels", "asdr_tuner_export_channels_device", "asdr_tuner_import_channels_device",
                 "asdr_tuner_bank_state_bytes", "asdr_tuner_export_bank_state", "asdr_tuner_import_bank_state",
                 "asdr_tuner_create_from_bank_state"]

MAX_UP = 2048
MID_RANGE = (44100, 176400)
MAX_CHANNEL_TAPS = 129
MAX_FILTERS = 64             # palette slots of a fast-convolution bank (include/asdr_tuner.h, "Filter palette and gain")
MAX_GAIN = 32768.0
CHANNEL_FILTER_BETA = 7.857  # Kaiser window of the default channel filter: 80 dB
CHANNEL_FILTER_DELTA = 0.0392   # its transition width for 129 taps, in units of Fs_mid
# input formats (include/asdr_tuner.h, "Input formats"): name -> (ASDR_TUNER_IN_*, numpy dtype, values per stored sample)
INPUT_FORMATS = {"cs16": (0, np.int16, 2), "cu8": (1, np.uint8, 2), "cs8": (2, np.int8, 2), "cf32": (3, np.float32, 2),
                 "rs16": (4, np.int16, 1)}
# monitors (include/asdr_tuner.h, "Monitors"): ASDR_TUNER_WIN_* and ASDR_TUNER_MON_* by name
SPECTRUM_WINDOWS = {"rect": 0, "hann": 1}
SPECTRUM_MODES = {"sum": 0, "peak": 1}

# source conditioning (include/asdr_tuner.h, "Source conditioning"): asdr_tuner_iq_t and asdr_tuner_iq_stats_t
IQ_CORRECTION_DTYPE = np.dtype([("dc_re", "<i4"), ("dc_im", "<i4"), ("cross_q16", "<i4"), ("gain_q16", "<i4")])
IQ_STATS_DTYPE = np.dtype([("n", "<i8"), ("sum_re", "<i8"), ("sum_im", "<i8"), ("sum_re2", "<i8"), ("sum_im2", "<i8"),
                           ("sum_reim", "<i8"), ("clipped", "<i8")])
IQ_IDENTITY = (0, 0, 0, 65536)
assert IQ_CORRECTION_DTYPE.itemsize == 16 and IQ_STATS_DTYPE.itemsize == 56

TUNER_STATE_DTYPE = np.dtype([("src", "<i4"), ("fw", "<u4"), ("pos_a", "<i8"), ("ph_a", "<u4"), ("reserved", "<u4")])
assert TUNER_STATE_DTYPE.itemsize == 24

# state records (include/asdr_tuner.h, "State records")
CHANNEL_RECORD_BYTES = 2560
_FIELD_TYPES = {"u32": "<u4", "i32": "<i4", "i64": "<i8", "f32": "<f4", "f64": "<f8"}

_u32, _sz, _d, _f, _i16p, _fp = C.c_uint32, C.c_size_t, C.c_double, C.c_float, C.POINTER(C.c_int16), C.POINTER(C.c_float)
_dp, _llp, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_int32)
_API = {"create": ([i, i, i, i], vp), "create_rate": ([i, i, ll, i, i], vp), "create_fastconv": ([i, i, ll, i, i], vp),
        "create_from_bank_state": ([vp, _sz, i, i], vp), "destroy": ([vp], None), "reset": ([vp], i), "synchronize": ([vp], i),
        "n_channels": ([vp], i), "n_sources": ([vp], i), "decimation": ([vp], i), "position": ([vp], ll), "rate": ([vp], ll),
        "ratio": ([vp, ip, ip], i), "output_position": ([vp], ll), "fft_size": ([vp], i), "last_kernel_ms": ([vp], _f),
        "set_source": ([vp, i, i], i), "set_frequency": ([vp, i, _d], i), "set_frequency_word": ([vp, i, _u32], i),
        "set_phase": ([vp, i, _u32], i), "set_filter": ([vp, _i16p, i, i], i), "get_filter": ([vp, _i16p, i, ip], i),
        "set_resampler": ([vp, _i16p, i, i], i), "get_resampler": ([vp, _i16p, i, ip], i),
        "set_channel_filter": ([vp, _fp, i], i), "get_channel_filter": ([vp, _fp, i], i), "read_state": ([vp, vp], i),
        "set_input_format": ([vp, i], i), "input_format": ([vp], i), "out_blocks": ([vp, i], i),
        "update": ([vp, _i16p, _i16p, _i16p, i], i), "update_device": ([vp, vp, lg, vp, vp, i, lg, vp], i),
        "update_rate": ([vp, _i16p, i, _i16p, _i16p, i], i), "update_rate_device": ([vp, vp, lg, i, vp, vp, i, lg, vp], i),
        "update_samples": ([vp, vp, i, _i16p, _i16p, i], i), "update_samples_device": ([vp, vp, lg, i, vp, vp, i, lg, vp], i),
        "spectrum_enable": ([vp, i, i, i], i), "spectrum_bins": ([vp], i), "spectrum_window": ([vp], i), "spectrum_mode": ([vp], i),
        "spectrum_read": ([vp, _dp, _llp, i], i), "spectrum_device": ([vp], vp), "spectrum_frames": ([vp], ll), "spectrum_clear": ([vp], i),
        "levels_enable": ([vp, i], i), "levels_enabled": ([vp], i), "levels_read": ([vp, _dp, _llp, i], i), "levels_device": ([vp], vp),
        "levels_frames": ([vp], ll), "levels_clear": ([vp], i),
        "palette_set": ([vp, i, _fp, i, i], i), "palette_get": ([vp, i, _fp, i, ip], i), "palette_clear": ([vp, i], i),
        "set_channel_slot": ([vp, i, i], i), "read_slots": ([vp, _i32p], i), "set_channel_gain": ([vp, i, _f], i), "read_gains": ([vp, _fp], i),
        "set_iq_correction": ([vp, i, vp], i), "get_iq_correction": ([vp, i, vp], i), "iq_stats_enable": ([vp, i], i),
        "iq_stats_enabled": ([vp], i), "iq_stats_read": ([vp, vp, i], i), "iq_stats_clear": ([vp], i), "iq_estimate": ([vp, vp], i),
        "iq_track": ([vp, i], i), "condition_launches": ([vp], ll),
        "channel_record_bytes": ([], _sz), "channel_record_field": ([i, ip, ip], C.c_char_p),
        "export_channels": ([vp, ip, i, vp], i), "import_channels": ([vp, ip, i, vp], i),
        "export_channels_device": ([vp, ip, i, vp, vp], i), "import_channels_device": ([vp, ip, i, vp, vp], i),
        "bank_state_bytes": ([vp], _sz), "export_bank_state": ([vp, vp, _sz], i), "import_bank_state": ([vp, vp, _sz], i)}
assert sorted("asdr_tuner_" + k for k in _API) == sorted(TUNER_EXPORTS)


def _lib():
    return typed_library("asdr_tuner_", _API)


def _p16(a):
    return a.ctypes.data_as(_i16p)


def rate_ratio(fs_in, decimation):
    """(U, M) = 44100 / (fs_in / D) in lowest terms if (fs_in, D) makes a valid rate bank (include/asdr_tuner.h), else None."""
    import math
    fs_in, D = int(fs_in), int(decimation)
    if fs_in <= 0 or not 1 <= D <= 64 or fs_in % D:
        return None
    mid = fs_in // D
    if not MID_RANGE[0] <= mid <= MID_RANGE[1]:
        return None
    g = math.gcd(44100, mid)
    return (44100 // g, mid // g) if 44100 // g <= MAX_UP else None


def suggest_decimation(fs_in):
    """The largest D <= 64 that makes a valid rate bank for fs_in (the least stage-2 work), or None."""
    for D in range(64, 0, -1):
        if rate_ratio(fs_in, D) is not None:
            return D
    return None


def fastconv_ratio(fs_in, R):
    """(U, M) = 44100 R / fs_in in lowest terms if (fs_in, R) makes a valid fast-convolution bank (include/asdr_tuner.h), else None."""
    import math
    fs_in, R = int(fs_in), int(R)
    if fs_in <= 0 or not 2 <= R <= 1024 or R & (R - 1):
        return None
    if not MID_RANGE[0] * R <= fs_in <= MID_RANGE[1] * R:
        return None
    g = math.gcd(44100 * R, fs_in)
    return (44100 * R // g, fs_in // g) if 44100 * R // g <= MAX_UP else None


def suggest_fft_decimation(fs_in):
    """The R that puts fs_in / R in [44100, 176400] with the smallest stage-2 U (ties: the larger R, the least work per channel),
    or None."""
    best = None
    for R in (1 << k for k in range(1, 11)):
        ud = fastconv_ratio(fs_in, R)
        if ud is not None and (best is None or ud[0] <= best[0]):
            best = (ud[0], R)
    return None if best is None else best[1]


def spectrum_frequencies(fs_in, n_bins):
    """Start frequency in Hz, relative to the capture's centre, of each of the n_bins output bins of the spectrum monitor (bin
    width fs_in / n_bins; FFT order: bins n_bins / 2 and up are the negative frequencies).  float64 [n_bins]."""
    n_bins = int(n_bins)
    j = np.arange(n_bins, dtype=np.float64)
    return np.where(j < n_bins // 2, j, j - n_bins) * (float(fs_in) / n_bins)


def design_channel_filter(fs_mid, lo_hz, hi_hz):
    """129 taps at fs_mid for a palette slot (TunerBank.set_palette_filter) that passes [lo_hz, hi_hz] about the tuned frequency:
    the default channel filter's design with another passband.  A low-pass prototype -- Kaiser window (beta 7.857: 80 dB), sum of
    the taps 1, cut-off (hi - lo) / 2 + fs_mid / 512 + delta / 2 with delta = 0.0392 fs_mid, the window's transition width --
    modulated to the centre (lo + hi) / 2 about tap 64.  The fs_mid / 512 on each side is there because the filter acts at a
    tone's offset from the channel's coarse bin, up to that far from its offset from the tuned frequency.  Flat over [lo, hi]
    whatever the residual tuning; 80 dB down beyond delta + fs_mid / 512 outside it.  complex64 [129]; float32 when lo = -hi.
    delta is 1.7 kHz at 44.1 kHz and 5.9 kHz at 150 kHz: this chooses among bandwidths of a few kHz and up, and sidedness."""
    fs_mid, lo, hi = float(fs_mid), float(lo_hz), float(hi_hz)
    L = MAX_CHANNEL_TAPS
    if not (fs_mid > 0 and lo < hi):
        raise AsdrError("design_channel_filter: needs fs_mid > 0 and lo_hz < hi_hz")
    fc = (0.5 * (hi - lo) + fs_mid / 512.0 + 0.5 * CHANNEL_FILTER_DELTA * fs_mid) / fs_mid
    if not (fc < 0.5 and -0.5 * fs_mid <= lo and hi <= 0.5 * fs_mid):
        raise AsdrError("design_channel_filter: [%g, %g] Hz with its transition does not fit fs_mid = %g Hz" % (lo, hi, fs_mid))
    n = np.arange(L, dtype=np.float64)
    x = n - 0.5 * (L - 1)
    u = 2.0 * n / (L - 1) - 1.0
    proto = np.where(x == 0, 2.0 * fc, np.sin(2.0 * np.pi * fc * x) / (np.pi * np.where(x == 0, 1.0, x)))
    proto = proto * np.i0(CHANNEL_FILTER_BETA * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(CHANNEL_FILTER_BETA)
    proto = proto / proto.sum()
    if lo == -hi:
        return proto.astype(np.float32)
    return (proto * np.exp(2j * np.pi * (0.5 * (lo + hi) / fs_mid) * x)).astype(np.complex64)


def estimate_iq_correction(stats):
    """asdr_tuner_iq_estimate on one source's statistics: an element of TunerBank.iq_stats(), or the seven values (n, sum_re, sum_im,
    sum_re2, sum_im2, sum_reim, clipped) in that order.  Returns the words (dc_re, dc_im, cross_q16, gain_q16); raises AsdrError
    where the estimator fails (include/asdr_tuner.h, "Source conditioning").  Host arithmetic only: no bank, no device."""
    L = _lib()
    st = np.zeros(1, dtype=IQ_STATS_DTYPE)
    vals = [stats[k] for k in IQ_STATS_DTYPE.names] if getattr(stats, "dtype", None) is not None and stats.dtype.names else list(stats)
    if len(vals) != len(IQ_STATS_DTYPE.names):
        raise AsdrError("estimate_iq_correction: needs the seven values of asdr_tuner_iq_stats_t")
    for k, v in zip(IQ_STATS_DTYPE.names, vals):
        st[k] = int(v)
    c = np.zeros(1, dtype=IQ_CORRECTION_DTYPE)
    if L.asdr_tuner_iq_estimate(st.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)) != 0:
        raise AsdrError(L.asdr_last_error().decode())
    return tuple(int(c[k][0]) for k in IQ_CORRECTION_DTYPE.names)


def tuner_channel_record_fields():
    """{name: (numpy dtype string, byte offset, count)} of a channel record's head (asdr_tuner_channel_record_field)."""
    L = _lib()
    out, k = {}, 0
    while True:
        off, cnt = C.c_int(), C.c_int()
        name = L.asdr_tuner_channel_record_field(k, C.byref(off), C.byref(cnt))
        if name is None:
            return out
        n, ty = name.decode().split(":")
        out[n] = (_FIELD_TYPES[ty], int(off.value), int(cnt.value))
        k += 1


def tuner_channel_field(records, name):
    """A writable view of field `name` of uint8 records [n, 2560] (or one record [2560]): [n] or [n, count] of the field's type;
    "carry" gives the carry section as uint32 [n, 576] (I low, Q high)."""
    records = np.asarray(records)
    if records.dtype != np.uint8 or records.shape[-1] != CHANNEL_RECORD_BYTES or not records.flags.c_contiguous:
        raise AsdrError("tuner_channel_field: needs C-contiguous uint8 records [n, %d]" % CHANNEL_RECORD_BYTES)
    r2 = records.reshape(-1, CHANNEL_RECORD_BYTES)
    if name == "carry":
        ty, off, cnt = "<u4", 256, 576
    else:
        fields = tuner_channel_record_fields()
        if name not in fields:
            raise AsdrError("tuner_channel_field: no field %r (one of %s, carry)" % (name, " ".join(fields)))
        ty, off, cnt = fields[name]
    v = r2[:, off:off + cnt * np.dtype(ty).itemsize].view(ty)
    return v[:, 0] if cnt == 1 else v


def _channel_list(channels, n_default):
    """(ctypes int pointer or None, n, the array kept alive) of a channel list; None names channels 0 .. n_default - 1."""
    if channels is None:
        return None, int(n_default), None
    ch = np.ascontiguousarray(channels, dtype=np.int32).reshape(-1)
    return ch.ctypes.data_as(C.POINTER(C.c_int)), int(ch.size), ch


class _DeviceRows:
    """A device allocation as a __cuda_array_interface__ object, so that torch.as_tensor wraps it without a copy."""

    def __init__(self, ptr, shape, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(ptr), False), "version": 2}


class TunerBank(ResetStage):
    """n_channels digital tuners over n_sources shared CS16 rows at decimation D (include/asdr_tuner.h).  fs_in (Hz) makes a rate
    bank: any integer input rate with fs_in / D in [44100, 176400], resampled to 44.1 kHz after the decimator.  device = NO_DEVICE
    (-1) gives the control plane only."""
    _prefix = "asdr_tuner_"

    def __init__(self, n_channels, n_sources=1, decimation=1, fs_in=None, device=0):
        self._L = _lib()
        if fs_in is None:
            self._create("asdr_tuner_create", self._L.asdr_tuner_create(int(n_channels), int(n_sources), int(decimation), int(device)))
        else:
            self._create("asdr_tuner_create_rate",
                         self._L.asdr_tuner_create_rate(int(n_channels), int(n_sources), int(fs_in), int(decimation), int(device)))
        self._geometry()

    def _geometry(self):
        self.n_channels, self.n_sources = int(self._L.asdr_tuner_n_channels(self._h)), int(self._L.asdr_tuner_n_sources(self._h))
        self.decimation, self.fs_in = int(self._L.asdr_tuner_decimation(self._h)), int(self._L.asdr_tuner_rate(self._h))

    @classmethod
    def fastconv(cls, n_channels, n_sources, fs_in, R, device=0):
        """A fast-convolution bank (include/asdr_tuner.h, "Fast-convolution banks"): overlap-save stage 1 with one FFT of N = 256 R
        points per source and frame, fs_in / R in [44100, 176400], then the rate-bank stage 2.  `decimation` is R."""
        self = cls.__new__(cls)
        self._L = _lib()
        self._create("asdr_tuner_create_fastconv",
                     self._L.asdr_tuner_create_fastconv(int(n_channels), int(n_sources), int(fs_in), int(R), int(device)))
        self._geometry()
        return self

    # state records (include/asdr_tuner.h, "State records")
    @classmethod
    def from_bank_state(cls, blob, n_channels, device=0):
        """A new bank of the blob's kind and geometry with n_channels channels, holding the blob's state: every channel in creation
        state at the blob's position, to be filled by import_channels."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
        self = cls.__new__(cls)
        self._L = _lib()
        self._create("asdr_tuner_create_from_bank_state",
                     self._L.asdr_tuner_create_from_bank_state(blob.ctypes.data_as(C.c_void_p), int(blob.size), int(n_channels), int(device)))
        self._geometry()
        return self

    def bank_state_bytes(self):
        return int(self._L.asdr_tuner_bank_state_bytes(self._h))

    def export_bank_state(self):
        """uint8 [bank_state_bytes()]: everything bank-wide and per source; waits for the bank's work and changes nothing."""
        blob = np.zeros(self.bank_state_bytes(), dtype=np.uint8)
        self._chk(self._L.asdr_tuner_export_bank_state(self._h, blob.ctypes.data_as(C.c_void_p), int(blob.size)))
        return blob

    def import_bank_state(self, blob):
        """Validates the whole blob, then resets the bank and installs it; the channels follow by import_channels."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
        self._chk(self._L.asdr_tuner_import_bank_state(self._h, blob.ctypes.data_as(C.c_void_p), int(blob.size)))

    def export_channels(self, channels=None):
        """uint8 [n, 2560]: the records of `channels` (any order; None: every channel)."""
        p, n, _keep = _channel_list(channels, self.n_channels)
        rec = np.zeros((n, CHANNEL_RECORD_BYTES), dtype=np.uint8)
        self._chk(self._L.asdr_tuner_export_channels(self._h, p, n, rec.ctypes.data_as(C.c_void_p)))
        return rec

    def import_channels(self, records, channels=None):
        """records: uint8 [n, 2560]; record i goes to channels[i] (None: channel i).  All-or-nothing."""
        records = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, CHANNEL_RECORD_BYTES)
        p, n, _keep = _channel_list(channels, records.shape[0])
        if n != records.shape[0]:
            raise AsdrError("import_channels: %d records for %d channels" % (records.shape[0], n))
        self._chk(self._L.asdr_tuner_import_channels(self._h, p, n, records.ctypes.data_as(C.c_void_p)))

    def export_channels_device(self, ptr, channels=None, stream=0, n=None):
        """Records of `channels` (None: channels 0 .. n - 1, n defaulting to all) to device memory at ptr (16-byte aligned, n x 2560
        bytes), asynchronous on `stream` in the bank's stream order."""
        p, n, _keep = _channel_list(channels, self.n_channels if n is None else n)
        self._chk(self._L.asdr_tuner_export_channels_device(self._h, p, n, C.c_void_p(ptr), C.c_void_p(stream)))

    def import_channels_device(self, ptr, channels=None, stream=0, n=None):
        """Record i at ptr to channels[i]; the heads are validated on the host first (a wait on `stream`), the rest runs on `stream`."""
        p, n, _keep = _channel_list(channels, self.n_channels if n is None else n)
        self._chk(self._L.asdr_tuner_import_channels_device(self._h, p, n, C.c_void_p(ptr), C.c_void_p(stream)))

    def fft_size(self):
        """N of a fast-convolution bank, 0 for a direct-form bank."""
        return int(self._L.asdr_tuner_fft_size(self._h))

    def set_channel_filter(self, g):
        """Real taps (float32, 1..129) at Fs_mid of a fast-convolution bank."""
        g = np.ascontiguousarray(g, dtype=np.float32)
        self._chk(self._L.asdr_tuner_set_channel_filter(self._h, g.ctypes.data_as(_fp), int(g.size)))

    def get_channel_filter(self):
        """float32 [Lg]."""
        n = self._chk(self._L.asdr_tuner_get_channel_filter(self._h, None, 0))
        g = np.zeros(n, dtype=np.float32)
        self._chk(self._L.asdr_tuner_get_channel_filter(self._h, g.ctypes.data_as(_fp), n))
        return g

    # filter palette and gain of a fast-convolution bank (include/asdr_tuner.h, "Filter palette and gain")
    def set_palette_filter(self, slot, taps):
        """Define (or redefine) slot 1..63: 1..129 taps at Fs_mid; a complex dtype gives complex taps, anything else real ones.
        Applies to the frames of the next update call, for every channel on the slot."""
        taps = np.asarray(taps)
        cx = np.iscomplexobj(taps)
        taps = np.ascontiguousarray(taps, dtype=np.complex64 if cx else np.float32).reshape(-1)
        self._chk(self._L.asdr_tuner_palette_set(self._h, int(slot), taps.view(np.float32).ctypes.data_as(_fp),
                                                 int(taps.size), int(cx)))

    def get_palette_filter(self, slot):
        """The slot's taps, float32 or complex64 [Lg]; None for an undefined slot.  Slot 0 is the channel filter."""
        cx = C.c_int()
        n = self._chk(self._L.asdr_tuner_palette_get(self._h, int(slot), None, 0, C.byref(cx)))
        if n == 0:
            return None
        g = np.zeros(n, dtype=np.complex64 if cx.value else np.float32)
        self._chk(self._L.asdr_tuner_palette_get(self._h, int(slot), g.view(np.float32).ctypes.data_as(_fp), n, None))
        return g

    def clear_palette_filter(self, slot):
        """Slot 1..63 back to undefined; refused while a channel is on it."""
        self._chk(self._L.asdr_tuner_palette_clear(self._h, int(slot)))

    def set_channel_slot(self, slot, ch=ALL):
        """The channel's filter is the palette's slot (0, the bank's channel filter, or a defined one) from the next update call."""
        self._chk(self._L.asdr_tuner_set_channel_slot(self._h, int(ch), int(slot)))

    def slots(self):
        """int32 [n_channels]."""
        out = np.zeros(self.n_channels, dtype=np.int32)
        self._chk(self._L.asdr_tuner_read_slots(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def set_gain(self, gain, ch=ALL):
        """The channel's output is multiplied by gain (finite, |gain| <= 32768) before the rounding, from the next update call;
        the level monitor reads the signal without it."""
        self._chk(self._L.asdr_tuner_set_channel_gain(self._h, int(ch), float(gain)))

    def gains(self):
        """float32 [n_channels]."""
        out = np.zeros(self.n_channels, dtype=np.float32)
        self._chk(self._L.asdr_tuner_read_gains(self._h, out.ctypes.data_as(_fp)))
        return out

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

    def ratio(self):
        """(U, M): stage 2 resamples Fs_in / D by U / M to 44.1 kHz."""
        u, m = C.c_int(), C.c_int()
        self._chk(self._L.asdr_tuner_ratio(self._h, C.byref(u), C.byref(m)))
        return int(u.value), int(m.value)

    def output_position(self):
        return int(self._L.asdr_tuner_output_position(self._h))

    def set_resampler(self, h2, gain_shift=0):
        h2 = np.ascontiguousarray(h2, dtype=np.int16)
        self._chk(self._L.asdr_tuner_set_resampler(self._h, _p16(h2), int(h2.size), int(gain_shift)))

    def get_resampler(self):
        """(h2 int16 [U K], gain_shift)."""
        n = self._chk(self._L.asdr_tuner_get_resampler(self._h, None, 0, None))
        h, g = np.zeros(n, dtype=np.int16), C.c_int()
        self._chk(self._L.asdr_tuner_get_resampler(self._h, _p16(h), n, C.byref(g)))
        return h, int(g.value)

    def out_blocks(self, n_frames):
        """Output blocks the next call of n_frames frames (128 D input samples per source each) will write."""
        return self._chk(self._L.asdr_tuner_out_blocks(self._h, int(n_frames)))

    def update_rate(self, iq):
        """iq: int16 [n_sources][n_frames * 128 * D][2] on the host.  Returns (I, Q), int16 [n_channels][n][128] for the n blocks
        this call writes (n may be 0)."""
        iq = np.ascontiguousarray(iq, dtype=np.int16)
        per = BLOCK * self.decimation
        assert iq.shape[0] == self.n_sources and iq.shape[-1] == 2 and iq.shape[1] % per == 0, iq.shape
        nf = iq.shape[1] // per
        nb = self.out_blocks(nf)
        I = np.empty((self.n_channels, max(nb, 1), BLOCK), dtype=np.int16)
        Q = np.empty_like(I)
        got = self._chk(self._L.asdr_tuner_update_rate(self._h, _p16(iq), nf, _p16(I), _p16(Q), nb))
        assert got == nb, (got, nb)
        return I[:, :nb], Q[:, :nb]

    def update_rate_device(self, dIQ, dI, dQ, n_frames, out_capacity_blocks, in_stride_samples=None, out_stride_blocks=None, stream=0):
        """Device pointers (ints); asynchronous on `stream`.  Returns the number of blocks written to each row."""
        ins = in_stride_samples or n_frames * BLOCK * self.decimation
        return self._chk(self._L.asdr_tuner_update_rate_device(
            self._h, C.c_void_p(dIQ), int(ins), int(n_frames), C.c_void_p(dI), C.c_void_p(dQ), int(out_capacity_blocks),
            int(out_stride_blocks or out_capacity_blocks), C.c_void_p(stream)))

    def set_input_format(self, fmt):
        """fmt: "cs16" (the default), "cu8", "cs8", "cf32" or "rs16" (include/asdr_tuner.h, "Input formats"), or an ASDR_TUNER_IN_*
        value.  Applies to the rows of the next call."""
        if isinstance(fmt, str):
            if fmt.lower() not in INPUT_FORMATS:
                raise AsdrError("unknown input format %r (one of %s)" % (fmt, " ".join(INPUT_FORMATS)))
            fmt = INPUT_FORMATS[fmt.lower()][0]
        self._chk(self._L.asdr_tuner_set_input_format(self._h, int(fmt)))

    def input_format(self):
        """The bank's format by name."""
        v = int(self._L.asdr_tuner_input_format(self._h))
        for k, f in INPUT_FORMATS.items():
            if f[0] == v:
                return k
        raise AsdrError("asdr_tuner_input_format returned %d (a closed bank?)" % v)

    def update_samples(self, x):
        """x: rows in the bank's format on the host, [n_sources][n_frames * 128 * D][2] of dtype int16 (cs16), uint8 (cu8), int8
        (cs8) or float32 (cf32), or [n_sources][n_frames * 128 * D] int16 (rs16).  dtype and shape must be the format's: nothing is
        converted here.  Returns what update_rate returns."""
        name = self.input_format()
        _, dtype, parts = INPUT_FORMATS[name]
        if not isinstance(x, np.ndarray) or x.dtype != np.dtype(dtype):
            raise AsdrError("update_samples: a %s bank takes a numpy array of dtype %s, not %s" % (
                name, np.dtype(dtype).name, getattr(x, "dtype", type(x).__name__)))
        per = BLOCK * self.decimation
        want = (self.n_sources, "n_frames * %d" % per) + ((2,) if parts == 2 else ())
        if x.ndim != len(want) or x.shape[0] != self.n_sources or x.shape[1] % per != 0 or (parts == 2 and x.shape[2] != 2):
            raise AsdrError("update_samples: a %s bank takes rows of shape %s, not %s" % (name, list(want), list(x.shape)))
        x = np.ascontiguousarray(x)
        nf = x.shape[1] // per
        nb = self.out_blocks(nf)
        I = np.empty((self.n_channels, max(nb, 1), BLOCK), dtype=np.int16)
        Q = np.empty_like(I)
        got = self._chk(self._L.asdr_tuner_update_samples(self._h, x.ctypes.data_as(C.c_void_p), nf, _p16(I), _p16(Q), nb))
        assert got == nb, (got, nb)
        return I[:, :nb], Q[:, :nb]

    def update_samples_device(self, dIn, dI, dQ, n_frames, out_capacity_blocks, in_stride_samples=None, out_stride_blocks=None, stream=0):
        """update_rate_device with rows of the bank's format at dIn: row starts 16-byte aligned (the pointer, and in_stride_samples
        times the format's bytes per sample a multiple of 16).  Returns the number of blocks written to each row."""
        ins = in_stride_samples or n_frames * BLOCK * self.decimation
        return self._chk(self._L.asdr_tuner_update_samples_device(
            self._h, C.c_void_p(dIn), int(ins), int(n_frames), C.c_void_p(dI), C.c_void_p(dQ), int(out_capacity_blocks),
            int(out_stride_blocks or out_capacity_blocks), C.c_void_p(stream)))

    def last_kernel_ms(self):
        return float(self._L.asdr_tuner_last_kernel_ms(self._h))

    # monitors of a fast-convolution bank (include/asdr_tuner.h, "Monitors")
    def enable_spectrum(self, n_bins, window="hann", mode="sum"):
        """Accumulate every source's wideband power spectrum in n_bins bins (a power of two in 256..N; 0 switches it off) from the
        next update call on.  window: "rect" or "hann"; mode: "sum" or "peak" (or the ASDR_TUNER_* values)."""
        if isinstance(window, str):
            if window.lower() not in SPECTRUM_WINDOWS:
                raise AsdrError("unknown spectrum window %r (one of %s)" % (window, " ".join(SPECTRUM_WINDOWS)))
            window = SPECTRUM_WINDOWS[window.lower()]
        if isinstance(mode, str):
            if mode.lower() not in SPECTRUM_MODES:
                raise AsdrError("unknown spectrum mode %r (one of %s)" % (mode, " ".join(SPECTRUM_MODES)))
            mode = SPECTRUM_MODES[mode.lower()]
        self._chk(self._L.asdr_tuner_spectrum_enable(self._h, int(n_bins), int(window), int(mode)))

    def spectrum_bins(self):
        """B, 0 when the spectrum monitor is off."""
        return int(self._L.asdr_tuner_spectrum_bins(self._h))

    def spectrum_config(self):
        """(n_bins, window, mode) by name, or None when the spectrum monitor is off."""
        B = self.spectrum_bins()
        if not B:
            return None
        w, m = int(self._L.asdr_tuner_spectrum_window(self._h)), int(self._L.asdr_tuner_spectrum_mode(self._h))
        return (B, next(k for k, v in SPECTRUM_WINDOWS.items() if v == w), next(k for k, v in SPECTRUM_MODES.items() if v == m))

    def spectrum(self, clear=True):
        """(float64 [n_sources, B], frames accumulated); waits for the bank's work.  Mode sum: acc / frames is the mean power per
        bin (int16^2 units); mode peak: acc is the largest frame.  Bin j starts at spectrum_frequencies(fs_in, B)[j]."""
        out = np.zeros((self.n_sources, self.spectrum_bins()), dtype=np.float64)
        frames = C.c_longlong()
        self._chk(self._L.asdr_tuner_spectrum_read(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(frames), int(bool(clear))))
        return out, int(frames.value)

    def spectrum_frames(self):
        return int(self._L.asdr_tuner_spectrum_frames(self._h))

    def clear_spectrum(self):
        self._chk(self._L.asdr_tuner_spectrum_clear(self._h))

    def spectrum_tensor(self):
        """The device rows as a torch float64 [n_sources, B] view (no copy, no synchronisation): valid in stream order after an
        update call, until the next enable_spectrum() or close()."""
        import torch
        p = self._L.asdr_tuner_spectrum_device(self._h)
        if not p:
            raise AsdrError(self._L.asdr_last_error().decode())
        return torch.as_tensor(_DeviceRows(p, (self.n_sources, self.spectrum_bins()), self), device="cuda")

    def enable_levels(self, on=True):
        """Accumulate every channel's power before rounding and clamp (sum of |y|^2 over its Fs_mid samples) from the next update
        call on."""
        self._chk(self._L.asdr_tuner_levels_enable(self._h, int(bool(on))))

    def levels_enabled(self):
        return bool(self._L.asdr_tuner_levels_enabled(self._h))

    def levels(self, clear=True):
        """(float64 [n_channels] in channel order, frames accumulated); waits for the bank's work.  level / (128 frames) is the mean
        power per Fs_mid sample.  A retune does not clear a channel's level."""
        out = np.zeros(self.n_channels, dtype=np.float64)
        frames = C.c_longlong()
        self._chk(self._L.asdr_tuner_levels_read(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(frames), int(bool(clear))))
        return out, int(frames.value)

    def levels_frames(self):
        return int(self._L.asdr_tuner_levels_frames(self._h))

    def clear_levels(self):
        self._chk(self._L.asdr_tuner_levels_clear(self._h))

    def levels_tensor(self):
        """The device accumulators as a torch float64 [n_channels] view, as spectrum_tensor()."""
        import torch
        p = self._L.asdr_tuner_levels_device(self._h)
        if not p:
            raise AsdrError(self._L.asdr_last_error().decode())
        return torch.as_tensor(_DeviceRows(p, (self.n_channels,), self), device="cuda")

    # source conditioning (include/asdr_tuner.h, "Source conditioning"): every bank kind
    def set_iq_correction(self, dc=(0, 0), cross=0.0, gain=1.0, source=ALL, words=None):
        """The source's (or every source's) DC and I/Q-imbalance correction, from the next update call: x' = (xr - dc[0],
        cross (xr - dc[0]) + gain (xi - dc[1])), in the header's integer arithmetic.  dc in int16 units (rounded to integers),
        cross in [-0.5, 0.5] and gain in [0.5, 2] rounded to Q16 -- or words = (dc_re, dc_im, cross_q16, gain_q16), the words
        themselves (dc, cross and gain are then not looked at)."""
        if words is None:
            words = (int(np.rint(dc[0])), int(np.rint(dc[1])), int(np.rint(65536.0 * float(cross))), int(np.rint(65536.0 * float(gain))))
        if len(words) != 4 or any(not -2**31 <= int(w) < 2**31 for w in words):
            raise AsdrError("set_iq_correction: needs four words (dc_re, dc_im, cross_q16, gain_q16) that fit int32")
        c = np.array([tuple(int(w) for w in words)], dtype=IQ_CORRECTION_DTYPE)
        self._chk(self._L.asdr_tuner_set_iq_correction(self._h, int(source), c.ctypes.data_as(C.c_void_p)))

    def iq_correction(self, source):
        """The source's words (dc_re, dc_im, cross_q16, gain_q16); the identity is (0, 0, 0, 65536)."""
        c = np.zeros(1, dtype=IQ_CORRECTION_DTYPE)
        self._chk(self._L.asdr_tuner_get_iq_correction(self._h, int(source), c.ctypes.data_as(C.c_void_p)))
        return tuple(int(c[k][0]) for k in IQ_CORRECTION_DTYPE.names)

    def enable_iq_stats(self, on=True):
        """Accumulate every source's exact moments and clip count of the uncorrected samples from the next update call on;
        enabling and disabling both clear them."""
        self._chk(self._L.asdr_tuner_iq_stats_enable(self._h, int(bool(on))))

    def iq_stats_enabled(self):
        return bool(self._L.asdr_tuner_iq_stats_enabled(self._h))

    def iq_stats(self, clear=True):
        """Structured array [n_sources] of IQ_STATS_DTYPE (n, sum_re, sum_im, sum_re2, sum_im2, sum_reim, clipped; int64, exact);
        waits for the bank's work."""
        st = np.zeros(self.n_sources, dtype=IQ_STATS_DTYPE)
        self._chk(self._L.asdr_tuner_iq_stats_read(self._h, st.ctypes.data_as(C.c_void_p), int(bool(clear))))
        return st

    def clear_iq_stats(self):
        self._chk(self._L.asdr_tuner_iq_stats_clear(self._h))

    def track_iq(self, source=ALL):
        """Read the statistics, set the estimated correction of `source` (or of every source), clear the statistics.  A source
        whose estimate fails keeps its correction; returns the number of sources set."""
        return self._chk(self._L.asdr_tuner_iq_track(self._h, int(source)))

    def condition_launches(self):
        """Pre-pass launches since creation: 0 for a bank that never had a correction off the identity or the statistics on."""
        return int(self._L.asdr_tuner_condition_launches(self._h))
