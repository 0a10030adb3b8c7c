"""ctypes binding of the CPU oracle (oracle/libasdr_oracle.so).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg.  Nothing under audiosdr_amd/ imports this module.

`OracleSDR` mirrors the reference class surface (AudioSDR.h:88-156): same method names, same
argument meaning, one instance == one reference `AudioSDR` object.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libasdr_oracle.so")

BLOCK = 128
LSBmode, USBmode, CW_LSBmode, CW_USBmode, AMmode, SAMmode, WSPRmode = range(7)
(audioAM, audioCW, audioWSPR, audio2100, audio2300, audio2500, audio2700, audio2900, audio3100, audio3300,
 audioBypass) = range(11)
AGCoff, AGCfast, AGCmedium, AGCslow = range(4)

TAPS = ["SCALED_I", "SCALED_Q", "NB_I", "NB_Q", "IF_I", "IF_Q", "MIX_I", "MIX_Q", "DEMOD", "AUDIO_FILT", "AGC", "ALS"]


def build(force=False):
    """Compile the oracle with gcc (seconds).  Building the checker is not using it."""
    src = os.path.join(_HERE, "asdr_oracle.c")
    deps = [src, os.path.join(_HERE, "asdr_oracle.h"), os.path.join(_HERE, "asdr_front_oracle.c"),
            os.path.join(_HERE, "asdr_front_oracle.h"),
            os.path.join(_HERE, "..", "audiosdr_amd", "csrc", "asdr_tables.h"),
            os.path.join(_HERE, "..", "audiosdr_amd", "csrc", "asdr_front_tables.h")]
    if not force and os.path.exists(_LIB_PATH) and all(
            os.path.getmtime(_LIB_PATH) >= os.path.getmtime(d) for d in deps):
        return _LIB_PATH
    subprocess.check_call(["make", "-C", _HERE, "-B", "libasdr_oracle.so"], stdout=subprocess.DEVNULL)
    return _LIB_PATH


class PreState(C.Structure):
    """ao_pre_state_t (asdr_front_oracle.h)."""
    _fields_ = [("correction", C.c_int16), ("saved_sample", C.c_int16), ("failure_count", C.c_int16), ("success_count", C.c_int16),
                ("auto_detect", C.c_int32), ("swap", C.c_int32), ("max_line", C.c_int32), ("strong", C.c_int32),
                ("max_power", C.c_float), ("avg_power", C.c_float), ("ratio", C.c_float)]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    build()
    L = C.CDLL(_LIB_PATH)
    vp, f32, i32, u16, i16p = C.c_void_p, C.c_float, C.c_int, C.c_uint16, C.POINTER(C.c_int16)
    fp = C.POINTER(C.c_float)
    L.ao_create.restype = vp
    L.ao_destroy.argtypes = [vp]
    L.ao_enable_taps.argtypes = [vp, i32]
    L.ao_set_unknown_mode_silence.argtypes = [vp, i32]
    L.ao_set_pll_wrap_bound.argtypes = [vp, i32]
    L.ao_pll_stalled.argtypes = [vp]; L.ao_pll_stalled.restype = i32
    L.ao_test_set_pll_phase.argtypes = [vp, f32]
    L.ao_test_get_pll_phase.argtypes = [vp]; L.ao_test_get_pll_phase.restype = f32
    L.ao_get_chain_constants.argtypes = [vp, fp]
    L.ao_tap.argtypes = [vp, i32]
    L.ao_tap.restype = fp
    L.ao_update.argtypes = [vp, i16p, i16p, i16p]
    L.ao_als_taps.argtypes = [vp]; L.ao_als_taps.restype = fp
    L.ao_als_history.argtypes = [vp]; L.ao_als_history.restype = fp

    def sig(name, args, res=None):
        fn = getattr(L, name)
        fn.argtypes = [vp] + args
        fn.restype = res

    for n in ["init", "enableAudioFilter", "disableAudioFilter", "enableALSfilter", "disableALSfilter",
              "setALSfilterNotch", "setALSfilterPeak", "setALSfilterAdaptive", "setALSfilterStatic", "enableAGC",
              "disableAGC", "enableNoiseBlanker", "disableNoiseBlanker"]:
        sig("ao_" + n, [])
    for n in ["setInputGain", "setIQgainBalance", "setOutputGain", "setAGCthreshold", "setAGCslope", "setAGCkneeWidth",
              "setAGCattackTime", "setAGCreleaseTime", "setAGChangTime", "setAGCstaticGain", "setNoiseBlankerThreshold",
              "setNoiseBlankerThresholdDb"]:
        sig("ao_" + n, [f32])
    for n in ["setMute", "setAudioFilter", "setAGCmode"]:
        sig("ao_" + n, [i32])
    sig("ao_setDemodMode", [i32], f32)
    sig("ao_setALSfilterParams", [C.c_uint, f32, f32])
    for n in ["getTuningOffset", "getBPFlower", "getBPFupper", "getAGCthreshold", "getAGCslope", "getAGCkneeWidth",
              "getAGCattack", "getAGCrelease", "getAAGalphaAttack", "getAGCbetaAttack", "getAGCalphaRelease",
              "getAGCbetaRelease", "getAGCstaticGain", "getAMcarrierLevel", "getSAMfrequency"]:
        sig("ao_" + n, [], f32)
    sig("ao_getAGClookup", [i32], f32)
    sig("ao_getAGChangCount", [], C.c_uint32)
    sig("ao_test_get_agc_hang_counter", [], C.c_uint32)
    sig("ao_test_get_agc_envelope", [], f32)
    sig("ao_getDemodMode", [], C.c_int16)
    for n in ["getMute", "getAudioFilter", "ALSfilterIsEnabled", "ALSfilterIsNotch", "ALSfilterIsPeak",
              "ALSfilterIsAdaptive", "AGCisEnabled", "AGCisActive", "NoiseBlankerisEnabled", "NoiseBlankerDetection",
              "getSAMphaseLockStatus"]:
        sig("ao_" + n, [], i32)
    # stage-level
    L.ao_sin_f32.argtypes = [f32]; L.ao_sin_f32.restype = f32
    L.ao_cos_f32.argtypes = [f32]; L.ao_cos_f32.restype = f32
    L.ao_sin_index.argtypes = [f32]; L.ao_sin_index.restype = u16
    L.ao_sin_from_index.argtypes = [u16]; L.ao_sin_from_index.restype = f32
    L.ao_approx_atan2_f32.argtypes = [f32, f32]; L.ao_approx_atan2_f32.restype = f32
    L.ao_fast_sqrt_f32.argtypes = [f32, i32]; L.ao_fast_sqrt_f32.restype = f32
    L.ao_log2_approx_f32.argtypes = [f32]; L.ao_log2_approx_f32.restype = f32
    L.ao_biquad_cascade_df1.argtypes = [fp, fp, i32, fp, fp, i32]
    L.ao_freq_shifter.argtypes = [fp, fp, f32, f32]; L.ao_freq_shifter.restype = f32
    L.ao_scale_sample.argtypes = [C.c_int16, f32]; L.ao_scale_sample.restype = C.c_double
    L.ao_agc_static_compressor.argtypes = [fp, u16]; L.ao_agc_static_compressor.restype = f32
    L.ao_hilbert_taps.restype = fp
    L.ao_sine_table.restype = fp
    L.ao_biquad_table.argtypes = [i32]; L.ao_biquad_table.restype = fp
    L.ao_check_sin_index_division.argtypes = [C.c_uint32, C.c_uint32]; L.ao_check_sin_index_division.restype = C.c_uint64
    L.ao_check_scale_division.restype = i32
    L.ao_check_scale_unit_gain.restype = i32
    L.ao_check_sin_interp_f32.restype = i32
    L.ao_bench_run.argtypes = [i32, i32, i32, i16p, i16p, i16p, i32]
    L.ao_bench_run.restype = C.c_double
    L.ao_spin_calibrate.argtypes = [i32, C.c_long]
    L.ao_spin_calibrate.restype = C.c_double
    # blocks around the hot path (asdr_front_oracle.h)
    L.ao_pre_create.restype = vp; L.ao_pre_destroy.argtypes = [vp]
    L.ao_pre_update.argtypes = [vp, i16p, i16p]
    for n in ("startAutoI2SerrorDetection", "stopAutoI2SerrorDetection"):
        getattr(L, "ao_pre_" + n).argtypes = [vp]
    L.ao_pre_getAutoI2SerrorDetectionStatus.argtypes = [vp]; L.ao_pre_getAutoI2SerrorDetectionStatus.restype = i32
    L.ao_pre_setI2SerrorCompensation.argtypes = [vp, i32]
    L.ao_pre_getI2SerrorCompensation.argtypes = [vp]; L.ao_pre_getI2SerrorCompensation.restype = C.c_int16
    L.ao_pre_swapIQ.argtypes = [vp, i32]
    L.ao_pre_get_state.argtypes = [vp, C.POINTER(PreState)]
    L.ao_pre_power_spectrum.argtypes = [vp]; L.ao_pre_power_spectrum.restype = fp
    L.ao_fft128.argtypes = [fp]
    L.ao_iqgen_create.restype = vp; L.ao_iqgen_destroy.argtypes = [vp]
    L.ao_iqgen_update.argtypes = [vp, i16p, i16p, i16p]
    L.ao_iqgen_setGainBalance.argtypes = [vp, f32]
    L.ao_iqgen_hilbert_taps.restype = fp
    L.ao_grab_create.restype = vp; L.ao_grab_destroy.argtypes = [vp]
    L.ao_grab_update.argtypes = [vp, i16p, i16p]
    L.ao_grab_newDataAvailable.argtypes = [vp]; L.ao_grab_newDataAvailable.restype = i32
    L.ao_grab_grab.argtypes = [vp, i16p]
    L.ao_front_check_div32767.restype = i32
    L.ao_fft256.argtypes = [fp]
    L.ao_grab_power_spectrum.argtypes = [i16p, fp]
    _lib = L
    return L


def _i16p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int16))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# The oracle's default is the reference's behaviour everywhere.  The GPU parity tests compare with the HIP product, whose SAM PLL
# bounds the reference's two unbounded phase-wrap loops (defined differences): tests/conftest.py sets this for tests
# marked `gpu`, so that every OracleSDR they create models that bound (ao_set_pll_wrap_bound).
PRODUCT_PLL_BOUND = False


class OracleSDR:
    """One reference-equivalent AudioSDR instance on the host CPU."""

    def __init__(self, taps=False, pll_wrap_bound=None):
        self._L = lib()
        self._h = self._L.ao_create()
        if taps:
            self._L.ao_enable_taps(self._h, 1)
        if PRODUCT_PLL_BOUND if pll_wrap_bound is None else pll_wrap_bound:
            self._L.ao_set_pll_wrap_bound(self._h, 1)

    def chain_constants(self):
        out = np.zeros(12, dtype=np.float32)
        self._L.ao_get_chain_constants(self._h, _fp(out))
        return int(self._L.ao_getAGChangCount(self._h)), out

    def agc_running(self):
        """(running hang counter, envelope) as the last block left them: test aid, read-only."""
        return int(self._L.ao_test_get_agc_hang_counter(self._h)), float(self._L.ao_test_get_agc_envelope(self._h))

    def set_unknown_mode_silence(self, on=True):
        """Model the HIP product's defined difference for unknown mode values (oracle/asdr_oracle.h)."""
        self._L.ao_set_unknown_mode_silence(self._h, 1 if on else 0)

    def __del__(self):
        try:
            if self._h:
                self._L.ao_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def __getattr__(self, name):
        # every other reference method maps to ao_<name>(handle, ...)
        fn = getattr(self._L, "ao_" + name)
        return lambda *a: fn(self._h, *a)

    def update(self, I, Q):
        """I, Q: int16 arrays of n*128 samples -> int16 mono audio, n*128 samples."""
        I = np.ascontiguousarray(I, dtype=np.int16).reshape(-1, BLOCK)
        Q = np.ascontiguousarray(Q, dtype=np.int16).reshape(-1, BLOCK)
        out = np.empty_like(I)
        for b in range(I.shape[0]):
            self._L.ao_update(self._h, _i16p(I[b]), _i16p(Q[b]), _i16p(out[b]))
        return out.reshape(-1)

    def tap(self, name):
        p = self._L.ao_tap(self._h, TAPS.index(name))
        return np.ctypeslib.as_array(p, shape=(BLOCK,)).copy()

    def als_taps(self):
        """The ALS filter's 128 taps as the last block left them (a copy)."""
        return np.ctypeslib.as_array(self._L.ao_als_taps(self._h), shape=(BLOCK,)).copy()

    def als_history(self):
        """The ALS filter's input buffer, previous block then last block: 256 floats (a copy)."""
        return np.ctypeslib.as_array(self._L.ao_als_history(self._h), shape=(2 * BLOCK,)).copy()


def run_channels(configure, I, Q):
    """I, Q: int16 [channels][blocks][128].  `configure(sdr, channel)` applies setters.
    Returns (out int16 [channels][blocks][128], list of OracleSDR)."""
    I = np.ascontiguousarray(I, dtype=np.int16)
    Q = np.ascontiguousarray(Q, dtype=np.int16)
    out = np.empty_like(I)
    sdrs = []
    for c in range(I.shape[0]):
        s = OracleSDR()
        configure(s, c)
        out[c] = s.update(I[c], Q[c]).reshape(I.shape[1], BLOCK)
        sdrs.append(s)
    return out, sdrs


def bench_run(config, I, Q, n_threads=1):
    """Time `config` (0 = C2 USB chain, 1 = AM, 2 = SAM) on I/Q [ch][blk][128]; seconds + output."""
    I = np.ascontiguousarray(I, dtype=np.int16)
    Q = np.ascontiguousarray(Q, dtype=np.int16)
    out = np.empty_like(I)
    t = lib().ao_bench_run(config, I.shape[0], I.shape[1], _i16p(I), _i16p(Q), _i16p(out), n_threads)
    return t, out


def host_parallel_capacity(n_threads, iters=100_000_000):
    """How many threads' worth of register-only float arithmetic this process really gets on n_threads threads."""
    t1 = lib().ao_spin_calibrate(1, iters)
    tn = lib().ao_spin_calibrate(n_threads, iters)
    return n_threads * t1 / tn


# --- numpy views of the data tables (for independent cross-checks) ---
def hilbert_taps():
    return np.ctypeslib.as_array(lib().ao_hilbert_taps(), shape=(64,)).copy()


def sine_table():
    return np.ctypeslib.as_array(lib().ao_sine_table(), shape=(257,)).copy()


def biquad_table(i):
    return np.ctypeslib.as_array(lib().ao_biquad_table(i), shape=(4, 5)).copy()


def biquad_cascade(coefs, state, x):
    coefs = np.ascontiguousarray(coefs, dtype=np.float32).reshape(-1)
    state = np.ascontiguousarray(state, dtype=np.float32).reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(x)
    lib().ao_biquad_cascade_df1(_fp(coefs), _fp(state), coefs.size // 5, _fp(x), _fp(y), x.size)
    return y, state


# --- the blocks around the hot path (asdr_front_oracle.h) ---
class OraclePreProcessor:
    """One reference-equivalent AudioSDRpreProcessor (AudioSDRpreProcessor.h:49-84)."""

    def __init__(self):
        self._L = lib()
        self._h = self._L.ao_pre_create()

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ao_pre_destroy(self._h)
            self._h = None

    def update(self, I, Q):
        """I, Q: int16 [n_blocks*128]; returns the conditioned (I, Q) (the reference rewrites its blocks in place)."""
        I = np.array(I, dtype=np.int16).reshape(-1).copy()
        Q = np.array(Q, dtype=np.int16).reshape(-1).copy()
        assert I.size == Q.size and I.size % BLOCK == 0
        for b in range(I.size // BLOCK):
            self._L.ao_pre_update(self._h, _i16p(I[b * BLOCK:]), _i16p(Q[b * BLOCK:]))
        return I, Q

    def startAutoI2SerrorDetection(self):
        self._L.ao_pre_startAutoI2SerrorDetection(self._h)

    def stopAutoI2SerrorDetection(self):
        self._L.ao_pre_stopAutoI2SerrorDetection(self._h)

    def getAutoI2SerrorDetectionStatus(self):
        return int(self._L.ao_pre_getAutoI2SerrorDetectionStatus(self._h))

    def setI2SerrorCompensation(self, correction):
        self._L.ao_pre_setI2SerrorCompensation(self._h, int(correction))

    def getI2SerrorCompensation(self):
        return int(self._L.ao_pre_getI2SerrorCompensation(self._h))

    def swapIQ(self, swap):
        self._L.ao_pre_swapIQ(self._h, 1 if swap else 0)

    def state(self):
        s = PreState()
        self._L.ao_pre_get_state(self._h, C.byref(s))
        return {n: getattr(s, n) for n, _ in PreState._fields_}

    def power_spectrum(self):
        return np.ctypeslib.as_array(self._L.ao_pre_power_spectrum(self._h), shape=(128,)).copy()


class OracleIQgenerator:
    """One reference-equivalent AudioIQgenerator (AudioIQgenerator.h:48-106)."""

    def __init__(self):
        self._L = lib()
        self._h = self._L.ao_iqgen_create()

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ao_iqgen_destroy(self._h)
            self._h = None

    def setGainBalance(self, balance):
        self._L.ao_iqgen_setGainBalance(self._h, float(balance))

    def update(self, x):
        """x: int16 [n_blocks*128] real input; returns (I, Q) int16 of the same length."""
        x = np.ascontiguousarray(x, dtype=np.int16).reshape(-1)
        assert x.size % BLOCK == 0
        I, Q = np.empty_like(x), np.empty_like(x)
        for b in range(x.size // BLOCK):
            self._L.ao_iqgen_update(self._h, _i16p(x[b * BLOCK:]), _i16p(I[b * BLOCK:]), _i16p(Q[b * BLOCK:]))
        return I, Q


class OracleGrabber:
    """One reference-equivalent AudioGrabberComplex256 (AudioGrabberComplex256.h:44-63)."""

    def __init__(self):
        self._L = lib()
        self._h = self._L.ao_grab_create()

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ao_grab_destroy(self._h)
            self._h = None

    def update(self, I, Q):
        I = np.ascontiguousarray(I, dtype=np.int16).reshape(-1)
        Q = np.ascontiguousarray(Q, dtype=np.int16).reshape(-1)
        for b in range(I.size // BLOCK):
            self._L.ao_grab_update(self._h, _i16p(I[b * BLOCK:]), _i16p(Q[b * BLOCK:]))

    def newDataAvailable(self):
        return int(self._L.ao_grab_newDataAvailable(self._h))

    def grab(self, destination=None):
        d = np.zeros(512, dtype=np.int16) if destination is None else destination
        self._L.ao_grab_grab(self._h, _i16p(d))
        return d


def fft128_interleaved(buf):
    """ao_fft128 on 256 float32 words (re, im interleaved), as the reference hands its buffer to arm_cfft_f32; returns the 256 words."""
    b = np.ascontiguousarray(buf, dtype=np.float32).copy().reshape(256)
    lib().ao_fft128(_fp(b))
    return b


def fft128(x):
    """The reference's 128-point float32 FFT (CMSIS arm_cfft_f32 restated, asdr_front_oracle.h) of a complex vector."""
    buf = np.empty(256, dtype=np.float32)
    x = np.asarray(x)
    buf[0::2] = x.real.astype(np.float32); buf[1::2] = x.imag.astype(np.float32)
    lib().ao_fft128(_fp(buf))
    return buf[0::2].astype(np.complex64) + 1j * buf[1::2]


def grab_power_spectrum(buffer):
    """|FFT256|^2 of one grabber buffer (int16 [512], interleaved re/im), this project's float32 FFT; natural bin order."""
    b = np.ascontiguousarray(buffer, dtype=np.int16).reshape(512)
    out = np.empty(256, dtype=np.float32)
    lib().ao_grab_power_spectrum(_i16p(b), _fp(out))
    return out


def iqgen_hilbert_taps():
    return np.ctypeslib.as_array(lib().ao_iqgen_hilbert_taps(), shape=(64,)).copy()
