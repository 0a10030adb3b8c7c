"""Numpy restatement of the tuner bank's input formats (include/asdr_tuner.h, "Input formats"), written from that table and not
from the kernels: to_cs16() turns stored samples into the x = (xr, xi) int16 pairs every other statement starts from; the
generators make stored samples that reach both ends of each format's range (for CF32 also ties, NaN, +-inf and values past +-1);
HalfSizeFFT is a float32 model of the statement's RS16 form (a transform of N / 2 complex points and the untangling step) that
sizes the tolerance of the RS16 fast-convolution tests next to TunerFastconvRef.stage1_f32."""
import numpy as np

FORMATS = {"cs16": (np.int16, 2), "cu8": (np.uint8, 2), "cs8": (np.int8, 2), "cf32": (np.float32, 2), "rs16": (np.int16, 1)}
COMPLEX_FORMATS = ["cu8", "cs8", "cf32"]
BYTES = {"cs16": 4, "cu8": 2, "cs8": 2, "cf32": 8, "rs16": 2}


def to_cs16(raw, fmt):
    """Stored samples ([...][2], or [...] for rs16) -> int16 [...][2]: the table of include/asdr_tuner.h."""
    raw = np.asarray(raw)
    dtype, parts = FORMATS[fmt]
    assert raw.dtype == np.dtype(dtype) and (parts == 1 or raw.shape[-1] == 2), (fmt, raw.dtype, raw.shape)
    if fmt == "cs16":
        return raw.copy()
    if fmt == "cu8":
        return (256 * raw.astype(np.int64) - 32640).astype(np.int16)
    if fmt == "cs8":
        return (256 * raw.astype(np.int64)).astype(np.int16)
    if fmt == "cf32":
        v = 32768.0 * raw.astype(np.float64)                  # exact: a float32 times 2^15 in float64
        with np.errstate(invalid="ignore"):
            r = np.clip(np.rint(v), -32768.0, 32767.0)        # rint: round half to even; +-inf clip to the ends
        return np.where(np.isnan(v), 0.0, r).astype(np.int16)
    assert fmt == "rs16"
    return np.stack([raw, np.zeros_like(raw)], axis=-1)


def from_cs16(iq, fmt):
    """Stored samples whose conversion is as close to the int16 pairs iq as the format allows (cf32: exactly iq)."""
    iq = np.asarray(iq, dtype=np.int64)
    if fmt == "cs16":
        return iq.astype(np.int16)
    if fmt == "cu8":
        return np.clip(np.floor_divide(iq + 32640 + 128, 256), 0, 255).astype(np.uint8)
    if fmt == "cs8":
        return np.clip(np.floor_divide(iq + 128, 256), -128, 127).astype(np.int8)
    if fmt == "cf32":
        return (iq / 32768.0).astype(np.float32)
    assert fmt == "rs16"
    return iq[..., 0].astype(np.int16)


CF32_SPECIALS = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, 1.5, -1.5, 3e38, -3e38, 32767.0 / 32768.0, 32767.5 / 32768.0,
                          -32768.5 / 32768.0, 0.5 / 32768.0, 1.5 / 32768.0, 2.5 / 32768.0, -0.5 / 32768.0, -1.5 / 32768.0,
                          -2.5 / 32768.0, 12345.5 / 32768.0, -12344.5 / 32768.0, 1e-45, -0.0, 0.49999997 / 32768.0,
                          0.50000006 / 32768.0], dtype=np.float32)


def specials(fmt):
    """Stored part values that reach both ends of the format's range (cf32: also ties, NaN, +-inf, values past +-1, a denormal)."""
    if fmt == "cu8":
        return np.array([0, 255, 127, 128, 1, 254], dtype=np.uint8)
    if fmt == "cs8":
        return np.array([-128, 127, 0, -1, 1, -127], dtype=np.int8)
    if fmt == "cf32":
        return CF32_SPECIALS
    return np.array([-32768, 32767, 0, -1, 1, -32767], dtype=np.int16)


def raw_noise(rng, fmt, n_src, n, amp=20000, tones=(), fs=1.0):
    """Stored rows [n_src][n][2] ([n_src][n] for rs16): noise in +-amp (in int16 units) plus tones (source, Hz, amplitude), with
    the format's specials on the parts of every row's first samples.  cf32 noise carries fractions of an LSB, so its conversion
    rounds, and a quarter of its parts are exact ties."""
    parts = FORMATS[fmt][1]
    x = rng.uniform(-amp, amp, size=(n_src, n, parts))
    m = np.arange(n)
    for s, f, a in tones:
        x[s, :, 0] += a * np.cos(2 * np.pi * f * m / fs)
        if parts == 2:
            x[s, :, 1] += a * np.sin(2 * np.pi * f * m / fs)
    if fmt == "cf32":
        raw = (x / 32768.0).astype(np.float32)
        half = rng.random(size=raw.shape) < 0.25
        raw = np.where(half, ((np.floor(x) + 0.5) / 32768.0).astype(np.float32), raw)
    elif parts == 2:
        raw = from_cs16(np.clip(np.rint(x), -32768, 32767), fmt)
    else:
        raw = np.clip(np.rint(x[..., 0]), -32768, 32767).astype(np.int16)
    sp = specials(fmt)
    k = sp.size
    if parts == 2:
        raw[:, :k, 0] = sp
        raw[:, :k, 1] = sp[::-1]
        raw[:, k:2 * k, 0] = sp[0]                            # both parts at one end, then at the other
        raw[:, k:2 * k, 1] = sp[1]
    else:
        raw[:, :k] = sp
    return np.ascontiguousarray(raw)


class HalfSizeFFT:
    """np.fft / scipy.fft stand-in for TunerFastconvRef._stage1 whose forward transform of a real window is the statement's RS16
    form held in complex64: z[n] = w[2n] + j w[2n + 1], Z = DFT_{N/2}(z) (scipy.fft keeps complex64), and
    X[k] = (Z[k] + conj Z[N/2 - k]) / 2 - (j / 2) W_N^k (Z[k] - conj Z[N/2 - k]), X[N - k] = conj X[k], X[N/2] = Re Z[0] - Im Z[0];
    W_N from float64, rounded to complex64.  A model of what float32 costs that form -- of no kernel's pass order."""

    @staticmethod
    def fft(win, axis=1):
        import scipy.fft
        assert axis == 1 and win.dtype == np.complex64 and not win.imag.any()
        w = win.real
        N = w.shape[1]
        M = N // 2
        z = (w[:, 0::2] + np.complex64(1j) * w[:, 1::2]).astype(np.complex64)
        Z = scipy.fft.fft(z, axis=1)
        assert Z.dtype == np.complex64
        k = np.arange(M)
        Zm = np.conj(Z[:, (M - k) % M])
        W = np.exp(-2j * np.pi * k / N).astype(np.complex64)
        half = np.float32(0.5)
        Xk = (Z + Zm) * half - np.complex64(1j) * (W[None, :] * ((Z - Zm) * half))
        assert Xk.dtype == np.complex64
        X = np.empty((w.shape[0], N), dtype=np.complex64)
        X[:, :M] = Xk
        X[:, M] = Z[:, 0].real - Z[:, 0].imag
        X[:, M + 1:] = np.conj(Xk[:, 1:][:, ::-1])
        return X

    @staticmethod
    def ifft(Z, axis=1):
        import scipy.fft
        return scipy.fft.ifft(Z, axis=axis)


def stage1_half_f32(ref, iq):
    """TunerFastconvRef.stage1_f32 with the forward transform by HalfSizeFFT; iq must be real ((a, 0) pairs)."""
    return ref._stage1(iq, HalfSizeFFT, np.complex64).astype(np.complex128)
