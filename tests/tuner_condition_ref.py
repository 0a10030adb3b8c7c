"""Numpy restatement of the tuner banks' source conditioning (include/asdr_tuner.h, "Source conditioning"), written from that
section and not from the kernel: condition() is the correction on converted samples, stats() the seven exact sums of stored
samples, estimate() the float64 estimator in the header's order of operations.  known_answer_rows() is the quality known answer
(one tone through a receiver with gain and phase imbalance and a DC offset) that the CPU and the GPU tests share."""
import math

import numpy as np

import tuner_formats_ref as FM

IDENTITY = (0, 0, 0, 65536)
RANGES = ((-32768, 32767), (-32768, 32767), (-32768, 32768), (32768, 131072))   # d_r, d_i, p, g
STAT_NAMES = ("n", "sum_re", "sum_im", "sum_re2", "sum_im2", "sum_reim", "clipped")


def in_range(c):
    return all(lo <= int(v) <= hi for v, (lo, hi) in zip(c, RANGES))


def condition(x, c, fmt="cs16"):
    """x: converted samples, int16 [...][2] (FM.to_cs16 of the stored ones); c = (d_r, d_i, p, g).  Returns x', int16 [...][2].
    fmt "rs16": only d_r acts and xi' = 0."""
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.shape[-1] == 2 and in_range(c), (x.dtype, x.shape, c)
    d_r, d_i, p, g = (int(v) for v in c)
    a = x[..., 0].astype(np.int64) - d_r
    b = x[..., 1].astype(np.int64) - d_i
    out = np.empty(x.shape, dtype=np.int16)
    out[..., 0] = np.clip(a, -32768, 32767)
    if fmt == "rs16":
        out[..., 1] = 0
    else:
        out[..., 1] = np.clip((p * a + g * b + 32768) >> 16, -32768, 32767)   # int64; >> is an arithmetic shift
    return out


def condition_raw(raw, c, fmt):
    """Stored samples of format fmt -> the corrected rows as the CS16 yardstick bank takes them: int16 [...][2], or for rs16 the
    stored form [...] of the corrected real samples."""
    y = condition(FM.to_cs16(raw, fmt), c, fmt)
    return y[..., 0].copy() if fmt == "rs16" else y


def clipped(raw, fmt):
    """Per stored sample: a part at the format's rail."""
    raw = np.asarray(raw)
    if fmt == "cu8":
        at = (raw == 0) | (raw == 255)
    elif fmt == "cs8":
        at = (raw == -128) | (raw == 127)
    elif fmt == "cf32":
        with np.errstate(invalid="ignore"):
            at = ~(np.abs(raw.astype(np.float64)) < 1.0)          # |a| >= 1, +-inf, NaN
    else:
        at = (raw == -32768) | (raw == 32767)
    return at if fmt == "rs16" else at.any(axis=-1)


def stats(raw, fmt):
    """One source's stored samples ([n][2], or [n] for rs16) -> the seven sums as Python ints (exact), in STAT_NAMES' order."""
    x = FM.to_cs16(raw, fmt).astype(np.int64).reshape(-1, 2)
    xr, xi = x[:, 0], x[:, 1]
    vals = (x.shape[0], xr.sum(), xi.sum(), (xr * xr).sum(), (xi * xi).sum(), (xr * xi).sum(), clipped(raw, fmt).sum())
    return tuple(int(v) for v in vals)


def add_stats(a, b):
    return tuple(int(u) + int(v) for u, v in zip(a, b))


def estimate(st, unrounded=False):
    """The header's estimator on the seven sums: the words (d_r, d_i, p, g), or None where it fails.  unrounded: the four values
    before rint (for choosing test cases away from ties), or None."""
    n, s_r, s_i, s_rr, s_ii, s_ri = (int(v) for v in st[:6])
    if n < 2:
        return None
    f = np.float64
    nn = f(n)
    m_r, m_i = f(s_r) / nn, f(s_i) / nn
    ph, gh = f(0.0), f(1.0)
    if s_i != 0 or s_ii != 0 or s_ri != 0:
        v_rr = f(s_rr) / nn - m_r * m_r
        v_ii = f(s_ii) / nn - m_i * m_i
        v_ri = f(s_ri) / nn - m_r * m_i
        if not v_rr > 0.0:
            return None
        det = v_rr * v_ii - v_ri * v_ri
        if not det > 0.0:
            return None
        gh = v_rr / f(math.sqrt(det))
        ph = -gh * v_ri / v_rr
    raw = (m_r, m_i, f(65536.0) * ph, f(65536.0) * gh)
    words = tuple(int(np.rint(v)) for v in raw)
    if not in_range(words):
        return None
    return tuple(float(v) for v in raw) if unrounded else words


# ---- the quality known answer -----------------------------------------------------------------------------------------------
KA_N, KA_BIN, KA_AMP, KA_GAIN, KA_PHASE_DEG, KA_DC = 65536, 5001, 12000.0, 1.06, 4.0, (310.4, -777.3)
KA_WORDS = (310, -777, -4583, 61977)


def known_answer_rows():
    """int16 [65536][2]: I = A cos(theta) + dc_r, Q = 1.06 A sin(theta + 4 deg) + dc_i, theta = 2 pi 5001 m / 65536, rounded."""
    th = 2.0 * np.pi * KA_BIN * np.arange(KA_N) / KA_N
    i = KA_AMP * np.cos(th) + KA_DC[0]
    q = KA_GAIN * KA_AMP * np.sin(th + np.deg2rad(KA_PHASE_DEG)) + KA_DC[1]
    return np.stack([np.rint(i), np.rint(q)], axis=-1).astype(np.int16)


def image_and_dc_db(x):
    """(image at -bin, DC) of int16 [65536][2] rows in dB relative to the tone at +bin."""
    X = np.fft.fft(x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64))
    tone = abs(X[KA_BIN])
    return 20 * np.log10(abs(X[-KA_BIN]) / tone), 20 * np.log10(max(abs(X[0]), 1e-300) / tone)
