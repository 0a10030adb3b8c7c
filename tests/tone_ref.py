"""The tone squelch's statement (include/asdr_tone.h) in numpy, written from the header's text and independent of the C++: the
third-order CIC decimator, the correlator bank over the tone table, the Q28 biquad cascade, the mute and the per-window verdict with
its open / hang / close rule.  The GPU tests hold the kernel to it at tolerance 0; tests/test_tone_ref.py holds it to float64 filters
and to known answers.  Everything is computed in int64 / uint64 and wrapped where the header says int32."""
import math

import numpy as np

FS = 44100
PASS, ANY = -2, -1
MAX_TONES = 64
CTCSS = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3,
         131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9, 192.8,
         196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1)
STATE_NAMES = ("hist", "hp", "last_power", "last_other", "windows", "matches", "openings", "open_blocks", "detected", "last_best",
               "window_block", "hang_left", "open", "reserved", "acc")
STATE_OFFSETS = (0, 96, 144, 152, 160, 164, 168, 172, 176, 178, 180, 182, 183, 184, 192)
STATE_DTYPE = np.dtype({"names": list(STATE_NAMES), "offsets": list(STATE_OFFSETS), "itemsize": 704,
                        "formats": [("<i2", (48,)), ("<i4", (3, 4)), "<u8", "<u8", "<u4", "<u4", "<u4", "<u4", "<i2", "<i2", "<u2", "u1", "u1",
                                    ("<u4", (2,)), ("<i4", (64, 2))]})
H = np.convolve(np.convolve(np.ones(16, dtype=np.int64), np.ones(16, dtype=np.int64)), np.ones(16, dtype=np.int64))   # 46 taps, sum 4096
C = np.floor(16384.0 * np.cos(2.0 * np.pi * np.arange(1024) / 1024.0) + 0.5).astype(np.int64)
U = np.uint64


def w32(x):
    """int64 -> the int32 it wraps to, as int64."""
    return ((np.asarray(x, dtype=np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def steps_from_hz(hz):
    """floor(f 16 2^32 / 44100 + 0.5) per tone; None for a table the header refuses."""
    hz = [float(f) for f in hz]
    if not 1 <= len(hz) <= MAX_TONES or any(not 0.0 < f < 1378.0 for f in hz):
        return None
    s = [int(math.floor(f * 16.0 * 2.0 ** 32 / FS + 0.5)) for f in hz]
    return s if all(b > a for a, b in zip(s, s[1:])) else None


def highpass_design(fc_hz, sections):
    """The bilinear Butterworth high-pass of order 2 sections as Q28 rows (b0, b1, b2, a1, a2)."""
    K = math.tan(math.pi * fc_hz / FS)
    rows = []
    for k in range(sections):
        q = 2.0 * math.sin(math.pi * (2 * k + 1) / (4.0 * sections))
        n = 1.0 / (1.0 + q * K + K * K)
        rows.append([int(math.floor(c * 2.0 ** 28 + 0.5)) for c in (n, -2.0 * n, n, 2.0 * (K * K - 1.0) * n, (1.0 - q * K + K * K) * n)])
    return rows


def min_power(amplitude, W):
    """floor((128 amplitude W)^2 / 4) for an integer amplitude."""
    return (128 * int(amplitude) * int(W)) ** 2 // 4


def decimate(hist, x):
    """Step 1: hist int64 [n][48], x int64 [n][128 m] -> d int64 [n][8 m]."""
    ext = np.concatenate([hist, x], axis=1)
    out = np.empty((x.shape[0], x.shape[1] // 16), dtype=np.int64)
    for k in range(out.shape[1]):
        newest = 48 + 16 * k + 15
        out[:, k] = (ext[:, newest - 45:newest + 1][:, ::-1] @ H + 2048) >> 12
    return out


def highpass(x, coef, hp):
    """Step 3 over x int64 [n][m] with the states hp int64 [n][3][4] (advanced in place): y int64 [n][m]."""
    if not coef:
        return x.copy()
    y = np.empty_like(x)
    lo, hi = -(1 << 30), (1 << 30) - 1
    for k in range(x.shape[1]):
        u = x[:, k] << 8
        for s, (b0, b1, b2, a1, a2) in enumerate(coef):
            acc = b0 * u + b1 * hp[:, s, 0] + b2 * hp[:, s, 1] - a1 * hp[:, s, 2] - a2 * hp[:, s, 3]   # int64, wraps
            o = np.clip((acc + (1 << 27)) >> 28, lo, hi)
            hp[:, s, 1], hp[:, s, 0], hp[:, s, 3], hp[:, s, 2] = hp[:, s, 0].copy(), u, hp[:, s, 2].copy(), o
            u = o
        y[:, k] = np.clip((u + 128) >> 8, -32768, 32767)
    return y


class ToneRef:
    """n_channels tone squelches, one numpy array per setting and per state field (st[name][c])."""

    def __init__(self, n_channels):
        self.n = int(n_channels)
        self.hz = list(CTCSS)
        self.steps = steps_from_hz(CTCSS)
        self.window, self.dominance, self.coef = 64, 64, []
        self.want = np.full(self.n, PASS, dtype=np.int64)
        self.min_power = np.zeros(self.n, dtype=U)
        self.hang_windows = np.zeros(self.n, dtype=np.int64)
        self.reset()

    def _sel(self, ch):
        return slice(None) if ch == -1 else int(ch)

    # bank-wide
    def _restart(self):
        self.st["acc"][:] = 0
        self.st["window_block"][:] = 0

    def set_tones(self, hz):
        s = steps_from_hz(hz)
        assert s is not None
        self.hz, self.steps = [float(f) for f in hz], s
        self._restart()

    def set_window(self, W):
        assert 16 <= W <= 128
        self.window = int(W)
        self._restart()

    def set_dominance(self, q4):
        assert 16 <= q4 <= 1024
        self.dominance = int(q4)

    def set_highpass(self, coef=None):
        coef = [] if coef is None else [[int(v) for v in row] for row in coef]
        assert len(coef) <= 3 and all(len(r) == 5 and all(-2**31 <= v < 2**31 for v in r) for r in coef)
        self.coef = coef

    # per channel
    def set_want(self, want, ch=-1):
        assert PASS <= want < len(self.steps)
        self.want[self._sel(ch)] = want

    def set_min_power(self, p, ch=-1):
        assert 0 <= p < 2**64
        self.min_power[self._sel(ch)] = p

    def set_hang(self, h, ch=-1):
        assert 0 <= h <= 255
        self.hang_windows[self._sel(ch)] = h

    def correlate(self, d):
        """Step 2 of one block: d int64 [n][8]."""
        st, T = self.st, len(self.steps)
        p = 8 * st["window_block"][:, None] + np.arange(8)[None, :]                                     # [n][8]
        i = ((np.asarray(self.steps, dtype=np.int64)[None, None, :] * p[:, :, None]) & 0xFFFFFFFF) >> 22   # [n][8][T]
        R = (d[:, :, None] * C[i]).sum(axis=1)
        S = (d[:, :, None] * C[(i - 256) & 1023]).sum(axis=1)
        st["acc"][:, :T, 0] = w32(st["acc"][:, :T, 0] + (R >> 9))
        st["acc"][:, :T, 1] = w32(st["acc"][:, :T, 1] + (S >> 9))

    def window_end(self, e):
        """Step 5's verdict for the channels e (an index array) whose window is complete."""
        st, T = self.st, len(self.steps)
        re, im = st["acc"][e, :T, 0], st["acc"][e, :T, 1]
        P = (re * re).astype(U) + (im * im).astype(U)                                                    # mod 2^64
        best = np.argmax(P, axis=1)                                                                       # the lowest index of the maximum
        far = np.abs(np.arange(T)[None, :] - best[:, None]) >= 2
        other = np.where(far, P, U(0)).max(axis=1).astype(U)
        Pb = P[np.arange(len(e)), best]
        ok = (Pb >= self.min_power[e]) & (U(16) * (Pb >> U(8)) >= U(self.dominance) * (other >> U(8)))
        det = np.where(ok, best, -1)
        want = self.want[e]
        match = np.where(want == PASS, True, np.where(want == ANY, det >= 0, det == want))
        was = st["open"][e] == 1
        hang = ~match & was & (st["hang_left"][e] > 0)
        shut = ~match & was & ~hang
        st["openings"][e] = (st["openings"][e] + (match & ~was)) & 0xFFFFFFFF
        st["open"][e] = np.where(match, 1, np.where(shut, 0, st["open"][e]))
        st["hang_left"][e] = np.where(match, self.hang_windows[e], st["hang_left"][e] - hang)
        st["windows"][e] = (st["windows"][e] + 1) & 0xFFFFFFFF
        st["matches"][e] = (st["matches"][e] + match) & 0xFFFFFFFF
        st["detected"][e], st["last_best"][e], st["last_power"][e], st["last_other"][e] = det, best, Pb, other
        st["acc"][e] = 0
        st["window_block"][e] = 0

    def update(self, x, n_blocks=None):
        """x int16 [n_channels][stride_blocks][128], of which the first n_blocks blocks are new.  Returns (out int16
        [n_channels][n_blocks][128], unmuted uint8 [n_channels][n_blocks]: whether each block left unmuted)."""
        x = np.asarray(x)
        assert x.dtype == np.int16 and x.shape[0] == self.n and x.shape[2] == 128
        nb = x.shape[1] if n_blocks is None else int(n_blocks)
        st = self.st
        out, unmuted = np.zeros((self.n, nb, 128), dtype=np.int16), np.zeros((self.n, nb), dtype=np.uint8)
        for b in range(nb):
            xb = x[:, b].astype(np.int64)
            d = decimate(st["hist"], xb)
            st["hist"] = np.concatenate([st["hist"], xb], axis=1)[:, -48:]
            self.correlate(d)
            y = highpass(xb, self.coef, st["hp"])
            keep = (self.want == PASS) | (st["open"] == 1)
            out[:, b] = np.where(keep[:, None], y, 0)
            unmuted[:, b] = keep
            st["open_blocks"] = (st["open_blocks"] + keep) & 0xFFFFFFFF
            st["window_block"] += 1
            e = np.flatnonzero(st["window_block"] == self.window)
            if e.size:
                self.window_end(e)
        self.blocks += nb
        return out, unmuted

    def clear(self):
        for k in ("windows", "matches", "openings", "open_blocks"):
            self.st[k][:] = 0
        self.blocks = 0

    def reset(self):
        n = self.n
        self.st = {"hist": np.zeros((n, 48), dtype=np.int64), "hp": np.zeros((n, 3, 4), dtype=np.int64), "last_power": np.zeros(n, dtype=U),
                   "last_other": np.zeros(n, dtype=U), "windows": np.zeros(n, dtype=np.int64), "matches": np.zeros(n, dtype=np.int64),
                   "openings": np.zeros(n, dtype=np.int64), "open_blocks": np.zeros(n, dtype=np.int64),
                   "detected": np.full(n, -1, dtype=np.int64), "last_best": np.full(n, -1, dtype=np.int64),
                   "window_block": np.zeros(n, dtype=np.int64), "hang_left": np.zeros(n, dtype=np.int64), "open": np.zeros(n, dtype=np.int64),
                   "reserved": np.zeros((n, 2), dtype=np.int64), "acc": np.zeros((n, 64, 2), dtype=np.int64)}
        self.blocks = 0

    def records(self):
        """The state as a structured array [n] of STATE_DTYPE."""
        rec = np.zeros(self.n, dtype=STATE_DTYPE)
        for k in STATE_NAMES:
            rec[k] = self.st[k]
        return rec

    def put(self, ch, record):
        """Writes one channel's state from a STATE_DTYPE (or equally named) record."""
        for k in STATE_NAMES:
            self.st[k][ch] = record[k]

    def decoded_hz(self):
        d = self.st["detected"]
        return np.where(d >= 0, np.asarray(self.hz)[np.clip(d, 0, len(self.hz) - 1)], np.nan)


# ---- signals
def to_int16(x):
    return np.clip(np.floor(np.asarray(x, dtype=np.float64) + 0.5), -32768, 32767).astype(np.int16)


def tone_wave(n_samples, hz, amplitude, phase=0.0, first=0):
    k = np.arange(first, first + n_samples, dtype=np.float64)
    return amplitude * np.sin(2.0 * np.pi * hz * k / FS + phase)


def voice_noise(rng, shape, rms):
    """Gaussian noise band-limited to 300 .. 3000 Hz along the last axis (an FFT brick wall), scaled to `rms`."""
    m = shape[-1]
    X = np.fft.rfft(rng.normal(0.0, 1.0, size=shape), axis=-1)
    f = np.fft.rfftfreq(m, 1.0 / FS)
    X[..., (f < 300.0) | (f > 3000.0)] = 0.0
    x = np.fft.irfft(X, n=m, axis=-1)
    return x * (rms / np.sqrt((x * x).mean(axis=-1, keepdims=True)))
