"""Independent numpy restatement of a fast-convolution bank's monitors (include/asdr_tuner.h, "Monitors"), written from that
statement and not from the kernels.  MonitorRef runs next to a tuner_fastconv_ref.TunerFastconvRef, whose channel state (src, fw,
G) it reads and whose stage 1 it never calls: it keeps the sources' windows itself, takes X = DFT_N(window) per frame in float64,
and from it the spectrum (window combine, |W|^2 / N^2, groups of g bins, sum or peak over frames) and the levels (the 256 gathered
bins times G, the inverse transform, the kept half's |y|^2, before NCO, rounding and clamp).  powers(..., f32=True) is a float32
model of the spectrum's statement -- of no kernel's order of operations -- that sizes the GPU test's tolerance."""
import numpy as np

import tuner_fastconv_ref as F

WINDOWS = ("rect", "hann")
MODES = ("sum", "peak")


def powers(X, n_bins, window, f32=False):
    """P_b[j] of one frame: X complex [n_src][N] -> float64 [n_src][n_bins].  f32: X is complex64 and the combine, |W|^2 / N^2 and
    the group sums stay in float32."""
    N = X.shape[1]
    g = N // n_bins
    assert window in WINDOWS and n_bins * g == N and n_bins >= 256 and n_bins & (n_bins - 1) == 0
    if f32:
        assert X.dtype == np.complex64
        half, quarter, inv = np.float32(0.5), np.float32(0.25), np.float32(1.0 / N) * np.float32(1.0 / N)
    else:
        X = X.astype(np.complex128)
        half, quarter, inv = 0.5, 0.25, 1.0 / (float(N) * float(N))
    W = X if window == "rect" else X * half - (np.roll(X, 1, axis=1) + np.roll(X, -1, axis=1)) * quarter
    p = (W.real * W.real + W.imag * W.imag) * inv
    assert p.dtype == (np.float32 if f32 else np.float64)
    return p.reshape(X.shape[0], n_bins, g).sum(axis=2).astype(np.float64)


def frequencies(fs_in, n_bins):
    """Start of output bin j in Hz relative to the capture's centre (FFT order)."""
    j = np.arange(n_bins)
    return np.where(j < n_bins // 2, j, j - n_bins) * (fs_in / n_bins)


class MonitorRef:
    """The monitors of the bank that `ref` (a TunerFastconvRef) restates.  update(iq) takes the rows ref.update() takes (converted
    samples: CS16 pairs or complex) and must see the same calls; retunes and filter changes are read from ref at each call."""

    def __init__(self, ref, n_bins=0, window="hann", mode="sum", levels=False):
        self.ref = ref
        self.H, self.N = ref.H, ref.N
        self.hist = np.zeros((ref.n_src, self.H), dtype=np.complex128)
        self.b = 0                                            # frames since creation / reset
        self.enable_spectrum(n_bins, window, mode)
        self.enable_levels(levels)

    def enable_spectrum(self, n_bins, window="hann", mode="sum"):
        assert window in WINDOWS and mode in MODES
        self.n_bins, self.window, self.mode = int(n_bins), window, mode
        self.clear_spectrum()

    def enable_levels(self, on=True):
        self.levels_on = bool(on)
        self.clear_levels()

    def clear_spectrum(self):
        self.acc = np.zeros((self.ref.n_src, self.n_bins), dtype=np.float64)
        self.frames = 0

    def clear_levels(self):
        self.level = np.zeros(self.ref.n, dtype=np.float64)
        self.level_frames = 0

    def reset(self):
        self.hist[:] = 0
        self.b = 0
        self.clear_spectrum(); self.clear_levels()

    def place_at(self, P, hist):
        """As TunerFastconvRef.place_at: the windows a run of P samples would have left."""
        hist = np.asarray(hist)
        h = hist.astype(np.complex128) if np.iscomplexobj(hist) else hist[..., 0].astype(np.float64) + 1j * hist[..., 1].astype(np.float64)
        assert h.shape == self.hist.shape and P % self.H == 0
        self.hist, self.b = h, P // self.H

    def windows(self, iq):
        """The call's windows, complex128 [n_frames][n_src][N]; advances the history."""
        iq = np.asarray(iq)
        x = iq.astype(np.complex128) if np.iscomplexobj(iq) else iq[..., 0].astype(np.float64) + 1j * iq[..., 1].astype(np.float64)
        nf = x.shape[1] // self.H
        assert x.shape == (self.ref.n_src, nf * self.H)
        out = []
        for f in range(nf):
            win = np.concatenate([self.hist, x[:, f * self.H:(f + 1) * self.H]], axis=1)
            out.append(win)
            self.hist = win[:, self.H:]
            self.b += 1
        return out

    def frame_energy(self, X):
        """e_b[c] of one frame from X [n_src][N] (float64): sum over n = 128 .. 255 of |y[n]|^2."""
        r = self.ref
        k0, _ = F.coarse(r.fw, r.R)
        Z = X[r.src[:, None], (k0[:, None] + r.m[None, :]) % self.N] * r.G[None, :]
        n = np.arange(128, 256)
        E = np.exp(2j * np.pi * np.outer(r.m, n) / 256.0)      # the statement's sum, not an FFT routine
        y = (Z @ E) / self.N
        return (y.real ** 2 + y.imag ** 2).sum(axis=1)

    def update(self, iq):
        """Accumulate one call.  Returns the per-frame (P_b or None, e_b or None) for tests that look at single frames."""
        per_frame = []
        for win in self.windows(iq):
            X = np.fft.fft(win, axis=1)
            P = e = None
            if self.n_bins:
                P = powers(X, self.n_bins, self.window)
                self.acc = self.acc + P if self.mode == "sum" else np.maximum(self.acc, P)
                self.frames += 1
            if self.levels_on:
                e = self.frame_energy(X)
                self.level += e
                self.level_frames += 1
            per_frame.append((P, e))
        return per_frame

    def amplitude(self):
        """sqrt(acc / frames) (sum) or sqrt(acc) (peak): the domain the GPU test compares in."""
        return amplitude(self.acc, self.frames, self.mode)

    def rms(self):
        return np.sqrt(self.level / (128.0 * max(self.level_frames, 1)))


def amplitude(acc, frames, mode):
    return np.sqrt(acc / max(frames, 1)) if mode == "sum" else np.sqrt(acc)
