"""Independent numpy restatement of a fast-convolution bank (include/asdr_tuner.h, "Fast-convolution banks"), written from that
statement and not from the kernels.  Stage 1 runs frame by frame in float64 with np.fft: the N-point DFT of each source's window,
256 bins around the channel's coarse bin weighted by G, a 256-point inverse DFT, the second half kept, the coarse sign and the
fine NCO applied exactly.  Stage 2 is tuner_rate_ref's resampler and block timing, unchanged."""
import math

import numpy as np

import tuner_rate_ref as RR

BLOCK = 128
TAPS = 129
BETA = 7.857
PASS_HZ = 11500.0


def sizes(R):
    """(H, N, q): frame hop, FFT size and 2^32 / N."""
    return 128 * R, 256 * R, (1 << 32) // (256 * R)


def ratio(fs_in, R):
    """(U, M) = 44100 R / Fs_in in lowest terms."""
    g = math.gcd(44100 * R, fs_in)
    return 44100 * R // g, fs_in // g


def valid(fs_in, R):
    if R < 2 or R > 1024 or R & (R - 1) or fs_in <= 0:
        return False
    if not 44100 * R <= fs_in <= 176400 * R:
        return False
    return ratio(fs_in, R)[0] <= 2048


def coarse(fw, R):
    """(k0, rw) of frequency words fw (uint32 ints or arrays): k0 = floor(((int32) fw + q/2) / q), rw = (int32)(fw - k0 q)."""
    _, _, q = sizes(R)
    fw = np.asarray(fw, dtype=np.int64) & 0xFFFFFFFF
    s = np.where(fw >= 1 << 31, fw - (1 << 32), fw)
    k0 = (s + q // 2) // q
    rw = (fw - k0 * q) & 0xFFFFFFFF
    return k0, np.where(rw >= 1 << 31, rw - (1 << 32), rw)


def default_channel_filter(fs_mid):
    """Kaiser (beta 7.857) windowed sinc of 129 taps, cut-off 11.5 kHz + delta / 2 with delta = 0.0392 Fs_mid, sum 1 (float64)."""
    fc = (PASS_HZ + 0.5 * 0.0392 * fs_mid) / fs_mid
    n = np.arange(TAPS, dtype=np.float64)
    x = n - 0.5 * (TAPS - 1)
    u = 2.0 * n / (TAPS - 1) - 1.0
    s = np.where(x == 0, 2.0 * fc, np.sin(2.0 * np.pi * fc * x) / (np.pi * np.where(x == 0, 1.0, x)))
    w = s * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(BETA)
    return w / w.sum()


def response(g, m):
    """G at m (bins of Fs_mid / 256, any real m): sum_n g[n] e^{-j 2 pi m n / 256}, float64."""
    g = np.asarray(g, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    return (g[None, :] * np.exp(-2j * np.pi * np.outer(m.reshape(-1), np.arange(g.size)) / 256.0)).sum(axis=1).reshape(m.shape)


def response_table(g):
    """G[m] for m in [-128, 128), computed in float64 and rounded to complex64 as the host does, in m' = m mod 256 order."""
    m = np.concatenate([np.arange(0, 128), np.arange(-128, 0)])
    G = response(np.asarray(g, dtype=np.float32).astype(np.float64), m)
    return G.astype(np.complex64).astype(np.complex128), m


class TunerFastconvRef:
    """A fast-convolution bank: stage 1 in float64 as stated, then the rate-bank stage 2 with every channel's whole u kept."""

    def __init__(self, n_channels, n_sources, fs_in, R, g=None, h2=None, g2=1):
        self.n, self.n_src, self.fs_in, self.R = int(n_channels), int(n_sources), int(fs_in), int(R)
        assert valid(self.fs_in, self.R)
        self.H, self.N, self.q = sizes(self.R)
        self.fs_mid = self.fs_in / self.R
        self.U, self.M = ratio(self.fs_in, self.R)
        self.set_channel_filter(default_channel_filter(self.fs_mid) if g is None else g)
        self.h2 = None                                        # stage 1 alone (stage1()) needs no stage 2
        if h2 is not None or self.U == self.M == 1:
            self.set_resampler((16384,) if h2 is None else h2, g2)
        self.reset()

    def reset(self):
        self.P = 0
        self.src = np.zeros(self.n, dtype=np.int64)
        self.fw = np.zeros(self.n, dtype=np.int64)
        self.pos_a = np.zeros(self.n, dtype=np.int64)
        self.ph_a = np.zeros(self.n, dtype=np.int64)
        self.hist = np.zeros((self.n_src, self.H), dtype=np.complex128)
        self.u = np.zeros((self.n, 2, 0), dtype=np.int64)
        self.out_pos = 0
        self.zero_before = 0
        self.stale = False

    # control plane
    def set_channel_filter(self, g):
        self.g = np.asarray(g, dtype=np.float32).astype(np.float64)
        self.G, self.m = response_table(self.g)

    def get_channel_filter(self):
        return self.g.astype(np.float32)

    def set_resampler(self, h2, g2):
        self.h2, self.g2 = np.asarray(h2, dtype=np.int64), int(g2)
        assert self.h2.size % self.U == 0

    def _chans(self, ch):
        return range(self.n) if ch == -1 else [ch]

    def theta(self, c, pos):
        """Fine-NCO phase of channel c at input position pos (uint32)."""
        _, rw = coarse(self.fw[c], self.R)
        return (int(self.ph_a[c]) + int(rw) * (pos - int(self.pos_a[c]))) & 0xFFFFFFFF

    def _retune(self, ch, **kw):
        for c in self._chans(ch):
            self.ph_a[c] = self.theta(c, self.P)
            self.pos_a[c] = self.P
            for k, v in kw.items():
                getattr(self, k)[c] = v

    def set_source(self, s, ch=-1):
        self._retune(ch, src=s)

    def set_frequency_word(self, fw, ch=-1):
        self._retune(ch, fw=int(fw) & 0xFFFFFFFF)

    def set_frequency(self, hz, ch=-1):
        self.set_frequency_word(RR.fw_from_hz(hz, self.fs_in), ch)

    def set_phase(self, ph, ch=-1):
        self._retune(ch, ph_a=int(ph) & 0xFFFFFFFF)

    # stage 1
    def stage1(self, iq):
        """iq: [n_sources][n_frames * H][2].  Returns u before rounding, complex128 [n_channels][n_frames * 128]; advances P."""
        return self._stage1(iq, np.fft, np.complex128)

    def stage1_f32(self, iq):
        """stage1() with the arithmetic of the statement held in float32: the window, X, G, the gathered product, the inverse
        transform, the 1 / N scale and the NCO product are complex64 (scipy.fft keeps complex64; numpy's would promote).  The phase
        theta stays an exact integer and its phasor is the float64 one rounded to complex64.  A model of what float32 costs the
        statement -- of no kernel's pass order -- used to size the tests' tolerance."""
        import scipy.fft
        return self._stage1(iq, scipy.fft, np.complex64).astype(np.complex128)

    def _stage1(self, iq, fft, ctype):
        iq = np.asarray(iq)                                   # CS16 pairs, or complex samples for known-answer checks
        x = iq.astype(np.complex128) if np.iscomplexobj(iq) else iq[..., 0].astype(np.float64) + 1j * iq[..., 1].astype(np.float64)
        nf = x.shape[1] // self.H
        assert x.shape == (self.n_src, nf * self.H)
        k0, rw = coarse(self.fw, self.R)
        out = np.zeros((self.n, nf * BLOCK), dtype=ctype)
        n_keep = np.arange(BLOCK)
        G = self.G.astype(ctype)
        scale = (np.float32 if ctype is np.complex64 else np.float64)(256.0 / self.N)
        for f in range(nf):
            b = self.P // self.H
            win = np.concatenate([self.hist, x[:, f * self.H:(f + 1) * self.H]], axis=1)
            X = fft.fft(win.astype(ctype), axis=1)
            Z = X[self.src[:, None], (k0[:, None] + self.m[None, :]) % self.N] * G[None, :]
            y = fft.ifft(Z, axis=1)[:, 128:] * scale
            y = y * np.where((k0 * (b - 1)) % 2 == 0, 1.0, -1.0)[:, None].astype(ctype)
            i = 128 * b + n_keep
            th = (self.ph_a[:, None] + rw[:, None] * ((i[None, :] * self.R - self.pos_a[:, None]) % (1 << 32))) % (1 << 32)
            th = np.where(th >= 1 << 31, th - (1 << 32), th)
            out[:, f * BLOCK:(f + 1) * BLOCK] = y * np.exp(-2j * np.pi * th / 4294967296.0).astype(ctype)
            assert out.dtype == X.dtype == y.dtype == ctype
            self.hist = win[:, self.H:]
            self.P += self.H
        return out

    def place_at(self, P, hist):
        """Put a pass-through bank where a run of P input samples per source would have left it, without running it: P (a multiple
        of H), the output position 128 P / H, the sources' windows hist [n_sources][H] (CS16 pairs or complex: the last H samples
        fed).  Channels (src, fw, anchors) stay as they are -- an anchor set at position 0 stays (0, ph_a), as it would have.  Stage
        1 keeps nothing else between frames; a resampling stage 2 would (its u history), hence pass-through only."""
        assert self.pass_through() and P % self.H == 0 and P >= 0
        hist = np.asarray(hist)
        h = hist.astype(np.complex128) if np.iscomplexobj(hist) else hist[..., 0].astype(np.float64) + 1j * hist[..., 1].astype(np.float64)
        assert h.shape == (self.n_src, self.H)
        self.P, self.hist = int(P), h
        self.out_pos = BLOCK * (self.P // self.H)
        self.u = np.zeros((self.n, 2, 0), dtype=np.int64)
        self.stale = True

    @staticmethod
    def round16(z):
        return (np.clip(np.rint(z.real), -32768, 32767).astype(np.int64), np.clip(np.rint(z.imag), -32768, 32767).astype(np.int64))

    # stage 2 (tuner_rate_ref's, unchanged)
    def pass_through(self):
        return RR.is_pass_through(self.h2, self.g2, self.U, self.M)

    def out_blocks(self, n_frames):
        if self.pass_through():
            return n_frames
        return max(0, RR.blocks_out(self.u.shape[-1] + BLOCK * n_frames, self.U, self.M) - self.out_pos // BLOCK)

    def update(self, iq, keep_float=False, f32=False):
        """iq: [n_sources][n_frames * H][2].  Returns (I, Q) int16 [n_channels][blocks written][128] (and u before rounding).
        f32: stage 1 by stage1_f32()."""
        assert self.h2 is not None, "give the stage-2 taps of a resampling bank"
        nf = np.asarray(iq).shape[1] // self.H
        nb = self.out_blocks(nf)
        z = self.stage1_f32(iq) if f32 else self.stage1(iq)
        I1, Q1 = self.round16(z)
        n_u0 = self.u.shape[-1]
        self.u = np.concatenate([self.u, np.stack([I1, Q1], axis=1)], axis=-1)
        if self.pass_through():
            self.stale = True
            self.out_pos += nf * BLOCK
            res = (I1.reshape(self.n, nf, BLOCK).astype(np.int16), Q1.reshape(self.n, nf, BLOCK).astype(np.int16))
        else:
            if self.stale:
                self.zero_before, self.stale = n_u0, False
            y = RR.resample(self.u, self.h2, self.U, self.M, self.g2, self.out_pos, nb * BLOCK, self.zero_before)
            self.out_pos += nb * BLOCK
            res = (y[:, 0].reshape(self.n, nb, BLOCK).astype(np.int16), y[:, 1].reshape(self.n, nb, BLOCK).astype(np.int16))
        return res + (z,) if keep_float else res
