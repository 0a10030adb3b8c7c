"""Independent numpy restatement of a fast-convolution bank's filter palette and gains (include/asdr_tuner.h, "Filter palette and
gain"), written from that statement and not from the kernels.  TunerPaletteRef is tuner_fastconv_ref.TunerFastconvRef with a
palette of up to 64 responses (slot 0 is the channel filter), a slot and a gain per channel, stage 1 (float64, and the float32
model stage1_f32 that sizes the GPU tests' tolerance) with G_{f_c} and a_c, and reset() putting every channel back to slot 0 and
gain 1 with the palette kept.  PaletteMonitorRef is tuner_monitor_ref.MonitorRef with the channel's own G in the level, gain
excluded."""
import numpy as np

import tuner_fastconv_ref as F
import tuner_monitor_ref as M

MAX_FILTERS = 64
MAX_GAIN = 32768.0
BLOCK = F.BLOCK


def response_table(taps):
    """G_s[m] for m in [-128, 128) in m' = m mod 256 order: float64 sums of the float32 (or complex64) taps, each part rounded to
    float.  Real taps go through tuner_fastconv_ref.response_table, so a slot holding filter 0's taps holds filter 0's G."""
    taps = np.asarray(taps)
    if not np.iscomplexobj(taps):
        return F.response_table(taps)[0]
    g = taps.astype(np.complex64).astype(np.complex128)
    m = np.concatenate([np.arange(0, 128), np.arange(-128, 0)]).astype(np.float64)
    G = (g[None, :] * np.exp(-2j * np.pi * np.outer(m, np.arange(g.size)) / 256.0)).sum(axis=1)
    return G.astype(np.complex64).astype(np.complex128)


class TunerPaletteRef(F.TunerFastconvRef):
    def __init__(self, *args, **kw):
        self.palette = {}                                     # slot -> (taps as given: float32 or complex64, G)
        super().__init__(*args, **kw)

    def reset(self):
        super().reset()
        self.slot = np.zeros(self.n, dtype=np.int64)
        self.gain = np.ones(self.n, dtype=np.float32)

    # control plane
    def set_palette_filter(self, slot, taps):
        taps = np.asarray(taps)
        taps = taps.astype(np.complex64 if np.iscomplexobj(taps) else np.float32).reshape(-1)
        assert 1 <= slot < MAX_FILTERS and 1 <= taps.size <= F.TAPS and np.isfinite(taps).all()
        self.palette[int(slot)] = (taps, response_table(taps))

    def get_palette_filter(self, slot):
        if slot == 0:
            return self.get_channel_filter()
        return self.palette[slot][0] if slot in self.palette else None

    def clear_palette_filter(self, slot):
        assert 1 <= slot < MAX_FILTERS and not (self.slot == slot).any()
        self.palette.pop(int(slot), None)

    def set_channel_slot(self, slot, ch=-1):
        assert slot == 0 or slot in self.palette
        for c in self._chans(ch):
            self.slot[c] = slot

    def set_gain(self, gain, ch=-1):
        gain = np.float32(gain)
        assert np.isfinite(gain) and abs(float(gain)) <= MAX_GAIN
        for c in self._chans(ch):
            self.gain[c] = gain

    def slots(self):
        return self.slot.astype(np.int32)

    def gains(self):
        return self.gain.copy()

    def channel_G(self):
        """G_{f_c} of every channel, complex128 [n_channels][256] in m' order, as the palette stands now."""
        return np.stack([self.G if s == 0 else self.palette[int(s)][1] for s in self.slot])

    # stage 1: the parent's statement with G_{f_c}[m] for G[m], and a_c after the 1 / N scale and the coarse sign
    def _stage1(self, iq, fft, ctype):
        iq = np.asarray(iq)
        x = iq.astype(np.complex128) if np.iscomplexobj(iq) else iq[..., 0].astype(np.float64) + 1j * iq[..., 1].astype(np.float64)
        nf = x.shape[1] // self.H
        assert x.shape == (self.n_src, nf * self.H)
        k0, rw = F.coarse(self.fw, self.R)
        out = np.zeros((self.n, nf * BLOCK), dtype=ctype)
        n_keep = np.arange(BLOCK)
        G = self.channel_G().astype(ctype)
        real = np.float32 if ctype is np.complex64 else np.float64
        scale = real(256.0 / self.N)
        gain = self.gain.astype(real)[:, None]
        for f in range(nf):
            b = self.P // self.H
            win = np.concatenate([self.hist, x[:, f * self.H:(f + 1) * self.H]], axis=1)
            X = fft.fft(win.astype(ctype), axis=1)
            Z = X[self.src[:, None], (k0[:, None] + self.m[None, :]) % self.N] * G
            y = fft.ifft(Z, axis=1)[:, 128:] * scale
            y = y * np.where((k0 * (b - 1)) % 2 == 0, 1.0, -1.0)[:, None].astype(ctype)
            y = y * gain
            i = 128 * b + n_keep
            th = (self.ph_a[:, None] + rw[:, None] * ((i[None, :] * self.R - self.pos_a[:, None]) % (1 << 32))) % (1 << 32)
            th = np.where(th >= 1 << 31, th - (1 << 32), th)
            out[:, f * BLOCK:(f + 1) * BLOCK] = y * np.exp(-2j * np.pi * th / 4294967296.0).astype(ctype)
            assert out.dtype == X.dtype == y.dtype == ctype
            self.hist = win[:, self.H:]
            self.P += self.H
        return out


class PaletteMonitorRef(M.MonitorRef):
    """MonitorRef next to a TunerPaletteRef: the level is |y|^2 with the channel's G_{f_c} and without a_c."""

    def frame_energy(self, X):
        r = self.ref
        k0, _ = F.coarse(r.fw, r.R)
        Z = X[r.src[:, None], (k0[:, None] + r.m[None, :]) % self.N] * r.channel_G()
        n = np.arange(128, 256)
        E = np.exp(2j * np.pi * np.outer(r.m, n) / 256.0)      # the statement's sum, not an FFT routine
        y = (Z @ E) / self.N
        return (y.real ** 2 + y.imag ** 2).sum(axis=1)
