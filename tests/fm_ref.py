"""The FM demodulator's statement (include/asdr_fm.h) in numpy and Python integers, written from the header's text and independent
of the C++: the conjugate product, the 20-iteration integer CORDIC, the gain, the noise probe, DC removal, de-emphasis and the noise
squelch.  The GPU tests hold the kernel to it at tolerance 0; tests/test_fm_ref.py holds it to float64 atan2 and to known answers.
Everything is computed in int64 and wrapped where the header says int32."""
import math

import numpy as np

STATE_NAMES = ("prev_i", "prev_q", "v1", "v2", "s", "m", "last_noise", "last_power", "openings", "open_blocks", "hang_left", "open",
               "reserved", "reserved2")
STATE_TYPES = ("i2", "i2", "i2", "i2", "i4", "i4", "u8", "u8", "u4", "u4", "u2", "u1", "u1", "u4")
STATE_OFFSETS = (0, 2, 4, 6, 8, 12, 16, 24, 32, 36, 40, 42, 43, 44)
FS = 44100
ITERS = 20
MAX_GAIN = 1 << 24
MAX_NOISE = 1 << 41
ATAN = [int(math.floor(math.atan(2.0 ** -k) / (2.0 * math.pi) * 2.0 ** 32 + 0.5)) for k in range(ITERS)]


def gain_from_deviation(hz):
    """floor(32767 * 44100 / (2 hz) + 0.5); None outside 1 .. 2^24."""
    if not hz > 0:
        return None
    g = math.floor(32767.0 * FS / (2.0 * hz) + 0.5)
    return int(g) if 1 <= g <= MAX_GAIN else None


def deemphasis_from_tau_us(t):
    """floor(32768 * (1 - exp(-1e6 / (44100 t))) + 0.5); None outside 1 .. 32768."""
    if not t > 0:
        return None
    a = math.floor(32768.0 * (1.0 - math.exp(-1e6 / (FS * t))) + 0.5)
    return int(a) if 1 <= a <= 32768 else None


def w32(x):
    """int64 -> the int32 it wraps to, as int64."""
    return ((np.asarray(x, dtype=np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def clamp16(x):
    return np.clip(x, -32768, 32767)


def conj_product(I, Q, Ip, Qp):
    """Step 1 on int64 arrays: (re, im)."""
    I, Q, Ip, Qp = (np.asarray(v).astype(np.int64) for v in (I, Q, Ip, Qp))
    return I * Ip + Q * Qp, Q * Ip - I * Qp


def discriminator(re, im, with_peak=False):
    """Step 2: theta as int64 holding the int32 value (2^31 = pi).  with_peak: also the largest register magnitude met."""
    re, im = np.asarray(re, dtype=np.int64).copy(), np.asarray(im, dtype=np.int64).copy()
    big = np.maximum(np.abs(re), np.abs(im))
    zero = big == 0
    L = np.frexp(big.astype(np.float64))[1].astype(np.int64)        # the bit length: exact below 2^53
    sh = 29 - L
    left, right = np.maximum(sh, 0), np.maximum(-sh, 0)
    re, im = (re << left) >> right, (im << left) >> right
    neg = re < 0
    re, im = np.where(neg, -re, re), np.where(neg, -im, im)
    theta = np.where(neg, np.int64(1) << 31, np.int64(0))
    peak = np.maximum(np.abs(re), np.abs(im))
    for k in range(ITERS):
        up = im >= 0
        re, im = np.where(up, re + (im >> k), re - (im >> k)), np.where(up, im - (re >> k), im + (re >> k))
        theta = theta + np.where(up, ATAN[k], -ATAN[k])
        peak = np.maximum(peak, np.maximum(np.abs(re), np.abs(im)))
    theta = np.where(zero, 0, w32(theta))
    return (theta, peak) if with_peak else theta


def gain_stage(theta, G):
    """Step 3: v = clamp((theta * G) >> 31)."""
    return clamp16((np.asarray(theta, dtype=np.int64) * np.asarray(G, dtype=np.int64)) >> 31)


class FmRef:
    """n_channels demodulators, one numpy array per setting and per state field (st[name][c])."""

    def __init__(self, n_channels):
        self.n = int(n_channels)
        self.gain = np.full(self.n, gain_from_deviation(5000.0), dtype=np.int64)
        self.deemphasis = np.full(self.n, 32768, dtype=np.int64)
        self.hp_shift = np.zeros(self.n, dtype=np.int64)
        self.open_noise = np.full(self.n, MAX_NOISE, dtype=np.uint64)
        self.close_noise = np.full(self.n, MAX_NOISE, dtype=np.uint64)
        self.hang_blocks = np.zeros(self.n, dtype=np.uint16)
        self.reset()

    def _sel(self, ch):
        return slice(None) if ch == -1 else int(ch)

    def set_gain(self, g, ch=-1):
        assert 1 <= g <= MAX_GAIN
        self.gain[self._sel(ch)] = g

    def set_deemphasis(self, a, ch=-1):
        assert 1 <= a <= 32768
        self.deemphasis[self._sel(ch)] = a

    def set_dc_shift(self, k, ch=-1):
        assert 0 <= k <= 15
        self.hp_shift[self._sel(ch)] = k

    def set_squelch(self, open_noise, close_noise, hang_blocks, ch=-1):
        assert 0 <= open_noise <= close_noise <= MAX_NOISE and 0 <= hang_blocks <= 65535
        sel = self._sel(ch)
        self.open_noise[sel], self.close_noise[sel], self.hang_blocks[sel] = open_noise, close_noise, hang_blocks

    def demodulate(self, I, Q):
        """Steps 1 to 4 of new samples I, Q int16 [n][m]: v int64 [n][m], w [n][m]; advances prev_i, prev_q, v1, v2."""
        st = self.st
        I, Q = np.asarray(I).astype(np.int64), np.asarray(Q).astype(np.int64)
        Ip = np.concatenate([st["prev_i"].astype(np.int64)[:, None], I[:, :-1]], axis=1)
        Qp = np.concatenate([st["prev_q"].astype(np.int64)[:, None], Q[:, :-1]], axis=1)
        re, im = conj_product(I, Q, Ip, Qp)
        v = gain_stage(discriminator(re, im), self.gain[:, None])
        ext = np.concatenate([st["v2"].astype(np.int64)[:, None], st["v1"].astype(np.int64)[:, None], v], axis=1)
        w = ext[:, 2:] - 2 * ext[:, 1:-1] + ext[:, :-2]
        st["prev_i"][:], st["prev_q"][:] = I[:, -1], Q[:, -1]
        st["v1"][:], st["v2"][:] = ext[:, -1], ext[:, -2]
        return v, w

    def filters(self, v):
        """Steps 5 and 6, sample by sample over all channels: y int64 [n][m]; advances m and s."""
        st = self.st
        m, s = st["m"].astype(np.int64), st["s"].astype(np.int64)
        hp, a, on = self.hp_shift, self.deemphasis, self.hp_shift > 0
        y = np.empty_like(v)
        for k in range(v.shape[1]):
            vk = v[:, k]
            m = np.where(on, w32(m + (w32((vk << 15) - m) >> hp)), m)
            x = np.where(on, clamp16(vk - (w32(m + (1 << 14)) >> 15)), vk)
            s = w32(s + ((w32((x << 15) - s) * a) >> 15))
            y[:, k] = clamp16(w32(s + (1 << 14)) >> 15)
        st["m"][:], st["s"][:] = m, s
        return y

    def squelch(self, N, P):
        """One block of every channel: N, P uint64 [n].  Returns open after the block, uint8 [n]."""
        st = self.st
        was = st["open"] == 1
        quiet = N <= self.open_noise                          # if N <= open_noise
        hold = ~quiet & was & (N <= self.close_noise)         # elif open and N <= close_noise
        hang = ~quiet & ~hold & was & (st["hang_left"] > 0)   # elif open and hang_left > 0
        shut = ~quiet & ~hold & ~hang & was                   # elif open
        st["openings"] += (quiet & ~was).astype(np.uint32)
        st["open"][quiet] = 1
        st["open"][shut] = 0
        st["hang_left"][quiet | hold] = self.hang_blocks[quiet | hold]
        st["hang_left"][hang] -= 1
        st["open_blocks"] += st["open"].astype(np.uint32)
        st["last_noise"][:] = N
        st["last_power"][:] = P
        return st["open"].copy()

    def update(self, I, Q, n_blocks=None):
        """I, Q int16 [n_channels][stride_blocks][128], of which the first n_blocks blocks are new.  Returns (out int16
        [n_channels][n_blocks][128], opens uint8 [n_channels][n_blocks]: open after each block)."""
        I, Q = np.asarray(I), np.asarray(Q)
        assert I.dtype == np.int16 and Q.dtype == np.int16 and I.shape == Q.shape and I.shape[0] == self.n and I.shape[2] == 128
        nb = I.shape[1] if n_blocks is None else int(n_blocks)
        if nb == 0:
            return np.zeros((self.n, 0, 128), dtype=np.int16), np.zeros((self.n, 0), dtype=np.uint8)
        I, Q = I[:, :nb].reshape(self.n, nb * 128), Q[:, :nb].reshape(self.n, nb * 128)
        v, w = self.demodulate(I, Q)
        y = self.filters(v).reshape(self.n, nb, 128)
        N = (w * w).reshape(self.n, nb, 128).sum(axis=2).astype(np.uint64)
        I64, Q64 = I.astype(np.int64), Q.astype(np.int64)
        P = (I64 * I64 + Q64 * Q64).reshape(self.n, nb, 128).sum(axis=2).astype(np.uint64)
        opens = np.stack([self.squelch(N[:, b], P[:, b]) for b in range(nb)], axis=1)
        self.blocks += nb
        out = np.where(opens[:, :, None] == 1, y, 0).astype(np.int16)
        return out, opens

    def clear(self):
        self.st["openings"][:] = 0
        self.st["open_blocks"][:] = 0
        self.blocks = 0

    def reset(self):
        self.st = {k: np.zeros(self.n, dtype=t) for k, t in zip(STATE_NAMES, STATE_TYPES)}
        self.blocks = 0

    def put(self, ch, values):
        """Writes one channel's state from a tuple in STATE_NAMES order (as state_tuples() gives)."""
        for k, v in zip(STATE_NAMES, values):
            self.st[k][ch] = v

    def state_tuples(self):
        return list(zip(*[self.st[k].tolist() for k in STATE_NAMES]))

    def offset_hz(self, deviation_hz):
        """The tuning offset the DC meter reads: m / 2^15 is the mean of v, and v = 32767 at deviation_hz."""
        return self.st["m"].astype(np.float64) / 32768.0 / 32767.0 * float(deviation_hz)


def record_tuples(records):
    """A structured FM_STATE_DTYPE array as the list FmRef.state_tuples() gives."""
    return list(zip(*[records[k].tolist() for k in STATE_NAMES]))


def fm_iq(n_samples, amplitude, mod_hz=1000.0, deviation_hz=3000.0, offset_hz=0.0, noise=0.0, rng=None, phase0=0.0):
    """int16 (I, Q) [n_samples] of an FM carrier at baseband: a tone of mod_hz at deviation_hz, a tuning offset, complex Gaussian
    noise of standard deviation `noise` per component.  The phase is the exact integral of the instantaneous frequency."""
    n = np.arange(n_samples, dtype=np.float64)
    phi = phase0 + 2.0 * np.pi * offset_hz * n / FS
    if deviation_hz:
        phi = phi + deviation_hz / mod_hz * np.sin(2.0 * np.pi * mod_hz * n / FS)
    I, Q = amplitude * np.cos(phi), amplitude * np.sin(phi)
    if noise:
        I, Q = I + rng.normal(0.0, noise, n_samples), Q + rng.normal(0.0, noise, n_samples)
    r = lambda x: np.clip(np.floor(x + 0.5), -32768, 32767).astype(np.int16)
    return r(I), r(Q)
