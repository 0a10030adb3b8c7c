"""Independent numpy restatement of the digital tuner bank's arithmetic (include/asdr_tuner.h), written from that statement and not
from the kernel.  Integer-only: the mixer runs in int64; the filter sums run as float64 dot products, which are exact here because
every product is an integer below 2^31 and every sum of at most 1024 of them stays below 2^53."""
import math

import numpy as np

BLOCK = 128
NCO_SIZE = 4096


def nco_table():
    """(C, S) int64 [4096]: round(32767 cos / sin (2 pi k / 4096)) in float64."""
    k = np.arange(NCO_SIZE, dtype=np.float64)
    return (np.round(32767.0 * np.cos(2.0 * np.pi * k / NCO_SIZE)).astype(np.int64),
            np.round(32767.0 * np.sin(2.0 * np.pi * k / NCO_SIZE)).astype(np.int64))


NCO_C, NCO_S = nco_table()


def sat16(v):
    return np.clip(v, -32768, 32767)


def fw_from_hz(hz, D):
    """The frequency word set_frequency(hz) stores: (uint32)(int64) llround(hz * 2^32 / Fs_in), Fs_in = D * 44100."""
    v = hz * 4294967296.0 / (44100.0 * D)
    r = math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1)      # llround: halves away from zero
    return int(r) & 0xFFFFFFFF


def theta(m, pos_a, ph_a, fw):
    """NCO phase at global sample indices m (int64 array, m >= pos_a meaningful): ph_a + (m - pos_a) fw mod 2^32."""
    d = (np.asarray(m, dtype=np.int64) - np.int64(pos_a)).astype(np.uint64) & np.uint64(0xFFFFFFFF)   # the product stays below 2^64
    return ((np.uint64(ph_a) + d * np.uint64(fw)) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def mix(xr, xi, th):
    """zr, zi of samples (xr, xi) at phases th (int64 arrays)."""
    k = th >> 20
    c, s = NCO_C[k], NCO_S[k]
    xr, xi = np.asarray(xr, dtype=np.int64), np.asarray(xi, dtype=np.int64)
    return sat16((xr * c + xi * s + 16384) >> 15), sat16((xi * c - xr * s + 16384) >> 15)


def fir_decimate(z, h, D, g, n_out):
    """I[n] = sat16((sum_k h[k] z[nD + D - 1 - k] + r) >> s) for n < n_out, with z given from sample D - L on (z[0] = sample D - L,
    the first input of output 0); returns int64 [n_out]."""
    L = len(h)
    z = np.asarray(z, dtype=np.float64)
    assert z.size == (n_out - 1) * D + L
    W = np.lib.stride_tricks.sliding_window_view(z, L)[::D][:n_out]
    acc = np.rint(W @ np.asarray(h, dtype=np.float64)[::-1]).astype(np.int64)
    s = 15 - g
    r = (1 << (s - 1)) if s else 0
    return sat16((acc + r) >> s)


def default_filter_spec(D):
    """(passband edge Hz, stopband start Hz, Fs_in) of the default filter's response requirement."""
    return 11200.0, 32100.0, 44100.0 * D


def fed_tail(buf, counts, T):
    """The last T samples per row of a feed whose call i took the first counts[i] samples of every row of buf."""
    parts, need = [], T
    for n in reversed(counts):
        take = min(n, need)
        parts.append(buf[:, n - take:n])
        need -= take
        if need == 0:
            break
    assert need == 0
    return np.concatenate(parts[::-1], axis=1)


class TunerRef:
    """The bank's state machine: position P, per-channel (src, fw, pos_a, ph_a), one filter, and every source's input from sample
    x0 on (x0 = 0: the whole input; place_at() keeps a tail only)."""

    def __init__(self, n_channels, n_sources, D, h=(16384,), g=1):
        self.n, self.n_src, self.D = n_channels, n_sources, D
        self.P = 0
        self.src = np.zeros(n_channels, dtype=np.int64)
        self.fw = np.zeros(n_channels, dtype=np.int64)
        self.pos_a = np.zeros(n_channels, dtype=np.int64)
        self.ph_a = np.zeros(n_channels, dtype=np.int64)
        self.x0 = 0
        self.x = [np.zeros((0, 2), dtype=np.int64) for _ in range(n_sources)]
        self.set_filter(h, g)

    def set_filter(self, h, g):
        self.h, self.g = np.asarray(h, dtype=np.int64), int(g)

    def _chans(self, ch):
        return range(self.n) if ch == -1 else [ch]

    def _reanchor(self, c):
        self.ph_a[c] = int(theta(self.P, self.pos_a[c], self.ph_a[c], self.fw[c]))
        self.pos_a[c] = self.P

    def set_source(self, s, ch=-1):
        for c in self._chans(ch):
            self._reanchor(c); self.src[c] = s

    def set_frequency_word(self, fw, ch=-1):
        for c in self._chans(ch):
            self._reanchor(c); self.fw[c] = int(fw) & 0xFFFFFFFF

    def set_frequency(self, hz, ch=-1):
        self.set_frequency_word(fw_from_hz(hz, self.D), ch)

    def set_phase(self, ph, ch=-1):
        for c in self._chans(ch):
            self.pos_a[c] = self.P; self.ph_a[c] = int(ph) & 0xFFFFFFFF

    def place_at(self, P, tail=None):
        """Put the reference where a run of P input samples per source would have left it, without running it.  tail
        [n_sources][T][2] holds the last T samples fed (samples P - T .. P - 1), T >= 1024 or all P of them: the longest filter
        reaches 1023 samples back.  Channels (src, fw, anchors) stay as they are -- an anchor set at position 0 stays (0, ph_a), as
        it would have; the bank keeps nothing else between calls.  Without a tail only P moves (setters then re-anchor there) and no
        sample is held: the next update() needs a place_at() with a tail first, unless every channel was re-anchored."""
        P = int(P)
        assert P >= 0 and P % (BLOCK * self.D) == 0
        if tail is None:
            tail = np.zeros((self.n_src, 0, 2), dtype=np.int64)
        else:
            tail = np.asarray(tail, dtype=np.int64)
            assert tail.shape[0] == self.n_src and tail.shape[2:] == (2,) and (tail.shape[1] >= 1024 or tail.shape[1] == P)
            assert tail.shape[1] <= P
        self.P, self.x0 = P, P - tail.shape[1]
        self.x = [tail[s].copy() for s in range(self.n_src)]

    def z(self, c, m):
        """zr, zi of channel c at global sample indices m: zero before the anchor and before 0, as the statement has it; every other
        sample must be one of those held (a sample that is not there is an error, never a zero)."""
        x = self.x[self.src[c]]
        ok = (m >= self.pos_a[c]) & (m >= 0)
        i = m - self.x0
        assert ((i >= 0) & (i < x.shape[0]))[ok].all(), "sample outside the %d held from %d on" % (x.shape[0], self.x0)
        mm, i = np.where(ok, m, self.pos_a[c]), np.where(ok, i, 0)
        zr, zi = mix(x[i, 0], x[i, 1], theta(mm, self.pos_a[c], self.ph_a[c], self.fw[c]))
        return np.where(ok, zr, 0), np.where(ok, zi, 0)

    def outputs(self, n0, n_out):
        """(I, Q) int16 [n][n_out]: outputs n0 .. n0 + n_out - 1 of every channel as it stands, from the samples held."""
        L = len(self.h)
        m = np.arange(n0 * self.D + self.D - L, (n0 + n_out) * self.D, dtype=np.int64)
        I = np.empty((self.n, n_out), dtype=np.int16)
        Q = np.empty_like(I)
        done = {}
        for c in range(self.n):
            key = (int(self.src[c]), int(self.fw[c]), int(self.pos_a[c]), int(self.ph_a[c]))
            if key not in done:
                zr, zi = self.z(c, m)
                done[key] = (fir_decimate(zr, self.h, self.D, self.g, n_out), fir_decimate(zi, self.h, self.D, self.g, n_out))
            I[c], Q[c] = done[key]
        return I, Q

    def update(self, iq):
        """iq: [n_sources][n_blocks * 128 * D][2].  Returns (I, Q) int16 [n][n_blocks][128]."""
        iq = np.asarray(iq, dtype=np.int64)
        N = iq.shape[1]
        nb = N // (BLOCK * self.D)
        assert N == nb * BLOCK * self.D
        for s in range(self.n_src):
            self.x[s] = np.concatenate([self.x[s], iq[s]])
        I, Q = self.outputs(self.P // self.D, nb * BLOCK)
        self.P += N
        return I.reshape(self.n, nb, BLOCK), Q.reshape(self.n, nb, BLOCK)
