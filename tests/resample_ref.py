"""The audio resampler's statement (include/asdr_resample.h) in numpy and Python integers, written from the header's text and
independent of the C++: the rate, the filter's acceptance rule, the outputs of a call from the position N and the 256-sample
records, and the default design.  The GPU tests hold the kernels to it at tolerance 0; tests/test_resample_ref.py holds it to an
explicit per-output Python loop and to the header's known answers."""
import math

import numpy as np

FS_IN = 44100
STATE = 256
MAX_UP, MAX_RATIO, MAX_TAPS, MAX_ABS_SUM = 512, 16, 256, 65535
DEFAULT_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000)


def ratio(fs_out):
    """(U, M) of Fs_out = 44100 U / M."""
    g = math.gcd(int(fs_out), FS_IN)
    return int(fs_out) // g, FS_IN // g


def accepted(up, down, taps, shift):
    """The header's acceptance rule for a rate and a filter h[k U + phi]."""
    h = np.asarray(taps, dtype=np.int64).reshape(-1)
    if not (1 <= up <= MAX_UP and up <= down <= MAX_RATIO * up and 0 <= shift <= 15):
        return False
    if h.size == 0 or h.size % up or not 1 <= h.size // up <= MAX_TAPS or h.min() < -32768 or h.max() > 32767:
        return False
    return int(np.abs(h.reshape(-1, up)).sum(axis=0).max()) <= MAX_ABS_SUM


def ceil_div(a, b):
    return -((-int(a)) // int(b))


def out_range(n0, n1, up, down):
    """The outputs a call that takes N from n0 to n1 writes: j0 .. j1 - 1."""
    return ceil_div(n0 * up, down), ceil_div(n1 * up, down)


def default_filter(fs_out):
    """The default design: (taps int16 [U K] as h[k U + phi], shift).  44100 Hz gives the identity {16384}, shift 14."""
    up, down = ratio(fs_out)
    if up == down == 1:
        return np.array([16384], dtype=np.int16), 14
    dw = 2.0 * np.pi * 0.16 * fs_out / (up * FS_IN)
    K = 2 * int(math.ceil((80.0 - 7.95) / (2.285 * dw) / (2.0 * up)))
    L = up * K
    fc = 0.5 * fs_out / (up * FS_IN)
    proto = 2.0 * fc * np.sinc(2.0 * fc * (np.arange(L) - 0.5 * (L - 1))) * np.kaiser(L, 0.1102 * (80.0 - 8.7))
    ph = proto.reshape(K, up)
    q = np.rint(32768.0 * ph / ph.sum(axis=0)).astype(np.int64)
    big = np.abs(q).argmax(axis=0)
    q[big, np.arange(up)] += 32768 - q.sum(axis=0)
    return q.reshape(-1).astype(np.int16), 15


def response_db(taps, up, n_fft=1 << 20):
    """|H| in dB of the prototype h (at U 44100 Hz, DC gain U) relative to its DC gain, and the frequencies in Hz."""
    h = np.asarray(taps, dtype=np.float64)
    H = np.abs(np.fft.rfft(h, n_fft)) / abs(h.sum())
    f = np.arange(H.size) * (up * FS_IN / n_fft)
    return 20.0 * np.log10(np.maximum(H, 1e-12)), f


class ResampleRef:
    """n_channels resamplers in lockstep: N, the 256-sample records, and update(), which forms a call's outputs for all channels
    at once: one gather of the K samples behind every output, one product, one sum, in int64."""

    def __init__(self, n_channels, up, down, taps, shift):
        assert accepted(up, down, taps, shift)
        self.n, self.up, self.down = int(n_channels), int(up), int(down)
        self.set_filter(taps, shift)
        self.reset()

    def set_filter(self, taps, shift):
        assert accepted(self.up, self.down, taps, shift)
        self.h = np.asarray(taps, dtype=np.int64).reshape(-1, self.up)      # [k][phi]
        self.K, self.shift = self.h.shape[0], int(shift)
        self.round = (1 << (self.shift - 1)) if self.shift else 0

    def reset(self):
        self.N = 0
        self.state = np.zeros((self.n, STATE), dtype=np.int16)

    def out_samples(self, n_blocks):
        j0, j1 = out_range(self.N, self.N + 128 * int(n_blocks), self.up, self.down)
        return j1 - j0

    def output_position(self):
        return ceil_div(self.N * self.up, self.down)

    def update(self, audio, n_blocks=None):
        """audio int16 [n_channels][stride_blocks][128], of which the first n_blocks blocks are new.  Returns int16
        [n_channels][count]: this call's outputs of every channel."""
        audio = np.asarray(audio)
        assert audio.dtype == np.int16 and audio.shape[0] == self.n and audio.shape[2] == 128
        nb = audio.shape[1] if n_blocks is None else int(n_blocks)
        new = audio[:, :nb].reshape(self.n, nb * 128)
        n0, n1 = self.N, self.N + nb * 128
        j0, j1 = out_range(n0, n1, self.up, self.down)
        x = np.concatenate([self.state, new], axis=1).astype(np.int64)       # x[:, p] is sample n0 - 256 + p
        jm = [j * self.down for j in range(j0, j1)]                          # Python integers: any N
        b = np.array([v // self.up - n0 for v in jm], dtype=np.int64)        # relative to the call's first sample
        phi = np.array([v % self.up for v in jm], dtype=np.int64)
        assert b.size == 0 or (b.min() >= 0 and b.max() < nb * 128)
        k = np.arange(self.K)
        pos = STATE + b[:, None] - k[None, :]                                # [count][K], >= 1
        taps = self.h[k[None, :], phi[:, None]]                              # [count][K]
        step = max(1, (1 << 22) // max(1, pos.size))                         # channels per gather: bounds the temporary
        acc = np.concatenate([(x[c:c + step][:, pos] * taps[None]).sum(axis=2) for c in range(0, self.n, step)], axis=0)
        self.acc_range = (int(acc.min()), int(acc.max())) if acc.size else (0, 0)   # of this call's sums, before rounding
        y = np.clip((acc + self.round) >> self.shift, -32768, 32767).astype(np.int16)
        self.state = np.concatenate([self.state, new], axis=1)[:, -STATE:].copy()
        self.N = n1
        return y


def loop_outputs(x, up, down, taps, shift, j0, j1):
    """Outputs j0 .. j1 - 1 of one channel whose samples from position 0 on are x (Python integers, one product at a time)."""
    h = [int(v) for v in np.asarray(taps).reshape(-1)]
    K = len(h) // up
    rnd = (1 << (shift - 1)) if shift else 0
    out = []
    for j in range(j0, j1):
        b, phi = (j * down) // up, (j * down) % up
        acc = 0
        for k in range(K):
            if b - k >= 0:
                acc += h[k * up + phi] * int(x[b - k])
        out.append(max(-32768, min(32767, (acc + rnd) >> shift)))
    return np.array(out, dtype=np.int16)
