"""Independent numpy restatement of a rate bank (include/asdr_tuner.h, "Rate banks"), written from that statement and not from the
kernels: stage 1 is tuner_ref.TunerRef (its frequency word taken at the bank's Fs_in), stage 2 the polyphase rational resampler
U / M and its block timing.  Integer-only: stage-2 sums run in int64."""
import math

import numpy as np

import tuner_ref as R

BLOCK = R.BLOCK


def ratio(fs_in, D):
    """(U, M) = 44100 / (fs_in / D) in lowest terms."""
    mid = fs_in // D
    g = math.gcd(44100, mid)
    return 44100 // g, mid // g


def fw_from_hz(hz, fs_in):
    """(uint32)(int64) llround(hz * 2^32 / Fs_in)."""
    v = hz * 4294967296.0 / float(fs_in)
    r = math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1)
    return int(r) & 0xFFFFFFFF


def b_phi(j, U, M):
    """b_j = floor(j M / U) and phi_j = j M - b_j U, exact for Python ints or int64 arrays."""
    j = np.asarray(j, dtype=np.int64)
    jq, jr = j // U, j % U
    return jq * M + (jr * M) // U, (jr * M) % U


def blocks_out(n_u, U, M):
    """Blocks 0 .. n - 1 are out once n_u u samples exist: block J is out when b_{128 J + 127} <= n_u - 1."""
    num = n_u * U - 1 - 127 * M
    return 0 if num < 0 else num // (128 * M) + 1


def is_pass_through(h2, g2, U, M):
    return U == 1 and M == 1 and len(h2) == 1 and g2 >= 1 and int(h2[0]) == 1 << (15 - g2)


def accumulate(u, h2, U, M, j0, n, zero_before=0, base=0):
    """The sums sum_k h2[k U + phi_j] u[b_j - k] for j0 <= j < j0 + n over u (int [..., N_u - base]: samples base .. N_u - 1;
    u[i] = 0 for i < max(0, zero_before)); int64 [..., n].  A sample before base that is not such a zero is an error."""
    h2 = np.asarray(h2, dtype=np.int64)
    K = h2.size // U
    u = np.asarray(u, dtype=np.int64)
    b, phi = b_phi(np.arange(j0, j0 + n, dtype=np.int64), U, M)
    acc = np.zeros(u.shape[:-1] + (n,), dtype=np.int64)
    for k in range(K):
        i = b - k
        assert (i - base < u.shape[-1]).all()
        ok = i >= max(0, zero_before)
        assert (i[ok] >= base).all(), "u sample before the %d held from %d on" % (u.shape[-1], base)
        acc += h2[k * U + phi] * np.where(ok, u[..., np.where(ok, i - base, 0)], 0)
    return acc


def resample(u, h2, U, M, g2, j0, n, zero_before=0, base=0):
    """y[j] = sat16((sum + r) >> s) for j0 <= j < j0 + n (accumulate()); int64 [..., n]."""
    s = 15 - g2
    r = (1 << (s - 1)) if s else 0
    return R.sat16((accumulate(u, h2, U, M, j0, n, zero_before, base) + r) >> s)


class TunerRateRef(R.TunerRef):
    """A rate bank: stage 1 (TunerRef) at Fs_in, then stage 2 with every channel's u kept from sample u0 on (u0 = 0: the whole of
    it; place_at() keeps its end only)."""

    def __init__(self, n_channels, n_sources, D, fs_in, h=(16384,), g=1, h2=None, g2=1):
        super().__init__(n_channels, n_sources, D, h, g)
        self.fs_in = int(fs_in)
        self.U, self.M = ratio(self.fs_in, D)
        if h2 is None:
            assert self.U == self.M == 1, "give the stage-2 taps of a resampling bank"
            h2 = (16384,)
        self.set_resampler(h2, g2)
        self._stage2_reset()

    def _stage2_reset(self):
        self.u0 = 0
        self.u = np.zeros((self.n, 2, 0), dtype=np.int64)
        self.out_pos = 0
        self.zero_before = 0
        self.stale = False

    def set_resampler(self, h2, g2):
        self.h2, self.g2 = np.asarray(h2, dtype=np.int64), int(g2)
        assert self.h2.size % self.U == 0

    def set_frequency(self, hz, ch=-1):
        self.set_frequency_word(fw_from_hz(hz, self.fs_in), ch)

    def reset(self):
        h, g = self.h, self.g
        R.TunerRef.__init__(self, self.n, self.n_src, self.D, h, g)
        self._stage2_reset()

    def n_u(self):
        return self.u0 + self.u.shape[-1]

    def tail_needed(self):
        """Input samples per source that place_at() needs: the stage-1 filter's run-in of L - D samples before the first u sample
        rebuilt, and D samples for each u sample that the next outputs can reach back to.  The next output block J is not out yet,
        so b_{128 J + 127} >= N_u, b_{128 J} >= N_u - ceil(127 M / U), and its first output reads K - 1 samples before that; two
        more for the floors."""
        K = self.h2.size // self.U
        return max(len(self.h) - self.D, 0) + self.D * (K - 1 + -(-127 * self.M // self.U) + 2)

    def place_at(self, P, tail=None):
        """Put a resampling bank where a run of P input samples per source would have left it, every call of that run having written
        all its blocks (so out_pos = 128 blocks_out(P / D)): stage 1 as TunerRef.place_at, and the end of every channel's u rebuilt
        by running stage 1 over the tail at the absolute positions and phases.  That rebuilds what the run computed only if
        nothing that shapes u changed inside the tail: the filter is the caller's to keep, the anchors are checked (a retune
        inside the tail left u samples of the old tuning behind).  A bank whose stage 2 is or was a pass-through keeps no u
        history (stale, zero_before) and is refused.  Without a tail only the positions move and no u is held."""
        assert not self.pass_through() and not self.stale and self.zero_before == 0
        if tail is not None:
            T = np.asarray(tail).shape[1]
            assert T >= self.tail_needed(), "a tail of %d samples: %d needed" % (T, self.tail_needed())
        R.TunerRef.place_at(self, P, tail)
        n_end = self.P // self.D
        self.u0, self.u = n_end, np.zeros((self.n, 2, 0), dtype=np.int64)
        if tail is not None:
            assert (self.pos_a <= self.x0).all(), "a retune inside the tail"
            n0 = -(-(self.x0 + max(len(self.h) - self.D, 0)) // self.D)   # the first u sample whose inputs are all held
            I1, Q1 = self.outputs(n0, n_end - n0)
            self.u0, self.u = n0, np.stack([I1, Q1], axis=1).astype(np.int64)
        self.out_pos = BLOCK * blocks_out(n_end, self.U, self.M)

    def out_blocks(self, n_frames):
        if self.pass_through():
            return n_frames
        return max(0, blocks_out(self.n_u() + BLOCK * n_frames, self.U, self.M) - self.out_pos // BLOCK)

    def pass_through(self):
        return is_pass_through(self.h2, self.g2, self.U, self.M)

    def update(self, iq):
        """iq: [n_sources][n_frames * 128 * D][2].  Returns (I, Q) int16 [n][blocks written][128]."""
        nf = np.asarray(iq).shape[1] // (BLOCK * self.D)
        nb = self.out_blocks(nf)
        I1, Q1 = R.TunerRef.update(self, iq)
        n_u0 = self.n_u()
        self.u = np.concatenate([self.u, np.stack([I1.reshape(self.n, -1), Q1.reshape(self.n, -1)], axis=1).astype(np.int64)], axis=-1)
        if self.pass_through():
            self.stale = True
            self.out_pos += nf * BLOCK
            return I1, Q1
        if self.stale:
            self.zero_before, self.stale = n_u0, False
        y = resample(self.u, self.h2, self.U, self.M, self.g2, self.out_pos, nb * BLOCK, self.zero_before, self.u0)
        self.out_pos += nb * BLOCK
        return (y[:, 0].reshape(self.n, nb, BLOCK).astype(np.int16), y[:, 1].reshape(self.n, nb, BLOCK).astype(np.int16))
