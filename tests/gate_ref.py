"""The audio gate's statement (include/asdr_gate.h) in numpy and Python integers, written from the header's text and independent of
the C++: block energy and peak, the squelch recurrence, the delivered list and the packet.  The GPU tests hold the kernels to it at
tolerance 0; tests/test_gate_ref.py holds it to a per-sample Python loop and to the header's known sequences."""
import numpy as np

STATE_NAMES = ("energy", "last_energy", "peak", "openings", "open_blocks", "hang_left", "open", "reserved")
FULL_SCALE_ENERGY = 128 * 32767 * 32767
MAX_ENERGY = 1 << 37
M64 = (1 << 64) - 1


def energy_from_dbfs(db):
    """floor(128 * 32767^2 * 10^(db / 10) + 0.5), clamped to [0, 2^37]."""
    v = np.floor(np.float64(FULL_SCALE_ENERGY) * np.float64(10.0) ** (np.float64(db) / 10.0) + 0.5)
    if not v > 0:
        return 0
    return MAX_ENERGY if v >= MAX_ENERGY else int(v)


def block_energy_peak(rows):
    """rows int16 [..., 128] -> (E uint64 [...], P int64 [...]): sum of squares (exact: at most 2^37) and max |x|."""
    x = np.asarray(rows).astype(np.int64)
    return (x * x).sum(axis=-1).astype(np.uint64), np.abs(x).max(axis=-1)


STATE_TYPES = ("u8", "u8", "i4", "u4", "u4", "u2", "u1", "u1")   # the arithmetic of each field wraps as its width says


class GateRef:
    """n_channels gates, one numpy array per setting and per state field (st[name][c]); the recurrence runs block by block over
    all channels at once, each branch of the header's rule as a mask."""

    def __init__(self, n_channels):
        self.n = int(n_channels)
        self.open_energy = np.zeros(self.n, dtype=np.uint64)
        self.close_energy = np.zeros(self.n, dtype=np.uint64)
        self.hang_blocks = np.zeros(self.n, dtype=np.uint16)
        self.reset()

    @property
    def settings(self):
        return list(zip(self.open_energy.tolist(), self.close_energy.tolist(), self.hang_blocks.tolist()))

    def set_squelch(self, open_energy, close_energy, hang_blocks, ch=-1):
        assert 0 <= close_energy <= open_energy <= M64 and 0 <= hang_blocks <= 65535
        sel = slice(None) if ch == -1 else int(ch)
        self.open_energy[sel], self.close_energy[sel], self.hang_blocks[sel] = open_energy, close_energy, hang_blocks

    def step(self, E, P):
        """One block of every channel: E uint64 [n], P [n].  Returns open after the block, uint8 [n]."""
        st = self.st
        was = st["open"] == 1
        loud = E >= self.open_energy                          # if E >= open_energy
        hold = ~loud & was & (E >= self.close_energy)         # elif open and E >= close_energy
        hang = ~loud & ~hold & was & (st["hang_left"] > 0)    # elif open and hang_left > 0
        shut = ~loud & ~hold & ~hang & was                    # elif open
        st["openings"] += (loud & ~was).astype(np.uint32)
        st["open"][loud] = 1
        st["open"][shut] = 0
        st["hang_left"][loud | hold] = self.hang_blocks[loud | hold]
        st["hang_left"][hang] -= 1
        st["open_blocks"] += st["open"].astype(np.uint32)
        st["energy"] += E                                     # uint64: mod 2^64
        st["last_energy"][:] = E
        st["peak"][:] = np.maximum(st["peak"], P.astype(np.int32))
        return st["open"].copy()

    def update(self, audio, n_blocks=None, capacity_rows=None):
        """audio int16 [n_channels][stride_blocks][128], of which the first n_blocks blocks are new.  Returns (index int32 ascending,
        packet int16 [min(count, capacity_rows)][n_blocks][128], opens uint8 [n_channels][n_blocks]: open after each block)."""
        audio = np.asarray(audio)
        assert audio.dtype == np.int16 and audio.shape[0] == self.n and audio.shape[2] == 128
        nb = audio.shape[1] if n_blocks is None else int(n_blocks)
        new = audio[:, :nb]
        E, P = block_energy_peak(new)
        opens = np.stack([self.step(E[:, b], P[:, b]) for b in range(nb)], axis=1) if nb else np.zeros((self.n, 0), dtype=np.uint8)
        self.blocks += nb
        index = np.flatnonzero(opens.any(axis=1)).astype(np.int32)
        cap = len(index) if capacity_rows is None else min(len(index), int(capacity_rows))
        return index, new[index[:cap]].copy(), opens

    def clear(self):
        for k in ("energy", "last_energy", "peak", "openings", "open_blocks"):
            self.st[k][:] = 0
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


def record_tuples(records):
    """A structured GATE_STATE_DTYPE array as the list GateRef.state_tuples() gives."""
    return list(zip(*[records[k].tolist() for k in STATE_NAMES]))


def rows_with_energy(energies, rng=None):
    """int16 [len(energies)][128] whose block energies are exactly `energies` (each in 0 .. 2^37), greedy in squares: the largest
    square that fits goes to the next sample, signs alternating (32768 only as -32768); a remainder that 128 samples cannot hold
    is an error.  rng shuffles the positions."""
    import math
    out = np.zeros((len(energies), 128), dtype=np.int16)
    for k, e in enumerate(energies):
        e = int(e)
        for n in range(128):
            if e == 0:
                break
            r = min(32768, math.isqrt(e))
            out[k, n] = -r if (n & 1) or r == 32768 else r
            e -= r * r
        assert e == 0, "energy does not fit 128 samples"
    if rng is not None:
        for k in range(len(out)):
            out[k] = out[k][rng.permutation(128)]
    return out
