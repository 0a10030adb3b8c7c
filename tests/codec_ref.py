"""Independent numpy restatement of include/asdr_codec.h: G.711 mu-law and A-law, IMA ADPCM, the packet rows, and a CodecRef that
carries per-channel state through the three row mappings.  Integers only; the kernels and asdr_codec_decode are held to it bit for
bit.  tests/test_codec_ref.py pins this file on its own (known answers, round trips, and Python's audioop where it imports)."""
import numpy as np

ULAW, ALAW, ADPCM = 1, 2, 3
KINDS = {"ulaw": ULAW, "alaw": ALAW, "adpcm": ADPCM}
MAX_SAMPLES = 8388480
HEADER = 4
STEPS = np.array([7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
                  130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
                  1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484,
                  7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767],
                 dtype=np.int64)
assert STEPS.size == 89


def floor_log2(a):
    """floor(log2 a) of positive integers below 2^16, by counting shifts."""
    a = np.asarray(a, dtype=np.int64)
    return sum(((a >> k) > 0).astype(np.int64) for k in range(1, 16))


# ---- G.711
def ulaw_encode(x):
    m = np.asarray(x, dtype=np.int64) >> 2
    neg = m < 0
    a = np.minimum(np.abs(m), 8158) + 33
    e = floor_log2(a) - 5
    code = (e << 4) | ((a >> (e + 1)) & 15)
    return (code ^ np.where(neg, 0x7F, 0xFF)).astype(np.uint8)


def ulaw_decode(b):
    u = ~np.asarray(b, dtype=np.int64) & 0xFF
    e, q = (u >> 4) & 7, u & 15
    t = (((q << 3) + 132) << e) - 132
    return np.where(u & 0x80, -t, t).astype(np.int16)


def alaw_encode(x):
    m = np.asarray(x, dtype=np.int64) >> 3
    neg = m < 0
    a = np.where(neg, -m - 1, m)
    e = np.maximum(floor_log2(np.maximum(a, 1)) - 4, 0)
    q = np.where(e < 2, (a >> 1) & 15, (a >> e) & 15)
    return (((e << 4) | q) ^ np.where(neg, 0x55, 0xD5)).astype(np.uint8)


def alaw_decode(b):
    a = np.asarray(b, dtype=np.int64) ^ 0x55
    e, q = (a >> 4) & 7, a & 15
    t = np.where(e == 0, (q << 4) + 8, ((q << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


# ---- IMA ADPCM: all channels of x [k][n] in step, one sample at a time
def _advance(p, i, c, sign, s):
    v = (s >> 3) + np.where(c & 4, s, 0) + np.where(c & 2, s >> 1, 0) + np.where(c & 1, s >> 2, 0)
    p = np.clip(np.where(sign, p - v, p + v), -32768, 32767)
    i = np.clip(i + np.where(c < 4, -1, 2 * (c - 3)), 0, 88)
    return p, i


def adpcm_encode(x, p, i):
    """x int [k][n], p and i int [k]: (nibbles uint8 [k][n], the predictor after every sample int16 [k][n], p, i)."""
    x = np.asarray(x, dtype=np.int64)
    p, i = np.array(p, dtype=np.int64), np.array(i, dtype=np.int64)
    nib = np.zeros(x.shape, dtype=np.uint8)
    pred = np.zeros(x.shape, dtype=np.int16)
    for t in range(x.shape[1]):
        s = STEPS[i]
        d = x[:, t] - p
        sign = d < 0
        d = np.abs(d)
        c = np.zeros_like(d)
        hit = d >= s
        c |= np.where(hit, 4, 0); d = d - np.where(hit, s, 0)
        hit = d >= (s >> 1)
        c |= np.where(hit, 2, 0); d = d - np.where(hit, s >> 1, 0)
        c |= np.where(d >= (s >> 2), 1, 0)
        p, i = _advance(p, i, c, sign, s)
        nib[:, t] = c | np.where(sign, 8, 0)
        pred[:, t] = p
    return nib, pred, p, i


def adpcm_decode(nib, p, i):
    """nibbles [k][n], p and i int [k]: (samples int16 [k][n], p, i)."""
    nib = np.asarray(nib, dtype=np.int64)
    p, i = np.array(p, dtype=np.int64), np.array(i, dtype=np.int64)
    y = np.zeros(nib.shape, dtype=np.int16)
    for t in range(nib.shape[1]):
        p, i = _advance(p, i, nib[:, t] & 7, (nib[:, t] & 8) != 0, STEPS[i])
        y[:, t] = p
    return y, p, i


# ---- packet rows
def row_bytes(kind, n):
    return HEADER + (n + 1) // 2 if kind == ADPCM else n


def padded_bytes(kind, n):
    return (row_bytes(kind, n) + 3) & ~3


def pack_adpcm(nib, p0, i0):
    """Rows uint8 [k][padded]: the header from the state before the first sample, then sample 2k low, 2k + 1 high."""
    k, n = nib.shape
    rows = np.zeros((k, padded_bytes(ADPCM, n)), dtype=np.uint8)
    p0 = np.asarray(p0, dtype=np.int64) & 0xFFFF
    rows[:, 0], rows[:, 1], rows[:, 2] = p0 & 0xFF, p0 >> 8, np.asarray(i0, dtype=np.int64)
    even = np.zeros((k, 2 * ((n + 1) // 2)), dtype=np.uint8)
    even[:, :n] = nib
    rows[:, HEADER:HEADER + (n + 1) // 2] = even[:, 0::2] | (even[:, 1::2] << 4)
    return rows


def unpack_adpcm(rows, n):
    """(nibbles [k][n], p0 [k], i0 [k]) of packet rows."""
    rows = np.asarray(rows, dtype=np.uint8)
    body = rows[:, HEADER:HEADER + (n + 1) // 2]
    nib = np.zeros((rows.shape[0], 2 * body.shape[1]), dtype=np.uint8)
    nib[:, 0::2], nib[:, 1::2] = body & 15, body >> 4
    p0 = (rows[:, 0].astype(np.int64) | (rows[:, 1].astype(np.int64) << 8)).astype(np.uint16).view(np.int16).astype(np.int64)
    return nib[:, :n], p0, rows[:, 2].astype(np.int64)


def decode_rows(kind, rows, n):
    """Packet rows uint8 [k][>= row_bytes] back to int16 [k][n]."""
    rows = np.asarray(rows, dtype=np.uint8)
    if kind == ULAW:
        return ulaw_decode(rows[:, :n])
    if kind == ALAW:
        return alaw_decode(rows[:, :n])
    nib, p0, i0 = unpack_adpcm(rows, n)
    return adpcm_decode(nib, p0, i0)[0]


class CodecRef:
    """The codec's statement with state: encode(x, ...) returns the packet rows a call writes, uint8 [k][padded], row by row."""

    def __init__(self, n_channels, kind):
        self.n, self.kind = n_channels, KINDS.get(kind, kind)
        self.reset()

    def reset(self):
        self.p = np.zeros(self.n, dtype=np.int64)
        self.i = np.zeros(self.n, dtype=np.int64)

    def state_tuples(self):
        return [(int(p), int(i), 0) for p, i in zip(self.p, self.i)]

    def encode(self, x, index=None, count=None, capacity=None, compact=False):
        """x int16 [rows][n]: the input rows.  index None: row c is channel c.  Otherwise output row r is channel index[r] for
        r < min(count, capacity), read from input row index[r], or from input row r when compact.  Only those channels' states
        advance.  Returns (channels [k], rows uint8 [k][padded])."""
        x = np.asarray(x)
        n = x.shape[1]
        if index is None:
            chans = np.arange(self.n)
            src = x[:self.n]
        else:
            k = max(0, min(count, capacity, self.n))
            chans = np.asarray(index[:k], dtype=np.int64)
            assert len(set(chans.tolist())) == len(chans) and ((chans >= 0) & (chans < self.n)).all()
            src = x[:k] if compact else x[chans]
        if self.kind == ULAW or self.kind == ALAW:
            rows = np.zeros((len(chans), padded_bytes(self.kind, n)), dtype=np.uint8)
            rows[:, :n] = (ulaw_encode if self.kind == ULAW else alaw_encode)(src)
            return chans, rows
        p0, i0 = self.p[chans], self.i[chans]
        nib, _, p1, i1 = adpcm_encode(src, p0, i0)
        self.p[chans], self.i[chans] = p1, i1
        return chans, pack_adpcm(nib, p0, i0)
