"""The DCS squelch's statement (include/asdr_dcs.h) in numpy, written from the header's text and independent of the C++: the Golay
(23, 12) words of the codes, the third-order CIC decimator it shares with the tone squelch, the 20-sample bit filter, the slicer with
its bit clock, the 23-bit register with the table scan, and the confirm / hold / open rule.  The GPU tests hold the kernel to it at
tolerance 0; tests/test_dcs_ref.py holds it to known answers and to signals in noise.  Vectorised over channels, int64 throughout."""
import numpy as np

import tone_ref as TR

FS = 44100
PASS, ANY = -2, -1
MAX_CODES = 128
POLY = 0xC75
PERIOD, HALF, STEP = 2625, 1312, 128          # the bit clock: 2625 / 128 decimated samples per bit; a bit is taken at the middle
BIT_RATE = 134.4
CODES = tuple(int(c, 8) for c in """023 025 026 031 032 036 043 047 051 053 054 065 071 072 073 074 114 115 116 122 125 131 132 134 143
145 152 155 156 162 165 172 174 205 212 223 225 226 243 244 245 246 251 252 255 261 263 265 266 271 274 306 311 315 325 331 332 343 346
351 356 364 365 371 411 412 413 423 431 432 445 446 452 454 455 462 464 465 466 503 506 516 523 526 532 546 565 606 612 624 627 631 632
654 662 664 703 712 723 731 732 734 743 754""".split())
STATE_NAMES = ("hist", "dhist", "sr", "bits", "hits", "detections", "openings", "open_blocks", "edges", "detected", "cand", "clk",
               "quiet", "age", "run", "b", "open", "reserved")
STATE_OFFSETS = (0, 96, 144, 148, 152, 156, 160, 164, 168, 172, 174, 176, 178, 180, 181, 182, 183, 184)
STATE_DTYPE = np.dtype({"names": list(STATE_NAMES), "offsets": list(STATE_OFFSETS), "itemsize": 192,
                        "formats": [("<i2", (48,)), ("<i2", (24,)), "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<i2", "<i2", "<u2",
                                    "<u2", "u1", "u1", "u1", "u1", ("<u4", (2,))]})
COUNTERS = ("bits", "hits", "detections", "openings", "open_blocks", "edges")
_PC = np.array([bin(v).count("1") for v in range(2048)], dtype=np.int64)


def popcount23(x):
    x = np.asarray(x, dtype=np.int64)
    return _PC[x & 0x7FF] + _PC[(x >> 11) & 0x7FF] + _PC[(x >> 22) & 0x7FF]


def word(code):
    """w = p << 12 | d with d = 0x800 | code and p = (d x^11) mod g over GF(2), g = 0xC75; None for a code above 0777."""
    code = int(code)
    if not 0 <= code <= 0o777:
        return None
    d = 0x800 | code
    r = d << 11
    for k in range(22, 10, -1):
        if r >> k & 1:
            r ^= POLY << (k - 11)
    return r << 12 | d


def rotations(w):
    """The 23 rotations of a 23-bit word."""
    return [((w >> k) | (w << (23 - k))) & 0x7FFFFF for k in range(23)]


def min_distance(words):
    """The smallest number of differing bits over the pairs of a table; 23 for a table of one."""
    w = np.asarray(words, dtype=np.int64)
    if w.size < 2:
        return 23
    d = popcount23(w[:, None] ^ w[None, :])
    return int(d[~np.eye(w.size, dtype=bool)].min())


def find(table_words, code, inverted=False):
    """The lowest table index whose word is a rotation of the code's word (of its complement if inverted); -1 if none is."""
    w = word(code)
    if w is None:
        return -1
    rot = set(rotations(w ^ 0x7FFFFF if inverted else w))
    return next((k for k, t in enumerate(table_words) if t in rot), -1)


class DcsRef:
    """n_channels DCS squelches, one numpy array per setting and per state field (st[name][c])."""

    def __init__(self, n_channels):
        self.n = int(n_channels)
        self.codes = list(CODES)
        self.words = [word(c) for c in CODES]
        self.max_errors, self.confirm, self.hold_bits = 0, 2, 46
        self.want = np.full(self.n, PASS, dtype=np.int64)
        self.hysteresis = np.zeros(self.n, dtype=np.int64)
        self.reset()

    def _sel(self, ch):
        return slice(None) if ch == -1 else int(ch)

    # bank-wide
    def set_codes(self, codes):
        codes = [int(c) for c in codes]
        words = [word(c) for c in codes]
        assert 1 <= len(codes) <= MAX_CODES and None not in words and min_distance(words) >= 2 * self.max_errors + 1
        self.codes, self.words = codes, words
        st = self.st
        st["sr"][:] = 0; st["cand"][:] = -1; st["age"][:] = 255; st["run"][:] = 0; st["detected"][:] = -1; st["quiet"][:] = 0

    def set_max_errors(self, m):
        assert 0 <= m <= 3 and min_distance(self.words) >= 2 * m + 1
        self.max_errors = int(m)

    def set_confirm(self, k):
        assert 1 <= k <= 8
        self.confirm = int(k)

    def set_hold_bits(self, h):
        assert 23 <= h <= 1023
        self.hold_bits = int(h)

    # per channel
    def set_want(self, want, ch=-1):
        assert PASS <= want < len(self.words)
        self.want[self._sel(ch)] = want

    def set_hysteresis(self, h, ch=-1):
        assert 0 <= h < 2**32
        self.hysteresis[self._sel(ch)] = h

    def find(self, code, inverted=False):
        return find(self.words, code, inverted)

    def take_bit(self, e):
        """Step 4 for the channels e (an index array) whose clock passed a bit's middle; b is the slicer's bit there."""
        st = self.st
        sr = (st["sr"][e] >> 1) | (st["b"][e] << 22)
        st["sr"][e] = sr
        st["bits"][e] = (st["bits"][e] + 1) & 0xFFFFFFFF
        age = np.minimum(st["age"][e] + 1, 255)
        quiet = np.minimum(st["quiet"][e] + 1, 65535)
        dist = popcount23(sr[:, None] ^ np.asarray(self.words, dtype=np.int64)[None, :])
        best = np.argmin(dist, axis=1)                                # the lowest index of the minimum
        hit = dist[np.arange(len(e)), best] <= self.max_errors
        st["hits"][e] = (st["hits"][e] + hit) & 0xFFFFFFFF
        again = (best == st["cand"][e]) & (age == 23)
        run = np.where(hit, np.where(again, np.minimum(st["run"][e] + 1, 255), 1), st["run"][e])
        st["run"][e] = run
        st["cand"][e] = np.where(hit, best, st["cand"][e])
        age = np.where(hit, 0, age)
        sure = hit & (run >= self.confirm)
        det = st["detected"][e]
        st["detections"][e] = (st["detections"][e] + (sure & (det != best))) & 0xFFFFFFFF
        det = np.where(sure, best, det)
        quiet = np.where(sure, 0, quiet)
        det = np.where((det >= 0) & (quiet > self.hold_bits), -1, det)
        st["age"][e], st["quiet"][e], st["detected"][e] = age, quiet, det
        want = self.want[e]
        match = np.where(want == PASS, True, np.where(want == ANY, det >= 0, det == want))
        st["openings"][e] = (st["openings"][e] + (match & (st["open"][e] == 0))) & 0xFFFFFFFF
        st["open"][e] = match

    def update(self, x, n_blocks=None):
        """x int16 [n_channels][stride_blocks][128], of which the first n_blocks blocks are new.  Returns (out int16
        [n_channels][n_blocks][128], unmuted uint8 [n_channels][n_blocks]: whether each block left unmuted)."""
        x = np.asarray(x)
        assert x.dtype == np.int16 and x.shape[0] == self.n and x.shape[2] == 128
        nb = x.shape[1] if n_blocks is None else int(n_blocks)
        st = self.st
        out, unmuted = np.zeros((self.n, nb, 128), dtype=np.int16), np.zeros((self.n, nb), dtype=np.uint8)
        for blk in range(nb):
            xb = x[:, blk].astype(np.int64)
            keep = (self.want == PASS) | (st["open"] == 1)            # open as it stood at the block's start
            out[:, blk] = np.where(keep[:, None], xb, 0)
            unmuted[:, blk] = keep
            st["open_blocks"] = (st["open_blocks"] + keep) & 0xFFFFFFFF
            d = TR.decimate(st["hist"], xb)                           # step 1
            st["hist"] = np.concatenate([st["hist"], xb], axis=1)[:, -48:]
            ext = np.concatenate([st["dhist"], d], axis=1)            # step 2
            st["dhist"] = ext[:, -24:]
            taken = np.zeros(self.n, dtype=np.int64)
            for k in range(8):                                        # step 3
                s = ext[:, 24 + k - 19:24 + k + 1].sum(axis=1)
                b, clk = st["b"], st["clk"]
                nbit = np.where(s > self.hysteresis, 1, np.where(s < -self.hysteresis, 0, b))
                edge = nbit != b
                err = np.where(clk < HALF, clk, clk - PERIOD)
                clk = np.where(edge, (clk - (err >> 2)) % PERIOD, clk)
                st["b"] = nbit
                st["edges"] = (st["edges"] + edge) & 0xFFFFFFFF
                p = clk
                clk = clk + STEP
                e = np.flatnonzero((p < HALF) & (clk >= HALF))
                st["clk"] = np.where(clk >= PERIOD, clk - PERIOD, clk)
                if e.size:
                    taken[e] += 1
                    self.take_bit(e)
            assert taken.max() <= 1                                   # at most one bit per block
        self.blocks += nb
        return out, unmuted

    def clear(self):
        for k in COUNTERS:
            self.st[k][:] = 0
        self.blocks = 0

    def reset(self):
        n = self.n
        z = lambda *shape: np.zeros((n,) + shape, dtype=np.int64)
        self.st = {"hist": z(48), "dhist": z(24), "sr": z(), "bits": z(), "hits": z(), "detections": z(), "openings": z(), "open_blocks": z(),
                   "edges": z(), "detected": z() - 1, "cand": z() - 1, "clk": z(), "quiet": z(), "age": z() + 255, "run": z(), "b": z(),
                   "open": z(), "reserved": z(2)}
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


# ---- signals
def dcs_wave(n_samples, w, amplitude, rate=BIT_RATE, start_bit=0.0, lowpass_hz=300.0):
    """float64 [n_samples]: the word w as NRZ (bit 0 first, repeated without a gap; a 1 is positive) at `rate` bit/s, its mean
    removed, through a two-pole Butterworth low-pass (applied on the FFT; 0 for none)."""
    k = np.arange(n_samples, dtype=np.float64)
    bit = np.floor(start_bit + k * rate / FS).astype(np.int64) % 23
    level = 2.0 * ((int(w) >> bit) & 1) - 1.0
    level -= (2.0 * bin(int(w)).count("1") - 23.0) / 23.0
    if lowpass_hz:
        X = np.fft.rfft(level)
        s = 1j * np.fft.rfftfreq(n_samples, 1.0 / FS) / lowpass_hz
        level = np.fft.irfft(X / (s * s + np.sqrt(2.0) * s + 1.0), n=n_samples)
    return amplitude * level


to_int16 = TR.to_int16
voice_noise = TR.voice_noise
