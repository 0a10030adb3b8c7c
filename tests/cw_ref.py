"""The CW decoder's statement (include/asdr_cw.h) in numpy and plain Python, written from the header's text and independent of the
C++: the mixer with its 1024-entry cosine table, the 128-sample sliding envelope at 1378.125 Hz, the two level trackers and the raw
key, the glitch filter, the dot / dash decision with the speed tracker, the gaps, the Morse table, the per-channel rings and the
ascending delivery.  The GPU tests hold the kernel to it at tolerance 0; tests/test_cw_ref.py holds it to keyed text, in noise too.
Steps 1 and 2 are vectorised over channels and blocks (int64 throughout); steps 3 to 7 walk each channel's envelope in order."""
import numpy as np

FS = 44100
ENV_HZ = FS / 32.0
PITCH_HZ = 774
MIN_POWER, GLITCH, MAX_GLITCH, SLOW, FAST = 16, 4, 16, 10, 2
WPM, MIN_WPM, MAX_WPM = 20, 5, 60
DIT_UNITS, MIN_D, MAX_D = 26460, 441, 5292
RING, MAX_RING = 16, 64
M32 = 0xFFFFFFFF

MORSE = {"A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....", "I": "..", "J": ".---",
         "K": "-.-", "L": ".-..", "M": "--", "N": "-.", "O": "---", "P": ".--.", "Q": "--.-", "R": ".-.", "S": "...", "T": "-",
         "U": "..-", "V": "...-", "W": ".--", "X": "-..-", "Y": "-.--", "Z": "--..",
         "0": "-----", "1": ".----", "2": "..---", "3": "...--", "4": "....-", "5": ".....", "6": "-....", "7": "--...", "8": "---..",
         "9": "----.",
         ".": ".-.-.-", ",": "--..--", "?": "..--..", "'": ".----.", "!": "-.-.--", "/": "-..-.", "(": "-.--.", ")": "-.--.-",
         "&": ".-...", ":": "---...", ";": "-.-.-.", "=": "-...-", "+": ".-.-.", "-": "-....-", "_": "..--.-", '"': ".-..-.",
         "$": "...-..-", "@": ".--.-."}


def sym_of(code):
    """The symbol register of a code: a leading 1, then 0 = dot and 1 = dash, the first element highest."""
    s = 1
    for e in code:
        s = 2 * s + (1 if e == "-" else 0)
    return s


TABLE = np.zeros(256, dtype=np.uint8)
for _ch, _code in MORSE.items():
    assert TABLE[sym_of(_code)] == 0
    TABLE[sym_of(_code)] = ord(_ch)
COS = np.floor(1024.0 * np.cos(2.0 * np.pi * np.arange(1024) / 1024.0) + 0.5).astype(np.int64)

STATE_NAMES = ("ph", "prev_i", "prev_q", "hi", "lo", "D", "run", "marks", "chars", "unknown", "glitches", "cnt", "key", "sym", "gap",
               "reserved")
STATE_OFFSETS = (0, 4, 16, 28, 32, 36, 40, 44, 48, 52, 56, 60, 61, 62, 63, 64)
STATE_DTYPE = np.dtype({"names": list(STATE_NAMES), "offsets": list(STATE_OFFSETS), "itemsize": 80,
                        "formats": ["<u4", ("<i4", (3,)), ("<i4", (3,)), "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "u1",
                                    "u1", "u1", "u1", ("<u4", (4,))]})
EVENT_DTYPE = np.dtype({"names": ["channel", "seq", "block", "ch", "wpm", "sym", "flags"], "offsets": [0, 4, 8, 12, 13, 14, 15],
                        "itemsize": 16, "formats": ["<u4", "<u4", "<u4", "u1", "u1", "u1", "u1"]})
COUNTERS = ("marks", "unknown", "glitches")            # what clear zeroes (and lost); chars, the source of seq, stays
SCALARS = ("hi", "lo", "D", "run", "marks", "chars", "unknown", "glitches", "cnt", "key", "sym", "gap")


def pitch_step(hz):
    """floor(hz 2^32 / 44100 + 0.5); hz in 100 .. 3000."""
    assert 100 <= hz <= 3000
    return int(np.floor(hz * 4294967296.0 / FS + 0.5))


def dit_of(wpm):
    return (DIT_UNITS + wpm // 2) // wpm


def wpm_of(D):
    return (DIT_UNITS + D // 2) // D


class CwRef:
    """n_channels CW decoders: one numpy array per state field (st[name][c]), a list of waiting events per channel."""

    def __init__(self, n_channels, ring=RING):
        assert 1 <= ring <= MAX_RING
        self.n, self.ring = int(n_channels), int(ring)
        self.pitch_step = np.full(self.n, pitch_step(PITCH_HZ), dtype=np.int64)
        self.min_power = np.full(self.n, MIN_POWER, dtype=np.int64)
        self.glitch = np.full(self.n, GLITCH, dtype=np.int64)
        self.track = np.ones(self.n, dtype=np.int64)
        self.reset()

    @staticmethod
    def _sel(ch):
        return slice(None) if ch == -1 else int(ch)

    def set_pitch_step(self, step, ch=-1):
        assert 0 <= step <= M32
        self.pitch_step[self._sel(ch)] = step

    def set_min_power(self, p, ch=-1):
        assert 0 <= p <= M32
        self.min_power[self._sel(ch)] = p

    def set_glitch(self, g, ch=-1):
        assert 1 <= g <= MAX_GLITCH
        self.glitch[self._sel(ch)] = g

    def set_track(self, t, ch=-1):
        assert t in (0, 1)
        self.track[self._sel(ch)] = t

    def set_speed(self, wpm, ch=-1):
        assert MIN_WPM <= wpm <= MAX_WPM
        self.st["D"][self._sel(ch)] = dit_of(wpm)

    def envelope(self, x):
        """Steps 1 and 2 over a call: x int64 [n][nb][128] -> P int64 [n][nb * 4]; advances ph, prev_i and prev_q.  Also returns the
        largest |a| of the call."""
        st = self.st
        n, nb = x.shape[:2]
        N = nb * 128
        phase = (st["ph"][:, None] + np.arange(N, dtype=np.int64)[None, :] * self.pitch_step[:, None]) & M32
        j = phase >> 22
        xs = x.reshape(n, N)
        a_i = (xs * COS[j]).reshape(n, nb * 4, 32).sum(axis=2) >> 10
        a_q = (xs * COS[(j - 256) & 1023]).reshape(n, nb * 4, 32).sum(axis=2) >> 10
        st["ph"] = (st["ph"] + N * self.pitch_step) & M32
        big = int(max(np.abs(a_i).max(), np.abs(a_q).max()))
        ext_i = np.concatenate([st["prev_i"], a_i], axis=1)            # a of envelope sample m at ext[:, 3 + m]
        ext_q = np.concatenate([st["prev_q"], a_q], axis=1)
        m = nb * 4
        i_w = ext_i[:, 0:m] + ext_i[:, 1:m + 1] + ext_i[:, 2:m + 2] + ext_i[:, 3:m + 3]
        q_w = ext_q[:, 0:m] + ext_q[:, 1:m + 1] + ext_q[:, 2:m + 2] + ext_q[:, 3:m + 3]
        st["prev_i"], st["prev_q"] = ext_i[:, -3:], ext_q[:, -3:]
        return (i_w * i_w + q_w * q_w) >> 14, big

    def update(self, x, n_blocks=None):
        """x int16 [n_channels][stride_blocks][128], of which the first n_blocks blocks are new.  Returns (the largest |a|, the
        largest P) of the call."""
        x = np.asarray(x)
        assert x.dtype == np.int16 and x.shape[0] == self.n and x.shape[2] == 128
        nb = x.shape[1] if n_blocks is None else int(n_blocks)
        if nb == 0:
            return 0, 0
        P, big = self.envelope(x[:, :nb].astype(np.int64))
        rows = P.tolist()
        for c in range(self.n):
            self.walk(c, rows[c])
        self.blocks += nb
        return big, int(P.max())

    def walk(self, c, P_row):
        """Steps 3 to 7 of channel c over the call's envelope."""
        st = self.st
        hi, lo, D, run, marks, chars, unknown, glitches, cnt, key, sym, gap = (int(st[k][c]) for k in SCALARS)
        min_power, glitch, track = int(self.min_power[c]), int(self.glitch[c]), int(self.track[c])

        def emit(ch, sym_field, flags, m):
            nonlocal chars
            e = np.zeros((), dtype=EVENT_DTYPE)
            e["channel"], e["seq"], e["block"] = c, chars & M32, (self.blocks + m // 4) & M32
            e["ch"], e["wpm"], e["sym"], e["flags"] = ch, wpm_of(D), sym_field, flags
            chars = (chars + 1) & M32
            if len(self.waiting[c]) == self.ring:
                self.waiting[c].pop(0)
                self.lost[c] += 1
            self.waiting[c].append(e)

        for m, P in enumerate(P_row):
            # step 3
            if P > hi:
                hi += (P - hi) >> FAST
            else:
                hi -= (hi - P) >> SLOW
            if P < lo:
                lo -= (lo - P) >> FAST
            else:
                lo += (P - lo) >> SLOW
            span = hi - lo if hi > lo else 0
            r = 1 if span > 0 and P >= min_power and P > lo + (span >> (3 if key else 2)) else 0
            # step 4
            run = (run + 1) & M32
            if r != key:
                cnt += 1
            else:
                if cnt > 0:
                    glitches = (glitches + 1) & M32
                cnt = 0
            if cnt == glitch:
                L = (run - glitch) & M32
                old, key, run, cnt = key, r, glitch, 0
                if old == 1:
                    # step 5
                    marks = (marks + 1) & M32
                    dash = 1 if 16 * L >= 2 * D else 0
                    sym = 0 if sym >= 128 or sym == 0 else 2 * sym + dash
                    if track:
                        D += ((16 * L // 3 if dash else 16 * L) - D) >> 3
                        D = min(max(D, MIN_D), MAX_D)
            # step 6
            if key == 0:
                if sym != 1 and 16 * run >= 2 * D:
                    ch = int(TABLE[sym])
                    if ch == 0:
                        unknown = (unknown + 1) & M32
                        emit(ord("?"), sym, 1, m)
                    else:
                        emit(ch, sym, 0, m)
                    sym, gap = 1, 1
                if gap == 1 and 16 * run >= 5 * D:
                    emit(ord(" "), 1, 0, m)
                    gap = 0
        for k, v in zip(SCALARS, (hi, lo, D, run, marks, chars, unknown, glitches, cnt, key, sym, gap)):
            st[k][c] = v

    def collect(self, max_events):
        """The events a collect delivers, EVENT_DTYPE [count]: ascending by channel and, in a channel, from the oldest on, the first
        max_events of that order; they leave their rings."""
        out = []
        for c in range(self.n):
            while self.waiting[c] and len(out) < max_events:
                out.append(self.waiting[c].pop(0))
        return np.array(out, dtype=EVENT_DTYPE).reshape(-1)

    def ring_state(self):
        return np.array([len(w) for w in self.waiting], dtype=np.uint32), self.lost.astype(np.uint32)

    def clear(self):
        for k in COUNTERS:
            self.st[k][:] = 0
        self.lost[:] = 0
        self.blocks = 0

    def reset(self):
        n = self.n
        z = lambda *shape: np.zeros((n,) + shape, dtype=np.int64)
        self.st = {k: z() for k in SCALARS}
        self.st.update(ph=z(), prev_i=z(3), prev_q=z(3), reserved=z(4))
        self.st["D"] += dit_of(WPM)
        self.st["sym"] += 1
        self.waiting = [[] for _ in range(n)]
        self.lost = np.zeros(n, dtype=np.int64)
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


def text_of(events, channel=None):
    """The characters of the events (of one channel), joined."""
    return "".join(chr(int(e["ch"])) for e in events if channel is None or int(e["channel"]) == channel)


# ---- signals
def key_times(text, wpm, jitter=0.0, rng=None):
    """[(start, end)] in seconds of every mark of `text` keyed by the standard timing: dot 1, dash 3, between elements 1, between
    characters 3, between words 7 dits of 1.2 / wpm s; every element and gap stretched by a factor uniform in 1 +- jitter."""
    dit = 1.2 / wpm
    f = (lambda: 1.0 + jitter * rng.uniform(-1.0, 1.0)) if jitter else (lambda: 1.0)
    t, marks = 0.0, []
    for w, word in enumerate(text.split(" ")):
        if w:
            t += 7 * dit * f()
        for k, ch in enumerate(word):
            if k:
                t += 3 * dit * f()
            for e, el in enumerate(MORSE[ch]):
                if e:
                    t += dit * f()
                d = (3 if el == "-" else 1) * dit * f()
                marks.append((t, t + d))
                t += d
    return marks


def keyed_tone(text, wpm, amplitude=8000.0, hz=float(PITCH_HZ), lead=0.3, tail=1.2, jitter=0.0, rng=None, rise=0.002):
    """float64: `text` keyed on a tone, `lead` seconds of silence in front and `tail` behind (longer than a word gap at 12 WPM); the
    keying is a 0 / 1 gate smoothed by a Hann window of `rise` seconds (edges of that length, centred on the key times)."""
    marks = key_times(text, wpm, jitter, rng)
    n = int(np.ceil((lead + marks[-1][1] + tail) * FS))
    edges = np.zeros(n + 1)
    for a, b in marks:
        edges[int(round((lead + a) * FS))] += 1.0
        edges[int(round((lead + b) * FS))] -= 1.0
    w = np.hanning(max(3, int(rise * FS) | 1))
    env = np.convolve(np.cumsum(edges)[:n], w / w.sum(), mode="same")
    return amplitude * env * np.cos(2.0 * np.pi * hz * np.arange(n) / FS)


def keyed_carrier_iq(text, wpm=WPM, amplitude=3000.0, if_hz=7164.0, lead=1.0):
    """(I, Q) int16 [nb][128]: `text` keyed on a complex carrier at if_hz, for the chain in CW_USBmode (tuning offset 6390 Hz: the
    audio is at if_hz - 6390, 774 Hz for the default)."""
    gate = keyed_tone(text, wpm, amplitude=1.0, hz=0.0, lead=lead)
    n = gate.size // 128 * 128
    z = amplitude * gate[:n] * np.exp(2j * np.pi * if_hz * np.arange(n) / FS)
    return to_int16(z.real).reshape(-1, 128), to_int16(z.imag).reshape(-1, 128)


def to_int16(x):
    return np.clip(np.floor(np.asarray(x, dtype=np.float64) + 0.5), -32768, 32767).astype(np.int16)


def blocks_of(x):
    """A signal padded with zeros to whole blocks: int16 [nb][128]."""
    x = to_int16(x)
    nb = -(-x.size // 128)
    return np.concatenate([x, np.zeros(nb * 128 - x.size, dtype=np.int16)]).reshape(nb, 128)


def decode(x, **settings):
    """The text a fresh one-channel decoder makes of the signal x (float or int16, any length); settings: wpm, track, glitch,
    min_power, hz.  Returns (text with the trailing space stripped, the decoder)."""
    r = CwRef(1, ring=MAX_RING)
    if "wpm" in settings:
        r.set_speed(settings["wpm"])
    if "track" in settings:
        r.set_track(settings["track"])
    if "glitch" in settings:
        r.set_glitch(settings["glitch"])
    if "min_power" in settings:
        r.set_min_power(settings["min_power"])
    if "hz" in settings:
        r.set_pitch_step(pitch_step(settings["hz"]))
    rows = blocks_of(x)
    out = []
    for a in range(0, rows.shape[0], 256):
        r.update(rows[None, a:a + 256])
        out += list(r.collect(MAX_RING))
    return text_of(out).rstrip(" "), r
