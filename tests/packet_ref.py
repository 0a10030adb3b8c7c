"""The packet decoder's statement (include/asdr_packet.h) in numpy and plain Python, written from the header's text and independent of
the C++: the third-order decimator by 4, the 1200 / 2200 Hz correlators over one bit, the slicer with its bit clock, NRZI, the HDLC
framing with the FCS, the per-channel rings and the ascending delivery.  The GPU tests hold the kernel to it at tolerance 0;
tests/test_packet_ref.py holds it to known answers and to signals in noise.  Steps 1 and 2 are vectorised over channels and blocks
(int64 throughout); steps 3 to 6 walk each channel's slicer signs in order."""
import numpy as np

FS = 44100
FS_D = 11025
BAUD = 1200.0
MARK, SPACE = 1200.0, 2200.0
PERIOD, HALF, STEP = 147, 74, 16              # the bit clock: 147 / 16 decimated samples per bit; a bit is taken at the middle
H = np.array([1, 3, 6, 10, 12, 12, 10, 6, 3, 1], dtype=np.int64)
MIN_LEN, MAX_LEN = 17, 332                    # frame bytes with the FCS
MIN_BOOST, MAX_BOOST, MAX_RING = 64, 4096, 16
FLAG = 0x7E


def taps(f):
    """(C_f, S_f): floor(256 cos(2 pi f j / 11025) + 0.5) and likewise with sin, j = 0 .. 8."""
    j = np.arange(9)
    return (np.floor(256.0 * np.cos(2.0 * np.pi * f * j / FS_D) + 0.5).astype(np.int64),
            np.floor(256.0 * np.sin(2.0 * np.pi * f * j / FS_D) + 0.5).astype(np.int64))


C1200, S1200 = taps(1200)
C2200, S2200 = taps(2200)
STATE_NAMES = ("hist", "dhist", "bits", "edges", "flags", "frames", "crc_errors", "aborts", "clk", "len", "crc", "b", "prev", "sr", "cur",
               "nb", "in_frame", "reserved", "buf")
STATE_OFFSETS = (0, 16, 32, 36, 40, 44, 48, 52, 56, 58, 60, 62, 63, 64, 65, 66, 67, 68, 112)
STATE_DTYPE = np.dtype({"names": list(STATE_NAMES), "offsets": list(STATE_OFFSETS), "itemsize": 448,
                        "formats": [("<i2", (8,)), ("<i2", (8,)), "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u2", "<u2", "<u2", "u1", "u1",
                                    "u1", "u1", "u1", "u1", ("<u4", (11,)), ("u1", (336,))]})
FRAME_DTYPE = np.dtype({"names": ["channel", "seq", "block", "length", "flags", "data"], "offsets": [0, 4, 8, 12, 14, 16], "itemsize": 352,
                        "formats": ["<u4", "<u4", "<u4", "<u2", "<u2", ("u1", (336,))]})
COUNTERS = ("bits", "edges", "flags", "crc_errors", "aborts")      # what clear zeroes (and lost); frames stays
SCALARS = STATE_NAMES[2:17]


def crc_step(crc, byte):
    for s in range(8):
        crc = (crc >> 1) ^ (0x8408 if (crc ^ (byte >> s)) & 1 else 0)
    return crc


def fcs(data):
    """The AX.25 frame check sequence of bytes: 0x906E for b"123456789"."""
    crc = 0xFFFF
    for v in bytes(data):
        crc = crc_step(crc, v)
    return crc ^ 0xFFFF


def clock_step(clk, edge):
    """One decimated sample of step 3's clock: (clk after, whether a bit is taken)."""
    if edge:
        r = clk if clk < HALF else clk - PERIOD
        clk = (clk - (r >> 2)) % PERIOD
    p = clk
    clk += STEP
    take = p < HALF <= clk
    return (clk - PERIOD if clk >= PERIOD else clk), take


def format_address(frame):
    """ "SRC>DST,PATH" of a payload's address field; None where it is not one."""
    frame = bytes(frame)
    calls, n = [], 0
    while True:
        if n == 10 or 7 * n + 7 > len(frame):
            return None
        a = frame[7 * n:7 * n + 7]
        if any(v & 1 or not 0x20 <= v >> 1 <= 0x7E for v in a[:6]):
            return None
        text = "".join(chr(v >> 1) for v in a[:6]).replace(" ", "")
        ssid = (a[6] >> 1) & 15
        calls.append(text + ("-%d" % ssid if ssid else "") + ("*" if n >= 2 and a[6] & 0x80 else ""))
        n += 1
        if a[6] & 1:
            break
    if n < 2:
        return None
    return calls[1] + ">" + calls[0] + "".join("," + c for c in calls[2:])


class PacketRef:
    """n_channels packet decoders: one numpy array per state field (st[name][c]), a list of waiting frames per channel."""

    def __init__(self, n_channels, ring=4):
        assert 1 <= ring <= MAX_RING
        self.n, self.ring = int(n_channels), int(ring)
        self.space_boost = np.full(self.n, 256, dtype=np.int64)
        self.reset()

    def set_space_boost(self, boost, ch=-1):
        assert MIN_BOOST <= boost <= MAX_BOOST
        self.space_boost[slice(None) if ch == -1 else int(ch)] = boost

    def signs(self, x):
        """Steps 1 and 2 over a call: x int64 [n][nb][128] -> the sign of e, int64 [n][nb * 32]; advances hist and dhist."""
        st = self.st
        n, nb = x.shape[:2]
        ext = np.concatenate([st["hist"], x.reshape(n, nb * 128)], axis=1)          # sample i of the call at ext[:, 8 + i]
        d = np.full((n, nb * 32), 32, dtype=np.int64)
        for j in range(10):
            d += H[j] * ext[:, 8 + 3 - j:8 + 3 - j + 4 * (nb * 32 - 1) + 1:4]
        d >>= 6
        st["hist"] = ext[:, -8:]
        dext = np.concatenate([st["dhist"], d], axis=1)                             # d_m of the call at dext[:, 8 + m]
        m = nb * 32
        acc = [np.zeros((n, m), dtype=np.int64) for _ in range(4)]
        for j in range(9):
            w = dext[:, 8 - j:8 - j + m]
            for a, t in zip(acc, (C1200, S1200, C2200, S2200)):
                a += w * t[j]
        i1, q1, i2, q2 = (a >> 8 for a in acc)
        e = (i1 * i1 + q1 * q1) * 256 - (i2 * i2 + q2 * q2) * self.space_boost[:, None]
        st["dhist"] = dext[:, -8:]
        return np.sign(e)

    def update(self, x, n_blocks=None):
        """x int16 [n_channels][stride_blocks][128], of which the first n_blocks blocks are new.  Returns the most bits any channel
        took in a block of the call."""
        x = np.asarray(x)
        assert x.dtype == np.int16 and x.shape[0] == self.n and x.shape[2] == 128
        nb = x.shape[1] if n_blocks is None else int(n_blocks)
        if nb == 0:
            return 0
        sg = self.signs(x[:, :nb].astype(np.int64)).tolist()
        most = 0
        for c in range(self.n):
            most = max(most, self.walk(c, sg[c], nb))
        self.blocks += nb
        return most

    def walk(self, c, sg, nb):
        """Steps 3 to 6 of channel c over the call's signs."""
        st = self.st
        g = {k: int(st[k][c]) for k in SCALARS}
        bits, edges, flags, frames, crc_errors, aborts = (g[k] for k in ("bits", "edges", "flags", "frames", "crc_errors", "aborts"))
        clk, ln, crc, b, prev, sr, cur, nbit, in_frame = (g[k] for k in ("clk", "len", "crc", "b", "prev", "sr", "cur", "nb", "in_frame"))
        buf = st["buf"][c]
        most = 0
        for blk in range(nb):
            before = bits
            for e in sg[32 * blk:32 * blk + 32]:
                new = 1 if e > 0 else (0 if e < 0 else b)
                if new != b:
                    r = clk if clk < HALF else clk - PERIOD
                    clk = (clk - (r >> 2)) % PERIOD
                    b = new
                    edges += 1
                p = clk
                clk += STEP
                take = p < HALF <= clk
                if clk >= PERIOD:
                    clk -= PERIOD
                if not take:
                    continue
                v = 1 if b == prev else 0
                prev = b
                bits += 1
                sr = (sr >> 1) | (v << 7)
                if sr == 0x7E:
                    flags += 1
                    if in_frame and nbit == 7 and ln >= MIN_LEN:
                        if crc == 0xF0B8:
                            self.complete(c, frames, self.blocks + blk, buf[:ln - 2])
                            frames += 1
                        else:
                            crc_errors += 1
                    in_frame, nbit, cur, ln, crc = 1, 0, 0, 0, 0xFFFF
                elif sr == 0xFE:
                    if in_frame and ln > 0:
                        aborts += 1
                    in_frame = 0
                elif (sr & 0xFC) == 0x7C:
                    pass
                elif in_frame:
                    cur |= v << nbit
                    nbit += 1
                    if nbit == 8:
                        if ln == MAX_LEN:
                            in_frame = 0
                        else:
                            buf[ln] = cur
                            ln += 1
                            crc = crc_step(crc, cur)
                        cur, nbit = 0, 0
            most = max(most, bits - before)
        for k, v in zip(SCALARS, (bits, edges, flags, frames, crc_errors, aborts, clk, ln, crc, b, prev, sr, cur, nbit, in_frame)):
            st[k][c] = v & 0xFFFFFFFF
        return most

    def complete(self, c, seq, block, payload):
        """Step 6."""
        f = np.zeros((), dtype=FRAME_DTYPE)
        f["channel"], f["seq"], f["block"], f["length"] = c, seq & 0xFFFFFFFF, block & 0xFFFFFFFF, len(payload)
        f["data"][:len(payload)] = payload
        if len(self.waiting[c]) == self.ring:
            self.waiting[c].pop(0)
            self.lost[c] += 1
        self.waiting[c].append(f)

    def collect(self, max_frames):
        """The frames a collect delivers, FRAME_DTYPE [count]: ascending by channel and, in a channel, from the oldest on, the first
        max_frames of that order; they leave their rings."""
        out = []
        for c in range(self.n):
            while self.waiting[c] and len(out) < max_frames:
                out.append(self.waiting[c].pop(0))
        return np.array(out, dtype=FRAME_DTYPE).reshape(-1)

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
        self.st.update(hist=z(8), dhist=z(8), reserved=z(11), buf=z(336))
        self.st["crc"] += 0xFFFF
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


# ---- signals
def frame_bits(payload, flags_before=4, flags_after=2, with_fcs=True):
    """The line bits (before NRZI) of one frame: flags, the payload and its FCS (the low byte first) with a 0 stuffed behind every
    five 1s, flags.  Every byte goes the low bit first."""
    body = bytes(payload)
    if with_fcs:
        v = fcs(body)
        body += bytes([v & 0xFF, v >> 8])
    out, ones = [], 0
    for byte in body:
        for s in range(8):
            bit = (byte >> s) & 1
            out.append(bit)
            ones = ones + 1 if bit else 0
            if ones == 5:
                out.append(0)
                ones = 0
    flag = [(FLAG >> s) & 1 for s in range(8)]
    return flag * flags_before + out + flag * flags_after


def afsk_wave(bits, amplitude, rate=1.0, lead=0.0, tail=64, fs=FS):
    """float64: the line bits as NRZI (a 0 changes the tone, a 1 keeps it) in phase-continuous 1200 / 2200 Hz AFSK at BAUD * rate,
    `lead` bit times of the starting tone in front and `tail` samples of silence behind."""
    bits = np.asarray(bits, dtype=np.int64)
    tone = np.concatenate([[0], np.cumsum(1 - bits) & 1])                  # 0: mark; the tone of bit k is tone[k + 1]
    n = int(np.ceil((lead + bits.size) * fs / (BAUD * rate)))
    k = np.floor(np.arange(n) * (BAUD * rate) / fs - lead).astype(np.int64)
    f = np.where(tone[np.clip(k + 1, 0, bits.size)] == 0, MARK, SPACE)
    phase = 2.0 * np.pi * np.cumsum(f) / fs
    return np.concatenate([amplitude * np.cos(phase), np.zeros(tail)])


def to_int16(x):
    return np.clip(np.floor(np.asarray(x, dtype=np.float64) + 0.5), -32768, 32767).astype(np.int16)


def blocks_of(x):
    """A signal padded with zeros to whole blocks: int16 [nb][128]."""
    x = to_int16(x)
    nb = -(-x.size // 128)
    return np.concatenate([x, np.zeros(nb * 128 - x.size, dtype=np.int16)]).reshape(nb, 128)


def ax25_address(call, ssid=0, last=False, repeated=False):
    return bytes((ord(ch) << 1) for ch in call.ljust(6)) + bytes([0x60 | (ssid << 1) | (1 if last else 0) | (0x80 if repeated else 0)])


def ui_frame(src="N0CALL", dst="APRS", path=(), info=b">hello"):
    """A UI frame's payload: addresses, control 0x03, PID 0xF0, info."""
    hops = [dst, src] + list(path)
    out = b""
    for k, h in enumerate(hops):
        name, _, ssid = h.rstrip("*").partition("-")
        out += ax25_address(name, int(ssid or 0), last=k == len(hops) - 1, repeated=h.endswith("*"))
    return out + b"\x03\xf0" + bytes(info)
