"""The packet decoder on the GPU (include/asdr_packet.h; audiosdr_amd/csrc/asdr_packet.hip) against tests/packet_ref.py at tolerance 0:
every state field, the records' bytes, blocks(), the ring state and every byte of the delivered frames (a guard pattern fills the
frame buffer and a slot behind it), the input left as it was, over partial workgroups of both instantiations, calls that end before,
in and behind a frame, strides, a different space_boost on every channel, every phase of the bit clock, the arithmetic's extremes,
ring overruns, the cut of a collect at max_frames, deliver, a sequence split in two ways, streams, setters between calls, a channel
moved mid-frame, and end to end behind a tuner bank and the FM demodulator.
The sizes are the smallest that reach each seam: a workgroup holds gpu.PACKET_NARROW_ROWS = 16 channels in a bank below
gpu.PACKET_WIDE_CHANNELS = 32768 channels and gpu.PACKET_ROWS = 64 from there on (a lane of its first wave each in the sequential
part)."""
import numpy as np
import pytest

import fm_ref as FR
import packet_ref as PR

pytestmark = pytest.mark.gpu
GAP = 0x7FFF        # fills the input strides' gaps: must not be read
PATTERN = 0xA5      # pre-fills the frame buffer: must stay wherever nothing is written


class Rig:
    """A packet decoder and its reference side by side; call() runs one update on both and compares everything, collect() one
    collect."""

    def __init__(self, A, n, ring=4):
        import torch
        self.torch, self.A, self.n, self.ring = torch, A, n, ring
        self.dec, self.ref = A.PacketDecoder(n, ring=ring), PR.PacketRef(n, ring=ring)

    def both(self, method, *args, **kw):
        getattr(self.dec, method)(*args, **kw)
        getattr(self.ref, method)(*args, **kw)

    def put(self, rec, channels=None):
        """Records into both sides."""
        self.dec.write_state(rec, channels=channels)
        for k, c in enumerate(range(len(rec)) if channels is None else channels):
            self.ref.put(c, rec[k])

    def call(self, x, extra_in=0, stream=None):
        """x int16 [n][nb][128]."""
        torch = self.torch
        n, nb = x.shape[:2]
        px = np.full((n, nb + extra_in, 128), GAP, dtype=np.int16)
        px[:, :nb] = x
        d_in = torch.from_numpy(px).cuda()
        torch.cuda.synchronize()
        self.dec.update_device(d_in.data_ptr(), nb, in_stride_blocks=nb + extra_in, stream=stream.cuda_stream if stream is not None else 0)
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        assert self.ref.update(x) <= 5
        assert np.array_equal(d_in.cpu().numpy(), px)
        self.check_state()

    def check_state(self):
        got, want = self.dec.read_state(), self.ref.records()
        for k in PR.STATE_NAMES:
            bad = [c for c in range(self.n) if not np.array_equal(got[k][c], want[k][c])]
            assert not bad, (k, len(bad), bad[0], got[k][bad[0]].tolist(), want[k][bad[0]].tolist())
        assert got.tobytes() == want.tobytes()
        assert self.dec.blocks() == self.ref.blocks
        pending, lost = self.dec.ring_state()
        want_pending, want_lost = self.ref.ring_state()
        assert np.array_equal(pending, want_pending) and np.array_equal(lost, want_lost), (pending.tolist(), want_pending.tolist())

    def collect(self, max_frames, stream=None):
        """One collect_device into a patterned buffer of max_frames slots and a guard slot; returns the reference's frames."""
        torch = self.torch
        d_frames = torch.full(((max_frames + 1) * 352,), PATTERN, dtype=torch.uint8, device="cuda")
        d_count = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.dec.collect_device(d_count.data_ptr(), d_frames.data_ptr(), max_frames, stream=stream.cuda_stream if stream is not None else 0)
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        want = self.ref.collect(max_frames)
        count = d_count.cpu().numpy()
        assert count[0] == len(want) and (count[1:] == 0x5A5A5A5A).all(), (count.tolist(), len(want))
        got = d_frames.cpu().numpy()
        frames = got[:len(want) * 352].view(PR.FRAME_DTYPE)
        for k in PR.FRAME_DTYPE.names:
            bad = [j for j in range(len(want)) if not np.array_equal(frames[k][j], want[k][j])]
            assert not bad, (k, len(bad), bad[0], frames[k][bad[0]].tolist(), want[k][bad[0]].tolist())
        assert frames.tobytes() == want.tobytes()
        assert (got[len(want) * 352:] == PATTERN).all(), "written behind the delivered frames"
        key = [(int(f["channel"]), int(f["seq"])) for f in want]
        assert key == sorted(key)
        self.check_state()
        return want

    def close(self):
        self.dec.close()


def payload_of(f):
    return f["data"][:int(f["length"])].tobytes()


def frames_in_noise(rng, n, nb, amplitude=4000.0, sigma=300.0, first=15, flags_first=4):
    """int16 [n][nb][128]: channel c carries frame after frame (the first of `first` bytes, the others of 15 to 40) in white noise,
    0 to 3 flags between them, starting a different fraction of a bit in; every fifth channel noise alone."""
    x = rng.normal(0.0, sigma, size=(n, nb * 128))
    for c in range(n):
        if c % 5 == 4:
            continue
        bits, size = [], first
        while len(bits) * 36.75 < nb * 128:
            p = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
            bits += PR.frame_bits(p, flags_before=flags_first if not bits else int(rng.integers(0, 4)), flags_after=1)
            size = int(rng.integers(15, 41))
        w = PR.afsk_wave(bits, amplitude, lead=2.0 + 0.13 * (c % 23))[:nb * 128]
        x[c, :w.size] += w
    return PR.to_int16(x).reshape(n, nb, 128)


def vary_boost(r):
    """Every channel different, inside one wave too."""
    for c in range(r.n):
        r.both("set_space_boost", (64, 128, 256, 400, 1024, 4000)[c % 6] + c % 97, ch=c)


# ---- partial workgroups of the narrow form; calls around a frame's end; strides; settings
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_channels_calls_and_strides(gpu, n):
    """One less, equal and one more than a workgroup's 16 channels; 33: three workgroups, the last with one channel.  A 17-byte frame
    behind three flags ends in block 48 to 50, by the channel's lead: calls of 1, 2, 3, 44, 45 and 100 blocks end before it, on
    either side of its end (the fourth call ends with block 49) and behind later frames.  Strides larger than n_blocks; a different
    space_boost on every channel; a collect between the calls and one behind them; a call of 0 blocks does nothing."""
    assert gpu.PACKET_NARROW_ROWS == 16 and n < gpu.PACKET_WIDE_CHANNELS
    rng = np.random.default_rng(100 + n)
    r = Rig(gpu, n)
    vary_boost(r)
    x = frames_in_noise(rng, n, 195, flags_first=3)
    a, delivered = 0, []
    for nb, ein in ((1, 0), (2, 3), (3, 1), (44, 0), (45, 2), (100, 0)):
        r.call(x[:, a:a + nb], extra_in=ein)
        a += nb
        if a == 95:
            delivered += list(r.collect(n * 4))
    delivered += list(r.collect(n * 4))
    st = r.ref.st
    assert (st["bits"] >= 660).all() and (st["bits"] <= 700).all()         # 195 blocks are 679 bits; edges in noise move the clock
    assert st["frames"].sum() >= n and len(delivered) == st["frames"].sum() - r.ref.lost.sum()
    if n >= 15:
        first = np.array([int(f["block"]) for f in delivered if f["seq"] == 0 and f["length"] == 15])
        assert first.size >= n // 2 and first.min() <= 49 and first.max() >= 50                          # either side of the fourth call's end
        assert not st["frames"][4::5].any() and st["frames"][np.arange(n) % 5 != 4].sum() >= n         # noise alone gives no frame
    d = r.torch.zeros((n, 2, 128), dtype=r.torch.int16, device="cuda")
    r.dec.update_device(d.data_ptr(), 0, in_stride_blocks=2)                                          # nothing happens
    r.check_state()
    r.close()


# ---- banks of PACKET_WIDE_CHANNELS channels and more: 64 channels per workgroup
DISTINCT = 37       # coprime to 64 and to 16: every workgroup sees another alignment of the repeated rows, records and settings


@pytest.fixture(scope="module")
def wide_reference():
    """The reference of 37 distinct channels, once: 44 blocks on the reference alone (every carried frame is under way), its records
    then, and on a fresh reference started from those records the last 8 blocks, in which the first frames end: (rows of the 8 blocks,
    boosts, the records before, the records after, the frames, the ring state)."""
    rng = np.random.default_rng(38)
    x = frames_in_noise(rng, DISTINCT, 52)
    boosts = [(128, 256, 400, 1024)[c % 4] + c for c in range(DISTINCT)]
    first = PR.PacketRef(DISTINCT)
    for c, b in enumerate(boosts):
        first.set_space_boost(b, ch=c)
    first.update(x[:, :44])
    start = first.records()
    assert not first.st["frames"].any() and (first.st["in_frame"] == 1).sum() > DISTINCT // 2 and (first.st["len"] > 8).sum() > DISTINCT // 2
    ref = PR.PacketRef(DISTINCT)
    for c, b in enumerate(boosts):
        ref.set_space_boost(b, ch=c)
        ref.put(c, start[c])
    ref.update(x[:, 44:])
    assert 5 <= ref.st["frames"].sum() < DISTINCT and len(set(ref.st["clk"].tolist())) > 10
    pending, lost = ref.ring_state()
    return x[:, 44:], boosts, start, ref.records(), [list(w) for w in ref.waiting], pending, lost


@pytest.mark.parametrize("n", [32768, 32769])
def test_wide_banks(gpu, wide_reference, n):
    """The size at which a workgroup takes 64 channels (PACKET_ROWS), and one channel more (a last workgroup of one channel): channels
    mid-frame written through write_state, 8 blocks with a stride larger than n_blocks, against the repeated reference: every record,
    the ring state, and every byte of every delivered frame."""
    import torch
    assert gpu.PACKET_WIDE_CHANNELS == 32768 and gpu.PACKET_ROWS == 64
    x, boosts, start, after, waiting, pending, lost = wide_reference
    sel = np.arange(n) % DISTINCT
    f = gpu.PacketDecoder(n, ring=2)
    L, h = f._L, f._h
    for c in range(n):
        assert L.asdr_packet_set_space_boost(h, c, boosts[c % DISTINCT]) == 0
    f.write_state(start[sel])
    px = np.full((n, 9, 128), GAP, dtype=np.int16)
    px[:, :8] = x[sel]
    d_in = torch.from_numpy(px).cuda()
    torch.cuda.synchronize()
    f.update_device(d_in.data_ptr(), 8, in_stride_blocks=9)
    f.synchronize()
    assert f.read_state().tobytes() == after[sel].tobytes() and f.blocks() == 8
    got_pending, got_lost = f.ring_state()
    assert np.array_equal(got_pending, pending[sel]) and np.array_equal(got_lost, lost[sel])
    want = []
    for c in range(n):
        for w in waiting[c % DISTINCT]:
            w = w.copy(); w["channel"] = c
            want.append(w)
    want = np.array(want, dtype=PR.FRAME_DTYPE).reshape(-1)
    total = len(want)
    assert total == int(pending[sel].sum()) and total > n // 8
    d_frames = torch.full(((total + 1) * 352,), PATTERN, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    f.collect_device(d_count.data_ptr(), d_frames.data_ptr(), total - 1)         # the cut falls in the last workgroups' channels
    f.synchronize()
    got = d_frames.cpu().numpy()
    assert int(d_count.cpu()[0]) == total - 1 and got[:(total - 1) * 352].tobytes() == want[:-1].tobytes() and (got[(total - 1) * 352:] == PATTERN).all()
    rest = f.deliver()
    assert rest.tobytes() == want[-1:].tobytes() and not f.ring_state()[0].any()
    assert np.array_equal(d_in.cpu().numpy(), px)
    f.close()


# ---- every clock phase
def test_every_clock_phase(gpu):
    """147 channels started, through write_state, from every clk in 0 .. 146 and both b, their signal shifted a sample at a time over
    37 channels (a bit is 36.75 samples: every phase between the sender's clock and the block grid is there); a call of one block,
    then the rest."""
    n = PR.PERIOD
    rng = np.random.default_rng(4)
    bits = PR.frame_bits(rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), flags_before=6)
    w = PR.afsk_wave(bits, 5000.0, lead=3.0)
    nb = -(-(w.size + 40) // 128)
    x = np.zeros((n, nb * 128))
    for c in range(n):
        x[c, c % 37:c % 37 + w.size] = w
    x = PR.to_int16(x + rng.normal(0.0, 200.0, x.shape)).reshape(n, nb, 128)
    r = Rig(gpu, n)
    rec = r.dec.read_state()
    rec["clk"] = np.arange(n); rec["b"] = np.arange(n) & 1; rec["prev"] = (np.arange(n) >> 1) & 1
    r.put(rec)
    r.call(x[:, :1])
    r.call(x[:, 1:], extra_in=1)
    frames = r.collect(n)
    assert len(frames) == n and all(payload_of(f) == payload_of(frames[0]) for f in frames)
    clks = np.array(r.ref.st["clk"][:37].tolist())
    assert len(set(clks.tolist())) >= 20                        # a sample's shift is 4 of clk's 147 units
    r.close()


# ---- extremes
def test_extremes_and_rows_of_zeros(gpu):
    """Constant -32768 and +32767, full-scale square waves at 1200 Hz, 2200 Hz and the decimated rate's half, a full-scale frame
    (clipped), rows of zeros, and zeros behind a signal; space_boost at both ends."""
    n, nb = 12, 70
    k = np.arange(nb * 128)
    x = np.zeros((n, nb * 128))
    x[0], x[1] = -32768, 32767
    for c, f in ((2, 1200.0), (3, 2200.0), (4, 11025.0 / 2), (5, 1700.0)):
        x[c] = np.where(np.floor(k * 2 * f / PR.FS) % 2 == 0, 32767, -32768)
    rng = np.random.default_rng(6)
    w = PR.afsk_wave(PR.frame_bits(rng.integers(0, 256, 15, dtype=np.uint8).tobytes()), 60000.0)
    for c in (6, 7, 8, 9):
        x[c, :w.size] = w
    x[9, w.size - 2000:] = 0                                    # cut off before the closing flag
    r = Rig(gpu, n)
    for c, b in ((2, 64), (3, 4096), (6, 64), (7, 4096)):
        r.both("set_space_boost", b, ch=c)
    x = PR.to_int16(x).reshape(n, nb, 128)
    r.call(x[:, :33])
    r.call(x[:, 33:], extra_in=1)
    rec = r.ref.records()
    assert int(rec["dhist"].min()) == -32768 and int(rec["dhist"].max()) == 32767
    st = r.ref.st
    assert not st["edges"][[10, 11]].any() and (st["bits"][[0, 1, 10, 11]] > 230).all()            # bits are taken from the held b
    assert st["frames"][8] == 1 and st["frames"][9] == 0
    r.call(np.zeros((n, 6, 128), dtype=np.int16))
    r.collect(n)
    r.close()


# ---- ring overruns
@pytest.mark.parametrize("ring", [1, 2])
def test_ring_overrun(gpu, ring):
    """Three or four frames a channel and no collect in between: the ring keeps the newest `ring`, lost counts the others, and the frames
    that arrive are the newest by seq.  Then clear (lost goes, the waiting frames stay) and reset (they go)."""
    rng = np.random.default_rng(7 + ring)
    n = 5
    r = Rig(gpu, n, ring=ring)
    x = frames_in_noise(rng, n, 260, first=15)
    r.call(x[:, :130])
    r.call(x[:, 130:])
    pending, lost = r.ref.ring_state()
    made = r.ref.st["frames"]
    assert (made[:4] > ring).all() and pending[:4].tolist() == [ring] * 4 and np.array_equal(lost, made - pending) and lost[:4].min() >= 1
    r.both("clear")
    r.check_state()
    assert not r.dec.ring_state()[1].any() and r.dec.ring_state()[0][:4].tolist() == [ring] * 4 and r.dec.blocks() == 0
    frames = r.collect(1)
    frames = np.concatenate([frames, r.collect(n * ring)])
    assert len(frames) == 4 * ring
    for c in range(4):
        assert frames["seq"][frames["channel"] == c].tolist() == list(range(made[c] - ring, made[c]))
    r.call(x[:, :130])
    assert r.ref.ring_state()[0].any()
    r.both("reset")
    r.check_state()
    assert not r.dec.ring_state()[0].any() and r.dec.read_state().tobytes() == PR.PacketRef(n).records().tobytes()
    assert len(r.collect(4)) == 0
    r.call(x[:, :60])
    r.collect(n)
    r.close()


def test_reset_and_clear_are_done_on_return_for_a_call_on_any_stream(gpu):
    """reset, then clear, each followed at once (no state call, no synchronisation in between) by a call and a collect on a caller's
    non-blocking stream: the rings are empty for that call, nothing of it is wiped afterwards, and the frames it decodes arrive.  A
    ring of 3 slots (no power of two) that turns several times, with collects in between."""
    import torch
    rng = np.random.default_rng(21)
    n = 18
    r = Rig(gpu, n, ring=3)
    x = frames_in_noise(rng, n, 520)
    s = torch.cuda.Stream()
    r.call(x[:, :200], stream=s)
    assert r.ref.ring_state()[0].max() >= 2
    for method, a, b in (("reset", 0, 200), ("clear", 200, 360)):
        d_in = torch.from_numpy(x[:, a:b].copy()).cuda()
        torch.cuda.synchronize()
        getattr(r.dec, method)()
        r.dec.update_device(d_in.data_ptr(), b - a, stream=s.cuda_stream)
        getattr(r.ref, method)()
        r.ref.update(x[:, a:b])
        assert len(r.collect(2, stream=s)) == 2
        r.check_state()
    r.call(x[:, 360:], stream=s)
    assert r.ref.st["frames"].max() >= 7 and r.ref.lost.sum() > 0                              # the rings turned and overran
    assert len(r.collect(n * 3, stream=s)) > n
    r.close()


# ---- the cut of a collect; deliver
def test_collect_cuts_at_max_frames_and_deliver(gpu):
    """max_frames of 0, of one less than the total and of the total; the rest arrive on the next collect, ascending by (channel,
    seq); deliver with frames waiting, with a cut, and with none."""
    rng = np.random.default_rng(9)
    n = 21
    r = Rig(gpu, n, ring=4)
    x = frames_in_noise(rng, n, 200)
    r.call(x[:, :120])
    total = int(r.ref.ring_state()[0].sum())
    assert total > n // 2 and r.ref.ring_state()[0].max() >= 2
    assert len(r.collect(0)) == 0
    assert int(r.dec.ring_state()[0].sum()) == total
    part = r.collect(total - 1)
    assert len(part) == total - 1
    last = r.collect(total)
    assert len(last) == 1 and (int(last[0]["channel"]), int(last[0]["seq"])) > (int(part[-1]["channel"]), int(part[-1]["seq"]))
    assert len(r.collect(total)) == 0
    r.call(x[:, 120:])
    want = r.ref.collect(3)
    got = r.dec.deliver(3)
    assert len(want) == 3 and got.dtype == gpu.PACKET_FRAME_DTYPE and got.tobytes() == want.tobytes()
    r.check_state()
    want = r.ref.collect(n * 4)
    got = r.dec.deliver()
    assert len(want) > 3 and got.tobytes() == want.tobytes()
    assert gpu.packet_format_address(PR.ui_frame()) == "N0CALL>APRS"
    r.check_state()
    got = r.dec.deliver()                                       # no frame pending
    assert got.shape == (0,) and len(r.dec.deliver(0)) == 0
    r.check_state()
    r.close()


# ---- split invariance
def test_one_sequence_as_one_call_and_as_many(gpu):
    import torch
    rng = np.random.default_rng(800)
    n, nb = 21, 190
    x = frames_in_noise(rng, n, nb)
    d_in = torch.from_numpy(x).cuda()
    recs, frames, rings = [], [], []
    for sizes in ((nb,), (1, 2, 3, 5, 8, 13, 21, 34, 53, 50), tuple([1] * 20 + [170])):
        assert sum(sizes) == nb
        f = gpu.PacketDecoder(n, ring=8)
        for c in range(n):
            f.set_space_boost((128, 256, 400)[c % 3] + c, ch=c)
        a = 0
        for size in sizes:
            f.update_device(d_in[:, a:].data_ptr(), size, in_stride_blocks=nb)
            a += size
        f.synchronize()
        recs.append(f.read_state()); rings.append(f.ring_state()); frames.append(f.deliver())
        assert f.blocks() == nb
        f.close()
    ref = PR.PacketRef(n, ring=8)
    for c in range(n):
        ref.set_space_boost((128, 256, 400)[c % 3] + c, ch=c)
    ref.update(x)
    assert recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes() == ref.records().tobytes()
    assert all(np.array_equal(g[0], rings[0][0]) and np.array_equal(g[1], rings[0][1]) for g in rings)
    want = ref.collect(n * 8)
    assert frames[0].tobytes() == frames[1].tobytes() == frames[2].tobytes() == want.tobytes() and len(want) > n


# ---- streams, setters between calls, and a channel moved mid-frame
def test_streams_setters_between_calls_and_a_channel_moved_mid_frame(gpu):
    """A call and a collect on a caller's stream; 130 blocks as 1 + 64 + 65 alternating between two streams with no host
    synchronisation in between; space_boost changed between calls.  Then a channel mid-frame moves to a slot of another handle
    through read_state / write_state: its next frame is bit-identical to the uninterrupted one."""
    import torch
    rng = np.random.default_rng(700)
    n = 37
    r = Rig(gpu, n)
    vary_boost(r)
    x = frames_in_noise(rng, n, 230, first=30)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    r.call(x[:, :5], stream=streams[0])
    d_in = torch.from_numpy(x[:, 5:135].copy()).cuda()
    torch.cuda.synchronize()
    for k, (a, size) in enumerate(((0, 1), (1, 64), (65, 65))):
        r.dec.update_device(d_in[:, a:].data_ptr(), size, in_stride_blocks=130, stream=streams[k & 1].cuda_stream)
    r.dec.synchronize()
    r.ref.update(x[:, 5:135])
    r.check_state()
    assert np.array_equal(d_in.cpu().numpy(), x[:, 5:135])
    assert len(r.collect(n * 4, stream=streams[1])) >= n // 2
    r.both("set_space_boost", 300, ch=2); r.both("set_space_boost", 64)
    r.both("set_space_boost", 256); r.both("set_space_boost", 333, ch=n - 1)
    r.call(x[:, 135:150], stream=streams[1])
    mid = [c for c in range(n) if r.ref.st["in_frame"][c] == 1 and 10 < r.ref.st["len"][c] < 25 and c != n - 1]
    assert mid
    c = mid[0]
    rec = r.dec.read_state()[c:c + 1]
    b = Rig(gpu, 19)
    b.both("set_space_boost", 256)
    b.put(rec, channels=[18])
    x2 = frames_in_noise(rng, 19, 80)
    x2[18] = x[c, 150:]
    b.call(x2)
    r.call(x[:, 150:])
    moved = [f for f in b.collect(19 * 4) if f["channel"] == 18]
    stayed = [f for f in r.collect(n * 4) if f["channel"] == c]
    assert moved and len(moved) == len(stayed)
    for f, g in zip(moved, stayed):
        assert f["seq"] == g["seq"] and f["length"] == g["length"] and f["data"].tobytes() == g["data"].tobytes()
        assert int(f["block"]) == int(g["block"]) - 150
    assert b.dec.read_state()[18].tobytes() == r.ref.records()[c].tobytes()
    for field, value, why in (("clk", 147, "clk"), ("len", 333, "len"), ("nb", 8, "nb"), ("b", 2, "b must"), ("in_frame", 2, "in_frame"),
                              ("reserved", 1, "reserved")):
        bad = rec.copy(); bad[field] = value
        with pytest.raises(gpu.AsdrError, match=why):
            b.dec.write_state(bad, channels=[0])
    b.check_state()
    r.close(); b.close()


def test_refusals_change_nothing(gpu):
    import torch
    r = Rig(gpu, 10)
    d = torch.zeros((10, 4, 128), dtype=torch.int16, device="cuda")
    fr = torch.zeros(8 * 352, dtype=torch.uint8, device="cuda")
    i, o = d.data_ptr(), fr.data_ptr()
    for kw, why in ((dict(in_ptr=i + 2, n_blocks=1), "16-byte"), (dict(in_ptr=i, n_blocks=3, in_stride_blocks=2), "stride"),
                    (dict(in_ptr=i, n_blocks=65536, in_stride_blocks=65536), "n_blocks"), (dict(in_ptr=i, n_blocks=-1), "n_blocks"),
                    (dict(in_ptr=0, n_blocks=1), "null")):
        with pytest.raises(gpu.AsdrError, match=why):
            r.dec.update_device(**kw)
    for args, why in (((o + 2, o + 16, 4), "aligned"), ((o, o + 8, 4), "aligned"), ((0, o, 4), "null"), ((o, 0, 4), "null"),
                      ((o, o + 16, -1), "max_frames"), ((o, o + 16, (1 << 24) + 1), "max_frames")):
        with pytest.raises(gpu.AsdrError, match=why):
            r.dec.collect_device(*args)
    with pytest.raises(gpu.AsdrError, match="max_frames"):
        r.dec.deliver(-1)
    r.check_state()
    assert not fr.cpu().numpy().any()
    r.close()


# ---- end to end
def test_tuner_bank_to_fm_to_packet_decoder(gpu):
    """A CU8 wideband source at 48 x 44.1 kHz with two FM carriers (3 kHz deviation) whose modulation is AFSK carrying one frame each;
    channels 0 and 2 are tuned to them, channels 1 and 3 beside them where there is only noise.  Tuner bank, FM demodulator (a = 32768:
    no de-emphasis, as advised for packet channels) and packet decoder run on one stream with no host step in between.  The frames
    equal those of fm_ref -> packet_ref on the I/Q rows the bank wrote (the bank itself is held to its own restatement elsewhere), and
    they are the frames that were sent."""
    import torch
    D, n = 48, 4
    payloads = [PR.ui_frame(src="DL1ABC-7", path=("WIDE1-1",), info=b"!4903.50N/07201.75W-end to end"), PR.ui_frame(info=b">second carrier")]
    mods = [PR.afsk_wave(PR.frame_bits(p, flags_before=10), 1.0, lead=2.0 + k, tail=3000 * D, fs=PR.FS * D) for k, p in enumerate(payloads)]
    nb = -(-max(m.size for m in mods) // (128 * D))
    fs, N = 44100 * D, nb * 128 * D
    rng = np.random.default_rng(5)
    t = np.arange(N) / fs
    x = np.zeros(N, dtype=np.complex128)
    carriers = [100e3, 300e3]
    for fc, m in zip(carriers, mods):
        m = np.concatenate([m, np.zeros(N - m.size)])
        x += 25.0 * np.exp(1j * (2 * np.pi * fc * t + 2 * np.pi * 3000.0 * np.cumsum(m) / fs))
    x = x + rng.normal(0.0, 1.5, N) + 1j * rng.normal(0.0, 1.5, N)
    raw = np.clip(np.floor(np.stack([x.real, x.imag], axis=-1) + 128.0), 0, 255).astype(np.uint8)[None]
    bank = gpu.TunerBank(n, 1, D)
    bank.set_input_format("cu8")
    for c in range(n):
        bank.set_frequency(carriers[c // 2] + (50e3 if c & 1 else 0.0), ch=c)
    fm, dec = gpu.FmDemodulator(n), gpu.PacketDecoder(n)
    fm.set_deemphasis(a=32768)
    s = torch.cuda.Stream()
    d_raw = torch.from_numpy(raw).cuda()
    dI, dQ, d_audio = (torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda") for _ in range(3))
    d_frames = torch.full((5 * 352,), PATTERN, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert bank.update_samples_device(d_raw.data_ptr(), dI.data_ptr(), dQ.data_ptr(), nb, nb, stream=s.cuda_stream) == nb
    fm.update_device(dI.data_ptr(), dQ.data_ptr(), d_audio.data_ptr(), nb, stream=s.cuda_stream)
    dec.update_device(d_audio.data_ptr(), nb, stream=s.cuda_stream)
    dec.collect_device(d_count.data_ptr(), d_frames.data_ptr(), 4, stream=s.cuda_stream)
    s.synchronize()
    fref, pref = FR.FmRef(n), PR.PacketRef(n)
    fref.set_deemphasis(32768)
    audio = fref.update(dI.cpu().numpy(), dQ.cpu().numpy())[0]
    assert np.array_equal(d_audio.cpu().numpy(), audio)
    pref.update(audio)
    assert dec.read_state().tobytes() == pref.records().tobytes()
    want = pref.collect(4)
    assert [(int(f["channel"]), payload_of(f)) for f in want] == [(0, payloads[0]), (2, payloads[1])]
    got = d_frames.cpu().numpy()
    assert int(d_count.cpu()[0]) == 2 and got[:2 * 352].tobytes() == want.tobytes() and (got[2 * 352:] == PATTERN).all()
    frames = got[:2 * 352].view(gpu.PACKET_FRAME_DTYPE)
    assert gpu.packet_format_address(frames[0]) == "DL1ABC-7>APRS,WIDE1-1" and gpu.packet_format_address(frames[1]) == "N0CALL>APRS"
    bank.close(); fm.close(); dec.close()
