"""The CW decoder on the GPU (include/asdr_cw.h; audiosdr_amd/csrc/asdr_cw.hip) against tests/cw_ref.py at tolerance 0: every state
field, the records' bytes, blocks(), the ring state and every byte of the delivered events (a guard pattern fills the event buffer
and a slot behind it), the input left as it was, over partial workgroups of both instantiations, calls of 1, 2 and 7 blocks and
longer, strides, different settings on every channel, phases and steps at the ends of 32 bits, the arithmetic's extremes, ring
overruns, the cut of a collect at max_events, deliver, a sequence split in two ways, streams, setters between calls, a channel moved
mid-character, and end to end behind the chain in CW mode.
The sizes are the smallest that reach each seam: a workgroup holds gpu.CW_NARROW_ROWS = 16 channels in a bank below
gpu.CW_WIDE_CHANNELS = 32768 channels and gpu.CW_ROWS = 64 from there on (a lane of its first wave each in steps 2 to 7)."""
import numpy as np
import pytest

import cw_ref as R

pytestmark = pytest.mark.gpu
GAP = 0x7FFF        # fills the input strides' gaps: must not be read
PATTERN = 0xA5      # pre-fills the event buffer: must stay wherever nothing is written


class Rig:
    """A CW decoder and its reference side by side; call() runs one update on both and compares everything, collect() one collect."""

    def __init__(self, A, n, ring=16):
        import torch
        self.torch, self.A, self.n, self.ring = torch, A, n, ring
        self.dec, self.ref = A.CwDecoder(n, ring=ring), R.CwRef(n, ring=ring)

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
        big, p_max = self.ref.update(x)
        assert big <= 1 << 20 and p_max < 1 << 31
        assert np.array_equal(d_in.cpu().numpy(), px)
        self.check_state()

    def check_state(self):
        got, want = self.dec.read_state(), self.ref.records()
        for k in R.STATE_NAMES:
            bad = [c for c in range(self.n) if not np.array_equal(got[k][c], want[k][c])]
            assert not bad, (k, len(bad), bad[0], got[k][bad[0]].tolist(), want[k][bad[0]].tolist())
        assert got.tobytes() == want.tobytes()
        assert self.dec.blocks() == self.ref.blocks
        pending, lost = self.dec.ring_state()
        want_pending, want_lost = self.ref.ring_state()
        assert np.array_equal(pending, want_pending) and np.array_equal(lost, want_lost), (pending.tolist(), want_pending.tolist())

    def collect(self, max_events, stream=None):
        """One collect_device into a patterned buffer of max_events slots and a guard slot; returns the reference's events."""
        torch = self.torch
        d_events = torch.full(((max_events + 1) * 16,), PATTERN, dtype=torch.uint8, device="cuda")
        d_count = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.dec.collect_device(d_count.data_ptr(), d_events.data_ptr(), max_events, stream=stream.cuda_stream if stream is not None else 0)
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        want = self.ref.collect(max_events)
        count = d_count.cpu().numpy()
        assert count[0] == len(want) and (count[1:] == 0x5A5A5A5A).all(), (count.tolist(), len(want))
        got = d_events.cpu().numpy()
        events = got[:len(want) * 16].view(R.EVENT_DTYPE)
        for k in R.EVENT_DTYPE.names:
            bad = [j for j in range(len(want)) if events[k][j] != want[k][j]]
            assert not bad, (k, len(bad), bad[0], int(events[k][bad[0]]), int(want[k][bad[0]]), int(want["channel"][bad[0]]))
        assert events.tobytes() == want.tobytes()
        assert (got[len(want) * 16:] == PATTERN).all(), "written behind the delivered events"
        key = [(int(e["channel"]), int(e["seq"])) for e in want]
        assert key == sorted(key)
        self.check_state()
        return want

    def close(self):
        self.dec.close()


PITCHES = (774.0, 600.0, 1000.0, 450.5, 2999.0, 100.0)


def keyed_rows(rng, n, nb):
    """int16 [n][nb][128]: channel c carries random keying (marks of 1 or 3 dits, gaps of 1, 3 or 7) at 40 to 60 WPM on the tone
    PITCHES[c % 6] with an amplitude of 1,000 to 20,000 in noise of rms 100 to 400, its edges anywhere in a block; every fifth
    channel noise alone, of rms 3,000, which keys characters, glitches and unknown codes of its own."""
    N = nb * 128
    x = np.zeros((n, N))
    t = np.arange(N)
    for c in range(n):
        if c % 5 == 4:
            x[c] = rng.normal(0.0, 3000.0, N)
            continue
        dit = R.FS * 1.2 / rng.uniform(40.0, 60.0)
        gate, a = np.zeros(N), int(rng.integers(0, 400))
        while a < N:
            m = int(dit * (1 if rng.random() < 0.55 else 3) * rng.uniform(0.9, 1.1))
            gate[a:a + m] = 1.0
            a += m + int(dit * (1, 1, 1, 3, 3, 7)[int(rng.integers(0, 6))] * rng.uniform(0.9, 1.1))
        x[c] = rng.uniform(1000.0, 20000.0) * gate * np.cos(2 * np.pi * PITCHES[c % 6] * t / R.FS + rng.uniform(0, 6.28)) + \
            rng.normal(0.0, rng.uniform(100.0, 400.0), N)
    return R.to_int16(x).reshape(n, nb, 128)


def vary_settings(r):
    """Every channel different, inside one wave too; the speed near the senders' (D of the record)."""
    r.both("set_speed", 50)
    for c in range(r.n):
        r.both("set_pitch_step", R.pitch_step(PITCHES[c % 6]) + c % 7, ch=c)
        r.both("set_min_power", (16, 0, 500, 100000)[c % 4], ch=c)
        r.both("set_glitch", 1 + (c * 5) % 16, ch=c)
        r.both("set_track", 0 if c % 9 == 8 else 1, ch=c)


# ---- partial workgroups of the narrow form; short calls; strides; settings
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65])
def test_channels_calls_and_strides(gpu, n):
    """One less, equal and one more than a workgroup's 16 channels, and around four workgroups; calls of 1, 2 and 7 blocks and longer
    ones, strides larger than n_blocks; different settings on every channel; a collect between the calls and one behind them; a call
    of 0 blocks does nothing."""
    assert gpu.CW_NARROW_ROWS == 16 and n < gpu.CW_WIDE_CHANNELS
    rng = np.random.default_rng(100 + n)
    r = Rig(gpu, n)
    vary_settings(r)
    x = keyed_rows(rng, n, 300)
    a, delivered = 0, []
    for nb, ein in ((1, 0), (2, 3), (7, 1), (1, 2), (40, 0), (2, 0), (7, 0), (240, 5)):
        r.call(x[:, a:a + nb], extra_in=ein)
        a += nb
        if a == 60:
            delivered += list(r.collect(n * 16))
    assert a == 300
    delivered += list(r.collect(n * 16))
    st = r.ref.st
    assert len(delivered) == int(st["chars"].sum() - r.ref.lost.sum()) and st["marks"].sum() >= n
    if n >= 15:
        assert st["glitches"].sum() > 0 and len({int(e["ch"]) for e in delivered}) > 5 and len(set(st["D"].tolist())) > n // 2
    if n >= 63:
        assert st["unknown"].sum() > 0 and {int(e["flags"]) for e in delivered} == {0, 1}
    d = r.torch.zeros((n, 2, 128), dtype=r.torch.int16, device="cuda")
    r.dec.update_device(d.data_ptr(), 0, in_stride_blocks=2)                                          # nothing happens
    r.check_state()
    r.close()


# ---- banks of CW_WIDE_CHANNELS channels and more: 64 channels per workgroup
DISTINCT = 37       # coprime to 64 and to 16: every workgroup sees another alignment of the repeated rows, records and settings
WIDE_SETTINGS = [(R.pitch_step(PITCHES[c % 6]) + c, (16, 0, 500)[c % 3], 1 + c % 16, 0 if c % 9 == 8 else 1) for c in range(DISTINCT)]


def wide_ref():
    ref = R.CwRef(DISTINCT, ring=2)
    ref.set_speed(50)
    for c, (step, power, glitch, track) in enumerate(WIDE_SETTINGS):
        ref.set_pitch_step(step, ch=c); ref.set_min_power(power, ch=c); ref.set_glitch(glitch, ch=c); ref.set_track(track, ch=c)
    return ref


@pytest.fixture(scope="module")
def wide_reference():
    """The reference of 37 distinct channels, once: 200 blocks on the reference alone (every carried channel is mid-message), its
    records then, and on a fresh reference started from those records the next 24 blocks: (rows of the 24 blocks, the records before,
    the records after, the events, the ring state)."""
    rng = np.random.default_rng(38)
    x = keyed_rows(rng, DISTINCT, 224)
    first = wide_ref()
    first.update(x[:, :200])
    start = first.records()
    assert (first.st["marks"] > 0).sum() > DISTINCT // 2 and len(set(first.st["ph"].tolist())) == DISTINCT
    ref = wide_ref()
    for c in range(DISTINCT):
        ref.put(c, start[c])
    ref.update(x[:, 200:])
    pending, lost = ref.ring_state()
    assert pending.sum() >= 5
    return x[:, 200:], start, ref.records(), [list(w) for w in ref.waiting], pending, lost


@pytest.mark.parametrize("n", [32768, 32831])
def test_wide_banks(gpu, wide_reference, n):
    """The size at which a workgroup takes 64 channels (CW_ROWS), and 63 channels more (a last workgroup one row short): channels
    mid-message written through write_state, 24 blocks with a stride larger than n_blocks, against the repeated reference: every
    record, the ring state, and every byte of every delivered event."""
    import torch
    assert gpu.CW_WIDE_CHANNELS == 32768 and gpu.CW_ROWS == 64
    x, start, after, waiting, pending, lost = wide_reference
    sel = np.arange(n) % DISTINCT
    f = gpu.CwDecoder(n, ring=2)
    L, h = f._L, f._h
    for c in range(n):
        step, power, glitch, track = WIDE_SETTINGS[c % DISTINCT]
        assert L.asdr_cw_set_pitch_step(h, c, step) == 0 and L.asdr_cw_set_min_power(h, c, power) == 0
        assert L.asdr_cw_set_glitch(h, c, glitch) == 0 and L.asdr_cw_set_track(h, c, track) == 0
    f.write_state(start[sel])
    px = np.full((n, 25, 128), GAP, dtype=np.int16)
    px[:, :24] = x[sel]
    d_in = torch.from_numpy(px).cuda()
    torch.cuda.synchronize()
    f.update_device(d_in.data_ptr(), 24, in_stride_blocks=25)
    f.synchronize()
    assert f.read_state().tobytes() == after[sel].tobytes() and f.blocks() == 24
    got_pending, got_lost = f.ring_state()
    assert np.array_equal(got_pending, pending[sel]) and np.array_equal(got_lost, lost[sel])
    want = []
    for c in range(n):
        for w in waiting[c % DISTINCT]:
            w = w.copy(); w["channel"] = c
            want.append(w)
    want = np.array(want, dtype=R.EVENT_DTYPE).reshape(-1)
    total = len(want)
    assert total == int(pending[sel].sum()) and total >= 5 * (n // DISTINCT)
    d_events = torch.full(((total + 1) * 16,), PATTERN, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    f.collect_device(d_count.data_ptr(), d_events.data_ptr(), total - 1)         # the cut falls in the last workgroups' channels
    f.synchronize()
    got = d_events.cpu().numpy()
    assert int(d_count.cpu()[0]) == total - 1 and got[:(total - 1) * 16].tobytes() == want[:-1].tobytes() and (got[(total - 1) * 16:] == PATTERN).all()
    rest = f.deliver()
    assert rest.tobytes() == want[-1:].tobytes() and not f.ring_state()[0].any()
    assert np.array_equal(d_in.cpu().numpy(), px)
    f.close()


# ---- phases, steps and the arithmetic's extremes
def test_phases_steps_extremes_and_rows_of_zeros(gpu):
    """Steps of 0, 1, 2^31, 2^32 - 1 and of 3,000 Hz, started (through write_state) from phases at and next to the wrap; constant
    -32768 and +32767, the square wave aligned with the pitch (the most a row can put on it), full-scale alternation, rows of zeros,
    and zeros behind a signal; min_power at both ends; prev_i / prev_q at their bounds."""
    n, nb = 14, 40
    k = np.arange(nb * 128)
    x = np.zeros((n, nb * 128))
    x[0], x[1] = -32768, 32767
    x[2] = np.where(np.cos(2 * np.pi * R.PITCH_HZ * k / R.FS) >= 0, 32767, -32768)
    x[3] = np.where(k % 2 == 0, 32767, -32768)
    x[4] = np.where(k // 28 % 2 == 0, -32768, 32767)
    rng = np.random.default_rng(6)
    for c in range(5, 12):
        x[c] = keyed_rows(rng, 1, nb)[0].reshape(-1) * 3.0                     # clipped
    x[11, 2000:] = 0
    steps = {5: 0, 6: 1, 7: 1 << 31, 8: (1 << 32) - 1, 9: R.pitch_step(3000), 10: R.pitch_step(100)}
    r = Rig(gpu, n)
    for c, s in steps.items():
        r.both("set_pitch_step", s, ch=c)
    r.both("set_min_power", (1 << 32) - 1, ch=1); r.both("set_min_power", 0, ch=2); r.both("set_min_power", 0, ch=13)
    rec = r.dec.read_state()
    rec["ph"] = [(1 << 32) - 1 - 7 * c if c % 2 else 5 * c for c in range(n)]
    rec["prev_i"][12] = (1 << 20, 1 << 20, 1 << 20); rec["prev_q"][12] = (-(1 << 20), -(1 << 20), -(1 << 20))
    rec["prev_i"][13] = (-(1 << 20), 1 << 20, 7); rec["hi"][13] = (1 << 32) - 1; rec["lo"][13] = (1 << 32) - 1; rec["run"][13] = (1 << 32) - 2
    r.put(rec)
    x = R.to_int16(x).reshape(n, nb, 128)
    r.call(x[:, :1])
    r.call(x[:, 1:3], extra_in=1)
    r.call(x[:, 3:])
    assert int(r.ref.st["key"][1]) == 0 and int(r.ref.st["marks"][1]) == 0                   # min_power at its end keys nothing
    r.call(np.zeros((n, 6, 128), dtype=np.int16))
    r.collect(n * 16)
    r.close()


# ---- ring overruns
@pytest.mark.parametrize("ring", [1, 3])
def test_ring_overrun(gpu, ring):
    """Many characters a channel and no collect in between: the ring keeps the newest `ring`, lost counts the others, and the events
    that arrive are the newest by seq.  Then clear (lost goes, the waiting events stay, chars stays) and reset (they go)."""
    rng = np.random.default_rng(7 + ring)
    n = 5
    r = Rig(gpu, n, ring=ring)
    x = keyed_rows(rng, n, 700)
    r.both("set_speed", 50)
    r.call(x[:, :330])
    r.call(x[:, 330:])
    pending, lost = r.ref.ring_state()
    made = r.ref.st["chars"].copy()
    assert (made > ring).sum() >= 4 and np.array_equal(pending, np.minimum(made, ring)) and np.array_equal(lost, made - pending)
    r.both("clear")
    r.check_state()
    assert not r.dec.ring_state()[1].any() and np.array_equal(r.dec.ring_state()[0], pending) and r.dec.blocks() == 0
    assert np.array_equal(r.dec.read_state()["chars"], made)
    events = r.collect(1)
    events = np.concatenate([events, r.collect(n * ring)])
    assert len(events) == int(pending.sum())
    for c in range(n):
        assert events["seq"][events["channel"] == c].tolist() == list(range(made[c] - pending[c], made[c]))
    r.call(x[:, :330])
    assert r.ref.ring_state()[0].any()
    r.both("reset")
    r.check_state()
    assert not r.dec.ring_state()[0].any() and r.dec.read_state().tobytes() == R.CwRef(n).records().tobytes()
    assert len(r.collect(4)) == 0
    r.call(x[:, :60])
    r.collect(n * ring)
    r.close()


def test_reset_and_clear_are_done_on_return_for_a_call_on_any_stream(gpu):
    """reset, then clear, each followed at once (no state call, no synchronisation in between) by a call and a collect on a caller's
    non-blocking stream: the rings are empty for that call, nothing of it is wiped afterwards, and the events it decodes arrive.  A
    ring of 3 slots (no power of two) that turns several times, with collects in between."""
    import torch
    rng = np.random.default_rng(21)
    n = 18
    r = Rig(gpu, n, ring=3)
    x = keyed_rows(rng, n, 900)
    r.both("set_speed", 50)
    s = torch.cuda.Stream()
    r.call(x[:, :300], stream=s)
    assert r.ref.ring_state()[0].max() >= 2
    for method, a, b in (("reset", 0, 300), ("clear", 300, 600)):
        d_in = torch.from_numpy(x[:, a:b].copy()).cuda()
        torch.cuda.synchronize()
        getattr(r.dec, method)()
        r.dec.update_device(d_in.data_ptr(), b - a, stream=s.cuda_stream)
        getattr(r.ref, method)()
        r.ref.update(x[:, a:b])
        assert len(r.collect(2, stream=s)) == 2
        r.check_state()
    r.call(x[:, 600:], stream=s)
    assert r.ref.st["chars"].max() >= 7 and r.ref.lost.sum() > 0                               # the rings turned and overran
    assert len(r.collect(n * 3, stream=s)) > n
    r.close()


# ---- the cut of a collect; deliver
def test_collect_cuts_at_max_events_and_deliver(gpu):
    """max_events of 0, of one less than the total and of the total; the rest arrive on the next collect, ascending by (channel,
    seq); deliver with events waiting, with a cut, and with none; CwDecoder.text joins a channel's characters."""
    rng = np.random.default_rng(9)
    n = 21
    r = Rig(gpu, n, ring=8)
    x = keyed_rows(rng, n, 400)
    r.both("set_speed", 50)
    r.call(x[:, :240])
    total = int(r.ref.ring_state()[0].sum())
    assert total > n and r.ref.ring_state()[0].max() >= 2
    assert len(r.collect(0)) == 0
    assert int(r.dec.ring_state()[0].sum()) == total
    part = r.collect(total - 1)
    assert len(part) == total - 1
    last = r.collect(total)
    assert len(last) == 1 and (int(last[0]["channel"]), int(last[0]["seq"])) > (int(part[-1]["channel"]), int(part[-1]["seq"]))
    assert len(r.collect(total)) == 0
    r.call(x[:, 240:])
    want = r.ref.collect(3)
    got = r.dec.deliver(3)
    assert len(want) == 3 and got.dtype == gpu.CW_EVENT_DTYPE and got.tobytes() == want.tobytes()
    r.check_state()
    want = r.ref.collect(n * 8)
    got = r.dec.deliver()
    assert len(want) > 3 and got.tobytes() == want.tobytes()
    c = int(want[0]["channel"])
    assert gpu.CwDecoder.text(got, channel=c) == R.text_of(want, channel=c) != ""
    r.check_state()
    got = r.dec.deliver()                                       # no event pending
    assert got.shape == (0,) and len(r.dec.deliver(0)) == 0
    r.check_state()
    r.close()


# ---- split invariance
def test_one_sequence_as_one_call_and_as_many(gpu):
    import torch
    rng = np.random.default_rng(800)
    n, nb = 21, 380
    x = keyed_rows(rng, n, nb)
    d_in = torch.from_numpy(x).cuda()
    recs, events, rings = [], [], []
    for sizes in ((nb,), (1, 2, 3, 5, 8, 13, 21, 34, 53, 240), tuple([1] * 20 + [360])):
        assert sum(sizes) == nb
        f = gpu.CwDecoder(n, ring=32)
        f.set_speed(50)
        for c in range(n):
            f.set_pitch(PITCHES[c % 6], ch=c); f.set_glitch(1 + c % 16, ch=c)
        a = 0
        for size in sizes:
            f.update_device(d_in[:, a:].data_ptr(), size, in_stride_blocks=nb)
            a += size
        f.synchronize()
        recs.append(f.read_state()); rings.append(f.ring_state()); events.append(f.deliver())
        assert f.blocks() == nb
        f.close()
    ref = R.CwRef(n, ring=32)
    ref.set_speed(50)
    for c in range(n):
        ref.set_pitch_step(R.pitch_step(PITCHES[c % 6]), ch=c); ref.set_glitch(1 + c % 16, ch=c)
    ref.update(x)
    assert recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes() == ref.records().tobytes()
    assert all(np.array_equal(g[0], rings[0][0]) and np.array_equal(g[1], rings[0][1]) for g in rings)
    want = ref.collect(n * 32)
    assert events[0].tobytes() == events[1].tobytes() == events[2].tobytes() == want.tobytes() and len(want) > n


# ---- streams, setters between calls, and a channel moved mid-character
def test_streams_setters_between_calls_and_a_channel_moved_mid_character(gpu):
    """A call and a collect on a caller's stream; 260 blocks as 1 + 128 + 131 alternating between two streams with no host
    synchronisation in between; every setting and the speed changed between calls.  Then a channel mid-character moves to a slot
    of another handle through read_state / write_state: its next events are bit-identical to the uninterrupted ones."""
    import torch
    rng = np.random.default_rng(700)
    n = 37
    r = Rig(gpu, n)
    vary_settings(r)
    x = keyed_rows(rng, n, 460)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    r.call(x[:, :5], stream=streams[0])
    d_in = torch.from_numpy(x[:, 5:265].copy()).cuda()
    torch.cuda.synchronize()
    for k, (a, size) in enumerate(((0, 1), (1, 128), (129, 131))):
        r.dec.update_device(d_in[:, a:].data_ptr(), size, in_stride_blocks=260, stream=streams[k & 1].cuda_stream)
    r.dec.synchronize()
    r.ref.update(x[:, 5:265])
    r.check_state()
    assert np.array_equal(d_in.cpu().numpy(), x[:, 5:265])
    assert len(r.collect(n * 16, stream=streams[1])) >= n // 2
    r.both("set_glitch", 2, ch=2); r.both("set_min_power", 64); r.both("set_track", 0, ch=3); r.both("set_pitch_step", R.pitch_step(774), ch=0)
    r.both("set_speed", 45, ch=1); r.both("set_speed", 30, ch=n - 1)
    r.call(x[:, 265:280], stream=streams[1])
    r.both("set_speed", 55)
    r.check_state()
    r.call(x[:, 280:290], stream=streams[0])
    mid = [c for c in range(n) if int(r.ref.st["sym"][c]) > 1 and c % 5 != 4 and c != n - 1]
    assert mid
    c = mid[0]
    rec = r.dec.read_state()[c:c + 1]
    b = Rig(gpu, 19)
    step, power, glitch, track = r.dec.get_settings(c)
    b.both("set_pitch_step", step, ch=18); b.both("set_min_power", power, ch=18); b.both("set_glitch", glitch, ch=18); b.both("set_track", track, ch=18)
    b.put(rec, channels=[18])
    x2 = keyed_rows(rng, 19, 170)
    x2[18] = x[c, 290:]
    b.call(x2)
    r.call(x[:, 290:])
    moved = [e for e in b.collect(19 * 16) if e["channel"] == 18]
    stayed = [e for e in r.collect(n * 16) if e["channel"] == c]
    assert moved and len(moved) == len(stayed)
    for e, g in zip(moved, stayed):
        assert all(e[k] == g[k] for k in ("seq", "ch", "wpm", "sym", "flags")) and int(e["block"]) == int(g["block"]) - 290
    assert b.dec.read_state()[18].tobytes() == r.ref.records()[c].tobytes()
    for field, value, why in (("D", 440, "D must"), ("D", 5293, "D must"), ("key", 2, "key"), ("gap", 2, "gap"), ("cnt", 17, "cnt"),
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
    ev = torch.zeros(8 * 16, dtype=torch.uint8, device="cuda")
    i, o = d.data_ptr(), ev.data_ptr()
    for kw, why in ((dict(in_ptr=i + 2, n_blocks=1), "16-byte"), (dict(in_ptr=i, n_blocks=3, in_stride_blocks=2), "stride"),
                    (dict(in_ptr=i, n_blocks=65536, in_stride_blocks=65536), "n_blocks"), (dict(in_ptr=i, n_blocks=-1), "n_blocks"),
                    (dict(in_ptr=0, n_blocks=1), "null")):
        with pytest.raises(gpu.AsdrError, match=why):
            r.dec.update_device(**kw)
    for args, why in (((o + 2, o + 16, 4), "aligned"), ((o, o + 8, 4), "aligned"), ((0, o, 4), "null"), ((o, 0, 4), "null"),
                      ((o, o + 16, -1), "max_events"), ((o, o + 16, (1 << 26) + 1), "max_events")):
        with pytest.raises(gpu.AsdrError, match=why):
            r.dec.collect_device(*args)
    with pytest.raises(gpu.AsdrError, match="max_events"):
        r.dec.deliver(-1)
    for call in (lambda: r.dec.set_glitch(17), lambda: r.dec.set_track(2), lambda: r.dec.set_speed(61), lambda: r.dec.set_speed(20, ch=10)):
        with pytest.raises(gpu.AsdrError):
            call()
    r.check_state()
    assert not ev.cpu().numpy().any()
    r.close()


# ---- end to end
def test_the_chain_in_cw_mode_to_the_cw_decoder(gpu, ao):
    """The keyed carrier of tests/test_cw_ref.py's chain test (amplitude 3,000 at IF 7,164 Hz, 20 WPM, behind a VVV), shorter:
    AudioSDRBatch.update_device in CW_USBmode with the audioCW filter and the AGC, then CwDecoder.update_device and collect_device, on
    one stream with no host step in between.  The audio equals the oracle's, the events and the record equal those of the CPU run
    (the oracle's audio through cw_ref), and the text ends with the text that was sent."""
    import torch
    sent = "HOW VEXINGLY QUICK"
    I, Q = R.keyed_carrier_iq("VVV " + sent)
    nb = I.shape[0]
    o = ao.OracleSDR()
    o.setDemodMode(ao.CW_USBmode); o.setAudioFilter(ao.audioCW); o.enableAudioFilter()
    audio = o.update(I, Q).reshape(1, nb, 128)
    ref = R.CwRef(1, ring=64)
    ref.update(audio)
    want = ref.collect(64)
    assert R.text_of(want).rstrip(" ").endswith(" " + sent)
    sdr, dec = gpu.AudioSDRBatch(1), gpu.CwDecoder(1, ring=64)
    sdr.setDemodMode(gpu.CW_USBmode); sdr.setAudioFilter(gpu.audioCW); sdr.enableAudioFilter()
    s = torch.cuda.Stream()
    dI, dQ = torch.from_numpy(I[None].copy()).cuda(), torch.from_numpy(Q[None].copy()).cuda()
    d_audio = torch.zeros((1, nb, 128), dtype=torch.int16, device="cuda")
    d_events = torch.full((65 * 16,), PATTERN, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sdr.update_device(dI.data_ptr(), dQ.data_ptr(), d_audio.data_ptr(), nb, stream=s.cuda_stream)
    dec.update_device(d_audio.data_ptr(), nb, stream=s.cuda_stream)
    dec.collect_device(d_count.data_ptr(), d_events.data_ptr(), 64, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_audio.cpu().numpy(), audio)
    assert dec.read_state().tobytes() == ref.records().tobytes()
    got = d_events.cpu().numpy()
    assert int(d_count.cpu()[0]) == len(want) and got[:len(want) * 16].tobytes() == want.tobytes() and (got[len(want) * 16:] == PATTERN).all()
    assert gpu.CwDecoder.text(got[:len(want) * 16].view(gpu.CW_EVENT_DTYPE), channel=0).rstrip(" ").endswith(" " + sent)
    sdr.close(); dec.close()
