"""The DCS squelch on the GPU (include/asdr_dcs.h; audiosdr_amd/csrc/asdr_dcs.hip) against tests/dcs_ref.py at tolerance 0: every
byte of the output buffer (a guard pattern fills the stride gaps and a row behind the last), the input left as it was, every state
field, the records' bytes and blocks(), over partial workgroups of both instantiations, calls that hold no bit, one bit and a word's
end, strides, every phase of the bit clock, the arithmetic's extremes, tables and setters between calls, streams, the state calls, a
sequence split in two ways, and end to end behind the FM demodulator and in front of a tone squelch and a gate.
The sizes are the smallest that reach each seam: a workgroup holds gpu.DCS_NARROW_ROWS = 16 channels in a bank below
gpu.DCS_WIDE_CHANNELS = 32768 channels and gpu.DCS_ROWS = 64 from there on (a lane of its first wave each in the sequential part)."""
import numpy as np
import pytest

import dcs_ref as DR
import fm_ref as FR
import gate_ref as GR
import tone_ref as TR

pytestmark = pytest.mark.gpu
GAP = 0x7FFF        # fills the input strides' gaps: must not be read
PATTERN = 0x5A5B    # pre-fills the output buffer: must stay wherever nothing is written


class Rig:
    """A DCS squelch and its reference side by side; call() runs one update on both and compares everything."""

    def __init__(self, A, n):
        import torch
        self.torch, self.A, self.n = torch, A, n
        self.sq, self.ref = A.DcsSquelch(n), DR.DcsRef(n)

    def both(self, method, *args, **kw):
        getattr(self.sq, method)(*args, **kw)
        getattr(self.ref, method)(*args, **kw)

    def put(self, rec, channels=None):
        """Records into both sides."""
        self.sq.write_state(rec, channels=channels)
        for k, c in enumerate(range(len(rec)) if channels is None else channels):
            self.ref.put(c, rec[k])

    def call(self, x, extra_in=0, extra_out=0, stream=None):
        """x int16 [n][nb][128].  Returns the reference's (out, unmuted)."""
        torch = self.torch
        n, nb = x.shape[:2]
        px = np.full((n, nb + extra_in, 128), GAP, dtype=np.int16)
        px[:, :nb] = x
        d_in = torch.from_numpy(px).cuda()
        d_out = torch.full((n * (nb + extra_out) + 1, 128), PATTERN, dtype=torch.int16, device="cuda")   # one guard row behind
        torch.cuda.synchronize()
        self.sq.update_device(d_in.data_ptr(), d_out.data_ptr(), nb, in_stride_blocks=nb + extra_in, out_stride_blocks=nb + extra_out,
                              stream=stream.cuda_stream if stream is not None else 0)
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        out, unmuted = self.ref.update(x)
        expect = np.full((n, nb + extra_out, 128), PATTERN, dtype=np.int16)
        expect[:, :nb] = out
        got = d_out.cpu().numpy()
        bad = np.argwhere(got[:-1].reshape(expect.shape) != expect)
        assert bad.size == 0, (len(bad), bad[0].tolist())
        assert (got[-1] == PATTERN).all(), "written behind the last row"
        assert np.array_equal(d_in.cpu().numpy(), px)
        self.check_state()
        return out, unmuted

    def check_state(self):
        got, want = self.sq.read_state(), self.ref.records()
        for k in DR.STATE_NAMES:
            bad = [c for c in range(self.n) if not np.array_equal(got[k][c], want[k][c])]
            assert not bad, (k, len(bad), bad[0], got[k][bad[0]].tolist(), want[k][bad[0]].tolist())
        assert got.tobytes() == want.tobytes()
        assert self.sq.blocks() == self.ref.blocks

    def close(self):
        self.sq.close()


def words_in_noise(rng, n, nb, words, amplitude=2000.0, sigma=400.0, stop=None):
    """int16 [n][nb][128]: channel c carries words[c % len(words)] in white noise, up to block `stop` if given; every fifth channel
    noise alone.  A word's first bit is 18 to 23 bits away, so that the register, which is compared with a word in one rotation only,
    holds it some 28 bits in and again 23 bits later."""
    x = rng.normal(0.0, sigma, size=(n, nb * 128))
    m = nb * 128 if stop is None else stop * 128
    for c in range(n):
        if c % 5 != 4:
            x[c, :m] += DR.dcs_wave(m, words[c % len(words)], amplitude, start_bit=18.0 + c % 5 + 0.13 * (c % 7))
    return DR.to_int16(x).reshape(n, nb, 128)


def vary_settings(r, n_codes):
    """Every channel different, inside one wave too: PASS, ANY, the channel's own code, another code; hysteresis 0 or a level."""
    for c in range(r.n):
        r.both("set_want", (DR.PASS, DR.ANY, c % n_codes, (c + 3) % n_codes)[c % 4], ch=c)
        r.both("set_hysteresis", (0, 3000, 12000)[c % 3], ch=c)


# ---- partial workgroups of the narrow form; calls with no bit, one bit and a word's end; strides
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_channels_calls_and_strides(gpu, n):
    """One less, equal and one more than a workgroup's 16 channels; 33: three workgroups, the last with one channel.  The word is
    there for 150 blocks (58 bits: lock and two words) and gone for 80, in which a hold of 23 bits runs out.  Calls of 1, 2, 3, 59,
    60 and 105 blocks: a bit takes 2.56 blocks, so the first holds no bit or one, the fourth and fifth a word's end, the last more.
    Strides larger than n_blocks on both sides; a call of 0 blocks does nothing."""
    assert gpu.DCS_NARROW_ROWS == 16 and n < gpu.DCS_WIDE_CHANNELS
    rng = np.random.default_rng(100 + n)
    r = Rig(gpu, n)
    r.both("set_hold_bits", 23)
    vary_settings(r, 8)
    x = words_in_noise(rng, n, 230, r.ref.words[:8], stop=150)
    seen, a = [], 0
    for nb, ein, eout in ((1, 0, 0), (2, 3, 1), (3, 1, 2), (59, 0, 3), (60, 2, 0), (105, 0, 0)):
        seen.append(r.call(x[:, a:a + nb], extra_in=ein, extra_out=eout)[1])
        a += nb
    unmuted = np.concatenate(seen, axis=1)
    st = r.ref.st
    assert (st["bits"] >= 85).all() and (st["bits"] <= 92).all()         # 230 blocks are 89.7 bits; edges in noise move the clock
    if n >= 15:
        carried = np.array([c % 5 != 4 for c in range(n)])
        assert (st["detections"][carried] == 1).all() and not st["detections"][~carried].any()       # every carried code was named ...
        assert (st["detected"] == -1).all()                                                            # ... and every hold ran out
        wanted = carried & (np.arange(n) % 4 != 3)
        assert (st["openings"][wanted] == 1).all()
        opened = unmuted[wanted & (np.arange(n) % 4 != 0)]                                             # ANY and the own code: open and close again
        assert opened.size and (opened[:, :60] == 0).all() and opened.any(axis=1).all() and (opened[:, -1] == 0).all()
        assert not unmuted[np.arange(n) % 4 == 3].any() and unmuted[np.arange(n) % 4 == 0].all()       # another code: muted; PASS: never
    d = r.torch.zeros((2, n, 2, 128), dtype=r.torch.int16, device="cuda")
    r.sq.update_device(d[0].data_ptr(), d[1].data_ptr(), 0, in_stride_blocks=2, out_stride_blocks=2)   # nothing happens
    r.check_state()
    r.close()


# ---- banks of DCS_WIDE_CHANNELS channels and more: 64 channels per workgroup
PERIOD = 1021       # a prime: every workgroup sees another alignment of the repeated rows and settings


@pytest.fixture(scope="module")
def wide_reference():
    """The reference of 1021 channels, once: 140 blocks of words in noise on the reference alone (the codes are named, channels are
    open), its records then, and after a call of 1 block and one of 3 blocks (out, records).  Different settings per channel."""
    rng = np.random.default_rng(38)
    ref = DR.DcsRef(PERIOD)
    ref.set_hold_bits(23)
    sets = [((DR.PASS, DR.ANY, c % 104, (c + 3) % 104)[c % 4], (0, 3000, 12000)[c % 3]) for c in range(PERIOD)]
    for c, (w, h) in enumerate(sets):
        ref.set_want(w, ch=c); ref.set_hysteresis(h, ch=c)
    x = words_in_noise(rng, PERIOD, 144, ref.words)
    ref.update(x[:, :140])
    start = ref.records()
    assert (ref.st["detected"] >= 0).sum() > PERIOD // 2 and 0 < ref.st["open"].sum() < PERIOD
    steps = []
    for a, b in ((140, 141), (141, 144)):
        out, unmuted = ref.update(x[:, a:b])
        assert 0 < unmuted.sum() < unmuted.size
        steps.append((out, ref.records()))
    assert len(set(ref.st["clk"].tolist())) > 100 and ref.st["bits"].max() > ref.st["bits"].min()
    return x[:, 140:], sets, start, steps


@pytest.mark.parametrize("n", [32767, 32768, 32769, 32768 + 63, 32768 + 65, 32768 + 129])
def test_wide_banks(gpu, wide_reference, n):
    """Either side of the size at which a workgroup takes 64 channels (DCS_ROWS), and last workgroups of one less than, equal to
    and one more than 64 channels (1 channel after full ones: 32769 and 32768 + 65; 63: 32768 + 63; the full 64: 32768) and one
    more than two workgroups behind the switch: channels in lock written through write_state, a one-block call, then three blocks
    with strides larger than n_blocks, against the repeated reference; every output byte, the guard row and every record."""
    import torch
    assert gpu.DCS_WIDE_CHANNELS == 32768 and gpu.DCS_ROWS == 64
    x, sets, start, steps = wide_reference
    sel = np.arange(n) % PERIOD
    f = gpu.DcsSquelch(n)
    L, h = f._L, f._h
    for c in range(n):
        w, hy = sets[c % PERIOD]
        assert L.asdr_dcs_set_want(h, c, w) == 0 and L.asdr_dcs_set_hysteresis(h, c, hy) == 0
    f.set_hold_bits(23)
    f.write_state(start[sel])
    for (a, b, ein, eout), (out, rec) in zip(((0, 1, 0, 0), (1, 4, 1, 2)), steps):
        nb = b - a
        px = np.full((n, nb + ein, 128), GAP, dtype=np.int16)
        px[:, :nb] = x[sel, a:b]
        d_in = torch.from_numpy(px).cuda()
        d_out = torch.full((n * (nb + eout) + 1, 128), PATTERN, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        f.update_device(d_in.data_ptr(), d_out.data_ptr(), nb, in_stride_blocks=nb + ein, out_stride_blocks=nb + eout)
        f.synchronize()
        got = d_out.cpu().numpy()
        assert (got[-1] == PATTERN).all(), "written behind the last row"
        got = got[:-1].reshape(n, nb + eout, 128)
        assert np.array_equal(got[:, :nb], out[sel]) and (got[:, nb:] == PATTERN).all()
        assert f.read_state().tobytes() == rec[sel].tobytes()
    assert f.blocks() == 4
    f.close()


# ---- every clock phase
def test_every_clock_phase_with_an_edge_at_every_position(gpu):
    """Channels written through write_state: clk at 0, 1, 127, 1183, 1184, 1311, 1312, 1313, 1440, 2496, 2497 and 2624 (each side of
    the bit's middle, of the step that reaches it and of the wrap), b both ways, and a dhist that puts the slicer's edge at each of
    a block's 8 positions or nowhere while the block itself is zeros (s_k is then the sum of dhist from 5 + k on).  One block, then
    two of noise."""
    clks = (0, 1, 127, 1183, 1184, 1311, 1312, 1313, 1440, 2496, 2497, 2624)
    cases = [(clk, b, k) for clk in clks for b in (0, 1) for k in range(9)]
    n = len(cases)
    r = Rig(gpu, n)
    r.both("set_confirm", 1)
    r.both("set_want", DR.ANY)
    rec = r.sq.read_state()
    for c, (clk, b, k) in enumerate(cases):
        sign = 1 if b else -1                                   # s starts on b's side and crosses to the other at position k
        rec["dhist"][c, 23] = -100 * sign
        if 1 <= k <= 7:
            rec["dhist"][c, 4 + k] = 1000 * sign
        if k == 8:                                              # no edge: s stays on b's side
            rec["dhist"][c, 23] = 100 * sign
        rec["clk"][c], rec["b"][c] = clk, b
        rec["sr"][c] = (r.ref.words[c % 104] << 1) & 0x7FFFFF | (r.ref.words[c % 104] >> 22)   # one bit before the word
    r.put(rec)
    r.call(np.zeros((n, 1, 128), dtype=np.int16))
    st = r.ref.st
    edges = st["edges"].reshape(len(clks), 2, 9)
    assert (edges[:, :, :8] == 1).all() and not edges[:, :, 8].any()
    took = st["bits"].reshape(len(clks), 2, 9)
    assert took.max() == 1 and took.min() == 0 and took[clks.index(1311)].all() and not took[clks.index(1312)].any()
    assert 0 < st["hits"].sum() < st["bits"].sum()                 # the bit that completes the word, and the one that does not
    x = DR.to_int16(np.random.default_rng(5).normal(0.0, 3000.0, size=(n, 2 * 128))).reshape(n, 2, 128)
    r.call(x, extra_in=1, extra_out=1)
    r.close()


# ---- extremes
@pytest.mark.parametrize("hold_bits,confirm,max_errors,n_codes", [(23, 1, 3, 1), (1023, 8, 0, 128), (23, 2, 3, 128)])
def test_extremes(gpu, hold_bits, confirm, max_errors, n_codes):
    """Constant -32768 and +32767, a full-scale square wave at the bit rate and at twice it, and full-scale words; hysteresis 0 and
    above 20 * 32768 (b never moves); the ends of hold_bits, confirm and max_errors; tables of 1 and of 128 words.  Then rows of
    zeros: bits are still taken from the held b, so quiet runs on and a hold of 23 bits runs out; what the restatement gives."""
    n, nb = 12, 150
    table = ([c for c in range(512) if DR.find([DR.word(k) for k in DR.CODES], c) < 0][:24] + list(DR.CODES))[:n_codes]
    if n_codes == 1:
        table = [0o023]
    r = Rig(gpu, n)
    r.both("set_codes", table); r.both("set_max_errors", max_errors); r.both("set_confirm", confirm); r.both("set_hold_bits", hold_bits)
    r.both("set_want", DR.ANY)
    k = np.arange(nb * 128)
    x = np.zeros((n, nb * 128))
    x[0], x[1] = -32768, 32767
    x[2] = np.where(np.floor(k * DR.BIT_RATE / DR.FS) % 2 == 0, 32767, -32768)
    x[3] = np.where(np.floor(k * 2 * DR.BIT_RATE / DR.FS) % 2 == 0, 32767, -32768)
    for c in range(4, n):
        x[c] = DR.dcs_wave(nb * 128, r.ref.words[0], 40000.0, start_bit=18.0 + c % 4, lowpass_hz=0.0 if c % 2 else 300.0)   # clipped at full scale
    for c in (5, 8):
        r.both("set_hysteresis", 20 * 32768 + 1, ch=c)
    r.both("set_hysteresis", 2**32 - 1, ch=9)
    r.both("set_hysteresis", 20 * 32768 - 1, ch=10)
    x = DR.to_int16(x).reshape(n, nb, 128)
    r.call(x[:, :70])
    r.call(x[:, 70:], extra_in=1)
    st = r.ref.st
    assert int(np.abs(r.ref.records()["dhist"]).max()) >= 32767
    assert not st["edges"][[5, 8, 9]].any() and st["edges"][[4, 6, 7]].all() and (st["bits"] > 50).all()
    named = st["detected"][[4, 6, 7, 11]]
    assert (named == 0).all() if confirm < 8 else (named == -1).all()                 # 150 blocks are 58 bits: two words, not eight
    _, unmuted = r.call(np.zeros((n, 75, 128), dtype=np.int16), extra_out=1)         # 29 bits of the held b
    assert (st["quiet"][[4, 6, 7, 11]] > 23).all() and (st["bits"] > 79).all()
    if confirm < 8:
        assert (st["detected"][[4, 6, 7, 11]] == (-1 if hold_bits == 23 else 0)).all()
        assert unmuted[4, 0] == 1 and unmuted[4, -1] == (0 if hold_bits == 23 else 1)
    r.close()


# ---- tables and setters between calls
def test_tables_and_setters_between_calls(gpu):
    """set_codes restores sr, cand, age, run, detected and quiet and keeps open and the counters; want changed on an open channel
    acts at the next bit, and the rows from the block after it."""
    rng = np.random.default_rng(300)
    n = 10
    r = Rig(gpu, n)
    r.both("set_want", DR.ANY)
    x = words_in_noise(rng, n, 140, r.ref.words[:8])
    r.call(x)
    st = r.ref.st
    carried = np.array([c % 5 != 4 for c in range(n)])
    assert (st["detected"][carried] >= 0).all() and (st["open"][carried] == 1).all()
    counters = {k: st[k].copy() for k in DR.COUNTERS}
    r.both("set_codes", list(DR.CODES[:8])[::-1])                       # the same words under other indices
    r.check_state()
    got = r.sq.read_state()
    assert (got["detected"] == -1).all() and (got["cand"] == -1).all() and (got["age"] == 255).all() and not got["sr"].any()
    assert (got["open"][carried] == 1).all() and all(np.array_equal(got[k], counters[k]) for k in DR.COUNTERS)
    r.both("set_want", 7 - 1, ch=1)                                     # channel 1 carries word 1, now entry 6 ...
    r.both("set_want", 1, ch=2)                                         # ... and channel 2 wants an entry it does not carry
    y = words_in_noise(rng, n, 140, r.ref.words[::-1])                  # the words again, from their starts
    bits = st["bits"].copy()
    first = r.call(y[:, :3])[1]                                         # open stands until a bit is taken, 2.56 blocks at the most ...
    assert (st["bits"] > bits).all()
    later = r.call(y[:, 3:], extra_in=2, extra_out=1)[1]                # ... then no code is named for two words
    assert first[:, 0].tolist() == carried.tolist() and not later[2].any() and not later[1, :100].any() and later[1, -1] == 1
    assert st["detected"][1] == 6 and st["detected"][2] == 5 and st["open"].tolist() == [1, 1, 0, 1, 0, 1, 1, 1, 1, 0]
    r.both("set_max_errors", 2); r.both("set_confirm", 1); r.both("set_hysteresis", 5000, ch=3); r.both("set_hold_bits", 30)
    r.call(x[:, :40])
    r.close()


# ---- streams and the state calls
def test_calls_on_the_callers_streams_and_the_state_calls(gpu):
    """A call on a caller's stream, then 130 blocks as 1 + 64 + 65 alternating between two streams with no host synchronisation
    in between: outputs and state equal the reference's.  Then a channel in lock moves to another handle; clear and reset."""
    import torch
    rng = np.random.default_rng(700)
    n = 37
    r = Rig(gpu, n)
    vary_settings(r, 104)
    x = words_in_noise(rng, n, 175, r.ref.words)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    r.call(x[:, :5], stream=streams[0])
    d_in = torch.from_numpy(x[:, 5:135].copy()).cuda()
    d_out = torch.full((n, 130, 128), PATTERN, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for k, (a, size) in enumerate(((0, 1), (1, 64), (65, 65))):
        r.sq.update_device(d_in[:, a:].data_ptr(), d_out[:, a:].data_ptr(), size, in_stride_blocks=130, out_stride_blocks=130,
                           stream=streams[k & 1].cuda_stream)
    r.sq.synchronize()
    torch.cuda.synchronize()
    out, _ = r.ref.update(x[:, 5:135])
    assert np.array_equal(d_out.cpu().numpy(), out)
    r.check_state()
    rec = r.sq.read_state()[2:3]                                   # channel 2 wants its own code and hears it
    assert int(rec["open"][0]) == 1 and int(rec["detected"][0]) == 2 and rec["dhist"].any() and rec["hist"].any()
    b = Rig(gpu, 19)
    b.both("set_want", 2, ch=18); b.both("set_hysteresis", 12000, ch=18)       # channel 2's settings
    b.put(rec, channels=[18])
    x2 = words_in_noise(rng, 19, 40, b.ref.words)
    x2[18] = x[2, 135:]
    got = b.call(x2)[0]
    want = r.ref.update(x[:, 135:])[0]                              # the uninterrupted reference
    assert np.array_equal(got[18], want[2]) and want[2].any()
    assert b.sq.read_state()[18].tobytes() == r.ref.records()[2].tobytes()
    for field, value, why in (("open", 2, "open must be 0 or 1"), ("clk", 2625, "clk"), ("sr", 1 << 23, "sr"), ("detected", 104, "detected"),
                              ("cand", -2, "cand"), ("b", 2, "b must"), ("reserved", 1, "reserved")):
        bad = rec.copy(); bad[field] = value
        with pytest.raises(gpu.AsdrError, match=why):
            b.sq.write_state(bad, channels=[0])
    b.check_state()
    b.both("clear")
    b.check_state()
    b.call(x2[:, :3], stream=streams[1])
    b.both("reset")
    b.check_state()
    assert b.sq.read_state().tobytes() == DR.DcsRef(19).records().tobytes()
    b.call(x2[:, :2])
    r.close(); b.close()


# ---- split invariance
def test_one_sequence_as_one_call_and_as_many(gpu):
    import torch
    rng = np.random.default_rng(800)
    n, nb = 21, 190
    x = words_in_noise(rng, n, nb, [DR.word(c) for c in DR.CODES], stop=140)
    d_in = torch.from_numpy(x).cuda()
    outs, recs = [], []
    for sizes in ((nb,), (1, 2, 3, 5, 8, 13, 21, 34, 53, 50), tuple([1] * 20 + [170])):
        assert sum(sizes) == nb
        f = gpu.DcsSquelch(n)
        f.set_hold_bits(23)
        for c in range(n):
            f.set_want((DR.PASS, DR.ANY, c % 104, (c + 3) % 104)[c % 4], ch=c)
        d_out = torch.full((n, nb, 128), PATTERN, dtype=torch.int16, device="cuda")
        a = 0
        for size in sizes:
            f.update_device(d_in[:, a:].data_ptr(), d_out[:, a:].data_ptr(), size, in_stride_blocks=nb, out_stride_blocks=nb)
            a += size
        f.synchronize()
        outs.append(d_out.cpu().numpy()); recs.append(f.read_state())
        assert f.blocks() == nb
        f.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes()
    assert recs[0]["detections"].sum() > n // 2 and 0 < (outs[0] != 0).any(axis=2).sum() < n * nb


def test_update_device_refusals_change_nothing(gpu):
    import torch
    r = Rig(gpu, 10)
    d = torch.zeros((2, 10, 4, 128), dtype=torch.int16, device="cuda")
    i, o = d[0].data_ptr(), d[1].data_ptr()
    for kw, why in ((dict(in_ptr=i + 2, out_ptr=o, n_blocks=1), "16-byte"), (dict(in_ptr=i, out_ptr=o + 8, n_blocks=1), "16-byte"),
                    (dict(in_ptr=i, out_ptr=o, n_blocks=3, in_stride_blocks=2), "stride"),
                    (dict(in_ptr=i, out_ptr=o, n_blocks=3, out_stride_blocks=2), "stride"),
                    (dict(in_ptr=i, out_ptr=o, n_blocks=65536, in_stride_blocks=65536, out_stride_blocks=65536), "n_blocks"),
                    (dict(in_ptr=i, out_ptr=o, n_blocks=-1), "n_blocks"),
                    (dict(in_ptr=0, out_ptr=o, n_blocks=1), "null"), (dict(in_ptr=i, out_ptr=0, n_blocks=1), "null"),
                    (dict(in_ptr=i, out_ptr=i + 256, n_blocks=2, in_stride_blocks=4, out_stride_blocks=4), "overlaps"),
                    (dict(in_ptr=i, out_ptr=i, n_blocks=4), "overlaps")):
        with pytest.raises(gpu.AsdrError, match=why):
            r.sq.update_device(**kw)
    r.check_state()
    r.close()


# ---- end to end
def fm_carrier(modulation, amplitude=8000.0, deviation_hz=5000.0):
    """int16 (I, Q) of an FM carrier at baseband whose instantaneous frequency is deviation_hz * modulation."""
    phi = 2.0 * np.pi * deviation_hz / 44100.0 * np.cumsum(modulation)
    return DR.to_int16(amplitude * np.cos(phi)), DR.to_int16(amplitude * np.sin(phi))


def test_fm_to_dcs_squelch_to_tone_highpass_to_gate(gpu):
    """Three FM channels whose modulation is a 1 kHz tone (0.2 of the deviation) over, at a tenth of the deviation, code 023, code
    023 again, or nothing.  FM demodulator (hp_shift 12: the code reaches the audio rows), DCS squelch (channel 0 wants 023, channel
    1 wants 025, channel 2 any), tone squelch (want = PASS, the three-section 300 Hz high-pass, which takes the code out of the
    audio) and gate (open_energy 1) run on one stream with no host step in between, as two calls of 100 blocks.  Expectations come
    from fm_ref -> dcs_ref -> tone_ref -> gate_ref; on the reference itself: the first call delivers nothing, the second only
    channel 0, and the named codes are 023, 023 and none."""
    import torch
    n, nb = 3, 200
    m = np.tile(0.2 * TR.tone_wave(nb * 128, 1000.0, 1.0), (n, 1))
    for c in (0, 1):
        m[c] += DR.dcs_wave(nb * 128, DR.word(0o023), 0.1, start_bit=5.0 * c)
    I, Q = (np.stack(v).reshape(n, nb, 128) for v in zip(*[fm_carrier(m[c]) for c in range(n)]))
    fm, dcs, sq, gate = gpu.FmDemodulator(n), gpu.DcsSquelch(n), gpu.ToneSquelch(n), gpu.AudioGate(n)
    fref, dref, tref, gref = FR.FmRef(n), DR.DcsRef(n), TR.ToneRef(n), GR.GateRef(n)
    fm.set_dc_shift(12); fref.set_dc_shift(12)
    own, other = dcs.find(0o023), dcs.find(0o025)
    assert (own, other) == (dref.find(0o023), dref.find(0o025)) == (0, 1)
    for c, w in enumerate((own, other, gpu.DCS_ANY)):
        dcs.set_want(w, ch=c); dref.set_want(w, ch=c)
    sq.set_highpass(fc_hz=300.0, sections=3); tref.set_highpass(TR.highpass_design(300.0, 3))
    gate.set_squelch(energies=(1, 1), hang_blocks=0); gref.set_squelch(1, 1, 0)
    s = torch.cuda.Stream()
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    d_v, d_w, d_y = (torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda") for _ in range(3))
    d_rows = torch.full((2, n, 100, 128), PATTERN, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    counts, indices = [], []
    for k, a in enumerate((0, 100)):
        fm.update_device(dI[:, a:].data_ptr(), dQ[:, a:].data_ptr(), d_v[:, a:].data_ptr(), 100, in_stride_blocks=nb, out_stride_blocks=nb,
                         stream=s.cuda_stream)
        dcs.update_device(d_v[:, a:].data_ptr(), d_w[:, a:].data_ptr(), 100, in_stride_blocks=nb, out_stride_blocks=nb, stream=s.cuda_stream)
        sq.update_device(d_w[:, a:].data_ptr(), d_y[:, a:].data_ptr(), 100, in_stride_blocks=nb, out_stride_blocks=nb, stream=s.cuda_stream)
        gate.update_device(d_y[:, a:].data_ptr(), 100, stride_blocks=nb, rows_ptr=d_rows[k].data_ptr(), capacity_rows=n, stream=s.cuda_stream)
        s.synchronize()
        counts.append(int(gate.count_tensor().cpu()[0]))
        indices.append(gate.index_tensor().cpu().numpy()[:counts[-1]].tolist())
    v = fref.update(I, Q)[0]
    assert np.array_equal(d_v.cpu().numpy(), v)
    w1, w2 = dref.update(v[:, :100])[0], dref.update(v[:, 100:])[0]
    assert np.array_equal(d_w.cpu().numpy(), np.concatenate([w1, w2], axis=1))
    assert dcs.read_state().tobytes() == dref.records().tobytes()
    y1, y2 = tref.update(w1)[0], tref.update(w2)[0]
    assert np.array_equal(d_y.cpu().numpy(), np.concatenate([y1, y2], axis=1))
    assert sq.read_state().tobytes() == tref.records().tobytes()
    i1, rows1, _ = gref.update(y1)
    i2, rows2, _ = gref.update(y2)
    assert i1.tolist() == [] and i2.tolist() == [0] and not y1.any() and y2[0].any() and not y2[1:].any()
    assert dref.st["detected"].tolist() == [own, own, -1] and dcs.decoded_codes().tolist() == [0o023, 0o023, -1]
    assert counts == [0, 1] and indices == [[], [0]]
    assert np.array_equal(d_rows[1].cpu().numpy().reshape(-1, 128)[:100], rows2[0]) and (d_rows[0].cpu().numpy() == PATTERN).all()
    # the code is gone from the delivered audio and the voice-band tone is there: the delivered rows' spectrum at 1 kHz and below 300 Hz
    open_from = int(np.flatnonzero(w2[0].any(axis=1))[0]) + 30
    spec_v, spec_y = (np.abs(np.fft.rfft(z[0, 100 + open_from:].reshape(-1).astype(np.float64))) for z in (v, np.concatenate([y1, y2], axis=1)))
    f = np.fft.rfftfreq((100 - open_from) * 128, 1.0 / 44100.0)
    low, tone = (f > 20.0) & (f < 200.0), np.abs(f - 1000.0) < 30.0
    assert spec_y[tone].max() > 0.8 * spec_v[tone].max() and spec_y[low].max() < spec_v[low].max() / 30.0
    fm.close(); dcs.close(); sq.close(); gate.close()
