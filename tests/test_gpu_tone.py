"""The tone squelch on the GPU (include/asdr_tone.h; audiosdr_amd/csrc/asdr_tone.hip) against tests/tone_ref.py at tolerance 0: every
byte of the output buffer (a guard pattern fills the stride gaps and a row behind the last) and every state field, over partial waves
and workgroups, calls in which a window ends at the end, inside and twice, strides, tables and windows, the arithmetic's extremes,
per-channel settings, muting, streams, the state calls, and end to end behind the FM demodulator and in front of a gate.
The sizes are the smallest that reach each seam: a workgroup holds gpu.TONE_ROWS = 16 channels (a lane of its first wave each in the
recurrence) and a wave correlates gpu.TONE_WAVE_ROWS = 4 of them; there is one instantiation of the kernel."""
import numpy as np
import pytest

import fm_ref as FR
import gate_ref as GR
import tone_ref as TR

pytestmark = pytest.mark.gpu
GAP = 0x7FFF        # fills the input strides' gaps: must not be read
PATTERN = 0x5A5B    # pre-fills the output buffer: must stay wherever nothing is written
TABLE8 = [70.0 + 30.0 * k for k in range(8)]   # a window of 16 blocks (46 ms) resolves 21.5 Hz: these tones are told apart in it


class Rig:
    """A tone squelch and its reference side by side; call() runs one update on both and compares everything."""

    def __init__(self, A, n):
        import torch
        self.torch, self.A, self.n = torch, A, n
        self.sq, self.ref = A.ToneSquelch(n), TR.ToneRef(n)

    def both(self, method, *args, **kw):
        getattr(self.sq, method)(*args, **kw)
        getattr(self.ref, method)(*args, **kw)

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
        for k in TR.STATE_NAMES:
            bad = [c for c in range(self.n) if not np.array_equal(got[k][c], want[k][c])]
            assert not bad, (k, len(bad), bad[0], got[k][bad[0]].tolist(), want[k][bad[0]].tolist())
        assert got.tobytes() == want.tobytes()
        assert self.sq.blocks() == self.ref.blocks

    def close(self):
        self.sq.close()


def tones_in_noise(rng, n, nb, table, amplitude=3000.0, sigma=2000.0, first=0):
    """int16 [n][nb][128]: channel c carries table[c % len(table)] in white noise; every fifth channel noise alone."""
    x = rng.normal(0.0, sigma, size=(n, nb * 128))
    for c in range(n):
        if c % 5 != 4:
            x[c] += TR.tone_wave(nb * 128, table[c % len(table)], amplitude, phase=float(c), first=128 * first)
    return TR.to_int16(x).reshape(n, nb, 128)


def vary_settings(r, n_tones):
    """Every channel different, inside one wave too: PASS, ANY, the channel's own tone, another tone; min_power 0 or a level; hang
    0, 1, 2."""
    for c in range(r.n):
        r.both("set_want", (TR.PASS, TR.ANY, c % n_tones, (c + 3) % n_tones)[c % 4], ch=c)
        r.both("set_min_power", (0, TR.min_power(1000, 16), TR.min_power(30000, 16))[c % 3], ch=c)
        r.both("set_hang", (0, 1, 2, 0, 1)[c % 5], ch=c)


# ---- partial waves and workgroups, windows ending at a call's end, inside a call and twice in a call, strides
@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 33])
def test_channels_calls_and_strides(gpu, n):
    """One less, equal and one more than a wave's 4 channels and a workgroup's 16; 33: three workgroups, the last with one channel.
    W = 16 and calls of 16, 1, 2, 15, 17 and 33 blocks: the window ends at the first call's end, inside the fourth and the fifth,
    and twice in the sixth.  Strides larger than n_blocks on both sides; a call of 0 blocks does nothing."""
    assert gpu.TONE_ROWS == 16 and gpu.TONE_WAVE_ROWS == 4
    rng = np.random.default_rng(100 + n)
    r = Rig(gpu, n)
    r.both("set_tones", TABLE8); r.both("set_window", 16); r.both("set_highpass", TR.highpass_design(300.0, 1))
    vary_settings(r, 8)
    x = tones_in_noise(rng, n, 84, TABLE8)
    seen, a = [], 0
    for nb, ein, eout in ((16, 0, 0), (1, 0, 0), (2, 3, 1), (15, 1, 2), (17, 0, 3), (33, 2, 0)):
        seen.append(r.call(x[:, a:a + nb], extra_in=ein, extra_out=eout)[1])
        a += nb
    unmuted = np.concatenate(seen, axis=1)
    assert (r.ref.st["windows"] == 5).all() and (r.ref.st["window_block"] == 4).all()
    if n >= 15:
        assert 0 < unmuted.sum() < unmuted.size and (r.ref.st["detected"] >= 0).sum() > n // 2 and (r.ref.st["detected"] < 0).any()
    d = r.torch.zeros((2, n, 2, 128), dtype=r.torch.int16, device="cuda")
    r.sq.update_device(d[0].data_ptr(), d[1].data_ptr(), 0, in_stride_blocks=2, out_stride_blocks=2)   # nothing happens
    r.check_state()
    r.close()


# ---- tables and windows
@pytest.mark.parametrize("n_tones,W", [(1, 16), (2, 16), (50, 128), (64, 16), (64, 128)])
def test_tables_and_windows(gpu, n_tones, W):
    """Tables of 1, 2, 50 (the creation table) and 64 tones, windows of 16 and 128 blocks; the calls end a window inside the second.
    Tones of a 64-entry table that the window resolves are decoded; the slots from n_tones on stay zero."""
    rng = np.random.default_rng(200 + n_tones + W)
    n = 6
    table = {1: [123.0], 2: [100.0, 1377.9], 50: list(TR.CTCSS), 64: [60.0 + 20.0 * k for k in range(64)]}[n_tones]
    r = Rig(gpu, n)
    if n_tones != 50:
        r.both("set_tones", table)
    r.both("set_window", W); r.both("set_want", TR.ANY); r.both("set_min_power", TR.min_power(1000, W))
    x = tones_in_noise(rng, n, W + 8, [table[(11 * c) % n_tones] for c in range(n)])
    r.call(x[:, :W - 3], extra_in=1)
    _, unmuted = r.call(x[:, W - 3:], extra_out=1)
    det = r.ref.st["detected"].tolist()
    assert det == [(11 * c) % n_tones if c != 4 else -1 for c in range(n)]            # channel 4 is noise alone
    assert unmuted[:, :3].sum() == 0 and unmuted[:, 3:].all(axis=1).tolist() == [c != 4 for c in range(n)]
    assert not r.sq.read_state()["acc"][:, n_tones:].any()
    assert np.array_equal(r.sq.decoded_hz(), r.ref.decoded_hz(), equal_nan=True)
    r.close()


# ---- sections and per-channel settings
@pytest.mark.parametrize("sections", [0, 1, 3])
def test_sections_and_settings_that_differ_inside_a_wave(gpu, sections):
    rng = np.random.default_rng(300 + sections)
    n = 9
    r = Rig(gpu, n)
    r.both("set_tones", TABLE8); r.both("set_window", 16); r.both("set_highpass", TR.highpass_design(300.0, sections))
    vary_settings(r, 8)
    x = tones_in_noise(rng, n, 40, TABLE8, amplitude=8000.0, sigma=9000.0)          # the noise reaches the clamps now and then
    r.call(x[:, :7])
    out, unmuted = r.call(x[:, 7:], extra_in=1, extra_out=1)
    assert 0 < unmuted.sum() < unmuted.size
    if sections:
        assert not np.array_equal(out[0], x[0, 7:])
    else:
        assert np.array_equal(out[0], x[0, 7:])                                       # PASS, no sections: an exact pass
    r.close()


# ---- extremes
def test_constant_minus_32768(gpu):
    """d = -32768 on every decimated sample; on a tone whose phase stays in table slot 0 the block's sum is R = -2^32."""
    r = Rig(gpu, 5)
    r.both("set_tones", [0.0001, 100.0, 200.0]); r.both("set_window", 16); r.both("set_highpass", TR.highpass_design(300.0, 3))
    x = np.full((5, 18, 128), -32768, dtype=np.int16)
    out, _ = r.call(x[:, :3])
    r.call(x[:, 3:], extra_out=1)
    assert int(r.ref.st["last_best"][0]) == 0 and int(r.ref.st["last_power"][0]) > 2**52 and np.abs(out[:, 2]).max() < 32768
    r.close()


def test_alternating_full_scale(gpu):
    r = Rig(gpu, 5)
    r.both("set_tones", TABLE8); r.both("set_window", 16); r.both("set_highpass", TR.highpass_design(300.0, 3))
    x = np.empty((5, 17, 128), dtype=np.int16)
    x[:, :, 0::2], x[:, :, 1::2] = 32767, -32768
    out, _ = r.call(x, extra_in=1)
    assert out.max() == 32767 and out.min() == -32768                                  # the high-pass passes the Nyquist tone at full scale
    r.close()


def test_full_scale_square_wave_on_a_table_tone_over_a_window_of_128(gpu):
    """67.0 Hz, the creation table's first tone: the accumulators' largest values (0.31 * 2^31 in the reference's own test)."""
    W = 128
    k = np.arange((W + 1) * 128)
    sq = np.where(np.sin(2.0 * np.pi * 67.0 * k / 44100.0) >= 0.0, 32767, -32768).astype(np.int16).reshape(W + 1, 128)
    r = Rig(gpu, 2)
    r.both("set_window", W); r.both("set_want", 0)
    x = np.stack([sq, -1 - sq])
    r.call(x[:, :W - 1])
    assert int(np.abs(r.ref.st["acc"]).max()) > 2**29
    _, unmuted = r.call(x[:, W - 1:])
    assert r.ref.st["detected"].tolist() == [0, 0] and unmuted.tolist() == [[0, 1], [0, 1]] and int(r.ref.st["last_power"][0]) > 2**57
    r.close()


def test_verdicts_exactly_at_min_power_and_at_the_dominance(gpu):
    """Four channels hear the same tone.  min_power = P_best and P_best + 1 (P_best from a first, unconditioned run of the
    reference): detected and not.  Then accumulators written through write_state whose powers are 1024, 1024, 256, 256: at
    dominance 64 the comparison 16 * 4 >= 64 * 1 holds with equality, at 65 it fails; a block of zeros (d = 0) ends the window."""
    rng = np.random.default_rng(400)
    one = tones_in_noise(rng, 1, 16, [TABLE8[2]])
    x = np.repeat(one, 4, axis=0)
    probe = TR.ToneRef(1)
    probe.set_tones(TABLE8); probe.set_window(16)
    probe.update(one)
    P = int(probe.st["last_power"][0])
    assert int(probe.st["detected"][0]) == 2 and P > 0
    r = Rig(gpu, 4)
    r.both("set_tones", TABLE8); r.both("set_window", 16); r.both("set_want", TR.ANY)
    for c, p in enumerate((P, P + 1, P - 1, 0)):
        r.both("set_min_power", p, ch=c)
    r.call(x)
    assert r.ref.st["detected"].tolist() == [2, -1, 2, 2] and r.ref.st["last_power"].tolist() == [P] * 4
    for dominance, want in ((64, 0), (65, -1)):
        r.both("reset"); r.both("set_dominance", dominance); r.both("set_min_power", 0)
        rec = r.sq.read_state()
        rec["window_block"] = 15
        rec["acc"][:, :4, 0] = [32, 32, 16, 16]
        r.sq.write_state(rec)
        for c in range(4):
            r.ref.put(c, rec[c])
        _, unmuted = r.call(np.zeros((4, 2, 128), dtype=np.int16))
        assert r.ref.st["detected"].tolist() == [want] * 4 and r.ref.st["last_other"].tolist() == [256] * 4
        assert unmuted.tolist() == [[0, int(want == 0)]] * 4
    r.close()


# ---- muting
def test_muting_every_want_kind_and_hang(gpu):
    """The tone is there for two windows of 16 blocks and gone for three.  A channel that wants it opens with the block after the
    first window and closes with the block after the third (hang 0), the fourth (hang 1) or not at all (hang 255); PASS is never
    muted, ANY follows the wanted tone's channel, another tone never opens."""
    rng = np.random.default_rng(500)
    n, W = 8, 16
    x = TR.to_int16(rng.normal(0.0, 500.0, size=(n, 5 * W * 128))).reshape(n, 5 * W, 128)
    x[:, :2 * W] = TR.to_int16(x[:, :2 * W].reshape(n, -1) + TR.tone_wave(2 * W * 128, TABLE8[3], 3000.0)[None, :]).reshape(n, 2 * W, 128)
    r = Rig(gpu, n)
    r.both("set_tones", TABLE8); r.both("set_window", W); r.both("set_highpass", TR.highpass_design(300.0, 1))
    r.both("set_min_power", TR.min_power(1000, W))
    for c, (want, hang) in enumerate(((3, 0), (3, 1), (3, 255), (TR.PASS, 0), (TR.ANY, 0), (TR.ANY, 1), (5, 0), (5, 255))):
        r.both("set_want", want, ch=c); r.both("set_hang", hang, ch=c)
    parts = [r.call(x[:, a:b])[1] for a, b in ((0, 17), (17, 48), (48, 49), (49, 80))]
    unmuted = np.concatenate(parts, axis=1)
    shape = lambda *runs: sum(([v] * k for v, k in runs), [])
    assert unmuted[0].tolist() == unmuted[4].tolist() == shape((0, 16), (1, 32), (0, 32))
    assert unmuted[1].tolist() == unmuted[5].tolist() == shape((0, 16), (1, 48), (0, 16))
    assert unmuted[2].tolist() == shape((0, 16), (1, 64)) and unmuted[3].all() and not unmuted[6:].any()
    st = r.sq.read_state()
    assert st["openings"].tolist() == [1, 1, 1, 1, 1, 1, 0, 0] and st["open_blocks"].tolist() == [32, 48, 64, 80, 32, 48, 0, 0]
    assert st["hang_left"][2] == 252 and st["matches"].tolist() == [2, 2, 2, 5, 2, 2, 0, 0] and (st["windows"] == 5).all()
    r.close()


# ---- state
def test_write_state_with_channels_at_different_window_blocks_then_one_call(gpu):
    rng = np.random.default_rng(600)
    n, W = 21, 16
    r = Rig(gpu, n)
    r.both("set_tones", TABLE8); r.both("set_window", W); r.both("set_highpass", TR.highpass_design(300.0, 1))
    vary_settings(r, 8)
    x = tones_in_noise(rng, n, 24, TABLE8)
    r.call(x[:, :5])
    rec = r.sq.read_state()
    rec["window_block"] = (np.arange(n) * 7) % W                   # 0 .. 15, different inside a wave
    rec["open"] = np.arange(n) % 2
    rec["hang_left"] = np.arange(n) % 3
    rec["detected"] = np.arange(n) % 9 - 1
    r.sq.write_state(rec)
    for c in range(n):
        r.ref.put(c, rec[c])
    r.check_state()
    r.call(x[:, 5:], extra_in=1)
    assert sorted(set(r.ref.st["window_block"].tolist())) == list(range(W)) and set(r.ref.st["windows"].tolist()) == {1, 2}
    r.close()


def test_a_running_channel_moves_mid_window_to_another_handle(gpu):
    """Channel 2 of a 5-channel handle goes, 21 blocks in (5 into its second window), to channel 18 of a 19-channel handle; its next
    blocks and its record there equal the uninterrupted reference's.  Then write_state's refusals, clear, reset and setters
    between calls."""
    rng = np.random.default_rng(601)
    W = 16

    def rig(n):
        r = Rig(gpu, n)
        r.both("set_tones", TABLE8); r.both("set_window", W); r.both("set_highpass", TR.highpass_design(300.0, 3))
        r.both("set_want", 2); r.both("set_hang", 1); r.both("set_min_power", TR.min_power(1000, W))
        return r
    x = tones_in_noise(rng, 5, 40, [TABLE8[2]])
    a = rig(5)
    a.call(x[:, :21])
    rec = a.sq.read_state()[2:3]
    assert int(rec["open"][0]) == 1 and int(rec["window_block"][0]) == 5 and rec["acc"].any() and rec["hp"].any() and rec["hist"].any()
    b = rig(19)
    b.sq.write_state(rec, channels=[18])
    b.ref.put(18, a.ref.records()[2])
    x2 = tones_in_noise(rng, 19, 19, TABLE8)
    x2[18] = x[2, 21:]
    out = b.call(x2)[0]
    want = a.ref.update(x[:, 21:])[0]                              # the uninterrupted reference
    assert np.array_equal(out[18], want[2]) and want[2].any()
    assert b.sq.read_state()[18].tobytes() == a.ref.records()[2].tobytes()
    for field, value, why in (("open", 2, "open must be 0 or 1"), ("window_block", W, "window_block"), ("detected", 8, "detected"),
                              ("last_best", -2, "last_best"), ("reserved", 1, "reserved")):
        bad = rec.copy(); bad[field] = value
        with pytest.raises(gpu.AsdrError, match=why):
            b.sq.write_state(bad, channels=[0])
    bad = rec.copy(); bad["acc"][0, 8, 1] = 1
    with pytest.raises(gpu.AsdrError, match="acc must be 0"):
        b.sq.write_state(bad, channels=[0])
    b.check_state()
    b.both("clear")
    b.check_state()
    b.call(x2[:, :3])
    b.both("set_window", 17)                                       # restarts every window; open, detected and the counters stay
    b.check_state()
    assert not b.sq.read_state()["window_block"].any() and b.sq.read_state()["open"].any()
    b.both("set_dominance", 32); b.both("set_highpass", None); b.both("set_want", TR.ANY, ch=3); b.both("set_hang", 0)
    b.call(x2[:, 3:], extra_out=2)
    b.both("set_tones", TABLE8[:5])
    b.check_state()
    b.call(x2[:, :18])
    b.both("reset")
    b.check_state()
    b.call(x2[:, :2])
    a.close(); b.close()


# ---- streams
def test_calls_on_the_callers_streams(gpu):
    """A call on a caller's stream, then 35 blocks as 1 + 17 + 17 alternating between two streams with no host synchronisation in
    between: outputs and state equal the reference's."""
    import torch
    rng = np.random.default_rng(700)
    n, W = 37, 16
    r = Rig(gpu, n)
    r.both("set_tones", TABLE8); r.both("set_window", W); r.both("set_highpass", TR.highpass_design(300.0, 1))
    vary_settings(r, 8)
    x = tones_in_noise(rng, n, 40, TABLE8)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    r.call(x[:, :5], stream=streams[0])
    d_in = torch.from_numpy(x[:, 5:].copy()).cuda()
    d_out = torch.full((n, 35, 128), PATTERN, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for k, (a, size) in enumerate(((0, 1), (1, 17), (18, 17))):
        r.sq.update_device(d_in[:, a:].data_ptr(), d_out[:, a:].data_ptr(), size, in_stride_blocks=35, out_stride_blocks=35,
                           stream=streams[k & 1].cuda_stream)
    r.sq.synchronize()
    torch.cuda.synchronize()
    out, _ = r.ref.update(x[:, 5:])
    assert np.array_equal(d_out.cpu().numpy(), out)
    r.check_state()
    r.close()


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
    return TR.to_int16(amplitude * np.cos(phi)), TR.to_int16(amplitude * np.sin(phi))


def test_fm_to_tone_squelch_to_gate(gpu):
    """Three FM channels whose modulation is 300 .. 3000 Hz noise (0.18 of the deviation, rms) plus, at a tenth of the deviation,
    the wanted tone (141.3 Hz), another tone (100.0 Hz), or none.  FM demodulator (hp_shift 12: the tone reaches the audio rows),
    tone squelch (the creation table, W = 64, the three-section 300 Hz high-pass, want = 141.3 Hz) and gate (open_energy 1) run on
    one stream with no host step in between, as a call of 64 blocks and one of 66.  Expectations come from fm_ref -> tone_ref ->
    gate_ref; on the reference itself: the first call delivers nothing (every window starts closed), the second only channel 0,
    and the decoded tones are 141.3 Hz, 100.0 Hz and none."""
    import torch
    n, W, nb = 3, 64, 130
    rng = np.random.default_rng(800)
    m = 0.18 * TR.voice_noise(rng, (n, nb * 128), 1.0)
    m[0] += 0.1 * TR.tone_wave(nb * 128, 141.3, 1.0)
    m[1] += 0.1 * TR.tone_wave(nb * 128, 100.0, 1.0)
    I, Q = (np.stack(v).reshape(n, nb, 128) for v in zip(*[fm_carrier(m[c]) for c in range(n)]))
    wanted = TR.CTCSS.index(141.3)
    fm, sq, gate = gpu.FmDemodulator(n), gpu.ToneSquelch(n), gpu.AudioGate(n)
    fm.set_dc_shift(12)
    sq.set_highpass(fc_hz=300.0, sections=3); sq.set_want(wanted); sq.set_min_power(gpu.tone_min_power(1000, W))
    gate.set_squelch(energies=(1, 1), hang_blocks=0)
    fref, tref, gref = FR.FmRef(n), TR.ToneRef(n), GR.GateRef(n)
    fref.set_dc_shift(12)
    tref.set_highpass(TR.highpass_design(300.0, 3)); tref.set_want(wanted); tref.set_min_power(TR.min_power(1000, W))
    gref.set_squelch(1, 1, 0)
    s = torch.cuda.Stream()
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    d_v, d_y = (torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda") for _ in range(2))
    d_rows = torch.full((2, n, 66, 128), PATTERN, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    counts, indices = [], []
    for k, (a, size) in enumerate(((0, 64), (64, 66))):
        fm.update_device(dI[:, a:].data_ptr(), dQ[:, a:].data_ptr(), d_v[:, a:].data_ptr(), size, in_stride_blocks=nb, out_stride_blocks=nb,
                         stream=s.cuda_stream)
        sq.update_device(d_v[:, a:].data_ptr(), d_y[:, a:].data_ptr(), size, in_stride_blocks=nb, out_stride_blocks=nb, stream=s.cuda_stream)
        gate.update_device(d_y[:, a:].data_ptr(), size, stride_blocks=nb, rows_ptr=d_rows[k].data_ptr(), capacity_rows=n, stream=s.cuda_stream)
        s.synchronize()
        counts.append(int(gate.count_tensor().cpu()[0]))
        indices.append(gate.index_tensor().cpu().numpy()[:counts[-1]].tolist())
    v = fref.update(I, Q)[0]
    assert np.array_equal(d_v.cpu().numpy(), v)
    y1, y2 = tref.update(v[:, :64])[0], tref.update(v[:, 64:])[0]
    assert np.array_equal(d_y.cpu().numpy(), np.concatenate([y1, y2], axis=1))
    assert sq.read_state().tobytes() == tref.records().tobytes()
    i1, rows1, _ = gref.update(y1)
    i2, rows2, _ = gref.update(y2)
    assert i1.tolist() == [] and i2.tolist() == [0] and not y1.any() and y2[0].any() and not y2[1:].any()
    assert tref.st["detected"].tolist() == [wanted, TR.CTCSS.index(100.0), -1]
    assert counts == [0, 1] and indices == [[], [0]]
    assert np.array_equal(d_rows[1].cpu().numpy().reshape(-1, 128)[:66], rows2[0]) and (d_rows[0].cpu().numpy() == PATTERN).all()
    hz = sq.decoded_hz()
    assert hz[0] == 141.3 and hz[1] == 100.0 and np.isnan(hz[2])
    # the hum is gone: what is left of the tone in channel 0's delivered audio, against what the demodulator gave
    k = np.arange(64 * 128, 130 * 128)
    probe = np.exp(-2j * np.pi * 141.3 * k / 44100.0)
    before, after = abs((v[0, 64:].reshape(-1) * probe).sum()), abs((y2[0].reshape(-1) * probe).sum())
    assert after < before / 30.0
    fm.close(); sq.close(); gate.close()
