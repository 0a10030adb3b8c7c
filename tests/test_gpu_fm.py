"""The FM demodulator on the GPU (include/asdr_fm.h; audiosdr_amd/csrc/asdr_fm.hip) against tests/fm_ref.py at tolerance 0: every
byte of the output buffer (a guard pattern fills the stride gaps and a row behind the last) and every state field, over partial
waves and workgroups, block counts either side of the LDS chunk, strides, the arithmetic's extremes, per-channel settings, the
squelch, streams, the state calls, and end to end behind a tuner bank and in front of a gate.
The sizes are the smallest that reach each seam: a workgroup holds gpu.FM_NARROW_ROWS = 16 channels in a bank below
gpu.FM_WIDE_CHANNELS = 32768 channels and gpu.FM_ROWS = 64 from there on (a lane of its first wave each in the recurrence part; 4
rows per wave and 16 per workgroup and pass in the pointwise part) and stages gpu.FM_CHUNK_BLOCKS = 1 block.  Banks of 32768
channels and more share one reference of 1021 channels, repeated."""
import numpy as np
import pytest

import fm_ref as FR
import gate_ref as GR

pytestmark = pytest.mark.gpu
GAP = 0x7FFF        # fills the input strides' gaps: must not be read
PATTERN = 0x5A5B    # pre-fills the output buffer: must stay wherever nothing is written


class Rig:
    """A demodulator and its reference side by side; call() runs one update on both and compares everything."""

    def __init__(self, A, n):
        import torch
        self.torch, self.A, self.n = torch, A, n
        self.fm, self.ref = A.FmDemodulator(n), FR.FmRef(n)

    def each(self, method, *args, ch=-1):
        getattr(self.fm, method)(*args, ch=ch)
        getattr(self.ref, method)(*args, ch=ch)

    def call(self, I, Q, extra_in=0, extra_out=0, stream=None, want=None):
        """I, Q int16 [n][nb][128].  Returns the reference's (out, opens); `want` gives them where they are already known."""
        torch = self.torch
        n, nb = I.shape[:2]
        pI, pQ = (np.full((n, nb + extra_in, 128), GAP, dtype=np.int16) for _ in range(2))
        pI[:, :nb], pQ[:, :nb] = I, Q
        dI, dQ = torch.from_numpy(pI).cuda(), torch.from_numpy(pQ).cuda()
        d_out = torch.full((n * (nb + extra_out) + 1, 128), PATTERN, dtype=torch.int16, device="cuda")   # one guard row behind
        torch.cuda.synchronize()
        self.fm.update_device(dI.data_ptr(), dQ.data_ptr(), d_out.data_ptr(), nb, in_stride_blocks=nb + extra_in,
                              out_stride_blocks=nb + extra_out, stream=stream.cuda_stream if stream is not None else 0)
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        out, opens = self.ref.update(I, Q) if want is None else want
        expect = np.full((n, nb + extra_out, 128), PATTERN, dtype=np.int16)
        expect[:, :nb] = out
        got = d_out.cpu().numpy()
        bad = np.argwhere(got[:-1].reshape(expect.shape) != expect)
        assert bad.size == 0, (len(bad), bad[0].tolist())
        assert (got[-1] == PATTERN).all(), "written behind the last row"
        assert np.array_equal(dI.cpu().numpy(), pI) and np.array_equal(dQ.cpu().numpy(), pQ)
        if want is None:
            self.check_state()
        return out, opens

    def check_state(self):
        got, want = FR.record_tuples(self.fm.read_state()), self.ref.state_tuples()
        bad = [c for c in range(self.n) if got[c] != want[c]]
        assert not bad, (len(bad), bad[0], got[bad[0]], want[bad[0]])
        assert self.fm.blocks() == self.ref.blocks

    def close(self):
        self.fm.close()


def full_noise(rng, n, nb):
    return tuple(rng.integers(-32768, 32768, size=(n, nb, 128)).astype(np.int16) for _ in range(2))


def mixed_levels(rng, n, nb):
    """Full-range noise shifted down by 0 .. 14 bits per block, an eighth of the blocks all zero."""
    out = []
    for _ in range(2):
        a = (rng.integers(-32768, 32768, size=(n, nb, 128)) >> rng.integers(0, 15, size=(n, nb, 1))).astype(np.int16)
        a[rng.random((n, nb)) < 0.125] = 0
        out.append(a)
    return tuple(out)


def tone_rows(n, nb, amplitude=8000.0, first=0, **kw):
    """int16 (I, Q) [n][nb][128]: the 1 kHz tone at 3 kHz deviation, channel c starting at phase c (radians); samples first .."""
    rows = [FR.fm_iq(128 * (first + nb), amplitude, phase0=float(c), **kw) for c in range(n)]
    I, Q = (np.stack([r[k][128 * first:] for r in rows]).reshape(n, nb, 128) for k in range(2))
    return I, Q


def vary_settings(r):
    """Every channel different, inside one wave too: the gains' two ends, a = 1 and 32768, hp_shift 0 / 1 / 15."""
    gains = [1, 1 << 24, 144502, 1000, 7, (1 << 24) - 1, 30000, 2500000]
    deemph = [32768, 1, 976, 8550, 32767, 2, 20000]
    shifts = [0, 1, 15, 8, 4]
    for c in range(r.n):
        r.each("set_gain", gains[c % 8] if c < 16 else 1 + (c * 2654435761) % (1 << 24), ch=c)
        r.each("set_deemphasis", deemph[c % 7], ch=c)
        r.each("set_dc_shift", shifts[c % 5], ch=c)


# ---- partial waves and workgroups, blocks either side of the chunk, strides
@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257])
def test_channels_blocks_and_strides(gpu, n):
    """One less and one more than a wave's 4 rows, a workgroup's 16 and a wave of workgroups' 64; 257: seventeen workgroups, the
    last with one channel.  Calls of 1 block (the chunk), 2 and 3 blocks, then 5, with different per-channel settings and strides
    larger than n_blocks on both sides; a call of 0 blocks does nothing."""
    assert gpu.FM_NARROW_ROWS == 16 and gpu.FM_CHUNK_BLOCKS == 1 and n < gpu.FM_WIDE_CHANNELS
    rng = np.random.default_rng(n)
    r = Rig(gpu, n)
    vary_settings(r)
    r.each("set_squelch", 4 * 10**11, 7 * 10**11, 1)
    seen = []
    for nb, ein, eout in ((1, 0, 0), (2, 3, 1), (3, 1, 2), (5, 0, 3)):
        I, Q = mixed_levels(rng, n, nb) if nb != 2 else full_noise(rng, n, nb)
        seen.append(r.call(I, Q, extra_in=ein, extra_out=eout)[1])
    opens = np.concatenate(seen, axis=1)
    if n >= 15:
        assert 0 < opens.sum() < opens.size
    d = r.torch.zeros((n, 2, 128), dtype=r.torch.int16, device="cuda")
    r.fm.update_device(d.data_ptr(), d.data_ptr(), d.data_ptr(), 0, in_stride_blocks=2, out_stride_blocks=2)   # nothing happens
    r.check_state()
    r.close()


# ---- arithmetic
def test_rows_of_zero(gpu):
    r = Rig(gpu, 20)
    vary_settings(r)
    z = np.zeros((20, 2, 128), dtype=np.int16)
    out, opens = r.call(z, z, extra_out=1)
    assert not out.any() and opens.all() and not r.fm.read_state()["last_noise"].any()
    r.close()


def test_rows_of_minus_32768(gpu):
    """re = 2^31 and im = 0 on every sample but the first, the case that needs more than 32 bits; P = 2^38 per block."""
    r = Rig(gpu, 9)
    x = np.full((9, 3, 128), -32768, dtype=np.int16)
    out, _ = r.call(x, x, extra_in=1)
    st = r.fm.read_state()
    assert np.abs(out).max() <= 1 and (st["last_power"] == 1 << 38).all() and (st["prev_i"] == -32768).all()
    r.close()


def test_the_largest_im_and_the_largest_noise(gpu):
    """Samples alternating between (-32768, 32767) and (32767, 32767) reach |im| = 2^31 - 2^15; quarter turns to and fro under the
    largest gain make v alternate between the clamps: |w| = 32767 + 2 * 32768 + 32767 on every sample, N just under 2^41."""
    n = 5
    I, Q = np.empty((n, 2, 128), dtype=np.int16), np.full((n, 2, 128), 32767, dtype=np.int16)
    I[:, :, 0::2], I[:, :, 1::2] = -32768, 32767
    r = Rig(gpu, n)
    r.each("set_gain", 1 << 24)
    out, _ = r.call(I, Q)
    assert out.min() == -32768 and out.max() == 32767
    assert int(r.fm.read_state()["last_noise"][0]) == 128 * 131070 ** 2 > 1 << 40
    r.close()


def test_amplitude_3_noise(gpu):
    rng = np.random.default_rng(33)
    n = 70
    I, Q = (rng.integers(-3, 4, size=(n, 3, 128)).astype(np.int16) for _ in range(2))
    r = Rig(gpu, n)
    vary_settings(r)
    out, _ = r.call(I, Q, extra_in=2, extra_out=2)
    assert out.any()
    r.close()


def test_full_range_noise_with_filters(gpu):
    rng = np.random.default_rng(34)
    n = 130
    r = Rig(gpu, n)
    vary_settings(r)
    for nb in (4, 1):
        I, Q = full_noise(rng, n, nb)
        r.call(I, Q)
    st = r.fm.read_state()
    assert (st["last_noise"] > 10**11).sum() > n // 4 and len(set(st["m"].tolist())) > n // 2
    r.close()


def test_known_answer_1khz_tone(gpu):
    """The noiseless 1 kHz tone at 3 kHz deviation, amplitude 8000, gain for 5 kHz: the reference's bits, and within 10 LSB of
    0.6 * 32767 * sinc(1000 / 44100) * cos(2 pi 1000 (n - 0.5) / 44100) from sample 2 on."""
    nb = 4
    I, Q = tone_rows(1, nb)
    r = Rig(gpu, 1)
    out = r.call(I, Q)[0].reshape(-1).astype(np.float64)
    k = np.arange(out.size)
    want = 0.6 * 32767.0 * np.sinc(1000.0 / 44100.0) * np.cos(2.0 * np.pi * 1000.0 * (k - 0.5) / 44100.0)
    assert np.abs(out - want)[2:].max() <= 10.0
    r.close()


# ---- the squelch
def test_squelch_tones_drop_out_mid_call(gpu):
    """Even channels carry the tone in blocks 0 .. 2 and noise from block 3 on, odd channels noise throughout; thresholds 10^11 /
    3 10^11, hang 2.  A tone channel is open for its three blocks and the two of the hang; a noise channel never opens."""
    rng = np.random.default_rng(35)
    n, nb = 130, 8
    I, Q = (np.clip(np.floor(rng.normal(0.0, 3000.0, size=(n, nb, 128)) + 0.5), -32768, 32767).astype(np.int16) for _ in range(2))
    tI, tQ = tone_rows(n // 2, 3)
    I[0::2, :3], Q[0::2, :3] = tI, tQ
    r = Rig(gpu, n)
    r.each("set_squelch", 10**11, 3 * 10**11, 2)
    r.each("set_deemphasis", 976); r.each("set_dc_shift", 8)
    out, opens = r.call(I, Q, extra_out=1)
    assert opens[0::2].tolist() == [[1, 1, 1, 1, 1, 0, 0, 0]] * (n // 2) and not opens[1::2].any()
    assert not out[0::2, 5:].any() and not out[1::2].any() and all(out[0::2, b].any() for b in range(5))
    st = r.fm.read_state()
    assert st["open"].tolist() == [0] * n and st["openings"].tolist() == [1, 0] * (n // 2) and st["open_blocks"].tolist() == [5, 0] * (n // 2)
    assert st["hang_left"].tolist() == [0] * n and (st["last_noise"] > 3 * 10**11).all()
    tI, tQ = tone_rows(n // 2, 2, first=3)                       # the tones return: hang_left is 2 again, then runs down by one
    I2, Q2 = I[:, :3].copy(), Q[:, :3].copy()
    I2[0::2, :2], Q2[0::2, :2] = tI, tQ
    I2[:, 2], Q2[:, 2] = I[:, 5], Q[:, 5]
    opens = r.call(I2, Q2)[1]
    assert opens[0::2].tolist() == [[1, 1, 1]] * (n // 2) and not opens[1::2].any()
    st = r.fm.read_state()
    assert st["hang_left"].tolist() == [1, 0] * (n // 2) and st["openings"].tolist() == [2, 0] * (n // 2)
    r.close()


# ---- calls and streams
def test_seven_blocks_as_1_2_4_on_two_streams(gpu):
    """The calls alternate between two streams with no host synchronisation between them; outputs and state equal one call of 7."""
    import torch
    rng = np.random.default_rng(36)
    n, nb = 150, 7
    I, Q = mixed_levels(rng, n, nb)
    whole = Rig(gpu, n)
    vary_settings(whole)
    whole.each("set_squelch", 4 * 10**11, 7 * 10**11, 1)
    out, opens = whole.call(I, Q)
    assert 0 < opens.sum() < opens.size
    f = gpu.FmDemodulator(n)
    for c in range(n):
        f.set_gain(int(whole.ref.gain[c]), ch=c); f.set_deemphasis(int(whole.ref.deemphasis[c]), ch=c); f.set_dc_shift(int(whole.ref.hp_shift[c]), ch=c)
    f.set_squelch(4 * 10**11, 7 * 10**11, 1)
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    d_out = torch.full((n, nb, 128), PATTERN, dtype=torch.int16, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for k, (a, size) in enumerate(((0, 1), (1, 2), (3, 4))):
        f.update_device(dI[:, a:].data_ptr(), dQ[:, a:].data_ptr(), d_out[:, a:].data_ptr(), size, in_stride_blocks=nb, out_stride_blocks=nb,
                        stream=streams[k & 1].cuda_stream)
    f.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), out)
    assert f.read_state().tobytes() == whole.fm.read_state().tobytes() and f.blocks() == 7
    f.close(); whole.close()


def test_a_running_channel_moves_to_another_handle(gpu):
    """Channel 2 of a 5-channel handle goes, after two blocks, to channel 70 of a 71-channel handle with read_state / write_state;
    its next block there is bit for bit the block the uninterrupted reference gives."""
    rng = np.random.default_rng(37)
    I, Q = mixed_levels(rng, 5, 3)
    I[2], Q[2] = tone_rows(1, 3, noise=300.0, rng=rng)
    a = Rig(gpu, 5)
    a.each("set_deemphasis", 8550); a.each("set_dc_shift", 6); a.each("set_squelch", 10**11, 3 * 10**11, 2)
    a.call(I[:, :2], Q[:, :2])
    rec = a.fm.read_state()[2:3]
    assert int(rec["open"][0]) == 1 and int(rec["s"][0]) != 0 and int(rec["m"][0]) != 0
    b = Rig(gpu, 71)
    b.each("set_deemphasis", 8550); b.each("set_dc_shift", 6); b.each("set_squelch", 10**11, 3 * 10**11, 2)
    b.fm.write_state(rec, channels=[70])
    b.ref.put(70, a.ref.state_tuples()[2])
    I2, Q2 = mixed_levels(rng, 71, 1)
    I2[70], Q2[70] = I[2, 2:], Q[2, 2:]
    out = b.call(I2, Q2)[0]
    want = a.ref.update(I[:, 2:], Q[:, 2:])[0]                   # the uninterrupted reference
    assert np.array_equal(out[70], want[2]) and want[2].any()
    assert FR.record_tuples(b.fm.read_state())[70] == a.ref.state_tuples()[2]
    with pytest.raises(gpu.AsdrError, match="open must be 0 or 1"):
        bad = rec.copy(); bad["open"] = 2
        b.fm.write_state(bad, channels=[0])
    b.check_state()
    b.fm.clear(); b.ref.clear()
    b.check_state()
    b.fm.reset(); b.ref.reset()
    b.check_state()
    b.call(I2, Q2)
    a.close(); b.close()


def test_update_device_refusals_change_nothing(gpu):
    import torch
    r = Rig(gpu, 10)
    d = torch.zeros((3, 10, 4, 128), dtype=torch.int16, device="cuda")
    i, q, o = (d[k].data_ptr() for k in range(3))
    for kw, why in ((dict(i_ptr=i + 2, q_ptr=q, out_ptr=o, n_blocks=1), "16-byte"), (dict(i_ptr=i, q_ptr=q, out_ptr=o + 8, n_blocks=1), "16-byte"),
                    (dict(i_ptr=i, q_ptr=q, out_ptr=o, n_blocks=3, in_stride_blocks=2), "stride"),
                    (dict(i_ptr=i, q_ptr=q, out_ptr=o, n_blocks=3, out_stride_blocks=2), "stride"),
                    (dict(i_ptr=i, q_ptr=q, out_ptr=o, n_blocks=65536, in_stride_blocks=65536, out_stride_blocks=65536), "n_blocks"),
                    (dict(i_ptr=0, q_ptr=q, out_ptr=o, n_blocks=1), "null"), (dict(i_ptr=i, q_ptr=q, out_ptr=0, n_blocks=1), "null"),
                    (dict(i_ptr=i, q_ptr=q, out_ptr=i + 256, n_blocks=2, in_stride_blocks=4, out_stride_blocks=4), "overlaps"),
                    (dict(i_ptr=i, q_ptr=q, out_ptr=q, n_blocks=4), "overlaps")):
        with pytest.raises(gpu.AsdrError, match=why):
            r.fm.update_device(**kw)
    r.check_state()
    r.close()


# ---- end to end
def test_tuner_bank_to_fm_to_gate(gpu):
    """A CU8 wideband source at 48 x 44.1 kHz with four FM carriers; channel 2 k is tuned to carrier k, channel 2 k + 1 beside it
    where there is only noise.  Tuner bank, FM demodulator and gate run on one stream with no host step in between; the gate's
    open_energy = 1 delivers exactly the channels the squelch left unmuted, and their rows equal the reference's on the I/Q rows the
    bank wrote (the bank itself is held to its own restatement elsewhere)."""
    import torch
    D, n, nb = 48, 8, 6
    fs, N = 44100 * D, nb * 128 * D
    rng = np.random.default_rng(5)
    t = np.arange(N) / fs
    carriers = [100e3 * (k + 1) for k in range(4)]
    x = sum(25.0 * np.exp(1j * (2 * np.pi * fc * t + 3.0 * np.sin(2 * np.pi * 1000.0 * t))) for fc in carriers)
    x = x + rng.normal(0.0, 1.5, N) + 1j * rng.normal(0.0, 1.5, N)
    raw = np.clip(np.floor(np.stack([x.real, x.imag], axis=-1) + 128.0), 0, 255).astype(np.uint8)[None]
    bank = gpu.TunerBank(n, 1, D)
    bank.set_input_format("cu8")
    for c in range(n):
        bank.set_frequency(carriers[c // 2] + (50e3 if c & 1 else 0.0), ch=c)
    fm, gate = gpu.FmDemodulator(n), gpu.AudioGate(n)
    fm.set_squelch(10**11, 3 * 10**11, 2); fm.set_deemphasis(tau_us=750.0); fm.set_dc_shift(10)
    gate.set_squelch(energies=(1, 1), hang_blocks=0)
    s = torch.cuda.Stream()
    d_raw = torch.from_numpy(raw).cuda()
    dI, dQ, d_audio = (torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda") for _ in range(3))
    d_rows = torch.full((n, nb, 128), PATTERN, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert bank.update_samples_device(d_raw.data_ptr(), dI.data_ptr(), dQ.data_ptr(), nb, nb, stream=s.cuda_stream) == nb
    fm.update_device(dI.data_ptr(), dQ.data_ptr(), d_audio.data_ptr(), nb, stream=s.cuda_stream)
    gate.update_device(d_audio.data_ptr(), nb, rows_ptr=d_rows.data_ptr(), capacity_rows=n, stream=s.cuda_stream)
    s.synchronize()
    ref = FR.FmRef(n)
    ref.set_squelch(10**11, 3 * 10**11, 2); ref.set_deemphasis(976); ref.set_dc_shift(10)
    out, opens = ref.update(dI.cpu().numpy(), dQ.cpu().numpy())
    assert opens[0::2].all() and not opens[1::2].any()          # the carriers are heard, the gaps are not
    assert np.array_equal(d_audio.cpu().numpy(), out)
    gref = GR.GateRef(n)
    gref.set_squelch(1, 1, 0)
    index, rows, _ = gref.update(out)
    assert index.tolist() == [0, 2, 4, 6]
    count = int(gate.count_tensor().cpu()[0])
    assert count == 4 and np.array_equal(gate.index_tensor().cpu().numpy()[:4], index)
    got = d_rows.cpu().numpy()
    assert np.array_equal(got[:4], rows) and (got[4:] == PATTERN).all()
    idx2, rows2 = gate.deliver(d_audio.data_ptr(), nb)           # and through the host entry
    assert idx2.tolist() == [0, 2, 4, 6] and np.array_equal(rows2, out[0::2])
    assert np.abs(fm.offset_hz(5000.0)[0::2]).max() < 100.0      # tuned on the carriers
    assert FR.record_tuples(fm.read_state()) == ref.state_tuples()
    bank.close(); fm.close(); gate.close()


# ---- banks of FM_WIDE_CHANNELS channels and more: 64 channels per workgroup
PERIOD = 1021       # a prime: every workgroup sees another alignment of the repeated rows and settings


@pytest.fixture(scope="module")
def wide_reference():
    """The reference of 1021 channels, once: a call of 1 block, then one of 3 blocks; different settings per channel; every seventh
    channel a noisy tone, the others noise at mixed levels.  Returns (I, Q) [1021][4][128], the settings, and after each call
    (out, records)."""
    rng = np.random.default_rng(38)
    I, Q = mixed_levels(rng, PERIOD, 4)
    I[5::7], Q[5::7] = tone_rows((PERIOD + 1) // 7, 4, noise=200.0, rng=rng)
    ref = FR.FmRef(PERIOD)
    sets = [(1 + (c * 2654435761) % (1 << 24) if c % 7 != 5 else 144502, (32768, 1, 976, 8550, 32767, 2, 20000)[c % 7], (0, 1, 15, 8, 4)[c % 5])
            for c in range(PERIOD)]
    for c, (g, a, k) in enumerate(sets):
        ref.set_gain(g, ch=c); ref.set_deemphasis(a, ch=c); ref.set_dc_shift(k, ch=c)
    ref.set_squelch(10**11, 3 * 10**11, 1)
    steps = []
    for a, b in ((0, 1), (1, 4)):
        out, opens = ref.update(I[:, a:b], Q[:, a:b])
        assert 0 < opens.sum() < opens.size
        rec = np.zeros(PERIOD, dtype=[(k, t) for k, t in zip(FR.STATE_NAMES, FR.STATE_TYPES)])
        for k in FR.STATE_NAMES:
            rec[k] = ref.st[k]
        steps.append((out, rec))
    return I, Q, sets, steps


@pytest.mark.parametrize("n", [32767, 32768, 32769, 32768 + 63, 32768 + 65, 65536])
def test_wide_banks(gpu, wide_reference, n):
    """Either side of the size at which a workgroup takes 64 channels, a last workgroup of 1, 63 and 1 (after a full one) channels,
    and the full size of 65,536: a one-block call, then three blocks with strides larger than n_blocks, against the repeated
    reference; every output byte, the guard row and every state field."""
    import torch
    assert gpu.FM_WIDE_CHANNELS == 32768 and gpu.FM_ROWS == 64
    I, Q, sets, steps = wide_reference
    sel = np.arange(n) % PERIOD
    f = gpu.FmDemodulator(n)
    L, h = f._L, f._h
    for c in range(n):
        g, a, k = sets[c % PERIOD]
        assert L.asdr_fm_set_gain(h, c, g) == 0 and L.asdr_fm_set_deemphasis(h, c, a) == 0 and L.asdr_fm_set_dc_shift(h, c, k) == 0
    f.set_squelch(10**11, 3 * 10**11, 1)
    for (a, b, ein, eout), (out, rec) in zip(((0, 1, 0, 0), (1, 4, 1, 2)), steps):
        nb = b - a
        pI, pQ = (np.full((n, nb + ein, 128), GAP, dtype=np.int16) for _ in range(2))
        pI[:, :nb], pQ[:, :nb] = I[sel, a:b], Q[sel, a:b]
        dI, dQ = torch.from_numpy(pI).cuda(), torch.from_numpy(pQ).cuda()
        d_out = torch.full((n * (nb + eout) + 1, 128), PATTERN, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        f.update_device(dI.data_ptr(), dQ.data_ptr(), d_out.data_ptr(), nb, in_stride_blocks=nb + ein, out_stride_blocks=nb + eout)
        f.synchronize()
        got = d_out.cpu().numpy()
        assert (got[-1] == PATTERN).all(), "written behind the last row"
        got = got[:-1].reshape(n, nb + eout, 128)
        assert np.array_equal(got[:, :nb], out[sel]) and (got[:, nb:] == PATTERN).all()
        assert f.read_state().tobytes() == rec[sel].tobytes()
    assert f.blocks() == 4
    f.close()
