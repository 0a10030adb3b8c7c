"""The audio resampler on the GPU (include/asdr_resample.h; audiosdr_amd/csrc/asdr_resample.hip) against tests/resample_ref.py at
tolerance 0: every default rate over partial workgroups and call sizes from one tile to many, splitting, custom filters at the ends of
every range and at the int32 edge, strides and guard samples, the index form alone and behind a real gate, positions past 2^31,
2^32 and 2^40, the state calls, streams, and end to end behind the chain on the oracle's audio.
The sizes are the smallest that reach each seam: a workgroup is 64 rows (a lane of every wave owns a row: 67 and 257 channels
leave a partial group) by one tile of outputs, sized so that 64 windows fit 64 KiB of LDS (98 outputs at 12 kHz, 54 at 8 kHz:
a one-block call is one tile, the 5-block call two or more, the 37-block call 13 or more with a partial last one); the four waves
of a workgroup take outputs w, w + 4, ... of the tile."""
import numpy as np
import pytest

import gate_ref as GR
import resample_ref as RR

pytestmark = pytest.mark.gpu
GAP = 0x7FFF        # fills the stride gaps of the audio rows: must not be read
PATTERN = 0x5A5B    # pre-fills the output buffer: must stay wherever nothing is to be written
GUARD = 64          # samples behind the last output row


def full_range(rng, n, nb):
    return rng.integers(-32768, 32768, size=(n, nb, 128)).astype(np.int16)


class Rig:
    """A resampler and its reference side by side; call() runs one update on both and compares everything."""

    def __init__(self, A, n, fs=12000, custom=None):
        import torch
        self.torch, self.A, self.n = torch, A, n
        if custom is None:
            self.rs = A.AudioResampler(n, fs_out=fs)
        else:
            up, down, taps, shift = custom
            self.rs = A.AudioResampler(n, up=up, down=down, taps=taps, shift=shift)
        taps, shift = self.rs.get_taps()
        self.ref = RR.ResampleRef(n, self.rs.up, self.rs.down, taps, shift)

    def place(self, n0, history):
        """Both sides at position n0 with the given records."""
        self.rs.set_position(n0); self.rs.write_state(history)
        self.ref.N = int(n0); self.ref.state = np.array(history, dtype=np.int16).reshape(self.n, 256).copy()

    def set_filter(self, taps, shift):
        self.rs.set_filter(taps, shift); self.ref.set_filter(taps, shift)

    def call(self, audio, extra_stride=0, out_extra=0, index=None, count=None, capacity=None, stream=None):
        """audio int16 [n][nb][128].  index (int32 list) / count / capacity select the index form.  Returns the reference's
        outputs of all channels, int16 [n][returned count]."""
        torch = self.torch
        n, nb = audio.shape[:2]
        padded = np.full((n, nb + extra_stride, 128), GAP, dtype=np.int16)
        padded[:, :nb] = audio
        want_n = self.ref.out_samples(nb)
        assert self.rs.out_samples(nb) == want_n
        stride = want_n + out_extra
        if index is None:
            rows, k, chans = n, n, np.arange(n)
        else:
            rows = capacity
            k = min(count, capacity)
            chans = np.asarray(index[:k], dtype=np.int64)
            d_index = torch.from_numpy(np.asarray(index, dtype=np.int32).copy()).cuda()
            d_count = torch.tensor([count], dtype=torch.int32, device="cuda")
        d_audio = torch.from_numpy(padded).cuda()
        d_out = torch.full((max(rows, 1) * stride + GUARD,), PATTERN, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        got_n = self.rs.update_device(d_audio.data_ptr(), nb, d_out.data_ptr(), stride, stride_blocks=nb + extra_stride,
                                      index_ptr=0 if index is None else d_index.data_ptr(), count_ptr=0 if index is None else d_count.data_ptr(),
                                      capacity_rows=0 if index is None else capacity, stream=stream.cuda_stream if stream is not None else 0)
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        want = self.ref.update(padded, n_blocks=nb)
        assert got_n == want_n == want.shape[1]
        out = d_out.cpu().numpy()
        body = out[:max(rows, 1) * stride].reshape(max(rows, 1), stride)
        assert np.array_equal(body[:k, :want_n], want[chans]), "outputs differ from the reference"
        assert (body[:k, want_n:] == PATTERN).all(), "a row is written past the returned count"
        assert (body[k:] == PATTERN).all(), "rows past min(count, capacity_rows) are written"
        assert (out[max(rows, 1) * stride:] == PATTERN).all(), "the buffer is written behind the last row"
        assert np.array_equal(d_audio.cpu().numpy(), padded)
        assert self.rs.position() == self.ref.N and self.rs.output_position() == self.ref.output_position()
        return want

    def check_state(self):
        assert np.array_equal(self.rs.read_state(), self.ref.state)

    def close(self):
        self.rs.close()


# ---- every default rate, partial workgroups, both regimes
@pytest.mark.parametrize("n", [1, 7, 8, 9, 67, 257])
@pytest.mark.parametrize("fs", RR.DEFAULT_RATES)
def test_default_rates_channel_counts_and_call_sizes(gpu, fs, n):
    """Calls of 1, 1, 2, 5 and 37 blocks: a one-block call is one tile whose four waves share 24 .. 93 outputs, 37 blocks are
    many tiles with a partial last one; 1 .. 9 channels are a partial wave of rows, 67 and 257 a full workgroup of rows plus a
    few."""
    rng = np.random.default_rng(fs + n)
    r = Rig(gpu, n, fs)
    for k, nb in enumerate((1, 1, 2, 5, 37)):
        r.call(full_range(rng, n, nb), extra_stride=k & 1, out_extra=(k >> 1) & 1)
    r.check_state()
    r.close()


def test_the_same_48_blocks_in_four_splittings(gpu):
    rng = np.random.default_rng(48)
    n = 5
    audio = full_range(rng, n, 48)
    random_split = []
    while sum(random_split) < 48:
        random_split.append(int(min(rng.integers(1, 12), 48 - sum(random_split))))
    rows = []
    for sizes in ([1] * 48, [8] * 6, [48], random_split):
        r = Rig(gpu, n, 12000)
        parts, b = [], 0
        for size in sizes:
            parts.append(r.call(audio[:, b:b + size]))
            b += size
        rows.append(np.concatenate(parts, axis=1))              # the reference's rows, which every call was held to
        r.check_state()
        r.close()
    assert all(np.array_equal(rows[0], x) for x in rows[1:])


# ---- custom filters
def test_identity(gpu):
    rng = np.random.default_rng(1)
    r = Rig(gpu, 3, custom=(1, 1, [16384], 14))
    audio = full_range(rng, 3, 4)
    want = r.call(audio)
    assert np.array_equal(want, audio.reshape(3, -1))
    r44 = Rig(gpu, 3, 44100)                                   # the default at 44.1 kHz is that filter
    assert np.array_equal(r44.call(audio), audio.reshape(3, -1))
    r.close(); r44.close()


@pytest.mark.parametrize("up,down,K,shift", [(1, 7, 1, 0), (1, 7, 255, 15), (3, 4, 256, 15), (3, 4, 1, 15), (3, 4, 255, 0), (1, 1, 256, 15),
                                             (512, 8192, 2, 15), (257, 300, 3, 6), (1, 16, 5, 15), (512, 512, 4, 15), (1, 16, 256, 15),
                                             (512, 8192, 256, 0)])
def test_custom_filters_at_the_ends_of_the_ranges(gpu, up, down, K, shift):
    """K = 1, 255 and 256 (odd, even, and the longest reach behind a call); U = 1 / M = 7 and U = 3 / M = 4; shifts 0 and 15; the
    corners of the accepted rates (M = 16 U with K = 256: the longest windows and the shortest tiles, 13 outputs)."""
    rng = np.random.default_rng(up * 1000 + K)
    bound = min(32767, 65535 // K)
    taps = rng.integers(-bound, bound + 1, size=up * K).astype(np.int16)
    assert RR.accepted(up, down, taps, shift)
    r = Rig(gpu, 9, custom=(up, down, taps, shift))
    for nb in (1, 2, 7):
        r.call(full_range(rng, 9, nb), extra_stride=1, out_extra=3)
    r.check_state()
    r.close()


@pytest.mark.parametrize("shift", [0, 15])
def test_the_int32_edge_and_both_clamps(gpu, shift):
    """One phase with sum |h| = 65535, every tap negative.  A stretch of -32768 gives the largest sum a filter can reach,
    65535 * 32768 = 2^31 - 32768: with the rounding constant 16384 still below 2^31.  A stretch of +32767 gives
    -65535 * 32767.  Both clamps are reached, and the test says so."""
    up, down, K = 1, 2, 256
    taps = np.full(K, -255, dtype=np.int16)
    taps[0] = -510                                             # 255 * 255 + 510 = 65535
    assert int(np.abs(taps.astype(int)).sum()) == 65535 and RR.accepted(up, down, taps, shift)
    audio = np.empty((2, 6, 128), dtype=np.int16)
    audio[0, :3], audio[0, 3:] = -32768, 32767
    audio[1, :3], audio[1, 3:] = 32767, -32768
    r = Rig(gpu, 2, custom=(up, down, taps, shift))
    want = r.call(audio, extra_stride=1)
    assert r.ref.acc_range == (-65535 * 32767, 65535 * 32768)
    assert want.max() == 32767 and want.min() == -32768
    r.close()


# ---- strides and guards
@pytest.mark.parametrize("nb,extra,out_extra", [(1, 5, 1), (3, 1, 7), (9, 2, 128)])
def test_strides_and_guard_samples(gpu, nb, extra, out_extra):
    """stride_blocks > n_blocks with gap blocks of 0x7FFF that no output may see, out_stride > count with a pattern behind every
    row and behind the last row that must survive (Rig.call asserts both)."""
    rng = np.random.default_rng(nb)
    r = Rig(gpu, 11, 8000)
    r.call(full_range(rng, 11, nb), extra_stride=extra, out_extra=out_extra)
    r.call(full_range(rng, 11, nb), extra_stride=extra, out_extra=out_extra)
    r.check_state()
    r.close()


def test_update_device_refusals_change_nothing(gpu):
    import torch
    r = Rig(gpu, 10)
    d = torch.zeros((10, 4, 128), dtype=torch.int16, device="cuda")
    o = torch.zeros((10, 256), dtype=torch.int16, device="cuda")
    i = torch.zeros(10, dtype=torch.int32, device="cuda")
    ok = dict(ptr=d.data_ptr(), n_blocks=2, out_ptr=o.data_ptr(), out_stride=256, stride_blocks=4)
    for kw, why in ((dict(ptr=d.data_ptr() + 2), "16-byte"), (dict(stride_blocks=1), "stride"), (dict(n_blocks=65536, stride_blocks=65536), "n_blocks"),
                    (dict(ptr=0), "null"), (dict(out_ptr=0), "null"), (dict(out_ptr=o.data_ptr() + 1), "2-byte"), (dict(out_stride=69), "output row stride"),
                    (dict(out_ptr=d.data_ptr() + 512), "overlaps"), (dict(index_ptr=i.data_ptr(), capacity_rows=3), "count"),
                    (dict(index_ptr=i.data_ptr(), count_ptr=i.data_ptr(), capacity_rows=-1), "negative")):
        with pytest.raises(gpu.AsdrError, match=why):
            r.rs.update_device(**dict(ok, **kw))
    assert r.rs.update_device(**dict(ok, n_blocks=0)) == 0     # no blocks: nothing happens
    assert r.rs.position() == 0
    r.check_state()
    r.close()


# ---- the index form
@pytest.mark.parametrize("nb", [1, 9])
def test_index_form_counts_and_capacity(gpu, nb):
    """count 0, count = n, a random third, and capacity_rows below the count: rows past min(count, capacity_rows) stay untouched
    and every channel's carry advances (each later call is held to the reference, which never skipped a channel)."""
    rng = np.random.default_rng(60 + nb)
    n = 40
    r = Rig(gpu, n, 12000)
    third = np.sort(rng.permutation(n)[:n // 3]).astype(np.int32)
    for index, count, capacity in (([0] * n, 0, n), (list(range(n)), n, n), (third, len(third), n), (third, len(third), 5),
                                   (list(range(n - 1, -1, -1)), n, n), (list(range(n)), n, 0)):
        r.call(full_range(rng, n, nb), index=index, count=count, capacity=capacity, out_extra=2)
    r.check_state()
    r.close()


def test_a_channel_undelivered_for_five_calls_has_its_history(gpu):
    rng = np.random.default_rng(65)
    n = 12
    r = Rig(gpu, n, 12000)
    others = [c for c in range(n) if c != 4]
    for _ in range(5):
        r.call(full_range(rng, n, 1), index=others, count=len(others), capacity=n)
    want = r.call(full_range(rng, n, 1), index=[4], count=1, capacity=n)    # held to the rig's reference, which never stopped
    assert want.shape[1] in (34, 35) and np.abs(want[4].astype(int)).max() > 1000
    r.check_state()
    r.close()


def test_behind_a_real_gate_on_one_stream(gpu):
    """Gate and resampler on one stream, no host step between them: the rows written are the reference rows of exactly
    index[0 .. count).  A third of the channels is loud."""
    import torch
    rng = np.random.default_rng(70)
    n, nb = 300, 2
    audio = rng.integers(-20, 21, size=(n, nb, 128)).astype(np.int16)
    loud = np.sort(rng.permutation(n)[:n // 3])
    audio[loud] = rng.integers(-20000, 20001, size=(len(loud), nb, 128)).astype(np.int16)
    thr = 128 * 2000 * 2000
    gate, gref = gpu.AudioGate(n), GR.GateRef(n)
    gate.set_squelch(energies=(thr, thr), hang_blocks=0); gref.set_squelch(thr, thr, 0)
    want_index = gref.update(audio)[0]
    assert np.array_equal(want_index, loud)
    r = Rig(gpu, n, 12000)
    want = r.ref.update(audio)
    count = want.shape[1]
    s = torch.cuda.Stream()
    d_audio = torch.from_numpy(audio).cuda()
    d_out = torch.full((n, count + 3), PATTERN, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    gate.update_device(d_audio.data_ptr(), nb, stream=s.cuda_stream)
    got = r.rs.update_device(d_audio.data_ptr(), nb, d_out.data_ptr(), count + 3, index_ptr=gate.index_tensor().data_ptr(),
                             count_ptr=gate.count_tensor().data_ptr(), capacity_rows=n, stream=s.cuda_stream)
    s.synchronize()
    out = d_out.cpu().numpy()
    assert got == count and int(gate.count_tensor().cpu()[0]) == len(loud)
    assert np.array_equal(out[:len(loud), :count], want[loud])
    assert (out[len(loud):] == PATTERN).all() and (out[:, count:] == PATTERN).all()
    r.check_state()
    gate.close(); r.close()


# ---- positions
@pytest.mark.parametrize("fs", [12000, 8000])
@pytest.mark.parametrize("n0", [2**31 - 384, 2**32 - 384, 2**40 + 5 * 128])
def test_large_positions(gpu, fs, n0):
    """set_position + write_state place the resampler three blocks before 2^31 and 2^32, and past 2^40; the reference stands at the
    same N with the same history.  The next six calls cross the power of two."""
    rng = np.random.default_rng(n0 % 1000 + fs)
    n = 9
    r = Rig(gpu, n, fs)
    r.place(n0, rng.integers(-32768, 32768, size=(n, 256)).astype(np.int16))
    assert r.rs.position() == n0 and r.rs.output_position() == RR.ceil_div(n0 * r.ref.up, r.ref.down)
    for nb in (1, 1, 1, 2, 1, 9):
        r.call(full_range(rng, n, nb))
    assert r.rs.position() == n0 + 15 * 128
    r.check_state()
    r.close()


# ---- state
def test_records_move_between_resamplers(gpu):
    """Read after 9 blocks, written into a second 12 kHz resampler placed at the same N and into an 8 kHz one: each continues
    bit for bit as a reference that never stopped.  Then reset."""
    rng = np.random.default_rng(80)
    n = 6
    a = Rig(gpu, n, 12000)
    first, rest = full_range(rng, n, 9), full_range(rng, n, 4)
    a.call(first[:, :4]); a.call(first[:, 4:])
    rec = a.rs.read_state()
    assert np.array_equal(rec, first.reshape(n, -1)[:, -256:])
    b = Rig(gpu, n, 12000)
    b.place(a.rs.position(), rec)
    got_b = b.call(rest)
    assert np.array_equal(got_b, a.call(rest))                 # a goes on uninterrupted
    c = Rig(gpu, n + 2, 8000)                                  # another rate, other channels, its own N
    c.call(full_range(rng, n + 2, 3))
    chans = [7, 0, 3, 2, 5, 1]
    c.rs.write_state(rec, channels=chans); c.ref.state[chans] = rec
    c.call(full_range(rng, n + 2, 2))
    c.check_state()
    with pytest.raises(gpu.AsdrError, match="bad channel"):
        c.rs.write_state(rec, channels=[0, 1, 2, 3, 4, 8])
    c.check_state()
    c.rs.reset(); c.ref.reset()
    assert c.rs.position() == 0 and not c.rs.read_state().any()
    c.call(full_range(rng, n + 2, 1))
    c.check_state()
    a.close(); b.close(); c.close()


def test_set_filter_between_calls(gpu):
    rng = np.random.default_rng(81)
    n = 4
    r = Rig(gpu, n, 12000)
    r.call(full_range(rng, n, 2))
    K = 31
    taps = rng.integers(-1000, 1001, size=40 * K).astype(np.int16)
    r.set_filter(taps, 12)
    r.call(full_range(rng, n, 3))
    r.set_filter(*RR.default_filter(12000))
    r.call(full_range(rng, n, 1))
    r.check_state()
    r.close()


# ---- streams
def test_two_streams_without_host_synchronisation(gpu):
    """Two consecutive calls on different streams with no host synchronisation between them equal the same calls on one
    stream: the second call's history is the first call's carry, so it must have waited on the device."""
    import torch
    rng = np.random.default_rng(90)
    n, nb = 3000, 1
    audio = full_range(rng, n, 2 * nb)
    d_audio = torch.from_numpy(audio).cuda()
    ref = None
    results = []
    for streams in ((torch.cuda.Stream(), torch.cuda.Stream()), (torch.cuda.Stream(),) * 2):
        rs = gpu.AudioResampler(n, fs_out=12000)
        if ref is None:
            ref = RR.ResampleRef(n, rs.up, rs.down, *rs.get_taps())
            want = [ref.update(audio[:, :nb]), ref.update(audio[:, nb:])]
        outs = [torch.full((n, 40), PATTERN, dtype=torch.int16, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        counts = [rs.update_device(d_audio[:, k * nb:].data_ptr(), nb, outs[k].data_ptr(), 40, stride_blocks=2 * nb, stream=streams[k].cuda_stream)
                  for k in range(2)]
        rs.synchronize()
        torch.cuda.synchronize()
        results.append([o.cpu().numpy() for o in outs])
        for k in range(2):
            assert counts[k] == want[k].shape[1] and np.array_equal(results[-1][k][:, :counts[k]], want[k])
        assert np.array_equal(rs.read_state(), ref.state)
        rs.close()
    assert all(np.array_equal(x, y) for x, y in zip(*results))


# ---- size edges
@pytest.mark.parametrize("n,nb", [(65536, 1), (512, 646)])
def test_size_edges(gpu, n, nb):
    """A C2 step's audio (65,536 x 1 block) and a capture-sink call (512 x 646 blocks), each compared on 16 channels spread over
    the range, the last included; two calls, so that the second starts from the first's carry."""
    import torch
    rng = np.random.default_rng(n)
    chans = np.unique(np.concatenate([np.linspace(0, n - 1, 15).astype(np.int64), [n - 1, n - 2]]))[-16:]
    rs = gpu.AudioResampler(n, fs_out=12000)
    ref = RR.ResampleRef(len(chans), rs.up, rs.down, *rs.get_taps())
    for call in range(2):
        audio = full_range(rng, n, nb)
        d_audio = torch.from_numpy(audio).cuda()
        count = rs.out_samples(nb)
        d_out = torch.full((n, count + 1), PATTERN, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        assert rs.update_device(d_audio.data_ptr(), nb, d_out.data_ptr(), count + 1) == count
        torch.cuda.synchronize()
        want = ref.update(audio[chans])
        got = d_out[torch.from_numpy(chans).cuda()].cpu().numpy()
        assert want.shape[1] == count and np.array_equal(got[:, :count], want) and (got[:, count] == PATTERN).all()
        assert bool((d_out[:, count] == PATTERN).all())
    assert np.array_equal(rs.read_state()[chans], ref.state)
    rs.close()


# ---- end to end
def test_end_to_end_behind_the_chain_and_the_capture_sink(gpu, ao):
    """16 USB receivers (AGC on, no blanker), 24 blocks, chain and resampler on one stream in two calls of 12 blocks; the rows
    equal resample_ref applied to the oracle's audio.  The same 24 blocks through a capture sink's device pointer with
    stride_blocks = capacity."""
    import torch
    from audiosdr_amd.synth import make_iq
    n, nb = 16, 24
    I, Q = make_iq(n, nb, fc=6290.0, A=np.linspace(0.02, 0.3, n), noise=0.001)
    orcs = [ao.OracleSDR() for _ in range(n)]
    for o in orcs:
        o.setDemodMode(1); o.disableNoiseBlanker()
    oracle_audio = np.stack([orcs[c].update(I[c], Q[c]).reshape(nb, 128) for c in range(n)])
    assert np.abs(oracle_audio).max() > 1000
    taps, shift = RR.default_filter(12000)
    ref = RR.ResampleRef(n, 40, 147, taps, shift)
    want = [ref.update(oracle_audio[:, :12]), ref.update(oracle_audio[:, 12:])]
    whole = RR.ResampleRef(n, 40, 147, taps, shift).update(oracle_audio)
    assert np.array_equal(np.concatenate(want, axis=1), whole)

    s = torch.cuda.Stream()
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    batch = gpu.AudioSDRBatch(n)
    batch.setDemodMode(1); batch.disableNoiseBlanker()
    rs = gpu.AudioResampler(n, fs_out=12000)
    assert np.array_equal(rs.get_taps()[0], taps)
    d_audio = torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda")
    stride = whole.shape[1] + 8
    d_out = torch.full((2, n, stride), PATTERN, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    counts = []
    for k, a in enumerate((0, 12)):
        batch.update_device_strided(dI[:, a:].data_ptr(), dQ[:, a:].data_ptr(), d_audio[:, a:].data_ptr(), 12, nb, nb, stream=s.cuda_stream)
        counts.append(rs.update_device(d_audio[:, a:].data_ptr(), 12, d_out[k].data_ptr(), stride, stride_blocks=nb, stream=s.cuda_stream))
    s.synchronize()
    assert np.array_equal(d_audio.cpu().numpy(), oracle_audio)
    for k in range(2):
        got = d_out[k].cpu().numpy()
        assert counts[k] == want[k].shape[1] and np.array_equal(got[:, :counts[k]], want[k]) and (got[:, counts[k]:] == PATTERN).all()
    rs.close(); batch.close()

    sink = gpu.AudioSDRBatch(n)                                 # the capture sink's rows, stride_blocks = capacity
    sink.setDemodMode(1); sink.disableNoiseBlanker()
    sink.capture_open(nb + 5)
    rs = gpu.AudioResampler(n, fs_out=12000)
    d_one = torch.full((n, stride), PATTERN, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    sink.capture_update_device(dI.data_ptr(), dQ.data_ptr(), nb, stream=s.cuda_stream)
    assert sink.capture_capacity == nb + 5
    count = rs.update_device(sink.capture_device_ptr(), nb, d_one.data_ptr(), stride, stride_blocks=sink.capture_capacity, stream=s.cuda_stream)
    s.synchronize()
    got = d_one.cpu().numpy()
    assert count == whole.shape[1] and np.array_equal(got[:, :count], whole) and (got[:, count:] == PATTERN).all()
    rs.close(); sink.capture_close(); sink.close()
