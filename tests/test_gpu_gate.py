"""The audio gate on the GPU (include/asdr_gate.h; audiosdr_amd/csrc/asdr_gate.hip) against tests/gate_ref.py at tolerance 0: the
state records, count, index and the packet's bytes, over partial waves and tiles, strides, the arithmetic's extremes, every
threshold seam, the shapes of the list, streams, the state calls, and end to end behind the chain on the oracle's audio.
The sizes are the smallest that reach each seam (ASDR_GATE_TILE = 256 channels per workgroup and per tile of the index step, 8
channels per row of lanes, 64 per wave; the index step's offset loop takes a second turn past 256 tiles)."""
import numpy as np
import pytest

import gate_ref as GR

pytestmark = pytest.mark.gpu
GAP = 0x7FFF        # fills the stride gaps: must not count
PATTERN = 0x5A5B    # pre-fills the packet buffer: must stay where nothing is delivered


class Rig:
    """A gate and its reference side by side; call() runs one update on both and compares everything."""

    def __init__(self, A, n, settings=None):
        import torch
        self.torch, self.A, self.n = torch, A, n
        self.gate, self.ref = A.AudioGate(n), GR.GateRef(n)
        for ch, (o, c, h) in (settings or {}).items():
            self.set(o, c, h, ch)

    def set(self, o, c, h, ch=-1):
        self.gate.set_squelch(energies=(o, c), hang_blocks=h, ch=ch)
        self.ref.set_squelch(o, c, h, ch)

    def call(self, audio, extra_stride=0, capacity=None, stream=None, packet=True):
        """audio int16 [n][nb][128].  Returns the reference's (index, packet, opens)."""
        torch = self.torch
        n, nb = audio.shape[:2]
        padded = np.full((n, nb + extra_stride, 128), GAP, dtype=np.int16)
        padded[:, :nb] = audio
        cap = n if capacity is None else capacity
        d_audio = torch.from_numpy(padded).cuda()
        d_rows = torch.full((max(cap, 1) + 1, nb, 128), PATTERN, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        self.gate.update_device(d_audio.data_ptr(), nb, stride_blocks=nb + extra_stride, rows_ptr=d_rows.data_ptr() if packet else 0,
                                capacity_rows=cap if packet else 0, stream=stream.cuda_stream if stream is not None else 0)
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        want_index, want_rows, opens = self.ref.update(padded, n_blocks=nb, capacity_rows=cap)
        count = int(self.gate.count_tensor().cpu()[0])
        assert count == len(want_index), (count, len(want_index))
        assert np.array_equal(self.gate.index_tensor().cpu().numpy()[:count], want_index)
        rows = d_rows.cpu().numpy()
        k = len(want_rows) if packet else 0
        assert np.array_equal(rows[:k], want_rows[:k])
        assert (rows[k:] == PATTERN).all(), "the packet buffer is written past min(count, capacity_rows) rows"
        assert np.array_equal(d_audio.cpu().numpy(), padded)
        self.check_state()
        return want_index, want_rows, opens

    def check_state(self):
        assert GR.record_tuples(self.gate.read_state()) == self.ref.state_tuples()
        assert self.gate.blocks() == self.ref.blocks

    def close(self):
        self.gate.close()


def mixed_rows(rng, n, nb):
    """Random rows over the whole range of levels: full range shifted down by 0 .. 15 bits per block, a quarter of the blocks 0."""
    a = (rng.integers(-32768, 32768, size=(n, nb, 128)) >> rng.integers(0, 16, size=(n, nb, 1))).astype(np.int16)
    a[rng.random((n, nb)) < 0.25] = 0
    return a


def median_threshold(audio, q=0.5):
    """The q-quantile (the median) of the nonzero block energies: a threshold that some blocks cross and some do not."""
    E = GR.block_energy_peak(audio)[0]
    return int(np.quantile(E[E > 0].astype(np.float64), q))


# ---- partial waves and tiles
@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 65, 255, 256, 257, 511, 513, 4097, 65536 + 257])
def test_partial_waves_and_tiles(gpu, n):
    """One more and one less than the lanes of a channel group (8), a wave (64) and a tile (gpu.GATE_TILE = 256); 17 tiles; and 258
    tiles, where a workgroup of the index step adds more than 256 tile counts.  A one-block call (the fused form), then a
    three-block call (energy, fold) on the same gate."""
    assert gpu.GATE_TILE == 256
    rng = np.random.default_rng(n)
    r = Rig(gpu, n)
    a1, a3 = mixed_rows(rng, n, 1), mixed_rows(rng, n, 3)
    thr = median_threshold(np.concatenate([a1, a3], axis=1))
    r.set(thr, thr // 4, 1)
    i1 = r.call(a1)[0]
    i3 = r.call(a3)[0]
    if n >= 63:
        assert 0 < len(i1) < n and 0 < len(i3) < n
    r.close()


# ---- blocks and strides
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("nb", [1, 2, 3, 17])
def test_blocks_and_strides(gpu, nb, extra):
    rng = np.random.default_rng(100 + nb)
    n = 37
    r = Rig(gpu, n)
    audio = mixed_rows(rng, n, nb)
    thr = median_threshold(audio, 0.5 if nb < 4 else 0.9)      # 17 blocks: few channels have none above the median
    assert thr < 128 * GAP * GAP                               # a gap block would open every gate
    r.set(thr, thr // 2, 1)
    index = r.call(audio, extra_stride=extra)[0]
    assert 0 < len(index) < n
    assert all(p < GAP or (audio[c] == GAP).any() for c, p in enumerate(r.ref.st["peak"].tolist()))
    r.call(mixed_rows(rng, n, nb), extra_stride=extra, capacity=5)
    r.close()


@pytest.mark.parametrize("nb", [8, 9, 16, 27, 48])
def test_the_folds_batches(gpu, nb):
    """The fold step reads the scratch 16 blocks at a time, then 8 at a time, then a partial batch of up to 7: one batch of 8
    exactly, 8 + 1, one of 16 exactly, 16 + 8 + 3, and three of 16."""
    rng = np.random.default_rng(200 + nb)
    n = 70
    r = Rig(gpu, n)
    audio = mixed_rows(rng, n, nb)
    thr = median_threshold(audio, 0.8)
    r.set(thr, thr // 3, 2)
    opens = r.call(audio, extra_stride=1)[2]
    assert 0 < opens.sum() < opens.size and r.ref.st["openings"].max() >= 2
    r.close()


# ---- arithmetic
def test_rows_of_minus_32768(gpu):
    """E = 2^37 per block: nine of them, as calls of 1 and 8 blocks.  16 such squares exceed 32 bits."""
    r = Rig(gpu, 9)
    r.call(np.full((9, 1, 128), -32768, dtype=np.int16))
    r.call(np.full((9, 8, 128), -32768, dtype=np.int16), extra_stride=1)
    st = r.gate.read_state()
    assert (st["energy"] == 9 << 37).all() and (st["last_energy"] == 1 << 37).all() and (st["peak"] == 32768).all()
    assert (st["open_blocks"] == 9).all() and (st["openings"] == 1).all()
    r.close()


def test_rows_of_zero(gpu):
    r = Rig(gpu, 20)
    r.set(1, 1, 0)
    index = r.call(np.zeros((20, 2, 128), dtype=np.int16), extra_stride=2)[0]
    assert len(index) == 0
    r.set(0, 0, 0)                                             # E = 0 >= 0: open
    assert len(r.call(np.zeros((20, 1, 128), dtype=np.int16))[0]) == 20
    r.close()


@pytest.mark.parametrize("nb", [1, 2])
def test_a_single_one_at_each_position(gpu, nb):
    """Channel 2 k + s has (-1)^s at position k of its last block and nothing else: E = 1 and P = 1 for each, so a skipped or a
    doubled piece shows."""
    audio = np.zeros((256, nb, 128), dtype=np.int16)
    for k in range(128):
        audio[2 * k, nb - 1, k], audio[2 * k + 1, nb - 1, k] = 1, -1
    r = Rig(gpu, 256)
    r.set(1, 1, 0)
    index = r.call(audio)[0]
    st = r.gate.read_state()
    assert len(index) == 256 and (st["energy"] == 1).all() and (st["peak"] == 1).all() and (st["open_blocks"] == 1).all()
    r.set(2, 2, 0)
    assert len(r.call(audio)[0]) == 0
    r.close()


def test_random_full_range_rows(gpu):
    rng = np.random.default_rng(7)
    n = 70
    audio = rng.integers(-32768, 32768, size=(n, 5, 128)).astype(np.int16)
    r = Rig(gpu, n)
    thr = median_threshold(audio)
    r.set(thr, thr - 1, 0)
    index = r.call(audio, extra_stride=3)[0]
    assert 0 < len(index) <= n and (r.gate.read_state()["energy"] > 1 << 36).all()
    r.call(audio[:, :1])
    r.close()


def test_the_energy_sum_wraps(gpu):
    r = Rig(gpu, 3)
    rec = np.zeros(3, dtype=gpu.GATE_STATE_DTYPE)
    rec["energy"] = 2**64 - 5
    r.gate.write_state(rec)
    r.ref.st["energy"][:] = 2**64 - 5
    r.call(GR.rows_with_energy([3, 5, 1 << 37]).reshape(3, 1, 128))
    assert r.gate.read_state()["energy"].tolist() == [2**64 - 2, 0, (1 << 37) - 5]
    r.call(GR.rows_with_energy([3, 5, 7, 9, 11, 13]).reshape(3, 2, 128))
    r.close()


# ---- thresholds
OPEN, CLOSE = 1_000_003, 40_001


def level_rows(levels):
    """levels [n][nb] of block energies -> int16 [n][nb][128] with exactly those energies."""
    levels = np.asarray(levels, dtype=object)
    rows = GR.rows_with_energy(levels.reshape(-1).tolist(), rng=np.random.default_rng(3))
    assert GR.block_energy_peak(rows)[0].tolist() == [int(v) for v in levels.reshape(-1)]
    return rows.reshape(levels.shape + (128,))


def test_energies_exactly_at_the_thresholds(gpu):
    """A block at open_energy opens, one below does not; an open gate with hang 0 holds at close_energy and closes one below."""
    seqs = [[OPEN, CLOSE, CLOSE - 1, 0],                       # 1 1 0 0
            [OPEN - 1, OPEN, CLOSE, CLOSE],                    # 0 1 1 1
            [OPEN - 1, CLOSE, OPEN - 1, 0],                    # 0 0 0 0
            [OPEN, CLOSE - 1, OPEN, CLOSE - 1],                # 1 0 1 0
            [CLOSE - 1, CLOSE, OPEN - 1, OPEN]]                # 0 0 0 1
    want = [[1, 1, 0, 0], [0, 1, 1, 1], [0, 0, 0, 0], [1, 0, 1, 0], [0, 0, 0, 1]]
    audio = level_rows(seqs)
    for cuts in ([0, 4], [0, 1, 2, 3, 4], [0, 3, 4]):
        r = Rig(gpu, 5)
        r.set(OPEN, CLOSE, 0)
        opens = np.concatenate([r.call(audio[:, a:b])[2] for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
        assert opens.tolist() == want
        assert r.gate.read_state()["openings"].tolist() == [1, 1, 0, 2, 1]
        r.close()


@pytest.mark.parametrize("nb", [1, 4])
def test_hang_values(gpu, nb):
    """hang_blocks 0, 1, n_blocks - 1, n_blocks and 65535, one per channel inside one wave: a loud block, then quiet calls of
    n_blocks blocks -- the hang runs out inside a call, exactly at a call's end, in the following call, or never."""
    hangs = [0, 1, max(nb - 1, 0), nb, 65535, 2 * nb, nb + 1]
    r = Rig(gpu, len(hangs), {c: (OPEN, CLOSE, h) for c, h in enumerate(hangs)})
    loud = level_rows([[OPEN]] * len(hangs))
    quiet = level_rows([[CLOSE - 1] * nb] * len(hangs))
    r.call(loud)
    seen = []
    for _ in range(4):
        index, _, opens = r.call(quiet)
        seen.append(opens)
    opens = np.concatenate(seen, axis=1)
    for c, h in enumerate(hangs):                              # open for exactly min(h, all) quiet blocks
        assert int(opens[c].sum()) == min(h, 4 * nb) and (np.diff(opens[c].astype(int)) <= 0).all(), (c, h)
    st = r.gate.read_state()
    assert int(st["hang_left"][4]) == 65535 - 4 * nb and int(st["open"][4]) == 1
    r.close()


def test_the_same_24_blocks_as_calls_of_1_2_3_and_24(gpu):
    rng = np.random.default_rng(24)
    n = 19
    audio = mixed_rows(rng, n, 24)
    thr = median_threshold(audio)
    states = []
    for size in (1, 2, 3, 24):
        r = Rig(gpu, n)
        r.set(thr, thr // 8, 2)
        r.set(thr // 2, thr // 2, 0, ch=3)
        for a in range(0, 24, size):
            r.call(audio[:, a:a + size], extra_stride=size & 1)
        states.append(r.gate.read_state().tobytes())
        r.close()
    assert states[0] == states[1] == states[2] == states[3]


# ---- lists
def list_case(gpu, n, open_channels, nb=2, capacity=None):
    audio = np.zeros((n, nb, 128), dtype=np.int16)
    audio[:, :, 5] = 3                                         # E = 9 everywhere
    for c in open_channels:
        audio[c, nb - 1, 7] = 100                              # E = 10009 in the last block
    r = Rig(gpu, n)
    r.set(10009, 10009, 0)
    index, rows, _ = r.call(audio, capacity=capacity)
    assert index.tolist() == sorted(open_channels)
    return r, audio


def test_list_none_open(gpu):
    r, audio = list_case(gpu, 300, [])
    d_audio = r.torch.from_numpy(audio).cuda()
    index, rows = r.gate.deliver(d_audio.data_ptr(), 2)
    r.ref.update(audio)
    assert index.shape == (0,) and rows.shape == (0, 2, 128)
    r.check_state()
    r.close()


@pytest.mark.parametrize("which", ["all", "first", "last", "every_second", "every_second_odd"])
def test_list_shapes(gpu, which):
    n = 300
    chans = {"all": list(range(n)), "first": [0], "last": [n - 1], "every_second": list(range(0, n, 2)),
             "every_second_odd": list(range(1, n, 2))}[which]
    r, audio = list_case(gpu, n, chans)
    d_audio = r.torch.from_numpy(audio).cuda()                 # the same through the host entry
    index, rows = r.gate.deliver(d_audio.data_ptr(), 2)
    want_index, want_rows, _ = r.ref.update(audio)
    assert np.array_equal(index, want_index) and np.array_equal(rows, want_rows) and len(index) == len(chans)
    out = np.full((n + 1, 2, 128), PATTERN, dtype=np.int16)    # and into the caller's array
    index, rows = r.gate.deliver(d_audio.data_ptr(), 2, rows_out=out)
    r.ref.update(audio)
    assert np.array_equal(index, want_index) and np.array_equal(out[:len(chans)], want_rows) and (out[len(chans):] == PATTERN).all()
    assert rows.base is not None and np.shares_memory(rows, out)
    with pytest.raises(gpu.AsdrError, match="rows_out"):
        r.gate.deliver(d_audio.data_ptr(), 2, rows_out=out[:5])
    r.check_state()
    r.close()


def test_different_settings_per_channel_inside_one_wave(gpu):
    rng = np.random.default_rng(12)
    n = 64
    audio = mixed_rows(rng, n, 6)
    thr = median_threshold(audio)
    r = Rig(gpu, n, {c: (thr >> (c % 5), thr >> (c % 5 + c % 3), c % 4) for c in range(n)})
    index = r.call(audio)[0]
    assert 0 < len(index) < n
    assert len({tuple(s) for s in r.ref.settings}) > 8
    r.call(audio[:, :1])
    r.close()


@pytest.mark.parametrize("nb", [1, 3, 17])
def test_capacity_below_count(gpu, nb):
    """The first capacity_rows rows are written and nothing after them; index and the count are complete.  17 blocks make a row of
    272 pieces: more than one workgroup of the packet step per row."""
    n, cap = 300, 37
    chans = list(range(3, n, 2))
    r, audio = list_case(gpu, n, chans, nb=nb, capacity=cap)
    d_audio = r.torch.from_numpy(audio).cuda()
    L, C = r.gate._L, gpu.gate.C
    host_index = np.full(n, -1, dtype=np.int32)
    host_rows = np.full((cap + 2, nb, 128), PATTERN, dtype=np.int16)
    n_open = C.c_int(-1)
    got = L.asdr_gate_deliver(r.gate._h, C.c_void_p(d_audio.data_ptr()), nb, nb, host_index.ctypes.data_as(C.c_void_p),
                              host_rows.ctypes.data_as(C.c_void_p), cap, C.byref(n_open))
    want_index, want_rows, _ = r.ref.update(audio, capacity_rows=cap)
    assert got == cap and n_open.value == len(chans) == len(want_index)
    assert np.array_equal(host_index[:len(chans)], want_index) and (host_index[len(chans):] == -1).all()
    assert np.array_equal(host_rows[:cap], want_rows) and (host_rows[cap:] == PATTERN).all()
    index, rows = r.gate.deliver(d_audio.data_ptr(), nb, capacity_rows=0)
    r.ref.update(audio)
    assert len(index) == len(chans) and rows.shape[0] == 0
    r.check_state()
    r.close()


def test_deliver_grows_its_kept_buffers_and_reuses_them(gpu):
    """deliver's packet buffer and the scratch of block energies are kept between calls: a call of 1 block, one of 4 blocks that
    needs both larger, one of 2 blocks that fits what the second left.  All 3 channels are open (the default squelch), so the packet
    is 3 n_blocks rows of 256 bytes each time; every call's index and rows are the reference's."""
    rng = np.random.default_rng(31)
    r = Rig(gpu, 3)
    for nb in (1, 4, 2):
        audio = mixed_rows(rng, 3, nb)
        d_audio = r.torch.from_numpy(audio).cuda()
        index, rows = r.gate.deliver(d_audio.data_ptr(), nb)
        want_index, want_rows, _ = r.ref.update(audio)
        assert want_index.tolist() == [0, 1, 2] and want_rows.shape == (3, nb, 128)
        assert np.array_equal(index, want_index) and np.array_equal(rows, want_rows)
        r.check_state()
    r.close()


def test_update_device_refusals_change_nothing(gpu):
    import torch
    r = Rig(gpu, 10)
    d = torch.zeros((10, 4, 128), dtype=torch.int16, device="cuda")
    for kw, why in ((dict(ptr=d.data_ptr() + 2, n_blocks=1), "16-byte"), (dict(ptr=d.data_ptr(), n_blocks=3, stride_blocks=2), "stride"),
                    (dict(ptr=d.data_ptr(), n_blocks=65536, stride_blocks=65536), "n_blocks"), (dict(ptr=0, n_blocks=1), "null"),
                    (dict(ptr=d.data_ptr(), n_blocks=2, stride_blocks=4, rows_ptr=d.data_ptr() + 256, capacity_rows=1), "overlaps"),
                    (dict(ptr=d.data_ptr(), n_blocks=1, stride_blocks=4, capacity_rows=-1, rows_ptr=d.data_ptr()), "negative")):
        with pytest.raises(gpu.AsdrError, match=why):
            r.gate.update_device(**kw)
    r.gate.update_device(d.data_ptr(), 0, stride_blocks=4)      # no blocks: nothing happens
    r.check_state()
    r.close()


# ---- streams
def test_null_stream_and_a_callers_stream(gpu):
    import torch
    rng = np.random.default_rng(31)
    n = 130
    audio = mixed_rows(rng, n, 4)
    thr = median_threshold(audio)
    r = Rig(gpu, n)
    r.set(thr, thr // 2, 1)
    s = torch.cuda.Stream()
    r.call(audio[:, :2])
    r.call(audio[:, 2:], stream=s)
    r.call(audio[:, :1], stream=s)
    r.call(audio[:, 1:])
    r.close()


def test_consecutive_calls_on_two_streams_see_each_others_state(gpu):
    """Twelve one- and two-block calls alternate between two streams with no host synchronisation between them: each call's
    state is the previous call's, so the final records equal the reference's only if every call waited for the one before."""
    import torch
    rng = np.random.default_rng(32)
    n, nb = 1000, 18
    audio = mixed_rows(rng, n, nb)
    thr = median_threshold(audio)
    g, ref = gpu.AudioGate(n), GR.GateRef(n)
    g.set_squelch(energies=(thr, thr // 16), hang_blocks=2); ref.set_squelch(thr, thr // 16, 2)
    d_audio = torch.from_numpy(audio).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    b, k = 0, 0
    while b < nb:
        size = 1 + (k & 1)
        g.update_device(d_audio[:, b:].data_ptr(), size, stride_blocks=nb, stream=streams[k & 1].cuda_stream)
        index = ref.update(audio[:, b:b + size])[0]
        b += size; k += 1
    g.synchronize()
    torch.cuda.synchronize()
    assert GR.record_tuples(g.read_state()) == ref.state_tuples() and g.blocks() == nb
    count = int(g.count_tensor().cpu()[0])
    assert count == len(index) and np.array_equal(g.index_tensor().cpu().numpy()[:count], index)
    g.close()


# ---- state
def test_clear_and_reset(gpu):
    hangs = [0, 3, 9]
    r = Rig(gpu, 3, {c: (OPEN, CLOSE, h) for c, h in enumerate(hangs)})
    r.call(level_rows([[OPEN, CLOSE - 1]] * 3))
    assert r.gate.read_state()["open"].tolist() == [0, 1, 1] and r.gate.read_state()["hang_left"].tolist() == [0, 2, 8]
    r.gate.clear(); r.ref.clear()
    r.check_state()
    st = r.gate.read_state()
    assert st["open"].tolist() == [0, 1, 1] and st["hang_left"].tolist() == [0, 2, 8] and r.gate.blocks() == 0
    assert not st["energy"].any() and not st["peak"].any() and not st["openings"].any() and not st["open_blocks"].any()
    r.call(level_rows([[CLOSE - 1] * 3] * 3))                  # the hang goes on from where it was
    r.gate.reset(); r.ref.reset()
    r.check_state()
    assert r.gate.get_squelch(2) == (OPEN, CLOSE, 9) and not np.frombuffer(r.gate.read_state().tobytes(), dtype=np.uint8).any()
    r.call(level_rows([[OPEN, 0]] * 3))
    r.close()


def test_a_channel_mid_hang_moves_to_another_gate(gpu):
    """Channel 2 of a 5-channel gate, two blocks into a hang of 4, goes to channel 6 of a 9-channel gate with read_state /
    write_state and decides there as the uninterrupted reference does."""
    seq = [OPEN, CLOSE - 1, CLOSE - 1, CLOSE - 1, CLOSE - 1, CLOSE - 1, CLOSE - 1, OPEN, 0]
    a = Rig(gpu, 5)
    a.set(OPEN, CLOSE, 4)
    first = level_rows([[0] * 3] * 2 + [seq[:3]] + [[0] * 3] * 2)
    a.call(first)
    rec = a.gate.read_state()[2:3]
    assert int(rec["open"][0]) == 1 and int(rec["hang_left"][0]) == 2
    b = Rig(gpu, 9)
    b.set(OPEN, CLOSE, 4)
    b.gate.write_state(rec, channels=[6])
    b.ref.put(6, a.ref.state_tuples()[2])
    rest = level_rows([[0] * 6] * 6 + [seq[3:]] + [[0] * 6] * 2)
    index, _, opens = b.call(rest)
    assert opens[6].tolist() == [1, 1, 0, 0, 1, 1] and index.tolist() == [6]
    whole = GR.GateRef(1)                                      # the uninterrupted reference
    whole.set_squelch(OPEN, CLOSE, 4)
    whole.update(level_rows([seq]))
    assert GR.record_tuples(b.gate.read_state())[6] == whole.state_tuples()[0]
    with pytest.raises(gpu.AsdrError, match="open must be 0 or 1"):
        bad = rec.copy(); bad["open"] = 2
        b.gate.write_state(bad, channels=[0])
    b.check_state()
    a.close(); b.close()


# ---- end to end
E2E_OPEN_DB, E2E_CLOSE_DB, E2E_HANG = -34.0, -43.5, 2


def e2e_inputs():
    """24 receivers x 8 blocks: channels 0 mod 3 get the noise floor alone, 1 mod 3 a tone throughout, 2 mod 3 the tone in blocks
    3 and 4 only (amplitude 0.25 throughout, 0.02 for the bursts; noise 0.001)."""
    from audiosdr_amd.synth import make_iq
    n, nb = 24, 8
    kind = np.arange(n) % 3
    I, Q = make_iq(n, nb, fc=6290.0, A=np.choose(kind, [0.0, 0.25, 0.02]), noise=0.001)
    Is, Qs = make_iq(n, nb, fc=6290.0, A=0.0, noise=0.001)
    for b in (0, 1, 2, 5, 6, 7):
        I[kind == 2, b], Q[kind == 2, b] = Is[kind == 2, b], Qs[kind == 2, b]
    return I, Q


def test_end_to_end_behind_the_chain(gpu, ao):
    """USB with AGC (on by default), without the blanker (it delays the audio by two blocks); the burst receivers run the fast
    AGC.  With these levels the oracle's audio of a steady tone never falls below -42.9 dBFS, the block after a burst lies at
    -44.2 dBFS and the noise floor below -53 dBFS: thresholds of -34 / -43.5 dBFS with hang 2 give all three kinds of channel,
    which the test asserts on the oracle's audio before it looks at the GPU's."""
    import torch
    I, Q = e2e_inputs()
    n, nb = I.shape[:2]
    orcs = [ao.OracleSDR() for _ in range(n)]
    batch = gpu.AudioSDRBatch(n)
    batch.setDemodMode(1); batch.disableNoiseBlanker()
    for c, o in enumerate(orcs):
        o.setDemodMode(1); o.disableNoiseBlanker()
        if c % 3 == 2:
            o.setAGCmode(gpu.AGCfast); batch.setAGCmode(gpu.AGCfast, ch=c)
    oracle_audio = np.stack([orcs[c].update(I[c], Q[c]).reshape(nb, 128) for c in range(n)])
    o_e, c_e = gpu.energy_from_dbfs(E2E_OPEN_DB), gpu.energy_from_dbfs(E2E_CLOSE_DB)
    assert (o_e, c_e) == (GR.energy_from_dbfs(E2E_OPEN_DB), GR.energy_from_dbfs(E2E_CLOSE_DB))
    # the expectation, two calls of four blocks, from the oracle's audio; first that it holds all three kinds of channel
    ref = GR.GateRef(n)
    ref.set_squelch(o_e, c_e, E2E_HANG)
    want = [ref.update(oracle_audio[:, a:a + 4]) for a in (0, 4)]
    opens = np.concatenate([w[2] for w in want], axis=1)
    never = [c for c in range(n) if not opens[c].any()]
    always = [c for c in range(n) if all(c in w[0] for w in want)]
    d = np.diff(opens.astype(int), axis=1)
    open_close = [c for c in range(n) if opens[c, 0] == 0 and opens[c, -1] == 0 and (d[c] == 1).sum() == 1 and (d[c] == -1).sum() == 1]
    assert never == list(range(0, n, 3)) and always == list(range(1, n, 3)) and open_close == list(range(2, n, 3)), (never, always, open_close)
    # the product: chain and gate on one stream, no host step in between
    g = gpu.AudioGate(n)
    g.set_squelch(open_db=E2E_OPEN_DB, close_db=E2E_CLOSE_DB, hang_blocks=E2E_HANG)
    s = torch.cuda.Stream()
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    d_out = torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda")
    d_rows = torch.full((2, n, 4, 128), PATTERN, dtype=torch.int16, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    indexes = torch.zeros((2, n), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for k, a in enumerate((0, 4)):
            batch.update_device_strided(dI[:, a:].data_ptr(), dQ[:, a:].data_ptr(), d_out[:, a:].data_ptr(), 4, nb, nb, stream=s.cuda_stream)
            g.update_device(d_out[:, a:].data_ptr(), 4, stride_blocks=nb, rows_ptr=d_rows[k].data_ptr(), capacity_rows=n, stream=s.cuda_stream)
            counts[k:k + 1].copy_(g.count_tensor()); indexes[k].copy_(g.index_tensor())   # consumers on the same stream
    s.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), oracle_audio)
    for k, (index, rows, _) in enumerate(want):
        assert int(counts[k]) == len(index) and np.array_equal(indexes[k].cpu().numpy()[:len(index)], index)
        got = d_rows[k].cpu().numpy()
        assert np.array_equal(got[:len(index)], rows) and (got[len(index):] == PATTERN).all()
    assert GR.record_tuples(g.read_state()) == ref.state_tuples()
    g.close(); batch.close()
