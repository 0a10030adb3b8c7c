"""The audio codec on the GPU (include/asdr_codec.h; audiosdr_amd/csrc/asdr_codec.hip) against tests/codec_ref.py at tolerance 0: all
three kinds over partial waves and workgroups, sample counts around every piece and chunk boundary, splitting, the aligned and the
two unaligned row geometries, the ADPCM extremes, both index forms alone and behind a real gate, the whole path gate -> resampler ->
codec -> deliver, deliver into pageable and pinned memory, the state calls, streams, and one full-size call.
The sizes are the smallest that reach each seam: the G.711 pass gives a lane one 16-byte piece (8 samples) and packs rows shorter than
256 pieces into shared workgroups; the ADPCM pass gives a lane a row and a wave 64 rows (63 / 64 / 65 / 257 channels: a partial wave, a
full one, one row more, several workgroups) and stages 64 samples at a time, forming 16 samples between stores (1 .. 9 samples: less
than a piece, a piece, one more; 34 / 35: a 12 kHz block, odd; 128 / 129 / 640: whole chunks, one sample more, many)."""
import numpy as np
import pytest

import codec_ref as CR
import gate_ref as GR
import resample_ref as RR

pytestmark = pytest.mark.gpu
KINDS = ("ulaw", "alaw", "adpcm")
GAP = 0x7FFF        # fills the input between and behind the rows: never encoded
PATTERN = 0xA5      # pre-fills the output buffer: must stay wherever nothing is to be written
GUARD = 64          # bytes behind the last output row
COUNTS = (1, 2, 7, 8, 9, 34, 35, 128, 129, 128 * 5)


def full_range(rng, rows, n):
    return rng.integers(-32768, 32768, size=(rows, n)).astype(np.int16)


def up8(n):
    return (n + 7) & ~7


class Rig:
    """A codec and its reference side by side; call() runs one encode on both and compares every byte of the output buffer."""

    def __init__(self, A, n, kind):
        import torch
        self.torch, self.A, self.n, self.kind = torch, A, n, kind
        self.codec = A.AudioCodec(n, kind=kind)
        self.ref = CR.CodecRef(n, kind)

    def call(self, x, stride=None, offset=0, out_extra=0, index=None, count=None, capacity=None, compact=False, stream=None):
        """x int16 [input rows][n_samples].  stride: the input row stride in samples (default: n_samples rounded up to 8, the aligned
        geometry); offset: samples between the 256-byte aligned buffer and row 0; out_extra: dwords of slack in the output stride.
        index (int32 list) / count / capacity select an index form, compact the row mapping.  Returns (channels, reference rows)."""
        torch = self.torch
        x = np.asarray(x, dtype=np.int16)
        in_rows, ns = x.shape
        stride = up8(ns) if stride is None else stride
        held = max(in_rows, min(capacity, self.n) if compact else 0)           # a compact buffer has room for capacity_rows rows
        flat = np.full(offset + (held - 1) * stride + ns + 24, GAP, dtype=np.int16)
        for r in range(in_rows):
            flat[offset + r * stride:offset + r * stride + ns] = x[r]
        padded = CR.padded_bytes(self.ref.kind, ns)
        ostride = padded + 4 * out_extra
        if index is None:
            rows = self.n
        else:
            rows = capacity
            d_index = torch.from_numpy(np.asarray(index, dtype=np.int32).copy()).cuda()
            d_count = torch.tensor([count], dtype=torch.int32, device="cuda")
        d_in = torch.from_numpy(flat).cuda()
        d_out = torch.full((max(rows, 1) * ostride + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        got = self.codec.encode_device(d_in.data_ptr() + 2 * offset, ns, d_out.data_ptr(), ostride, row_stride_samples=stride, rows_compact=compact,
                                       index_ptr=0 if index is None else d_index.data_ptr(), count_ptr=0 if index is None else d_count.data_ptr(),
                                       capacity_rows=0 if index is None else capacity, stream=stream.cuda_stream if stream is not None else 0)
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        chans, want = self.ref.encode(x, index=index, count=count, capacity=capacity, compact=compact)
        k = len(chans)
        assert got == CR.row_bytes(self.ref.kind, ns) == self.codec.row_bytes(ns) and want.shape == (k, padded)
        out = d_out.cpu().numpy()
        body = out[:max(rows, 1) * ostride].reshape(max(rows, 1), ostride)
        assert np.array_equal(body[:k, :padded], want), "packet rows differ from the reference"
        assert not body[:k, got:padded].any(), "the bytes up to the next multiple of 4 are not zero"
        assert (body[:k, padded:] == PATTERN).all(), "a row is written past its bytes rounded up to 4"
        assert (body[k:] == PATTERN).all(), "rows past min(count, capacity_rows) are written"
        assert (out[max(rows, 1) * ostride:] == PATTERN).all(), "the buffer is written behind the last row"
        assert np.array_equal(d_in.cpu().numpy(), flat), "the input changed"
        return chans, want

    def check_state(self):
        st = self.codec.read_state()
        assert list(zip(st["predictor"].tolist(), st["step_index"].tolist(), st["reserved"].tolist())) == self.ref.state_tuples()

    def place(self, records, channels):
        """Both sides' records of `channels` to (predictor, step_index) pairs."""
        rec = np.array([(p, i, 0) for p, i in records], dtype=self.A.CODEC_STATE_DTYPE)
        self.codec.write_state(rec, channels=channels)
        for c, (p, i) in zip(channels, records):
            self.ref.p[c], self.ref.i[c] = p, i

    def close(self):
        self.codec.close()


# ---- channels x sample counts x kinds, the geometry changing from call to call
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", KINDS)
def test_channel_counts_and_sample_counts(gpu, kind, n):
    """Ten calls on one codec, so every ADPCM call but the first starts from the state the one before left.  The geometry cycles
    through aligned, a base one sample off, an odd stride, and an output stride with slack."""
    rng = np.random.default_rng(n * 7 + len(kind))
    r = Rig(gpu, n, kind)
    for k, ns in enumerate(COUNTS):
        geo = (dict(), dict(offset=1), dict(stride=ns | 1), dict(out_extra=3))[k & 3]
        r.call(full_range(rng, n, ns), **geo)
    r.check_state()
    r.close()


@pytest.mark.parametrize("kind", KINDS)
def test_37_blocks_in_one_call_and_in_four(gpu, kind):
    """128 * 37 samples at once and as 1, 5, 2 and 29 blocks: the same bytes behind the headers and the same final state."""
    rng = np.random.default_rng(37)
    n, nb = 67, 37
    x = full_range(rng, n, 128 * nb)
    whole = Rig(gpu, n, kind)
    _, rows = whole.call(x)
    head = CR.HEADER if kind == "adpcm" else 0
    parts, b = [], 0
    split = Rig(gpu, n, kind)
    for size in (1, 5, 2, 29):
        _, part = split.call(x[:, 128 * b:128 * (b + size)])
        parts.append(part[:, head:CR.row_bytes(split.ref.kind, 128 * size)])
        b += size
    assert np.array_equal(np.concatenate(parts, axis=1), rows[:, head:])
    whole.check_state(); split.check_state()
    assert np.array_equal(whole.codec.read_state(), split.codec.read_state())
    whole.close(); split.close()


# ---- row geometry
@pytest.mark.parametrize("geo", [dict(), dict(stride=40), dict(offset=1), dict(offset=3, stride=43), dict(stride=35), dict(offset=4, stride=48),
                                 dict(out_extra=1), dict(offset=1, stride=35, out_extra=5)],
                         ids=["aligned", "stride40", "off1", "off3odd", "odd35", "off4", "slack", "all"])
@pytest.mark.parametrize("kind", KINDS)
def test_row_geometry(gpu, kind, geo):
    """35 samples (a 12 kHz block) and 131: a 16-byte aligned base with a stride that is a multiple of 8 takes the 16-byte loads, a
    base off by 1, 3 or 4 samples or an odd stride the sample-by-sample path.  The gaps hold 0x7FFF, which no row may show."""
    rng = np.random.default_rng(len(str(geo)))
    r = Rig(gpu, 70, kind)
    for ns in (35, 131):
        g = dict(geo)
        if ns > g.get("stride", ns):
            g["stride"] += 128
        r.call(full_range(rng, 70, ns), **g)
    r.check_state()
    r.close()


# ---- ADPCM extremes
def test_adpcm_extremes_and_placed_states(gpu):
    rng = np.random.default_rng(11)
    n, ns = 66, 200
    t = np.arange(ns)
    r = Rig(gpu, n, "adpcm")
    alt = np.where(t & 1, 32767, -32768).astype(np.int16)
    r.call(np.tile(alt, (n, 1)))                                               # +-full scale: i climbs to 88, p clamps
    assert (r.ref.i == 88).all() and r.ref.p.max() == 32767
    r.call(full_range(rng, n, ns))                                             # full-range noise from the top of the table
    r.call(np.zeros((n, ns), dtype=np.int16))                                  # silence after noise: i falls to 0
    assert (r.ref.i == 0).all()
    r.call(rng.integers(-2, 3, size=(n, ns)).astype(np.int16))                 # near silence at the bottom of the table
    r.check_state()
    corners = [(32767, 88), (-32768, 88), (32767, 0), (-32768, 0), (0, 88), (-1, 44), (12345, 87), (-32767, 88)]
    r.place(corners, channels=list(range(8, 16)))
    r.check_state()
    x = full_range(rng, n, 35)
    x[8:12] = np.array([32767, -32768, -32768, 32767], dtype=np.int16)[:, None]   # at the clamp: from p = 32767 up, from -32768 down ...
    x[15] = -32768                                                             # p - v below -32768 from p = -32767
    _, rows = r.call(x)
    assert rows[8:16, :4].tolist() == [[p & 0xFF, (p >> 8) & 0xFF, i, 0] for p, i in corners]   # the headers are the placed states
    pred = CR.adpcm_encode(x[[8, 9, 15]], [32767, -32768, -32767], [88, 88, 88])[1]
    assert (pred[0] == 32767).all() and pred[1].min() == -32768 and pred[2, 0] == -32768      # both clamps are reached
    r.check_state()
    r.close()


# ---- the index forms
@pytest.mark.parametrize("compact", [False, True], ids=["rows_by_channel", "rows_compact"])
@pytest.mark.parametrize("kind", ["ulaw", "adpcm"])
def test_index_forms_counts_and_capacity(gpu, kind, compact):
    """count 0, below, equal to and above the capacity, capacity 0, a descending index, and the wave boundary (64 of 150 rows).
    Undelivered channels' records do not move (check_state after every call); channel 5 is delivered, skipped twice, delivered
    again, and its second row continues from its first (the reference only ever advanced it in those two calls)."""
    rng = np.random.default_rng(60 + compact)
    n, ns = 150, 35
    r = Rig(gpu, n, kind)
    third = np.sort(rng.permutation(n)[:n // 3]).astype(np.int32)
    third = third[third != 5]
    cases = (([5, 9, 140], 3, n), ([0] * n, 0, n), (third, len(third), n), (third, len(third), 7), (third, 3, 7), (list(range(n - 1, -1, -1)), n, n),
             (list(range(n)), n, 0), (list(range(n)), n + 50, 64), ([149, 5], 2, 2))
    before = None
    for index, count, capacity in cases:
        k = max(0, min(count, capacity, n))
        rows = k if compact else n
        x = full_range(rng, max(rows, 1), ns)
        chans, want = r.call(x, index=index, count=count, capacity=capacity, compact=compact, stride=40, out_extra=1)
        assert len(chans) == k
        r.check_state()
        if 5 in chans.tolist() and kind == "adpcm":
            row = want[chans.tolist().index(5)]
            if before is not None:
                assert row[:3].tolist() == before                              # the header is where the earlier row ended
            before = [int(r.ref.p[5]) & 0xFF, (int(r.ref.p[5]) >> 8) & 0xFF, int(r.ref.i[5])]
    r.close()


def test_behind_a_real_gate_on_one_stream(gpu):
    """Gate and codec on one stream, no host step between them: the rows written are the reference rows of exactly
    index[0 .. count), read from the chain's rows by channel.  A third of the channels is loud."""
    import torch
    rng = np.random.default_rng(70)
    n, nb = 300, 2
    audio = rng.integers(-20, 21, size=(n, nb, 128)).astype(np.int16)
    loud = np.sort(rng.permutation(n)[:n // 3])
    audio[loud] = rng.integers(-20000, 20001, size=(len(loud), nb, 128)).astype(np.int16)
    thr = 128 * 2000 * 2000
    gate, gref = gpu.AudioGate(n), GR.GateRef(n)
    gate.set_squelch(energies=(thr, thr), hang_blocks=0); gref.set_squelch(thr, thr, 0)
    assert np.array_equal(gref.update(audio)[0], loud)
    for kind in KINDS:
        codec, ref = gpu.AudioCodec(n, kind=kind), CR.CodecRef(n, kind)
        chans, want = ref.encode(audio.reshape(n, -1), index=loud, count=len(loud), capacity=n)
        padded = want.shape[1]
        s = torch.cuda.Stream()
        d_audio = torch.from_numpy(audio).cuda()
        d_out = torch.full((n, padded + 4), PATTERN, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gate.reset()
        gate.update_device(d_audio.data_ptr(), nb, stream=s.cuda_stream)
        got = codec.encode_device(d_audio.data_ptr(), 128 * nb, d_out.data_ptr(), padded + 4, index_ptr=gate.index_tensor().data_ptr(),
                                  count_ptr=gate.count_tensor().data_ptr(), capacity_rows=n, stream=s.cuda_stream)
        s.synchronize()
        out = d_out.cpu().numpy()
        assert got == codec.row_bytes(128 * nb) and int(gate.count_tensor().cpu()[0]) == len(loud)
        assert np.array_equal(out[:len(loud), :padded], want)
        assert (out[len(loud):] == PATTERN).all() and (out[:, padded:] == PATTERN).all()
        st = codec.read_state()
        assert list(zip(st["predictor"].tolist(), st["step_index"].tolist(), st["reserved"].tolist())) == ref.state_tuples()
        codec.close()
    gate.close()


# ---- end to end
@pytest.mark.parametrize("kind", KINDS)
def test_gate_resampler_codec_deliver(gpu, kind):
    """Synthetic rows -> gate -> resampler at 12 kHz behind the gate's index -> codec over the resampler's compact rows -> deliver,
    all on one stream, three calls; held to gate_ref, resample_ref and codec_ref chained, and the host rows decoded with
    asdr_codec_decode.  The loud set changes from call to call, so a channel's ADPCM stream pauses and resumes."""
    import torch
    rng = np.random.default_rng(90)
    n, nb, out_stride = 130, 1, 40                                             # 34 or 35 outputs per block in rows of 40 samples
    thr = 128 * 2000 * 2000
    gate, gref = gpu.AudioGate(n), GR.GateRef(n)
    gate.set_squelch(energies=(thr, thr), hang_blocks=0); gref.set_squelch(thr, thr, 0)
    rs = gpu.AudioResampler(n, fs_out=12000)
    rref = RR.ResampleRef(n, rs.up, rs.down, *rs.get_taps())
    codec, cref = gpu.AudioCodec(n, kind=kind), CR.CodecRef(n, kind)
    s = torch.cuda.Stream()
    for call in range(3):
        audio = rng.integers(-20, 21, size=(n, nb, 128)).astype(np.int16)
        loud = np.sort(rng.permutation(n)[:n // 2])
        audio[loud] = rng.integers(-20000, 20001, size=(len(loud), nb, 128)).astype(np.int16)
        index = gref.update(audio)[0]
        assert np.array_equal(index, loud)
        low = rref.update(audio)                                               # every channel's carry advances
        ns = low.shape[1]
        chans, want = cref.encode(low[index], index=index, count=len(index), capacity=n, compact=True)
        d_audio = torch.from_numpy(audio).cuda()
        d_low = torch.full((n, out_stride), GAP, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        gate.update_device(d_audio.data_ptr(), nb, stream=s.cuda_stream)
        ip, cp = gate.index_tensor().data_ptr(), gate.count_tensor().data_ptr()
        got_ns = rs.update_device(d_audio.data_ptr(), nb, d_low.data_ptr(), out_stride, index_ptr=ip, count_ptr=cp, capacity_rows=n, stream=s.cuda_stream)
        assert got_ns == ns
        count, host_index, host_rows = codec.deliver(d_low.data_ptr(), ns, row_stride_samples=out_stride, rows_compact=True, index_ptr=ip, count_ptr=cp,
                                                     capacity_rows=n, stream=s.cuda_stream)
        assert count == len(index) and np.array_equal(host_index, index) and np.array_equal(host_rows, want)
        decoded = gpu.AudioCodec.decode(kind, host_rows, ns)
        assert np.array_equal(decoded, CR.decode_rows(cref.kind, want, ns))
        if kind != "adpcm":                                                    # G.711's round-trip bound (test_codec_ref.py)
            assert np.abs(decoded.astype(int) - low[index]).max() <= (644 if kind == "ulaw" else 512)
    st = codec.read_state()
    assert list(zip(st["predictor"].tolist(), st["step_index"].tolist(), st["reserved"].tolist())) == cref.state_tuples()
    codec.close(); rs.close(); gate.close()


# ---- deliver
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("kind", ["alaw", "adpcm"])
def test_deliver_into_pageable_and_pinned_memory(gpu, kind, pinned):
    """All channels, then an index with the count below, at and above the capacity and 0, with and without a host index; only
    min(count, capacity_rows) rows arrive and the rest of the host buffer keeps its fill."""
    import torch
    rng = np.random.default_rng(100 + pinned)
    n, ns = 90, 35
    codec, ref = gpu.AudioCodec(n, kind=kind), CR.CodecRef(n, kind)
    padded = CR.padded_bytes(ref.kind, ns)
    buf = torch.empty((n, padded), dtype=torch.uint8)
    if pinned:
        buf = buf.pin_memory()
    host = buf.numpy()
    x = full_range(rng, n, ns)
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    host[:] = PATTERN
    count, index, rows = codec.deliver(d_x.data_ptr(), ns, rows_out=host)
    want = ref.encode(x)[1]
    assert count == n and index.tolist() == list(range(n)) and np.array_equal(rows, want) and np.array_equal(host, want)
    for idx, cnt, cap, want_index in (([3, 80, 41], 3, n, True), ([7, 6, 5, 4], 4, 2, True), ([1, 2], 2, 2, False), ([0] * 4, 0, 4, True),
                                      (list(range(n)), n + 9, n, False)):
        x = full_range(rng, n, ns)
        d_x = torch.from_numpy(x).cuda()
        d_index = torch.tensor(idx, dtype=torch.int32, device="cuda")
        d_count = torch.tensor([cnt], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        host[:] = PATTERN
        count, index, rows = codec.deliver(d_x.data_ptr(), ns, index_ptr=d_index.data_ptr(), count_ptr=d_count.data_ptr(), capacity_rows=cap,
                                           rows_out=host, want_index=want_index)
        chans, want = ref.encode(x, index=idx, count=cnt, capacity=cap)
        k = len(chans)
        assert count == cnt and rows.shape == (k, padded) and np.array_equal(rows, want)
        assert (index is None) if not want_index else index.tolist() == chans.tolist()
        assert (host[k:] == PATTERN).all()
        fresh = codec.deliver(d_x.data_ptr(), ns, index_ptr=d_index.data_ptr(), count_ptr=d_count.data_ptr(), capacity_rows=0)   # nothing to encode
        assert fresh[0] == cnt and fresh[2].shape == (0, padded)
    st = codec.read_state()
    assert list(zip(st["predictor"].tolist(), st["step_index"].tolist(), st["reserved"].tolist())) == ref.state_tuples()
    codec.close()


def test_deliver_grows_its_kept_buffer_and_reuses_it(gpu):
    """deliver's packet buffer is kept between calls: a call of 128 samples, one of 512 that needs a larger buffer, one of 256 that
    fits what the second left; every call's count, index and rows are the reference's, the ADPCM state running through all three."""
    import torch
    rng = np.random.default_rng(32)
    n = 3
    codec, ref = gpu.AudioCodec(n, kind="adpcm"), CR.CodecRef(n, "adpcm")
    for ns in (128, 512, 256):
        x = full_range(rng, n, ns)
        d_x = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        count, index, rows = codec.deliver(d_x.data_ptr(), ns)
        chans, want = ref.encode(x)
        assert count == n and index.tolist() == chans.tolist() == [0, 1, 2]
        assert rows.shape == (n, CR.padded_bytes(ref.kind, ns)) and np.array_equal(rows, want)
    st = codec.read_state()
    assert list(zip(st["predictor"].tolist(), st["step_index"].tolist(), st["reserved"].tolist())) == ref.state_tuples()
    codec.close()


# ---- state
def test_records_move_between_codecs_and_reset(gpu):
    """Read after two calls and written into other channels of a second codec: each channel continues bit for bit as in a codec
    that never stopped.  A refused write changes nothing.  Then reset."""
    rng = np.random.default_rng(80)
    n, ns = 6, 128
    a = Rig(gpu, n, "adpcm")
    first, second, rest = (full_range(rng, n, ns) for _ in range(3))
    a.call(first); a.call(second)
    rec = a.codec.read_state()
    b = Rig(gpu, n + 2, "adpcm")
    b.call(full_range(rng, n + 2, 35))
    chans = [7, 0, 3, 2, 5, 1]
    b.codec.write_state(rec, channels=chans)
    b.ref.p[chans], b.ref.i[chans] = a.ref.p, a.ref.i
    b.check_state()
    x = full_range(rng, n + 2, ns)
    x[chans] = rest
    _, got_b = b.call(x)
    _, got_a = a.call(rest)                                                    # a goes on uninterrupted
    assert np.array_equal(got_b[chans], got_a)
    bad = rec.copy()
    bad["step_index"][5] = 89
    with pytest.raises(gpu.AsdrError, match="step_index"):
        b.codec.write_state(bad, channels=chans)
    with pytest.raises(gpu.AsdrError, match="bad channel"):
        b.codec.write_state(rec, channels=[0, 1, 2, 3, 4, 8])
    b.check_state()
    b.codec.reset(); b.ref.reset()
    assert not b.codec.read_state().view(np.uint8).any()
    _, rows = b.call(x)
    assert not rows[:, :4].any()                                               # fresh headers
    b.check_state()
    g = Rig(gpu, 4, "ulaw")                                                    # a G.711 codec's records stay zero
    g.call(full_range(rng, 4, 35))
    assert not g.codec.read_state().view(np.uint8).any()
    a.close(); b.close(); g.close()


def test_encode_refusals_change_nothing(gpu):
    import torch
    r = Rig(gpu, 10, "adpcm")
    r.call(full_range(np.random.default_rng(1), 10, 35))
    d = torch.zeros((10, 256), dtype=torch.int16, device="cuda")
    o = torch.zeros((10, 256), dtype=torch.uint8, device="cuda")
    i = torch.zeros(10, dtype=torch.int32, device="cuda")
    ok = dict(ptr=d.data_ptr(), n_samples=128, out_ptr=o.data_ptr(), out_stride_bytes=68, row_stride_samples=256)
    for kw, why in ((dict(ptr=d.data_ptr() + 1), "2-byte"), (dict(row_stride_samples=127), "stride"), (dict(n_samples=0), "n_samples"),
                    (dict(n_samples=8388481, row_stride_samples=8388481), "n_samples"), (dict(ptr=0), "null"), (dict(out_ptr=0), "null"),
                    (dict(out_ptr=o.data_ptr() + 2), "4-byte"), (dict(out_stride_bytes=70), "multiple of 4"), (dict(out_stride_bytes=64), "shorter"),
                    (dict(out_ptr=d.data_ptr() + 512), "overlaps"), (dict(index_ptr=i.data_ptr(), capacity_rows=3), "count"),
                    (dict(index_ptr=i.data_ptr(), count_ptr=i.data_ptr(), capacity_rows=-1), "negative")):
        with pytest.raises(gpu.AsdrError, match=why):
            r.codec.encode_device(**dict(ok, **kw))
    r.check_state()
    r.close()


# ---- streams
def test_a_call_on_a_second_stream_after_one_on_the_first(gpu):
    """Two consecutive calls on different streams with no host synchronisation between them equal the same calls on one stream:
    the second call's start state is the first call's end state, so it must have waited on the device."""
    import torch
    rng = np.random.default_rng(91)
    n, ns = 3000, 128 * 6
    x = [full_range(rng, n, ns) for _ in range(2)]
    d_x = [torch.from_numpy(v).cuda() for v in x]
    ref = CR.CodecRef(n, "adpcm")
    want = [ref.encode(v)[1] for v in x]
    padded = want[0].shape[1]
    for streams in ((torch.cuda.Stream(), torch.cuda.Stream()), (torch.cuda.Stream(),) * 2):
        codec = gpu.AudioCodec(n, kind="adpcm")
        outs = [torch.full((n, padded), PATTERN, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for k in range(2):
            assert codec.encode_device(d_x[k].data_ptr(), ns, outs[k].data_ptr(), padded, stream=streams[k].cuda_stream) == 4 + ns // 2
        codec.synchronize()
        torch.cuda.synchronize()
        for k in range(2):
            assert np.array_equal(outs[k].cpu().numpy(), want[k])
        st = codec.read_state()
        assert list(zip(st["predictor"].tolist(), st["step_index"].tolist(), st["reserved"].tolist())) == ref.state_tuples()
        codec.close()


# ---- size
def test_a_c2_block_of_65536_channels(gpu):
    """65,536 channels x one 128-sample block, ADPCM, two calls so that the second starts from the first's state: every row."""
    import torch
    rng = np.random.default_rng(65536)
    n, ns = 65536, 128
    codec, ref = gpu.AudioCodec(n, kind="adpcm"), CR.CodecRef(n, "adpcm")
    for call in range(2):
        x = full_range(rng, n, ns)
        d_x = torch.from_numpy(x).cuda()
        d_out = torch.full((n, 72), PATTERN, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert codec.encode_device(d_x.data_ptr(), ns, d_out.data_ptr(), 72) == 68
        torch.cuda.synchronize()
        want = ref.encode(x)[1]
        out = d_out.cpu().numpy()
        assert np.array_equal(out[:, :68], want) and (out[:, 68:] == PATTERN).all()
    st = codec.read_state()
    assert np.array_equal(st["predictor"], ref.p.astype(np.int16)) and np.array_equal(st["step_index"], ref.i.astype(np.uint8))
    codec.close()
