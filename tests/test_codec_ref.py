"""tests/codec_ref.py pinned on its own, against the text of include/asdr_codec.h: known answers, the G.711 round trip over all 65,536
inputs, the ADPCM decoder reproducing the encoder's predictor, call splitting, odd counts, the ends of the state's range -- and,
where Python's audioop imports, that module as an independent pin (never the only check: it left the standard library in 3.13)."""
import numpy as np
import pytest

import codec_ref as CR

ALL = np.arange(-32768, 32768, dtype=np.int64)
BYTES = np.arange(256, dtype=np.int64)


def test_the_codec_is_part_of_the_package(A):
    """The package under test carries the codec this file restates."""
    assert A.AudioCodec is not None and A.CODEC_KINDS == CR.KINDS and A.CODEC_MAX_SAMPLES == CR.MAX_SAMPLES


def test_g711_known_answers():
    """mu-law of 0 is 0xFF and of 32767 is 0x80; A-law of 0 is 0xD5.  mu-law of -1: m = -1 >> 2 = -1, a = 1 + 33 = 34, e = 0,
    code = (34 >> 1) & 15 = 1, byte = 1 ^ 0x7F = 0x7E -- the statement's own arithmetic, and what audioop.lin2ulaw returns.  0x7F
    (negative zero) is the one byte this encoder never produces: it would need |m| = 0 with m < 0."""
    assert CR.ulaw_encode([0, -1, 32767, -32768]).tolist() == [0xFF, 0x7E, 0x80, 0x00]
    assert 0x7F not in set(CR.ulaw_encode(ALL).tolist()) and len(set(CR.ulaw_encode(ALL).tolist())) == 255
    assert CR.alaw_encode([0, -1, 32767, -32768]).tolist() == [0xD5, 0x55, 0xAA, 0x2A]
    assert len(set(CR.alaw_encode(ALL).tolist())) == 256
    assert CR.ulaw_decode([0xFF, 0x7F, 0x80, 0x00]).tolist() == [0, 0, 32124, -32124]
    assert CR.alaw_decode([0xD5, 0x55, 0xAA, 0x2A]).tolist() == [8, -8, 32256, -32256]


@pytest.mark.parametrize("enc,dec,bound", [(CR.ulaw_encode, CR.ulaw_decode, 644), (CR.alaw_encode, CR.alaw_decode, 512)])
def test_g711_round_trip_over_all_inputs(enc, dec, bound):
    """decode(encode(x)) takes exactly the decoder's values, is monotonic, a fixed point, and within 644 (mu-law) / 512 (A-law) of
    x, the maximum at the clipped top of the range."""
    y = dec(enc(ALL)).astype(np.int64)
    assert set(y.tolist()) == set(dec(BYTES).astype(np.int64).tolist())
    assert (np.diff(y) >= 0).all()
    assert np.array_equal(dec(enc(y)), y)
    err = np.abs(y - ALL)
    assert err.max() == bound and abs(int(ALL[np.argmax(err)])) >= 32767 - bound


def signals(rng, n):
    t = np.arange(n)
    return np.stack([rng.integers(-32768, 32768, size=n), np.round(30000 * np.sin(0.05 * t)), np.where(t & 1, 32767, -32768),
                     rng.integers(-3, 4, size=n), np.zeros(n)]).astype(np.int64)


def test_adpcm_decoder_reproduces_the_encoders_predictor():
    rng = np.random.default_rng(1)
    x = signals(rng, 301)                                        # an odd count
    p0, i0 = rng.integers(-32768, 32768, size=5), rng.integers(0, 89, size=5)
    nib, pred, p1, i1 = CR.adpcm_encode(x, p0, i0)
    y, p2, i2 = CR.adpcm_decode(nib, p0, i0)
    assert np.array_equal(y, pred) and np.array_equal(p1, p2) and np.array_equal(i1, i2) and np.array_equal(y[:, -1], p1)
    assert nib.max() <= 15 and i1.min() >= 0 and i1.max() <= 88
    sine = np.abs(y[1, 50:].astype(int) - x[1, 50:])
    assert sine.max() < 3000                                     # it tracks a sine once the step has grown


def test_adpcm_first_steps_by_hand():
    """A fresh channel, x = 100: s = 7, d = 100: c = 7, v = 0 + 7 + 3 + 1 = 11, p = 11, i = 0 + 8 = 8; then s = T[8] = 16, d = 89:
    c = 7, v = 2 + 16 + 8 + 4 = 30, p = 41, i = 16.  x = -5 from p = 41, i = 16: s = 34, d = 46 negative: c = 4 | 0 | 1 (46 - 34 = 12
    < 17, 12 >= 8), v = 4 + 34 + 8 = 46, p = -5, i = 16 + 2 (5 - 3) = 20."""
    nib, pred, p, i = CR.adpcm_encode([[100, 100, -5]], [0], [0])
    assert nib.tolist() == [[7, 7, 13]] and pred.tolist() == [[11, 41, -5]] and (int(p[0]), int(i[0])) == (-5, 20)


def test_adpcm_call_splitting_and_odd_counts():
    rng = np.random.default_rng(2)
    x = signals(rng, 257)
    whole = CR.adpcm_encode(x, np.zeros(5), np.zeros(5))
    for sizes in ([1] * 257, [7, 250], [128, 129], [35, 34, 35, 153]):
        p, i, parts, b = np.zeros(5), np.zeros(5), [], 0
        for size in sizes:
            nib, _, p, i = CR.adpcm_encode(x[:, b:b + size], p, i)
            parts.append(nib); b += size
        assert np.array_equal(np.concatenate(parts, axis=1), whole[0]) and np.array_equal(p, whole[2]) and np.array_equal(i, whole[3])


def test_adpcm_ends_of_the_state_range():
    n = 64
    alt = np.where(np.arange(n) & 1, 32767, -32768)[None]
    for p0, i0 in ((0, 0), (32767, 88), (-32768, 88), (32767, 0), (-32768, 0)):
        nib, pred, p, i = CR.adpcm_encode(alt, [p0], [i0])
        assert int(i[0]) == 88 and (int(pred.max()) == 32767 or int(pred.min()) == -32768)     # driven to the top of the table, p at an end
        y = CR.adpcm_decode(nib, [p0], [i0])[0]
        assert np.array_equal(y, pred)
    # both clamps, by hand at i = 88 (s = 32767, s >> 3 = 4095): x = p = 32767 gives c = 0, p + 4095 -> 32767; x = -32768 from
    # p = -32767 gives d = -1: c = 0 with the sign, p - 4095 -> -32768
    nib, pred, p, i = CR.adpcm_encode([[32767], [-32768]], [32767, -32767], [88, 88])
    assert nib.tolist() == [[0], [8]] and p.tolist() == [32767, -32768] and i.tolist() == [87, 87]
    nib, pred, p, i = CR.adpcm_encode(np.zeros((1, 200), dtype=np.int64), [12345], [88])       # silence drives i to 0
    assert int(i[0]) == 0 and abs(int(p[0])) <= 8


def test_packet_rows():
    rng = np.random.default_rng(3)
    assert [CR.row_bytes(CR.ADPCM, n) for n in (1, 2, 35, 128)] == [5, 5, 22, 68]
    assert [CR.row_bytes(CR.ULAW, n) for n in (1, 2, 35, 128)] == [1, 2, 35, 128] and CR.padded_bytes(CR.ALAW, 35) == 36
    assert CR.padded_bytes(CR.ADPCM, 34) == 24 and CR.padded_bytes(CR.ADPCM, 35) == 24 and CR.padded_bytes(CR.ADPCM, 128) == 68
    nib = rng.integers(0, 16, size=(3, 35)).astype(np.uint8)
    rows = CR.pack_adpcm(nib, [-2, 258, 32767], [88, 0, 5])
    assert rows.shape == (3, 24) and rows[:, :4].tolist() == [[0xFE, 0xFF, 88, 0], [2, 1, 0, 0], [0xFF, 0x7F, 5, 0]]
    assert rows[0, 4] == nib[0, 0] | (nib[0, 1] << 4) and rows[0, 21] == nib[0, 34] and not rows[:, 22:].any()
    back, p0, i0 = CR.unpack_adpcm(rows, 35)
    assert np.array_equal(back, nib) and p0.tolist() == [-2, 258, 32767] and i0.tolist() == [88, 0, 5]


def test_codec_ref_carries_state_through_the_three_mappings():
    rng = np.random.default_rng(4)
    n, m = 6, 35
    x = [rng.integers(-20000, 20000, size=(n, m)) for _ in range(3)]
    whole = CR.CodecRef(n, "adpcm")
    full = [whole.encode(v)[1] for v in x]
    ref = CR.CodecRef(n, CR.ADPCM)
    chans, rows = ref.encode(x[0], index=[4, 1, 5, 0], count=3, capacity=6)                   # chain rows behind an index
    assert chans.tolist() == [4, 1, 5] and np.array_equal(rows, full[0][[4, 1, 5]])
    assert ref.state_tuples()[0] == (0, 0, 0) and ref.state_tuples()[4] != (0, 0, 0)          # undelivered: unchanged
    compact = x[1][[4, 5]]
    chans, rows = ref.encode(compact, index=[4, 5], count=2, capacity=1, compact=True)        # compact rows, capacity below count
    assert chans.tolist() == [4] and np.array_equal(rows, full[1][[4]])
    chans, rows = ref.encode(x[1], index=[1], count=1, capacity=6)                            # channel 1 skipped a call: continues
    assert np.array_equal(rows, full[1][[1]])
    for kind, enc in ((CR.ULAW, CR.ulaw_encode), (CR.ALAW, CR.alaw_encode)):
        g = CR.CodecRef(n, kind)
        chans, rows = g.encode(x[2], index=[2, 3], count=2, capacity=2)
        assert rows.shape == (2, 36) and np.array_equal(rows[:, :35], enc(x[2][[2, 3]])) and not rows[:, 35].any()
        assert g.state_tuples() == [(0, 0, 0)] * n
        assert np.array_equal(CR.decode_rows(kind, rows, m), (CR.ulaw_decode if kind == CR.ULAW else CR.alaw_decode)(rows[:, :35]))
    assert np.array_equal(CR.decode_rows(CR.ADPCM, full[0], m), CR.adpcm_encode(x[0], np.zeros(n), np.zeros(n))[1])


# ---- audioop, where the interpreter still has it
def test_audioop_g711():
    audioop = pytest.importorskip("audioop")
    pcm = ALL.astype("<i2").tobytes()
    assert np.array_equal(np.frombuffer(audioop.lin2ulaw(pcm, 2), dtype=np.uint8), CR.ulaw_encode(ALL))
    assert np.array_equal(np.frombuffer(audioop.lin2alaw(pcm, 2), dtype=np.uint8), CR.alaw_encode(ALL))
    every = bytes(range(256))
    assert np.array_equal(np.frombuffer(audioop.ulaw2lin(every, 2), dtype="<i2"), CR.ulaw_decode(BYTES))
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(every, 2), dtype="<i2"), CR.alaw_decode(BYTES))


def test_audioop_adpcm():
    """audioop packs the first sample of a byte into the high nibble; after the swap nibbles, decoded samples and final state agree."""
    audioop = pytest.importorskip("audioop")
    rng = np.random.default_rng(5)
    x = signals(rng, 400)
    p0, i0 = rng.integers(-32768, 32768, size=5), rng.integers(0, 89, size=5)
    p0[0], i0[0] = 0, 0
    nib, pred, p1, i1 = CR.adpcm_encode(x, p0, i0)
    for k in range(5):
        data, (vp, vi) = audioop.lin2adpcm(x[k].astype("<i2").tobytes(), 2, (int(p0[k]), int(i0[k])))
        b = np.frombuffer(data, dtype=np.uint8)
        theirs = np.stack([b >> 4, b & 15], axis=1).reshape(-1)
        assert np.array_equal(theirs, nib[k]) and (vp, vi) == (int(p1[k]), int(i1[k]))
        back, (wp, wi) = audioop.adpcm2lin(data, 2, (int(p0[k]), int(i0[k])))
        assert np.array_equal(np.frombuffer(back, dtype="<i2"), pred[k]) and (wp, wi) == (vp, vi)
