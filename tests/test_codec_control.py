"""The audio codec's control plane (include/asdr_codec.h) on an ASDR_NO_DEVICE codec: the exported names, row sizes, every refusal
(each leaves everything as it was), the state calls on the host copy, the calls that need a device, and the host decoder against
tests/codec_ref.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import codec_ref as CR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KINDS = ("ulaw", "alaw", "adpcm")


def records(A, values):
    return np.array(values, dtype=A.CODEC_STATE_DTYPE)


def test_every_declared_name_is_exported_and_bound(A):
    with open(os.path.join(ROOT, "include", "asdr_codec.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(asdr_codec_\w+)\s*\(", text)))
    assert len(declared) == 12 and "asdr_codec_encode_device" in declared and "asdr_codec_deliver" in declared and "asdr_codec_decode" in declared
    L = ctypes.CDLL(A.library_path())
    for n in declared:
        assert hasattr(L, n), n
    assert sorted(A.CODEC_EXPORTS) == declared
    others = set(A.binding.EXPORTS) | set(A.GATE_EXPORTS) | set(A.TUNER_EXPORTS) | set(A.FRONT_EXPORTS) | set(A.RESAMPLE_EXPORTS)
    assert not [n for n in A.CODEC_EXPORTS if n in others]
    assert A.CODEC_KINDS == CR.KINDS == {"ulaw": 1, "alaw": 2, "adpcm": 3} and A.CODEC_MAX_SAMPLES == CR.MAX_SAMPLES == 65535 * 128
    assert A.CODEC_STATE_DTYPE.itemsize == 4 and A.CODEC_STATE_DTYPE.names == ("predictor", "step_index", "reserved")
    for name, value in (("ASDR_CODEC_ULAW", 1), ("ASDR_CODEC_ALAW", 2), ("ASDR_CODEC_ADPCM", 3), ("ASDR_CODEC_MAX_SAMPLES", 8388480)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name


def test_creation_values_and_row_bytes(A):
    for kind in KINDS:
        c = A.AudioCodec(5, kind=kind, device=A.NO_DEVICE)
        assert (c.n_channels, c.kind) == (5, CR.KINDS[kind]) and c._L.asdr_codec_n_channels(c._h) == 5
        assert c.read_state().shape == (5,) and not c.read_state().view(np.uint8).any()
        for n in (1, 2, 35, 128, 34, 8388480):
            assert c.row_bytes(n) == CR.row_bytes(CR.KINDS[kind], n) == A.codec_row_bytes(kind, n)
        c.close()
    assert [A.codec_row_bytes("adpcm", n) for n in (1, 2, 35, 128)] == [5, 5, 22, 68]
    assert [A.codec_row_bytes("ulaw", n) for n in (1, 2, 35, 128)] == [1, 2, 35, 128]
    assert [A.codec_row_bytes(2, n) for n in (1, 2, 35, 128)] == [1, 2, 35, 128]
    assert A.AudioCodec(2, kind=3, device=A.NO_DEVICE).kind == 3                  # the header's numbers are taken too


def test_creation_and_row_bytes_refusals(A):
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(A.AsdrError, match="n_channels"):
            A.AudioCodec(n, device=A.NO_DEVICE)
    c = A.AudioCodec(1 << 20, kind="ulaw", device=A.NO_DEVICE)                    # the largest bank is accepted
    assert c.n_channels == 1 << 20
    c.close()
    for kind in (0, 4, -1):
        with pytest.raises(A.AsdrError, match="kind"):
            A.AudioCodec(3, kind=kind, device=A.NO_DEVICE)
        with pytest.raises(A.AsdrError, match="kind"):
            A.codec_row_bytes(kind, 128)
        with pytest.raises(A.AsdrError, match="kind"):
            A.AudioCodec.decode(kind, np.zeros(8, dtype=np.uint8), 4)
    with pytest.raises(A.AsdrError, match="kind"):
        A.AudioCodec(3, kind="opus", device=A.NO_DEVICE)
    for n in (0, -1, 8388481, 2**40):
        with pytest.raises(A.AsdrError, match="n_samples"):
            A.codec_row_bytes("adpcm", n)


@pytest.mark.parametrize("kind", KINDS)
def test_encode_arguments_are_refused_before_a_device_is_asked_for(A, kind):
    """The pointers are never dereferenced on the host: a bad argument is refused by its own message, a good call by the missing
    device."""
    c = A.AudioCodec(3, kind=kind, device=A.NO_DEVICE)
    padded = (c.row_bytes(35) + 3) & ~3                                           # 36 for G.711, 24 for ADPCM
    ok = dict(ptr=4096, n_samples=35, out_ptr=1 << 20, out_stride_bytes=padded, row_stride_samples=35)
    for kw, why in ((dict(n_samples=0), "n_samples"), (dict(n_samples=-1), "n_samples"), (dict(n_samples=8388481, row_stride_samples=8388481), "n_samples"),
                    (dict(row_stride_samples=34), "row stride shorter"), (dict(ptr=4097), "2-byte"), (dict(ptr=0), "null"), (dict(out_ptr=0), "null"),
                    (dict(out_ptr=(1 << 20) + 2), "4-byte"), (dict(out_stride_bytes=padded + 2), "multiple of 4"),
                    (dict(out_stride_bytes=padded - 4), "shorter than the row"), (dict(out_stride_bytes=0), "shorter than the row"),
                    (dict(index_ptr=8192, capacity_rows=3), "count"), (dict(index_ptr=8192, count_ptr=8192, capacity_rows=-1), "negative")):
        with pytest.raises(A.AsdrError, match=why):
            c.encode_device(**dict(ok, **kw))
    for kw in (dict(), dict(out_stride_bytes=padded + 4), dict(ptr=4098, row_stride_samples=37)):
        with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
            c.encode_device(**dict(ok, **kw))
    with pytest.raises(A.AsdrError, match="n_samples"):
        c.deliver(4096, 0)
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        c.deliver(4096, 128)
    c.close()


def test_the_signal_path_needs_a_device(A):
    c = A.AudioCodec(3, device=A.NO_DEVICE)
    c.write_state(records(A, [(7, 8, 0)]), channels=[1])
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        c.encode_device(4096, 128, 8192, 68)
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        c.deliver(4096, 128)
    assert c.read_state().tolist() == [(0, 0, 0), (7, 8, 0), (0, 0, 0)]
    L = c._L
    assert L.asdr_codec_n_channels(None) == -1 and L.asdr_codec_kind(None) == -1 and L.asdr_codec_reset(None) == -1
    assert L.asdr_codec_synchronize(None) == -1 and L.asdr_codec_read_state(None, None) == -1
    assert L.asdr_codec_encode_device(None, None, 0, 0, 0, None, 0, None, None, 0, None) == -1
    c.close()


def test_state_round_trip_refusals_and_reset(A):
    c = A.AudioCodec(6, kind="adpcm", device=A.NO_DEVICE)
    rec = records(A, [(-32768, 88, 0), (32767, 0, 0), (-1, 44, 0)])
    c.write_state(rec, channels=[5, 0, 2])
    want = np.zeros(6, dtype=A.CODEC_STATE_DTYPE)
    want[[5, 0, 2]] = rec
    assert np.array_equal(c.read_state(), want)
    good = records(A, [(1, 1, 0), (2, 2, 0), (3, 3, 0)])
    for bad, why in (((3, 89, 0), "step_index"), ((3, 255, 0), "step_index"), ((3, 3, 1), "reserved"), ((0, 0, 128), "reserved")):
        r = good.copy()
        r[2] = bad                                                                # the last record is bad: none is written
        with pytest.raises(A.AsdrError, match=why):
            c.write_state(r, channels=[1, 3, 4])
    for chans in ([1, 3, 6], [1, -1, 3], [1 << 20, 0, 1]):
        with pytest.raises(A.AsdrError, match="bad channel"):
            c.write_state(good, channels=chans)
    with pytest.raises(A.AsdrError, match="more records"):
        c.write_state(np.zeros(7, dtype=A.CODEC_STATE_DTYPE))
    with pytest.raises(A.AsdrError, match="records for"):
        c.write_state(good, channels=[1, 2])
    assert np.array_equal(c.read_state(), want)                                   # every refusal left the records alone
    c.write_state(good[:2])                                                       # channels 0, 1
    want[:2] = good[:2]
    assert np.array_equal(c.read_state(), want)
    moved = A.AudioCodec(8, kind="adpcm", device=A.NO_DEVICE)
    moved.write_state(c.read_state(), channels=[7, 6, 5, 4, 3, 2])
    assert np.array_equal(moved.read_state()[[7, 6, 5, 4, 3, 2]], want) and not moved.read_state()[:2].view(np.uint8).any()
    c.reset()
    assert not c.read_state().view(np.uint8).any()
    c.synchronize()
    c.close(); moved.close()


@pytest.mark.parametrize("kind", ["ulaw", "alaw"])
def test_a_g711_codecs_records_stay_zero(A, kind):
    c = A.AudioCodec(4, kind=kind, device=A.NO_DEVICE)
    for bad in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        with pytest.raises(A.AsdrError, match="G.711|reserved"):
            c.write_state(records(A, [(0, 0, 0), bad]))
    c.write_state(np.zeros(4, dtype=A.CODEC_STATE_DTYPE))                         # zero records are accepted
    assert not c.read_state().view(np.uint8).any()
    c.close()


@pytest.mark.parametrize("n", [1, 2, 35, 128])
def test_the_host_decoder_equals_the_restatement(A, n):
    rng = np.random.default_rng(n)
    x = rng.integers(-32768, 32768, size=(7, n))
    for kind in ("ulaw", "alaw"):
        rows = CR.CodecRef(7, kind).encode(x)[1]
        got = A.AudioCodec.decode(kind, rows, n)
        assert got.dtype == np.int16 and np.array_equal(got, CR.decode_rows(CR.KINDS[kind], rows, n))
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(A.AudioCodec.decode("ulaw", every, 256), CR.ulaw_decode(every))
    assert np.array_equal(A.AudioCodec.decode("alaw", every, 256), CR.alaw_decode(every))
    ref = CR.CodecRef(7, "adpcm")
    ref.p[:] = [0, 32767, -32768, -1, 258, 1000, -20000]                          # non-zero headers
    ref.i[:] = [0, 88, 88, 0, 44, 87, 1]
    for _ in range(2):
        rows = ref.encode(x)[1]
        assert rows[:, 2].any() and np.array_equal(A.AudioCodec.decode("adpcm", rows, n), CR.decode_rows(CR.ADPCM, rows, n))
    one = A.AudioCodec.decode(3, rows[4], n)                                      # one row, by number
    assert one.shape == (n,) and np.array_equal(one, CR.decode_rows(CR.ADPCM, rows[4:5], n)[0])


def test_the_host_decoder_refuses_bad_rows(A):
    row = np.zeros(24, dtype=np.uint8)
    for k, v, why in ((2, 89, "step_index"), (3, 1, "header byte")):
        bad = row.copy()
        bad[k] = v
        with pytest.raises(A.AsdrError, match=why):
            A.AudioCodec.decode("adpcm", bad, 35)
    with pytest.raises(A.AsdrError, match="rows must be"):
        A.AudioCodec.decode("adpcm", row[:21], 35)                                # 22 bytes are needed
    for n in (0, 8388481):
        with pytest.raises(A.AsdrError, match="n_samples"):
            A.AudioCodec.decode("ulaw", row, n)
    assert A.AudioCodec.decode("adpcm", row[:22], 35).tolist() == CR.decode_rows(CR.ADPCM, row[None, :22], 35)[0].tolist()
