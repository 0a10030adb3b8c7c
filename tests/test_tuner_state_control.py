"""Tuner state records, host half (include/asdr_tuner.h, "State records") on ASDR_NO_DEVICE banks: sizes, the field table, the
control-only round trips of channel records and bank-state blobs for all three bank kinds, and every import as a transaction: each
refusal leaves read_state / slots / gains / filters as they were."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

NEW = ["asdr_tuner_channel_record_bytes", "asdr_tuner_channel_record_field", "asdr_tuner_export_channels", "asdr_tuner_import_channels",
       "asdr_tuner_export_channels_device", "asdr_tuner_import_channels_device", "asdr_tuner_bank_state_bytes",
       "asdr_tuner_export_bank_state", "asdr_tuner_import_bank_state", "asdr_tuner_create_from_bank_state"]
CX = (np.arange(1, 8) * (0.5 - 0.25j)).astype(np.complex64)
KINDS = ["plain", "rate", "fastconv"]


def make(A, kind, n=6, s=3):
    if kind == "plain":
        return A.TunerBank(n, s, 7, device=A.NO_DEVICE)
    if kind == "rate":
        return A.TunerBank(n, s, 50, fs_in=2400000, device=A.NO_DEVICE)
    return A.TunerBank.fastconv(n, s, 2400000, 16, device=A.NO_DEVICE)


def dress(t, kind, seed=0):
    """Settings off every default: retunes, filters, format, corrections, statistics; palette, gains and monitors on a
    fast-convolution bank."""
    r = np.random.RandomState(seed)
    for c in range(t.n_channels):
        t.set_source(int(r.randint(0, t.n_sources)), ch=c); t.set_frequency_word(int(r.randint(0, 2**32, dtype=np.uint64)), ch=c)
        t.set_phase(int(r.randint(0, 2**32, dtype=np.uint64)), ch=c)
    t.set_input_format("cs8")
    t.set_iq_correction(words=(3, -4, 100, 65000), source=1)
    t.enable_iq_stats(True)
    U = t.ratio()[0]
    t.set_resampler((np.arange(U * 3) % 5 + 1).astype(np.int16), 2)
    if kind == "fastconv":
        t.set_channel_filter(np.array([0.25, 0.5, 0.25], dtype=np.float32))
        t.set_palette_filter(5, CX); t.set_palette_filter(63, np.array([1.0, -1.0], dtype=np.float32))
        t.set_channel_slot(5, ch=1); t.set_channel_slot(63, ch=2); t.set_gain(-2.5, ch=0); t.set_gain(0.0, ch=2)
        t.enable_spectrum(512, "rect", "peak"); t.enable_levels(True)
    else:
        t.set_filter(np.array([100, -200, 300, 7], dtype=np.int16), 3)


def settings(t, kind):
    out = [t.read_state().tobytes(), t.position(), t.output_position(), t.input_format(), t.get_resampler()[0].tobytes(), t.get_resampler()[1],
           [t.iq_correction(s) for s in range(t.n_sources)], t.iq_stats_enabled()]
    if kind == "fastconv":
        out += [t.get_channel_filter().tobytes(), [None if g is None else (str(g.dtype), g.tobytes()) for g in map(t.get_palette_filter, range(64))],
                t.slots().tobytes(), t.gains().tobytes(), t.spectrum_config(), t.levels_enabled()]
    else:
        out += [t.get_filter()[0].tobytes(), t.get_filter()[1]]
    return out


def test_the_new_functions_are_declared_and_exported(A):
    with open(os.path.join(ROOT, "include", "asdr_tuner.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = C.CDLL(A.library_path())
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, text) and hasattr(L, n) and n in A.TUNER_EXPORTS, n
    assert re.search(r"#define ASDR_TUNER_CHANNEL_RECORD_BYTES 2560\b", text)


def test_sizes_and_field_table(A):
    assert A.tuner._lib().asdr_tuner_channel_record_bytes() == 2560 == A.tuner.CHANNEL_RECORD_BYTES == 10 * 256
    fields = A.tuner_channel_record_fields()
    spans = sorted((off, off + cnt * np.dtype(ty).itemsize, n) for n, (ty, off, cnt) in fields.items())
    assert spans[0][0] == 0 and spans[-1][1] == 256
    for (a0, a1, _), (b0, b1, _) in zip(spans, spans[1:]):
        assert a1 == b0, (a0, a1, b0, b1)          # no gap, no overlap
    for n, (ty, off, cnt) in fields.items():
        assert off % np.dtype(ty).itemsize == 0, n
    assert fields["level"] == ("<f8", 96, 1) and fields["src"][1] == 64 and fields["kind"][1] == 16
    # the blob: header + filter + U x 64 resampler taps + corrections, no device sections without a device
    t = make(A, "plain", s=3)
    assert t.bank_state_bytes() == 256 + 2048 + 1 * 64 * 2 + 3 * 16
    t = make(A, "rate", s=2)
    assert t.ratio() == (147, 160) and t.bank_state_bytes() == 256 + 2048 + 147 * 64 * 2 + 2 * 16
    t = make(A, "fastconv", s=5)
    assert t.bank_state_bytes() == 256 + 528 + 147 * 64 * 2 + 63 * 1056 + 5 * 16
    assert A.tuner._lib().asdr_tuner_bank_state_bytes(None) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_control_only_round_trip(A, kind):
    a = make(A, kind)
    dress(a, kind, 1)
    blob, rec = a.export_bank_state(), a.export_channels()
    assert blob.size == a.bank_state_bytes() and rec.shape == (6, 2560)
    assert bytes(rec[0, :4]) == b"ASTC" and bytes(blob[:4]) == b"ASTB"
    f = lambda n: A.tuner_channel_field(rec, n)
    assert (f("version") == 1).all() and (f("bytes") == 2560).all() and (f("content") == 0).all()
    assert (f("kind") == (kind == "fastconv")).all() and (f("decimation") == a.decimation).all() and (f("fs_in") == a.fs_in).all()
    assert (f("up") == a.ratio()[0]).all() and (f("down") == a.ratio()[1]).all() and (f("position") == 0).all()
    st = a.read_state()
    for k in ("src", "fw", "pos_a", "ph_a"):
        assert (f(k) == st[k]).all(), k
    assert not rec[:, 104:].any() and not f("pad0").any() and not f("pad1").any() and (f("level") == 0).all()
    if kind == "fastconv":
        assert (f("slot") == a.slots()).all() and f("gain").tobytes() == a.gains().tobytes()
    else:
        assert (f("slot") == 0).all() and (f("gain") == 1).all()
    # a new bank of another channel count from the blob, then a permuted subset and a clone
    b = A.TunerBank.from_bank_state(blob, 9, device=A.NO_DEVICE)
    assert (b.n_sources, b.decimation, b.fs_in, b.ratio()) == (a.n_sources, a.decimation, a.fs_in, a.ratio())
    assert settings(b, kind)[1:8] == settings(a, kind)[1:8]
    assert not b.read_state().tobytes().strip(b"\0")            # creation state
    b.import_channels(rec, channels=[8, 0, 3, 4, 7, 1])
    sb = b.read_state()
    for i, c in enumerate([8, 0, 3, 4, 7, 1]):
        assert sb[c].tobytes() == st[i].tobytes()
    b.import_channels(rec[[2, 2]], channels=[5, 6])              # one record, two destinations
    assert b.read_state()[5].tobytes() == b.read_state()[6].tobytes() == st[2].tobytes()
    if kind == "fastconv":
        assert list(b.slots()) == [5, 0, 0, 63, 0, 63, 63, 0, 0] and b.gains()[8] == -2.5 and b.gains()[5] == 0.0
    # the same bytes come back; an existing bank takes the blob too
    assert b.export_bank_state().tobytes() == blob.tobytes()
    assert b.export_channels([8, 0, 3, 4, 7, 1]).tobytes() == rec.tobytes()
    c = make(A, kind)
    c.import_bank_state(blob); c.import_channels(rec)
    assert settings(c, kind) == settings(a, kind)
    assert c.export_bank_state().tobytes() == blob.tobytes() and c.export_channels().tobytes() == rec.tobytes()


def refused(A, t, kind, rec, channels, what):
    before = settings(t, kind)
    with pytest.raises(A.AsdrError, match=what):
        t.import_channels(rec, channels=channels)
    assert settings(t, kind) == before


@pytest.mark.parametrize("kind", KINDS)
def test_every_refused_channel_import_leaves_the_bank_alone(A, kind):
    a, t = make(A, kind), make(A, kind)
    dress(a, kind, 2); dress(t, kind, 3)
    good = a.export_channels()
    n = t.n_channels

    def bad(field, value, i=n - 1):     # the LAST record is wrong: the first ones must not have been written
        r = good.copy()
        A.tuner_channel_field(r, field)[i] = value
        return r
    refused(A, t, kind, good[:2], [0, n], "record 1: channel %d out of range" % n)
    refused(A, t, kind, good[:2], [0, -1], "out of range")
    refused(A, t, kind, good[:3], [1, 4, 1], "record 2: channel 1 named twice")
    refused(A, t, kind, bad("magic", 0x12345678), None, r"record %d \(channel %d\): bad magic" % (n - 1, n - 1))
    refused(A, t, kind, bad("version", 2), None, "version")
    refused(A, t, kind, bad("bytes", 2561), None, "bytes")
    refused(A, t, kind, bad("content", 8), None, "unknown content bits")
    refused(A, t, kind, bad("content", 2), None, "without the signal part")
    refused(A, t, kind, bad("kind", 1 - (kind == "fastconv")), None, "another kind")
    refused(A, t, kind, bad("decimation", 8), None, "taken at another")
    refused(A, t, kind, bad("fs_in", a.fs_in + 1), None, "Fs_in")
    refused(A, t, kind, bad("up", 3), None, "U / M")
    refused(A, t, kind, bad("down", 3), None, "U / M")
    refused(A, t, kind, bad("position", 128 * a.decimation), None, "position P = %d, the bank is at 0" % (128 * a.decimation))
    refused(A, t, kind, bad("output_position", 128), None, "output position 128")
    refused(A, t, kind, bad("src", t.n_sources), None, "source %d out of range" % t.n_sources)
    refused(A, t, kind, bad("src", -1), None, "out of range")
    refused(A, t, kind, bad("pos_a", 1), None, "anchor")
    refused(A, t, kind, bad("gain", np.float32(np.nan)), None, "gain")
    refused(A, t, kind, bad("gain", np.float32(32769.0)), None, "gain")
    if kind == "fastconv":
        refused(A, t, kind, bad("slot", 7), None, "slot 7 is undefined")
        refused(A, t, kind, bad("slot", 64), None, "slot")
        refused(A, t, kind, bad("slot", -1), None, "slot")
    else:
        refused(A, t, kind, bad("slot", 1), None, "slot must be 0")
        refused(A, t, kind, bad("gain", np.float32(2.0)), None, "gain must be 1")
    L = A.tuner._lib()
    before = settings(t, kind)
    for n_bad in (0, -1, n + 1):
        assert L.asdr_tuner_import_channels(t._h, None, n_bad, good.ctypes.data_as(C.c_void_p)) == -1
        assert L.asdr_tuner_export_channels(t._h, None, n_bad, good.ctypes.data_as(C.c_void_p)) == -1
    assert L.asdr_tuner_import_channels(t._h, None, 1, None) == -1 and L.asdr_tuner_export_channels(t._h, None, 1, None) == -1
    # the device forms need a device
    assert L.asdr_tuner_export_channels_device(t._h, None, 1, C.c_void_p(256), None) == -1 and b"ASDR_NO_DEVICE" in L.asdr_last_error()
    assert L.asdr_tuner_import_channels_device(t._h, None, 1, C.c_void_p(256), None) == -1 and b"ASDR_NO_DEVICE" in L.asdr_last_error()
    assert settings(t, kind) == before
    t.import_channels(good)             # ... and the good records still go in
    assert t.read_state().tobytes() == a.read_state().tobytes()


def test_a_wrong_geometry_refuses_records_and_blobs(A):
    a = make(A, "rate")
    rec, blob = a.export_channels(), a.export_bank_state()
    others = [A.TunerBank(6, 3, 25, fs_in=2400000, device=A.NO_DEVICE), A.TunerBank(6, 3, 50, fs_in=4410000, device=A.NO_DEVICE),
              A.TunerBank.fastconv(6, 3, 2400000, 16, device=A.NO_DEVICE), make(A, "plain")]
    for t in others:
        before = settings(t, "rate" if t.fft_size() == 0 else "fastconv")
        with pytest.raises(A.AsdrError, match="record 0"):
            t.import_channels(rec)
        with pytest.raises(A.AsdrError, match="bank state: taken"):
            t.import_bank_state(blob)
        assert settings(t, "rate" if t.fft_size() == 0 else "fastconv") == before
    t = A.TunerBank(6, 4, 50, fs_in=2400000, device=A.NO_DEVICE)       # another source count: records go in, the blob does not
    t.import_channels(rec)
    with pytest.raises(A.AsdrError, match="3 sources, this one has 4"):
        t.import_bank_state(blob)


@pytest.mark.parametrize("kind", KINDS)
def test_every_refused_blob_leaves_the_bank_alone(A, kind):
    a, t = make(A, kind), make(A, kind)
    dress(a, kind, 4); dress(t, kind, 5)
    good = a.export_bank_state()
    before = settings(t, kind)
    i32 = lambda b: b[:256].view("<i4")
    i64 = lambda b: b[:256].view("<i8")

    def no(blob, what, size=None):
        with pytest.raises(A.AsdrError, match="bank state: .*" + what):
            t.import_bank_state(blob if size is None else blob[:size])
        with pytest.raises(A.AsdrError, match="bank state: .*" + what):
            A.TunerBank.from_bank_state(blob if size is None else blob[:size], 2, device=A.NO_DEVICE)
        assert settings(t, kind) == before

    def edit(f):
        b = good.copy()
        f(b)
        return b
    no(good, "truncated", 255)
    no(good, "truncated", good.size - 1)
    no(good, "truncated", 0)
    no(edit(lambda b: b.__setitem__(0, 66)), "bad magic")
    no(edit(lambda b: i32(b).__setitem__(1, 2)), "version")
    no(edit(lambda b: i64(b).__setitem__(1, good.size + 16)), "the `bytes` word")
    no(edit(lambda b: i32(b).__setitem__(4, 4)), "unknown content bits")
    no(edit(lambda b: i64(b).__setitem__(16, 999)), "directory")                  # dir[0].offset
    no(edit(lambda b: i32(b).__setitem__(16, 5)), "input format")
    no(edit(lambda b: i64(b).__setitem__(6, 128 * a.decimation - 1)), "frame boundary")
    no(edit(lambda b: i64(b).__setitem__(7, 64)), "block boundary")
    no(edit(lambda b: i32(b).__setitem__(19, 0)), "length must be in")                # stage-1 taps
    no(edit(lambda b: i32(b).__setitem__(20, 16)), "gain shift")                      # g2
    no(edit(lambda b: i32(b).__setitem__(21, 65)), "K")
    no(edit(lambda b: i32(b).__setitem__(30, 2)), "statistics switch")
    off_h2, off_corr = int(i64(good)[18]), int(i64(good)[22])
    U = a.ratio()[0]
    no(edit(lambda b: b[off_h2:off_h2 + 2 * (2 * U + 1)].view("<i2").__setitem__(slice(None, None, U), 32767)), "65535")   # the three taps of phase 0
    no(edit(lambda b: b[off_corr + 12:off_corr + 16].view("<i4").__setitem__(0, 7)), "source 0: gain_q16")
    off_f = int(i64(good)[16])
    if kind == "fastconv":
        off_p = int(i64(good)[20])
        no(edit(lambda b: b[off_f:off_f + 4].view("<f4").__setitem__(0, np.inf)), "finite")
        no(edit(lambda b: b[off_p:off_p + 4].view("<i4").__setitem__(0, 130)), "palette slot 1")
        no(edit(lambda b: b[off_p + 4 * 1056 + 16:off_p + 4 * 1056 + 20].view("<f4").__setitem__(0, np.nan)), "palette slot 5")
        no(edit(lambda b: i32(b).__setitem__(22, 300)), "spectrum bins")
        no(edit(lambda b: i32(b).__setitem__(23, 2)), "window")
        no(edit(lambda b: i32(b).__setitem__(24, 2)), "mode")
        no(edit(lambda b: i32(b).__setitem__(25, 2)), "levels switch")
    else:
        no(edit(lambda b: i32(b).__setitem__(18, 16)), "gain shift")
        no(edit(lambda b: b[off_f:off_f + 8].view("<i2").__setitem__(slice(None), 32767)), r"sum of \|h\|")
        no(edit(lambda b: i32(b).__setitem__(25, 1)), "monitors")
    t.import_bank_state(good)
    assert not t.read_state().tobytes().strip(b"\0")        # every channel in creation state ...
    if kind == "fastconv":
        assert not t.slots().any() and (t.gains() == 1).all()
    t.import_channels(a.export_channels())                  # ... until its record follows
    assert settings(t, kind) == settings(a, kind)


def test_null_handles(A):
    L = A.tuner._lib()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    for rc in (L.asdr_tuner_export_channels(None, None, 1, p), L.asdr_tuner_import_channels(None, None, 1, p),
               L.asdr_tuner_export_channels_device(None, None, 1, p, None), L.asdr_tuner_import_channels_device(None, None, 1, p, None),
               L.asdr_tuner_export_bank_state(None, p, 4096), L.asdr_tuner_import_bank_state(None, p, 4096)):
        assert rc == -1 and b"null tuner bank" in L.asdr_last_error()
    t = make(A, "plain")
    assert L.asdr_tuner_export_bank_state(t._h, None, 4096) == -1 and L.asdr_tuner_import_bank_state(t._h, None, 4096) == -1
    assert L.asdr_tuner_export_bank_state(t._h, p, 100) == -1 and b"capacity" in L.asdr_last_error()
    assert not L.asdr_tuner_create_from_bank_state(None, 4096, 1, A.NO_DEVICE)
    assert L.asdr_tuner_channel_record_field(-1, None, None) is None and L.asdr_tuner_channel_record_field(1000, None, None) is None
