"""Receiver state records, host half (include/asdr.h "receiver state records"): the record's shape, the Chan <-> control-part round trip
with every hidden member, routing over shards, and the import as a transaction -- on control-plane-only batches (ASDR_NO_DEVICE)."""
import ctypes as C

import numpy as np
import pytest

from helpers import f32_bits
from test_control_plane import F_GETTERS, I_GETTERS

N_A, N_B = 13, 17
PERM = [(5 * c + 3) % N_B for c in range(N_A)]


def getters(b, ch):
    return ([f32_bits(np.float32(getattr(b, g)(ch))).item() for g in F_GETTERS] + [int(getattr(b, g)(ch)) for g in I_GETTERS] +
            [f32_bits(np.float32(b.getAGClookup(i, ch))).item() for i in range(130)] + [b.chain_constants(ch)[0]])


def script(b, ch, seed):
    """A seeded walk over the whole setter surface for one channel (the scripts of tests/test_control_plane*.py are the model); the AGC
    triple is distinct per seed."""
    r = np.random.RandomState(1000 + seed)
    b.setAGCthreshold(-60.0 + 1.5 * seed, ch=ch); b.setAGCslope(0.1 + 0.02 * seed, ch=ch); b.setAGCkneeWidth(2.0 + 0.25 * seed, ch=ch)
    steps = [
        lambda: b.setDemodMode(int(r.randint(0, 7)), ch=ch), lambda: b.setDemodMode(int(r.choice([7, -1, 9])), ch=ch),
        lambda: b.setInputGain(float(r.uniform(-1, 12)), ch=ch), lambda: b.setIQgainBalance(float(r.uniform(0.8, 1.2)), ch=ch),
        lambda: b.setOutputGain(float(r.uniform(0, 2)), ch=ch), lambda: b.setMute(int(r.randint(0, 2)), ch=ch),
        lambda: b.setAudioFilter(int(r.randint(0, 11)), ch=ch), lambda: b.enableAudioFilter(ch=ch), lambda: b.disableAudioFilter(ch=ch),
        lambda: b.enableALSfilter(ch=ch), lambda: b.disableALSfilter(ch=ch), lambda: b.setALSfilterPeak(ch=ch), lambda: b.setALSfilterNotch(ch=ch),
        lambda: b.setALSfilterStatic(ch=ch), lambda: b.setALSfilterAdaptive(ch=ch),
        lambda: b.setALSfilterParams(int(r.randint(0, 200)), float(r.uniform(0.01, 0.9)), float(r.randint(0, 70)), ch=ch),
        lambda: b.setAGCmode(int(r.randint(0, 4)), ch=ch), lambda: b.enableAGC(ch=ch), lambda: b.setAGChangTime(float(r.uniform(0, 900)), ch=ch),
        lambda: b.setAGCattackTime(float(r.uniform(0.5, 20)), ch=ch), lambda: b.setAGCreleaseTime(float(r.uniform(50, 2000)), ch=ch),
        lambda: b.setAGCstaticGain(float(r.uniform(1, 30)), ch=ch), lambda: b.setAGCslope(0.1 + 0.02 * seed, ch=ch),
        lambda: b.setNoiseBlankerThreshold(float(r.uniform(1.1, 4)), ch=ch), lambda: b.setNoiseBlankerThresholdDb(float(r.uniform(3, 20)), ch=ch),
        lambda: b.disableNoiseBlanker(ch=ch), lambda: b.enableNoiseBlanker(ch=ch),
    ]
    for i in r.randint(0, len(steps), size=40):
        steps[i]()
    if seed % 3 == 0:
        b.setIQgainBalance(1.0 + 0.01 * (seed + 1), ch=ch)      # ... so that the follow-up's setInputGain meets in_gain_i != in_gain_q


def follow_up(b, ch, seed):
    b.setInputGain(0.5 + 0.1 * seed, ch=ch)      # multiplies the MEMBER gain_balance (never the balance set above): AudioSDR.cpp:232-244
    b.setMute(1, ch=ch); b.setMute(0, ch=ch)     # out_gain -> current_out_gain
    b.setAGChangTime(33.0 + seed, ch=ch)         # lands in getAGClookup(129)


def make(A, n, devices=None):
    return A.AudioSDRBatch(n, device=A.NO_DEVICE) if devices is None else A.AudioSDRBatch(n, devices=devices)


def test_record_shape_header_and_field_table(A):
    n = A.state_record_bytes()
    assert n % 256 == 0 and n == A.AudioSDRBatch.STATE_RECORD_BYTES and n == A.load_library().asdr_state_record_bytes()
    a = make(A, 3)
    script(a, 1, 4)
    rec = a.export_state()
    assert rec.shape == (3, n) and rec.dtype == np.uint8
    hdr = rec[:, :16].view("<u4")
    assert (hdr[:, 0] == 0x52445341).all() and rec[0, :4].tobytes() == b"ASDR" and (hdr[:, 1] == 1).all() and (hdr[:, 2] == n).all()
    assert (hdr[:, 3] == 0).all()                     # a control-plane-only batch: neither "signal present" nor "audio_prev kept"
    fields = A.state_record_fields()
    assert [f[0] for f in fields[:4]] == ["magic", "version", "bytes", "content"] and len({f[0] for f in fields}) == len(fields)
    cover = np.zeros(n, int)
    for name, off, dt, shape in fields:
        size = dt.itemsize * (shape[0] if shape else 1)
        assert off % dt.itemsize == 0 and 0 <= off and off + size <= n, name
        cover[off:off + size] += 1
    assert cover.max() == 1, "fields overlap"
    assert not rec[:, cover == 0].any(), "a byte outside every field is not zero"
    for name in ("small", "nb_hist", "hil_q", "hil_i", "als_x", "als_w", "audio_prev"):   # every section 16-byte aligned
        off = {"small": 160}.get(name) or [f[1] for f in fields if f[0] == name][0]
        assert off % 16 == 0, name
    assert [f[1] for f in fields if f[0] == "in_gain"][0] == 16 and [f[1] for f in fields if f[0] == "nb_mask"][0] % 16 == 0
    assert float(A.state_field(rec, "agc_threshold")[1]) == a.getAGCthreshold(1)
    a.close()


def _round_trip(A, a, b):
    for c in range(N_A):
        script(a, c, c)
    for c in range(N_B):
        script(b, c, 50 + c)
    before_b = [getters(b, c) for c in range(N_B)]
    rec = a.export_state()
    b.import_state(rec, PERM)
    for c in range(N_A):
        assert getters(b, PERM[c]) == getters(a, c), "channel %d -> %d" % (c, PERM[c])
    for c in range(N_B):
        if c not in PERM:
            assert getters(b, c) == before_b[c], "untouched channel %d changed" % c
    assert np.array_equal(b.export_state(PERM), rec)
    for c in range(N_A):
        follow_up(a, c, c); follow_up(b, PERM[c], c)
    for c in range(N_A):
        assert getters(b, PERM[c]) == getters(a, c), "after the follow-up: channel %d -> %d" % (c, PERM[c])
    assert np.array_equal(b.export_state(PERM), a.export_state())
    return rec


def test_control_round_trip_with_hidden_members(A):
    a, b = make(A, N_A), make(A, N_B)
    _round_trip(A, a, b)
    # the destination's table pool: one live row per distinct triple in use (the padding channel's included), reference counts intact
    st = b.control_plane_flush()
    triples = {tuple(getters(b, c)[3:6]) for c in range(N_B)}
    assert st["agc_tables_alive"] in (len(triples), len(triples) + 1), (st, len(triples))
    a.close(); b.close()


def test_sharded_round_trip_across_shard_boundaries(A):
    """3 shards x 10 channels (boundaries at 3 and 6): an unsorted list that crosses both, into and out of sharded batches."""
    a, b = make(A, N_A), make(A, N_B)
    _round_trip(A, a, b)
    s = make(A, 10, devices=[A.NO_DEVICE] * 3)
    assert [s.shard_range(g) for g in range(3)] == [(0, 3), (3, 6), (6, 10)]
    order = [7, 2, 9, 4, 0, 5, 3]
    rec = b.export_state(PERM[:len(order)])
    for c in range(10):
        script(s, c, 80 + c)
    before = [getters(s, c) for c in range(10)]
    s.import_state(rec, order)
    for i, c in enumerate(order):
        assert getters(s, c) == getters(b, PERM[i]), "record %d -> sharded channel %d" % (i, c)
    for c in range(10):
        if c not in order:
            assert getters(s, c) == before[c]
    assert np.array_equal(s.export_state(order), rec)
    assert np.array_equal(s.export_state()[order], rec)                        # channels == NULL: every channel, in order
    for i, c in enumerate(order):
        follow_up(s, c, 100 + i); follow_up(b, PERM[i], 100 + i)
    for i, c in enumerate(order):
        assert getters(s, c) == getters(b, PERM[i]), "after the follow-up: record %d -> sharded channel %d" % (i, c)
    assert np.array_equal(s.export_state(order), b.export_state(PERM[:len(order)]))
    a.close(); b.close(); s.close()


@pytest.mark.parametrize("sharded", [False, True])
def test_rejections_change_nothing(A, sharded):
    src = make(A, 6)
    for c in range(6):
        script(src, c, 20 + c)
    good = src.export_state()
    b = make(A, 8, devices=[A.NO_DEVICE] * 2) if sharded else make(A, 8)
    for c in range(8):
        script(b, c, 30 + c)
    before = b.export_state()
    L, ip = A.load_library(), C.POINTER(C.c_int)

    def call(rec, chans, n=None):
        ch = np.asarray(chans, np.int32)
        rc = L.asdr_import_state(b._h, ch.ctypes.data_as(ip), len(chans) if n is None else n, rec.ctypes.data_as(C.c_void_p))
        msg = L.asdr_last_error().decode()
        assert np.array_equal(b.export_state(), before), "a rejected import changed the batch: %s" % msg
        return rc, msg

    ok = [6, 1, 4, 0, 7, 2]
    for field, value, word in (("magic", 0x12345678, "magic"), ("version", 2, "version"), ("bytes", 6144, "size")):
        bad = good.copy()
        A.state_field(bad, field)[3] = value           # records 0..2 in front of it are good ones
        rc, msg = call(bad, ok)
        assert rc < 0 and "record 3" in msg and word in msg, msg
    bad = good.copy(); A.state_field(bad, "content")[5] = 4
    rc, msg = call(bad, ok); assert rc < 0 and "record 5" in msg
    bad = good.copy(); A.state_field(bad, "if_table")[1] = 9
    rc, msg = call(bad, ok); assert rc < 0 and "record 1" in msg
    for chans, word in (([6, 1, 4, 8, 7, 2], "out of range"), ([6, 1, 4, -1, 7, 2], "out of range"), ([6, 1, 4, 0, 6, 2], "twice")):
        rc, msg = call(good, chans)
        assert rc < 0 and word in msg and ("record 3" in msg or "record 4" in msg), msg
    rc, msg = call(good, ok, n=-1)
    assert rc < 0 and "n < 0" in msg
    rc = L.asdr_export_state(b._h, np.asarray([0, 8], np.int32).ctypes.data_as(ip), 2, good.ctypes.data_as(C.c_void_p))
    assert rc < 0 and "out of range" in L.asdr_last_error().decode()
    assert L.asdr_export_state(b._h, None, -1, good.ctypes.data_as(C.c_void_p)) < 0
    b.import_state(good, ok)                           # ... and the same call with good records goes through
    assert np.array_equal(b.export_state(ok), good)
    with pytest.raises(A.AsdrError):
        b.export_state_device(4096)                    # the device forms need a device
    src.close(); b.close()
