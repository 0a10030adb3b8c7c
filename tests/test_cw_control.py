"""The CW decoder's control plane (include/asdr_cw.h) on an ASDR_NO_DEVICE handle: the creation values, every setter and getter with
its ends, that each refusal leaves everything as it was, set_speed, write_state's validation, clear and reset, the helpers and the
tables against the restatement, the calls that need a device, the exported names and the layouts of the record and the event."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cw_ref as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STEP = R.pitch_step(774)


def decoder(A, n=6, ring=4):
    return A.CwDecoder(n, ring=ring, device=A.NO_DEVICE)


def settings(t):
    return [t.get_settings(c) for c in range(t.n_channels)]


def creation_records(n):
    return R.CwRef(n).records().tobytes()


def test_every_declared_name_is_exported_and_bound(A):
    with open(os.path.join(ROOT, "include", "asdr_cw.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(asdr_cw_\w+)\s*\(", text)))
    assert len(declared) == 21 and "asdr_cw_update_device" in declared and "asdr_cw_collect_device" in declared
    L = ctypes.CDLL(A.library_path())
    for n in declared:
        assert hasattr(L, n), n
    assert sorted(A.CW_EXPORTS) == declared
    assert sorted("asdr_cw_" + k for k in A.cw._API) == declared               # every one has its types set
    other_lists = (A.binding.EXPORTS, A.GATE_EXPORTS, A.TUNER_EXPORTS, A.FRONT_EXPORTS, A.RESAMPLE_EXPORTS, A.CODEC_EXPORTS,
                   A.SPECTROGRAM_EXPORTS, A.FM_EXPORTS, A.TONE_EXPORTS, A.DCS_EXPORTS, A.PACKET_EXPORTS)
    others = set().union(*other_lists)
    assert not [n for n in A.CW_EXPORTS if n in others]
    for lst in other_lists:
        assert not [n for n in lst if n.startswith("asdr_cw_")]
    for name in ("CwDecoder", "CW_EXPORTS", "CW_STATE_DTYPE", "CW_EVENT_DTYPE", "CW_ROWS", "CW_NARROW_ROWS", "CW_WIDE_CHANNELS",
                 "CW_MAX_RING", "CW_FLAG_UNKNOWN", "cw_pitch_step"):
        assert hasattr(A, name), name
    for method in ("set_pitch_step", "set_pitch", "set_min_power", "set_glitch", "set_track", "get_settings", "set_speed", "update_device",
                   "collect_device", "deliver", "ring_state", "read_state", "write_state", "clear", "reset", "blocks", "synchronize",
                   "close", "text"):
        assert callable(getattr(A.CwDecoder, method)), method


def test_the_record_is_80_bytes_and_the_event_16(A):
    assert A.CW_STATE_DTYPE.itemsize == 80 and A.CW_STATE_DTYPE.names == R.STATE_NAMES
    assert tuple(A.CW_STATE_DTYPE.fields[k][1] for k in R.STATE_NAMES) == R.STATE_OFFSETS
    assert all(A.CW_STATE_DTYPE.fields[k][0] == R.STATE_DTYPE.fields[k][0] for k in R.STATE_NAMES)
    assert A.CW_EVENT_DTYPE.itemsize == 16 and A.CW_EVENT_DTYPE.names == R.EVENT_DTYPE.names
    assert all(A.CW_EVENT_DTYPE.fields[k] == R.EVENT_DTYPE.fields[k] for k in R.EVENT_DTYPE.names)
    src = ("#include <stddef.h>\n#include \"asdr_cw.h\"\n"
           "_Static_assert(sizeof(asdr_cw_state_t) == 80 && sizeof(asdr_cw_state_t) % 16 == 0, \"size\");\n"
           "_Static_assert(sizeof(asdr_cw_event_t) == 16, \"event\");\n")
    for name, off in zip(R.STATE_NAMES, R.STATE_OFFSETS):
        src += "_Static_assert(offsetof(asdr_cw_state_t, %s) == %d, \"%s\");\n" % (name, off, name)
    for name in R.EVENT_DTYPE.names:
        src += "_Static_assert(offsetof(asdr_cw_event_t, %s) == %d, \"%s\");\n" % (name, R.EVENT_DTYPE.fields[name][1], name)
    src += ("_Static_assert(ASDR_CW_PITCH_HZ == 774 && ASDR_CW_MIN_POWER == 16 && ASDR_CW_GLITCH == 4 && ASDR_CW_MAX_GLITCH == 16 && "
            "ASDR_CW_SLOW_SHIFT == 10 && ASDR_CW_FAST_SHIFT == 2 && ASDR_CW_MIN_D == 441 && ASDR_CW_MAX_D == 5292 && "
            "ASDR_CW_DIT_UNITS == 26460 && ASDR_CW_MAX_RING == 64 && ASDR_CW_RING == 16 && sizeof(ASDR_CW_TABLE) == 256, \"constants\");\n")
    r = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t = decoder(A, 3)
    st = t.read_state()                                        # the library fills exactly 3 * 80 bytes
    assert st.shape == (3,) and st.nbytes == 240


def test_creation_values(A):
    t = decoder(A)
    assert t.n_channels == 6 and t._L.asdr_cw_n_channels(t._h) == 6 and t.blocks() == 0
    ref = R.CwRef(6)
    assert settings(t) == [(STEP, 16, 4, 1)] * 6 == list(zip(ref.pitch_step.tolist(), ref.min_power.tolist(), ref.glitch.tolist(), ref.track.tolist()))
    st = t.read_state()
    assert st.tobytes() == creation_records(6) and (st["D"] == 1323).all() and (st["sym"] == 1).all()
    pending, lost = t.ring_state()
    assert pending.tolist() == [0] * 6 and lost.tolist() == [0] * 6
    assert A.CwDecoder(2, device=A.NO_DEVICE).ring == 16                        # the default ring
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(A.AsdrError, match="n_channels"):
            A.CwDecoder(n, device=A.NO_DEVICE)
    for ring in (0, 65, -1, 1 << 20):
        with pytest.raises(A.AsdrError, match="ring"):
            A.CwDecoder(4, ring=ring, device=A.NO_DEVICE)
    for ring in (1, 64):
        A.CwDecoder(4, ring=ring, device=A.NO_DEVICE).close()


def test_the_setters_their_ends_and_refusals(A):
    t = decoder(A)
    t.set_pitch_step(12345); t.set_min_power(700); t.set_glitch(9); t.set_track(0)          # broadcast
    assert settings(t) == [(12345, 700, 9, 0)] * 6
    t.set_pitch_step(0, ch=0); t.set_pitch_step(2**32 - 1, ch=5); t.set_pitch(600.0, ch=2)
    t.set_min_power(0, ch=0); t.set_min_power(2**32 - 1, ch=5)
    t.set_glitch(1, ch=0); t.set_glitch(16, ch=5)
    t.set_track(1, ch=3)
    want = [(0, 0, 1, 0), (12345, 700, 9, 0), (R.pitch_step(600.0), 700, 9, 0), (12345, 700, 9, 1), (12345, 700, 9, 0),
            (2**32 - 1, 2**32 - 1, 16, 0)]
    assert settings(t) == want
    state = t.read_state().tobytes()
    for ch in (0, 5, A.ALL):
        for g in (0, 17, -1, 1 << 20):
            with pytest.raises(A.AsdrError, match="glitch"):
                t.set_glitch(g, ch=ch)
        for v in (2, -1, 255):
            with pytest.raises(A.AsdrError, match="track"):
                t.set_track(v, ch=ch)
        for v in (-1, 2**32):
            with pytest.raises(A.AsdrError, match="pitch_step"):
                t.set_pitch_step(v, ch=ch)
            with pytest.raises(A.AsdrError, match="min_power"):
                t.set_min_power(v, ch=ch)
        for hz in (99.9, 3000.1, -774.0, float("nan")):
            with pytest.raises(A.AsdrError, match="100..3000"):
                t.set_pitch(hz, ch=ch)
        for wpm in (4, 61, 0, -20):
            with pytest.raises(A.AsdrError, match="wpm"):
                t.set_speed(wpm, ch=ch)
    for ch in (-2, 6, 1 << 20):
        for call in (lambda: t.set_pitch_step(1, ch=ch), lambda: t.set_min_power(1, ch=ch), lambda: t.set_glitch(4, ch=ch),
                     lambda: t.set_track(1, ch=ch), lambda: t.set_speed(20, ch=ch), lambda: t.get_settings(ch)):
            with pytest.raises(A.AsdrError, match="bad channel"):
                call()
    with pytest.raises(A.AsdrError, match="bad channel"):
        t.get_settings(A.ALL)
    assert settings(t) == want and t.read_state().tobytes() == state
    assert t._L.asdr_cw_set_glitch(None, 0, 4) == -1 and t._L.asdr_cw_blocks(None) == -1
    assert t._L.asdr_cw_n_channels(None) == -1 and t._L.asdr_cw_ring_state(None, None, None) == -1
    assert t._L.asdr_cw_ring_state(t._h, None, None) == 0      # either array may be NULL
    assert t._L.asdr_cw_get_settings(t._h, 0, None, None, None, None) == 0
    t.reset()                                                   # keeps the settings
    assert settings(t) == want and t.read_state().tobytes() == creation_records(6)


def test_set_speed_writes_d(A):
    t = decoder(A)
    ref = R.CwRef(6)
    for wpm, ch in ((5, 0), (60, 5), (12, 2)):
        t.set_speed(wpm, ch=ch); ref.set_speed(wpm, ch=ch)
    assert t.read_state()["D"].tolist() == [5292, 1323, 2205, 1323, 1323, 441] and t.read_state().tobytes() == ref.records().tobytes()
    rec = t.read_state(); rec["marks"] = 7; rec["sym"] = 5
    t.write_state(rec)
    t.set_speed(35)                                             # every channel; nothing else of the record moves
    rec["D"] = 756
    assert t.read_state().tobytes() == rec.tobytes() and R.dit_of(35) == 756


def filled_records(A):
    rec = np.zeros(3, dtype=A.CW_STATE_DTYPE)
    rec["ph"] = [2**32 - 1, 0, 123456789]
    rec["prev_i"] = [[1 << 20, -(1 << 20), 5], [0, 0, 0], [-7, 8, -9]]
    rec["prev_q"] = [[-(1 << 20), 1 << 20, -5], [0, 0, 0], [70, -80, 90]]
    rec["hi"] = [2**32 - 1, 0, 5000]; rec["lo"] = [2**32 - 1, 0, 6000]
    rec["D"] = [5292, 441, 1323]; rec["run"] = [2**32 - 1, 0, 99]
    for k, name in enumerate(("marks", "chars", "unknown", "glitches")):
        rec[name] = [2**32 - 1, 0, k + 1]
    rec["cnt"] = [16, 0, 3]; rec["key"] = [1, 0, 1]; rec["sym"] = [255, 0, 1]; rec["gap"] = [1, 0, 1]
    return rec


def test_write_state_checks_every_record_before_it_writes_one(A):
    t = decoder(A)
    rec = filled_records(A)
    t.write_state(rec, channels=[5, 0, 2])
    want = R.CwRef(6).records()
    for k, c in enumerate([5, 0, 2]):
        want[c] = rec[k]
    assert t.read_state().tobytes() == want.tobytes()
    bad = rec.copy(); bad["marks"] = 77
    reserved_low, reserved_high = [0] * 4, [0] * 4
    reserved_low[0], reserved_high[3] = 1, 1 << 31
    for field, value, why in (("D", 440, "D must"), ("D", 5293, "D must"), ("D", 0, "D must"), ("D", 2**32 - 1, "D must"),
                              ("key", 2, "key must be 0 or 1"), ("key", 255, "key"), ("gap", 2, "gap must be 0 or 1"), ("cnt", 17, "cnt"),
                              ("cnt", 255, "cnt"), ("prev_i", [0, (1 << 20) + 1, 0], "prev_i"), ("prev_q", [0, 0, -(1 << 20) - 1], "prev_i"),
                              ("reserved", reserved_low, "reserved"), ("reserved", reserved_high, "reserved")):
        b = bad.copy(); b[field][2] = value                                     # the LAST record is the bad one
        with pytest.raises(A.AsdrError, match=why):
            t.write_state(b, channels=[1, 3, 4])
    for chans in ([1, 3, 6], [1, -1, 3], [1 << 20, 0, 1]):
        with pytest.raises(A.AsdrError, match="bad channel"):
            t.write_state(bad, channels=chans)
    with pytest.raises(A.AsdrError, match="more records"):
        t.write_state(np.zeros(7, dtype=A.CW_STATE_DTYPE))
    with pytest.raises(A.AsdrError, match="records for"):
        t.write_state(bad, channels=[1, 2])
    assert t.read_state().tobytes() == want.tobytes()
    t.write_state(rec[:2])                                                      # channels 0, 1
    assert t.read_state()[:2].tobytes() == rec[:2].tobytes()


def test_clear_and_reset(A):
    t = decoder(A)
    t.set_glitch(7, ch=1)
    t.write_state(filled_records(A), channels=[0, 3, 4])
    before = t.read_state()
    t.clear()                                                                   # zeroes three counters; chars and everything else stay
    st = t.read_state()
    ref = R.CwRef(6)
    for c in range(6):
        ref.put(c, before[c])
    ref.clear()
    assert st.tobytes() == ref.records().tobytes()
    for k in R.STATE_NAMES:
        if k in R.COUNTERS:
            assert not st[k].any() and before[k].any(), k
        else:
            assert np.array_equal(st[k], before[k]), k
    assert st["chars"].tolist() == [2**32 - 1, 0, 0, 0, 2, 0] and "chars" not in R.COUNTERS
    assert t.blocks() == 0 and t.ring_state()[1].tolist() == [0] * 6
    t.reset()
    assert t.read_state().tobytes() == creation_records(6) and t.blocks() == 0 and settings(t)[1] == (STEP, 16, 7, 1)
    assert t.ring_state()[0].tolist() == [0] * 6


def test_the_helpers_and_the_tables_agree_with_the_restatement(A):
    L = A.load_library()
    A.cw._lib()
    for hz in (100, 774, 600.5, 1000, 2999.99, 3000):
        assert A.cw_pitch_step(hz) == R.pitch_step(hz), hz
    assert A.cw_pitch_step(774) == STEP == 75381059
    for hz in (99.999, 3000.001, 0, -1):
        with pytest.raises(A.AsdrError, match="100..3000"):
            A.cw_pitch_step(hz)
    assert [L.asdr_cw_cos(j) for j in range(1024)] == R.COS.tolist()
    assert L.asdr_cw_cos(1024) == 1024 and L.asdr_cw_cos(-256) == R.COS[768]
    ev = np.zeros(5, dtype=A.CW_EVENT_DTYPE)
    ev["channel"] = [0, 1, 0, 1, 0]; ev["ch"] = [ord(c) for c in "CAQB "]
    assert A.CwDecoder.text(ev) == "CAQB " and A.CwDecoder.text(ev, channel=0) == "CQ " and A.CwDecoder.text(ev, channel=1) == "AB"
    assert A.CwDecoder.text(ev[:0]) == ""


def test_the_signal_path_and_the_delivery_need_a_device(A):
    t = decoder(A)
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        t.update_device(4096, 1)
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        t.collect_device(4096, 8192, 4)
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        t.deliver()
    t.synchronize()
    assert t.blocks() == 0 and t.read_state().tobytes() == creation_records(6)
