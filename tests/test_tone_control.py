"""The tone squelch's control plane (include/asdr_tone.h) on an ASDR_NO_DEVICE handle: the creation values, the bank-wide and
per-channel setters and getters with their ends, that each refusal leaves everything as it was, write_state's validation, the two
helpers against the restatement, the call that needs a device, the exported names and the record's layout."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import tone_ref as TR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def squelch(A, n=6):
    return A.ToneSquelch(n, device=A.NO_DEVICE)


def settings(t):
    hz, steps = t.get_tones()
    return (hz.tolist(), steps.tolist(), t.get_window(), t.get_dominance(), t.get_highpass().tolist(),
            [(t.get_want(c), t.get_min_power(c), t.get_hang(c)) for c in range(t.n_channels)])


def creation_records(n):
    return TR.ToneRef(n).records().tobytes()


def test_every_declared_name_is_exported_and_bound(A):
    with open(os.path.join(ROOT, "include", "asdr_tone.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(asdr_tone_\w+)\s*\(", text)))
    assert len(declared) == 26 and "asdr_tone_update_device" in declared and "asdr_tone_highpass_design" in declared
    L = ctypes.CDLL(A.library_path())
    for n in declared:
        assert hasattr(L, n), n
    assert sorted(A.TONE_EXPORTS) == declared
    assert sorted("asdr_tone_" + k for k in A.tone._API) == declared     # every one has its types set
    other_lists = (A.binding.EXPORTS, A.GATE_EXPORTS, A.TUNER_EXPORTS, A.FRONT_EXPORTS, A.RESAMPLE_EXPORTS, A.CODEC_EXPORTS,
                   A.SPECTROGRAM_EXPORTS, A.FM_EXPORTS)
    others = set().union(*other_lists)
    assert not [n for n in A.TONE_EXPORTS if n in others]
    for lst in other_lists:
        assert not [n for n in lst if n.startswith("asdr_tone_")]
    for name in ("ToneSquelch", "TONE_EXPORTS", "TONE_STATE_DTYPE", "CTCSS_TONES", "tone_highpass_design", "tone_min_power"):
        assert hasattr(A, name), name


def test_the_state_record_is_704_bytes_and_the_header_holds_the_ctcss_table(A):
    assert A.TONE_STATE_DTYPE.itemsize == 704 and A.TONE_STATE_DTYPE.names == TR.STATE_NAMES
    assert tuple(A.TONE_STATE_DTYPE.fields[k][1] for k in TR.STATE_NAMES) == TR.STATE_OFFSETS
    assert all(A.TONE_STATE_DTYPE.fields[k][0] == TR.STATE_DTYPE.fields[k][0] for k in TR.STATE_NAMES)
    src = "#include <stddef.h>\n#include \"asdr_tone.h\"\n_Static_assert(sizeof(asdr_tone_state_t) == 704 && sizeof(asdr_tone_state_t) % 16 == 0, \"size\");\n"
    for name, off in zip(TR.STATE_NAMES, TR.STATE_OFFSETS):
        src += "_Static_assert(offsetof(asdr_tone_state_t, %s) == %d, \"%s\");\n" % (name, off, name)
    src += "_Static_assert(sizeof(ASDR_CTCSS_TONES) == 50 * sizeof(double) && ASDR_TONE_PASS == -2 && ASDR_TONE_ANY == -1, \"table\");\n"
    r = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(ROOT, "include", "asdr_tone.h")) as f:
        body = re.search(r"ASDR_CTCSS_TONES\[ASDR_CTCSS_COUNT\] = \{(.*?)\};", f.read(), flags=re.S).group(1)
    assert tuple(float(v) for v in body.split(",")) == A.CTCSS_TONES == TR.CTCSS and len(A.CTCSS_TONES) == 50
    assert (A.TONE_PASS, A.TONE_ANY) == (TR.PASS, TR.ANY) == (-2, -1)
    t = squelch(A, 3)
    st = t.read_state()                                        # the library fills exactly 3 * 704 bytes
    assert st.shape == (3,) and st.nbytes == 2112


def test_creation_values(A):
    t = squelch(A)
    assert t.n_channels == 6 and t._L.asdr_tone_n_channels(t._h) == 6 and t.blocks() == 0
    ref = TR.ToneRef(6)                                         # the restatement starts from the same values
    want = (list(TR.CTCSS), TR.steps_from_hz(TR.CTCSS), 64, 64, [], [(TR.PASS, 0, 0)] * 6)
    assert settings(t) == want
    assert (ref.hz, ref.steps, ref.window, ref.dominance, ref.coef) == want[:5]
    assert list(zip(ref.want.tolist(), ref.min_power.tolist(), ref.hang_windows.tolist())) == want[5]
    st = t.read_state()
    assert st.tobytes() == creation_records(6) and (st["detected"] == -1).all() and (st["last_best"] == -1).all()
    assert np.isnan(t.decoded_hz()).all()
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(A.AsdrError, match="n_channels"):
            A.ToneSquelch(n, device=A.NO_DEVICE)


def test_bank_wide_setters_their_ends_and_refusals(A):
    t = squelch(A)
    rec = t.read_state()
    rec["acc"][:, :50] = 7; rec["window_block"] = 9; rec["open"] = 1; rec["detected"] = 3; rec["windows"] = 5; rec["hist"] = 11
    t.write_state(rec)
    kept = t.read_state()
    kept["acc"] = 0; kept["window_block"] = 0                                   # what a new table or window leaves

    t.set_window(16)
    assert t.get_window() == 16 and t.read_state().tobytes() == kept.tobytes()
    t.write_state(rec)
    t.set_window(128)
    assert t.get_window() == 128 and t.read_state().tobytes() == kept.tobytes()
    t.set_dominance(16); assert t.get_dominance() == 16
    t.set_dominance(1024); assert t.get_dominance() == 1024
    sixty_four = [20.0 + 21.0 * k for k in range(64)]
    t.write_state(rec)
    t.set_tones(sixty_four)
    assert t.get_tones()[0].tolist() == sixty_four and t.get_tones()[1].tolist() == TR.steps_from_hz(sixty_four)
    assert t.read_state().tobytes() == kept.tobytes()
    t.set_tones([1377.9]); assert t.get_tones()[1].tolist() == TR.steps_from_hz([1377.9])
    t.set_tones([100.0, 200.0, 300.0])
    c3 = TR.highpass_design(300.0, 3)
    t.set_highpass(c3); assert t.get_highpass().tolist() == c3
    t.set_highpass(fc_hz=150.0, sections=1); assert t.get_highpass().tolist() == TR.highpass_design(150.0, 1)
    t.set_highpass([[2**31 - 1, -2**31, 0, 1, -1]]); assert t.get_highpass().tolist() == [[2**31 - 1, -2**31, 0, 1, -1]]
    t.set_highpass(None); assert t.get_highpass().tolist() == []
    t.set_highpass(c3[:2])
    t.set_want(2, ch=1); t.set_min_power(2**64 - 1, ch=2); t.set_hang(255, ch=3)
    before, state = settings(t), t.read_state().tobytes()

    for table, why in (([100.0, 100.0], "ascend"), ([100.0, 90.0], "ascend"), ([100.0, 100.0 + 1e-9], "ascend"),
                       ([10.0 + k for k in range(65)], "n_tones"), ([], "n_tones"), ([1378.0], "below 1378"), ([0.0, 5.0], "above 0"),
                       ([-5.0], "above 0"), ([float("nan")], "above 0")):
        with pytest.raises(A.AsdrError, match=why):
            t.set_tones(table)
    for W in (15, 129, 0, -1, 1 << 20):
        with pytest.raises(A.AsdrError, match="window"):
            t.set_window(W)
    for d in (15, 1025, 0, -64):
        with pytest.raises(A.AsdrError, match="dominance"):
            t.set_dominance(d)
    with pytest.raises(A.AsdrError, match="sections"):
        t.set_highpass(c3 + c3[:1])                                             # 4 sections
    with pytest.raises(A.AsdrError, match="int32"):
        t.set_highpass([[2**31, 0, 0, 0, 0]])
    with pytest.raises(A.AsdrError, match="sections"):
        A.tone_highpass_design(300.0, 4)
    for fc in (0.0, 22050.0, -1.0):
        with pytest.raises(A.AsdrError, match="fc_hz"):
            A.tone_highpass_design(fc, 2)
    assert settings(t) == before and t.read_state().tobytes() == state          # every refusal left everything as it was
    assert before[0] == [100.0, 200.0, 300.0] and before[2:5] == (128, 1024, c3[:2])
    assert t._L.asdr_tone_set_window(None, 64) == -1 and t._L.asdr_tone_blocks(None) == -1 and t._L.asdr_tone_get_window(None) == -1
    t.reset()                                                                   # keeps the settings
    assert settings(t) == before and t.read_state().tobytes() == creation_records(6)


def test_per_channel_setters_their_ends_and_refusals(A):
    t = squelch(A)
    t.set_want(A.TONE_ANY); t.set_min_power(10**13); t.set_hang(2)               # broadcast
    assert settings(t)[5] == [(-1, 10**13, 2)] * 6
    t.set_want(49, ch=4); t.set_min_power(2**64 - 1, ch=4); t.set_hang(255, ch=4)   # the upper ends
    t.set_want(A.TONE_PASS, ch=0); t.set_min_power(0, ch=0); t.set_hang(0, ch=0)    # the lower ends
    t.set_want(0, ch=2)
    want = [(-2, 0, 0), (-1, 10**13, 2), (0, 10**13, 2), (-1, 10**13, 2), (49, 2**64 - 1, 255), (-1, 10**13, 2)]
    assert settings(t)[5] == want
    for ch in (0, 4, A.ALL):
        for w in (50, -3, 64, 1 << 20):
            with pytest.raises(A.AsdrError, match="want"):
                t.set_want(w, ch=ch)
        for h in (256, -1, 1 << 20):
            with pytest.raises(A.AsdrError, match="hang_windows"):
                t.set_hang(h, ch=ch)
        for p in (-1, 2**64):
            with pytest.raises(A.AsdrError, match="min_power"):
                t.set_min_power(p, ch=ch)
    for ch in (-2, 6, 1 << 20):
        for call in (lambda: t.set_want(0, ch=ch), lambda: t.set_min_power(5, ch=ch), lambda: t.set_hang(5, ch=ch), lambda: t.get_want(ch),
                     lambda: t.get_min_power(ch), lambda: t.get_hang(ch)):
            with pytest.raises(A.AsdrError, match="bad channel"):
                call()
    with pytest.raises(A.AsdrError, match="bad channel"):
        t.get_want(A.ALL)
    assert settings(t)[5] == want


def test_write_state_checks_every_record_before_it_writes_one(A):
    t = squelch(A)
    t.set_tones([100.0, 200.0, 300.0, 400.0]); t.set_window(20)
    rec = np.zeros(3, dtype=A.TONE_STATE_DTYPE)
    rec["hist"] = np.arange(144).reshape(3, 48) - 70; rec["hist"][0, :2] = (-32768, 32767)
    rec["hp"] = np.arange(36).reshape(3, 3, 4) * 10**7 - 2**30; rec["hp"][1, 0, :2] = (-2**31, 2**31 - 1)
    rec["last_power"] = [2**64 - 1, 0, 9]; rec["last_other"] = [2**63, 1, 2]
    rec["windows"] = [2**32 - 1, 0, 1]; rec["matches"] = [5, 0, 1]; rec["openings"] = [2**32 - 1, 0, 1]; rec["open_blocks"] = [5, 0, 1]
    rec["detected"] = [3, -1, 0]; rec["last_best"] = [-1, 3, 2]; rec["window_block"] = [19, 0, 7]; rec["hang_left"] = [255, 0, 9]
    rec["open"] = [1, 0, 1]
    rec["acc"][:, :4] = np.array([[-2**31, 2**31 - 1], [1, -1], [0, 5], [7, 0]])
    t.write_state(rec, channels=[5, 0, 2])
    want = TR.ToneRef(6).records()
    for k, c in enumerate([5, 0, 2]):
        want[c] = rec[k]
    assert t.read_state().tobytes() == want.tobytes()                           # hang_left above hang_windows (0) is allowed
    assert np.array_equal(t.decoded_hz(), [np.nan, np.nan, 100.0, np.nan, np.nan, 400.0], equal_nan=True)
    bad = rec.copy(); bad["windows"] = 77
    for field, value, why in (("open", 2, "open must be 0 or 1"), ("open", 255, "open must be 0 or 1"), ("window_block", 20, "window_block"),
                              ("window_block", 65535, "window_block"), ("detected", 4, "detected"), ("detected", -2, "detected"),
                              ("last_best", 4, "last_best"), ("last_best", -32768, "last_best"), ("reserved", (1, 0), "reserved"),
                              ("reserved", (0, 1 << 31), "reserved")):
        b = bad.copy(); b[field][2] = value                                     # the LAST record is the bad one
        with pytest.raises(A.AsdrError, match=why):
            t.write_state(b, channels=[1, 3, 4])
    for slot in ((4, 0), (4, 1), (63, 1)):
        b = bad.copy(); b["acc"][2][slot] = 1
        with pytest.raises(A.AsdrError, match="acc must be 0"):
            t.write_state(b, channels=[1, 3, 4])
    for chans in ([1, 3, 6], [1, -1, 3], [1 << 20, 0, 1]):
        with pytest.raises(A.AsdrError, match="bad channel"):
            t.write_state(bad, channels=chans)
    with pytest.raises(A.AsdrError, match="more records"):
        t.write_state(np.zeros(7, dtype=A.TONE_STATE_DTYPE))
    with pytest.raises(A.AsdrError, match="records for"):
        t.write_state(bad, channels=[1, 2])
    assert t.read_state().tobytes() == want.tobytes()
    t.write_state(rec[:2])                                                      # channels 0, 1
    assert t.read_state()[:2].tobytes() == rec[:2].tobytes()
    before = t.read_state()
    t.clear()                                                                   # zeroes the four counters only
    st = t.read_state()
    for k in TR.STATE_NAMES:
        if k in ("windows", "matches", "openings", "open_blocks"):
            assert not st[k].any() and before[k].any(), k
        else:
            assert np.array_equal(st[k], before[k]), k
    t.reset()
    assert t.read_state().tobytes() == creation_records(6) and t.blocks() == 0


def test_the_helpers_agree_with_the_restatement(A):
    for fc in (300.0, 150.0, 67.0, 1000.0, 0.5, 20000.0):
        for sections in (1, 2, 3):
            assert A.tone_highpass_design(fc, sections).tolist() == TR.highpass_design(fc, sections), (fc, sections)
    assert A.tone_highpass_design(300.0, 0).shape == (0, 5)
    for amplitude in (0, 1, 1000, 3277, 32767, 32768):
        for W in (16, 64, 127, 128):
            assert A.tone_min_power(amplitude, W) == TR.min_power(amplitude, W) == (128 * amplitude * W) ** 2 // 4
    assert A.tone_min_power(1000, 64) == 16777216000000
    for amplitude, W in ((1000, 15), (1000, 129), (-1, 64), (32769, 64), (float("nan"), 64)):
        with pytest.raises(A.AsdrError, match="window|amplitude"):
            A.tone_min_power(amplitude, W)


def test_the_signal_path_needs_a_device(A):
    t = squelch(A)
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        t.update_device(4096, 16384, 1)
    t.synchronize()
    assert t.blocks() == 0 and t.read_state().tobytes() == creation_records(6)
