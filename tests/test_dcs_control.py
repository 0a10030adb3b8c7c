"""The DCS squelch's control plane (include/asdr_dcs.h) on an ASDR_NO_DEVICE handle: the creation values, the bank-wide and
per-channel setters and getters with their ends, that each refusal leaves everything as it was (the distance rule between the table and
max_errors, in both orders, among them), write_state's validation, the helpers against the restatement, the call
that needs a device, the exported names and the record's layout."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dcs_ref as DR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def squelch(A, n=6):
    return A.DcsSquelch(n, device=A.NO_DEVICE)


def settings(t):
    codes, words = t.get_codes()
    return (codes.tolist(), words.tolist(), t.get_max_errors(), t.get_confirm(), t.get_hold_bits(),
            [(t.get_want(c), t.get_hysteresis(c)) for c in range(t.n_channels)])


def creation_records(n):
    return DR.DcsRef(n).records().tobytes()


def test_every_declared_name_is_exported_and_bound(A):
    with open(os.path.join(ROOT, "include", "asdr_dcs.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(asdr_dcs_\w+)\s*\(", text)))
    assert len(declared) == 24 and "asdr_dcs_update_device" in declared and "asdr_dcs_find" in declared
    L = ctypes.CDLL(A.library_path())
    for n in declared:
        assert hasattr(L, n), n
    assert sorted(A.DCS_EXPORTS) == declared
    assert sorted("asdr_dcs_" + k for k in A.dcs._API) == declared       # every one has its types set
    other_lists = (A.binding.EXPORTS, A.GATE_EXPORTS, A.TUNER_EXPORTS, A.FRONT_EXPORTS, A.RESAMPLE_EXPORTS, A.CODEC_EXPORTS,
                   A.SPECTROGRAM_EXPORTS, A.FM_EXPORTS, A.TONE_EXPORTS)
    others = set().union(*other_lists)
    assert not [n for n in A.DCS_EXPORTS if n in others]
    for lst in other_lists:
        assert not [n for n in lst if n.startswith("asdr_dcs_")]
    for name in ("DcsSquelch", "DCS_EXPORTS", "DCS_STATE_DTYPE", "DCS_CODES", "DCS_PASS", "DCS_ANY", "dcs_word", "DCS_ROWS",
                 "DCS_NARROW_ROWS", "DCS_WIDE_CHANNELS"):
        assert hasattr(A, name), name
    assert callable(A.DcsSquelch.find)


def test_the_state_record_is_192_bytes_and_the_header_holds_the_code_table(A):
    assert A.DCS_STATE_DTYPE.itemsize == 192 and A.DCS_STATE_DTYPE.names == DR.STATE_NAMES
    assert tuple(A.DCS_STATE_DTYPE.fields[k][1] for k in DR.STATE_NAMES) == DR.STATE_OFFSETS
    assert all(A.DCS_STATE_DTYPE.fields[k][0] == DR.STATE_DTYPE.fields[k][0] for k in DR.STATE_NAMES)
    src = "#include <stddef.h>\n#include \"asdr_dcs.h\"\n_Static_assert(sizeof(asdr_dcs_state_t) == 192 && sizeof(asdr_dcs_state_t) % 16 == 0, \"size\");\n"
    for name, off in zip(DR.STATE_NAMES, DR.STATE_OFFSETS):
        src += "_Static_assert(offsetof(asdr_dcs_state_t, %s) == %d, \"%s\");\n" % (name, off, name)
    src += ("_Static_assert(sizeof(ASDR_DCS_CODES) == 104 * sizeof(uint16_t) && ASDR_DCS_PASS == -2 && ASDR_DCS_ANY == -1 && "
            "ASDR_DCS_CLOCK == 2625 && ASDR_DCS_MAX_CODES == 128, \"table\");\n")
    r = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(ROOT, "include", "asdr_dcs.h")) as f:
        body = re.search(r"ASDR_DCS_CODES\[ASDR_DCS_COUNT\] = \{(.*?)\};", f.read(), flags=re.S).group(1)
    assert tuple(int(v, 8) for v in body.split(",")) == A.DCS_CODES == DR.CODES and len(A.DCS_CODES) == 104
    assert (A.DCS_PASS, A.DCS_ANY) == (DR.PASS, DR.ANY) == (-2, -1)
    t = squelch(A, 3)
    st = t.read_state()                                        # the library fills exactly 3 * 192 bytes
    assert st.shape == (3,) and st.nbytes == 576


def test_creation_values(A):
    t = squelch(A)
    assert t.n_channels == 6 and t._L.asdr_dcs_n_channels(t._h) == 6 and t.blocks() == 0
    ref = DR.DcsRef(6)                                          # the restatement starts from the same values
    want = (list(DR.CODES), [DR.word(c) for c in DR.CODES], 0, 2, 46, [(DR.PASS, 0)] * 6)
    assert settings(t) == want
    assert (ref.codes, ref.words, ref.max_errors, ref.confirm, ref.hold_bits) == want[:5]
    assert list(zip(ref.want.tolist(), ref.hysteresis.tolist())) == want[5]
    st = t.read_state()
    assert st.tobytes() == creation_records(6) and (st["detected"] == -1).all() and (st["cand"] == -1).all() and (st["age"] == 255).all()
    assert (t.decoded_codes() == -1).all()
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(A.AsdrError, match="n_channels"):
            A.DcsSquelch(n, device=A.NO_DEVICE)


def test_bank_wide_setters_their_ends_and_refusals(A):
    t = squelch(A)
    rec = t.read_state()
    rec["sr"] = 0x123456; rec["cand"] = 0; rec["age"] = 7; rec["run"] = 3; rec["detected"] = 0; rec["quiet"] = 9
    rec["open"] = 1; rec["bits"] = 50; rec["hits"] = 2; rec["detections"] = 1; rec["openings"] = 1; rec["open_blocks"] = 8; rec["edges"] = 40
    rec["clk"] = 77; rec["b"] = 1; rec["hist"] = 11; rec["dhist"] = -3
    t.write_state(rec)
    kept = t.read_state()                                       # what a new table leaves: open, the counters, the clock, the filters
    kept["sr"] = 0; kept["cand"] = -1; kept["age"] = 255; kept["run"] = 0; kept["detected"] = -1; kept["quiet"] = 0

    t.set_codes([0o023])                                        # a table of one ...
    assert t.get_codes()[0].tolist() == [0o023] and t.get_codes()[1].tolist() == [0x763813] and t.read_state().tobytes() == kept.tobytes()
    t.set_max_errors(3)                                         # ... allows every max_errors
    one_of_each_class = list(DR.CODES) + [c for c in range(512) if DR.find([DR.word(k) for k in DR.CODES], c) < 0][:24]
    assert len(one_of_each_class) == 128 and DR.min_distance([DR.word(c) for c in one_of_each_class]) >= 7
    t.write_state(rec)
    t.set_codes(one_of_each_class)                              # 128 words, 7 bits apart, at max_errors 3
    assert t.get_codes()[0].tolist() == one_of_each_class and t.get_codes()[1].tolist() == [DR.word(c) for c in one_of_each_class]
    assert t.read_state().tobytes() == kept.tobytes()
    for m in (0, 3): t.set_max_errors(m); assert t.get_max_errors() == m
    for k in (1, 8): t.set_confirm(k); assert t.get_confirm() == k
    for h in (23, 1023): t.set_hold_bits(h); assert t.get_hold_bits() == h
    t.set_want(127, ch=1); t.set_hysteresis(2**32 - 1, ch=2)
    before, state = settings(t), t.read_state().tobytes()

    for table, why in (([0o023, 0o023], "differ"), ([0o023, 0o025, 0o023], "differ"), ([], "n_codes"), (list(range(129)), "n_codes"),
                       ([0o1000], "0777"), ([0o023, -1], "0777"), ([1 << 20], "0777")):
        with pytest.raises(A.AsdrError, match=why):
            t.set_codes(table)
    for m in (4, -1, 1 << 20):
        with pytest.raises(A.AsdrError, match="max_errors"):
            t.set_max_errors(m)
    for k in (0, 9, -1):
        with pytest.raises(A.AsdrError, match="confirm"):
            t.set_confirm(k)
    for h in (22, 1024, 0, -1):
        with pytest.raises(A.AsdrError, match="hold_bits"):
            t.set_hold_bits(h)
    assert settings(t) == before and t.read_state().tobytes() == state          # every refusal left everything as it was
    assert before[2:5] == (3, 8, 1023)

    # The distance rule in both orders.  Every code's word is a word of the cyclic (23, 12) Golay code, so two different table words
    # differ in at least 7 bits and only a repeated code breaks the rule: it is refused at max_errors 0 as at 3, and no table that
    # went in ever stands in the way of a max_errors (the restatement's own check agrees on all 512 codes and their rotations)
    every = sorted({r for c in range(512) for r in DR.rotations(DR.word(c))})
    assert DR.min_distance(every) == 7
    t.set_max_errors(0)
    with pytest.raises(A.AsdrError, match="differ"):
        t.set_codes([0o025, 0o025])
    t.set_codes([0, 1, 0o777])                                  # no standard codes; 7 apart all the same
    t.set_max_errors(3)
    before = settings(t)
    assert before[0] == [0, 1, 0o777] and before[2] == 3
    with pytest.raises(A.AsdrError, match="want"):              # channel 1's want 127 stays, though past the table now; no new one goes in
        t.set_want(3, ch=1)
    assert t.get_want(1) == 127 and settings(t) == before
    assert t._L.asdr_dcs_set_confirm(None, 2) == -1 and t._L.asdr_dcs_blocks(None) == -1 and t._L.asdr_dcs_get_hold_bits(None) == -1
    t.reset()                                                                   # keeps the settings
    assert settings(t) == before and t.read_state().tobytes() == creation_records(6)


def test_per_channel_setters_their_ends_and_refusals(A):
    t = squelch(A)
    t.set_want(A.DCS_ANY); t.set_hysteresis(20000)                                # broadcast
    assert settings(t)[5] == [(-1, 20000)] * 6
    t.set_want(103, ch=4); t.set_hysteresis(2**32 - 1, ch=4)                      # the upper ends
    t.set_want(A.DCS_PASS, ch=0); t.set_hysteresis(0, ch=0)                       # the lower ends
    t.set_want(0, ch=2)
    want = [(-2, 0), (-1, 20000), (0, 20000), (-1, 20000), (103, 2**32 - 1), (-1, 20000)]
    assert settings(t)[5] == want
    for ch in (0, 4, A.ALL):
        for w in (104, -3, 128, 1 << 20):
            with pytest.raises(A.AsdrError, match="want"):
                t.set_want(w, ch=ch)
        for h in (-1, 2**32):
            with pytest.raises(A.AsdrError, match="hysteresis"):
                t.set_hysteresis(h, ch=ch)
    for ch in (-2, 6, 1 << 20):
        for call in (lambda: t.set_want(0, ch=ch), lambda: t.set_hysteresis(5, ch=ch), lambda: t.get_want(ch), lambda: t.get_hysteresis(ch)):
            with pytest.raises(A.AsdrError, match="bad channel"):
                call()
    with pytest.raises(A.AsdrError, match="bad channel"):
        t.get_want(A.ALL)
    assert settings(t)[5] == want


def test_write_state_checks_every_record_before_it_writes_one(A):
    t = squelch(A)
    t.set_codes([0o023, 0o025, 0o026, 0o031])
    rec = np.zeros(3, dtype=A.DCS_STATE_DTYPE)
    rec["hist"] = np.arange(144).reshape(3, 48) - 70; rec["hist"][0, :2] = (-32768, 32767)
    rec["dhist"] = np.arange(72).reshape(3, 24) * 900 - 32768; rec["dhist"][1, :2] = (-32768, 32767)
    rec["sr"] = [2**23 - 1, 0, 0x763813]
    for k, name in enumerate(DR.COUNTERS):
        rec[name] = [2**32 - 1, 0, k + 1]
    rec["detected"] = [3, -1, 0]; rec["cand"] = [-1, 3, 2]; rec["clk"] = [2624, 0, 1312]; rec["quiet"] = [65535, 0, 9]
    rec["age"] = [255, 0, 23]; rec["run"] = [255, 0, 2]; rec["b"] = [1, 0, 1]; rec["open"] = [1, 0, 1]
    t.write_state(rec, channels=[5, 0, 2])
    want = DR.DcsRef(6).records()
    for k, c in enumerate([5, 0, 2]):
        want[c] = rec[k]
    assert t.read_state().tobytes() == want.tobytes()
    assert t.decoded_codes().tolist() == [-1, -1, 0o023, -1, -1, 0o031]
    bad = rec.copy(); bad["bits"] = 77
    for field, value, why in (("open", 2, "open must be 0 or 1"), ("open", 255, "open must be 0 or 1"), ("b", 2, "b must be 0 or 1"),
                              ("clk", 2625, "clk"), ("clk", 65535, "clk"), ("sr", 2**23, "sr"), ("sr", 2**32 - 1, "sr"),
                              ("detected", 4, "detected"), ("detected", -2, "detected"), ("cand", 4, "cand"), ("cand", -32768, "cand"),
                              ("reserved", (1, 0), "reserved"), ("reserved", (0, 1 << 31), "reserved")):
        b = bad.copy(); b[field][2] = value                                     # the LAST record is the bad one
        with pytest.raises(A.AsdrError, match=why):
            t.write_state(b, channels=[1, 3, 4])
    for chans in ([1, 3, 6], [1, -1, 3], [1 << 20, 0, 1]):
        with pytest.raises(A.AsdrError, match="bad channel"):
            t.write_state(bad, channels=chans)
    with pytest.raises(A.AsdrError, match="more records"):
        t.write_state(np.zeros(7, dtype=A.DCS_STATE_DTYPE))
    with pytest.raises(A.AsdrError, match="records for"):
        t.write_state(bad, channels=[1, 2])
    assert t.read_state().tobytes() == want.tobytes()
    t.write_state(rec[:2])                                                      # channels 0, 1
    assert t.read_state()[:2].tobytes() == rec[:2].tobytes()
    before = t.read_state()
    t.clear()                                                                   # zeroes the six counters only
    st = t.read_state()
    for k in DR.STATE_NAMES:
        if k in DR.COUNTERS:
            assert not st[k].any() and before[k].any(), k
        else:
            assert np.array_equal(st[k], before[k]), k
    t.reset()
    assert t.read_state().tobytes() == creation_records(6) and t.blocks() == 0


def test_the_helpers_agree_with_the_restatement(A):
    assert A.dcs_word(0o023) == 0x763813
    for code in range(512):
        assert A.dcs_word(code) == DR.word(code), oct(code)
    for code in (0o1000, -1, 1 << 20, 2**40):
        with pytest.raises(A.AsdrError, match="0777"):
            A.dcs_word(code)
    t = squelch(A, 1)
    words = [DR.word(c) for c in DR.CODES]
    for code in range(512):
        for inverted in (False, True):
            assert t.find(code, inverted) == DR.find(words, code, inverted), (oct(code), inverted)
    assert t.find(0o023, True) == t.find(0o047) == DR.CODES.index(0o047) and t.find(0o340) == t.find(0o766) == t.find(0o023) == 0
    assert all(t.find(c) == k and t.find(c, True) >= 0 and t.find(c, True) != k for k, c in enumerate(DR.CODES))
    assert t.find(0) == -1                                                      # a code of no class of the table
    for code in (0o1000, -1):
        with pytest.raises(A.AsdrError, match="0777"):
            t.find(code)
    t.set_codes([0o047, 0o340])                                                 # find follows the table
    assert (t.find(0o023), t.find(0o023, True), t.find(0o025)) == (1, 0, -1)
    assert (DR.find([DR.word(0o047), DR.word(0o340)], 0o023), DR.find([DR.word(0o047), DR.word(0o340)], 0o023, True)) == (1, 0)
    assert t._L.asdr_dcs_find(None, 0o023, 0) == -1


def test_the_signal_path_needs_a_device(A):
    t = squelch(A)
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        t.update_device(4096, 16384, 1)
    t.synchronize()
    assert t.blocks() == 0 and t.read_state().tobytes() == creation_records(6)
