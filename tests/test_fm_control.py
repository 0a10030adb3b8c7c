"""The FM demodulator's control plane (include/asdr_fm.h) on an ASDR_NO_DEVICE handle: the creation values, broadcast and
per-channel setters and getters, that each refusal leaves everything as it was, write_state's validation, the call that needs a
device, the exported names and the record's layout."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fm_ref as FR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
MAXN = 1 << 41


def demod(A, n=6):
    return A.FmDemodulator(n, device=A.NO_DEVICE)


def settings(f):
    return [(f.get_gain(c), f.get_deemphasis(c), f.get_dc_shift(c)) + f.get_squelch(c) for c in range(f.n_channels)]


def test_every_declared_name_is_exported_and_bound(A):
    with open(os.path.join(ROOT, "include", "asdr_fm.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(asdr_fm_\w+)\s*\(", text)))
    assert len(declared) == 20 and "asdr_fm_update_device" in declared and "asdr_fm_gain_from_deviation" in declared
    L = ctypes.CDLL(A.library_path())
    for n in declared:
        assert hasattr(L, n), n
    assert sorted(A.FM_EXPORTS) == declared
    assert sorted("asdr_fm_" + k for k in A.fm._API) == declared       # every one has its types set
    others = (set(A.binding.EXPORTS) | set(A.GATE_EXPORTS) | set(A.TUNER_EXPORTS) | set(A.FRONT_EXPORTS) | set(A.RESAMPLE_EXPORTS)
              | set(A.CODEC_EXPORTS) | set(A.SPECTROGRAM_EXPORTS))
    assert not [n for n in A.FM_EXPORTS if n in others]
    for lst in (A.GATE_EXPORTS, A.RESAMPLE_EXPORTS, A.CODEC_EXPORTS, A.SPECTROGRAM_EXPORTS, A.TUNER_EXPORTS, A.FRONT_EXPORTS, A.binding.EXPORTS):
        assert not [n for n in lst if n.startswith("asdr_fm_")]


def test_the_state_record_is_48_bytes(A):
    assert A.FM_STATE_DTYPE.itemsize == 48 and A.FM_STATE_DTYPE.names == FR.STATE_NAMES
    assert tuple(A.FM_STATE_DTYPE.fields[k][1] for k in FR.STATE_NAMES) == FR.STATE_OFFSETS
    assert tuple(A.FM_STATE_DTYPE.fields[k][0].str.lstrip("<|") for k in FR.STATE_NAMES) == FR.STATE_TYPES
    src = "#include <stddef.h>\n#include \"asdr_fm.h\"\n_Static_assert(sizeof(asdr_fm_state_t) == 48, \"size\");\n"
    for name, off in zip(FR.STATE_NAMES, FR.STATE_OFFSETS):
        src += "_Static_assert(offsetof(asdr_fm_state_t, %s) == %d, \"%s\");\n" % (name, off, name)
    r = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    f = demod(A, 3)
    st = f.read_state()                                        # the library fills exactly 3 * 48 bytes
    assert st.shape == (3,) and st.nbytes == 144


def test_creation_values(A):
    f = demod(A)
    assert f.n_channels == 6 and f._L.asdr_fm_n_channels(f._h) == 6 and f.blocks() == 0
    assert settings(f) == [(144502, 32768, 0, MAXN, MAXN, 0)] * 6
    assert FR.record_tuples(f.read_state()) == [(0,) * 14] * 6
    ref = FR.FmRef(6)                                          # the restatement starts from the same values
    assert list(zip(ref.gain.tolist(), ref.deemphasis.tolist(), ref.hp_shift.tolist(), ref.open_noise.tolist(), ref.close_noise.tolist(),
                    ref.hang_blocks.tolist())) == settings(f)
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(A.AsdrError, match="n_channels"):
            A.FmDemodulator(n, device=A.NO_DEVICE)
    assert A.FmDemodulator(1 << 20, device=A.NO_DEVICE).n_channels == 1 << 20


def test_setters_getters_and_refusals(A):
    f = demod(A)
    f.set_gain(1000); f.set_deemphasis(976); f.set_dc_shift(8); f.set_squelch(10**11, 3 * 10**11, 2)     # broadcast
    assert settings(f) == [(1000, 976, 8, 10**11, 3 * 10**11, 2)] * 6
    f.set_gain(1 << 24, ch=4); f.set_deemphasis(32768, ch=4); f.set_dc_shift(15, ch=4); f.set_squelch(MAXN, MAXN, 65535, ch=4)   # the upper ends
    f.set_gain(1, ch=0); f.set_deemphasis(1, ch=0); f.set_dc_shift(0, ch=0); f.set_squelch(0, 0, 0, ch=0)                        # the lower ends
    f.set_deviation(2500.0, ch=2); f.set_deemphasis(tau_us=75.0, ch=2); f.set_squelch(7, ch=2)
    want = [(1, 1, 0, 0, 0, 0), (1000, 976, 8, 10**11, 3 * 10**11, 2), (FR.gain_from_deviation(2500.0), 8550, 8, 7, 7, 0),
            (1000, 976, 8, 10**11, 3 * 10**11, 2), (1 << 24, 32768, 15, MAXN, MAXN, 65535), (1000, 976, 8, 10**11, 3 * 10**11, 2)]
    assert settings(f) == want
    for ch in (0, 4, A.ALL):
        for g in (0, (1 << 24) + 1, 2**32 - 1):
            with pytest.raises(A.AsdrError, match="gain"):
                f.set_gain(g, ch=ch)
        for a in (0, 32769, 2**32 - 1):
            with pytest.raises(A.AsdrError, match="de-emphasis"):
                f.set_deemphasis(a, ch=ch)
        for k in (16, -1, 1 << 20):
            with pytest.raises(A.AsdrError, match="hp_shift"):
                f.set_dc_shift(k, ch=ch)
        with pytest.raises(A.AsdrError, match="open_noise"):
            f.set_squelch(11, 10, ch=ch)
        for o, c in ((5, MAXN + 1), (MAXN + 1, MAXN + 1), (0, 2**64 - 1)):
            with pytest.raises(A.AsdrError, match="2\\^41"):
                f.set_squelch(o, c, ch=ch)
        for hang in (65536, -1, 1 << 20):
            with pytest.raises(A.AsdrError, match="hang_blocks"):
                f.set_squelch(5, 10, hang_blocks=hang, ch=ch)
        with pytest.raises(A.AsdrError, match="outside"):
            f.set_deviation(10.0, ch=ch)
        with pytest.raises(A.AsdrError, match="outside"):
            f.set_deemphasis(tau_us=1e9, ch=ch)
    for ch in (-2, 6, 1 << 20):
        for call in (lambda: f.set_gain(5, ch=ch), lambda: f.set_deemphasis(5, ch=ch), lambda: f.set_dc_shift(5, ch=ch),
                     lambda: f.set_squelch(5, 10, ch=ch), lambda: f.get_gain(ch), lambda: f.get_deemphasis(ch), lambda: f.get_dc_shift(ch),
                     lambda: f.get_squelch(ch)):
            with pytest.raises(A.AsdrError, match="bad channel"):
                call()
    with pytest.raises(A.AsdrError, match="bad channel"):
        f.get_gain(A.ALL)
    with pytest.raises(A.AsdrError, match="give a or tau_us"):
        f.set_deemphasis()
    assert settings(f) == want                                                # every refusal left everything as it was
    assert f._L.asdr_fm_set_gain(None, 0, 1) == -1 and f._L.asdr_fm_blocks(None) == -1
    f.reset()                                                                 # keeps the settings
    assert settings(f) == want


def test_state_calls_work_on_the_host_copy_and_write_state_is_all_or_nothing(A):
    f = demod(A)
    rec = np.zeros(3, dtype=A.FM_STATE_DTYPE)
    rec["prev_i"] = [-32768, 1, 2]; rec["prev_q"] = [32767, -1, 3]; rec["v1"] = [-32768, 7, 0]; rec["v2"] = [32767, -7, 1]
    rec["s"] = [-2**31, 5, 2**31 - 1]; rec["m"] = [2**31 - 1, -5, -2**31]; rec["last_noise"] = [MAXN, 0, 9]; rec["last_power"] = [2**38, 1, 2]
    rec["openings"] = [2**32 - 1, 0, 1]; rec["open_blocks"] = [5, 0, 1]; rec["hang_left"] = [65535, 0, 9]; rec["open"] = [1, 0, 1]
    f.write_state(rec, channels=[5, 0, 2])
    want = [(0,) * 14] * 6
    for k, c in enumerate([5, 0, 2]):
        want[c] = FR.record_tuples(rec)[k]
    assert FR.record_tuples(f.read_state()) == want                           # hang_left above hang_blocks (0) is allowed
    bad = rec.copy(); bad["s"] = 77
    for field, value, why in (("open", 2, "open must be 0 or 1"), ("open", 255, "open must be 0 or 1"), ("reserved", 1, "reserved"),
                              ("reserved2", 1 << 31, "reserved")):
        b = bad.copy(); b[field][2] = value                                   # the LAST record is the bad one
        with pytest.raises(A.AsdrError, match=why):
            f.write_state(b, channels=[1, 3, 4])
    for chans in ([1, 3, 6], [1, -1, 3], [1 << 20, 0, 1]):
        with pytest.raises(A.AsdrError, match="bad channel"):
            f.write_state(bad, channels=chans)
    with pytest.raises(A.AsdrError, match="more records"):
        f.write_state(np.zeros(7, dtype=A.FM_STATE_DTYPE))
    with pytest.raises(A.AsdrError, match="records for"):
        f.write_state(bad, channels=[1, 2])
    assert FR.record_tuples(f.read_state()) == want
    f.write_state(rec[:2])                                                    # channels 0, 1
    assert FR.record_tuples(f.read_state())[:2] == FR.record_tuples(rec[:2])
    m = f.read_state()["m"].astype(np.float64)
    assert np.array_equal(f.offset_hz(5000.0), m / 32768.0 / 32767.0 * 5000.0) and f.offset_hz(5000.0)[0] > 4999.0
    before = f.read_state()
    f.clear()                                                                 # zeroes openings and open_blocks only
    st = f.read_state()
    assert not st["openings"].any() and not st["open_blocks"].any() and before["openings"].any()
    for k in FR.STATE_NAMES:
        if k not in ("openings", "open_blocks"):
            assert np.array_equal(st[k], before[k]), k
    f.reset()
    assert FR.record_tuples(f.read_state()) == [(0,) * 14] * 6 and f.blocks() == 0


def test_the_signal_path_needs_a_device(A):
    f = demod(A)
    with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
        f.update_device(4096, 8192, 16384, 1)
    f.synchronize()
    assert f.blocks() == 0 and FR.record_tuples(f.read_state()) == [(0,) * 14] * 6
