"""The digital tuner bank's control plane on an ASDR_NO_DEVICE bank (include/asdr_tuner.h): argument checks, the frequency-word
rounding, the filter rules, the default filter's response, read_state after every setter, and the header as C99."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tuner_ref as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

# Stop-band rejection the default filter reaches after Q15 rounding: the Kaiser design itself clears 80 dB, the
# rounding of 12 D + 1 taps to 1/32768 leaves an error floor that rises with the tap count.
STOPBAND_DB = {2: 78.0, 8: 71.0, 48: 62.0, 64: 62.0}


@pytest.fixture
def T(A):
    return lambda n=4, s=2, D=8: A.TunerBank(n, s, D, device=A.NO_DEVICE)


def test_exports_every_declared_symbol(A):
    import ctypes
    import re
    with open(os.path.join(ROOT, "include", "asdr_tuner.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(asdr_tuner_\w+)\s*\(", text)))
    L = ctypes.CDLL(A.library_path())
    assert [n for n in names if not hasattr(L, n)] == []
    assert set(A.TUNER_EXPORTS) == set(names)


def test_creation_state_and_ranges(A, T):
    t = T(5, 3, 7)
    st = t.read_state()
    assert t.position() == 0 and not st["src"].any() and not st["fw"].any() and not st["pos_a"].any() and not st["ph_a"].any()
    for args in ((0, 1, 1), (4, 0, 1), (4, 1, 0), (4, 1, 65)):
        with pytest.raises(A.AsdrError):
            A.TunerBank(*args, device=A.NO_DEVICE)
    with pytest.raises(A.AsdrError, match="source"):
        t.set_source(3, ch=0)
    with pytest.raises(A.AsdrError, match="source"):
        t.set_source(-1)
    with pytest.raises(A.AsdrError, match="channel"):
        t.set_frequency_word(1, ch=5)
    with pytest.raises(A.AsdrError, match="HIP device"):
        t.update(np.zeros((3, 128 * 7, 2), dtype=np.int16))


def test_frequency_word_rounding_and_range(A, T):
    for D in (1, 2, 48, 64):
        t = T(2, 1, D)
        fs = 44100.0 * D
        for hz in (0.0, 1.0, -1.0, 1234.5678, -fs / 2, fs / 2, fs / 3, -fs / 7, fs / 2 ** 33, 0.5 * fs / 2 ** 32 * 3):
            t.set_frequency(hz, ch=1)
            assert int(t.read_state()["fw"][1]) == R.fw_from_hz(hz, D), (D, hz)
        for bad in (fs / 2 * (1 + 1e-12), -fs / 2 - 1.0, float("nan"), float("inf")):
            with pytest.raises(A.AsdrError, match="frequency"):
                t.set_frequency(bad, ch=0)
        assert int(t.read_state()["fw"][0]) == 0


def test_filter_rules(A, T):
    t = T(1, 1, 4)
    h0, g0 = t.get_filter()
    for h, g, what in (([1] * 1025, 0, "length"), ([], 0, "length"), ([1, 2], 16, "gain"), ([1, 2], -1, "gain"),
                       ([32767, 32767, 2], 0, "65535"), ([-32768, -32768], 3, "65535")):
        with pytest.raises(A.AsdrError, match=what):
            t.set_filter(np.array(h, dtype=np.int16), g)
        h1, g1 = t.get_filter()
        assert np.array_equal(h1, h0) and g1 == g0                      # the old filter is kept
    t.set_filter([32767, 32767, 1], 15)                                 # sum |h| = 65535 exactly: accepted
    h1, g1 = t.get_filter()
    assert list(h1) == [32767, 32767, 1] and g1 == 15
    t.set_filter(np.arange(-512, 512, dtype=np.int16) // 16, 5)
    assert t.get_filter()[0].size == 1024


def test_default_filter_d1_is_a_pass_through(T):
    h, g = T(1, 1, 1).get_filter()
    assert list(h) == [16384] and g == 1
    z = np.arange(-32768, 32768, 7, dtype=np.int64)
    assert np.array_equal(R.fir_decimate(z, h, 1, g, z.size), z)


@pytest.mark.parametrize("D", sorted(STOPBAND_DB))
def test_default_filter_response(T, D):
    h, g = T(1, 1, D).get_filter()
    L = h.size
    assert L % 2 == 1 and L <= 12 * D + 1 and g == 0 and np.abs(h.astype(int)).sum() <= 65535
    assert np.array_equal(h, h[::-1])                                   # linear phase
    pb, sb, fs = R.default_filter_spec(D)
    n = 1 << 18
    H = np.abs(np.fft.rfft(h.astype(np.float64) / 32768.0, n))
    f = np.arange(H.size) * fs / n
    passband = 20 * np.log10(H[f <= pb])
    assert passband.max() - passband.min() <= 0.1, passband.max() - passband.min()
    assert abs(passband.mean()) < 0.05                                 # unit gain
    rejection = -20 * np.log10(H[f >= sb].max())
    assert rejection >= STOPBAND_DB[D], rejection


def test_read_state_after_every_setter(A, T):
    t = T(4, 3, 2)
    ref = R.TunerRef(4, 3, 2)

    def same():
        st = t.read_state()
        for k, v in (("src", ref.src), ("fw", ref.fw), ("pos_a", ref.pos_a), ("ph_a", ref.ph_a)):
            assert [int(x) for x in st[k]] == [int(x) for x in v], k

    for step in (lambda o: o.set_source(2, ch=1), lambda o: o.set_frequency_word(0x9000_0001, ch=1),
                 lambda o: o.set_frequency(-12_000.0, ch=3), lambda o: o.set_phase(0xABCD_0000, ch=0),
                 lambda o: o.set_frequency_word(0x10), lambda o: o.set_source(1), lambda o: o.set_phase(5, ch=2)):
        step(t); step(ref)
        same()
    t.reset()
    assert t.position() == 0 and not t.read_state()["fw"].any()


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "asdr_tuner.h"\nint main(void) { asdr_tuner_state_t s; (void)s; return (int)sizeof(asdr_tuner_state_t) - 24; }\n')
    out = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                          str(src), "-o", str(tmp_path / "t")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0
