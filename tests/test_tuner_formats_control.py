"""Input formats of the digital tuner (include/asdr_tuner.h, "Input formats") on ASDR_NO_DEVICE banks of all three kinds: the
default, the set / get round trip, unknown values, reset, the errors of the int16 and the new update entry points (wrong format,
misaligned rows, no device) with position() unchanged, the Python checks of dtype and shape, and the restatement
tests/tuner_formats_ref.py against known answers."""
import ctypes as C

import numpy as np
import pytest

import tuner_formats_ref as FM

NAMES = ["cs16", "cu8", "cs8", "cf32", "rs16"]


def banks(A):
    return [("plain", A.TunerBank(3, 2, 4, device=A.NO_DEVICE)),
            ("rate", A.TunerBank(3, 2, 50, fs_in=2400000, device=A.NO_DEVICE)),
            ("fastconv", A.TunerBank.fastconv(3, 2, 2400000, 16, device=A.NO_DEVICE))]


def test_default_round_trip_unknown_values_and_reset(A):
    for kind, t in banks(A):
        assert t.input_format() == "cs16" and t._L.asdr_tuner_input_format(t._h) == 0, kind
        for v, name in enumerate(NAMES):
            t.set_input_format(name)
            assert t.input_format() == name and t._L.asdr_tuner_input_format(t._h) == v
            t.set_input_format(v)
            assert t.input_format() == name
            for bad in (-1, 5, 255, 1 << 20):
                with pytest.raises(A.AsdrError, match="unknown input format"):
                    t.set_input_format(bad)
                assert t.input_format() == name, (kind, bad)
            with pytest.raises(A.AsdrError, match="unknown input format"):
                t.set_input_format("cs12")
            t.reset()
            assert t.input_format() == name and t.position() == 0, kind
        t.set_input_format("CU8")                              # names in either case
        assert t.input_format() == "cu8"
    assert A.TunerBank(1, 1, 1, device=A.NO_DEVICE)._L.asdr_tuner_input_format(None) == -1
    assert A.TunerBank(1, 1, 1, device=A.NO_DEVICE)._L.asdr_tuner_set_input_format(None, 0) == -1


def test_int16_entry_points_refuse_other_formats_and_name_them(A):
    for kind, t in banks(A):
        per = 128 * t.decimation
        iq = np.zeros((2, per, 2), np.int16)
        for name in NAMES[1:]:
            t.set_input_format(name)
            for call in (lambda: t.update(iq), lambda: t.update_rate(iq),
                         lambda: t.update_device(4096, 8192, 12288, 1), lambda: t.update_rate_device(4096, 8192, 12288, 1, 2)):
                with pytest.raises(A.AsdrError, match=r"input format is %s.*update_samples" % name.upper()):
                    call()
                assert t.position() == 0 and t.output_position() == 0, (kind, name)
        t.set_input_format("cs16")                             # back to CS16: the old errors
        with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
            t.update_rate(iq)
        if kind == "plain":
            with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
                t.update(iq)
        assert t.position() == 0


def test_update_samples_reports_no_device_and_misaligned_rows(A):
    for kind, t in banks(A):
        per = 128 * t.decimation
        for name in NAMES:
            t.set_input_format(name)
            dtype, parts = FM.FORMATS[name]
            x = np.zeros((2, per) + ((2,) if parts == 2 else ()), dtype)
            with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
                t.update_samples(x)
            with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
                t.update_samples_device(4096, 1 << 20, 1 << 21, 1, 2)
            unit = 16 // FM.BYTES[name]                       # samples per 16 bytes
            with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
                t.update_samples_device(4096, 1 << 20, 1 << 21, 1, 2, in_stride_samples=per + unit)
            for stride in (per + 1, per + unit // 2, per + unit + 1):
                if (stride * FM.BYTES[name]) % 16:
                    with pytest.raises(A.AsdrError, match="16-byte aligned.*%s" % name.upper()):
                        t.update_samples_device(4096, 1 << 20, 1 << 21, 1, 2, in_stride_samples=stride)
            for ptr in (4096 + 8, 4096 + 2, 4097):
                with pytest.raises(A.AsdrError, match="16-byte aligned"):
                    t.update_samples_device(ptr, 1 << 20, 1 << 21, 1, 2)
            assert t.position() == 0 and t.output_position() == 0, (kind, name)


def test_update_samples_checks_dtype_and_shape_and_converts_nothing(A):
    t = A.TunerBank(3, 2, 4, device=A.NO_DEVICE)
    per = 512
    for name in NAMES:
        t.set_input_format(name)
        dtype, parts = FM.FORMATS[name]
        good = (2, per, 2) if parts == 2 else (2, per)
        for other in (np.int16, np.uint8, np.int8, np.float32, np.float64, np.int32):
            if np.dtype(other) != np.dtype(dtype):
                with pytest.raises(A.AsdrError, match="dtype"):
                    t.update_samples(np.zeros(good, other))
        with pytest.raises(A.AsdrError, match="dtype"):
            t.update_samples([[0] * per] * 2)
        for shape in ((2, per, 2) if parts == 1 else (2, per), (3,) + good[1:], (2, per + 1) + good[2:], (2, per, 3), (2 * per,)):
            with pytest.raises(A.AsdrError, match="shape"):
                t.update_samples(np.zeros(shape, dtype))
    assert t.position() == 0


def test_exports_and_the_c_entry_points_by_hand(A):
    """The new entry points straight through ctypes: NULL banks, and a CU8 bank refusing an int16 call."""
    L = C.CDLL(A.library_path())
    for n in ("asdr_tuner_set_input_format", "asdr_tuner_input_format", "asdr_tuner_update_samples_device", "asdr_tuner_update_samples"):
        assert hasattr(L, n) and n in A.TUNER_EXPORTS
    t = A.TunerBank(1, 1, 1, device=A.NO_DEVICE)
    assert t._L.asdr_tuner_update_samples(None, None, 1, None, None, 1) == -1
    assert t._L.asdr_tuner_update_samples_device(None, None, 128, 1, None, None, 1, 1, None) == -1
    assert b"null tuner bank" in t._L.asdr_last_error()


def test_to_cs16_known_answers():
    assert FM.to_cs16(np.array([[0, 255], [127, 128]], np.uint8), "cu8").tolist() == [[-32640, 32640], [-128, 128]]
    assert FM.to_cs16(np.array([[-128, 127], [0, -1]], np.int8), "cs8").tolist() == [[-32768, 32512], [0, -256]]
    assert FM.to_cs16(np.array([5, -7], np.int16), "rs16").tolist() == [[5, 0], [-7, 0]]
    f = np.array([[np.nan, np.inf], [-np.inf, 1.0], [-1.0, 0.5 / 32768], [1.5 / 32768, 2.5 / 32768], [-0.5 / 32768, -1.5 / 32768],
                  [32767.5 / 32768, -32768.5 / 32768], [3e38, -3e38], [0.25, 1e-45]], np.float32)
    assert FM.to_cs16(f, "cf32").tolist() == [[0, 32767], [-32768, 32767], [-32768, 0], [2, 2], [0, -2], [32767, -32768],
                                               [32767, -32768], [8192, 0]]
    iq = np.array([[-32768, 32767], [123, -456]], np.int16)
    assert np.array_equal(FM.to_cs16(iq, "cs16"), iq)
    assert np.array_equal(FM.to_cs16(FM.from_cs16(iq, "cf32"), "cf32"), iq)


def test_generators_reach_the_ends_of_every_format():
    rng = np.random.default_rng(5)
    for name in NAMES[1:]:
        raw = FM.raw_noise(rng, name, 2, 1024)
        dtype, parts = FM.FORMATS[name]
        assert raw.dtype == np.dtype(dtype) and raw.shape == ((2, 1024, 2) if parts == 2 else (2, 1024))
        x = FM.to_cs16(raw, name)
        lo, hi = {"cu8": (-32640, 32640), "cs8": (-32768, 32512), "cf32": (-32768, 32767), "rs16": (-32768, 32767)}[name]
        assert x[..., 0].min() == lo and x[..., 0].max() == hi and x.dtype == np.int16
        if parts == 2:
            assert x[..., 1].min() == lo and x[..., 1].max() == hi
        else:
            assert not x[..., 1].any()
    raw = FM.raw_noise(rng, "cf32", 1, 4096)
    v = 32768.0 * raw.astype(np.float64)
    assert np.isnan(v).any() and np.isinf(v).any() and (np.abs(v[np.isfinite(v)]) > 40000).any()
    fin = np.where(np.isfinite(v), v, 0.25)
    ties = fin - np.floor(fin) == 0.5
    assert ties.mean() > 0.2                                   # exact half-integers x 2^-15


def test_half_size_model_is_the_dft_of_the_real_window():
    rng = np.random.default_rng(6)
    for N in (512, 1024, 4096):
        w = rng.integers(-32768, 32767, size=(2, N)).astype(np.float64)
        X = FM.HalfSizeFFT.fft(w.astype(np.complex64))
        want = np.fft.fft(w, axis=1)
        assert X.dtype == np.complex64 and X.shape == want.shape
        assert np.abs(X - want).max() <= 2e-6 * np.abs(want).max()
