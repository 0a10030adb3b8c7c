"""The control plane of the filter palette and the gains (include/asdr_tuner.h, "Filter palette and gain") on ASDR_NO_DEVICE
banks: the creation state, the getters, every rejected call with the old state kept, palette_clear refused while a channel is on
the slot, reset, direct-form and rate banks and a NULL bank failing, and the exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

NEW = ["asdr_tuner_palette_set", "asdr_tuner_palette_get", "asdr_tuner_palette_clear", "asdr_tuner_set_channel_slot",
       "asdr_tuner_read_slots", "asdr_tuner_set_channel_gain", "asdr_tuner_read_gains"]
CX = (np.arange(1, 8) * (0.5 - 0.25j)).astype(np.complex64)
RE = np.array([0.5, -0.25, 0.125], dtype=np.float32)


@pytest.fixture
def T(A):
    return lambda fs=2400000, R=16, n=4, s=2: A.TunerBank.fastconv(n, s, fs, R, device=A.NO_DEVICE)


def state(t):
    return ([None if g is None else (g.dtype, g.tobytes()) for g in map(t.get_palette_filter, range(64))], list(t.slots()), list(t.gains()))


def test_the_new_functions_are_declared_and_exported(A):
    with open(os.path.join(ROOT, "include", "asdr_tuner.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = C.CDLL(A.library_path())
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, text) and hasattr(L, n) and n in A.TUNER_EXPORTS, n
    assert re.search(r"#define ASDR_TUNER_FC_MAX_FILTERS 64\b", text)
    assert A.design_channel_filter is A.tuner.design_channel_filter and A.tuner.MAX_FILTERS == 64


def test_creation_state_and_getters(A, T):
    t = T()
    assert t.slots().dtype == np.int32 and list(t.slots()) == [0] * 4
    assert t.gains().dtype == np.float32 and list(t.gains()) == [1.0] * 4
    assert all(t.get_palette_filter(s) is None for s in range(1, 64))
    g0 = t.get_palette_filter(0)
    assert g0.dtype == np.float32 and g0.tobytes() == t.get_channel_filter().tobytes()
    t.set_palette_filter(1, CX); t.set_palette_filter(63, RE); t.set_palette_filter(2, [1, 2, 3])
    assert t.get_palette_filter(1).dtype == np.complex64 and t.get_palette_filter(1).tobytes() == CX.tobytes()
    assert t.get_palette_filter(63).dtype == np.float32 and t.get_palette_filter(63).tobytes() == RE.tobytes()
    assert list(t.get_palette_filter(2)) == [1.0, 2.0, 3.0]
    t.set_palette_filter(1, RE)                                 # redefined: real now
    assert t.get_palette_filter(1).dtype == np.float32
    t.set_channel_slot(63); t.set_channel_slot(1, ch=2); t.set_gain(-0.5); t.set_gain(32768.0, ch=0); t.set_gain(0.0, ch=3)
    assert list(t.slots()) == [63, 63, 1, 63] and list(t.gains()) == [32768.0, -0.5, -0.5, 0.0]
    t.set_channel_filter(RE)                                    # slot 0 follows the channel filter
    assert t.get_palette_filter(0).tobytes() == RE.tobytes()
    buf, cx = (C.c_float * 4)(9, 9, 9, 9), C.c_int(7)           # cap counts taps: one complex tap is two floats
    t.set_palette_filter(5, CX)
    assert t._L.asdr_tuner_palette_get(t._h, 5, buf, 1, C.byref(cx)) == CX.size and cx.value == 1
    assert list(buf) == [CX[0].real, CX[0].imag, 9.0, 9.0]
    st = t.read_state()                                         # the channel state is as it was
    assert st.dtype.itemsize == 24 and not st["fw"].any()


def test_rejected_calls_keep_the_old_state(A, T):
    t = T()
    t.set_palette_filter(3, CX); t.set_channel_slot(3, ch=1); t.set_gain(2.0, ch=2)
    before = state(t)
    for slot, match in ((0, "slot 0"), (-1, "1..63"), (64, "1..63"), (1000, "1..63")):
        with pytest.raises(A.AsdrError, match=match):
            t.set_palette_filter(slot, RE)
        with pytest.raises(A.AsdrError, match=match):
            t.clear_palette_filter(slot)
        assert state(t) == before
    for taps in (np.zeros(0, np.float32), np.zeros(130, np.float32), np.zeros(130, np.complex64)):
        with pytest.raises(A.AsdrError, match="1..129"):
            t.set_palette_filter(3, taps)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(A.AsdrError, match="finite"):
            t.set_palette_filter(3, np.array([1.0, bad], np.float32))
        with pytest.raises(A.AsdrError, match="finite"):
            t.set_palette_filter(3, np.array([1.0, 1j * bad], np.complex64))
        with pytest.raises(A.AsdrError, match="gain"):
            t.set_gain(bad)
    assert t._L.asdr_tuner_palette_set(t._h, 3, None, 3, 0) == -1
    assert state(t) == before
    t.set_palette_filter(4, np.zeros(129, np.complex64))        # the longest
    before = state(t)
    for slot in (5, 62, -1, 64):                                # undefined, or out of range
        with pytest.raises(A.AsdrError, match="undefined|0..63"):
            t.set_channel_slot(slot)
        with pytest.raises(A.AsdrError, match="undefined|0..63"):
            t.set_channel_slot(slot, ch=0)
    for gain in (32768.5, -40000.0, 1e30):
        with pytest.raises(A.AsdrError, match="32768"):
            t.set_gain(gain, ch=1)
    for ch in (4, -2):
        with pytest.raises(A.AsdrError, match="channel"):
            t.set_channel_slot(3, ch=ch)
        with pytest.raises(A.AsdrError, match="channel"):
            t.set_gain(2.0, ch=ch)
    with pytest.raises(A.AsdrError, match="0..63"):
        t.get_palette_filter(64)
    assert state(t) == before
    t.set_gain(-32768.0, ch=0)
    assert t.gains()[0] == -32768.0


def test_clear_is_refused_while_a_channel_is_on_the_slot(A, T):
    t = T()
    t.set_palette_filter(9, RE); t.set_channel_slot(9, ch=3)
    with pytest.raises(A.AsdrError, match="in use by channel 3"):
        t.clear_palette_filter(9)
    assert t.get_palette_filter(9).tobytes() == RE.tobytes() and list(t.slots()) == [0, 0, 0, 9]
    t.set_channel_slot(0, ch=3)
    t.clear_palette_filter(9)
    assert t.get_palette_filter(9) is None
    t.clear_palette_filter(9)                                   # clearing an undefined slot is no error
    with pytest.raises(A.AsdrError, match="undefined"):
        t.set_channel_slot(9)


def test_reset_puts_channels_back_and_keeps_the_palette(A, T):
    t = T()
    t.set_palette_filter(1, CX); t.set_channel_slot(1); t.set_gain(3.0); t.set_frequency(1000.0)
    t.reset()
    assert list(t.slots()) == [0] * 4 and list(t.gains()) == [1.0] * 4 and not t.read_state()["fw"].any()
    assert t.get_palette_filter(1).tobytes() == CX.tobytes()
    t.set_channel_slot(1, ch=0)                                 # still defined
    t.set_frequency(5.0); t.set_source(1); t.set_input_format("cu8"); t.enable_levels()      # none of these touches them
    assert list(t.slots()) == [1, 0, 0, 0] and list(t.gains()) == [1.0] * 4


def test_direct_form_and_rate_banks_refuse_with_a_message(A):
    for d in (A.TunerBank(2, 1, 4, device=A.NO_DEVICE), A.TunerBank(2, 1, 50, fs_in=2400000, device=A.NO_DEVICE)):
        for call in (lambda: d.set_palette_filter(1, RE), lambda: d.get_palette_filter(1), lambda: d.get_palette_filter(0),
                     lambda: d.clear_palette_filter(1), lambda: d.set_channel_slot(0), d.slots, lambda: d.set_gain(1.0), d.gains):
            with pytest.raises(A.AsdrError, match="fast-convolution"):
                call()


def test_a_null_bank_fails(A, T):
    L = T()._L
    f, i32 = (C.c_float * 2)(1, 2), (C.c_int32 * 2)()
    for rc in (L.asdr_tuner_palette_set(None, 1, f, 2, 0), L.asdr_tuner_palette_get(None, 1, f, 2, None), L.asdr_tuner_palette_clear(None, 1),
               L.asdr_tuner_set_channel_slot(None, 0, 0), L.asdr_tuner_read_slots(None, i32), L.asdr_tuner_set_channel_gain(None, 0, 1.0),
               L.asdr_tuner_read_gains(None, f)):
        assert rc == -1 and b"null tuner bank" in L.asdr_last_error()
    t = T()
    assert L.asdr_tuner_read_slots(t._h, None) == -1 and L.asdr_tuner_read_gains(t._h, None) == -1
