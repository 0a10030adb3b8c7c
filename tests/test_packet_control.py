"""The packet decoder's control plane (include/asdr_packet.h) on an ASDR_NO_DEVICE handle: the creation values, the setter and getter
with their ends, that each refusal leaves everything as it was, write_state's validation, clear and reset, the helpers against the
restatement, the calls that need a device, the exported names and the layouts of the record and the slot."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import packet_ref as PR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def decoder(A, n=6, ring=4):
    return A.PacketDecoder(n, ring=ring, device=A.NO_DEVICE)


def settings(t):
    return [t.get_space_boost(c) for c in range(t.n_channels)]


def creation_records(n):
    return PR.PacketRef(n).records().tobytes()


def test_every_declared_name_is_exported_and_bound(A):
    with open(os.path.join(ROOT, "include", "asdr_packet.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(asdr_packet_\w+)\s*\(", text)))
    assert len(declared) == 17 and "asdr_packet_update_device" in declared and "asdr_packet_collect_device" in declared
    L = ctypes.CDLL(A.library_path())
    for n in declared:
        assert hasattr(L, n), n
    assert sorted(A.PACKET_EXPORTS) == declared
    assert sorted("asdr_packet_" + k for k in A.packet._API) == declared       # every one has its types set
    other_lists = (A.binding.EXPORTS, A.GATE_EXPORTS, A.TUNER_EXPORTS, A.FRONT_EXPORTS, A.RESAMPLE_EXPORTS, A.CODEC_EXPORTS,
                   A.SPECTROGRAM_EXPORTS, A.FM_EXPORTS, A.TONE_EXPORTS, A.DCS_EXPORTS)
    others = set().union(*other_lists)
    assert not [n for n in A.PACKET_EXPORTS if n in others]
    for lst in other_lists:
        assert not [n for n in lst if n.startswith("asdr_packet_")]
    for name in ("PacketDecoder", "PACKET_EXPORTS", "PACKET_STATE_DTYPE", "PACKET_FRAME_DTYPE", "PACKET_ROWS", "PACKET_NARROW_ROWS",
                 "PACKET_WIDE_CHANNELS", "PACKET_MAX_RING", "packet_fcs", "packet_format_address"):
        assert hasattr(A, name), name
    for method in ("set_space_boost", "get_space_boost", "update_device", "collect_device", "deliver", "ring_state", "read_state",
                   "write_state", "clear", "reset", "blocks", "synchronize", "close"):
        assert callable(getattr(A.PacketDecoder, method)), method


def test_the_record_is_448_bytes_and_the_slot_352(A):
    assert A.PACKET_STATE_DTYPE.itemsize == 448 and A.PACKET_STATE_DTYPE.names == PR.STATE_NAMES
    assert tuple(A.PACKET_STATE_DTYPE.fields[k][1] for k in PR.STATE_NAMES) == PR.STATE_OFFSETS
    assert all(A.PACKET_STATE_DTYPE.fields[k][0] == PR.STATE_DTYPE.fields[k][0] for k in PR.STATE_NAMES)
    assert A.PACKET_FRAME_DTYPE.itemsize == 352 and A.PACKET_FRAME_DTYPE.names == PR.FRAME_DTYPE.names
    assert all(A.PACKET_FRAME_DTYPE.fields[k] == PR.FRAME_DTYPE.fields[k] for k in PR.FRAME_DTYPE.names)
    src = ("#include <stddef.h>\n#include \"asdr_packet.h\"\n"
           "_Static_assert(sizeof(asdr_packet_state_t) == 448 && sizeof(asdr_packet_state_t) % 16 == 0, \"size\");\n"
           "_Static_assert(sizeof(asdr_packet_frame_t) == 352 && sizeof(asdr_packet_frame_t) % 16 == 0, \"slot\");\n")
    for name, off in zip(PR.STATE_NAMES, PR.STATE_OFFSETS):
        src += "_Static_assert(offsetof(asdr_packet_state_t, %s) == %d, \"%s\");\n" % (name, off, name)
    for name in PR.FRAME_DTYPE.names:
        src += "_Static_assert(offsetof(asdr_packet_frame_t, %s) == %d, \"%s\");\n" % (name, PR.FRAME_DTYPE.fields[name][1], name)
    src += ("_Static_assert(ASDR_PACKET_CLOCK == 147 && ASDR_PACKET_MAX_LEN == 332 && ASDR_PACKET_MIN_LEN == 17 && ASDR_PACKET_MAX_RING == 16 && "
            "ASDR_PACKET_MIN_BOOST == 64 && ASDR_PACKET_MAX_BOOST == 4096 && sizeof(ASDR_PACKET_C1200) == 18, \"constants\");\n")
    r = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (PR.PERIOD, PR.MAX_LEN, PR.MIN_LEN, PR.MAX_RING, PR.MIN_BOOST, PR.MAX_BOOST) == (147, 332, 17, 16, 64, 4096)
    t = decoder(A, 3)
    st = t.read_state()                                        # the library fills exactly 3 * 448 bytes
    assert st.shape == (3,) and st.nbytes == 1344


def test_creation_values(A):
    t = decoder(A)
    assert t.n_channels == 6 and t._L.asdr_packet_n_channels(t._h) == 6 and t.blocks() == 0
    assert settings(t) == [256] * 6 == PR.PacketRef(6).space_boost.tolist()
    st = t.read_state()
    assert st.tobytes() == creation_records(6) and (st["crc"] == 0xFFFF).all() and st.tobytes() != bytes(6 * 448)
    pending, lost = t.ring_state()
    assert pending.tolist() == [0] * 6 and lost.tolist() == [0] * 6
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(A.AsdrError, match="n_channels"):
            A.PacketDecoder(n, device=A.NO_DEVICE)
    for ring in (0, 17, -1, 1 << 20):
        with pytest.raises(A.AsdrError, match="ring"):
            A.PacketDecoder(4, ring=ring, device=A.NO_DEVICE)
    for ring in (1, 16):
        A.PacketDecoder(4, ring=ring, device=A.NO_DEVICE).close()


def test_the_setter_its_ends_and_refusals(A):
    t = decoder(A)
    t.set_space_boost(700)                                      # broadcast
    assert settings(t) == [700] * 6
    t.set_space_boost(64, ch=0); t.set_space_boost(4096, ch=5); t.set_space_boost(256, ch=2)
    want = [64, 700, 256, 700, 700, 4096]
    assert settings(t) == want
    state = t.read_state().tobytes()
    for ch in (0, 5, A.ALL):
        for b in (63, 4097, 0, -1, 2**32 - 1, 2**32):
            with pytest.raises(A.AsdrError, match="space_boost"):
                t.set_space_boost(b, ch=ch)
    for ch in (-2, 6, 1 << 20):
        for call in (lambda: t.set_space_boost(256, ch=ch), lambda: t.get_space_boost(ch)):
            with pytest.raises(A.AsdrError, match="bad channel"):
                call()
    with pytest.raises(A.AsdrError, match="bad channel"):
        t.get_space_boost(A.ALL)
    assert settings(t) == want and t.read_state().tobytes() == state
    assert t._L.asdr_packet_set_space_boost(None, 0, 256) == -1 and t._L.asdr_packet_blocks(None) == -1
    assert t._L.asdr_packet_n_channels(None) == -1 and t._L.asdr_packet_ring_state(None, None, None) == -1
    assert t._L.asdr_packet_ring_state(t._h, None, None) == 0   # either array may be NULL
    t.reset()                                                   # keeps the setting
    assert settings(t) == want and t.read_state().tobytes() == creation_records(6)


def filled_records(A):
    rec = np.zeros(3, dtype=A.PACKET_STATE_DTYPE)
    rec["hist"] = np.arange(24).reshape(3, 8) * 2000 - 20000; rec["hist"][0, :2] = (-32768, 32767)
    rec["dhist"] = np.arange(24).reshape(3, 8) * 2500 - 32768; rec["dhist"][1, 6:] = (-32768, 32767)
    for k, name in enumerate(("bits", "edges", "flags", "frames", "crc_errors", "aborts")):
        rec[name] = [2**32 - 1, 0, k + 1]
    rec["clk"] = [146, 0, 74]; rec["len"] = [332, 0, 17]; rec["crc"] = [0xFFFF, 0, 0xF0B8]
    rec["b"] = [1, 0, 1]; rec["prev"] = [1, 0, 0]; rec["sr"] = [255, 0, 0x7E]; rec["cur"] = [255, 0, 0x40]; rec["nb"] = [7, 0, 3]
    rec["in_frame"] = [1, 0, 1]
    rec["buf"] = (np.arange(3 * 336).reshape(3, 336) * 7) & 0xFF
    return rec


def test_write_state_checks_every_record_before_it_writes_one(A):
    t = decoder(A)
    rec = filled_records(A)
    t.write_state(rec, channels=[5, 0, 2])
    want = PR.PacketRef(6).records()
    for k, c in enumerate([5, 0, 2]):
        want[c] = rec[k]
    assert t.read_state().tobytes() == want.tobytes()
    bad = rec.copy(); bad["bits"] = 77
    reserved_low, reserved_high = [0] * 11, [0] * 11
    reserved_low[0], reserved_high[10] = 1, 1 << 31
    for field, value, why in (("clk", 147, "clk"), ("clk", 65535, "clk"), ("len", 333, "len"), ("len", 65535, "len"), ("nb", 8, "nb"),
                              ("nb", 255, "nb"), ("b", 2, "b must be 0 or 1"), ("prev", 2, "prev must be 0 or 1"),
                              ("in_frame", 2, "in_frame must be 0 or 1"), ("in_frame", 255, "in_frame"),
                              ("reserved", reserved_low, "reserved"), ("reserved", reserved_high, "reserved")):
        b = bad.copy(); b[field][2] = value                                     # the LAST record is the bad one
        with pytest.raises(A.AsdrError, match=why):
            t.write_state(b, channels=[1, 3, 4])
    for chans in ([1, 3, 6], [1, -1, 3], [1 << 20, 0, 1]):
        with pytest.raises(A.AsdrError, match="bad channel"):
            t.write_state(bad, channels=chans)
    with pytest.raises(A.AsdrError, match="more records"):
        t.write_state(np.zeros(7, dtype=A.PACKET_STATE_DTYPE))
    with pytest.raises(A.AsdrError, match="records for"):
        t.write_state(bad, channels=[1, 2])
    assert t.read_state().tobytes() == want.tobytes()
    t.write_state(rec[:2])                                                      # channels 0, 1
    assert t.read_state()[:2].tobytes() == rec[:2].tobytes()


def test_clear_and_reset(A):
    t = decoder(A)
    t.set_space_boost(300, ch=1)
    t.write_state(filled_records(A), channels=[0, 3, 4])
    before = t.read_state()
    t.clear()                                                                   # zeroes five counters; frames and everything else stay
    st = t.read_state()
    ref = PR.PacketRef(6)
    for c in range(6):
        ref.put(c, before[c])
    ref.clear()
    assert st.tobytes() == ref.records().tobytes()
    for k in PR.STATE_NAMES:
        if k in PR.COUNTERS:
            assert not st[k].any() and before[k].any(), k
        else:
            assert np.array_equal(st[k], before[k]), k
    assert st["frames"].tolist() == [2**32 - 1, 0, 0, 0, 4, 0] and "frames" not in PR.COUNTERS
    assert t.blocks() == 0 and t.ring_state()[1].tolist() == [0] * 6
    t.reset()
    assert t.read_state().tobytes() == creation_records(6) and t.blocks() == 0 and settings(t)[1] == 300
    assert t.ring_state()[0].tolist() == [0] * 6


def test_the_helpers_agree_with_the_restatement(A):
    assert A.packet_fcs(b"123456789") == 0x906E == PR.fcs(b"123456789")
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 15, 330, 1000):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert A.packet_fcs(data) == PR.fcs(data), n
    for kw, text in ((dict(), "N0CALL>APRS"), (dict(src="DB0XYZ-15", dst="APDR16-1"), "DB0XYZ-15>APDR16-1"),
                     (dict(src="K1A", path=("WIDE1-1*", "WIDE2-2")), "K1A>APRS,WIDE1-1*,WIDE2-2"),
                     (dict(path=tuple("DIGI%d-%d%s" % (k, k + 1, "*" if k < 5 else "") for k in range(8))),
                      "N0CALL>APRS," + ",".join("DIGI%d-%d%s" % (k, k + 1, "*" if k < 5 else "") for k in range(8)))):
        p = PR.ui_frame(**kw)
        assert A.packet_format_address(p) == text == PR.format_address(p)
        f = np.zeros((), dtype=A.PACKET_FRAME_DTYPE)
        f["length"] = len(p); f["data"][:len(p)] = np.frombuffer(p, dtype=np.uint8)
        assert A.packet_format_address(f[()]) == text
    good = PR.ui_frame()
    no_end = bytes(v & 0xFE if k % 7 == 6 else v for k, v in enumerate(good[:14]))      # two addresses and nothing behind them
    odd = bytes([good[0] | 1]) + good[1:]
    control = bytes([0x02]) + good[1:]                                          # character 0x01 shifted
    early = good[:6] + bytes([good[6] | 1]) + good[7:]                          # the end mark in the destination
    for frame, why in ((good[:13], "14 bytes"), (no_end, "end mark"), (odd, "printable"), (control, "printable"), (early, "end mark"),
                       (PR.ui_frame(path=tuple("D%d" % k for k in range(9))), "end mark")):
        assert PR.format_address(frame) is None
        with pytest.raises(A.AsdrError, match=why):
            A.packet_format_address(frame)
    L = A.load_library()
    out = ctypes.create_string_buffer(11)
    assert L.asdr_packet_format_address(good, len(good), out, 11) == -1 and b"out_size" in L.asdr_last_error()
    out = ctypes.create_string_buffer(12)
    assert L.asdr_packet_format_address(good, len(good), out, 12) == 11 and out.value == b"N0CALL>APRS"
    assert L.asdr_packet_format_address(None, 14, out, 12) == -1


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
