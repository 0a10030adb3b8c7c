"""The audio gate's control plane (include/asdr_gate.h) on an ASDR_NO_DEVICE gate: the creation values, broadcast and per-channel
setters and getters, that each refusal leaves everything as it was, write_state's validation, the calls that need a device, the
exported names and the record size, and the C dBFS helper against tests/gate_ref.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import gate_ref as GR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def gate(A, n=6):
    return A.AudioGate(n, device=A.NO_DEVICE)


def test_every_declared_name_is_exported_and_bound(A):
    with open(os.path.join(ROOT, "include", "asdr_gate.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(asdr_gate_\w+)\s*\(", text)))
    assert len(declared) == 16 and "asdr_gate_deliver" in declared and "asdr_gate_update_device" in declared
    L = ctypes.CDLL(A.library_path())
    for n in declared:
        assert hasattr(L, n), n
    assert sorted(A.GATE_EXPORTS) == declared
    assert not [n for n in A.GATE_EXPORTS if n in A.binding.EXPORTS]


def test_the_state_record_is_32_bytes(A):
    assert A.GATE_STATE_DTYPE.itemsize == 32 and A.GATE_STATE_DTYPE.names == GR.STATE_NAMES
    assert [A.GATE_STATE_DTYPE.fields[k][1] for k in GR.STATE_NAMES] == [0, 8, 16, 20, 24, 28, 30, 31]
    src = "#include \"asdr_gate.h\"\n_Static_assert(sizeof(asdr_gate_state_t) == 32, \"size\");\n"
    import subprocess
    inc = os.path.join(ROOT, "include")
    r = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", inc, "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = gate(A, 3)
    st = g.read_state()                                        # the library fills exactly 3 * 32 bytes
    assert st.shape == (3,) and st.nbytes == 96


def test_creation_values(A):
    g = gate(A)
    assert g.n_channels == 6 and g._L.asdr_gate_n_channels(g._h) == 6 and g.blocks() == 0
    assert all(g.get_squelch(c) == (0, 0, 0) for c in range(6))
    assert GR.record_tuples(g.read_state()) == [(0,) * 8] * 6
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(A.AsdrError, match="n_channels"):
            A.AudioGate(n, device=A.NO_DEVICE)
    assert A.AudioGate(1 << 20, device=A.NO_DEVICE).n_channels == 1 << 20


def test_setters_getters_and_refusals(A):
    g = gate(A)
    g.set_squelch(energies=(1000, 10), hang_blocks=3)                        # broadcast
    assert all(g.get_squelch(c) == (1000, 10, 3) for c in range(6))
    g.set_squelch(energies=(2**64 - 1, 2**64 - 1), hang_blocks=65535, ch=4)  # the ends of every range
    g.set_squelch(energies=(7, 7), hang_blocks=0, ch=0)
    want = [(7, 7, 0)] + [(1000, 10, 3)] * 3 + [(2**64 - 1, 2**64 - 1, 65535), (1000, 10, 3)]
    assert [g.get_squelch(c) for c in range(6)] == want
    for ch in (0, 4, A.ALL):
        with pytest.raises(A.AsdrError, match="close_energy"):
            g.set_squelch(energies=(10, 11), ch=ch)
        for hang in (-1, 65536, 1 << 20):
            with pytest.raises(A.AsdrError, match="hang_blocks"):
                g.set_squelch(energies=(10, 5), hang_blocks=hang, ch=ch)
    for ch in (-2, 6, 1 << 20):
        with pytest.raises(A.AsdrError, match="bad channel"):
            g.set_squelch(energies=(10, 5), ch=ch)
        with pytest.raises(A.AsdrError, match="bad channel"):
            g.get_squelch(ch)
    with pytest.raises(A.AsdrError, match="bad channel"):
        g.get_squelch(A.ALL)
    assert [g.get_squelch(c) for c in range(6)] == want                      # every refusal left everything as it was
    assert g._L.asdr_gate_set_squelch(None, 0, 1, 1, 0) == -1 and g._L.asdr_gate_blocks(None) == -1
    g.set_squelch(open_db=-20.0, close_db=-26.0, hang_blocks=2, ch=1)        # the dBFS form
    assert g.get_squelch(1) == (GR.energy_from_dbfs(-20.0), GR.energy_from_dbfs(-26.0), 2)
    g.set_squelch(open_db=-30.0, ch=2)
    assert g.get_squelch(2) == (GR.energy_from_dbfs(-30.0),) * 2 + (0,)
    g.set_squelch(ch=3)
    assert g.get_squelch(3) == (0, 0, 0)
    g.reset()                                                                # keeps the settings
    assert g.get_squelch(4) == want[4] and g.get_squelch(0) == want[0]


def test_write_state_validation_is_all_or_nothing(A):
    g = gate(A)
    rec = np.zeros(3, dtype=A.GATE_STATE_DTYPE)
    rec["energy"] = [2**64 - 5, 1, 2]; rec["last_energy"] = [1 << 37, 0, 9]; rec["peak"] = [32768, 0, 3]
    rec["openings"] = [2**32 - 1, 0, 1]; rec["open_blocks"] = [5, 0, 1]; rec["hang_left"] = [65535, 0, 9]; rec["open"] = [1, 0, 1]
    g.write_state(rec, channels=[5, 0, 2])
    want = [(0,) * 8] * 6
    for k, c in enumerate([5, 0, 2]):
        want[c] = GR.record_tuples(rec)[k]
    assert GR.record_tuples(g.read_state()) == want                          # hang_left above hang_blocks (0) is allowed
    bad = rec.copy(); bad["energy"] = 77
    for field, value, why in (("open", 2, "open must be 0 or 1"), ("open", 255, "open must be 0 or 1"), ("reserved", 1, "reserved")):
        b = bad.copy(); b[field][2] = value                                  # the LAST record is the bad one
        with pytest.raises(A.AsdrError, match=why):
            g.write_state(b, channels=[1, 3, 4])
    for chans in ([1, 3, 6], [1, -1, 3], [1 << 20, 0, 1]):
        with pytest.raises(A.AsdrError, match="bad channel"):
            g.write_state(bad, channels=chans)
    with pytest.raises(A.AsdrError, match="more records"):
        g.write_state(np.zeros(7, dtype=A.GATE_STATE_DTYPE))
    with pytest.raises(A.AsdrError, match="records for"):
        g.write_state(bad, channels=[1, 2])
    assert GR.record_tuples(g.read_state()) == want
    g.write_state(rec[:2])                                                   # channels 0, 1
    assert GR.record_tuples(g.read_state())[:2] == GR.record_tuples(rec[:2])
    g.clear()                                                                # keeps open and hang_left
    st = g.read_state()
    assert st["open"].tolist() == [1, 0, 1, 0, 0, 1] and st["hang_left"].tolist() == [65535, 0, 9, 0, 0, 65535]
    assert all(int(st[k].astype(np.uint64).sum()) == 0 for k in ("energy", "last_energy", "peak", "openings", "open_blocks", "reserved"))
    g.reset()
    assert GR.record_tuples(g.read_state()) == [(0,) * 8] * 6 and g.blocks() == 0


def test_the_signal_path_needs_a_device(A):
    g = gate(A)
    for call in (lambda: g.update_device(4096, 1), lambda: g.deliver(4096, 1), g.count_tensor, g.index_tensor):
        with pytest.raises(A.AsdrError, match="ASDR_NO_DEVICE"):
            call()
    g.synchronize()
    assert g.blocks() == 0


@pytest.mark.parametrize("db", [0.0, -20.0, -60.0, -120.0, 3.0, -3.01, -200.0, 100.0, float("-inf"), float("inf")])
def test_the_c_helper_equals_the_reference(A, db):
    assert A.energy_from_dbfs(db) == GR.energy_from_dbfs(db)


def test_the_c_helper_known_answers(A):
    got = [A.energy_from_dbfs(db) for db in (0.0, -20.0, -60.0, -120.0, 3.0)]
    assert got == [137430564992, 1374305650, 137431, 0, 1 << 37]
    assert A.energy_from_dbfs(float("nan")) == 0
