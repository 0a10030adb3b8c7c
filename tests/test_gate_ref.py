"""tests/gate_ref.py, the numpy statement of the audio gate (include/asdr_gate.h), against a plain per-sample Python loop on random
rows, the header's two known sequences, the split property (any split into calls equals one call), the dBFS known answers, and the
extremes of one block (E = 2^37, peak 32768)."""
import numpy as np
import pytest

import gate_ref as GR


def plain_gate(rows, open_energy, close_energy, hang_blocks):
    """One channel, sample by sample and block by block, in Python integers: the header's text once more, without numpy and without
    gate_ref.step.  rows: a list of 128-sample lists.  Returns (state tuple in STATE_NAMES order, open after each block)."""
    energy = last = peak = openings = open_blocks = hang = is_open = 0
    opens = []
    for row in rows:
        E = P = 0
        for x in row:
            x = int(x)
            E += x * x
            P = max(P, -x if x < 0 else x)
        if E >= open_energy:
            if not is_open:
                openings += 1
            is_open, hang = 1, hang_blocks
        elif is_open and E >= close_energy:
            hang = hang_blocks
        elif is_open and hang > 0:
            hang -= 1
        elif is_open:
            is_open = 0
        open_blocks += is_open
        energy = (energy + E) % 2**64
        last, peak = E, max(peak, P)
        opens.append(is_open)
    return (energy, last, peak, openings, open_blocks, hang, is_open, 0), opens


def test_the_two_known_sequences():
    for energies, (o, c, h), want in (([0, 10, 0, 0, 0, 0, 0, 0], (10, 5, 2), [0, 1, 1, 1, 0, 0, 0, 0]),
                                      ([9, 10, 9, 4, 4], (10, 5, 0), [0, 1, 1, 0, 0])):
        g = GR.GateRef(1)
        g.set_squelch(o, c, h)
        rows = GR.rows_with_energy(energies)
        assert GR.block_energy_peak(rows)[0].tolist() == energies
        index, packet, opens = g.update(rows[None])
        assert opens[0].tolist() == want
        assert index.tolist() == [0] and np.array_equal(packet[0], rows)
        assert g.st["openings"][0] == 1 and g.st["open_blocks"][0] == sum(want) and g.blocks == len(energies)


def test_against_the_per_sample_loop_on_random_rows():
    rng = np.random.default_rng(11)
    n, nb = 12, 40
    scale = rng.integers(0, 16, size=(n, nb, 1))
    audio = (rng.integers(-32768, 32768, size=(n, nb, 128)) >> scale).astype(np.int16)
    audio[rng.random((n, nb)) < 0.3] = 0
    g = GR.GateRef(n)
    settings = []
    for c in range(n):
        o = int(rng.integers(0, 1 << 36))
        settings.append((o, int(rng.integers(0, o + 1)), int(rng.integers(0, 5))))
        g.set_squelch(*settings[c], ch=c)
    index, packet, opens = g.update(audio)
    delivered = []
    for c in range(n):
        st, op = plain_gate(audio[c].tolist(), *settings[c])
        assert g.state_tuples()[c] == st and opens[c].tolist() == op, c
        if any(op):
            delivered.append(c)
    assert index.tolist() == delivered and 0 < len(delivered) < n
    assert np.array_equal(packet, audio[delivered])
    assert 0 < opens.sum() < opens.size and g.st["openings"].max() >= 2


def test_any_split_into_calls_equals_one_call():
    rng = np.random.default_rng(5)
    n, nb = 6, 30
    audio = (rng.integers(-3000, 3000, size=(n, nb, 128)) * (rng.random((n, nb, 1)) < 0.4)).astype(np.int16)
    thr = int(np.median(GR.block_energy_peak(audio)[0][GR.block_energy_peak(audio)[0] > 0]))

    def run(cuts):
        g = GR.GateRef(n)
        g.set_squelch(thr, thr // 2, 2)
        opens = [g.update(audio[:, a:b])[2] for a, b in zip(cuts[:-1], cuts[1:])]
        return g.state_tuples(), np.concatenate(opens, axis=1), g.blocks

    one = run([0, nb])
    assert 0 < one[1].sum() < one[1].size
    for cuts in ([0, 1, nb], list(range(nb + 1)), [0, 7, 8, 19, nb], [0] + sorted(rng.choice(np.arange(1, nb), 5, replace=False).tolist()) + [nb]):
        got = run(cuts)
        assert got[0] == one[0] and np.array_equal(got[1], one[1]) and got[2] == nb, cuts


def test_capacity_clear_and_reset():
    g = GR.GateRef(4)
    audio = np.full((4, 3, 128), 100, dtype=np.int16)
    index, packet, _ = g.update(audio, n_blocks=2, capacity_rows=3)
    assert index.tolist() == [0, 1, 2, 3] and packet.shape == (3, 2, 128)
    g.set_squelch(10**9, 0, 7)
    g.update(audio)                        # below open, above close: stays open, hang re-armed
    assert (g.st["open"] == 1).all() and (g.st["hang_left"] == 7).all() and (g.st["open_blocks"] == 5).all()
    g.clear()
    assert g.blocks == 0 and g.state_tuples() == [(0, 0, 0, 0, 0, 7, 1, 0)] * 4
    g.reset()
    assert g.state_tuples() == [(0,) * 8] * 4 and g.settings[0] == (10**9, 0, 7)


@pytest.mark.parametrize("db, want", [(0.0, 137430564992), (-20.0, 1374305650), (-60.0, 137431), (-120.0, 0), (3.0, 1 << 37)])
def test_dbfs_known_answers(db, want):
    assert GR.energy_from_dbfs(db) == want


def test_a_full_scale_sine_sits_3_dB_down():
    x = np.rint(32767 * np.sin(2 * np.pi * 5 * np.arange(128) / 128)).astype(np.int16)
    E = int(GR.block_energy_peak(x)[0])
    assert GR.energy_from_dbfs(-3.02) < E < GR.energy_from_dbfs(-3.00)


def test_the_extremes_of_one_block():
    E, P = GR.block_energy_peak(np.full((1, 128), -32768, dtype=np.int16))
    assert int(E[0]) == 1 << 37 and int(P[0]) == 32768
    g = GR.GateRef(1)
    g.st["energy"][0] = 2**64 - 5
    g.update(np.full((1, 1, 128), -32768, dtype=np.int16))
    assert g.state_tuples()[0][:3] == ((1 << 37) - 5, 1 << 37, 32768)
