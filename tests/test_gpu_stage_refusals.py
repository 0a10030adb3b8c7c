"""The refusals of a block-row call on the GPU, stage by stage (FM demodulator, tone squelch, DCS squelch, packet decoder, gate): the
whole text a bad call leaves, and which of two simultaneous faults is reported.  The order is that of the checks in front of the
kernels, which write through the caller's pointers: a null pointer, n_blocks outside 0..65535, a stride shorter than n_blocks, a stride
above 2^30, a pointer off 16 bytes, then -- unless n_blocks is 0, which returns success -- the overlap of the spans.  The control
tests cannot reach these: an ASDR_NO_DEVICE handle refuses earlier.  After every refused call the records and blocks() are what they
were.  Handles of 2 channels, buffers of 4 blocks; every pointer of a row that is not null lies inside one 64 KiB allocation, and so
does every span whose strides are not the point of the row."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, NB = 2, 4                       # channels, blocks
REGION = 4096                      # bytes between the row buffers below: N * NB * 256 = 2048 are used
BIG = (1 << 30) + 1                # a stride one block too large

NULL = "null device pointer"
BLOCKS = "n_blocks must be in 0..65535"
SHORT = "row stride shorter than n_blocks"
LARGE = "row stride too large"
ALIGNED = "device pointers must be 16-byte aligned"
OVERLAP_AN = "output span overlaps an input span"
OVERLAP_THE = "output span overlaps the input span"
OVERLAP_PACKET = "packet span overlaps the audio span"
CAPACITY = "capacity_rows is negative"


@pytest.fixture(scope="module")
def rows(gpu):
    """(tensor, I, Q, O): one device allocation of random int16 and three disjoint row buffers in it, 16-byte aligned."""
    import torch
    rng = np.random.default_rng(20)
    t = torch.from_numpy(rng.integers(-12000, 12000, size=32768, dtype=np.int16)).cuda()
    torch.cuda.synchronize()
    base = t.data_ptr()
    assert base % 16 == 0
    return t, base, base + REGION, base + 2 * REGION


def in_out_table(a, o, overlap):
    """(in_ptr, out_ptr, n_blocks, in_stride, out_stride, text or None) of a stage with one input and one output."""
    return [
        (0, o, NB, NB, NB, NULL), (a, 0, NB, NB, NB, NULL), (0, 0, NB, NB, NB, NULL),
        (0, o, -1, NB, NB, NULL), (a, 0, 0, NB, NB, NULL), (0, o + 2, NB, 3, BIG, NULL),          # a null pointer comes first
        (a, o, -1, NB, NB, BLOCKS), (a, o, 65536, 65536, 65536, BLOCKS),
        (a + 2, o, 65536, 3, NB, BLOCKS), (a, o, -1, 0, BIG, BLOCKS),                             # ... then n_blocks
        (a, o, NB, 3, NB, SHORT), (a, o, NB, NB, 3, SHORT), (a, o, 1, 0, 1, SHORT),
        (a + 2, o, NB, 3, NB, SHORT), (a, o + 8, NB, NB, 3, SHORT),                               # a misaligned pointer and a short stride
        (a, o, NB, 3, BIG, SHORT), (a, o, NB, BIG, 3, SHORT),                                     # one stride short, the other too large
        (a, o, NB, BIG, NB, LARGE), (a, o, NB, NB, BIG, LARGE), (a + 2, o + 2, NB, BIG, BIG, LARGE),
        (a, a, 0, NB, BIG, LARGE),                                                                # n_blocks = 0 still checks its arguments
        (a + 2, o, NB, NB, NB, ALIGNED), (a, o + 8, NB, NB, NB, ALIGNED), (a + 14, o + 2, NB, NB, NB, ALIGNED),
        (a, a + 8, NB, NB, NB, ALIGNED), (a + 2, a + 2, NB, NB, NB, ALIGNED),                     # misaligned and overlapping
        (a, a + 2, 0, NB, NB, ALIGNED),
        (a, a, NB, NB, NB, overlap), (a, a + 256, 2, NB, NB, overlap), (a + 2032, a, NB, NB, NB, overlap),
        (a, a + 2032, NB, NB, NB, overlap), (o, o + 1024 + 240, 1, NB, NB, overlap),              # the second row's one block
        (a, a, 0, NB, NB, None), (a, a + 256, 0, NB, NB, None),                                   # n_blocks = 0 and overlapping spans: success
        (a, a + 2048, NB, NB, NB, None),                                                          # spans that touch: the call runs
    ]


def run_table(gpu, stage, table, call, nb_at):
    """Every row of the table through call(*row[:-1]), whose argument nb_at is n_blocks.  A refused row leaves its whole text, and the
    records and blocks() as they were; so does a row of no blocks, which succeeds."""
    before, blocks = stage.read_state().tobytes(), stage.blocks()
    assert blocks == NB
    for row in table:
        args, text = row[:-1], row[-1]
        if text is None:
            call(*args)
            stage.synchronize()
            blocks += args[nb_at]
            if args[nb_at] > 0:
                before = stage.read_state().tobytes()
        else:
            with pytest.raises(gpu.AsdrError) as e:
                call(*args)
            assert str(e.value) == text, (row, str(e.value))
        assert stage.read_state().tobytes() == before and stage.blocks() == blocks, row


def test_fm_refusals(gpu, rows):
    _, i, q, o = rows
    fm = gpu.FmDemodulator(N)
    fm.update_device(i, q, o, NB)
    fm.synchronize()
    # (i_ptr, q_ptr, out_ptr, n_blocks, in_stride, out_stride, text): the input's fault in I, then in Q
    table = [(r[0], q) + r[1:] for r in in_out_table(i, o, OVERLAP_AN)] + [(i, r[0]) + r[1:] for r in in_out_table(i, o, OVERLAP_AN)]
    table += [(0, 0, 0, NB, NB, NB, NULL), (i, q, q, NB, NB, NB, OVERLAP_AN), (i, q, q + 256, 2, NB, NB, OVERLAP_AN),
              (i, i, o, NB, NB, NB, None)]                                                        # I and Q may be the same rows
    run_table(gpu, fm, table, lambda ip, qp, op, nb, si, so: fm.update_device(ip, qp, op, nb, in_stride_blocks=si, out_stride_blocks=so), 3)
    fm.close()


@pytest.mark.parametrize("name", ["ToneSquelch", "DcsSquelch"])
def test_tone_and_dcs_refusals(gpu, rows, name):
    _, a, _, o = rows
    sq = getattr(gpu, name)(N)
    sq.update_device(a, o, NB)
    sq.synchronize()
    run_table(gpu, sq, in_out_table(a, o, OVERLAP_THE), lambda ip, op, nb, si, so: sq.update_device(ip, op, nb, in_stride_blocks=si, out_stride_blocks=so), 2)
    sq.close()


def test_packet_refusals(gpu, rows):
    _, a, _, _ = rows
    pk = gpu.PacketDecoder(N)
    pk.update_device(a, NB)
    pk.synchronize()
    ring = [v.tobytes() for v in pk.ring_state()]
    table = [(0, NB, NB, NULL), (0, -1, NB, NULL), (0, 0, BIG, NULL), (a, -1, NB, BLOCKS), (a, 65536, 65536, BLOCKS), (a + 2, 65536, 3, BLOCKS),
             (a, NB, 3, SHORT), (a, 1, 0, SHORT), (a + 2, NB, 3, SHORT), (a, NB, BIG, LARGE), (a + 8, NB, BIG, LARGE), (a, 0, BIG, LARGE),
             (a + 2, NB, NB, ALIGNED), (a + 8, 1, NB, ALIGNED), (a + 8, 0, NB, ALIGNED), (a, 0, NB, None), (a, 0, 0, None)]
    run_table(gpu, pk, table, lambda ip, nb, si: pk.update_device(ip, nb, in_stride_blocks=si), 1)
    assert [v.tobytes() for v in pk.ring_state()] == ring
    pk.close()


def test_gate_refusals(gpu, rows):
    _, a, _, o = rows
    g = gpu.AudioGate(N)
    g.update_device(a, NB)
    g.synchronize()
    # (ptr, n_blocks, stride_blocks, rows_ptr, capacity_rows, text)
    table = [(0, NB, NB, 0, 0, NULL), (0, -1, NB, o, -1, NULL), (a, -1, NB, 0, 0, BLOCKS), (a, 65536, 65536, 0, 0, BLOCKS), (a + 2, 65536, 3, o, -1, BLOCKS),
             (a, NB, 3, 0, 0, SHORT), (a + 2, NB, 3, o, N, SHORT), (a, NB, 3, o + 8, -1, SHORT), (a, NB, BIG, 0, 0, LARGE), (a + 2, NB, BIG, o, -1, LARGE),
             (a + 2, NB, NB, 0, 0, ALIGNED), (a + 8, NB, NB, o, -1, ALIGNED),                     # the audio rows are checked first
             (a, NB, NB, o, -1, CAPACITY), (a, NB, NB, 0, -1, CAPACITY), (a, NB, NB, a + 8, -1, CAPACITY), (a, 0, NB, o, -1, CAPACITY),
             (a, NB, NB, o + 8, N, ALIGNED), (a, NB, NB, a + 8, N, ALIGNED), (a, NB, NB, o + 2, 1, ALIGNED),
             (a, NB, NB, a, N, OVERLAP_PACKET), (a, 2, NB, a + 256, 1, OVERLAP_PACKET), (a, NB, NB, a + 2032, 1, OVERLAP_PACKET),
             (a + 1024, NB, NB, a, 1, None),                                                      # one packet row ends where the audio begins
             (a + 1024, NB, NB, a, N, OVERLAP_PACKET),                                            # two do not
             (a, 0, NB, a, N, None), (a, 0, NB, a + 8, N, None), (a, 0, NB, o, 0, None),          # n_blocks = 0: success, whatever the packet rows
             (a, NB, NB, a, 0, None), (a, NB, NB, o, N, None)]                                    # no room for a packet: its pointer is not looked at
    run_table(gpu, g, table, lambda p, nb, st, rp, cap: g.update_device(p, nb, stride_blocks=st, rows_ptr=rp, capacity_rows=cap), 1)
    g.close()
