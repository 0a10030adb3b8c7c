"""What tests/test_gpu_alternate_order.py relies on, shown without a GPU: every scenario of tests/alternate_order_scenarios.py, built on a
control-plane-only batch, gives the plain waves, the direct groups and the uniform groups its census assertions expect (so that no GPU case
falls back to another launch form), its plan and its script fit together, and the control surface of the order exists on such a batch."""
import numpy as np
import pytest

import alternate_order_scenarios as AO
import four_wave_scenarios as F
from test_four_wave_scenarios import _direct_slots


@pytest.mark.parametrize("sc", AO.all_scenarios(), ids=lambda sc: sc.name)
def test_launch_form_expectations(A, sc):
    b = A.AudioSDRBatch(sc.n, device=-1)
    F.apply_to_batch(b, sc.setup, sc.n)
    for blk in range(sc.total):
        F.apply_to_batch(b, sc.script.get(blk, ()), sc.n)
        st = b.control_plane_flush()
        assert st["waves_plain"] == sc.plain_waves, blk
        assert b.params_uniform_groups()[0] == sc.uniform_groups(blk), blk
        assert _direct_slots(b) == sc.direct_slots(blk), blk
    b.close()


@pytest.mark.parametrize("sc", AO.all_scenarios(), ids=lambda sc: sc.name)
def test_plans(sc):
    """script entries and switches sit in front of a call, never inside one; the four-wave forms are reached (64 waves of one direct group);
    both parities are launched in the ordered kernels"""
    starts, blk = set(), 0
    for blocks, stream, before in sc.plan:
        assert stream in ("batch", "caller")
        starts.add(blk); blk += blocks
    assert blk == sc.total and set(sc.script) <= starts
    ordered = [k for k in range(sc.total) if sc.direct_slots(k) > 0 and any(n in AO.ORDERED for n in (sc.census(k) or {}))]
    assert {k % 2 for k in ordered} == {0, 1}
    assert sum(AO.reversed_in_block(sc, k) for k in range(sc.total)) >= 2
    assert sc.direct_slots(ordered[0]) >= 512


def test_every_channel_has_a_row_of_its_own():
    I, Q = AO.rows(1024, 2)
    assert len({I[c].tobytes() for c in range(1024)}) == 1024 and len({Q[c].tobytes() for c in range(1024)}) == 1024


def test_partial_workgroups():
    assert [(sc.n // 8) % 4 for sc in AO.partial()] == [1, 2, 3, 1] and all(sc.n % 8 == 0 for sc in AO.partial())


def test_toggling_expectation():
    sc = AO.toggling()
    assert [AO.reversed_in_block(sc, k) for k in range(8)] == [0, 1, 0, 0, 0, 1, 0, 1]


def test_multi_block_expectation():
    """calls of 3, 4 and 2 blocks: the parity runs on through the calls; on the lanes both halves of an odd block are reversed"""
    assert [AO.reversed_in_block(AO.multi_block(False), k) for k in range(9)] == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    assert [AO.reversed_in_block(AO.multi_block(True), k) for k in range(9)] == [0, 1, 0, 1, 0, 1, 0, 2, 0]


def test_control_surface_without_a_device(A):
    b = A.AudioSDRBatch(64, device=-1)
    assert b.reversed_launches() == 0
    b.set_alternate_order(False); b.set_alternate_order(True)
    assert b.reversed_launches() == 0
    b.close()
