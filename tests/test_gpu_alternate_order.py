"""The alternating channel order (include/asdr.h asdr_set_alternate_order, switched on here: it ships off): the plain kind's one-block direct
launches walk their channels forwards in one launched block and backwards in the next.  Only which workgroup takes which channels changes, so
everything is the oracle's at tolerance 0: int16 audio of every channel and block, the status getters of every channel after every call.  Every channel has an input
row of its own (tests/alternate_order_scenarios.py): a row or a state row taken from another workgroup's channel cannot cancel out.

EVERY case asserts, call by call, the launch census (the kernel the scenario names ran, never a fall-back) and asdr_reversed_launches (the
launches of odd launched blocks ran reversed, the others did not).  tests/test_alternate_order_scenarios.py shows without a GPU that the
schedules give the launch forms asserted here."""
import numpy as np
import pytest

import alternate_order_scenarios as AO
import four_wave_scenarios as F
from test_gpu_four_wave import _Oracles, _check_status
from test_gpu_uniform_params import _Run, _census

pytestmark = pytest.mark.gpu

_REFERENCES = {}


def _reference(ao, sc):
    """inputs and oracles of a scenario: computed once, shared, left alone"""
    if sc.name not in _REFERENCES:
        bI, bQ = sc.rows()
        run = _Oracles(ao, sc, bI, bQ)
        want = run.want()
        want.setflags(write=False)
        _REFERENCES[sc.name] = (bI, bQ, run, want)
    return _REFERENCES[sc.name]


def _run(gpu, ao, sc):
    bI, bQ, run, want = _reference(ao, sc)

    def configure(b):
        F.apply_to_batch(b, sc.setup, sc.n)
        b.set_alternate_order(True)                      # (off by default: the form is run explicitly)

    r = _Run(gpu, sc.n, bI, bQ, configure)
    try:
        assert r.b.reversed_launches() == 0
        blk, rev = 0, 0
        for blocks, stream, before in sc.plan:
            if blk in sc.script or before is not None:
                r.b.synchronize(); r.hip.sync(r.caller)
                F.apply_to_batch(r.b, sc.script.get(blk, ()), sc.n)
                if before is not None:
                    before(r.b)
            off = r.pos * 256
            r.b.update_device_strided(r.dI + off, r.dQ + off, r.dO + off, blocks, r.total, r.total, gpu.STREAM_BATCH if stream == "batch" else r.caller)
            r.pos += blocks
            got, expect, rev_call = _census(gpu), {}, 0
            for k in range(blk, blk + blocks):
                assert k == blk or k not in sc.script, "a script entry inside a call"
                c = sc.census(k, AO.launches_per_block(sc, k))
                if c is None:
                    expect = None
                else:
                    for name, v in c.items():
                        expect[name] = expect.get(name, 0) + v
                rev_call += AO.reversed_in_block(sc, k)
            if expect is None:                           # no direct group here: whatever runs, none of the kernels that take the order
                assert got and not any(k in got for k in AO.ORDERED), "blocks %d..: %s" % (blk, got)
            else:
                assert got == expect, "blocks %d..%d: launched %s, expected %s" % (blk, blk + blocks - 1, got, expect)
            rev += rev_call
            assert r.b.reversed_launches() == rev, "blocks %d..%d: %d reversed launches so far, expected %d" % (blk, blk + blocks - 1, r.b.reversed_launches(), rev)
            blk += blocks
            _check_status(r, run, blk - 1)
        got = r.audio()
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%d samples differ, first at (channel, block, sample) %s" % (len(bad), bad[0].tolist())
    finally:
        r.close()


@pytest.mark.parametrize("sc", [AO.uniform(), AO.mixed()], ids=lambda sc: sc.name)
def test_both_orders_on_the_batch_stream_and_on_a_callers(gpu, ao, sc):
    """1,024 channels with C2's settings, by broadcast (asdr_update_kernel_mw_u) and with one field of one mid-workgroup channel changed
    (asdr_update_kernel_mw): 8 single-block calls on ASDR_STREAM_BATCH, 8 on a caller's stream -- both parities several times on either,
    the state handed across every turn and across the change of stream."""
    _run(gpu, ao, sc)


@pytest.mark.parametrize("sc", AO.partial(), ids=lambda sc: sc.name)
def test_partial_last_workgroup_dispatched_first(gpu, ao, sc):
    """520, 528, 536 and 552 channels: the last LOGICAL workgroup holds 1, 2, 3 and 1 waves; under reversal it is hardware workgroup 0 and
    its padding waves work on the dummy channel."""
    _run(gpu, ao, sc)


def test_direct_group_behind_other_channels(gpu, ao):
    """a direct group that starts at channel 512 behind 512 SAM channels (direct_ch0 != 0); the SAM launches keep the ascending order"""
    _run(gpu, ao, AO.offset())


def test_staggered_mixer_phases(gpu, ao):
    """bench.py's stagger_divergent_phases on 1,024 channels: 8 different mixer phases in every wave, under both orders"""
    _run(gpu, ao, AO.stagger())


@pytest.mark.parametrize("lanes", [False, True], ids=["ordinary", "lanes"])
def test_order_alternates_inside_a_multi_block_call(gpu, ao, lanes):
    """8,192 channels: calls of 3 and of 4 blocks as one launch per block with a setter in between, then a call of 2 blocks -- on the
    lanes (each lane reverses within its own half) or the ordinary way"""
    _run(gpu, ao, AO.multi_block(lanes))


def test_switching_the_order_off_and_on(gpu, ao):
    """asdr_set_alternate_order(0) for blocks 3 and 4 of 8: the same audio, and the reversed-launch counter stands still meanwhile"""
    _run(gpu, ao, AO.toggling())


def test_blanker_general_path_across_the_turn(gpu, ao):
    """an impulse in every block of every channel: detections, mask rows and re-scanned envelopes carried from one order into the other"""
    _run(gpu, ao, AO.blanker())


def test_off_by_default(gpu, ao):
    """a batch nobody switched runs every launch in the ascending order: the counter stays at 0 over both parities (audio as in every case)"""
    sc = AO.uniform()
    bI, bQ, run, want = _reference(ao, sc)
    r = _Run(gpu, sc.n, bI, bQ, lambda b: F.apply_to_batch(b, sc.setup, sc.n))
    try:
        r.step(4, gpu.STREAM_BATCH)
        r.step(4, r.caller)
        got = r.audio()
        assert _census(gpu) == {AO.MW_U: 8} and r.b.reversed_launches() == 0
        assert np.array_equal(got[:, :8], want[:, :8])
    finally:
        r.close()
