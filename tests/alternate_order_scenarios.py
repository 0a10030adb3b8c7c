"""Scenario definitions for the alternating channel order of the plain kind's one-block direct launches (include/asdr.h
asdr_set_alternate_order), shared by tests/test_gpu_alternate_order.py (GPU, against the oracle) and tests/test_alternate_order_scenarios.py
(CPU: the schedule gives the launch forms asserted there).

The scenario type, the setters and the oracle harness are tests/four_wave_scenarios.py's.  What differs: EVERY channel has an input row of
its own (a carrier offset and a noise seed per channel), so U = n -- a workgroup that took the rows of another one (channel c <-> c + 32 k)
would meet the same row again under c % 8 or c % 16 -- and a scenario carries a PLAN: the calls it is run as.

    plan = [(blocks, stream, before)]   blocks: blocks of the call; stream: "batch" / "caller"; before: callable(batch) or None, applied in
                                        front of the call beside the scenario's script (switches that are no setters of the oracle)
"""
import numpy as np

import four_wave_scenarios as F
from cases import LSB, USB, SAM, imp, am
from helpers import S

MW_U, MW, MIXED = F.MW_U, F.MW, F.MIXED
ONE = "asdr_update_kernel_one"
ORDERED = (MW_U, MW, ONE)                                # the kernels that take the order (in a direct group's launch)
C2 = [S("setDemodMode", USB), S("enableAudioFilter")]


def rows(n, total, sig=imp, impulse_every=1300, noise=0.02, spread=3000.0):
    """n input rows: channel c's carrier spread / n Hz from its neighbours' (all inside the IF passband), noise seed 12345 + c"""
    from audiosdr_amd.synth import make_iq
    p = dict(sig)
    fc = p.pop("fc") - 0.5 * spread + spread * np.arange(n) / n
    p.setdefault("noise", noise)
    p["impulse_every"] = impulse_every
    return make_iq(n, total, fc=fc, **p)


class Scenario(F.Scenario):
    def __init__(self, name, total, setup, plan, script=None, n=1024, expect="u", sig=imp, impulse_every=1300, spread=3000.0, **kw):
        super().__init__(name, lambda: rows(n, total, sig, impulse_every, spread=spread), setup, script, n=n, expect=expect, **kw)
        self.total, self.plan = total, plan
        assert sum(p[0] for p in plan) == total

    def alternate(self, blk):
        """asdr_set_alternate_order as it stands while block blk runs (the toggling scenario overrides)"""
        return True


def single_blocks(total, on_caller):
    """`total` single-block calls, those from block `on_caller` on on a caller's stream"""
    return [(1, "batch" if k < on_caller else "caller", None) for k in range(total)]


def uniform():
    return Scenario("uniform-1024", 16, C2, single_blocks(16, 8))


def mixed():
    return Scenario("mixed-1024", 16, C2 + [S("setOutputGain", 0.7, sel=F.MID)], single_blocks(16, 8), expect="r")


def partial():
    """a last workgroup of 1, 2, 3 and (17 workgroups in front of it) 1 waves: the first one dispatched under reversal"""
    return [Scenario("n%d" % n, 6, C2, single_blocks(6, 4), n=n) for n in (520, 528, 536, 552)]


def offset():
    sam = [S("setDemodMode", SAM, sel=lambda c: c < 512), S("setDemodMode", USB, sel=lambda c: c >= 512), S("enableAudioFilter")]
    three = {k: 1 for k in F.SAM_KERNELS}
    return Scenario("sam512-usb512", 6, sam, single_blocks(6, 4), expect=dict(three, **{MW_U: 1}), sig=am, impulse_every=500, spread=200.0,
                    plain_waves=64, uniform_groups=2, direct_slots=1024)


STAGGER_BLOCKS = 14


def stagger():
    """bench.py's stagger_divergent_phases: all channels start in LSB, the channels with c mod 8 == j switch to USB in front of block j.  Blocks
    0..6: every wave holds both modes -- one schedule key, but no direct group: the one-wave kernel reads its schedule slots and keeps the
    ascending order (nothing reversed).  From block 7 on one direct group whose every wave holds 8 different mixer phases: the oscillator
    cache's writer finds no common phase, every wave runs the per-channel lookups."""
    script = {j: [S("setDemodMode", USB, sel=lambda c, j=j: c % 8 == j)] for j in range(8)}
    sc = Scenario("stagger-1024", STAGGER_BLOCKS, [S("setDemodMode", LSB), S("enableAudioFilter")], single_blocks(STAGGER_BLOCKS, 11), script,
                  expect=lambda blk: {ONE: 1} if blk < 7 else "u")
    sc.direct_slots = lambda blk: 0 if blk < 7 else sc.n
    return sc


def multi_block(lanes):
    """8,192 channels = 1,024 waves, from which a multi-block call is issued as one launch per block: a call of 3 blocks, a broadcast setter, a call
    of 4 blocks (both flush, so both run the ordinary per-block loop), then a call of 2 blocks that takes the lanes when they are on (each lane
    its own half, block by block)."""
    lanes_on = (lambda b: b.set_lanes(True)) if lanes else (lambda b: b.set_lanes(False))
    sc = Scenario("multi-block-%s" % ("lanes" if lanes else "ordinary"), 9, C2, [(3, "caller", lanes_on), (4, "caller", None), (2, "batch", None)],
                  script={3: [S("setOutputGain", 0.7)]}, n=8192)
    sc.launches_per_block = lambda blk: 2 if (lanes and blk >= 7) else 1
    return sc


def toggling():
    """the order switched off in front of block 3 and on again in front of block 5"""
    plan = single_blocks(8, 6)
    plan[3] = (1, "batch", lambda b: b.set_alternate_order(False))
    plan[5] = (1, "batch", lambda b: b.set_alternate_order(True))
    sc = Scenario("toggling-1024", 8, C2, plan)
    sc.alternate = lambda blk: not (3 <= blk < 5)
    return sc


def blanker():
    """an impulse in every block of every channel: the blanker's general path, its mask row handed across the turn"""
    return Scenario("impulse-every-block-1024", 8, C2, single_blocks(8, 5), impulse_every=128)


def all_scenarios():
    return [uniform(), mixed()] + partial() + [offset(), stagger(), multi_block(False), multi_block(True), toggling(), blanker()]


def launches_per_block(sc, blk):
    return getattr(sc, "launches_per_block", lambda blk: 1)(blk)


def reversed_in_block(sc, blk):
    """launches of block blk that run in the reversed order: the batch's parity advances with every launched block, whatever the switch says,
    and every launch of an odd block that runs a DIRECT group on one of the ORDERED kernels is reversed while the switch is on"""
    census = sc.census(blk, launches_per_block(sc, blk)) or {}
    return sum(v for k, v in census.items() if k in ORDERED) if (sc.alternate(blk) and blk % 2 == 1 and sc.direct_slots(blk) > 0) else 0
