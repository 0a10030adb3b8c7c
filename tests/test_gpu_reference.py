"""The HIP path against the REFERENCE'S OWN CODE, with no oracle in between.  oracle/_ref/ (oracle/ref_build.py: the reference's
sources compiled on the stand-in headers of oracle/ref_shim/, shipped with the tree by build()) is all this file reads; missing or stale
binaries fail it.  The reference runs in fresh child processes (which never open the GPU), all of them before this file creates its
first GPU object.  Inputs, exclusions and comparison rules: tests/ref_scenarios.py (the same as tests/test_reference_binary.py); the
out-of-int32 mask comes from the product's own ALS stage tap.

  * every channel of every case (less the one exclusion) in ONE mixed batch padded to the longest case, run block by block and as one
    multi-block update: audio, 27 getters and the AGC table of every channel against its own reference process;
  * the same channels tiled to ~4,000 (the four-wave form, host-sorted sub-ranges), every channel against its reference output;
  * fuzz seeds 1-24, each channel's setters applied between the batch's update calls;
  * 728-block runs in which every AGC mode's hang time runs out;
  * AudioIQgeneratorBatch, AudioGrabberComplex256Batch, AudioSDRpreProcessorBatch's fixed corrections and swap, and every image
    detector scenario as channels of one batch, outputs and both getters after every block."""
import numpy as np
import pytest

import ref_scenarios as R
from cases import CASES
from oracle import ref_build

pytestmark = pytest.mark.gpu
N_LARGE = 4000


@pytest.fixture(scope="module")
def ref():
    R.require_binaries(skip_without_either=False)
    pad = max(CASES[n][1] for n in R.CASE_NAMES)
    cases, fuzz, agc = R.case_channels(pad_to=pad), R.fuzz_channels(), R.long_agc_channels()
    jobs = {("sdr", ch["label"]): (ref_build.run_sdr, (ch["script"], ch["I"], ch["Q"])) for ch in cases + fuzz + agc}
    for label, bal, x in R.iqgen_inputs():
        jobs[("iqgen", label)] = (ref_build.run_iqgen, (bal, x))
    gI, gQ = R.grab_input()
    for after in R.GRAB_AFTER:
        jobs[("grab", after)] = (ref_build.run_grab, (gI, gQ, after))
    for corr, swap in R.PRE_FIXED:
        jobs[("pre", corr, swap)] = (ref_build.run_pre_fixed, (corr, swap, gI, gQ))
    scen = R.detector_scenarios()
    for sc in scen:
        jobs[("det", sc["name"])] = (R.run_detector_reference, (sc,))
    return dict(out=R.run_all(jobs), cases=cases, fuzz=fuzz, agc=agc, scen=scen, grab=(gI, gQ))


@pytest.fixture(scope="module")
def dev(ref, request):
    """The product's binding and a device -- requested only once every reference process of this file has run."""
    return request.getfixturevalue("gpu")


def _stack(chans):
    return np.ascontiguousarray(np.stack([ch["I"] for ch in chans])), np.ascontiguousarray(np.stack([ch["Q"] for ch in chans]))


def _apply(batch, c, setters):
    for m, a in setters:
        getattr(batch, m)(*a, ch=c)


def _blockwise(A, chans):
    """One update() per block, each channel's setters between the calls, ALS stage taps on: (batch, audio [ch][blocks][128], mask)."""
    n, nb = len(chans), chans[0]["I"].shape[0]
    I, Q = _stack(chans)
    batch = A.AudioSDRBatch(n)
    batch.enable_taps(True)
    by = [R.setters_by_block(ch["script"], nb) for ch in chans]
    og = np.stack([R.output_gains(ch["script"], nb) for ch in chans])
    got, oob = np.empty((n, nb, 128), np.int16), np.empty((n, nb, 128), bool)
    for b in range(nb):
        for c in range(n):
            _apply(batch, c, by[c].get(b, []))
        got[:, b] = batch.update(I[:, b:b + 1], Q[:, b:b + 1])[:, 0]
        oob[:, b] = R.beyond_int32(batch.read_taps()["ALS"], og[:, b:b + 1])
    for c in range(n):
        _apply(batch, c, by[c].get(nb, []))
    return batch, got, oob


def _check(ref, batch, chans, got, oob, what):
    """Channel c of the batch carries chans[c % len(chans)]: audio (oob: the mask of that source channel), getters, AGC table."""
    for c in range(got.shape[0]):
        ch = chans[c % len(chans)]
        audio, g = ref["out"][("sdr", ch["label"])]
        label = "%s, channel %d (%s)" % (what, c, ch["label"])
        R.check_audio(got[c], audio, oob[c % len(chans)], label)
        R.check_getters(lambda name, *a: getattr(batch, name)(*a, ch=c), g, label)


@pytest.fixture(scope="module")
def cases_blockwise(ref, dev):
    batch, got, oob = _blockwise(dev, ref["cases"])
    yield batch, got, oob
    batch.close()


def test_cases_mixed_batch_block_by_block(ref, cases_blockwise):
    batch, got, oob = cases_blockwise
    _check(ref, batch, ref["cases"], got, oob, "mixed batch, block by block")


def test_cases_mixed_batch_one_multi_block_call(ref, dev, cases_blockwise):
    chans = ref["cases"]
    I, Q = _stack(chans)
    batch = dev.AudioSDRBatch(len(chans))
    for c, ch in enumerate(chans):
        _apply(batch, c, ch["script"])
    got = batch.update(I, Q)
    _check(ref, batch, chans, got, cases_blockwise[2], "mixed batch, one call of %d blocks" % I.shape[1])
    batch.close()


def test_cases_tiled_large_batch(ref, dev, cases_blockwise):
    """The case channels tiled to ~4,000: one call of 1 block, then one of the rest."""
    chans = ref["cases"]
    reps = -(-N_LARGE // len(chans))
    n = reps * len(chans)
    I, Q = _stack(chans)
    I, Q = np.ascontiguousarray(np.tile(I, (reps, 1, 1))), np.ascontiguousarray(np.tile(Q, (reps, 1, 1)))
    batch = dev.AudioSDRBatch(n)
    for c in range(n):
        _apply(batch, c, chans[c % len(chans)]["script"])
    got = np.concatenate([batch.update(I[:, :1], Q[:, :1]), batch.update(I[:, 1:], Q[:, 1:])], axis=1)
    _check(ref, batch, chans, got, cases_blockwise[2], "%d-channel batch" % n)
    batch.close()


def test_fuzz_seeds(ref, dev):
    batch, got, oob = _blockwise(dev, ref["fuzz"])
    _check(ref, batch, ref["fuzz"], got, oob, "fuzz batch")
    batch.close()


def test_long_agc_mode_runs(ref, dev):
    """The AGC modes' hang times run out (hundreds of blocks), one update() per block."""
    batch, got, oob = _blockwise(dev, ref["agc"])
    _check(ref, batch, ref["agc"], got, oob, "long AGC batch")
    batch.close()


def test_iq_generator(ref, dev):
    inputs = R.iqgen_inputs()
    x = np.ascontiguousarray(np.stack([v[2] for v in inputs]))
    for blockwise in (False, True):
        g = dev.AudioIQgeneratorBatch(len(inputs))
        for c, (_, bal, _x) in enumerate(inputs):
            if bal != 0.0:
                g.setGainBalance(bal, ch=c)
        if blockwise:
            parts = [g.update(x[:, b:b + 1]) for b in range(x.shape[1])]
            I, Q = np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)
        else:
            I, Q = g.update(x)
        for c, (label, _, _x) in enumerate(inputs):
            rI, rQ = ref["out"][("iqgen", label)]
            assert np.array_equal(I[c], rI) and np.array_equal(Q[c], rQ), (label, blockwise)
        g.close()


def test_grabber(ref, dev):
    gI, gQ = ref["grab"]
    n = len(R.GRAB_AFTER)
    g = dev.AudioGrabberComplex256Batch(n)
    I, Q = np.ascontiguousarray(np.tile(gI, (n, 1, 1))), np.ascontiguousarray(np.tile(gQ, (n, 1, 1)))
    for b in range(I.shape[1]):
        g.update(I[:, b:b + 1], Q[:, b:b + 1])
        for c, after in enumerate(R.GRAB_AFTER):
            if after == b:
                buf, new, new_after = ref["out"][("grab", after)]
                assert g.newDataAvailable(c) == new, after
                _, got = g.grab(c, np.zeros(512, np.int16))
                assert np.array_equal(got, buf), after
                assert g.newDataAvailable(c) == new_after, after
    g.close()


def test_pre_fixed_corrections_and_swap(ref, dev):
    gI, gQ = ref["grab"]
    n = len(R.PRE_FIXED)
    p = dev.AudioSDRpreProcessorBatch(n)
    p.stopAutoI2SerrorDetection()
    for c, (corr, swap) in enumerate(R.PRE_FIXED):
        p.setI2SerrorCompensation(corr, ch=c); p.swapIQ(swap, ch=c)
    I, Q = p.update(np.tile(gI, (n, 1, 1)), np.tile(gQ, (n, 1, 1)))
    for c, (corr, swap) in enumerate(R.PRE_FIXED):
        rI, rQ, r_corr, r_status = ref["out"][("pre", corr, swap)]
        assert np.array_equal(I[c], rI) and np.array_equal(Q[c], rQ), (corr, swap)
        assert (p.getI2SerrorCompensation(c), p.getAutoI2SerrorDetectionStatus(c)) == (r_corr, r_status), (corr, swap)
    p.close()


def test_detector_scenarios(ref, dev):
    """Every detector scenario as a channel of one batch, one update() per block, each channel's setters between the calls."""
    scen = ref["scen"]
    n, nb = len(scen), R.N_DET
    I, Q = np.ascontiguousarray(np.stack([sc["I"] for sc in scen])), np.ascontiguousarray(np.stack([sc["Q"] for sc in scen]))
    by = [R.setters_by_block(R.pre_script(sc), nb) for sc in scen]
    p = dev.AudioSDRpreProcessorBatch(n)
    got_i, got_q = np.empty_like(I), np.empty_like(Q)
    corr, status = np.empty((n, nb), int), np.empty((n, nb), int)
    for b in range(nb):
        for c in range(n):
            _apply(p, c, by[c].get(b, []))
        oi, oq = p.update(I[:, b:b + 1], Q[:, b:b + 1])
        got_i[:, b], got_q[:, b] = oi[:, 0], oq[:, 0]
        for c in range(n):
            corr[c, b], status[c, b] = p.getI2SerrorCompensation(c), p.getAutoI2SerrorDetectionStatus(c)
    for c, sc in enumerate(scen):
        rI, rQ, r_corr, r_status = ref["out"][("det", sc["name"])]
        for what, g, w in (("I", got_i[c], rI), ("Q", got_q[c], rQ), ("getI2SerrorCompensation", corr[c], r_corr),
                           ("getAutoI2SerrorDetectionStatus", status[c], r_status)):
            bad = np.nonzero((g != w).reshape(nb, -1).any(axis=1))[0]
            assert bad.size == 0, "%s: %s differs from the reference from block %d on (%d blocks)" % (sc["name"], what, bad[0], bad.size)
    p.close()
