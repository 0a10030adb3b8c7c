"""The CPU oracle against the REFERENCE'S OWN CODE: oracle/_ref/ (oracle/ref_build.py) is the reference's AudioSDR.cpp,
AudioIQgenerator.cpp, AudioGrabberComplex256.cpp and AudioSDRpreProcessor.cpp compiled on the stand-in Teensy / CMSIS headers of
oracle/ref_shim/ (the stand-in FFT is pinned by tests/test_ref_shim_cmsis.py).  One reference process per channel, 8 at a time.

Checked bit for bit: every tests/cases.py case and channel (int16 audio of every block, 27 getters, 129 AGC table entries); fuzz seeds
1-24 (6 channels x 24 blocks each, setters between blocks); 728-block runs in which every AGC mode's hang time runs out; the IQ generator, the grabber, the pre-processor's fixed corrections and swap;
and the pre-processor's image detector in every scenario of tests/ref_scenarios.py, block by block with both getters.  The only
differences allowed are the two documented ones (tests/ref_scenarios.py: the excluded case, and samples beyond int32 that the reference's
x86 build turns into 0)."""
import numpy as np
import pytest

import ref_scenarios as R
from oracle import ref_build


@pytest.fixture(scope="module")
def ref():
    """Every reference process of this file, run before any comparison."""
    R.require_binaries()
    cases, fuzz, agc = R.case_channels(), R.fuzz_channels(), R.long_agc_channels()
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


def _oracle_sdr(ao, script, I, Q):
    """The oracle through a script, block by block: (int16 [blocks][128], difference 2's mask from its ALS tap, the instance)."""
    nb = I.shape[0]
    o = ao.OracleSDR(taps=True, pll_wrap_bound=False)
    by, og = R.setters_by_block(script, nb), R.output_gains(script, nb)
    want, oob = np.empty((nb, 128), np.int16), np.empty((nb, 128), bool)
    for b in range(nb):
        for m, a in by.get(b, []):
            getattr(o, m)(*a)
        want[b] = o.update(I[b], Q[b])
        oob[b] = R.beyond_int32(o.tap("ALS"), og[b])
    for m, a in by.get(nb, []):
        getattr(o, m)(*a)
    return want, oob, o


def _check_channels(ref, ao, channels):
    n_oob = 0
    for ch in channels:
        audio, g = ref["out"][("sdr", ch["label"])]
        want, oob, o = _oracle_sdr(ao, ch["script"], ch["I"], ch["Q"])
        n_oob += R.check_audio(want, audio, oob, ch["label"])
        R.check_getters(lambda k, *a: getattr(o, k)(*a), g, ch["label"])
    return n_oob


def test_exclusions_are_exactly_the_documented_one():
    assert R.EXCLUDED_CASES == ("usb_als_m_plus_delay_over_128",)
    assert set(R.CASE_NAMES) | set(R.EXCLUDED_CASES) == set(__import__("cases").CASES)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_case(ref, ao, name):
    chans = [ch for ch in ref["cases"] if ch["label"].rsplit(" ch ", 1)[0] == name]
    assert chans
    _check_channels(ref, ao, chans)


def test_fuzz_seeds(ref, ao):
    assert len(ref["fuzz"]) == 6 * len(R.FUZZ_SEEDS)
    n_oob = _check_channels(ref, ao, ref["fuzz"])
    assert n_oob > 0          # the fuzz does reach difference 2 (adaptive ALS diverging with the AGC off): the mask is exercised


def test_long_agc_mode_runs(ref, ao):
    """The AGC modes' hang times run out (hundreds of blocks): audio, getters and table against the reference."""
    _check_channels(ref, ao, ref["agc"])


def test_iq_generator(ref, ao):
    for label, bal, x in R.iqgen_inputs():
        rI, rQ = ref["out"][("iqgen", label)]
        g = ao.OracleIQgenerator()
        if bal != 0.0:
            g.setGainBalance(bal)
        I, Q = g.update(x)
        assert np.array_equal(I.reshape(-1, 128), rI) and np.array_equal(Q.reshape(-1, 128), rQ), label


def test_grabber(ref, ao):
    gI, gQ = ref["grab"]
    for after in R.GRAB_AFTER:
        buf, new, new_after = ref["out"][("grab", after)]
        g = ao.OracleGrabber()
        g.update(gI[:after + 1], gQ[:after + 1])
        assert g.newDataAvailable() == new, after
        assert np.array_equal(g.grab(), buf), after
        assert g.newDataAvailable() == new_after, after


def test_pre_fixed_corrections_and_swap(ref, ao):
    gI, gQ = ref["grab"]
    for corr, swap in R.PRE_FIXED:
        rI, rQ, r_corr, r_status = ref["out"][("pre", corr, swap)]
        o = ao.OraclePreProcessor()
        o.stopAutoI2SerrorDetection(); o.setI2SerrorCompensation(corr); o.swapIQ(swap)
        I, Q = o.update(gI, gQ)
        assert np.array_equal(I.reshape(-1, 128), rI) and np.array_equal(Q.reshape(-1, 128), rQ), (corr, swap)
        assert (o.getI2SerrorCompensation(), o.getAutoI2SerrorDetectionStatus()) == (r_corr, r_status), (corr, swap)


def oracle_detector(ao, sc):
    """The oracle through a detector scenario, block by block: (I, Q [blocks][128], both getters, max_line and whether the two TIE lines
    have bit-equal powers, after every block)."""
    nb = sc["I"].shape[0]
    o = ao.OraclePreProcessor()
    by = R.setters_by_block(R.pre_script(sc), nb)
    I, Q = np.empty((nb, 128), np.int16), np.empty((nb, 128), np.int16)
    corr, status, line, tie = np.empty(nb, int), np.empty(nb, int), np.empty(nb, int), np.empty(nb, bool)
    for b in range(nb):
        for m, a in by.get(b, []):
            getattr(o, m)(*a)
        I[b], Q[b] = o.update(sc["I"][b], sc["Q"][b])
        corr[b], status[b], line[b] = o.getI2SerrorCompensation(), o.getAutoI2SerrorDetectionStatus(), o.state()["max_line"]
        p = o.power_spectrum().view(np.uint32)
        tie[b] = p[R.TIE[0]] == p[R.TIE[1]] and p[R.TIE[0]] == p[5:123].max()
    return I, Q, corr, status, line, tie


@pytest.mark.parametrize("k", range(len(R.detector_scenarios())), ids=[sc["name"] for sc in R.detector_scenarios()])
def test_detector(ref, ao, k):
    sc = ref["scen"][k]
    rI, rQ, r_corr, r_status = ref["out"][("det", sc["name"])]
    I, Q, corr, status, line, tie = oracle_detector(ao, sc)
    for what, got, want in (("I", I, rI), ("Q", Q, rQ), ("getI2SerrorCompensation", corr, r_corr),
                            ("getAutoI2SerrorDetectionStatus", status, r_status)):
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %s differs from the reference from block %d on (%d blocks)" % (sc["name"], what, bad[0], bad.size)
    # ... and the scenario does what its name says (on the reference's own answers)
    name = sc["name"]
    if name.startswith("clean tone"):
        off = int(np.argmin(r_status))
        assert r_status[0] == 1 and r_status[-1] == 0 and (r_corr == 0).all() and 1000 <= off < R.N_DET, off
    if name.startswith("Q one sample late"):
        assert r_corr[-1] == 1 and r_status[-1] == 0
    if name.startswith("I one sample late"):
        assert r_corr[-1] == -1 and r_status[-1] == 0
    if name.startswith("silence"):
        assert (line == 0).all() and (r_corr == 0).all() and (r_status == 1).all()
    if name == R.TIE_NAME:           # the tie holds in every block the detector ran, and the first line won it
        active = np.concatenate([[True], r_status[:-1] == 1])
        assert tie[active].all() and (line[active] == R.TIE[0]).all() and 1000 <= active.sum() < R.N_DET
        assert (r_corr == 0).all() and r_status[-1] == 0
    if name.startswith("real tone"):
        assert set(r_corr.tolist()) == {-1, 0, 1} and (r_status == 1).all()
    if name.startswith("fixed +1"):
        assert (r_status[:5] == 0).all() and (r_corr[:5] == 1).all() and r_status[400] == 1 and r_status[1050] == 1
