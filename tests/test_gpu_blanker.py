"""The impulse noise blanker of every launch form that contains it, on the designed inputs of tests/blanker_scenarios.py, against the oracle
at tolerance 0: the int16 audio of every channel and block and nb_detected after every call; on the plain one-block form also the NB_I /
NB_Q taps as bit patterns on sampled channels (taps switch the lanes and the pipeline off: only there).  tests/test_blanker_scenarios.py
shows without a GPU which seam of the blanker each recipe reaches -- every impulse position and ring phase, merging and touching windows,
runs with 128 detections and more, level steps, dense noise, impulses at the threshold, one disturbed lane per wave, setters arriving on
a carried mask -- and that the recipes tell wrong blankers apart.

EVERY case asserts the launch census call by call (binding.kernels_launched): the recipe ran in the kernel the form names.

    form        bank                            kernel(s)
    one         U channels, one block per call  asdr_update_kernel_one
    loop        U, calls of 2, 3 and 5 blocks   asdr_update_kernel (the in-kernel block loop)
    mw_u        512, broadcast settings         asdr_update_kernel_mw_u
    mw          512, thresholds that alternate  asdr_update_kernel_mw
                from one tile of U channels to
                the next, one output gain
    pipe-*      U, USB / AM, calls of 8 to 12   asdr_stream_kernel (one FIR helper wave) / asdr_stream_kernel_h3 (three)
    sam3        U, SAM, three launches          asdr_sam_pre_kernel_uniform (the blanker) | asdr_sam_pll_kernel | asdr_sam_post_kernel_uniform
    sam-fused   U, SAM                          asdr_update_kernel_sam
    als         U, USB + the ALS filter         asdr_update_kernel_als_small_one
    mixed       U + 5, USB / LSB / AM by        asdr_update_kernel_mixed (every mode's remainder) beside the whole waves'
                channel                         asdr_update_kernel_one (the 16-row recipes have no whole wave of one mode)

(U is rounded up to whole waves; channel c takes row c % U.)  positions, pairs and dense go through every form, the other recipes through
one (with and without taps), mw_u, mw and the pipeline."""
import numpy as np
import pytest

import blanker_scenarios as B
import four_wave_scenarios as F
from cases import USB, LSB, AM, SAM
from helpers import S, Hip, f32_bits

pytestmark = pytest.mark.gpu

ONE, LOOP, MIXED = "asdr_update_kernel_one", "asdr_update_kernel", "asdr_update_kernel_mixed"
STREAM, STREAM_H3 = "asdr_stream_kernel", "asdr_stream_kernel_h3"
# what a pipeline call launches around the pipeline itself: the snapshot in front, and behind it the launches that act only if a wait ran out
STREAM_AROUND = {"asdr_stream_snapshot_kernel", "asdr_stream_restore_kernel", "asdr_stream_ack_kernel", LOOP}
SAM_FUSED, ALS_ONE = "asdr_update_kernel_sam", "asdr_update_kernel_als_small_one"
C2 = [S("setDemodMode", USB), S("enableAudioFilter")]
TAP_EVERY = 5                                     # taps on channels 0, 5, 10, ...: every row of a wave over the bank


def _whole_waves(n):
    return (n + 7) // 8 * 8


class Form:
    def __init__(self, name, front=C2, n=None, behind=(), plan="one", kernels=None, prepare=None, pipe=None, taps=False, mode=USB):
        self.name, self.front, self.n, self.behind, self.plan, self.kernels = name, list(front), n, behind, plan, kernels
        self.prepare, self.pipe, self.taps, self.mode = prepare, pipe, taps, mode

    def bank(self, recipe):
        return self.n(recipe.U) if callable(self.n) else (_whole_waves(recipe.U) if self.n is None else self.n)

    def calls(self, recipe):
        """block counts of the calls; every block of the recipe's script starts one"""
        T, cuts = recipe.T, sorted(recipe.script)
        if self.plan == "one":
            return [1] * T
        if self.plan == "pipe":
            out = [1, 1, 1, 9, 12] if T == B.T_STD else [9, 8, 8, 8]
            assert sum(out) == T and all(c in np.cumsum(out) for c in cuts)
            return out
        out, pos, k = [], 0, 0
        while pos < T:                            # loop: 2, 3, 5, 2, ... cut short in front of a setter and at the end
            nxt = min([c for c in cuts if c > pos] + [T])
            out.append(min((2, 3, 5)[k % 3], nxt - pos)); pos += out[-1]; k += 1
        return out

    def census(self, k, n):
        """the launches of a call of k blocks on a bank of n channels (None: the pipeline's, checked by _check_pipeline)"""
        if self.kernels is not None:
            kernels = self.kernels(n) if callable(self.kernels) else self.kernels
            return {name: v * k for name, v in kernels.items()}
        if self.plan == "pipe" and k >= 8:
            return None
        return {ONE: 1} if k == 1 else {LOOP: 1}


def _mw_behind(U):
    """thresholds that differ from one tile of U channels to the next (tile 0 keeps the recipe's own), one channel's output gain"""
    return [S("setNoiseBlankerThreshold", 1.5, sel=lambda c: (c // U) % 2 == 1), S("setOutputGain", 0.7, sel=F.MID)]


def _sam(fused):
    return lambda b: b.set_sam_launch_form(fused, 8)


def _mixed_kernels(n):
    """three modes by channel: the whole waves of each mode (if it has any) in one launch, every mode's remainder in the general kernel's"""
    whole = sum(len(range(j, n, 3)) // 8 for j in range(3))
    return {ONE: 1, MIXED: 1} if whole else {MIXED: 1}


_AMF = [S("setDemodMode", AM), S("enableAudioFilter")]
_SAMF = [S("setDemodMode", SAM), S("enableAudioFilter")]
_BY_CHANNEL = [S("setDemodMode", USB, sel=lambda c: c % 3 == 0), S("setDemodMode", LSB, sel=lambda c: c % 3 == 1),
               S("setDemodMode", AM, sel=lambda c: c % 3 == 2), S("enableAudioFilter")]
FORMS = {f.name: f for f in (
    Form("one"), Form("one-taps", taps=True), Form("loop", plan="loop"),
    Form("mw_u", n=F.N, kernels={F.MW_U: 1}), Form("mw", n=F.N, behind=_mw_behind, kernels={F.MW: 1}),
    Form("pipe-usb-h1", plan="pipe", pipe=0), Form("pipe-usb-h3", plan="pipe", pipe=1),
    Form("pipe-am-h1", front=_AMF, plan="pipe", pipe=0, mode=AM), Form("pipe-am-h3", front=_AMF, plan="pipe", pipe=1, mode=AM),
    Form("sam3", front=_SAMF, prepare=_sam(False), kernels={k: 1 for k in F.SAM_KERNELS}, mode=SAM),
    Form("sam-fused", front=_SAMF, prepare=_sam(True), kernels={SAM_FUSED: 1}, mode=SAM),
    Form("als", front=C2 + [S("enableALSfilter")], kernels={ALS_ONE: 1}),
    Form("mixed", front=_BY_CHANNEL, n=lambda U: _whole_waves(U) + 5, kernels=_mixed_kernels))}
EVERY = list(FORMS)
SOME = ["one", "one-taps", "mw_u", "mw", "pipe-usb-h3"]


class _Oracles(F.OracleRun):
    def __init__(self, ao, sc, bI, bQ, taps_for):
        self.nb = np.zeros((sc.n, 0), np.int64)
        self._nb = {}
        super().__init__(ao, sc, bI, bQ, taps_for=taps_for)
        T = bI.shape[1]
        per_key = np.array([[self._nb[(i, t)] for t in range(T)] for i in range(len(self.index))])
        self.nb = per_key[self.of_channel]                                   # [n][T]

    def after_block(self, i, blk, o):
        self._nb[(i, blk)] = o.NoiseBlankerDetection()


_ORACLES = {}


def _case(ao, recipe, form):
    """(scenario, oracles): one oracle run per (recipe, settings, bank), shared by the forms that differ in the launch only"""
    n = form.bank(recipe)
    behind = form.behind(recipe.U) if callable(form.behind) else list(form.behind)
    key = (recipe.name, form.mode, n, bool(behind), form.taps, form.name if form.front not in (C2, _AMF, _SAMF) else "")
    if key not in _ORACLES:
        sc = B.scenario(recipe, n=n, front=form.front, behind=behind)
        bI, bQ = recipe.rows()
        taps_for = list(range(0, n, TAP_EVERY)) if form.taps else None
        run = _Oracles(ao, sc, bI, bQ, taps_for)
        run.audio.setflags(write=False)
        _ORACLES[key] = (sc, run)
    return _ORACLES[key]


def _tile(a, n):
    return np.ascontiguousarray(np.tile(a, ((n + a.shape[0] - 1) // a.shape[0], 1, 1))[:n])


def _check_pipeline(got, form, b, launches):
    kernel = STREAM_H3 if form.pipe == 1 else STREAM
    assert got.get(kernel) == 1 and set(got) <= STREAM_AROUND | {kernel}, got
    assert b.stream_pipeline_launches() == launches and b.stream_pipeline_recoveries() == 0


def _run(gpu, ao, recipe, form):
    sc, run = _case(ao, recipe, form)
    bI, bQ = recipe.rows()
    n, T = sc.n, recipe.T
    hip = Hip()
    b = gpu.AudioSDRBatch(n)
    try:
        dI, dQ, dO = hip.upload(_tile(bI, n)), hip.upload(_tile(bQ, n)), hip.malloc(n * T * 256)
        if form.prepare:
            form.prepare(b)
        if form.pipe is not None:
            b.set_stream_fir_helpers(form.pipe)
        if form.taps:
            b.enable_taps(True)
        F.apply_to_batch(b, sc.setup, n)
        gpu.binding.kernels_launched(reset=True)
        pos = pipelined = 0
        for k in form.calls(recipe):
            if pos in sc.script:
                F.apply_to_batch(b, sc.script[pos], n)
            b.update_device_strided(dI + pos * 256, dQ + pos * 256, dO + pos * 256, k, T, T, 0)
            b.synchronize()
            pos += k
            got = {name: v for name, v in gpu.binding.kernels_launched(reset=True).items() if name != "asdr_reset_kernel"}
            want = form.census(k, n)
            if want is None:
                pipelined += 1
                _check_pipeline(got, form, b, pipelined)
            else:
                assert got == want, "call of %d blocks ending at %d: launched %s, expected %s" % (k, pos, got, want)
            nb = b.read_status()["nb_detected"]
            bad = np.flatnonzero(nb != run.nb[:, pos - 1])
            assert bad.size == 0, "nb_detected after block %d: %d channels differ, first %d" % (pos - 1, bad.size, bad[0])
            if form.taps:
                taps = b.read_taps()
                for c in range(0, n, TAP_EVERY):
                    ref = run.taps[run.of_channel[c]][pos - 1]
                    for name in ("NB_I", "NB_Q"):
                        assert np.array_equal(f32_bits(taps[name][c]), f32_bits(ref[gpu.TAPS.index(name)])), "block %d channel %d tap %s" % (pos - 1, c, name)
        if form.plan == "pipe":
            assert pipelined == sum(1 for k in form.calls(recipe) if k >= 8) >= 2
        got = hip.download(dO, (n, T, 128), np.int16)
        bad = np.argwhere(got != run.want())
        assert bad.size == 0, "%d samples differ, first at (channel, block, sample) %s" % (len(bad), bad[0].tolist())
    finally:
        hip.free_all(); b.close()


def _ids(forms):
    return dict(argvalues=forms, ids=forms)


@pytest.mark.parametrize("form", **_ids(EVERY))
def test_every_impulse_position(gpu, ao, form):
    """One strong impulse at sample p of three blocks (ring phases 0, 1, 2) in row p: a trailing edge at every i = 128..255, found a call
    later from the carried codes for p >= 117, the ramp's head in the block being output, the window spilling into the newest block."""
    _run(gpu, ao, B.POSITIONS, FORMS[form])


@pytest.mark.parametrize("form", **_ids(EVERY))
def test_pairs_of_impulses(gpu, ao, form):
    """Windows that merge, touch, leave a gap of 1, 7 and 8 samples; pairs across the re-scan's start at 78 and across the block's end."""
    _run(gpu, ao, B.PAIRS, FORMS[form])


@pytest.mark.parametrize("form", **_ids(EVERY))
@pytest.mark.parametrize("recipe", B.DENSE, ids=lambda r: r.name)
def test_dense_noise(gpu, ao, recipe, form):
    """Heavy-tailed noise at ratio 1.2 and 2.0: detections in every block, a scan in which every sample is one, never a trivial carried mask."""
    _run(gpu, ao, recipe, FORMS[form])


@pytest.mark.parametrize("form", **_ids(["one", "one-taps", "loop", "mw_u", "mw", "pipe-usb-h1", "pipe-usb-h3", "pipe-am-h3"]))
def test_runs_and_level_steps(gpu, ao, form):
    """2 to 300 strong samples in a row from three starts -- output blocks that are zero throughout, scans of 178 detections, count bytes
    with the top bit set --, a level step up, one down, and a step onto a raised average (detections behind the 127th that only the first
    scan makes)."""
    _run(gpu, ao, B.RUNS_RECIPE, FORMS[form])


@pytest.mark.parametrize("form", **_ids(SOME))
@pytest.mark.parametrize("recipe", B.MARGINALS, ids=lambda r: r.name)
def test_impulses_at_the_threshold(gpu, ao, recipe, form):
    """Isolated impulses within a few per cent of threshold x average, five thresholds through both setters; samples at 78..127 that one
    of their two scans detects and the other does not, both ways."""
    _run(gpu, ao, recipe, FORMS[form])


@pytest.mark.parametrize("recipe,form", [(r, f) for r, fs in zip(B.ONE_IN_A_WAVE, (SOME, ["one", "one-taps", "mw", "pipe-usb-h3"], ["one", "one-taps", "mixed"])) for f in fs],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_one_disturbed_channel_in_a_wave(gpu, ao, recipe, form):
    """Rows 0, 9, 18, ... carry the impulses: wave k leaves the quiet path for lane k alone; by broadcast, with two thresholds that
    alternate by channel, and with the blanker off on one more channel in eight (whose channels the schedule gathers in waves of their own)."""
    _run(gpu, ao, recipe, FORMS[form])


@pytest.mark.parametrize("form", **_ids(SOME))
@pytest.mark.parametrize("kind", list(B.SETTER_KINDS))
def test_setter_on_a_carried_mask(gpu, ao, kind, form):
    """setNoiseBlankerThreshold, setNoiseBlankerThresholdDb, disableNoiseBlanker + enableNoiseBlanker and setDemodMode away and back in
    front of blocks at all three ring phases, on dense rows and on rows whose run of strong samples is in the carried mask just then."""
    f = FORMS[form]
    _run(gpu, ao, B.setter_recipe(kind, pipe=f.plan == "pipe", mode=f.mode), f)
