"""The monitors of a fast-convolution bank on the GPU (include/asdr_tuner.h, "Monitors"; asdr_tuner_monitor.hip) against the
float64 restatement tests/tuner_monitor_ref.py.

Spectrum: compared in the amplitude domain, A = sqrt(acc / frames) (sum) or sqrt(acc) (peak), |A_gpu - A_ref| <= EPS_A for every
bin.  A float32 FFT's error is roughly uniform over the bins, so a bound relative to each bin's power would be loose on the strong
bins and unreachable on the weak ones.  EPS_A[recipe, R] is 8 x the largest amplitude difference that a complex64 model of the
statement (scipy.fft in complex64 -- for RS16 tuner_formats_ref.HalfSizeFFT -- then the three-bin combine, |W|^2 / N^2 and the
group sums in float32; frames accumulated in float64) shows against float64 on the test's own inputs, over all of the recipe's
(B, window, mode): the rule and the factor of EPS in test_gpu_tuner_fastconv.py.  Produced by
    python tests/test_gpu_tuner_monitor.py
Levels: rms = sqrt(level / (128 frames)) against the restatement's within the EPS table of test_gpu_tuner_fastconv.py for the same
recipe: every |z| is within EPS / 8 of float64 there, and an rms moves by no more than its largest term's error."""
import numpy as np
import pytest

import test_gpu_tuner_fastconv as T
import tuner_condition_ref as CR
import tuner_fastconv_ref as F
import tuner_formats_ref as FM
import tuner_monitor_ref as M
from helpers import Hip

pytestmark = pytest.mark.gpu

SPEC_R = {"cs16": [2, 16, 32, 128, 1024], "cu8": [16], "cf32": [16], "rs16": [16, 32]}   # rs16 at R = 32: the four-step half-size path
CALLS = [1, 3, 2]                                             # frames per call: unequal, 6 in all
N_SRC = 3


def configs(R):
    N = 256 * R
    return [(B, w, m) for B in sorted({N, min(N, 4096), 256}) for w in M.WINDOWS for m in M.MODES]


def spec_inputs(fmt, R):
    """Per call (stored rows of the format, their converted CS16 pairs): the cs16 helper's noise in +-20000 plus, per source, a
    tone of 6000 at a random frequency; source 0 also a tone of 5000 a quarter bin below 0 (between bin N - 1 and bin 0, so both
    Hann neighbours of the seam carry it), source 1 one on the centre of bin N - 1."""
    fs = 44100 * R
    H, N, _ = F.sizes(R)
    rng = np.random.default_rng(7000 + R + 13 * sorted(SPEC_R).index(fmt))
    tones = [(s, float(rng.uniform(-fs / 2, fs / 2)), 6000.0) for s in range(N_SRC)] + [(0, -0.25 * fs / N, 5000.0), (1, -1.0 * fs / N, 4000.0)]
    iq = T.cs16(rng, N_SRC, sum(CALLS) * H, tones, fs)
    raw = FM.from_cs16(iq, fmt)
    out, at = [], 0
    for nf in CALLS:
        r = np.ascontiguousarray(raw[:, at:at + nf * H])
        out.append((r, FM.to_cs16(r, fmt)))
        at += nf * H
    return out


def reference(calls, n_src, R, cfgs, real=False, place=None, skip_frames=0):
    """calls: converted rows per call.  {cfg: (acc float64, frames)} of the restatement, and the largest amplitude difference of the
    complex64 model against it over cfgs.  place = (P, hist): start there; skip_frames: frames seen before the monitor is on."""
    import scipy.fft
    mon = M.MonitorRef(F.TunerFastconvRef(1, n_src, 44100 * R, R))
    if place:
        mon.place_at(*place)
    acc = {c: [np.zeros((n_src, c[0])), np.zeros((n_src, c[0])), 0] for c in cfgs}
    seen = 0
    for rows in calls:
        for win in mon.windows(rows):
            seen += 1
            if seen <= skip_frames:
                continue
            X = np.fft.fft(win, axis=1)
            X32 = FM.HalfSizeFFT.fft(win.astype(np.complex64)) if real else scipy.fft.fft(win.astype(np.complex64), axis=1)
            assert X32.dtype == np.complex64
            for c, a in acc.items():
                P, P32 = M.powers(X, c[0], c[1]), M.powers(X32, c[0], c[1], f32=True)
                a[0] = a[0] + P if c[2] == "sum" else np.maximum(a[0], P)
                a[1] = a[1] + P32 if c[2] == "sum" else np.maximum(a[1], P32)
                a[2] += 1
    worst = max(float(np.abs(M.amplitude(a[0], a[2], c[2]) - M.amplitude(a[1], a[2], c[2])).max()) for c, a in acc.items())
    peak = max(float(M.amplitude(a[0], a[2], c[2]).max()) for c, a in acc.items())
    return {c: (a[0], a[2]) for c, a in acc.items()}, worst, peak


FULL = dict(fs=2400000, R=16, n_ch=65536, n_src=16, nf=16, calls=3, cfg=(4096, "hann", "sum"))
MID_SKIP = 5                                                  # test_monitors_enabled_mid_stream: frames before the monitor is on


def full_inputs():
    rng = np.random.default_rng(65537)
    srcs = (np.arange(FULL["n_ch"]) * 7) % FULL["n_src"]
    fws = rng.integers(0, 2 ** 32, size=FULL["n_ch"], dtype=np.uint64)
    sample = sorted(set([0, 1, FULL["n_ch"] - 1] + [int(c) for c in rng.integers(0, FULL["n_ch"], size=61)]))
    iqs = [T.cs16(rng, FULL["n_src"], FULL["nf"] * 128 * FULL["R"]) for _ in range(FULL["calls"])]
    return srcs, fws, sample, iqs


def wrap_inputs():
    """T.wrap_case's events after the feeding: (set-up fn, fed rows, (P0, hist), the remaining events as a list)."""
    ev = iter(T.wrap_case().events)
    fn, fed, place = next(ev)[1], next(ev)[1], next(ev)[1:]
    return fn, fed, place, list(ev)


WRAP_CFG = (4096, "hann", "sum")


def measure(recipe, R):
    if recipe == "full":
        return reference(full_inputs()[3], FULL["n_src"], R, [FULL["cfg"]])[1:]
    if recipe == "wrap":
        _, _, place, rest = wrap_inputs()
        return reference([e[1] for e in rest if e[0] == "iq"], 1, R, [WRAP_CFG], place=place)[1:]
    if recipe == "mid":
        return reference([c for _, c in spec_inputs("cs16", R)], N_SRC, R, [(256, "hann", "sum"), (256 * R, "rect", "peak")], skip_frames=MID_SKIP)[1:]
    return reference([c for _, c in spec_inputs(recipe, R)], N_SRC, R, configs(R), real=recipe == "rs16")[1:]


MEASURED = dict(SPEC_R, full=[16], wrap=[1024], mid=[16])

# EPS_A[recipe, R] = 8 x measure(recipe, R)[0] to three digits (amplitude, int16 units).
EPS_A = {
    ("cs16", 2): 0.00427,   # measured 0.000534 at peak amplitude 6645
    ("cs16", 16): 0.00277,   # measured 0.000346 at peak amplitude 6614
    ("cs16", 32): 0.00613,   # measured 0.000766 at peak amplitude 6242
    ("cs16", 128): 0.00873,   # measured 0.00109 at peak amplitude 6122
    ("cs16", 1024): 0.00452,   # measured 0.000565 at peak amplitude 6104
    ("cu8", 16): 0.00383,   # measured 0.000479 at peak amplitude 6205
    ("cf32", 16): 0.00634,   # measured 0.000793 at peak amplitude 6260
    ("rs16", 16): 0.00176,   # measured 0.00022 at peak amplitude 4505
    ("rs16", 32): 0.002,   # measured 0.000249 at peak amplitude 4499
    ("full", 16): 0.000127,   # measured 1.59e-05 at peak amplitude 207
    ("wrap", 1024): 0.000113,   # measured 1.41e-05 at peak amplitude 178
    ("mid", 16): 0.00289,   # measured 0.000362 at peak amplitude 5887
}


def check_spectrum(got, frames, want, eps, cfg, what=""):
    acc, n = want
    assert frames == n, (what, cfg, frames, n)
    d = np.abs(M.amplitude(got, frames, cfg[2]) - M.amplitude(acc, n, cfg[2]))
    print(what, cfg, "max |A_gpu - A_ref| = %.3g (bound %.3g) at peak amplitude %.0f" % (d.max(), eps, M.amplitude(acc, n, cfg[2]).max()))
    assert d.max() <= eps, (what, cfg, float(d.max()), eps, np.argwhere(d == d.max())[0])


@pytest.mark.parametrize("fmt,R", [(f, R) for f in sorted(SPEC_R) for R in SPEC_R[f]])
def test_spectrum_matches_the_restatement(gpu, fmt, R):
    """Every (B, window, mode) of the recipe on one bank: three calls of unequal frame counts, read without and with clear, then
    reset() (which clears and keeps B) and the same frames in one call."""
    calls = spec_inputs(fmt, R)
    cfgs = configs(R)
    want, _, _ = reference([c for _, c in calls], N_SRC, R, cfgs, real=fmt == "rs16")
    eps = EPS_A[fmt, R]
    bank = gpu.TunerBank.fastconv(1, N_SRC, 44100 * R, R)
    bank.set_input_format(fmt)
    whole = np.ascontiguousarray(np.concatenate([r for r, _ in calls], axis=1))
    for cfg in cfgs:
        bank.reset()
        bank.enable_spectrum(*cfg)
        assert bank.spectrum_config() == cfg
        for r, _ in calls:
            bank.update_samples(r)
        got, frames = bank.spectrum(clear=False)
        assert got.shape == (N_SRC, cfg[0]) and got.dtype == np.float64
        check_spectrum(got, frames, want[cfg], eps, cfg, "three calls")
        assert frames == sum(CALLS) == bank.spectrum_frames()
        again, frames2 = bank.spectrum(clear=True)
        assert np.array_equal(again, got) and frames2 == frames
        zero, frames3 = bank.spectrum()
        assert not zero.any() and frames3 == 0
        bank.update_samples(calls[0][0])                      # something to clear
        bank.reset()
        assert bank.spectrum_config() == cfg and bank.spectrum_frames() == 0 and not bank.spectrum(clear=False)[0].any()
        bank.update_samples(whole)
        got1, frames1 = bank.spectrum()
        check_spectrum(got1, frames1, want[cfg], eps, cfg, "one call")
    bank.close()


def test_spectrum_at_positions_past_2_to_the_32(gpu):
    """T.wrap_case (R = 1024): the bank is fed to P = 2^32 - 2 H with the monitors off, then both go on and see the frames across
    2^32 and the retunes beyond it.  The monitors have no position arithmetic of their own."""
    case = T.wrap_case()
    fn, fed, place, rest = wrap_inputs()
    bank, ref = T.pair(gpu, case)
    fn(bank); fn(ref)
    hip = Hip()
    s = hip.stream()
    nf = T.WRAP_FRAMES
    dIQ = hip.upload(fed)
    dI, dQ = hip.malloc(case.n_ch * nf * 256), hip.malloc(case.n_ch * nf * 256)
    for _ in range(511):
        bank.update_device(dIQ, dI, dQ, nf, stream=s)
    bank.update_device(dIQ, dI, dQ, nf - 2, out_stride_blocks=nf, stream=s)
    hip.sync(s)
    assert bank.position() == place[0]
    ref.place_at(*place)
    mon = M.MonitorRef(ref, *WRAP_CFG, levels=True)
    mon.place_at(*place)
    bank.enable_spectrum(*WRAP_CFG); bank.enable_levels()
    n = 0
    for ev in rest:
        if ev[0] == "set":
            ev[1](bank); ev[1](ref)
        elif ev[0] == "iq":
            I, Q = bank.update(ev[1])
            mon.update(ev[1])
            T.compare_u((I, Q), ref.update(ev[1], keep_float=True)[2], T.EPS["wrap", case.R], ev[2])
            n += ev[1].shape[1] // ref.H
    assert n == 6 and bank.position() == (1 << 32) + 4 * ref.H
    got, frames = bank.spectrum()
    check_spectrum(got, frames, (mon.acc, mon.frames), EPS_A["wrap", case.R], WRAP_CFG, "past 2^32")
    check_levels(bank, mon, T.EPS["wrap", case.R], "past 2^32")
    hip.free_all()
    bank.close()


class WithMonitor:
    """A reference and its monitors as one object for a case's "set" events: calls go to the reference; reset() to both."""

    def __init__(self, ref, mon):
        self._ref, self._mon = ref, mon

    def __getattr__(self, name):
        return getattr(self._ref, name)

    def reset(self):
        self._ref.reset(); self._mon.reset()


def check_levels(bank, mon, eps, what=""):
    lv, frames = bank.levels(clear=False)
    assert frames == mon.level_frames == bank.levels_frames(), (what, frames, mon.level_frames)
    rms = np.sqrt(lv / (128.0 * max(frames, 1)))
    d = np.abs(rms - mon.rms())
    print(what, "max |rms_gpu - rms_ref| = %.3g (bound %.3g) at peak rms %.0f" % (d.max(), eps, mon.rms().max()))
    assert d.max() <= eps, (what, float(d.max()), eps, int(np.argmax(d)))
    return lv


@pytest.mark.parametrize("recipe,R", [(r, R) for r in ("edge", "flat", "asym", "sat") for R in
                                      (T.CASE_R[r] if r in ("edge", "sat") else [2, 16, 128, 1024])])
def test_levels_match_the_restatement(gpu, recipe, R):
    """The recipes of test_gpu_tuner_fastconv.py with levels on: after every call the accumulated rms of every channel, retunes,
    filter changes and a reset (which clears) included; I and Q stay within compare_u's bound.  sat: the level is taken before
    the clamp, so the doubled filter's call reads above anything a clamped output could carry."""
    case = T.CASES[recipe](R)
    bank, ref = T.pair(gpu, case)
    mon = M.MonitorRef(ref, levels=True)
    both = WithMonitor(ref, mon)
    bank.enable_levels()
    eps = T.EPS[recipe, R]
    calls = 0
    for ev in case.events:
        if ev[0] == "set":
            ev[1](bank); ev[1](both)
        elif ev[0] == "iq":
            before = bank.levels(clear=False)[0]
            I, Q = bank.update(ev[1])
            mon.update(ev[1])
            z = ref.update(ev[1], keep_float=True)[2]
            T.compare_u((I, Q), z, eps, ev[2])
            lv = check_levels(bank, mon, eps, (recipe, ev[2]))
            calls += 1
            if recipe == "sat" and calls == 3:
                nf = ev[1].shape[1] // ref.H
                power = (lv - before) / (128.0 * nf)          # this call's mean |y|^2 per channel
                assert np.abs(I[0].astype(np.int64)).min() >= 32767 and np.abs(Q[0].astype(np.int64)).min() >= 32767   # channel 0 sits on the rails
                assert power[0] > 2 * 32768.0 ** 2, power[0]  # more than |(-32768, -32768)|^2, the most an int16 pair can carry
                assert abs(np.sqrt(power[0]) - 65536.0 * np.sqrt(2.0)) < 1.0
    assert calls >= 2
    lv, frames = bank.levels(clear=True)
    assert frames > 0 and lv.any()
    lv, frames = bank.levels()
    assert frames == 0 and not lv.any()
    bank.close()


def run_events(bank, events, out):
    for ev in events:
        if ev[0] == "set":
            ev[1](bank)
        elif ev[0] == "iq":
            out.append(bank.update(ev[1]))


@pytest.mark.parametrize("recipe,R", [("edge", 16), ("switch", 8)])
def test_outputs_are_bit_identical_with_the_monitors_on(gpu, recipe, R):
    """Two banks, one with both monitors on: every int16 of every call equal, over retunes, a reset and a filter change."""
    outs = []
    for on in (False, True):
        case = T.CASES[recipe](R)
        bank = gpu.TunerBank.fastconv(case.n_ch, case.n_src, case.fs, R)
        if on:
            bank.enable_spectrum(256 * R, "hann", "peak"); bank.enable_levels()
        o = []
        run_events(bank, case.events, o)
        bank.set_channel_filter(T.G_ASYM)
        bank.set_frequency(case.fs * 0.2, ch=1)
        o.append(bank.update(T.cs16(np.random.default_rng(5), case.n_src, 3 * 128 * R)))
        if on:
            assert bank.spectrum_frames() > 0 and bank.levels()[0].any()
        outs.append(o)
        bank.close()
    assert len(outs[0]) == len(outs[1]) >= 3
    for (I0, Q0), (I1, Q1) in zip(*outs):
        assert np.array_equal(I0, I1) and np.array_equal(Q0, Q1)


def test_outputs_are_bit_identical_behind_a_real_stage_2(gpu):
    fs, R, n_ch, n_src = 2400000, 16, 6, 2
    outs = []
    for on in (False, True):
        rng = np.random.default_rng(2400)
        bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
        T.setup(bank, [c % n_src for c in range(n_ch)], T.edge_words(R)[:n_ch])
        if on:
            bank.enable_spectrum(4096); bank.enable_levels()
        o = []
        for k, nf in enumerate([1, 4, 2, 7]):
            if k == 2:
                bank.set_frequency(-fs * 0.3, ch=1); bank.set_channel_filter(T.G_SHORT)
            o.append(bank.update_rate(T.cs16(rng, n_src, nf * 128 * R, [(0, fs * 0.01, 6000.0)], fs)))
        outs.append(o)
        bank.close()
    for (I0, Q0), (I1, Q1) in zip(*outs):
        assert I0.shape == I1.shape and np.array_equal(I0, I1) and np.array_equal(Q0, Q1)
    assert sum(I.shape[1] for I, _ in outs[0]) > 0


def test_monitors_enabled_mid_stream(gpu):
    """A monitor enabled after 5 frames accumulates frames 5 ...; disabled and enabled again it starts from zero.  Levels under the
    "edge" bound of this R: the same noise and tones of the same size through the same default filter."""
    R = 16
    calls = [c for _, c in spec_inputs("cs16", R)]            # 1 + 3 + 2 frames
    whole = np.concatenate(calls, axis=1)
    H = 128 * R
    cfgs = [(256, "hann", "sum"), (256 * R, "rect", "peak")]
    want, _, _ = reference(calls, N_SRC, R, cfgs, skip_frames=MID_SKIP)
    for cfg in cfgs:
        bank = gpu.TunerBank.fastconv(2, N_SRC, 44100 * R, R)
        ref = F.TunerFastconvRef(2, N_SRC, 44100 * R, R, g=bank.get_channel_filter())
        T.setup_pair(bank, ref, [0, 2], [0x12345678, 0x9E3779B9])
        mon = M.MonitorRef(ref)
        bank.update(whole[:, :MID_SKIP * H]); mon.update(whole[:, :MID_SKIP * H])
        bank.enable_spectrum(*cfg); bank.enable_levels(); mon.enable_levels()
        bank.update(whole[:, MID_SKIP * H:]); mon.update(whole[:, MID_SKIP * H:])
        got, frames = bank.spectrum(clear=False)
        assert frames == 1 == want[cfg][1]
        check_spectrum(got, frames, want[cfg], EPS_A["mid", R], cfg, "enabled after 5 frames")
        check_levels(bank, mon, T.EPS["edge", R], "enabled after 5 frames")
        bank.enable_spectrum(0); bank.enable_levels(False)
        bank.update(calls[0])
        bank.enable_spectrum(*cfg); bank.enable_levels()
        assert bank.spectrum_frames() == 0 and bank.levels_frames() == 0
        assert not bank.spectrum(clear=False)[0].any() and not bank.levels(clear=False)[0].any()
        bank.close()


def test_device_views_on_the_update_stream(gpu):
    """spectrum_tensor() / levels_tensor() copied on the update's stream, with no host synchronise in between, equal the reads."""
    import torch
    R, n_ch = 16, 8
    rng = np.random.default_rng(11)
    bank = gpu.TunerBank.fastconv(n_ch, 2, 44100 * R, R)
    T.setup(bank, [c % 2 for c in range(n_ch)], T.edge_words(R)[:n_ch])
    bank.enable_spectrum(1024, "hann", "sum"); bank.enable_levels()
    st, lt = bank.spectrum_tensor(), bank.levels_tensor()
    assert st.shape == (2, 1024) and lt.shape == (n_ch,) and st.dtype == lt.dtype == torch.float64 and st.is_cuda
    s = torch.cuda.Stream()
    nf = 4
    dIQ = torch.from_numpy(T.cs16(rng, 2, 2 * nf * 128 * R)).cuda()
    dI = torch.empty((n_ch, nf, 128), dtype=torch.int16, device="cuda")
    dQ = torch.empty_like(dI)
    torch.cuda.synchronize()
    snaps = []
    with torch.cuda.stream(s):
        for k in range(2):
            bank.update_device(dIQ[:, k * nf * 128 * R:].data_ptr(), dI.data_ptr(), dQ.data_ptr(), nf,
                               in_stride_samples=2 * nf * 128 * R, stream=s.cuda_stream)
            snaps.append((st.clone(), lt.clone()))
    s.synchronize()
    spec, frames = bank.spectrum(clear=False)
    lev, lframes = bank.levels(clear=False)
    assert frames == lframes == 2 * nf
    assert np.array_equal(snaps[1][0].cpu().numpy(), spec) and np.array_equal(snaps[1][1].cpu().numpy(), lev)
    assert (snaps[0][0].cpu().numpy() <= spec).all() and snaps[0][0].any().item() and (snaps[0][1].cpu().numpy() < lev).all()
    assert st.data_ptr() == bank.spectrum_tensor().data_ptr()
    bank.close()


def test_65536_channels_16_sources_with_both_monitors(gpu):
    """The geometry of test_65536_channels_16_sources_at_2_4_msps with both monitors on: 64 sampled channels' levels and all 16
    spectra.  Levels under the "edge" bound of this R: the same noise through the same default filter, without the tones."""
    fs, R, n_ch, n_src, nf = FULL["fs"], FULL["R"], FULL["n_ch"], FULL["n_src"], FULL["nf"]
    srcs, fws, sample, iqs = full_inputs()
    bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
    for c in range(n_ch):
        bank.set_source(int(srcs[c]), ch=c); bank.set_frequency_word(int(fws[c]), ch=c)
    ref = F.TunerFastconvRef(len(sample), n_src, fs, R, g=bank.get_channel_filter())
    for i, c in enumerate(sample):
        ref.src[i], ref.fw[i] = int(srcs[c]), int(fws[c])
    mon = M.MonitorRef(ref, *FULL["cfg"], levels=True)
    bank.enable_spectrum(*FULL["cfg"]); bank.enable_levels()
    hip = Hip()
    cap = nf + 1
    dI, dQ = hip.malloc(n_ch * cap * 256), hip.malloc(n_ch * cap * 256)
    s = hip.stream()
    for iq in iqs:
        bank.update_rate_device(hip.upload(iq), dI, dQ, nf, cap, stream=s)
        mon.update(iq)
    hip.sync(s)
    got, frames = bank.spectrum()
    check_spectrum(got, frames, (mon.acc, mon.frames), EPS_A["full", R], FULL["cfg"], "65536 channels")
    lv, lframes = bank.levels()
    assert lframes == mon.level_frames == nf * len(iqs) and lv.shape == (n_ch,)
    d = np.abs(np.sqrt(lv[sample] / (128.0 * lframes)) - mon.rms())
    print("65536 channels: max |rms_gpu - rms_ref| = %.3g (bound %.3g) at peak rms %.0f" % (d.max(), T.EPS["edge", R], mon.rms().max()))
    assert d.max() <= T.EPS["edge", R], (float(d.max()), sample[int(np.argmax(d))])
    assert (lv > 0).all()
    hip.free_all()
    bank.close()


if __name__ == "__main__":                                    # the EPS_A table: measured on the CPU, pasted in above
    for recipe, Rs in MEASURED.items():
        for R in Rs:
            worst, peak = measure(recipe, R)
            print('    ("%s", %d): %.3g,   # measured %.3g at peak amplitude %.0f' % (recipe, R, 8 * worst, worst, peak), flush=True)


def test_kept_buffers_grow_and_are_reused(gpu):
    """R = 2, 3 channels on 2 sources, source 1 with a correction off the identity, levels on, fed through the host form
    update_samples in calls of 1, 3, 1 and 2 frames: the host staging, X, the conditioning scratch and the level partials all grow for
    the second call and are reused, larger than needed, by the two behind it.  The outputs against test_gpu_tuner_condition.py's
    yardstick, tolerance 0 (a bank without a correction, fed tuner_condition_ref's corrected rows); the levels against the
    restatement as test_levels_match_the_restatement holds them, the inputs being the edge recipe's (noise in +-20000, the default
    filter, edge_words)."""
    R, n_ch, n_src = 2, 3, 2
    fs = 44100 * R
    rng = np.random.default_rng(2)
    srcs, fws = [0, 1, 1], T.edge_words(R)[4:4 + n_ch]
    bank, plain = (gpu.TunerBank.fastconv(n_ch, n_src, fs, R) for _ in range(2))
    ref = F.TunerFastconvRef(n_ch, n_src, fs, R, g=bank.get_channel_filter())
    for o in (bank, plain, ref):
        T.setup(o, srcs, fws)
    mon = M.MonitorRef(ref, levels=True)
    bank.set_iq_correction(words=CR.KA_WORDS, source=1)
    bank.enable_levels(); plain.enable_levels()
    hip = Hip()
    for k, nf in enumerate((1, 3, 1, 2)):
        raw = T.cs16(rng, n_src, nf * 128 * R)
        fixed = raw.copy()
        fixed[1] = CR.condition(raw[1], CR.KA_WORDS)
        got = bank.update_samples(raw)
        dIn, dI, dQ = hip.upload(fixed), hip.malloc(n_ch * nf * 256), hip.malloc(n_ch * nf * 256)
        assert plain.update_samples_device(dIn, dI, dQ, nf, nf) == nf
        plain.synchronize()
        want = [hip.download(p, (n_ch, nf, 128), np.int16) for p in (dI, dQ)]
        assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k
        assert got[0].any()
        mon.update(fixed); ref.update(fixed)
        check_levels(bank, mon, T.EPS["edge", R], ("grow", k))
    assert bank.condition_launches() == 4 and plain.condition_launches() == 0
    hip.free_all()
    bank.close(); plain.close()
