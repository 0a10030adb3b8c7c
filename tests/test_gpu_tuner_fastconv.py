"""Fast-convolution banks of the digital tuner on the GPU (include/asdr_tuner.h, "Fast-convolution banks";
asdr_tuner_fastconv.hip): u against the float64 restatement tests/tuner_fastconv_ref.py -- within 0.5 + EPS of the unrounded value
(compare_u; EPS from a float32 model of the statement) and, as before, within +-1 with at most 2 % of samples off -- at every FFT
size with filters that weigh all 256 bins, call splits bit-identical, rate configurations through the unchanged stage 2 (+-2, the
mismatch fraction capped by the reference's own), a 65,536-channel bank, and the chain behind it.  The input recipes (CASES) and
compare helpers are shared with test_gpu_tuner_fastconv_edges.py and test_tuner_fastconv_ref.py."""
import collections

import numpy as np
import pytest

import tuner_fastconv_ref as F
from helpers import Hip

pytestmark = pytest.mark.gpu

ALL_R = [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]


def edge_words(R):
    H, N, q = F.sizes(R)
    return [0, 1 << 31, (1 << 31) - 1, (1 << 32) - 1, q // 2, q // 2 - 1, (1 << 32) - q // 2, (N // 2 - 1) * q + q // 2,
            0x9E3779B9, 0x01234567]


def cs16(rng, n_src, n, tones=(), fs=1.0, lo=-20000, hi=20000):
    x = rng.integers(lo, hi, size=(n_src, n, 2), endpoint=True).astype(np.float64)
    m = np.arange(n)
    for s, f, a in tones:
        x[s, :, 0] += a * np.cos(2 * np.pi * f * m / fs)
        x[s, :, 1] += a * np.sin(2 * np.pi * f * m / fs)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def compare(got, want, tol=1, frac=0.02, what=""):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert d.max(initial=0) <= tol, (what, int(d.max()), np.argwhere(d == d.max())[0])
    assert d.size == 0 or (d != 0).mean() <= frac, (what, float((d != 0).mean()))


def clip16(v):
    return np.clip(v, -32768.0, 32767.0)


def compare_u(got, z, eps, what=""):
    """got = (I, Q) int16 [n_channels][n][128], z = stage 1 before rounding (float64, complex [n_channels][n * 128]):
    max |got - clip(z, -32768, 32767)| <= 0.5 + eps on each part.  got being an integer, that is got == rint(z) wherever z is
    further than eps from a half-integer, and one of the two neighbours otherwise."""
    for g, w, part in ((got[0], z.real, "re"), (got[1], z.imag, "im")):
        d = np.abs(g.reshape(g.shape[0], -1).astype(np.float64) - clip16(w))
        assert d.max(initial=0.0) <= 0.5 + eps, (what, part, float(d.max()), 0.5 + eps, np.argwhere(d == d.max())[0])


def setup_pair(bank, ref, srcs, fws):
    for o in (bank, ref):
        setup(o, srcs, fws)


def setup(o, srcs, fws):
    for c, (s, fw) in enumerate(zip(srcs, fws)):
        o.set_source(s, ch=c); o.set_frequency_word(fw, ch=c)


# ---- input recipes of the pass-through comparisons.  A case is a bank's shape and a stream of events that the GPU test applies to
# the bank and the reference, and measure() to the float64 and the float32 reference: ("set", fn) -> fn(o) on each;
# ("iq", iq, label) -> one update() call; ("state",) -> read_state() against the reference's anchors; ("place", P, hist) -> the
# reference is put at position P (place_at), where the test has brought the bank by feeding it.
Case = collections.namedtuple("Case", "n_ch n_src fs R events")


def edge_case(R):
    """Noise in +-20000 plus tones, the default filter, edge_words, retunes between calls, read_state, a reset."""
    fs = 44100 * R
    rng = np.random.default_rng(R)
    fws = edge_words(R)
    n_ch, n_src = len(fws), 3
    srcs = [c % n_src for c in range(n_ch)]

    def events():
        yield ("set", lambda o: setup(o, srcs, fws))
        for k, nf in enumerate([1, 3, 2] if R == 1024 else [1, 3, 2, 5]):
            if k == 1:
                yield ("set", lambda o: (o.set_frequency(fs * 0.123, ch=2), o.set_phase(0xDEADBEEF, ch=5), o.set_source(0, ch=4)))
            if k == 2:
                yield ("set", lambda o: (o.set_frequency_word(0x7FFFF000, ch=0), o.set_phase(12345)))
            tones = [(s, float(rng.uniform(-fs / 2, fs / 2)), 6000.0) for s in range(n_src)] + [(0, fs * 0.123 + 2000.0, 5000.0)]
            yield ("iq", cs16(rng, n_src, nf * 128 * R, tones, fs), (R, k))
        yield ("state",)
        yield ("set", lambda o: (o.reset(), setup(o, srcs, fws)))
        yield ("iq", cs16(rng, n_src, 2 * 128 * R), "after reset")
    return Case(n_ch, n_src, fs, R, events())


def bin_words(R):
    """edge_words plus a channel at k0 = N / 2 - 1 (odd) and, from edge_words, the one at k0 = -N / 2 (fw = 2^31)."""
    H, N, q = F.sizes(R)
    return edge_words(R) + [(N // 2 - 1) * q + 12345 % (q // 2)]


G_FLAT = np.array([1.0], dtype=np.float32)                    # G = 1 on all 256 bins
G_SHORT = np.array([0.75, -0.5], dtype=np.float32)
_ramp = np.random.default_rng(129).uniform(-1.0, 1.0, size=129) / 16.0 * np.linspace(0.25, 1.75, 129)
G_ASYM = _ramp.astype(np.float32)                             # no symmetry: a general complex G with weight on every bin


def all_bins_case(R, filters, seed):
    """Every gathered bin carries signal: noise of amplitude min(20000, 5000 sqrt R) (with G = 1 the 256 of N bins taken leave
    about a sqrt(256 / N) of it, so |z| stays below 30000 at every R) plus four tones of 2500, one within half a bin of k0 + 127
    and one of k0 - 128 for the channel at k0 = N / 2 - 1 and the one at -N / 2, so the wrap of the gather carries signal.
    filters[0] is set before the first call (1 frame, then 3: both parities of b - 1, and a larger X / scratch in the second),
    every further filter before one more 1-frame call, then a reset after which get_channel_filter() must still return it."""
    fs = 44100 * R
    H, N, q = F.sizes(R)
    rng = np.random.default_rng(seed + R)
    fws = bin_words(R)
    n_ch, n_src = len(fws), 3
    srcs = [c % n_src for c in range(n_ch)]
    amp = int(min(20000.0, 5000.0 * np.sqrt(R)))
    tones = []
    for c in (1, n_ch - 1):                                   # k0 = -N / 2 and N / 2 - 1
        k0 = int(F.coarse(fws[c], R)[0])
        for m in (127, -128):
            k = (k0 + m + N // 2) % N - N // 2                # the bin as a frequency in [-N / 2, N / 2)
            tones.append((srcs[c], (k + float(rng.uniform(-0.5, 0.5))) * fs / N, 2500.0))

    def events():
        yield ("set", lambda o: (setup(o, srcs, fws), o.set_channel_filter(filters[0])))
        for k, nf in enumerate([1, 3]):
            yield ("iq", cs16(rng, n_src, nf * H, tones, fs, -amp, amp), (R, k))
        for i, g in enumerate(filters[1:]):
            yield ("set", lambda o, g=g: o.set_channel_filter(g))
            yield ("iq", cs16(rng, n_src, H, tones, fs, -amp, amp), (R, "filter", i + 1))
    return Case(n_ch, n_src, fs, R, events())


def sat_case(R):
    """Full-scale sources through the default filter, then through twice the default filter (|z| passes 40000).  Source 0 is
    (-32768, -32768) throughout (channels at fw = 0 with phase 0 and half a turn: z = -+32768 (1 + j)), source 1 alternates
    (32767, -32768), (-32768, 32767) (channels at Fs_in / 2), source 2 is 32767 e^{j 2 pi f m / Fs_in} 1 kHz above channel 4's
    centre."""
    fs = 44100 * R
    H, N, q = F.sizes(R)
    f0 = 0.1234 * fs
    fws = [0, 0, 1 << 31, 1 << 31, F.RR.fw_from_hz(f0, fs), F.RR.fw_from_hz(f0 + 1500.0, fs)]
    srcs = [0, 0, 1, 1, 2, 2]

    def source(m0, n):
        m = m0 + np.arange(n)
        x = np.zeros((3, n, 2))
        x[0] = -32768
        x[1, :, 0] = np.where(m % 2 == 0, 32767, -32768)
        x[1, :, 1] = np.where(m % 2 == 0, -32768, 32767)
        x[2, :, 0] = np.round(32767.0 * np.cos(2 * np.pi * (f0 + 1000.0) * m / fs))
        x[2, :, 1] = np.round(32767.0 * np.sin(2 * np.pi * (f0 + 1000.0) * m / fs))
        return x.astype(np.int16)

    def events():
        yield ("set", lambda o: (setup(o, srcs, fws), o.set_phase(1 << 31, ch=1), o.set_phase(1 << 30, ch=3)))
        at = 0
        for k, nf in enumerate([1, 3, 2]):
            if k == 2:
                yield ("set", lambda o: o.set_channel_filter(2.0 * np.asarray(o.get_channel_filter(), dtype=np.float32)))
            yield ("iq", source(at, nf * H), (R, k))
            at += nf * H
    return Case(len(fws), 3, fs, R, events())


WRAP_FRAMES, WRAP_P0 = 64, (1 << 32) - 2 * 131072


def wrap_case(R=1024):
    """Positions past 2^32: R = 1024 (H = 131072), one source.  The test feeds the bank `fed` (64 frames of noise) 511 times plus
    its first 62 frames, so P = 2^32 - 2 H, where the reference is placed; then 4 frames (2^32 is crossed after the second),
    two retunes at P > 2^32, 2 more frames and read_state.  Every other channel keeps its anchor of position 0."""
    assert R == 1024
    fs = 44100 * R
    H, N, q = F.sizes(R)
    rng = np.random.default_rng(1 << 32)
    fws = edge_words(R) + [12345 * q + q // 2 - 3, (-54321 * q - q // 2 + 1) & 0xFFFFFFFF]      # odd k0, rw at its ends
    fed = cs16(rng, 1, WRAP_FRAMES * H)

    def events():
        yield ("set", lambda o: (setup(o, [0] * len(fws), fws), o.set_phase(0xCAFEF00D, ch=3)))
        yield ("feed", fed)
        yield ("place", WRAP_P0, fed[:, 61 * H:62 * H])
        for k in range(4):
            yield ("iq", cs16(rng, 1, H), ("frame", k))
        yield ("set", lambda o: (o.set_frequency_word(0x2468ACE1, ch=4), o.set_phase(0x13579BDF, ch=10)))
        yield ("iq", cs16(rng, 1, 2 * H), "after the retunes")
        yield ("state",)
    return Case(len(fws), 1, fs, R, events())


def switch_case(R=8):
    """The pass-through calls of a 44100 R bank that is then given a real stage 2 (the edges module goes on from here)."""
    fs = 44100 * R
    rng = np.random.default_rng(44100)
    fws = edge_words(R)[:6]

    def events():
        yield ("set", lambda o: setup(o, [c % 2 for c in range(6)], fws))
        for k, nf in enumerate([2, 1]):
            yield ("iq", cs16(rng, 2, nf * 128 * R, [(0, 3000.0, 6000.0)], fs), (R, k))
    return Case(6, 2, fs, R, events())


CASES = {"edge": edge_case, "flat": lambda R: all_bins_case(R, [G_FLAT], 1000),
         "asym": lambda R: all_bins_case(R, [G_ASYM, G_SHORT], 2000), "sat": sat_case, "wrap": wrap_case, "switch": switch_case}
CASE_R = {"edge": [2, 16, 128, 1024], "flat": ALL_R, "asym": ALL_R, "sat": [2, 32], "wrap": [1024], "switch": [8]}


def measure(recipe, R):
    """(largest |stage1_f32 - stage1| on either part, both clipped to the int16 range as compare_u clips; peak |z|) over the
    recipe's own inputs."""
    case = CASES[recipe](R)
    a, b = (F.TunerFastconvRef(case.n_ch, case.n_src, case.fs, R) for _ in range(2))
    worst = peak = 0.0
    for ev in case.events:
        if ev[0] == "set":
            ev[1](a); ev[1](b)
        elif ev[0] == "place":
            a.place_at(ev[1], ev[2]); b.place_at(ev[1], ev[2])
        elif ev[0] == "iq":
            z = a.update(ev[1], keep_float=True)[2]
            w = b.update(ev[1], keep_float=True, f32=True)[2]
            worst = max(worst, float(np.abs(clip16(w.real) - clip16(z.real)).max()), float(np.abs(clip16(w.imag) - clip16(z.imag)).max()))
            peak = max(peak, float(np.abs(z).max()))
    return worst, peak


# EPS[recipe, R] = 8 x measure(recipe, R)[0] to three digits.  8: two correct float32 implementations differ in pass
# order, twiddle tables, the NCO's float phase and the place of 1 / N, and a float32 FFT's error lies between sqrt(log N) and log N
# times 2^-24 of the signal; 8 covers that spread and stays far below one LSB (every entry <= 0.1).  Produced by
#     python tests/test_gpu_tuner_fastconv.py
# (test_tuner_fastconv_ref.py recomputes the entries with R <= 16).
EPS = {
    ("edge", 2): 0.0386,   # measured 0.00482 at peak |z| 23666
    ("edge", 16): 0.018,   # measured 0.00225 at peak |z| 12609
    ("edge", 128): 0.017,   # measured 0.00212 at peak |z| 8222
    ("edge", 1024): 0.00182,   # measured 0.000228 at peak |z| 1115
    ("flat", 2): 0.0196,   # measured 0.00245 at peak |z| 12821
    ("flat", 4): 0.0214,   # measured 0.00267 at peak |z| 14694
    ("flat", 8): 0.0212,   # measured 0.00265 at peak |z| 15204
    ("flat", 16): 0.0193,   # measured 0.00241 at peak |z| 15862
    ("flat", 32): 0.0149,   # measured 0.00186 at peak |z| 12072
    ("flat", 64): 0.014,   # measured 0.00175 at peak |z| 9993
    ("flat", 128): 0.0103,   # measured 0.00128 at peak |z| 8537
    ("flat", 256): 0.0109,   # measured 0.00137 at peak |z| 9466
    ("flat", 512): 0.0101,   # measured 0.00127 at peak |z| 9067
    ("flat", 1024): 0.0127,   # measured 0.00158 at peak |z| 8462
    ("asym", 2): 0.0154,   # measured 0.00192 at peak |z| 12805
    ("asym", 4): 0.0175,   # measured 0.00219 at peak |z| 13779
    ("asym", 8): 0.0199,   # measured 0.00249 at peak |z| 14581
    ("asym", 16): 0.0211,   # measured 0.00264 at peak |z| 15219
    ("asym", 32): 0.0153,   # measured 0.00191 at peak |z| 13073
    ("asym", 64): 0.0119,   # measured 0.00149 at peak |z| 10617
    ("asym", 128): 0.0128,   # measured 0.0016 at peak |z| 9605
    ("asym", 256): 0.0123,   # measured 0.00154 at peak |z| 9206
    ("asym", 512): 0.013,   # measured 0.00162 at peak |z| 10106
    ("asym", 1024): 0.0123,   # measured 0.00154 at peak |z| 11835
    ("sat", 2): 0.0901,   # measured 0.0113 at peak |z| 92682
    ("sat", 32): 0.1,   # measured 0.015 at peak |z| 92682: 8 x is 0.12, held to the 0.1 ceiling (the doubled filter's 65534 tone)
    ("wrap", 1024): 0.00164,   # measured 0.000205 at peak |z| 1091
    ("switch", 8): 0.0189,   # measured 0.00236 at peak |z| 15210
}
assert max(EPS.values()) <= 0.1


def run_pass_through(bank, ref, events, eps, plus_old=False):
    """Apply a case to the bank and the reference; every call's output under compare_u (and the older compare()).  Returns the
    calls' (I, Q, z)."""
    outs = []
    for ev in events:
        if ev[0] == "set":
            ev[1](bank); ev[1](ref)
        elif ev[0] == "state":
            st = bank.read_state()
            assert list(st["ph_a"]) == list(ref.ph_a) and list(st["pos_a"]) == list(ref.pos_a)
            assert list(st["fw"]) == list(ref.fw) and list(st["src"]) == list(ref.src)
        elif ev[0] == "iq":
            I, Q = bank.update(ev[1])
            wI, wQ, z = ref.update(ev[1], keep_float=True)
            print(ev[2], "max |got - z| = %.4f re, %.4f im (bound %.4f)" % (
                np.abs(I.reshape(I.shape[0], -1) - clip16(z.real)).max(), np.abs(Q.reshape(Q.shape[0], -1) - clip16(z.imag)).max(), 0.5 + eps))
            compare_u((I, Q), z, eps, ev[2])
            if plus_old:
                compare(I, wI, what=ev[2]); compare(Q, wQ, what=ev[2])
            assert bank.position() == ref.P and bank.output_position() == ref.out_pos
            outs.append((I, Q, z))
        else:
            raise AssertionError(ev[0])
    return outs


def pair(gpu, case):
    """The bank of a case and a reference with the bank's own default taps."""
    bank = gpu.TunerBank.fastconv(case.n_ch, case.n_src, case.fs, case.R)
    assert bank.ratio() == (1, 1) and bank.fft_size() == 256 * case.R
    return bank, F.TunerFastconvRef(case.n_ch, case.n_src, case.fs, case.R, g=bank.get_channel_filter())


class Stage2Cap:
    """Outputs behind a real stage 2: +-2 on every sample (one LSB of u through a phase of sum |h2| <= 65535 is at most 2 LSB of
    y), and no more samples off than the reference itself shows when its own u is moved by +-1 on a seeded random 2 % of samples
    (stage 1's older cap, above what a stage 1 that passes compare_u can do) and resampled again.  Counted over all the calls of
    a test, since single calls write as little as no block."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.off = self.cap_off = self.n = 0

    def update(self, ref, iq):
        """ref.update(iq), and the count for the perturbed u of the same call."""
        j0 = ref.out_pos
        wI, wQ = ref.update(iq)
        assert not ref.pass_through()
        n = wI.shape[1] * 128
        if n:
            d = self.rng.choice([-1, 1], size=ref.u.shape) * (self.rng.random(ref.u.shape) < 0.02)
            y = F.RR.resample(np.clip(ref.u + d, -32768, 32767), ref.h2, ref.U, ref.M, ref.g2, j0, n, ref.zero_before)
            self.cap_off += int((y[:, 0].reshape(wI.shape) != wI).sum()) + int((y[:, 1].reshape(wQ.shape) != wQ).sum())
        return wI, wQ

    def check(self, got, want, what=""):
        compare(got, want, tol=2, frac=1.0, what=what)
        self.off += int((got != want).sum())
        self.n += got.size

    def finish(self, what=""):
        assert self.n > 0
        msg = "%s: %.4f of samples off, the reference's own cap %.4f" % (what, self.off / self.n, self.cap_off / self.n)
        print(msg)
        assert self.off <= self.cap_off, msg


@pytest.mark.parametrize("R", [2, 16, 128, 1024])
def test_u_matches_the_restatement_with_pass_through_stage_2(gpu, R):
    case = edge_case(R)
    bank, ref = pair(gpu, case)
    outs = run_pass_through(bank, ref, case.events, EPS["edge", R], plus_old=True)
    assert len(outs) == (4 if R == 1024 else 5)
    bank.close()


@pytest.mark.parametrize("recipe", ["flat", "asym"])
@pytest.mark.parametrize("R", ALL_R)
def test_every_fft_size_with_filters_that_weigh_every_bin(gpu, R, recipe):
    """All ten N with g = [1] (G = 1 on 256 bins) and with an asymmetric 129-tap filter, tones at both ends of the gather where it
    wraps around N; for the second, a change to g = [0.75, -0.5] between calls applies from the next call's first sample, and
    the filter survives reset() bit for bit."""
    case = CASES[recipe](R)
    bank, ref = pair(gpu, case)
    outs = run_pass_through(bank, ref, case.events, EPS[recipe, R])
    assert len(outs) == (2 if recipe == "flat" else 3)
    if recipe == "flat":
        assert max(float(np.abs(z).max()) for _, _, z in outs) < 30000.0
    last = G_FLAT if recipe == "flat" else G_SHORT
    bank.reset()
    g = bank.get_channel_filter()
    assert g.dtype == np.float32 and g.tobytes() == last.tobytes()
    bank.close()


@pytest.mark.parametrize("R", [16, 32])
def test_call_splits_are_bit_identical(gpu, R):
    fs = 44100 * R
    rng = np.random.default_rng(7 + R)
    n_ch, n_src, total = 9, 2, 12
    fws = [int(v) for v in rng.integers(0, 2 ** 32, size=n_ch, dtype=np.uint64)]
    iq = cs16(rng, n_src, total * 128 * R)
    outs = []
    for split in ([total], [1] * total, [5, 1, 2, 4], [3, 7, 2]):
        bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
        for c in range(n_ch):
            bank.set_source(c % n_src, ch=c); bank.set_frequency_word(fws[c], ch=c)
        parts, at = [], 0
        for nf in split:
            parts.append(bank.update(iq[:, at:at + nf * 128 * R]))
            at += nf * 128 * R
        outs.append((np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)))
        bank.close()
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])


@pytest.mark.parametrize("fs,R", [(2400000, 16), (20000000, 128), (61440000, 512)])
def test_rate_configurations_through_stage_2(gpu, fs, R):
    rng = np.random.default_rng(fs // 1000)
    n_ch, n_src = 6, 2
    bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
    h2, g2 = bank.get_resampler()
    ref = F.TunerFastconvRef(n_ch, n_src, fs, R, g=bank.get_channel_filter(), h2=h2, g2=g2)
    fws = edge_words(R)[:n_ch]
    setup_pair(bank, ref, [c % n_src for c in range(n_ch)], fws)
    cap = Stage2Cap(fs)
    for k, nf in enumerate([1, 4, 2, 7, 1, 3]):
        if k == 3:
            for o in (bank, ref):
                o.set_frequency(-fs * 0.3, ch=1); o.set_phase(0x40000000, ch=2)
        iq = cs16(rng, n_src, nf * 128 * R, [(0, fs * 0.01, 6000.0)], fs)
        n = bank.out_blocks(nf)
        assert n == ref.out_blocks(nf)
        I, Q = bank.update_rate(iq)
        wI, wQ = cap.update(ref, iq)
        assert I.shape == wI.shape == (n_ch, n, 128)
        cap.check(I, wI, what=k); cap.check(Q, wQ, what=k)
        assert bank.output_position() == ref.out_pos
    cap.finish((fs, R))
    bank.close()


def test_65536_channels_16_sources_at_2_4_msps(gpu):
    fs, R, n_ch, n_src, nf = 2400000, 16, 65536, 16, 16
    rng = np.random.default_rng(65536)
    bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
    h2, g2 = bank.get_resampler()
    srcs = (np.arange(n_ch) * 7) % n_src
    fws = rng.integers(0, 2 ** 32, size=n_ch, dtype=np.uint64)
    for c in range(n_ch):
        bank.set_source(int(srcs[c]), ch=c); bank.set_frequency_word(int(fws[c]), ch=c)
    sample = sorted(set([0, 1, n_ch - 1] + [int(c) for c in rng.integers(0, n_ch, size=61)]))
    ref = F.TunerFastconvRef(len(sample), n_src, fs, R, g=bank.get_channel_filter(), h2=h2, g2=g2)
    for i, c in enumerate(sample):
        ref.src[i], ref.fw[i] = int(srcs[c]), int(fws[c])
    hip = Hip()
    s2 = Stage2Cap(65536)
    cap = nf + 1
    dI, dQ = hip.malloc(n_ch * cap * 256), hip.malloc(n_ch * cap * 256)
    s = hip.stream()
    for call in range(3):
        iq = cs16(rng, n_src, nf * 128 * R)
        dIQ = hip.upload(iq)
        n = bank.update_rate_device(dIQ, dI, dQ, nf, cap, stream=s)
        hip.sync(s)
        wI, wQ = s2.update(ref, iq)
        assert n == wI.shape[1]
        for i, c in enumerate(sample):
            gI = hip.download(dI, (n, 128), np.int16, offset_bytes=c * cap * 256)
            gQ = hip.download(dQ, (n, 128), np.int16, offset_bytes=c * cap * 256)
            s2.check(gI, wI[i], what=(call, c)); s2.check(gQ, wQ[i], what=(call, c))
    s2.finish("65536 channels")
    hip.free_all()
    bank.close()


def test_fastconv_bank_into_the_chain_on_one_stream(gpu, ao):
    """Fast-convolution bank (2.4 MS/s, R = 16) -> asdr_update_device (USB) on one stream: the chain's audio equals the oracle run
    on the tuner's own output, bit for bit, and the tuner's output is the restatement's within +-2."""
    fs, R, nf = 2400000, 16, 48
    fc = 7_000_000.0
    dials = [fc + 250_000.0, fc - 410_000.0]
    rng = np.random.default_rng(24)
    n = nf * 128 * R
    t = np.arange(n) / fs
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 2.0
    for f, a in ((dials[0] + 1200.0 - fc, 3000.0), (dials[1] + 700.0 - fc, 3000.0)):
        z = z + a * np.exp(2j * np.pi * f * t)
    iq = np.stack([np.round(z.real), np.round(z.imag)], axis=-1).astype(np.int16)
    sdr = gpu.AudioSDRBatch(2)
    tuner = gpu.TunerBank.fastconv(2, 1, fs, R)
    h2, g2 = tuner.get_resampler()
    ref = F.TunerFastconvRef(2, 1, fs, R, g=tuner.get_channel_filter(), h2=h2, g2=g2)
    cap = Stage2Cap(24)
    sdr.setDemodMode(gpu.USBmode)
    for c in range(2):
        hz = dials[c] - fc - sdr.getTuningOffset(c)
        tuner.set_frequency(hz, ch=c); ref.set_frequency(hz, ch=c)
    hip = Hip()
    s = hip.stream()
    dIQ = hip.upload(iq[None])
    nb = tuner.out_blocks(nf)
    row = nb * 128 * 2
    dI, dQ, dOut = hip.malloc(2 * row), hip.malloc(2 * row), hip.malloc(2 * row)
    assert tuner.update_rate_device(dIQ, dI, dQ, nf, nb, stream=s) == nb
    sdr.update_device(dI, dQ, dOut, nb, stream=s)
    hip.sync(s)
    got = hip.download(dOut, (2, nb, 128), np.int16)
    tI, tQ = hip.download(dI, (2, nb, 128), np.int16), hip.download(dQ, (2, nb, 128), np.int16)
    wI, wQ = cap.update(ref, iq[None])
    cap.check(tI, wI); cap.check(tQ, wQ)
    cap.finish("into the chain")
    want, _ = ao.run_channels(lambda o, c: o.setDemodMode(ao.USBmode), tI, tQ)
    assert np.array_equal(got, want)
    for c, tone in enumerate((1200.0, 700.0)):
        a = got[c].reshape(-1)[nb * 128 // 2:].astype(float)
        spec = np.abs(np.fft.rfft((a - a.mean()) * np.hanning(a.size)))
        peak = np.fft.rfftfreq(a.size, 1 / 44100.0)[np.argmax(spec)]
        assert abs(peak - tone) < 20.0, (c, peak)
    hip.free_all()
    sdr.close(); tuner.close()


if __name__ == "__main__":                                    # the EPS table: measured on the CPU, pasted in above
    for recipe, Rs in CASE_R.items():
        for R in Rs:
            worst, peak = measure(recipe, R)
            print('    ("%s", %d): %.3g,   # measured %.3g at peak |z| %.0f' % (recipe, R, 8 * worst, worst, peak), flush=True)
