"""The composed restatement of a fully loaded bank (tests/tuner_full_ref.py) and the recipes of tests/test_gpu_tuner_full.py, on
the CPU.  (a) Closure: with everything at the defaults the composition is TunerFastconvRef, with only the palette in use it is
TunerPaletteRef, bit for bit.  (b) Sensitivity: on every recipe of the GPU file, each of eight deliberately wrong compositions
moves at least one compared quantity by more than 10 x that quantity's bound on the recipe's own inputs -- the evidence that the GPU
tests would notice a kernel that is wrong in that way.  (c) The R = 2 entries of the GPU file's tolerance tables recomputed from
the float32 models.  And the conditions that keep the recipes honest: no sample of an unclamped channel near the clamp, no
conditioned sample clipped but the rail-valued ones at the row ends."""
import numpy as np
import pytest

import test_gpu_tuner_full as TF
import tuner_condition_ref as CR
import tuner_fastconv_ref as F
import tuner_formats_ref as FM
import tuner_full_ref as FR
import tuner_palette_ref as P

T, TP = TF.T, TF.TP
MARGIN = 10.0


# ---- (a) closure ---------------------------------------------------------------------------------------------------------------
def test_with_everything_at_the_defaults_it_is_the_plain_restatement():
    R = 4
    fs = 44100 * R
    rng = np.random.default_rng(40)
    fws = T.edge_words(R)
    n_ch = len(fws)
    plain = F.TunerFastconvRef(n_ch, 2, fs, R, g=T.G_ASYM)
    full = FR.LoadedBankRef(n_ch, 2, fs, R, g=T.G_ASYM)
    for o in (plain, full):
        T.setup(o, [c % 2 for c in range(n_ch)], fws)
    full.set_input_format("cs16"); full.set_iq_correction(words=CR.IDENTITY)
    for k, nf in enumerate((1, 3, 2)):
        if k == 1:
            for o in (plain, full):
                o.set_frequency_word(0x7FFFF000, ch=0); o.set_phase(12345, ch=3)
        iq = T.cs16(rng, 2, nf * 128 * R)
        a, b = plain.update(iq, keep_float=True), full.update_samples(iq)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert full.position() == plain.P and full.output_position() == plain.out_pos
    assert full.condition_launches() == 0 and list(full.slots()) == [0] * n_ch and list(full.gains()) == [1.0] * n_ch
    assert full.spectrum()[1] == 0 and full.mon.level_frames == 0


def test_with_only_the_palette_in_use_it_is_the_palette_restatement():
    R = 2
    case = TP.parity_case(R)
    pal = P.TunerPaletteRef(case.n_ch, case.n_src, case.fs, R)
    full = FR.LoadedBankRef(case.n_ch, case.n_src, case.fs, R)
    n = 0
    for ev in case.events:
        if ev[0] == "set":
            ev[1](pal); ev[1](full)
        else:
            a, b = pal.update(ev[1], keep_float=True), full.update_samples(ev[1])
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            n += 1
    assert n == 2 and list(full.slots()) == list(pal.slots()) and (full.gains() != 1.0).any()
    iq = T.cs16(np.random.default_rng(3), case.n_src, 128 * R, (), 1.0, -2000, 2000)
    full.f32 = True
    assert np.array_equal(pal.stage1_f32(iq), full.update_samples(iq)[2])


# ---- (b) the wrong compositions ------------------------------------------------------------------------------------------------
class CorrectionDropped(FR.LoadedBankRef):
    """The correction dropped on source 1."""
    def correct(self, x):
        kept = list(self.corr)
        self.corr[1] = CR.IDENTITY
        out = super().correct(x)
        self.corr = kept
        return out


class CorrectionOnTheOtherSource(FR.LoadedBankRef):
    """The two sources' corrections exchanged: the one at the identity gets the other's."""
    def correct(self, x):
        self.corr.reverse()
        out = super().correct(x)
        self.corr.reverse()
        return out


class GainInTheLevel(FR.LoadedBankRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        energy = self.mon.frame_energy
        self.mon.frame_energy = lambda X: energy(X) * self.ref.gain.astype(np.float64) ** 2


class SpectrumOfTheUnconditionedRows(FR.LoadedBankRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.spec = P.PaletteMonitorRef(self.ref)

    def enable_spectrum(self, *a):
        super().enable_spectrum(*a); self.spec.enable_spectrum(*a)

    def monitor(self, x, xc):
        super().monitor(x, xc); self.spec.update(x)

    def spectrum(self):
        return self.spec.acc, self.spec.frames


class StatisticsOfTheConditionedRows(FR.LoadedBankRef):
    def stats_of(self, raw, x, xc):
        if self.fmt == "rs16":
            return [CR.stats(xc[s][:, 0], "rs16") for s in range(self.ref.n_src)]
        return [CR.stats(xc[s], "cs16") for s in range(self.ref.n_src)]


class SlotsSwapped(FR.LoadedBankRef):
    """Channels 0 and 1 each on the other's slot, in stage 1 and in the level."""
    def update_samples(self, raw, run=None):
        s = self.ref.slot
        s[0], s[1] = s[1], s[0]
        assert s[0] != s[1]
        out = super().update_samples(raw, run)
        s[0], s[1] = s[1], s[0]
        return out


class Cu8ReadAsCs8(FR.LoadedBankRef):
    def convert(self, raw):
        return FM.to_cs16(raw.view(np.int8), "cs8") if self.fmt == "cu8" else super().convert(raw)


class StraddlingHistoryUnconditioned(FR.LoadedBankRef):
    """In the first call after the last correction has gone back to the identity, the windows' first half is x of the call before
    and not x': what a switch of kernel families that re-read the caller's rows would leave."""
    before = None

    def update_samples(self, raw, run=None):
        ident = all(c == CR.IDENTITY for c in self.corr)
        if ident and self.before is not None and not self.before[0]:
            h = self.before[1]
            self.ref.hist = h[..., 0].astype(np.float64) + 1j * h[..., 1].astype(np.float64)
            self.mon.hist = self.ref.hist.copy()
        self.before = (ident, self.convert(raw)[:, -self.ref.H:])
        return super().update_samples(raw, run)


WRONG = {"correction dropped on one source": CorrectionDropped, "correction on the source at the identity": CorrectionOnTheOtherSource,
         "gain included in the level": GainInTheLevel, "spectrum of the unconditioned rows": SpectrumOfTheUnconditionedRows,
         "statistics of the conditioned rows": StatisticsOfTheConditionedRows, "two channels' slots swapped": SlotsSwapped,
         "a cu8 row read as cs8": Cu8ReadAsCs8, "straddling frame's history unconditioned": StraddlingHistoryUnconditioned}
MUST_MOVE = {"gain included in the level": "levels", "spectrum of the unconditioned rows": "spectrum",
             "statistics of the conditioned rows": "statistics"}


def observe(s, kw, cls):
    """Per call what the GPU test compares: the output (z, clipped as compare_u clips, or (I, Q) behind a real stage 2), the
    spectrum's amplitude, the rms levels, the statistics."""
    L = TF.composed(s, kw, cls=cls)
    out = []
    for ev in s.events:
        if ev[0] == "set":
            ev[1](L)
        else:
            I, Q, z = L.update_samples(ev[1])
            y = np.stack([I, Q]).astype(np.float64) if not L.pass_through() else np.stack([T.clip16(z.real), T.clip16(z.imag)])
            acc, frames = L.spectrum()
            out.append((y, TF.TM.M.amplitude(acc, frames, TF.SPEC[2]), L.rms().copy(), L.iq_stats(clear=False)))
    return out


_right = {}


def right(key, A):
    if key not in _right:
        s = TF.stream(key, A)
        _right[key] = (TF.taps(A, s), observe(s, TF.taps(A, s), FR.LoadedBankRef))
    return _right[key]


CU8_ONLY = "a cu8 row read as cs8"                             # applies where the recipe has CU8 rows


@pytest.mark.parametrize("key,wrong", [(k, w) for k in TF.KEYS for w in WRONG if w != CU8_ONLY or k[0].startswith("cu8")],
                         ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else "%s-%d" % v)
def test_every_recipe_tells_a_wrong_composition_apart(A, key, wrong):
    """Margins: the largest difference between the wrong and the right composition over the recipe's calls, in units of the bound
    the GPU test holds that quantity to -- 0.5 + EPS for the output (+-2 behind a real stage 2), EPS_A for the spectrum, EPS for
    the levels; the statistics are exact, so any difference there is past every multiple of the bound."""
    kw, want = right(key, A)
    got = observe(TF.stream(key, A), kw, WRONG[wrong])
    out_bound = 2.0 if key[0].endswith("+s2") else 0.5 + TF.EPS[key]
    margins = {"output": max(float(np.abs(g[0] - w[0]).max(initial=0.0)) for g, w in zip(got, want)) / out_bound,
               "spectrum": max(float(np.abs(g[1] - w[1]).max()) for g, w in zip(got, want)) / TF.EPS_A[key],
               "levels": max(float(np.abs(g[2] - w[2]).max()) for g, w in zip(got, want)) / TF.EPS[key],
               "statistics": np.inf if any(g[3] != w[3] for g, w in zip(got, want)) else 0.0}
    print(key, wrong, {k: "%.3g" % v for k, v in margins.items()})
    assert max(margins.values()) > MARGIN, (key, wrong, margins)
    if wrong in MUST_MOVE:
        assert margins[MUST_MOVE[wrong]] > MARGIN, (key, wrong, margins)


INT_WRONG = ["correction dropped on one source", "correction on the source at the identity", "statistics of the conditioned rows",
             "a cu8 row read as cs8", "straddling frame's history unconditioned"]


@pytest.mark.parametrize("kind,fmt,wrong", [(k, f, w) for k, f in TF.INT_CASES for w in INT_WRONG if w != CU8_ONLY or f == "cu8"])
def test_the_integer_recipes_tell_a_wrong_composition_apart(A, kind, fmt, wrong):
    """The direct-form and rate recipes are held at tolerance 0: a wrong composition must change an output sample (or, for the
    statistics, a sum)."""
    banks = [TF.int_pair(A, kind, device=A.NO_DEVICE) for _ in range(2)]
    (_, ref), (_, bad) = banks
    differs = False
    for k, (raw, corr) in enumerate(zip(TF.int_rows(kind, fmt), TF.INT_CORRECTIONS)):
        want = FR.integer_bank_update(ref, raw, fmt, corr)
        x = FM.to_cs16(raw, fmt)
        xc = FR.conditioned(raw, fmt, corr)
        if wrong == "correction dropped on one source":
            xw = FR.conditioned(raw, fmt, [corr[0], CR.IDENTITY])
        elif wrong == "correction on the source at the identity":
            xw = FR.conditioned(raw, fmt, corr[::-1])
        elif wrong == "a cu8 row read as cs8":
            xw = FR.conditioned(raw.view(np.int8), "cs8", corr)
        else:
            xw = xc
        if wrong == "straddling frame's history unconditioned" and k == 2:
            for s in range(TF.INT_N_SRC):
                bad.x[s][-before.shape[1]:] = before[s]
        if wrong == "statistics of the conditioned rows":
            differs |= any(CR.stats(raw[s], fmt) != CR.stats(xc[s][:, 0] if fmt == "rs16" else xc[s], "rs16" if fmt == "rs16" else "cs16")
                           for s in range(TF.INT_N_SRC))
        got = bad.update(xw)
        differs |= any(not np.array_equal(g, w) for g, w in zip(got, want))
        before = x
    for bank, _ in banks:
        bank.close()
    assert differs, (kind, fmt, wrong)


# ---- (c) the tolerance tables --------------------------------------------------------------------------------------------------
def test_the_tolerance_tables_are_eight_times_the_float32_models(A):
    assert set(TF.EPS) == set(TF.EPS_A) == set(TF.KEYS) and max(TF.EPS.values()) <= 0.1
    done = 0
    for key in TF.KEYS:
        if key[1] == 2:
            m = TF.measure(key, A)
            want, want_a = min(8 * m[0], 0.1), 8 * m[2]
            assert abs(TF.EPS[key] - want) <= 0.1 * want, (key, TF.EPS[key], want)
            assert abs(TF.EPS_A[key] - want_a) <= 0.1 * want_a, (key, TF.EPS_A[key], want_a)
            done += 1
    assert done == len(TF.FMTS)


# ---- the conditions that keep the recipes honest -------------------------------------------------------------------------------
@pytest.mark.parametrize("key", TF.KEYS, ids=lambda k: "%s-%d" % k)
def test_recipes_stay_off_the_clamp_and_off_the_conditioning_clip(A, key):
    """Conditioned samples differ from the unclipped correction nowhere but on the first and last sample of a row, where the
    stored rows sit on the rails.  Peak |z| of the float64 restatement stays below 32000 on every channel that is never clamped,
    and on every channel outside the reach of those rail-valued row ends (the 129 taps behind one, a sample ahead); every clamped
    sample lies within that reach (the ends drive the gain-8 channels, and the channels at Fs_in / 2 where two ends of opposite
    sign meet), and more than 40 % of every channel's samples lie outside it."""
    s = TF.stream(key, A)
    L = TF.composed(s, TF.taps(A, s))
    zs, ends = [], []
    for ev in s.events:
        if ev[0] == "set":
            ev[1](L)
            continue
        raw = ev[1]
        ends += [L.position(), L.position() + raw.shape[1] - 1]
        x = L.convert(raw).astype(np.int64)
        xc = L.correct(L.convert(raw)).astype(np.int64)
        for src in range(s.n_src):
            d_r, d_i, p, g = L.corr[src]
            a, b = x[src, :, 0] - d_r, x[src, :, 1] - d_i
            free = np.stack([a, np.zeros_like(a) if s.fmt == "rs16" else (p * a + g * b + 32768) >> 16], axis=-1)
            clipped = np.argwhere((free != xc[src]).any(axis=-1)).reshape(-1)
            assert set(clipped.tolist()) <= {0, raw.shape[1] - 1}, (key, ev[2], src, clipped[:8])
            inner = xc[src, 1:-1]
            assert inner.min() > -32768 and inner.max() < 32767, (key, ev[2], src)
        zs.append(L.update_samples(raw)[2])
    z = np.concatenate(zs, axis=1)
    over = (np.abs(z.real) > 32767.0) | (np.abs(z.imag) > 32767.0)
    clamped = over.any(axis=1)
    n = np.arange(z.shape[1])
    near = np.zeros(z.shape[1], dtype=bool)
    for p in ends:
        near |= ((n - 130) * s.R <= p) & (p <= (n + 2) * s.R)
    print(key, "peak |z| %.0f on unclamped channels, %.0f outside the row ends' reach (%.0f %% of the samples); clamped channels %s" % (
        np.abs(z[~clamped]).max(), np.abs(z[:, ~near]).max(), 100.0 * (~near).mean(), np.flatnonzero(clamped).tolist()))
    assert np.abs(z[~clamped]).max() < 32000.0 and np.abs(z[:, ~near]).max() < 32000.0
    assert not over[:, ~near].any() and (~near).mean() > 0.4
