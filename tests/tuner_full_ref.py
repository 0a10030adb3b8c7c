"""The composed restatement of a fully loaded tuner bank: an input format, per-source corrections with statistics, a filter palette
with slots and gains, both monitors and, optionally, a real stage 2, all on at once (include/asdr_tuner.h).  No arithmetic of its
own: LoadedBankRef chains the existing restatements in the order the header states them --
    stored rows --tuner_formats_ref.to_cs16--> x --tuner_condition_ref.condition, per source--> x'
    x' --> tuner_palette_ref.PaletteMonitorRef (the spectrum of X, the level with G_{f_c} and without a_c)
    x' --> tuner_palette_ref.TunerPaletteRef (stage 1 with G_{f_c} and a_c, then tuner_rate_ref's stage 2)
    stored rows --tuner_condition_ref.stats--> the seven sums (of x, before the correction)
-- in float64; f32 = True runs stage 1 by the float32 models that size the GPU tests' tolerances (stage1_f32, for real rows
tuner_formats_ref.stage1_half_f32; the spectrum by the complex64 model of test_gpu_tuner_monitor.reference).  Every step is a
method of its own, so tests/test_tuner_full_ref.py can put a deliberately wrong one in its place.  integer_bank_update() is the
same composition in front of a direct-form or rate bank's integer restatement."""
import numpy as np

import tuner_condition_ref as CR
import tuner_formats_ref as FM
import tuner_palette_ref as P


class _PaletteRef(P.TunerPaletteRef):
    """TunerPaletteRef whose float32 model of real rows is the half-size transform's."""
    real_rows = False

    def stage1_f32(self, iq):
        return FM.stage1_half_f32(self, iq) if self.real_rows else super().stage1_f32(iq)


class LoadedBankRef:
    """A fast-convolution bank with everything on.  Takes the bank's setters: those of the channels, the palette and the resampler
    go to the TunerPaletteRef (`ref`), those of the monitors to the PaletteMonitorRef over it (`mon`); the format, the corrections
    and the statistics are kept here."""

    def __init__(self, n_channels, n_sources, fs_in, R, g=None, h2=None, g2=1, f32=False):
        self.ref = _PaletteRef(n_channels, n_sources, fs_in, R, g=g, h2=h2, g2=g2)
        self.mon = P.PaletteMonitorRef(self.ref)
        self.f32 = bool(f32)
        self.fmt = "cs16"
        self.corr = [CR.IDENTITY] * self.ref.n_src
        self.stats_on = False
        self.launches = 0
        self.rows = []                                        # x' of every call since creation / reset (for spectrum_model_error)
        self.clear_iq_stats()

    def __getattr__(self, name):                              # set_source, set_frequency_word, set_palette_filter, slots, ...
        return getattr(self.ref, name)

    # what the bank keeps besides the channels
    def set_input_format(self, fmt):
        assert fmt in FM.FORMATS
        self.fmt = fmt

    def set_iq_correction(self, words=CR.IDENTITY, source=-1):
        words = tuple(int(w) for w in words)
        assert CR.in_range(words)
        for s in (range(self.ref.n_src) if source == -1 else [source]):
            self.corr[s] = words

    def enable_iq_stats(self, on=True):
        self.stats_on = bool(on)
        self.clear_iq_stats()

    def clear_iq_stats(self):
        self.stats = [(0,) * 7] * self.ref.n_src

    def iq_stats(self, clear=True):
        st = list(self.stats)
        if clear:
            self.clear_iq_stats()
        return st

    def enable_spectrum(self, n_bins, window="hann", mode="sum"):
        self.mon.enable_spectrum(n_bins, window, mode)

    def enable_levels(self, on=True):
        self.mon.enable_levels(on)

    def reset(self):
        """As asdr_tuner_reset: the format and the corrections stay, the statistics and both monitors are cleared."""
        self.ref.reset(); self.mon.reset()
        self.clear_iq_stats()
        self.rows = []

    def position(self):
        return self.ref.P

    def output_position(self):
        return self.ref.out_pos

    def condition_launches(self):
        return self.launches

    # the steps of one call, in the header's order
    def convert(self, raw):
        return FM.to_cs16(raw, self.fmt)

    def correct(self, x):
        return np.stack([CR.condition(x[s], self.corr[s], self.fmt) for s in range(self.ref.n_src)])

    def stats_of(self, raw, x, xc):
        """The statistics are taken of the stored rows: of x, before the correction."""
        return [CR.stats(raw[s], self.fmt) for s in range(self.ref.n_src)]

    def monitor(self, x, xc):
        """Both monitors read the X of the conditioned input."""
        self.mon.update(xc)

    def stage(self, xc, run=None):
        self.ref.real_rows = self.fmt == "rs16"
        if run is not None:
            return run(self.ref, xc)
        return self.ref.update(xc, keep_float=True, f32=self.f32)

    def update_samples(self, raw, run=None):
        """raw: stored rows of the bank's format, [n_sources][n_frames * H][2] ([n_sources][n_frames * H] for rs16).  Returns
        (I, Q, z) as TunerPaletteRef.update(keep_float=True) -- or what run(ref, x') returns in its place (Stage2Cap.update)."""
        x = self.convert(raw)
        xc = self.correct(x)
        assert xc.dtype == np.int16 and xc.shape == (self.ref.n_src, x.shape[1], 2)
        if self.stats_on:
            self.stats = [CR.add_stats(a, b) for a, b in zip(self.stats, self.stats_of(raw, x, xc))]
        if self.stats_on or any(c != CR.IDENTITY for c in self.corr):
            self.launches += 1                                # the header's "cost": one pre-pass launch in such a call
        self.rows.append(xc)
        self.monitor(x, xc)
        return self.stage(xc, run)

    # reads
    def spectrum(self):
        return self.mon.acc, self.mon.frames

    def rms(self):
        return self.mon.rms()

    def spectrum_model_error(self):
        """(largest amplitude difference of the complex64 spectrum model against float64, peak amplitude) over every call since
        creation, for the configuration the monitor has had throughout."""
        import test_gpu_tuner_monitor as TM
        cfg = (self.mon.n_bins, self.mon.window, self.mon.mode)
        assert self.mon.frames == sum(r.shape[1] for r in self.rows) // self.ref.H, "the spectrum was not on from the first call"
        return TM.reference(self.rows, self.ref.n_src, self.ref.R, [cfg], real=self.fmt == "rs16")[1:]


def conditioned(raw, fmt, corrections):
    """x' of stored rows [n_sources][n]...: condition(to_cs16(raw)) per source, int16 [n_sources][n][2]."""
    return np.stack([CR.condition(FM.to_cs16(raw[s], fmt), corrections[s], fmt) for s in range(len(corrections))])


def integer_bank_update(ref, raw, fmt, corrections):
    """One call of a direct-form or rate bank with a format and corrections: TunerRef.update / TunerRateRef.update of x'.  Those
    paths are integer throughout, so the GPU must give this bit for bit."""
    return ref.update(conditioned(raw, fmt, corrections))
