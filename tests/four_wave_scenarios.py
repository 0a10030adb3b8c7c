"""Scenario definitions for the four-wave chain kernels (asdr_update_kernel_mw_u / asdr_update_kernel_mw): settings scripts, input
recipes and seeds, shared by tests/test_gpu_four_wave.py (which runs them on the GPU against the oracle) and
tests/test_four_wave_scenarios.py (which shows on the CPU that they reach the regimes and the launch forms they claim).

A scenario is a bank of `n` channels, `U` distinct input rows (channel c gets row c % U), a list of setters applied before the first
block and a script {block: setters} applied in front of that block.  A setter is helpers.S(method, *args, sel=None): sel = None is a
BROADCAST call (one call for the whole bank -- what keeps a group on the launch-constant form), a predicate sel(c) means one call per
selected channel.  `expect(block)` names the launch form of that block:
    "u"   asdr_update_kernel_mw_u alone (one direct group, equal rows)
    "r"   asdr_update_kernel_mw alone   (one direct group, rows that differ)
    "off" neither (the plain kind's uniform part is no direct group)
or a dict {kernel: launches per block} where other kernels run beside them (remainders, SAM)."""
import numpy as np

from cases import LSB, USB, CW_LSB, CW_USB, AM, SAM, WSPR, tone, am, imp, two, CASES
from helpers import S

MW_U, MW = "asdr_update_kernel_mw_u", "asdr_update_kernel_mw"
MIXED = "asdr_update_kernel_mixed"
SAM_KERNELS = ("asdr_sam_pre_kernel_uniform", "asdr_sam_pll_kernel", "asdr_sam_post_kernel_uniform")
N = 512                                   # 64 waves: the smallest direct group that takes the four-wave form (16 workgroups)
MID = 7 * 32 + 13                         # a channel in the middle of a workgroup (wave 1 of workgroup 7)
HANG_COUNTS = (0, 1, 127, 128, 129, 255, 256, 4410)


def hang_ms(count):
    """a hang time whose sample count (float product, / 1000.0, truncated: AudioSDR.cpp:563-566) is `count`"""
    return 0.0 if count == 0 else float(np.float32((count + 0.5) / 44.1))


class Scenario:
    def __init__(self, name, rows, setup, script=None, n=N, expect="u", taps=False, plain_waves=None, uniform_groups=None, direct_slots=None):
        self.name, self.rows, self.setup, self.script, self.n, self.taps = name, rows, list(setup), dict(script or {}), n, taps
        self._expect = expect
        self.plain_waves = (n + 7) // 8 if plain_waves is None else plain_waves     # control_plane_flush()["waves_plain"]
        self._uniform_groups, self._direct_slots = uniform_groups, direct_slots

    def expect(self, blk):
        return self._expect(blk) if callable(self._expect) else self._expect

    def census(self, blk, launches=1):
        e = self.expect(blk)
        if e == "off":
            return None
        return {k: v * launches for k, v in ({MW_U: 1} if e == "u" else {MW: 1} if e == "r" else e).items()}

    def uniform_groups(self, blk):
        """params_uniform_groups()[0] in front of block blk"""
        if self._uniform_groups is not None:
            return self._uniform_groups
        return 1 if self.expect(blk) == "u" else 0

    def direct_slots(self, blk):
        """channels in direct groups (what one pass over the groups' rows compares) in front of block blk"""
        if self._direct_slots is not None:
            return self._direct_slots
        return 0 if self.expect(blk) == "off" else self.n // 8 * 8

    def all_setters(self):
        """[(block or -1, setter)] in the order they are applied"""
        return [(-1, s) for s in self.setup] + [(blk, s) for blk in sorted(self.script) for s in self.script[blk]]

    def channel_keys(self, U):
        """per channel: (input row, indices of the setters that reach it).  Channels with equal keys share one oracle."""
        sigs = [[] for _ in range(self.n)]
        for j, (_b, s) in enumerate(self.all_setters()):
            for c in selected(s[2], self.n):
                sigs[c].append(j)
        return [(c % U, tuple(sigs[c])) for c in range(self.n)]


def selected(sel, n):
    """the channels a setter reaches: sel = None (all: a broadcast), one channel index, or a predicate"""
    if sel is None:
        return range(n)
    if isinstance(sel, int):
        return (sel,)
    return [c for c in range(n) if sel(c)]


def apply_to_batch(b, setters, n):
    for meth, args, sel in setters:
        if sel is None:
            getattr(b, meth)(*args)                     # broadcast: one call
        else:
            for c in selected(sel, n):
                getattr(b, meth)(*args, ch=c)


def apply_to_oracle(o, meth, args):
    if meth == "set_exact_unknown_mode":                # the product's opt-out and the oracle's model of it
        o.set_unknown_mode_silence(not args[0])
    else:
        getattr(o, meth)(*args)


class OracleRun:
    """One oracle per distinct channel key, stepped block by block through the scenario's calls."""

    def __init__(self, ao, sc, bI, bQ, taps_for=None, observe_agc=False):
        U, T = bI.shape[0], bI.shape[1]
        self.keys = sc.channel_keys(U)
        uniq = sorted(set(self.keys))
        self.index = {k: i for i, k in enumerate(uniq)}
        self.of_channel = np.array([self.index[k] for k in self.keys])
        tap_keys = set() if taps_for is None else {self.keys[c] for c in taps_for}
        allset = sc.all_setters()
        self.audio = np.empty((len(uniq), T, 128), np.int16)
        self.taps = {}                                   # key index -> [T][12][128] float32
        self.oracles = []
        self.status = {}                                 # block -> {key index: status words} (filled by a subclass's after_block)
        if observe_agc:                                  # at the START of every block: hang counter, envelope; of the block: max |AGC input| clamped to 1
            self.hc0 = np.zeros((len(uniq), T), np.int64); self.env0 = np.zeros((len(uniq), T), np.float32)
            self.bmax = np.zeros((len(uniq), T), np.float32); self.hc_end = np.zeros((len(uniq), T), np.int64)
        for k in uniq:
            i = self.index[k]
            want_taps = k in tap_keys or observe_agc
            o = ao.OracleSDR(taps=want_taps)
            if k in tap_keys:
                self.taps[i] = np.empty((T, 12, 128), np.float32)
            row, sig = k
            calls = {}
            for j in sig:                                # (in the order the batch gets them: the setup, then block 0's script, ...)
                calls.setdefault(max(allset[j][0], 0), []).append(allset[j][1])
            for blk in range(T):
                for s in calls.get(blk, ()):
                    apply_to_oracle(o, s[0], s[1])
                if observe_agc:
                    self.hc0[i, blk], self.env0[i, blk] = o.agc_running()
                self.audio[i, blk] = o.update(bI[row, blk], bQ[row, blk])
                if observe_agc:
                    self.bmax[i, blk] = np.minimum(np.abs(o.tap("AUDIO_FILT")), np.float32(1.0)).max()
                    self.hc_end[i, blk] = o.agc_running()[0]
                if k in tap_keys:
                    for t, name in enumerate(ao.TAPS):
                        self.taps[i][blk, t] = o.tap(name)
                self.after_block(i, blk, o)
            self.oracles.append(o)

    def after_block(self, i, blk, o):
        """hook: oracle o of key index i has just processed block blk"""

    def want(self):
        return self.audio[self.of_channel]               # [n][T][128]

    def channel_oracles(self):
        return [self.oracles[i] for i in self.of_channel]


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def signal_rows(total, sig, U=8, noise=0.02, **kw):
    """U input rows of one of tests/cases.py's signals: a carrier offset of its own per row, a little noise"""
    from audiosdr_amd.synth import make_iq
    p = dict(sig); p.update(kw)
    fc = p.pop("fc") + 25.0 * np.arange(U)
    p.setdefault("noise", noise)
    return make_iq(U, total, fc=fc, **p)


def shaped_rows(total, level, detune, U=16, fc0=6290.0, noise=0.0008):
    """a carrier per row (its own offset, plus detune[row][sample] Hz: phase-continuous) times level[row][sample], plus a little noise"""
    from audiosdr_amd.synth import make_iq
    nI, nQ = make_iq(U, total, A=0.0, noise=noise)
    f = (fc0 + 25.0 * np.arange(U))[:, None] + detune
    ph = 2.0 * np.pi * np.cumsum(f, axis=1) / 44100.0
    I = np.trunc(32767.0 * level * np.cos(ph)) + nI.reshape(U, -1)
    Q = np.trunc(32767.0 * level * np.sin(ph)) + nQ.reshape(U, -1)
    I = np.clip(I, -32768, 32767).astype(np.int16); Q = np.clip(Q, -32768, 32767).astype(np.int16)
    return I.reshape(U, total, 128), Q.reshape(U, total, 128)


AGC_BLOCKS = 48
AGC_BURSTS = (8, 11, 15, 18, 22, 27, 30, 34, 37, 41, 44)     # first block of each burst; the tail behind it lasts until the next one
OUT_OF_BAND = 8000.0                                          # Hz: from the audio passband into the IF filter's stop band


def agc_rows(total=AGC_BLOCKS, U=16):
    """Blocks 0..7: a carrier with deep slow modulation (0.9 at 120 Hz, as cases.py's agc_slow_hang): attacks on the crests, hang in the
    troughs.  Then bursts of a little more than one block, each followed by a quiet tail of 2 to 4 blocks; a burst ends at a sample of
    its own in every row (and in every burst), which moves the last attack -- and with it the sample at which a hang counter passes 128
    or runs out -- across the block: inside it, at its end, at the start of the next one.  The next burst is the late attack that re-arms
    the counters still running (hang time 100 ms: 4,410 samples).  Burst and tail are ONE carrier of constant amplitude that leaves the
    passband for the tail: the blanker (on, as in C2: it would gate a step in amplitude as one long impulse) sees a steady magnitude."""
    t = np.arange(total * 128, dtype=np.float64)
    lvl = np.empty((U, total * 128)); det = np.zeros((U, total * 128))
    for r in range(U):
        lvl[r] = 0.12 * (1.0 + 0.9 * np.sin(2.0 * np.pi * 120.0 * t / 44100.0))
        lvl[r, AGC_BURSTS[0] * 128:] = 0.2
        det[r, AGC_BURSTS[0] * 128:] = OUT_OF_BAND
        for k, b0 in enumerate(AGC_BURSTS):
            det[r, b0 * 128:(b0 + 1) * 128 + (r * 37 + k * 53) % 128] = 0.0
    return shaped_rows(total, lvl, det)


def agc_default_rows(total=46):
    """the level drops for good after 4 blocks: the default hang counter (4,410) crosses 128 and runs out around block 41 of a fresh bank"""
    U = 16
    lvl = np.full((U, total * 128), 0.2); det = np.full((U, total * 128), OUT_OF_BAND)
    for r in range(U):
        det[r, :4 * 128 + (r * 37) % 128] = 0.0
    return shaped_rows(total, lvl, det)


def pattern_rows(n_blk=10):
    """the five patterns of test_pathological_inputs, plus silence"""
    t = np.arange(n_blk * 128)
    pats = [
        (np.where((t // 3) % 2 == 0, 32767, -32768), np.where((t // 5) % 2 == 0, -32768, 32767)),
        (np.where(t % 2 == 0, 32767, -32767), np.where(t % 2 == 0, -32767, 32767)),
        (np.full_like(t, 12345), np.full_like(t, -23456)),
        (np.where(t % 257 == 0, 32767, 0), np.where(t % 263 == 0, -32768, 0)),
        (np.full_like(t, -32768), np.full_like(t, -32768)),
        (np.zeros_like(t), np.zeros_like(t)),
    ]
    I = np.stack([p[0] for p in pats]).astype(np.int16).reshape(len(pats), n_blk, 128)
    Q = np.stack([p[1] for p in pats]).astype(np.int16).reshape(len(pats), n_blk, 128)
    return I, Q


def denormal_rows(mode):
    from audiosdr_amd.synth import make_iq
    I, Q = make_iq(4, 12, fc=(6890.0 if mode != USB else 6290.0) + 25.0 * np.arange(4), A=0.3, m=0.5)
    Z = np.zeros((4, 400, 128), np.int16)
    return np.concatenate([I, Z, I], axis=1), np.concatenate([Q, Z, Q], axis=1)


# ---- the mode and enable matrix -----------------------------------------------------------------------------------------------------
# (mode, blanker, audio filter, AGC, mute) -- every mode twice, the second time with every enable the other way: each mode meets each
# enable on and off; the sixteen rows are the full product of the four enables.
_MODES = [("lsb", LSB, imp), ("usb", USB, two), ("cwl", CW_LSB, dict(fc=7390 - 700.0, A=0.2)), ("cwu", CW_USB, dict(fc=6390 + 700.0, A=0.2)),
          ("am", AM, am), ("wspr", WSPR, dict(fc=6890.0, A=0.05)), ("m7", 7, imp), ("m65535", 65535, two)]
_ENABLES = [(1, 1, 1, 0), (1, 0, 0, 1), (1, 1, 0, 0), (1, 0, 1, 1), (1, 0, 1, 0), (1, 1, 1, 1), (1, 1, 0, 1), (1, 0, 0, 0)]
_AUDIO_FILTER = {"cwl": 1, "cwu": 1, "wspr": 2, "am": 0}       # setAudioFilter where the audio filter is on (10, the bypass value: in USB's filter-off row)
_ONE_ROW = [S("setOutputGain", 0.7), S("setInputGain", 2.0), S("setIQgainBalance", 1.03), S("setNoiseBlankerThreshold", 3.0),
            S("setAGCstaticGain", 20.0), S("setAGCattackTime", 3.0), S("setAGChangTime", 5.0), S("setAGCreleaseTime", 200.0)]
MATRIX_BLOCKS = 8


def matrix_configs():
    out = []
    for k, (mname, mode, sig) in enumerate(_MODES):
        for flip in (0, 1):
            nb, af, agc, mute = [e ^ flip for e in _ENABLES[k]]
            out.append((mname, mode, sig, nb, af, agc, mute, len(out)))
    return out


def matrix_scenario(cfg, rows_differ):
    mname, mode, sig, nb, af, agc, mute, idx = cfg
    unknown = not (0 <= mode <= 6)
    setup = [S("setDemodMode", USB if unknown else mode)]
    setup.append(S("enableNoiseBlanker") if nb else S("disableNoiseBlanker"))
    if af:
        setup.append(S("enableAudioFilter"))
        if mname in _AUDIO_FILTER:
            setup.append(S("setAudioFilter", _AUDIO_FILTER[mname]))
    elif mname == "usb":                                # the bypass value switches the audio filter off again (AudioSDR.cpp:298-311)
        setup += [S("enableAudioFilter"), S("setAudioFilter", 10)]
    if agc:
        setup.append(S("setAGCmode", 1 + idx % 3))
    else:
        setup.append(S("setAGCmode", 0) if idx % 4 == 1 else S("disableAGC"))
    if mute:
        setup.append(S("setMute", 1))
    script = {}
    if unknown:                                         # three blocks of USB leave the row an unknown mode value keeps re-processing
        script[3] = [S("setDemodMode", mode)]
        if mname == "m7" and not mute:
            setup.append(S("set_exact_unknown_mode", False))
    if mute:                                            # ... and the state carried through the muted blocks is heard afterwards
        script.setdefault(5, []).append(S("setMute", 0))
    if rows_differ:
        m, a, _ = _ONE_ROW[idx % len(_ONE_ROW)]
        setup.append(S(m, *a, sel=MID))
    name = "%s-nb%d-af%d-agc%d-mute%d-%s" % (mname, nb, af, agc, mute, "rows" if rows_differ else "uniform")
    return Scenario(name, lambda: signal_rows(MATRIX_BLOCKS, sig, impulse_every=sig.get("impulse_every", 1300)), setup, script,
                    expect="r" if rows_differ else "u")


# ---- rows that differ inside one direct group ---------------------------------------------------------------------------------------
_P_IN = (1.0, 0.5, 2.0, 3.3, 0.8)                       # index c % 5
_P_BAL = (1.0, 1.02, 0.98, 1.0, 1.05, 0.95, 1.01)       # c % 7
_P_OUT = (0.5, 0.7, 0.9)                                # c % 3
_P_NB = (("setNoiseBlankerThreshold", 3.0), ("setNoiseBlankerThresholdDb", 10.0), ("setNoiseBlankerThreshold", 5.0), ("setNoiseBlankerThresholdDb", 6.0))   # c % 4
_P_STATIC = (10.0, 15.0, 20.0, 25.0, 12.0, 17.0, 22.0, 27.0, 30.0, 8.0, 5.0)    # c % 11
_P_ATTACK = (5.0, 2.0, 10.0)                            # (c // 3) % 3
_P_RELEASE = (500.0, 100.0, 250.0, 50.0, 20.0)          # (c // 5) % 5
_P_HANG = (100.0, hang_ms(127), 0.0, hang_ms(128), 20.0, hang_ms(1), 500.0)     # (c // 7) % 7
ROWS_BLOCKS = 10
CUT = 8 * 33                                            # a multiple of 8, not of 32: workgroup 8 holds waves of both halves


def channel_settings(c):
    """the settings of channel c in the every-row-differs bank, as (method, value) pairs"""
    return (("setInputGain", _P_IN[c % 5]), ("setIQgainBalance", _P_BAL[c % 7]), ("setOutputGain", _P_OUT[c % 3]), _P_NB[c % 4],
            ("setAGCstaticGain", _P_STATIC[c % 11]), ("setAGCattackTime", _P_ATTACK[(c // 3) % 3]), ("setAGCreleaseTime", _P_RELEASE[(c // 5) % 5]),
            ("setAGChangTime", _P_HANG[(c // 7) % 7]))


def rows_scenarios():
    rows = lambda: signal_rows(ROWS_BLOCKS, imp, impulse_every=333)
    c2 = [S("setDemodMode", USB), S("enableAudioFilter")]
    every = list(c2)
    for c in range(N):
        for m, v in channel_settings(c):
            every.append(S(m, v, sel=c))
    # The schedule sorts by (kind, mode, flags, IF table, audio table, AGC table, channel): a direct group needs the table indices to
    # ascend with the channel index.  Audio tables are indexed by the filter's id; AGC tables by the order in which their (threshold,
    # slope, knee) first appeared in the batch -- the power-on table is index 0, every later one is higher.
    audio = c2 + [S("setAudioFilter", 3, sel=lambda c: c < CUT), S("setAudioFilter", 8, sel=lambda c: c >= CUT)]
    agc = c2 + [S("setAGCthreshold", -40.0, sel=lambda c: c >= CUT), S("setAGCslope", 0.3, sel=lambda c: c >= CUT), S("setAGCkneeWidth", 6.0, sel=lambda c: c >= CUT)]
    return [Scenario("every-row-differs", rows, every, expect="r"), Scenario("audio-table-halves", rows, audio, expect="r"),
            Scenario("agc-table-halves", rows, agc, expect="r")]


# ---- AGC regimes --------------------------------------------------------------------------------------------------------------------
def _hang_setters(count_of):
    return [S("setAGChangTime", hang_ms(h), sel=lambda c, h=h: count_of(c) == h) for h in HANG_COUNTS if h != 4410]


def agc_count_of(name):
    return {"per-workgroup": lambda c: HANG_COUNTS[(c // 32) % 8],                       # (a) some workgroups lean, others general, in one launch
            "mixed": lambda c: HANG_COUNTS[(c + c // 16) % 8],                            # (b) every wave holds all eight counts (and every count meets every input row)
            "one-per-workgroup": lambda c: 127 if c % 32 == 13 else 4410}[name]          # (c)


def agc_scenarios():
    c2 = [S("setDemodMode", USB), S("enableAudioFilter")]
    out = [Scenario("agc-" + k, agc_rows, c2 + _hang_setters(agc_count_of(k)), expect="r") for k in ("per-workgroup", "mixed", "one-per-workgroup")]
    out += [Scenario("agc-mode%d" % m, agc_rows, c2 + [S("setAGCmode", m)]) for m in (1, 2, 3)]
    out.append(Scenario("agc-default-runs-out", agc_default_rows, c2))
    return out


# ---- settings changing on a running bank --------------------------------------------------------------------------------------------
CHANGING_BLOCKS = 36
_FIELDS = {"setOutputGain": (0.7, 0.61, 0.9, 0.45), "setInputGain": (2.0, 0.5, 1.5, 3.0), "setIQgainBalance": (1.02, 0.97, 1.05),
           "setNoiseBlankerThresholdDb": (10.0, 6.0, 13.0, 8.0), "setAGCstaticGain": (22.0, 17.0, 28.0), "setAGCattackTime": (3.0, 7.0, 1.5),
           "setAGCreleaseTime": (200.0, 350.0, 120.0), "setAGChangTime": (5.0, hang_ms(127), 50.0, 0.0)}
_KEYED = (("setAudioFilter", (3, 5, 8)), ("setAGCthreshold", (-40.0, -50.0)), ("setAGCslope", (0.3, 0.2)), ("setAGCmode", (1, 2, 3)))   # fields of the schedule key: by broadcast only


def changing_scenario(seed):
    """Key fields by broadcast at fixed blocks (blanker off / on, USB -> AM -> CW -> USB, an unknown mode and back), one channel's mode
    away for three blocks, and non-key fields by broadcast or on random single channels in between.  The launch form of every block
    follows from which fields currently hold a channel that differs from the bank."""
    rng = np.random.default_rng(seed)
    script = {4: [S("disableNoiseBlanker")], 8: [S("enableNoiseBlanker")], 10: [S("setDemodMode", AM)], 14: [S("setDemodMode", int(rng.choice([CW_LSB, CW_USB])))],
              18: [S("setDemodMode", USB)], 27: [S("setDemodMode", int(rng.choice([7, 9, 65535])))], 30: [S("setDemodMode", int(rng.choice([USB, LSB])))]}
    away = int(rng.integers(0, N))
    script[21] = [S("setDemodMode", AM, sel=away)]
    script[24] = [S("setDemodMode", USB, sel=away)]
    deviants = {f: set() for f in _FIELDS}
    current = {f: None for f in _FIELDS}
    expect = {}
    for blk in range(CHANGING_BLOCKS):
        if blk >= 1 and blk not in script and rng.random() < 0.6:
            if rng.random() < 0.2:
                m, vals = _KEYED[int(rng.integers(len(_KEYED)))]
                script[blk] = [S(m, vals[int(rng.integers(len(vals)))])]
                if m == "setAGCmode":
                    for f in ("setAGCattackTime", "setAGCreleaseTime", "setAGChangTime"):
                        deviants[f].clear(); current[f] = "mode"
            else:
                f = list(_FIELDS)[int(rng.integers(len(_FIELDS)))]
                vals = [v for v in _FIELDS[f] if v != current[f]]
                v = vals[int(rng.integers(len(vals)))]
                if rng.random() < 0.5 or deviants[f]:       # broadcast (always when a channel differs in this field: the bank comes back)
                    script[blk] = [S(f, v)]
                    deviants[f].clear(); current[f] = v
                    if f == "setInputGain":             # (.cpp:232-238: the I gain is formed with the balance the object was created with, 1.0)
                        deviants["setIQgainBalance"].clear(); current["setIQgainBalance"] = None
                else:
                    k = int(rng.integers(0, N))
                    script[blk] = [S(f, v, sel=k)]
                    deviants[f].add(k)
        expect[blk] = "off" if 21 <= blk < 24 else ("r" if any(deviants.values()) else "u")
    return Scenario("changing-%d" % seed, lambda: signal_rows(CHANGING_BLOCKS, dict(fc=6600.0, A=0.3, m=0.4), impulse_every=777, f2=7300.0, a2=0.1),
                    [S("setDemodMode", USB), S("enableAudioFilter")], script, expect=lambda blk: expect[blk])


# ---- edge inputs --------------------------------------------------------------------------------------------------------------------
def edge_scenarios():
    out = []
    for mname, mode in (("usb", USB), ("cw", CW_USB), ("am", AM)):
        base = [S("setDemodMode", mode), S("enableAudioFilter"), S("setOutputGain", 1.0)]
        out.append(Scenario("patterns-%s-gain1" % mname, pattern_rows, base + [S("setInputGain", 1.0)]))
        out.append(Scenario("patterns-%s-gain4" % mname, pattern_rows, base + [S("setInputGain", 4.0)]))
        out.append(Scenario("patterns-%s-gain1and4" % mname, pattern_rows, base + [S("setInputGain", 4.0, sel=lambda c: c % 2 == 1)], expect="r"))
    n_ch, n_blk, setters, sig = CASES["int16_wrap_no_agc"]
    out.append(Scenario("int16-wrap", lambda: signal_rows(n_blk, sig, noise=0.01), setters))
    return out


def denormal_scenarios():
    """12 signal blocks, 400 silent ones, 12 signal blocks.  A third of the channels releases at once (no hang time, 1 ms release), so
    that their envelopes do fall through the denormals within the silence -- rows that differ: asdr_update_kernel_mw.  (Switching the
    AGC off on a third of the channels changes the enables, a field of the schedule key: such a bank has no direct group and takes
    neither four-wave kernel -- test_four_wave_scenarios.py shows it; the bank with the AGC off everywhere is the third case here.)"""
    out = []
    for mname, mode in (("usb", USB), ("am", AM)):
        base = [S("setDemodMode", mode), S("enableAudioFilter"), S("setNoiseBlankerThresholdDb", 10.0)]
        third = [S("setAGChangTime", 0.0, sel=lambda c: c % 3 == 1), S("setAGCreleaseTime", 1.0, sel=lambda c: c % 3 == 1)]
        out.append(Scenario("denormals-%s-third-releases" % mname, lambda mode=mode: denormal_rows(mode), base + third, expect="r"))
    out.append(Scenario("denormals-usb-agc-off", lambda: denormal_rows(USB), [S("setDemodMode", USB), S("enableAudioFilter"),
                                                                               S("setNoiseBlankerThresholdDb", 10.0), S("disableAGC")]))
    return out


# ---- taps and geometry --------------------------------------------------------------------------------------------------------------
TAP_CHANNELS = sorted(set(range(0, N, 37)) | {N - 1})
TAP_BLOCKS = 6


def tap_scenarios():
    out = []
    for mname, mode, sig in (("usb", USB, imp), ("am", AM, am)):
        base = [S("setDemodMode", mode), S("enableAudioFilter")]
        rows = lambda sig=sig: signal_rows(TAP_BLOCKS, sig, impulse_every=300)
        out.append(Scenario("taps-%s-uniform" % mname, rows, base, taps=True))
        out.append(Scenario("taps-%s-rows" % mname, rows, base + [S("setOutputGain", 0.7, sel=37), S("setInputGain", 2.0, sel=N - 1)],
                            expect="r", taps=True))
    return out


GEOMETRY_BLOCKS = 6


def geometry_scenarios():
    c2 = [S("setDemodMode", USB), S("enableAudioFilter")]
    rows = lambda: signal_rows(GEOMETRY_BLOCKS, imp, impulse_every=500)
    out = [Scenario("n%d" % n, rows, c2, n=n) for n in (520, 528, 536)]
    # 64 whole waves and five channels left over: the remainders' wave runs on the general instantiation beside the four-wave launch
    out.append(Scenario("n517", rows, c2, n=517, expect={MW_U: 1, MIXED: 1}, uniform_groups=1, direct_slots=512))
    am_rows = lambda: signal_rows(GEOMETRY_BLOCKS, am, impulse_every=500)
    sam = [S("setDemodMode", SAM, sel=lambda c: c < 512), S("setDemodMode", USB, sel=lambda c: c >= 512), S("enableAudioFilter")]
    three = {k: 1 for k in SAM_KERNELS}
    out.append(Scenario("sam512-usb512", am_rows, sam, n=1024, expect=dict(three, **{MW_U: 1}), plain_waves=64, uniform_groups=2, direct_slots=1024))
    out.append(Scenario("sam512-usb512-one-row", am_rows, sam + [S("setOutputGain", 0.7, sel=512 + MID)], n=1024,
                        expect=dict(three, **{MW: 1}), plain_waves=64, uniform_groups=1, direct_slots=1024))
    return out


def all_scenarios():
    out = [matrix_scenario(cfg, r) for cfg in matrix_configs() for r in (False, True)]
    out += rows_scenarios() + agc_scenarios() + [changing_scenario(s) for s in CHANGING_SEEDS]
    out += edge_scenarios() + denormal_scenarios() + tap_scenarios() + geometry_scenarios()
    return out


CHANGING_SEEDS = (201, 202, 203, 204)
