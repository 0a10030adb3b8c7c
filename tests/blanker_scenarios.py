"""Designed inputs for the impulse noise blanker (AudioSDR.cpp:606-650; oracle/asdr_oracle.c nb_process; the chain kernels' byte-code
restatement in audiosdr_amd/csrc/asdr_kernels.hip), shared by tests/test_blanker_scenarios.py (which shows on the CPU, against the oracle,
that every recipe reaches the seam it names) and tests/test_gpu_blanker.py / tests/test_gpu_state.py (which hold the launch forms to the
oracle bit for bit on these rows).

A recipe is int16 I/Q rows [U][T][128] -- a quiet background (a weak tone plus noise, synth.make_iq with impulse_every=0) with disturbances
ADDED in the int16 domain and clipped --, the blanker setters it needs (helpers.S) and a script {block: setters}.  scenario() turns a
recipe into a four_wave_scenarios.Scenario for a bank of n channels (channel c gets row c % U) with the settings of a launch form in front.

The blanker comes first in the chain and the input gain stays 1.0, so what it does to a row depends on the row and on the blanker's own
setters only: the claims shown for a recipe hold in every demodulation mode and launch form.

Coordinates.  The call that takes input block t has block t as its NEWEST block [256, 384), block t-1 as the MIDDLE one [128, 256) -- the one
it scans, together with samples 78..127 of the OLDEST block t-2, which it outputs.  A disturbance at sample p of block b is therefore first
scanned by call b+1 at i = 128 + p and, for p >= 78, again by call b+2 at i = p.  The batch-wide ring phase is the call's index mod 3.

Restatement is the channel-vectorised numpy form of nb_process used for the claims: it records, per call, the detection flags of
i = 78..255, the trailing edges found at i = 128..255, the mask of the output block and the mask [128, 266) carried to the next call.  Its
`variant` argument switches on one deliberately wrong blanker (VARIANTS)."""
import ctypes
import ctypes.util

import numpy as np

import four_wave_scenarios as F
from cases import USB, AM
from helpers import S

WARM = 10                                   # the average starts at 10.0 (AudioSDR.h:242): 10 x 0.995^(178 x 10) = 1.3e-3 -- settled
T_STD = 24
EVENTS = (12, 16, 20)                       # blocks = ring phases 0, 1, 2, four blocks apart: a bump of the average has decayed by 0.41^4
PIPE_EVENTS = (9, 17, 25)                   # ... the same at the boundaries of calls of 9, 8, 8 and 8 blocks (phases 0, 2, 1)
T_PIPE = 33
STRONG = (20000, -16000)                    # added to (I, Q): |.| = 0.78 of full scale on a background of 0.05
BG_A, BG_NOISE = 0.05, 0.002                # the envelope stays within 6 % of the tone: quiet at every threshold >= 1.2
TRANS = np.array([0.933, 0.750, 0.500, 0.250, 0.067, 0.000, 0.000], np.float32)
MASK_VALUES = (0.0, 1.0, 0.933, 0.75, 0.5, 0.25, 0.067)
_ALPHA = np.float32(0.995)
_BETA = np.float32(1.0 - float(_ALPHA))
_powf = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").powf
_powf.argtypes = [ctypes.c_float, ctypes.c_float]; _powf.restype = ctypes.c_float

VARIANTS = ("window9", "no_rescan", "edge_misses_128", "ramp_not_below_128", "counts_saturate_127", "carried_spill_dropped",
            "no_average_on_rescan")


def threshold_of(meth, v):
    """the float the setter leaves in the threshold (AudioSDR.cpp:663-674)"""
    if meth == "setNoiseBlankerThreshold":
        return np.float32(v)
    return np.float32(_powf(10.0, np.float32(float(v) / 20.0)))


def fast_sqrt1(x):
    """fast_sqrt_f32(x, 1) (AudioSDR.h:460-476) on a float32 array"""
    x = np.ascontiguousarray(x, np.float32)
    i = x.view(np.uint32).astype(np.uint64)
    i = ((((i - (1 << 23)) & 0xFFFFFFFF) >> 1) + (1 << 29)) & 0xFFFFFFFF
    out = i.astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        return (0.5 * (out + x / out).astype(np.float64)).astype(np.float32)


class Restatement:
    """nb_process for K independent channels at once.  step(sI, sQ) takes the scaled block [K][128] and returns the blanker's output; the
    records of the call are left in .det [K][178] (i = 78..255), .edges [K][128] (i = 128..255), .spill [K] (a zero in mask[256..265]
    before the shift), .out_mask [K][128], .carry_nontrivial [K] (mask[128..265] after the call is not all ones), .detected [K]."""

    def __init__(self, K, variant=None):
        assert variant is None or variant in VARIANTS
        self.K, self.variant = K, variant
        self.hi = np.zeros((K, 384), np.float32); self.hq = np.zeros((K, 384), np.float32)
        self.mask = np.ones((K, 384), np.float32)
        self.avg = np.full(K, 10.0, np.float32); self.thr = np.full(K, 1.2, np.float32)
        self.en = np.ones(K, bool); self.detected = np.zeros(K, np.int64)
        self.det = np.zeros((K, 178), bool); self.edges = np.zeros((K, 128), bool); self.spill = np.zeros(K, bool)
        self.out_mask = np.ones((K, 128), np.float32); self.carry_nontrivial = np.zeros(K, bool)

    def _reset(self, rows):
        self.hi[rows] = 0.0; self.hq[rows] = 0.0; self.mask[rows] = 1.0

    def setter(self, rows, meth, args):
        if meth in ("setNoiseBlankerThreshold", "setNoiseBlankerThresholdDb"):
            self.thr[rows] = threshold_of(meth, args[0]); self._reset(rows)
        elif meth == "enableNoiseBlanker":
            self.en[rows] = True; self._reset(rows)
        elif meth == "disableNoiseBlanker":
            self.en[rows] = False

    def step(self, sI, sQ):
        v = self.variant
        oI, oQ = np.array(sI, np.float32), np.array(sQ, np.float32)
        e = np.flatnonzero(self.en)
        self.det[:] = False; self.edges[:] = False; self.spill[:] = False; self.out_mask[:] = 1.0
        if e.size == 0:
            return oI, oQ
        hi, hq, mask, avg, thr = self.hi[e], self.hq[e], self.mask[e], self.avg[e], self.thr[e]
        hi[:, :256] = hi[:, 128:]; hi[:, 256:] = sI[e]
        hq[:, :256] = hq[:, 128:]; hq[:, 256:] = sQ[e]
        mask[:, :256] = mask[:, 128:]; mask[:, 256:] = 1.0
        if v == "carried_spill_dropped":
            mask[:, 128:138] = 1.0
        mag = fast_sqrt1(hi[:, 78:256] * hi[:, 78:256] + hq[:, 78:256] * hq[:, 78:256])
        det = np.zeros((e.size, 178), bool)
        count = np.zeros(e.size, np.int64)
        w = 9 if v == "window9" else 10
        for t in range(50 if v == "no_rescan" else 0, 178):
            i = 78 + t
            d = mag[:, t] > avg * thr
            det[:, t] = d
            z = d & (count < 127) if v == "counts_saturate_127" else d
            count += d
            r = np.flatnonzero(z)
            if r.size:
                mask[r, i - w:i + w + 1] = 0.0
            if not (v == "no_average_on_rescan" and i < 128):
                avg = _ALPHA * avg + _BETA * mag[:, t]
        spill = (mask[:, 256:266] == 0.0).any(axis=1)
        edges = np.zeros((e.size, 128), bool)
        for i in range(129 if v == "edge_misses_128" else 128, 256):
            ed = (mask[:, i] == 1.0) & (mask[:, i - 1] == 0.0)
            edges[:, i - 128] = ed
            r = np.flatnonzero(ed)
            if r.size:
                lo = max(i - 7, 128) if v == "ramp_not_below_128" else i - 7
                mask[r, lo:i] = TRANS[lo - (i - 7):]
        oI[e] = mask[:, :128] * hi[:, :128]; oQ[e] = mask[:, :128] * hq[:, :128]
        self.hi[e], self.hq[e], self.mask[e], self.avg[e] = hi, hq, mask, avg
        self.det[e], self.edges[e], self.spill[e], self.out_mask[e] = det, edges, spill, mask[:, :128]
        self.detected[e] = det.any(axis=1)
        self.carry_nontrivial = (self.mask[:, 128:266] != 1.0).any(axis=1)
        return oI, oQ


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def background(U, T, A=BG_A, noise=BG_NOISE, seed0=12345):
    """[U][T * 128] int32 I and Q: cases.imp's tone (a carrier offset per row), weak, plus noise"""
    from audiosdr_amd.synth import make_iq
    I, Q = make_iq(U, T, fc=6290.0 + 25.0 * (np.arange(U) % 8), A=A, noise=noise, impulse_every=0, seed0=seed0)
    return I.reshape(U, -1).astype(np.int32), Q.reshape(U, -1).astype(np.int32)


def _finish(I, Q):
    U = I.shape[0]
    I = np.clip(I, -32768, 32767).astype(np.int16).reshape(U, -1, 128); Q = np.clip(Q, -32768, 32767).astype(np.int16).reshape(U, -1, 128)
    I.setflags(write=False); Q.setflags(write=False)
    return I, Q


def _strong(I, Q, row, t0, length=1):
    I[row, t0:t0 + length] += STRONG[0]; Q[row, t0:t0 + length] += STRONG[1]


class Recipe:
    def __init__(self, name, make, setup=(), script=None, facts=None):
        self.name, self._make, self.setup, self.script, self.facts = name, make, list(setup), dict(script or {}), dict(facts or {})
        self._rows = None

    def rows(self):
        if self._rows is None:
            self._rows = self._make()
        return self._rows

    @property
    def U(self):
        return self.rows()[0].shape[0]

    @property
    def T(self):
        return self.rows()[0].shape[1]


def _positions_rows():
    I, Q = background(128, T_STD)
    for p in range(128):
        for b in EVENTS:
            _strong(I, Q, p, b * 128 + p)
    return _finish(I, Q)


PAIR_D = (1, 7, 10, 11, 20, 21, 22, 28, 29)
PAIR_P0 = (3, 70, 77, 100, 117, 120, 127)


def pair_row(d, p0):
    return PAIR_D.index(d) * len(PAIR_P0) + PAIR_P0.index(p0)


def _pairs_rows():
    I, Q = background(64, T_STD)                 # 63 pairs and one quiet row
    for d in PAIR_D:
        for p0 in PAIR_P0:
            for b in EVENTS:
                _strong(I, Q, pair_row(d, p0), b * 128 + p0); _strong(I, Q, pair_row(d, p0), b * 128 + p0 + d)
    return _finish(I, Q)


RUN_L = (2, 21, 64, 128, 178, 300)
RUN_START = (5, 100, 120)
RUNS = [(L, s) for L in RUN_L for s in RUN_START] + [(7, 124), (45, 90), (11, 0), (250, 60)]
RUN_BLOCK = 11
STEP_AT = 12 * 128 + 40
STEP_UP_ROW, STEP_DOWN_ROW, STEP_TWICE_ROW = len(RUNS), len(RUNS) + 1, len(RUNS) + 2
STEP_FACTOR = 10.0
STEP_TWICE = ((6 * 128, 8.0), (14 * 128 + 60, 16.0))     # (from this sample on, the tone at this many times BG_A): 0.05 -> 0.4 -> 0.8


def _runs_rows():
    U = len(RUNS) + 3
    I, Q = background(U, T_STD)
    for r, (L, s) in enumerate(RUNS):
        _strong(I, Q, r, RUN_BLOCK * 128 + s, L)
    hI, hQ = background(U, T_STD, A=BG_A * STEP_FACTOR)          # the same carriers and noise, ten times the tone
    I[STEP_UP_ROW, STEP_AT:] = hI[STEP_UP_ROW, STEP_AT:]; Q[STEP_UP_ROW, STEP_AT:] = hQ[STEP_UP_ROW, STEP_AT:]
    I[STEP_DOWN_ROW, :STEP_AT] = hI[STEP_DOWN_ROW, :STEP_AT]; Q[STEP_DOWN_ROW, :STEP_AT] = hQ[STEP_DOWN_ROW, :STEP_AT]
    # a step onto an average that is already half the new level: the average passes level / 1.2 about 219 samples later, INSIDE the scan
    # whose first 151 samples are detections -- the samples behind the 127th are detected by that scan only, not by their second one
    for t0, f in STEP_TWICE:
        hI, hQ = background(U, T_STD, A=BG_A * f)
        I[STEP_TWICE_ROW, t0:] = hI[STEP_TWICE_ROW, t0:]; Q[STEP_TWICE_ROW, t0:] = hQ[STEP_TWICE_ROW, t0:]
    return _finish(I, Q)


def dense_noise(U, T, seed):
    """[U][T * 128] int32 I, Q of noise alone: make_iq's noise (0.03) times 1 or, on a random 8 % of the samples, 25 -- heavy-tailed, so
    that ratio 2.0 is crossed in every block too -- and, once per row (from a sample of its own in one of the blocks 12..17 on), 185
    samples of random phase whose modulus starts at 0.15, above twice the average, and doubles every 69 samples: the average (time
    constant 200 samples) trails it by a factor of 3 -- every sample of a scan is a detection, at ratio 2.0 as well -- and the surge ends
    below the spikes' reach, which stand out again at once."""
    from audiosdr_amd.synth import make_iq
    nI, nQ = make_iq(U, T, A=0.0, noise=0.03, seed0=777 + seed)
    rng = np.random.default_rng(seed)
    scale = np.where(rng.random((U, T * 128)) < 0.08, 25.0, 1.0)
    I, Q = np.trunc(nI.reshape(U, -1) * scale), np.trunc(nQ.reshape(U, -1) * scale)
    modulus = 32767.0 * 0.15 * 2.0 ** (np.arange(185) / 69.0)
    for r in range(U):
        t0 = (12 + r % 6) * 128 + (r * 37) % 128
        phase = rng.random(185) * 2.0 * np.pi
        I[r, t0:t0 + 185] = np.trunc(modulus * np.cos(phase)); Q[r, t0:t0 + 185] = np.trunc(modulus * np.sin(phase))
    return I.astype(np.int32), Q.astype(np.int32)


def _dense_rows():
    return _finish(*dense_noise(16, T_STD, 1))


MARGINAL = (("setNoiseBlankerThreshold", 1.2), ("setNoiseBlankerThreshold", 3.0), ("setNoiseBlankerThresholdDb", 6.0),
            ("setNoiseBlankerThresholdDb", 10.0), ("setNoiseBlankerThresholdDb", 20.0))
MARGINAL_ROWS = 16
MARGINAL_BLOCKS = tuple(range(WARM, T_STD - 2, 2))
MARGINAL_RISE, MARGINAL_DROP = 20, 16        # blocks with an impulse in every row in which the level has just risen / dropped


def marginal_high(thr):
    """the higher of the tone's two levels, in units of BG_A: below the threshold by more than the noise's 6 %, so that the level changes
    themselves are not detected"""
    return 1.1 if thr < 1.9 else 1.5


def marginal_level(blk, thr):
    """the tone's level in block blk: low and high in turns of four blocks, so that the average both rises (blocks 12, 20) and falls (16)"""
    return marginal_high(thr) if (blk // 4) % 2 == 1 else 1.0


def marginal_impulses(row, thr):
    """[(block, sample, g)]: one isolated impulse every second block, whose envelope is g x threshold x the tone's level there.  In most
    blocks at samples below 78 and at 78..127 in turn, g on a grid of 16 steps from 0.85 to 1.15.  In blocks 16 and 20, p samples after
    the level has changed, every row's impulse is at a sample p in 78..127 and g lies between the average (over the level) at its first
    scan, 1 + (H - 1) 0.995^p resp. 1 - (1 - 1 / H) 0.995^p, and at its second one, 49 samples later, to which the impulse itself has
    added 0.995^49 x 0.005 x (g x threshold - 1): at a fraction of the way that goes with the row."""
    H, own = marginal_high(thr), 0.995 ** 49 * 0.005 * (float(thr) - 1.0)
    out = []
    for k, b in enumerate(MARGINAL_BLOCKS):
        if b in (MARGINAL_RISE, MARGINAL_DROP):
            p = 78 + (3 * row) % 50
            d = (H - 1.0 if b == MARGINAL_DROP else -(1.0 - 1.0 / H))
            first, second = 1.0 + d * 0.995 ** p, 1.0 + d * 0.995 ** (p + 49) + own
            out.append((b, p, first + (second - first) * (row + 0.5) / MARGINAL_ROWS))
            continue
        p = (11 + 9 * row + 5 * k) % 67 if (k + row) % 2 == 0 else 78 + (7 * row + 11 * k) % 50
        out.append((b, p, 0.85 + 0.3 * ((5 * row + 3 * k) % 16) / 15.0))
    return out


def _marginal_rows(thr):
    def make():
        U = MARGINAL_ROWS
        I, Q = background(U, T_STD)
        hI, hQ = background(U, T_STD, A=BG_A * marginal_high(thr))
        for b in range(T_STD):
            if marginal_level(b, thr) != 1.0:
                I[:, b * 128:(b + 1) * 128] = hI[:, b * 128:(b + 1) * 128]; Q[:, b * 128:(b + 1) * 128] = hQ[:, b * 128:(b + 1) * 128]
        for r in range(U):
            for b, p, g in marginal_impulses(r, thr):
                t = b * 128 + p
                i0, q0 = float(I[r, t]), float(Q[r, t])
                k = g * float(thr) * BG_A * marginal_level(b, thr) * 32767.0 / np.hypot(i0, q0)      # along the background's own sample
                I[r, t] += int(np.trunc((k - 1.0) * i0)); Q[r, t] += int(np.trunc((k - 1.0) * q0))
        return _finish(I, Q)
    return make


WAVE_ROWS = tuple(range(0, 64, 9))           # row 9 k: lane k of wave k
WAVE_HITS = ((12, None), (14, 120), (16, None), (20, None))   # (block, sample; None: a sample of the row's own)


def _wave_rows():
    I, Q = background(64, T_STD)
    for r in WAVE_ROWS:
        for b, p in WAVE_HITS:
            _strong(I, Q, r, b * 128 + ((r * 13 + 5) % 128 if p is None else p))
    return _finish(I, Q)


def _wave_off(c):
    return c % 8 == (c // 8 + 1) % 8


def _setter_rows(events, T):
    """rows 0..7: dense noise; rows 8..15: the background with 64 strong samples from sample 100 + row of the block two in front of every
    event on -- the run's window is in the carried mask when the setter arrives"""
    def make():
        I, Q = dense_noise(16, T, 2)
        bI, bQ = background(16, T)
        I[8:], Q[8:] = bI[8:], bQ[8:]
        for r in range(8, 16):
            for ev in events:
                _strong(I, Q, r, (ev - 2) * 128 + 100 + (r - 8), 64)
        return _finish(I, Q)
    return make


SETTER_KINDS = {"ratio": lambda away, back: [S("setNoiseBlankerThreshold", 1.5)],
                "db": lambda away, back: [S("setNoiseBlankerThresholdDb", 6.0)],
                "off-on": lambda away, back: [S("disableNoiseBlanker"), S("enableNoiseBlanker")],
                "mode": lambda away, back: [S("setDemodMode", away), S("setDemodMode", back)]}


def setter_recipe(kind, pipe=False, mode=USB):
    events, T = (PIPE_EVENTS, T_PIPE) if pipe else (EVENTS, T_STD)
    away = AM if mode != AM else USB
    return Recipe("setter-%s%s" % (kind, "-pipe" if pipe else ""), _ROWS[("setter", pipe)],
                  script={ev: SETTER_KINDS[kind](away, mode) for ev in events}, facts=dict(events=events))


class _Shared:
    """rows made once and handed to every recipe that names them"""

    def __init__(self, make):
        self.make, self.rows = make, None

    def __call__(self):
        if self.rows is None:
            self.rows = self.make()
        return self.rows


_ROWS = {}
_DENSE = _Shared(_dense_rows)
_WAVE = _Shared(_wave_rows)
for _pipe, _ev, _t in ((False, EVENTS, T_STD), (True, PIPE_EVENTS, T_PIPE)):
    _ROWS[("setter", _pipe)] = _Shared(_setter_rows(_ev, _t))

POSITIONS = Recipe("positions", _positions_rows)
PAIRS = Recipe("pairs", _pairs_rows)
RUNS_RECIPE = Recipe("runs", _runs_rows)
DENSE = [Recipe("dense-1.2", _DENSE), Recipe("dense-2.0", _DENSE, setup=[S("setNoiseBlankerThreshold", 2.0)])]
MARGINALS = [Recipe("marginal-%s%g" % ("db" if m.endswith("Db") else "x", v), _marginal_rows(threshold_of(m, v)), setup=[S(m, v)],
                    facts=dict(threshold=threshold_of(m, v))) for m, v in MARGINAL]
ONE_IN_A_WAVE = [Recipe("one-in-a-wave-broadcast", _WAVE, setup=[S("setNoiseBlankerThreshold", 1.5)]),
                 Recipe("one-in-a-wave-thresholds", _WAVE, setup=[S("setNoiseBlankerThreshold", 1.5, sel=lambda c: c % 2 == 0),
                                                                  S("setNoiseBlankerThreshold", 3.0, sel=lambda c: c % 2 == 1)]),
                 Recipe("one-in-a-wave-off-lanes", _WAVE, setup=[S("setNoiseBlankerThreshold", 1.5, sel=lambda c: c % 2 == 0),
                                                                 S("setNoiseBlankerThreshold", 3.0, sel=lambda c: c % 2 == 1),
                                                                 S("disableNoiseBlanker", sel=_wave_off)])]
SETTERS = [setter_recipe(k) for k in SETTER_KINDS]
SETTERS_PIPE = [setter_recipe(k, pipe=True) for k in SETTER_KINDS]


# block counts after which tests/test_gpu_state.py cuts a bank: ring phases 0, 1, 2 (in some order), the carried mask of every disturbed row not
# all ones (pairs: two calls behind each event block, whose call scans the pair)
STATE_CUTS = {"dense-1.2": (13, 14, 15), "pairs": tuple(b + 2 for b in EVENTS)}


def all_recipes():
    return [POSITIONS, PAIRS, RUNS_RECIPE] + DENSE + MARGINALS + ONE_IN_A_WAVE + SETTERS + SETTERS_PIPE


def every_form():
    """the recipes that go through every launch form"""
    return [POSITIONS, PAIRS] + DENSE


def scenario(recipe, n=None, front=(), behind=(), expect="off", **kw):
    """the recipe on a bank of n channels (default: its own U rows), the launch form's settings in front of the recipe's and `behind` them"""
    n = recipe.U if n is None else n
    return F.Scenario(recipe.name, recipe.rows, list(front) + recipe.setup + list(behind), recipe.script, n=n, expect=expect, **kw)
