"""Designed parameter layouts for the adaptive line suppressor (the ALS notch / peak filter, AudioSDR.cpp:324-352; oracle/asdr_oracle.c
als_process; als_compute in audiosdr_amd/csrc/asdr_kernels.hip), shared by tests/test_als_scenarios.py (which shows on the CPU that the
recipes reach every arithmetic path of als_compute, stay finite, tell wrong filters apart and agree with the reference's own code) and
tests/test_gpu_als.py (which holds every launch form that carries the filter to the oracle bit for bit: audio, taps, history, census).

A recipe is a layout of per-channel filter settings (P) over the eight rows of a wave, a second layout for the five channels a mixed form
appends, and events (block, wave, lane, method, args) applied in front of a block.  Channel c takes input row c % 8 -- a carrier and a
second tone for the filter to lock on (synth.make_iq, A = 0.3, a2 = 0.12), AGC on, T = 10 blocks.  Every recipe exists in two classes:

    compact   every enabled channel has 0 <= M <= 64, D >= 0 and D + M <= 65: the host sends it to the kinds with compact rows (64 history
              samples, 64 taps: ASDR_KERNEL_ALS_SMALL, ASDR_KERNEL_SAM_ALS)
    full      M > 64, D < 0 or D + M > 65: the 516-float rows (ASDR_KERNEL_ALS)

and a form takes the class its kernels are compiled for (FORMS[..].klass).  What a recipe holds in each class -- a row with M > 64 cannot
be in a compact form:

    recipe               compact                                             full
    lengths              M 0 1 2 7 8 9 15 16 17 54 55 56 63 64, D = 1        M 65 100 127 128, D = 0
    lengths_in_one_wave  8 different M (55 among them); 7 x 55 + 1 x 54      the same with D + M >= 66
    delays               M 8 33 55 64 with those of D 0 1 3 65-M 66-M 128-M   ... that do not; (128,0) (128,20) (100,29) (8,121);
                         that fit                                            D -1 -3 (M 8), -5 (M 64)
    kinds                notch / peak x adaptive / static, 55 taps, delay 3  100 taps, delay 7; static taps with D = -3
    lambdas              0 1e-6 0.05 0.5 1.0 on (55, ., 3)                   on (100, ., 7)
    migrations           100 -> 40 -> 100 taps (crosses the classes: in both); 55 -> 8 -> 55; off two blocks; on mid-run; compact: mode away and back
    partly_enabled       channels with the filter off among enabled ones     the same on (100, 0.5, 7)          (mixed forms only)

The launch census of a call is not a table here but a restatement of the host's plan (census(): kernel kind per channel, settings groups,
whole waves and the shared remainder sub-range, the launcher's choice per sub-range: asdr_host.cpp flush_host / plan_launches,
asdr_kernels.hip asdr_launch_update_ordered / asdr_launch_als_role), because migrations move a bank between kernels from call to call.
FORMS[..].stated is what a form launches on a bank that is regular for it (whole waves of enabled channels of its class, plus the five
appended ones in a mixed form); tests/test_als_scenarios.py holds census() to it.

The compact rows have no general instantiation: since the settings groups' remainders share one sub-range (run by
asdr_update_kernel_als_mixed as soon as one of them has the filter on), no sub-range of kind ASDR_KERNEL_ALS_SMALL or ASDR_KERNEL_SAM_ALS
is ever non-uniform.  The two kernels that served such sub-ranges (GONE) had no launch path left and were taken out of the build with
this suite: nothing could have run them, so nothing could have held them to the oracle."""
import numpy as np

from cases import USB, SAM
from helpers import S

T = 10
U = 8
REM = 5                                           # channels a mixed form appends: the shared remainder sub-range
DEFAULT = (55, 0.5, 3)                            # AudioSDR.h:198-200
ALS_SMALL_ONE, ALS_SMALL = "asdr_update_kernel_als_small_one", "asdr_update_kernel_als_small"
ALS_FULL, ALS_MIXED = "asdr_update_kernel_als", "asdr_update_kernel_als_mixed"
ALS_PRE, ALS_PRE_LOOP, ALS_K, ALS_BACK, ALS_SEED = ("asdr_als_pre_kernel", "asdr_als_pre_loop_kernel", "asdr_als_kernel", "asdr_als_back_loop_kernel",
                                                    "asdr_als_stage_seed_kernel")
SAM_PRE_U, SAM_PLL, SAM_POST_U, SAM_POST_ALS_U = ("asdr_sam_pre_kernel_uniform", "asdr_sam_pll_kernel", "asdr_sam_post_kernel_uniform",
                                                  "asdr_sam_post_als_kernel_uniform")
SAM_PRE_LOOP_U, SAM_FUSED = "asdr_sam_pre_loop_kernel_uniform", "asdr_update_kernel_sam"
PLAIN_ONE, PLAIN_LOOP, PLAIN_MIXED = "asdr_update_kernel_one", "asdr_update_kernel", "asdr_update_kernel_mixed"
GONE = ("asdr_update_kernel_als_small_mixed", "asdr_sam_post_als_kernel")
ALS_CHUNK = 8                                     # ASDR_ALS_CHUNK: blocks per launch of the role streams


class P:
    """one channel's filter settings"""

    def __init__(self, M=DEFAULT[0], lam=DEFAULT[1], D=DEFAULT[2], notch=True, adaptive=True, en=True):
        self.M, self.lam, self.D, self.notch, self.adaptive, self.en = M, lam, D, notch, adaptive, en

    def copy(self):
        return P(self.M, self.lam, self.D, self.notch, self.adaptive, self.en)

    def small(self):
        """the host's rule for the compact rows (asdr_host.cpp kernel_kind)"""
        return 0 <= self.M <= 64 and self.D >= 0 and self.D + self.M <= 65

    def in_domain(self):
        """inside the reference's own buffer (outside it the oracle's zero-reading rule is the definition)"""
        return self.D >= 0 and self.M + self.D <= 128

    def key(self):
        return (self.M, self.lam, self.D, self.notch, self.adaptive, self.en)

    def setters(self):
        out = []
        if self.en:
            out.append(("enableALSfilter", ()))
        if (self.M, self.lam, self.D) != DEFAULT:
            out.append(("setALSfilterParams", (self.M, self.lam, float(self.D))))
        if not self.notch:
            out.append(("setALSfilterPeak", ()))
        if not self.adaptive:
            out.append(("setALSfilterStatic", ()))
        return out


def apply(mode, p, meth, args):
    """a setter's effect on a channel's (mode, P): what census() and the reach predicates follow the events with (asdr_host.cpp:2433-2447)"""
    if meth == "enableALSfilter": p.en = True
    elif meth == "disableALSfilter": p.en = False
    elif meth == "setALSfilterNotch": p.notch = True
    elif meth == "setALSfilterPeak": p.notch = False
    elif meth == "setALSfilterAdaptive": p.adaptive = True
    elif meth == "setALSfilterStatic": p.adaptive = False
    elif meth == "setALSfilterParams": p.M, p.lam, p.D = min(int(args[0]), 128), args[1], int(args[2])
    elif meth == "setDemodMode": mode = args[0]
    else: raise KeyError(meth)
    return mode


def W(*ps):
    """a wave: one P for all eight rows, or eight"""
    assert len(ps) in (1, 8)
    return [ps[0].copy() for _ in range(8)] if len(ps) == 1 else [p.copy() for p in ps]


class Recipe:
    def __init__(self, name, klass, waves, rem=None, events=(), every_call=False):
        """events: (block, wave index or "rem", lane or None for the whole wave, method, args); a setDemodMode event's argument is "away" /
        "back": the form's own mode and the other one of USB / SAM"""
        self.name, self.klass, self.waves, self.events, self.every_call = name, klass, waves, list(events), every_call
        self.rem = [p.copy() for p in (rem if rem is not None else waves[0][:REM])]
        assert len(self.rem) == REM and all(0 < e[0] < T for e in self.events)


def _base(klass, **kw):
    return P(*DEFAULT, **kw) if klass == "compact" else P(100, 0.5, 7, **kw)


LENGTHS = {"compact": (0, 1, 2, 7, 8, 9, 15, 16, 17, 54, 55, 56, 63, 64), "full": (65, 100, 127, 128)}


def lengths(klass):
    """one wave per M, uniform inside the wave"""
    return Recipe("lengths", klass, [W(P(M, 0.5, 1 if klass == "compact" else 0)) for M in LENGTHS[klass]])


def lengths_in_one_wave(klass):
    """eight different M in one wave, 55 among them (neither the default nor the uniform path); seven channels at 55 and one at 54"""
    if klass == "compact":
        return Recipe("lengths_in_one_wave", klass, [W(*[P(M, 0.5, 1) for M in (1, 2, 7, 9, 55, 54, 64, 17)]),
                                                    W(*[P(54 if r == 5 else 55, 0.5, 1) for r in range(8)])])
    return Recipe("lengths_in_one_wave", klass, [W(*[P(M, 0.5, D) for M, D in ((65, 0), (100, 0), (55, 11), (128, 0), (127, 0), (33, 33), (8, 58), (64, 2))]),
                                                W(*[P(54 if r == 5 else 55, 0.5, 73) for r in range(8)])])


DELAY_M = (8, 33, 55, 64)
DELAY_PAIRS = ((128, 0), (128, 20), (100, 29), (8, 121))        # the last three read outside the history
DELAY_NEGATIVE = ((8, -1), (8, -3), (64, -5))


def delays(klass):
    """per M one wave and class: D in 0, 1, 3, 65 - M, 66 - M, 128 - M by row, those of the class in turn (M = 64: D = 3 is a full row);
    full: also the pairs and the negative ones"""
    def wave(M):
        ds = [D for D in sorted({0, 1, 3, 65 - M, 66 - M, 128 - M}) if P(M, 0.5, D).small() == (klass == "compact")]
        return W(*[P(M, 0.5, ds[r % len(ds)]) for r in range(8)])
    if klass == "compact":
        return Recipe("delays", klass, [wave(M) for M in DELAY_M])
    waves = [wave(M) for M in DELAY_M]
    waves.append(W(*[P(M, 0.5, D) for M, D in DELAY_PAIRS * 2]))
    waves.append(W(*[P(M, 0.5, D) for M, D in (DELAY_NEGATIVE[0],) * 3 + (DELAY_NEGATIVE[1],) * 3 + (DELAY_NEGATIVE[2],) * 2]))
    return Recipe("delays", klass, waves)


def kinds(klass):
    """waves 0, 1: notch / peak, adaptive -- static from block 3 on (on the taps three blocks of adaptation left), adaptive again from block 7
    on; waves 2, 3: notch / peak, static from zero taps.  Each of the four kinds is alone in a wave at some time.  The appended channels
    -- the left-over channels of the groups: one wave of the general instantiation -- are one of each kind and one more adaptive notch; two
    of them move with waves 0 and 1: all four kinds in ONE wave in blocks 0..2 and 7..9, static taps that adaptation left beside an
    adaptive channel in blocks 3..6."""
    b = lambda **kw: _base(klass, **kw)
    waves = [W(b()), W(b(notch=False)), W(b(adaptive=False)), W(b(notch=False, adaptive=False))]
    moving = [(0, None), (1, None), ("rem", 0), ("rem", 1)]
    if klass == "full":                           # ... and static taps read through the bounds check (D < 0)
        waves.append(W(P(8, 0.5, -3)))
        moving.append((4, None))
    events = [(3, w, lane, "setALSfilterStatic", ()) for w, lane in moving] + [(7, w, lane, "setALSfilterAdaptive", ()) for w, lane in moving]
    rem = [b(), b(notch=False), b(adaptive=False), b(notch=False, adaptive=False), b()]
    return Recipe("kinds", klass, waves, rem, events)


LAMBDAS = (0.0, 1e-6, 0.05, 0.5, 1.0)


def lambdas(klass):
    m, _l, d = _base(klass).key()[:3]
    return Recipe("lambdas", klass, [W(P(m, lam, d)) for lam in LAMBDAS])


def migrations(klass):
    """setters between calls, no enableALSfilter in between unless named.  wave 0: (100, 0.5, 7) -> (40, 0.5, 7) -> (100, 0.5, 7): full ->
    compact -> full, and the reference keeps taps 64..99 meanwhile; wave 1: 55 -> 8 -> 55 taps; wave 2: the mode away (USB <-> SAM) and
    back with the filter on (compact class: in the full class the wave stays as it is); wave 3: disableALSfilter for two blocks, then enableALSfilter (which resets); wave 4: row 3 starts with the
    filter off and gets enableALSfilter in front of block 4, in a wave of enabled channels."""
    d1 = 3 if klass == "compact" else 20
    waves = [W(P(100, 0.5, 7)), W(P(55, 0.5, d1)), W(_base(klass)), W(_base(klass)), W(*[_base(klass, en=(r != 3)) for r in range(8)])]
    rem = [_base(klass) for _ in range(REM)]
    events = [(3, 0, None, "setALSfilterParams", (40, 0.5, 7.0)), (6, 0, None, "setALSfilterParams", (100, 0.5, 7.0)),
              (3, 1, None, "setALSfilterParams", (8, 0.5, float(d1 if klass == "compact" else 60))), (6, 1, None, "setALSfilterParams", (55, 0.5, float(d1))),
              (3, 3, None, "disableALSfilter", ()), (5, 3, None, "enableALSfilter", ()),
              (4, 4, 3, "enableALSfilter", ())]
    if klass == "compact":
        events += [(3, 2, None, "setDemodMode", ("away",)), (6, 2, None, "setDemodMode", ("back",))]
    return Recipe("migrations", klass, waves, rem, events, every_call=True)


def partly_enabled(klass):
    """two waves of enabled channels, one with rows 0 and 2 off, and of the five appended channels two off: 25 enabled channels (three
    whole waves and one left over) and four plain ones -- the left-over sub-range holds both, in one wave of the general instantiation"""
    b = lambda **kw: _base(klass, **kw)
    return Recipe("partly_enabled", klass, [W(b()), W(b()), W(*[b(en=r not in (0, 2)) for r in range(8)])],
                  rem=[b(), b(en=False), b(), b(en=False), b()])


RECIPES = {f.__name__: f for f in (lengths, lengths_in_one_wave, delays, kinds, lambdas, migrations, partly_enabled)}
EVERY_FORM = ("lengths", "delays", "kinds")
SOME_FORMS = ("lengths_in_one_wave", "lambdas", "migrations")
MIXED_ONLY = ("partly_enabled",)                  # different flags in one wave: a uniform-group form would lose its form


# ---- forms --------------------------------------------------------------------------------------------------------------------------
class Form:
    """klass: the class of recipe rows; mode: the bank's demodulation mode; rem: five channels appended; plan: "one" block per call or the
    "loop" of 2, 3, 5; env: the environment read at asdr_create; sam / als: the launch-form switches set on the batch"""

    def __init__(self, name, klass, stated, mode=USB, rem=False, plan="one", env=None, sam=None, als_split=0, taps=False):
        self.name, self.klass, self.stated, self.mode, self.rem, self.plan = name, klass, stated, mode, rem, plan
        self.env, self.sam, self.als_split, self.taps = dict(env or {}), sam, als_split, taps

    def calls(self, recipe):
        cuts = sorted({e[0] for e in recipe.events})
        if self.plan == "one":
            return [1] * T
        out, pos, k = [], 0, 0
        while pos < T:                            # 2, 3, 5, 2, ... cut short in front of an event and at the end
            nxt = min([c for c in cuts if c > pos] + [T])
            out.append(min((2, 3, 5)[k % 3], nxt - pos)); pos += out[-1]; k += 1
        return out


_NO_ROLES = {"ASDR_NO_ALS_ROLE_STREAMS": "1"}
_SAM3 = {SAM_PRE_U: 1, SAM_PLL: 1, SAM_POST_ALS_U: 1}
# stated: the launches of a call on a regular bank; {1: ..., 2: ...} where a call of one block and one of several differ
FORMS = {f.name: f for f in (
    Form("one", "compact", {ALS_SMALL_ONE: 1}),
    Form("loop", "compact", {1: {ALS_SMALL_ONE: 1}, 2: {ALS_SMALL: 1}}, plan="loop", env=_NO_ROLES),
    Form("small_mixed", "compact", {ALS_SMALL_ONE: 1, ALS_MIXED: 1}, rem=True),      # (the remainders run on the 516-float rows: see GONE)
    Form("full", "full", {ALS_FULL: 1}),
    Form("full_mixed", "full", {ALS_FULL: 1, ALS_MIXED: 1}, rem=True),
    Form("split", "compact", {ALS_PRE: 1, ALS_K: 1}, als_split=8),
    Form("roles2", "compact", {1: {ALS_SMALL_ONE: 1}, 2: {ALS_SEED: 1, ALS_PRE_LOOP: 1, ALS_K: 1}}, plan="loop", env={"ASDR_ALS_ROLE_STAGES": "2"}),
    Form("roles3", "compact", {1: {ALS_SMALL_ONE: 1}, 2: {ALS_SEED: 1, SAM_PRE_LOOP_U: 1, ALS_BACK: 1, ALS_K: 1}}, plan="loop",
         env={"ASDR_ALS_ROLE_STAGES": "3"}),
    Form("sam3", "compact", _SAM3, mode=SAM, sam=(False, 8)),
    Form("sam3_mixed", "compact", dict(_SAM3, **{ALS_MIXED: 1}), mode=SAM, rem=True, sam=(False, 8)),
    Form("sam_fused", "compact", {ALS_FULL: 1}, mode=SAM, sam=(True, 0)),                # the SAM + ALS kind without exchange tiles
    Form("one-taps", "compact", {ALS_SMALL_ONE: 1}, taps=True),
    Form("full-taps", "full", {ALS_FULL: 1}, taps=True))}
OTHER_FORMS = ("one", "full", "split", "roles2", "sam3")
MIXED_FORMS = ("small_mixed", "full_mixed", "sam3_mixed")


def cells():
    """every (form, recipe) that runs; what is not here is inadmissible by the table at the top (a form takes the recipe in ITS class)"""
    out = [(f, r) for r in EVERY_FORM for f in FORMS]
    out += [(f, r) for r in SOME_FORMS for f in OTHER_FORMS]
    out += [(f, r) for r in MIXED_ONLY for f in MIXED_FORMS]
    return out


# ---- banks --------------------------------------------------------------------------------------------------------------------------
class Bank:
    """a recipe in a form: n channels (channel c: input row c % 8), their settings in front of block 0 and the events by block"""

    def __init__(self, recipe, form):
        self.recipe, self.form = recipe, form
        self.initial = [(form.mode, p.copy()) for w in recipe.waves for p in w]
        rem0 = len(self.initial)
        if form.rem:
            self.initial += [(form.mode, p.copy()) for p in recipe.rem]
        self.n = len(self.initial)
        assert self.n <= 160
        away = SAM if form.mode == USB else USB
        self.events = {}
        for blk, w, lane, meth, args in recipe.events:
            if w == "rem":
                if not form.rem:
                    continue
                chans = [rem0 + lane]
            else:
                chans = [8 * w + r for r in (range(8) if lane is None else (lane,))]
            args = tuple({"away": away, "back": form.mode}.get(a, a) if isinstance(a, str) else a for a in args)
            self.events.setdefault(blk, []).append((chans, meth, args))

    def setup(self):
        """helpers.S setters in front of block 0: the form's, then every channel's own"""
        out = [S("setDemodMode", self.form.mode), S("setNoiseBlankerThresholdDb", 10.0), S("enableAudioFilter")]
        for c, (_m, p) in enumerate(self.initial):
            out += [S(m, *a, sel=c) for m, a in p.setters()]
        return out

    def states(self):
        """[block][channel] -> (mode, P) in force while that block is processed"""
        cur, out = [(m, p.copy()) for m, p in self.initial], []
        for blk in range(T):
            for chans, meth, args in self.events.get(blk, ()):
                for c in chans:
                    m, p = cur[c]
                    cur[c] = (apply(m, p, meth, args), p)
            out.append([(m, p.copy()) for m, p in cur])
        return out

    def channel_script(self, c):
        """[(block, method, args)] of channel c, the setup as block 0"""
        out = [(0, m, a) for m, a, sel in self.setup() if sel is None or sel == c]
        return out + [(blk, meth, args) for blk in sorted(self.events) for chans, meth, args in self.events[blk] if c in chans]


_ROWS = {}


def rows(mode):
    """int16 I, Q [8][T][128]: USB rows -- a carrier 600 Hz into the passband and a second tone 1 kHz above it; SAM rows -- a modulated carrier
    near the IF centre and a tone beside it"""
    if mode not in _ROWS:
        from audiosdr_amd.synth import make_iq
        r = np.arange(U)
        if mode == SAM:
            I, Q = make_iq(U, T, fc=6890.0 + (r - 4) * 35.0, A=0.3, m=0.4, f2=7600.0, a2=0.12, noise=0.01)
        else:
            I, Q = make_iq(U, T, fc=6290.0 + 25.0 * r, A=0.3, f2=7290.0 + 40.0 * r, a2=0.12, noise=0.01)
        I.setflags(write=False); Q.setflags(write=False)
        _ROWS[mode] = (I, Q)
    return _ROWS[mode]


# ---- the host's plan, restated ------------------------------------------------------------------------------------------------------
def kind_of(mode, p):
    if p.en:
        return "als" if not p.small() else ("sam_als" if mode == SAM else "als_small")
    return "sam" if mode == SAM else "plain"


_HEAVIEST_FIRST = ("als", "sam_als", "als_small", "sam", "plain")


def sub_ranges(chans, form):
    """[(kind, uniform)] of a bank's schedule and (sam_split, als_split) as the call's plan sees them (flush_host, plan_launches).  The
    settings groups: kernel kind, mode and the flag bits (enable, notch, adaptive -- the other enables are the bank's)."""
    groups = {}
    for m, p in chans:
        k = (kind_of(m, p), m, p.en, p.notch, p.adaptive)
        groups[k] = groups.get(k, 0) + 1
    n_sam = sum(g for k, g in groups.items() if k[0] in ("sam", "sam_als"))
    fused, sam_min = form.sam if form.sam else (False, 512)
    sam_split = not fused and n_sam >= (sam_min or 512)
    als_split = form.als_split > 0 and sum(g for k, g in groups.items() if k[0] == "als_small") >= form.als_split
    uni, rem, left, left_general = {}, {}, 0, False
    for k, g in groups.items():
        if k[0] == "sam" and not sam_split:       # the fused SAM instantiation has only the general form
            rem[k[0]] = rem.get(k[0], 0) + g
        else:
            uni[k[0]] = uni.get(k[0], 0) + g // 8 * 8
            left += g % 8
            left_general = left_general or (g % 8 > 0 and k[0] != "plain")
    subs = [("als" if left_general else "plain", False)] if left else []
    for kind in _HEAVIEST_FIRST:
        if uni.get(kind, 0) > 0: subs.append((kind, True))
        if rem.get(kind, 0) > 0: subs.append((kind, False))
    sam_slots = sum(uni.get(k, 0) + rem.get(k, 0) for k in ("sam", "sam_als"))
    return subs, sam_split and sam_slots > 0, als_split and not form.taps and uni.get("als_small", 0) > 0


def census(chans, k, form):
    """{kernel: launches} of a call of k blocks on channels [(mode, P)] (asdr_launch_update_ordered, launch_als_roles); the reset kernel aside"""
    subs, sam_split, als_split = sub_ranges(chans, form)
    assert k == 1 or not (sam_split or als_split), "one launch per block, lanes and SAM role streams are not restated here"
    roles = ("ASDR_NO_ALS_ROLE_STREAMS" not in form.env and k >= 2 and not form.taps and not sam_split and not als_split and
             subs == [("als_small", True)] and chans[0][0] <= 6)
    out = {}

    def add(*names):
        for name in names:
            out[name] = out.get(name, 0) + 1

    if roles:
        chunks = (k + ALS_CHUNK - 1) // ALS_CHUNK
        add(ALS_SEED)
        for _ in range(chunks):
            add(*((ALS_PRE_LOOP, ALS_K) if form.env.get("ASDR_ALS_ROLE_STAGES") == "2" else (SAM_PRE_LOOP_U, ALS_BACK, ALS_K)))
        return out
    for kind, uniform in subs:
        if kind == "als" or (kind == "sam_als" and not sam_split):
            add(ALS_FULL if uniform else ALS_MIXED)
        elif kind == "als_small":
            assert uniform
            if als_split: add(ALS_PRE, ALS_K)
            else: add(ALS_SMALL_ONE if k == 1 else ALS_SMALL)
        elif kind in ("sam", "sam_als") and sam_split:
            assert uniform
            add(SAM_PRE_U, SAM_PLL, SAM_POST_ALS_U if kind == "sam_als" else SAM_POST_U)
        elif kind == "sam":
            add(SAM_FUSED)
        else:
            add((PLAIN_ONE if k == 1 else PLAIN_LOOP) if uniform else PLAIN_MIXED)
    return out


def regular(bank):
    """the bank is what its form's `stated` census speaks of: every channel enabled, in the form's mode and class, throughout"""
    want_small = bank.form.klass == "compact"
    return all(m == bank.form.mode and p.en and p.small() == want_small for st in bank.states() for m, p in st)


# ---- the wave predicates of als_compute ---------------------------------------------------------------------------------------------
def wave_paths(ps, AH):
    """the arithmetic paths of als_compute a wave of eight channels [P] (disabled ones: the dummy channel included) takes on rows with AH
    history samples: a subset of static, default, uniform, per_lane, checked"""
    en = [p for p in ps if p.en]
    safe = AH == 64 or all(p.D >= 0 and p.D + p.M <= AH + 1 for p in en)
    m_uniform = len(en) == len(ps) and all(p.adaptive and p.M == ps[0].M for p in ps)
    m_default = m_uniform and safe and ps[0].M == 55
    out = set()
    if any(not p.adaptive for p in en):
        out.add("static" if safe else "static_checked")
    if m_default:
        out.add("default")
    elif any(p.adaptive for p in en):
        out.add("checked" if not safe else "uniform" if m_uniform else "per_lane")
    return out


def bank_waves(bank, blk_states):
    """the waves of a bank's schedule in front of a block as lists of P and the AH of the rows they run on: whole waves of a settings group
    on their kind's rows, the left-over channels (padded with the dummy channel, filter off) on the 516-float rows"""
    groups = {}
    for m, p in blk_states:
        groups.setdefault((kind_of(m, p), m, p.en, p.notch, p.adaptive), []).append(p)
    out, left = [], []
    for k, ps in groups.items():
        whole = len(ps) // 8 * 8
        AH = 64 if k[0] in ("als_small", "sam_als") and not (k[0] == "sam_als" and bank.form.sam and bank.form.sam[0]) else 128
        out += [(ps[i:i + 8], AH) for i in range(0, whole, 8)]
        left += ps[whole:]
    out += [((left[i:i + 8] + [P(en=False)] * 8)[:8], 128) for i in range(0, len(left), 8)]
    return out
