"""What tests/als_scenarios.py claims, shown without a GPU: the classes hold what their table says, the restated host plan gives every
form's stated census on a regular bank, the recipes reach every arithmetic path of als_compute on both row layouts and both sides of the
two D + M edges, the oracle stays finite on every recipe channel (a condition: bit comparison says nothing about NaN and values beyond
int32), the recipes tell seven wrong filters from the right one, the oracle agrees with the reference's own code on every recipe setting
inside the reference's defined domain, and the forms name every kernel of the launch census that carries the filter."""
import os
import re

import numpy as np
import pytest

import als_scenarios as L
import ref_scenarios as R
from cases import USB, SAM
from oracle import ref_build
from test_signal_path_independent import RefSDR, S, N

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KLASSES = ("compact", "full")
_USB_FORM = {"compact": "small_mixed", "full": "full_mixed"}      # the USB form of a class with the appended channels: every recipe channel


def _banks():
    """every bank the GPU file runs, once per (recipe, class, mode, appended channels)"""
    seen, out = set(), []
    for f, r in L.cells():
        form = L.FORMS[f]
        key = (r, form.klass, form.mode, form.rem)
        if key not in seen:
            seen.add(key); out.append(L.Bank(L.RECIPES[r](form.klass), form))
    return out


def test_every_recipe_row_is_of_its_class():
    """compact rows fit the compact kinds, full rows do not, throughout -- but for the one wave that migrates between the classes"""
    for name, make in L.RECIPES.items():
        for klass in KLASSES:
            rec = make(klass)
            bank = L.Bank(rec, L.FORMS[_USB_FORM[klass]])
            for blk, st in enumerate(bank.states()):
                for c, (_m, p) in enumerate(st):
                    if name == "migrations" and c < 8:
                        assert p.small() == (3 <= blk < 6), (klass, blk, c)
                    elif p.en:
                        assert p.small() == (klass == "compact"), (name, klass, blk, c, p.key())
    assert len(L.cells()) == 3 * len(L.FORMS) + 3 * len(L.OTHER_FORMS) + len(L.MIXED_FORMS)
    assert all(L.FORMS[f].rem for f in L.MIXED_FORMS) and not any(L.FORMS[f].rem for f in L.OTHER_FORMS)


def test_stated_census_is_the_plan_on_a_regular_bank():
    """Every form's stated kernels are what the restated host plan gives for every call on every regular bank of the form; every form has one."""
    had = set()
    for f, r in L.cells():
        form = L.FORMS[f]
        bank = L.Bank(L.RECIPES[r](form.klass), form)
        assert bank.n % 8 == (L.REM if form.rem else 0) and 8 <= bank.n <= 160
        if not L.regular(bank):
            continue
        had.add(f)
        states, pos = bank.states(), 0
        for k in form.calls(bank.recipe):
            stated = form.stated[min(k, 2)] if 1 in form.stated else form.stated
            assert L.census(states[pos], k, form) == stated, (f, r, pos, k)
            pos += k
        assert pos == L.T
    assert had == set(L.FORMS)
    multi = [f for f in L.FORMS if L.FORMS[f].plan == "loop"]
    assert sorted(multi) == ["loop", "roles2", "roles3"]
    for f in multi:                                  # the calls of several blocks do happen, with and without events
        for r in ("lengths", "kinds"):
            assert max(L.FORMS[f].calls(L.RECIPES[r]("compact"))) >= 3


def test_branch_reach():
    """The wave predicates of als_compute on every wave of every bank and block: static taps, the default-length register path, uniform M,
    per-lane M on both row layouts; the bounds-checked path, which exists on the 516-float rows only; static and adaptive channels in one
    wave; eight different M in one wave; D + M on both sides of 65 | 66 and of 128 | 129; the stand-alone filter kernel (split, roles)."""
    reached = {64: set(), 128: set()}
    both_kinds = lengths8 = False
    sums = set()
    for bank in _banks():
        for st in bank.states():
            sums |= {p.D + p.M for _m, p in st if p.en}
            for ps, AH in L.bank_waves(bank, st):
                paths = L.wave_paths(ps, AH)
                reached[AH] |= paths
                en = [p for p in ps if p.en]
                both_kinds = both_kinds or (any(p.adaptive for p in en) and any(not p.adaptive for p in en))
                if len({p.M for p in en}) == 8 and 55 in {p.M for p in en}:
                    lengths8 = True
                    assert "per_lane" in paths
    assert reached[64] == {"static", "default", "uniform", "per_lane"}
    assert reached[128] == {"static", "static_checked", "default", "uniform", "per_lane", "checked"}
    assert both_kinds and lengths8
    assert {65, 66, 128, 129} <= sums and min(p.D for b in _banks() for _m, p in b.initial) < 0
    # seven channels at 55 and one at 54: uniform is lost, and so is the default path
    for klass in KLASSES:
        w = L.lengths_in_one_wave(klass).waves[1]
        assert sorted(p.M for p in w) == [54] + [55] * 7 and L.wave_paths(w, 64 if klass == "compact" else 128) == {"per_lane"}
    # the stand-alone kernel (its output row overlays the history) runs the compact class of every recipe but partly_enabled
    stand_alone = {r for f, r in L.cells() if L.ALS_K in str(L.FORMS[f].stated)}
    assert stand_alone == set(L.EVERY_FORM) | set(L.SOME_FORMS)


def _oracle_channel(ao, bank, c, taps=True):
    """the oracle through channel c of a bank: yields (block, oracle) after every block"""
    I, Q = L.rows(bank.form.mode)
    o = ao.OracleSDR(taps=taps, pll_wrap_bound=False)
    by = {}
    for blk, meth, args in bank.channel_script(c):
        by.setdefault(blk, []).append((meth, args))
    for blk in range(L.T):
        for meth, args in by.get(blk, ()):
            getattr(o, meth)(*args)
        audio = o.update(I[c % L.U, blk], Q[c % L.U, blk])
        yield blk, o, audio


def test_oracle_stays_finite(ao):
    """|ALS tap| < 4.0 for every recipe channel in every block (lambda <= 1.0 everywhere: a filter that diverges ends beyond int32 and in NaN)."""
    worst = 0.0
    for bank in _banks():
        for c in range(bank.n):
            for blk, o, _a in _oracle_channel(ao, bank, c):
                t = o.tap("ALS")
                assert np.isfinite(t).all() and np.abs(t).max() < 4.0, (bank.recipe.name, bank.form.klass, bank.form.mode, c, blk, float(np.abs(t).max()))
                worst = max(worst, float(np.abs(t).max()))
    assert 0.0 < worst < 4.0


# ---- wrong filters ------------------------------------------------------------------------------------------------------------------
FAULTS = ("tap55_in_the_default_path", "previous_tap_sets_error", "history_index_off_by_one", "compact_kind_zeroes_taps_64_127",
          "history_shorter_than_64", "static_taps_updated", "static_notch_peak_swapped")
_M55, _M64 = L.LENGTHS["compact"].index(55), L.LENGTHS["compact"].index(64)
# (recipe, class, wave, row): the channels a fault is looked for on; the right filter must agree with the oracle on every one of them
CANDIDATES = {"tap55_in_the_default_path": [("lengths", "compact", _M55, 0), ("lambdas", "compact", 3, 1)],
              "previous_tap_sets_error": [("lengths", "compact", _M55, 0), ("delays", "full", 1, 2)],
              "history_index_off_by_one": [("lengths", "compact", _M55, 0), ("delays", "compact", 0, 3)],
              "compact_kind_zeroes_taps_64_127": [("migrations", "compact", 0, 0), ("migrations", "full", 0, 5)],
              "history_shorter_than_64": [("lengths", "compact", _M64, 0), ("delays", "compact", 0, 3)],
              "static_taps_updated": [("kinds", "compact", 2, 0), ("kinds", "full", 0, 1)],
              "static_notch_peak_swapped": [("kinds", "compact", 2, 0), ("kinds", "compact", 1, 2)]}


class AlsUnderTest(RefSDR):
    """the independent restatement's ALS filter (tests/test_signal_path_independent.py) with the setters the recipes use and, on request,
    one planted fault; without a fault als() IS the restatement's"""

    def __init__(self, ao, fault=None):
        super().__init__(ao)
        assert fault is None or fault in FAULTS
        self.fault, self.prev_e = fault, S(0)

    def disableALSfilter(self): self.als_on = False
    def setALSfilterNotch(self): self.notch = True
    def setALSfilterPeak(self): self.notch = False
    def setALSfilterAdaptive(self): self.adaptive = True
    def setALSfilterStatic(self): self.adaptive = False

    def setALSfilterParams(self, m, lam, delay):
        self.M, self.lam, self.delay = min(int(m), N), S(lam), int(delay)
        if self.fault == "compact_kind_zeroes_taps_64_127" and L.P(self.M, lam, self.delay).small():
            self.als_w[64:] = [S(0)] * (N - 64)

    def als(self):
        f = self.fault
        if f is None:
            return RefSDR.als(self)
        M = 56 if (f == "tap55_in_the_default_path" and self.M == 55 and self.adaptive) else self.M
        off = 1 if f == "history_index_off_by_one" else 0

        def x(i, back):
            if f == "history_shorter_than_64" and back > 63:
                return S(0)
            return self.als_in[i - back]
        count = 0
        self.als_in[0:N] = self.als_in[N:2 * N]; self.als_in[N:2 * N] = list(self.audio)
        for i in range(N, 2 * N):
            y = S(0.0)
            for j in range(M):
                y = S(y + S(self.als_w[j] * x(i, self.delay + j + off)))
            e = S(self.als_in[i] - y)
            if self.adaptive or f == "static_taps_updated":
                if count == 0:
                    eu = self.prev_e if f == "previous_tap_sets_error" else e
                    for j in range(M):
                        g = S(eu * x(i, self.delay + j + off))
                        self.als_w[j] = S(self.als_w[j] + S(self.lam * g))
                    self.prev_e = e
                count = (count + 1) % 4
            notch = (not self.notch) if (f == "static_notch_peak_swapped" and not self.adaptive) else self.notch
            self.audio[i - N] = e if notch else y


def _differs(ao, cand, fault):
    """does the restatement's filter with `fault` differ from the oracle, in the filter's output or in its taps, on this channel?"""
    name, klass, wave, row = cand
    bank = L.Bank(L.RECIPES[name](klass), L.FORMS[_USB_FORM[klass]])
    c = 8 * wave + row
    assert all(p.in_domain() for st in bank.states() for p in [st[c][1]])
    r = AlsUnderTest(ao, fault)
    script = {}
    for blk, meth, args in bank.channel_script(c):
        script.setdefault(blk, []).append((meth, args))
    with np.errstate(all="ignore"):
        for blk, o, _a in _oracle_channel(ao, bank, c):
            for meth, args in script.get(blk, ()):
                getattr(r, meth)(*args)
            if not r.als_on:
                continue
            r.audio = [S(v) for v in o.tap("AGC")]
            r.als()
            out, w = np.array(r.audio, np.float32), np.array(r.als_w, np.float32)
            if out.tobytes() != o.tap("ALS").tobytes() or w.tobytes() != o.als_taps().tobytes():
                return True
    return False


def test_the_restatement_agrees_with_the_oracle_on_every_candidate(ao):
    for cand in sorted({c for cs in CANDIDATES.values() for c in cs}):
        assert not _differs(ao, cand, None), cand


@pytest.mark.parametrize("fault", FAULTS)
def test_recipes_tell_wrong_filters_apart(ao, fault):
    assert any(_differs(ao, cand, fault) for cand in CANDIDATES[fault]), fault


# ---- the reference's own code -------------------------------------------------------------------------------------------------------
def _reference_channels():
    """one channel per distinct setting (the setters a channel gets, with their blocks) of every recipe channel that ever has the filter on
    and stays inside the reference's defined domain (D >= 0, M + D <= 128); USB banks, the appended channels included"""
    seen, out = set(), []
    for name, make in L.RECIPES.items():
        for klass in KLASSES:
            bank = L.Bank(make(klass), L.FORMS[_USB_FORM[klass]])
            states = bank.states()
            for c in range(bank.n):
                ps = [st[c][1] for st in states]
                if not any(p.en for p in ps) or not all(p.in_domain() for p in ps):
                    continue
                cs = bank.channel_script(c)
                key = tuple(cs)
                if key in seen:
                    continue
                seen.add(key)
                script, at = [], 0
                for blk, meth, args in cs:
                    if blk > at:
                        script.append(("run", (blk - at,))); at = blk
                    script.append((meth, args))
                out.append(dict(label="%s %s ch %d" % (name, klass, c), bank=bank, c=c, script=script))
    return out


def test_reference_channels_cover_the_domain():
    chans = _reference_channels()
    assert 40 <= len(chans) <= 64, len(chans)
    outside = [(p.M, p.D) for b in _banks() for _m, p in b.initial if p.en and not p.in_domain()]
    assert set(outside) == set(L.DELAY_PAIRS[1:]) | set(L.DELAY_NEGATIVE)        # the defined difference: these run against the oracle alone


def test_oracle_equals_the_reference_binary(ao):
    """The int16 audio of every block, bit for bit, from the reference's own AudioSDR.cpp (oracle/_ref, as tests/test_reference_binary.py)."""
    R.require_binaries()
    chans = _reference_channels()
    I, Q = L.rows(USB)
    out = R.run_all({ch["label"]: (ref_build.run_sdr, (ch["script"], I[ch["c"] % L.U], Q[ch["c"] % L.U])) for ch in chans})
    for ch in chans:
        want = np.stack([a for _b, _o, a in _oracle_channel(ao, ch["bank"], ch["c"], taps=False)])
        audio, _g = out[ch["label"]]
        assert np.array_equal(want, audio), "%s: first differing block %d" % (ch["label"], int(np.nonzero((want != audio).any(axis=1))[0][0]))


# ---- census closure -----------------------------------------------------------------------------------------------------------------
def test_census_closure():
    """Every kernel of the launch census whose name contains `als` is launched by a form: named by its stated census, and by the restated
    plan on some call of some cell."""
    src = open(os.path.join(ROOT, "audiosdr_amd", "csrc", "asdr_kernels.hip")).read()
    table = re.search(r"k_kernel_names\[\] = \{(.*?)\};", src, flags=re.S).group(1)
    names = set(re.findall(r'"(\w+)"', table))
    carrying = {n for n in names if "als" in n}
    stated, planned = set(), set()
    for form in L.FORMS.values():
        for d in (form.stated.values() if 1 in form.stated else [form.stated]):
            stated |= set(d)
    for f, r in L.cells():
        form = L.FORMS[f]
        bank = L.Bank(L.RECIPES[r](form.klass), form)
        states, pos = bank.states(), 0
        for k in form.calls(bank.recipe):
            planned |= set(L.census(states[pos], k, form)); pos += k
    assert stated <= names and planned <= names
    assert not set(L.GONE) & names               # (the two kernels no plan could reach: als_scenarios.GONE)
    assert len(carrying) == 10
    assert carrying <= stated, sorted(carrying - stated)
    assert carrying <= planned, sorted(carrying - planned)
