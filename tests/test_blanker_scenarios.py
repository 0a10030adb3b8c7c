"""The blanker recipes of tests/blanker_scenarios.py reach the seams they name -- shown on the CPU, against the oracle, with taps on.

For every recipe the oracles' SCALED_I/Q and NB_I/Q taps give the mask of every output block (the ratio, wherever the delayed scaled sample
is not zero).  Claims about detection indices, edges and the carried mask use blanker_scenarios.Restatement, the channel-vectorised numpy
form of nb_process, AFTER it has reproduced the oracle's NB_I/Q taps and NoiseBlankerDetection() bit for bit on these very rows.

Then the recipes are shown to separate wrong blankers: every variant of the restatement below changes the masked output of the recipes
named beside it (CATCHES: asserted, and no variant is caught by none):

    window9                  a window of +-9                        every family
    no_rescan                78..127 not scanned again              every family
    edge_misses_128          the edge test starts at i = 129        positions, pairs, dense, marginal, setter
    ramp_not_below_128       no ramp entry below 128 is written     every family
    counts_saturate_127      detections behind the 127th of a scan  runs (the step onto a raised average), dense, setter
                             zero nothing
    carried_spill_dropped    mask[256..265] is not carried          runs, dense, marginal
    no_average_on_rescan     the re-scan leaves the average alone   runs, dense, marginal, setter

(families: positions, pairs, runs, dense, marginal, one-in-a-wave, setter.)  Two of these are hidden by the second scan wherever it
repeats the first one's detections: a strong isolated impulse at 118..127 is detected again at i = p by the next call, which zeroes
mask[p - 10 .. p + 10] anew -- the carried spill is only needed where that second detection fails (the dense rows' surge, the marginal
impulses, the step rows); and the detections a saturated count drops are the scan's last, i >= 205, all of them scanned again -- only
the step onto an average already at half the new level, and the noise surge, are detected by the first scan alone.

The marginal recipes' second claim, a sample at 78..127 detected by one of its two scans only, is reached in both directions at every
threshold: by the first scan only where the average rises between the two (49 samples apart; the impulse's own envelope adds to that),
by the second only where it falls by more than the impulse itself adds -- behind a drop of the tone from 1.5 (1.1 at ratio 1.2) to 1.0."""
import numpy as np
import pytest

import blanker_scenarios as B
import four_wave_scenarios as F
from helpers import f32_bits


class _Oracles(F.OracleRun):
    def __init__(self, ao, sc, bI, bQ):
        self.nb_detected = {}
        super().__init__(ao, sc, bI, bQ, taps_for=range(sc.n))

    def after_block(self, i, blk, o):
        self.nb_detected[(i, blk)] = o.NoiseBlankerDetection()


class Analysis:
    """One recipe through its oracles (taps on) and through the restatement.  K = distinct channels (key index = row for the recipes here)."""

    def __init__(self, ao, recipe):
        self.recipe = recipe
        bI, bQ = recipe.rows()
        self.sc = sc = B.scenario(recipe)
        run = _Oracles(ao, sc, bI, bQ)
        self.K, self.T = len(run.index), bI.shape[1]
        K, T = self.K, self.T
        assert K == recipe.U and all(run.index[k] == k[0] for k in run.index), "one key per row, in row order"
        taps = np.stack([run.taps[i] for i in range(K)])                        # [K][T][12][128]
        self.sI, self.sQ, self.oI, self.oQ = (np.ascontiguousarray(taps[:, :, j]) for j in range(4))
        self.o_detected = np.array([[run.nb_detected[(i, t)] for t in range(T)] for i in range(K)])
        self.events = {}                                                        # block -> {index into all_setters(): key indices it reaches}
        allset = sc.all_setters()
        for k, i in run.index.items():
            for j in k[1]:
                self.events.setdefault(max(allset[j][0], 0), {}).setdefault(j, []).append(i)
        self.allset = allset
        self.rI, self.rQ = self.restate(None, record=True)

    def restate(self, variant, record=False):
        K, T = self.K, self.T
        m = B.Restatement(K, variant)
        rI, rQ = np.empty_like(self.oI), np.empty_like(self.oQ)
        if record:
            self.det = np.zeros((K, T, 178), bool); self.edges = np.zeros((K, T, 128), bool); self.spill = np.zeros((K, T), bool)
            self.out_mask = np.ones((K, T, 128), np.float32); self.carry = np.zeros((K, T), bool); self.r_detected = np.zeros((K, T), np.int64)
        for t in range(T):
            for j in sorted(self.events.get(t, {})):
                m.setter(np.array(self.events[t][j]), self.allset[j][1][0], self.allset[j][1][1])
            rI[:, t], rQ[:, t] = m.step(self.sI[:, t], self.sQ[:, t])
            if record:
                self.det[:, t], self.edges[:, t], self.spill[:, t] = m.det, m.edges, m.spill
                self.out_mask[:, t], self.carry[:, t], self.r_detected[:, t] = m.out_mask, m.carry_nontrivial, m.detected
        return rI, rQ

    def enabled(self):
        """[K] the blanker is on (recipes without a script: as the setup leaves it)"""
        en = np.ones(self.K, bool)
        for j, (_blk, s) in enumerate(self.allset):
            if s[0] in ("disableNoiseBlanker", "enableNoiseBlanker"):
                en[self.events[0][j]] = s[0] == "enableNoiseBlanker"
        return en

    def recovered_mask(self):
        """[K][T][128] mask codes 0..6 (index into MASK_VALUES) from the taps alone, -1 where both delayed scaled samples are zero"""
        K, T = self.K, self.T
        dI = np.zeros_like(self.sI); dQ = np.zeros_like(self.sQ)
        # (the output is two blocks late, counted from the blanker's last reset: a plain delay of the SCALED taps holds for the recipes
        # without a script, the only ones this is used on)
        dI[:, 2:], dQ[:, 2:] = self.sI[:, :-2], self.sQ[:, :-2]
        code = np.full((K, T, 128), -1, np.int64)
        known = ((dI != 0) | (dQ != 0)) & self.enabled()[:, None, None]
        for c, v in enumerate(B.MASK_VALUES):
            v = np.float32(v)
            hit = known & (f32_bits(v * dI) == f32_bits(self.oI)) & (f32_bits(v * dQ) == f32_bits(self.oQ)) & (code < 0)
            code[hit] = c
        assert not (known & (code < 0)).any(), "%s: an output sample is no mask value times the delayed input" % self.recipe.name
        return code


_CACHE = {}


def analysis(ao, recipe):
    if recipe.name not in _CACHE:
        _CACHE[recipe.name] = Analysis(ao, recipe)
    return _CACHE[recipe.name]


ALL = B.all_recipes()


@pytest.mark.parametrize("recipe", ALL, ids=lambda r: r.name)
def test_restatement_reproduces_the_oracle(ao, recipe):
    a = analysis(ao, recipe)
    for name, got, want in (("NB_I", a.rI, a.oI), ("NB_Q", a.rQ, a.oQ)):
        bad = np.argwhere(f32_bits(got) != f32_bits(want))
        assert bad.size == 0, "%s: %d words differ, first at (row, block, sample) %s" % (name, len(bad), bad[0].tolist())
    bad = np.argwhere(a.r_detected != a.o_detected)
    assert bad.size == 0, "NoiseBlankerDetection: first at (row, block) %s" % bad[0].tolist()


@pytest.mark.parametrize("recipe", [r for r in ALL if not r.script], ids=lambda r: r.name)
def test_mask_recovered_from_the_taps_is_the_restatements(ao, recipe):
    a = analysis(ao, recipe)
    code = a.recovered_mask()
    want = np.array(B.MASK_VALUES, np.float32)
    en = a.enabled()
    known = code >= 0
    assert np.array_equal(want[code[known]], a.out_mask[known])
    assert known[en][:, 2:].mean() > 0.99                                       # (the first two output blocks are the empty ring)


def test_all_seven_mask_values_occur(ao):
    seen = set()
    for r in ALL:
        if not r.script:
            seen |= set(np.unique(analysis(ao, r).recovered_mask()).tolist())
    assert seen >= set(range(7)), seen


# ---- the claims -----------------------------------------------------------------------------------------------------------------------
def test_positions(ao):
    a = analysis(ao, B.POSITIONS)
    for b in B.EVENTS:
        found = set()
        for p in range(128):
            at = [(t, int(i)) for t in range(b + 1, b + 4) for i in np.flatnonzero(a.edges[p, t])]
            if p <= 116:
                assert at == [(b + 1, 11 + p)], (b, p, at)                      # i = 139 + p, in the call that scans the impulse
            else:
                assert at == [(b + 2, p - 117)], (b, p, at)                     # i = 11 + p: one call later, from the carried mask
                assert a.carry[p, b + 1]
            found.add(128 + at[0][1])
            assert a.spill[p, b + 1] == (p >= 118), (b, p)
            assert not a.spill[p, b + 2]
            if 117 <= p <= 123:                                                 # i = 128..134: the ramp's head lands in the block being output
                i = 11 + p
                assert np.array_equal(a.out_mask[p, b + 2, i - 7:], B.TRANS[:128 - (i - 7)]), (b, p)
            assert a.det[p, b + 1, 50 + p] and a.det[p, b + 1].sum() == 1
        assert found == set(range(128, 256)), "phase %d" % (b % 3)
    assert {b % 3 for b in B.EVENTS} == {0, 1, 2}


def test_pairs(ao):
    a = analysis(ao, B.PAIRS)
    for d in B.PAIR_D:
        for p0 in B.PAIR_P0:
            r = B.pair_row(d, p0)
            for b in B.EVENTS:
                n_edges = int(a.edges[r, b + 1:b + 4].sum())
                assert n_edges == (1 if d <= 21 else 2), (d, p0, b, n_edges)
                assert a.det[r, b + 1:b + 3].sum() >= 2
    for b in B.EVENTS:                                                          # p0 = 3: both runs inside one block, never scanned again
        for d in (22, 28, 29):
            m = a.out_mask[B.pair_row(d, 3), b + 2]
            want = np.ones(128, np.float32)
            want[0:14] = 0.0; want[7:14] = B.TRANS                              # first run 0..13, its ramp over its tail
            want[3 + d - 10:3 + d + 11] = 0.0; want[3 + d + 4:3 + d + 11] = B.TRANS
            assert np.array_equal(m, want), (d, b)
            assert (m[14:3 + d - 10] == 1.0).all() and 3 + d - 10 - 14 == d - 21  # the gap: 1, 7 and 8 samples
        m = a.out_mask[B.pair_row(21, 3), b + 2]                                # d = 21: the windows touch: one run, one ramp
        want = np.ones(128, np.float32); want[0:35] = 0.0; want[28:35] = B.TRANS
        assert np.array_equal(m, want)
    assert not a.det[63].any()                                                  # the quiet row
    assert {k % 3 for k in B.STATE_CUTS["pairs"]} == {0, 1, 2}
    for k in B.STATE_CUTS["pairs"]:                                             # where tests/test_gpu_state.py cuts this bank
        assert a.carry[:63, k - 1].all()


def test_runs(ao):
    a = analysis(ao, B.RUNS_RECIPE)
    n = len(B.RUNS)
    assert (a.out_mask[:n] == 0.0).all(axis=2).any(), "no output block is zero throughout"
    assert (a.det[:n].sum(axis=2) >= 128).any(), "no scan with 128 detections"
    assert (a.det[:n].sum(axis=2) == 178).any(), "no scan detected throughout"
    up, down, t0 = B.STEP_UP_ROW, B.STEP_DOWN_ROW, B.STEP_AT // 128
    assert a.det[up, t0 + 1].sum() >= 64, "the step is gated as one long impulse"
    assert not a.det[up, t0 + 4:].any() and not a.det[up, :t0 + 1].any()
    assert not a.det[down].any()
    twice, t1 = B.STEP_TWICE_ROW, B.STEP_TWICE[1][0] // 128
    n_det = a.det[twice, t1 + 2].sum()                                          # the call that scans the whole block behind the second step
    assert 128 <= n_det < 178 and a.det[twice, t1 + 2, :128].all(), n_det       # ... detects up to where the average arrives, behind the 128th
    assert not a.det[twice, t1 + 3, :50].any()                                  # and its last detections are not made again by their second scan


@pytest.mark.parametrize("recipe", B.DENSE, ids=lambda r: r.name)
def test_dense(ao, recipe):
    a = analysis(ao, recipe)
    assert a.det[:, B.WARM:].any(axis=2).all(), "a block without a detection"
    assert (a.det.sum(axis=2) >= 128).any()
    assert a.carry[:, B.WARM - 1:].all(), "a call boundary with a trivial carried mask"
    assert {k % 3 for k in B.STATE_CUTS["dense-1.2"]} == {0, 1, 2} and min(B.STATE_CUTS["dense-1.2"]) > B.WARM


@pytest.mark.parametrize("recipe", B.MARGINALS, ids=lambda r: r.name)
def test_marginal(ao, recipe):
    a = analysis(ao, recipe)
    first, both, first_only, second_only = [], 0, 0, 0
    expected = np.zeros_like(a.det)
    for r in range(B.MARGINAL_ROWS):
        for b, p, _g in B.marginal_impulses(r, recipe.facts["threshold"]):
            d1 = bool(a.det[r, b + 1, 50 + p]); expected[r, b + 1, 50 + p] = True
            first.append(d1)
            if p >= 78:
                d2 = bool(a.det[r, b + 2, p - 78]); expected[r, b + 2, p - 78] = True
                both += d1 and d2; first_only += d1 and not d2; second_only += d2 and not d1
    assert not (a.det & ~expected).any(), "a detection that is no placed impulse"
    share = np.mean(first)
    print("%s: %d impulses, %.2f detected; at 78..127 both %d, first only %d, second only %d" % (recipe.name, len(first), share, both, first_only, second_only))
    assert 0.25 <= share <= 0.75
    assert first_only >= 1 and second_only >= 1


@pytest.mark.parametrize("recipe", B.ONE_IN_A_WAVE, ids=lambda r: r.name)
def test_one_in_a_wave(ao, recipe):
    a = analysis(ao, recipe)
    active = a.det.any(axis=2)
    active[:, 1:] |= a.carry[:, :-1]                                            # ... or a carried mask that is not all ones in front of the call
    per_wave = active.reshape(8, 8, a.T).sum(axis=1)
    assert per_wave.max() == 1
    for k in range(8):
        assert active[9 * k].sum() == active[8 * k:8 * k + 8].sum()            # the one is lane k of wave k
        for b, _p in B.WAVE_HITS:
            assert active[9 * k, b + 1] and active[9 * k, b + 2]
    assert a.spill[list(B.WAVE_ROWS), 15].all()                                 # the impulse at sample 120 reaches the next call by the carried mask only


@pytest.mark.parametrize("recipe", B.SETTERS + B.SETTERS_PIPE, ids=lambda r: r.name)
def test_setter_mid_burst(ao, recipe):
    a = analysis(ao, recipe)
    events = recipe.facts["events"]
    assert {ev % 3 for ev in events} == {0, 1, 2}
    for ev in events:
        assert a.carry[:, ev - 1].all(), "event at block %d: rows %s have nothing to discard" % (ev, np.flatnonzero(~a.carry[:, ev - 1]).tolist())


# ---- the recipes separate wrong blankers ----------------------------------------------------------------------------------------------
_EVERY = {"positions", "pairs", "runs", "dense", "marginal", "one-in-a-wave", "setter"}
CATCHES = {"window9": _EVERY, "no_rescan": _EVERY, "edge_misses_128": {"positions", "pairs", "dense", "marginal", "setter"},
           "ramp_not_below_128": _EVERY, "counts_saturate_127": {"runs", "dense", "setter"},
           "carried_spill_dropped": {"runs", "dense", "marginal"}, "no_average_on_rescan": {"runs", "dense", "marginal", "setter"}}


def _family(name):
    for f in ("marginal", "one-in-a-wave", "setter", "dense"):
        if name.startswith(f):
            return f
    return name


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_wrong_blankers_are_caught(ao, variant):
    caught = set()
    for r in ALL:
        a = analysis(ao, r)
        rI, rQ = a.restate(variant)
        if not (np.array_equal(f32_bits(rI), f32_bits(a.oI)) and np.array_equal(f32_bits(rQ), f32_bits(a.oQ))):
            caught.add(_family(r.name))
    print(variant, sorted(caught))
    assert caught, "no recipe notices %s" % variant
    assert caught == CATCHES[variant], (variant, sorted(caught))
