"""The chain kernels on the 512-byte ChanSmall row (asdr_device.h: the plain kind's fields in the first 256 bytes, the AM image state and the PLL words
behind them), on sequences in which the blanker's carried state matters from block to block, and the state records across that row
(asdr_state.hip translates between the record's original member order and the row): every case is held to the oracle at tolerance 0 --
the int16 audio of every channel and block, nb_detected after every call -- with the launch census asserted call by call.

    form     bank                                   kernel
    mw_u     512 channels, broadcast settings       asdr_update_kernel_mw_u
    mw       512, one channel's output gain differs asdr_update_kernel_mw
    one-8    8 channels  (one wave)                 asdr_update_kernel_one
    one-24   24 channels (three waves)              asdr_update_kernel_one

Inputs are rows of tests/blanker_scenarios.py whose carried mask is not all ones -- one impulse at p >= 117, pairs across the block's end,
dense noise at ratio 2.0, the rows that disturb one lane of a wave alone --, with six quiet blocks appended: ten quiet blocks lead in,
events at blocks 12, 16 and 20 leave codes other than 1 in the carried mask row, and the row is all ones again between them and in the
tail.

(The file was written for a word in ChanSmall that let these kernels skip the carried mask row while it is all ones; that change did not
pass its timing gate -- profiles/README.md, top section; profiles/experiments/mask_word.diff -- and the sequences stayed: they are the
ones in which a stale or misplaced scalar of the row shows in the audio.)"""
import numpy as np
import pytest

import blanker_scenarios as B
import four_wave_scenarios as F
import test_gpu_blanker as G
from cases import USB
from helpers import S, Hip

pytestmark = pytest.mark.gpu

ONE, LOOP, STREAM = G.ONE, G.LOOP, G.STREAM
C2 = [S("setDemodMode", USB), S("enableAudioFilter")]
TAIL = 6                                          # quiet blocks behind the recipe's own 24
FORMS = {"mw_u": (F.N, [], F.MW_U), "mw": (F.N, [S("setOutputGain", 0.7, sel=F.MID)], F.MW), "one-8": (8, [], ONE), "one-24": (24, [], ONE)}
EVERY = list(FORMS)


def _with_tail(I, Q):
    tI, tQ = B._finish(*B.background(I.shape[0], TAIL, seed0=4242))
    I, Q = np.concatenate([I, tI], axis=1), np.concatenate([Q, tQ], axis=1)
    I.setflags(write=False); Q.setflags(write=False)
    return I, Q


def _live_rows():
    """32 rows, interleaved so that the first 8 hold every kind: 11 single impulses at p = 117..127 (the trailing edge is found a call later from
    the carried codes), 13 pairs whose second impulse lies in the next block, 8 rows of dense noise"""
    pos, pairs, dense = B.POSITIONS.rows(), B.PAIRS.rows(), B.DENSE[1].rows()
    across = [B.pair_row(d, p0) for p0 in B.PAIR_P0 for d in B.PAIR_D if p0 < 128 <= p0 + d]
    assert len(across) == 24
    pick = [(pos, 117), (pairs, across[-1]), (dense, 0), (pos, 127), (pairs, across[0]), (dense, 1), (pos, 122), (pairs, across[9])]
    pick += [(pos, p) for p in range(117, 128) if p not in (117, 122, 127)] + [(pairs, r) for r in across[1:-1:2] if r != across[9]][:10] + \
            [(dense, r) for r in range(2, 8)]
    assert len(pick) == 32 and len(set((id(src), r) for src, r in pick)) == 32
    return _with_tail(np.stack([src[0][r] for src, r in pick]), np.stack([src[1][r] for src, r in pick]))


def _wave_rows():
    return _with_tail(*B.ONE_IN_A_WAVE[0].rows())


LIVE = B.Recipe("live+tail", B._Shared(_live_rows), setup=[S("setNoiseBlankerThreshold", 2.0)])
WAVE = B.Recipe("one-in-a-wave+tail", B._Shared(_wave_rows), setup=[S("setNoiseBlankerThreshold", 1.5)])
_ORACLES = {}


def _case(ao, recipe, form):
    """(scenario, oracle run) of a recipe on a form's bank: computed once, shared, read-only"""
    n, behind, _k = FORMS[form]
    key = (recipe.name, n, bool(behind))
    if key not in _ORACLES:
        sc = B.scenario(recipe, n=n, front=C2, behind=behind)
        bI, bQ = recipe.rows()
        run = G._Oracles(ao, sc, bI, bQ, None)
        run.audio.setflags(write=False)
        _ORACLES[key] = (sc, run)
    return _ORACLES[key]


class _Bank:
    """the recipe's blocks on the device, and the calls that play them into a batch against the oracle run"""

    def __init__(self, gpu, ao, recipe, form):
        self.gpu, self.form, self.recipe = gpu, form, recipe
        self.sc, self.run = _case(ao, recipe, form)
        self.n, self.T = self.sc.n, recipe.T
        bI, bQ = recipe.rows()
        self.hip = Hip()
        self.dI, self.dQ = self.hip.upload(G._tile(bI, self.n)), self.hip.upload(G._tile(bQ, self.n))
        self.batches = []

    def batch(self, configure=True):
        b = self.gpu.AudioSDRBatch(self.n)
        self.batches.append(b)
        b.set_stream_fir_helpers(0)
        if configure:
            F.apply_to_batch(b, self.sc.setup, self.n)
        return b

    def play(self, b, pos, calls, script=True):
        """calls of the given block counts from block `pos` on; returns the block behind the last one"""
        n, T = self.n, self.T
        dO = self.hip.malloc(n * T * 256)
        first = pos
        pipelined = b.stream_pipeline_launches()
        self.gpu.binding.kernels_launched(reset=True)
        for k in calls:
            if script and pos in self.sc.script:
                F.apply_to_batch(b, self.sc.script[pos], n)
            b.update_device_strided(self.dI + pos * 256, self.dQ + pos * 256, dO + pos * 256, k, T, T, 0)
            b.synchronize()
            pos += k
            got = {name: v for name, v in self.gpu.binding.kernels_launched(reset=True).items() if name != "asdr_reset_kernel"}
            if k >= 8:                            # the block pipeline (one FIR helper wave), bracketed by its snapshot / fallback launches
                pipelined += 1
                assert got.get(STREAM) == 1 and set(got) <= G.STREAM_AROUND | {STREAM}, got
                assert b.stream_pipeline_launches() == pipelined and b.stream_pipeline_recoveries() == 0
            else:
                want = {FORMS[self.form][2]: 1} if k == 1 else {LOOP: 1}
                assert got == want, "call of %d blocks ending at %d: launched %s, expected %s" % (k, pos, got, want)
            nb = b.read_status()["nb_detected"]
            bad = np.flatnonzero(nb != self.run.nb[:, pos - 1])
            assert bad.size == 0, "nb_detected after block %d: %d channels differ, first %d" % (pos - 1, bad.size, bad[0])
        got = self.hip.download(dO, (n, T, 128), np.int16)[:, first:pos]
        bad = np.argwhere(got != self.run.want()[:, first:pos])
        assert bad.size == 0, "%d samples differ, first at (channel, block - %d, sample) %s" % (len(bad), first, bad[0].tolist())
        return pos

    def close(self):
        self.hip.free_all()
        for b in self.batches:
            b.close()


def _ids(values):
    return dict(argvalues=values, ids=values)


@pytest.mark.parametrize("form", **_ids(EVERY))
@pytest.mark.parametrize("recipe", [LIVE, WAVE], ids=lambda r: r.name)
def test_live_and_quiet_blocks_in_turn(gpu, ao, recipe, form):
    """One-block calls: twelve quiet blocks, then events at blocks 12, 16 and 20 -- each scanned by the next call, which writes the carried
    mask row; p >= 117, the pairs across the block's end and the dense rows keep codes other than 1 in the row for a call or more, which the
    following calls must read -- with quiet blocks between them and six behind the last.  With the one-in-a-wave rows a single lane of a wave
    carries the live mask and takes its wave along."""
    bank = _Bank(gpu, ao, recipe, form)
    try:
        assert bank.play(bank.batch(), 0, [1] * bank.T) == B.T_STD + TAIL
    finally:
        bank.close()


@pytest.mark.parametrize("form", **_ids(EVERY))
@pytest.mark.parametrize("kind", ["ratio", "off-on", "mode"])
def test_reset_on_a_live_mask(gpu, ao, kind, form):
    """A threshold setter, the blanker off and on, and a mode change away and back (ASDR_R_NB) in front of blocks at all three ring phases, on
    rows whose carried mask is not all ones just then: the reset fills the row with ones and zeroes the ring's gains in ChanSmall."""
    bank = _Bank(gpu, ao, B.setter_recipe(kind), form)
    try:
        bank.play(bank.batch(), 0, [1] * bank.T)
    finally:
        bank.close()


@pytest.mark.parametrize("form", **_ids(EVERY))
@pytest.mark.parametrize("recipe,cut", [(LIVE, 14), (WAVE, 11)], ids=["live-mask", "all-ones-mask"])
def test_state_record_across_the_row(gpu, ao, recipe, cut, form):
    """A bank exported after block cut - 1 -- LIVE at 14: two calls behind the event of block 12, every disturbed row's carried mask is not all
    ones; WAVE at 11: every mask all ones, the event comes a block later -- into fresh batches that have run 0, 1 and 2 blocks (all three
    positions of the blanker ring: the gains in ChanSmall rotate with it); the rest of the recipe follows on each.  The records read back right
    after the import are the source's, byte for byte."""
    bank = _Bank(gpu, ao, recipe, form)
    try:
        src = bank.batch()
        bank.play(src, 0, [1] * cut)
        rec = src.export_state()
        for k_dst in range(3):
            d = bank.batch(configure=False)
            for k in range(k_dst):                # (unrelated settings, unrelated input: only the ring position matters)
                d.update_device_strided(bank.dI + k * 256, bank.dQ + k * 256, bank.hip.malloc(bank.n * 256), 1, bank.T, 1, 0)
            d.import_state(rec)
            assert np.array_equal(d.export_state(), rec), "records differ right after the import (destination at %d blocks)" % k_dst
            bank.play(d, cut, [1] * (bank.T - cut))
        bank.play(src, cut, [1] * (bank.T - cut))  # export reads only
    finally:
        bank.close()


@pytest.mark.parametrize("form", **_ids(["one-8", "one-24"]))
def test_multi_block_calls_then_one_block_calls(gpu, ao, form):
    """The in-kernel block loop (a call of 3 blocks over the event of block 12) and the block pipeline (a call of 8 blocks that ends two calls
    behind the event of block 20, on a live mask; its snapshot copies the whole ChanSmall row) followed by one-block calls."""
    bank = _Bank(gpu, ao, LIVE, form)
    try:
        calls = [1] * 11 + [3, 1, 8] + [1] * 7
        assert sum(calls) == bank.T
        bank.play(bank.batch(), 0, calls)
    finally:
        bank.close()

