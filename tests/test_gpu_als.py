"""The adaptive line suppressor in every launch form that carries it, on the parameter layouts of tests/als_scenarios.py, against the oracle
at tolerance 0.  One case per (form, recipe):

  - the int16 audio of every channel and block;
  - after the last call (migrations: after every call) the state records' als_w (128 floats) and als_x (256 floats) of every channel whose
    filter is enabled, as bit patterns against the oracle's taps and input buffer.  A record's als_x is in canonical order (DESIGN 3.9:
    slot j of the record is physical slot j xor als_phase xor 1): first the block processed last, then the slot the next block goes to,
    which holds the block before it -- the oracle's buffer is the other way round, previous block then last block;
  - on the taps forms the ALS and AGC stage taps of every fifth channel after every call;
  - the launch census of every call (binding.kernels_launched) against als_scenarios.census, the host's plan restated -- on a regular bank
    that is the form's stated dict (tests/test_als_scenarios.py holds the two together).

    form         how it is reached                                          kernels of a call on a regular bank
    one          one block per call                                         asdr_update_kernel_als_small_one
    loop         calls of 2, 3, 5 blocks, ASDR_NO_ALS_ROLE_STREAMS           asdr_update_kernel_als_small
    small_mixed  whole waves + 5                                            ..._als_small_one + asdr_update_kernel_als_mixed (the remainders)
    full         M > 64, D < 0 or D + M > 65                                asdr_update_kernel_als
    full_mixed   ... whole waves + 5                                        asdr_update_kernel_als + asdr_update_kernel_als_mixed
    split        set_als_launch_form(8)                                     asdr_als_pre_kernel + asdr_als_kernel
    roles2       ASDR_ALS_ROLE_STAGES=2, calls of 2, 3, 5                   asdr_als_stage_seed_kernel, asdr_als_pre_loop_kernel, asdr_als_kernel
    roles3       ASDR_ALS_ROLE_STAGES=3, calls of 2, 3, 5                   seed, asdr_sam_pre_loop_kernel_uniform, asdr_als_back_loop_kernel, asdr_als_kernel
    sam3         SAM, set_sam_launch_form(False, 8)                         asdr_sam_pre_kernel_uniform | asdr_sam_pll_kernel | asdr_sam_post_als_kernel_uniform
    sam3_mixed   ... whole waves + 5                                        ... + asdr_update_kernel_als_mixed (the remainders)
    sam_fused    SAM, set_sam_launch_form(True)                             asdr_update_kernel_als
    one-taps, full-taps: one / full with enable_taps

These are all ten kernels of the launch census whose name contains `als` (tests/test_als_scenarios.py::test_census_closure)."""
import numpy as np
import pytest

import als_scenarios as L
import four_wave_scenarios as F
from helpers import Hip, f32_bits

pytestmark = pytest.mark.gpu
TAP_EVERY = 5


class _Oracles:
    """one oracle per channel of a bank, block by block: audio, the filter's taps and input buffer and the ALS / AGC stage taps after every block"""

    def __init__(self, ao, bank):
        n = bank.n
        I, Q = L.rows(bank.form.mode)
        self.audio = np.empty((n, L.T, 128), np.int16)
        self.w = np.empty((n, L.T, 128), np.float32); self.x = np.empty((n, L.T, 256), np.float32)
        self.taps = {"ALS": np.empty((n, L.T, 128), np.float32), "AGC": np.empty((n, L.T, 128), np.float32)}
        self.enabled = np.array([[p.en for _m, p in st] for st in bank.states()]).T          # [n][T]
        for c in range(n):
            o = ao.OracleSDR(taps=True)
            by = {}
            for blk, meth, args in bank.channel_script(c):
                by.setdefault(blk, []).append((meth, args))
            for blk in range(L.T):
                for meth, args in by.get(blk, ()):
                    getattr(o, meth)(*args)
                self.audio[c, blk] = o.update(I[c % L.U, blk], Q[c % L.U, blk])
                self.w[c, blk], self.x[c, blk] = o.als_taps(), o.als_history()
                for name in self.taps:
                    self.taps[name][c, blk] = o.tap(name)
        for a in (self.audio, self.w, self.x):
            a.setflags(write=False)


_ORACLES = {}


def _case(ao, form, recipe_name):
    """(bank, oracles): one oracle run per (recipe, class, mode, appended channels), shared by the forms that differ in the launch only"""
    bank = L.Bank(L.RECIPES[recipe_name](form.klass), form)
    key = (recipe_name, form.klass, form.mode, form.rem)
    if key not in _ORACLES:
        _ORACLES[key] = _Oracles(ao, bank)
    return bank, _ORACLES[key]


def _tile(a, n):
    return np.ascontiguousarray(np.tile(a, ((n + a.shape[0] - 1) // a.shape[0], 1, 1))[:n])


def _compare_state(gpu, b, run, blk, what):
    """the records of every channel whose filter is enabled against the oracle as block blk left it"""
    rec = b.export_state()
    on = np.flatnonzero(run.enabled[:, blk])
    w = gpu.binding.state_field(rec, "als_w")[on]
    x = gpu.binding.state_field(rec, "als_x")[on]
    bad = np.flatnonzero((f32_bits(w) != f32_bits(run.w[on, blk])).any(axis=1))
    assert bad.size == 0, "%s: als_w of %d channels differs, first channel %d (taps %s)" % (
        what, bad.size, on[bad[0]], np.flatnonzero(f32_bits(w[bad[0]]) != f32_bits(run.w[on[bad[0]], blk]))[:8].tolist())
    for half, lo in (("the last block", 128), ("the block before it", 0)):      # canonical order: see the head of this file
        got = x[:, :128] if lo == 128 else x[:, 128:]
        bad = np.flatnonzero((f32_bits(got) != f32_bits(run.x[on, blk, lo:lo + 128])).any(axis=1))
        assert bad.size == 0, "%s: als_x (%s) of %d channels differs, first channel %d" % (what, half, bad.size, on[bad[0]])


def _run(gpu, ao, form, recipe_name, monkeypatch):
    for name in ("ASDR_NO_ALS_ROLE_STREAMS", "ASDR_ALS_ROLE_STAGES", "ASDR_ALS_SPLIT_MIN"):
        monkeypatch.delenv(name, raising=False)
    for name, value in form.env.items():          # (read at asdr_create)
        monkeypatch.setenv(name, value)
    bank, run = _case(ao, form, recipe_name)
    recipe, n = bank.recipe, bank.n
    I, Q = L.rows(form.mode)
    states = bank.states()
    hip = Hip()
    b = gpu.AudioSDRBatch(n)
    try:
        dI, dQ, dO = hip.upload(_tile(I, n)), hip.upload(_tile(Q, n)), hip.malloc(n * L.T * 256)
        if form.sam is not None:
            b.set_sam_launch_form(*form.sam)
        if form.als_split:
            b.set_als_launch_form(form.als_split)
        if form.taps:
            b.enable_taps(True)
        F.apply_to_batch(b, bank.setup(), n)
        pos, calls = 0, form.calls(recipe)
        for k in calls:
            for chans, meth, args in bank.events.get(pos, ()):
                for c in chans:
                    getattr(b, meth)(*args, ch=c)
            gpu.binding.kernels_launched(reset=True)
            b.update_device_strided(dI + pos * 256, dQ + pos * 256, dO + pos * 256, k, L.T, L.T, 0)
            b.synchronize()
            got = {name: v for name, v in gpu.binding.kernels_launched(reset=True).items() if name != "asdr_reset_kernel"}
            want = L.census(states[pos], k, form)
            pos += k
            assert got == want, "call of %d blocks ending at %d: launched %s, expected %s" % (k, pos, got, want)
            if form.taps:
                taps = b.read_taps()
                for c in range(0, n, TAP_EVERY):
                    for name in ("ALS", "AGC"):
                        assert np.array_equal(f32_bits(taps[name][c]), f32_bits(run.taps[name][c, pos - 1])), "block %d channel %d tap %s" % (pos - 1, c, name)
            if recipe.every_call or pos == L.T:
                _compare_state(gpu, b, run, pos - 1, "after block %d" % (pos - 1))
        got = hip.download(dO, (n, L.T, 128), np.int16)
        bad = np.argwhere(got != run.audio)
        assert bad.size == 0, "%d samples differ, first at (channel, block, sample) %s" % (len(bad), bad[0].tolist())
    finally:
        hip.free_all(); b.close()


@pytest.mark.parametrize("form,recipe", L.cells(), ids=lambda v: v)
def test_als(gpu, ao, form, recipe, monkeypatch):
    _run(gpu, ao, L.FORMS[form], recipe, monkeypatch)
