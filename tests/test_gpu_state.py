"""Receiver state records on the GPU (include/asdr.h "receiver state records"): a receiver that is exported, imported
somewhere else -- another batch, another channel index, another block count, another shard, another launch form -- and run on gives,
bit for bit, the int16 audio, the 12 stage taps and every getter of the oracle instance that was never interrupted.  Tolerance 0
everywhere; every call goes through the C ABI."""
import numpy as np
import pytest

from cases import CASES
from helpers import S, Hip, apply_setters, f32_bits
from test_control_plane import F_GETTERS, I_GETTERS

pytestmark = pytest.mark.gpu


# ---- the oracle side: one uninterrupted run per (case, script), recorded block by block and shared ------------------------------------------
def _orc_getters(o):
    return ([f32_bits(np.float32(getattr(o, g)())).item() for g in F_GETTERS] + [int(getattr(o, g)()) for g in I_GETTERS] +
            [f32_bits(np.float32(o.getAGClookup(i))).item() for i in range(130)])


def _batch_getters(b, ch):
    return ([f32_bits(np.float32(getattr(b, g)(ch))).item() for g in F_GETTERS] + [int(getattr(b, g)(ch)) for g in I_GETTERS] +
            [f32_bits(np.float32(b.getAGClookup(i, ch))).item() for i in range(130)])


def _orc_status(o):
    return (int(o.AGCisActive()), int(o.NoiseBlankerDetection()), int(o.getSAMphaseLockStatus()),
            f32_bits(np.float32(o.getSAMfrequency())).item(), f32_bits(np.float32(o.getAMcarrierLevel())).item())


def _batch_status(st, ch):
    return (int(st["agc_active"][ch]), int(st["nb_detected"][ch]), int(st["sam_locked"][ch]),
            f32_bits(st["sam_frequency"][ch]).item(), f32_bits(st["am_carrier"][ch]).item())


class Ref:
    """Oracles of one case run for `total` blocks with `script` = {block: setters applied in front of it}: audio [c][b][128], taps
    [b][t][c][128] (bits), status [b][c], getters [b][c] as each block left them."""

    def __init__(self, ao, gpu, name, total, script=None):
        from audiosdr_amd.synth import make_iq
        self.n, _, self.setters, sig = CASES[name]
        self.total, self.script = total, script or {}
        self.I, self.Q = make_iq(self.n, total, **sig)
        orcs = [ao.OracleSDR(taps=True) for _ in range(self.n)]
        apply_setters(None, orcs, self.setters)
        self.audio = np.zeros((self.n, total, 128), np.int16)
        self.taps = np.zeros((total, len(gpu.TAPS), self.n, 128), np.uint32)
        self.status, self.getters, self.extra = [], [], []
        for b in range(total):
            apply_setters(None, orcs, self.script.get(b, []))
            for c, o in enumerate(orcs):
                self.audio[c, b] = o.update(self.I[c, b], self.Q[c, b])
                for t, tn in enumerate(gpu.TAPS):
                    self.taps[b, t, c] = f32_bits(o.tap(tn))
            self.status.append([_orc_status(o) for o in orcs])
            self.getters.append([_orc_getters(o) for o in orcs])
            self.extra.append([o.agc_running() + (o.chain_constants()[0],) for o in orcs])
        for a in (self.I, self.Q, self.audio, self.taps):
            a.setflags(write=False)


_REFS = {}


def _ref(ao, gpu, name, total, script_key=None, script=None):
    key = (name, total, script_key)
    if key not in _REFS:
        _REFS[key] = Ref(ao, gpu, name, total, script)
    return _REFS[key]


GRID_SCRIPT = {4: [S("setDemodMode", 4, sel=lambda c: c in (3, 11))],
               5: [S("setDemodMode", 3, sel=lambda c: c == 3), S("setDemodMode", 4, sel=lambda c: c == 11)]}   # (their modes of the case: c % 7)


def _grid_ref(ao, gpu):
    return _ref(ao, gpu, "mixed_modes_als_c4", 20, "grid", GRID_SCRIPT)


def _source(gpu, ref, upto, taps=False):
    """The case's batch, run through blocks 0 .. upto-1 (its script applied), audio compared on the way."""
    b = gpu.AudioSDRBatch(ref.n)
    if taps:
        b.enable_taps(True)
    apply_setters(b, [_Null()] * ref.n, ref.setters)
    _run_source(b, ref, 0, upto)
    return b


class _Null:
    def __getattr__(self, name):
        return lambda *a: None


def _run_source(b, ref, lo, hi, status=True, script=True):
    for k in range(lo, hi):
        if script:
            apply_setters(b, [_Null()] * ref.n, ref.script.get(k, []))
        got = b.update(ref.I[:, k:k + 1], ref.Q[:, k:k + 1])[:, 0]
        assert np.array_equal(got, ref.audio[:, k]), "source block %d" % k
        if status:
            st = b.read_status()
            assert [_batch_status(st, c) for c in range(ref.n)] == ref.status[k], "source status after block %d" % k


def _destination(gpu, n, k_run, seed=7, taps=True):
    """A batch of n channels with unrelated settings, advanced k_run blocks on unrelated input."""
    from audiosdr_amd.synth import make_iq
    d = gpu.AudioSDRBatch(n)
    if taps:
        d.enable_taps(True)
    for c in range(n):
        d.setDemodMode((3 * c + seed) % 7, ch=c)
        d.setAGCthreshold(-50.0 + c % 5, ch=c)
        d.setOutputGain(0.25 + 0.05 * (c % 4), ch=c)
    d.setNoiseBlankerThreshold(2.0)
    d.enableALSfilter(ch=n // 2); d.setALSfilterParams(40, 0.3, 5.0, ch=n // 2)
    d.enableAudioFilter(); d.setAudioFilter(4, ch=1 % n)
    if k_run:
        I, Q = make_iq(n, k_run, fc=7100.0, A=0.4, m=0.3, noise=0.05, impulse_every=300)
        d.update(I, Q)
    return d


def _follow(gpu, d, ref, dest_of, k0, n_blocks, tap_channels=None, taps=True):
    """Blocks k0 .. k0+n_blocks-1 of the case's input into destination channels dest_of[c]; audio, taps, status, getters vs the oracles."""
    nd = d.n_channels
    chans = list(range(ref.n))
    for k in range(k0, k0 + n_blocks):
        I = np.zeros((nd, 1, 128), np.int16); Q = np.zeros((nd, 1, 128), np.int16)
        for c in chans:
            I[dest_of[c], 0] = ref.I[c, k]; Q[dest_of[c], 0] = ref.Q[c, k]
        got = d.update(I, Q)[:, 0]
        tp = d.read_taps() if taps else None
        st = d.read_status()
        for c in chans:
            dc = dest_of[c]
            assert np.array_equal(got[dc], ref.audio[c, k]), "block %d receiver %d (channel %d)" % (k, c, dc)
            assert _batch_status(st, dc) == ref.status[k][c], "status after block %d receiver %d" % (k, c)
            if taps and (tap_channels is None or c in tap_channels):
                for t, tn in enumerate(gpu.TAPS):
                    assert np.array_equal(f32_bits(tp[tn][dc]), ref.taps[k, t, c]), "block %d receiver %d tap %s" % (k, c, tn)
    for c in chans:
        assert _batch_getters(d, dest_of[c]) == ref.getters[k0 + n_blocks - 1][c], "getters of receiver %d" % c


# ---- 6 + 8: the phase grid, and the canonical bytes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_src", [6, 7, 8, 9, 10, 11])
def test_phase_grid(gpu, ao, k_src):
    """Source after k_src blocks (blanker ring at k_src % 3, ALS ring at k_src % 2, channels 3 and 11 with the other Hilbert parity: a block
    in AM) into destinations that have run k_dst = 0 .. 5 blocks, receiver c to channel (5 c + 3) % 29; 8 blocks follow.  The records
    read back from the destination right after the import -- and again after one more block on both sides -- are the source's, byte for
    byte.  The source runs on to block 20 against its oracles: export reads only."""
    ref = _grid_ref(ao, gpu)
    dest_of = [(5 * c + 3) % 29 for c in range(ref.n)]
    src = _source(gpu, ref, k_src)
    rec = src.export_state()
    assert rec.shape == (ref.n, gpu.AudioSDRBatch.STATE_RECORD_BYTES)
    _run_source(src, ref, k_src, k_src + 1)
    rec1 = src.export_state()
    for k_dst in range(6):
        d = _destination(gpu, 29, k_dst, seed=k_dst)
        before = d.export_state()
        d.import_state(rec, dest_of)
        after = d.export_state()
        assert np.array_equal(after[dest_of], rec), "k_dst %d: records differ right after the import" % k_dst
        others = [c for c in range(29) if c not in dest_of]
        assert np.array_equal(after[others], before[others]), "k_dst %d: untouched channels changed" % k_dst
        _follow(gpu, d, ref, dest_of, k_src, 1)
        assert np.array_equal(d.export_state(dest_of), rec1), "k_dst %d: records differ one block later" % k_dst
        _follow(gpu, d, ref, dest_of, k_src + 1, 7)
        d.close()
    _run_source(src, ref, k_src + 1, 20)
    src.close()


# ---- 7: every case of tests/cases.py --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_cut_twice(gpu, ao, name):
    """The case's own channel count, setters and signal for its block count + 8: cut after block 5 into a fresh batch (phase 0) and after
    block 7 into a batch that has run 4 blocks; the rest of the signal follows.  Taps on channel 0 and the last one."""
    n_ch, n_blk = CASES[name][0], CASES[name][1]
    ref = _ref(ao, gpu, name, n_blk + 8)
    if name == "sam_c3":
        assert all(s[2] == 1 for s in ref.status[5]), "the case is meant to be locked at the cut"
    if name == "agc_slow_hang":
        assert all(0 < e[0] < e[2] for e in ref.extra[5]), "the hang counter is meant to be mid-count at the cut: %s" % (ref.extra[5],)
    src = _source(gpu, ref, 6)
    for cut, k_dst in ((6, 0), (8, 4)):
        _run_source(src, ref, 6, cut)
        d = _destination(gpu, n_ch + 3, k_dst, seed=cut)
        dest_of = [(c + 2) % (n_ch + 3) for c in range(n_ch)]
        d.import_state(src.export_state(), dest_of)
        _follow(gpu, d, ref, dest_of, cut, ref.total - cut, tap_channels=(0, n_ch - 1))
        d.close()
    src.close()


# ---- 9: pending setters ------------------------------------------------------------------------------------------------------------------------
def test_setters_pending_at_the_export(gpu, ao):
    """Setters called after block 6 and exported WITHOUT an update in between: the resets they leave pending (IF state, ALS rows, blanker
    ring, audio filter state) act on the imported receivers' next block as on the oracles'."""
    script = dict(GRID_SCRIPT)
    script[7] = [S("setDemodMode", 1, sel=lambda c: c in (2, 9)), S("enableALSfilter", sel=lambda c: c == 4),
                 S("setNoiseBlankerThresholdDb", 6.0, sel=lambda c: c == 5), S("enableAudioFilter", sel=lambda c: c in (6, 9)),
                 S("setAudioFilter", 3, sel=lambda c: c in (6, 9))]
    ref = _ref(ao, gpu, "mixed_modes_als_c4", 13, "pending", script)
    src = _source(gpu, ref, 7)
    apply_setters(src, [_Null()] * ref.n, script[7])
    rec = src.export_state()
    d = _destination(gpu, 29, 2)
    dest_of = [(5 * c + 3) % 29 for c in range(ref.n)]
    d.import_state(rec, dest_of)
    _follow(gpu, d, ref, dest_of, 7, 6)
    d.close()
    _run_source(src, ref, 7, 13, script=False)   # the source goes on too (the setters are already applied to it)
    src.close()


# ---- 10: device form, shards, streams --------------------------------------------------------------------------------------------------------
def test_device_form_between_shards_on_streams(gpu, ao):
    """A 2-shard batch on device 0, 32 channels (USB / AM / SAM).  After 6 blocks, with no host synchronisation anywhere: the records of
    channels 2..13 (shard 0) to device memory on a caller's stream, from there into channels 29..18 (shard 1, reversed), then 6 single-block
    calls on the batch's own stream.  The moved receivers continue their oracles, every other channel is unaffected."""
    from audiosdr_amd.synth import make_iq
    n, T = 32, 12
    I, Q = make_iq(n, T, fc=6890.0 + (np.arange(n) % 5 - 2) * 30.0, A=0.3, m=0.5, noise=0.01, impulse_every=800)
    mode = lambda c: (1, 4, 5)[c % 3]
    orcs = [ao.OracleSDR() for _ in range(n)]
    b = gpu.AudioSDRBatch(n, devices=[0, 0])
    for c in range(n):
        b.setDemodMode(mode(c), ch=c); orcs[c].setDemodMode(mode(c))
    b.setNoiseBlankerThresholdDb(10.0)
    for o in orcs:
        o.setNoiseBlankerThresholdDb(10.0)
    want = np.stack([orcs[c].update(I[c], Q[c]).reshape(T, 128) for c in range(n)])
    src = list(range(2, 14)); dst = list(range(29, 17, -1))
    Iin, Qin = I.copy(), Q.copy()
    for s_, d_ in zip(src, dst):
        Iin[d_, 6:] = I[s_, 6:]; Qin[d_, 6:] = Q[s_, 6:]
    hip = Hip()
    dI, dQ, dO = hip.upload(Iin), hip.upload(Qin), hip.malloc(n * T * 256)
    dR = hip.malloc(len(src) * b.STATE_RECORD_BYTES)
    s1, s2 = hip.stream(), hip.stream()
    for k in range(6):
        b.update_device_strided(dI + k * 256, dQ + k * 256, dO + k * 256, 1, T, T, s1)
    b.export_state_device(dR, src, stream=s2)
    b.import_state_device(dR, dst, stream=s2)
    for k in range(6, T):
        b.update_device_strided(dI + k * 256, dQ + k * 256, dO + k * 256, 1, T, T, gpu.STREAM_BATCH)
    b.synchronize(); hip.sync()
    got = hip.download(dO, (n, T, 128), np.int16)
    for c in range(n):
        if c in dst:
            s_ = src[dst.index(c)]
            assert np.array_equal(got[c, 6:], want[s_, 6:]), "moved receiver %d in channel %d" % (s_, c)
            assert np.array_equal(got[c, :6], want[c, :6])
        else:
            assert np.array_equal(got[c], want[c]), "channel %d" % c
    st = b.read_status()
    for c in range(n):
        o = orcs[src[dst.index(c)]] if c in dst else orcs[c]
        assert _batch_status(st, c) == _orc_status(o), "status of channel %d" % c
    hip.free_all(); b.close()


# ---- 11: four-wave bank ------------------------------------------------------------------------------------------------------------------------
def test_four_wave_bank_keeps_its_launch_form(gpu, ao):
    """512 channels with C2's settings: 7 blocks, everything exported and imported in reversed channel order into a fresh bank that has run
    2 blocks.  The next 6 blocks equal the oracles' and run on the launch-constant four-wave kernel (the imported rows are equal); one
    record's output gain edited on the host sends the group to the kernel that reads the rows, and the audio follows an oracle with that gain."""
    from test_gpu_uniform_params import MW, MW_U, UNIQ, _Run, _c2, _census, _inputs, _oracle
    n, T = 512, 16
    bI, bQ = _inputs(T, impulse_every=1300)
    want = _oracle(ao, bI, bQ, _c2)
    want_g = _oracle(ao, bI, bQ, _c2, changes=((13, lambda o: o.setOutputGain(0.8)),))
    src = _Run(gpu, n, bI, bQ, _c2)
    src.step(7, gpu.STREAM_BATCH)
    rec = src.b.export_state()
    # destination channel d holds receiver 511 - d, whose input row is (511 - d) % UNIQ
    rows = [(n - 1 - d) % UNIQ for d in range(n)]
    dst = _Run(gpu, n, bI[rows[:UNIQ]], bQ[rows[:UNIQ]], _c2)     # (n - 1 - d) % 8 has period 8 in d
    dst.step(2, gpu.STREAM_BATCH)
    dst.pos = 7
    dst.b.import_state(rec, list(range(n - 1, -1, -1)))
    _census(gpu)
    dst.step(6, gpu.STREAM_BATCH)
    got = dst.audio()
    assert _census(gpu) == {MW_U: 6}
    assert dst.b.params_uniform_groups()[0] == 1
    for d in range(n):
        assert np.array_equal(got[d, 7:13], want[rows[d], 7:13]), "channel %d" % d
    one = dst.b.export_state([5])
    gpu.state_field(one, "output_gain")[0] = np.float32(0.8)
    dst.b.import_state(one, [5])
    dst.step(3, gpu.STREAM_BATCH)
    got = dst.audio()
    assert _census(gpu) == {MW: 3}
    for d in range(n):
        w = want_g if d == 5 else want
        assert np.array_equal(got[d, 13:16], w[rows[d], 13:16]), "channel %d after the edit" % d
    src.close(); dst.close()


# ---- 12: multi-block calls after an import ------------------------------------------------------------------------------------------------
def test_multi_block_calls_after_import(gpu, ao):
    """wspr_sketch on 16 channels, cut after 5 blocks into a batch at phase 1; then ONE call of 7 blocks and one of 2."""
    from audiosdr_amd.synth import make_iq
    n, T = 16, 14
    setters, sig = CASES["wspr_sketch"][2], CASES["wspr_sketch"][3]
    I, Q = make_iq(n, T, **sig)
    orcs = [ao.OracleSDR() for _ in range(n)]
    src = gpu.AudioSDRBatch(n)
    apply_setters(src, orcs, setters)
    want = np.stack([orcs[c].update(I[c], Q[c]).reshape(T, 128) for c in range(n)])
    assert np.array_equal(src.update(I[:, :5], Q[:, :5]), want[:, :5])
    d = _destination(gpu, n, 1, taps=False)
    d.import_state(src.export_state())
    assert np.array_equal(d.update(I[:, 5:12], Q[:, 5:12]), want[:, 5:12])
    assert np.array_equal(d.update(I[:, 12:], Q[:, 12:]), want[:, 12:])
    st = d.read_status()
    assert [_batch_status(st, c) for c in range(n)] == [_orc_status(o) for o in orcs]
    src.close(); d.close()


# ---- 13: a control-only record ------------------------------------------------------------------------------------------------------------------
def test_control_only_record_starts_from_power_on(gpu, ao):
    """Records of an ASDR_NO_DEVICE batch carry settings only: loaded into a device batch that has run 5 blocks, the channels equal oracles
    configured the same way from power-on."""
    from audiosdr_amd.synth import make_iq
    name = "mixed_modes_als_c4"
    n, _, setters, sig = CASES[name]
    ref = _ref(ao, gpu, name, 8)
    cp = gpu.AudioSDRBatch(n, device=gpu.NO_DEVICE)
    apply_setters(cp, [_Null()] * n, setters)
    rec = cp.export_state()
    assert not gpu.state_field(rec, "content").any() and not rec[:, 160:].any()
    d = _destination(gpu, 29, 5)
    dest_of = [(5 * c + 3) % 29 for c in range(n)]
    d.import_state(rec, dest_of)
    _follow(gpu, d, ref, dest_of, 0, 8)
    cp.close(); d.close()


# ---- 14: rejection on the device ----------------------------------------------------------------------------------------------------------------
def test_rejected_import_leaves_a_running_batch_alone(gpu, ao):
    """A call whose third record has a bad version, on a batch mid-run: < 0, and the batch's next 4 blocks equal the oracles' (validation is
    on the host, before any launch).  Host form and device form."""
    ref = _grid_ref(ao, gpu)
    src = _source(gpu, ref, 6)
    rec = src.export_state()
    bad = rec.copy()
    gpu.state_field(bad, "version")[2] = 2
    with pytest.raises(gpu.AsdrError, match="record 2"):
        src.import_state(bad, list(range(ref.n))[::-1])
    hip = Hip()
    dR = hip.upload(bad)
    with pytest.raises(gpu.AsdrError, match="record 2"):
        src.import_state_device(dR, list(range(ref.n))[::-1])
    assert np.array_equal(src.export_state(), rec)
    _run_source(src, ref, 6, 10)
    hip.free_all(); src.close()


# ---- 15: the blanker's carried mask, all nine pairs of ring phases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense-1.2", "pairs"])
def test_blanker_carried_mask_across_ring_phases(gpu, ao, name):
    """Banks on the designed blanker inputs of tests/blanker_scenarios.py (heavy-tailed noise: detections in every block; pairs of impulses
    whose windows merge, touch or leave a gap), cut after three block counts with ring phases 0, 1 and 2 at which every receiver's carried
    mask codes are not all ones (tests/test_blanker_scenarios.py shows it), each into destinations that have run 0, 1 and 2 blocks: the
    nine pairs of source and destination phase.  Audio and nb_detected of the next five blocks against the uninterrupted oracles; the
    source runs on to the end against them too."""
    import blanker_scenarios as B
    import four_wave_scenarios as F
    from test_gpu_blanker import FORMS, _case
    recipe = {r.name: r for r in B.all_recipes()}[name]
    sc, run = _case(ao, recipe, FORMS["one"])
    I, Q = recipe.rows()
    n, T, want = sc.n, recipe.T, run.want()
    assert n == recipe.U and {k % 3 for k in B.STATE_CUTS[name]} == {0, 1, 2}
    nd = n + 3
    dest_of = [(c + 2) % nd for c in range(n)]
    src = gpu.AudioSDRBatch(n)
    F.apply_to_batch(src, sc.setup, n)
    pos = 0
    for cut in B.STATE_CUTS[name]:
        assert np.array_equal(src.update(I[:, pos:cut], Q[:, pos:cut]), want[:, pos:cut]), "source blocks %d..%d" % (pos, cut - 1)
        pos = cut
        rec = src.export_state()
        for k_dst in (0, 1, 2):
            d = _destination(gpu, nd, k_dst, seed=cut + k_dst, taps=False)
            d.import_state(rec, dest_of)
            for k in range(cut, min(T, cut + 5)):
                dI = np.zeros((nd, 1, 128), np.int16); dQ = np.zeros((nd, 1, 128), np.int16)
                dI[dest_of, 0] = I[:, k]; dQ[dest_of, 0] = Q[:, k]
                got = d.update(dI, dQ)[:, 0]
                bad = np.argwhere(got[dest_of] != want[:, k])
                assert bad.size == 0, "cut %d into phase %d, block %d: first at (receiver, sample) %s" % (cut, k_dst, k, bad[0].tolist())
                assert np.array_equal(d.read_status()["nb_detected"][dest_of], run.nb[:, k]), "cut %d into phase %d: nb_detected after block %d" % (cut, k_dst, k)
            d.close()
    assert np.array_equal(src.update(I[:, pos:], Q[:, pos:]), want[:, pos:])
    src.close()
