"""What tests/test_gpu_four_wave.py cannot see on the GPU, shown here from the oracle and the control plane alone (no GPU):

* which AGC chain a workgroup of the four-wave kernels takes is decided inside the kernel (asdr_kernels.hip, "the LEAN chain"): the AGC
  scenarios are stepped through the oracle block by block and must contain every regime they are there for;
* which kernel the launcher takes follows from the schedule: every scenario's settings are built on a control-plane-only batch and must
  give the plain waves, the direct groups and the uniform groups the GPU file's census assertions expect."""
import numpy as np
import pytest

import four_wave_scenarios as F
from test_gpu_uniform_params import _oracle, _tile


# ---- AGC regimes ------------------------------------------------------------------------------------------------------------------------
def _regimes(ao, sc):
    """Per workgroup (32 channels) and block, from the oracles' state in front of the block, as the kernel decides it:
    a wave is QUIET when every channel of it has counter >= 128, hang count >= 8 and no |AGC input| (the AUDIO_FILT tap, clamped to 1)
    above the envelope carried in; the AGC duty runs the chains of the channels of the waves that are not quiet (the ACTIVE ones) and takes
    the LEAN chain when every active channel has counter >= 128 and hang count >= 128, the general chain otherwise."""
    bI, bQ = sc.rows()
    run = F.OracleRun(ao, sc, bI, bQ, observe_agc=True)
    ch = run.of_channel
    hang = np.array([o.chain_constants()[0] for o in run.channel_oracles()])[:, None]
    hc0, env0, bmax, hc_end = run.hc0[ch], run.env0[ch], run.bmax[ch], run.hc_end[ch]          # [n][T]
    n, T = hc0.shape
    attacks = bmax > env0                                                                       # (some sample above the envelope carried in)
    ch_quiet = (hc0 >= 128) & (hang >= 8) & ~attacks
    wave_quiet = ch_quiet.reshape(n // 8, 8, T).all(axis=1)
    active = np.repeat(~wave_quiet, 8, axis=0)
    ok = (hc0 >= 128) & (hang >= 128)
    wg = lambda a: a.reshape(n // 32, 32, T)
    any_active = wg(active).any(axis=1)
    lean = any_active & wg(~active | ok).all(axis=1)
    general = any_active & ~lean
    return dict(hang=hang, hc0=hc0, env0=env0, attacks=attacks, hc_end=hc_end, lean=lean, general=general, quiet=~any_active,
                lean_attack=lean & wg(active & attacks).any(axis=1),
                mixed=wg(hc0 < 128).any(axis=1) & wg(hc0 >= 128).any(axis=1))


@pytest.fixture(scope="module")
def agc_regimes(ao):
    return {sc.name: _regimes(ao, sc) for sc in F.agc_scenarios()}


def test_hang_times_give_the_hang_counts(ao, A):
    b = A.AudioSDRBatch(8, device=-1)
    for c, h in enumerate(F.HANG_COUNTS):
        o = ao.OracleSDR()
        if h != 4410:                                      # (the default, 100 ms, is left alone)
            o.setAGChangTime(F.hang_ms(h)); b.setAGChangTime(F.hang_ms(h), ch=c)
        assert o.chain_constants()[0] == h and b.chain_constants(c)[0] == h
    b.close()


def test_count_arrangements():
    """(a) one count per workgroup, (b) all eight in every wave, (c) a single channel per workgroup at 127"""
    a, b, c = (F.agc_count_of(k) for k in ("per-workgroup", "mixed", "one-per-workgroup"))
    for w in range(16):
        assert len({a(ch) for ch in range(32 * w, 32 * w + 32)}) == 1
        assert sorted(c(ch) for ch in range(32 * w, 32 * w + 32)) == [127] + [4410] * 31
    assert {a(32 * w) for w in range(16)} == set(F.HANG_COUNTS)
    for w in range(64):
        assert {b(ch) for ch in range(8 * w, 8 * w + 8)} == set(F.HANG_COUNTS)
    assert {(b(ch), ch % 16) for ch in range(F.N)} == {(h, r) for h in F.HANG_COUNTS for r in range(16)}


def _assert_witnesses(name, r):
    lean, general, quiet = r["lean"], r["general"], r["quiet"]
    hc0, hc_end, attacks, hang = r["hc0"], r["hc_end"], r["attacks"], r["hang"]
    found = {
        "lean block in which a channel attacks": r["lean_attack"].any(),
        "counters on both sides of 128 in one workgroup": (r["mixed"] & (lean | general)).any(),
        "counter reaching 0 strictly inside a block": ((hc0 > 0) & (hc0 < 128) & ~attacks & (hc_end == 0)).any(),
        "counter running out exactly at a block end": ((hc0 == 128) & ~attacks & (hc_end == 0)).any(),
        "counter of exactly 128 at a block start": (hc0 == 128).any(),
        "running counter re-armed by a late attack": ((hc0 > 0) & (hc0 < hang) & (hc_end > hc0)).any(),
        "lean block directly followed by a general one": (lean[:, :-1] & general[:, 1:]).any(),
        "general block directly followed by a lean one": (general[:, :-1] & lean[:, 1:]).any(),
        "block that is quiet for a whole workgroup": quiet.any(),
    }
    return found


def test_agc_scenarios_reach_every_regime(agc_regimes):
    """Each witness at least once in the three hang-count arrangements; what each arrangement is there for, in that arrangement."""
    per = {name: _assert_witnesses(name, r) for name, r in agc_regimes.items()}
    for w in per["agc-per-workgroup"]:
        assert any(per[k][w] for k in ("agc-per-workgroup", "agc-mixed", "agc-one-per-workgroup")), w
    a = agc_regimes["agc-per-workgroup"]
    assert (a["lean"].any(axis=0) & a["general"].any(axis=0)).any(), "lean and general workgroups in one launch"
    for w in ("lean block in which a channel attacks", "lean block directly followed by a general one", "general block directly followed by a lean one",
              "block that is quiet for a whole workgroup", "counter of exactly 128 at a block start", "counter reaching 0 strictly inside a block"):
        assert per["agc-per-workgroup"][w], w
    assert per["agc-mixed"]["counters on both sides of 128 in one workgroup"]
    assert per["agc-mixed"]["counter reaching 0 strictly inside a block"] and agc_regimes["agc-mixed"]["general"].all()
    c = agc_regimes["agc-one-per-workgroup"]
    assert per["agc-one-per-workgroup"]["counters on both sides of 128 in one workgroup"]
    assert c["general"].all()                               # (the wave that holds the channel at 127 is never quiet, and its channel never lean-eligible)
    for m in (1, 2, 3):                                     # hang times of 4,410 / 22,050 / 88,200 samples: lean and quiet blocks only
        r = agc_regimes["agc-mode%d" % m]
        assert r["lean_attack"].any() and r["quiet"].any()


def test_default_counter_crosses_128_on_a_fresh_bank(agc_regimes):
    r = agc_regimes["agc-default-runs-out"]
    hc0, T = r["hc0"], r["hc0"].shape[1]
    assert T > 40 and (r["hang"] == 4410).all()
    last_attack = np.array([np.flatnonzero(a)[-1] for a in r["attacks"]])
    assert set(last_attack) <= {6, 7}                       # the level drops for good after 4 blocks; the blanker delays by two, the filters by a little more
    crossing = np.array([np.flatnonzero((h < 128) & (h > 0))[0] for h in hc0])
    assert set(crossing - last_attack) <= {34, 35} and crossing.min() > 40      # 4,410 - (127 - u) - 128 j < 128 from j = 33 or 34 on
    assert (r["hc_end"][np.arange(len(hc0)), crossing] == 0).all() and r["general"][:, crossing.min():crossing.max() + 1].any()
    assert r["lean"][:, :8].any() and r["quiet"][:, 9:40].all()


# ---- launch forms, from the control plane ---------------------------------------------------------------------------------------------
def _direct_slots(b):
    """Channels in direct groups: a broadcast setter of a field no kernel of these banks reads (the ALS filter is off) refills every row,
    and the flush then passes once over the rows of every direct group (asdr_params_uniform_groups counts the rows compared)."""
    before = b.params_uniform_groups()[1]
    b.setALSfilterParams(32, 0.1, 1.0)
    b.control_plane_flush()
    return b.params_uniform_groups()[1] - before


@pytest.mark.parametrize("sc", F.all_scenarios(), ids=lambda sc: sc.name)
def test_launch_form_expectations(A, sc):
    b = A.AudioSDRBatch(sc.n, device=-1)
    F.apply_to_batch(b, sc.setup, sc.n)
    T = max(list(sc.script) + [0]) + 1
    for blk in range(T):
        F.apply_to_batch(b, sc.script.get(blk, ()), sc.n)
        st = b.control_plane_flush()
        assert st["waves_plain"] == sc.plain_waves, blk
        assert b.params_uniform_groups()[0] == sc.uniform_groups(blk), blk
        assert _direct_slots(b) == sc.direct_slots(blk), blk
        assert b.params_uniform_groups()[0] == sc.uniform_groups(blk), blk
    b.close()


def test_every_row_differs_inside_every_workgroup():
    rows = [F.channel_settings(c) for c in range(F.N)]
    for w in range(F.N // 32):
        assert len(set(rows[32 * w:32 * w + 32])) == 32
    for w in range(F.N // 8):                               # unit gain and unit balance beside other values in one wave
        gains = {r[0][1] for r in rows[8 * w:8 * w + 8]}; bal = {r[1][1] for r in rows[8 * w:8 * w + 8]}
        assert 1.0 in gains and len(gains) > 1 and 1.0 in bal and len(bal) > 1
    assert sum(r[0][1] == 1.0 and r[1][1] == 1.0 for r in rows) >= 16                   # (channels on the unit-gain path: I and Q gain both exactly 1)


def test_matrix_covers_modes_and_enables():
    cfgs = F.matrix_configs()
    assert len(cfgs) == 16 and len({c[3:7] for c in cfgs}) == 16          # the full product of the four enables
    for mname in {c[0] for c in cfgs}:
        for e in range(4):
            assert {c[3 + e] for c in cfgs if c[0] == mname} == {0, 1}, (mname, e)
    assert {c[0] for c in cfgs} == {"lsb", "usb", "cwl", "cwu", "am", "wspr", "m7", "m65535"}
    assert any(c[0] == "am" and c[5] == 1 for c in cfgs)                     # AM with the AGC on
    setters = [s for c in cfgs for s in F.matrix_scenario(c, False).setup]
    assert {s[1][0] for s in setters if s[0] == "setAudioFilter"} == {0, 1, 2, 10}
    assert {s[1][0] for s in setters if s[0] == "setAGCmode"} == {0, 1, 2, 3}
    assert any(s[0] == "set_exact_unknown_mode" and s[1] == (False,) for s in setters)


def test_enables_are_key_fields(A):
    """Switching the AGC off on a third of a bank's channels splits the bank into two settings groups: no direct group, so neither
    four-wave kernel -- why the denormal banks of the GPU file differ in AGC time constants instead."""
    b = A.AudioSDRBatch(F.N, device=-1)
    b.setDemodMode(A.USBmode); b.enableAudioFilter()
    for c in range(1, F.N, 3):
        b.disableAGC(ch=c)
    b.control_plane_flush()
    assert b.params_uniform_groups()[0] == 0 and _direct_slots(b) == 0
    b.close()


def test_per_key_oracles_agree_with_the_shared_harness(ao):
    """The C2 bank through test_gpu_uniform_params's own oracle helper: both harnesses name the same audio."""
    sc = F.geometry_scenarios()[0]
    bI, bQ = sc.rows()
    want = _tile(_oracle(ao, bI, bQ, lambda o: (o.setDemodMode(1), o.enableAudioFilter())), sc.n)
    assert np.array_equal(F.OracleRun(ao, sc, bI, bQ).want(), want)
