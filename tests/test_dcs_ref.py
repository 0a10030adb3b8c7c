"""tests/dcs_ref.py, the numpy restatement of include/asdr_dcs.h, held to known answers: the words and their classes, the decimator
against tone_ref's, the clock's at most one bit per block over every phase and edge pattern, every code of the creation table named
under voice-band noise with the bit clock off by 0.3 %, nothing named from noise alone, the confirm / hold / open rule on designed bit
streams, and that splitting a sequence into calls changes nothing.  The figures DESIGN.md 3.18 quotes are printed by these tests."""
import numpy as np
import pytest

import dcs_ref as DR
import tone_ref as TR

SECONDS = 2
NB = SECONDS * DR.FS // 128          # 689 blocks, 268 bits


def test_words_known_answers():
    assert DR.word(0o023) == 0x763813 and DR.word(0o1000) is None and DR.word(-1) is None
    words = [DR.word(c) for c in DR.CODES]
    assert len(DR.CODES) == 104 and all(w >> 9 & 7 == 4 and w & 0x1FF == c for w, c in zip(words, DR.CODES))   # the fixed bits 100
    classes = {min(DR.rotations(w)) for w in words}
    assert len(classes) == 104                                                     # 104 different rotation classes
    every = sorted({r for w in words for r in DR.rotations(w)})
    assert len(every) == 2392 and DR.min_distance(every) == 7
    assert all(min(DR.rotations(r ^ 0x7FFFFF)) in classes for r in every)          # complements stay in the table's classes ...
    assert all(min(DR.rotations(w ^ 0x7FFFFF)) != min(DR.rotations(w)) for w in words)   # ... in another class each
    assert DR.find(words, 0o023, True) == DR.find(words, 0o047) == DR.CODES.index(0o047)
    assert DR.find(words, 0o340) == DR.find(words, 0o766) == DR.find(words, 0o023) == 0
    assert DR.word(0o340) in DR.rotations(DR.word(0o023)) and DR.word(0o766) in DR.rotations(DR.word(0o023))
    assert DR.find(words, 0) == -1 and DR.find(words, 0o1000) == -1
    assert DR.STATE_DTYPE.itemsize == 192 and DR.popcount23(np.array([0, 1, 0x7FFFFF, 0x400001])).tolist() == [0, 1, 23, 2]


def test_the_decimator_is_the_tone_squelchs_and_the_bit_filter_sums_twenty():
    rng = np.random.default_rng(1)
    x = DR.to_int16(rng.normal(0.0, 9000.0, size=(3, 5 * 128))).reshape(3, 5, 128)
    r = DR.DcsRef(3)
    r.update(x[:, :2]); r.update(x[:, 2:])
    d = TR.decimate(np.zeros((3, 48), dtype=np.int64), x.reshape(3, -1).astype(np.int64))      # tone_ref's d_k on the same input
    assert np.array_equal(r.st["dhist"], d[:, -24:]) and np.array_equal(r.st["hist"], x.reshape(3, -1)[:, -48:])
    t = TR.ToneRef(3)
    t.update(x)
    assert np.array_equal(t.st["hist"], r.st["hist"])
    # one positive sample of 4096 * 16 would be d = 16 at most; a constant 1000 gives d = 1000 and s = 20000
    c = DR.DcsRef(1)
    c.update(np.full((1, 6, 128), 1000, dtype=np.int16))
    assert (c.st["dhist"][0, -20:] == 1000).all() and int(c.st["b"][0]) == 1 and int(c.st["edges"][0]) == 1


def bits_per_block(back_below):
    """The most bits a block takes over every clk and every pattern of edges, with an edge pulling the clock back below
    `back_below` and pushing it forward from there on."""
    clk = np.repeat(np.arange(DR.PERIOD), 256)
    pattern = np.tile(np.arange(256), DR.PERIOD)
    taken = np.zeros_like(clk)
    for k in range(8):
        err = np.where(clk < back_below, clk, clk - DR.PERIOD)
        clk = np.where((pattern >> k) & 1 == 1, (clk - (err >> 2)) % DR.PERIOD, clk)
        p, clk = clk, clk + DR.STEP
        taken += (p < DR.HALF) & (clk >= DR.HALF)
        clk = np.where(clk >= DR.PERIOD, clk - DR.PERIOD, clk)
    return int(taken.max())


def test_a_block_takes_at_most_one_bit():
    """Over all 2625 x 256 cases.  With the edge rule's threshold one higher (e = clk for clk < 1313) an edge at clk = 1312, right
    behind a taken bit, pulls the clock back to 984 and the block takes a second bit three steps later: that is why it is 1312."""
    assert bits_per_block(DR.HALF) == 1 and DR.HALF == 1312
    assert bits_per_block(DR.HALF + 1) == 2


def run_named(ref, x, want):
    """Block by block: (first bit count at which `want` was named or -1, whether it was ever lost after, whether another was named)."""
    n = ref.n
    first, lost, wrong = np.full(n, -1), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for b in range(x.shape[1]):
        ref.update(x[:, b:b + 1])
        det = ref.st["detected"]
        wrong |= (det >= 0) & (det != want)
        lost |= (first >= 0) & (det != want)
        first = np.where((first < 0) & (det == want), ref.st["bits"], first)
    return first, lost, wrong


def coded_channels(rng, codes, amplitude):
    """Every code normal and complemented, the bit clock 0.3 % fast and slow: 4 channels a code, two seconds, through a two-pole
    300 Hz low-pass with the word's mean removed, under 300 .. 3000 Hz noise of rms 6000 plus white noise of rms 300."""
    cases = [(c, inv, rate) for c in codes for inv in (False, True) for rate in (1.003, 0.997)]
    m = NB * 128
    x = np.stack([DR.dcs_wave(m, DR.word(c) ^ (0x7FFFFF if inv else 0), amplitude, rate=DR.BIT_RATE * rate, start_bit=rng.uniform(0.0, 23.0))
                  for c, inv, rate in cases])
    x += DR.voice_noise(rng, x.shape, 6000.0) + rng.normal(0.0, 300.0, size=x.shape)
    return cases, DR.to_int16(x).reshape(len(cases), NB, 128)


def test_all_104_codes_normal_and_complemented_under_voice_noise():
    """Amplitude 1,000, max_errors 0: each is named as the index find gives, from some bit on without a dropout, and no other code
    ever is.  The first detection needs the clock and the filters to settle (3 bits at the most here), the register to hold the word
    in the table's rotation (up to 22 bits after its first 23) and one more word: 71 bits at the most."""
    rng = np.random.default_rng(2024)
    cases, x = coded_channels(rng, DR.CODES, 1000.0)
    ref = DR.DcsRef(len(cases))
    want = np.array([ref.find(c, inv) for c, inv, _ in cases])
    assert (want >= 0).all() and all(want[4 * k] == k and want[4 * k + 2] != k for k in range(104))
    first, lost, wrong = run_named(ref, x, want)
    print("codes 104 x normal / complemented x fast / slow: latest first detection at bit", int(first.max()), "earliest", int(first.min()),
          "fewest hits", int(ref.st["hits"].min()), "of", int(ref.st["bits"].min()), "bits")
    assert (first >= 0).all() and not lost.any() and not wrong.any()
    assert first.max() <= 71 and (ref.st["detections"] == 1).all() and (ref.st["hits"] >= 8).all()


@pytest.mark.parametrize("max_errors,amplitude", [(1, 1000.0), (3, 1000.0), (0, 3000.0), (3, 3000.0)])
def test_a_subset_with_errors_allowed_and_at_a_higher_level(max_errors, amplitude):
    rng = np.random.default_rng(7 + max_errors)
    cases, x = coded_channels(rng, DR.CODES[::8], amplitude)                       # 13 codes
    ref = DR.DcsRef(len(cases))
    ref.set_max_errors(max_errors)
    want = np.array([ref.find(c, inv) for c, inv, _ in cases])
    first, lost, wrong = run_named(ref, x, want)
    print("max_errors", max_errors, "amplitude", amplitude, "latest first detection at bit", int(first.max()))
    assert (first >= 0).all() and not lost.any() and not wrong.any() and first.max() <= 71


def test_noise_alone_names_nothing():
    """The voice-band noise of the tests above, and white noise of rms 10,000, two seconds of 16 channels each, at max_errors 0 .. 3
    with confirm = 2: no detection; the unconfirmed hits are printed."""
    rng = np.random.default_rng(99)
    m = NB * 128
    voice = DR.voice_noise(rng, (16, m), 6000.0) + rng.normal(0.0, 300.0, size=(16, m))
    white = rng.normal(0.0, 10000.0, size=(16, m))
    x = DR.to_int16(np.concatenate([voice, white])).reshape(32, NB, 128)
    for max_errors in range(4):
        ref = DR.DcsRef(32)
        ref.set_max_errors(max_errors)
        ref.set_want(DR.ANY)
        out, unmuted = ref.update(x)
        print("max_errors", max_errors, "hits on voice-band noise", int(ref.st["hits"][:16].sum()), "on white noise", int(ref.st["hits"][16:].sum()),
              "in", int(ref.st["bits"].sum()), "bits; most in a channel", int(ref.st["hits"].max()))
        assert not ref.st["detections"].any() and (ref.st["detected"] == -1).all() and not unmuted.any() and not out.any()
        assert (ref.st["bits"] > 150).all() and ref.st["edges"].min() > 100   # edges pull the clock back: 167 .. 267 bits of 268
        if max_errors == 0:
            assert not ref.st["hits"].any()


def bits_to_rows(bits, amplitude=3000):
    """int16 [1][nb][128]: the bits as NRZ at exactly 2625 / 8 samples a bit, no filter, no noise."""
    nb = int(np.ceil(len(bits) * 2625 / 8 / 128))
    k = np.arange(nb * 128)
    idx = np.minimum(k * 8 // 2625, len(bits) - 1)
    return (amplitude * (2 * np.asarray(bits)[idx] - 1)).astype(np.int16).reshape(1, nb, 128)


def test_confirm_hold_and_open_on_designed_bits():
    """Word 023 four times, then word 025 twice, then a constant: confirm 2 names 023 with its second word and 025 with its
    second; 025's first word does not refresh 023's hold, and a constant register matches nothing, so with hold_bits = 30 a
    detection lapses 31 bits after its last confirmed word and the channel closes; the counters count what happened."""
    w23, w25 = ([(DR.word(c) >> k) & 1 for k in range(23)] for c in (0o023, 0o025))
    bits = w23 * 4 + w25 * 2 + [1] * 60
    x = bits_to_rows(bits)
    ref = DR.DcsRef(1)
    ref.set_hold_bits(30); ref.set_want(1)                                          # wants 025
    seen = []
    for b in range(x.shape[1]):
        _, unmuted = ref.update(x[:, b:b + 1])
        seen.append((int(ref.st["bits"][0]), int(ref.st["detected"][0]), int(ref.st["open"][0]), int(unmuted[0, 0])))
    named = [d for _, d, _, _ in seen]
    assert [d for k, d in enumerate(named) if k == 0 or named[k - 1] != d] == [-1, 0, -1, 1, -1]   # 023 lapses 31 bits after its last word, 8 bits before 025's second
    st = ref.st
    assert int(st["hits"][0]) == 6 and int(st["detections"][0]) == 2 and int(st["openings"][0]) == 1
    first_25 = next(bits_ for bits_, d, _, _ in seen if d == 1)
    assert first_25 - next(bits_ for bits_, d, _, _ in seen if d == 0) == 4 * 23      # 023's second word to 025's second word
    lapsed = next(bits_ for bits_, d, _, _ in seen[named.index(1):] if d == -1)
    assert lapsed - first_25 == 31                                                  # quiet > 30
    opened = [u for _, _, _, u in seen]
    assert sum(opened) == int(st["open_blocks"][0]) and 0 < sum(opened) < len(opened) and opened[0] == 0 and opened[-1] == 0
    # open is read at a block's start: the rows follow the verdict by one block
    assert [o for _, _, o, _ in seen][:-1] == opened[1:]
    # confirm 1 names with the first word, confirm 3 with the third
    for confirm, at in ((1, 1), (3, 3)):
        r = DR.DcsRef(1)
        r.set_confirm(confirm)
        r.update(x[:, :int(4 * 23 * 2625 / 1024) + 4])
        assert int(r.st["hits"][0]) == 4 and int(r.st["detected"][0]) == 0 and int(r.st["run"][0]) == 4 and at <= 4


def test_rows_of_zeros_move_nothing_but_the_clock():
    r = DR.DcsRef(2)
    out, _ = r.update(np.zeros((2, 100, 128), dtype=np.int16))
    st = r.st
    assert not st["edges"].any() and not st["b"].any() and not st["sr"].any() and not st["hits"].any() and (st["detected"] == -1).all()
    assert (st["bits"] == 39).all() and (st["clk"] == (100 * 1024) % 2625).all() and (st["open"] == 1).all() and not out.any()


def test_splitting_a_sequence_into_calls_changes_nothing():
    rng = np.random.default_rng(5)
    n, nb = 8, 180
    x = np.stack([DR.dcs_wave(nb * 128, DR.word(DR.CODES[c]), 1500.0, start_bit=18.0 + c) for c in range(n)]) + rng.normal(0.0, 800.0, size=(n, nb * 128))
    x = DR.to_int16(x).reshape(n, nb, 128)
    outs, recs = [], []
    for sizes in ((nb,), (1, 2, 3, 59, 60, 55), tuple([1] * nb)):
        r = DR.DcsRef(n)
        for c in range(n):
            r.set_want((DR.PASS, DR.ANY, c, (c + 1) % n)[c % 4], ch=c); r.set_hysteresis(1000 * (c % 3), ch=c)
        a, parts = 0, []
        for s in sizes:
            parts.append(r.update(x[:, a:a + s])[0]); a += s
        outs.append(np.concatenate(parts, axis=1)); recs.append(r.records().tobytes())
        assert r.blocks == nb
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]) and recs[0] == recs[1] == recs[2]
    assert (r.st["detected"] == np.arange(n)).all() and 0 < (outs[0] != 0).any(axis=2).sum() < n * nb
