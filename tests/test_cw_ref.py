"""The CW decoder's restatement (tests/cw_ref.py, from include/asdr_cw.h) alone: the header's tables and constants, keyed text at
12, 20 and 35 WPM from the default speed, at a fixed speed, with jittered element lengths, in white noise, noise alone, the range of
speeds the tracker acquires, the mechanics (glitch lengths, the symbol register's overflow, D's clamps, hi <= lo, a gap that ends
inside the glitch delay, the arithmetic's bounds, split invariance), and the chain end to end on the CPU: the oracle's CW_USBmode
with the audioCW filter and AGC into the restatement.

The designed message is a pangram, the digits and every punctuation code.  It begins with H, four dots, on purpose: the one speed
tracker moves D by an eighth of the difference a mark, so about four marks pass before D is near a speed 1.7 times off the default
in either direction, and until then a dash at 35 WPM (103 ms) is shorter than two dits at 20 WPM (120 ms) and reads as a dot, and
a character gap at 12 WPM (300 ms) is as long as five dits at 20 WPM and reads as a word gap.  No decision on four dots depends on
D that much.  What a message that begins with a dash gives at 35 WPM is printed, not asserted; DESIGN.md 7 leaves acquisition
beyond this out."""
import difflib
import os
import re

import numpy as np
import pytest

import cw_ref as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
TEXT = "HOW VEXINGLY QUICK DAFT ZEBRAS JUMP 0123456789 .,?'!/()&:;=+-_\"$@"
SPEEDS = (12, 20, 35)
AMPLITUDE = 8000.0
GATE = 1000000            # min_power of the noise tests: 12 dB under the tone's P = A^2 / 4 = 16,000,000
NOISE_RMS = (1000, 2000, 4000, 6000, 8000)
NOISE_ASSERTED = 4000     # the largest of NOISE_RMS at which a run of the restatement decoded all three messages, both seeds


def errors(got, want):
    """Characters inserted, deleted or replaced."""
    ops = difflib.SequenceMatcher(None, got, want, autojunk=False).get_opcodes()
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")


@pytest.fixture(scope="module")
def tones():
    return {wpm: R.keyed_tone(TEXT, wpm, AMPLITUDE) for wpm in SPEEDS}


def test_the_message_and_the_headers_tables_and_constants():
    assert set(TEXT) - {" "} == set(R.MORSE) and len(R.MORSE) == 54
    with open(os.path.join(ROOT, "include", "asdr_cw.h")) as f:
        text = f.read()
    body = re.search(r"ASDR_CW_TABLE\[256\] = \{(.*?)\};", text, flags=re.S).group(1)
    table = [int(v) for v in body.replace("\n", " ").split(",") if v.strip()]
    assert table == R.TABLE.tolist() and sum(1 for v in table if v) == 54
    assert R.TABLE[R.sym_of(".-")] == ord("A") and R.TABLE[R.sym_of("...-..-")] == ord("$") and R.sym_of("...-..-") == 137
    assert R.TABLE[0] == 0 and R.TABLE[1] == 0 and R.TABLE[2] == ord("E") and R.TABLE[3] == ord("T")
    for name, value in (("PITCH_HZ", R.PITCH_HZ), ("MIN_POWER", R.MIN_POWER), ("GLITCH", R.GLITCH), ("MAX_GLITCH", R.MAX_GLITCH),
                        ("SLOW_SHIFT", R.SLOW), ("FAST_SHIFT", R.FAST), ("WPM", R.WPM), ("MIN_WPM", R.MIN_WPM), ("MAX_WPM", R.MAX_WPM),
                        ("DIT_UNITS", R.DIT_UNITS), ("MIN_D", R.MIN_D), ("MAX_D", R.MAX_D), ("MAX_RING", R.MAX_RING), ("RING", R.RING)):
        assert re.search(r"#define ASDR_CW_%s %d\b" % (name, value), text), name
    assert R.DIT_UNITS == round(1.2 * R.ENV_HZ * 16) and R.dit_of(20) == 1323 and (R.dit_of(60), R.dit_of(5)) == (R.MIN_D, R.MAX_D)
    assert all(R.wpm_of(R.dit_of(w)) == w for w in range(5, 61))
    assert R.COS[0] == 1024 and R.COS[256] == 0 and R.COS[512] == -1024 and R.COS[768] == 0 and int(np.abs(R.COS).max()) == 1024
    assert R.pitch_step(774) == 75381059 == (774 * 2**33 + 44100) // 88200         # exact: floor(f 2^32 / 44100 + 1 / 2)
    assert R.STATE_DTYPE.itemsize == 80 and R.EVENT_DTYPE.itemsize == 16
    rec = R.CwRef(2).records()
    assert (rec["D"] == 1323).all() and (rec["sym"] == 1).all() and not rec["hi"].any()


# ---- keyed text
@pytest.mark.parametrize("wpm", SPEEDS)
def test_keyed_text_from_the_default_speed(tones, wpm):
    got, r = R.decode(tones[wpm])
    print(wpm, "WPM: D", int(r.st["D"][0]), "of", R.dit_of(wpm), "glitches", int(r.st["glitches"][0]))
    assert got == TEXT
    assert abs(int(r.st["D"][0]) - R.dit_of(wpm)) <= R.dit_of(wpm) // 20 and r.st["unknown"][0] == 0
    assert int(r.st["marks"][0]) == sum(len(R.MORSE[ch]) for ch in TEXT if ch != " ")


def test_a_message_that_begins_with_a_dash_at_35_wpm_is_printed():
    sent = "THE QUICK BROWN FOX"
    got, _ = R.decode(R.keyed_tone(sent, 35, AMPLITUDE))
    print("35 WPM from 20:", repr(sent), "->", repr(got), errors(got, sent), "errors")
    assert got.endswith("QUICK BROWN FOX")              # the tracker has acquired within the first word


@pytest.mark.parametrize("wpm", SPEEDS)
def test_fixed_speed_at_the_true_speed(tones, wpm):
    got, r = R.decode(tones[wpm], wpm=wpm, track=0)
    assert got == TEXT and int(r.st["D"][0]) == R.dit_of(wpm)


@pytest.mark.parametrize("wpm", SPEEDS)
def test_element_lengths_jittered_by_a_fifth(wpm):
    """Every element and every gap stretched by a factor uniform in 0.8 .. 1.2, three seeds, the decoder started at the sender's
    nominal speed with the tracker on: a dot is 0.8 .. 1.2 dits and a dash 2.4 .. 3.6 against the threshold 2, the gaps 0.8 .. 1.2,
    2.4 .. 3.6 and 5.6 .. 8.4 against 2 and 5, and a mark moves D by an eighth of at most a fifth."""
    for seed in (1, 2, 3):
        got, _ = R.decode(R.keyed_tone(TEXT, wpm, AMPLITUDE, jitter=0.2, rng=np.random.default_rng(seed)), wpm=wpm)
        assert got == TEXT, seed


def test_white_noise(tones):
    """Tone amplitude 8,000 (P = 16,000,000) in white noise over the whole 22 kHz, min_power at GATE so that the noise in front of
    the message keys nothing.  No floor follows from reasoning alone: the decision is a threshold between two trackers, not a matched
    filter.  So the bound is the largest rms of NOISE_RMS at which a run of the restatement decoded every message; the next rms up
    is printed with its errors."""
    table = {}
    for rms in NOISE_RMS:
        table[rms] = []
        for seed in (7, 8):
            rng = np.random.default_rng(seed)
            table[rms].append([errors(R.decode(tones[w] + rng.normal(0.0, rms, tones[w].size), min_power=GATE)[0], TEXT) for w in SPEEDS])
        print("noise rms", rms, "errors at", SPEEDS, "WPM, two seeds:", table[rms])
    nxt = NOISE_RMS[NOISE_RMS.index(NOISE_ASSERTED) + 1]
    print("asserted at rms", NOISE_ASSERTED, "; next, rms", nxt, ":", table[nxt])
    for rms in NOISE_RMS[:NOISE_RMS.index(NOISE_ASSERTED) + 1]:
        assert table[rms] == [[0, 0, 0], [0, 0, 0]], rms
    got, _ = R.decode(tones[20] + np.random.default_rng(7).normal(0.0, 2000.0, tones[20].size))
    print("creation min_power, rms 2000:", repr(got[:24]), "...")
    assert got.endswith(TEXT[8:])                       # without a gate the noise in front of the message keys characters of its own


def test_noise_alone_is_counted_not_asserted():
    """60 s of white noise of rms 5,000 (an AGC holds noise near its target level when there is no signal): the decoder has no
    confidence gate and makes characters of it.  The rate is printed and recorded in DESIGN.md 3.20."""
    for rms in (1000, 5000):
        got, r = R.decode(np.random.default_rng(3).normal(0.0, rms, 60 * R.FS))
        print("noise alone, rms", rms, ":", int(r.st["chars"][0]), "characters a minute,", int(r.st["unknown"][0]), "unknown,",
              int(r.st["marks"][0]), "marks,", int(r.st["glitches"][0]), "glitches;", repr(got[:40]))
        assert int(r.st["chars"][0]) >= len(got)        # decode() strips the spaces at the end


def test_the_speeds_the_tracker_acquires_from_20_wpm_are_measured():
    """The message at 6 .. 60 WPM into a decoder at the default 20: the speeds with no error are printed (12 .. 36 when this was
    written); the asserted ones are the three designed speeds above."""
    ok = []
    for wpm in range(6, 61, 2):
        got, _ = R.decode(R.keyed_tone(TEXT, wpm, AMPLITUDE, tail=2.5))
        if got == TEXT:
            ok.append(wpm)
    print("acquired from 20 WPM with no error:", ok)
    assert set(ok) >= {12, 20}


# ---- mechanics, on synthetic envelopes through steps 3 to 7
ON, OFF = 1000000, 0


def keyed(pattern):
    """An envelope from ("k" key down / "s" key up, envelope samples) pairs."""
    out = []
    for kind, n in pattern:
        out += [ON if kind == "k" else OFF] * n
    return out


def elements(code, dit=83):
    p = []
    for k, e in enumerate(code):
        if k:
            p.append(("s", dit))
        p.append(("k", 3 * dit if e == "-" else dit))
    return p


def run_envelope(P, **settings):
    r = R.CwRef(1, ring=R.MAX_RING)
    for k, v in settings.items():
        getattr(r, "set_" + k)(v)
    r.walk(0, list(P))
    return r


@pytest.mark.parametrize("glitch", range(1, R.MAX_GLITCH + 1))
def test_every_glitch_length(glitch):
    """A drop-out of glitch - 1 samples inside a dash is one mark and one glitch; one of `glitch` samples splits it in two.  A spike
    of glitch - 1 samples in a gap is no mark.  The measured length of a mark is its true length."""
    dash = 249
    r = run_envelope(keyed([("s", 50), ("k", 100), ("s", glitch - 1), ("k", dash - 100 - (glitch - 1)), ("s", 500)]), glitch=glitch, track=0)
    assert int(r.st["marks"][0]) == 1 and int(r.st["glitches"][0]) == (1 if glitch > 1 else 0)
    assert R.text_of(r.collect(9)) == "T "
    r = run_envelope(keyed([("s", 50), ("k", 100), ("s", glitch), ("k", dash - 100 - glitch), ("s", 500)]), glitch=glitch, track=0)
    assert int(r.st["marks"][0]) == 2 and R.text_of(r.collect(9)) == "I "
    r = run_envelope(keyed([("s", 50), ("k", glitch - 1), ("s", 500)]), glitch=glitch)
    assert int(r.st["marks"][0]) == 0 and not r.collect(9).size
    for n, want in ((165, "E"), (166, "T")):                                    # 16 L >= 2 D = 2646 from L = 166 on
        r = run_envelope(keyed([("s", 50), ("k", n), ("s", 500)]), glitch=glitch, track=0)
        assert R.text_of(r.collect(9)) == want + " ", n


def test_the_symbol_register_overflows_at_8_and_9_elements():
    for code, ch, flags, sym in (("...-..-", "$", 0, 137), ("...-..-.", "?", 1, 0), ("...-..-..", "?", 1, 0), ("......", "?", 1, 64),
                                 ("-.-.-", "?", 1, 53)):
        r = run_envelope(keyed([("s", 30)] + elements(code) + [("s", 600)]), track=0)
        ev = r.collect(9)
        assert R.text_of(ev) == ch + " " and int(ev[0]["flags"]) == flags and int(ev[0]["sym"]) == sym, code
        assert int(ev[1]["sym"]) == 1 and int(ev[1]["flags"]) == 0 and int(ev[0]["wpm"]) == 20
        assert int(r.st["unknown"][0]) == flags and int(r.st["marks"][0]) == len(code) and int(r.st["sym"][0]) == 1


def test_d_stops_at_both_clamps():
    r = run_envelope(keyed([("s", 30)] + [("k", 3000), ("s", 100)] * 40))
    assert int(r.st["D"][0]) == R.MAX_D == 5292 and R.wpm_of(R.MAX_D) == 5
    r = run_envelope(keyed([("s", 30)] + [("k", 6), ("s", 6)] * 200))
    assert int(r.st["D"][0]) == R.MIN_D == 441 and R.wpm_of(R.MIN_D) == 60
    r = run_envelope(keyed([("s", 30)] + [("k", 3000), ("s", 100)] * 40), track=0)
    assert int(r.st["D"][0]) == 1323


def test_hi_at_or_below_lo_keys_nothing():
    r = R.CwRef(1)
    rec = r.records()
    rec["hi"], rec["lo"] = 1000, 900000
    r.put(0, rec[0])
    r.walk(0, [500000] * 3)                              # hi attacks, lo falls: still hi <= lo for the first samples
    assert int(r.st["hi"][0]) <= int(r.st["lo"][0]) and int(r.st["cnt"][0]) == 0 and int(r.st["key"][0]) == 0
    r = R.CwRef(1)
    rec = r.records()
    rec["hi"], rec["lo"] = 5000, 5000
    r.put(0, rec[0])
    r.walk(0, [5000] * 5000)                             # hi == lo == P: span 0, whatever min_power allows
    assert int(r.st["marks"][0]) == 0 and int(r.st["key"][0]) == 0 and int(r.st["hi"][0]) == int(r.st["lo"][0]) == 5000


def test_a_gap_that_ends_inside_the_glitch_delay():
    """D = 1323: a character gap is one of 16 s >= 2646, s >= 166.  run counts a gap from its true start, but the key stays up for
    glitch - 1 = 3 samples of the next mark: a gap of 163 samples reaches s = 166 and splits the character, one of 162 does not."""
    for gap, want in ((162, "A "), (163, "ET ")):
        r = run_envelope(keyed([("s", 30), ("k", 83), ("s", gap), ("k", 249), ("s", 700)]), track=0)
        assert R.text_of(r.collect(9)) == want, gap
    for gap, want in ((410, "EE "), (411, "E E ")):          # a word gap: 16 s >= 5 D = 6615 from s = 414 on
        r = run_envelope(keyed([("s", 30), ("k", 83), ("s", gap), ("k", 83), ("s", 700)]), track=0)
        assert R.text_of(r.collect(9)) == want, gap


def test_the_bounds_of_the_arithmetic_hold_at_the_extremes():
    n = np.arange(64 * 128)
    aligned = np.where(np.cos(2 * np.pi * R.PITCH_HZ * n / R.FS) >= 0, 32767, -32768)       # the most a row can put on the pitch
    rows = np.stack([np.full(n.size, -32768), np.full(n.size, 32767), aligned, -aligned - 1,
                     np.where(n % 2 == 0, 32767, -32768), np.where(n // 28 % 2 == 0, -32768, 32767)]).astype(np.int16)
    r = R.CwRef(rows.shape[0])
    r.set_pitch_step(R.pitch_step(3000), ch=4)
    r.set_pitch_step(R.pitch_step(100), ch=1)
    big, p_max = r.update(rows.reshape(rows.shape[0], 64, 128))
    print("largest |a|", big, "of", 1 << 20, "; largest P", p_max, "of", 1 << 31)
    assert big <= 1 << 20 and p_max < 1 << 31
    assert p_max > 1 << 28                               # the aligned square wave: (2 / pi)^2 of the bound 2^30


def test_split_invariance_over_random_call_sizes():
    rng = np.random.default_rng(11)
    nb = 700
    x = np.zeros((5, nb * 128))
    for c, (wpm, hz) in enumerate(((20, 774.0), (35, 600.0), (12, 1000.0), (28, 774.0))):
        w = R.keyed_tone("CQ DE K1ABC", wpm, 4000.0 + 3000 * c, hz=hz)[:nb * 128]
        x[c, :w.size] = w
    x += rng.normal(0.0, 300.0, x.shape)
    x = R.to_int16(x).reshape(5, nb, 128)

    def run(sizes, ring):
        r = R.CwRef(5, ring=ring)
        for c, hz in enumerate((774.0, 600.0, 1000.0, 774.0, 2999.0)):
            r.set_pitch_step(R.pitch_step(hz) + c, ch=c)
        r.set_glitch(2, ch=3)
        a = 0
        for s in sizes:
            r.update(x[:, a:a + s])
            a += s
        assert a == nb
        return r.records().tobytes(), r.collect(5 * ring).tobytes(), r.ring_state()[1].tolist()

    whole = run((nb,), 64)
    for _ in range(3):
        cuts = np.sort(rng.choice(np.arange(1, nb), size=25, replace=False))
        sizes = np.diff(np.concatenate([[0], cuts, [nb]])).tolist()
        assert run(sizes, 64) == whole
    assert run([1] * nb, 64) == whole
    assert run((nb,), 3) == run([7] * 100, 3) and sum(run((nb,), 3)[2]) > 0          # with overruns too


# ---- end to end on the CPU: the oracle's chain into the restatement
def test_the_chain_in_cw_mode_into_the_restatement(ao):
    """A carrier of amplitude 3,000 at IF 7,164 Hz, keyed at 20 WPM, through the oracle's chain in CW_USBmode (tuning offset 6,390 Hz)
    with the audioCW filter and the AGC at its creation values: the audio is at 774 Hz, the decoder's default pitch.  The chain's AGC
    starts from rest: the first mark comes out at about 30 times the settled power (printed), `hi` follows it and needs about a
    second to come down, and the key drops out meanwhile.  So the text is sent behind a 'VVV' (the customary test signal), and what is
    asserted is that the decoded text ends with the sent text; what the VVV became is printed."""
    I, Q = R.keyed_carrier_iq("VVV " + TEXT)
    o = ao.OracleSDR()
    o.setDemodMode(ao.CW_USBmode); o.setAudioFilter(ao.audioCW); o.enableAudioFilter()
    audio = o.update(I, Q)
    sec = audio[R.FS:3 * R.FS].astype(np.float64)
    peak = np.argmax(np.abs(np.fft.rfft(sec))) * R.FS / sec.size
    assert abs(peak - R.PITCH_HZ) <= 1.0
    r = R.CwRef(1)
    P, _ = r.envelope(audio.reshape(1, -1, 128).astype(np.int64))
    first = int(P[0, 1378:1378 + 120].max())
    print("P: the first mark's peak", first, ", the median of the marks", int(np.median(P[0][P[0] > 1000])))
    got, r = R.decode(audio)
    print(repr(got))
    assert got.endswith(" " + TEXT)
    beside = R.CwRef(1)
    beside.set_pitch_step(R.pitch_step(R.PITCH_HZ + 500.0))
    P_beside, _ = beside.envelope(audio.reshape(1, -1, 128).astype(np.int64))
    assert np.median(P[0][P[0] > 1000]) > 10 * np.percentile(P_beside[0], 99)     # the audio's power is at the default pitch
