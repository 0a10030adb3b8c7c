"""The packet decoder's restatement (tests/packet_ref.py, from include/asdr_packet.h) against known answers: the FCS, the header's tap
tables, frames built by a bit-stuffer of this file's own (random payloads, the densest stuffing, the shortest and the longest frame, an
overlong one, two frames sharing a flag, a corrupted bit, an abort), signals in noise, off-rate senders, a weak signal, de-emphasised
audio, noise alone, and the most bits a block takes over every clock phase and every pattern of edges."""
import os
import re

import numpy as np
import pytest

import packet_ref as PR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


# ---- an independent sender: bytes to line bits, written apart from packet_ref.frame_bits
def x25(data):
    """CRC-16/X-25 by the bitwise definition on the reflected polynomial: init 0xFFFF, xorout 0xFFFF."""
    reg = 0xFFFF
    for byte in data:
        reg ^= byte
        for _ in range(8):
            reg = (reg >> 1) ^ 0x8408 if reg & 1 else reg >> 1
    return reg ^ 0xFFFF


def stuff(data):
    """The bits of bytes, the low bit first, with a 0 behind every run of five 1s."""
    bits = "".join(format(v, "08b")[::-1] for v in data)
    return [int(ch) for ch in bits.replace("11111", "111110")]


FLAG_BITS = [0, 1, 1, 1, 1, 1, 1, 0]


def line_bits(payloads, flags_before=6, flags_between=1, flags_after=2, fcs_xor=0):
    out = FLAG_BITS * flags_before
    for k, p in enumerate(payloads):
        f = x25(p) ^ fcs_xor
        out = out + stuff(bytes(p) + bytes([f & 0xFF, f >> 8])) + FLAG_BITS * (flags_between if k + 1 < len(payloads) else flags_after)
    return out


def decode(waves, boost=256, ring=16):
    """A reference of len(waves) channels over the waves (float arrays, zero-padded to the longest): (ref, frames)."""
    nb = max(-(-len(w) // 128) for w in waves)
    x = np.zeros((len(waves), nb * 128), dtype=np.int16)
    for c, w in enumerate(waves):
        x[c, :len(w)] = PR.to_int16(w)
    ref = PR.PacketRef(len(waves), ring=ring)
    ref.set_space_boost(boost)
    most = ref.update(x.reshape(len(waves), nb, 128))
    assert most <= 5
    return ref, ref.collect(len(waves) * ring)


def payload_of(f):
    return f["data"][:int(f["length"])].tobytes()


def test_fcs_and_taps_and_the_headers_tables():
    assert PR.fcs(b"123456789") == 0x906E == x25(b"123456789")
    assert PR.fcs(b"") == 0 and all(PR.fcs(bytes([v])) == x25(bytes([v])) for v in range(256))
    with open(os.path.join(ROOT, "include", "asdr_packet.h")) as f:
        text = f.read()
    for name, want in (("C1200", PR.C1200), ("S1200", PR.S1200), ("C2200", PR.C2200), ("S2200", PR.S2200)):
        body = re.search(r"ASDR_PACKET_%s\[9\] = \{(.*?)\};" % name, text).group(1)
        assert [int(v) for v in body.split(",")] == want.tolist(), name
    assert PR.C1200.tolist() == [256, 198, 52, -118, -235, -246, -146, 19, 176] and PR.S2200.tolist() == [0, 243, 152, -149, -244, -4, 242, 155, -146]
    assert PR.H.tolist() == np.convolve(np.convolve([1, 1, 1, 1], [1, 1, 1, 1]), [1, 1, 1, 1]).tolist() and PR.H.sum() == 64
    rng = np.random.default_rng(3)
    for n in (0, 1, 15, 200):                                  # the two senders agree
        p = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert PR.frame_bits(p, 6, 2) == line_bits([p])
    # a frame with its FCS leaves the residue the statement compares with
    crc = 0xFFFF
    for v in b"123456789" + bytes([0x6E, 0x90]):
        crc = PR.crc_step(crc, v)
    assert crc == 0xF0B8


def test_frames_of_the_independent_stuffer_decode_to_their_payloads():
    rng = np.random.default_rng(11)
    payloads = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in (15, 16, 40, 77, 120, 256)]
    payloads += [bytes([0xFF, 0x7E] * 30), bytes([0xFF] * 50), bytes([0x7E] * 33), bytes(15), bytes(range(74, 74 + 15))]
    payloads += [rng.integers(0, 256, 330, dtype=np.uint8).tobytes(), bytes([0xFF] * 330)]
    ref, frames = decode([PR.afsk_wave(line_bits([p]), 8000.0, lead=1.0 + 0.37 * k) for k, p in enumerate(payloads)])
    assert len(frames) == len(payloads) and frames["channel"].tolist() == list(range(len(payloads)))
    for f, p in zip(frames, payloads):
        assert payload_of(f) == p and not f["data"][len(p):].any() and f["seq"] == 0 and f["flags"] == 0
    st = ref.st
    assert (st["frames"] == 1).all() and not st["crc_errors"].any() and not st["aborts"].any() and (st["flags"] >= 7).all()
    pending, lost = ref.ring_state()
    assert not pending.any() and not lost.any()
    # the block in which the closing flag's last bit was taken: a frame's bits before it, at 1200 bit/s of 344.5 blocks a second
    for f, p in zip(frames, payloads):
        n_bits = len(line_bits([p], flags_after=1))
        assert abs(int(f["block"]) - n_bits * 44100.0 / 1200.0 / 128.0) < 3, (len(p), int(f["block"]))


def test_too_short_and_overlong_frames_are_dropped():
    rng = np.random.default_rng(12)
    short, longest, overlong = (rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (14, 330, 331))
    ref, frames = decode([PR.afsk_wave(line_bits([p]), 8000.0) for p in (short, longest, overlong)])
    assert len(frames) == 1 and frames["channel"].tolist() == [1] and payload_of(frames[0]) == longest
    assert ref.st["frames"].tolist() == [0, 1, 0] and ref.st["len"].tolist() == [0, 0, 0]
    assert ref.st["crc_errors"].tolist() == [0, 0, 0]           # neither is a CRC error: the short one is no frame, the long one was left
    ref, frames = decode([PR.afsk_wave(line_bits([overlong, longest]), 8000.0)])     # the decoder goes on behind an overlong frame
    assert len(frames) == 1 and payload_of(frames[0]) == longest


def test_two_frames_sharing_one_flag_and_a_corrupted_bit_and_an_abort():
    rng = np.random.default_rng(13)
    a, b, c = (rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (30, 45, 20))
    shared = line_bits([a, b, c], flags_between=1)
    bad = line_bits([a], fcs_xor=0x0400) + line_bits([b], flags_before=1)
    cut = line_bits([a], flags_after=0)[:6 * 8 + 100] + [1] * 7 + [0] + line_bits([c], flags_before=2)
    ref, frames = decode([PR.afsk_wave(v, 8000.0) for v in (shared, bad, cut)])
    got = [(int(f["channel"]), int(f["seq"]), payload_of(f)) for f in frames]
    assert got == [(0, 0, a), (0, 1, b), (0, 2, c), (1, 0, b), (2, 0, c)]
    assert ref.st["crc_errors"].tolist() == [0, 1, 0] and ref.st["aborts"].tolist() == [0, 0, 1] and ref.st["frames"].tolist() == [3, 1, 1]
    assert np.all(np.diff(frames["block"][:3].astype(int)) > 0)


def test_every_frame_decodes_in_white_noise():
    """Amplitude 3,000 in white noise of rms 1,000: 20 of 20 frames.  At rms 2,000 (the full-band signal-to-noise ratio is 0.5 dB
    there) the figure is printed, not set: 19 of 20 with this file's noise; whatever is delivered there is one of the frames sent.
    No floor is asserted at rms 2,000 because none follows from reasoning: Eb/N0 is 13.2 dB there (A^2 / 2 / 1200 over
    sigma^2 / 22050), at which ideal non-coherent FSK loses one frame of 600 bits in a hundred (BER exp(-Eb / 2 N0) / 2 = 1.6e-5), and
    each dB that the 9-tap correlators, the decimator's droop and the clock's jitter under noisy edges cost multiplies the BER by 5
    to 8: the expectation is 19.8 of 20 without loss, 18.5 at 1 dB, 12.9 at 2 dB and 3.7 at 3 dB, and the statement does not pin that
    loss.  A floor would have to be read off this decoder's own result."""
    rng = np.random.default_rng(14)
    payloads = [PR.ui_frame(src="N%dCALL" % (k % 10), info=rng.integers(32, 127, 40 + k, dtype=np.uint8).tobytes()) for k in range(20)]
    for sigma in (1000.0, 2000.0):
        waves = []
        for k, p in enumerate(payloads):
            w = PR.afsk_wave(line_bits([p], flags_before=12), 3000.0, lead=2.0 + 0.21 * k)
            waves.append(w + rng.normal(0.0, sigma, w.size))
        ref, frames = decode(waves)
        print("rms %d: %d of %d frames, %d CRC errors" % (sigma, len(frames), len(payloads), ref.st["crc_errors"].sum()))
        if sigma == 1000.0:
            assert [payload_of(f) for f in frames] == payloads, (sigma, len(frames))
            assert PR.format_address(payload_of(frames[3])) == "N3CALL>APRS"
        assert all(payload_of(f) == payloads[int(f["channel"])] for f in frames)


def test_off_rate_senders_and_a_weak_one():
    """Bit rates 0.98 to 1.02 of nominal at amplitude 5,000 with 120-byte frames, and amplitude 30."""
    rng = np.random.default_rng(15)
    rates = (0.98, 0.99, 1.0, 1.01, 1.02)
    payloads = [rng.integers(0, 256, 120, dtype=np.uint8).tobytes() for _ in rates]
    ref, frames = decode([PR.afsk_wave(line_bits([p]), 5000.0, rate=r) for p, r in zip(payloads, rates)])
    assert [payload_of(f) for f in frames] == payloads
    ref, frames = decode([PR.afsk_wave(line_bits(payloads[:1]), 30.0)])
    assert [payload_of(f) for f in frames] == payloads[:1]


def deemphasis(x, a):
    """Step 6 of asdr_fm.h on float samples rounded to int16: s += (((x << 15) - s) * a) >> 15; y = (s + 2^14) >> 15."""
    s, out = 0, np.zeros(x.size, dtype=np.int64)
    for k, v in enumerate(PR.to_int16(x).tolist()):
        s += (((v << 15) - s) * a) >> 15
        out[k] = (s + (1 << 14)) >> 15
    return out.astype(np.float64)


@pytest.mark.parametrize("a", [8550, 976])
def test_deemphasised_audio_decodes_at_the_creation_space_boost(a):
    rng = np.random.default_rng(16)
    payloads = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (20, 60, 120)]
    ref, frames = decode([deemphasis(PR.afsk_wave(line_bits([p]), 8000.0), a) for p in payloads], boost=256)
    assert [payload_of(f) for f in frames] == payloads


def test_white_noise_alone_gives_no_frame():
    rng = np.random.default_rng(17)
    ref, frames = decode([rng.normal(0.0, 6000.0, 4 * 44100)])
    assert len(frames) == 0 and ref.st["frames"][0] == 0 and ref.st["bits"][0] > 4000 and ref.st["edges"][0] > 1000


def test_the_most_bits_a_block_takes():
    """Over every clk and every pattern of edges in a block's 32 decimated samples, by going through the clock's states backwards
    (whether an edge falls on a sample is free, and nothing but clk carries over): 5 bits at the most from some clk, 4 at the most
    from every other; edges that keep pulling the clock back can hold a block to no bit at all; 3 or 4 on an undisturbed clock.  A random sweep of patterns never exceeds what the exhaustive search says."""
    most, least = [0] * PR.PERIOD, [0] * PR.PERIOD
    for _ in range(32):
        nxt = [[PR.clock_step(c, e) for e in (False, True)] for c in range(PR.PERIOD)]
        most, least = ([f(int(t) + tab[c2] for c2, t in nxt[c]) for c in range(PR.PERIOD)] for f, tab in ((max, most), (min, least)))
    assert max(most) == 5 and min(most) == 4 and max(least) == 0
    free = set()
    for c in range(PR.PERIOD):
        clk, bits = c, 0
        for _ in range(32):
            clk, t = PR.clock_step(clk, False)
            bits += t
        free.add(bits)
    assert free == {3, 4}
    rng = np.random.default_rng(18)
    seen = 0
    for _ in range(4000):
        clk, bits = int(rng.integers(0, PR.PERIOD)), 0
        start = clk
        for e in rng.random(32) < rng.random():
            clk, t = PR.clock_step(clk, bool(e))
            bits += t
        assert least[start] <= bits <= most[start]
        seen = max(seen, bits)
    assert seen >= 4
