"""The time-domain tuner bank (asdr_tuner.hip), its format kernels and the rate bank's stage 2 (asdr_tuner_resample.hip, the host's
block arithmetic) at the input positions a running receiver reaches: a channel's anchor 2^30 samples behind P (the mixer's `first`
changes branch), P past 2^32 (the phase product wraps), output and u counters past 2^31 and 2^32.  One seeded device buffer is fed
to the bank over and over on one stream; at each checkpoint a reference (tests/tuner_ref.py, tests/tuner_rate_ref.py) is placed
from P and the buffer's last samples alone -- place_at, pinned against stepping by tests/test_tuner_ref.py and
tests/test_tuner_rate_control.py -- and the next calls are compared bit for bit, every channel and every sample."""
import time

import numpy as np
import pytest

import tuner_formats_ref as FM
import tuner_rate_ref as RR
import tuner_ref as R
from helpers import Hip
from test_gpu_tuner import FWS, random_taps
from test_gpu_tuner_rate import random_resampler

pytestmark = pytest.mark.gpu

ODD = FWS[4]
assert FWS[0] == 0 and FWS[1] == 1 << 31 and ODD & 1


def full_scale(rng, shape, dtype=np.int16):
    i = np.iinfo(dtype)
    return rng.integers(i.min, i.max, size=shape, dtype=dtype, endpoint=True)


class Feed:
    """A bank, one device buffer of n_frames frames per source in the bank's format (raw; conv is the same as CS16 pairs, for the
    reference) and one stream.  Every call takes the buffer's first frames; the calls' lengths are kept, so that tail() gives the
    samples before P.  how: "plain" (update_device), "samples" (update_samples_device) or "rate" (update_rate_device)."""

    def __init__(self, bank, how, raw, conv, n_ch, cap_row):
        self.bank, self.how, self.conv, self.n_ch, self.cap_row = bank, how, conv, n_ch, cap_row
        self.blk = 128 * bank.decimation
        self.nf = raw.shape[1] // self.blk
        self.hip = Hip()
        self.s = self.hip.stream()
        self.d_in = self.hip.upload(raw)
        self.d_i, self.d_q = self.hip.malloc(n_ch * cap_row * 256), self.hip.malloc(n_ch * cap_row * 256)
        self.counts, self.blocks = [], 0

    def call(self, nf, out_stride):
        """One call of nf frames; returns the blocks written to each row."""
        b, row = self.bank, self.nf * self.blk
        if self.how == "plain":
            b.update_device(self.d_in, self.d_i, self.d_q, nf, in_stride_samples=row, out_stride_blocks=out_stride, stream=self.s)
            n = nf
        else:
            n = b.out_blocks(nf)                                       # the capacity: what the call is to write, asked just before
            fn = b.update_samples_device if self.how == "samples" else b.update_rate_device
            got = fn(self.d_in, self.d_i, self.d_q, nf, n, in_stride_samples=row, out_stride_blocks=out_stride, stream=self.s)
            assert got == n, (got, n)
        self.counts.append(nf * self.blk)
        self.blocks += n
        return n

    def feed_to(self, P):
        assert P % self.blk == 0 and P >= self.bank.position()
        left = (P - self.bank.position()) // self.blk
        while left:
            nf = min(left, self.nf)
            self.call(nf, self.cap_row)
            left -= nf
        self.hip.sync(self.s)
        assert self.bank.position() == P and self.bank.output_position() == 128 * self.blocks

    def tail(self, T):
        return R.fed_tail(self.conv, self.counts[-(T // self.blk + 2):], T)

    def compare(self, ref, nf):
        """One call of nf frames against the reference: counts, I and Q bit for bit, positions."""
        rate = isinstance(ref, RR.TunerRateRef)
        stride = max(self.bank.out_blocks(nf), 1)
        assert not rate or self.bank.out_blocks(nf) == ref.out_blocks(nf)
        n = self.call(nf, stride)
        self.hip.sync(self.s)
        gI = self.hip.download(self.d_i, (self.n_ch, stride, 128), np.int16)[:, :n]
        gQ = self.hip.download(self.d_q, (self.n_ch, stride, 128), np.int16)[:, :n]
        wI, wQ = ref.update(self.conv[:, :nf * self.blk])
        assert gI.shape == wI.shape == (self.n_ch, n, 128)
        bad = np.argwhere((gI != wI) | (gQ != wQ))
        assert bad.size == 0, "P = %d: first mismatch at %s of %s" % (ref.P, bad[0], gI.shape)
        assert self.bank.position() == ref.P
        if rate:
            assert self.bank.output_position() == ref.out_pos == 128 * self.blocks
        return gI, gQ

    def close(self):
        self.hip.free_all()
        self.bank.close()


def same_state(bank, ref):
    st = bank.read_state()
    for k in ("src", "fw", "pos_a", "ph_a"):
        assert [int(v) for v in st[k]] == [int(v) for v in getattr(ref, k)], k


def checkpoint(feed, ref, P, calls, T=1024):
    """Feed up to P, place the reference there from the buffer's last samples, compare the calls."""
    feed.feed_to(P)
    ref.place_at(P, feed.tail(T))
    assert feed.bank.position() == ref.P == P
    if isinstance(ref, RR.TunerRateRef):
        assert feed.bank.output_position() == ref.out_pos       # the host's block arithmetic over every call so far, on its own
    for nf in calls:
        feed.compare(ref, nf)
    same_state(feed.bank, ref)


def both(objs, fn):
    for o in objs:
        fn(o)


def plain_pair(gpu, rng, D, L, n_src, srcs, fws, g=2):
    h = random_taps(rng, L)
    bank, ref = gpu.TunerBank(len(fws), n_src, D), R.TunerRef(len(fws), n_src, D, h, g)
    bank.set_filter(h, g)
    for c, (s, fw) in enumerate(zip(srcs, fws)):
        both((bank, ref), lambda o: (o.set_source(s, ch=c), o.set_frequency_word(fw, ch=c)))
    return bank, ref


def test_plain_bank_across_2_30_and_2_32(gpu):
    """D = 64, L = 1024, g = 2, two sources, six channels (words 0, 2^31, an odd one, 0xFFFFFFFF among them), a buffer of 1,024
    blocks per source (64 MB) fed by update_device.  Channel 2 is retuned at P_r = 2^29 + 3 blocks, so its rel passes 2^30 away
    from P = 2^30.  Checkpoints one block before P = 2^30, before P = P_r + 2^30 and before P = 2^32: the reference placed, calls
    of 1, 3 and 2 blocks compared, read_state compared.  Past 2^32 every setter kind with a compared call after each (the first
    outputs after an anchor: a small rel at a large position), the untouched channels' anchors still 0, then reset() and a
    compared call from position 0.
    Wall time on an MI355X: 0.2 s, the feeding included (a full call of 1,024 blocks: 0.25 ms by device events)."""
    t0 = time.time()
    D, L, NB = 64, 1024, 1024
    blk = 128 * D
    rng = np.random.default_rng(230)
    srcs, fws = [0, 1, 0, 1, 1, 0], [0, 1 << 31, ODD, 0xFFFFFFFF, FWS[5], FWS[6]]
    bank, ref = plain_pair(gpu, rng, D, L, 2, srcs, fws)
    buf = full_scale(rng, (2, NB * blk, 2))
    assert buf.nbytes <= 64 << 20
    feed = Feed(bank, "plain", buf, buf, 6, NB)
    P_r = (1 << 29) + 3 * blk
    feed.feed_to(P_r)
    ref.place_at(P_r)
    both((bank, ref), lambda o: o.set_frequency_word(FWS[2] | 1, ch=2))
    for P in ((1 << 30) - blk, P_r + (1 << 30) - blk, (1 << 32) - blk):
        checkpoint(feed, ref, P, (1, 3, 2))
    assert bank.position() == (1 << 32) + 5 * blk
    h1 = random_taps(rng, 777)
    for fn in (lambda o: o.set_frequency(12_345.6, ch=1),
               lambda o: o.set_frequency_word(FWS[2], ch=3),
               lambda o: o.set_phase(0xDEADBEEF, ch=4),
               lambda o: o.set_source(0, ch=1),
               lambda o: o.set_filter(h1, 3)):
        both((bank, ref), fn)
        feed.compare(ref, 1)
        same_state(bank, ref)
    st = bank.read_state()
    assert int(st["pos_a"][0]) == int(st["pos_a"][5]) == 0 and int(st["pos_a"][2]) == P_r and int(st["pos_a"][3]) > 1 << 32
    for fn in (lambda o: o.set_phase(77 << 20), lambda o: o.set_frequency(-40_000.0), lambda o: o.set_source(1)):     # ASDR_ALL
        both((bank, ref), fn)
        feed.compare(ref, 2)
        same_state(bank, ref)
    bank.reset()
    ref = R.TunerRef(6, 2, D, h1, 3)                              # reset keeps the filter and clears the channels
    assert bank.position() == 0
    same_state(bank, ref)
    for c in range(6):
        both((bank, ref), lambda o: (o.set_source(srcs[c], ch=c), o.set_frequency_word(fws[c], ch=c)))
    feed.compare(ref, 2)
    feed.compare(ref, 1)
    feed.close()
    print("wall time %.1f s" % (time.time() - t0))


def test_plain_bank_odd_d_across_2_32(gpu):
    """D = 7, L = 85, one source, four channels, a buffer of 16,384 blocks (56 MB).  128 * 7 does not divide 2^32: the checkpoint
    is two block boundaries before 2^32, so the second compared call (3 blocks) has 2^32 inside a block and, the position being
    odd against the packed phase pairs, inside a pair.  One retune beyond, and read_state.
    Wall time on an MI355X: 0.1 s, the feeding included."""
    t0 = time.time()
    D, L, NB = 7, 85, 16384
    blk = 128 * D
    rng = np.random.default_rng(7)
    bank, ref = plain_pair(gpu, rng, D, L, 1, [0] * 4, [1 << 31, ODD, 0xFFFFFFFF, FWS[3]])
    buf = full_scale(rng, (1, NB * blk, 2))
    assert buf.nbytes <= 64 << 20
    feed = Feed(bank, "plain", buf, buf, 4, NB)
    P0 = ((1 << 32) // blk - 1) * blk
    assert (1 << 32) % blk and P0 + blk < 1 << 32 < P0 + 4 * blk
    checkpoint(feed, ref, P0, (1, 3, 2))
    both((bank, ref), lambda o: o.set_frequency_word(FWS[6], ch=1))
    feed.compare(ref, 1)
    both((bank, ref), lambda o: o.set_frequency(-3_210.9))
    feed.compare(ref, 2)
    same_state(bank, ref)
    assert int(bank.read_state()["pos_a"][0]) > 1 << 32
    feed.close()
    print("wall time %.1f s" % (time.time() - t0))


@pytest.mark.parametrize("fmt", ["cu8", "rs16"])
def test_format_kernels_across_2_30_and_2_32(gpu, fmt):
    """asdr_tuner_fmt_kernel<F> has its own copy of the position code: a CU8 bank (two samples per load) and an RS16 bank (the real
    mixer), D = 64, L = 1024, two sources, four channels, fed by update_samples_device; the checkpoints one block before P = 2^30
    and before P = 2^32, against a placed TunerRef on the samples converted as tests/tuner_formats_ref.py converts them.
    Wall time on an MI355X: 0.3 s (CU8) and 0.1 s (RS16), the feeding included."""
    t0 = time.time()
    D, L, NB = 64, 1024, 1024
    blk = 128 * D
    rng = np.random.default_rng(len(fmt))
    bank, ref = plain_pair(gpu, rng, D, L, 2, [0, 1, 1, 0], [0, 1 << 31, ODD, 0xFFFFFFFF])
    bank.set_input_format(fmt)
    raw = full_scale(rng, (2, NB * blk, 2), np.uint8) if fmt == "cu8" else full_scale(rng, (2, NB * blk))
    feed = Feed(bank, "samples", raw, FM.to_cs16(raw, fmt), 4, NB)
    for P in ((1 << 30) - blk, (1 << 32) - blk):
        checkpoint(feed, ref, P, (1, 3, 2))
    both((bank, ref), lambda o: o.set_frequency_word(FWS[6], ch=1))
    feed.compare(ref, 1)
    same_state(bank, ref)
    feed.close()
    print("wall time %.1f s" % (time.time() - t0))


def rate_pair(gpu, rng, fs, D, L, K, fws, g2=1):
    bank = gpu.TunerBank(len(fws), 1, D, fs_in=fs)
    U, M = bank.ratio()
    h, h2 = random_taps(rng, L), random_resampler(rng, U, K)
    bank.set_filter(h, 1); bank.set_resampler(h2, g2)
    ref = RR.TunerRateRef(len(fws), 1, D, fs, h, 1, h2, g2)
    for c, fw in enumerate(fws):
        both((bank, ref), lambda o: o.set_frequency_word(fw, ch=c))
    return bank, ref


def test_rate_bank_48k_counters_past_2_31_and_2_32(gpu):
    """48 kHz, D = 1 (147 / 160), L = 33, K = 12, g2 = 1, two channels, a buffer of 32,768 frames fed by update_rate_device: every
    call's count equals out_blocks asked just before, their sum output_position() / 128.  Checkpoints one frame before
    output_position() reaches 2^31 (P near 2.34e9) and one frame before P = N_u = 2^32: the placed reference's out_pos equals
    the bank's before anything is compared, then calls of 1, 2, 7 and 1 frames; after the second a retune, a new resampler and a
    new filter, a compared call after each.
    Wall time on an MI355X: 0.2 s, the feeding (about a thousand calls, 33 million stage-1 workgroups per channel)
    included: two channels stay."""
    t0 = time.time()
    fs, D, NF = 48000, 1, 32768
    rng = np.random.default_rng(48000)
    bank, ref = rate_pair(gpu, rng, fs, D, 33, 12, [ODD, 0xFFFFFFFF])
    U, M = bank.ratio()
    assert (U, M) == (147, 160)
    buf = full_scale(rng, (1, NF * 128, 2))
    feed = Feed(bank, "rate", buf, buf, 2, NF * U // M + 3)
    f1 = ((1 << 31) * M // U) // 128 - 2                       # the first frame count whose blocks reach 2^31 output samples
    while 128 * RR.blocks_out(128 * f1, U, M) < 1 << 31:
        f1 += 1
    assert 128 * RR.blocks_out(128 * (f1 - 1), U, M) < 1 << 31 and 128 * (f1 - 1) > 1 << 31
    T = max(1024, ref.tail_needed())
    checkpoint(feed, ref, 128 * (f1 - 1), (1,), T)
    assert bank.output_position() >= 1 << 31
    for nf in (2, 7, 1):
        feed.compare(ref, nf)
    checkpoint(feed, ref, (1 << 32) - 128, (1, 2, 7, 1), T)
    assert bank.position() == (1 << 32) + 10 * 128
    h1, r1 = random_taps(rng, 21), random_resampler(rng, U, 5)
    for fn in (lambda o: o.set_frequency(1_234.5, ch=0), lambda o: o.set_resampler(r1, 2), lambda o: o.set_filter(h1, 3)):
        both((bank, ref), fn)
        feed.compare(ref, 2)
    same_state(bank, ref)
    feed.close()
    print("wall time %.1f s" % (time.time() - t0))


def test_rate_bank_10msps_across_2_32(gpu):
    """10 MS/s, D = 64 (882 / 3125), L = 1024, K = 64, three channels, a buffer of 2,048 frames (64 MB): one frame before P = 2^32
    the reference is placed, then calls of 1, 16 (several 512-output tiles), 3 and 1 frames, a retune, one more call.  Stage 1
    crosses 2^32 here while stage 2's counters are still small (N_u = 2^26): the two stages' failures are kept apart.
    Wall time on an MI355X: 0.1 s, the feeding included."""
    t0 = time.time()
    fs, D, NF = 10000000, 64, 2048
    blk = 128 * D
    rng = np.random.default_rng(10)
    bank, ref = rate_pair(gpu, rng, fs, D, 1024, 64, [ODD, 1 << 31, 0xFFFFFFFF])
    U, M = bank.ratio()
    assert (U, M) == (882, 3125)
    buf = full_scale(rng, (1, NF * blk, 2))
    assert buf.nbytes <= 64 << 20
    feed = Feed(bank, "rate", buf, buf, 3, NF * U // M + 3)
    checkpoint(feed, ref, (1 << 32) - blk, (1, 16, 3, 1), ref.tail_needed())
    both((bank, ref), lambda o: o.set_frequency(-2_345_678.9, ch=1))
    feed.compare(ref, 7)
    same_state(bank, ref)
    feed.close()
    print("wall time %.1f s" % (time.time() - t0))
