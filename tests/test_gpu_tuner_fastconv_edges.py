"""Fast-convolution banks on the GPU, the edges (include/asdr_tuner.h, "Fast-convolution banks"; asdr_tuner_fastconv.hip,
asdr_tuner_host.cpp): full-scale inputs into both clamps, input positions past 2^32, strided rows and the capacity error, calls
alternating between two streams, retunes / filter changes / reset while stage 2 resamples, and a 44100 R bank switched from the
pass-through to a real stage 2.  Recipes, EPS and the compare helpers are test_gpu_tuner_fastconv's."""
import time

import numpy as np
import pytest

import test_gpu_tuner_fastconv as T
import tuner_fastconv_ref as F
from helpers import Hip

pytestmark = pytest.mark.gpu


def random_taps(rng, L, total=60000):
    h = rng.standard_normal(L)
    h = np.round(h * total / max(np.abs(h).sum(), 1e-9)).astype(np.int64)
    while np.abs(h).sum() > 65535:
        h = h * 9 // 10
    if not h.any():
        h[0] = 1
    return h.astype(np.int16)


def random_resampler(rng, U, K):
    """U K taps, every phase with sum |h2| <= 65535 (with gain shift 0 that keeps one LSB of u within 2 LSB of y)."""
    h2 = np.zeros((K, U), dtype=np.int16)
    for ph in range(U):
        h2[:, ph] = random_taps(rng, K)
    return h2.reshape(-1)


@pytest.mark.parametrize("R", [2, 32])
def test_saturation_and_full_scale_words(gpu, R):
    """Sources at the ends of int16 (T.sat_case) in the one-workgroup and the four-step form: the -32768 word, full-scale outputs
    at the rail with the default filter, |z| up to 92,682 with twice the default filter so that the +-40000 clamps and sat16 both
    act.  compare_u against the clipped z, and the rails must be reached (the first call is the filter's rise and need not)."""
    case = T.sat_case(R)
    bank, ref = T.pair(gpu, case)
    outs = T.run_pass_through(bank, ref, case.events, T.EPS["sat", R])
    assert len(outs) == 3
    for I, Q, z in outs[1:]:
        got = np.stack([I, Q])
        assert got.max() == 32767 and got.min() == -32768
    z = outs[2][2]
    assert z.real.max() > 40000.0 and z.real.min() < -40000.0 and z.imag.max() > 40000.0 and z.imag.min() < -40000.0
    bank.close()


def test_positions_past_2_to_the_32(gpu):
    """R = 1024, one source, 12 channels (T.wrap_case): 32,766 frames fed from one device buffer bring P to 2^32 - 2 H; the
    reference is placed there (place_at; test_tuner_fastconv_ref pins that shortcut), then 4 frames across 2^32, two retunes
    beyond it, 2 more frames and read_state.  The untouched channels keep their anchors of position 0: rw (uint32)(b H - pos_a)
    and the parity of b - 1 come from a frame index past 2^15 and a position past 2^32.
    Wall time on an MI355X: 0.4 s, the feeding included."""
    t0 = time.time()
    case = T.wrap_case()
    H = F.sizes(case.R)[0]
    bank, ref = T.pair(gpu, case)
    ev = iter(case.events)
    fn = next(ev)[1]
    fn(bank); fn(ref)
    fed = next(ev)[1]
    hip = Hip()
    s = hip.stream()
    nf = T.WRAP_FRAMES
    dIQ = hip.upload(fed)
    dI, dQ = hip.malloc(case.n_ch * nf * 256), hip.malloc(case.n_ch * nf * 256)
    for _ in range(511):
        bank.update_device(dIQ, dI, dQ, nf, stream=s)
    bank.update_device(dIQ, dI, dQ, nf - 2, out_stride_blocks=nf, stream=s)
    hip.sync(s)
    _, P0, hist = next(ev)
    assert P0 == (511 * nf + nf - 2) * H == (1 << 32) - 2 * H == bank.position()
    ref.place_at(P0, hist)
    assert bank.output_position() == ref.out_pos
    outs = T.run_pass_through(bank, ref, ev, T.EPS["wrap", case.R])      # positions and read_state are compared in there
    assert len(outs) == 5 and bank.position() == ref.P == (1 << 32) + 4 * H
    st = bank.read_state()
    assert [int(p) for p in st["pos_a"]] == [0, 0, 0, 0, (1 << 32) + 2 * H, 0, 0, 0, 0, 0, (1 << 32) + 2 * H, 0]
    hip.free_all()
    bank.close()
    print("wall time %.1f s" % (time.time() - t0))


def test_strided_rows_and_the_capacity_error(gpu):
    """2.4 MS/s, R = 16 (147 / 500): rows in_stride = n_frames H + 48 and out_stride = capacity + 3 apart, canaries in every gap
    of the input and the output buffers; the outputs equal a twin bank's contiguous calls bit for bit.  A capacity one block
    short is refused and leaves the bank where it was."""
    fs, R, n_ch, n_src = 2400000, 16, 5, 2
    H = 128 * R
    rng = np.random.default_rng(9)
    twin, dev = (gpu.TunerBank.fastconv(n_ch, n_src, fs, R) for _ in range(2))
    for b in (twin, dev):
        T.setup(b, [c % n_src for c in range(n_ch)], T.edge_words(R)[3:3 + n_ch])
    hip = Hip()
    s = hip.stream()
    cap = 6
    out_stride = cap + 3
    out_bytes = n_ch * out_stride * 256
    dI, dQ = hip.malloc(out_bytes + 512), hip.malloc(out_bytes + 512)
    seen = 0
    for nf in (3, 1, 5, 2, 7):
        iq = T.cs16(rng, n_src, nf * H)
        in_stride = nf * H + 48
        padded = np.full((n_src, in_stride, 2), 0x7777, dtype=np.int16)
        padded[:, :nf * H] = iq
        dIQ = hip.upload(padded)
        n = dev.out_blocks(nf)
        if n > 0:                                                         # one block short: refused, nothing changes
            pos, opos = dev.position(), dev.output_position()
            with pytest.raises(gpu.AsdrError, match="capacity"):
                dev.update_rate_device(dIQ, dI, dQ, nf, n - 1, in_stride_samples=in_stride, out_stride_blocks=out_stride, stream=s)
            assert dev.position() == pos and dev.output_position() == opos and dev.out_blocks(nf) == n
        with pytest.raises(gpu.AsdrError, match="stride"):
            dev.update_rate_device(dIQ, dI, dQ, nf, cap, in_stride_samples=in_stride, out_stride_blocks=cap - 1, stream=s)
        with pytest.raises(gpu.AsdrError, match="stride"):
            dev.update_rate_device(dIQ, dI, dQ, nf, cap, in_stride_samples=nf * H - 1, out_stride_blocks=out_stride, stream=s)
        hip.fill(dI, 0x55, out_bytes + 512); hip.fill(dQ, 0x55, out_bytes + 512)
        got = dev.update_rate_device(dIQ, dI + 256, dQ + 256, nf, cap, in_stride_samples=in_stride, out_stride_blocks=out_stride,
                                     stream=s)
        hip.sync(s)
        assert got == n
        seen += n
        gI = hip.download(dI, (n_ch, out_stride, 128), np.int16, offset_bytes=256)
        gQ = hip.download(dQ, (n_ch, out_stride, 128), np.int16, offset_bytes=256)
        wI, wQ = twin.update_rate(iq)
        assert wI.shape[1] == n and np.array_equal(gI[:, :n], wI) and np.array_equal(gQ[:, :n], wQ)
        assert (gI[:, n:] == 0x5555).all() and (gQ[:, n:] == 0x5555).all()     # nothing outside the rows' blocks
        for d in (dI, dQ):
            assert (hip.download(d, (128,), np.int16) == 0x5555).all()
            assert (hip.download(d, (128,), np.int16, offset_bytes=256 + out_bytes) == 0x5555).all()
        assert np.array_equal(hip.download(dIQ, padded.shape, np.int16), padded)       # the input rows and their gaps
        assert dev.position() == twin.position() and dev.output_position() == twin.output_position()
    assert seen >= 4
    hip.free_all()
    twin.close(); dev.close()


@pytest.mark.parametrize("fs,R", [(44100 * 32, 32), (2400000, 16)])
def test_calls_alternating_between_two_streams(gpu, fs, R):
    """Calls alternate between two streams with no host synchronisation in between (the bank orders them by its event, as the
    header's stream rule says); the outputs equal a twin's on one stream bit for bit.  A four-step pass-through bank and a
    resampling one; the third call is larger, so X (and the intermediate) grow between calls."""
    n_ch, n_src = 7, 2
    rng = np.random.default_rng(R)
    two, one = (gpu.TunerBank.fastconv(n_ch, n_src, fs, R) for _ in range(2))
    for b in (two, one):
        T.setup(b, [c % n_src for c in range(n_ch)], T.edge_words(R)[:n_ch])
    hip = Hip()
    ss = [hip.stream(), hip.stream()]
    s1 = hip.stream()
    splits = [2, 2, 4, 1, 3, 4]
    ins = [hip.upload(T.cs16(rng, n_src, nf * 128 * R)) for nf in splits]
    caps = [nf + 1 for nf in splits]
    bufs = [[hip.malloc(n_ch * c * 256) for _ in range(4)] for c in caps]
    hip.sync()
    ns = []
    for k, nf in enumerate(splits):
        a = two.update_rate_device(ins[k], bufs[k][0], bufs[k][1], nf, caps[k], stream=ss[k % 2])
        b = one.update_rate_device(ins[k], bufs[k][2], bufs[k][3], nf, caps[k], stream=s1)
        assert a == b
        ns.append(a)
    hip.sync()
    assert sum(ns) > 0 and two.output_position() == one.output_position()
    for k, n in enumerate(ns):
        g = [hip.download(p, (n_ch, caps[k], 128), np.int16)[:, :n] for p in bufs[k]]
        assert np.array_equal(g[0], g[2]) and np.array_equal(g[1], g[3]), k
        assert n == 0 or g[0].any()
    hip.free_all()
    two.close(); one.close()


def test_retunes_filter_and_resampler_changes_and_reset_while_resampling(gpu):
    """20 MS/s, R = 128 (882 / 3125): a retune of every kind, a new channel filter, two new resamplers (gain shift 0, so +-1 of
    u stays +-2 of y) and a reset between calls, against the restatement under Stage2Cap."""
    fs, R, n_ch, n_src = 20000000, 128, 6, 3
    rng = np.random.default_rng(17)
    bank = gpu.TunerBank.fastconv(n_ch, n_src, fs, R)
    U, M = bank.ratio()
    assert (U, M) == (882, 3125)
    h2, g2 = bank.get_resampler()
    ref = F.TunerFastconvRef(n_ch, n_src, fs, R, g=bank.get_channel_filter(), h2=h2, g2=g2)
    T.setup_pair(bank, ref, [c % n_src for c in range(n_ch)], T.edge_words(R)[:n_ch])
    cap = T.Stage2Cap(17)

    def check(nf, what):
        iq = T.cs16(rng, n_src, nf * 128 * R, [(0, fs * 0.01, 6000.0), (2, -700_000.0 + 3000.0, 6000.0)], fs)
        n = bank.out_blocks(nf)
        assert n == ref.out_blocks(nf)
        I, Q = bank.update_rate(iq)
        wI, wQ = cap.update(ref, iq)
        assert I.shape == wI.shape == (n_ch, n, 128)
        cap.check(I, wI, what); cap.check(Q, wQ, what)
        assert bank.position() == ref.P and bank.output_position() == ref.out_pos

    r1, r2 = random_resampler(rng, U, 7), random_resampler(rng, U, 33)
    steps = [lambda o: o.set_frequency(123_456.7, ch=1),
             lambda o: o.set_frequency_word(0x01234567, ch=2),
             lambda o: o.set_phase(0xDEADBEEF, ch=3),
             lambda o: o.set_source(2, ch=0),
             lambda o: o.set_channel_filter(T.G_ASYM * 4),
             lambda o: o.set_resampler(r1, 0),
             lambda o: o.set_frequency(-700_000.0),
             lambda o: o.set_resampler(r2, 0),
             lambda o: o.set_source(1)]
    check(7, "start")
    for i, st in enumerate(steps):
        st(bank); st(ref)
        check(4 + 3 * (i % 3), ("step", i))
    st = bank.read_state()
    assert list(st["ph_a"]) == list(ref.ph_a) and list(st["pos_a"]) == list(ref.pos_a) and list(st["fw"]) == list(ref.fw)
    bank.reset(); ref.reset()
    assert bank.position() == 0 and bank.output_position() == 0
    T.setup_pair(bank, ref, [c % n_src for c in range(n_ch)], T.edge_words(R)[:n_ch])
    for nf in (4, 2, 9):
        check(nf, ("after reset", nf))
    cap.finish("retunes at 20 MS/s")
    bank.close()


def test_pass_through_then_a_real_stage_2_at_44100_r(gpu):
    """A 44100 R bank (R = 8): pass-through calls under compare_u, then a 9-tap stage 2 at U = M = 1: u before that call counts
    as 0 (the header's rule; zero_before in the restatement), the plain entry point refuses, outputs under Stage2Cap."""
    case = T.switch_case(8)
    bank, ref = T.pair(gpu, case)
    assert len(T.run_pass_through(bank, ref, case.events, T.EPS["switch", 8], plus_old=True)) == 2
    rng = np.random.default_rng(21)
    r1 = random_taps(rng, 9)
    bank.set_resampler(r1, 0); ref.set_resampler(r1, 0)
    with pytest.raises(gpu.AsdrError, match="update_rate"):
        bank.update(T.cs16(rng, 2, 128 * 8))
    assert bank.position() == ref.P
    cap = T.Stage2Cap(21)
    for nf in (1, 3, 2):
        iq = T.cs16(rng, 2, nf * 128 * 8, [(0, 3000.0, 6000.0)], case.fs)
        assert bank.out_blocks(nf) == ref.out_blocks(nf) == nf
        I, Q = bank.update_rate(iq)
        wI, wQ = cap.update(ref, iq)
        cap.check(I, wI, nf); cap.check(Q, wQ, nf)
        assert bank.position() == ref.P and bank.output_position() == ref.out_pos
    assert ref.zero_before == 3 * 128
    cap.finish("44100 R, K = 9")
    bank.close()
