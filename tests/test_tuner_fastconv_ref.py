"""The fast-convolution restatement (tests/tuner_fastconv_ref.py) against the statement itself and against known answers: an
explicit-sum evaluation of the definition at a small N, multitone inputs through the coarse bin, the filter and the fine NCO
(across frames, both ends of the spectrum and retunes), the default channel filter's response, and an off-channel tone through
the default stage 2; the float32 model stage1_f32 against stage1, the GPU suite's EPS table recomputed from it at R <= 16, and
a reference placed at a position against one stepped there.  CPU only; one test reads the default stage 2 from an
ASDR_NO_DEVICE bank."""
import numpy as np
import pytest

import test_gpu_tuner_fastconv as T
import tuner_fastconv_ref as F


def explicit_stage1(x, fs_in, R, fw, g, n_frames):
    """The definition with explicit sums (no FFT library), one channel with anchor (0, 0) on a complex source x."""
    H, N, q = F.sizes(R)
    k0, rw = (int(v) for v in F.coarse(fw, R))
    G = np.asarray(g, dtype=np.float32).astype(np.float64)
    Gm = {m: complex(F.response(G, np.array([m]))[0].astype(np.complex64)) for m in range(-128, 128)}
    nn = np.arange(N)
    out = []
    for b in range(n_frames):
        win = np.array([x[(b - 1) * H + n] if (b - 1) * H + n >= 0 else 0.0 for n in range(N)], dtype=np.complex128)
        for n in range(128, 256):
            s = 0j
            for m in range(-128, 128):
                k = (k0 + m) % N
                Xk = (win * np.exp(-2j * np.pi * k * nn / N)).sum()
                s += Xk * Gm[m] * np.exp(2j * np.pi * m * n / 256)
            y = s / N * (-1) ** ((k0 * (b - 1)) & 1)
            i = 128 * b + n - 128
            th = (rw * i * R) & 0xFFFFFFFF
            th = th - (1 << 32) if th >= 1 << 31 else th
            out.append(y * np.exp(-2j * np.pi * th / 2 ** 32))
    return np.array(out)


def test_restatement_equals_the_explicit_sums_at_a_small_n():
    fs_in, R, nf = 44100 * 2, 2, 3
    H, N, q = F.sizes(R)
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(nf * H) + 1j * rng.standard_normal(nf * H)) * 3000.0
    g = rng.standard_normal(37).astype(np.float32) / 10
    for fw in (0x12345678, 0xF0000001, (N // 2 - 1) * q + 7):
        ref = F.TunerFastconvRef(1, 1, fs_in, R, g=g)
        ref.set_frequency_word(fw)
        got = ref.stage1(x[None])[0]
        want = explicit_stage1(x, fs_in, R, fw, g, nf)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), fw


def test_coarse_bin_and_residual():
    for R in (2, 16, 1024):
        H, N, q = F.sizes(R)
        fws = np.array([0, 1, q // 2 - 1, q // 2, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, (1 << 32) - q // 2, 0x9E3779B9])
        k0, rw = F.coarse(fws, R)
        assert ((rw >= -q // 2) & (rw < q // 2)).all()
        assert (((k0 * q + rw) & 0xFFFFFFFF) == fws).all()
        assert k0[0] == 0 and k0[3] == 1 and k0[4] == N // 2 and k0[5] == -N // 2


def tone_run(fs_in, R, f_ch, tones, retunes=(), n_frames=6, g=None):
    """Stage 1 of one channel on a sum of complex tones (f, A); retunes = {frame: hz}.  Returns (u before rounding, expected)."""
    H, N, q = F.sizes(R)
    ref = F.TunerFastconvRef(1, 1, fs_in, R, g=g)
    ref.set_frequency(f_ch)
    m = np.arange(n_frames * H)
    x = sum(A * np.exp(2j * np.pi * f * (m / fs_in)) for f, A in tones)
    got, want = [], []
    for b in range(n_frames):
        if b in retunes:
            ref.set_frequency(retunes[b])
        got.append(ref.stage1(x[None, b * H:(b + 1) * H])[0])
        k0, rw = (int(v) for v in F.coarse(ref.fw[0], R))
        f_c = k0 * fs_in / N
        i = 128 * b + np.arange(128)
        th = (int(ref.ph_a[0]) + rw * (i * R - int(ref.pos_a[0]))) % (1 << 32)
        ph = 2 * np.pi * (np.outer(i * R, [f for f, _ in tones]) / fs_in) - 2 * np.pi * (k0 * (i * R) % N / N)[:, None] \
            - 2 * np.pi * (th / 2 ** 32)[:, None]
        off = [(f - f_c + fs_in / 2) % fs_in - fs_in / 2 for f, _ in tones]   # tones beyond +-Fs_mid / 2 of the bin are not taken
        Gf = np.array([F.response(ref.g, np.array([d * 256 / ref.fs_mid]))[0] if abs(d) < ref.fs_mid / 2 else 0.0 for d in off])
        want.append((np.array([A for _, A in tones])[None, :] * Gf[None, :] * np.exp(1j * ph)).sum(axis=1))
    return np.array(got), np.array(want)


@pytest.mark.parametrize("fs_in,R", [(2400000, 16), (20000000, 128), (44100 * 4, 4)])
def test_multitone_known_answers(fs_in, R):
    H, N, q = F.sizes(R)
    A = 5000.0
    edge = fs_in / 2 - 3000.0
    for f_ch, retunes in ((123_456.7, {}), (-0.31 * fs_in, {3: 0.2 * fs_in}), (edge, {}), (-edge, {4: edge - 20000.0})):
        offs = (-11000.0, -4321.0, 250.0, 10999.0)
        tones = [(f_ch + o, A) for o in offs]
        for b, hz in retunes.items():              # the retuned channel gets tones of its own
            tones += [(hz + o, A) for o in (-7000.0, 5555.0)]
        got, want = tone_run(fs_in, R, f_ch, tones, retunes)
        err = np.abs(got[2:] - want[2:]).max()
        assert 20 * np.log10(err / A) <= -90.0, (fs_in, R, f_ch, 20 * np.log10(err / A))


def test_a_tone_30_khz_off_is_rejected_in_stage_1():
    fs_in, R = 2400000, 16
    got, _ = tone_run(fs_in, R, 400_000.0, [(430_000.0, 10000.0)])
    assert 20 * np.log10(np.abs(got[2:]).max() / 10000.0) <= -85.0


@pytest.mark.parametrize("fs_mid", [44100.0, 150000.0, 156250.0, 176400.0])
def test_default_filter_response(fs_mid):
    g = F.default_channel_filter(fs_mid).astype(np.float32)
    assert g.size == 129 and abs(float(g.astype(np.float64).sum()) - 1.0) < 1e-6
    fp = np.linspace(-11500.0, 11500.0, 1001)
    dbp = 20 * np.log10(np.abs(F.response(g, fp * 256 / fs_mid)))
    assert np.abs(dbp).max() <= 0.05, np.abs(dbp).max()
    delta = 0.0392 * fs_mid
    fs = np.linspace(11500.0 + delta, fs_mid / 2, 2001)
    for sgn in (1, -1):
        dbs = 20 * np.log10(np.abs(F.response(g, sgn * fs * 256 / fs_mid)))
        assert dbs.max() <= -78.0, dbs.max()


def test_off_channel_tone_through_the_default_stage_2(A):
    """2.4 MS/s, R = 16 (stage 2: 147 / 500): a tone 30 kHz off the channel is <= -75 dB of an in-channel tone at 44.1 kHz."""
    fs_in, R, nf = 2400000, 16, 120
    bank = A.TunerBank.fastconv(1, 1, fs_in, R, device=A.NO_DEVICE)
    h2, g2 = bank.get_resampler()
    g = bank.get_channel_filter()
    ref = F.TunerFastconvRef(1, 1, fs_in, R, g=g, h2=h2, g2=g2)
    f_ch = 321_000.0
    ref.set_frequency(f_ch)
    m = np.arange(nf * 128 * R)
    for f, name in ((f_ch + 30000.0, "off"), (f_ch + 1000.0, "on")):
        ref.reset()
        ref.set_frequency(f_ch)
        x = np.exp(2j * np.pi * f * m / fs_in) * 16000.0
        iq = np.stack([np.round(x.real), np.round(x.imag)], axis=-1).astype(np.int16)
        I, Q = ref.update(iq[None])
        z = (I.astype(float) + 1j * Q.astype(float)).reshape(-1)[1024:]
        if name == "off":
            off = np.abs(z).max()
        else:
            on = np.abs(z).mean()
    assert on > 15000.0 and 20 * np.log10(max(off, 0.5) / on) <= -75.0, (on, off)


@pytest.mark.parametrize("R", [2, 8, 64])
def test_float32_model_against_the_float64_statement(R):
    """stage1_f32 is stage1 in float32: the same values to about sqrt(log2 N) 2^-24 of the peak, and not closer than float32 can
    be (it would then be float64 under another name).  State advances alike."""
    fs = 44100 * R
    rng = np.random.default_rng(R)
    a, b = (F.TunerFastconvRef(4, 2, fs, R, g=T.G_ASYM * 4) for _ in range(2))
    for o in (a, b):
        T.setup(o, [0, 1, 0, 1], T.edge_words(R)[6:10])
    iq = T.cs16(rng, 2, 3 * 128 * R)
    z, w = a.stage1(iq), b.stage1_f32(iq)
    assert z.dtype == w.dtype == np.complex128 and a.P == b.P == 3 * 128 * R and np.array_equal(a.hist, b.hist)
    err, peak = np.abs(w - z).max(), np.abs(z).max()
    assert 2.0 ** -27 * peak <= err <= 16 * 2.0 ** -24 * peak, (err, peak)
    assert np.array_equal(b.update(iq, keep_float=True, f32=True)[2], b.__class__.stage1_f32(a, iq))   # update(f32=True) is it


def test_eps_table_is_eight_times_the_float32_model():
    """The committed EPS of the GPU suite: an entry for every (recipe, R) it runs, none above 0.1, and 8 x the model's largest
    error on the recipe's own inputs (recomputed here for R <= 16) within 10 %."""
    assert set(T.EPS) == {(r, R) for r, Rs in T.CASE_R.items() for R in Rs}
    assert max(T.EPS.values()) <= 0.1
    done = 0
    for (recipe, R), eps in sorted(T.EPS.items()):
        if R <= 16:
            worst, _ = T.measure(recipe, R)
            assert abs(eps - 8 * worst) <= 0.1 * 8 * worst, (recipe, R, eps, 8 * worst)
            done += 1
    assert done == 12


def test_a_placed_reference_equals_a_stepped_one():
    """place_at(P, hist) against 300 frames of stepping at R = 2 (the GPU suite places a reference at 2^32 - 2 H, where stepping
    is out of reach): positions, and the next frames' u before rounding bit for bit, across a retune."""
    R, n_fed, reps = 2, 20, 15
    fs = 44100 * R
    H = 128 * R
    rng = np.random.default_rng(300)
    fws = T.edge_words(R) + [0x6789ABCD]
    a, b = (F.TunerFastconvRef(len(fws), 1, fs, R, g=T.G_ASYM) for _ in range(2))
    for o in (a, b):
        T.setup(o, [0] * len(fws), fws)
        o.set_phase(0xCAFEF00D, ch=3)
    fed = T.cs16(rng, 1, n_fed * H)
    for _ in range(reps):
        a.update(fed)
    b.place_at(reps * n_fed * H, fed[:, -H:])
    assert a.P == b.P == 300 * H and a.out_pos == b.out_pos == 300 * 128
    for k in range(3):
        if k == 1:
            for o in (a, b):
                o.set_frequency_word(0x2468ACE1, ch=4); o.set_phase(0x13579BDF, ch=10)
        iq = T.cs16(rng, 1, (k + 1) * H)
        ra, rb = a.update(iq, keep_float=True), b.update(iq, keep_float=True)
        assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
        assert a.P == b.P and a.out_pos == b.out_pos
    assert list(a.pos_a) == list(b.pos_a) and list(a.ph_a) == list(b.ph_a)
