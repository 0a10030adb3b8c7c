"""The RS16 fast-convolution tolerances of tests/test_gpu_tuner_formats.py, checked on the CPU: its RS_EPS table has an entry
for every (recipe, R) it runs, none above 0.1, and the entries with R <= 16 are min(8 x measure(), 0.1) recomputed to 10 %; and the
inputs of its real-stage-2 case (64.8 MS/s, R = 512) satisfy the Stage2Cap condition before any kernel is asked to: the float32
model stage1_f32, rounded and resampled, stays within +-2 and within the restatement's own count of samples off."""

import test_gpu_tuner_formats as T
import tuner_fastconv_ref as F
import tuner_formats_ref as FM


def test_rs_eps_table_is_eight_times_the_float32_models():
    assert set(T.RS_EPS) == {(r, R) for r, Rs in T.RS_CASE_R.items() for R in Rs}
    assert max(T.RS_EPS.values()) <= 0.1
    done = 0
    for (recipe, R), eps in sorted(T.RS_EPS.items()):
        if R <= 16:
            worst, _ = T.measure(recipe, R)
            want = min(8 * worst, 0.1)
            assert abs(eps - want) <= 0.1 * want, (recipe, R, eps, want)
            done += 1
    assert done == 5


def test_rs_recipes_place_the_gathers_where_the_docstring_says():
    for R in T.RS_R:
        H, N, q = F.sizes(R)
        k0, rw = F.coarse(T.rs_words(R), R)
        assert list(k0) == T.rs_bins(R)
        lo, hi = k0 - 128, k0 + 127
        assert lo[2] < 0 < hi[2] and lo[3] < 0 < hi[3]                       # (i) across bin 0
        assert lo[4] < N // 2 <= hi[4] and k0[5] == -N // 2                  # (ii) across N / 2
        assert -N // 2 <= lo[6] and hi[6] < 0 and -N // 2 <= lo[7] and hi[7] < 0   # (iii) wholly in the conjugate half
        assert k0[0] == 0 and k0[1] == N // 2 - 1 and rw[0] == rw[1] == 0    # (iv)


def test_the_stage_2_case_meets_the_cap_with_the_float32_model(A):
    """With the bank's own default filters, read from an ASDR_NO_DEVICE bank."""
    fs, R, n_ch = T.RS64["fs"], T.RS64["R"], T.RS64["n_ch"]
    assert F.ratio(fs, R) == (392, 1125) and F.sizes(R)[1] == 131072
    fws, calls = T.rs64_inputs()
    bank = A.TunerBank.fastconv(n_ch, 1, fs, R, device=A.NO_DEVICE)
    h2, g2 = bank.get_resampler()
    ref, model = (F.TunerFastconvRef(n_ch, 1, fs, R, g=bank.get_channel_filter(), h2=h2, g2=g2) for _ in range(2))
    for o in (ref, model):
        for c, fw in enumerate(fws):
            o.set_frequency_word(fw, ch=c)
    cap = T.Stage2Cap(648)
    for k, a in enumerate(calls):
        iq = FM.to_cs16(a, "rs16")
        got = model.update(iq, f32=True)
        wI, wQ = cap.update(ref, iq)
        cap.check(got[0], wI, what=k); cap.check(got[1], wQ, what=k)
    cap.finish("stage1_f32 at 64.8 MS/s")
