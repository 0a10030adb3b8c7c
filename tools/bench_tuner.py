#!/usr/bin/env python3
"""Digital tuner bank (include/asdr_tuner.h) on the MI355X: one JSON line per config.  (GPU box.)

  T1        skimmer: 1 source, D = 1, 512 channels, L = 257, 256 blocks per call
  T2        one SDR: 1 source, D = 48, 4,096 channels, default filter, 64 blocks per call
  T3        wide bank: 16 sources, D = 48, 65,536 channels (4,096 per source), default filter, 16 blocks per call
  T3+chain  T3 followed by asdr_update_device (USB) on the same stream
  T4        rate bank: 16 sources at 2.4 MS/s, D = 50 (stage 2: 147 / 160), 65,536 channels, default filters, 16 frames per call
  T4+chain  T4 followed by asdr_update_device (USB) on the same stream
  S48       skimmer on sound-card I/Q: 1 source at 48 kHz, D = 1 (147 / 160), 4,096 channels, default filters, 64 frames per call
  F4        fast-convolution bank, T4's geometry: 16 sources at 2.4 MS/s, R = 16 (N = 4,096; stage 2: 147 / 500), 65,536 channels,
            default filters, 16 frames per call
  F4+chain  F4 followed by asdr_update_device (USB) on the same stream
  F20       fast-convolution bank: 16 sources at 20 MS/s, R = 128 (N = 32,768; 882 / 3125), 65,536 channels, 16 frames per call
  F61       fast-convolution bank: 4 sources at 61.44 MS/s, R = 512 (N = 131,072; 147 / 400), 16,384 channels, 16 frames per call
  F4u8      F4 with CU8 rows (RTL-SDR bytes; include/asdr_tuner.h, "Input formats")
  F20s8     F20 with CS8 rows (HackRF bytes)
  R64       skimmer on a direct-sampling receiver: 1 source of real int16 (RS16) at 64.8 MS/s, R = 512 (N = 131,072; Fs_mid =
            126.5625 kHz, 392 / 1125), 512 channels, 16 frames per call
  R64z      R64's signal as CS16 with zero Q (what such a source had to be blown up to before), for comparison
  F4m       F4 with both monitors on (include/asdr_tuner.h, "Monitors"): spectrum of 4,096 bins, hann, sum, and the levels
  F20m      F20 with both monitors on, likewise; run beside F4 / F20 in one process: monitors off is the code path without them
  F4p       F4 with a palette in use (include/asdr_tuner.h, "Filter palette and gain"): channel c on slot c mod 4 -- the default
            filter, +-5 kHz, 300 .. 3000 Hz, -3000 .. -300 Hz (design_channel_filter at Fs_mid = 150 kHz) -- at gain 1, 0.5, 2, -1,
            4 by c mod 5; F4's inputs.  Run beside F4 in one process: F4 is the code path without the palette
  F4c       F4 with source conditioning (include/asdr_tuner.h, "Source conditioning"): every source carries a correction off the
            identity (CONDITION_WORDS by source) and the statistics are on; F4's inputs.  Run beside F4 in one process: F4 is the
            code path without the pre-pass
  F20c      F20 with source conditioning, likewise

Call time is from device events around the timed calls (warmed; at least 1 s of timed work).  Model counts per call: integer
multiply-adds 4 D + 2 L per output sample and channel (mixer + filter) and the bytes the call must move (CS16 input once per
source, int16 I and Q out, the history rows); their share of the VALU issue bound and of HBM, and which of the two bounds the
call.  Rate banks (T4, S48) add stage 2's 2 K multiply-adds per output and the intermediate rows' traffic; x real time is input
time per call over call time.  The first call of each config is checked against tests/tuner_ref.py / tuner_rate_ref.py on a few
channels.  Fast-convolution banks (F*) have no operation model here (DESIGN.md 3.8.2 counts them); their first call is checked
against tests/tuner_fastconv_ref.py, a float64 statement, so "parity" there means every sample within +-2.  Inputs are seeded.

  python tools/bench_tuner.py [T1 T2 T3 T3+chain T4 T4+chain S48 F4 F4+chain F20 F61 F4u8 F20s8 R64 R64z F4m F20m F4p F4c F20c]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: one HIP runtime per process)
import audiosdr_amd as A  # noqa: E402
import tuner_condition_ref as CR  # noqa: E402
import tuner_fastconv_ref as FR  # noqa: E402
import tuner_formats_ref as FM  # noqa: E402
import tuner_palette_ref as PR  # noqa: E402
import tuner_rate_ref as RR  # noqa: E402
import tuner_ref as R  # noqa: E402

VALU_LANE_OPS = 256 * 4 * 64 / 2 * 2.4e9     # CUs x SIMDs x wave64 lanes per 2-cycle issue x max clock: 7.86e13 lane-ops/s
HBM_BPS = 6.29e12                             # measured float4 copy (MI355X_MICROARCH), not the 8 TB/s spec

CONFIGS = {
    "T1": dict(n_src=1, D=1, n_ch=512, L=257, nb=256),
    "T2": dict(n_src=1, D=48, n_ch=4096, L=None, nb=64),
    "T3": dict(n_src=16, D=48, n_ch=65536, L=None, nb=16),
    "T3+chain": dict(n_src=16, D=48, n_ch=65536, L=None, nb=16, chain=True),
    "T4": dict(n_src=16, D=50, n_ch=65536, L=None, nb=16, fs_in=2400000),
    "T4+chain": dict(n_src=16, D=50, n_ch=65536, L=None, nb=16, chain=True, fs_in=2400000),
    "S48": dict(n_src=1, D=1, n_ch=4096, L=None, nb=64, fs_in=48000),
    "F4": dict(n_src=16, D=16, n_ch=65536, L=None, nb=16, fs_in=2400000, fastconv=True),
    "F4+chain": dict(n_src=16, D=16, n_ch=65536, L=None, nb=16, chain=True, fs_in=2400000, fastconv=True),
    "F20": dict(n_src=16, D=128, n_ch=65536, L=None, nb=16, fs_in=20000000, fastconv=True),
    "F61": dict(n_src=4, D=512, n_ch=16384, L=None, nb=16, fs_in=61440000, fastconv=True),
    "F4u8": dict(n_src=16, D=16, n_ch=65536, L=None, nb=16, fs_in=2400000, fastconv=True, fmt="cu8"),
    "F20s8": dict(n_src=16, D=128, n_ch=65536, L=None, nb=16, fs_in=20000000, fastconv=True, fmt="cs8"),
    "R64": dict(n_src=1, D=512, n_ch=512, L=None, nb=16, fs_in=64800000, fastconv=True, fmt="rs16", seed=648),
    "R64z": dict(n_src=1, D=512, n_ch=512, L=None, nb=16, fs_in=64800000, fastconv=True, real=True, seed=648),
    "F4m": dict(n_src=16, D=16, n_ch=65536, L=None, nb=16, fs_in=2400000, fastconv=True, monitors=True, seed=sum(map(ord, "F4"))),
    "F20m": dict(n_src=16, D=128, n_ch=65536, L=None, nb=16, fs_in=20000000, fastconv=True, monitors=True, seed=sum(map(ord, "F20"))),
    "F4p": dict(n_src=16, D=16, n_ch=65536, L=None, nb=16, fs_in=2400000, fastconv=True, palette=True, seed=sum(map(ord, "F4"))),
    "F4c": dict(n_src=16, D=16, n_ch=65536, L=None, nb=16, fs_in=2400000, fastconv=True, condition=True, seed=sum(map(ord, "F4"))),
    "F20c": dict(n_src=16, D=128, n_ch=65536, L=None, nb=16, fs_in=20000000, fastconv=True, condition=True, seed=sum(map(ord, "F20"))),
}
PALETTE_BANDS = [None, (-5000.0, 5000.0), (300.0, 3000.0), (-3000.0, -300.0)]   # slot 0 is the default filter
PALETTE_GAINS = [1.0, 0.5, 2.0, -1.0, 4.0]


def condition_words(s):
    """Source s's correction (dc_re, dc_im, cross_q16, gain_q16) of the F*c configs: a few hundred LSB of DC, up to +-4 degrees of
    phase and +-6 % of gain, none the identity."""
    return (310 - 40 * s, -777 + 90 * s, -4583 + 600 * s, 61977 + 450 * s)


def run(name, n_src, D, n_ch, L, nb, chain=False, fs_in=None, fastconv=False, fmt="cs16", real=False, seed=None, monitors=False,
        palette=False, condition=False):
    """nb = blocks per call of a plain bank, frames per call of a rate bank (fs_in given); D is R for a fast-convolution bank.
    fmt: the bank's input format (rows go through update_samples_device); real: CS16 rows with zero Q; monitors: the spectrum
    (4,096 bins, hann, sum) and the levels of a fast-convolution bank are on; palette: channel c is on slot c mod 4 of
    PALETTE_BANDS at gain PALETTE_GAINS[c mod 5]; condition: source s carries condition_words(s) and the I/Q statistics are on."""
    rng = np.random.default_rng(sum(map(ord, name)) if seed is None else seed)
    bank = A.TunerBank.fastconv(n_ch, n_src, fs_in, D) if fastconv else A.TunerBank(n_ch, n_src, D, fs_in=fs_in)
    bank.set_input_format(fmt)
    if monitors:
        bank.enable_spectrum(4096, "hann", "sum"); bank.enable_levels()
    if condition:
        for s in range(n_src):
            bank.set_iq_correction(words=condition_words(s), source=s)
        bank.enable_iq_stats()
    rate = fs_in is not None
    cap = nb + 1 if rate else nb
    if L is not None:
        h = np.round(np.hamming(L) * np.sinc((np.arange(L) - (L - 1) / 2) * 0.5) * 16384 / 2).astype(np.int16)
        bank.set_filter(h, 0)
    h, g = (bank.get_channel_filter(), 0) if fastconv else bank.get_filter()
    L = h.size
    srcs = np.arange(n_ch) % n_src
    fws = rng.integers(0, 2**32, size=n_ch, dtype=np.uint64)
    for c in range(n_ch):
        bank.set_source(int(srcs[c]), ch=c); bank.set_frequency_word(int(fws[c]), ch=c)
    if palette:
        for k, band in enumerate(PALETTE_BANDS):
            if band:
                bank.set_palette_filter(k, A.design_channel_filter(fs_in / D, *band))
        for c in range(n_ch):
            bank.set_channel_slot(c % len(PALETTE_BANDS), ch=c); bank.set_gain(PALETTE_GAINS[c % len(PALETTE_GAINS)], ch=c)
    N = nb * 128 * D
    calls = 4                                              # distinct seeded inputs, cycled
    if fmt == "rs16" or real:
        raw = rng.integers(-12000, 12000, size=(calls, n_src, N), endpoint=True).astype(np.int16)
        if real:
            raw = np.stack([raw, np.zeros_like(raw)], axis=-1)
    elif fmt == "cu8":
        raw = rng.integers(0, 255, size=(calls, n_src, N, 2), endpoint=True).astype(np.uint8)
    elif fmt == "cs8":
        raw = rng.integers(-128, 127, size=(calls, n_src, N, 2), endpoint=True).astype(np.int8)
    else:
        raw = rng.integers(-12000, 12000, size=(calls, n_src, N, 2), endpoint=True).astype(np.int16)
    iq = [FM.to_cs16(raw[0], fmt)]                            # the first call's rows as the restatements take them
    if condition:
        iq = [np.stack([CR.condition(iq[0][s], condition_words(s)) for s in range(n_src)])]
    dIQ = torch.from_numpy(raw).cuda()
    dI = torch.empty((n_ch, cap, 128), dtype=torch.int16, device="cuda")
    dQ = torch.empty_like(dI)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    sdr, dOut = None, None
    if chain:
        sdr = A.AudioSDRBatch(n_ch)
        sdr.setDemodMode(A.USBmode)
        dOut = torch.empty_like(dI)

    out_blocks = []

    def call(k):
        if fmt != "cs16":
            n = bank.update_samples_device(dIQ[k % calls].data_ptr(), dI.data_ptr(), dQ.data_ptr(), nb, cap, stream=sp)
        elif rate:
            n = bank.update_rate_device(dIQ[k % calls].data_ptr(), dI.data_ptr(), dQ.data_ptr(), nb, cap, stream=sp)
        else:
            bank.update_device(dIQ[k % calls].data_ptr(), dI.data_ptr(), dQ.data_ptr(), nb, stream=sp)
            n = nb
        out_blocks.append(n)
        if chain and rate and n > 0:
            sdr.update_device_strided(dI.data_ptr(), dQ.data_ptr(), dOut.data_ptr(), n, cap, cap, stream=sp)
        elif chain:
            sdr.update_device(dI.data_ptr(), dQ.data_ptr(), dOut.data_ptr(), nb, stream=sp)

    # parity of the first call on 8 channels
    check = sorted(set([0, 1, n_ch - 1] + [int(c) for c in rng.integers(0, n_ch, size=5)]))
    if fastconv:
        h2, g2 = bank.get_resampler()
        ref = (PR.TunerPaletteRef if palette else FR.TunerFastconvRef)(len(check), n_src, fs_in, D, h, h2, g2)
        if palette:
            for k, band in enumerate(PALETTE_BANDS):
                if band:
                    ref.set_palette_filter(k, bank.get_palette_filter(k))
            for i, c in enumerate(check):
                ref.set_channel_slot(c % len(PALETTE_BANDS), ch=i); ref.set_gain(PALETTE_GAINS[c % len(PALETTE_GAINS)], ch=i)
    elif rate:
        h2, g2 = bank.get_resampler()
        ref = RR.TunerRateRef(len(check), n_src, D, fs_in, h, g, h2, g2)
    else:
        ref = R.TunerRef(len(check), n_src, D, h, g)
    for i, c in enumerate(check):
        ref.src[i], ref.fw[i] = int(srcs[c]), int(fws[c])
    call(0)
    torch.cuda.synchronize()
    wI, wQ = ref.update(iq[0])
    n0 = out_blocks[0]
    if fastconv:
        dmax = max(int(np.abs(dI.cpu().numpy()[check, :n0].astype(np.int64) - wI).max(initial=0)),
                   int(np.abs(dQ.cpu().numpy()[check, :n0].astype(np.int64) - wQ).max(initial=0)))
        parity = dmax <= 2
    else:
        parity = bool(np.array_equal(dI.cpu().numpy()[check, :n0], wI) and np.array_equal(dQ.cpu().numpy()[check, :n0], wQ))
    # warm, then size the timed window to >= 1 s
    for k in range(1, 6):
        call(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(3):
        call(k)
    torch.cuda.synchronize()
    est = max((time.perf_counter() - t0) / 3, 1e-5)
    reps = max(10, int(1.2 / est) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    del out_blocks[:]
    e0.record(stream)
    for k in range(reps):
        call(k)
    e1.record(stream)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / reps
    n_mid = n_ch * nb * 128                                   # stage-1 outputs per call
    n_out = n_ch * sum(out_blocks) * 128 / reps               # outputs per call (mean)
    macs = n_mid * (4 * D + 2 * L)
    nbytes = n_src * N * FM.BYTES[fmt] + n_mid * 4 + 2 * n_src * 1024 * 4
    K2 = 0
    if rate:
        U2 = bank.ratio()[0]
        K2 = bank.get_resampler()[0].size // U2
        if not (U2 == 1 and K2 == 1):
            macs += n_out * 2 * K2
            nbytes += n_mid * 4 + n_out * 4 + 2 * n_ch * 576 * 4     # intermediate read back, outputs, carry
    t_valu, t_hbm = macs / VALU_LANE_OPS, nbytes / HBM_BPS
    bound = "valu" if t_valu >= t_hbm else "hbm"
    model = {"int_mult_adds": int(macs), "bytes": int(nbytes), "valu_bound_ms": round(t_valu * 1e3, 4),
             "hbm_bound_ms": round(t_hbm * 1e3, 4), "bound": bound, "share_of_bound": round(max(t_valu, t_hbm) / (ms * 1e-3), 4),
             "note": "tuner model only" if chain else None}
    out = {"config": name, "sources": n_src, "decimation": D, "channels": n_ch, "taps": int(L), "blocks_per_call": nb,
           "chain": "USB" if chain else None, "timed_calls": reps, "timed_s": round(ms * reps / 1e3, 3),
           "ms_per_call": round(ms, 4), "output_samples_per_s": round(n_out / (ms * 1e-3), 1),
           "realtime_factor": round(N / float(fs_in or 44100 * D) / (ms * 1e-3), 2),
           "fs_in": int(fs_in or 44100 * D), "input_format": fmt, "ratio": list(bank.ratio()), "resampler_taps_per_phase": int(K2) if rate else None,
           "output_blocks_per_call": round(sum(out_blocks) / reps, 3),
           "model": None if fastconv else model,
           "parity_channels": len(check), "parity": parity}
    if fastconv:
        out.update({"kind": "fastconv", "fft_size": bank.fft_size(), "parity_max_abs_diff": dmax})
    if palette:
        out.update({"palette": {"slots_in_use": sorted(set(int(v) for v in bank.slots())), "bands_hz": PALETTE_BANDS,
                                "gains": PALETTE_GAINS}})
    if condition:
        st = bank.iq_stats()
        out.update({"condition": {"words": [list(condition_words(s)) for s in range(n_src)], "launches": bank.condition_launches(),
                                  "launches_expected": len(out_blocks) + 9, "stats_samples_per_source": [int(v) for v in st["n"]],
                                  "stats_clipped": [int(v) for v in st["clipped"]]}})
    if monitors:
        spec, frames = bank.spectrum()
        lev, lframes = bank.levels()
        out.update({"monitors": {"spectrum_bins": 4096, "window": "hann", "mode": "sum", "spectrum_frames": frames, "level_frames": lframes,
                                 "mean_power_per_source": [round(float(v), 1) for v in spec.sum(axis=1) / max(frames, 1)],
                                 "channels_with_level": int((lev > 0).sum())}})
    print(json.dumps(out), flush=True)
    bank.close()
    if sdr is not None:
        sdr.close()
    return parity


def main():
    names = sys.argv[1:] or list(CONFIGS)
    ok = True
    for n in names:
        ok = run(n, **CONFIGS[n]) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
