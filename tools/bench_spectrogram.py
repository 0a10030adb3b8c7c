"""Audio spectrogram (include/asdr_spectrogram.h): time of the pass at the sizes a bank is used at.

    python tools/bench_spectrogram.py [config ...]        (default: S5 S2 S2i)

    S5     512 rows x 1,440,000 samples at 12 kHz (a WSPR slot of 512 receivers), N = 8192, H = 4096, Hann, bins 956 .. 1092
    S2     65,536 channels x 1,024 new samples at 44.1 kHz, N = 1024, H = 512, Hann, bins 0 .. 255 (two frames per call, the first
           of which begins in the record)
    S2i    S2 behind an index of 10 % of the channels

Prints ONE JSON line per configuration.  The rows are full-range noise from a seed (the pass takes the same instructions whatever
the data).  Every line carries the algorithmic bytes from the shapes: the pass reads the new samples of the written rows once (and
their records where a frame begins there) and writes frames * B floats per row; the carry reads and writes n_channels * N samples.
Timed with device events on one stream around enough warmed calls to fill 0.3 s, three repeats (all three are printed, the median is
used for the ratios).  Beside it, from the same run, two yardsticks: a device-to-device copy of the same input bytes, and what a
user does without this pass -- torch's unfold of the same rows (with the record's tail in front where frames begin there; the
concatenation is not timed) + float + window + torch.fft.rfft + |.|^2 + the band's slice.  torch_ms is null ("absent") when torch.fft
does not run on the box; a few of its bins are compared with the pass's before anything is timed."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: one HIP runtime per process)
import audiosdr_amd as A  # noqa: E402
from audiosdr_amd import build  # noqa: E402

# name -> (channels, new samples per call, fs, N, H, k0, B, share of rows written; None: all channels, no index)
CONFIGS = {"S5": (512, 1440000, 12000, 8192, 4096, 956, 137, None),
           "S2": (65536, 1024, 44100, 1024, 512, 0, 256, None),
           "S2i": (65536, 1024, 44100, 1024, 512, 0, 256, 0.1)}
FILL_S, REPEATS = 0.3, 3


def events_ms(fn, stream):
    """ms per call of fn (asynchronous on `stream`): REPEATS figures."""
    for _ in range(3):
        fn()
    stream.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        fn()
    stream.synchronize()
    reps = max(5, int(FILL_S / max((time.perf_counter() - t0) / 3, 1e-6)) + 1)
    out = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        out.append(round(e0.elapsed_time(e1) / reps, 5))
    return out, reps


def med(v):
    return sorted(v)[len(v) // 2]


def run(name):
    n, ns, fs, N, H, k0, B, share = CONFIGS[name]
    stream = torch.cuda.Stream()
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_x = torch.randint(-32768, 32768, (n, ns), generator=gen, device="cuda", dtype=torch.int32).to(torch.int16)
    sp = A.AudioSpectrogram(n, n_fft=N, hop=H, first_bin=k0, n_bins=B, window="hann", kind="power")
    # the steady state: T a multiple of H past N, the record = the rows' own tail (so every call computes the same frames)
    t0 = 0 if ns >= 16 * N else 64 * H
    record = np.ascontiguousarray(d_x[:, -N:].cpu().numpy()) if t0 else np.zeros((n, N), dtype=np.int16)
    sp.write_state(record); sp.set_position(t0)
    frames = sp.out_frames(ns)
    k = n if share is None else int(round(share * n))
    form = {}
    if share is not None:
        index = np.sort(np.random.default_rng(1).permutation(n)[:k]).astype(np.int32)
        d_index, d_count = torch.from_numpy(index).cuda(), torch.tensor([k], dtype=torch.int32, device="cuda")
        form = dict(index_ptr=d_index.data_ptr(), count_ptr=d_count.data_ptr(), capacity_rows=n)
    else:
        index = np.arange(n)
    d_out = sp.out_tensor(frames + 2, rows=k, fill=-1.0)
    d_copy = torch.empty_like(d_x)
    d_w = torch.from_numpy(sp.get_window()).cuda()
    reach = (sp.frame_position() * H - t0) if t0 else 0        # where the call's first frame begins: <= 0, in the record
    d_rows = d_x[torch.from_numpy(index).cuda()] if share is not None else d_x
    d_seq = torch.cat([torch.from_numpy(record[index][:, N + reach:]).cuda(), d_rows], dim=1) if reach else d_rows
    torch.cuda.synchronize()

    def the_pass():
        return sp.update_device(d_x.data_ptr(), ns, d_out.data_ptr(), frames + 2, stream=stream.cuda_stream, **form)

    def torch_way():
        f = d_seq.unfold(1, N, H).to(torch.float32) * d_w
        X = torch.fft.rfft(f, dim=-1)[..., k0:k0 + B] * (1.0 / N)
        return X.real ** 2 + X.imag ** 2

    # the first call, from T = t0, is the one compared with torch; the timed calls run on from where it ended (set_position would
    # put a host round trip into every call).  S2's calls repeat exactly; S5's alternate between 351 and 352 frames (1,440,000 is
    # no multiple of H), which the output rows have room for
    assert the_pass() == frames
    stream.synchronize()
    got = d_out[:, :frames].cpu().numpy()
    torch_ms, agree = None, None
    try:
        with torch.cuda.stream(stream):
            want = torch_way()
            stream.synchronize()
            agree = float((want[:8].sqrt() - torch.from_numpy(got[:8]).cuda().sqrt()).abs().max())
            assert want.shape == got.shape and agree < 0.05, agree
            del want
            torch_ms, _ = events_ms(torch_way, stream)
    except RuntimeError as e:                                   # torch.fft absent on the box: reported, not hidden
        print("torch.fft yardstick absent: %s" % str(e).splitlines()[0], file=sys.stderr)

    with torch.cuda.stream(stream):
        ms, reps = events_ms(the_pass, stream)
        d2d, _ = events_ms(lambda: d_copy.copy_(d_x, non_blocking=True), stream)
    in_bytes = n * ns * 2
    read_bytes = k * (ns - reach) * 2 + n * N * 2               # the written rows' samples, and the carry's reads (at most)
    write_bytes = k * frames * B * 4 + n * N * 2
    line = {"bench": "audio_spectrogram", "config": name, "n_channels": n, "n_samples": ns, "fs": fs, "n_fft": N, "hop": H, "first_bin": k0,
            "n_bins": B, "window": "hann", "kind": "power", "share_written": share, "rows": k, "frames_per_call": frames,
            "transforms_per_call": k * frames, "input_bytes": in_bytes, "read_bytes": read_bytes, "write_bytes": write_bytes,
            "source_sha256": build.source_sha256()[:16], "timed_calls": reps, "spectrogram_ms": ms, "d2d_copy_ms": d2d, "torch_ms": torch_ms,
            "torch_vs_pass_max_amplitude_difference": agree,
            "transforms_per_s": round(k * frames / (med(ms) * 1e-3)),
            "spectrogram_over_d2d": round(med(ms) / med(d2d), 4),
            "torch_over_spectrogram": None if torch_ms is None else round(med(torch_ms) / med(ms), 3)}
    print(json.dumps(line), flush=True)
    sp.close()


def main():
    args = sys.argv[1:]
    for name in (args or list(CONFIGS)):
        if name not in CONFIGS:
            print("unknown configuration %r (one of %s)" % (name, " ".join(CONFIGS)), file=sys.stderr)
            return 2
        run(name)
    return 0


if __name__ == "__main__":
    sys.exit(main())
