"""Tone squelch (include/asdr_tone.h): time of the pass at the sizes a bank is used at.

    python tools/bench_tone.py [config ...]        (default: T2 T2x8 T5)

    T2     65,536 channels x 1 block of 44.1 kHz audio rows (128 samples: an FM demodulator step's output)
    T2x8   65,536 channels x 8 blocks
    T5     512 channels x 646 blocks      (a capture-sink call)

Prints ONE JSON line per configuration.  The rows are a CTCSS tone in voice-band-like noise per channel from a seed (the kernel takes
the same instructions whatever the data); the creation table of 50 tones, W = 64, the three-section 300 Hz high-pass, and a wanted
tone that some channels carry and some do not.  Every line carries the algorithmic bytes from the shapes: the pass reads one int16
row and writes one, and reads and writes every channel's 704-byte record once per call.  Timed with device events on one stream around
enough warmed calls to fill 0.3 s, three repeats (all three are printed, the median is used for the ratios).  Beside them, from the
same run, the yardsticks: a device-to-device copy of a buffer of the same input plus output plus record (read and written) bytes, and
the time per launch of a one-element kernel (the pass is one kernel)."""
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

CONFIGS = {"T2": (65536, 1), "T2x8": (65536, 8), "T5": (512, 646)}      # name -> (channels, blocks)
FILL_S, REPEATS = 0.3, 3
WINDOW, SECTIONS, RECORD = 64, 3, 704


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


def audio(rng, n, nb):
    """int16 [n][nb][128]: noise of rms 6000 plus, on three channels of four, a CTCSS tone of amplitude 3277 (channel c: tone c % 50)."""
    k = np.arange(nb * 128, dtype=np.float64)
    x = rng.normal(0.0, 6000.0, size=(n, nb * 128))
    for c in range(n):
        if c % 4 != 3:
            x[c] += 3277.0 * np.sin(2.0 * np.pi * A.CTCSS_TONES[c % 50] * k / 44100.0 + c)
    return np.clip(np.floor(x + 0.5), -32768, 32767).astype(np.int16).reshape(n, nb, 128)


def run(name):
    n, nb = CONFIGS[name]
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    x = audio(np.random.default_rng(1), 64, nb)                      # 64 different channels, repeated
    d_in = torch.from_numpy(x).cuda().repeat(n // len(x), 1, 1)
    d_out = torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda")
    samples = n * nb * 128
    read_bytes, write_bytes = samples * 2 + n * RECORD, samples * 2 + n * RECORD
    d_src = torch.zeros(read_bytes + write_bytes, dtype=torch.uint8, device="cuda")
    d_dst = torch.empty_like(d_src)
    one = torch.zeros(1, device="cuda")
    t = A.ToneSquelch(n)
    t.set_window(WINDOW); t.set_highpass(fc_hz=300.0, sections=SECTIONS); t.set_min_power(A.tone_min_power(1000, WINDOW))
    for c in range(64):                                              # of four channels: decode only, the own tone, another tone, any tone
        w = (A.TONE_PASS, c % 50, (c + 7) % 50, A.TONE_ANY)[c % 4]
        for k in range(c, n, 64):
            t._L.asdr_tone_set_want(t._h, k, w)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        launch, _ = events_ms(lambda: one.add_(0.0), stream)
        d2d, _ = events_ms(lambda: d_dst.copy_(d_src, non_blocking=True), stream)   # a copy of as many bytes as the pass reads and writes
    ms, reps = events_ms(lambda: t.update_device(d_in.data_ptr(), d_out.data_ptr(), nb, stream=sp), stream)
    st = t.read_state()
    assert t.blocks() > 0 and int(st["windows"].min()) > 0 and 0 < int(st["open"].sum()) < n      # the squelch separates the channels
    line = {"bench": "tone_squelch", "config": name, "n_channels": n, "n_blocks": nb, "samples": samples, "read_bytes": read_bytes,
            "write_bytes": write_bytes, "record_bytes_each_way": n * RECORD, "source_sha256": build.source_sha256()[:16],
            "n_tones": 50, "window_blocks": WINDOW, "sections": SECTIONS, "timed_calls": reps, "pass_ms": ms,
            "d2d_copy_of_pass_bytes_ms": d2d, "tiny_launch_ms": launch,
            "rows_per_workgroup": A.TONE_ROWS, "workgroups": (n + A.TONE_ROWS - 1) // A.TONE_ROWS,
            "pass_gb_per_s": round((read_bytes + write_bytes) / (med(ms) * 1e-3) / 1e9, 2),
            "msamples_per_s": round(samples / (med(ms) * 1e-3) / 1e6, 1),
            "us_per_block_of_a_workgroup": round(med(ms) * 1e3 / nb, 3),
            "pass_over_d2d_plus_launch": round(med(ms) / (med(d2d) + med(launch)), 3)}
    print(json.dumps(line), flush=True)
    t.close()


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
