"""FM demodulator (include/asdr_fm.h): time of the pass at the sizes a bank is used at.

    python tools/bench_fm.py [config ...]        (default: M2 M2x8 M5)

    M2     65,536 channels x 1 block of 44.1 kHz I/Q rows (128 samples: a tuner step's output)
    M2x8   65,536 channels x 8 blocks
    M5     512 channels x 646 blocks      (a capture-sink call)

Prints ONE JSON line per configuration.  The rows are a noisy FM carrier per channel from a seed (the kernel takes the same
instructions whatever the data); de-emphasis of 750 us, DC removal and a squelch that some channels fail are on.  Every line carries
the algorithmic bytes from the shapes (the pass reads two int16 rows and writes one) and the arithmetic model of the pointwise
part: samples x POINTWISE_OPS vector instructions per sample, as counted in the built kernel, against the chip's issue rate.  Timed
with device events on one stream around enough warmed calls to fill 0.3 s, three repeats (all three are printed, the median is
used for the ratios).  Beside them, from the same run, the yardsticks: a device-to-device copy of a buffer of the same input plus
output bytes, and the time per launch of a one-element kernel (the pass is one kernel)."""
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

CONFIGS = {"M2": (65536, 1), "M2x8": (65536, 8), "M5": (512, 646)}      # name -> (channels, blocks)
FILL_S, REPEATS = 0.3, 3
# vector instructions per sample of the pointwise part (conjugate product, normalisation, 20 CORDIC iterations of 11, gain, probe,
# sums, staging), counted in the pass loop of the built kernel: 2,218 per piece of 8 samples
POINTWISE_OPS = 277
# wave-instructions per second the chip issues: 256 CUs x 4 SIMDs, one wave64 instruction per 2 cycles, 2.4 GHz
ISSUE_PER_S = 256 * 4 * 2.4e9 / 2


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


def carriers(rng, n, nb):
    """int16 (I, Q) [n][nb][128]: a 1 kHz tone at 3 kHz deviation on a carrier of amplitude 8000, per channel a phase and a noise
    level between a clean channel and noise alone."""
    k = np.arange(nb * 128, dtype=np.float64)
    phi = rng.uniform(0.0, 2.0 * np.pi, size=(n, 1)) + 3.0 * np.sin(2.0 * np.pi * 1000.0 * k / 44100.0)
    amp = np.where(rng.random((n, 1)) < 0.25, 0.0, 8000.0)
    sigma = rng.uniform(50.0, 3000.0, size=(n, 1))
    out = []
    for f in (np.cos, np.sin):
        x = amp * f(phi) + rng.normal(0.0, 1.0, size=phi.shape) * sigma
        out.append(np.clip(np.floor(x + 0.5), -32768, 32767).astype(np.int16).reshape(n, nb, 128))
    return out


def run(name):
    n, nb = CONFIGS[name]
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    I, Q = carriers(np.random.default_rng(1), 64, nb)                # 64 different channels, repeated
    dI, dQ = (torch.from_numpy(x).cuda().repeat(n // len(x), 1, 1) for x in (I, Q))
    d_out = torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda")
    d_src, d_dst = torch.zeros((3, n, nb, 128), dtype=torch.int16, device="cuda"), torch.empty((3, n, nb, 128), dtype=torch.int16, device="cuda")
    one = torch.zeros(1, device="cuda")
    f = A.FmDemodulator(n)
    f.set_deemphasis(tau_us=750.0); f.set_dc_shift(8); f.set_squelch(10**11, 3 * 10**11, 2)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        launch, _ = events_ms(lambda: one.add_(0.0), stream)
        d2d, _ = events_ms(lambda: d_dst.copy_(d_src, non_blocking=True), stream)   # a copy of as many bytes as the pass reads and writes
    ms, reps = events_ms(lambda: f.update_device(dI.data_ptr(), dQ.data_ptr(), d_out.data_ptr(), nb, stream=sp), stream)
    st = f.read_state()
    assert f.blocks() > 0 and 0 < int(st["open"].sum()) < n      # the squelch separates the channels
    samples = n * nb * 128
    rows = A.FM_ROWS if n >= A.FM_WIDE_CHANNELS else A.FM_NARROW_ROWS
    read_bytes, write_bytes = 2 * samples * 2, samples * 2
    model_ms = samples / 64 * POINTWISE_OPS / ISSUE_PER_S * 1e3
    line = {"bench": "fm_demodulator", "config": name, "n_channels": n, "n_blocks": nb, "samples": samples, "read_bytes": read_bytes,
            "write_bytes": write_bytes, "source_sha256": build.source_sha256()[:16], "timed_calls": reps, "pass_ms": ms,
            "d2d_copy_of_pass_bytes_ms": d2d, "tiny_launch_ms": launch,
            "pointwise_ops_per_sample": POINTWISE_OPS, "pointwise_issue_model_ms": round(model_ms, 5),
            "rows_per_workgroup": rows, "workgroups": (n + rows - 1) // rows,
            "pass_gb_per_s": round((read_bytes + write_bytes) / (med(ms) * 1e-3) / 1e9, 2),
            "msamples_per_s": round(samples / (med(ms) * 1e-3) / 1e6, 1),
            "pass_over_issue_model": round(med(ms) / model_ms, 3),
            "pass_over_d2d_plus_launch": round(med(ms) / (med(d2d) + med(launch)), 3)}
    print(json.dumps(line), flush=True)
    f.close()


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
