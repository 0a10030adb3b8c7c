"""Audio resampler (include/asdr_resample.h): time of the pass at the sizes a bank is used at.

    python tools/bench_resample.py [case ...] [--c2-ms MS]      (default: every case)

    R2        65,536 receivers x 1 block at 12 kHz     (a C2 step's audio)
    R2x8      65,536 receivers x 8 blocks
    R5        512 receivers x 646 blocks               (a capture-sink call)
    R5slot    512 receivers x 41,344 blocks            (a 2-minute slot straight from a capture-sink-shaped buffer; skipped with
                                                        the reason in the line when the memory is not there)
    R2@8k     R2 at 8 kHz
    R2i10     R2 in the index form, 10 % of the channels delivered
    R2i100    R2 in the index form, every channel delivered

Prints ONE JSON line per case and appends it to profiles/audio_resample.jsonl.  Timed with device events on one stream around
enough warmed calls to fill 0.3 s, three repeats (all three are printed, the median is used for the ratios).  Beside them, from the
same run: a device-to-device hipMemcpyAsync of the same input rows, the time per launch of a one-element kernel (the price of a
launch; a call is two launches: the pass and the carry), and the arithmetic model -- n * n_out * K / 2 dot instructions of 64 lanes
at 7.86e13 lane-ops/s.  --c2-ms is `ms_per_step` of `python bench.py` of the same visit, carried in every line."""
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

# case -> (n_channels, n_blocks, fs_out, delivered share or None for the direct form)
CASES = {"R2": (65536, 1, 12000, None), "R2x8": (65536, 8, 12000, None), "R5": (512, 646, 12000, None), "R5slot": (512, 41344, 12000, None),
         "R2@8k": (65536, 1, 8000, None), "R2i10": (65536, 1, 12000, 0.1), "R2i100": (65536, 1, 12000, 1.0)}
FILL_S, REPEATS = 0.3, 3
LANE_OPS_PER_S = 7.86e13
OUT = os.path.join(ROOT, "profiles", "audio_resample.jsonl")


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


def run(name, c2_ms):
    n, nb, fs, share = CASES[name]
    base = {"bench": "audio_resample", "case": name, "n_channels": n, "n_blocks": nb, "fs_out": fs, "share_delivered": share,
            "read_bytes": n * nb * 256, "source_sha256": build.source_sha256()[:16], "bench_py_c2_ms_per_step": c2_ms}
    free = torch.cuda.mem_get_info()[0]
    need = 2 * n * nb * 256 + n * nb * 80 + (1 << 28)            # the rows, their copy, the output rows, and slack
    if need > free:
        return dict(base, skipped="needs %.1f GB of device memory, %.1f GB free" % (need / 1e9, free / 1e9))
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    rs = A.AudioResampler(n, fs_out=fs)
    K, count = rs.taps_per_phase(), rs.out_samples(nb)
    gen = torch.Generator(device="cuda").manual_seed(1)
    d_audio = torch.randint(-20000, 20001, (n, nb, 128), dtype=torch.int16, device="cuda", generator=gen)
    d_copy = torch.empty_like(d_audio)
    stride = count + 2                                           # 34 and 35 outputs alternate: room for either
    rows = n if share is None else int(round(share * n))
    d_out = torch.zeros((max(rows, 1), stride), dtype=torch.int16, device="cuda")
    one = torch.zeros(1, device="cuda")
    kw = {}
    if share is not None:
        index = np.sort(np.random.default_rng(1).permutation(n)[:rows]).astype(np.int32)
        d_index, d_count = torch.from_numpy(index).cuda(), torch.tensor([rows], dtype=torch.int32, device="cuda")
        kw = dict(index_ptr=d_index.data_ptr(), count_ptr=d_count.data_ptr(), capacity_rows=rows)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        launch, _ = events_ms(lambda: one.add_(0.0), stream)
        d2d, _ = events_ms(lambda: d_copy.copy_(d_audio, non_blocking=True), stream)
    ms, reps = events_ms(lambda: rs.update_device(d_audio.data_ptr(), nb, d_out.data_ptr(), stride, stream=sp, **kw), stream)
    n_out = rows * count
    model_ms = n_out * K / 2 / LANE_OPS_PER_S * 1e3
    line = dict(base, up=rs.up, down=rs.down, taps_per_phase=K, out_samples_per_row=count, rows_written=rows, launches=2, timed_calls=reps,
                resample_ms=ms, d2d_copy_ms=d2d, tiny_launch_ms=launch, arithmetic_model_ms=round(model_ms, 5),
                input_tb_per_s=round(n * nb * 256 / (med(ms) * 1e-3) / 1e12, 4),
                over_copy_plus_launches=round(med(ms) / (med(d2d) + 2 * med(launch)), 3),
                over_arithmetic_model=round(med(ms) / model_ms, 3),
                over_c2_step=None if not c2_ms else round(med(ms) / (c2_ms * nb), 4))
    rs.close()
    return line


def main():
    args = sys.argv[1:]
    c2_ms = None
    if "--c2-ms" in args:
        k = args.index("--c2-ms")
        c2_ms = float(args[k + 1])
        del args[k:k + 2]
    for name in (args or list(CASES)):
        if name not in CASES:
            print("unknown case %r (one of %s)" % (name, " ".join(CASES)), file=sys.stderr)
            return 2
        line = json.dumps(run(name, c2_ms))
        print(line, flush=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
