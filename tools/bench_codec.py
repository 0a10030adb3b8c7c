"""Audio codec (include/asdr_codec.h): time of the encoding pass and of asdr_codec_deliver at the sizes a bank is used at.

    python tools/bench_codec.py [config ...] [--kinds ulaw,alaw,adpcm]        (default: K2 K2r K2x8 K5, all kinds)

    K2     65,536 receivers x 1 block of 44.1 kHz rows (128 samples: a C2 step's audio), all channels
    K2r    65,536 receivers x 35-sample rows in strides of 40, as a 12 kHz resampler leaves one block; the compact index form
           (rows_compact = 1) with 10 % and 100 % of the channels delivered
    K2x8   65,536 receivers x 8 blocks
    K5     512 receivers x 646 blocks      (a capture-sink call)

Prints ONE JSON line per configuration, kind and share.  The rows are full-range noise from a seed (the ADPCM chain takes the same
instructions whatever the data; its table reads spread over the whole table).  Every line carries the algorithmic bytes from the
shapes: the pass reads rows * n_samples * 2 and writes rows * the row's bytes rounded up to 4.  Timed with device events on one
stream around enough warmed calls to fill 0.3 s, three repeats (all three are printed, the median is used for the ratios); deliver
is synchronous, writes its rows into pinned memory and is timed by the wall clock.  Beside them, from the same run, the yardsticks:
a device-to-device copy of the same input bytes plus the time per launch of a one-element kernel (the pass is one kernel), and a
device-to-host copy of the delivered rows' raw int16 samples into pinned memory (what crosses PCIe without a codec)."""
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

# name -> (channels, samples per row, row stride in samples, shares of delivered channels; None: all channels, no index)
CONFIGS = {"K2": (65536, 128, 128, (None,)), "K2r": (65536, 35, 40, (0.1, 1.0)), "K2x8": (65536, 1024, 1024, (None,)),
           "K5": (512, 646 * 128, 646 * 128, (None,))}
KINDS = ("ulaw", "alaw", "adpcm")
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


def wall_ms(fn):
    for _ in range(2):
        fn()
    t0 = time.perf_counter()
    fn()
    reps = max(3, int(FILL_S / max(time.perf_counter() - t0, 1e-6)) + 1)
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append(round((time.perf_counter() - t0) / reps * 1e3, 5))
    return out, reps


def med(v):
    return sorted(v)[len(v) // 2]


def run(name, kinds):
    n, ns, stride, shares = CONFIGS[name]
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    rng = np.random.default_rng(1)
    x = rng.integers(-32768, 32768, size=(n, stride), dtype=np.int16)
    d_x = torch.from_numpy(x).cuda()
    one = torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        launch, _ = events_ms(lambda: one.add_(0.0), stream)
    for share in shares:
        k = n if share is None else int(round(share * n))
        index = np.sort(rng.permutation(n)[:k]).astype(np.int32)
        d_index = torch.from_numpy(index).cuda()
        d_count = torch.tensor([k], dtype=torch.int32, device="cuda")
        d_copy = torch.empty((k, stride), dtype=torch.int16, device="cuda")
        pinned_raw = torch.empty((k, stride), dtype=torch.int16).pin_memory()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):                          # the yardsticks: the same k rows, device to device and to the host
            d2d, _ = events_ms(lambda: d_copy.copy_(d_x[:k], non_blocking=True), stream)
            d2h, _ = events_ms(lambda: pinned_raw.copy_(d_x[:k], non_blocking=True), stream)
        for kind in kinds:
            c = A.AudioCodec(n, kind=kind)
            row_bytes = c.row_bytes(ns)
            padded = (row_bytes + 3) & ~3
            d_out = torch.empty((k, padded), dtype=torch.uint8, device="cuda")
            pinned = torch.empty((n, padded), dtype=torch.uint8).pin_memory()
            form = dict() if share is None else dict(rows_compact=True, index_ptr=d_index.data_ptr(), count_ptr=d_count.data_ptr(), capacity_rows=n)
            torch.cuda.synchronize()
            enc, reps = events_ms(lambda: c.encode_device(d_x.data_ptr(), ns, d_out.data_ptr(), padded, row_stride_samples=stride, stream=sp, **form),
                                  stream)
            dl, _ = wall_ms(lambda: c.deliver(d_x.data_ptr(), ns, row_stride_samples=stride, stream=sp, rows_out=pinned.numpy(), **form))
            count, _, got = c.deliver(d_x.data_ptr(), ns, row_stride_samples=stride, stream=sp, **form)
            assert count == k and got.shape == (k, padded)
            back = A.AudioCodec.decode(kind, got[:4], ns)        # a listener's view of the first rows: the codec's error bound, or a header
            if kind != "adpcm":
                assert np.abs(back.astype(int) - x[:4, :ns]).max() <= 644
            read_bytes, write_bytes = k * ns * 2, k * padded
            line = {"bench": "audio_codec", "config": name, "kind": kind, "n_channels": n, "n_samples": ns, "row_stride_samples": stride,
                    "share_delivered": share, "rows": k, "row_bytes": row_bytes, "read_bytes": read_bytes, "write_bytes": write_bytes,
                    "raw_bytes_to_host": read_bytes, "coded_bytes_to_host": write_bytes + 4 + (0 if share is None else 4 * k),
                    "source_sha256": build.source_sha256()[:16], "timed_calls": reps, "encode_ms": enc, "deliver_ms": dl,
                    "d2d_copy_ms": d2d, "d2h_pinned_raw_ms": d2h, "tiny_launch_ms": launch,
                    "encode_gb_per_s": round((read_bytes + write_bytes) / (med(enc) * 1e-3) / 1e9, 2),
                    "encode_over_d2d_plus_launch": round(med(enc) / (med(d2d) + med(launch)), 4),
                    "deliver_over_raw_d2h": round(med(dl) / med(d2h), 4)}
            print(json.dumps(line), flush=True)
            c.close()


def main():
    args = sys.argv[1:]
    kinds = KINDS
    if "--kinds" in args:                                      # e.g. --kinds adpcm for a kernel trace of one case
        k = args.index("--kinds")
        kinds = tuple(args[k + 1].split(","))
        del args[k:k + 2]
    for name in (args or list(CONFIGS)):
        if name not in CONFIGS or any(kind not in KINDS for kind in kinds):
            print("unknown configuration %r or kind (one of %s; %s)" % (name, " ".join(CONFIGS), " ".join(KINDS)), file=sys.stderr)
            return 2
        run(name, kinds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
