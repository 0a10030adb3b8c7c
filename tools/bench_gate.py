"""Audio gate (include/asdr_gate.h): time of the pass and of asdr_gate_deliver at the sizes a bank is used at.

    python tools/bench_gate.py [config ...] [--shares 0,0.1,1]        (default: G2 G2x8 G5)

    G2     65,536 receivers x 1 block      (a C2 step's audio)
    G2x8   65,536 receivers x 8 blocks
    G5     512 receivers x 646 blocks      (a capture-sink call)

Prints ONE JSON line per configuration and share of open channels (0 %, 10 %, 100 %).  The rows are made from a seed: the chosen
share of the channels (a seeded permutation's first k) carries noise of amplitude 2000, the rest of amplitude 20, and the
threshold lies between the two block energies, so exactly that share is delivered (the line's `count`, read back, says so).
Every line carries the algorithmic bytes from the shapes: the pass reads n * n_blocks * 256, the packet adds 2 * open * n_blocks * 256
(read and written).  Timed with device events on one stream around enough warmed calls to fill 0.3 s, three repeats (all three are
printed, the median is used for the rates); deliver is synchronous, writes its rows into pinned memory and is timed by the wall clock.  Beside them, from the same run: a
device-to-device hipMemcpyAsync of the same rows, a device-to-host copy of all rows into pinned memory, and the time per launch of a
one-element kernel (the price of a launch)."""
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

CONFIGS = {"G2": (65536, 1), "G2x8": (65536, 8), "G5": (512, 646)}
SHARES = (0.0, 0.1, 1.0)
LOUD, QUIET = 2000, 20
THRESHOLD = 128 * 200 * 200        # between 128 * QUIET^2 and the energy of any block of uniform noise of amplitude LOUD
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


def rows(n, nb, share, seed):
    rng = np.random.default_rng(seed)
    k = int(round(share * n))
    loud = np.zeros(n, dtype=bool)
    loud[rng.permutation(n)[:k]] = True
    a = rng.integers(-QUIET, QUIET + 1, size=(n, nb, 128), dtype=np.int16)
    a[loud] = rng.integers(-LOUD, LOUD + 1, size=(k, nb, 128), dtype=np.int16)
    E = (a.astype(np.int64) ** 2).sum(-1)
    assert (E[loud] >= THRESHOLD).all() and (E[~loud] < THRESHOLD).all()
    return a, k


def run(name):
    n, nb = CONFIGS[name]
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    read_bytes = n * nb * 256
    d_copy = torch.empty((n, nb, 128), dtype=torch.int16, device="cuda")
    d_rows = torch.empty((n, nb, 128), dtype=torch.int16, device="cuda")
    pinned = torch.empty((n, nb, 128), dtype=torch.int16).pin_memory()
    one = torch.zeros(1, device="cuda")
    base = {"bench": "audio_gate", "config": name, "n_channels": n, "n_blocks": nb, "read_bytes": read_bytes,
            "source_sha256": build.source_sha256()[:16]}
    with torch.cuda.stream(stream):
        launch, _ = events_ms(lambda: one.add_(0.0), stream)
    for share in SHARES:
        a, k = rows(n, nb, share, seed=1)
        d_audio = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        g = A.AudioGate(n)
        g.set_squelch(energies=(THRESHOLD, THRESHOLD), hang_blocks=0)
        with torch.cuda.stream(stream):
            d2d, _ = events_ms(lambda: d_copy.copy_(d_audio, non_blocking=True), stream)
            d2h, _ = events_ms(lambda: pinned.copy_(d_audio, non_blocking=True), stream)
        p, reps = events_ms(lambda: g.update_device(d_audio.data_ptr(), nb, stream=sp), stream)
        pk, _ = events_ms(lambda: g.update_device(d_audio.data_ptr(), nb, rows_ptr=d_rows.data_ptr(), capacity_rows=n, stream=sp), stream)
        count = int(g.count_tensor().cpu()[0])
        assert count == k, (count, k)
        dl, _ = wall_ms(lambda: g.deliver(d_audio.data_ptr(), nb, rows_out=pinned.numpy()))   # into the same pinned memory
        index, got = g.deliver(d_audio.data_ptr(), nb)
        assert len(index) == k and np.array_equal(got, a[index])
        packet_bytes = 2 * k * nb * 256
        kernels = (2 if nb == 1 else 3)
        line = dict(base, share_open=share, count=count, packet_bytes=packet_bytes, pass_kernels=kernels, timed_calls=reps,
                    pass_ms=p, pass_packet_ms=pk, deliver_ms=dl, d2d_copy_ms=d2d, d2h_pinned_ms=d2h, tiny_launch_ms=launch,
                    pass_tb_per_s=round(read_bytes / (med(p) * 1e-3) / 1e12, 4),
                    pass_packet_tb_per_s=round((read_bytes + packet_bytes) / (med(pk) * 1e-3) / 1e12, 4),
                    pass_over_d2d_plus_launches=round(med(p) / (med(d2d) + kernels * med(launch)), 4),
                    deliver_over_full_d2h=round(med(dl) / med(d2h), 4))
        print(json.dumps(line), flush=True)
        g.close()


def main():
    global SHARES
    args = sys.argv[1:]
    if "--shares" in args:                                     # e.g. --shares 0.1 for a kernel trace of one case
        k = args.index("--shares")
        SHARES = tuple(float(v) for v in args[k + 1].split(","))
        del args[k:k + 2]
    for name in (args or list(CONFIGS)):
        if name not in CONFIGS:
            print("unknown configuration %r (one of %s)" % (name, " ".join(CONFIGS)), file=sys.stderr)
            return 2
        run(name)
    return 0


if __name__ == "__main__":
    sys.exit(main())
