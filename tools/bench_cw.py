"""CW decoder (include/asdr_cw.h): time of the pass and of the delivery at the sizes a bank is used at.

    python tools/bench_cw.py [config ...]        (default: W2 W2x8 W5 WC)

    W2     65,536 channels x 1 block of 44.1 kHz audio rows (128 samples: a chain step's output)
    W2x8   65,536 channels x 8 blocks
    W5     512 channels x 646 blocks      (a capture-sink call)
    W1n, W1w   32,767 and 32,768 channels x 8 blocks: either side of the size at which a workgroup takes 64 channels instead of 16
    WC     65,536 channels, one in a hundred holding an event: collect_device and deliver

Prints ONE JSON line per configuration.  The rows are random keying at 40 to 60 WPM on a 774 Hz tone of amplitude 3000 in noise of rms
300 on three channels of four from a seed, noise alone (rms 3000) on the fourth; 64 different channels, repeated.  Every line carries
the algorithmic bytes from the shapes: the pass reads one int16 row, and reads and writes the first 64 bytes of every channel's record
and its 16 bytes of ring bookkeeping once per call (and reads its 16 bytes of settings).  Timed with device events on one stream
around enough warmed calls to fill 0.3 s, three repeats (all three are printed, the median is used for the ratios).  Beside them, from
the same run, the yardsticks: a device-to-device copy of a buffer of the same bytes, and the time per launch of a one-element kernel
(the pass is one kernel, a collect three).  WC refills the rings before every timed collect (a call of the character's blocks, not
timed), so its figures are single calls between two events, five of them."""
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

CONFIGS = {"W2": (65536, 1), "W2x8": (65536, 8), "W5": (512, 646), "W1n": (32767, 8), "W1w": (32768, 8), "WC": (65536, 0)}
DEFAULT = ("W2", "W2x8", "W5", "WC")
FILL_S, REPEATS = 0.3, 3
LOADED, BOOKKEEPING, SETTING, SLOT, DISTINCT = 64, 16, 16, 16, 64
FS, WARM = 44100, 200


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
    """int16 [n][nb][128]: noise of rms 300 plus, on three channels of four, random keying of amplitude 3000; noise of rms 3000 on the
    fourth."""
    N = nb * 128
    x = rng.normal(0.0, 300.0, size=(n, N))
    t = np.arange(N)
    for c in range(n):
        if c % 4 == 3:
            x[c] *= 10.0
            continue
        dit = FS * 1.2 / rng.uniform(40.0, 60.0)
        gate, a = np.zeros(N), int(rng.integers(0, 400))
        while a < N:
            m = int(dit * (1 if rng.random() < 0.55 else 3))
            gate[a:a + m] = 1.0
            a += m + int(dit * (1, 1, 1, 3, 3, 7)[int(rng.integers(0, 6))])
        x[c] += 3000.0 * gate * np.cos(2 * np.pi * 774.0 * t / FS)
    return np.clip(np.floor(x + 0.5), -32768, 32767).astype(np.int16).reshape(n, nb, 128)


def yardsticks(stream, n_bytes):
    d_src = torch.zeros(max(n_bytes, 16), dtype=torch.uint8, device="cuda")
    d_dst = torch.empty_like(d_src)
    one = torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        launch, _ = events_ms(lambda: one.add_(0.0), stream)
        d2d, _ = events_ms(lambda: d_dst.copy_(d_src, non_blocking=True), stream)
    return d2d, launch


def run_pass(name):
    n, nb = CONFIGS[name]
    stream = torch.cuda.Stream()
    x = audio(np.random.default_rng(1), DISTINCT, max(nb, WARM))
    warm = torch.from_numpy(x[:, :WARM].copy()).cuda().repeat((n + DISTINCT - 1) // DISTINCT, 1, 1)[:n].contiguous()
    d_in = torch.from_numpy(x[:, :nb].copy()).cuda().repeat((n + DISTINCT - 1) // DISTINCT, 1, 1)[:n].contiguous()
    samples = n * nb * 128
    read_bytes, write_bytes = samples * 2 + n * (LOADED + BOOKKEEPING + SETTING), n * (LOADED + BOOKKEEPING)
    t = A.CwDecoder(n, ring=16)
    t.set_speed(50)
    t.update_device(warm.data_ptr(), WARM)                      # the trackers have found the levels; marks are under way
    st = t.read_state()
    assert int((st["marks"] > 0).sum()) > n // 2
    d2d, launch = yardsticks(stream, read_bytes + write_bytes)
    ms, reps = events_ms(lambda: t.update_device(d_in.data_ptr(), nb, stream=stream.cuda_stream), stream)
    st = t.read_state()
    chars = int(st["chars"].astype(np.int64).sum())
    assert t.blocks() > 0 and chars > 0
    rows = A.CW_ROWS if n >= A.CW_WIDE_CHANNELS else A.CW_NARROW_ROWS
    line = {"bench": "cw_decoder", "config": name, "n_channels": n, "n_blocks": nb, "samples": samples, "read_bytes": read_bytes,
            "write_bytes": write_bytes, "source_sha256": build.source_sha256()[:16], "timed_calls": reps, "characters_decoded": chars,
            "pass_ms": ms, "d2d_copy_of_pass_bytes_ms": d2d, "tiny_launch_ms": launch, "rows_per_workgroup": rows,
            "workgroups": (n + rows - 1) // rows, "pass_gb_per_s": round((read_bytes + write_bytes) / (med(ms) * 1e-3) / 1e9, 2),
            "msamples_per_s": round(samples / (med(ms) * 1e-3) / 1e6, 1), "us_per_block_of_a_workgroup": round(med(ms) * 1e3 / nb, 3),
            "pass_over_d2d_plus_launch": round(med(ms) / (med(d2d) + med(launch)), 3)}
    print(json.dumps(line), flush=True)
    t.close()


def run_collect(name):
    n = CONFIGS[name][0]
    stream = torch.cuda.Stream()
    nb = 80                                                     # a dash of 40 blocks behind 10 of silence, then 30 of silence: one 'T'
    w = np.zeros(nb * 128)
    w[1280:6400] = 3000.0 * np.cos(2 * np.pi * 774.0 * np.arange(5120) / FS)
    w = np.floor(w + 0.5).astype(np.int16).reshape(nb, 128)
    d_in = torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda")
    d_in[::100] = torch.from_numpy(w).cuda()
    holders = len(range(0, n, 100))
    max_events = 4096
    d_events = torch.zeros(max_events * SLOT, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = A.CwDecoder(n, ring=16)
    t.set_speed(50)
    t.set_track(0)

    def refill():
        t.reset()
        t.set_speed(50)
        t.update_device(d_in.data_ptr(), nb, stream=stream.cuda_stream)

    n_bytes = 2 * n * BOOKKEEPING + 2 * holders * SLOT + holders * (4 + BOOKKEEPING)
    d2d, launch = yardsticks(stream, n_bytes)
    full, host = [], []
    for _ in range(5):
        refill()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t.collect_device(d_count.data_ptr(), d_events.data_ptr(), max_events, stream=stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        assert int(d_count.cpu()[0]) == holders, (int(d_count.cpu()[0]), holders)
        full.append(round(e0.elapsed_time(e1), 5))
    empty, reps = events_ms(lambda: t.collect_device(d_count.data_ptr(), d_events.data_ptr(), max_events, stream=stream.cuda_stream), stream)
    stream.synchronize()
    assert int(d_count.cpu()[0]) == 0
    for _ in range(5):
        refill()
        t.synchronize()
        t0 = time.perf_counter()
        got = t.deliver(max_events)
        host.append(round((time.perf_counter() - t0) * 1e3, 5))
        assert len(got) == holders and got["channel"].tolist() == list(range(0, n, 100)) and A.CwDecoder.text(got) == "T" * holders
    line = {"bench": "cw_collect", "config": name, "n_channels": n, "ring": 16, "max_events": max_events, "events": holders,
            "bytes": n_bytes, "source_sha256": build.source_sha256()[:16], "collect_ms": full, "collect_nothing_waiting_ms": empty,
            "timed_calls_nothing_waiting": reps, "deliver_host_ms": host, "d2d_copy_of_collect_bytes_ms": d2d, "tiny_launch_ms": launch,
            "collect_over_d2d_plus_3_launches": round(med(full) / (med(d2d) + 3 * med(launch)), 3)}
    print(json.dumps(line), flush=True)
    t.close()


def main():
    args = sys.argv[1:]
    for name in (args or list(DEFAULT)):
        if name not in CONFIGS:
            print("unknown configuration %r (one of %s)" % (name, " ".join(CONFIGS)), file=sys.stderr)
            return 2
        (run_collect if name == "WC" else run_pass)(name)
    return 0


if __name__ == "__main__":
    sys.exit(main())
