"""DCS squelch (include/asdr_dcs.h): time of the pass at the sizes a bank is used at.

    python tools/bench_dcs.py [config ...]        (default: D2 D2x8 D5)

    D2     65,536 channels x 1 block of 44.1 kHz audio rows (128 samples: an FM demodulator step's output)
    D2x8   65,536 channels x 8 blocks
    D5     512 channels x 646 blocks      (a capture-sink call)
    D1n, D1w   32,767 and 32,768 channels x 8 blocks: either side of the size at which a workgroup takes 64 channels instead of 16

Prints ONE JSON line per configuration.  The rows are a DCS word (NRZ at 134.4 bit/s, amplitude 1000) in noise of rms 3000 on three
channels of four from a seed, noise alone on the fourth; the creation table of 104 codes, and a want that is, of four channels, PASS,
the own code, another code and ANY.  Every channel starts from the record of a channel in lock (200 blocks through a bank of 64, its
records written into the timed bank), so open channels and muted ones are both there.  Every line carries the algorithmic bytes from
the shapes: the pass reads one int16 row and writes one, and reads and writes every channel's 192-byte record once per call.  Timed
with device events on one stream around enough warmed calls to fill 0.3 s, three repeats (all three are printed, the median is used
for the ratios).  Beside them, from the same run, the yardsticks: a device-to-device copy of a buffer of the same input plus output
plus record (read and written) bytes, and the time per launch of a one-element kernel (the pass is one kernel)."""
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

CONFIGS = {"D2": (65536, 1), "D2x8": (65536, 8), "D5": (512, 646), "D1n": (32767, 8), "D1w": (32768, 8)}   # name -> (channels, blocks)
DEFAULT = ("D2", "D2x8", "D5")
FILL_S, REPEATS = 0.3, 3
RECORD, LOCK_BLOCKS, DISTINCT = 192, 200, 64


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


def want_of(c):
    """Of four channels: search only, the own code, another code, any code."""
    return (A.DCS_PASS, c % 104, (c + 7) % 104, A.DCS_ANY)[c % 4]


def audio(rng, n, nb, first_block=0):
    """int16 [n][nb][128]: noise of rms 3000 plus, on three channels of four, the word of code c % 104 as NRZ of amplitude 1000;
    the search-only channels (c % 4 == 0) are the ones with noise alone."""
    k = np.arange(128 * first_block, 128 * (first_block + nb), dtype=np.float64)
    bit = np.floor(k * 134.4 / 44100.0).astype(np.int64)
    x = rng.normal(0.0, 3000.0, size=(n, nb * 128))
    for c in range(n):
        if c % 4 != 0:
            w = A.dcs_word(A.DCS_CODES[c % 104])
            x[c] += 1000.0 * (2.0 * ((w >> ((bit + c) % 23)) & 1) - 1.0)
    return np.clip(np.floor(x + 0.5), -32768, 32767).astype(np.int16).reshape(n, nb, 128)


def locked_records():
    """The records of DISTINCT channels after LOCK_BLOCKS blocks of their signal."""
    t = A.DcsSquelch(DISTINCT)
    for c in range(DISTINCT):
        t.set_want(want_of(c), ch=c)
    x = torch.from_numpy(audio(np.random.default_rng(0), DISTINCT, LOCK_BLOCKS)).cuda()
    y = torch.zeros_like(x)
    t.update_device(x.data_ptr(), y.data_ptr(), LOCK_BLOCKS)
    rec = t.read_state()
    t.close()
    return rec


def run(name):
    n, nb = CONFIGS[name]
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    x = audio(np.random.default_rng(1), DISTINCT, nb, first_block=LOCK_BLOCKS)      # 64 different channels, repeated
    d_in = torch.from_numpy(x).cuda().repeat((n + DISTINCT - 1) // DISTINCT, 1, 1)[:n].contiguous()
    d_out = torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda")
    samples = n * nb * 128
    read_bytes, write_bytes = samples * 2 + n * RECORD, samples * 2 + n * RECORD
    d_src = torch.zeros(read_bytes + write_bytes, dtype=torch.uint8, device="cuda")
    d_dst = torch.empty_like(d_src)
    one = torch.zeros(1, device="cuda")
    t = A.DcsSquelch(n)
    for c in range(DISTINCT):
        for k in range(c, n, DISTINCT):
            t._L.asdr_dcs_set_want(t._h, k, want_of(c))
    rec = locked_records()
    t.write_state(rec[np.arange(n) % DISTINCT])
    opened, named = int(rec["open"].sum()), int((rec["detected"] >= 0).sum())
    assert 0 < opened < DISTINCT and named > DISTINCT // 2, (opened, named)           # the squelch separates the channels
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        launch, _ = events_ms(lambda: one.add_(0.0), stream)
        d2d, _ = events_ms(lambda: d_dst.copy_(d_src, non_blocking=True), stream)   # a copy of as many bytes as the pass reads and writes
    ms, reps = events_ms(lambda: t.update_device(d_in.data_ptr(), d_out.data_ptr(), nb, stream=sp), stream)
    st = t.read_state()
    assert t.blocks() > 0 and int(st["bits"].min()) > 0 and int(st["open_blocks"].max()) > 0
    rows = A.DCS_ROWS if n >= A.DCS_WIDE_CHANNELS else A.DCS_NARROW_ROWS
    line = {"bench": "dcs_squelch", "config": name, "n_channels": n, "n_blocks": nb, "samples": samples, "read_bytes": read_bytes,
            "write_bytes": write_bytes, "record_bytes_each_way": n * RECORD, "source_sha256": build.source_sha256()[:16],
            "n_codes": 104, "channels_in_lock_of_64": named, "channels_open_of_64": opened, "timed_calls": reps, "pass_ms": ms,
            "d2d_copy_of_pass_bytes_ms": d2d, "tiny_launch_ms": launch,
            "rows_per_workgroup": rows, "workgroups": (n + rows - 1) // rows,
            "pass_gb_per_s": round((read_bytes + write_bytes) / (med(ms) * 1e-3) / 1e9, 2),
            "msamples_per_s": round(samples / (med(ms) * 1e-3) / 1e6, 1),
            "us_per_block_of_a_workgroup": round(med(ms) * 1e3 / nb, 3),
            "pass_over_d2d_plus_launch": round(med(ms) / (med(d2d) + med(launch)), 3)}
    print(json.dumps(line), flush=True)
    t.close()


def main():
    args = sys.argv[1:]
    for name in (args or list(DEFAULT)):
        if name not in CONFIGS:
            print("unknown configuration %r (one of %s)" % (name, " ".join(CONFIGS)), file=sys.stderr)
            return 2
        run(name)
    return 0


if __name__ == "__main__":
    sys.exit(main())
