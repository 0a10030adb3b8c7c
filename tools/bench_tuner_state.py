"""Tuner state records (include/asdr_tuner.h "State records"): time of the device forms
asdr_tuner_export_channels_device / asdr_tuner_import_channels_device for all channels of an F4-sized fast-convolution bank (65,536
channels, 16 sources, 2.4 MS/s, R = 16; stage 2 resamples 147 / 500, so every channel has a live carry row), and of the host forms
asdr_tuner_export_bank_state / asdr_tuner_import_bank_state of the same bank.

    python tools/bench_tuner_state.py [channels]        (default: 65536)

Prints ONE JSON line.  Channel records: ms per export and per import (device events around warmed calls on one stream, at least 0.5 s
of timed work each), bytes moved (every byte of a record is read once and written once: 2 x channels x 2,560) / time, beside the copy
rate an MI355X reaches with 16-byte accesses (6.29 TB/s measured).  The export is one launch and a 256-byte-per-channel upload of the
heads; the import first brings those 256 bytes per channel to the host and checks them -- host work that the event pair includes.
Bank state: wall-clock ms per call (the calls synchronise) and the blob's size."""
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

COPY_RATE = 6.29e12     # bytes / s, float4 copy
FS, R, N_SRC = 2400000, 16, 16


def run(n_ch):
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    t = A.TunerBank.fastconv(n_ch, N_SRC, FS, R)
    rng = np.random.default_rng(1)
    for c in range(0, n_ch, max(1, n_ch // 64)):
        t.set_source(c % N_SRC, ch=c); t.set_frequency(float(rng.uniform(-1e6, 1e6)), ch=c)
    nf = 2
    x = torch.from_numpy(rng.integers(-8000, 8000, size=(N_SRC, nf * 128 * R, 2), dtype=np.int16)).cuda()
    cap = t.out_blocks(nf) + 1
    dI = torch.empty((n_ch, cap, 128), dtype=torch.int16, device="cuda")
    dQ = torch.empty_like(dI)
    for _ in range(2):                                                     # a running bank: every carry row holds signal
        t.update_samples_device(x.data_ptr(), dI.data_ptr(), dQ.data_ptr(), nf, cap, stream=sp)
    RB = A.tuner.CHANNEL_RECORD_BYTES
    rec = torch.zeros(n_ch * RB, dtype=torch.uint8, device="cuda")
    res = {}
    for what, fn in (("export", lambda: t.export_channels_device(rec.data_ptr(), None, sp)),
                     ("import", lambda: t.import_channels_device(rec.data_ptr(), None, sp))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        est = max((time.perf_counter() - t0) / 3, 1e-5)
        reps = max(10, int(0.6 / est) + 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        moved = 2 * n_ch * RB
        res[what] = {"ms": round(ms, 4), "timed_calls": reps, "bytes_moved": moved, "tb_per_s": round(moved / (ms * 1e-3) / 1e12, 4),
                     "share_of_copy_rate": round(moved / (ms * 1e-3) / COPY_RATE, 4)}
    blob = t.export_bank_state()
    bank = {"bytes": int(blob.size)}
    for what, fn in (("export", t.export_bank_state), ("import", lambda: t.import_bank_state(blob))):
        fn()
        t0 = time.perf_counter()
        for _ in range(10):
            fn()
        bank[what + "_ms"] = round((time.perf_counter() - t0) / 10 * 1e3, 4)
    # the bank still runs after all of it (the import left every channel in creation state at the blob's position)
    t.update_samples_device(x.data_ptr(), dI.data_ptr(), dQ.data_ptr(), nf, cap, stream=sp)
    t.synchronize()
    t.close()
    return {"channels": res, "bank_state": bank}


def main():
    n_ch = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    out = {"bench": "tuner_state_records", "config": "F4 (fast convolution, %d sources, %d S/s, R = %d)" % (N_SRC, FS, R), "n_channels": n_ch,
           "record_bytes": A.tuner.CHANNEL_RECORD_BYTES, "copy_rate_tb_per_s": COPY_RATE / 1e12, "source_sha256": build.source_sha256()[:16]}
    out.update(run(n_ch))
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
