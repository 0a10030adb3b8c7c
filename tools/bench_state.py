"""Receiver state records (include/asdr.h): time of the device forms asdr_export_state_device / asdr_import_state_device
for a C2 bank (USB, audio filter; blanker and AGC on) of 65,536 and of 1,024 channels, all channels per call.

    python tools/bench_state.py [channels ...]        (default: 65536 1024)

Prints ONE JSON line.  Per size: ms per export, ms per import (device events around warmed calls on one stream, at least 0.5 s of timed
work each), bytes moved (every byte of a record is read once and written once: 2 x channels x record size) / time, beside the copy rate
an MI355X reaches with 16-byte accesses (6.29 TB/s measured, 79 % of the 8 TB/s specification).  The export is one asynchronous launch
and a 160-byte-per-channel upload of the control parts; the import first brings those 160 bytes per channel to the host, checks them and
converts them to the host rows -- host work that the event pair includes."""
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


def run(n_ch):
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    b = A.AudioSDRBatch(n_ch)
    b.setDemodMode(A.USBmode); b.enableAudioFilter()
    rng = np.random.default_rng(1)
    nb = 4
    I = torch.from_numpy(rng.integers(-8000, 8000, size=(n_ch, nb, 128), dtype=np.int16)).cuda()
    Q = torch.from_numpy(rng.integers(-8000, 8000, size=(n_ch, nb, 128), dtype=np.int16)).cuda()
    out = torch.empty_like(I)
    b.update_device(I.data_ptr(), Q.data_ptr(), out.data_ptr(), nb, stream=sp)      # a running bank: every row holds signal state
    R = b.STATE_RECORD_BYTES
    rec = torch.zeros(n_ch * R, dtype=torch.uint8, device="cuda")
    res = {}
    for what, fn in (("export", lambda: b.export_state_device(rec.data_ptr(), stream=sp)),
                     ("import", lambda: b.import_state_device(rec.data_ptr(), stream=sp))):
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
        moved = 2 * n_ch * R
        res[what] = {"ms": round(ms, 4), "timed_calls": reps, "bytes_moved": moved, "tb_per_s": round(moved / (ms * 1e-3) / 1e12, 4),
                     "share_of_copy_rate": round(moved / (ms * 1e-3) / COPY_RATE, 4)}
    # the bank still runs, and the records it exported are the ones it holds
    b.update_device(I.data_ptr(), Q.data_ptr(), out.data_ptr(), nb, stream=sp)
    b.synchronize()
    b.close()
    return res


def main():
    out = {"bench": "state_records", "config": "C2 (USB, audio filter)", "record_bytes": A.state_record_bytes(),
           "copy_rate_tb_per_s": COPY_RATE / 1e12, "source_sha256": build.source_sha256()[:16], "sizes": {}}
    for n_ch in ([int(a) for a in sys.argv[1:]] or [65536, 1024]):
        out["sizes"][str(n_ch)] = run(n_ch)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
