"""Packet decoder (include/asdr_packet.h): time of the pass and of the delivery at the sizes a bank is used at.

    python tools/bench_packet.py [config ...]        (default: P2 P2x8 P5 PC)

    P2     65,536 channels x 1 block of 44.1 kHz audio rows (128 samples: an FM demodulator step's output)
    P2x8   65,536 channels x 8 blocks
    P5     512 channels x 646 blocks      (a capture-sink call)
    P1n, P1w   32,767 and 32,768 channels x 8 blocks: either side of the size at which a workgroup takes 64 channels instead of 16
    PC     65,536 channels, one in a hundred holding a frame: collect_device and deliver

Prints ONE JSON line per configuration.  The rows are AX.25 frames of 15 to 40 bytes as 1200-baud AFSK of amplitude 3000 in noise of
rms 1000 on three channels of four from a seed, noise alone on the fourth; 64 different channels, repeated.  Every line carries the
algorithmic bytes from the shapes: the pass reads one int16 row, and reads and writes the first 80 bytes of every channel's record and
its 16 bytes of ring bookkeeping once per call (and reads its 4-byte setting).  Timed with device events on one stream around enough
warmed calls to fill 0.3 s, three repeats (all three are printed, the median is used for the ratios).  Beside them, from the same run,
the yardsticks: a device-to-device copy of a buffer of the same bytes, and the time per launch of a one-element kernel (the pass is one
kernel, a collect three).  PC refills the rings before every timed collect (a call of the frame's blocks, not timed), so its figures
are single calls between two events, five of them."""
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

CONFIGS = {"P2": (65536, 1), "P2x8": (65536, 8), "P5": (512, 646), "P1n": (32767, 8), "P1w": (32768, 8), "PC": (65536, 0)}
DEFAULT = ("P2", "P2x8", "P5", "PC")
FILL_S, REPEATS = 0.3, 3
LOADED, BOOKKEEPING, SETTING, SLOT, DISTINCT = 80, 16, 4, 352, 64


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


def line_bits(payload, flags_before, flags_after=1):
    """Flags, the payload and its FCS with a 0 behind every five 1s, flags; every byte the low bit first."""
    fcs = A.packet_fcs(payload)
    body = "".join(format(v, "08b")[::-1] for v in bytes(payload) + bytes([fcs & 0xFF, fcs >> 8])).replace("11111", "111110")
    flag = "01111110"
    return [int(ch) for ch in flag * flags_before + body + flag * flags_after]


def afsk(bits, n_samples, amplitude, lead_bits=2.0):
    """float64 [n_samples]: the bits as NRZI (a 0 changes the tone) in phase-continuous 1200 / 2200 Hz AFSK at 1200 bit/s."""
    bits = np.asarray(bits, dtype=np.int64)
    tone = np.concatenate([[0], np.cumsum(1 - bits) & 1])
    k = np.floor(np.arange(n_samples) * 1200.0 / 44100.0 - lead_bits).astype(np.int64)
    live = k < bits.size
    f = np.where(tone[np.clip(k + 1, 0, bits.size)] == 0, 1200.0, 2200.0)
    return np.where(live, amplitude * np.cos(2.0 * np.pi * np.cumsum(f) / 44100.0), 0.0)


def audio(rng, n, nb):
    """int16 [n][nb][128]: noise of rms 1000 plus, on three channels of four, frame after frame of amplitude 3000."""
    x = rng.normal(0.0, 1000.0, size=(n, nb * 128))
    for c in range(n):
        if c % 4 != 3:
            bits = []
            while len(bits) * 36.75 < nb * 128:
                bits += line_bits(rng.integers(0, 256, int(rng.integers(15, 41)), dtype=np.uint8).tobytes(), 3 if not bits else int(rng.integers(0, 3)))
            x[c] += afsk(bits, nb * 128, 3000.0, lead_bits=2.0 + 0.1 * c)
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
    x = audio(np.random.default_rng(1), DISTINCT, max(nb, 60))
    warm = torch.from_numpy(x[:, :60].copy()).cuda().repeat((n + DISTINCT - 1) // DISTINCT, 1, 1)[:n].contiguous()
    d_in = torch.from_numpy(x[:, :nb].copy()).cuda().repeat((n + DISTINCT - 1) // DISTINCT, 1, 1)[:n].contiguous()
    samples = n * nb * 128
    read_bytes, write_bytes = samples * 2 + n * (LOADED + BOOKKEEPING + SETTING), n * (LOADED + BOOKKEEPING)
    t = A.PacketDecoder(n, ring=4)
    t.update_device(warm.data_ptr(), 60)                        # a frame is under way on the carried channels
    st = t.read_state()
    assert int(st["in_frame"].sum()) > n // 2
    d2d, launch = yardsticks(stream, read_bytes + write_bytes)
    ms, reps = events_ms(lambda: t.update_device(d_in.data_ptr(), nb, stream=stream.cuda_stream), stream)
    st = t.read_state()
    frames = int(st["frames"].astype(np.int64).sum())
    assert t.blocks() > 0 and int(st["bits"].min()) > 0 and (frames > 0 or nb < 200)
    rows = A.PACKET_ROWS if n >= A.PACKET_WIDE_CHANNELS else A.PACKET_NARROW_ROWS
    line = {"bench": "packet_decoder", "config": name, "n_channels": n, "n_blocks": nb, "samples": samples, "read_bytes": read_bytes,
            "write_bytes": write_bytes, "source_sha256": build.source_sha256()[:16], "timed_calls": reps, "frames_decoded": frames,
            "pass_ms": ms, "d2d_copy_of_pass_bytes_ms": d2d, "tiny_launch_ms": launch, "rows_per_workgroup": rows,
            "workgroups": (n + rows - 1) // rows, "pass_gb_per_s": round((read_bytes + write_bytes) / (med(ms) * 1e-3) / 1e9, 2),
            "msamples_per_s": round(samples / (med(ms) * 1e-3) / 1e6, 1), "us_per_block_of_a_workgroup": round(med(ms) * 1e3 / nb, 3),
            "pass_over_d2d_plus_launch": round(med(ms) / (med(d2d) + med(launch)), 3)}
    print(json.dumps(line), flush=True)
    t.close()


def run_collect(name):
    n = CONFIGS[name][0]
    stream = torch.cuda.Stream()
    bits = line_bits(bytes(range(15)), 3, 2)
    nb = -(-int((len(bits) + 4) * 36.75) // 128)
    w = np.clip(np.floor(afsk(bits, nb * 128, 3000.0) + 0.5), -32768, 32767).astype(np.int16).reshape(nb, 128)
    d_in = torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda")
    d_in[::100] = torch.from_numpy(w).cuda()
    holders = len(range(0, n, 100))
    max_frames = 4096
    d_frames = torch.zeros(max_frames * SLOT, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = A.PacketDecoder(n, ring=4)
    refill = lambda: t.update_device(d_in.data_ptr(), nb, stream=stream.cuda_stream)
    n_bytes = 2 * n * BOOKKEEPING + 2 * holders * SLOT + holders * (4 + BOOKKEEPING)
    d2d, launch = yardsticks(stream, n_bytes)
    full, host = [], []
    for _ in range(5):
        refill()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t.collect_device(d_count.data_ptr(), d_frames.data_ptr(), max_frames, stream=stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        assert int(d_count.cpu()[0]) == holders
        full.append(round(e0.elapsed_time(e1), 5))
    empty, reps = events_ms(lambda: t.collect_device(d_count.data_ptr(), d_frames.data_ptr(), max_frames, stream=stream.cuda_stream), stream)
    stream.synchronize()
    assert int(d_count.cpu()[0]) == 0
    for _ in range(5):
        refill()
        t.synchronize()
        t0 = time.perf_counter()
        got = t.deliver(max_frames)
        host.append(round((time.perf_counter() - t0) * 1e3, 5))
        assert len(got) == holders and got["channel"].tolist() == list(range(0, n, 100)) and (got["length"] == 15).all()
    line = {"bench": "packet_collect", "config": name, "n_channels": n, "ring": 4, "max_frames": max_frames, "frames": holders,
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
        (run_collect if name == "PC" else run_pass)(name)
    return 0


if __name__ == "__main__":
    sys.exit(main())
