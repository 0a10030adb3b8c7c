"""The audio spectrogram on the GPU (include/asdr_spectrogram.h; audiosdr_amd/csrc/asdr_spectrogram.hip) against
tests/spectrogram_ref.py: every N, both windows and a custom one, both kinds, channel counts that leave partial workgroups, bands at
both ends, hops at both ends and odd, calls of 0, 1 and several frames, one sequence in many splittings (bit-identical), odd strides
and offsets, full-scale input, both index forms alone and behind a real gate, behind the chain and a resampler, the capture sink's
geometry, the state calls, streams, and one full-size call.

Tolerance (the rule of 3.8.4: taken from the number formats, not from the kernels), in the amplitude domain:
|X_gpu - X_ref| <= EPS_A per bin for `complex`, |sqrt p_gpu - sqrt p_ref| <= EPS_A for `power`.  EPS_A[N, window] is 8 x the largest
amplitude difference that a complex64 model of the statement (float32 window product, scipy's rfft in complex64, 1 / N) shows against
float64 on tolerance_frames(N): 16 frames of full-range uniform noise, the distribution every noise test here draws from.  A test
whose input is something else (a custom window, a square wave, the chain's audio) takes 8 x the same model's error on its own frames
(Rig.eps_of_input).  `python tests/test_gpu_spectrogram.py` prints the table; tests/test_spectrogram_ref.py recomputes it to 10 %.

The sizes are the smallest that reach each seam: up to N = 1024 a wave owns a transform and four share a workgroup (items are
row * n_frames + frame: 3 and 5 channels leave partial workgroups, 65 and 257 many workgroups with a partial last one); from
N = 2048 a workgroup owns one."""
import numpy as np
import pytest

import gate_ref as GR
import spectrogram_ref as SR

pytestmark = pytest.mark.gpu
GAP = 0x7FFF            # fills the stride gaps of the audio rows: must not be read
PATTERN = 0x5A5B5C5D    # pre-fills the output buffer (as bits): must stay wherever nothing is to be written
GUARD = 64              # floats behind the last output row

# 8 x the complex64 model's largest amplitude error on tolerance_frames(N); printed by `python tests/test_gpu_spectrogram.py`
EPS_A = {
    (128, "rect"): 4.153e-03, (128, "hann"): 2.196e-03,
    (256, "rect"): 2.929e-03, (256, "hann"): 2.266e-03,
    (512, "rect"): 2.046e-03, (512, "hann"): 1.757e-03,
    (1024, "rect"): 1.684e-03, (1024, "hann"): 9.944e-04,
    (2048, "rect"): 1.409e-03, (2048, "hann"): 8.514e-04,
    (4096, "rect"): 1.110e-03, (4096, "hann"): 6.735e-04,
    (8192, "rect"): 7.897e-04, (8192, "hann"): 5.158e-04,
}


def tolerance_frames(N):
    return np.random.default_rng(1000 + N).integers(-32768, 32768, size=(16, N)).astype(np.int16)


def compute_eps(N, window):
    w = SR.window(window, N) if isinstance(window, str) else np.asarray(window, dtype=np.float32)
    return 8.0 * SR.model_error(tolerance_frames(N), w, N)


def noise(rng, n, ns):
    return rng.integers(-32768, 32768, size=(n, ns)).astype(np.int16)


def custom_window(N):
    """A Blackman window with a sign flip in its second half: nothing symmetric, nothing a named window would hide."""
    i = np.arange(N, dtype=np.float64)
    w = 0.42 - 0.5 * np.cos(2 * np.pi * i / N) + 0.08 * np.cos(4 * np.pi * i / N)
    w[N // 2:] *= -1.25
    return w.astype(np.float32)


class Rig:
    """A spectrogram and its reference side by side; call() runs one update on both and compares everything."""

    def __init__(self, A, n, N, H, k0=0, B=None, window="hann", kind="power", eps=None):
        import torch
        self.torch, self.A, self.n = torch, A, n
        B = N // 2 + 1 - k0 if B is None else B
        self.sp = A.AudioSpectrogram(n, n_fft=N, hop=H, first_bin=k0, n_bins=B, window=window, kind=kind)
        w = self.sp.get_window()
        if isinstance(window, str):
            assert np.array_equal(w, SR.window(window, N)) and self.sp.window_kind == window
            self.eps = EPS_A[N, window] if eps is None else eps
        else:
            assert np.array_equal(w, np.asarray(window, dtype=np.float32)) and self.sp.window_kind == "custom"
            self.eps = compute_eps(N, window) if eps is None else eps
        self.ref = SR.SpectrogramRef(n, N, H, k0, B, w, kind)
        self.N, self.H, self.B, self.kind, self.ff = N, H, B, kind, self.sp.frame_floats

    def place(self, t, records):
        self.sp.set_position(t); self.sp.write_state(records)
        self.ref.T = int(t); self.ref.state = np.array(records, dtype=np.int16).reshape(self.n, self.N).copy()

    def compare(self, got, want):
        """got float32 [k][frames][ff], want the reference's rows [k][frames][B]: the amplitude-domain bound."""
        assert np.isfinite(got).all()
        if self.kind == "complex":
            g = got.astype(np.float64).reshape(got.shape[:2] + (self.B, 2))
            err = np.abs(g[..., 0] + 1j * g[..., 1] - want)
        else:
            assert (got >= 0).all()
            err = np.abs(np.sqrt(got.astype(np.float64)) - np.sqrt(want))
        worst = float(err.max()) if err.size else 0.0
        print("N %d %s: worst amplitude error %.3g of %.3g" % (self.N, self.kind, worst, self.eps))
        assert worst <= self.eps, (worst, self.eps)

    def call(self, x, extra_stride=0, offset=0, out_extra=0, index=None, count=None, capacity=None, stream=None):
        """x int16 [n][ns], laid out at `offset` samples into a buffer with stride ns + extra_stride.  index (int32 list) / count /
        capacity select the index form.  Returns the GPU's written rows, float32 [k][frames][ff]."""
        torch = self.torch
        n, ns = x.shape
        stride = ns + extra_stride
        flat = np.full(offset + n * stride + 3, GAP, dtype=np.int16)
        body = flat[offset:offset + n * stride].reshape(n, stride)
        body[:, :ns] = x
        nf = self.ref.out_frames(ns)
        assert self.sp.out_frames(ns) == nf
        ostride = nf + out_extra
        if index is None:
            rows, k, chans = n, n, np.arange(n)
        else:
            rows = capacity
            k = min(count, capacity)
            chans = np.asarray(index[:k], dtype=np.int64)
            d_index = torch.from_numpy(np.asarray(index, dtype=np.int32).copy()).cuda()
            d_count = torch.tensor([count], dtype=torch.int32, device="cuda")
        d_audio = torch.from_numpy(flat).cuda()
        words = max(rows, 1) * ostride * self.ff
        d_out = torch.full((words + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        got_n = self.sp.update_device(d_audio.data_ptr() + 2 * offset, ns, d_out.data_ptr(), ostride, stride_samples=stride,
                                      index_ptr=0 if index is None else d_index.data_ptr(), count_ptr=0 if index is None else d_count.data_ptr(),
                                      capacity_rows=0 if index is None else capacity, stream=stream.cuda_stream if stream is not None else 0)
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        want = self.ref.update(x)
        assert got_n == nf == want.shape[1]
        bits = d_out.cpu().numpy()
        out = bits[:words].reshape(max(rows, 1), ostride, self.ff)
        assert (out[:k, nf:] == PATTERN).all(), "a row is written past the returned count"
        assert (out[k:] == PATTERN).all(), "rows past min(count, capacity_rows) are written"
        assert (bits[words:] == PATTERN).all(), "the buffer is written behind the last row"
        assert np.array_equal(d_audio.cpu().numpy(), flat)
        got = np.ascontiguousarray(out[:k, :nf]).view(np.float32)
        self.compare(got, want[chans])
        assert self.sp.position() == self.ref.T and self.sp.frame_position() == self.ref.frame_position()
        return got

    def eps_of_input(self):
        """8 x the complex64 model's error on the frames of the reference's last call (whole spectrum)."""
        return 8.0 * SR.model_error(self.ref.cut.reshape(-1, self.N), self.ref.w, self.N)

    def check_state(self):
        assert np.array_equal(self.sp.read_state(), self.ref.state)

    def close(self):
        self.sp.close()


# ---- every N, window and kind; calls of 0, 1 and several frames
@pytest.mark.parametrize("kind", ["power", "complex"])
@pytest.mark.parametrize("window", ["rect", "hann", "custom"])
@pytest.mark.parametrize("N", SR.SIZES)
def test_sizes_windows_and_kinds(gpu, N, window, kind):
    """N - 1 samples complete no frame, one more completes exactly one, 3 H + 5 more several; then a call inside a hop (0 again)."""
    rng = np.random.default_rng(N + len(window) + len(kind))
    n, H = 3, N // 2
    r = Rig(gpu, n, N, H, window=custom_window(N) if window == "custom" else window, kind=kind)
    for k, (ns, frames) in enumerate(((N - 1, 0), (1, 1), (3 * H + 5, 3), (H - 6, 0), (1, 1))):
        got = r.call(noise(rng, n, ns), extra_stride=k & 1, out_extra=(k >> 1) & 1)
        assert got.shape[1] == frames
    r.check_state()
    r.close()


@pytest.mark.parametrize("N,H,k0,B,n", [(N, H, k0, B, n) for N, H, k0, B in ((128, 37, 0, 1), (1024, 511, 300, 137), (2048, 1001, 700, 137))
                                        for n in ((1, 3, 5, 65, 257) if N <= 1024 else (1, 3, 5))])
def test_channel_counts(gpu, N, H, k0, B, n):
    """Up to N = 1024 four transforms share a workgroup: 65 and 257 channels x 2 or 5 frames leave partial ones (a large transform
    has a workgroup of its own: more channels reach no seam there).  Odd hops."""
    rng = np.random.default_rng(N + n)
    r = Rig(gpu, n, N, H, k0, B, window="hann", kind="complex")
    for ns in (N + H, 5 * H + 1):
        r.call(noise(rng, n, ns), extra_stride=1, out_extra=1)
    r.check_state()
    r.close()


@pytest.mark.parametrize("hop", ["N", "N/2", "N/16", "odd"])
@pytest.mark.parametrize("band", ["dc", "whole", "nyquist", "middle"])
@pytest.mark.parametrize("N", [512, 4096])
def test_bands_and_hops(gpu, N, band, hop):
    k0, B = {"dc": (0, 1), "whole": (0, N // 2 + 1), "nyquist": (N // 2 - 6, 7), "middle": (N // 4 - 68, 137)}[band]
    H = {"N": N, "N/2": N // 2, "N/16": N // 16, "odd": N // 3 + (N // 3 + 1) % 2}[hop]
    rng = np.random.default_rng(N + k0 + H)
    r = Rig(gpu, 3, N, H, k0, B, window="rect", kind="power")
    r.call(noise(rng, 3, N + 2 * H + 1))
    r.call(noise(rng, 3, 3 * H), out_extra=2)
    r.check_state()
    r.close()


# ---- splitting
@pytest.mark.parametrize("N,H", [(128, 8), (1024, 512), (2048, 301)])
def test_one_sequence_in_many_splittings_is_bit_identical(gpu, N, H):
    """Whole, and in pieces of 1 (N = 128 only: 3 N calls), 35, H, H + 1 and N - 1 samples."""
    rng = np.random.default_rng(N)
    n, total = 3, 3 * N + 7
    x = noise(rng, n, total)
    sizes = [total, 35, H, H + 1, N - 1] + ([1] if N == 128 else [])
    rows = []
    for size in sizes:
        r = Rig(gpu, n, N, H, k0=1, B=N // 2, window="hann", kind="complex")
        parts, at = [], 0
        while at < total:
            parts.append(r.call(x[:, at:at + size]))
            at += size
        rows.append(np.concatenate(parts, axis=1))
        r.check_state()
        r.close()
    assert rows[0].shape[1] == SR.frames_at(total, N, H)
    for size, got in zip(sizes[1:], rows[1:]):
        assert np.array_equal(rows[0].view(np.uint32), got.view(np.uint32)), "pieces of %d samples change bits" % size


# ---- strides, offsets, full scale
@pytest.mark.parametrize("N", [256, 2048])
@pytest.mark.parametrize("offset,extra", [(1, 0), (1, 1), (0, 1), (3, 2)])
def test_odd_strides_and_odd_sample_offsets(gpu, N, offset, extra):
    """Rows that start on odd samples and strides that put every other row on one: the dword path and the two-short path of the
    loads, and the pair that straddles the record's end (an odd call size before it)."""
    rng = np.random.default_rng(N + offset + extra)
    r = Rig(gpu, 5, N, N // 4, window="hann", kind="complex")
    for ns in (N + 1, N // 2 + 3, N // 2):
        r.call(noise(rng, 5, ns), extra_stride=extra, offset=offset)
    r.check_state()
    r.close()


@pytest.mark.parametrize("N", [1024, 8192])
@pytest.mark.parametrize("kind", ["power", "complex"])
def test_full_scale_square_input(gpu, N, kind):
    """-32768 / +32767 with a period of 74 samples (no divisor of N), and a row of -32768 throughout (DC = -32768, power 2^30):
    nothing overflows, nothing is NaN, and the bins are within 8 x the model's error on this very input."""
    n = 2
    x = np.empty((n, 2 * N), dtype=np.int16)
    x[0] = np.where((np.arange(2 * N) // 37) % 2 == 0, 32767, -32768)
    x[1] = -32768
    probe = SR.SpectrogramRef(n, N, N // 2, 0, N // 2 + 1, SR.window("rect", N), kind)
    probe.update(x)
    eps = 8.0 * SR.model_error(probe.cut.reshape(-1, N), probe.w, N)
    r = Rig(gpu, n, N, N // 2, window="rect", kind=kind, eps=eps)
    got = r.call(x)
    assert got.shape[1] == 3 and float(np.abs(got).max()) > (1e9 if kind == "power" else 3e4)
    r.close()


def test_update_device_refusals_change_nothing(gpu):
    import torch
    r = Rig(gpu, 10, 256, 128)
    d = torch.zeros((10, 1024), dtype=torch.int16, device="cuda")
    o = torch.zeros((10, 8, 129), dtype=torch.float32, device="cuda")
    i = torch.zeros(10, dtype=torch.int32, device="cuda")
    ok = dict(ptr=d.data_ptr(), n_samples=512, out_ptr=o.data_ptr(), out_stride=8, stride_samples=1024)
    for kw, why in ((dict(ptr=d.data_ptr() + 1), "2-byte"), (dict(stride_samples=100), "stride"), (dict(n_samples=2**24 + 1, stride_samples=2**25), "n_samples"),
                    (dict(ptr=0), "null"), (dict(out_ptr=0), "null"), (dict(out_ptr=o.data_ptr() + 2), "4-byte"), (dict(out_stride=2), "output row stride"),
                    (dict(out_ptr=d.data_ptr() + 512), "overlaps"), (dict(index_ptr=i.data_ptr(), capacity_rows=3), "count"),
                    (dict(index_ptr=i.data_ptr(), count_ptr=i.data_ptr(), capacity_rows=-1), "negative")):
        with pytest.raises(gpu.AsdrError, match=why):
            r.sp.update_device(**dict(ok, **kw))
    assert r.sp.update_device(**dict(ok, n_samples=0)) == 0    # no samples: nothing happens
    assert r.sp.position() == 0
    r.check_state()
    r.close()


# ---- the index form
@pytest.mark.parametrize("N", [256, 2048])
def test_index_form_counts_and_capacity(gpu, N):
    """count 0, count = n, a random third, capacity_rows below the count, a reversed list, capacity 0: rows past
    min(count, capacity_rows) stay untouched and every channel's carry advances (each later call is held to the reference, which
    never skipped a channel)."""
    rng = np.random.default_rng(60 + N)
    n = 21
    r = Rig(gpu, n, N, N // 2, k0=3, B=40, kind="power")
    third = np.sort(rng.permutation(n)[:n // 3]).astype(np.int32)
    for index, count, capacity in (([0] * n, 0, n), (list(range(n)), n, n), (third, len(third), n), (third, len(third), 5),
                                   (list(range(n - 1, -1, -1)), n, n), (list(range(n)), n, 0)):
        r.call(noise(rng, n, N + 5), index=index, count=count, capacity=capacity, out_extra=1)
    r.check_state()
    r.close()


def test_a_channel_unwatched_for_five_calls_has_its_history(gpu):
    rng = np.random.default_rng(65)
    n, N = 6, 512
    r = Rig(gpu, n, N, N // 2, kind="complex")
    others = [c for c in range(n) if c != 4]
    for _ in range(5):
        r.call(noise(rng, n, 200), index=others, count=len(others), capacity=n)
    got = r.call(noise(rng, n, 300), index=[4], count=1, capacity=n)    # held to the rig's reference, which never stopped
    assert got.shape[:2] == (1, 2)
    r.check_state()
    r.close()


def test_behind_a_real_gate_on_one_stream(gpu):
    """Gate and spectrogram on one stream, no host step between them: the rows written are the reference rows of exactly
    index[0 .. count).  A third of the channels is loud."""
    import torch
    rng = np.random.default_rng(70)
    n, nb, N = 300, 4, 256
    audio = rng.integers(-20, 21, size=(n, nb, 128)).astype(np.int16)
    loud = np.sort(rng.permutation(n)[:n // 3])
    audio[loud] = rng.integers(-20000, 20001, size=(len(loud), nb, 128)).astype(np.int16)
    thr = 128 * 2000 * 2000
    gate, gref = gpu.AudioGate(n), GR.GateRef(n)
    gate.set_squelch(energies=(thr, thr), hang_blocks=0); gref.set_squelch(thr, thr, 0)
    assert np.array_equal(gref.update(audio)[0], loud)
    r = Rig(gpu, n, N, N // 2, k0=10, B=50, kind="power")
    want = r.ref.update(audio.reshape(n, -1))
    nf = want.shape[1]
    s = torch.cuda.Stream()
    d_audio = torch.from_numpy(audio).cuda()
    d_out = torch.full((n, nf + 1, 50), PATTERN, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gate.update_device(d_audio.data_ptr(), nb, stream=s.cuda_stream)
    got_n = r.sp.update_device(d_audio.data_ptr(), nb * 128, d_out.data_ptr(), nf + 1, index_ptr=gate.index_tensor().data_ptr(),
                               count_ptr=gate.count_tensor().data_ptr(), capacity_rows=n, stream=s.cuda_stream)
    s.synchronize()
    out = d_out.cpu().numpy()
    assert got_n == nf == 3 and int(gate.count_tensor().cpu()[0]) == len(loud)
    r.compare(np.ascontiguousarray(out[:len(loud), :nf]).view(np.float32), want[loud])
    assert (out[len(loud):] == PATTERN).all() and (out[:, nf:] == PATTERN).all()
    r.check_state()
    gate.close(); r.close()


# ---- the two paths
def test_behind_the_chain_and_a_resampler_and_on_the_capture_sink(gpu):
    """16 USB receivers, 24 blocks in two calls of 12: chain -> AudioResampler(12000) -> spectrogram on one stream, the resampler's
    rows (34 or 35 samples per block, a stride of its own) as the spectrogram's input; held to the restatement applied to the
    resampler's own rows, within 8 x the model's error on them.  Then the same audio through a capture sink's device pointer with
    stride = capacity blocks."""
    import torch
    from audiosdr_amd.synth import make_iq
    n, nb, N, H = 16, 24, 256, 64
    I, Q = make_iq(n, nb, fc=6290.0, A=np.linspace(0.02, 0.3, n), noise=0.001)
    s = torch.cuda.Stream()
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    batch = gpu.AudioSDRBatch(n)
    batch.setDemodMode(1); batch.disableNoiseBlanker()
    rs = gpu.AudioResampler(n, fs_out=12000)
    r = Rig(gpu, n, N, H, k0=20, B=60, window="hann", kind="complex")
    d_audio = torch.zeros((n, nb, 128), dtype=torch.int16, device="cuda")
    rstride = 12 * 35 + 1                                         # odd
    d_rs = torch.full((2, n, rstride), GAP, dtype=torch.int16, device="cuda")
    d_out = torch.full((2, n, 8, 60, 2), PATTERN, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    counts, frames = [], []
    for k, a in enumerate((0, 12)):
        batch.update_device_strided(dI[:, a:].data_ptr(), dQ[:, a:].data_ptr(), d_audio[:, a:].data_ptr(), 12, nb, nb, stream=s.cuda_stream)
        counts.append(rs.update_device(d_audio[:, a:].data_ptr(), 12, d_rs[k].data_ptr(), rstride, stride_blocks=nb, stream=s.cuda_stream))
        frames.append(r.sp.update_device(d_rs[k].data_ptr(), counts[k], d_out[k].data_ptr(), 8, stride_samples=rstride, stream=s.cuda_stream))
    s.synchronize()
    rows, out = d_rs.cpu().numpy(), d_out.cpu().numpy()
    assert np.abs(rows[0][:, :counts[0]]).max() > 1000
    for k in range(2):
        want = r.ref.update(rows[k][:, :counts[k]])
        assert frames[k] == want.shape[1] > 0 and (out[k][:, frames[k]:] == PATTERN).all()
        r.eps = r.eps_of_input()
        r.compare(np.ascontiguousarray(out[k][:, :frames[k]]).reshape(n, frames[k], 120).view(np.float32), want)
    r.check_state()
    rs.close(); batch.close(); r.close()

    sink = gpu.AudioSDRBatch(n)                                   # the capture sink's rows, stride = capacity blocks
    sink.setDemodMode(1); sink.disableNoiseBlanker()
    sink.capture_open(nb + 5)
    r = Rig(gpu, n, 1024, 512, k0=0, B=137, window="hann", kind="power")
    d_one = torch.full((n, 6, 137), PATTERN, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sink.capture_update_device(dI.data_ptr(), dQ.data_ptr(), nb, stream=s.cuda_stream)
    got_n = r.sp.update_device(sink.capture_device_ptr(), nb * 128, d_one.data_ptr(), 6, stride_samples=sink.capture_capacity * 128, stream=s.cuda_stream)
    s.synchronize()
    want = r.ref.update(d_audio.cpu().numpy().reshape(n, -1))     # a fresh chain with the same settings: the sink's rows are d_audio's
    out = d_one.cpu().numpy()
    assert got_n == want.shape[1] == 5 and (out[:, 5:] == PATTERN).all()
    r.eps = r.eps_of_input()
    r.compare(np.ascontiguousarray(out[:, :5]).view(np.float32), want)
    r.close(); sink.capture_close(); sink.close()


# ---- state
@pytest.mark.parametrize("N", [512, 4096])
def test_records_move_a_channel_between_spectrograms_mid_stream(gpu, N):
    """Channel 2's record, read in the middle of a frame, written into channel 4 of a second object placed at the same T: its next
    frames are bit-identical to the uninterrupted object's.  Then a refused write, reset, and set_position."""
    rng = np.random.default_rng(80 + N)
    n, H = 5, N // 4
    a = Rig(gpu, n, N, H, k0=5, B=99, kind="complex")
    first, rest = noise(rng, n, 2 * N + 77), noise(rng, n, N + 3 * H)
    a.call(first[:, :N + 10]); a.call(first[:, N + 10:])
    rec = a.sp.read_state()
    assert np.array_equal(rec, first[:, -N:])
    b = Rig(gpu, n + 1, N, H, k0=5, B=99, kind="complex")
    b.call(noise(rng, n + 1, 123))
    moved = b.sp.read_state()
    moved[4] = rec[2]
    b.sp.set_position(a.sp.position()); b.sp.write_state(rec[2], channels=[4])
    b.ref.T, b.ref.state = a.sp.position(), moved
    rest_b = noise(rng, n + 1, rest.shape[1])
    rest_b[4] = rest[2]
    got_a, got_b = a.call(rest), b.call(rest_b)
    assert got_a.shape[1] == got_b.shape[1] > 0 and np.array_equal(got_a[2].view(np.uint32), got_b[4].view(np.uint32))
    with pytest.raises(gpu.AsdrError, match="bad channel"):
        b.sp.write_state(rec[:2], channels=[0, n + 1])
    b.check_state()
    b.sp.reset(); b.ref.reset()
    assert b.sp.position() == 0 and b.sp.frame_position() == 0 and not b.sp.read_state().any()
    b.call(noise(rng, n + 1, N + 1))
    b.place(2**40 + 12345, noise(rng, n + 1, N))                  # frames continue from a position past 2^40
    b.call(noise(rng, n + 1, N))
    b.check_state()
    a.close(); b.close()


# ---- streams
def test_two_streams_without_host_synchronisation(gpu):
    """Two consecutive calls on different streams with no host synchronisation between them equal the same calls on one stream:
    the second call's frames begin in the first call's carry, so it must have waited on the device."""
    import torch
    rng = np.random.default_rng(90)
    n, N, H, ns = 2000, 256, 128, 300
    x = noise(rng, n, 2 * ns)
    d_x = torch.from_numpy(x).cuda()
    results = []
    for streams in ((torch.cuda.Stream(), torch.cuda.Stream()), (torch.cuda.Stream(),) * 2):
        r = Rig(gpu, n, N, H, k0=0, B=16, kind="power")
        outs = [torch.full((n, 3, 16), PATTERN, dtype=torch.int32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        counts = [r.sp.update_device(d_x[:, k * ns:].data_ptr(), ns, outs[k].data_ptr(), 3, stride_samples=2 * ns, stream=streams[k].cuda_stream)
                  for k in range(2)]
        r.sp.synchronize()
        torch.cuda.synchronize()
        results.append([o.cpu().numpy() for o in outs])
        for k in range(2):
            want = r.ref.update(x[:, k * ns:(k + 1) * ns])
            assert counts[k] == want.shape[1] == (1, 2)[k]
            r.compare(np.ascontiguousarray(results[-1][k][:, :counts[k]]).view(np.float32), want)
        r.check_state()
        r.close()
    assert all(np.array_equal(p, q) for p, q in zip(*results))


# ---- full size
def test_one_full_size_call(gpu):
    """512 rows x 120 000 samples at N = 8192, H = 4096, the WSPR band's 137 bins; rows 0, 1, 255 and 511 compared, and the frame
    behind every row's last untouched."""
    import torch
    n, ns, N, H, k0, B = 512, 120000, 8192, 4096, 956, 137
    chans = np.array([0, 1, 255, 511])
    gen = torch.Generator(device="cuda").manual_seed(5)
    d_x = torch.randint(-32768, 32768, (n, ns), generator=gen, device="cuda", dtype=torch.int32).to(torch.int16)
    sp = gpu.AudioSpectrogram(n, n_fft=N, hop=H, first_bin=k0, n_bins=B, window="hann", kind="power")
    ref = SR.SpectrogramRef(len(chans), N, H, k0, B, sp.get_window(), "power")
    nf = sp.out_frames(ns)
    d_out = torch.full((n, nf + 1, B), PATTERN, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert sp.update_device(d_x.data_ptr(), ns, d_out.data_ptr(), nf + 1) == nf == 28
    torch.cuda.synchronize()
    want = ref.update(d_x[torch.from_numpy(chans).cuda()].cpu().numpy())
    got = np.ascontiguousarray(d_out[torch.from_numpy(chans).cuda()].cpu().numpy()[:, :nf]).view(np.float32)
    err = float(np.abs(np.sqrt(got.astype(np.float64)) - np.sqrt(want)).max())
    print("worst amplitude error %.3g of %.3g" % (err, EPS_A[N, "hann"]))
    assert np.isfinite(got).all() and err <= EPS_A[N, "hann"]
    assert bool((d_out[:, nf] == PATTERN).all()) and not bool((d_out[:, :nf] == PATTERN).any())
    assert np.array_equal(sp.read_state()[chans], ref.state)
    sp.close()


if __name__ == "__main__":
    print("EPS_A = {")
    for N in SR.SIZES:
        print("    " + " ".join('(%d, "%s"): %.3e,' % (N, w, compute_eps(N, w)) for w in ("rect", "hann")))
    print("}")
