"""Independent numpy restatement of include/asdr_spectrogram.h in float64: the frame arithmetic F(T), the window, the frames of a band,
the state record, and a complex64 model of the statement whose distance from float64 sets the GPU tests' tolerance.
Nothing here shares code with the library."""
import numpy as np

SIZES = (128, 256, 512, 1024, 2048, 4096, 8192)
MAX_OVERLAP = 16
MAX_SAMPLES = 1 << 24
MAX_POSITION = 1 << 50


def accepted(N, H, k0, B):
    return N in SIZES and N <= MAX_OVERLAP * H and 1 <= H <= N and k0 >= 0 and B >= 1 and k0 + B <= N // 2 + 1


def frames_at(T, N, H):
    """F(T): the frames that lie wholly in the first T samples."""
    return 0 if T < N else (T - N) // H + 1


def window(name, N):
    """float32 [N]: 'rect' or 'hann' (formed in float64, rounded to float32)."""
    if name == "rect":
        return np.ones(N, dtype=np.float32)
    assert name == "hann"
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)


def frames64(x, w, N, k0, B):
    """float64 statement of frames already cut: x [..., N] (any integer type), w float32 [N] -> complex128 [..., B]."""
    v = np.asarray(x, dtype=np.float64) * np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.fft.rfft(v, axis=-1)[..., k0:k0 + B] / N


def frames32(x, w, N, k0, B):
    """The complex64 model: a float32 window product, scipy's rfft in complex64, and the 1 / N."""
    import scipy.fft
    v = np.asarray(x, dtype=np.float32) * np.asarray(w, dtype=np.float32)
    X = scipy.fft.rfft(v, axis=-1)
    assert X.dtype == np.complex64
    return (X[..., k0:k0 + B] * np.float32(1.0 / N)).astype(np.complex64)


def model_error(x, w, N, k0=0, B=None):
    """The largest amplitude difference between the complex64 model and float64 over the frames x [..., N]."""
    B = N // 2 + 1 - k0 if B is None else B
    return float(np.abs(frames32(x, w, N, k0, B).astype(np.complex128) - frames64(x, w, N, k0, B)).max())


class SpectrogramRef:
    """The bank: n channels in lockstep.  update(x) takes int16 [n][n_samples] and returns the call's frames, complex128
    [n][frames][B] ('complex') or float64 [n][frames][B] ('power')."""

    def __init__(self, n, N, H, k0, B, w, kind="power"):
        assert accepted(N, H, k0, B) and kind in ("power", "complex")
        self.n, self.N, self.H, self.k0, self.B, self.kind = n, N, H, k0, B, kind
        self.w = np.asarray(w, dtype=np.float32).copy()
        assert self.w.shape == (N,) and np.isfinite(self.w).all()
        self.reset()

    def reset(self):
        self.T = 0
        self.state = np.zeros((self.n, self.N), dtype=np.int16)

    def frame_position(self):
        return frames_at(self.T, self.N, self.H)

    def out_frames(self, n_samples):
        return frames_at(self.T + n_samples, self.N, self.H) - frames_at(self.T, self.N, self.H)

    def update(self, x):
        x = np.asarray(x, dtype=np.int16).reshape(self.n, -1)
        ns = x.shape[1]
        f0, f1 = frames_at(self.T, self.N, self.H), frames_at(self.T + ns, self.N, self.H)
        seq = np.concatenate([self.state, x], axis=1)           # seq[:, N + s] is sample s of the call
        starts = [self.N + f * self.H - self.T for f in range(f0, f1)]
        assert all(0 < s and s + self.N <= seq.shape[1] for s in starts)
        cut = np.stack([seq[:, s:s + self.N] for s in starts], axis=1) if starts else np.zeros((self.n, 0, self.N), dtype=np.int16)
        self.cut = cut                                          # the call's frames as cut: what a test's tolerance is taken on
        X = frames64(cut, self.w, self.N, self.k0, self.B)
        self.state = seq[:, -self.N:].copy()
        self.T += ns
        return X if self.kind == "complex" else X.real ** 2 + X.imag ** 2
