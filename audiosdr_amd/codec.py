"""ctypes mirror of include/asdr_codec.h: the audio codec (delivered int16 audio rows as G.711 mu-law / A-law bytes or IMA ADPCM
packet rows, for every channel or for the channels a gate delivered, and their delivery to the host).  Same rules as binding.py: the
encoders run in libasdr_hip.so on the GPU; there is no CPU fallback (tests/codec_ref.py is the independent numpy statement the tests
compare with).  Only the decoder, a listener's side, is host code."""
import ctypes as C

import numpy as np

from ._stage import RecordStage, _stride, i, ip, lg, typed_library, vp
from .binding import AsdrError

CODEC_EXPORTS = ["asdr_codec_create", "asdr_codec_destroy", "asdr_codec_n_channels", "asdr_codec_kind", "asdr_codec_row_bytes",
                 "asdr_codec_encode_device", "asdr_codec_deliver", "asdr_codec_decode", "asdr_codec_read_state",
                 "asdr_codec_write_state", "asdr_codec_reset", "asdr_codec_synchronize"]

CODEC_STATE_DTYPE = np.dtype([("predictor", "<i2"), ("step_index", "u1"), ("reserved", "u1")])
assert CODEC_STATE_DTYPE.itemsize == 4
CODEC_KINDS = {"ulaw": 1, "alaw": 2, "adpcm": 3}     # ASDR_CODEC_ULAW, ASDR_CODEC_ALAW, ASDR_CODEC_ADPCM
CODEC_MAX_SAMPLES = 8388480                          # per row and call (ASDR_CODEC_MAX_SAMPLES)

_API = {"create": ([i, i, i], vp), "destroy": ([vp], None), "n_channels": ([vp], i), "kind": ([vp], i), "reset": ([vp], i),
        "synchronize": ([vp], i), "row_bytes": ([i, lg], lg), "encode_device": ([vp, vp, lg, lg, i, vp, lg, vp, vp, i, vp], lg),
        "deliver": ([vp, vp, lg, lg, i, vp, vp, vp, vp, i, vp], lg), "decode": ([i, vp, lg, vp], i), "read_state": ([vp, vp], i),
        "write_state": ([vp, ip, i, vp], i)}


def _lib():
    return typed_library("asdr_codec_", _API)


def _kind(kind):
    """A kind's name ("ulaw", "alaw", "adpcm") or number as the header's number; an unknown name raises, an unknown number is the
    library's to refuse."""
    if isinstance(kind, str):
        if kind not in CODEC_KINDS:
            raise AsdrError("codec: kind must be one of %s" % ", ".join(sorted(CODEC_KINDS)))
        return CODEC_KINDS[kind]
    return int(kind)


def _fits_long(*values):
    if not all(-2**63 <= int(v) < 2**63 for v in values):
        raise AsdrError("codec: argument out of range")


class AudioCodec(RecordStage):
    """Encoder of n_channels receivers' int16 audio rows into packet rows of one kind (include/asdr_codec.h).
    device = NO_DEVICE (-1) gives the control plane and the state records only."""
    _prefix = "asdr_codec_"
    _state_dtype = CODEC_STATE_DTYPE

    def __init__(self, n_channels, kind="adpcm", device=0):
        self._L = _lib()
        self._create("asdr_codec_create", self._L.asdr_codec_create(int(n_channels), _kind(kind), int(device)))
        self.n_channels = int(n_channels)
        self.kind = int(self._L.asdr_codec_kind(self._h))

    def row_bytes(self, n_samples):
        """Bytes of a packet row of n_samples samples: n for the G.711 kinds, 4 + ceil(n / 2) for ADPCM.  A row in a buffer is
        followed by zeros up to the next multiple of 4."""
        return codec_row_bytes(self.kind, n_samples)

    # the pass
    def encode_device(self, ptr, n_samples, out_ptr, out_stride_bytes, row_stride_samples=None, rows_compact=False, index_ptr=0, count_ptr=0,
                      capacity_rows=0, stream=0):
        """Raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle as int).  ptr: int16 rows [..][row_stride_samples]
        (defaults to n_samples); out_ptr: uint8 rows [..][out_stride_bytes].  With index_ptr / count_ptr (device int32 [..] and int32,
        e.g. a gate's index_tensor().data_ptr() / count_tensor().data_ptr()) output row i is channel index[i] for
        i < min(count, capacity_rows), read from input row index[i], or from input row i with rows_compact (a resampler's rows
        behind the same index); otherwise row c is channel c.  Returns the row's byte count."""
        stride = _stride(row_stride_samples, n_samples)
        _fits_long(stride, n_samples, out_stride_bytes)
        return int(self._chk(self._L.asdr_codec_encode_device(self._h, C.c_void_p(ptr or None), stride, int(n_samples), int(bool(rows_compact)),
                                                              C.c_void_p(out_ptr or None), int(out_stride_bytes), C.c_void_p(index_ptr or None),
                                                              C.c_void_p(count_ptr or None), int(capacity_rows), C.c_void_p(stream or None))))

    def deliver(self, ptr, n_samples, row_stride_samples=None, rows_compact=False, index_ptr=0, count_ptr=0, capacity_rows=None, stream=0,
                rows_out=None, want_index=True):
        """asdr_codec_deliver: (count, index int32 [k] or None, rows uint8 [k, row_bytes rounded up to 4]) with
        k = min(count, capacity_rows).  The pass is enqueued on `stream`, which is synchronized on return; only the count, k index
        entries and k packet rows cross PCIe.  capacity_rows defaults to n_channels.  rows_out: a C-contiguous uint8 array
        [capacity_rows or more, row_bytes rounded up to 4] to receive the rows (pinned memory copies fastest; the returned rows are
        then a view of it) instead of a new array per call.  want_index = False passes no host index."""
        stride = _stride(row_stride_samples, n_samples)
        _fits_long(stride, n_samples)
        cap = self.n_channels if capacity_rows is None else int(capacity_rows)
        room = self.n_channels if not index_ptr else max(0, min(cap, self.n_channels))
        padded = (max(self.row_bytes(n_samples), 0) + 3) & ~3
        if rows_out is None:
            rows = np.empty((room, padded), dtype=np.uint8)
        else:
            rows = rows_out
            if rows.dtype != np.uint8 or not rows.flags.c_contiguous or rows.ndim != 2 or rows.shape[1] != padded or rows.shape[0] < room:
                raise AsdrError("deliver: rows_out must be C-contiguous uint8 [>= capacity_rows, row_bytes rounded up to 4]")
        index = np.empty(room, dtype=np.int32) if want_index else None
        count = int(self._chk(self._L.asdr_codec_deliver(self._h, C.c_void_p(ptr or None), stride, int(n_samples), int(bool(rows_compact)),
                                                         index.ctypes.data_as(C.c_void_p) if want_index and room else None,
                                                         rows.ctypes.data_as(C.c_void_p) if rows.size else None, C.c_void_p(index_ptr or None),
                                                         C.c_void_p(count_ptr or None), cap, C.c_void_p(stream or None))))
        k = min(count, room)
        return count, (index[:k] if want_index else None), rows[:k]

    @staticmethod
    def decode(kind, rows, n_samples):
        """asdr_codec_decode over packet rows uint8 [k, >= row_bytes] (or one row): int16 [k, n_samples].  Host code."""
        return codec_decode(kind, rows, n_samples)


def codec_row_bytes(kind, n_samples):
    """asdr_codec_row_bytes: a pure function of the kind and the sample count."""
    L = _lib()
    _fits_long(n_samples)
    rc = int(L.asdr_codec_row_bytes(_kind(kind), int(n_samples)))
    if rc < 0:
        raise AsdrError(L.asdr_last_error().decode())
    return rc


def codec_decode(kind, rows, n_samples):
    """asdr_codec_decode over packet rows uint8 [k, >= row_bytes] (or one row [>= row_bytes]): int16 [k, n_samples] (or [n_samples])."""
    L = _lib()
    k = _kind(kind)
    need = codec_row_bytes(k, n_samples)
    r = np.ascontiguousarray(rows, dtype=np.uint8)
    one = r.ndim == 1
    r = r.reshape(1, -1) if one else r
    if r.ndim != 2 or r.shape[1] < need:
        raise AsdrError("decode: the rows must be uint8 [k, >= %d]" % need)
    out = np.zeros((r.shape[0], int(n_samples)), dtype=np.int16)
    for j in range(r.shape[0]):
        if L.asdr_codec_decode(k, r[j].ctypes.data_as(C.c_void_p), int(n_samples), out[j].ctypes.data_as(C.c_void_p)) != 0:
            raise AsdrError(L.asdr_last_error().decode())
    return out[0] if one else out
