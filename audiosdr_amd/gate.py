"""ctypes mirror of include/asdr_gate.h: the audio gate (per-receiver block energy and peak meters, a squelch with hang, the
ascending list of the channels a call delivers and the packet of their rows).  Same rules as binding.py: the work happens in
libasdr_hip.so on the GPU; there is no CPU fallback (tests/gate_ref.py is the independent numpy statement the tests compare with)."""
import ctypes as C

import numpy as np

from ._stage import RecordStage, _stride, i, ip, lg, typed_library, vp
from .binding import ALL, BLOCK, AsdrError

GATE_EXPORTS = ["asdr_gate_create", "asdr_gate_destroy", "asdr_gate_n_channels", "asdr_gate_set_squelch", "asdr_gate_get_squelch",
                "asdr_gate_energy_from_dbfs", "asdr_gate_update_device", "asdr_gate_count_device", "asdr_gate_index_device",
                "asdr_gate_deliver", "asdr_gate_read_state", "asdr_gate_write_state", "asdr_gate_clear", "asdr_gate_reset",
                "asdr_gate_blocks", "asdr_gate_synchronize"]

GATE_STATE_DTYPE = np.dtype([("energy", "<u8"), ("last_energy", "<u8"), ("peak", "<i4"), ("openings", "<u4"), ("open_blocks", "<u4"),
                             ("hang_left", "<u2"), ("open", "u1"), ("reserved", "u1")])
assert GATE_STATE_DTYPE.itemsize == 32
GATE_TILE = 256          # channels per tile of the index step's scan (ASDR_GATE_TILE)

_u64, _u64p = C.c_uint64, C.POINTER(C.c_uint64)
_API = {"create": ([i, i], vp), "destroy": ([vp], None), "n_channels": ([vp], i), "clear": ([vp], i), "reset": ([vp], i),
        "synchronize": ([vp], i), "set_squelch": ([vp, i, _u64, _u64, i], i), "get_squelch": ([vp, i, _u64p, _u64p, ip], i),
        "energy_from_dbfs": ([C.c_double], _u64), "update_device": ([vp, vp, lg, i, vp, i, vp], i), "count_device": ([vp], vp),
        "index_device": ([vp], vp), "deliver": ([vp, vp, lg, i, vp, vp, i, ip], i), "read_state": ([vp, vp], i),
        "write_state": ([vp, ip, i, vp], i), "blocks": ([vp], C.c_longlong)}


def _lib():
    return typed_library("asdr_gate_", _API)


def energy_from_dbfs(db):
    """asdr_gate_energy_from_dbfs: the block energy floor(128 * 32767^2 * 10^(db / 10) + 0.5), clamped to [0, 2^37]."""
    return int(_lib().asdr_gate_energy_from_dbfs(float(db)))


class _DeviceInts:
    """A device allocation as a __cuda_array_interface__ object, so that torch.as_tensor wraps it without a copy."""

    def __init__(self, ptr, shape, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<i4", "data": (int(ptr), False), "version": 2}


class AudioGate(RecordStage):
    """Audio meters and squelch of n_channels receivers over the chain's int16 audio rows (include/asdr_gate.h).
    device = NO_DEVICE (-1) gives the control plane and the state records only."""
    _prefix = "asdr_gate_"
    _state_dtype = GATE_STATE_DTYPE

    def __init__(self, n_channels, device=0):
        self._L = _lib()
        self._create("asdr_gate_create", self._L.asdr_gate_create(int(n_channels), int(device)))
        self.n_channels = int(n_channels)

    # settings
    def set_squelch(self, open_db=None, close_db=None, hang_blocks=0, ch=ALL, energies=None):
        """The channel's (or every channel's) squelch, from the next call.  open_db / close_db are block energies in dBFS
        (energy_from_dbfs; close_db defaults to open_db, and open_db = None to an always-open gate) -- or energies = (open_energy,
        close_energy), the uint64 thresholds themselves.  hang_blocks in 0..65535."""
        if energies is None:
            o = 0 if open_db is None else energy_from_dbfs(open_db)
            c = o if close_db is None else energy_from_dbfs(close_db)
        else:
            o, c = (int(v) for v in energies)
        if not (0 <= o < 2**64 and 0 <= c < 2**64):
            raise AsdrError("set_squelch: the energies must fit uint64")
        if not -2**31 <= int(hang_blocks) < 2**31:
            raise AsdrError("hang_blocks must be in 0..65535")
        self._chk(self._L.asdr_gate_set_squelch(self._h, int(ch), o, c, int(hang_blocks)))

    def get_squelch(self, ch=0):
        """(open_energy, close_energy, hang_blocks) of a channel."""
        o, c, h = C.c_uint64(), C.c_uint64(), C.c_int()
        self._chk(self._L.asdr_gate_get_squelch(self._h, int(ch), C.byref(o), C.byref(c), C.byref(h)))
        return int(o.value), int(c.value), int(h.value)

    # the pass
    def update_device(self, ptr, n_blocks, stride_blocks=None, rows_ptr=0, capacity_rows=0, stream=0):
        """Raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle as int).  ptr: int16 rows
        [n_channels][stride_blocks][128] (stride_blocks defaults to n_blocks); rows_ptr: room for capacity_rows packet rows
        [n_blocks][128], or 0 for no packet.  count_tensor() / index_tensor() hold the result in stream order."""
        stride = _stride(stride_blocks, n_blocks)
        self._chk(self._L.asdr_gate_update_device(self._h, C.c_void_p(ptr), stride, int(n_blocks), C.c_void_p(rows_ptr or None),
                                                  int(capacity_rows), C.c_void_p(stream or None)))

    def deliver(self, ptr, n_blocks, stride_blocks=None, capacity_rows=None, rows_out=None):
        """asdr_gate_deliver: (index int32 [count], ascending; rows int16 [min(count, capacity_rows), n_blocks, 128]).  Synchronous;
        capacity_rows defaults to n_channels.  Only the count, the index and the delivered rows cross PCIe.  rows_out: a C-contiguous
        int16 array [capacity_rows or more, n_blocks, 128] to receive the rows (pinned memory copies fastest; the returned rows are
        then a view of it) instead of a new array per call."""
        stride = _stride(stride_blocks, n_blocks)
        cap = self.n_channels if capacity_rows is None else int(capacity_rows)
        index = np.empty(self.n_channels, dtype=np.int32)
        n_open = C.c_int(0)
        if rows_out is None:
            rows = np.empty((max(0, min(cap, self.n_channels)), int(n_blocks), BLOCK), dtype=np.int16)
        else:
            rows = rows_out
            if (rows.dtype != np.int16 or not rows.flags.c_contiguous or rows.ndim != 3 or rows.shape[1:] != (int(n_blocks), BLOCK)
                    or rows.shape[0] < min(cap, self.n_channels)):
                raise AsdrError("deliver: rows_out must be C-contiguous int16 [>= capacity_rows, n_blocks, 128]")
            rows = rows[:max(0, min(cap, self.n_channels))]
        got = self._chk(self._L.asdr_gate_deliver(self._h, C.c_void_p(ptr), stride, int(n_blocks), index.ctypes.data_as(C.c_void_p),
                                                  rows.ctypes.data_as(C.c_void_p) if rows.size else None, int(rows.shape[0]),
                                                  C.byref(n_open)))
        return index[:n_open.value].copy(), rows[:got]

    def count_tensor(self):
        """The device count as a torch int32 [1] view (no copy, no synchronisation): valid in stream order after update_device."""
        import torch
        p = self._L.asdr_gate_count_device(self._h)
        if not p:
            raise AsdrError(self._L.asdr_last_error().decode())
        return torch.as_tensor(_DeviceInts(p, (1,), self), device="cuda")

    def index_tensor(self):
        """The device index as a torch int32 [n_channels] view, as count_tensor(); its first count entries are the list."""
        import torch
        p = self._L.asdr_gate_index_device(self._h)
        if not p:
            raise AsdrError(self._L.asdr_last_error().decode())
        return torch.as_tensor(_DeviceInts(p, (self.n_channels,), self), device="cuda")
