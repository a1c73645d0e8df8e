"""ctypes binding of the qfec C-ABI (include/qfec.h) — test / bench plumbing.

The product is the native library ``libquic_amd/libqfec.so`` (HIP kernels +
C-ABI + the C++ QuicFecGroup host mirror).  This module only forwards calls;
it never computes FEC bytes itself and has no CPU fallback: if the library or
the GPU is missing, every call raises.

Buffers may be torch tensors (device or pinned host) or numpy arrays (host);
the caller picks ``host=True`` for host pointers (QFEC_PTR_HOST), or
``mapped=True`` for payloads in pinned host memory the kernels read in place
(QFEC_PTR_MAPPED; torch ``pin_memory()`` tensors or ``HostBuffer``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libqfec.so")

QFEC_OK = 0
QFEC_ERR_INTERNAL = -1
QFEC_ERR_INVALID_FEC_DATA = -5
QFEC_PTR_DEVICE = 0
QFEC_PTR_HOST = 1
QFEC_CACHED = 2
QFEC_PTR_MAPPED = 4
QFEC_ONE_PASS = 8
QFEC_ASYNC = 16
QFEC_SCRATCH_OUTPUT = 32
QFEC_SMALL_GROUPS = 64
QFEC_PENDING = 1
GROUP_COMPLETE = 0
GROUP_REVIVED = 1
GROUP_UNREVIVABLE = 2
QFEC_PKT_ADMITTED = 0
QFEC_PKT_FAILED = 1
QFEC_PKT_DUPLICATE = 2
QFEC_PKT_INVALID = 3
QFEC_NO_SLOT = 0xFFFFFFFF
QFEC_NO_KEY = 0xFFFFFFFFFFFFFFFF
QFEC_HDR_FAILED = 0x80
QFEC_HDR_NO_FLAGS = 0x81
QFEC_HDR_ILLEGAL_FLAGS = 0x82
QFEC_HDR_NO_OFFSET = 0x83
QFEC_HDR_BAD_OFFSET = 0x84
QFEC_HDR_RANGE = 0x85
QFEC_HDR_EMPTY = 0x86
QFEC_RCV_NOT_ACCEPTED = 0
QFEC_RCV_RANGE = 1
QFEC_RCV_STALE = 2
QFEC_RCV_OVERFLOW = 3
QFEC_RCV_DUPLICATE = 4
QFEC_RCV_RECORDED = 5
QFEC_CELL_RECEIVED = 1
QFEC_CELL_ENTROPY = 2
QFEC_CELL_REVIVED = 4
QFEC_FRM_OK = 0
QFEC_FRM_SKIPPED = 1
QFEC_FRM_NO_FRAMES = 2
QFEC_FRM_ILLEGAL_TYPE = 3
QFEC_FRM_STREAM = 4
QFEC_FRM_ACK = 5
QFEC_FRM_RST = 6
QFEC_FRM_CLOSE = 7
QFEC_FRM_GOAWAY = 8
QFEC_FRM_WINDOW_UPDATE = 9
QFEC_FRM_BLOCKED = 10
QFEC_FRM_STOP_WAITING = 11
QFEC_FRM_PATH_CLOSE = 12
QFEC_FRM_BAD_LEAST = 13
QFEC_FRM_TOO_MANY = 14
QFEC_FRM_PN_LEN = 15
QFEC_FRM_RANGE = 16
QFEC_FRAME_STREAM = 0x80
QFEC_FRAME_ACK = 0x40
QFEC_ACKW_WRITTEN = 0
QFEC_ACKW_CUT = 1
QFEC_ACKW_NO_ROOM = 2
QFEC_ACKW_RANGE = 3
MAX_PACKET_SIZE = 1452
DEFAULT_MAX_PACKET_SIZE = 1350
MAX_GROUP_PACKETS = 255

# Every symbol include/qfec.h declares: (name, restype, argtypes)
_vp, _u8p = C.c_void_p, C.c_void_p
SIGNATURES = [
    ("qfec_abi_version", C.c_int, []),
    ("qfec_create", C.c_void_p, [C.c_int]),
    ("qfec_destroy", None, [C.c_void_p]),
    ("qfec_set_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("qfec_get_stream", C.c_void_p, [C.c_void_p]),
    ("qfec_own_stream", C.c_void_p, [C.c_void_p]),
    ("qfec_sync", C.c_int, [C.c_void_p]),
    ("qfec_strerror", C.c_char_p, [C.c_int]),
    ("qfec_last_error", C.c_char_p, [C.c_void_p]),
    ("qfec_host_alloc", C.c_void_p, [C.c_size_t]),
    ("qfec_host_free", None, [C.c_void_p]),
    ("qfec_host_register", C.c_int, [C.c_void_p, C.c_size_t]),
    ("qfec_host_unregister", C.c_int, [C.c_void_p]),
    ("qfec_encode_batch", C.c_int,
     [_vp, _u8p, C.c_uint32, C.c_uint32, C.c_uint64, _u8p, C.c_uint32]),
    ("qfec_recover_batch", C.c_int,
     [_vp, _u8p, _u8p, _u8p, C.c_uint32, C.c_uint32, C.c_uint64, _u8p, C.c_uint32]),
    ("qfec_encode_batch_strided", C.c_int,
     [_vp, _u8p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, _u8p, C.c_uint64,
      C.c_uint32]),
    ("qfec_recover_batch_strided", C.c_int,
     [_vp, _u8p, _u8p, _u8p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
      C.c_uint64, _u8p, C.c_uint64, C.c_uint32]),
    ("qfec_recover_inslot_batch", C.c_int,
     [_vp, _u8p, _u8p, C.c_uint32, C.c_uint32, C.c_uint64, _u8p, C.c_uint32]),
    ("qfec_recover_inslot_batch_strided", C.c_int,
     [_vp, _u8p, _u8p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, _u8p,
      C.c_uint64, C.c_uint32]),
    ("qfec_revive_batch", C.c_int,
     [_vp, _u8p, _u8p, _u8p, C.c_uint32, C.c_uint32, C.c_uint64, _u8p, _u8p, _u8p, _vp, _vp,
      C.c_uint32]),
    ("qfec_revive_batch_strided", C.c_int,
     [_vp, _u8p, _u8p, _u8p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
      C.c_uint64, C.c_uint64, _u8p, C.c_uint64, _u8p, _u8p, _vp, _vp, C.c_uint32]),
    ("qfec_encode_ragged", C.c_int,
     [_vp, _u8p, _vp, _vp, _vp, C.c_uint64, _u8p, _vp, _vp, C.c_uint32]),
    ("qfec_revive_ragged", C.c_int,
     [_vp, _u8p, _vp, _vp, _vp, C.c_uint64, _u8p, _vp, _vp, _u8p, C.c_uint64, _u8p, _vp, _u8p,
      _u8p, _vp, _vp, C.c_uint32]),
    ("qfec_recover_ragged", C.c_int,
     [_vp, _u8p, _vp, _vp, _vp, C.c_uint64, _u8p, _vp, _vp, _u8p, _u8p, _vp, C.c_uint32]),
    ("qfec_accumulate_ragged", C.c_int,
     [_vp, _u8p, _vp, _vp, _vp, C.c_uint64, _u8p, C.c_uint64, _vp, _vp, C.c_uint64, C.c_uint32]),
    ("qfec_emit_accumulated", C.c_int,
     [_vp, _u8p, C.c_uint64, _vp, _vp, C.c_uint64, C.c_uint64, _u8p, _vp, _vp, C.c_int,
      C.c_uint32]),
    ("qfec_revive_accumulated", C.c_int,
     [_vp, _u8p, C.c_uint64, _vp, _vp, C.c_uint64, _u8p, _u8p, C.c_uint64, C.c_uint64, _u8p, _vp,
      _vp, _u8p, _u8p, _vp, _vp, C.c_uint32, C.c_uint32]),
    ("qfec_admit_ragged", C.c_int,
     [_vp, _vp, _vp, _u8p, _u8p, _vp, C.c_uint64, _vp, C.c_uint64, _u8p, _u8p, C.c_uint64, _vp,
      C.c_uint64, _vp, _vp, _vp, _u8p, _vp, C.c_uint32]),
    ("qfec_revive_tracked", C.c_int,
     [_vp, _u8p, C.c_uint64, _vp, _u8p, C.c_uint64, _u8p, _vp, C.c_uint64, C.c_uint64, _u8p, _vp,
      _vp, _u8p, _u8p, _vp, _vp, C.c_uint32, C.c_uint32]),
    ("qfec_bin_arrivals", C.c_int,
     [_vp, _vp, _vp, _vp, _u8p, _u8p, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _u8p, _u8p, _vp, _vp,
      C.c_uint32]),
    ("qfec_assign_slots", C.c_int,
     [_vp, _vp, _u8p, C.c_uint64, _vp, _u8p, _vp, C.c_uint64, _vp, _vp, C.c_uint32]),
    ("qfec_retire_groups", C.c_int,
     [_vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp,
      _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint32]),
    ("qfec_parse_opened", C.c_int,
     [_vp, _u8p, _vp, _vp, _vp, _vp, _u8p, C.c_uint64, C.c_int, C.c_uint32, _vp, _u8p, _vp, _vp,
      _u8p, _u8p, _vp, C.c_uint32]),
    ("qfec_write_private_headers", C.c_int,
     [_vp, _u8p, _vp, _u8p, _u8p, C.c_uint64, C.c_int, _vp, _vp, C.c_uint32]),
    ("qfec_scan_frames", C.c_int,
     [_vp, _u8p, _vp, _vp, _vp, _vp, _u8p, _u8p, C.c_uint64, C.c_int, C.c_uint32, _u8p, _vp, _vp,
      _u8p, _u8p, _vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _u8p, _vp, C.c_uint64, _vp,
      C.c_uint32]),
    ("qfec_record_received", C.c_int,
     [_vp, _vp, _vp, _u8p, _u8p, C.c_uint64, _u8p, _u8p, _vp, _vp, C.c_uint64, C.c_uint64,
      C.c_uint32, _vp, _vp, _u8p, C.c_uint64, _u8p, _vp, _vp, _u8p, C.c_uint64, C.c_uint32, _u8p,
      _vp, C.c_uint32]),
    ("qfec_build_acks", C.c_int,
     [_vp, _vp, C.c_uint64, _u8p, _vp, _vp, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
      _vp, _u8p, _u8p, _vp, _vp, _vp, _vp, _vp, C.c_uint32]),
    ("qfec_write_ack_frames", C.c_int,
     [_vp, _vp, C.c_uint64, _vp, _u8p, _u8p, _vp, _vp, _vp, _vp, _vp, _vp, _u8p, C.c_uint64,
      C.c_uint32, _u8p, _vp, _vp, C.c_uint32, _vp, _vp, _u8p, _u8p, _vp, C.c_uint32]),
    ("qfec_xor_into", C.c_int, [_vp, _u8p, C.c_uint64, _u8p, C.c_uint32]),
    ("qfec_wire_write_private_header", C.c_size_t, [_vp, _u8p, C.c_size_t]),
    ("qfec_wire_parse_private_header", C.c_size_t,
     [_u8p, C.c_size_t, C.c_int, C.c_uint64, _vp]),
    ("qfec_wire_write_revived", C.c_size_t, [_vp, C.c_size_t, C.c_size_t, _u8p, C.c_size_t]),
    ("qfec_wire_parse_revived", C.c_size_t, [_u8p, C.c_size_t, C.c_size_t, _vp, _vp]),
    ("qfec_wire_fec_packet_body", C.c_size_t,
     [C.c_uint64, C.c_uint64, C.c_int, _u8p, C.c_size_t, _u8p, C.c_size_t]),
    ("qfec_wire_write_ack_frame", C.c_size_t,
     [C.c_uint64, C.c_uint8, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_uint64, C.c_int, _vp, _vp,
      _u8p, C.c_size_t, _vp, _vp, _vp]),
    ("qfec_wire_parse_ack_frame", C.c_size_t,
     [_u8p, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("qfec_wire_scan_frames", C.c_size_t,
     [_u8p, C.c_size_t, C.c_int, C.c_uint64, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp,
      _vp, _vp, _vp]),
    ("qfec_null_encrypt_batch", C.c_int,
     [_vp, _u8p, _vp, _vp, _vp, _vp, C.c_uint64, _u8p, _vp, C.c_uint32]),
    ("qfec_null_decrypt_batch", C.c_int,
     [_vp, _u8p, _vp, _vp, _vp, _vp, C.c_uint64, _u8p, _vp, _u8p, C.c_uint32]),
    ("qfec_chacha20poly1305_seal_batch", C.c_int,
     [_vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp, _vp, _vp, _vp, C.c_uint64, _u8p, _vp, C.c_uint32]),
    ("qfec_chacha20poly1305_open_batch", C.c_int,
     [_vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp, _vp, _vp, _vp, C.c_uint64, _u8p, _vp, _u8p,
      C.c_uint32]),
    ("qfec_aes128gcm_seal_batch", C.c_int,
     [_vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp, _vp, _vp, _vp, C.c_uint64, _u8p, _vp, C.c_uint32]),
    ("qfec_aes128gcm_open_batch", C.c_int,
     [_vp, _vp, _vp, _vp, _vp, _vp, _u8p, _vp, _vp, _vp, _vp, C.c_uint64, _u8p, _vp, _u8p,
      C.c_uint32]),
    ("qfec_entropy_cumulative_batch", C.c_int,
     [_vp, _u8p, _vp, _u8p, C.c_uint64, C.c_uint64, _u8p, C.c_uint32]),
    ("qfec_entropy_validate_batch", C.c_int,
     [_vp, _u8p, _vp, _vp, _u8p, C.c_uint64, _vp, _vp, _u8p, _vp, _vp, _vp, C.c_uint64, _u8p,
      C.c_uint32]),
    ("qfec_stream_probe", C.c_int, [_vp, _u8p, C.c_uint64, _u8p, C.c_int]),
    ("qfec_phase_abandons", C.c_int, [_vp, _vp]),
    ("qfec_phase_backoff", C.c_int, [_vp]),
    ("qfec_debug_phase", C.c_int, [_vp, C.c_uint32, C.c_int]),
    ("qfec_debug_phase_min", C.c_int, [_vp, C.c_uint32]),
    ("qfec_debug_phase_regsteps", C.c_int, [_vp, C.c_int]),
    ("qfec_debug_phase_rtbatch", C.c_int, [_vp, C.c_uint32]),
    ("qfec_debug_phase_reserve", C.c_int, [_vp, C.c_uint32]),
    ("qfec_debug_other_service_cus", C.c_uint32, [_vp, C.POINTER(C.c_uint32)]),
    ("qfec_last_fixed_phased", C.c_int, [_vp]),
    ("qfec_debug_last_phase_grid", C.c_uint32, [_vp]),
    ("qfec_debug_fail_launches", C.c_int, [_vp, C.c_int]),
    ("qfec_debug_assign_probe", C.c_int, [_vp, C.c_int]),
    ("qfec_debug_service", C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64)]),
    ("qfec_debug_service_stamps", C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64)]),
    ("qfec_debug_service_trace", C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    ("qfec_debug_service_feed", C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64)]),
    ("qfec_debug_service_resident", C.c_uint64, [_vp, C.c_uint64]),
    ("qfec_debug_service_idle", C.c_uint64, [_vp, C.c_uint64]),
    ("qfec_debug_service_hold", C.c_int, [_vp, C.c_int]),
    ("qfec_complete", C.c_int, [_vp, C.c_int]),
    ("qfec_async_ticket", C.c_uint64, [_vp]),
    ("qfec_complete_ticket", C.c_int, [_vp, C.c_uint64, C.c_int]),
    ("qfec_service_warm", C.c_int, [_vp]),
    ("qfec_synth_fixed", C.c_int,
     [_vp, _u8p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
      C.c_uint64]),
    ("qfec_synth_ragged", C.c_int,
     [_vp, _u8p, _vp, _vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64]),
]

_lib = None


class QfecError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{msg} (code {code})")
        self.code = code


class InvalidFecData(QfecError):
    pass


def load(path: str = LIB_PATH):
    """Load libqfec.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (the HIP path has no CPU fallback)")
        lib = C.CDLL(path)
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _fl(host=False, mapped=False, cached=False, one_pass=False):
    return ((QFEC_PTR_HOST if host else 0) | (QFEC_PTR_MAPPED if mapped else 0)
            | (QFEC_CACHED if cached else 0) | (QFEC_ONE_PASS if one_pass else 0))


def pack_received(data_received, fec_received):
    """The receive maps of qfec_revive_batch: data_received [n, k] bool (data
    packet i of group g arrived), fec_received [n] bool (its FEC packet
    arrived) -> uint8 [n, ceil((k + 1) / 8)], bit i of a map being
    (map[i // 8] >> (i % 8)) & 1, the FEC packet's bit k."""
    import numpy as np
    d = np.asarray(data_received, dtype=bool)
    f = np.asarray(fec_received, dtype=bool)
    if d.ndim != 2 or f.shape != (d.shape[0],):
        raise ValueError("data_received is [n, k], fec_received [n]")
    bits = np.concatenate([d, f[:, None]], axis=1)
    return np.packbits(bits, axis=1, bitorder="little")


def pack_received_ragged(received, fec_received, grp_ptr, map_stride=None):
    """The receive maps of qfec_revive_ragged: received bool per packet in CSR
    order, fec_received bool per group, grp_ptr [n + 1] -> uint8 [n,
    map_stride]; bit i of group g's map is data packet grp_ptr[g] + i, bit k_g
    its FEC packet.  map_stride=None: max_g(k_g // 8 + 1).  ValueError for a
    group outside 1..255 packets or a map_stride too small for some group."""
    import numpy as np
    ptr = np.asarray(grp_ptr).astype(np.int64).ravel()
    f = np.asarray(fec_received, dtype=bool).ravel()
    r = np.asarray(received, dtype=bool).ravel()
    n = ptr.size - 1
    if n < 0 or f.size != n:
        raise ValueError("grp_ptr is [n + 1], fec_received [n]")
    ks = np.diff(ptr)
    if n and (ks.min() < 1 or ks.max() > MAX_GROUP_PACKETS):
        raise ValueError("a FEC group has 1..%d packets" % MAX_GROUP_PACKETS)
    if n and (ptr[0] < 0 or r.size < ptr[-1]):
        raise ValueError("received is shorter than grp_ptr[n]")
    need = int(ks.max()) // 8 + 1 if n else 1
    if map_stride is None:
        map_stride = need
    if map_stride < need:
        raise ValueError("map_stride %d below the %d bytes of the largest group's map"
                         % (map_stride, need))
    bits = np.zeros((n, 8 * map_stride), dtype=bool)
    if n:
        g = np.repeat(np.arange(n), ks)
        i = np.arange(ptr[0], ptr[-1]) - np.repeat(ptr[:-1], ks)
        bits[g, i] = r[ptr[0]:ptr[-1]]
        bits[np.arange(n), ks] = f
    return np.packbits(bits, axis=1, bitorder="little")


class HostBuffer:
    """n bytes of pinned, device-mapped host memory from qfec_host_alloc, as a
    numpy uint8 view (.array); freed with close()."""

    def __init__(self, n: int):
        import numpy as np
        self.lib = load()
        self.ptr = self.lib.qfec_host_alloc(n)
        if not self.ptr:
            raise QfecError(QFEC_ERR_INTERNAL, self.lib.qfec_last_error(None).decode())
        self.n = n
        self.array = np.ctypeslib.as_array((C.c_uint8 * n).from_address(self.ptr))

    def close(self):
        if self.ptr:
            self.array = None
            self.lib.qfec_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostRegistration:
    """Pins and device-maps an existing host buffer (a numpy array, a CPU torch
    tensor or a raw address + size) for mapped=True calls; unregister() (or the
    end of a with-block) releases it.  The buffer must outlive the
    registration."""

    def __init__(self, buf, nbytes=None):
        self.lib = load()
        self.ptr = _ptr(buf)
        self.n = int(nbytes if nbytes is not None else
                     (buf.nbytes if hasattr(buf, "nbytes") else buf.numel() * buf.element_size()))
        rc = self.lib.qfec_host_register(self.ptr, self.n)
        if rc != QFEC_OK:
            raise QfecError(rc, self.lib.qfec_last_error(None).decode())

    def unregister(self):
        if self.ptr:
            rc = self.lib.qfec_host_unregister(self.ptr)
            self.ptr = None
            if rc != QFEC_OK:
                raise QfecError(rc, self.lib.qfec_last_error(None).decode())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.unregister()


def _ptr(x):
    """Address of a torch tensor / numpy array / int / None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        assert x.flags["C_CONTIGUOUS"], "numpy buffers must be C-contiguous"
        return x.ctypes.data
    raise TypeError(f"unsupported buffer {type(x)!r}")


class Context:
    """One qfec_ctx (one device, one stream).  Thread-compatible, not thread-safe."""

    def __init__(self, device: int = 0):
        self.lib = load()
        self.ctx = self.lib.qfec_create(device)
        if not self.ctx:
            raise QfecError(QFEC_ERR_INTERNAL, self.lib.qfec_last_error(None).decode())
        self.device = device

    def close(self):
        if self.ctx:
            self.lib.qfec_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing --------------------------------------------------------
    def _check(self, rc: int):
        if rc != QFEC_OK:
            msg = self.lib.qfec_last_error(self.ctx).decode()
            if rc == QFEC_ERR_INVALID_FEC_DATA:
                raise InvalidFecData(rc, msg)
            raise QfecError(rc, msg)
        return rc

    def set_stream(self, stream):
        """stream: torch.cuda.Stream (its handle; torch's default stream is HIP's
        null stream, handle 0) / raw hipStream_t int / None (the context's own
        non-blocking stream)."""
        if stream is None:
            h = self.lib.qfec_own_stream(self.ctx)
        else:
            h = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        return self._check(self.lib.qfec_set_stream(self.ctx, h or None))

    def sync(self):
        return self._check(self.lib.qfec_sync(self.ctx))

    # -- fixed -------------------------------------------------------------
    def encode(self, rows, k, L, n_groups, parity_out, *, row_stride=None, group_stride=None,
               parity_stride=None, host=False, cached=False, mapped=False, one_pass=False):
        fl = _fl(host, mapped, cached, one_pass)
        if row_stride is None and group_stride is None and parity_stride is None:
            rc = self.lib.qfec_encode_batch(self.ctx, _ptr(rows), k, L, n_groups,
                                            _ptr(parity_out), fl)
        else:
            rs = L if row_stride is None else row_stride
            gs = k * rs if group_stride is None else group_stride
            ps = L if parity_stride is None else parity_stride
            rc = self.lib.qfec_encode_batch_strided(self.ctx, _ptr(rows), k, L, rs, gs, n_groups,
                                                    _ptr(parity_out), ps, fl)
        return self._check(rc)

    def recover(self, rows, parity, missing, k, L, n_groups, out, *, row_stride=None,
                group_stride=None, parity_stride=None, out_stride=None, host=False,
                cached=False, mapped=False, one_pass=False):
        fl = _fl(host, mapped, cached, one_pass)
        if row_stride is None and group_stride is None and parity_stride is None \
                and out_stride is None:
            rc = self.lib.qfec_recover_batch(self.ctx, _ptr(rows), _ptr(parity), _ptr(missing),
                                             k, L, n_groups, _ptr(out), fl)
        else:
            rs = L if row_stride is None else row_stride
            gs = k * rs if group_stride is None else group_stride
            ps = L if parity_stride is None else parity_stride
            os_ = L if out_stride is None else out_stride
            rc = self.lib.qfec_recover_batch_strided(self.ctx, _ptr(rows), _ptr(parity),
                                                     _ptr(missing), k, L, rs, gs, ps, n_groups,
                                                     _ptr(out), os_, fl)
        return self._check(rc)

    def recover_inslot(self, rows, missing, k, L, n_groups, out=None, *, row_stride=None,
                       group_stride=None, out_stride=None, host=False, cached=False,
                       mapped=False, one_pass=False):
        """In-slot recover: rows[g][missing[g]] holds the redundancy; out=None
        writes the lost packet in place there (device pointers only)."""
        fl = _fl(host, mapped, cached, one_pass)
        if row_stride is None and group_stride is None and out_stride is None:
            rc = self.lib.qfec_recover_inslot_batch(self.ctx, _ptr(rows), _ptr(missing), k, L,
                                                    n_groups, _ptr(out), fl)
        else:
            rs = L if row_stride is None else row_stride
            gs = k * rs if group_stride is None else group_stride
            os_ = L if out_stride is None else out_stride
            rc = self.lib.qfec_recover_inslot_batch_strided(self.ctx, _ptr(rows), _ptr(missing),
                                                            k, L, rs, gs, n_groups, _ptr(out),
                                                            os_, fl)
        return self._check(rc)

    def revive(self, rows, parity, received, k, L, n_groups, out=None, *, status,
               revived_idx=None, revived_list=None, counts=None, row_stride=None,
               group_stride=None, parity_stride=None, map_stride=None, out_stride=None,
               cached=False):
        """qfec_revive_batch: classify every group from its receive map
        (pack_received) and rebuild the lost packet of the revivable ones, into
        out or (out=None) in place in rows.  status uint8[n]; revived_idx
        uint8[n], revived_list uint64[n] and counts uint64[3] are optional.
        Device pointers only; queued on the context's stream (sync() before
        reading the results)."""
        fl = _fl(cached=cached)
        if row_stride is None and group_stride is None and parity_stride is None \
                and map_stride is None and out_stride is None:
            rc = self.lib.qfec_revive_batch(self.ctx, _ptr(rows), _ptr(parity), _ptr(received),
                                            k, L, n_groups, _ptr(out), _ptr(status),
                                            _ptr(revived_idx), _ptr(revived_list), _ptr(counts),
                                            fl)
        else:
            rs = L if row_stride is None else row_stride
            gs = k * rs if group_stride is None else group_stride
            ps = L if parity_stride is None else parity_stride
            ms = k // 8 + 1 if map_stride is None else map_stride
            os_ = L if out_stride is None else out_stride
            rc = self.lib.qfec_revive_batch_strided(self.ctx, _ptr(rows), _ptr(parity),
                                                    _ptr(received), k, L, rs, gs, ps, ms,
                                                    n_groups, _ptr(out), os_, _ptr(status),
                                                    _ptr(revived_idx), _ptr(revived_list),
                                                    _ptr(counts), fl)
        return self._check(rc)

    # -- ragged ------------------------------------------------------------
    def encode_ragged(self, data, pkt_off, pkt_len, grp_ptr, n_groups, parity_out, parity_off,
                      parity_len_out, *, host=False, mapped=False, async_=False,
                      small_groups=False):
        rc = self.lib.qfec_encode_ragged(self.ctx, _ptr(data), _ptr(pkt_off), _ptr(pkt_len),
                                         _ptr(grp_ptr), n_groups, _ptr(parity_out),
                                         _ptr(parity_off), _ptr(parity_len_out),
                                         _fl(host, mapped) | (QFEC_ASYNC if async_ else 0)
                                         | (QFEC_SMALL_GROUPS if small_groups else 0))
        return self._check(rc)

    def recover_ragged(self, data, pkt_off, pkt_len, grp_ptr, n_groups, parity, parity_off,
                       parity_len, missing, out, out_off, *, host=False, mapped=False,
                       async_=False, small_groups=False):
        rc = self.lib.qfec_recover_ragged(self.ctx, _ptr(data), _ptr(pkt_off), _ptr(pkt_len),
                                          _ptr(grp_ptr), n_groups, _ptr(parity),
                                          _ptr(parity_off), _ptr(parity_len), _ptr(missing),
                                          _ptr(out), _ptr(out_off),
                                          _fl(host, mapped) | (QFEC_ASYNC if async_ else 0)
                                          | (QFEC_SMALL_GROUPS if small_groups else 0))
        return self._check(rc)

    def revive_ragged(self, data, pkt_off, pkt_len, grp_ptr, n_groups, parity, parity_off,
                      parity_len, received, map_stride, out, out_off, *, status,
                      revived_idx=None, revived_list=None, counts=None):
        """qfec_revive_ragged: classify every group of a CSR batch from its
        receive map (pack_received_ragged) and write the lost packet of the
        revivable ones to out + out_off[g].  status uint8[n]; revived_idx
        uint8[n], revived_list uint64[n] and counts uint64[3] are optional.
        Device pointers only; queued on the context's stream (sync() before
        reading the results)."""
        rc = self.lib.qfec_revive_ragged(self.ctx, _ptr(data), _ptr(pkt_off), _ptr(pkt_len),
                                         _ptr(grp_ptr), n_groups, _ptr(parity),
                                         _ptr(parity_off), _ptr(parity_len), _ptr(received),
                                         map_stride, _ptr(out), _ptr(out_off), _ptr(status),
                                         _ptr(revived_idx), _ptr(revived_list), _ptr(counts), 0)
        return self._check(rc)

    def accumulate_ragged(self, data, pkt_off, pkt_len, grp_ptr, n_groups, acc, acc_stride,
                          acc_len, *, slot=None, n_slots=None):
        """qfec_accumulate_ragged: fold this turn's packets of every group of a
        CSR batch into the group's running row acc + s * acc_stride, s =
        slot[g] (uint32[n]; None: s = g), and raise acc_len[s] (uint16) to the
        longest packet folded.  n_slots=None: n_groups.  Device pointers only;
        queued on the context's stream (sync() before reading the results)."""
        ns = n_groups if n_slots is None else n_slots
        rc = self.lib.qfec_accumulate_ragged(self.ctx, _ptr(data), _ptr(pkt_off), _ptr(pkt_len),
                                             _ptr(grp_ptr), n_groups, _ptr(acc), acc_stride,
                                             _ptr(acc_len), _ptr(slot), ns, 0)
        return self._check(rc)

    def emit_accumulated(self, acc, acc_stride, acc_len, n_groups, out, out_off, out_len, *,
                         slot=None, n_slots=None, release=False, flags=0):
        """qfec_emit_accumulated: copy acc_len[s] bytes of every group's
        running row acc + s * acc_stride, s = slot[g] (uint32[n]; None: s = g),
        to out + out_off[g] (uint64[n]) and the length to out_len[g]
        (uint16[n]); release zeroes acc_len[s] afterwards.  n_slots=None:
        n_groups.  Device pointers only; queued on the context's stream
        (sync() before reading the results)."""
        ns = n_groups if n_slots is None else n_slots
        rc = self.lib.qfec_emit_accumulated(self.ctx, _ptr(acc), acc_stride, _ptr(acc_len),
                                            _ptr(slot), ns, n_groups, _ptr(out), _ptr(out_off),
                                            _ptr(out_len), 1 if release else 0, flags)
        return self._check(rc)

    def revive_accumulated(self, acc, acc_stride, acc_len, group_k, received, map_stride,
                           n_groups, out, out_off, out_len, *, status, slot=None, n_slots=None,
                           revived_idx=None, revived_list=None, counts=None, release_mask=0,
                           flags=0):
        """qfec_revive_accumulated: classify every group from its receive map
        (group_k uint8[n] protected packets; the map says which packets have
        been folded into the row) and copy the row of the revivable ones to
        out + out_off[g] (out None: no copy, the row is the packet), its
        length to out_len[g] (uint16[n]; 0 for every other group).
        release_mask bit st: groups of status st get acc_len[s] = 0.  status
        uint8[n]; revived_idx uint8[n], revived_list uint64[n] and counts
        uint64[3] are optional.  n_slots=None: n_groups.  Device pointers
        only; queued on the context's stream (sync() before reading the
        results)."""
        ns = n_groups if n_slots is None else n_slots
        rc = self.lib.qfec_revive_accumulated(self.ctx, _ptr(acc), acc_stride, _ptr(acc_len),
                                              _ptr(slot), ns, _ptr(group_k), _ptr(received),
                                              map_stride, n_groups, _ptr(out), _ptr(out_off),
                                              _ptr(out_len), _ptr(status), _ptr(revived_idx),
                                              _ptr(revived_list), _ptr(counts), release_mask,
                                              flags)
        return self._check(rc)

    def admit_ragged(self, pkt_off, pkt_len, pkt_idx, pkt_ok, grp_ptr, n_groups, slot_k, acc_map,
                     map_stride, acc_len, acc_stride, grp_ptr_out, pkt_off_out, pkt_len_out,
                     verdict, *, slot=None, n_slots=None, counts=None, flags=0):
        """qfec_admit_ragged: filter a turn's candidates (CSR tables; pkt_idx
        uint8 the position in the group, pkt_ok uint8 the open call's ok or
        None) against the running map of slot s = slot[g] (uint32[n]; None:
        s = g) of K = slot_k[s] protected packets, acc_map + s * map_stride.
        verdict[p] (uint8) receives a QFEC_PKT_* code, grp_ptr_out (uint32[n +
        1]), pkt_off_out and pkt_len_out the tables of the admitted packets
        for accumulate_ragged, counts (uint64[4], optional) the verdicts per
        code; the maps gain the admitted bits.  n_slots=None: n_groups.
        Device pointers only; queued on the context's stream (sync() before
        reading the results)."""
        ns = n_groups if n_slots is None else n_slots
        rc = self.lib.qfec_admit_ragged(self.ctx, _ptr(pkt_off), _ptr(pkt_len), _ptr(pkt_idx),
                                        _ptr(pkt_ok), _ptr(grp_ptr), n_groups, _ptr(slot), ns,
                                        _ptr(slot_k), _ptr(acc_map), map_stride, _ptr(acc_len),
                                        acc_stride, _ptr(grp_ptr_out), _ptr(pkt_off_out),
                                        _ptr(pkt_len_out), _ptr(verdict), _ptr(counts), flags)
        return self._check(rc)

    def revive_tracked(self, acc, acc_stride, acc_len, acc_map, map_stride, slot_k, n_groups, out,
                       out_off, out_len, *, status, slot=None, n_slots=None, revived_idx=None,
                       revived_list=None, counts=None, release_mask=0, flags=0):
        """qfec_revive_tracked: revive_accumulated with K and the map read by
        slot (slot_k uint8[n_slots], acc_map + s * map_stride, as admit_ragged
        keeps them); a slot of length 0 counts as an all-clear map and is
        unrevivable.  Outputs, release_mask and out None as revive_accumulated.
        n_slots=None: n_groups.  Device pointers only; queued on the
        context's stream (sync() before reading the results)."""
        ns = n_groups if n_slots is None else n_slots
        rc = self.lib.qfec_revive_tracked(self.ctx, _ptr(acc), acc_stride, _ptr(acc_len),
                                          _ptr(acc_map), map_stride, _ptr(slot_k), _ptr(slot), ns,
                                          n_groups, _ptr(out), _ptr(out_off), _ptr(out_len),
                                          _ptr(status), _ptr(revived_idx), _ptr(revived_list),
                                          _ptr(counts), release_mask, flags)
        return self._check(rc)

    def bin_arrivals(self, pkt_slot, pkt_off, pkt_len, pkt_idx, pkt_ok, n_packets, n_slots,
                     grp_ptr_out, pkt_off_out, pkt_len_out, pkt_idx_out, *, pkt_ok_out=None,
                     src_out=None, counts=None, flags=0):
        """qfec_bin_arrivals: a turn's per-packet records in arrival order
        (pkt_slot uint32 the slot of the packet's group or QFEC_NO_SLOT,
        pkt_off uint64, pkt_len uint16, pkt_idx uint8, pkt_ok uint8 or None)
        binned by slot into the lockstep CSR tables admit_ragged reads with
        slot=None and n_groups = n_slots: grp_ptr_out (uint32[n_slots + 1]),
        pkt_off_out, pkt_len_out, pkt_idx_out, pkt_ok_out (with pkt_ok) and
        src_out (uint32, optional: the arrival index of every entry), each
        with room for n_packets entries, stable within a slot.  counts
        (uint64[3], optional): binned, QFEC_NO_SLOT, slot out of range (the
        last latched).  Device pointers only; queued on the context's stream
        (sync() before reading the results)."""
        rc = self.lib.qfec_bin_arrivals(self.ctx, _ptr(pkt_slot), _ptr(pkt_off), _ptr(pkt_len),
                                        _ptr(pkt_idx), _ptr(pkt_ok), n_packets, n_slots,
                                        _ptr(grp_ptr_out), _ptr(pkt_off_out), _ptr(pkt_len_out),
                                        _ptr(pkt_idx_out), _ptr(pkt_ok_out), _ptr(src_out),
                                        _ptr(counts), flags)
        return self._check(rc)

    def assign_slots(self, pkt_key, pkt_k, n_packets, slot_key, slot_k, acc_len, n_slots,
                     pkt_slot_out, *, counts=None, flags=0):
        """qfec_assign_slots: a turn's per-packet group keys in arrival order
        (pkt_key uint64, opaque, or QFEC_NO_KEY; pkt_k uint8, the group's K,
        read for a packet that opens a group) resolved to slots: the lowest
        open slot (acc_len > 0) whose slot_key equals the key, or the next
        free slot (acc_len == 0, whatever its slot_key) for the r-th new key
        by first arrival, which writes slot_key (uint64[n_slots]) and slot_k
        (uint8[n_slots]) there.  pkt_slot_out (uint32[n_packets]) is the
        pkt_slot bin_arrivals reads; QFEC_NO_SLOT for QFEC_NO_KEY and for a
        key no free slot was left for.  counts (uint64[5], optional): packets
        of open groups, packets of groups opened in this call, QFEC_NO_KEY,
        groups opened, packets turned away.  Device pointers only; queued on
        the context's stream (sync() before reading the results)."""
        rc = self.lib.qfec_assign_slots(self.ctx, _ptr(pkt_key), _ptr(pkt_k), n_packets,
                                        _ptr(slot_key), _ptr(slot_k), _ptr(acc_len), n_slots,
                                        _ptr(pkt_slot_out), _ptr(counts), flags)
        return self._check(rc)

    def retire_groups(self, pkt_key, n_packets, slot_key, acc_len, n_slots, conn_mark, n_conns,
                      key_shift, max_groups, pkt_key_out, *, raise_conn=None, raise_mark=None,
                      n_raise=0, closed_list=None, counts=None, flags=0):
        """qfec_retire_groups, in front of assign_slots: the one call that
        reads a key (conn = key >> key_shift, number = the bits below).
        conn_mark (uint64[n_conns]) holds every connection's watermark and is
        updated: raised by the turn's thresholds (raise_conn uint32, raise_mark
        uint64, n_raise of them), then, with max_groups in 1..16, to the
        max_groups-th largest distinct number at or above it among the
        connection's open keyed slots (acc_len > 0, slot_key uint64) and keyed
        packets (pkt_key uint64) where there are more than max_groups.  Every
        open keyed slot below its mark gets acc_len (uint16[n_slots]) = 0 and
        is listed ascending in closed_list (uint32[n_slots], optional);
        pkt_key_out (uint64[n_packets], may be pkt_key) is pkt_key with
        QFEC_NO_KEY where the number is below the mark, what assign_slots then
        reads.  counts (uint64[5], optional): slots closed, packets refused,
        QFEC_NO_KEY, packets passed, connections out of range (the last
        latched).  Device pointers only; queued on the context's stream
        (sync() before reading the results)."""
        rc = self.lib.qfec_retire_groups(self.ctx, _ptr(pkt_key), n_packets, _ptr(slot_key),
                                         _ptr(acc_len), n_slots, _ptr(conn_mark), n_conns,
                                         key_shift, max_groups, _ptr(raise_conn),
                                         _ptr(raise_mark), n_raise, _ptr(pkt_key_out),
                                         _ptr(closed_list), _ptr(counts), flags)
        return self._check(rc)

    def parse_opened(self, data, pkt_off, pkt_len, packet_number, pkt_conn, n_packets,
                     quic_version, key_shift, pkt_key_out, pkt_idx_out, body_off_out,
                     body_len_out, hdr_out, *, pkt_ok=None, entropy_out=None, counts=None,
                     flags=0):
        """qfec_parse_opened, in front of retire_groups: the private flags and
        the FEC group offset byte, encrypted on the wire, read from the opened
        packets.  Packet p's plaintext is pkt_len[p] (uint16) bytes at data +
        pkt_off[p] (uint64); packet_number (uint64) and pkt_conn (uint32) come
        from the public header, pkt_ok (uint8, optional) from the open call.
        hdr_out (uint8[n_packets]) is the flags byte, 0..7, of an accepted
        header, or a QFEC_HDR_* class (a FAILED packet's bytes are not read).
        In a group: pkt_key_out (uint64) = pkt_conn << key_shift |
        (packet_number - offset), pkt_idx_out (uint8) = offset, body_off_out
        (uint64) and body_len_out (uint16) the bytes behind the two header
        bytes; outside one QFEC_NO_KEY, 0 and the bytes behind the flags byte;
        a refused packet QFEC_NO_KEY, 0, pkt_off and 0.  entropy_out (uint8,
        optional): the packet's entropy hash, as entropy_cumulative reads it.
        counts (uint64[6], optional): data packets and FEC packets in a group,
        accepted outside any group, FAILED, headers rejected, RANGE (a
        connection or group number that does not fit the key: latched).
        Device pointers only; queued on the context's stream (sync() before
        reading the results)."""
        rc = self.lib.qfec_parse_opened(self.ctx, _ptr(data), _ptr(pkt_off), _ptr(pkt_len),
                                        _ptr(packet_number), _ptr(pkt_conn), _ptr(pkt_ok),
                                        n_packets, quic_version, key_shift, _ptr(pkt_key_out),
                                        _ptr(pkt_idx_out), _ptr(body_off_out),
                                        _ptr(body_len_out), _ptr(hdr_out), _ptr(entropy_out),
                                        _ptr(counts), flags)
        return self._check(rc)

    def write_private_headers(self, data, pkt_off, hdr, fec_offset, n_packets, quic_version, *,
                              body_off_out=None, counts=None, flags=0):
        """qfec_write_private_headers, in front of the seal: hdr[p] (uint8, the
        private flags byte) written at data + pkt_off[p] (uint64) and, where
        its FEC_GROUP bit is set, fec_offset[p] (uint8) behind it.
        body_off_out (uint64, optional) is where the frames or the redundancy
        go: pkt_off + 1 or + 2.  A record with FEC and no group, or with flags
        above the version's maximum, writes no byte, gets pkt_off and is
        latched.  counts (uint64[2], optional): written, refused.  Device
        pointers only; queued on the context's stream."""
        rc = self.lib.qfec_write_private_headers(self.ctx, _ptr(data), _ptr(pkt_off), _ptr(hdr),
                                                 _ptr(fec_offset), n_packets, quic_version,
                                                 _ptr(body_off_out), _ptr(counts), flags)
        return self._check(rc)

    def scan_frames(self, data, body_off, body_len, packet_number, pkt_conn, pkt_pn_len,
                    n_packets, quic_version, max_frames, frm_status, frm_ptr, sw_seen, sw_least,
                    sw_hash, sw_conn, n_conns, *, hdr=None, frm_pkt=None, frm_type=None,
                    frm_flags=None, frm_off=None, frm_len=None, frm_id=None, frm_val=None,
                    frm_code=None, frm_cap=0, counts=None, flags=0):
        """qfec_scan_frames, behind parse_opened and in front of retire_groups:
        QuicFramer::ProcessFrameData over the turn's packets.  Packet p's frame
        area is body_len[p] (uint16) bytes at data + body_off[p] (uint64), the
        parse's outputs; packet_number (uint64), pkt_conn (uint32) and
        pkt_pn_len (uint8: 1, 2, 4 or 6) come from the public header, hdr
        (uint8, optional) from the parse.  frm_status (uint8[n_packets]) is a
        QFEC_FRM_* verdict; frm_ptr (uint32[n_packets + 1]) the prefix sums of
        the frames listed, which only an OK packet does.  The table, with room
        for frm_cap entries: frm_pkt (uint32), frm_type and frm_flags (uint8),
        frm_off (uint64, into data), frm_len (uint16), frm_id (uint32), frm_val
        (uint64), frm_code (uint32).  The STOP_WAITING state per connection,
        all zero when new: sw_seen and sw_least (uint64), sw_hash (uint8);
        sw_conn (uint32) receives 0 .. n_conns - 1, and the four go to
        retire_groups and record_received as the raises with n_raise =
        n_conns.  counts (uint64[13], optional): packets OK, skipped, rejected,
        too many, caller errors; frames stream, ack, stop waiting, other; the
        total; the overflow; connections replaced; of those with a lower
        least_unacked.  Device pointers only; queued on the context's stream."""
        rc = self.lib.qfec_scan_frames(
            self.ctx, _ptr(data), _ptr(body_off), _ptr(body_len), _ptr(packet_number),
            _ptr(pkt_conn), _ptr(pkt_pn_len), _ptr(hdr), n_packets, quic_version, max_frames,
            _ptr(frm_status), _ptr(frm_ptr), _ptr(frm_pkt), _ptr(frm_type), _ptr(frm_flags),
            _ptr(frm_off), _ptr(frm_len), _ptr(frm_id), _ptr(frm_val), _ptr(frm_code), frm_cap,
            _ptr(sw_seen), _ptr(sw_least), _ptr(sw_hash), _ptr(sw_conn), n_conns, _ptr(counts),
            flags)
        return self._check(rc)

    def record_received(self, rcv_cells, rcv_least, rcv_largest, rcv_hash, n_conns, window, *,
                        packet_number=None, pkt_conn=None, n_packets=0, rcv_out=None, hdr=None,
                        entropy=None, status=None, revived_idx=None, slot=None, slot_key=None,
                        n_groups=0, n_slots=0, key_shift=0, raise_conn=None, raise_least=None,
                        raise_hash=None, n_raise=0, counts=None, flags=0):
        """qfec_record_received, behind revive_tracked: one turn into the ack
        state.  The state is the caller's, all zero for a new connection:
        rcv_cells (uint8[n_conns * window], window a power of two in 64..65536;
        the cell of packet pn is pn & (window - 1): QFEC_CELL_RECEIVED |
        QFEC_CELL_ENTROPY | QFEC_CELL_REVIVED), rcv_least and rcv_largest
        (uint64[n_conns]), rcv_hash (uint8[n_conns]).  Arrivals: packet_number
        (uint64), pkt_conn (uint32), hdr (uint8, optional: parse_opened's
        hdr_out, accepted below 0x80), entropy (uint8, optional: its
        entropy_out, non-zero = flag 1); rcv_out (uint8[n_packets]) gets a
        QFEC_RCV_* class per packet.  Revived: revive_tracked's status,
        revived_idx and slot with assign_slots' slot_key (uint64[n_slots]) and
        retire_groups' key_shift.  Raises: the turn's STOP_WAITING frames,
        raise_conn (uint32, at most one per connection), raise_least (uint64),
        raise_hash (uint8).  counts (uint64[12], optional): the six classes,
        cells newly set, revived recorded, revived not missing, raises
        applied, raises that dropped a missing packet, jumps.  Device pointers
        only; queued on the context's stream (sync() before reading)."""
        rc = self.lib.qfec_record_received(
            self.ctx, _ptr(packet_number), _ptr(pkt_conn), _ptr(hdr), _ptr(entropy), n_packets,
            _ptr(status), _ptr(revived_idx), _ptr(slot), _ptr(slot_key), n_groups, n_slots,
            key_shift, _ptr(raise_conn), _ptr(raise_least), _ptr(raise_hash), n_raise,
            _ptr(rcv_cells), _ptr(rcv_least), _ptr(rcv_largest), _ptr(rcv_hash), n_conns, window,
            _ptr(rcv_out), _ptr(counts), flags)
        return self._check(rc)

    def build_acks(self, ack_conn, n_acks, rcv_cells, rcv_least, rcv_largest, rcv_hash, n_conns,
                   window, max_ranges, max_revived, largest_observed, entropy_hash, truncated,
                   range_ptr, range_lo, range_hi, rev_ptr, rev_pn=None, *, flags=0):
        """qfec_build_acks: the ack frame's content for the connections
        ack_conn (uint32[n_acks], repeats allowed) from the state
        record_received keeps; the state is only read.  largest_observed
        (uint64), entropy_hash and truncated (uint8) per ack; the missing
        packets as ascending half-open intervals range_lo / range_hi (uint64,
        room for n_acks * max_ranges) under range_ptr (uint32[n_acks + 1]),
        the form entropy_validate reads; the revived packets rev_pn (uint64,
        room for n_acks * max_revived) under rev_ptr.  With more than
        max_ranges (1..255) intervals the lowest are kept, largest_observed
        falls to just below the first one dropped and truncated is 1.  Device
        pointers only; queued on the context's stream (sync() before
        reading)."""
        rc = self.lib.qfec_build_acks(
            self.ctx, _ptr(ack_conn), n_acks, _ptr(rcv_cells), _ptr(rcv_least), _ptr(rcv_largest),
            _ptr(rcv_hash), n_conns, window, max_ranges, max_revived, _ptr(largest_observed),
            _ptr(entropy_hash), _ptr(truncated), _ptr(range_ptr), _ptr(range_lo), _ptr(range_hi),
            _ptr(rev_ptr), _ptr(rev_pn), flags)
        return self._check(rc)

    def write_ack_frames(self, ack_conn, n_acks, largest_observed, entropy_hash, truncated,
                         range_ptr, range_lo, range_hi, rev_ptr, rev_pn, rcv_cells, n_conns,
                         window, out, out_off, out_cap, out_len, wire_largest, wire_hash,
                         ack_status, *, ack_delay_us=None, prefix_len=0, counts=None, flags=0):
        """qfec_write_ack_frames, behind build_acks: the built acks as v<=31
        ack frames.  ack_conn and build_acks' eight outputs; ack_delay_us
        (uint64, optional: all infinite); the ring rcv_cells, only read.  Ack
        a's frame goes to out + out_off[a] (uint64) and has out_cap[a]
        (uint16) bytes of room; with more nack ranges than fit the writer cuts
        the ack as the framer does.  out_len[a] (uint16) = prefix_len + the
        frame's length, 0 where nothing was written; wire_largest (uint64) and
        wire_hash (uint8) as written; ack_status (uint8) a QFEC_ACKW_* value;
        counts (uint64[4], optional): the acks per status.  Device pointers
        only; queued on the context's stream."""
        rc = self.lib.qfec_write_ack_frames(
            self.ctx, _ptr(ack_conn), n_acks, _ptr(largest_observed), _ptr(entropy_hash),
            _ptr(truncated), _ptr(range_ptr), _ptr(range_lo), _ptr(range_hi), _ptr(rev_ptr),
            _ptr(rev_pn), _ptr(ack_delay_us), _ptr(rcv_cells), n_conns, window, _ptr(out),
            _ptr(out_off), _ptr(out_cap), prefix_len, _ptr(out_len), _ptr(wire_largest),
            _ptr(wire_hash), _ptr(ack_status), _ptr(counts), flags)
        return self._check(rc)

    def xor_into(self, src, n, dst, *, host=False, mapped=False):
        return self._check(self.lib.qfec_xor_into(self.ctx, _ptr(src), n, _ptr(dst),
                                                  _fl(host, mapped)))

    # -- packet protection (ENCRYPTION_NONE) --------------------------------
    def null_encrypt(self, data, ad_off, ad_len, in_off, in_len, n, out, out_off, *, host=False):
        return self._check(self.lib.qfec_null_encrypt_batch(
            self.ctx, _ptr(data), _ptr(ad_off), _ptr(ad_len), _ptr(in_off), _ptr(in_len), n,
            _ptr(out), _ptr(out_off), QFEC_PTR_HOST if host else 0))

    def null_decrypt(self, data, ad_off, ad_len, in_off, in_len, n, out, out_off, ok, *,
                     host=False, scratch_out=False):
        """scratch_out: QFEC_SCRATCH_OUTPUT (one pass; a failed packet's output
        holds its unverified plaintext)."""
        fl = (QFEC_PTR_HOST if host else 0) | (QFEC_SCRATCH_OUTPUT if scratch_out else 0)
        return self._check(self.lib.qfec_null_decrypt_batch(
            self.ctx, _ptr(data), _ptr(ad_off), _ptr(ad_len), _ptr(in_off), _ptr(in_len), n,
            _ptr(out), _ptr(out_off), _ptr(ok), fl))

    def chacha20poly1305_seal(self, keys, prefixes, key_idx, packet_number, path_id, data, ad_off,
                              ad_len, in_off, in_len, n, out, out_off, *, host=False):
        return self._check(self.lib.qfec_chacha20poly1305_seal_batch(
            self.ctx, _ptr(keys), _ptr(prefixes), _ptr(key_idx), _ptr(packet_number),
            _ptr(path_id), _ptr(data), _ptr(ad_off), _ptr(ad_len), _ptr(in_off), _ptr(in_len), n,
            _ptr(out), _ptr(out_off), QFEC_PTR_HOST if host else 0))

    def chacha20poly1305_open(self, keys, prefixes, key_idx, packet_number, path_id, data, ad_off,
                              ad_len, in_off, in_len, n, out, out_off, ok, *, host=False,
                              scratch_out=False):
        fl = (QFEC_PTR_HOST if host else 0) | (QFEC_SCRATCH_OUTPUT if scratch_out else 0)
        return self._check(self.lib.qfec_chacha20poly1305_open_batch(
            self.ctx, _ptr(keys), _ptr(prefixes), _ptr(key_idx), _ptr(packet_number),
            _ptr(path_id), _ptr(data), _ptr(ad_off), _ptr(ad_len), _ptr(in_off), _ptr(in_len), n,
            _ptr(out), _ptr(out_off), _ptr(ok), fl))

    def aes128gcm_seal(self, keys, prefixes, key_idx, packet_number, path_id, data, ad_off,
                       ad_len, in_off, in_len, n, out, out_off, *, host=False):
        return self._check(self.lib.qfec_aes128gcm_seal_batch(
            self.ctx, _ptr(keys), _ptr(prefixes), _ptr(key_idx), _ptr(packet_number),
            _ptr(path_id), _ptr(data), _ptr(ad_off), _ptr(ad_len), _ptr(in_off), _ptr(in_len), n,
            _ptr(out), _ptr(out_off), QFEC_PTR_HOST if host else 0))

    def aes128gcm_open(self, keys, prefixes, key_idx, packet_number, path_id, data, ad_off,
                       ad_len, in_off, in_len, n, out, out_off, ok, *, host=False,
                       scratch_out=False):
        fl = (QFEC_PTR_HOST if host else 0) | (QFEC_SCRATCH_OUTPUT if scratch_out else 0)
        return self._check(self.lib.qfec_aes128gcm_open_batch(
            self.ctx, _ptr(keys), _ptr(prefixes), _ptr(key_idx), _ptr(packet_number),
            _ptr(path_id), _ptr(data), _ptr(ad_off), _ptr(ad_len), _ptr(in_off), _ptr(in_len), n,
            _ptr(out), _ptr(out_off), _ptr(ok), fl))

    # -- packet-entropy bookkeeping --------------------------------------------
    def entropy_cumulative(self, entropy, conn_ptr, cum_base, n_conns, cum, *, n_packets=0,
                           host=False):
        return self._check(self.lib.qfec_entropy_cumulative_batch(
            self.ctx, _ptr(entropy), _ptr(conn_ptr), _ptr(cum_base), n_conns, n_packets,
            _ptr(cum), QFEC_PTR_HOST if host else 0))

    def entropy_validate(self, cum, conn_ptr, first_pn, cum_base, n_conns, ack_conn, largest,
                         claimed, range_ptr, range_lo, range_hi, n_acks, ok, *, host=False):
        return self._check(self.lib.qfec_entropy_validate_batch(
            self.ctx, _ptr(cum), _ptr(conn_ptr), _ptr(first_pn), _ptr(cum_base), n_conns,
            _ptr(ack_conn), _ptr(largest), _ptr(claimed), _ptr(range_ptr), _ptr(range_lo),
            _ptr(range_hi), n_acks, _ptr(ok), QFEC_PTR_HOST if host else 0))

    def stream_probe(self, src, n, dst, copy=False):
        return self._check(self.lib.qfec_stream_probe(self.ctx, _ptr(src), n, _ptr(dst),
                                                      1 if copy else 0))

    # -- synthetic inputs ----------------------------------------------------
    def phase_backoff(self):
        """Large fixed batches left on the one-pass kernel (contention backoff)."""
        return self.lib.qfec_phase_backoff(self.ctx)

    def last_fixed_phased(self):
        """1 if the last device fixed-shape call ran the phased kernel, 0 the
        one-pass kernel, -1 none yet."""
        return self.lib.qfec_last_fixed_phased(self.ctx)

    def last_phase_grid(self):
        """Test hook: workgroups of the last phased launch (0: one-pass)."""
        return self.lib.qfec_debug_last_phase_grid(self.ctx)

    def debug_phase(self, extra, reset_backoff=True):
        """Test hook: extra workgroups in phased launches (forces the abandon
        path); reset_backoff clears the contention backoff."""
        return self._check(self.lib.qfec_debug_phase(self.ctx, extra, int(reset_backoff)))

    def debug_phase_min(self, min_phases):
        """Test hook: phased kernel from `min_phases` phases on (0 default,
        1 always, 0xFFFFFFFF never)."""
        return self._check(self.lib.qfec_debug_phase_min(self.ctx, min_phases))

    def async_ticket(self):
        """Ticket of the last ragged call if it was queued (QFEC_ASYNC), else 0."""
        return self.lib.qfec_async_ticket(self.ctx)

    def complete_ticket(self, ticket, wait=True):
        """Finish one queued op: 0 done, QFEC_PENDING (1) still running;
        raises its own error only."""
        rc = self.lib.qfec_complete_ticket(self.ctx, ticket, 1 if wait else 0)
        return rc if rc == 1 else self._check(rc)

    def service_warm(self):
        """qfec_service_warm: make sure the small-batch service's worker runs
        (an event loop's turn start); a no-op with the service off."""
        self._check(self.lib.qfec_service_warm(self.ctx))

    def debug_service(self, on=None, poison_next=False):
        """Small-batch service hook: on True / False enables / disables the
        resident worker (None leaves it); poison_next malforms the next job's
        ring entry (test of the ring-miss path); returns {launches, jobs, alive}."""
        st = (C.c_uint64 * 6)()
        mode = 2 if poison_next else (3 if on is None else int(bool(on)))
        self._check(self.lib.qfec_debug_service(self.ctx, mode, st))
        d = {"launches": st[0], "jobs": st[1], "alive": st[2]}
        if mode == 3:  # the registry's view: worker stream busy, us since last use
            d["stream_busy"], d["idle_us"], d["rotations"] = st[3], st[4], st[5]
        return d

    def debug_service_stamps(self, on=None):
        """Measurement hook: the worker's wall-clock stamps (10-ns ticks) of
        the last job: seen, entry, first group, all groups, fence, token."""
        st = (C.c_uint64 * 6)()
        self._check(self.lib.qfec_debug_service_stamps(self.ctx, -1 if on is None else int(bool(on)), st))
        return list(st)

    def debug_service_trace(self):
        """Measurement hook: the last service job end to end (44 words, see
        qfec.h qfec_debug_service_trace)."""
        st = (C.c_uint64 * 44)()
        self._check(self.lib.qfec_debug_service_trace(self.ctx, st))
        return list(st)

    def debug_service_feed(self, on):
        """Measurement hook: a native thread owning this context flushes
        one-group mapped batches back to back (on=True); on=False stops it and
        returns {jobs, wrong}."""
        st = (C.c_uint64 * 2)()
        self._check(self.lib.qfec_debug_service_feed(self.ctx, 1 if on else 0, st))
        return None if on else {"jobs": st[0], "wrong": st[1]}

    def debug_service_hold(self, hold):
        """Test hook: the service's followers wait at their start while held."""
        return self._check(self.lib.qfec_debug_service_hold(self.ctx, 1 if hold else 0))

    def debug_service_resident(self, ns):
        """Test hook: the worker's residency bound in ns (0: rotate at every
        job); returns the previous bound."""
        return int(self.lib.qfec_debug_service_resident(self.ctx, int(ns)))

    def debug_service_idle(self, us):
        """Test hook: the worker's idle time in us for later launches (default
        100); returns the previous value."""
        return int(self.lib.qfec_debug_service_idle(self.ctx, int(us)))

    def debug_phase_regsteps(self, on):
        """Test hook: phased launches with (True) or without their register-held steps."""
        return self._check(self.lib.qfec_debug_phase_regsteps(self.ctx, 1 if on else 0))

    def debug_other_service_cus(self):
        """Test hook: (CUs a phased launch here leaves to other contexts' workers, why-bits)."""
        why = C.c_uint32(0)
        n = self.lib.qfec_debug_other_service_cus(self.ctx, C.byref(why))
        return int(n), int(why.value)

    def debug_phase_reserve(self, cus):
        """Test hook: phased grids leave `cus` more CUs out (the CU-arbitration A/B)."""
        return self._check(self.lib.qfec_debug_phase_reserve(self.ctx, cus))

    def debug_phase_rtbatch(self, batch):
        """Test hook: the runtime-k phased body's load batch (16, 32; 0 = the
        default by operation: encode and in place 16, recover 32 up to
        k = 32 and 16 above)."""
        return self._check(self.lib.qfec_debug_phase_rtbatch(self.ctx, batch))

    def complete(self, wait=True):
        """Finish QFEC_ASYNC calls: 0 done, QFEC_PENDING (1) still running."""
        rc = self.lib.qfec_complete(self.ctx, 1 if wait else 0)
        return rc if rc == 1 else self._check(rc)

    def phase_abandons(self):
        """Phased fixed-shape launches that gave up their grid-wide meetings."""
        n = C.c_uint32(0)
        self._check(self.lib.qfec_phase_abandons(self.ctx, C.byref(n)))
        return n.value

    def synth_fixed(self, rows, k, L, g0, n_groups, seed, *, row_stride=None, group_stride=None):
        rs = L if row_stride is None else row_stride
        gs = k * rs if group_stride is None else group_stride
        return self._check(self.lib.qfec_synth_fixed(self.ctx, _ptr(rows), k, L, rs, gs, g0,
                                                     n_groups, seed))

    def synth_ragged(self, data, pkt_off, pkt_len, grp_ptr, g0, n_groups, seed):
        return self._check(self.lib.qfec_synth_ragged(self.ctx, _ptr(data), _ptr(pkt_off),
                                                      _ptr(pkt_len), _ptr(grp_ptr), g0,
                                                      n_groups, seed))


# -- v<=31 wire format (host-only C-ABI: no device, no context) -------------------
class FecHeader(C.Structure):
    """qfec_fec_header"""
    _fields_ = [("entropy_flag", C.c_uint8), ("fec_flag", C.c_uint8),
                ("in_fec_group", C.c_uint8), ("fec_group_offset", C.c_uint8)]


def _last_error():
    return load().qfec_last_error(None).decode()


def wire_write_private_header(entropy=False, fec=False, in_group=False, offset=0):
    """bytes written by qfec_wire_write_private_header (b"" on failure)."""
    h = FecHeader(int(entropy), int(fec), int(in_group), offset)
    buf = (C.c_uint8 * 4)()
    n = load().qfec_wire_write_private_header(C.byref(h), C.addressof(buf), 4)
    return bytes(buf[:n])


def wire_parse_private_header(data: bytes, version: int, packet_number: int):
    """(consumed, FecHeader) or (0, detailed_error)."""
    h = FecHeader()
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    n = load().qfec_wire_parse_private_header(C.addressof(buf), len(data), version,
                                              packet_number, C.byref(h))
    return (n, h) if n else (0, _last_error())


def wire_write_revived(revived, packet_number_length):
    arr = (C.c_uint64 * max(1, len(revived)))(*revived)
    cap = 1 + len(revived) * 8
    buf = (C.c_uint8 * cap)()
    n = load().qfec_wire_write_revived(C.addressof(arr), len(revived), packet_number_length,
                                       C.addressof(buf), cap)
    return bytes(buf[:n])


def wire_parse_revived(data: bytes, packet_number_length):
    """(consumed, [packet numbers]) or (0, detailed_error)."""
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    out = (C.c_uint64 * 256)()
    cnt = C.c_size_t(0)
    n = load().qfec_wire_parse_revived(C.addressof(buf), len(data), packet_number_length,
                                       C.addressof(out), C.byref(cnt))
    return (n, list(out[:cnt.value])) if n else (0, _last_error())


def wire_fec_packet_body(packet_number, fec_group, entropy, redundancy: bytes):
    red = (C.c_uint8 * max(1, len(redundancy))).from_buffer_copy(redundancy or b"\0")
    cap = 2 + len(redundancy)
    buf = (C.c_uint8 * cap)()
    n = load().qfec_wire_fec_packet_body(packet_number, fec_group, int(entropy),
                                         C.addressof(red), len(redundancy), C.addressof(buf), cap)
    return bytes(buf[:n])


ENTROPY_UP_TO = C.CFUNCTYPE(C.c_uint8, C.c_void_p, C.c_uint64)


def wire_write_ack_frame(largest, entropy_hash, ranges, revived, delay_us, cap, *, truncated=False,
                         entropy_up_to=None):
    """(frame bytes, largest written, hash written, truncated bit) of
    qfec_wire_write_ack_frame; the bytes are b"" where nothing fits.  ranges:
    ascending half-open (lo, hi) pairs; delay_us None: infinite; entropy_up_to:
    a function of a packet number, asked only when the writer cuts."""
    lo = (C.c_uint64 * max(1, len(ranges)))(*[r[0] for r in ranges])
    hi = (C.c_uint64 * max(1, len(ranges)))(*[r[1] for r in ranges])
    rev = (C.c_uint64 * max(1, len(revived)))(*revived)
    buf = (C.c_uint8 * max(1, cap))()
    wl, wh, wt = C.c_uint64(0), C.c_uint8(0), C.c_int(0)
    cb = ENTROPY_UP_TO((lambda user, pn: entropy_up_to(pn) & 0xFF) if entropy_up_to
                       else (lambda user, pn: 0))
    n = load().qfec_wire_write_ack_frame(
        largest, entropy_hash, C.addressof(lo), C.addressof(hi), len(ranges), C.addressof(rev),
        len(revived), (1 << 64) - 1 if delay_us is None else delay_us, int(truncated),
        C.cast(cb, C.c_void_p), None, C.addressof(buf), cap, C.addressof(wl), C.addressof(wh),
        C.addressof(wt))
    return bytes(buf[:n]), wl.value, wh.value, bool(wt.value)


def wire_parse_ack_frame(data: bytes):
    """(consumed, dict(largest, hash, delay (the ufloat16), truncated, ranges,
    revived)) or (0, detailed_error)."""
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    largest, h, delay, trunc = C.c_uint64(0), C.c_uint8(0), C.c_uint16(0), C.c_int(0)
    lo, hi, rev = (C.c_uint64 * 255)(), (C.c_uint64 * 255)(), (C.c_uint64 * 255)()
    n_r, n_v = C.c_size_t(0), C.c_size_t(0)
    n = load().qfec_wire_parse_ack_frame(
        C.addressof(buf), len(data), C.addressof(largest), C.addressof(h), C.addressof(delay),
        C.addressof(trunc), C.addressof(lo), C.addressof(hi), C.addressof(n_r), C.addressof(rev),
        C.addressof(n_v))
    if not n:
        return 0, _last_error()
    return n, dict(largest=largest.value, hash=h.value, delay=delay.value,
                   truncated=bool(trunc.value),
                   ranges=list(zip(lo[:n_r.value], hi[:n_r.value])), revived=list(rev[:n_v.value]))


def wire_scan_frames(body: bytes, quic_version, packet_number, pn_len, max_frames=255):
    """(status, listed, walked) of qfec_wire_scan_frames: the QFEC_FRM_* verdict,
    the frames the packet lists (none unless the verdict is OK) and the frames
    read before the verdict was reached, each a tuple (type, flags, off, len,
    id, val, code) with off counted from the body's first byte."""
    import numpy as np
    buf = (C.c_uint8 * max(1, len(body))).from_buffer_copy(body or b"\0")
    m = max(1, max_frames)
    t, fl = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    off, ln = np.zeros(m, np.uint32), np.zeros(m, np.uint16)
    fid, val, code = np.zeros(m, np.uint32), np.zeros(m, np.uint64), np.zeros(m, np.uint32)
    status, n_walked = C.c_uint8(0), C.c_size_t(0)
    n = load().qfec_wire_scan_frames(
        C.addressof(buf), len(body), quic_version, packet_number, pn_len, max_frames,
        C.addressof(status), C.addressof(n_walked), t.ctypes.data, fl.ctypes.data, off.ctypes.data,
        ln.ctypes.data, fid.ctypes.data, val.ctypes.data, code.ctypes.data)
    if n == C.c_size_t(-1).value:
        raise QfecError(-1, _last_error())
    walked = [(int(t[k]), int(fl[k]), int(off[k]), int(ln[k]), int(fid[k]), int(val[k]),
               int(code[k])) for k in range(n_walked.value)]
    return status.value, walked[:n], walked
