"""ctypes binding of libiyokan_hip.so — the C ABI declared in include/iyokan_hip.h.

Host-side mirror of the cuFHE surface Iyokan's GPU worker uses
(/root/reference/src/iyokan_cufhe.hpp:8-32,249-261; /root/reference/src/iyokan_cufhe.cpp:530-536,721):
`initialize()` = cufhe::SetGPUNum + cufhe::Initialize, `Stream` = CUFHEStream,
`Stream.gate_batch` = N x cufhe::Nand/And/.../Mux, `Stream.query` = cufhe::StreamQuery,
`cleanup()` = cufhe::CleanUp.  There is no CPU fallback: every call goes to the HIP library
and raises IykHipError if it is missing or reports an error.
"""
import ctypes
import os

import numpy as np

from .params import IykParams, OPS

_LIB = None
_u32p = ctypes.POINTER(ctypes.c_uint32)
_i32p = ctypes.POINTER(ctypes.c_int32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libiyokan_hip.so")

# every symbol include/iyokan_hip.h declares (tests check the built library exports them all)
EXPORTS = [
    "iyk_hip_init", "iyk_hip_cleanup", "iyk_hip_is_initialized", "iyk_hip_num_gpus", "iyk_hip_get_params",
    "iyk_hip_last_error", "iyk_hip_stream_create", "iyk_hip_stream_wrap", "iyk_hip_stream_destroy",
    "iyk_hip_stream_query", "iyk_hip_stream_sync", "iyk_hip_arena_alloc", "iyk_hip_arena_free",
    "iyk_hip_arena_upload", "iyk_hip_arena_download", "iyk_hip_gate_batch", "iyk_hip_gate_host",
    "iyk_hip_blind_rotate_batch", "iyk_hip_last_batch_timing", "iyk_hip_resident_key_bytes",
    "iyk_hip_timing_log_begin", "iyk_hip_timing_log_end", "iyk_hip_ntt_path", "iyk_hip_decomposition_levels", "iyk_hip_fft_round_error", "iyk_hip_level_cost_defaults", "iyk_hip_level_cost_table",
    "iyk_hip_level_cost_ms", "iyk_hip_calibrate",
    "iyk_hip_bootstrap_trlwe_batch", "iyk_hip_sample_extract_keyswitch_batch",
    "iyk_hip_stream_gpu", "iyk_hip_arena_upload_slots", "iyk_hip_arena_download_slots", "iyk_hip_arena_copy",
    "iyk_hip_arena_sync_slots", "iyk_hip_trlwe_alloc", "iyk_hip_trlwe_free", "iyk_hip_trlwe_upload",
    "iyk_hip_trlwe_download", "iyk_hip_rotation_round", "iyk_hip_arena_sync_slots_multi", "iyk_hip_peer_access",
    "iyk_hip_build_id", "iyk_hip_host_alloc", "iyk_hip_host_free", "iyk_hip_init_profile",
    "iyk_hip_trgsw_alloc", "iyk_hip_trgsw_free", "iyk_hip_trgsw_upload", "iyk_hip_cmux_batch",
    "iyk_hip_sample_extract_index_keyswitch_batch", "iyk_hip_cmux_chain_batch", "iyk_hip_trlwe_add_batch",
    "iyk_hip_privks_key_create", "iyk_hip_privks_key_upload", "iyk_hip_privks_key_free", "iyk_hip_privks_key_bytes",
    "iyk_hip_tlwe2_alloc", "iyk_hip_tlwe2_free", "iyk_hip_tlwe2_upload", "iyk_hip_tlwe2_download", "iyk_hip_privks_batch",
    "iyk_hip_trgsw_from_rows",
    "iyk_hip_bk2_key_create", "iyk_hip_bk2_key_upload", "iyk_hip_bk2_key_free", "iyk_hip_bk2_key_bytes", "iyk_hip_cb_rotate_batch",
    "iyk_hip_circuit_bootstrap_batch", "iyk_hip_cb_rotate_many_batch", "iyk_hip_circuit_bootstrap_many_batch", "iyk_hip_cb_rotate_form", "iyk_hip_bk2_key_create_form", "iyk_hip_bk2_key_form",
    "iyk_hip_cmux_rotate_chain_batch", "iyk_hip_cmux_tree_batch", "iyk_hip_stream_wait_stream",
    "iyk_hip_gate_batch_lanes",
    "iyk_hip_cmux_batch_lanes", "iyk_hip_cmux_chain_batch_lanes", "iyk_hip_cmux_rotate_chain_batch_lanes", "iyk_hip_cmux_tree_batch_lanes",
    "iyk_hip_privks_key_upload_seeded", "iyk_hip_bk2_key_upload_seeded",
]


CMUX_LANES = ("iyk_hip_cmux_batch_lanes", "iyk_hip_cmux_chain_batch_lanes", "iyk_hip_cmux_rotate_chain_batch_lanes",
              "iyk_hip_cmux_tree_batch_lanes")


class IykHipError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise IykHipError(f"{LIB_PATH} is missing — build it with __graft_entry__.build(); there is no CPU fallback")
        # Load order matters: PyTorch ships its own libamdhip64; if our library pulled in the system
        # HIP runtime first, torch.cuda would later find "No HIP GPUs".  Importing torch first makes
        # both share one runtime (torch is only plumbing here: device tensors, streams, RCCL).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        L.iyk_hip_last_error.restype = ctypes.c_char_p
        L.iyk_hip_init.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(IykParams), _u32p, _u32p]
        L.iyk_hip_get_params.argtypes = [ctypes.POINTER(IykParams)]
        L.iyk_hip_stream_create.argtypes = [ctypes.c_int, ctypes.POINTER(_vp)]
        L.iyk_hip_stream_wrap.argtypes = [ctypes.c_int, _vp, ctypes.POINTER(_vp)]
        for f in ("iyk_hip_stream_destroy", "iyk_hip_stream_query", "iyk_hip_stream_sync", "iyk_hip_stream_gpu"):
            getattr(L, f).argtypes = [_vp]
        L.iyk_hip_stream_wait_stream.argtypes = [_vp, _vp]
        u64 = ctypes.c_uint64
        L.iyk_hip_arena_alloc.argtypes = [ctypes.c_int, u64, ctypes.POINTER(_vp)]
        L.iyk_hip_arena_free.argtypes = [ctypes.c_int, _vp]
        L.iyk_hip_arena_upload.argtypes = [_vp, _vp, u64, u64, u64, _u32p]
        L.iyk_hip_arena_download.argtypes = [_vp, _vp, u64, u64, u64, _u32p]
        L.iyk_hip_arena_upload_slots.argtypes = [_vp, _vp, u64, u64, _i32p, _u32p]
        L.iyk_hip_arena_download_slots.argtypes = [_vp, _vp, u64, u64, _i32p, _u32p]
        L.iyk_hip_arena_copy.argtypes = [_vp, _vp, u64, u64, _vp, u64, u64, u64]
        L.iyk_hip_arena_sync_slots.argtypes = [_vp, _vp, u64, _vp, _vp, u64, u64, _i32p]
        L.iyk_hip_arena_sync_slots_multi.argtypes = [_vp, _vp, u64, ctypes.c_int, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                                     ctypes.POINTER(u64), u64, _i32p]
        L.iyk_hip_peer_access.argtypes = [ctypes.c_int, ctypes.c_int]
        L.iyk_hip_trlwe_alloc.argtypes = [ctypes.c_int, u64, ctypes.POINTER(_vp)]
        L.iyk_hip_trlwe_free.argtypes = [ctypes.c_int, _vp]
        L.iyk_hip_trlwe_upload.argtypes = [_vp, _vp, u64, u64, u64, _u32p]
        L.iyk_hip_trlwe_download.argtypes = [_vp, _vp, u64, u64, u64, _u32p]
        L.iyk_hip_gate_batch.argtypes = [_vp, _vp, u64, u64, _i32p, _i32p, _i32p, _i32p, _i32p]
        if hasattr(L, "iyk_hip_gate_batch_lanes"):   # a library from before the entry point still loads: Stream.gate_batch raises on lanes
            L.iyk_hip_gate_batch_lanes.argtypes = [_vp, _vp, u64, u64, _i32p, _i32p, _i32p, _i32p, _i32p, u64, u64]
        L.iyk_hip_gate_host.argtypes = [_vp, ctypes.c_int, _u32p, _u32p, _u32p, _u32p]
        L.iyk_hip_blind_rotate_batch.argtypes = [_vp, _vp, u64, u64, _i32p, _i32p, _i32p, _i32p, _u32p, _vp]
        L.iyk_hip_bootstrap_trlwe_batch.argtypes = [_vp, _vp, u64, u64, _i32p, _i32p, _i32p, _i32p, _u32p, _vp, u64, _i32p]
        L.iyk_hip_sample_extract_keyswitch_batch.argtypes = [_vp, _vp, u64, u64, _i32p, _i32p, _vp, u64]
        L.iyk_hip_sample_extract_index_keyswitch_batch.argtypes = [_vp, _vp, u64, u64, _i32p, _i32p, _i32p, _vp, u64]
        L.iyk_hip_trgsw_alloc.argtypes = [ctypes.c_int, u64, ctypes.POINTER(_vp)]
        L.iyk_hip_trgsw_free.argtypes = [ctypes.c_int, _vp]
        L.iyk_hip_trgsw_upload.argtypes = [_vp, _vp, u64, u64, u64, _u32p]
        L.iyk_hip_cmux_batch.argtypes = [_vp, _vp, u64, _vp, u64, u64, _i32p, _i32p, _i32p, _i32p, _i32p]
        L.iyk_hip_cmux_chain_batch.argtypes = [_vp, _vp, u64, _vp, u64, u64, _i32p, _i32p, _u32p, _i32p, _i32p, _i32p]
        L.iyk_hip_cmux_rotate_chain_batch.argtypes = [_vp, _vp, u64, _vp, u64, u64, _i32p, _i32p, _i32p, _i32p, _i32p]
        L.iyk_hip_cmux_tree_batch.argtypes = [_vp, _vp, u64, _vp, u64, u64, _i32p, _i32p, _i32p, _i32p]
        for f in CMUX_LANES:   # a library from before these entry points still loads: the Stream.cmux_*_batch calls raise on lanes
            if hasattr(L, f):
                getattr(L, f).argtypes = getattr(L, f[:-len("_lanes")]).argtypes + [ctypes.c_uint32, u64, u64]
        L.iyk_hip_trlwe_add_batch.argtypes = [_vp, _vp, u64, u64, _i32p, _i32p, _i32p, ctypes.c_uint32]
        u32 = ctypes.c_uint32
        L.iyk_hip_privks_key_create.argtypes = [ctypes.c_int, u32, u32, u32, ctypes.POINTER(_vp)]
        L.iyk_hip_privks_key_upload.argtypes = [_vp, _vp, u64, u64, _u32p]
        L.iyk_hip_privks_key_upload_seeded.argtypes = [_vp, _vp, ctypes.c_char_p, u64, u64, _u32p]
        L.iyk_hip_privks_key_free.argtypes = [_vp]
        L.iyk_hip_privks_key_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(u64)]
        L.iyk_hip_tlwe2_alloc.argtypes = [ctypes.c_int, u32, u64, ctypes.POINTER(_vp)]
        L.iyk_hip_tlwe2_free.argtypes = [ctypes.c_int, _vp]
        L.iyk_hip_tlwe2_upload.argtypes = [_vp, _vp, u32, u64, u64, u64, _u64p]
        L.iyk_hip_tlwe2_download.argtypes = [_vp, _vp, u32, u64, u64, u64, _u64p]
        L.iyk_hip_privks_batch.argtypes = [_vp, _vp, _vp, u64, u64, _i32p, _i32p, _vp, u64, _i32p]
        L.iyk_hip_bk2_key_create.argtypes = [ctypes.c_int, u32, u32, u32, ctypes.POINTER(_vp)]
        L.iyk_hip_bk2_key_create_form.argtypes = [ctypes.c_int, u32, u32, u32, ctypes.c_int, ctypes.POINTER(_vp)]
        L.iyk_hip_bk2_key_form.argtypes = [_vp, ctypes.POINTER(ctypes.c_int)]
        L.iyk_hip_bk2_key_upload.argtypes = [_vp, _vp, u64, u64, _u64p]
        L.iyk_hip_bk2_key_upload_seeded.argtypes = [_vp, _vp, ctypes.c_char_p, u64, u64, _u64p]
        L.iyk_hip_bk2_key_free.argtypes = [_vp]
        L.iyk_hip_bk2_key_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(u64)]
        L.iyk_hip_cb_rotate_batch.argtypes = [_vp, _vp, _vp, u64, u64, _i32p, _i32p, _u32p, _u64p, _vp, u64, _i32p]
        L.iyk_hip_cb_rotate_many_batch.argtypes = [_vp, _vp, _vp, u64, u64, _i32p, _i32p, _u32p, u32, _u64p, _vp, u64, _i32p]
        L.iyk_hip_cb_rotate_form.argtypes = [ctypes.c_int, u64, ctypes.POINTER(ctypes.c_int)]
        L.iyk_hip_trgsw_from_rows.argtypes = [_vp, _vp, u64, u64, _i32p, _vp, u64, _i32p]
        L.iyk_hip_circuit_bootstrap_batch.argtypes = [_vp, _vp, _vp, _vp, u64, _i32p, _i32p, _vp, u32, u64, u64, _vp, u64, _vp, u64, u64, u64]
        L.iyk_hip_circuit_bootstrap_many_batch.argtypes = L.iyk_hip_circuit_bootstrap_batch.argtypes
        L.iyk_hip_last_batch_timing.argtypes = [_vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.iyk_hip_resident_key_bytes.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
        L.iyk_hip_level_cost_ms.restype = ctypes.c_double
        L.iyk_hip_level_cost_ms.argtypes = [ctypes.c_int, ctypes.c_int]
        L.iyk_hip_fft_round_error.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        L.iyk_hip_timing_log_begin.argtypes = [_vp]
        L.iyk_hip_timing_log_end.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_double)]
        _LIB = L
    return _LIB


def _check(rc, what):
    if rc < 0:
        raise IykHipError(f"{what} failed ({rc}): {lib().iyk_hip_last_error().decode()}")
    return rc


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def initialize(keys, device_ids=(0,)):
    """cufhe::SetGPUNum(len(device_ids)) + cufhe::Initialize(ek)."""
    ids = (ctypes.c_int * len(device_ids))(*device_ids)
    bk = np.ascontiguousarray(keys.bk, dtype=np.uint32)
    ksk = np.ascontiguousarray(keys.ksk, dtype=np.uint32)
    _check(lib().iyk_hip_init(len(device_ids), ids, ctypes.byref(keys.params),
                              bk.ctypes.data_as(_u32p), ksk.ctypes.data_as(_u32p)), "iyk_hip_init")


def cleanup():
    _check(lib().iyk_hip_cleanup(), "iyk_hip_cleanup")


def is_initialized():
    return bool(lib().iyk_hip_is_initialized())


def resident_key_bytes():
    v = ctypes.c_uint64()
    _check(lib().iyk_hip_resident_key_bytes(ctypes.byref(v)), "iyk_hip_resident_key_bytes")
    return v.value


def ntt_path():
    """'fft' (complex FP64 FFT on 16-bit key halves, exact by a rounding bound: the default), 'fp50' (FP64 FMA field) or
    'goldilocks' (64-bit integer field)."""
    return {2: "fft", 1: "fp50", 0: "goldilocks"}[_check(lib().iyk_hip_ntt_path(), "iyk_hip_ntt_path")]


def fft_round_error(gpu=0):
    """IYK_HIP_DEBUG=1 at init: largest distance from an integer of any inverse-transform output of the FFT kernel so far."""
    v = ctypes.c_double()
    _check(lib().iyk_hip_fft_round_error(int(gpu), ctypes.byref(v)), "iyk_hip_fft_round_error")
    return v.value


def decomposition_levels():
    """Digit polynomials per accumulator polynomial and CMUX step (include/iyokan_hip.h: 3 for the 128-bit set; 80-bit set
    4 by default, 2 with IYK_HIP_DECOMP=direct at init)."""
    return _check(lib().iyk_hip_decomposition_levels(), "iyk_hip_decomposition_levels")


def build_id():
    """Source hash the loaded libiyokan_hip.so was built from (tools/src_hash.py), or 'unknown'."""
    f = lib().iyk_hip_build_id
    f.restype = ctypes.c_char_p
    return f().decode()


def peer_access(gpu_a, gpu_b):
    """True when GPU a reads GPU b's memory directly (peer access enabled at init), False when copies are host-staged."""
    return _check(lib().iyk_hip_peer_access(int(gpu_a), int(gpu_b)), "iyk_hip_peer_access") == 1


class IykLevelCost(ctypes.Structure):
    """include/iyokan_hip.h: iyk_level_cost — what a level of r rotations costs one GPU (the library's only copy)."""
    _fields_ = [("round", ctypes.c_int32), ("pass_", ctypes.c_int32), ("max_passes", ctypes.c_int32),
                ("calibrated", ctypes.c_int32), ("round_ms", ctypes.c_float), ("pass_ms", ctypes.c_float * 8),
                ("build_id", ctypes.c_char * 20)]

    def as_dict(self):
        return {"round": self.round, "pass": self.pass_, "max_passes": self.max_passes, "calibrated": bool(self.calibrated),
                "round_ms": float(self.round_ms), "pass_ms": [float(v) for v in self.pass_ms], "build_id": self.build_id.decode()}


def level_cost_defaults():
    """The compiled-in MI355X cost table of the loaded library (no GPU, no initialisation needed)."""
    c = IykLevelCost()
    _check(lib().iyk_hip_level_cost_defaults(ctypes.byref(c)), "iyk_hip_level_cost_defaults")
    return c.as_dict()


def level_cost_table(gpu=0):
    """GPU `gpu`'s cost table: its CU count, measured milliseconds once calibrate(gpu) has run."""
    c = IykLevelCost()
    _check(lib().iyk_hip_level_cost_table(int(gpu), ctypes.byref(c)), "iyk_hip_level_cost_table")
    return c.as_dict()


def calibrate(gpu=0):
    """~0.15 s self-calibration of the cost table (and of the dispatch's narrow-frontier threshold) on GPU `gpu`;
    gpu = -1: every GPU concurrently (returns GPU 0's table)."""
    _check(lib().iyk_hip_calibrate(int(gpu)), "iyk_hip_calibrate")
    return level_cost_table(max(int(gpu), 0))


def init_profile():
    """Steps of the last iyk_hip_init as [(name, gpu or None, milliseconds)]: alloc g, pin, enqueue g, wait g."""
    L = lib()
    L.iyk_hip_init_profile.restype = ctypes.c_char_p
    out = []
    for item in L.iyk_hip_init_profile().decode().split(";"):
        parts = item.split()
        if len(parts) == 3:
            out.append((parts[0], int(parts[1]), float(parts[2])))
        elif len(parts) == 2:
            out.append((parts[0], None, float(parts[1])))
    return out


def rotation_round(gpu=0):
    """Rotations in one full round of the default wave-per-rotation kernel on GPU `gpu` (resident waves x CUs)."""
    return _check(lib().iyk_hip_rotation_round(int(gpu)), "iyk_hip_rotation_round")


def current_params():
    p = IykParams()
    _check(lib().iyk_hip_get_params(ctypes.byref(p)), "iyk_hip_get_params")
    return p


class Arena:
    """Device-resident array of TLWE lvl0 ciphertexts, addressed by slot index."""

    def __init__(self, slots, gpu_index=0, device_ptr=None, owner=None):
        self.slots, self.gpu_index = int(slots), gpu_index
        self.n1 = current_params().n + 1
        self._owner = owner  # e.g. the torch tensor backing device_ptr
        if device_ptr is None:
            ptr = _vp()
            _check(lib().iyk_hip_arena_alloc(gpu_index, self.slots, ctypes.byref(ptr)), "iyk_hip_arena_alloc")
            self.ptr, self._owned = ptr.value, True
        else:
            self.ptr, self._owned = int(device_ptr), False

    @classmethod
    def from_torch(cls, tensor, gpu_index=0):
        """Wrap a contiguous int32/uint32-sized CUDA tensor of shape (slots, n+1)."""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.element_size() == 4
        return cls(tensor.shape[0], gpu_index, tensor.data_ptr(), owner=tensor)

    def free(self):
        if self._owned and self.ptr:
            _check(lib().iyk_hip_arena_free(self.gpu_index, self.ptr), "iyk_hip_arena_free")
        self.ptr = None

    def __del__(self):
        try:
            if is_initialized():
                self.free()
        except Exception:
            pass


class Trlwe:
    """Device-resident rows of TRLWE lvl1 ciphertexts (2N words each: a(X), then b(X)) — the cells of a ROM / RAM."""

    def __init__(self, slots, gpu_index=0):
        self.slots, self.gpu_index = int(slots), gpu_index
        self.words = 2 * current_params().N
        ptr = _vp()
        _check(lib().iyk_hip_trlwe_alloc(gpu_index, self.slots, ctypes.byref(ptr)), "iyk_hip_trlwe_alloc")
        self.ptr = ptr.value

    def upload(self, stream, first, host):
        host = np.ascontiguousarray(host, dtype=np.uint32).reshape(-1, self.words)
        _check(lib().iyk_hip_trlwe_upload(stream.h, self.ptr, self.slots, first, host.shape[0], host.ctypes.data_as(_u32p)),
               "iyk_hip_trlwe_upload")
        stream.sync()  # host buffer is pageable: finish before it can be garbage collected

    def download(self, stream, first, count):
        out = np.zeros((count, self.words), dtype=np.uint32)
        _check(lib().iyk_hip_trlwe_download(stream.h, self.ptr, self.slots, first, count, out.ctypes.data_as(_u32p)),
               "iyk_hip_trlwe_download")
        stream.sync()
        return out

    def free(self):
        if self.ptr:
            _check(lib().iyk_hip_trlwe_free(self.gpu_index, self.ptr), "iyk_hip_trlwe_free")
        self.ptr = None


class Trgsw:
    """Device-resident TRGSW lvl1 selectors in spectrum form (the TRGSWLvl1FFT inputs of the reference's ROM / RAM tasks)."""

    def __init__(self, slots, gpu_index=0):
        self.slots, self.gpu_index = int(slots), gpu_index
        p = current_params()
        self.words = (p.k + 1) * p.l * (p.k + 1) * p.N   # torus words of one host-side TRGSW
        ptr = _vp()
        _check(lib().iyk_hip_trgsw_alloc(gpu_index, self.slots, ctypes.byref(ptr)), "iyk_hip_trgsw_alloc")
        self.ptr = ptr.value

    def upload(self, stream, first, host):
        """Torus-domain rows u32 [count][(k+1) l][k+1][N] (client.encrypt_trgsw); copied before return, transformed on the stream."""
        host = np.ascontiguousarray(host, dtype=np.uint32).reshape(-1, self.words)
        _check(lib().iyk_hip_trgsw_upload(stream.h, self.ptr, self.slots, first, host.shape[0], host.ctypes.data_as(_u32p)),
               "iyk_hip_trgsw_upload")

    def free(self):
        if self.ptr:
            _check(lib().iyk_hip_trgsw_free(self.gpu_index, self.ptr), "iyk_hip_trgsw_free")
        self.ptr = None


def _mask_seed(mask_seed):
    """the 32 bytes of a key's public mask seed (client.new_mask_seed)"""
    seed = bytes(mask_seed)
    if len(seed) != 32:
        raise ValueError(f"a mask seed is 32 bytes, not {len(seed)}")
    return seed


class PrivKsKey:
    """Device-resident private key-switching key lvl2 -> lvl1 of one GPU: u32 [k+1][n_in+1][t][2^basebit-1][2N] (client.privks_key_rows),
    uploaded in windows of rows."""

    def __init__(self, n_in, t, basebit, gpu_index=0):
        self.n_in, self.t, self.basebit, self.gpu_index = int(n_in), int(t), int(basebit), gpu_index
        p = current_params()
        self.words = 2 * p.N
        self.rows = (p.k + 1) * (self.n_in + 1) * self.t * ((1 << self.basebit) - 1)
        h = _vp()
        _check(lib().iyk_hip_privks_key_create(gpu_index, self.n_in, self.t, self.basebit, ctypes.byref(h)), "iyk_hip_privks_key_create")
        self.h = h

    def upload(self, stream, first_row, host_rows):
        """Rows first_row .. of the host layout; copied before return, ordered on the stream."""
        host = np.ascontiguousarray(host_rows, dtype=np.uint32).reshape(-1, self.words)
        _check(lib().iyk_hip_privks_key_upload(stream.h, self.h, int(first_row), host.shape[0], host.ctypes.data_as(_u32p)),
               "iyk_hip_privks_key_upload")

    def upload_seeded(self, stream, mask_seed, first_row, b_rows):
        """Rows first_row .. of a seeded key: the b halves (rows, N) of client.privks_key_rows(..., mask_seed=) and the key's public
        32-byte mask seed; the a halves are expanded on the GPU.  Copied before return, ordered on the stream."""
        host = np.ascontiguousarray(b_rows, dtype=np.uint32).reshape(-1, self.words // 2)
        _check(lib().iyk_hip_privks_key_upload_seeded(stream.h, self.h, _mask_seed(mask_seed), int(first_row), host.shape[0],
                                                      host.ctypes.data_as(_u32p)), "iyk_hip_privks_key_upload_seeded")

    def free(self):
        if self.h:
            _check(lib().iyk_hip_privks_key_free(self.h), "iyk_hip_privks_key_free")
        self.h = None


def privks_key_bytes(gpu=0):
    """Device bytes of the live private key-switching keys of GPU `gpu`."""
    v = ctypes.c_uint64()
    _check(lib().iyk_hip_privks_key_bytes(int(gpu), ctypes.byref(v)), "iyk_hip_privks_key_bytes")
    return v.value


class Bk2Key:
    """Device-resident lvl2 bootstrapping key of one GPU (the lvl0 -> lvl2 rotation of circuit bootstrapping, Stream.cb_rotate_batch):
    the torus-domain rows u64 [n][(k+1) l2][k+1][N2] of client.bk2_rows, uploaded in windows of steps and transformed on the stream.
    form: "ntt" (the default) is the integer key (Z_P, 512 KiB per step), "fft" the FP64 key (the spectra of the signed 16-bit quarters,
    1 MiB per step, rotated by cb_rotate_fft_kernel); the output words are the same.  Everything that takes a Bk2Key takes either."""
    N2 = 2048
    FORMS = {"ntt": 0, "fft": 1}

    def __init__(self, n, l2=4, Bgbit2=9, gpu_index=0, form="ntt"):
        self.n, self.l2, self.Bgbit2, self.gpu_index = int(n), int(l2), int(Bgbit2), gpu_index
        self.step_words = 2 * self.l2 * 2 * self.N2
        h = _vp()
        if form not in self.FORMS:
            raise ValueError(f"Bk2Key form {form!r}: expected one of {sorted(self.FORMS)}")
        if form == "ntt":
            _check(lib().iyk_hip_bk2_key_create(gpu_index, self.n, self.l2, self.Bgbit2, ctypes.byref(h)), "iyk_hip_bk2_key_create")
        else:
            _check(lib().iyk_hip_bk2_key_create_form(gpu_index, self.n, self.l2, self.Bgbit2, self.FORMS[form], ctypes.byref(h)),
                   "iyk_hip_bk2_key_create_form")
        self.h = h
        v = ctypes.c_int()
        _check(lib().iyk_hip_bk2_key_form(self.h, ctypes.byref(v)), "iyk_hip_bk2_key_form")
        self.form = {c: name for name, c in self.FORMS.items()}[v.value]

    def upload(self, stream, first_step, host_steps):
        """Steps first_step .. of the host layout; copied before return, transformed on the stream."""
        host = np.ascontiguousarray(host_steps, dtype=np.uint64).reshape(-1, self.step_words)
        _check(lib().iyk_hip_bk2_key_upload(stream.h, self.h, int(first_step), host.shape[0], host.ctypes.data_as(_u64p)),
               "iyk_hip_bk2_key_upload")

    def upload_seeded(self, stream, mask_seed, first_step, b_steps):
        """Steps first_step .. of a seeded key: the b halves (steps, (k+1) l2, N2) of client.bk2_rows(..., mask_seed=) and the key's
        public 32-byte mask seed; the a halves are expanded on the GPU ahead of the transform.  Copied before return."""
        host = np.ascontiguousarray(b_steps, dtype=np.uint64).reshape(-1, self.step_words // 2)
        _check(lib().iyk_hip_bk2_key_upload_seeded(stream.h, self.h, _mask_seed(mask_seed), int(first_step), host.shape[0],
                                                   host.ctypes.data_as(_u64p)), "iyk_hip_bk2_key_upload_seeded")

    def free(self):
        if self.h:
            _check(lib().iyk_hip_bk2_key_free(self.h), "iyk_hip_bk2_key_free")
        self.h = None


def bk2_key_bytes(gpu=0):
    """Device bytes of the live lvl2 bootstrapping keys of GPU `gpu`."""
    v = ctypes.c_uint64()
    _check(lib().iyk_hip_bk2_key_bytes(int(gpu), ctypes.byref(v)), "iyk_hip_bk2_key_bytes")
    return v.value


def cb_rotate_form(count, gpu_index=0):
    """The kernel form a Stream.cb_rotate_batch of `count` rotations would run on GPU `gpu_index` now: 0 = cb_rotate_kernel (wide
    batches), 1 = cb_rotate_lat_kernel (narrow ones).  IYK_HIP_CB_KERNEL = wg / lat forces one; any other value is an IykHipError."""
    v = ctypes.c_int()
    _check(lib().iyk_hip_cb_rotate_form(int(gpu_index), int(count), ctypes.byref(v)), "iyk_hip_cb_rotate_form")
    return v.value


class Tlwe2:
    """Device-resident TLWE lvl2 ciphertexts, u64 [slots][n_in + 1]: the inputs of Stream.privks_batch."""

    def __init__(self, n_in, slots, gpu_index=0):
        self.n_in, self.slots, self.gpu_index = int(n_in), int(slots), gpu_index
        self.words = self.n_in + 1
        ptr = _vp()
        _check(lib().iyk_hip_tlwe2_alloc(gpu_index, self.n_in, self.slots, ctypes.byref(ptr)), "iyk_hip_tlwe2_alloc")
        self.ptr = ptr.value

    def upload(self, stream, first, host):
        host = np.ascontiguousarray(host, dtype=np.uint64).reshape(-1, self.words)
        _check(lib().iyk_hip_tlwe2_upload(stream.h, self.ptr, self.n_in, self.slots, first, host.shape[0], host.ctypes.data_as(_u64p)),
               "iyk_hip_tlwe2_upload")
        stream.sync()  # host buffer is pageable: finish before it can be garbage collected

    def download(self, stream, first, count):
        out = np.zeros((count, self.words), dtype=np.uint64)
        _check(lib().iyk_hip_tlwe2_download(stream.h, self.ptr, self.n_in, self.slots, first, count, out.ctypes.data_as(_u64p)),
               "iyk_hip_tlwe2_download")
        stream.sync()
        return out

    def free(self):
        if self.ptr:
            _check(lib().iyk_hip_tlwe2_free(self.gpu_index, self.ptr), "iyk_hip_tlwe2_free")
        self.ptr = None


class Stream:
    """CUFHEStream equivalent (/root/reference/src/iyokan_cufhe.hpp:8-27)."""

    def __init__(self, gpu_index=0, hip_stream=None):
        h = _vp()
        if hip_stream is None:
            _check(lib().iyk_hip_stream_create(gpu_index, ctypes.byref(h)), "iyk_hip_stream_create")
        else:
            _check(lib().iyk_hip_stream_wrap(gpu_index, _vp(int(hip_stream)), ctypes.byref(h)), "iyk_hip_stream_wrap")
        self.h, self.gpu_index = h, gpu_index

    def destroy(self):
        if self.h:
            _check(lib().iyk_hip_stream_destroy(self.h), "iyk_hip_stream_destroy")
            self.h = None

    def query(self):
        """cufhe::StreamQuery: True once everything enqueued so far has finished."""
        return bool(_check(lib().iyk_hip_stream_query(self.h), "iyk_hip_stream_query"))

    def sync(self):
        _check(lib().iyk_hip_stream_sync(self.h), "iyk_hip_stream_sync")

    def wait_stream(self, other):
        """What is enqueued on this stream from now on starts once everything enqueued on `other` (a Stream of the same GPU and
        replica) so far has finished: an event recorded there, waited for here, on the device.  The host does not block.  A refusal
        (IykHipError: the same stream, another GPU or replica, a destroyed stream) enqueues nothing."""
        _check(lib().iyk_hip_stream_wait_stream(self.h, other.h), "iyk_hip_stream_wait_stream")

    def upload(self, arena, first_slot, host):
        host = np.ascontiguousarray(host, dtype=np.uint32).reshape(-1, arena.n1)
        _check(lib().iyk_hip_arena_upload(self.h, arena.ptr, arena.slots, first_slot, host.shape[0],
                                          host.ctypes.data_as(_u32p)), "iyk_hip_arena_upload")
        self.sync()  # host buffer is pageable: finish before it can be garbage collected

    def download(self, arena, first_slot, count):
        out = np.zeros((count, arena.n1), dtype=np.uint32)
        _check(lib().iyk_hip_arena_download(self.h, arena.ptr, arena.slots, first_slot, count,
                                            out.ctypes.data_as(_u32p)), "iyk_hip_arena_download")
        self.sync()
        return out

    def upload_slots(self, arena, slots, host):
        """Mem::set of many cells in one transfer: host row j -> arena slot slots[j]."""
        slots = _i32(slots)
        host = np.ascontiguousarray(host, dtype=np.uint32).reshape(len(slots), arena.n1)
        _check(lib().iyk_hip_arena_upload_slots(self.h, arena.ptr, arena.slots, len(slots), slots.ctypes.data_as(_i32p),
                                                host.ctypes.data_as(_u32p)), "iyk_hip_arena_upload_slots")

    def download_slots(self, arena, slots):
        """Mem::get of many cells in one transfer."""
        slots = _i32(slots)
        out = np.zeros((len(slots), arena.n1), dtype=np.uint32)
        _check(lib().iyk_hip_arena_download_slots(self.h, arena.ptr, arena.slots, len(slots),
                                                  slots.ctypes.data_as(_i32p), out.ctypes.data_as(_u32p)),
               "iyk_hip_arena_download_slots")
        self.sync()
        return out

    def arena_copy(self, dst, dst_first, src, src_first, count):
        _check(lib().iyk_hip_arena_copy(self.h, dst.ptr, dst.slots, dst_first, src.ptr, src.slots, src_first, count),
               "iyk_hip_arena_copy")

    def sync_slots_to(self, src_arena, dst_stream, dst_arena, slots):
        """Level-boundary exchange between in-process GPU replicas: listed slots of src_arena (this stream's GPU)
        -> same slots of dst_arena (dst_stream's GPU), ordered by events on both streams."""
        slots = _i32(slots)
        _check(lib().iyk_hip_arena_sync_slots(self.h, src_arena.ptr, src_arena.slots, dst_stream.h, dst_arena.ptr,
                                              dst_arena.slots, len(slots), slots.ctypes.data_as(_i32p)),
               "iyk_hip_arena_sync_slots")

    def sync_slots_to_many(self, src_arena, dst_streams, dst_arenas, slots):
        """The same with ONE gather on this stream's GPU and several destination replicas (iyk_hip_arena_sync_slots_multi)."""
        slots = _i32(slots)
        n = len(dst_streams)
        assert n == len(dst_arenas)
        sts = (_vp * n)(*[s.h for s in dst_streams])
        ptrs = (_vp * n)(*[a.ptr for a in dst_arenas])
        caps = (ctypes.c_uint64 * n)(*[a.slots for a in dst_arenas])
        _check(lib().iyk_hip_arena_sync_slots_multi(self.h, src_arena.ptr, src_arena.slots, n, sts, ptrs, caps, len(slots),
                                                    slots.ctypes.data_as(_i32p)), "iyk_hip_arena_sync_slots_multi")

    def gate_batch(self, arena, ops, in0, in1, in2, out, lanes=1, lane_stride=None):
        """`len(ops)` independent gates on arena slots; asynchronous (poll query() / sync()).
        lanes / lane_stride given: the gates on `lanes` copies of the circuit's arena image, lane r in slots [r * lane_stride,
        (r + 1) * lane_stride) — the descriptors are ONE lane's (iyk_hip_gate_batch_lanes; lane_stride None: arena.slots // lanes)."""
        ops, in0, in1, in2, out = map(_i32, (ops, in0, in1, in2, out))
        n = len(ops)
        assert len(in0) == len(in1) == len(in2) == len(out) == n
        p = lambda a: a.ctypes.data_as(_i32p)
        if lanes == 1 and lane_stride is None:
            _check(lib().iyk_hip_gate_batch(self.h, arena.ptr, arena.slots, n, p(ops), p(in0), p(in1), p(in2), p(out)),
                   "iyk_hip_gate_batch")
            return
        if not hasattr(lib(), "iyk_hip_gate_batch_lanes"):
            raise IykHipError(f"{LIB_PATH} has no iyk_hip_gate_batch_lanes: it was built before lane batches — rebuild it")
        if lane_stride is None:
            lane_stride = arena.slots // lanes if lanes > 0 else 0
        _check(lib().iyk_hip_gate_batch_lanes(self.h, arena.ptr, arena.slots, n, p(ops), p(in0), p(in1), p(in2), p(out), int(lanes),
                                              int(lane_stride)), "iyk_hip_gate_batch_lanes")

    def gate_host(self, op, in0=None, in1=None, in2=None):
        """cufhe::Nand(out, in0, in1, st) shape: host in, host out (synchronised here)."""
        n1 = current_params().n + 1
        out = np.zeros(n1, dtype=np.uint32)
        args = [None if a is None else np.ascontiguousarray(a, dtype=np.uint32) for a in (in0, in1, in2)]
        ptr = lambda a: a.ctypes.data_as(_u32p) if a is not None else None
        code = OPS[op] if isinstance(op, str) else int(op)
        _check(lib().iyk_hip_gate_host(self.h, code, ptr(args[0]), ptr(args[1]), ptr(args[2]),
                                       out.ctypes.data_as(_u32p)), "iyk_hip_gate_host")
        self.sync()
        return out

    def blind_rotate_batch(self, arena, ia, ib, sa, sb, off, d_tlwe1_ptr):
        ia, ib, sa, sb = map(_i32, (ia, ib, sa, sb))
        off = np.ascontiguousarray(off, dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(_i32p)
        _check(lib().iyk_hip_blind_rotate_batch(self.h, arena.ptr, arena.slots, len(ia), p(ia), p(ib), p(sa), p(sb),
                                                off.ctypes.data_as(_u32p), _vp(int(d_tlwe1_ptr))),
               "iyk_hip_blind_rotate_batch")

    def bootstrap_trlwe_batch(self, arena, ia, ib, sa, sb, off, d_trlwe_ptr, trlwe_slots=None, trlwe_out=None):
        """GateBootstrappingTLWE2TRLWElvl01NTT shape: rotation only, TRLWE (2N words) per job, written to row
        trlwe_out[job] of the TRLWE buffer (row `job` when trlwe_out is None)."""
        ia, ib, sa, sb = map(_i32, (ia, ib, sa, sb))
        off = np.ascontiguousarray(off, dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(_i32p)
        to = None if trlwe_out is None else _i32(trlwe_out)
        _check(lib().iyk_hip_bootstrap_trlwe_batch(self.h, arena.ptr, arena.slots, len(ia), p(ia), p(ib), p(sa), p(sb),
                                                   off.ctypes.data_as(_u32p), _vp(int(d_trlwe_ptr)),
                                                   len(ia) if trlwe_slots is None else int(trlwe_slots),
                                                   None if to is None else p(to)),
               "iyk_hip_bootstrap_trlwe_batch")

    def sample_extract_keyswitch_batch(self, d_trlwe_ptr, trlwe_index, out_slot, arena, trlwe_slots=None):
        """SampleExtractAndKeySwitch shape: TRLWE -> TLWE lvl0 into arena slots."""
        ti, os_ = _i32(trlwe_index), _i32(out_slot)
        p = lambda a: a.ctypes.data_as(_i32p)
        nt = (int(ti.max()) + 1 if len(ti) else 0) if trlwe_slots is None else int(trlwe_slots)
        _check(lib().iyk_hip_sample_extract_keyswitch_batch(self.h, _vp(int(d_trlwe_ptr)), nt, len(ti), p(ti), p(os_),
                                                            arena.ptr, arena.slots),
               "iyk_hip_sample_extract_keyswitch_batch")

    def sample_extract_index_keyswitch_batch(self, trlwe, trlwe_index, coeff_index, out_slot, arena):
        """TaskTFHEppSEI shape: coefficient coeff_index[g] of row trlwe_index[g] of a Trlwe store -> TLWE lvl0 in arena slot out_slot[g]."""
        ti, ci, os_ = _i32(trlwe_index), _i32(coeff_index), _i32(out_slot)
        assert len(ti) == len(ci) == len(os_)
        p = lambda a: a.ctypes.data_as(_i32p)
        _check(lib().iyk_hip_sample_extract_index_keyswitch_batch(self.h, trlwe.ptr, trlwe.slots, len(ti), p(ti), p(ci), p(os_),
                                                                  arena.ptr, arena.slots),
               "iyk_hip_sample_extract_index_keyswitch_batch")

    def _cmux_call(self, name, trgsw, trlwe, count, arrays, lanes, sel_stride, row_stride):
        """iyk_hip_<name>, or iyk_hip_<name>_lanes where lanes / strides are given: the arrays are ONE lane's, lane r's selector slots are
        + r * sel_stride and its rows + r * row_stride (csrc/cmux_lane_jobs.hpp)."""
        head = (self.h, trgsw.ptr, trgsw.slots, trlwe.ptr, trlwe.slots, count) + tuple(arrays)
        if lanes == 1 and sel_stride is None and row_stride is None:
            _check(getattr(lib(), "iyk_hip_" + name)(*head), "iyk_hip_" + name)
            return
        f = "iyk_hip_" + name + "_lanes"
        if not hasattr(lib(), f):
            raise IykHipError(f"{LIB_PATH} has no {f}: it was built before CMUX memories had lanes — rebuild it")
        if not 0 <= int(lanes) < 1 << 32:
            raise ValueError(f"lanes {lanes} outside [0, 2^32)")
        _check(getattr(lib(), f)(*head, int(lanes), int(sel_stride or 0), int(row_stride or 0)), f)

    def cmux_batch(self, trgsw, trlwe, sel, in0, in1, rot, out, lanes=1, sel_stride=None, row_stride=None):
        """len(sel) independent CMUXes on rows of a Trlwe store, asynchronous: T[out] = T[in0] + S[sel] [.] (T[in1] - T[in0]) where
        in1 >= 0 (a selector of 1 selects in1), T[in0] + S[sel] [.] ((X^rot - 1) T[in0]) where in1 < 0.  A job may write over its
        own inputs; no out may be an input or the out of another job of the batch."""
        sel, in0, in1, rot, out = map(_i32, (sel, in0, in1, rot, out))
        assert len(in0) == len(in1) == len(rot) == len(out) == len(sel)
        p = lambda a: a.ctypes.data_as(_i32p)
        self._cmux_call("cmux_batch", trgsw, trlwe, len(sel), (p(sel), p(in0), p(in1), p(rot), p(out)), lanes, sel_stride, row_stride)

    def cmux_chain_batch(self, trgsw, trlwe, sel0, steps, pattern, src, mem, out, lanes=1, sel_stride=None, row_stride=None):
        """len(sel0) independent chains of CMUXes on rows of a Trlwe store, asynchronous (the RAM write-back of one cell per job):
        acc = T[src]; for j < steps, with S = selector slot sel0 + j: acc = T[mem] + S [.] (acc - T[mem]) where bit j of pattern is 1,
        acc + S [.] (T[mem] - acc) where it is 0; T[out] = acc.  Word for word what `steps` dependent cmux_batch jobs give.  A job may
        write over its own src or mem; no out may be the src / mem / out of another job of the batch."""
        sel0, steps, src, mem, out = map(_i32, (sel0, steps, src, mem, out))
        pattern = np.ascontiguousarray(pattern, dtype=np.uint32)
        assert len(steps) == len(pattern) == len(src) == len(mem) == len(out) == len(sel0)
        p = lambda a: a.ctypes.data_as(_i32p)
        self._cmux_call("cmux_chain_batch", trgsw, trlwe, len(sel0), (p(sel0), p(steps), pattern.ctypes.data_as(_u32p), p(src), p(mem), p(out)),
                        lanes, sel_stride, row_stride)

    def cmux_rotate_chain_batch(self, trgsw, trlwe, steps, sel, rot, src, out, lanes=1, sel_stride=None, row_stride=None):
        """len(steps) independent chains of rotate-form CMUXes on rows of a Trlwe store, asynchronous (the lower half of one ROM read
        per job): acc = T[src]; for j < steps[g]: acc = acc + S[sel_j] [.] ((X^rot_j - 1) acc); T[out] = acc.  sel and rot hold the jobs'
        steps one after the other, sum(steps) entries.  Word for word what steps[g] dependent cmux_batch rotate jobs give.  A job may
        write over its own src and jobs may share src; no out may be the src / out of another job of the batch."""
        steps, sel, rot, src, out = map(_i32, (steps, sel, rot, src, out))
        assert len(steps) == len(src) == len(out) and len(sel) == len(rot)
        # the library reads the entries of the jobs in front of the first steps[g] it refuses, never more: they must be there
        bad = np.flatnonzero((steps < 1) | (steps > 32))
        need = int(steps[: bad[0] if len(bad) else len(steps)].sum())
        if need > len(sel) or (not len(bad) and need != len(sel)):
            raise ValueError(f"sel and rot hold {len(sel)} steps, the jobs state {need}")
        p = lambda a: a.ctypes.data_as(_i32p)
        self._cmux_call("cmux_rotate_chain_batch", trgsw, trlwe, len(steps), (p(steps), p(sel), p(rot), p(src), p(out)), lanes, sel_stride, row_stride)

    def cmux_tree_batch(self, trgsw, trlwe, sel0, levels, first, out, lanes=1, sel_stride=None, row_stride=None):
        """len(sel0) independent CMUX read trees on rows of a Trlwe store, asynchronous (up to four levels of the upper half of one memory
        read per job): the 2^levels[g] leaves T[first[g] ..] are halved levels[g] times — level b takes selector slot sel0[g] + b, and job i
        of a level is the CMUX (in0 = candidate 2 i, in1 = candidate 2 i + 1) — and T[out[g]] is the row left.  Word for word what
        levels[g] dependent cmux_batch launches give; nothing but out is written.  A job may write over one of its own leaves and jobs
        may share leaves; no out may be a leaf or the out of another job of the batch."""
        sel0, levels, first, out = map(_i32, (sel0, levels, first, out))
        assert len(sel0) == len(levels) == len(first) == len(out)
        p = lambda a: a.ctypes.data_as(_i32p)
        self._cmux_call("cmux_tree_batch", trgsw, trlwe, len(sel0), (p(sel0), p(levels), p(first), p(out)), lanes, sel_stride, row_stride)

    def trlwe_add_batch(self, trlwe, a, b, out, b0_offset=0):
        """T[out] = T[a] + T[b] mod 2^32 on rows of a Trlwe store, b0_offset added to coefficient 0 of the b polynomial (the tail of
        HomMUXwoSE with b0_offset = mu); asynchronous.  out may be a or b of its own job, never a row of another job."""
        a, b, out = map(_i32, (a, b, out))
        assert len(a) == len(b) == len(out)
        p = lambda x: x.ctypes.data_as(_i32p)
        _check(lib().iyk_hip_trlwe_add_batch(self.h, trlwe.ptr, trlwe.slots, len(a), p(a), p(b), p(out),
                                             ctypes.c_uint32(int(b0_offset) & 0xFFFFFFFF)), "iyk_hip_trlwe_add_batch")

    def privks_batch(self, key, tlwe2, in_, c, trlwe, out):
        """len(in_) private key switches, asynchronous: row out[g] of a Trlwe store = R_{c[g]} of TLWE in_[g] of a Tlwe2 store under a
        PrivKsKey — a TRLWE of phase f_c (b - <a, s2>) / 2^32, f_1 = 1, f_0 = -s1(X).  No two jobs may write the same row."""
        in_, c, out = map(_i32, (in_, c, out))
        assert len(in_) == len(c) == len(out)
        if tlwe2.n_in != key.n_in:
            raise ValueError(f"the store holds TLWEs of n_in = {tlwe2.n_in}, the key switches n_in = {key.n_in}")
        p = lambda a: a.ctypes.data_as(_i32p)
        _check(lib().iyk_hip_privks_batch(self.h, key.h, tlwe2.ptr, tlwe2.slots, len(in_), p(in_), p(c), trlwe.ptr, trlwe.slots, p(out)),
               "iyk_hip_privks_batch")

    def cb_rotate_batch(self, key, arena, in_, sign, off, mu, tlwe2, out):
        """len(in_) lvl0 -> lvl2 blind rotations, asynchronous: slot out[g] of a Tlwe2 store of n_in = 2048 = a lvl2 TLWE of 2 mu[g] where
        the phase of sign[g] * arena[in_[g]] + (0, off[g]) is positive, of 0 where it is negative, under a Bk2Key.  `arena` holds TLWEs
        of key.n + 1 words (the arena, or Arena.from_torch of a (slots, key.n + 1) tensor).  No two jobs may write the same slot."""
        in_, sign, out = map(_i32, (in_, sign, out))
        off = np.ascontiguousarray(np.asarray(off, dtype=np.uint64) & np.uint64(0xFFFFFFFF), dtype=np.uint32)
        mu = np.ascontiguousarray(mu, dtype=np.uint64)
        assert len(in_) == len(sign) == len(off) == len(mu) == len(out)
        if tlwe2.n_in != key.N2:
            raise ValueError(f"the store holds TLWEs of n_in = {tlwe2.n_in}, the rotation writes n_in = {key.N2}")
        p = lambda a: a.ctypes.data_as(_i32p)
        _check(lib().iyk_hip_cb_rotate_batch(self.h, key.h, arena.ptr, arena.slots, len(in_), p(in_), p(sign), off.ctypes.data_as(_u32p),
                                             mu.ctypes.data_as(_u64p), tlwe2.ptr, tlwe2.slots, p(out)), "iyk_hip_cb_rotate_batch")

    def cb_rotate_many_batch(self, key, arena, in_, sign, off, mu, tlwe2, out):
        """The many-digit form of cb_rotate_batch: ONE rotation per job gives the l = len(mu) lvl2 TLWEs of the constants mu[0 .. l), shared
        by the batch — slot out[g] + r of the Tlwe2 store = a TLWE of 2 mu[r] where the phase of sign[g] * arena[in_[g]] + (0, off[g]) is
        positive, of 0 where it is negative.  1 <= l <= 4; no two jobs' ranges out[g] .. out[g] + l - 1 may overlap.  l = 1 gives
        cb_rotate_batch's words; for l > 1 the mod switch is coarser."""
        in_, sign, out = map(_i32, (in_, sign, out))
        off = np.ascontiguousarray(np.asarray(off, dtype=np.uint64) & np.uint64(0xFFFFFFFF), dtype=np.uint32)
        mu = np.ascontiguousarray(mu, dtype=np.uint64).ravel()
        assert len(in_) == len(sign) == len(off) == len(out)
        if tlwe2.n_in != key.N2:
            raise ValueError(f"the store holds TLWEs of n_in = {tlwe2.n_in}, the rotation writes n_in = {key.N2}")
        p = lambda a: a.ctypes.data_as(_i32p)
        _check(lib().iyk_hip_cb_rotate_many_batch(self.h, key.h, arena.ptr, arena.slots, len(in_), p(in_), p(sign), off.ctypes.data_as(_u32p),
                                                  len(mu), mu.ctypes.data_as(_u64p), tlwe2.ptr, tlwe2.slots, p(out)),
               "iyk_hip_cb_rotate_many_batch")

    def trgsw_from_rows(self, trgsw, out_slot, trlwe, rows):
        """Selector out_slot[g] of a Trgsw store from the (k+1) l torus-domain rows rows[g] of a Trlwe store (row order c l + r), on the
        device: the twin of Trgsw.upload for rows that never were on the host.  Asynchronous."""
        out_slot = _i32(out_slot).ravel()
        rows = _i32(rows).reshape(len(out_slot), -1)
        p = current_params()
        if rows.shape[1] != (p.k + 1) * p.l:
            raise ValueError(f"expected {(p.k + 1) * p.l} rows per selector, got {rows.shape[1]}")
        q = lambda a: a.ctypes.data_as(_i32p)
        _check(lib().iyk_hip_trgsw_from_rows(self.h, trgsw.ptr, trgsw.slots, len(out_slot), q(out_slot), trlwe.ptr, trlwe.slots, q(rows)),
               "iyk_hip_trgsw_from_rows")

    def circuit_bootstrap_batch(self, bk2, privks_key, arena, in_, sign, tlwe2, first, trlwe_scratch, trgsw, first_slot=0):
        """The selectors of len(in_) address bits from their lvl0 TLWEs (arena slot in_[bit], sign[bit] = -1: of the negated bit) into
        slots first_slot .. of a Trgsw store, as ONE checked call: what cmux.selectors_from_tlwe0 composes of cb_rotate_batch, privks_batch
        and trgsw_from_rows, with the same lvl2 slots (first + bit l + r) and scratch rows.  Every argument of all three is checked
        before the first launch; a refusal (IykHipError) launches nothing and changes no store.  Asynchronous."""
        in_, sign = _i32(in_).ravel(), _i32(sign).ravel()
        if len(in_) != len(sign):
            raise ValueError(f"{len(in_)} input slots, {len(sign)} signs")
        p = lambda a: a.ctypes.data_as(_i32p)
        _check(lib().iyk_hip_circuit_bootstrap_batch(self.h, bk2.h, privks_key.h, arena.ptr, arena.slots, p(in_), p(sign), tlwe2.ptr,
                                                     tlwe2.n_in, tlwe2.slots, int(first), trlwe_scratch.ptr, trlwe_scratch.slots, trgsw.ptr,
                                                     trgsw.slots, int(first_slot), len(in_)), "iyk_hip_circuit_bootstrap_batch")

    def circuit_bootstrap_many_batch(self, bk2, privks_key, arena, in_, sign, tlwe2, first, trlwe_scratch, trgsw, first_slot=0):
        """circuit_bootstrap_batch with the many-digit rotation: one rotation per address bit instead of l, the same arguments, checks,
        lvl2 slots, scratch rows and selector slots; cb_rotate_many_batch, privks_batch and trgsw_from_rows as ONE checked call."""
        in_, sign = _i32(in_).ravel(), _i32(sign).ravel()
        if len(in_) != len(sign):
            raise ValueError(f"{len(in_)} input slots, {len(sign)} signs")
        p = lambda a: a.ctypes.data_as(_i32p)
        _check(lib().iyk_hip_circuit_bootstrap_many_batch(self.h, bk2.h, privks_key.h, arena.ptr, arena.slots, p(in_), p(sign), tlwe2.ptr,
                                                          tlwe2.n_in, tlwe2.slots, int(first), trlwe_scratch.ptr, trlwe_scratch.slots,
                                                          trgsw.ptr, trgsw.slots, int(first_slot), len(in_)),
               "iyk_hip_circuit_bootstrap_many_batch")

    def last_batch_timing(self):
        """(blind_rotate_ms, keyswitch_ms) of the most recent batch, from HIP events on this stream."""
        br, ks = ctypes.c_float(), ctypes.c_float()
        _check(lib().iyk_hip_last_batch_timing(self.h, ctypes.byref(br), ctypes.byref(ks)),
               "iyk_hip_last_batch_timing")
        return br.value, ks.value

    def timing_log_begin(self):
        _check(lib().iyk_hip_timing_log_begin(self.h), "iyk_hip_timing_log_begin")

    def timing_log_end(self):
        """(batches, blind_rotate_ms_total, keyswitch_ms_total) since timing_log_begin(); synchronises."""
        nb, br, ks = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
        _check(lib().iyk_hip_timing_log_end(self.h, ctypes.byref(nb), ctypes.byref(br), ctypes.byref(ks)),
               "iyk_hip_timing_log_end")
        return nb.value, br.value, ks.value
