"""Foreign device arrays -- a training framework's tensors in HBM -- handed to the engine by protocol, without a copy.

The primary route is DLPack (`__dlpack__` / `__dlpack_device__`: PyTorch, CuPy and JAX provide it); `__cuda_array_interface__` v3 is the
fall-back.  This module imports no framework: it parses the legacy `DLManagedTensor` capsule with ctypes and keeps the capsule itself (not
renamed, so that its destructor still returns the tensor to its owner) as the keep-alive of the memory.

`ForeignArray` is what the rest of the package sees: device pointer, dtype name, shape, element count, and `keep` (the object that holds
the memory).  Every refusal raises before any stream work happens and names its reason: wrong device type or index, non-contiguous,
misaligned, unsupported dtype, read-only output (cuda-array-interface), and a tensor that requires grad (the framework's own error).
"""
import ctypes

import numpy as np

__all__ = ["ForeignArray", "is_foreign", "parse_dlpack_capsule", "parse_cuda_array_interface", "from_dlpack_object", "from_cai_object",
           "as_foreign", "KDL_CPU", "KDL_CUDA", "KDL_ROCM"]

KDL_CPU, KDL_CUDA, KDL_ROCM = 1, 2, 10

# DLDataTypeCode: kDLInt 0, kDLUInt 1, kDLFloat 2, kDLBfloat 4
_DL_DTYPES = {(0, 8): "int8", (0, 16): "int16", (0, 32): "int32", (0, 64): "int64", (1, 8): "uint8", (1, 16): "uint16", (1, 32): "uint32",
              (1, 64): "uint64", (2, 16): "float16", (2, 32): "float32", (2, 64): "float64", (4, 16): "bfloat16"}
_ITEMSIZE = {"int8": 1, "int16": 2, "int32": 4, "int64": 8, "uint8": 1, "uint16": 2, "uint32": 4, "uint64": 8, "float16": 2, "float32": 4,
             "float64": 8, "bfloat16": 2}
# __cuda_array_interface__ typestr (byte order '<' or '|') -> dtype name
_CAI_DTYPES = {"i1": "int8", "i2": "int16", "i4": "int32", "i8": "int64", "u1": "uint8", "u2": "uint16", "u4": "uint32", "u8": "uint64",
               "f2": "float16", "f4": "float32", "f8": "float64"}


class _DLDevice(ctypes.Structure):
    _fields_ = [("device_type", ctypes.c_int32), ("device_id", ctypes.c_int32)]


class _DLDataType(ctypes.Structure):
    _fields_ = [("code", ctypes.c_uint8), ("bits", ctypes.c_uint8), ("lanes", ctypes.c_uint16)]


class _DLTensor(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("device", _DLDevice), ("ndim", ctypes.c_int32), ("dtype", _DLDataType),
                ("shape", ctypes.POINTER(ctypes.c_int64)), ("strides", ctypes.POINTER(ctypes.c_int64)), ("byte_offset", ctypes.c_uint64)]


class _DLManagedTensor(ctypes.Structure):
    _fields_ = [("dl_tensor", _DLTensor), ("manager_ctx", ctypes.c_void_p), ("deleter", ctypes.c_void_p)]


_PyCapsule_IsValid = ctypes.pythonapi.PyCapsule_IsValid
_PyCapsule_IsValid.restype = ctypes.c_int
_PyCapsule_IsValid.argtypes = [ctypes.py_object, ctypes.c_char_p]
_PyCapsule_GetPointer = ctypes.pythonapi.PyCapsule_GetPointer
_PyCapsule_GetPointer.restype = ctypes.c_void_p
_PyCapsule_GetPointer.argtypes = [ctypes.py_object, ctypes.c_char_p]


class ForeignArray(object):
    """A C-contiguous array in device memory that the engine reads or writes in place.  ptr: address of element 0 (byte_offset applied);
    dtype: a name of _ITEMSIZE; keep: holds the memory alive (the DLPack capsule, or the producer object)."""

    def __init__(self, ptr, dtype, shape, device_type, device_id, keep, readonly=False, stream=None, source="dlpack"):
        self.ptr, self.dtype, self.shape = int(ptr or 0), dtype, tuple(int(v) for v in shape)
        self.device_type, self.device_id = int(device_type), int(device_id)
        self.keep, self.readonly, self.stream, self.source = keep, bool(readonly), stream, source

    @property
    def itemsize(self):
        return _ITEMSIZE[self.dtype]

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1

    @property
    def nbytes(self):
        return self.size * self.itemsize

    def __repr__(self):
        return f"ForeignArray({self.dtype}{list(self.shape)} at 0x{self.ptr:x}, device {self.device_type}:{self.device_id})"


def _check_contiguous(shape, strides, itemsize, what):
    """strides in ELEMENTS (None = C-contiguous); a dimension of extent 1 may carry any stride."""
    if strides is None:
        return
    expect = 1
    for ext, st in zip(reversed(shape), reversed(strides)):
        if ext != 1 and st != expect:
            raise ValueError(f"{what}: only C-contiguous arrays are accepted (shape {tuple(shape)}, strides {tuple(strides)} elements); "
                             "pass .contiguous() / a copy")
        expect *= ext


def _check_aligned(ptr, itemsize, what):
    if ptr % itemsize:
        raise ValueError(f"{what}: the data pointer 0x{ptr:x} is not aligned to the element size ({itemsize} bytes)")


def parse_dlpack_capsule(capsule, keep=None):
    """-> ForeignArray of a legacy "dltensor" capsule (the capsule is NOT consumed or renamed: it stays the owner of the memory and is
    kept in .keep).  Checks dtype, lanes, C-contiguity and alignment; not the device."""
    if not _PyCapsule_IsValid(capsule, b"dltensor"):
        raise TypeError("expected a DLPack capsule named 'dltensor' (the legacy DLManagedTensor); got a used or versioned one")
    addr = _PyCapsule_GetPointer(capsule, b"dltensor")
    t = _DLManagedTensor.from_address(addr).dl_tensor
    code, bits, lanes = int(t.dtype.code), int(t.dtype.bits), int(t.dtype.lanes)
    if lanes != 1 or (code, bits) not in _DL_DTYPES:
        raise TypeError(f"unsupported DLPack dtype (code {code}, bits {bits}, lanes {lanes})")
    dtype = _DL_DTYPES[(code, bits)]
    ndim = int(t.ndim)
    shape = [int(t.shape[i]) for i in range(ndim)]
    strides = [int(t.strides[i]) for i in range(ndim)] if ndim and bool(t.strides) else None
    _check_contiguous(shape, strides, _ITEMSIZE[dtype], "DLPack tensor")
    ptr = (int(t.data or 0) + int(t.byte_offset))
    if int(np.prod(shape, dtype=np.int64) if shape else 1):
        _check_aligned(ptr, _ITEMSIZE[dtype], "DLPack tensor")
    return ForeignArray(ptr, dtype, shape, t.device.device_type, t.device.device_id, keep if keep is not None else capsule)


def parse_cuda_array_interface(cai, owner=None):
    """-> ForeignArray of a __cuda_array_interface__ dict (v2 / v3): shape, typestr, data = (ptr, readonly), strides in BYTES (None =
    C-contiguous), stream (None, or the producer's stream as an int: 1 legacy default, 2 per-thread default).  The device is not part of
    the protocol: device_id -1 (the caller's)."""
    if cai.get("mask") is not None:
        raise TypeError("masked __cuda_array_interface__ arrays are not supported")
    typestr = str(cai["typestr"])
    if typestr[:1] not in "<|" or typestr[1:] not in _CAI_DTYPES:
        raise TypeError(f"unsupported __cuda_array_interface__ typestr {typestr!r}")
    dtype = _CAI_DTYPES[typestr[1:]]
    isz = _ITEMSIZE[dtype]
    shape = [int(v) for v in cai["shape"]]
    strides = cai.get("strides")
    if strides is not None:
        if any(int(s) % isz for s in strides):
            raise ValueError("__cuda_array_interface__: strides are not whole elements; only C-contiguous arrays are accepted")
        strides = [int(s) // isz for s in strides]
    _check_contiguous(shape, strides, isz, "__cuda_array_interface__ array")
    ptr, readonly = cai["data"]
    ptr = int(ptr or 0)
    if int(np.prod(shape, dtype=np.int64) if shape else 1):
        _check_aligned(ptr, isz, "__cuda_array_interface__ array")
    stream = cai.get("stream")
    if stream is not None:
        stream = int(stream)
        if stream == 0:
            raise ValueError("__cuda_array_interface__: stream 0 is disallowed by the protocol (use 1 for the legacy default stream)")
    return ForeignArray(ptr, dtype, shape, KDL_ROCM, -1, owner if owner is not None else cai, readonly=readonly, stream=stream,
                        source="cai")


def is_foreign(obj):
    """A framework array the engine can take by protocol (a NumPy array is not one: it stays on the host path)."""
    if isinstance(obj, np.ndarray):
        return False
    return hasattr(obj, "__dlpack__") and hasattr(obj, "__dlpack_device__") or hasattr(obj, "__cuda_array_interface__")


def _device_check(dev_type, dev_id, device):
    if dev_type != KDL_ROCM:
        name = {KDL_CPU: "CPU", KDL_CUDA: "CUDA"}.get(dev_type, str(dev_type))
        raise ValueError(f"the array lives on DLPack device type {name} ({dev_type}); this engine takes ROCm device memory (kDLROCM = 10) only")
    if dev_id != int(device):
        raise ValueError(f"the array lives on device {dev_id}, this engine on device {device}")


def from_dlpack_object(obj, device, stream):
    """DLPack handshake: __dlpack_device__() checked first (no stream work for a refused array), then __dlpack__(stream=stream) so that
    the producer orders its pending writes before work on `stream` (the engine's hipStream_t as an int)."""
    dev_type, dev_id = obj.__dlpack_device__()
    _device_check(int(dev_type), int(dev_id), device)
    capsule = obj.__dlpack__(stream=int(stream) if stream else None)
    fa = parse_dlpack_capsule(capsule)
    _device_check(fa.device_type, fa.device_id, device)
    return fa


def from_cai_object(obj):
    return parse_cuda_array_interface(obj.__cuda_array_interface__, owner=obj)


def as_foreign(obj, device, stream):
    """DLPack when the object speaks it, else __cuda_array_interface__.  `stream` is the consumer's stream for the DLPack handshake; a
    cuda-array-interface `stream` is returned in .stream for the consumer to wait on."""
    if hasattr(obj, "__dlpack__") and hasattr(obj, "__dlpack_device__"):
        return from_dlpack_object(obj, device, stream)
    if hasattr(obj, "__cuda_array_interface__"):
        return from_cai_object(obj)
    raise TypeError(f"{type(obj).__name__} exposes neither __dlpack__ nor __cuda_array_interface__")
