"""CPU-only: the foreign-array protocols of flashe_amd/interop.py (DLPack capsules parsed with ctypes, __cuda_array_interface__ dicts) and
the summation rule flashe_store_layers_dev follows for unnormalize's statistics -- NumPy's own np.sum of a C-contiguous float64 array,
emulated here in Python and compared with np.sum / np.mean / np.std bit for bit.  If a future NumPy changes its rule, this file fails
first and says so."""
import ctypes
import sys

import numpy as np
import pytest

from flashe_amd import interop


# ---------------------------------------------------------------- DLPack capsules
def test_dlpack_capsule_of_numpy_arrays():
    a = np.arange(12, dtype=np.int64).reshape(3, 4)
    fa = interop.parse_dlpack_capsule(a.__dlpack__())
    assert (fa.dtype, fa.shape, fa.ptr, fa.device_type) == ("int64", (3, 4), a.ctypes.data, interop.KDL_CPU)
    assert fa.size == 12 and fa.nbytes == 96
    for dt, name in ((np.uint64, "uint64"), (np.uint32, "uint32"), (np.int32, "int32"), (np.float32, "float32"), (np.float16, "float16"),
                     (np.float64, "float64")):
        b = np.zeros(5, dtype=dt)
        assert interop.parse_dlpack_capsule(b.__dlpack__()).dtype == name
    sl = np.arange(10, dtype=np.float64)[3:]                         # a view: its pointer is element 3
    assert interop.parse_dlpack_capsule(sl.__dlpack__()).ptr == sl.ctypes.data
    with pytest.raises(ValueError, match="C-contiguous"):
        interop.parse_dlpack_capsule(np.arange(10, dtype=np.float64)[::2].__dlpack__())
    with pytest.raises(ValueError, match="C-contiguous"):
        interop.parse_dlpack_capsule(np.zeros((3, 4), dtype=np.float32).T.__dlpack__())
    with pytest.raises(TypeError, match="unsupported DLPack dtype"):
        interop.parse_dlpack_capsule(np.zeros(3, dtype=np.complex64).__dlpack__())


def test_dlpack_capsule_of_torch_cpu_tensors():
    torch = pytest.importorskip("torch")
    t = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    fa = interop.parse_dlpack_capsule(t.__dlpack__())
    assert (fa.dtype, fa.shape, fa.ptr, fa.device_type) == ("float32", (2, 3, 4), t.data_ptr(), interop.KDL_CPU)
    bf = torch.zeros(7, dtype=torch.bfloat16)
    fb = interop.parse_dlpack_capsule(bf.__dlpack__())
    assert (fb.dtype, fb.shape, fb.itemsize) == ("bfloat16", (7,), 2)
    assert interop.parse_dlpack_capsule(torch.zeros(3, dtype=torch.float16).__dlpack__()).dtype == "float16"
    off = torch.arange(10, dtype=torch.int64)[4:]                   # byte_offset or a moved data pointer: the address of element 4
    assert interop.parse_dlpack_capsule(off.__dlpack__()).ptr == off.data_ptr()
    one = torch.zeros(1, 5)[:, 1:4]                                  # extent-1 dimension: any stride, still contiguous
    assert interop.parse_dlpack_capsule(one.__dlpack__()).shape == (1, 3)
    with pytest.raises(ValueError, match="C-contiguous"):
        interop.parse_dlpack_capsule(t.transpose(0, 2).__dlpack__())
    with pytest.raises(ValueError, match="C-contiguous"):
        interop.parse_dlpack_capsule(torch.arange(10.0)[::3].__dlpack__())


def test_the_capsule_keeps_the_memory_and_stays_unconsumed():
    a = np.arange(4, dtype=np.float64)
    cap = a.__dlpack__()
    fa = interop.parse_dlpack_capsule(cap)
    assert fa.keep is cap
    is_valid = ctypes.pythonapi.PyCapsule_IsValid
    is_valid.restype = ctypes.c_int
    is_valid.argtypes = [ctypes.py_object, ctypes.c_char_p]
    assert is_valid(cap, b"dltensor") == 1                          # not renamed to used_dltensor: its destructor still runs
    before = sys.getrefcount(a)
    del cap, fa
    assert sys.getrefcount(a) <= before


def test_device_is_checked_before_any_stream_handshake():
    class Producer:
        called = False

        def __dlpack_device__(self):
            return (interop.KDL_CPU, 0)

        def __dlpack__(self, stream=None):
            Producer.called = True
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="ROCm device memory"):
        interop.from_dlpack_object(Producer(), 0, 1234)
    assert not Producer.called

    class Other(Producer):
        def __dlpack_device__(self):
            return (interop.KDL_ROCM, 3)

    with pytest.raises(ValueError, match="device 3, this engine on device 0"):
        interop.from_dlpack_object(Other(), 0, 1234)
    assert not Producer.called
    assert not interop.is_foreign(np.zeros(3)) and interop.is_foreign(Other())


# ---------------------------------------------------------------- __cuda_array_interface__
def test_cuda_array_interface_dicts():
    base = {"shape": (4, 3), "typestr": "<f4", "data": (0x10000, False), "version": 3}
    fa = interop.parse_cuda_array_interface(dict(base))
    assert (fa.dtype, fa.shape, fa.ptr, fa.readonly, fa.stream) == ("float32", (4, 3), 0x10000, False, None)
    assert interop.parse_cuda_array_interface(dict(base, strides=(12, 4))).shape == (4, 3)          # the C strides, in bytes
    with pytest.raises(ValueError, match="C-contiguous"):
        interop.parse_cuda_array_interface(dict(base, strides=(4, 16)))
    with pytest.raises(ValueError, match="aligned"):
        interop.parse_cuda_array_interface(dict(base, data=(0x10002, False)))
    ro = interop.parse_cuda_array_interface(dict(base, data=(0x10000, True)))
    assert ro.readonly
    assert interop.parse_cuda_array_interface(dict(base, stream=1)).stream == 1
    assert interop.parse_cuda_array_interface(dict(base, stream=0xdead0)).stream == 0xdead0
    with pytest.raises(ValueError, match="stream 0"):
        interop.parse_cuda_array_interface(dict(base, stream=0))
    with pytest.raises(TypeError, match="typestr"):
        interop.parse_cuda_array_interface(dict(base, typestr="<c8"))
    assert interop.parse_cuda_array_interface(dict(base, typestr="<u8", shape=(5,))).dtype == "uint64"
    assert interop.parse_cuda_array_interface(dict(base, typestr="<i4", shape=(5,))).dtype == "int32"


# ---------------------------------------------------------------- NumPy's summation rule (what stat_blocks_kernel reproduces)
def _pairwise(a):
    n = a.shape[0]
    if n < 8:
        res = 0.0
        for v in a:
            res += float(v)
        return res
    if n <= 128:
        r = [float(v) for v in a[:8]]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] += float(a[i + j])
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[i:]:
            res += float(v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a[:n2]) + _pairwise(a[n2:])


def _blocked_sum(a, block):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    s = 0.0
    for i in range(0, a.shape[0], block):
        s += _pairwise(a[i:i + block])
    return s


def _mean_std(a):
    n = a.size
    s = np.float64(_blocked_sum(a, np.getbufsize()))
    mean = s / n
    dev = np.ascontiguousarray(a, dtype=np.float64).reshape(-1) - mean
    s2 = np.float64(_blocked_sum(dev * dev, np.getbufsize()))
    return s, mean, np.sqrt(s2 / n)


@pytest.mark.parametrize("n", [1, 7, 8, 127, 128, 129, 8191, 8192, 8193, 100003, 2 ** 20 + 17])
def test_blocked_pairwise_sum_is_numpys(n):
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n) * 3.0 + 0.25
    a[:: max(1, n // 7)] *= 1e6                                     # magnitudes apart: a different order would show
    s, mean, std = _mean_std(a)
    assert s == np.sum(a), f"NumPy {np.__version__} no longer sums in blocks of np.getbufsize() by the pairwise tree (n = {n})"
    assert mean == np.mean(a) and type(np.mean(a)) is np.float64
    assert std == np.std(a)


def test_blocked_pairwise_sum_of_a_4d_and_an_all_zero_layer():
    rng = np.random.default_rng(7)
    w = (rng.standard_normal((64, 32, 3, 3)) * 0.05).astype(np.float32).astype(np.float64) + 0.001
    s, mean, std = _mean_std(w)
    assert s == np.sum(w) and mean == np.mean(w) and std == np.std(w)
    z = np.zeros((17, 1000))
    s, mean, std = _mean_std(z)
    assert s == np.sum(z) and mean == np.mean(z) and std == np.std(z)                  # (up to the sign of zero: == is sign-blind)
