"""Thin object layer over the C ABI: one `Engine` = one flashe_ctx (device + stream + key +
int_bits); `DeviceBuffer` = a vector resident in HBM.  No arithmetic happens in Python.
"""
import ctypes
import os
import threading
import weakref

import numpy as np

from . import _lib
from ._lib import SCHEME_DOUBLE, SCHEME_SINGLE, FlasheError, PrfJob, c_int, c_u32, c_u32p, c_u64, c_u64p, c_vp

__all__ = ["Engine", "DeviceBuffer", "DeviceVector", "limbs_of", "SCHEME_SINGLE", "SCHEME_DOUBLE", "FlasheError",
           "chunks", "telescope", "prp_block"]


def limbs_of(int_bits):
    return 2 if int_bits > 64 else 1


def _u32_list(vals):
    arr = (c_u32 * max(len(vals), 1))(*[int(v) & 0xFFFFFFFF for v in vals])
    return ctypes.cast(arr, c_u32p), arr


def chunks(n, n_jobs):
    """chunks_idx(range(n), n_jobs) boundaries -- jzf_flashe.py:12-16."""
    out = (c_u64 * (n_jobs + 1))()
    rc = _lib.load().flashe_chunks(n, n_jobs, ctypes.cast(out, c_u64p))
    if rc:
        raise FlasheError(rc, "flashe_chunks: bad arguments")
    return [int(v) for v in out]


def telescope(raw_idx_list):
    """(add_idx, minus_idx) of set_idx_list(mode='decrypt') -- jzf_flashe.py:356-367."""
    k = len(raw_idx_list)
    raw, _r = _u32_list(list(raw_idx_list))
    add = (c_u32 * max(k, 1))()
    minus = (c_u32 * max(k, 1))()
    runs = c_int(0)
    rc = _lib.load().flashe_telescope(raw, k, ctypes.cast(add, c_u32p), ctypes.cast(minus, c_u32p), ctypes.byref(runs))
    if rc:
        raise FlasheError(rc, "flashe_telescope: bad arguments")
    return [int(v) for v in add[:runs.value]], [int(v) for v in minus[:runs.value]]


def prp_block(key, block):
    """AES-256-ECB of one 16-byte block on the host -- jzf_aes_prp.py:24-30."""
    out = (ctypes.c_uint8 * 16)()
    rc = _lib.load().flashe_prp_block((ctypes.c_uint8 * 32).from_buffer_copy(bytes(key)),
                                      (ctypes.c_uint8 * 16).from_buffer_copy(bytes(block)), out)
    if rc:
        raise FlasheError(rc, "flashe_prp_block: bad arguments")
    return bytes(out)


class _HostPool:
    """Recycled host memory behind the result arrays of the host-array API.  A fresh 160 MB array costs 4-7 ms of page faults on its
    first transfer -- more than the 2.9 ms PCIe Gen5 needs to fill it (tests/perf/e2e_calls.py) -- and NumPy hands large arrays
    straight back to the OS, so every call would pay that again.  Blocks the caller has dropped (all views of the array dead) are
    kept and reused, up to FLASHE_HOST_POOL_MB (default 4096; 0 = plain np.empty).

    Page-locked blocks: the host-pointer twins pipeline a large call (upload + kernel of one chunk beside the download of the
    previous one) only into a PINNED result array -- 85 -> 70 ms for the config-2 round (tests/perf/e2e_pinned.py) -- but pinning
    160 MB costs 30 ms, which only a caller that comes back earns.  FLASHE_HOST_POOL_PINNED = auto (default): the first
    PIN_AFTER leases of a size class are pageable, from then on the class is served from page-locked blocks (a long-running job ends up
    all pinned, a one-shot script never pays); 1: always; 0: never.

    A recycled block is handed out UNINITIALISED, like np.empty: it still holds whatever result it carried before (a ciphertext, or a
    decrypted aggregate) until the call that leased it has overwritten all of it -- every Engine method does.  FLASHE_HOST_POOL_WIPE=1
    zeroes blocks as they return to the pool."""
    MIN_BYTES = 1 << 20
    STEP = 2 << 20
    PIN_AFTER = 16                  # > the 12 result arrays of one config-2 round: a single round never pays for pinning

    def __init__(self):
        # re-entrant: _release runs from weakref.finalize callbacks, and a garbage collection triggered INSIDE the locked region
        # (it allocates) may finalise another pooled array on the same thread
        self._lock = threading.RLock()
        self._free = {}                 # capacity -> [block]
        self._leases = {}               # capacity -> how many arrays of that class have been handed out
        self._held = 0                  # bytes parked in the free lists
        self._budget = max(0, int(os.environ.get("FLASHE_HOST_POOL_MB", "4096"))) << 20
        mode = os.environ.get("FLASHE_HOST_POOL_PINNED", "auto").strip().lower()
        self._pinned = "never" if mode in ("", "0", "off", "no") else "always" if mode in ("1", "on", "yes") else "auto"
        self._wipe = os.environ.get("FLASHE_HOST_POOL_WIPE", "0") not in ("", "0")

    class _Pinned:
        pinned = True

        def __init__(self, cap):
            p = c_vp()
            rc = _lib.load().flashe_host_alloc(cap, ctypes.byref(p))
            if rc:
                raise MemoryError("flashe_host_alloc")
            self.addr = p.value

        def __del__(self):
            try:
                _lib.load().flashe_host_free(self.addr)
            except Exception:
                pass

    class _Pageable:
        pinned = False

        def __init__(self, cap):
            self.arr = np.empty(cap, dtype=np.uint8)
            self.addr = self.arr.ctypes.data

    def empty(self, shape, dtype):
        dtype = np.dtype(dtype)
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if nbytes < self.MIN_BYTES or self._budget == 0:
            return np.zeros(shape, dtype=dtype)
        cap = (nbytes + self.STEP - 1) // self.STEP * self.STEP
        block = None
        with self._lock:
            count = self._leases[cap] = self._leases.get(cap, 0) + 1
            want_pinned = self._pinned == "always" or (self._pinned == "auto" and count > self.PIN_AFTER)
            lst = self._free.get(cap)
            if lst:
                # a page-locked block if there is one; a pageable one only while the class is not being pinned
                pick = next((i for i in range(len(lst) - 1, -1, -1) if lst[i].pinned), None)
                if pick is None and not want_pinned:
                    pick = len(lst) - 1
                if pick is not None:
                    block = lst.pop(pick)
                    self._held -= cap
                elif self._held + cap > self._budget:
                    self._held -= cap                         # make room for the pinned replacement: one parked pageable block goes
                    lst.pop()
        if block is None:
            try:
                block = (self._Pinned if want_pinned else self._Pageable)(cap)
            except MemoryError:
                try:
                    block = self._Pageable(cap)
                except MemoryError:
                    return np.empty(shape, dtype=dtype)
        lease = (ctypes.c_char * nbytes).from_address(block.addr)      # dies with the last view of the array
        fin = weakref.finalize(lease, self._release, block, cap)
        fin.atexit = False
        return np.frombuffer(lease, dtype=dtype).reshape(shape)

    def _release(self, block, cap):
        if self._wipe:
            ctypes.memset(block.addr, 0, cap)
        with self._lock:
            lst = self._free.get(cap)
            if lst is None:
                lst = self._free[cap] = []
            if self._held + cap <= self._budget:
                lst.append(block)
                self._held += cap
            elif block.pinned:
                # a page-locked block is worth more than a parked pageable one of its class
                for i, other in enumerate(lst):
                    if not other.pinned:
                        lst[i] = block
                        break
        # otherwise the block dies here

    def trim(self):
        """Give every parked block back."""
        with self._lock:
            self._free.clear()
            self._held = 0


_HOST_POOL = _HostPool()


def host_empty(shape, dtype=np.uint64):
    """An uninitialised result array, from the recycling pool when it is large (see _HostPool)."""
    return _HOST_POOL.empty(shape, dtype)


class DeviceBuffer:
    """`nbytes` of HBM owned by an Engine.  `.ptr` is the raw device address."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.nbytes = int(nbytes)
        p = c_vp()
        engine._check(engine._lib.flashe_dev_alloc(engine._h, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr is not None and self.engine._h is not None:
            self.engine._check(self.engine._lib.flashe_dev_free(self.engine._h, self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.engine._check(self.engine._lib.flashe_memcpy_h2d(self.engine._h, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def upload_at(self, offset, arr):
        """Copy `arr` to byte `offset` of the block (layers of a model going into one flat buffer)."""
        arr = np.ascontiguousarray(arr)
        assert 0 <= offset and offset + arr.nbytes <= self.nbytes
        if arr.nbytes:
            self.engine._check(self.engine._lib.flashe_memcpy_h2d(self.engine._h, self.ptr + int(offset), arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype=np.uint64, count=None):
        n = self.nbytes // np.dtype(dtype).itemsize if count is None else count
        out = host_empty(n, dtype)
        self.engine._check(self.engine._lib.flashe_memcpy_d2h(self.engine._h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def download_at(self, offset, dtype, count):
        """`count` values of `dtype` from byte `offset` of the block (the mirror of upload_at: a window of a large vector)."""
        out = host_empty(int(count), dtype)
        assert 0 <= offset and offset + out.nbytes <= self.nbytes
        if out.nbytes:
            self.engine._check(self.engine._lib.flashe_memcpy_d2h(self.engine._h, out.ctypes.data, self.ptr + int(offset), out.nbytes))
        return out


class DeviceBufferView(DeviceBuffer):
    """`nbytes` at byte `offset` of another DeviceBuffer (one client's block of a cohort's buffer): the same surface, owns nothing and
    keeps its parent alive."""

    def __init__(self, parent, offset, nbytes):
        assert 0 <= offset and offset + nbytes <= parent.nbytes
        self.engine, self.nbytes, self.parent = parent.engine, int(nbytes), parent
        self.ptr = parent.ptr + int(offset)

    def free(self):
        self.ptr = None


class DeviceVector:
    """A vector of `n` elements (L = `limbs` uint64 limbs each) that STAYS in HBM between calls of the drop-in API: what
    FlasheCipher.encrypt / aggregate / decrypt return with device=True and accept in place of an ndarray, so that a round moves
    plaintexts up once and the result down once instead of bouncing every ciphertext device -> host -> device
    (jzf_weights.py:334-338 -> jzf_flashe_block.py:142-174 is the call chain this shortens).  `.to_host()` downloads it.

    The producing engine records an event behind its last write; a consumer on another engine (another FlasheCipher = another
    stream) makes its stream wait for it on the device, the host never blocks."""

    def __init__(self, engine, n, limbs=None, buf=None, elem_bytes=8):
        """elem_bytes = 4: the COMPACT layout of int_bits <= 32 -- the same values as a uint32 array (flashe_*_u32_dev), half the bytes
        of the one-limb layout in HBM and over PCIe."""
        self.engine, self.n = engine, int(n)
        self.elem_bytes = int(elem_bytes)
        self.limbs = 1 if self.elem_bytes == 4 else int(limbs or engine.limbs)
        if buf is not None:
            self.buf = buf
        else:
            self.buf = engine.alloc(max(4 * self.n, 16)) if self.elem_bytes == 4 else engine.alloc_vec(self.n, self.limbs)
        self._ready = None

    @property
    def compact(self):
        return self.elem_bytes == 4

    def __len__(self):
        return self.n

    @property
    def ptr(self):
        return self.buf.ptr

    @property
    def shape(self):
        return (self.n, self.limbs)

    @property
    def device(self):
        return getattr(self.engine, "device", 0)

    @classmethod
    def from_host(cls, engine, arr):
        """Upload a uint64 array of shape [n] or [n, k] -- or a 1-D uint32 array (compact layout, int_bits <= 32)."""
        if isinstance(arr, np.ndarray) and arr.dtype == np.uint32:
            arr = np.ascontiguousarray(arr).reshape(-1)
            return cls(engine, arr.shape[0], 1, buf=engine.upload(arr), elem_bytes=4)
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        if arr.ndim == 1:
            arr = arr.reshape(-1, 1)
        return cls(engine, arr.shape[0], arr.shape[1], buf=engine.upload(arr))

    def mark_ready(self):
        """Called by the producer after enqueueing the kernels that write the vector."""
        if hasattr(self.engine, "event"):
            if self._ready is None:
                self._ready = self.engine.event()
            self.engine.record(self._ready)
        return self

    def wait_on(self, engine):
        """Make `engine`'s stream wait (on the device) until the vector is complete."""
        if engine is not self.engine and self._ready is not None:
            engine.wait_event(self._ready)

    def to_host(self):
        """uint64 array [n, limbs] -- uint32 [n] for a compact vector -- (from the recycling host pool); blocks until the vector is
        complete."""
        if self.elem_bytes == 4:
            return self.buf.download(np.uint32, self.n)
        return self.buf.download(np.uint64, self.n * self.limbs).reshape(self.n, self.limbs)

    def widened(self, engine=None):
        """A compact vector as a one-limb DeviceVector (a device pass, flashe_widen_u32_dev); a one-limb vector as it is."""
        if self.elem_bytes != 4:
            return self
        eng = engine or self.engine
        self.wait_on(eng)
        out = DeviceVector(eng, self.n, 1)
        eng.widen_u32_dev(self.n, self.buf, out.buf)
        return out.mark_ready()

    def narrowed(self, engine=None):
        """A one-limb vector in the compact layout (flashe_narrow_u32_dev: the low 32 bits of every element)."""
        if self.elem_bytes == 4:
            return self
        assert self.limbs == 1
        eng = engine or self.engine
        self.wait_on(eng)
        out = DeviceVector(eng, self.n, 1, elem_bytes=4)
        eng.narrow_u32_dev(self.n, self.buf, out.buf)
        return out.mark_ready()

    # ---- the arbiter's literal reduce: reduce(lambda x, y: (x + y) % mod, models) (jzf_aggregator.py:419, :430) on weights objects whose
    # layers are handles (JZFOrderDictWeights.__add__ / __mod__, jzf_weights.py:340-357, :460-472 map `+` and `%` over the layers) ----
    def __add__(self, other):
        """Element-wise sum mod 2^int_bits of two device-resident vectors, as a new DeviceVector (one HBM-bound launch)."""
        if isinstance(other, (int, np.integer)) and int(other) == 0:
            return self                                            # sum(handles) starts from 0
        if not isinstance(other, DeviceVector):
            return NotImplemented
        eng = self.engine
        if len(other) != self.n:
            raise ValueError(f"operands could not be broadcast together with shapes ({self.n},) ({len(other)},) ")
        if other.device != self.device:
            raise ValueError(f"DeviceVector lives on device {other.device}, this one on device {self.device}")
        other.wait_on(eng)
        if self.compact and other.compact:
            out = DeviceVector(eng, self.n, 1, elem_bytes=4)
            eng.aggregate_elem_u32_dev([self.buf, other.buf], self.n, out.buf)
            return out.mark_ready()
        a, b = self.widened(eng), other.widened(eng)
        if a.limbs != eng.limbs or b.limbs != eng.limbs:
            raise ValueError(f"expected {eng.limbs} limbs per element, got {a.limbs} and {b.limbs}")
        out = DeviceVector(eng, self.n)
        eng.aggregate_elem_dev([a.buf, b.buf], self.n, out.buf)
        return out.mark_ready()

    __radd__ = __add__

    def __mod__(self, modulus):
        """`% (1 << int_bits)`: the vector itself -- every kernel already reduces mod 2^int_bits.  Any other modulus is refused."""
        if int(modulus) == 1 << self.engine.int_bits:
            return self
        raise ValueError(f"a DeviceVector of a {self.engine.int_bits}-bit cipher can only be reduced mod 2^{self.engine.int_bits}")

    def __del__(self):
        try:
            if self._ready is not None and self.engine._h is not None:
                self.engine.event_destroy(self._ready)
            self._ready = None
        except Exception:
            pass


class Graph:
    """A captured sequence of device calls (flashe_graph); launch() replays it on the engine's stream."""

    def __init__(self, engine, handle):
        self.engine, self._g = engine, handle

    def launch(self, iter_shift=0):
        """Replay.  iter_shift = r runs the captured calls as if each had been made with iter + r (round r after the
        captured one); 0 repeats the captured round, mask streams included."""
        self.engine._check(self.engine._lib.flashe_graph_launch_shifted(self.engine._h, self._g, int(iter_shift) & 0xFFFFFFFF))

    def __del__(self):
        try:
            if self._g:
                self.engine._lib.flashe_graph_destroy(self._g)
                self._g = None
        except Exception:
            pass


class PtrTable(object):
    """A table of device pointers built ONCE (the ctypes array a *_dev call hands to the library): what a per-round call takes in
    place of a list of buffers when the same clients' vectors are passed round after round -- for 50 clients building the arrays costs
    as much host time as the launches they describe.  Engine.ptr_table(items); keeps the buffers alive."""

    def __init__(self, engine, items):
        self.items = list(items)
        self.arr = (c_vp * max(len(self.items), 1))(*[engine._ptr(x) for x in self.items])
        self.ptr = ctypes.cast(self.arr, ctypes.POINTER(c_vp))

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)

    def __getitem__(self, i):
        return self.items[i]


class JobTable(object):
    """The job list of Engine.prf_jobs_dev built ONCE (Engine.job_table(jobs)): a hundred clients' jobs cost more host time to
    marshal than their launch takes on the device.  Keeps the buffers alive."""

    def __init__(self, engine, jobs):
        self.jobs = list(jobs)
        self.arr = (PrfJob * max(len(self.jobs), 1))()
        for e, job in enumerate(self.jobs):
            a, m, first, count, inp, in_limbs, out = job[:7]
            # optional tail: (n_in, in_stride_elements, sum_out_ptr or None) = the reduce of n_in vectors fused in
            n_in, in_stride, sum_out = job[7:10] if len(job) > 7 else (0, 0, None)
            self.arr[e] = PrfJob(a, 0 if m is None else m, 0 if m is None else 1, in_limbs, first, count,
                                 None if inp is None else engine._ptr(inp), engine._ptr(out), n_in, 0, in_stride,
                                 None if sum_out is None else engine._ptr(sum_out))

    def __len__(self):
        return len(self.jobs)


class U64Table(object):
    """The same for a per-client list of lengths (Engine.u64_table(values))."""

    def __init__(self, values):
        self.values = [int(v) for v in values]
        self.arr = (c_u64 * max(len(self.values), 1))(*self.values)

    def __len__(self):
        return len(self.values)

    def __iter__(self):
        return iter(self.values)

    def __getitem__(self, i):
        return self.values[i]


def _u64_array(vals):
    return vals.arr if isinstance(vals, U64Table) else (c_u64 * max(len(vals), 1))(*[int(v) for v in vals])


class SpanBounds:
    """flashe_span_bounds: where every client's strictly increasing location list enters every span of the dense vector, computed once
    per round's lists.  The handle is a table ABOUT the lists' contents: the C side can check pointers, lengths and total, not that the
    entries are still the ones the table was built from -- after ANY in-place change of a list call recompute() before the next sparse
    call that takes the handle (SparseShardedRound does, every round).  The handle keeps the list buffers alive (`keep`: the buffer
    objects when `locs` are bare addresses)."""

    def __init__(self, engine, total, locs, ks, keep=None):
        self.engine = engine
        self._keep = keep if keep is not None else (locs if isinstance(locs, PtrTable) else list(locs))
        p, _k = engine._ptr_array(locs)
        kk = _u64_array(ks)
        h = c_vp()
        engine._check(engine._lib.flashe_span_bounds_create(engine._h, int(total), len(locs), p, ctypes.cast(kk, c_u64p), ctypes.byref(h)))
        self._h = h.value

    def recompute(self, locs, ks, keep=None):
        """The table for the next round's lists (same number of clients, same total), in place; mandatory after the lists changed."""
        p, _k = self.engine._ptr_array(locs)
        kk = _u64_array(ks)
        self.engine._check(self.engine._lib.flashe_span_bounds_recompute(self.engine._h, self._h, p, ctypes.cast(kk, c_u64p)))
        self._keep = keep if keep is not None else (locs if isinstance(locs, PtrTable) else list(locs))
        return self

    def __del__(self):
        try:
            if self._h:
                self.engine._lib.flashe_span_bounds_destroy(self._h)
                self._h = None
        except Exception:
            pass


class _PhiloxDraws:
    """np.random.Philox as _draw_table takes a kind of generator: the segment struct and the segments one call holds; a state dict as a
    segment (n and offset are the table's to fill), a segment moved n draws on in place (flashe_philox_advance), and the segment's
    generator fields put back into the state dict."""
    Segment, max_segments = _lib.PhiloxSegment, 128

    @staticmethod
    def segment(state):
        if state.get("bit_generator") != "Philox":
            raise FlasheError(-22, f"the bit generator is {state.get('bit_generator')}, not Philox")
        seg = _lib.PhiloxSegment()
        seg.key[:] = [int(v) for v in state["state"]["key"]]
        seg.counter[:] = [int(v) for v in state["state"]["counter"]]
        seg.buffer[:] = [int(v) for v in state["buffer"]]
        seg.buffer_pos = int(state["buffer_pos"])
        return seg

    @staticmethod
    def move_on(seg, n):
        pos = c_u32(seg.buffer_pos)
        _lib.check(None, _lib.load().flashe_philox_advance(seg.key, seg.counter, ctypes.byref(pos), seg.buffer, n))
        seg.buffer_pos = pos.value

    @staticmethod
    def hand_back(state, seg):                      # (has_uint32 and uinteger stay as they are)
        state["state"]["counter"] = np.array(list(seg.counter), dtype=np.uint64)
        state["buffer"] = np.array(list(seg.buffer), dtype=np.uint64)
        state["buffer_pos"] = int(seg.buffer_pos)


class _Pcg64Draws:
    """np.random.PCG64 and np.random.PCG64DXSM, as _PhiloxDraws is Philox."""
    Segment, max_segments = _lib.Pcg64Segment, 128

    @staticmethod
    def segment(state):
        variant = {"PCG64": 0, "PCG64DXSM": 1}.get(state.get("bit_generator"))
        if variant is None:
            raise FlasheError(-22, f"the bit generator is {state.get('bit_generator')}, not PCG64 or PCG64DXSM")
        seg, m64 = _lib.Pcg64Segment(), (1 << 64) - 1
        for words, v in ((seg.state, int(state["state"]["state"])), (seg.inc, int(state["state"]["inc"]))):
            if not 0 <= v < 1 << 128:
                raise FlasheError(-22, "a PCG64 state or inc outside 128 bits")
            words[:] = [v & m64, v >> 64]
        seg.variant = variant
        return seg

    @staticmethod
    def move_on(seg, n):
        _lib.check(None, _lib.load().flashe_pcg64_advance(seg.variant, seg.state, seg.inc, (c_u64 * 2)(n, 0)))

    @staticmethod
    def hand_back(state, seg):                      # (has_uint32 and uinteger stay as they are)
        state["state"]["state"] = int(seg.state[0]) | (int(seg.state[1]) << 64)


def _draw_table(kind, generators_or_states, counts, offsets=None):
    """The segment table of a kind's *_random_dev call, built on the host: entry s of `generators_or_states` -- a np.random.Generator or a
    bit generator's state dict -- gives counts[s] draws to draws [offsets[s], offsets[s] + counts[s]) of the output (default: back to
    back).  An entry that appears again continues where its earlier segment leaves it.  Returns (segs, counts, offsets, hand_back):
    the C call advances every segment of segs in place, and hand_back() then puts each entry's latest segment into its state dict and
    its Generator.  Raises ValueError for lists of different lengths or more segments than the call holds, FlasheError for another bit
    generator or a count or offset outside 64 bits (ctypes would mask it silently); nothing has been advanced then."""
    counts = [int(c) for c in counts]
    if len(counts) != len(generators_or_states):
        raise ValueError(f"{len(generators_or_states)} generators, {len(counts)} counts")
    offsets = [sum(counts[:s]) for s in range(len(counts))] if offsets is None else [int(o) for o in offsets]
    if len(offsets) != len(counts):
        raise ValueError(f"{len(counts)} counts, {len(offsets)} offsets")
    if len(counts) > kind.max_segments:
        raise ValueError(f"{len(counts)} segments: one launch holds {kind.max_segments}")
    if not all(0 <= v < 1 << 64 for v in counts + offsets):
        raise FlasheError(-22, "a segment's n or offset overflows")
    segs = (kind.Segment * max(len(counts), 1))()
    latest = {}                       # id(entry) -> (entry, its state dict, its latest segment: where a repeat continues, what is handed back)
    for s, (g, n, off) in enumerate(zip(generators_or_states, counts, offsets)):
        if id(g) in latest:
            state, seg = latest[id(g)][1], kind.Segment.from_buffer_copy(latest[id(g)][2])
            kind.move_on(seg, seg.n)
        else:
            state = g.bit_generator.state if isinstance(g, np.random.Generator) else g
            seg = kind.segment(state)
        seg.n, seg.offset = n, off
        segs[s] = seg
        latest[id(g)] = (g, state, segs[s])

    def hand_back():
        for g, state, seg in latest.values():
            kind.hand_back(state, seg)
            if isinstance(g, np.random.Generator):
                g.bit_generator.state = state

    return segs, counts, offsets, hand_back


class Engine:
    """One device context of the cipher engine (wraps flashe_ctx)."""

    def __init__(self, key, int_bits, device=0, stream=None):
        self._lib = _lib.load()
        self._h = None
        key = bytes(key)
        if len(key) != 32:
            raise ValueError("key must be 32 bytes (AES-256)")
        h = c_vp()
        rc = self._lib.flashe_ctx_create(ctypes.byref(h), (ctypes.c_uint8 * 32).from_buffer_copy(key),
                                         int(int_bits), int(device), c_vp(stream) if stream else None)
        if rc:
            msg = self._lib.flashe_last_error(None)
            raise FlasheError(rc, msg.decode() if msg else "flashe_ctx_create failed")
        self._h = h.value
        self.int_bits = int(int_bits)
        self.limbs = limbs_of(int_bits)
        self.device = device
        self.shared_stream = bool(stream)       # created on the caller's stream (everything is stream-ordered with the framework)
        self._held = []                         # (event, keep-alive) of foreign arrays device work may still touch

    # -- plumbing -------------------------------------------------------------------------
    def _check(self, rc):
        return _lib.check(self._h, rc)

    def close(self):
        if self._h is not None:
            self._lib.flashe_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_key(self, key):
        key = bytes(key)
        assert len(key) == 32
        self._check(self._lib.flashe_ctx_set_key(self._h, (ctypes.c_uint8 * 32).from_buffer_copy(key)))

    def set_cu_limit(self, cus):
        """Persistent launches of this engine fill `cus` compute units (0 = all): leaves CUs free for kernels of another stream that
        cannot share a CU with a PRF workgroup (RCCL's)."""
        self._check(self._lib.flashe_ctx_set_cu_limit(self._h, int(cus)))

    @property
    def cu_count(self):
        return int(self._lib.flashe_ctx_cu_count(self._h))

    def set_prf_backend(self, backend):
        """0 = auto, 1 = LDS T-table kernel, 2 = bit-sliced VALU kernel (identical results)."""
        self._check(self._lib.flashe_ctx_set_prf_backend(self._h, int(backend)))

    def compact_supported(self):
        """True when the uint32 entry points (encrypt_batch_u32_dev, aggregate_decrypt_u32_dev, ...) run on this ctx: int_bits <= 32,
        the table PRF backend, the chained kernels.  The C side decides (flashe_ctx_compact_layout), so a caller never has to guess from
        environment variables what check_u32 will answer."""
        return int(self._lib.flashe_ctx_compact_layout(self._h)) == 1

    def selftest(self):
        self._check(self._lib.flashe_selftest(self._h))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def alloc_vec(self, n, limbs=None):
        return DeviceBuffer(self, max(int(n) * (limbs or self.limbs) * 8, 16))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, max(arr.nbytes, 16)).upload(arr)

    def sync(self):
        self._check(self._lib.flashe_sync(self._h))
        self._reap()

    # -- foreign device arrays (interop.py): stream hand-off and lifetime ----------------------------
    @property
    def stream(self):
        """The ctx's hipStream_t as an int (what a DLPack producer orders its pending writes before)."""
        p = c_vp()
        self._check(self._lib.flashe_ctx_stream(self._h, ctypes.byref(p)))
        return int(p.value or 0)

    def wait_stream(self, other):
        """This engine's stream waits, on the device, for the work queued so far on the hipStream_t `other` (int; 0 = null stream)."""
        self._check(self._lib.flashe_stream_wait_stream(self._h, c_vp(int(other)) if other else None))

    def event_query(self, ev):
        done = c_int(0)
        self._check(self._lib.flashe_event_query(self._h, ev, ctypes.byref(done)))
        return bool(done.value)

    def foreign(self, obj, writable=False, what="array"):
        """A framework array as an interop.ForeignArray on this engine's device: the DLPack handshake on this engine's stream, or a
        cuda-array-interface producer's `stream` waited for on the device.  writable: refuse a read-only (cuda-array-interface) array."""
        from . import interop
        fa = interop.as_foreign(obj, self.device, self.stream)
        if writable and fa.readonly:
            raise ValueError(f"{what}: the array is read-only (__cuda_array_interface__ data[1] is True)")
        if fa.stream is not None:
            self.wait_stream(0 if fa.stream in (1, 2) else fa.stream)
        return fa

    def hold(self, keep):
        """Keep `keep` (foreign arrays' owners) alive until the work queued so far on this engine's stream has finished: an event is
        recorded behind it and the pair released at a later call once the event reports done (own-stream mode: a tensor the caller drops
        right after the call must not go back to the framework's allocator while a kernel still reads it)."""
        self._reap()
        if keep:
            ev = self.event()
            self.record(ev)
            self._held.append((ev, keep))

    def _reap(self):
        if not self._held or self._h is None:
            return
        still = []
        for ev, keep in self._held:
            if self.event_query(ev):
                self.event_destroy(ev)
            else:
                still.append((ev, keep))
        self._held = still

    def quantize_encrypt_tensors_dev(self, it, idx, scheme, n, n_jobs, first, count, layers, element_bits, u, ct):
        """quantize_encrypt_model_dev with tensor layers: (start, ptr, alpha, shift, dtype code, flags) per layer (flashe_tensor_layer)."""
        arr, nl = self._tensor_layers(layers)
        self._check(self._lib.flashe_quantize_encrypt_tensors_dev(self._h, it, idx, scheme, n, n_jobs, first, count, arr, nl, element_bits,
                                                                  self._ptr(u), self._ptr(ct)))

    def _cohort_launch(self, name, it, idx, ns, n_jobs, layers, srcs, dtypes, bits, u, cts, *vecs):
        """The library's chained cohort launch `name` (_lib.COHORT_LAUNCHES): the shared table, the sources, the ciphertext pointers and -- a
        _runs_ form -- the checked cipher indices marshalled, one call.  ns = (n,) or (n_values, n_elems), bits = (element_bits,) or
        (element_bits, field_bits), vecs = the sum and what the form takes behind it (dmask, scratch).  False: the library declined."""
        arr, nl = self._tensor_layers(layers)
        C, ps, pd = self._cohort_sources(srcs, dtypes, nl)
        pc, _k = self._ptr_array(cts)
        idx = self._cohort_idx(idx, C)[0] if "_runs_" in name else int(idx)
        rc = getattr(self._lib, name)(self._h, it, idx, C, *(int(n) for n in ns), n_jobs, arr, nl, ps, pd, *bits, self._ptr(u), pc,
                                      *(self._ptr(v) for v in vecs))
        return self._took(rc)

    def quantize_encrypt_cohort_dev(self, it, first_idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, cts, sum_out, dmask=None):
        """A cohort's client steps as ONE chained launch (flashe_quantize_encrypt_cohort_dev): layers = the shared table, (start, None,
        alpha, shift, compute dtype code, flags) per layer; srcs[c][l] / dtypes[c][l] = device pointer and storage dtype code of client
        c's layer l; u = the len(srcs) * n draws, client-major; cts = one n-element vector per client; sum_out / dmask (optional) = their
        sum and the cohort's decrypt mask.  Returns False -- nothing was launched -- when the library declines the shape (FLASHE_ENOTSUP:
        the caller quantises per client and calls encrypt_batch_sum_dev), True otherwise."""
        return self._cohort_launch("flashe_quantize_encrypt_cohort_dev", it, first_idx, (n,), n_jobs, layers, srcs, dtypes, (element_bits,), u, cts, sum_out, dmask)

    def quantize_encrypt_cohort_u32_dev(self, it, first_idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, cts, sum_out):
        """quantize_encrypt_cohort_dev in the compact layout (flashe_quantize_encrypt_cohort_u32_dev, int_bits 16 / 20 / 23 / 24 / 32): cts and
        sum_out are uint32 vectors of n elements, there is no decrypt mask.  Returns False -- nothing was launched -- when the library
        declines the shape (FLASHE_ENOTSUP: the caller quantises per client and calls encrypt_batch_sum_u32_dev), True otherwise."""
        return self._cohort_launch("flashe_quantize_encrypt_cohort_u32_dev", it, first_idx, (n,), n_jobs, layers, srcs, dtypes, (element_bits,), u, cts, sum_out)

    def quantize_encrypt_cohort_u64_dev(self, it, first_idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, cts, sum_out):
        """quantize_encrypt_cohort_dev in the one-limb layout (flashe_quantize_encrypt_cohort_u64_dev, int_bits 33 .. 64): cts and sum_out are
        uint64 vectors of n elements, 8-byte aligned, there is no decrypt mask.  Returns False -- nothing was launched -- when the library
        declines the shape (FLASHE_ENOTSUP: the caller quantises per client and calls encrypt_batch_sum_dev), True otherwise."""
        return self._cohort_launch("flashe_quantize_encrypt_cohort_u64_dev", it, first_idx, (n,), n_jobs, layers, srcs, dtypes, (element_bits,), u, cts, sum_out)

    def cohort_cut_parts(self, n_clients, n, n_jobs, compact=False):
        """The pieces quantize_encrypt_cohort_cut_dev (compact: its _u32 form) will cut a cohort of n_clients clients with n values into
        (flashe_cohort_cut_parts): the caller sizes the scratch from it.  0: the library declines the shape (FLASHE_ENOTSUP)."""
        parts = ctypes.c_int(0)
        rc = self._lib.flashe_cohort_cut_parts(self._h, int(n_clients), int(n), n_jobs, 1 if compact else 0, ctypes.byref(parts))
        return parts.value if self._took(rc) else 0

    def quantize_encrypt_cohort_cut_dev(self, it, first_idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, cts, sum_out, dmask=None, scratch=None):
        """quantize_encrypt_cohort_dev for a vector of ANY length (flashe_quantize_encrypt_cohort_cut_dev): the summed chain cut into
        cohort_cut_parts(...) runs of consecutive clients and one combine pass.  scratch: 16-byte aligned, parts x n x 16 bytes, twice
        that with dmask; may be None when parts == 1.  Returns False -- nothing was launched -- when the library declines the shape
        (FLASHE_ENOTSUP), True otherwise."""
        return self._cohort_launch("flashe_quantize_encrypt_cohort_cut_dev", it, first_idx, (n,), n_jobs, layers, srcs, dtypes, (element_bits,), u, cts, sum_out,
                                   dmask, scratch)

    def quantize_encrypt_cohort_cut_u32_dev(self, it, first_idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, cts, sum_out, scratch=None):
        """quantize_encrypt_cohort_u32_dev for a vector of ANY length (flashe_quantize_encrypt_cohort_cut_u32_dev, int_bits 16 / 20 / 23 /
        24 / 32): scratch of cohort_cut_parts(..., compact=True) x n x 4 bytes, 16-byte aligned; may be None when parts == 1.  Returns
        False -- nothing was launched -- when the library declines the shape (FLASHE_ENOTSUP), True otherwise."""
        return self._cohort_launch("flashe_quantize_encrypt_cohort_cut_u32_dev", it, first_idx, (n,), n_jobs, layers, srcs, dtypes, (element_bits,), u, cts,
                                   sum_out, scratch)

    def quantize_batch_encrypt_cohort_dev(self, it, first_idx, n_values, n_elems, n_jobs, layers, srcs, dtypes, element_bits, field_bits, u, cts,
                                          sum_out, dmask=None):
        """quantize_encrypt_cohort_dev for a BATCHED job (flashe_quantize_batch_encrypt_cohort_dev, int_bits > 64, int_bits // field_bits
        in 5 .. 7): layers / srcs / dtypes describe the n_values values of the model as there, u = the len(srcs) * n_values draws,
        client-major; cts, sum_out and dmask (optional) are vectors of the n_elems batched elements.  Returns False -- nothing was
        launched -- when the library declines the shape (FLASHE_ENOTSUP: the caller runs quantize_batch_tensors_dev per client and
        encrypt_batch_sum_dev), True otherwise."""
        return self._cohort_launch("flashe_quantize_batch_encrypt_cohort_dev", it, first_idx, (n_values, n_elems), n_jobs, layers, srcs, dtypes,
                                   (element_bits, field_bits), u, cts, sum_out, dmask)

    def quantize_encrypt_cohort_runs_dev(self, it, idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, cts, sum_out, dmask=None):
        """quantize_encrypt_cohort_dev for a round in which clients dropped out (flashe_quantize_encrypt_cohort_runs_dev): idx = the cipher
        indices of the clients that report, strictly ascending and below 2^32 - 1 (ValueError for an index outside [0, 2^32)); srcs,
        dtypes, the draws and cts hold one entry per index.  One run of consecutive indices is quantize_encrypt_cohort_dev bit for bit;
        several runs share |idx| + runs streams and dmask receives the decrypt mask of telescope(idx).  Returns False -- nothing was
        launched -- when the library declines the shape (FLASHE_ENOTSUP: also more than 144 streams), True otherwise."""
        return self._cohort_launch("flashe_quantize_encrypt_cohort_runs_dev", it, idx, (n,), n_jobs, layers, srcs, dtypes, (element_bits,), u, cts, sum_out, dmask)

    def quantize_encrypt_cohort_runs_u32_dev(self, it, idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, cts, sum_out):
        """quantize_encrypt_cohort_u32_dev for a round in which clients dropped out (flashe_quantize_encrypt_cohort_runs_u32_dev, int_bits
        16 / 20 / 23 / 24 / 32): idx as in quantize_encrypt_cohort_runs_dev, cts and sum_out uint32 vectors of n elements, no decrypt mask
        (decrypt the sum with telescope(idx)).  One run of consecutive indices is quantize_encrypt_cohort_u32_dev bit for bit.  Returns
        False -- nothing was launched -- when the library declines the shape (FLASHE_ENOTSUP: also more than 144 streams), True otherwise."""
        return self._cohort_launch("flashe_quantize_encrypt_cohort_runs_u32_dev", it, idx, (n,), n_jobs, layers, srcs, dtypes, (element_bits,), u, cts, sum_out)

    def quantize_encrypt_cohort_runs_u64_dev(self, it, idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, cts, sum_out):
        """quantize_encrypt_cohort_u64_dev for a round in which clients dropped out (flashe_quantize_encrypt_cohort_runs_u64_dev, int_bits
        33 .. 64): idx as in quantize_encrypt_cohort_runs_dev, cts and sum_out uint64 vectors of n elements, 8-byte aligned, no decrypt mask
        (decrypt the sum with telescope(idx)).  One run of consecutive indices is quantize_encrypt_cohort_u64_dev bit for bit.  Returns
        False -- nothing was launched -- when the library declines the shape (FLASHE_ENOTSUP: also more than 144 streams), True otherwise."""
        return self._cohort_launch("flashe_quantize_encrypt_cohort_runs_u64_dev", it, idx, (n,), n_jobs, layers, srcs, dtypes, (element_bits,), u, cts, sum_out)

    def quantize_batch_encrypt_cohort_runs_dev(self, it, idx, n_values, n_elems, n_jobs, layers, srcs, dtypes, element_bits, field_bits, u, cts,
                                               sum_out, dmask=None):
        """quantize_batch_encrypt_cohort_dev with the cipher indices of the clients that report
        (flashe_quantize_batch_encrypt_cohort_runs_dev), under quantize_encrypt_cohort_runs_dev's rules."""
        return self._cohort_launch("flashe_quantize_batch_encrypt_cohort_runs_dev", it, idx, (n_values, n_elems), n_jobs, layers, srcs, dtypes,
                                   (element_bits, field_bits), u, cts, sum_out, dmask)

    def cohort_cut_pieces(self, idx, n, n_jobs, compact=False):
        """(parts, begins) of the cut launches that take cipher indices (flashe_cohort_cut_pieces): the pieces a cohort of the clients idx --
        strictly ascending, any number of runs up to 16 -- with n ELEMENTS (a batched job: its batched elements) is cut into, and the
        position in idx of every piece's first client (begins[parts] = len(idx)).  The caller sizes the scratch from parts.  (0, []): the
        library declines the shape (FLASHE_ENOTSUP)."""
        pi, _ki = self._cohort_idx(idx, len(idx))
        parts, begins = ctypes.c_int(0), (ctypes.c_int * 17)()
        rc = self._lib.flashe_cohort_cut_pieces(self._h, pi, len(idx), int(n), n_jobs, 1 if compact else 0, ctypes.byref(parts), begins)
        return (parts.value, list(begins[:parts.value + 1])) if self._took(rc) else (0, [])

    def quantize_encrypt_cohort_cut_runs_dev(self, it, idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, cts, sum_out, dmask=None, scratch=None):
        """quantize_encrypt_cohort_cut_dev with the cipher indices of the clients that report (flashe_quantize_encrypt_cohort_cut_runs_dev):
        quantize_encrypt_cohort_runs_dev's outputs for a vector of ANY length, every gap of idx a cut.  scratch: 16-byte aligned,
        cohort_cut_pieces(idx, n, ...) parts x n x 16 bytes, twice that with dmask.  Returns False -- nothing was launched -- when the
        library declines the shape (FLASHE_ENOTSUP: also more than 16 runs), True otherwise."""
        return self._cohort_launch("flashe_quantize_encrypt_cohort_cut_runs_dev", it, idx, (n,), n_jobs, layers, srcs, dtypes, (element_bits,), u, cts, sum_out,
                                   dmask, scratch)

    def quantize_encrypt_cohort_cut_runs_u32_dev(self, it, idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, cts, sum_out, scratch=None):
        """The same in the compact layout (flashe_quantize_encrypt_cohort_cut_runs_u32_dev, int_bits 16 / 20 / 23 / 24 / 32): scratch of
        cohort_cut_pieces(idx, n, ..., compact=True) parts x n x 4 bytes; no decrypt mask (decrypt the sum with telescope(idx))."""
        return self._cohort_launch("flashe_quantize_encrypt_cohort_cut_runs_u32_dev", it, idx, (n,), n_jobs, layers, srcs, dtypes, (element_bits,), u, cts,
                                   sum_out, scratch)

    def quantize_batch_encrypt_cohort_cut_runs_dev(self, it, idx, n_values, n_elems, n_jobs, layers, srcs, dtypes, element_bits, field_bits, u, cts,
                                                   sum_out, dmask=None, scratch=None):
        """quantize_batch_encrypt_cohort_runs_dev for a model of ANY length (flashe_quantize_batch_encrypt_cohort_cut_runs_dev): the batched
        chain cut into cohort_cut_pieces(idx, n_elems, ...) pieces and one combine pass.  scratch: parts x n_elems x 16 bytes, twice that
        with dmask."""
        return self._cohort_launch("flashe_quantize_batch_encrypt_cohort_cut_runs_dev", it, idx, (n_values, n_elems), n_jobs, layers, srcs, dtypes,
                                   (element_bits, field_bits), u, cts, sum_out, dmask, scratch)

    @staticmethod
    def _cohort_idx(idx, C):
        """The cipher indices of a cohort's C clients as a uint32 array (nothing is reduced mod 2^32 on the way)."""
        idx = [int(v) for v in idx]
        if len(idx) != C:
            raise ValueError(f"{len(idx)} cipher indices for {C} clients")
        if any(v < 0 or v >= 2 ** 32 for v in idx):
            raise ValueError("cipher indices must lie in [0, 2^32)")
        return _u32_list(idx)

    def cohort_masks_dev(self, it, first_idx, n_clients, n, n_jobs, masks, compact=False):
        """A cohort's precomputed encrypt masks as ONE chain of n_clients + 1 streams into the caller's vectors:
        masks[c][j] = term(it, first_idx + c)[j] - term(it, first_idx + c + 1)[j] mod 2^b.  Limb layout (n x L limbs each): n_clients linked
        jobs without an input through prf_jobs_dev; compact=True (int_bits <= 32, uint32 vectors): flashe_cohort_masks_u32_dev."""
        if compact:
            pm, _k = self._ptr_array(masks)
            self._check(self._lib.flashe_cohort_masks_u32_dev(self._h, it, int(first_idx), int(n_clients), int(n), n_jobs, pm))
        elif n and n_clients:
            self.prf_jobs_dev(it, n, n_jobs, [(int(first_idx) + c, int(first_idx) + c + 1, 0, n, None, 0, self._ptr(masks[c])) for c in range(n_clients)])

    def _prepared_cohort_launch(self, name, n, layers, srcs, dtypes, element_bits, draws, masks, cts, sum_out, batch=None):
        """The library's prepared cohort launch `name` (_lib.PREPARED_COHORT_LAUNCHES; a batch_ form: batch=(n_elems, field_bits)): the
        shared table, the sources, the mask and the ciphertext pointers marshalled, one call.  draws = the draw buffer, or _draw_table's
        arguments (kind, generators_or_states, counts, offsets): the generators get their advanced states back only when the call took.
        False: the library declined."""
        arr, nl = self._tensor_layers(layers)
        C, ps, pd = self._cohort_sources(srcs, dtypes, nl)
        pm, _a = self._ptr_array(masks)
        pc, _b = self._ptr_array(cts)
        hand_back = None
        if isinstance(draws, tuple):
            segs, counts, _offsets, hand_back = _draw_table(*draws)
            draws = (segs, len(counts))
        else:
            draws = (self._ptr(draws),)
        ns, bits = ((n,), (element_bits,)) if batch is None else ((n, batch[0]), (element_bits, int(batch[1])))
        took = self._took(getattr(self._lib, name)(self._h, C, *(int(v) for v in ns), arr, nl, ps, pd, *bits, *draws, pm, pc, self._ptr(sum_out)))
        if took and hand_back:
            hand_back()
        return took

    def quantize_combine_cohort_dev(self, n, layers, srcs, dtypes, element_bits, u, masks, cts, sum_out, compact=False, batch=None):
        """A precompute cohort's ONLINE step in one pass, no AES (flashe_quantize_combine_cohort_dev; compact=True: _u32_dev on uint32
        vectors; batch=(n_elems, field_bits): flashe_quantize_batch_combine_cohort_dev over the batched elements): cts[c] = (client c's
        plaintext + masks[c]) mod 2^b and sum_out (optional) = their sum.  layers / srcs / dtypes / u as quantize_encrypt_cohort_dev.
        Returns False -- nothing was launched -- when the library declines (FLASHE_ENOTSUP), True otherwise."""
        name = ("flashe_quantize_batch_combine_cohort_dev" if batch is not None else
                "flashe_quantize_combine_cohort_u32_dev" if compact else "flashe_quantize_combine_cohort_dev")
        return self._prepared_cohort_launch(name, n, layers, srcs, dtypes, element_bits, u, masks, cts, sum_out, batch)

    def quantize_combine_cohort_philox_dev(self, n, layers, srcs, dtypes, element_bits, generators_or_states, counts, offsets, masks, cts, sum_out,
                                           compact=False, batch=None):
        """quantize_combine_cohort_dev (un-batched) with the draws of np.random.Philox streams generated INSIDE the launch
        (flashe_quantize_combine_cohort_philox_dev; compact=True: its _u32 form): no draw buffer exists.  generators_or_states, counts,
        offsets: philox_random_dev's table (_draw_table) over the client-major draw positions -- client c rounds its value k with draw
        c n + k; one entry covers all clients of a shared generator, one entry per client a list of generators, and the same Generator
        listed twice continues itself in list order.  The entries must tile [0, C n) exactly, every client's draws inside one entry.  The
        advanced states are handed back only after the call has succeeded; a refusal raises and advances nothing.  Returns False --
        nothing was launched, nothing advanced -- when the library declines (FLASHE_ENOTSUP), True otherwise.
        batch=(n_elems, field_bits): the batched job (flashe_quantize_batch_combine_cohort_philox_dev) -- n counts the clients' VALUES,
        which is what the table tiles: client c rounds its flat value k with draw c n + k, an element's pads draw nothing."""
        name = ("flashe_quantize_batch_combine_cohort_philox_dev" if batch is not None else
                "flashe_quantize_combine_cohort_philox_u32_dev" if compact else "flashe_quantize_combine_cohort_philox_dev")
        return self._prepared_cohort_launch(name, n, layers, srcs, dtypes, element_bits, (_PhiloxDraws, generators_or_states, counts, offsets), masks, cts,
                                            sum_out, batch)

    def quantize_combine_cohort_pcg64_dev(self, n, layers, srcs, dtypes, element_bits, generators_or_states, counts, offsets, masks, cts, sum_out,
                                          compact=False):
        """quantize_combine_cohort_philox_dev (un-batched; there is no batched form) for generators over np.random.PCG64 -- the one
        np.random.default_rng returns -- or np.random.PCG64DXSM (flashe_quantize_combine_cohort_pcg64_dev; compact=True: its _u32 form):
        the launch generates the draws, no draw buffer exists.  generators_or_states, counts, offsets: pcg64_random_dev's table
        (_draw_table) over the client-major draw positions, under the same rules -- the entries tile [0, C n) exactly, every client's
        draws inside one entry -- and all of ONE variant.  The advanced states are handed back only after the call has succeeded (with
        has_uint32 / uinteger as they were); a refusal raises and advances nothing.  Returns False -- nothing was launched, nothing
        advanced -- when the library declines (FLASHE_ENOTSUP), True otherwise."""
        name = "flashe_quantize_combine_cohort_pcg64_u32_dev" if compact else "flashe_quantize_combine_cohort_pcg64_dev"
        return self._prepared_cohort_launch(name, n, layers, srcs, dtypes, element_bits, (_Pcg64Draws, generators_or_states, counts, offsets), masks, cts, sum_out)

    def quantize_batch_combine_cohort_philox_dev(self, n_values, n_elems, field_bits, layers, srcs, dtypes, element_bits, generators_or_states, counts,
                                                 offsets, masks, cts, sum_out):
        """quantize_combine_cohort_philox_dev(..., batch=(n_elems, field_bits)) under the name FlasheCohort looks the batched form up by."""
        return self.quantize_combine_cohort_philox_dev(n_values, layers, srcs, dtypes, element_bits, generators_or_states, counts, offsets, masks, cts,
                                                       sum_out, batch=(n_elems, field_bits))

    def combine_unbatch_unquantize_model_dev(self, layers, element_bits, field_bits, num_clients, inp, add, minus, n_elems, out):
        """unbatch_unquantize_model_dev over (inp + add - minus) mod 2^b, one memory-bound pass (add / minus: device vectors of n_elems
        elements or None); layers as for unbatch_unquantize_model_dev."""
        arr, nl = self._batch_layers(layers)
        self._check(self._lib.flashe_combine_unbatch_unquantize_model_dev(self._h, arr, nl, element_bits, field_bits, num_clients, self._ptr(inp),
                                                                          self._ptr(add), self._ptr(minus), int(n_elems), self._ptr(out)))

    def combine_unquantize_model_dev(self, n, inp, add, minus, layers, element_bits, num_clients, out):
        """out = unquantise((inp + add - minus) mod 2^b) as float64 over a flattened model, one memory-bound pass (add / minus: device
        vectors or None); layers as for decrypt_unquantize_model_dev."""
        arr, nl = self._codec_layers(layers)
        self._check(self._lib.flashe_combine_unquantize_model_dev(self._h, int(n), self._ptr(inp), self._ptr(add), self._ptr(minus), arr, nl,
                                                                  element_bits, num_clients, self._ptr(out)))

    def quantize_batch_tensors_dev(self, layers, n_values, element_bits, field_bits, u, n_elems, out):
        arr, nl = self._tensor_layers(layers)
        self._check(self._lib.flashe_quantize_batch_tensors_dev(self._h, arr, nl, int(n_values), element_bits, field_bits, self._ptr(u), int(n_elems),
                                                                self._ptr(out)))

    def store_layers_dev(self, inp, n, layers, block=0, stats=None):
        """The flat float64 vector `inp` into the layers' tensors (cast to their dtype, + shift with SHIFT); stats (device, 2 doubles per
        layer): NumPy-exact (sum, sum of squared deviations) of every non-empty layer over buffers of `block` values."""
        arr, nl = self._tensor_layers(layers)
        self._check(self._lib.flashe_store_layers_dev(self._h, self._ptr(inp), int(n), arr, nl, int(block), self._ptr(stats)))

    def stage_layers_dev(self, rows):
        """`weights *= degree` and normalize as ONE streaming pass (flashe_stage_layers_dev): rows of (src, dst, size, scale, shift, storage
        dtype code, STAGE_* flags) -- one model's layers or a cohort's C x L -- each from src as stored to dst as float32 (float64 with
        STAGE_OUT_F64), in the types NumPy gives the layer at each step."""
        rows = list(rows)
        arr = (_lib.StageRow * max(len(rows), 1))()
        for i, (src, dst, size, scale, shift, dtype, flags) in enumerate(rows):
            arr[i].src, arr[i].dst, arr[i].size, arr[i].scale, arr[i].shift, arr[i].src_dtype, arr[i].flags = (
                int(src) if src else None, int(dst) if dst else None, int(size), float(scale), float(shift), int(dtype), int(flags))
        self._check(self._lib.flashe_stage_layers_dev(self._h, arr, len(rows)))

    def finish_layers_dev(self, inp, n, rows, block=0, stats=None):
        """store_layers_dev with the aggregator's degree scaling (flashe_finish_layers_dev): rows of (start, dst, last, div_total, shift,
        div_own, dst dtype code, last dtype code, FINISH_* flags); y = ((inp / div_total + shift) / div_own) + last, every step under its
        flag, stored in dst's dtype; stats as store_layers_dev, over inp / div_total + shift."""
        rows = list(rows)
        arr = (_lib.FinishRow * max(len(rows), 1))()
        for i, (start, dst, last, div_total, shift, div_own, dtype, last_dtype, flags) in enumerate(rows):
            arr[i].start, arr[i].dst, arr[i].last = int(start), int(dst) if dst else None, int(last) if last else None
            arr[i].div_total, arr[i].shift, arr[i].div_own = float(div_total), float(shift), float(div_own)
            arr[i].dst_dtype, arr[i].last_dtype, arr[i].flags = int(dtype), int(last_dtype), int(flags)
        self._check(self._lib.flashe_finish_layers_dev(self._h, self._ptr(inp), int(n), arr, len(rows), int(block), self._ptr(stats)))

    @staticmethod
    def _tensor_layers(layers):
        layers = list(layers)
        arr = (_lib.TensorLayer * max(len(layers), 1))()
        for i, (start, ptr, alpha, shift, dtype, flags) in enumerate(layers):
            arr[i].start, arr[i].ptr, arr[i].alpha, arr[i].shift, arr[i].dtype, arr[i].flags = int(start), ptr, float(alpha), float(shift), int(dtype), int(flags)
        return arr, len(layers)

    @staticmethod
    def _cohort_sources(srcs, dtypes, nl):
        """(C, pointers, dtype codes) of a cohort launch: srcs[c][l] / dtypes[c][l] flattened client-major into C * nl entries."""
        C = len(srcs)
        ps = (c_vp * max(C * nl, 1))(*[int(p) if p else None for row in srcs for p in row])
        pd = (ctypes.c_int32 * max(C * nl, 1))(*[int(d) for row in dtypes for d in row])
        return C, ps, pd

    def _took(self, rc):
        """False when the library declined the shape (FLASHE_ENOTSUP: nothing was launched); any other error raises; True otherwise."""
        if rc == _lib.ENOTSUP:
            return False
        self._check(rc)
        return True

    def memset_dev(self, buf, byte, nbytes):
        """Fills the first nbytes of a device buffer with `byte` (asynchronous on the ctx stream)."""
        self._check(self._lib.flashe_memset_dev(self._h, self._ptr(buf), int(byte), int(nbytes)))

    # -- HIP graph capture / replay of a sequence of *_dev calls ---------------------------------
    def graph_begin(self):
        self._check(self._lib.flashe_graph_begin(self._h))

    def graph_end(self):
        g = c_vp()
        self._check(self._lib.flashe_graph_end(self._h, ctypes.byref(g)))
        return Graph(self, g)

    def event(self):
        ev = c_vp()
        self._check(self._lib.flashe_event_create(self._h, ctypes.byref(ev)))
        return ev.value

    def record(self, ev):
        self._check(self._lib.flashe_event_record(self._h, ev))

    def wait_event(self, ev):
        """Device-side wait of this engine's stream on an event recorded by another engine."""
        self._check(self._lib.flashe_stream_wait_event(self._h, ev))

    def elapsed_ms(self, start, stop):
        ms = ctypes.c_float(0)
        self._check(self._lib.flashe_event_elapsed_ms(self._h, start, stop, ctypes.byref(ms)))
        return float(ms.value)

    def event_destroy(self, ev):
        self._check(self._lib.flashe_event_destroy(self._h, ev))

    @staticmethod
    def _ptr(x):
        if x is None:
            return None
        return x.ptr if isinstance(x, (DeviceBuffer, DeviceVector)) else int(x)

    # -- device-pointer API (asynchronous on the ctx stream) -----------------------------------
    def mask_dev(self, it, idx_list, n, n_jobs, out):
        p, _keep = _u32_list(idx_list)
        self._check(self._lib.flashe_mask_dev(self._h, it, p, len(idx_list), n, n_jobs, self._ptr(out)))

    def encrypt_dev(self, it, idx, scheme, n, n_jobs, pt, pt_limbs, ct):
        self._check(self._lib.flashe_encrypt_dev(self._h, it, idx, scheme, n, n_jobs, self._ptr(pt), pt_limbs, self._ptr(ct)))

    def encrypt_batch_dev(self, it, idx_list, scheme, n, n_jobs, pts, pt_limbs, cts):
        """len(idx_list) independent encrypts of equal length in as few launches as possible."""
        pi, _k = _u32_list(idx_list)
        pp, _a = self._ptr_array(pts)
        pc, _b = self._ptr_array(cts)
        self._check(self._lib.flashe_encrypt_batch_dev(self._h, it, scheme, n, n_jobs, len(idx_list), pi, pp, pt_limbs, pc))

    def encrypt_batch_sum_dev(self, it, idx_list, scheme, n, n_jobs, pts, pt_limbs, cts, sum_out):
        """encrypt_batch_dev that also writes sum_out = sum of the ciphertexts mod 2^b (the local partial aggregate): one launch for
        a run of consecutive clients with int_bits > 64, the encrypts followed by the reduce otherwise."""
        pi, _k = _u32_list(idx_list)
        pp, _a = self._ptr_array(pts)
        pc, _b = self._ptr_array(cts)
        self._check(self._lib.flashe_encrypt_batch_sum_dev(self._h, it, scheme, n, n_jobs, len(idx_list), pi, pp, pt_limbs, pc,
                                                           self._ptr(sum_out)))

    def encrypt_batch_sum_decrypt_dev(self, it, idx_list, scheme, n, n_jobs, pts, pt_limbs, cts, sum_out, dec_out):
        """encrypt_batch_sum_dev followed by decrypt_dev(it, [idx_list[-1] + 1], [idx_list[0]], sum_out -> dec_out), the round of a device
        that plays the clients and the arbiter: one launch at int_bits 128 for a run of consecutive clients with one-limb plaintexts
        on a vector long enough to fill the device, those two calls (the same bytes) otherwise or with FLASHE_CHAIN_DEC=0."""
        pi, _k = _u32_list(idx_list)
        pp, _a = self._ptr_array(pts)
        pc, _b = self._ptr_array(cts)
        self._check(self._lib.flashe_encrypt_batch_sum_decrypt_dev(self._h, it, scheme, n, n_jobs, len(idx_list), pi, pp, pt_limbs, pc,
                                                                   self._ptr(sum_out), self._ptr(dec_out)))

    def encrypt_batch_range_dev(self, it, idx_list, scheme, n, n_jobs, first, count, pts, pt_limbs, cts, sum_out=None):
        """encrypt_batch_dev on elements [first, first + count) of the n-element vectors -- the launch of a GPU that owns that slice of
        every client's vector (pointers address element `first`); sum_out (optional) receives the slice of the ciphertexts' sum."""
        pi, _k = _u32_list(idx_list)
        pp, _a = self._ptr_array(pts)
        pc, _b = self._ptr_array(cts)
        self._check(self._lib.flashe_encrypt_batch_range_dev(self._h, it, scheme, n, n_jobs, first, count, len(idx_list), pi, pp, pt_limbs, pc,
                                                             self._ptr(sum_out)))

    def prf_jobs_dev(self, it, n, n_jobs, jobs):
        """jobs: iterable of (add_idx, minus_idx or None, first, count, in_ptr or None, in_limbs, out_ptr); each writes
        out[k] = in[k] + term(it, add_idx, first + k) - term(it, minus_idx, first + k) for k < count (one launch for
        int_bits > 64).  Pointers address element `first`."""
        tab = jobs if isinstance(jobs, JobTable) else JobTable(self, jobs)
        self._check(self._lib.flashe_prf_jobs_dev(self._h, it, n, n_jobs, len(tab), tab.arr))

    def job_table(self, jobs):
        """The job list of prf_jobs_dev as a table built once (JobTable): for calls that repeat round after round."""
        return JobTable(self, jobs)

    # -- mask precompute resident in the ctx (FlasheCipher.prepare_encrypt / prepare_decrypt, jzf_flashe.py:599-666) ---------------
    PREPARED_ENCRYPT, PREPARED_DECRYPT = 1, 2

    def prepare_encrypt(self, it_next, idx, scheme, num_params, n_jobs):
        self._check(self._lib.flashe_prepare_encrypt(self._h, it_next, idx, scheme, num_params, n_jobs))

    def prepare_decrypt(self, it, num_clients, num_params, n_jobs):
        self._check(self._lib.flashe_prepare_decrypt(self._h, it, num_clients, num_params, n_jobs))

    def prepared_query(self, which):
        """(held?, n, add device pointer, minus device pointer) of the ctx's encrypt / decrypt mask cache."""
        n, a, m = c_u64(0), c_vp(), c_vp()
        rc = self._lib.flashe_prepared_query(self._h, which, ctypes.byref(n), ctypes.byref(a), ctypes.byref(m))
        if rc < 0:
            self._check(rc)
        return bool(rc), int(n.value), a.value, m.value

    def prepared_discard(self, which):
        self._check(self._lib.flashe_prepared_discard(self._h, which))

    def prepared_download(self, which, part):
        """The cached `add` / `minus` mask as a uint64 array [n, L] (None when nothing is held)."""
        held, n, a, m = self.prepared_query(which)
        ptr = a if part == "add" else m
        if not held or not ptr:
            return None
        out = host_empty((n, self.limbs), np.uint64)
        if n:
            self._check(self._lib.flashe_memcpy_d2h(self._h, out.ctypes.data, ptr, out.nbytes))
        return out

    def encrypt_prepared_dev(self, n, pt, pt_limbs, ct):
        """ct = pt + add - minus from the ctx's prepared encrypt masks (no AES); consumes them."""
        self._check(self._lib.flashe_encrypt_prepared_dev(self._h, n, self._ptr(pt), pt_limbs, self._ptr(ct)))

    def decrypt_prepared_dev(self, it, add_idx, minus_idx, n, n_jobs, inp, out):
        """out = inp + add - minus from the ctx's prepared decrypt masks, plus the listed extra prefixes computed online; consumes them."""
        pa, _a = _u32_list(add_idx)
        pm, _m = _u32_list(minus_idx)
        self._check(self._lib.flashe_decrypt_prepared_dev(self._h, it, pa, len(add_idx), pm, len(minus_idx), n, n_jobs, self._ptr(inp), self._ptr(out)))

    # the model-wide codec with the ctx's prepared masks (no AES; the cache rules of encrypt_prepared_dev / decrypt_prepared_dev: a range
    # encrypt consumes the cache with the call that ends at n, a length mismatch leaves it valid)
    def quantize_encrypt_prepared_model_dev(self, n, first, count, layers, element_bits, u, ct):
        """quantize_encrypt_model_dev with the prepared encrypt masks in place of the PRF: ct = quantize + add - minus."""
        arr, nl = self._codec_layers(layers)
        self._check(self._lib.flashe_quantize_encrypt_prepared_model_dev(self._h, n, first, count, arr, nl, element_bits, self._ptr(u), self._ptr(ct)))

    def quantize_encrypt_prepared_tensors_dev(self, n, first, count, layers, element_bits, u, ct):
        arr, nl = self._tensor_layers(layers)
        self._check(self._lib.flashe_quantize_encrypt_prepared_tensors_dev(self._h, n, first, count, arr, nl, element_bits, self._ptr(u), self._ptr(ct)))

    def quantize_batch_encrypt_prepared_model_dev(self, layers, element_bits, field_bits, u, n_elems, ct):
        """quantize_batch_model_dev and the prepared encrypt of its result in one launch."""
        arr, nl = self._batch_layers(layers)
        self._check(self._lib.flashe_quantize_batch_encrypt_prepared_model_dev(self._h, arr, nl, element_bits, field_bits, self._ptr(u), int(n_elems),
                                                                               self._ptr(ct)))

    def quantize_batch_encrypt_prepared_tensors_dev(self, layers, n_values, element_bits, field_bits, u, n_elems, ct):
        arr, nl = self._tensor_layers(layers)
        self._check(self._lib.flashe_quantize_batch_encrypt_prepared_tensors_dev(self._h, arr, nl, int(n_values), element_bits, field_bits, self._ptr(u),
                                                                                 int(n_elems), self._ptr(ct)))

    def decrypt_prepared_unquantize_model_dev(self, it, add_idx, minus_idx, n, n_jobs, inp, layers, element_bits, num_clients, out):
        """decrypt_unquantize_model_dev with the prepared decrypt masks (+ the listed extra prefixes, computed online)."""
        pa, _a = _u32_list(add_idx)
        pm, _m = _u32_list(minus_idx)
        arr, nl = self._codec_layers(layers)
        self._check(self._lib.flashe_decrypt_prepared_unquantize_model_dev(self._h, it, pa, len(add_idx), pm, len(minus_idx), n, n_jobs, self._ptr(inp), arr,
                                                                           nl, element_bits, num_clients, self._ptr(out)))

    def decrypt_prepared_unbatch_unquantize_model_dev(self, it, add_idx, minus_idx, n_jobs, layers, element_bits, field_bits, num_clients, inp, n_elems,
                                                      out):
        pa, _a = _u32_list(add_idx)
        pm, _m = _u32_list(minus_idx)
        arr, nl = self._batch_layers(layers)
        self._check(self._lib.flashe_decrypt_prepared_unbatch_unquantize_model_dev(self._h, it, pa, len(add_idx), pm, len(minus_idx), n_jobs, arr, nl,
                                                                                   element_bits, field_bits, num_clients, self._ptr(inp), int(n_elems),
                                                                                   self._ptr(out)))

    def decrypt_dev(self, it, add_idx, minus_idx, n, n_jobs, inp, out):
        pa, _a = _u32_list(add_idx)
        pm, _m = _u32_list(minus_idx)
        self._check(self._lib.flashe_decrypt_dev(self._h, it, pa, len(add_idx), pm, len(minus_idx), n, n_jobs,
                                                 self._ptr(inp), self._ptr(out)))

    def mask_range_dev(self, it, idx_list, n, n_jobs, first, count, out):
        p, _keep = _u32_list(idx_list)
        self._check(self._lib.flashe_mask_range_dev(self._h, it, p, len(idx_list), n, n_jobs, first, count, self._ptr(out)))

    def encrypt_range_dev(self, it, idx, scheme, n, n_jobs, first, count, pt, pt_limbs, ct):
        self._check(self._lib.flashe_encrypt_range_dev(self._h, it, idx, scheme, n, n_jobs, first, count,
                                                       self._ptr(pt), pt_limbs, self._ptr(ct)))

    def decrypt_range_dev(self, it, add_idx, minus_idx, n, n_jobs, first, count, inp, out):
        pa, _a = _u32_list(add_idx)
        pm, _m = _u32_list(minus_idx)
        self._check(self._lib.flashe_decrypt_range_dev(self._h, it, pa, len(add_idx), pm, len(minus_idx), n, n_jobs,
                                                       first, count, self._ptr(inp), self._ptr(out)))

    def combine_dev(self, n, inp, in_limbs, add, minus, out):
        self._check(self._lib.flashe_combine_dev(self._h, n, self._ptr(inp), in_limbs, self._ptr(add), self._ptr(minus), self._ptr(out)))

    def combine_batch_dev(self, n, inps, in_limbs, adds, minuses, outs):
        """out[v] = inps[v] + adds[v] - minuses[v] for every v in one launch; adds / minuses: lists (entries may be None) or None."""
        pi, _a = self._ptr_array(inps)
        po, _b = self._ptr_array(outs)
        pa, _c = self._ptr_array(adds) if adds is not None else (None, None)
        pm, _d = self._ptr_array(minuses) if minuses is not None else (None, None)
        self._check(self._lib.flashe_combine_batch_dev(self._h, n, len(inps), pi, in_limbs, pa, pm, po))

    def combine_batch_sum_dev(self, n, inps, in_limbs, adds, minuses, outs, sum_out):
        """combine_batch_dev and sum_out = sum_v outs[v] mod 2^b from the same pass (online encrypts with precomputed masks + the
        arbiter's reduce of what they wrote)."""
        pi, _a = self._ptr_array(inps)
        po, _b = self._ptr_array(outs)
        pa, _c = self._ptr_array(adds) if adds is not None else (None, None)
        pm, _d = self._ptr_array(minuses) if minuses is not None else (None, None)
        self._check(self._lib.flashe_combine_batch_sum_dev(self._h, n, len(inps), pi, in_limbs, pa, pm, po, self._ptr(sum_out)))

    def combine_batch_sum_decrypt_dev(self, n, inps, in_limbs, adds, minuses, outs, sum_out, dec_add, dec_minus, dec_out):
        """combine_batch_sum_dev and dec_out = (sum_out + dec_add - dec_minus) mod 2^b from the same pass: the online encrypts with
        precomputed masks, the arbiter's reduce of them and the decrypt of that reduce with the decrypting party's precomputed masks."""
        pi, _a = self._ptr_array(inps)
        po, _b = self._ptr_array(outs)
        pa, _c = self._ptr_array(adds) if adds is not None else (None, None)
        pm, _d = self._ptr_array(minuses) if minuses is not None else (None, None)
        self._check(self._lib.flashe_combine_batch_sum_decrypt_dev(self._h, n, len(inps), pi, in_limbs, pa, pm, po, self._ptr(sum_out),
                                                                   self._ptr(dec_add) if dec_add is not None else None,
                                                                   self._ptr(dec_minus) if dec_minus is not None else None, self._ptr(dec_out)))

    def _ptr_array(self, items):
        if isinstance(items, PtrTable):
            return items.ptr, items
        arr = (c_vp * max(len(items), 1))(*[self._ptr(x) for x in items])
        return ctypes.cast(arr, ctypes.POINTER(c_vp)), arr

    def ptr_table(self, items):
        """A list of device buffers as an argument table built once (PtrTable): accepted wherever a *_dev method takes such a list."""
        return PtrTable(self, items)

    @staticmethod
    def u64_table(values):
        return U64Table(values)

    def _zeros_array(self, zeros):
        """per client a sequence of L limbs (or an int) -> the flat limb array; a prebuilt ctypes array passes through"""
        if isinstance(zeros, ctypes.Array):
            return zeros
        flat = []
        for z in zeros:
            z = [int(z) & (2 ** 64 - 1), int(z) >> 64] if isinstance(z, int) else [int(v) for v in z] + [0]
            flat += z[:self.limbs]
        return (c_u64 * max(len(flat), 1))(*flat)

    def zeros_table(self, zeros):
        return self._zeros_array(zeros)

    def aggregate_elem_dev(self, cts, n, out):
        p, _keep = self._ptr_array(cts)
        self._check(self._lib.flashe_aggregate_elem_dev(self._h, len(cts), p, n, self._ptr(out)))

    def aggregate_decrypt_range_dev(self, it, add_idx, minus_idx, n, n_jobs, first, count, cts, agg_out, out):
        """agg = sum of cts mod 2^b (stored to agg_out unless None), out = decrypt of agg on elements [first, first + count);
        one pass when the ciphertexts are equally spaced in memory.  Pointers address element `first`."""
        pa, _a = _u32_list(add_idx)
        pm, _m = _u32_list(minus_idx)
        p, _keep = self._ptr_array(cts)
        self._check(self._lib.flashe_aggregate_decrypt_range_dev(self._h, it, pa, len(add_idx), pm, len(minus_idx), n, n_jobs, first, count,
                                                                 len(cts), p, self._ptr(agg_out), self._ptr(out)))

    # -- compact layout for int_bits <= 32: the same values as uint32 arrays (half the bytes of the kernels bound by them) --------
    def encrypt_batch_u32_dev(self, it, idx_list, scheme, n, n_jobs, pts, cts):
        """encrypt_batch_dev on uint32 plaintext and ciphertext vectors (int_bits <= 32)."""
        pi, _k = _u32_list(idx_list)
        pp, _a = self._ptr_array(pts)
        pc, _b = self._ptr_array(cts)
        self._check(self._lib.flashe_encrypt_batch_u32_dev(self._h, it, scheme, n, n_jobs, len(idx_list), pi, pp, pc))

    def encrypt_batch_sum_u32_dev(self, it, idx_list, scheme, n, n_jobs, pts, cts, sum_out):
        """encrypt_batch_u32_dev and sum_out = sum of the ciphertexts (uint32 [n]) from the same launch where the shape allows it."""
        pi, _k = _u32_list(idx_list)
        pp, _a = self._ptr_array(pts)
        pc, _b = self._ptr_array(cts)
        self._check(self._lib.flashe_encrypt_batch_sum_u32_dev(self._h, it, scheme, n, n_jobs, len(idx_list), pi, pp, pc, self._ptr(sum_out)))

    def aggregate_decrypt_u32_dev(self, it, add_idx, minus_idx, n, n_jobs, first, count, cts, agg_out, out, out_elem_bytes=8):
        """aggregate_decrypt_range_dev on uint32 operands (one add, at most one minus prefix); agg_out / out are uint32 or uint64 arrays."""
        pa, _a = _u32_list(add_idx)
        pm, _m = _u32_list(minus_idx)
        p, _keep = self._ptr_array(cts)
        self._check(self._lib.flashe_aggregate_decrypt_u32_dev(self._h, it, pa, len(add_idx), pm, len(minus_idx), n, n_jobs, first, count,
                                                               len(cts), p, self._ptr(agg_out), self._ptr(out), int(out_elem_bytes)))

    def aggregate_elem_u32_dev(self, cts, n, out):
        p, _keep = self._ptr_array(cts)
        self._check(self._lib.flashe_aggregate_elem_u32_dev(self._h, len(cts), p, n, self._ptr(out)))

    def widen_u32_dev(self, n, inp, out):
        self._check(self._lib.flashe_widen_u32_dev(self._h, n, self._ptr(inp), self._ptr(out)))

    def narrow_u32_dev(self, n, inp, out):
        self._check(self._lib.flashe_narrow_u32_dev(self._h, n, self._ptr(inp), self._ptr(out)))

    def aggregate_packed_dev(self, packed, n_limbs, total_bits, out):
        p, _keep = self._ptr_array(packed)
        self._check(self._lib.flashe_aggregate_packed_dev(self._h, len(packed), p, n_limbs, total_bits, self._ptr(out)))

    def aggregate_packed_elems_dev(self, cts, n, out):
        """out = unpack(sum of pack(ct) mod 2^(int_bits n)) of n-element ciphertext vectors in the engine's layout, in one pass with no
        packed vector; out must not be an operand.  False -- nothing was launched -- when the library declines (FLASHE_ENOTSUP: more
        operands in a pass than 2^int_bits), True otherwise."""
        p, _keep = self._ptr_array(cts)
        return self._took(self._lib.flashe_aggregate_packed_elems_dev(self._h, len(cts), p, n, self._ptr(out)))

    def aggregate_packed_elems_u32_dev(self, cts, n, out):
        """aggregate_packed_elems_dev on uint32 vectors (the compact layout, int_bits <= 32)."""
        p, _keep = self._ptr_array(cts)
        return self._took(self._lib.flashe_aggregate_packed_elems_u32_dev(self._h, len(cts), p, n, self._ptr(out)))

    def packed_probe_dev(self, n_limbs, x, info):
        """info (device, 3 words) <- (x[0], body limbs [1, n_limbs-1) all ones, x[n_limbs-1]); asynchronous."""
        self._check(self._lib.flashe_packed_probe_dev(self._h, n_limbs, self._ptr(x), self._ptr(info)))

    def packed_add_carry_dev(self, n_limbs, total_bits, carry_in, x):
        """x <- (x + carry_in) mod 2^total_bits in place."""
        self._check(self._lib.flashe_packed_add_carry_dev(self._h, n_limbs, total_bits, carry_in, self._ptr(x)))

    def packed_resolve_carry_dev(self, n_limbs, total_bits, infos, n_below, x):
        """x <- (x + carry_in) mod 2^total_bits, carry_in derived on the device from the probe triples of the n_below slices below."""
        self._check(self._lib.flashe_packed_resolve_carry_dev(self._h, n_limbs, total_bits, self._ptr(infos), n_below, self._ptr(x)))

    def packed_resolve_carry_strided_dev(self, n_limbs, total_bits, infos, n_below, stride_words, x):
        self._check(self._lib.flashe_packed_resolve_carry_strided_dev(self._h, n_limbs, total_bits, self._ptr(infos), n_below, stride_words, self._ptr(x)))

    def pack_dev(self, n, inp, out):
        self._check(self._lib.flashe_pack_dev(self._h, n, self._ptr(inp), self._ptr(out)))

    def unpack_dev(self, n, inp, out):
        self._check(self._lib.flashe_unpack_dev(self._h, n, self._ptr(inp), self._ptr(out)))

    def expand_to_dense_dev(self, total, k, loc, vals, zero_limbs, out):
        z = (c_u64 * 2)(*([int(v) for v in zero_limbs] + [0])[:2])
        self._check(self._lib.flashe_expand_to_dense_dev(self._h, total, k, self._ptr(loc), self._ptr(vals),
                                                         ctypes.cast(z, c_u64p), self._ptr(out)))

    def span_bounds(self, total, locs, ks, keep=None):
        """The span bounds of a round's strictly increasing location lists, computed once: a SpanBounds handle that
        sparse_aggregate_dev / sparse_decrypt_dev take (bounds=...) instead of recomputing the table for the same lists.  After an
        in-place change of a list: handle.recompute(...) first.  keep: objects the handle should keep alive (locs given as addresses)."""
        return SpanBounds(self, total, locs, ks, keep=keep)

    def sparse_aggregate_dev(self, total, locs, ks, vals, zeros, out, sorted_lists=False, bounds=None):
        """out = sum over clients of expand_to_dense(total, locs[c], vals[c], zeros[c]) mod 2^b, without the dense
        intermediates.  zeros: per client a sequence of L limbs (or an int).  sorted_lists: every location list is
        strictly increasing (one-pass LDS-staged form).  bounds: a SpanBounds of exactly these lists (implies sorted_lists)."""
        pl, _kl = self._ptr_array(locs)
        pv, _kv = self._ptr_array(vals)
        k = _u64_array(ks)
        zz = self._zeros_array(zeros)
        if bounds is not None:
            self._check(self._lib.flashe_sparse_aggregate_bounds_dev(self._h, total, len(locs), pl, ctypes.cast(k, c_u64p), pv,
                                                                     ctypes.cast(zz, c_u64p), bounds._h, self._ptr(out)))
            return
        self._check(self._lib.flashe_sparse_aggregate_dev(self._h, total, len(locs), pl, ctypes.cast(k, c_u64p), pv,
                                                          ctypes.cast(zz, c_u64p), 1 if sorted_lists else 0, self._ptr(out)))

    def sparse_encrypt_aggregate_dev(self, it, idx, locs, ks, pts, pt_limbs, zeros, total, n_jobs, cts, agg, bounds=None, position_range=None):
        """The clients this device plays encrypt their compact uploads (single mask) and the sum of the expanded uploads is written in
        the same pass: cts[c] = encrypt(it, idx[c], SINGLE) of pts[c], agg = sparse_aggregate_dev(locs, cts, zeros).  Strictly increasing
        location lists.  int_bits > 64: one persistent launch per 64 clients with the PRF inside the span reduce.
        position_range = (first, count): only the positions [first, first + count) -- one GPU's share of a round sharded by position ranges;
        `agg` then addresses position `first`, the ciphertexts of entries outside the range are not written."""
        pl, _kl = self._ptr_array(locs)
        pp, _kp = self._ptr_array(pts)
        pc, _kc = self._ptr_array(cts)
        C = len(locs)
        k = _u64_array(ks)
        ii = idx if isinstance(idx, ctypes.Array) else (ctypes.c_uint32 * max(C, 1))(*[int(v) for v in idx])
        zz = self._zeros_array(zeros)
        if position_range is not None:
            first, count = position_range
            if bounds is None:
                raise ValueError("a position range needs the span bounds of the lists")
            self._check(self._lib.flashe_sparse_encrypt_aggregate_range_dev(self._h, it, n_jobs, total, C, ii, pl, ctypes.cast(k, c_u64p), pp, pt_limbs,
                                                                            ctypes.cast(zz, c_u64p), bounds._h, int(first), int(count), pc, self._ptr(agg)))
            return
        self._check(self._lib.flashe_sparse_encrypt_aggregate_dev(self._h, it, n_jobs, total, C, ii, pl, ctypes.cast(k, c_u64p), pp, pt_limbs,
                                                                  ctypes.cast(zz, c_u64p), bounds._h if bounds is not None else None, pc,
                                                                  self._ptr(agg)))

    def sparse_span(self):
        """Positions per span of the sparse passes with the PRF inside: position ranges start (and, unless they end the vector, end) at
        multiples of it."""
        return int(self._lib.flashe_sparse_span())

    def sparse_minus_mask_dev(self, it, locs, ks, total, n_jobs, out, sorted_lists=False):
        p, _keep = self._ptr_array(locs)
        k = _u64_array(ks)
        fn = self._lib.flashe_sparse_minus_mask_sorted_dev if sorted_lists else self._lib.flashe_sparse_minus_mask_dev
        self._check(fn(self._h, it, len(locs), p, ctypes.cast(k, c_u64p), total, n_jobs, self._ptr(out)))

    def sparse_decrypt_dev(self, it, locs, ks, total, n_jobs, agg, out, sorted_lists=False, bounds=None, position_range=None):
        """out = (agg - dense minus-mask of the location lists) mod 2^b in the pass that builds the mask.  position_range = (first, count):
        agg / out address position `first` and hold `count` elements (needs bounds)."""
        p, _keep = self._ptr_array(locs)
        k = _u64_array(ks)
        if position_range is not None:
            first, count = position_range
            if bounds is None:
                raise ValueError("a position range needs the span bounds of the lists")
            self._check(self._lib.flashe_sparse_decrypt_range_dev(self._h, it, len(locs), p, ctypes.cast(k, c_u64p), total, n_jobs, bounds._h,
                                                                  int(first), int(count), self._ptr(agg), self._ptr(out)))
            return
        if bounds is not None:
            self._check(self._lib.flashe_sparse_decrypt_bounds_dev(self._h, it, len(locs), p, ctypes.cast(k, c_u64p), total, n_jobs, bounds._h,
                                                                   self._ptr(agg), self._ptr(out)))
            return
        self._check(self._lib.flashe_sparse_decrypt_dev(self._h, it, len(locs), p, ctypes.cast(k, c_u64p), total, n_jobs,
                                                        1 if sorted_lists else 0, self._ptr(agg), self._ptr(out)))

    def sparse_double_masks_dev(self, it, locs, ks, total, add_out, minus_out):
        """Both dense masks of the sparse + double decrypt (set_idx_list's run analysis + _static_prepare_decrypt_spar) straight from
        the clients' strictly increasing location lists."""
        p, _keep = self._ptr_array(locs)
        k = (c_u64 * max(len(ks), 1))(*[int(v) for v in ks])
        self._check(self._lib.flashe_sparse_double_masks_dev(self._h, it, len(locs), p, ctypes.cast(k, c_u64p), total,
                                                             self._ptr(add_out), self._ptr(minus_out)))

    def dynamic_masking_cost_dev(self, locs, ks):
        """(single_cost, double_cost) of Arbiter.dynamic_masking (jzf_flashe_block.py:92-112) from device-resident, strictly increasing
        location lists: the positions consecutive clients share are counted on the device, no one-hot vectors."""
        p, _keep = self._ptr_array(locs)
        kk = (c_u64 * max(len(ks), 1))(*[int(v) for v in ks])
        single, double = c_u64(0), c_u64(0)
        self._check(self._lib.flashe_dynamic_masking_cost_dev(self._h, len(locs), p, kk, ctypes.byref(single), ctypes.byref(double)))
        return int(single.value), int(double.value)

    def sparse_dense_mask_dev(self, it, sels, total, out):
        p, _keep = self._ptr_array(sels)
        self._check(self._lib.flashe_sparse_dense_mask_dev(self._h, it, len(sels), p, total, self._ptr(out)))

    # -- host-array API (synchronous; numpy uint64 limb arrays in and out) -----------------------
    def _vec(self, arr, allow_pt=False):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        if arr.ndim == 1:
            arr = arr.reshape(-1, 1)
        if arr.shape[1] != self.limbs and not (allow_pt and arr.shape[1] == 1):
            raise ValueError(f"expected [n, {self.limbs}] uint64 limbs, got {arr.shape}")
        return arr

    def mask(self, it, idx_list, n, n_jobs):
        out = host_empty((n, self.limbs))
        p, _keep = _u32_list(idx_list)
        self._check(self._lib.flashe_mask(self._h, it, p, len(idx_list), n, n_jobs, out.ctypes.data))
        return out

    def encrypt(self, it, idx, scheme, n_jobs, pt):
        pt = self._vec(pt, allow_pt=True)
        n = pt.shape[0]
        ct = host_empty((n, self.limbs))
        self._check(self._lib.flashe_encrypt(self._h, it, idx, scheme, n, n_jobs, pt.ctypes.data, pt.shape[1], ct.ctypes.data))
        return ct

    def decrypt(self, it, add_idx, minus_idx, n_jobs, ct):
        ct = self._vec(ct)
        n = ct.shape[0]
        out = host_empty(ct.shape)
        pa, _a = _u32_list(add_idx)
        pm, _m = _u32_list(minus_idx)
        self._check(self._lib.flashe_decrypt(self._h, it, pa, len(add_idx), pm, len(minus_idx), n, n_jobs,
                                             ct.ctypes.data, out.ctypes.data))
        return out

    def combine(self, inp, add=None, minus=None):
        inp = self._vec(inp, allow_pt=True)
        n = inp.shape[0]
        add = self._vec(add) if add is not None else None
        minus = self._vec(minus) if minus is not None else None
        out = host_empty((n, self.limbs))
        self._check(self._lib.flashe_combine(self._h, n, inp.ctypes.data, inp.shape[1],
                                             add.ctypes.data if add is not None else None,
                                             minus.ctypes.data if minus is not None else None, out.ctypes.data))
        return out

    def aggregate_elem(self, cts):
        cts = [self._vec(c) for c in cts]
        n = cts[0].shape[0]
        if any(c.shape[0] != n for c in cts):
            raise ValueError("operands differ in length")
        out = host_empty((n, self.limbs))
        tab = (c_vp * len(cts))(*[c.ctypes.data for c in cts])
        self._check(self._lib.flashe_aggregate_elem(self._h, len(cts), ctypes.cast(tab, ctypes.POINTER(c_vp)), n, out.ctypes.data))
        return out

    def aggregate_packed(self, packed, total_bits):
        n_limbs = (total_bits + 63) // 64
        packed = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1) for p in packed]
        if any(p.shape[0] != n_limbs for p in packed):
            raise ValueError("operands must have ceil(total_bits / 64) limbs")
        out = np.zeros(n_limbs, dtype=np.uint64)
        tab = (c_vp * len(packed))(*[p.ctypes.data for p in packed])
        self._check(self._lib.flashe_aggregate_packed(self._h, len(packed), ctypes.cast(tab, ctypes.POINTER(c_vp)),
                                                      n_limbs, total_bits, out.ctypes.data))
        return out

    def pack(self, x):
        x = self._vec(x)
        n = x.shape[0]
        out = np.zeros((n * self.int_bits + 63) // 64, dtype=np.uint64)
        self._check(self._lib.flashe_pack(self._h, n, x.ctypes.data, out.ctypes.data))
        return out

    def unpack(self, p, n):
        p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1)
        if p.shape[0] != (n * self.int_bits + 63) // 64:
            raise ValueError("packed operand has the wrong number of limbs")
        out = host_empty((n, self.limbs))
        self._check(self._lib.flashe_unpack(self._h, n, p.ctypes.data, out.ctypes.data))
        return out

    def expand_to_dense(self, total, loc, vals, zero_limbs):
        loc = np.ascontiguousarray(loc, dtype=np.uint32)
        vals = self._vec(vals) if len(loc) else np.zeros((0, self.limbs), dtype=np.uint64)
        z = (c_u64 * 2)(*([int(v) for v in np.asarray(zero_limbs).reshape(-1)] + [0])[:2])
        out = host_empty((total, self.limbs))
        self._check(self._lib.flashe_expand_to_dense(self._h, total, len(loc), loc.ctypes.data, vals.ctypes.data,
                                                     ctypes.cast(z, c_u64p), out.ctypes.data))
        return out

    def sparse_minus_mask(self, it, locs, total, n_jobs):
        locs = [np.ascontiguousarray(l, dtype=np.uint32) for l in locs]
        tab = (c_vp * max(len(locs), 1))(*[l.ctypes.data for l in locs])
        k = (c_u64 * max(len(locs), 1))(*[len(l) for l in locs])
        out = host_empty((total, self.limbs))
        self._check(self._lib.flashe_sparse_minus_mask(self._h, it, len(locs), ctypes.cast(tab, ctypes.POINTER(c_vp)),
                                                       ctypes.cast(k, c_u64p), total, n_jobs, out.ctypes.data))
        return out

    def sparse_dense_mask(self, it, sels, total):
        sels = [np.ascontiguousarray(s, dtype=np.uint8) for s in sels]
        if any(s.shape[0] != total for s in sels):
            raise ValueError("selector length must equal total")
        tab = (c_vp * max(len(sels), 1))(*[s.ctypes.data for s in sels])
        out = host_empty((total, self.limbs))
        self._check(self._lib.flashe_sparse_dense_mask(self._h, it, len(sels), ctypes.cast(tab, ctypes.POINTER(c_vp)),
                                                       total, out.ctypes.data))
        return out

    # -- quantise / batch codec (jzf_quantize.py *_padding_asymmetric) ----------------------------
    def quantize_dev(self, n, x, x_is_f64, alpha, element_bits, u, q):
        self._check(self._lib.flashe_quantize_dev(self._h, n, self._ptr(x), 1 if x_is_f64 else 0, float(alpha), element_bits,
                                                  self._ptr(u), self._ptr(q)))

    def unquantize_dev(self, n, v, v_limbs, alpha, element_bits, num_clients, out):
        self._check(self._lib.flashe_unquantize_dev(self._h, n, self._ptr(v), v_limbs, float(alpha), element_bits, num_clients,
                                                    self._ptr(out)))

    def batch_dev(self, n, vals, field_bits, out):
        self._check(self._lib.flashe_batch_dev(self._h, n, self._ptr(vals), field_bits, self._ptr(out)))

    def unbatch_dev(self, n_batches, inp, field_bits, out):
        self._check(self._lib.flashe_unbatch_dev(self._h, n_batches, self._ptr(inp), field_bits, self._ptr(out)))

    def numpy_random_dev(self, n, out=None):
        """np.random.random(n) generated on the device, bit for bit, from NumPy's GLOBAL legacy generator: its MT19937 state is read,
        advanced on the device and put back, so host draws before and after continue one stream.  Returns the DeviceBuffer of n
        float64 (`out` or a new one).  Raises if the global generator is not MT19937."""
        st = np.random.get_state()
        if st[0] != "MT19937":
            raise FlasheError(-22, f"np.random's bit generator is {st[0]}, not MT19937")
        key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
        pos = c_u32(int(st[2]))
        out = out if out is not None else self.alloc(max(8 * int(n), 16))
        self._check(self._lib.flashe_mt19937_random_dev(self._h, key.ctypes.data_as(c_u32p), ctypes.byref(pos), int(n), self._ptr(out)))
        np.random.set_state((st[0], key, int(pos.value), st[3], st[4]))
        return out

    PHILOX_MAX_SEGMENTS = _PhiloxDraws.max_segments  # the segments one flashe_philox_random_dev launch holds

    def _draw_random_dev(self, kind, call, generators_or_states, counts, out, offsets):
        """philox_random_dev / pcg64_random_dev: the kind's table (_draw_table), its C call, and the advanced states handed back -- only
        after the call has succeeded, so that a refusal advances nothing."""
        segs, counts, offsets, hand_back = _draw_table(kind, generators_or_states, counts, offsets)
        if out is None:
            out = self.alloc(max(8 * max([o + n for o, n in zip(offsets, counts)], default=0), 16))
        self._check(call(self._h, segs, len(counts), self._ptr(out)))
        hand_back()
        return out

    def philox_random_dev(self, generators_or_states, counts, out=None, offsets=None):
        """Generator(np.random.Philox(...)).random(n) generated on the device, bit for bit, for every entry of `generators_or_states` in ONE
        asynchronous launch: entry s gives counts[s] draws to draws [offsets[s], offsets[s] + counts[s]) of `out` (a DeviceBuffer or a
        device address of float64, 8-byte aligned; default: the entries back to back in a new buffer).  An entry is a np.random.Generator
        over Philox -- its bit_generator.state is read and the advanced state put back, so host draws before and after continue one
        stream -- or such a state dict, advanced in place.  The same Generator may appear several times: its segments continue one
        another in list order (flashe_philox_advance), as sequential host draws would.  Returns the buffer.  Raises for another bit generator, overlapping ranges,
        a misaligned output, a count or offset outside 64 bits or more than PHILOX_MAX_SEGMENTS entries; nothing is advanced then."""
        return self._draw_random_dev(_PhiloxDraws, self._lib.flashe_philox_random_dev, generators_or_states, counts, out, offsets)

    def philox_grid(self, n, buffer_pos=4):
        """(workgroups, tiles) of the launch philox_random_dev makes for one segment of n draws: more tiles than workgroups are further
        trips of a workgroup's loop."""
        wg, tiles = c_u32(0), c_u64(0)
        self._check(self._lib.flashe_philox_grid(self._h, int(n), int(buffer_pos), ctypes.byref(wg), ctypes.byref(tiles)))
        return int(wg.value), int(tiles.value)

    PCG64_MAX_SEGMENTS = _Pcg64Draws.max_segments    # the segments one flashe_pcg64_random_dev call holds
    PCG64_STRETCH = 16               # the draws a lane of its launch walks, at a stride of the workgroup's 256 lanes

    def pcg64_random_dev(self, generators_or_states, counts, out=None, offsets=None):
        """Generator(np.random.PCG64(...)).random(n) -- the generator np.random.default_rng returns -- and Generator(np.random.PCG64DXSM(...))
        .random(n) generated on the device, bit for bit, for every entry of `generators_or_states` in ONE asynchronous call (one launch per
        variant present).  Arguments, result and refusals as philox_random_dev's, with PCG64_MAX_SEGMENTS entries at most: an entry is a
        np.random.Generator over PCG64 or PCG64DXSM, or such a state dict (a repeated one continues through flashe_pcg64_advance); the
        advanced state is put back with has_uint32 / uinteger as they were."""
        return self._draw_random_dev(_Pcg64Draws, self._lib.flashe_pcg64_random_dev, generators_or_states, counts, out, offsets)

    def pcg64_grid(self, n):
        """(workgroups, tiles, draws per tile) of the launch pcg64_random_dev makes for one segment of n draws: more tiles than workgroups are
        further trips of a workgroup's loop."""
        wg, tiles, draws = c_u32(0), c_u64(0), c_u32(0)
        self._check(self._lib.flashe_pcg64_grid(self._h, int(n), ctypes.byref(wg), ctypes.byref(tiles), ctypes.byref(draws)))
        return int(wg.value), int(tiles.value), int(draws.value)

    def pcg64_cohort_grid(self, n):
        """The workgroups of the launch quantize_combine_cohort_pcg64_dev makes for n values per client (256 lanes each, a lane owning runs
        of four values: more runs than lanes are further passes, which compose the lane's jump with the grid's stride jump)."""
        wg = c_u32(0)
        self._check(self._lib.flashe_pcg64_cohort_grid(self._h, int(n), ctypes.byref(wg)))
        return int(wg.value)

    @staticmethod
    def pcg64_cohort_lane_draws(generator_or_state, first, workgroups, run, iterations):
        """Host only: the 4 x iterations draws the lane that owns run `run` of that launch on a grid of `workgroups` generates in its first
        `iterations` passes for a client whose stretch starts `first` draws into the generator (flashe_pcg64_cohort_lane_draws: the
        header functions the kernel compiles) -- values 4 (run + 256 workgroups p) + i of that client.  Nothing is advanced."""
        g = generator_or_state
        seg = _Pcg64Draws.segment(g.bit_generator.state if isinstance(g, np.random.Generator) else g)
        out = np.empty(4 * int(iterations), dtype=np.float64)
        _lib.check(None, _lib.load().flashe_pcg64_cohort_lane_draws(seg.variant, seg.state, seg.inc, int(first), int(workgroups), int(run), int(iterations),
                                                                   out.ctypes.data_as(c_vp)))
        return out

    def quantize_encrypt_dev(self, it, idx, scheme, n, n_jobs, x, x_is_f64, alpha, element_bits, u, ct):
        """ct = encrypt(quantize(x)) in one launch (un-batched values); x float32 / float64, u float64 uniforms, all device-resident."""
        self._check(self._lib.flashe_quantize_encrypt_dev(self._h, it, idx, scheme, n, n_jobs, self._ptr(x), 1 if x_is_f64 else 0,
                                                          float(alpha), element_bits, self._ptr(u), self._ptr(ct)))

    def decrypt_unquantize_dev(self, it, add_idx, minus_idx, n, n_jobs, inp, alpha, element_bits, num_clients, out):
        """out (float64) = unquantize(decrypt(inp)) in one launch."""
        pa, _a = _u32_list(add_idx)
        pm, _m = _u32_list(minus_idx)
        self._check(self._lib.flashe_decrypt_unquantize_dev(self._h, it, pa, len(add_idx), pm, len(minus_idx), n, n_jobs, self._ptr(inp),
                                                            float(alpha), element_bits, num_clients, self._ptr(out)))

    @staticmethod
    def _codec_layers(layers):
        """layers: iterable of (start, x device pointer or None, alpha, x_is_f64) -> ctypes array of flashe_codec_layer."""
        layers = list(layers)
        arr = (_lib.CodecLayer * max(len(layers), 1))()
        for i, (start, x, alpha, is_f64) in enumerate(layers):
            arr[i].start, arr[i].x_dev, arr[i].alpha, arr[i].x_is_f64, arr[i].reserved = int(start), x, float(alpha), 1 if is_f64 else 0, 0
        return arr, len(layers)

    def quantize_encrypt_model_dev(self, it, idx, scheme, n, n_jobs, first, count, layers, element_bits, u, ct):
        """The fused quantise -> encrypt over elements [first, first + count) of a FLATTENED model of n values (PRF counters and, for
        int_bits <= 64, the chunking run across the layers, as in a reference job: jzf_aggregator.py:721-741).  layers: (start, device
        pointer of the layer's own first value, alpha, is_f64) in ascending start order; u / ct address element `first`."""
        arr, nl = self._codec_layers(layers)
        self._check(self._lib.flashe_quantize_encrypt_model_dev(self._h, it, idx, scheme, n, n_jobs, first, count, arr, nl, element_bits,
                                                                self._ptr(u), self._ptr(ct)))

    def decrypt_unquantize_model_dev(self, it, add_idx, minus_idx, n, n_jobs, first, count, inp, layers, element_bits, num_clients, out):
        """The fused decrypt -> unquantise of the same flattened vector: layers = (start, None, alpha, False) per layer."""
        pa, _a = _u32_list(add_idx)
        pm, _m = _u32_list(minus_idx)
        arr, nl = self._codec_layers(layers)
        self._check(self._lib.flashe_decrypt_unquantize_model_dev(self._h, it, pa, len(add_idx), pm, len(minus_idx), n, n_jobs, first, count,
                                                                  self._ptr(inp), arr, nl, element_bits, num_clients, self._ptr(out)))

    def unquantize_model_dev(self, n, first, count, inp, layers, element_bits, num_clients, out):
        """The codec back end alone over elements [first, first + count) of a flattened, already decrypted vector (the sparse job's way back)."""
        arr, nl = self._codec_layers(layers)
        self._check(self._lib.flashe_unquantize_model_dev(self._h, n, first, count, self._ptr(inp), arr, nl, element_bits, num_clients, self._ptr(out)))

    @staticmethod
    def _batch_layers(layers):
        """layers: iterable of (size, x device pointer or None, alpha, x_is_f64) -> ctypes array of flashe_batch_layer."""
        layers = list(layers)
        arr = (_lib.BatchLayer * max(len(layers), 1))()
        for i, (size, x, alpha, is_f64) in enumerate(layers):
            arr[i].size, arr[i].x_dev, arr[i].alpha, arr[i].x_is_f64, arr[i].reserved = int(size), x, float(alpha), 1 if is_f64 else 0, 0
        return arr, len(layers)

    def quantize_batch_model_dev(self, layers, element_bits, field_bits, u, n_elems, out):
        """The batched plaintext of a whole model in one launch: every layer quantised with its own alpha and batched on its own
        (int_bits // field_bits values per element, zero padded), the batched layers back to back in `out` (n_elems x L limbs)."""
        arr, nl = self._batch_layers(layers)
        self._check(self._lib.flashe_quantize_batch_model_dev(self._h, arr, nl, element_bits, field_bits, self._ptr(u), n_elems, self._ptr(out)))

    def unbatch_unquantize_model_dev(self, layers, element_bits, field_bits, num_clients, inp, n_elems, out):
        """The way back: the decrypted flattened batched vector -> the model's float64 values in walking order, one launch."""
        arr, nl = self._batch_layers(layers)
        self._check(self._lib.flashe_unbatch_unquantize_model_dev(self._h, arr, nl, element_bits, field_bits, num_clients, self._ptr(inp), n_elems,
                                                                  self._ptr(out)))

    def shift_dev(self, n, x, x_is_f64, shift, wide=False):
        """x <- x + shift in place (normalize: shift = -mean)."""
        self._check(self._lib.flashe_shift_dev(self._h, n, self._ptr(x), 1 if x_is_f64 else 0, float(shift), 1 if wide else 0))

    def mean_std_dev(self, n, x, x_is_f64):
        """(mean, std) of a device vector, float64 two-pass reduction (synchronous)."""
        m, s = ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.flashe_mean_std_dev(self._h, n, self._ptr(x), 1 if x_is_f64 else 0, ctypes.byref(m), ctypes.byref(s)))
        return float(m.value), float(s.value)

    def quantize(self, x, alpha, element_bits, u):
        x = np.ascontiguousarray(x)
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        x = x.reshape(-1)
        if u.shape[0] != x.shape[0]:
            raise ValueError("need one uniform draw per element")
        q = np.zeros(x.shape[0], dtype=np.uint64)
        self._check(self._lib.flashe_quantize(self._h, x.shape[0], x.ctypes.data, 1 if x.dtype == np.float64 else 0,
                                              float(alpha), element_bits, u.ctypes.data, q.ctypes.data))
        return q

    def unquantize(self, v, alpha, element_bits, num_clients):
        v = np.ascontiguousarray(v, dtype=np.uint64)
        if v.ndim == 1:
            v = v.reshape(-1, 1)
        out = np.zeros(v.shape[0], dtype=np.float64)
        self._check(self._lib.flashe_unquantize(self._h, v.shape[0], v.ctypes.data, v.shape[1], float(alpha), element_bits,
                                                num_clients, out.ctypes.data))
        return out

    def batch(self, vals, field_bits):
        vals = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1)
        bs = self.int_bits // field_bits
        nb = (vals.shape[0] + bs - 1) // bs
        out = np.zeros((nb, self.limbs), dtype=np.uint64)
        self._check(self._lib.flashe_batch(self._h, vals.shape[0], vals.ctypes.data, field_bits, out.ctypes.data))
        return out

    def unbatch(self, batched, field_bits):
        batched = self._vec(batched)
        bs = self.int_bits // field_bits
        out = np.zeros(batched.shape[0] * bs, dtype=np.uint64)
        self._check(self._lib.flashe_unbatch(self._h, batched.shape[0], batched.ctypes.data, field_bits, out.ctypes.data))
        return out

    # -- top-k sparsifier (Client.sparsify, jzf_aggregator.py:578-623) ---------------------------------
    def sparsify_dev(self, n, k, x, x_is_f64, residual, loc, vals):
        self._check(self._lib.flashe_sparsify_dev(self._h, n, k, self._ptr(x), 1 if x_is_f64 else 0, self._ptr(residual),
                                                  self._ptr(loc), self._ptr(vals)))

    def sparsify_batch_dev(self, ns, ks, x, x_is_f64, residual, loc, vals):
        """Top-k of every layer of a model in one set of launches: layers back to back in the flat device vectors x / residual, outputs
        back to back in loc / vals (locations relative to their layer)."""
        L = len(ns)
        an = (c_u64 * max(L, 1))(*[int(v) for v in ns])
        ak = (c_u64 * max(L, 1))(*[int(v) for v in ks])
        self._check(self._lib.flashe_sparsify_batch_dev(self._h, L, an, ak, self._ptr(x), 1 if x_is_f64 else 0, self._ptr(residual),
                                                        self._ptr(loc), self._ptr(vals)))

    def sparsify_tensors_dev(self, n, layers, ks, residual, loc, vals, packed=None, bits=0):
        """Top-k of every layer where its owner keeps it (flashe_sparsify_tensors_dev): layers = [(start, ptr, dtype code)] in model order,
        ks the entries each keeps.  The residual / value buffers hold layer after layer in its compute type (float64 for TENSOR_F64, else
        float32), each aligned to its element size; loc receives the model-wide locations, packed (optional) `_to_bytes(loc, bits)`."""
        arr, nl = self._tensor_layers([(start, ptr, 1.0, 0.0, dtype, 0) for start, ptr, dtype in layers])
        ak = (c_u64 * max(nl, 1))(*[int(v) for v in ks])
        self._check(self._lib.flashe_sparsify_tensors_dev(self._h, int(n), arr, nl, ak, self._ptr(residual), self._ptr(loc), self._ptr(vals),
                                                          self._ptr(packed), int(bits)))

    def sparsify_cohort_tensors_dev(self, n, layers, ks, srcs, dtypes, residual, residual_stride, loc, loc_stride, vals, vals_stride, packed=None,
                                    packed_stride=0, bits=0):
        """sparsify_tensors_dev for C models of one shape in one set of launches (flashe_sparsify_cohort_tensors_dev): layers = the shared
        table [(start, compute dtype code)], srcs[c][l] / dtypes[c][l] = client c's layer l and its storage dtype; client c's residuals,
        values, locations and packed locations are block c of the equal-stride buffers (byte strides for residual / vals, entries for loc,
        limbs for packed), each block in sparsify_tensors_dev's layout."""
        arr, nl = self._tensor_layers([(start, None, 1.0, 0.0, dtype, 0) for start, dtype in layers])
        C, ps, pd = self._cohort_sources(srcs, dtypes, nl)
        ak = (c_u64 * max(nl, 1))(*[int(v) for v in ks])
        self._check(self._lib.flashe_sparsify_cohort_tensors_dev(self._h, C, int(n), arr, nl, ak, ps, pd, self._ptr(residual), int(residual_stride),
                                                                 self._ptr(loc), int(loc_stride), self._ptr(vals), int(vals_stride), self._ptr(packed),
                                                                 int(packed_stride), int(bits)))

    def quantize_cohort_dev(self, n, layers, srcs, dtypes, element_bits, u, u_stride, zzz, zzz_is_f64, pts, tails, zeros):
        """The sparse job's codec front end for a cohort in one launch (flashe_quantize_cohort_dev): layers = the shared compact table
        (start, None, alpha, shift, compute dtype code, flags); srcs[c][l] / dtypes[c][l] = client c's compact layer l; client c's value j
        takes the draw u[c * u_stride + j], its 'zzz' value zzz[c] the draw u[c * u_stride + n]; pts[c] = its n one-limb plaintexts,
        tails[c] (or None) = where its quantised 'zzz' goes as a ciphertext-width element; zeros = device uint64[C] of those values."""
        arr, nl = self._tensor_layers(layers)
        C, ps, pd = self._cohort_sources(srcs, dtypes, nl)
        pz = (ctypes.c_double * max(C, 1))(*[float(z) for z in zzz])
        pp, _kp = self._ptr_array(pts)
        pt, _kt = self._ptr_array(tails) if tails is not None else (None, None)
        self._check(self._lib.flashe_quantize_cohort_dev(self._h, C, int(n), arr, nl, ps, pd, int(element_bits), self._ptr(u), int(u_stride), pz,
                                                         1 if zzz_is_f64 else 0, pp, pt, self._ptr(zeros)))

    def quantize_encrypt_sparse_cohort_dev(self, it, idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, u_stride, zzz, zzz_is_f64, cts, zeros):
        """quantize_cohort_dev and the clients' single-mask encrypts as ONE chained launch from the floats
        (flashe_quantize_encrypt_sparse_cohort_dev, int_bits 16 / 20 / 23 / 24 / 32): layers, srcs, dtypes, u, u_stride, zzz, zzz_is_f64 and
        zeros as quantize_cohort_dev takes them; idx[c] = client c's cipher index; cts[c] = its upload of n + 1 one-limb elements (n
        ciphertexts, then the plain quantised 'zzz').  Returns False -- nothing was launched -- when the library declines the shape
        (FLASHE_ENOTSUP: the caller runs quantize_cohort_dev and the encrypts), True otherwise."""
        arr, nl = self._tensor_layers(layers)
        C, ps, pd = self._cohort_sources(srcs, dtypes, nl)
        pz = (ctypes.c_double * max(C, 1))(*[float(z) for z in zzz])
        ii = (ctypes.c_uint32 * max(C, 1))(*[int(v) for v in idx])
        pc, _kc = self._ptr_array(cts)
        rc = self._lib.flashe_quantize_encrypt_sparse_cohort_dev(self._h, it, C, ii, int(n), n_jobs, arr, nl, ps, pd, int(element_bits), self._ptr(u),
                                                                 int(u_stride), pz, 1 if zzz_is_f64 else 0, pc, self._ptr(zeros))
        return self._took(rc)

    def sparsify_batch(self, layers, ks, residuals=None):
        """[(loc uint32[k_l] ascending, vals[k_l], new residual or None) per layer] -- Client.sparsify's layer loop
        (jzf_aggregator.py:585-613) as ONE upload, one set of launches and one download.  All layers share one float type."""
        flats = [np.ascontiguousarray(l).reshape(-1) for l in layers]
        dt = np.result_type(*[f.dtype for f in flats]) if flats else np.float64
        if dt not in (np.float32, np.float64):
            dt = np.float64
        ns = [int(f.size) for f in flats]
        ks = [int(v) for v in ks]
        x = np.concatenate([f.astype(dt, copy=False) for f in flats]) if flats else np.zeros(0, dtype=dt)
        res = None
        if residuals is not None:
            res = np.concatenate([np.ascontiguousarray(r, dtype=dt).reshape(-1) for r in residuals]) if flats else np.zeros(0, dtype=dt)
        loc = np.zeros(sum(ks), dtype=np.uint32)
        vals = np.zeros(sum(ks), dtype=dt)
        L = len(ns)
        an = (c_u64 * max(L, 1))(*ns)
        ak = (c_u64 * max(L, 1))(*ks)
        self._check(self._lib.flashe_sparsify_batch(self._h, L, an, ak, x.ctypes.data, 1 if dt == np.float64 else 0,
                                                    res.ctypes.data if res is not None else None, loc.ctypes.data, vals.ctypes.data))
        out, o, q = [], 0, 0
        for n_l, k_l in zip(ns, ks):
            out.append((loc[q:q + k_l], vals[q:q + k_l], None if res is None else res[o:o + n_l]))
            o += n_l
            q += k_l
        return out

    def sparsify_model(self, layers, ks, residual_dev=None, dtype=None):
        """sparsify_batch for a caller that keeps the residuals ON THE DEVICE between rounds: every layer is copied straight into its
        slot of one flat device buffer (no host-side concatenation), residual_dev (a DeviceBuffer of the flat residuals, updated in
        place; None = no residual) never crosses PCIe, only the k_l selected entries come back.  -> [(loc, vals) per layer]."""
        flats = [np.ascontiguousarray(l).reshape(-1) for l in layers]
        dt = np.dtype(dtype) if dtype is not None else (np.result_type(*[f.dtype for f in flats]) if flats else np.dtype(np.float64))
        if dt not in (np.float32, np.float64):
            dt = np.dtype(np.float64)
        ns = [int(f.size) for f in flats]
        ks = [int(v) for v in ks]
        total, total_k = sum(ns), sum(ks)
        dx = self.alloc(max(total * dt.itemsize, 16))
        off = 0
        for f in flats:
            f = f.astype(dt, copy=False)
            if f.size:
                self._check(self._lib.flashe_memcpy_h2d(self._h, dx.ptr + off, f.ctypes.data, f.nbytes))
            off += f.nbytes
        dl, dv = self.alloc(max(4 * total_k, 16)), self.alloc(max(dt.itemsize * total_k, 16))
        self.sparsify_batch_dev(ns, ks, dx, dt == np.float64, residual_dev, dl, dv)
        loc, vals = dl.download(np.uint32, total_k), dv.download(dt, total_k)
        out, q = [], 0
        for k_l in ks:
            out.append((loc[q:q + k_l], vals[q:q + k_l]))
            q += k_l
        return out

    def sparsify(self, layer, k, residual=None):
        """-> (loc uint32[k] ascending, vals[k] = layer + residual at loc, new residual or None)."""
        layer = np.ascontiguousarray(layer).reshape(-1)
        if layer.dtype not in (np.float32, np.float64):
            layer = layer.astype(np.float64)
        res = None if residual is None else np.ascontiguousarray(residual, dtype=layer.dtype).reshape(-1).copy()
        loc = np.zeros(k, dtype=np.uint32)
        vals = np.zeros(k, dtype=layer.dtype)
        self._check(self._lib.flashe_sparsify(self._h, layer.shape[0], k, layer.ctypes.data, 1 if layer.dtype == np.float64 else 0,
                                              res.ctypes.data if res is not None else None, loc.ctypes.data, vals.ctypes.data))
        return loc, vals, res
