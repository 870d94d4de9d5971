"""Stale state under the tests' control (test infrastructure; tests/test_gpu_stale.py, tests/test_stale_cpu.py).

A result may depend on state the launch did not write itself in two places, and this module poisons both:

* LDS.  tests/native/libstale_probe.so (stale_probe.hip, built by tests/native/Makefile) fills the whole LDS of every CU with a pattern;
  the product launch that follows ON THE SAME STREAM, with nothing in between, then reads that pattern wherever it reads a cell it did not
  write.  ``lds_probe(launch, result)`` = clean launch, poison 0xFFFFFFFF + launch, poison 0x3C003C00 + launch; the three results must have
  the same bits.  Two patterns: an fp32 / fp16 NaN reaches a result through any arithmetic but is laundered by fmaxf / v_med3 (into 0 or 6),
  a finite value (1.0 in both fp16 halves, 0.0078 as fp32) passes those and is killed by a zero mask.
* Allocations.  ``poisoned_empty(monkeypatch, fill)`` wraps torch.empty and its kin so that every device (and pinned host) result has all its
  bytes set to ``fill``: a schedule that reads a ring slot, pad channel, halo buffer or edge record before something wrote it gives other bits
  for 0x00 than for 0xFF.
"""
import contextlib
import ctypes
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "native", "libstale_probe.so")
NAN_PATTERN = 0xFFFFFFFF          # a NaN as fp32 and in both fp16 halves
FINITE_PATTERN = 0x3C003C00       # 1.0 in both fp16 halves, 7.8e-3 as fp32
PATTERNS = (NAN_PATTERN, FINITE_PATTERN)
# the poison grid = GRID_MULTIPLE x CU count workgroups, each holding HOLD_SLEEPS x s_sleep(127) (127 x 64 clocks, ~3.4 us at 2.4 GHz) after
# its fill: chosen on the MI355X so that one call reaches every CU (profiles/stale_state.txt)
GRID_MULTIPLE = 4
HOLD_SLEEPS = 8

_lib = None


def load():
    global _lib
    if _lib is None:
        lib = ctypes.CDLL(LIB)
        u32p, vp = ctypes.c_void_p, ctypes.c_void_p
        lib.stale_lds_bytes.restype = ctypes.c_int
        lib.stale_grid.restype = ctypes.c_int
        lib.stale_configure.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.stale_poison.argtypes = [ctypes.c_uint32, vp, u32p]
        lib.stale_canary.argtypes = [ctypes.c_uint32, vp, u32p]
        for f in (lib.stale_demo_good, lib.stale_demo_bad):
            f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, vp]
        assert lib.stale_configure(GRID_MULTIPLE, HOLD_SLEEPS) == 0
        _lib = lib
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_IDS = {}


def _ids_buffer(lib):
    """one record array per grid size, allocated once: nothing of torch's runs between a poison and the launch under test"""
    n = lib.stale_grid()
    assert n > 0, n
    if n not in _IDS:
        _IDS[n] = torch.zeros(n, dtype=torch.int32, device="cuda")
    return _IDS[n]


def poison(pattern):
    """fills the LDS of every CU with ``pattern`` on the current stream (asynchronous); returns the device array of the workgroups' CU ids"""
    lib = load()
    ids = _ids_buffer(lib)
    rc = lib.stale_poison(pattern, _stream(), ids.data_ptr())
    assert rc == ids.numel(), rc
    return ids


def coverage(pattern=NAN_PATTERN):
    """the set of CU ids one poison call ran on"""
    ids = poison(pattern)
    torch.cuda.synchronize()
    return set(ids.cpu().tolist())


def canary(pattern):
    """{CU id: [words still holding ``pattern``, one entry per canary workgroup that ran there]}, and the words a workgroup reads"""
    lib = load()
    out = torch.zeros(2 * lib.stale_grid(), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = lib.stale_canary(pattern, _stream(), out.data_ptr())
    assert rc == out.numel() // 2, rc
    torch.cuda.synchronize()
    seen = {}
    for cu, n in out.cpu().view(-1, 2).tolist():
        seen.setdefault(cu, []).append(n)
    return seen, lib.stale_lds_bytes() // 4


def lds_probe(launch, result):
    """``launch()`` issues the kernel(s) under test on the current stream through the library's own entry points (no torch kernel), ``result()``
    returns the tensor(s) they wrote.  Returns [clean, after the NaN pattern, after the finite pattern] as host copies."""
    load()
    torch.cuda.synchronize()
    runs = []
    for pattern in (None,) + PATTERNS:
        if pattern is not None:
            poison(pattern)
        launch()
        torch.cuda.synchronize()
        r = result()
        runs.append([t.detach().cpu().clone() for t in (r if isinstance(r, (list, tuple)) else [r])])
    return runs


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def probe_verdict(runs):
    """what every LDS case asserts of lds_probe's three results: the same bits, and no NaN"""
    clean = runs[0]
    return {"nan pattern": all(same_bits(a, b) for a, b in zip(clean, runs[1])),
            "finite pattern": all(same_bits(a, b) for a, b in zip(clean, runs[2])),
            "no NaN": not any(bool(torch.isnan(t).any()) for r in runs for t in r if t.is_floating_point())}


# ------------------------------------------------------------------------------------------------ allocations

def _device_or_pinned(t):
    return t.is_cuda or t.is_pinned()


def fill_bytes(t, fill):
    """every byte of the storage behind ``t`` (a fresh allocation owns all of it, strided or not).  The fill is complete on return: an
    allocation is ordered against no stream, so the caller may hand the tensor to any stream at once (pipeline.ClipPipeline uploads into a
    fresh staging buffer on its own stream) -- a fill still in flight on the allocating stream would race with that."""
    n = t.untyped_storage().nbytes()
    if n:
        torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage(), 0, (n,), (1,)).fill_(fill)
        if t.is_cuda:
            torch.cuda.current_stream(t.device).synchronize()


@contextlib.contextmanager
def poisoned_empty(monkeypatch, fill, where=_device_or_pinned):
    """Inside: torch.empty, torch.empty_like, torch.empty_strided and Tensor.new_empty give tensors whose bytes are all ``fill`` wherever
    ``where(tensor)`` holds (default: device memory and pinned host memory; the CPU tests pass their own).  Nothing is filled while the
    current stream is capturing (a fill would become a node of the graph).  The originals are back on exit."""
    fill = int(fill) & 0xFF

    def wrap(fn):
        def poisoned(*a, **kw):
            t = fn(*a, **kw)
            capturing = t.is_cuda and torch.cuda.is_current_stream_capturing()
            if not capturing and where(t):
                fill_bytes(t, fill)
            return t
        poisoned.__wrapped__ = fn
        return poisoned

    with monkeypatch.context() as mp:
        for owner, name in ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty")):
            mp.setattr(owner, name, wrap(getattr(owner, name)))
        yield
