"""torch.ops.truss_mi355.* -- the env step as PyTorch custom operators.

`csrc/truss_torch_ops.cpp` registers one operator per native entry point of its table (`entries()` lists them) with the
dispatcher (CPU / CUDA(=HIP) / Meta keys): tensors in, outputs mutated in place, launched on the stream the caller names,
capturable in a hipGraph, traceable.  The operators do no arithmetic; they call the C ABI of the native library that
`bind()` registered under an index -- the HIP product library, or (test-suite only) the CPU lane emulator.  `bind()` hands
over the library's path; the entry points are looked up by name there.  A library without a required one is refused, the
optional ones (`_lib._ENTRIES`) stay null and their operators then fail with "the bound native library has no ...".

There is no fallback: without `libtruss_torch_ops.so` (built by `make -C mop-truss-marl_amd/csrc`) loading fails.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib

OPS_LIB = os.path.join(os.path.dirname(_lib.DEFAULT_LIB), "libtruss_torch_ops.so")
_dll = None
_ids: dict = {}


def _load():
    global _dll
    if _dll is None:
        if not os.path.exists(OPS_LIB):
            raise _lib.TrussError(f"PyTorch operator library not found: {OPS_LIB}\nbuild it with `python -c 'import __graft_entry__ as g; "
                                  "g.build()'` (or `make -C mop-truss-marl_amd/csrc`).")
        torch.ops.load_library(OPS_LIB)              # runs the TORCH_LIBRARY registrations
        _dll = C.CDLL(OPS_LIB)                       # the same image: for truss_torch_bind
        _dll.truss_torch_bind.restype = C.c_int
        _dll.truss_torch_bind.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_char_p)]
        _dll.truss_torch_entries.restype = C.c_char_p
    return _dll


def entries() -> list:
    """Symbols of the native entry points the operators call (the table of csrc/truss_torch_ops.cpp)."""
    return _load().truss_torch_entries().decode().split(",")


def bind(lib: "_lib.TrussLib") -> int:
    """Index under which the operators reach this native library's entry points."""
    if lib.path not in _ids:
        idx, missing = len(_ids), C.c_char_p()
        rc = _load().truss_torch_bind(idx, os.fsencode(lib.path), C.byref(missing))
        if rc != 0:
            why = {-1: "more than 8 native libraries bound?", -2: "the library is not loaded in this process"}.get(rc) \
                or f"the library does not export {missing.value.decode()}"
            raise _lib.TrussError(f"truss_torch_bind({lib.path}) failed: {why}")
        _ids[lib.path] = idx
    return _ids[lib.path]


def stream_of(device) -> int:
    """hipStream_t of torch's current stream on `device` as an integer (0 = the default stream / CPU)."""
    if device.type == "cuda":
        return torch.cuda.current_stream(device).cuda_stream
    return 0


def namespace():
    _load()
    return torch.ops.truss_mi355


def call(op, *args):
    """Run an operator; a failure reported by the native library / the operator's argument checks surfaces as
    TrussError (what the ctypes binding raised), anything else is passed through."""
    try:
        return op(*args)
    except RuntimeError as e:
        msg = str(e)
        if "truss_" in msg:
            raise _lib.TrussError(msg.split("\nException raised from")[0]) from None
        raise
