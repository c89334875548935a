"""ctypes binding of libmvs_hip.so (C ABI: include/mvs_hip.h).

There is NO fallback: if the gfx950 library has not been built (``python -m mvsformerplusplus_amd.build``)
importing an op raises, and every op refuses tensors that are not on a ROCm device.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

import torch

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# MVS_HIP_LIB: measurement scripts point the binding at a variant build of the SAME C ABI (build.build(out=...)); unset = the product library
LIB_PATH = os.environ.get("MVS_HIP_LIB") or os.path.join(_HERE, "csrc", "libmvs_hip.so")

# named literals (greppable) of the header's enumerators; tests/test_abi_and_host.py holds every one of them to the header's value
OK = 0
ABI_VERSION = _header.CONSTANTS["MVS_ABI_VERSION"]
TR_EPI_BIAS, TR_EPI_GELU, TR_EPI_RES_LN = 0, 1, 2
DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
HEAD_CE_EVAL, HEAD_CE_TRAIN, HEAD_REG = 0, 1, 2
LAYOUT_PLANAR, LAYOUT_OCTET_TILED = 0, 1
REG_COSTREGNET, REG_COSTREGNET3D = 0, 1
PREC_FP32, PREC_BF16X3, PREC_BF16P, PREC_BF16X3_SPLIT, PREC_F16X2, PREC_ATTN16, PREC_F16, PREC_F16MIX = 0, 1, 2, 3, 4, 5, 6, 7
PRECISIONS = {"fp32": PREC_FP32, "bf16x3": PREC_BF16X3, "f16x2": PREC_F16X2, "f16": PREC_F16, "f16mix": PREC_F16MIX}
F16_FORMATS = ("f16x2", "f16", "f16mix")        # conv_precision values whose regulariser ACTIVATIONS are fp16 tensors (they share packed weights)
F16_CODES = (PREC_F16X2, PREC_F16, PREC_F16MIX)
VOLUME_F32, VOLUME_SPLIT, VOLUME_F16 = 0, 1, 2
CORR_F16, CORR_F32 = 0, 1


class MvsHipError(RuntimeError):
    pass


def bind(path: str) -> C.CDLL:
    """Load a build of the C ABI and attach the prototype of every function include/mvs_hip.h declares (_header.py reads them)."""
    lib = C.CDLL(path)
    for name, (res, args) in _header.PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.mvs_abi_version() != ABI_VERSION:
        raise MvsHipError("libmvs_hip ABI version mismatch: %d" % lib.mvs_abi_version())
    return _GuardedLib(lib, _header.STATUS)


_LIB: Optional[C.CDLL] = None
_REQUIRE_DEVICE = True        # product behaviour; only tests/hipemu flips this for host-emulated kernels


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise MvsHipError("%s not found: build the gfx950 HIP library first (python -m mvsformerplusplus_amd.build). "
                              "There is no CPU/PyTorch fallback for this path." % LIB_PATH)
        _LIB = bind(LIB_PATH)
    return _LIB


def _failed(L, what: str, rc: int) -> MvsHipError:
    msg = L.mvs_last_error()
    return MvsHipError("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else "?"))


def check(rc: int, what: str = "") -> None:
    """For a status code held in hand.  A bound library checks the functions the header declares mvs_status itself (_GuardedLib)."""
    if rc != OK:
        raise _failed(lib(), what or "libmvs_hip call", rc)


class _CallDevices(threading.local):
    """Devices of the tensors handed to ptr() while the arguments of ONE C-ABI call are evaluated - per thread (DataParallel
    replicas and autograd's per-device worker threads issue calls concurrently)."""

    def __init__(self):
        self.devs = []


_CALL_DEVICE = _CallDevices()


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Raw address of a dense tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise MvsHipError("internal: non-contiguous tensor handed to the C ABI")
    if _REQUIRE_DEVICE and not t.is_cuda:
        raise MvsHipError("libmvs_hip needs tensors on a ROCm device (got %s); there is no CPU path" % t.device)
    if t.is_cuda:
        _CALL_DEVICE.devs.append(t.device)
    return t.data_ptr()


class _GuardedLib:
    """Every C-ABI call runs with the tensors' device made current (HIP resolves the null stream and launches on the CURRENT
    device, not on the device that owns the pointers), and refuses tensors spread over several devices - what torch's own ops
    do with their device guard.  Python evaluates `lib.mvs_x` (this __getattr__: the record is cleared, so a ptr() that raised in an
    earlier, abandoned argument list leaves nothing behind), then the arguments (ptr() records the devices), then makes the call.
    A function the header declares mvs_status raises MvsHipError on a non-zero code, so no call site checks; predicates and
    counters return their value.  *_bytes / *_floats / mvs_abi_version / mvs_last_error take no tensors and are not wrapped."""

    def __init__(self, cdll, status=frozenset()):
        self._cdll = cdll
        self._status = status            # the functions the header declares mvs_status: a non-zero result raises
        self._calls = {}                 # name -> guarded wrapper, built on first use

    def __getattr__(self, name):
        call = self._calls.get(name)
        if call is None:
            fn = getattr(self._cdll, name)
            if not name.startswith("mvs_") or name in ("mvs_abi_version", "mvs_last_error") or name.endswith("_bytes") or name.endswith("_floats"):
                setattr(self, name, fn)      # unguarded, and found without __getattr__ from now on
                return fn
            call = self._calls[name] = self._guarded(name, fn, name in self._status)
        del _CALL_DEVICE.devs[:]
        return call

    def _guarded(self, name, fn, is_status):
        def call(*args):
            devs = set(_CALL_DEVICE.devs)
            del _CALL_DEVICE.devs[:]
            if len(devs) > 1:
                raise MvsHipError("%s: tensors on different devices %s" % (name, sorted(str(d) for d in devs)))
            dev = devs.pop() if devs else None
            if dev is not None and torch.cuda.current_device() != dev.index:
                with torch.cuda.device(dev):
                    rc = fn(*args)
            else:
                rc = fn(*args)
            if rc and is_status:
                raise _failed(self._cdll, name, rc)        # the message of THIS library, which need not be lib()
            return rc
        return call


def stream_of(t: torch.Tensor) -> Optional[int]:
    """The caller's current HIP stream ON THE TENSOR'S DEVICE (work is enqueued there, like any torch op)."""
    if t.is_cuda:
        return torch.cuda.current_stream(t.device).cuda_stream
    return None
