"""ctypes binding of the CPU model of the exact-fp32 mode (oracle/chain_ref.c).

TEST INFRASTRUCTURE ONLY.  ``conv3x3`` has the interface of ``oracle.conv_ref.conv3x3`` plus the chain's order, the documented-open
variants of it and the mutations the CPU tests use (see chain_ref.c); every operation is one fp32 fmaf / add / subtract.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_FP = ctypes.POINTER(ctypes.c_float)
ACT = {"none": 0, "relu": 1, "relu6": 2}

ORDER_MFMA, ORDER_EDGE = 0, 1
SWAP_K, BIAS_FIRST, TAP_MAJOR, ROUND11, DROP_TERM = 1, 2, 4, 8, 16


def build(force=False):
    so = os.path.join(_HERE, "libchain_ref.so")
    src = os.path.join(_HERE, "chain_ref.c")
    if force or not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", src, "-o", so, "-lm"])
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        _LIB.chain_conv3x3.restype = ctypes.c_int
        _LIB.chain_conv3x3.argtypes = ([_FP, _FP, _FP, ctypes.c_int, _FP, _FP] + [ctypes.c_int] * 7 + [_FP, _FP] +
                                       [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int])
    return _LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(_FP)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def conv3x3(cur, w, bias, prev_sl=None, next_sl=None, fold=0, stride=1, act="none", epilogue=0, extra=None, resid_ch=3, clamp=None,
            order=ORDER_MFMA, flags=0):
    """One frame, NCHW.  cur [Cin,H,W] -> [Cout,Ho,Wo] (epilogue 0/2) or [Cout/4,2Ho,2Wo] (epilogue 1)."""
    cur, w, bias, prev_sl, next_sl, extra = map(_c, (cur, w, bias, prev_sl, next_sl, extra))
    cin, h, wd = cur.shape
    cout = w.shape[0]
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    out = np.empty((cout // 4, 2 * ho, 2 * wo) if epilogue == 1 else (cout, ho, wo), dtype=np.float32)
    lo, hi = (0.0, 0.0) if clamp is None else clamp
    rc = lib().chain_conv3x3(_p(cur), _p(prev_sl), _p(next_sl), fold, _p(w), _p(bias), cin, cout, h, wd, stride, ACT[act], epilogue,
                             _p(extra), _p(out), min(resid_ch, cout), 0 if clamp is None else 1, lo, hi, order, flags)
    if rc != 0:
        raise ValueError("chain_conv3x3 rejected its arguments (%d)" % rc)
    return out
