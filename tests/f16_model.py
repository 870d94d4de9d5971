"""CPU model of the one-pass fp16 mode (ABI BSVD_F16, include/bsvd_hip.h) for TESTS ONLY, built on tests/split_model.py.

BSVD_F16 is the BSVD_F16X3 data contract with ONE MFMA pass: the operands are hi(w) = fp16(w) and hi(x) = fp16(x) -- for the Winograd form the
hi of each TRANSFORMED value's pair --, accumulated in fp32; nothing reads a `lo` half into an operand.  Behind the accumulator the layer is
split_model.finish: bias, activation, PS_ADD / RESID on operands decoded from full pairs.

`direct_one_pass` is direct_three_pass with x_lo = 0 and w_pairs = (w_hi, 0); `wino_one_pass` is the split branch of split_model._wino
keeping only Uh . Vh.  The tolerance of the GPU tests is split_model.bound with the three-pass mode's margins (M_DIRECT, M_WINO[2]): the
one-pass accumulation chain is a subset of the chain those margins were measured on.

`F16EmuExecutor` is the whole-network emulation: the oracle-backed executor with every MFMA layer's conv input and weights rounded to
fp16 and float64 accumulation.
"""
import numpy as np
import torch

import split_model as S
from oracle_exec import OracleExecutor

M_DIRECT = S.M_DIRECT
M_WINO2 = S.M_WINO[2]


def direct_one_pass(sp, x_hi, x_lo, w, bias=None, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1,
                    y_planar=None, w_pairs=None):
    """the reference of the mode for one fused direct-form layer.  Same signature as split_model.direct_three_pass so that a test can run
    both on the same operands: x_lo, the lo halves of the halos (halo_*: None or a pair of Halos, hi values / lo values) and w_pairs[1]
    are accepted and NOT read.  `extra` is the decoded skip / base tensor (full pairs)."""
    del x_lo
    w_hi = S.pairs(w)[0] if w_pairs is None else w_pairs[0]
    return S.finish(sp, S._lin(sp, x_hi, w_hi, S._h(halo_prev, 0), S._h(halo_next, 0)), bias, extra, extra_pstride, extra_cstride, y_planar)


def _wino_one_pass_pre(sp, x, w, m, halo_prev=None, halo_next=None, u_pairs=None):
    """split_model._wino's split branch with the two lo passes left out: float64 transforms, hi(V) and hi(U), one pass.  NCHW, no bias."""
    assert sp.stride == 1
    f = S.WINO[m]
    A = m + 2
    v = S.gather(sp, torch.as_tensor(S._np(x)).double(), halo_prev, halo_next).numpy()
    T, cin, H, W = v.shape
    nq = (W + m - 1) // m
    dp = np.zeros((T, cin, H + 2, nq * m + 2))
    dp[:, :, 1:H + 1, 1:W + 1] = v
    d = np.stack([dp[..., i:i + (nq - 1) * m + 1:m] for i in range(A)], axis=-1)
    V = np.einsum("xi,tcrqi->xtcrq", f["BT"], d)
    U = np.einsum("xk,ocyk->xocy", f["G"], np.asarray(S._np(w), dtype=np.float64))
    Vh = S.pairs(V)[0]
    Uh = S.pairs(U)[0] if u_pairs is None else u_pairs[0]
    M = np.zeros((A, T, U.shape[1], H, nq))
    for ky in range(3):
        M += S._bmm(Uh[..., ky], Vh[:, :, :, ky:ky + H])
    out = np.einsum("jx,xtorq->torqj", f["AT"], M)
    return out.reshape(T, U.shape[1], H, nq * m)[..., :W]


def wino_one_pass(sp, x, w, m=2, bias=None, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1):
    """the reference of the mode for a Winograd-form layer: x is the DECODED input (hi + lo; the kernel decodes before it transforms, so
    the input's own lo halves DO count -- what is dropped is the lo of the transformed pair)"""
    return S.finish(sp, _wino_one_pass_pre(sp, x, w, m, halo_prev, halo_next), bias, extra, extra_pstride, extra_cstride)


def _r16(t):
    return torch.as_tensor(t).float().clamp(-S.F16_MAX, S.F16_MAX).half().float()


class F16EmuExecutor(OracleExecutor):
    """OracleExecutor whose MFMA layers (every layer whose key is not in ``fp32_keys``) run on conv input and weights rounded to fp16,
    accumulated in float64; bias, activation and the epilogue's second operand stay fp32 values.  ``issued`` logs (key, 'f16' | 'fp32')."""

    def __init__(self, state, fp32_keys=()):
        super().__init__(state, double=True)
        self.state32 = self.state
        self.state16 = {k: (_r16(v) if k.endswith(".weight") else v) for k, v in self.state.items()}
        self.fp32_keys = set(fp32_keys)
        self.issued = []

    def conv(self, sp, x, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1,
             x_planar=False, y_planar=None, out=None):
        if out is not None:
            out.copy_(self.conv(sp, x, halo_prev, halo_next, extra, extra_pstride, extra_cstride, x_planar, y_planar))
            return out
        if sp.key in self.fp32_keys:
            self.issued.append((sp.key, "fp32"))
            return super().conv(sp, x, halo_prev, halo_next, extra, extra_pstride, extra_cstride, x_planar, y_planar)
        self.issued.append((sp.key, "f16"))
        rh = lambda h: None if h is None else type(h)(_r16(h.t), h.pstride, h.coff)
        self.state = self.state16
        try:
            return super().conv(sp, _r16(x), rh(halo_prev), rh(halo_next), extra, extra_pstride, extra_cstride, x_planar, y_planar)
        finally:
            self.state = self.state32
