"""CPU model of the split-fp16 arithmetic (ABI BSVD_F16X3, include/bsvd_hip.h) for TESTS ONLY: plain numpy / torch float64, no GPU, no
product code (netspec's ConvSpec is read for a layer's shape only).

A value v travels as an fp16 pair hi = fp16(v), lo = fp16(v - hi); a K block is three fp16 MFMAs, hi.hi + lo.hi + hi.lo, accumulated in
fp32.  `direct_three_pass` is the REFERENCE OF THE MODE: what a direct-form kernel computes when every pass reads the right operand, up to
the order of its fp32 accumulation.  It takes the two halves of every activation tensor separately: the kernels are linear in them, so a
test may feed halves that are not a canonical pair and see each pass at full strength.  `wino_model` is the same for the 1-D Winograd
forms F(2,3) / F(6,3) of bsvd_amd/csrc/wino_forms.h, whose pairs are formed from TRANSFORMED values.

The yardsticks of the GPU tests are the errors a plain float32 evaluation of the same operation makes on the same operands
(`fp32_chain`, `wino_fp32`); `bound` turns them into the tolerance.

Tensors: activations NHWC [T, H, W, C] (C == the layer's padded channel count; the tests use multiples of 16), weights [cout, cin, 3, 3],
results NHWC float64 in the oracle executor's conventions (tests/oracle_exec.py).  A temporal halo is a schedule.Halo(t, pstride, coff).
"""
from fractions import Fraction as Fr

import numpy as np
import torch
import torch.nn.functional as F

F16_MAX = 65504.0

# the margins of `bound` the GPU tests assert with (tests/test_gpu_split_passes.py, tests/test_gpu_range.py): the smallest powers of two the
# product kernels pass with on the MI355X.  Measured worst cases (profiles/f16x3_value_probes.txt): direct-form families 0.41 - 0.78 of
# the float32 chain's error and 1.007 for the planar exit with a split base; F(2,3) 0.69; F(6,3) 1.07.  Never above 8.
M_DIRECT = 2
M_WINO = {2: 1, 6: 2}
EPI_PLAIN, EPI_PS_ADD, EPI_RESID = 0, 1, 2

# ---------------------------------------------------------------------------------------------------------------------------------------
# the pair format


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def fp16(v, flush_subnormals=False):
    """round to nearest fp16 (saturating at +-65504 like the kernels' conversions), returned as float64"""
    h = np.clip(np.asarray(_np(v), dtype=np.float64), -F16_MAX, F16_MAX).astype(np.float16).astype(np.float64)
    if flush_subnormals:        # mutation: a conversion / MFMA that flushes fp16 subnormals
        h = np.where(np.abs(h) < 2.0 ** -14, 0.0, h)
    return h


def pairs(v, flush_subnormals=False):
    """(hi, lo) of the ABI: hi = fp16(v), lo = fp16(v - hi), both saturating; float64 arrays holding fp16 values"""
    v = np.asarray(_np(v), dtype=np.float64)
    hi = fp16(v, flush_subnormals)
    return hi, fp16(v - hi, flush_subnormals)


def container(hi, lo):
    """two fp16-valued halves [..., C] -> the split16 container (fp32 tensor [..., C]: per 16-channel chunk [hi x16 | lo x16]; C == 8: the
    compact half-chunk slice [hi x8 | lo x8]).  The halves need not be a canonical pair."""
    hi, lo = torch.as_tensor(_np(hi)), torch.as_tensor(_np(lo))
    *lead, C = hi.shape
    G = 16 if C % 16 == 0 else 8
    h, l = hi.reshape(*lead, C // G, G).to(torch.float16), lo.reshape(*lead, C // G, G).to(torch.float16)
    assert bool((h.double() == hi.reshape(h.shape).double()).all()) and bool((l.double() == lo.reshape(l.shape).double()).all()), \
        "container halves must be fp16 values"
    return torch.cat([h, l], dim=-1).contiguous().view(torch.float32).reshape(*lead, C)


def halves(s):
    """split16 container -> (hi, lo) float64 numpy arrays"""
    *lead, C = s.shape
    G = 16 if C % 16 == 0 else 8
    h = s.contiguous().view(torch.float16).reshape(*lead, C // G, 2 * G).double()
    return h[..., :G].reshape(*lead, C).numpy(), h[..., G:].reshape(*lead, C).numpy()


def lo_plane_weights(shape, rs, c=1.5 * 2.0 ** -5):
    """weights c + r with |r| just under half an fp16 ulp of c (c sits mid-binade): w_hi is the constant c everywhere and ALL the
    information is in w_lo -- the probe of the hi_x.lo_w pass and of the packer's lo plane"""
    ulp = 2.0 ** (np.floor(np.log2(c)) - 10)
    w = (c + 0.49 * ulp * rs.uniform(-1.0, 1.0, shape)).astype(np.float32)
    assert np.all(pairs(w)[0] == c)
    return w


# ---------------------------------------------------------------------------------------------------------------------------------------
# one fused layer, piece by piece (the conventions of oracle_exec.OracleExecutor.conv, in float64 throughout)


def _halo_slice(halo, hw, n):
    flat = torch.as_tensor(_np(halo.t)).reshape(-1)
    return torch.as_strided(flat, (hw, n), (halo.pstride, 1), storage_offset=flat.storage_offset() + halo.coff)


def gather(sp, x, halo_prev=None, halo_next=None):
    """NHWC [T,H,W,C] -> the conv's NCHW input [T,cin,H,W] (same dtype) after the temporal-shift gather"""
    x = torch.as_tensor(_np(x))
    T, H, W, _ = x.shape
    v = x[..., :sp.cin].permute(0, 3, 1, 2).contiguous()
    if sp.tsm:
        fold = sp.fold
        g = v.clone()
        g[:, :2 * fold] = 0
        if T > 1:
            g[:-1, :fold] = v[1:, :fold]
            g[1:, fold:2 * fold] = v[:-1, fold:2 * fold]
        if halo_next is not None:
            g[-1, :fold] = _halo_slice(halo_next, H * W, fold).t().reshape(fold, H, W).to(g.dtype)
        if halo_prev is not None:
            g[0, fold:2 * fold] = _halo_slice(halo_prev, H * W, fold).t().reshape(fold, H, W).to(g.dtype)
        v = g
    return v


def finish(sp, y, bias=None, extra=None, extra_pstride=0, extra_cstride=1, y_planar=None):
    """pre-bias conv result NCHW [T,cout,Ho,Wo] -> the layer's output (bias, activation, PS_ADD / RESID epilogue), NHWC float64"""
    y = torch.as_tensor(_np(y)).double()
    if bias is not None:
        y = y + torch.as_tensor(_np(bias)).double().reshape(1, -1, 1, 1)
    if sp.act == "relu6":
        y = y.clamp(0.0, 6.0)
    elif sp.act == "relu":
        y = y.clamp_min(0.0)
    T, _, Ho, Wo = y.shape
    if sp.epilogue == EPI_PS_ADD:
        cq = sp.cout // 4
        y = y.reshape(T, cq, 2, 2, Ho, Wo).permute(0, 1, 4, 2, 5, 3).reshape(T, cq, 2 * Ho, 2 * Wo)
        out = torch.zeros((T, 2 * Ho, 2 * Wo, sp.cout_pad // 4), dtype=torch.float64)
        out[..., :cq] = y.permute(0, 2, 3, 1)
        if extra is not None:
            e = torch.as_tensor(_np(extra)).double()
            ef = e.reshape(-1)
            ev = torch.as_strided(ef, (T, 4 * Ho * Wo, cq), (e[0].numel(), extra_pstride, extra_cstride))
            out[..., :cq] += ev.reshape(T, 2 * Ho, 2 * Wo, cq)
        return out
    out = torch.zeros((T, Ho, Wo, sp.cout_pad), dtype=torch.float64)
    out[..., :sp.cout] = y.permute(0, 2, 3, 1)
    if sp.epilogue == EPI_RESID:
        k = min(3, sp.cout)
        e = torch.as_tensor(_np(extra)).double()
        ef = e.reshape(-1)
        ev = torch.as_strided(ef, (T, Ho * Wo, k), (e[0].numel(), extra_pstride, extra_cstride))
        out[..., :k] = ev.reshape(T, Ho, Wo, k) - out[..., :k]
    if y_planar is not None:
        yc, clamp = y_planar
        out = out[..., :yc].permute(0, 3, 1, 2).contiguous()
        if clamp is not None:
            out = out.clamp(clamp[0], clamp[1])
    return out


def _lin(sp, x, w, hp=None, hn=None):
    """float64 conv3x3(gather(x), w), no bias: NCHW [T,cout,Ho,Wo]"""
    v = gather(sp, torch.as_tensor(_np(x)).double(), hp, hn)
    return F.conv2d(v, torch.as_tensor(_np(w)).double(), None, stride=sp.stride, padding=1)


def _h(halo, i):
    """halo given as a pair of Halos (hi values, lo values) -> half i; None stays None"""
    return None if halo is None else halo[i]


def _sum_halo(halo):
    if halo is None:
        return None
    return type(halo[0])(torch.as_tensor(_np(halo[0].t)).double() + torch.as_tensor(_np(halo[1].t)).double(), halo[0].pstride, halo[0].coff)


def direct_pre(sp, x_hi, x_lo, w, halo_prev=None, halo_next=None, drop=None, w_pairs=None):
    """the three passes, before bias: conv(x_hi, w_hi) + conv(x_lo, w_hi) + conv(x_hi, w_lo) in float64.  halo_*: None or a pair of Halos
    (hi values, lo values).  drop: mutation -- leave out one pass ('lo_x.hi_w' | 'hi_x.lo_w' | 'hi.hi').  w_pairs: mutation -- the
    packed weight halves to use instead of pairs(w)."""
    w_hi, w_lo = pairs(w) if w_pairs is None else w_pairs
    y = 0.0
    if drop != "hi.hi":
        y = y + _lin(sp, x_hi, w_hi, _h(halo_prev, 0), _h(halo_next, 0))
    if drop != "lo_x.hi_w":
        y = y + _lin(sp, x_lo, w_hi, _h(halo_prev, 1), _h(halo_next, 1))
    if drop != "hi_x.lo_w":
        y = y + _lin(sp, x_hi, w_lo, _h(halo_prev, 0), _h(halo_next, 0))
    return y


def direct_three_pass(sp, x_hi, x_lo, w, bias=None, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1,
                      y_planar=None, drop=None, w_pairs=None):
    """the reference of the mode for one fused direct-form layer (see the module docstring); `extra` is the decoded skip / base tensor"""
    return finish(sp, direct_pre(sp, x_hi, x_lo, w, halo_prev, halo_next, drop, w_pairs), bias, extra, extra_pstride, extra_cstride, y_planar)


def conv_f64(sp, x, w, bias=None, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1, y_planar=None):
    """the layer in float64 on decoded operands (halo_*: plain Halos of decoded values)"""
    return finish(sp, _lin(sp, x, w, halo_prev, halo_next), bias, extra, extra_pstride, extra_cstride, y_planar)


def format_terms(sp, x_hi, x_lo, w, halo_prev=None, halo_next=None):
    """the two deterministic error terms of the format, exactly from the operands (float64, NCHW pre-bias):
    sum |x| |w - (w_hi + w_lo)| (weight quantisation) and sum |x_lo| |w_lo| (the pass the mode drops).
    |three passes - float64 conv of (x_hi + x_lo, w)| <= their sum, element by element."""
    w = np.asarray(_np(w), dtype=np.float64)
    w_hi, w_lo = pairs(w)
    ab = lambda h: None if h is None else type(h)(torch.as_tensor(_np(h.t)).double().abs(), h.pstride, h.coff)
    x = np.abs(np.asarray(_np(x_hi), dtype=np.float64) + np.asarray(_np(x_lo), dtype=np.float64))
    quant = _lin(sp, x, np.abs(w - (w_hi + w_lo)), ab(_sum_halo(halo_prev)), ab(_sum_halo(halo_next)))
    lolo = _lin(sp, np.abs(_np(x_lo)), np.abs(w_lo), ab(_h(halo_prev, 1)), ab(_h(halo_next, 1)))
    return quant, lolo


def fp32_chain_pre(sp, x, w, halo_prev=None, halo_next=None):
    """conv3x3 of the decoded input with the fp32 weights as ONE float32 accumulation chain per output: tap by tap, channel by channel,
    a separately rounded multiply and add per term (numpy float32, vectorised over pixels and output channels).  NCHW, no bias."""
    v = gather(sp, torch.as_tensor(_np(x)).double(), halo_prev, halo_next).numpy().astype(np.float32)
    w = np.asarray(_np(w), dtype=np.float32)
    T, cin, H, W = v.shape
    s = sp.stride
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    vp = np.zeros((T, cin, H + 2, W + 2), dtype=np.float32)
    vp[:, :, 1:-1, 1:-1] = v
    acc = np.zeros((T, w.shape[0], Ho, Wo), dtype=np.float32)
    for ky in range(3):
        for kx in range(3):
            win = vp[:, :, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]
            for c in range(cin):
                acc += win[:, c, None] * w[None, :, c, ky, kx, None, None]
    return acc


def fp32_chain(sp, x, w, bias=None, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1, y_planar=None):
    """(layer through the float32 chain, layer in float64): the yardstick is the max-abs difference of the two"""
    pre = fp32_chain_pre(sp, x, w, halo_prev, halo_next)
    if bias is not None:
        pre = pre + np.asarray(_np(bias), dtype=np.float32).reshape(1, -1, 1, 1)
    return (finish(sp, pre, None, extra, extra_pstride, extra_cstride, y_planar),
            conv_f64(sp, x, w, bias, halo_prev, halo_next, extra, extra_pstride, extra_cstride, y_planar))


def chain_err(sp, x, w, bias=None, **kw):
    a, b = fp32_chain(sp, x, w, bias, **kw)
    return float((a - b).abs().max())


def bound(model, err_ref, m):
    """the tolerance of the GPU tests, elementwise: m x (the float32 reference's own max error) + the output pair's rounding"""
    return m * float(err_ref) + 2.0 ** -22 * torch.as_tensor(_np(model)).double().abs() + 2.0 ** -24


def needed(got, model, err_ref):
    """the margin m a result needs to pass `bound`: max over the elements of (|got - model| - the output pair's rounding) / err_ref"""
    model = torch.as_tensor(_np(model)).double()
    d = (torch.as_tensor(_np(got)).double() - model).abs() - (2.0 ** -22 * model.abs() + 2.0 ** -24)
    return max(0.0, float(d.max())) / float(err_ref)


def excess(got, model, err_ref, m):
    """max over the elements of |got - model| / bound: <= 1 passes"""
    model = torch.as_tensor(_np(model)).double()
    return float(((torch.as_tensor(_np(got)).double() - model).abs() / bound(model, err_ref, m)).max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the 1-D Winograd forms F(M,3) along x (bsvd_amd/csrc/wino_forms.h holds the same tables as constexpr C++; tests/test_split_model_cpu.py
# compares them entry by entry with what tests/native/wino_tables_dump.cpp prints from the header)

def _tab(rows):
    return np.array([[float(Fr(v)) for v in r] for r in rows], dtype=np.float64)


WINO = {
    2: dict(
        G=_tab([[1, 0, 0], ["1/2", "1/2", "1/2"], ["1/2", "-1/2", "1/2"], [0, 0, 1]]),
        BT=_tab([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]),
        AT=_tab([[1, 1, 1, 0], [0, 1, -1, -1]])),
    6: dict(
        G=_tab([["-64/9", 0, 0],
                ["32/21", "32/21", "32/21"],
                ["32/21", "-32/21", "32/21"],
                ["128/15", "64/15", "32/15"],
                ["128/15", "-64/15", "32/15"],
                ["-2048/315", "-512/105", "-128/35"],
                ["-2048/315", "512/105", "-128/35"],
                [0, 0, 1]]),
        BT=_tab([["-9/64", 0, "61/64", 0, "-29/16", 0, 1, 0],
                 [0, "9/64", "9/64", "-13/16", "-13/16", 1, 1, 0],
                 [0, "-9/64", "9/64", "13/16", "-13/16", -1, 1, 0],
                 [0, "9/32", "9/16", "-25/32", "-25/16", "1/2", 1, 0],
                 [0, "-9/32", "9/16", "25/32", "-25/16", "-1/2", 1, 0],
                 [0, "3/16", "1/4", "-15/16", "-5/4", "3/4", 1, 0],
                 [0, "-3/16", "1/4", "15/16", "-5/4", "-3/4", 1, 0],
                 [0, "-9/64", 0, "61/64", 0, "-29/16", 0, 1]]),
        AT=_tab([[1, 1, 1, 1, 1, 1, 1, 0],
                 [0, 1, -1, "1/2", "-1/2", "3/4", "-3/4", 0],
                 [0, 1, 1, "1/4", "1/4", "9/16", "9/16", 0],
                 [0, 1, -1, "1/8", "-1/8", "27/64", "-27/64", 0],
                 [0, 1, 1, "1/16", "1/16", "81/256", "81/256", 0],
                 [0, 1, -1, "1/32", "-1/32", "243/1024", "-243/1024", 1]])),
}


def _near_tie(v):
    """mask of the values whose PAIR is within 2^-20 of a quantum of a rounding tie: the pair resolves q = max(2^-24, ulp_fp16(v) 2^-11)"""
    q = np.maximum(2.0 ** -24, 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 1e-300))) - 21))
    t = np.abs(v) / q
    return np.abs(t - np.floor(t) - 0.5) < 2.0 ** -20


def detie_wino_weights(w, m):
    """Weights whose TRANSFORMED values U = G g are nowhere at a rounding tie of their fp16 pair: entries that are get moved by fp32 ulps.
    F(6,3)'s G has entries like 64/9 and 32/21, so U of an fp32 weight triple is an EXACT tie in real arithmetic whenever the
    triple's combination is divisible by 9, 21, ... (thousands of values per 128 x 128 layer); a double evaluation of G g then lands on either side of it depending on its operation order,
    and packer and model would legitimately differ by one whole quantum of the pair in that value.  The model must not hang on a coin
    toss, so the tests draw weights without such ties.  (Rows of G with dyadic entries only -- all of F(2,3) -- are exact in double in any
    order: nothing to do.)"""
    w = np.array(_np(w), dtype=np.float32)
    G = WINO[m]["G"]
    rows = [x for x in range(G.shape[0]) if np.any(np.abs(G[x] * 2.0 ** 20 - np.round(G[x] * 2.0 ** 20)) > 0)]
    if not rows:
        return w
    rs = np.random.RandomState(0)
    for _ in range(64):
        bad = _near_tie(np.einsum("xk,ocyk->xocy", G[rows], w.astype(np.float64))).any(axis=0)          # [o, c, ky]
        if not bad.any():
            return w
        step = rs.randint(-3, 4, w[bad].shape)          # a few fp32 ulps, each tap its own (a common step can keep a sum on its tie)
        w[bad] = (w[bad].view(np.int32) + step.astype(np.int32)).view(np.float32)
    raise AssertionError("detie_wino_weights did not converge")


def _bmm(u, v):
    """sum_c u[x,o,c] v[x,t,c,r,q] -> [x,t,o,r,q]"""
    A, T, C, R, Q = v.shape
    y = np.matmul(np.ascontiguousarray(u), np.ascontiguousarray(v.transpose(0, 2, 1, 3, 4)).reshape(A, C, T * R * Q))
    return y.reshape(A, u.shape[1], T, R, Q).transpose(0, 2, 1, 3, 4)


def _wino(sp, x, w, m, mode, halo_prev=None, halo_next=None, drop=None, flush=False):
    """the Winograd algorithm before bias, NCHW [T,cout,H,W].  mode 'split': float64 transforms, pairs(V), pairs(U), three passes (the model
    of the kernel); 'f64': float64 throughout; 'f32': float32 throughout -- fp32 BT, one fp32 chain over K per transformed position, fp32 AT."""
    assert sp.stride == 1
    f = WINO[m]
    A = m + 2
    dt = np.float32 if mode == "f32" else np.float64
    v = gather(sp, torch.as_tensor(_np(x)).double(), halo_prev, halo_next).numpy().astype(dt)
    T, cin, H, W = v.shape
    nq = (W + m - 1) // m
    dp = np.zeros((T, cin, H + 2, nq * m + 2), dtype=dt)
    dp[:, :, 1:H + 1, 1:W + 1] = v
    d = np.stack([dp[..., i:i + (nq - 1) * m + 1:m] for i in range(A)], axis=-1)          # [T,cin,H+2,nq,A]
    BT, G, AT = f["BT"].astype(dt), f["G"], f["AT"].astype(dt)
    if mode == "f32":
        V = np.zeros((A,) + d.shape[:-1], dtype=dt)
        for xi in range(A):
            for i in range(A):
                if BT[xi, i] != 0:
                    V[xi] += BT[xi, i] * d[..., i]
    else:
        V = np.einsum("xi,tcrqi->xtcrq", BT, d)
    U = np.einsum("xk,ocyk->xocy", G, np.asarray(_np(w), dtype=np.float64))               # weight transform: once, in double
    cout = U.shape[1]
    if mode == "split":
        Vh, Vl = pairs(V, flush)
        Uh, Ul = pairs(U, flush)
        M = np.zeros((A, T, cout, H, nq))
        for ky in range(3):
            vh, vl = Vh[:, :, :, ky:ky + H], Vl[:, :, :, ky:ky + H]
            if drop != "hi.hi":
                M += _bmm(Uh[..., ky], vh)
            if drop != "lo_x.hi_w":
                M += _bmm(Uh[..., ky], vl)
            if drop != "hi_x.lo_w":
                M += _bmm(Ul[..., ky], vh)
    elif mode == "f64":
        M = np.zeros((A, T, cout, H, nq))
        for ky in range(3):
            M += _bmm(U[..., ky], V[:, :, :, ky:ky + H])
    else:
        U = U.astype(dt)
        M = np.zeros((A, T, cout, H, nq), dtype=dt)
        for ky in range(3):
            for c in range(cin):
                M += U[:, None, :, c, ky, None, None] * V[:, :, c, None, ky:ky + H, :]
    if mode == "f32":
        out = np.zeros((T, cout, H, nq, m), dtype=dt)
        for j in range(m):
            for xi in range(A):
                if AT[j, xi] != 0:
                    out[..., j] += AT[j, xi] * M[xi]
    else:
        out = np.einsum("jx,xtorq->torqj", AT, M)
    return out.reshape(T, cout, H, nq * m)[..., :W]


def wino_model(sp, x, w, m, bias=None, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1, drop=None, flush=False):
    """the reference of the mode for a Winograd-form layer: x is the DECODED input (hi + lo; the kernel decodes before it transforms)"""
    return finish(sp, _wino(sp, x, w, m, "split", halo_prev, halo_next, drop, flush), bias, extra, extra_pstride, extra_cstride)


def wino_fp32(sp, x, w, m, bias=None, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1):
    """(the Winograd algorithm in float32 -- no fp16 anywhere --, the same in float64): the yardstick of the Winograd forms"""
    pre = _wino(sp, x, w, m, "f32", halo_prev, halo_next)
    if bias is not None:
        pre = pre + np.asarray(_np(bias), dtype=np.float32).reshape(1, -1, 1, 1)
    return (finish(sp, pre, None, extra, extra_pstride, extra_cstride),
            finish(sp, _wino(sp, x, w, m, "f64", halo_prev, halo_next), bias, extra, extra_pstride, extra_cstride))


def wino_err(sp, x, w, m, bias=None, **kw):
    a, b = wino_fp32(sp, x, w, m, bias, **kw)
    return float((a - b).abs().max())
