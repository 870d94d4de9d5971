"""The CPU model of the split-fp16 arithmetic (tests/split_model.py) pinned on the CPU, without the code under test:

  * its Winograd tables equal bsvd_amd/csrc/wino_forms.h entry by entry (a g++ program prints the header's),
  * its three passes stay within the format's two exact error terms of a float64 conv, through every epilogue and halo form, and
    agree with the oracle executor the GPU tests compare against,
  * the accuracy envelope of the mode over twelve octaves of weight scale (the table in DESIGN.md 4.1b): ordering and order of magnitude,
  * MUTATION CHECKS: the model with one pass dropped, with `lo` zeroed in one 16-channel chunk of one tap, with hi / lo swapped in one
    chunk, and with fp16 subnormals flushed to zero must each violate the bound the GPU tests assert (split_model.bound with the
    margins M_DIRECT / M_WINO tests/test_gpu_split_passes.py and tests/test_gpu_range.py use) at every point where those tests
    claim to be sensitive.  This is the proof that the bound catches what a flat 1.5e-4 cannot.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import split_model as S                                      # noqa: E402
from bsvd_amd.netspec import ConvSpec                        # noqa: E402
from bsvd_amd.schedule import Halo                           # noqa: E402
from oracle_exec import OracleExecutor                       # noqa: E402
M_DIRECT, M_WINO = S.M_DIRECT, S.M_WINO


def test_wino_tables_equal_the_header():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "wino_tables_dump")
        subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "bsvd_amd", "csrc"),
                        os.path.join(HERE, "native", "wino_tables_dump.cpp"), "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = set()
    for line in out.strip().splitlines():
        form, name, rows, cols, *vals = line.split()
        m = int(form[1:])
        t = np.array([float.fromhex(v) for v in vals]).reshape(int(rows), int(cols))
        mine = S.WINO[m][name]
        assert mine.shape == t.shape, (form, name)
        assert np.array_equal(mine, t), (form, name, mine - t)        # entry by entry, bit for bit
        seen.add((m, name))
    assert seen == {(m, n) for m in (2, 6) for n in ("G", "BT", "AT")}


def test_wino_model_in_float64_is_the_convolution():
    rs = np.random.RandomState(3)
    sp = ConvSpec("l", "l", 32, 16, 1, False, "none", 0)
    x, w = rs.standard_normal((2, 5, 13, 32)), rs.standard_normal((16, 32, 3, 3)) * 0.05
    ref = S._lin(sp, x, w).numpy()
    for m in (2, 6):
        got = S._wino(sp, x, w, m, "f64")
        assert np.abs(got - ref).max() < 1e-12 * np.abs(ref).max() * (100 if m == 6 else 1)


def test_pairs_and_containers():
    from test_gpu_f16x3 import from_split, to_split
    rs = np.random.RandomState(0)
    x = torch.from_numpy((rs.standard_normal((2, 3, 5, 32)) * 3).astype(np.float32))
    hi, lo = S.pairs(x)
    c = S.container(hi, lo)
    assert torch.equal(c.view(torch.int32), to_split(x).view(torch.int32))          # the ABI's canonical pair, bit for bit
    h2, l2 = S.halves(c)
    assert np.array_equal(h2, hi) and np.array_equal(l2, lo)
    assert np.array_equal(from_split(c).double().numpy(), (hi + lo).astype(np.float32).astype(np.float64))
    c8 = S.container(hi[..., :8], lo[..., :8])                                      # the fold-8 half chunk [hi x8 | lo x8]
    assert torch.equal(c8.view(torch.int32), to_split(x[..., :8].contiguous()).view(torch.int32))
    # saturating like the header says; lo is an fp16 SUBNORMAL for every |v| < 2^-3
    hi, lo = S.pairs(np.array([1e5, -7e4, 65519.0]))
    assert np.array_equal(hi, [65504.0, -65504.0, 65504.0]) and np.all(np.abs(lo) <= 65504.0)
    v = rs.uniform(-0.125, 0.125, 4096)
    hi, lo = S.pairs(v)
    assert np.all(np.abs(lo) < 2.0 ** -14) and np.all(np.abs(v - (hi + lo)) <= 2.0 ** -25)
    with pytest.raises(AssertionError):
        S.container(np.full((1, 16), 0.1), np.zeros((1, 16)))                       # 0.1 is not an fp16 value


def _state(sp, rs, wscale=1.0):
    w = (rs.standard_normal((sp.cout, sp.cin, 3, 3)) * (2.0 / (9 * sp.cin)) ** 0.5 * wscale).astype(np.float32)
    b = (rs.standard_normal(sp.cout) * 0.1 * wscale).astype(np.float32)
    return w, b


LAYERS = [
    # cin, cout, stride, tsm, act, epi, T, H, W
    (64, 64, 1, False, "relu6", 0, 1, 9, 11),
    (64, 64, 1, True, "relu", 0, 2, 6, 7),          # fold 8
    (128, 128, 1, True, "relu6", 0, 3, 5, 7),
    (64, 128, 2, False, "relu6", 0, 1, 9, 12),
    (128, 256, 1, False, "none", 1, 1, 4, 5),
    (64, 16, 1, False, "none", 2, 2, 5, 6),
]


def _case(cin, cout, stride, tsm, act, epi, T, H, W, rs):
    """canonical operands of one layer: decoded tensors for the oracle, (hi, lo) halves for the model"""
    sp = ConvSpec("l", "l", cin, cout if epi != 2 else 3, stride, tsm, act, epi)
    w, b = _state(sp, rs)
    q = lambda a: S.pairs(a.astype(np.float32))
    xh, xl = q(rs.standard_normal((T, H, W, cin)))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    kw = {}
    if epi == 1:
        eh, el = q(rs.standard_normal((T, 2 * Ho, 2 * Wo, cout // 4)))
        kw = dict(extra=eh + el, extra_pstride=cout // 4, extra_cstride=1)
    elif epi == 2:
        kw = dict(extra=rs.standard_normal((T, 4, Ho, Wo)).astype(np.float32), extra_pstride=1, extra_cstride=Ho * Wo)
    hal = [(None, None)]
    if tsm:
        f = sp.fold
        (ph, pl), (nh, nl) = q(rs.standard_normal((H, W, f))), q(rs.standard_normal((H, W, f)))
        hal.append(((Halo(ph, f, 0), Halo(pl, f, 0)), (Halo(nh, f, 0), Halo(nl, f, 0))))
        fh, fl = q(rs.standard_normal((1, H, W, cin)))
        hal.append(((Halo(fh, cin, f), Halo(fl, cin, f)), (Halo(fh, cin, 0), Halo(fl, cin, 0))))
    return sp, w, b, xh, xl, kw, hal


@pytest.mark.parametrize("cin,cout,stride,tsm,act,epi,T,H,W", LAYERS)
def test_three_passes_within_the_format_terms_of_float64(cin, cout, stride, tsm, act, epi, T, H, W):
    rs = np.random.RandomState(cin + cout + H)
    sp, w, b, xh, xl, kw, hal = _case(cin, cout, stride, tsm, act, epi, T, H, W, rs)
    oex = OracleExecutor({"l.weight": w, "l.bias": b}, double=True)
    for hp, hn in hal:
        pre, ref = S.direct_pre(sp, xh, xl, w, hp, hn), S._lin(sp, xh + xl, w, S._sum_halo(hp), S._sum_halo(hn))
        quant, lolo = S.format_terms(sp, xh, xl, w, hp, hn)
        assert bool(((pre - ref).abs() <= (quant + lolo) * (1 + 1e-9) + 1e-300).all())
        assert float((pre - ref).abs().max()) > 0.0                     # ... and the terms are not vacuous
        # every epilogue is 1-Lipschitz in the conv result: the same bound holds for the finished layer
        y = S.direct_three_pass(sp, xh, xl, w, b, hp, hn, **kw)
        y64 = S.conv_f64(sp, xh + xl, w, b, S._sum_halo(hp), S._sum_halo(hn), **kw)
        assert float((y - y64).abs().max()) <= float((quant + lolo).max()) * (1 + 1e-9)
        # the float64 side of the model is the oracle executor the GPU tests use (which returns float32)
        tt = lambda h: None if h is None else Halo(torch.as_tensor(h.t).float(), h.pstride, h.coff)
        extra = None if "extra" not in kw else torch.as_tensor(kw["extra"]).float()
        want = oex.conv(sp, torch.as_tensor(xh + xl).float(), tt(S._sum_halo(hp)), tt(S._sum_halo(hn)), extra,
                        kw.get("extra_pstride", 0), kw.get("extra_cstride", 1))
        assert float((want.double() - y64).abs().max()) <= 2.0 ** -23 * max(1.0, float(y64.abs().max()))
        # the yardstick is an honest float32 chain: a few ulp of the accumulated magnitude, never zero
        e = S.chain_err(sp, xh + xl, w, b, halo_prev=S._sum_halo(hp), halo_next=S._sum_halo(hn), **kw)
        assert 0.0 < e < 2.0 ** -24 * (9 * cin) ** 0.5 * 8 * max(1.0, float(y64.abs().max()))


TABLE = {0: (6.7e-7, 6.3e-7), -4: (1.4e-5, 9.0e-6), -8: (1.4e-4, 1.3e-4), -12: (2.3e-3, 2.1e-3)}      # predicted rel. error: K = 576, 2304


def _envelope(cin, s, rs, drop=None):
    sp = ConvSpec("l", "l", cin, 32, 1, False, "none", 0)
    xh, xl = S.pairs(rs.standard_normal((1, 8, 8, cin)).astype(np.float32))          # 2048 outputs
    w = (rs.standard_normal((32, cin, 3, 3)) * 0.03 * 2.0 ** s).astype(np.float32)
    ref = S._lin(sp, xh + xl, w)
    return float((S.direct_pre(sp, xh, xl, w, drop=drop) - ref).abs().max()) / float(ref.abs().max())


def test_accuracy_envelope_over_twelve_octaves_of_weight_scale():
    """fp32-class at the Kaiming scale, fp16-class twelve octaves below: `lo` is an fp16 subnormal (fixed quantum 2^-24) for |v| < 2^-3."""
    print("\nweight scale s | K = 576: max err / max|y| | K = 2304 | dropping the lo_x.hi_w pass instead")
    rel = {}
    for s in (0, -4, -8, -12):
        r = [_envelope(cin, s, np.random.RandomState(100 + cin - s)) for cin in (64, 256)]
        d = [_envelope(cin, s, np.random.RandomState(100 + cin - s), drop="lo_x.hi_w") for cin in (64, 256)]
        rel[s] = (r, [a / b for a, b in zip(d, r)])
        print("%4d | %.1e | %.1e | %.1fx / %.1fx worse" % (s, r[0], r[1], rel[s][1][0], rel[s][1][1]))
        for got, want in zip(r, TABLE[s]):
            assert want / 4 < got < want * 4, (s, got, want)
    for a, b in ((0, -4), (-4, -8), (-8, -12)):
        assert all(x * 4 < y for x, y in zip(rel[a][0], rel[b][0]))                   # decays steadily, octave by octave
    assert min(rel[0][1]) > 100 and 5 < min(rel[-4][1]) and max(rel[-4][1]) < 60
    assert 1.1 < min(rel[-8][1]) and max(rel[-8][1]) < 4 and max(rel[-12][1]) < 1.2   # at 2^-12 the mode IS plain fp16


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutation checks


def _swap_chunk(hi, lo, c0, axis):
    hi, lo = hi.copy(), lo.copy()
    sl = [slice(None)] * hi.ndim
    sl[axis] = slice(c0, c0 + 16)
    sl = tuple(sl)
    hi[sl], lo[sl] = lo[sl].copy(), hi[sl].copy()
    return hi, lo


def _probe_inputs(kind, cin, rs, shape):
    """the activation-side probes of tests/test_gpu_split_passes.py (fp16-valued halves)"""
    v = S.fp16(rs.standard_normal(shape))
    if kind == "canonical":
        return S.pairs(rs.standard_normal(shape).astype(np.float32))
    if kind == "hi_only":
        return v, np.zeros_like(v)
    if kind == "lo_only":
        return np.zeros_like(v), v
    return v, S.fp16(rs.standard_normal(shape))                                       # independent halves of the same magnitude


def _probe_weights(kind, shape, rs, scale):
    return S.lo_plane_weights(shape, rs) if kind == "lo_plane" else (rs.standard_normal(shape) * scale).astype(np.float32)


@pytest.mark.parametrize("cin", [64, 256])
def test_mutations_of_the_direct_form_violate_the_gpu_bound(cin):
    rs = np.random.RandomState(cin)
    sp = ConvSpec("l", "l", cin, 32, 1, False, "none", 0)
    shape = (1, 6, 7, cin)
    scale = (2.0 / (9 * cin)) ** 0.5
    ratios = {}

    def check(name, xk, wk, mutate, sensitive=True):
        xh, xl = _probe_inputs(xk, cin, rs, shape)
        w = _probe_weights(wk, (32, cin, 3, 3), rs, scale)
        model = S.direct_three_pass(sp, xh, xl, w)
        err = S.chain_err(sp, xh + xl, w)
        got = mutate(xh, xl, w)
        ex = S.excess(got, model, err, M_DIRECT)
        ratios[(name, xk, wk)] = ex
        if sensitive:
            assert ex > 1.0, (name, xk, wk, ex)
        return ex

    wl0 = lambda w, tap, c0: (lambda h, l: (h, np.where(_mask(l.shape, tap, c0), 0.0, l)))(*S.pairs(w))
    for c0 in (0, cin - 16):
        for tap in ((0, 0), (1, 2), (2, 1)):
            # weight lo plane zeroed / swapped in one chunk of one tap: seen by every probe whose hi half carries data
            for xk in ("canonical", "hi_only", "independent"):
                for wk in ("kaiming", "lo_plane"):
                    check("w_lo chunk zeroed", xk, wk, lambda xh, xl, w: S.direct_three_pass(sp, xh, xl, w, w_pairs=wl0(w, tap, c0)))
            check("w chunk hi<->lo", "canonical", "kaiming",
                  lambda xh, xl, w: S.direct_three_pass(sp, xh, xl, w, w_pairs=_swap_w(S.pairs(w), tap, c0)))
        # activation lo zeroed / halves swapped in one chunk (every tap reads it)
        for xk in ("canonical", "lo_only", "independent"):
            check("x_lo chunk zeroed", xk, "kaiming",
                  lambda xh, xl, w: S.direct_three_pass(sp, xh, np.where(_cmask(xl.shape, c0), 0.0, xl), w))
            check("x chunk hi<->lo", xk, "kaiming", lambda xh, xl, w: S.direct_three_pass(sp, *_swap_chunk(xh, xl, c0, 3), w))
    for drop in ("lo_x.hi_w", "hi_x.lo_w", "hi.hi"):
        for xk in ("canonical", "independent"):
            check("dropped " + drop, xk, "kaiming", lambda xh, xl, w: S.direct_three_pass(sp, xh, xl, w, drop=drop))
    check("dropped lo_x.hi_w", "lo_only", "kaiming", lambda xh, xl, w: S.direct_three_pass(sp, xh, xl, w, drop="lo_x.hi_w"))
    check("dropped hi_x.lo_w", "hi_only", "lo_plane", lambda xh, xl, w: S.direct_three_pass(sp, xh, xl, w, drop="hi_x.lo_w"))
    # a lo.lo pass the kernel must not have: visible on the independent halves only
    check("added lo.lo", "independent", "kaiming",
          lambda xh, xl, w: S.direct_three_pass(sp, xh, xl, w) + S.finish(sp, S._lin(sp, xl, S.pairs(w)[1])))
    print("\nK = %d, margin %d: smallest excess over the bound of any mutation = %.1f (%s)"
          % (9 * cin, M_DIRECT, min(ratios.values()), min(ratios, key=ratios.get)))
    # the same fault on ordinary data, in absolute terms: the class of the flat 1.5e-4 the layer tests used to rely on alone
    xh, xl = _probe_inputs("canonical", cin, rs, shape)
    w = _probe_weights("kaiming", (32, cin, 3, 3), rs, scale)
    old = float((S.direct_three_pass(sp, xh, xl, w, w_pairs=wl0(w, (1, 1), 0)) - S.direct_three_pass(sp, xh, xl, w)).abs().max())
    print("w_lo chunk zeroed, canonical data: max-abs %.1e (flat layer tolerance 1.5e-4)" % old)
    assert old < 4 * 1.5e-4


def _mask(shape, tap, c0):
    m = np.zeros(shape, dtype=bool)
    m[:, c0:c0 + 16, tap[0], tap[1]] = True
    return m


def _cmask(shape, c0):
    m = np.zeros(shape, dtype=bool)
    m[..., c0:c0 + 16] = True
    return m


def _swap_w(wp, tap, c0):
    h, l = wp[0].copy(), wp[1].copy()
    m = _mask(h.shape, tap, c0)
    h[m], l[m] = wp[1][m], wp[0][m]
    return h, l


SWEEP_S, SWEEP_T = (0, -4, -8, -12), (0, -6, -12)


@pytest.mark.parametrize("cin", [64, 256])
def test_sweep_mutations_violate_the_gpu_bound_where_the_sweep_is_sensitive(cin):
    """tests/test_gpu_range.py's low-range sweep claims: a dropped `lo` pass is seen at weight scales 2^0 and 2^-4 (below, the format itself
    has lost the bits the pass carries: the envelope table), flushed fp16 subnormals at EVERY point, the all-subnormal point included."""
    sp = ConvSpec("l", "l", cin, 32, 1, False, "relu", 0)
    for s in SWEEP_S:
        for t in SWEEP_T:
            rs = np.random.RandomState(cin - 7 * s - t)
            w = (rs.standard_normal((32, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5 * 2.0 ** s).astype(np.float32)
            b = (rs.standard_normal(32) * 0.1 * 2.0 ** (s + t)).astype(np.float32)
            xh, xl = S.pairs((rs.standard_normal((1, 6, 7, cin)) * 2.0 ** t).astype(np.float32))
            model = S.direct_three_pass(sp, xh, xl, w, b)
            err = S.chain_err(sp, xh + xl, w, b)
            for drop in ("lo_x.hi_w", "hi_x.lo_w"):
                ex = S.excess(S.direct_three_pass(sp, xh, xl, w, b, drop=drop), model, err, M_DIRECT)
                if s >= -4 and t > -12:
                    assert ex > 1.0, (s, t, drop, ex)
            fxh, fxl = S.pairs((xh + xl), flush_subnormals=True)
            ex = S.excess(S.direct_three_pass(sp, fxh, fxl, w, b, w_pairs=S.pairs(w, flush_subnormals=True)), model, err, M_DIRECT)
            assert ex > 1.0, (s, t, "flush", ex)
    xh, xl, w = _all_subnormal(cin, np.random.RandomState(5))
    model = S.direct_three_pass(sp, xh, xl, w)
    assert float(model.abs().max()) > 2.0 ** -21
    flushed = S.direct_three_pass(sp, *S.pairs(xh + xl, True), w, w_pairs=S.pairs(w, True))
    assert float(flushed.abs().max()) == 0.0
    assert S.excess(flushed, model, S.chain_err(sp, xh + xl, w), M_DIRECT) > 1.0


def _all_subnormal(cin, rs):
    """|x| < 2^-14 and |w| < 2^-14: every fp16 operand half is subnormal; positive operands, so the result is far from zero"""
    x = (rs.uniform(0.25, 0.99, (1, 6, 7, cin)) * 2.0 ** -14).astype(np.float32)
    w = (rs.uniform(0.25, 0.99, (32, cin, 3, 3)) * 2.0 ** -14).astype(np.float32)
    xh, xl = S.pairs(x)
    assert np.all(np.abs(xh) < 2.0 ** -14) and np.all(np.abs(S.pairs(w)[0]) < 2.0 ** -14)
    return xh, xl, w


@pytest.mark.parametrize("m", [2, 6])
def test_mutations_of_the_winograd_forms_violate_the_gpu_bound(m):
    rs = np.random.RandomState(m)
    cin = 128
    sp = ConvSpec("l", "l", cin, 32, 1, False, "none", 0)
    x = S.fp16(rs.standard_normal((1, 5, 14, cin)))
    w = (rs.standard_normal((32, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32)
    model = S.wino_model(sp, x, w, m)
    err = S.wino_err(sp, x, w, m)
    # the model is the convolution to within the format (F(6,3) amplifies: its own envelope)
    rel = float((model - S.conv_f64(sp, x, w)).abs().max()) / float(model.abs().max())
    print("\nF(%d,3): model vs float64 conv %.2e relative, float32 Winograd's own error %.2e" % (m, rel, err / float(model.abs().max())))
    assert rel < (2e-5 if m == 6 else 4e-6)
    for drop in ("lo_x.hi_w", "hi_x.lo_w", "hi.hi"):
        assert S.excess(S.wino_model(sp, x, w, m, drop=drop), model, err, M_WINO[m]) > 1.0, drop
    assert S.excess(S.wino_model(sp, x, w, m, flush=True), model, err, M_WINO[m]) > 1.0
    # a reader that takes one chunk's lo half from the wrong place: that chunk decodes to hi alone
    xh, xl = S.pairs(rs.standard_normal((1, 5, 14, cin)).astype(np.float32))
    model = S.wino_model(sp, xh + xl, w, m)
    err = S.wino_err(sp, xh + xl, w, m)
    bad = xh + np.where(_cmask(xl.shape, 32), 0.0, xl)
    assert S.excess(S.wino_model(sp, bad, w, m), model, err, M_WINO[m]) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# channel widths off the 16 / 32 / 64 / 128 / 256 / 512 grid (the cases of tests/test_gpu_widths.py)

WIDTH_LAYERS = [
    # cin, cout, stride, tsm, act, epi, T, H, W: 3, 5, 9 and 24 chunks; Cout % 32 == 16; Cout / 4 = 48 and 80
    (48, 48, 1, False, "relu6", 0, 1, 5, 6),
    (80, 64, 2, False, "relu6", 0, 2, 6, 7),
    (144, 160, 1, False, "none", 0, 1, 4, 5),
    (128, 192, 1, False, "none", 1, 1, 3, 4),
    (64, 320, 1, False, "none", 1, 1, 3, 4),
    (384, 384, 1, True, "relu6", 0, 2, 3, 4),      # fold 48
]


@pytest.mark.parametrize("cin,cout,stride,tsm,act,epi,T,H,W", WIDTH_LAYERS)
def test_three_passes_within_the_format_terms_at_odd_chunk_widths(cin, cout, stride, tsm, act, epi, T, H, W):
    test_three_passes_within_the_format_terms_of_float64(cin, cout, stride, tsm, act, epi, T, H, W)


def _pad(a, c):
    return np.concatenate([a, np.zeros(a.shape[:-1] + (c - a.shape[-1],), dtype=a.dtype)], axis=-1)


def test_models_at_padded_widths():
    """40 -> 70 real channels on 48 -> 80 padded ones (and a PixelShuffle layer with 70 real channels per sub-pixel on 80): the models read the
    real input channels only, return the PADDED width with exact zeros in the padding channels, and agree with the oracle executor."""
    rs = np.random.RandomState(4070)
    for sp, T, H, W in ((ConvSpec("l", "l", 40, 70, 1, False, "relu", 0), 1, 7, 9), (ConvSpec("l", "l", 64, 280, 1, False, "none", 1), 1, 3, 4)):
        w, b = _state(sp, rs)
        x = _pad(rs.standard_normal((T, H, W, sp.cin)).astype(np.float32), sp.cin_pad)
        xh, xl = S.pairs(x)
        kw = {}
        if sp.epilogue == 1:
            e = sum(S.pairs(_pad(rs.standard_normal((T, 2 * H, 2 * W, sp.out_channels)).astype(np.float32), sp.out_channels_pad)))
            kw = dict(extra=e, extra_pstride=sp.out_channels_pad, extra_cstride=1)
        y = S.direct_three_pass(sp, xh, xl, w, b, **kw)
        assert y.shape[-1] == sp.out_channels_pad > sp.out_channels and not bool(y[..., sp.out_channels:].any())
        garbage = xh.copy()
        garbage[..., sp.cin:] = 7.0                      # the model never reads a padding channel of x
        assert torch.equal(S.direct_three_pass(sp, garbage, xl, w, b, **kw), y)
        extra = None if not kw else torch.as_tensor(kw["extra"]).float()
        want = OracleExecutor({"l.weight": w, "l.bias": b}, double=True).conv(sp, torch.as_tensor(xh + xl).float(), None, None, extra,
                                                                              kw.get("extra_pstride", 0), 1)
        quant, lolo = S.format_terms(sp, xh, xl, w)
        assert want.shape == y.shape
        assert float((want.double() - y).abs().max()) <= float((quant + lolo).max()) * (1 + 1e-9) + 2.0 ** -23 * max(1.0, float(y.abs().max()))
        e = S.chain_err(sp, xh + xl, w, b, **kw)
        assert 0.0 < e < 2.0 ** -24 * (9 * sp.cin) ** 0.5 * 8 * max(1.0, float(y.abs().max()))
        if sp.epilogue == 0:
            for m in (2, 6):
                yw = S.wino_model(sp, xh + xl, w, m, b)
                assert yw.shape == y.shape and not bool(yw[..., sp.cout:].any())
                assert float((yw - y).abs().max()) < (2e-5 if m == 6 else 4e-6) * float(y.abs().max())
                assert 0.0 < S.wino_err(sp, xh + xl, w, m, b)


# Three faults a kernel can have at these widths only, applied to the model.  Each is the identity wherever its condition does not hold (an even
# chunk count, Cout % 32 == 0, a temporal source that exists), so the unmutated cases pass untouched; where it holds, it must violate
# needed <= M_DIRECT (M_WINO) on the case of tests/test_gpu_widths.py named here -- at that case's own shape.

def _drop_last_chunk_if_odd(sp, xh, xl):
    """the K loop's chunk-parity double buffer never consumes the last chunk of an odd count"""
    if (sp.cin_pad // 16) % 2 == 0:
        return xh, xl
    m = _cmask(xh.shape, sp.cin_pad - 16)
    return np.where(m, 0.0, xh), np.where(m, 0.0, xl)


def _half_granule_reads_the_row_below(sp, w):
    """Cout % 32 == 16: the live half of the last 32-channel granule is fed the weights one 16-channel row further down the pack"""
    if sp.cout_pad % 32 != 16 or sp.cout_pad < 32:
        return w
    w = np.array(w)
    lo, hi = sp.cout_pad - 16, min(sp.cout, sp.cout_pad)
    w[lo:hi] = w[lo - 16:hi - 16]
    return w


def _zero_skip_shifted_by_one_chunk(sp, xh, xl, T):
    """the zero-chunk skip of a frame without a `next` (`prev`) source leaves out chunks [1, 1 + fold/16) ([fold/16 + 1, 2 fold/16 + 1)) instead of
    the group itself: the first chunk behind the absent group is lost.  Returns the plain layer and the GATHERED halves it reads."""
    plain = ConvSpec(sp.name, sp.key, sp.cin, sp.cout, sp.stride, False, sp.act, sp.epilogue)
    out = []
    for half in (xh, xl):
        g = S.gather(sp, half).permute(0, 2, 3, 1).contiguous().numpy().copy()          # NHWC, temporal shift applied, no halos
        g[T - 1, ..., sp.fold:sp.fold + 16] = 0.0
        g[0, ..., 2 * sp.fold:2 * sp.fold + 16] = 0.0
        out.append(g)
    return plain, out[0], out[1]


def test_width_mutations_violate_the_gpu_bound():
    rs = np.random.RandomState(48)
    need = {}

    def operands(cin, cout, stride, tsm, act, epi, T, H, W):
        sp = ConvSpec("l", "l", cin, cout, stride, tsm, act, epi)
        w, b = _state(sp, rs)
        xh, xl = S.pairs(_pad(rs.standard_normal((T, H, W, cin)).astype(np.float32), sp.cin_pad))
        return sp, w, b, xh, xl

    # -- the last chunk of an odd count: (48,48) narrow tile, 3 chunks; (80,80) 5 chunks; F(2,3) / F(6,3) at (144,160), 9 chunks
    for case in ((48, 48, 1, False, "relu6", 0, 2, 21, 37), (80, 80, 1, False, "relu6", 0, 2, 20, 24)):
        sp, w, b, xh, xl = operands(*case)
        model, err = S.direct_three_pass(sp, xh, xl, w, b), S.chain_err(sp, xh + xl, w, b)
        need["odd chunk", case] = S.needed(S.direct_three_pass(sp, *_drop_last_chunk_if_odd(sp, xh, xl), w, b), model, err)
        assert need["odd chunk", case] > M_DIRECT
    sp, w, b, xh, xl = operands(144, 160, 1, False, "none", 0, 1, 17, 33)
    for m in (2, 6):
        model, err = S.wino_model(sp, xh + xl, w, m, b), S.wino_err(sp, xh + xl, w, m, b)
        need["odd chunk", "F(%d,3)" % m] = S.needed(S.wino_model(sp, sum(_drop_last_chunk_if_odd(sp, xh, xl)), w, m, b), model, err)
        assert need["odd chunk", "F(%d,3)" % m] > M_WINO[m]
    sp, w, b, xh, xl = operands(96, 96, 1, False, "none", 0, 2, 17, 21)                   # 6 chunks: the identity
    assert _drop_last_chunk_if_odd(sp, xh, xl)[0] is xh
    # -- the half-live granule: (48,48), (80,80) and the padded (40 -> 70)
    for case in ((48, 48, 1, False, "relu6", 0, 2, 21, 37), (80, 80, 1, False, "relu6", 0, 2, 20, 24), (40, 70, 1, False, "relu", 0, 1, 33, 37)):
        sp, w, b, xh, xl = operands(*case)
        model, err = S.direct_three_pass(sp, xh, xl, w, b), S.chain_err(sp, xh + xl, w, b)
        need["half granule", case] = S.needed(S.direct_three_pass(sp, xh, xl, _half_granule_reads_the_row_below(sp, w), b), model, err)
        assert need["half granule", case] > M_DIRECT
    sp, w, b, xh, xl = operands(64, 96, 1, False, "relu6", 0, 1, 21, 37)                  # 96 = 3 x 32: the identity
    assert _half_granule_reads_the_row_below(sp, w) is w
    # -- the zero-chunk skip of fold 48: (384,384) with three frames and no halos (both end frames skip a group)
    case = (384, 384, 1, True, "relu6", 0, 3, 10, 19)
    sp, w, b, xh, xl = operands(*case)
    model, err = S.direct_three_pass(sp, xh, xl, w, b), S.chain_err(sp, xh + xl, w, b)
    plain, gh, gl = _zero_skip_shifted_by_one_chunk(sp, xh, xl, 3)
    need["skip map", case] = S.needed(S.direct_three_pass(plain, gh, gl, w, b), model, err)
    assert need["skip map", case] > M_DIRECT
    # (the unshifted map IS the layer: gathering first and convolving plainly is the model itself)
    g = [S.gather(sp, h).permute(0, 2, 3, 1).contiguous().numpy() for h in (xh, xl)]
    assert torch.equal(S.direct_three_pass(plain, g[0], g[1], w, b), model)
    print("\nmargins the width mutants need (M_DIRECT %d, M_WINO %s):" % (M_DIRECT, M_WINO))
    for k, v in need.items():
        print("    %-14s %-50s %.1f" % (k[0], k[1], v))
