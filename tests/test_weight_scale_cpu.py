"""Per-layer power-of-two weight scale of the split mode (BsvdConvArgs.out_scale, ABI v12; engine.weight_scale_exponent),
the parts that need no GPU: the exponent, the ABI's struct and its refusals (-23, answered before any device call like the refusals of
tests/test_abi.py), the constructor keyword, and -- on the CPU model of the mode alone (tests/split_model.py) -- why the scale helps: the
three passes of 2^e w, times 2^-e, sit closer to float64 than the three passes of w once w is small."""
import ctypes
import math
import os

import numpy as np
import pytest

import split_model as S


def test_weight_scale_exponent():
    from bsvd_amd.engine import weight_scale_exponent as wse
    assert wse(0.0) == 0 and wse(-0.0) == 0
    for k in (-140, -126, -30, -12, -3, -1, 0, 1, 5, 20, 100, 127):
        p = math.ldexp(1.0, k)
        e = wse(p)
        if -126 <= -(k + 1) <= 126:
            assert e == -(k + 1) and math.ldexp(p, e) == 0.5, (k, e)          # a power of two lands on 0.5, the bottom of [0.5, 1)
        for v in (math.nextafter(p, 0.0), math.nextafter(p, math.inf), float(np.nextafter(np.float32(p), np.float32(0))),
                  float(np.nextafter(np.float32(p), np.float32(np.inf)))):
            e = wse(v)
            assert -126 <= e <= 126
            if abs(e) < 126 and v > 0.0:
                assert 0.5 <= math.ldexp(v, e) < 1.0, (v, e)
        assert wse(math.nextafter(p, 0.0)) == max(-126, min(126, -k))         # just under 2^k: one binade down
    assert wse(1e-30) == 99 and 0.5 <= 1e-30 * 2.0 ** 99 < 1.0
    assert wse(1e30) == -100 and 0.5 <= 1e30 * 2.0 ** -100 < 1.0
    assert wse(-0.3) == wse(0.3) == 1                                         # the magnitude counts
    # clamped: 2^-e (the epilogue's factor) and 2^e (the pack's) stay NORMAL fp32 numbers
    assert wse(1e-45) == 126 and wse(3e38) == -126
    for e in (wse(1e-45), wse(3e38), wse(1e-30), wse(1e30)):
        for f in (math.ldexp(1.0, e), math.ldexp(1.0, -e)):
            assert float(np.float32(f)) == f and f >= 2.0 ** -126
    assert wse(float("inf")) == 0 and wse(float("nan")) == 0                  # left to the range guards, which refuse them


def test_abi_version_12_and_struct_size():
    from bsvd_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 12 and lib.bsvd_abi_version() == 12
    A = _lib.BsvdConvArgs
    names = [f[0] for f in A._fields_]
    assert names[-5:] == ["x_v", "y_v", "out_scale", "head_out_scale", "pre_out_scale"]          # appended, in the header's order
    off = A.y_v.offset + 4
    for n in names[-3:]:
        assert getattr(A, n).offset == off and getattr(A, n).size == 4
        off += 4
    assert ctypes.sizeof(A) == (off + 7) // 8 * 8 == lib.bsvd_conv_args_size()
    a = A()
    assert a.out_scale == 0.0 and a.head_out_scale == 0.0 and a.pre_out_scale == 0.0             # a zeroed struct = no scale
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bsvd_hip.h")).read()
    assert "#define BSVD_ABI_VERSION 12" in hdr and "float out_scale, head_out_scale, pre_out_scale;" in hdr


def _args(**kw):
    from bsvd_amd import _lib
    a = _lib.BsvdConvArgs()
    a.x = a.y = a.w_packed = 256
    a.frames, a.H, a.W, a.Cin, a.Cout, a.stride, a.dtype = 1, 8, 8, 64, 64, 1, _lib.BSVD_F16X3
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD_SCALES = [3.0, -1.0, float("inf"), float("-inf"), float("nan"), 1e-40, -0.5, 0.75, 2.0 ** -3 * (1 + 2.0 ** -23)]


@pytest.mark.parametrize("field", ["out_scale", "head_out_scale", "pre_out_scale"])
@pytest.mark.parametrize("v", BAD_SCALES)
def test_a_scale_that_is_no_normal_positive_power_of_two_is_refused(field, v):
    """-23 from bsvd_conv3x3, the batch entry and the dry run alike; pointers are fakes: nothing may reach the device"""
    from bsvd_amd import _lib
    lib = _lib.load()
    a = _args(**{field: v})
    assert lib.bsvd_conv3x3(ctypes.byref(a), None) == -23
    assert field.encode() in lib.bsvd_last_error() and b"power of two" in lib.bsvd_last_error()
    assert lib.bsvd_conv3x3_batch(ctypes.byref(a), 1, None) == -23 and b"layer 0 of 1" in lib.bsvd_last_error()
    buf = ctypes.create_string_buffer(96)
    assert lib.bsvd_conv3x3_variant(ctypes.byref(a), buf, 96) == -23
    assert lib.bsvd_workspace_bytes(ctypes.byref(a)) == -23


def test_a_scale_needs_the_split_mode_and_its_pack():
    from bsvd_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(96)

    def rc(**kw):
        a = _args(**kw)
        r = lib.bsvd_conv3x3_variant(ctypes.byref(a), buf, 96)          # validates like bsvd_conv3x3, launches nothing
        if r < 0:
            assert lib.bsvd_conv3x3(ctypes.byref(a), None) == r
        return r, buf.value.decode(), lib.bsvd_last_error()

    plain = rc()
    assert plain[0] == 0 and "[f16x3]" in plain[1]
    # a valid scale changes nothing about the dispatch; 1.0 and 0 are the same request, in either mode
    for v in (2.0 ** -3, 2.0 ** 12, 2.0 ** -126, 2.0 ** 126, 1.0, 0.0):
        assert rc(out_scale=v)[:2] == plain[:2], v
    assert rc(dtype=_lib.BSVD_F32, out_scale=1.0)[0] == 0 and rc(dtype=_lib.BSVD_F32)[0] == 0
    r = rc(dtype=_lib.BSVD_F32, out_scale=2.0 ** -3)
    assert r[0] == -23 and b"BSVD_F16X3" in r[2]
    for f in ("head_out_scale", "pre_out_scale"):
        r = rc(**{f: 0.5})
        assert r[0] == -23 and b"without the pack" in r[2] and f.encode() in r[2]
        assert rc(**{f: 1.0})[0] == 0                                     # 1.0 asks for nothing
        assert rc(dtype=_lib.BSVD_F32, **{f: 0.5})[0] == -23
    # with its pack a first-conv scale passes this check (the fused pair: pre_cin -> Cin -> Cout, all of it dry)
    assert rc(pre_w_packed=256, pre_bias=256, pre_cin=64, pre_out_scale=4.0, out_scale=0.25)[0] == 0
    assert rc(x_planar_ch=4, head_w_packed=256, head_bias=256, head_out_scale=0.5, out_scale=2.0)[0] == 0
    # the unfused planar entry (head_kernel on an fp32 pack, split-stored output) has no scale to undo: refused, never silently ignored
    head = dict(x_planar_ch=4, Cin=16)
    r = rc(**head)
    assert r[0] == 0 and r[1].startswith("head_kernel<4>") and rc(out_scale=1.0, **head)[:2] == r[:2]
    r = rc(out_scale=0.5, **head)
    assert r[0] == -23 and b"unfused planar entry" in r[2]
    # the Winograd kernel takes the scale; the all-positions-per-wave measurement kernel (wino_m 12, 14) never learned it
    wino = dict(w_wino_packed=256, H=135, W=240, Cin=256, Cout=256)
    assert rc(wino_m=2, **wino)[0] == 0 and rc(wino_m=2, out_scale=2.0 ** 7, **wino)[:2] == rc(wino_m=2, **wino)[:2]
    assert rc(wino_m=46, out_scale=2.0 ** -7, **wino)[0] == 0
    for m in (12, 14):
        r = rc(wino_m=m, out_scale=0.5, **wino)
        assert r[0] == -23 and b"wino_m" in r[2]
        assert rc(wino_m=m, **wino)[0] == -19                             # without a scale: the product library's old answer


def test_constructor_keyword():
    import bsvd_amd
    from bsvd_amd import arch
    assert arch.WEIGHT_SCALE_DEFAULT == "off"
    kw = dict(chns=[64, 128, 256], mid_ch=64, norm="none", act="relu", interm_ch=30, blind=True, pretrain_ckpt=None)
    m = bsvd_amd.BSVD(**kw)
    assert m.weight_scale == "off" and "weight_scale=off" in m.extra_repr()
    m = bsvd_amd.BSVD(weight_scale="auto", **kw)
    assert m.weight_scale == "auto" and "weight_scale=auto" in m.extra_repr() and m.precision == "f16x3"
    m = bsvd_amd.BSVD(weight_scale="auto", precision="fp32", **kw)          # accepted in the exact mode, where it does nothing
    assert m.weight_scale == "auto" and m.precision == "fp32"
    for bad in (True, "on", None, 1):
        with pytest.raises(ValueError, match="weight_scale"):
            bsvd_amd.BSVD(weight_scale=bad, **kw)
        with pytest.raises(ValueError, match="weight_scale"):               # a later assignment is validated like the keyword
            m.weight_scale = bad
        assert m.weight_scale == "auto"
    m.weight_scale = "off"
    assert m.weight_scale == "off" and "weight_scale=off" in m.extra_repr()
    t = bsvd_amd.TSN(net2d_opt=dict(chns=[64, 128, 256], mid_ch=64, norm="none", act="relu", interm_ch=30, blind=True), weight_scale="auto")
    assert t.weight_scale == "auto" and bsvd_amd.TSN().weight_scale == "off"


def test_model_scaled_pairs_beat_unscaled_pairs_at_small_weights():
    """split_model alone, one K = 576 layer (64 channels x 9 taps), same operands: the three passes of 2^e w times 2^-e against the three
    passes of w, both against float64.  At s = 0 (Kaiming scale) the scale moves the weights less than five octaves and buys little; at
    s = -12 the unscaled pairs are down to a handful of bits (quantum 2^-24 against weights of 2^-16) and the scaled ones are where they
    were at s = 0.  Printed: the rows of DESIGN.md 4.1b's table."""
    from bsvd_amd.engine import weight_scale_exponent
    from bsvd_amd.netspec import ConvSpec
    sp = ConvSpec("l", "l", 64, 64, 1, False, "none", 0)
    rs = np.random.RandomState(5)
    w0 = (rs.standard_normal((64, 64, 3, 3)) * (2.0 / 576) ** 0.5).astype(np.float32)
    b0 = (rs.standard_normal(64) * 0.1).astype(np.float32)
    xh, xl = S.pairs(rs.standard_normal((1, 6, 7, 64)).astype(np.float32))
    env = {}
    for s in (0, -4, -8, -12):
        w, b = (w0 * np.float32(2.0 ** s)).astype(np.float32), (b0 * np.float32(2.0 ** s)).astype(np.float32)
        e = weight_scale_exponent(float(np.abs(w).max()))
        ws = np.ldexp(w, e)
        assert ws.dtype == np.float32 and 0.5 <= float(np.abs(ws).max()) < 1.0 and np.array_equal(np.ldexp(ws.astype(np.float64), -e), w.astype(np.float64))
        ref = S.conv_f64(sp, xh + xl, w, b)
        ymax = float(ref.abs().max())
        plain = S.direct_three_pass(sp, xh, xl, w, b)
        scaled = S.finish(sp, S.direct_pre(sp, xh, xl, ws) * 2.0 ** -e, b)
        env[s] = (float((plain - ref).abs().max()) / ymax, float((scaled - ref).abs().max()) / ymax)
        print("WSCALE-MODEL | K = 576 | s = %3d | e = %2d | unscaled pairs vs float64 %.2e | scaled pairs vs float64 %.2e" % ((s, e) + env[s]))
    assert env[-12][1] < env[-12][0]
    # a power-of-two scale commutes with every rounding of the pair format while nothing leaves the normal range: the scaled model is the
    # SAME relative error at every s -- which is the whole point
    for s in (-4, -8, -12):
        assert abs(env[s][1] - env[0][1]) <= 1e-3 * env[0][1], (s, env[s], env[0])
    # twelve octaves of weight scale against a fixed quantum: the unscaled pairs lose a factor 2^12 where the scale gains at most the 2^5
    # between the Kaiming scale and [0.5, 1) -- two orders of magnitude apart with room to spare
    assert env[-12][0] > 100 * env[-12][1]
