"""Stale state on the MI355X (tests/stale.py): results that depend on something the launch did not write itself.

A. LDS.  Every kernel that stages operands through LDS -- the direct-form tiles in exact fp32, f16x3 and f16, the head and tail kernels, the fused
   entry, the fused pair, the F(2,3) and F(6,3) Winograd kernels, the two kernels of frame_sigma -- is launched clean, right behind a poison of
   the whole LDS of every CU with 0xFFFFFFFF, and right behind one with 0x3C003C00, on the same stream with nothing in between.  Asserted: the
   three results have the same bits, hold no NaN, and the clean one is within the family's own bound of its own reference (TOL / TIGHT /
   WINO_TIGHT and the constructors of tests/test_gpu_strides.py; frame_sigma: the bits of tests/sigma_model.py).  The shapes are the ones at
   which a kernel skips a write: ragged tiles, patches almost all outside the image, zero pad chunks, absent temporal sources, masked output
   columns, the folded Winograd band, untouched histogram bins.  That the poison is there when the kernel starts is asserted first
   (CU coverage, canary), and that the harness sees a stale read, with either pattern, on a toy kernel that has one.
   (precision='f16' has no bound in test_gpu_strides.py -- its values are tests/test_gpu_f16.py's; here: the three runs' bits and no NaN.)

B. Allocations.  Every schedule builds a fresh model under stale.poisoned_empty with 0x00 and with 0xFF in every torch.empty: the two results
   and the unpatched one have the same bits and no NaN.
Measured figures and the list of cases: profiles/stale_state.txt."""
import ctypes
import functools
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sigma_model
import stale
from helpers import bsvd_keys
from oracle_exec import OracleExecutor
from seeded import seeded_state
from test_gpu_f16x3 import TIGHT, _Net, from_split, to_split
from test_gpu_f16x3 import _exec as _split_exec
from test_gpu_pair import _setup as _pair_setup
from test_gpu_parity import TOL, _gpu_exec, _one_layer_net
from test_gpu_strides import (WINO_TIGHT, _args, _dev, _entry, _head, _ident, _layer, _no_tweak, _pair, _quant, _randn, _state3, _storage,
                              _stream, _variant)
from test_gpu_v_handover import _layer as _v_layer
from test_gpu_v_handover import _to_v
from test_gpu_wino import _exec as _wino_exec

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the harness itself

def test_poison_reaches_every_cu_and_survives_a_dispatch():
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lib = stale.load()
    # all of a CU's LDS: no product kernel can ask for more (the static_asserts on LDS_BYTES in conv3x3_mfma.hip / conv3x3_winox.hip), so
    # wherever a product workgroup's allocation lands, it lands on poisoned words
    assert lib.stale_lds_bytes() == 160 * 1024
    for pattern in stale.PATTERNS:
        ids = stale.coverage(pattern)
        seen, words = stale.canary(pattern)
        missed = {cu: n for cu, n in seen.items() if any(v != words for v in n)}
        print("pattern %08x: %d bytes of LDS per workgroup, grid %d x %d, poison ran on %d of %d CUs, canary on %d, CUs with a word lost: %d"
              % (pattern, lib.stale_lds_bytes(), stale.GRID_MULTIPLE, n_cu, len(ids), n_cu, len(seen), len(missed)))
        assert len(ids) == n_cu
        assert seen and set(seen) <= ids and not missed, missed
    other, _ = stale.canary(stale.NAN_PATTERN)           # the canary counts a pattern, not whatever it finds
    assert all(v == 0 for n in other.values() for v in n)


def test_harness_passes_the_good_toy_kernel_and_flags_the_bad_one_with_both_patterns():
    """stale_demo_bad reads one LDS cell it never wrote: times a zero mask into lanes 0..62 (only a NaN survives that), through fmaxf into lane
    63 (only a finite value survives that).  On zeroed LDS it computes y = x like stale_demo_good.  Behind either pattern it must differ from
    y = x; stale_demo_good must not."""
    lib = stale.load()
    x = torch.arange(64, dtype=torch.float32, device=_dev()) - 20.5
    y = torch.zeros(64, device=_dev())
    want = x.cpu()
    flagged = {}
    for name in ("stale_demo_good", "stale_demo_bad"):
        fn = getattr(lib, name)

        def launch():
            assert fn(x.data_ptr(), y.data_ptr(), _stream()) == 0
        runs = stale.lds_probe(launch, lambda: y)
        flagged[name] = [not stale.same_bits(r[0], want) for r in runs[1:]]
        if name == "stale_demo_bad":
            nan_run, finite_run = runs[1][0], runs[2][0]
            assert bool(torch.isnan(nan_run[:63]).all()) and float(nan_run[63]) == float(want[63])          # fmaxf laundered the NaN
            assert torch.equal(finite_run[:63], want[:63]) and float(finite_run[63]) != float(want[63])      # the zero mask killed the finite value
            assert not all(stale.probe_verdict(runs).values())
        else:
            assert all(stale.probe_verdict(runs).values())
    assert flagged == {"stale_demo_good": [False, False], "stale_demo_bad": [True, True]}, flagged


# ------------------------------------------------------------------------------------------------ A. the kernel families

def _oracle_state(prec, cin, cout):
    return seeded_state([("l.weight", (cout, cin, 3, 3)), ("l.bias", (cout,))], 7) if prec == "f32" else _state3(cin, cout)


@functools.lru_cache(maxsize=None)
def _one_halo(which, *layer_args):
    """a temporal-fusion layer of test_gpu_strides._layer with compact halos, one of them taken away (NULL: that source is zeros), and its own
    reference"""
    c = _layer(*layer_args)
    prec, cin, cout = layer_args[:3]
    kw = dict(c.kw)
    kw.pop("halo_next" if which == "prev" else "halo_prev")
    split = prec != "f32"
    dec = (lambda t: from_split(t.cpu())) if split else (lambda t: t.cpu())
    from bsvd_amd.schedule import Halo
    okw = {k: Halo(dec(h.t), h.pstride, h.coff) for k, h in kw.items()}
    ref = OracleExecutor(_oracle_state(prec, cin, cout), double=True).conv(c.sp, dec(c.x), **okw)
    return SimpleNamespace(ex=c.ex, sp=c.sp, x=c.x, kw=kw, tweak=c.tweak, ref=ref, tol=c.tol, decode=c.decode)


@functools.lru_cache(maxsize=None)
def _padded(prec, cin, cout, tsm, T, H, W):
    """a layer whose Cin is no multiple of 16: the tensors carry cin_pad channels, the pad ones zero (zero pad chunks in x and in the pack);
    tsm: full neighbour frames as halos (fold = cin / 8 is no multiple of 4: the exact-fp32 kernel's generic gather)"""
    from bsvd_amd.netspec import ConvSpec
    from bsvd_amd.schedule import Halo
    rs = np.random.RandomState(cin * 1000 + cout + H)
    split = prec != "f32"
    st = _oracle_state(prec, cin, cout)
    if split:
        sp = ConvSpec("l", "l", cin, cout, 1, tsm, "relu6", 0)
        ex, tol = _split_exec(_Net(sp), st), TIGHT
    else:
        net, sp = _one_layer_net(cin, cout, 1, tsm, "relu6", 0)
        ex, tol = _gpu_exec(net, st), TOL
    enc, q = (to_split, _quant) if split else (_ident, _ident)

    def rnd(*shape):
        t = _randn(rs, *shape)
        t[..., cin:] = 0
        return q(t)
    x = rnd(T, H, W, sp.cin_pad)
    kw, okw = {}, {}
    if tsm:
        full = rnd(1, H, W, sp.cin_pad)
        okw = dict(halo_prev=Halo(full, sp.cin_pad, sp.fold), halo_next=Halo(full, sp.cin_pad, 0))
        fd = enc(full).to(_dev())
        kw = dict(halo_prev=Halo(fd, sp.cin_pad, sp.fold), halo_next=Halo(fd, sp.cin_pad, 0))
    ref = OracleExecutor(st, double=True).conv(sp, x, **okw)
    return SimpleNamespace(ex=ex, sp=sp, x=enc(x).to(_dev()), kw=kw, tweak=_no_tweak, ref=ref, tol=tol, decode=from_split if split else None)


@functools.lru_cache(maxsize=None)
def _f16(cin, cout, stride, tsm, T, H, W, halos):
    """precision='f16' on one tile: the f16x3 tensors through the one-pass pack.  No reference here (see the header)."""
    from bsvd_amd.engine import HipExecutor, PackedNet
    c = _layer("f16x3", cin, cout, stride, tsm, "relu6", 0, T, H, W, halos)
    st = _state3(cin, cout)
    ex = HipExecutor(PackedNet(_Net(c.sp), {k: torch.as_tensor(v) for k, v in st.items()}, _dev(), "f16"))
    return SimpleNamespace(ex=ex, sp=c.sp, x=c.x, kw=c.kw, tweak=_no_tweak, ref=None, tol=None, decode=from_split)


@functools.lru_cache(maxsize=None)
def _pair_mid32(T, H, W):
    """test_gpu_strides._pair with a 32-channel tensor between the convs: 64 -> 32 -> 64"""
    a, b, st, fused, _ = _pair_setup(64, 32, 64, "relu6", "relu6", 0)
    rs = np.random.RandomState(T * 100 + H + 32)
    x = _quant(torch.from_numpy((rs.rand(T, H, W, 64) * 3 - 0.5).astype(np.float32)))
    oex = OracleExecutor(st, double=True)
    mid = _quant(oex.conv(a, x).float())
    return SimpleNamespace(ex=fused, sp=b, x=to_split(x).to(_dev()), kw=dict(pre=a), tweak=_no_tweak, ref=oex.conv(b, mid), tol=TIGHT, decode=from_split)


RELU6 = ("relu6", 0)
LDS_CASES = {}
for _p in ("f32", "f16x3"):
    _n, _w, _s2 = (_p, 64, 64, 1, False) + RELU6, (_p, 128, 128, 1, True) + RELU6, (_p, 32, 64, 2, False) + RELU6
    LDS_CASES.update({
        # the 64-channel tile, the 128 x 128 tile, the stride-2 tile with 64 of its output columns masked: ragged right and bottom, and patches
        # almost all outside the image
        _p + " narrow 10x19": (_layer, _n + (2, 10, 19)),
        _p + " narrow 33x50": (_layer, _n + (1, 33, 50)),
        _p + " narrow 1x1": (_layer, _n + (1, 1, 1)),
        _p + " narrow 1x37": (_layer, _n + (2, 1, 37)),
        _p + " wide 10x19": (_layer, _w + (3, 10, 19, "full")),
        _p + " wide 33x50": (_layer, _w + (1, 33, 50, "compact")),
        _p + " wide 1x1": (_layer, _w + (1, 1, 1, "compact")),
        _p + " wide 1x37": (_layer, _w + (2, 1, 37, "full")),
        _p + " stride 2, 32 -> 64, 10x19": (_layer, _s2 + (2, 10, 19)),
        _p + " stride 2, 32 -> 64, 33x50": (_layer, _s2 + (1, 33, 50)),
        _p + " stride 2, 32 -> 64, 1x37": (_layer, _s2 + (2, 1, 37)),
        _p + " stride 2, 32 -> 64, 1x1": (_layer, _s2 + (1, 1, 1)),
        # zero pad chunks
        _p + " Cin 24": (_padded, (_p, 24, 64, False, 2, 10, 19)),
        _p + " Cin 30": (_padded, (_p, 30, 64, False, 1, 33, 50)),
        # one frame, both temporal sources absent (the zero-chunk skip); one of them absent
        _p + " fold 8, no halos": (_layer, (_p, 64, 64, 1, True) + RELU6 + (1, 10, 19)),
        _p + " fold 16, no halos": (_layer, _w + (1, 10, 19)),
        _p + " fold 32, no halos": (_layer, (_p, 256, 256, 1, True, "relu", 0, 1, 10, 19)),
        _p + " fold 8, halo_prev only": (_one_halo, ("prev", _p, 64, 64, 1, True) + RELU6 + (1, 10, 19, "compact")),
        _p + " fold 16, halo_next only": (_one_halo, ("next",) + _w + (1, 10, 19, "compact")),
        _p + " fold 16, halo_prev only, 3 frames": (_one_halo, ("prev",) + _w + (3, 10, 19, "compact")),
    })
LDS_CASES.update({
    "f32 fold 3, generic gather": (_padded, ("f32", 24, 64, True, 2, 10, 19)),
    "f32 fold 3, generic gather, one frame": (_padded, ("f32", 24, 64, True, 1, 1, 37)),
    # the 128-accumulator tile
    "f16x3 fat 10x19": (_layer, ("f16x3", 128, 128, 1, True) + RELU6 + (3, 10, 19, "full", "none", None, "direct", 0, 1)),
    "f16x3 fat 33x50": (_layer, ("f16x3", 128, 128, 1, True) + RELU6 + (1, 33, 50, "compact", "none", None, "direct", 0, 1)),
    "f16x3 fat 1x1": (_layer, ("f16x3", 128, 128, 1, True) + RELU6 + (2, 1, 1, "full", "none", None, "direct", 0, 1)),
    "f16x3 fat 1x37, no halos": (_layer, ("f16x3", 128, 128, 1, True) + RELU6 + (1, 1, 37, "none", "none", None, "direct", 0, 1)),
    "f16x3 fat PS_ADD": (_layer, ("f16x3", 128, 256, 1, False, "none", 1, 1, 10, 19, "none", "ps", None, "direct", 0, 1)),
    # epilogues
    "f32 PS_ADD": (_layer, ("f32", 256, 512, 1, False, "none", 1, 1, 10, 19, "none", "ps")),
    "f16x3 PS_ADD": (_layer, ("f16x3", 128, 256, 1, False, "none", 1, 2, 10, 19, "none", "ps")),
    "f32 RESID, NHWC base": (_layer, ("f32", 64, 64, 1, False, "none", 2, 2, 10, 19, "none", "nhwc64")),
    "f32 RESID, planar base": (_layer, ("f32", 64, 64, 1, False, "none", 2, 1, 33, 50, "none", "planar4")),
    "f16x3 exit, clamp": (_layer, ("f16x3", 64, 3, 1, False, "none", 2, 2, 10, 19, "none", "split64", (3, (0.0, 1.0)))),
    "f16x3 exit, clamp, 33x50": (_layer, ("f16x3", 64, 3, 1, False, "none", 2, 1, 33, 50, "none", "split64", (3, (0.0, 1.0)))),
    "f16 wide 10x19": (_f16, (128, 128, 1, True, 3, 10, 19, "full")),
    "f16 wide 1x37, no halos": (_f16, (128, 128, 1, True, 1, 1, 37, "none")),
    # the edge kernels of the exact-fp32 mode
    "head 4, 4x8": (_head, (4, 64, "relu6", 2, 4, 8)),
    "head 4, 9x130": (_head, (4, 64, "relu6", 1, 9, 130)),
    "head 3, 4x8": (_head, (3, 30, "relu", 1, 4, 8)),
    "head 3, 9x130": (_head, (3, 30, "relu", 2, 9, 130)),
    "tail 3, clamp, 4x8": (_layer, ("f32", 64, 3, 1, False, "none", 2, 2, 4, 8, "none", "planar4", (3, (0.0, 1.0)))),
    "tail 3, NHWC base, 9x130": (_layer, ("f32", 64, 3, 1, False, "none", 2, 1, 9, 130, "none", "nhwc64", (3, None))),
    "tail 4, 9x130": (_layer, ("f32", 64, 4, 1, False, "relu", 2, 2, 9, 130, "none", "planar4", (4, None))),
    # the fused entry (K = 4 x 9 = 36 padded to 48; 3 x 9 = 27 padded to 32) and the fused pair
    "entry 4, 17x21": (_entry, (4, 64, 64, "relu6", 2, 17, 21)),
    "entry 4, 1x1": (_entry, (4, 64, 64, "relu6", 1, 1, 1)),
    "entry 3, 17x21": (_entry, (3, 32, 64, "relu", 1, 17, 21)),
    "entry 3, 1x1": (_entry, (3, 32, 64, "relu", 2, 1, 1)),
    "pair mid 64, 10x19": (_pair, (64, 2, 10, 19)),
    "pair mid 64, 1x5": (_pair, (64, 1, 1, 5)),
    "pair mid 64, exit, 10x19": (_pair, (3, 2, 10, 19)),
    "pair mid 32, 10x19": (_pair_mid32, (2, 10, 19)),
    "pair mid 32, 1x5": (_pair_mid32, (1, 1, 5)),
})
# ---- Winograd forms: wino_m 2 / 6 take the half-height tile on these small grids, 42 / 46 the 16-row tile; H = 20: the last band of the 16-row
# grid has 4 rows (F(2,3): folded); W = 1, 7, 17, 48: less than a tile, ragged, exactly one F(6,3) tile
_HALOS = ("none", "compact", "full")
for _m in (2, 6):
    _wn, _t = "wino%d" % _m, ("f16x3", 128, 128, 1, True) + RELU6
    _i = 0
    for _H in (20, 9):
        for _W in (1, 7, 17, 48):
            for _code in (_m, 40 + _m):
                _T, _hl = 1 + _i % 3, _HALOS[(_i // 2) % 3]
                LDS_CASES["F(%d,3) code %d, %dx%dx%d, %s halos" % (_m, _code, _T, _H, _W, _hl)] = (
                    _layer, _t + (_T, _H, _W, _hl, "none", None, _wn, _code))
                _i += 1
    for _code in (_m, 40 + _m):
        LDS_CASES["F(%d,3) code %d, PS_ADD" % (_m, _code)] = (_layer, ("f16x3", 256, 512, 1, False, "none", 1, 1, 20, 17, "none", "ps", None, _wn, _code))
        LDS_CASES["F(%d,3) code %d, f32 in" % (_m, _code)] = (_layer, _t + (2, 20, 17, "full", "none", None, _wn, _code, 0, True, False))
        LDS_CASES["F(%d,3) code %d, f32 in and out" % (_m, _code)] = (_layer, _t + (1, 9, 48, "none", "none", None, _wn, _code, 0, True, True))


def _launcher(lib, a):
    def launch():
        rc = lib.bsvd_conv3x3(ctypes.byref(a), _stream())
        assert rc == 0, (rc, lib.bsvd_last_error())
    return launch


@pytest.mark.parametrize("case", list(LDS_CASES))
def test_layer_behind_poisoned_lds(case):
    build, bargs = LDS_CASES[case]
    c = build(*bargs)
    lib = c.ex.lib
    a, y = _args(c)
    rc, name = _variant(lib, a)
    assert rc == 0, (rc, lib.bsvd_last_error())
    out = _storage(y)
    out.zero_()
    runs = stale.lds_probe(_launcher(lib, a), lambda: out)
    v = stale.probe_verdict(runs)
    clean = runs[0][0]
    val = c.decode(clean) if c.decode else clean
    v["no NaN"] = v["no NaN"] and not bool(torch.isnan(val).any())
    err = None
    if c.ref is not None:
        err = float((val.double() - c.ref.double()).abs().max())
        v["within the bound"] = val.shape == c.ref.shape and err < c.tol
    print("STALE | %s | %s | %s | max-abs vs the oracle %s (bound %s)" % (case, name, v, err, c.tol))
    assert all(v.values()), (case, name, v, err)


def test_the_cases_run_the_tiles_they_name():
    """the variant names behind the case names above (bsvd_conv3x3_variant is a dry run): a dispatch change must not move a case off its tile"""
    want = {"f32 narrow 10x19": "<2,2,4,1,1>[f32]", "f16x3 narrow 10x19": "<4,1,2,2,1>[f16x3]", "f32 wide 10x19": "<2,2,2,2,1>[f32]",
            "f16x3 wide 10x19": "<2,2,2,2,1>[f16x3]", "f16x3 stride 2, 32 -> 64, 33x50": "<4,1,1,4,2>", "f16x3 fat 10x19": "<4,2,2,2,1>[f16x3]",
            "f16x3 fat 1x1": "<4,2,2,2,1>[f16x3]", "f16x3 fat 1x37, no halos": "<4,2,2,2,1>[f16x3]", "f16x3 fold 8, no halos": "[fold8]",
            "f32 fold 3, generic gather": "[generic]",
            "f16 wide 10x19": "[f16]", "head 4, 4x8": "head_kernel<4>", "head 3, 9x130": "head_kernel<3>", "tail 3, clamp, 4x8": "tail_kernel<3>",
            "tail 4, 9x130": "tail_kernel<4>", "entry 4, 17x21": "[fused entry]", "entry 3, 1x1": "[fused entry]", "pair mid 64, 10x19": "[fused pair]",
            "pair mid 32, 1x5": "[fused pair]", "pair mid 64, exit, 10x19": "[planar out][fused pair]", "f16x3 exit, clamp": "[planar out]"}
    for m in (2, 6):
        for case in LDS_CASES:
            if case.startswith("F(%d,3)" % m):
                want[case] = "winox_kernel<F(%d,3)" % m
    for case, piece in want.items():
        build, bargs = LDS_CASES[case]
        c = build(*bargs)
        a, _ = _args(c)
        rc, name = _variant(c.ex.lib, a)
        assert rc == 0 and piece in name, (case, rc, name)
        if case.startswith("F("):
            code = int(case.split("code ")[1].split(",")[0])
            assert ("[8 rows]" in name) == (code < 40), (case, name)
            assert ("[f32 in]" in name) == ("f32 in" in case), (case, name)


@pytest.mark.parametrize("x_v", [False, True])
@pytest.mark.parametrize("H,W", [(20, 50), (9, 17)])
def test_transformed_domain_producer_and_reader_behind_poisoned_lds(H, W, x_v):
    """F(6,3) with y_v (W = 50: two tiles, so the patch pass at their boundary runs) from an fp32 or a transformed input, then the x_v reader
    on what it wrote, each behind both patterns; the reader's result against the oracle's two convs under test_gpu_strides' bound."""
    T = 2
    sp, st = _v_layer(128, 128, False, "relu6", 0)
    ex = _wino_exec(_Net(sp), st, "wino6")
    lib = ex.lib
    xc = _randn(np.random.RandomState(H + W), T, H, W, 128)
    xd = xc.to(_dev())
    xin = _to_v(xd, 6) if x_v else xd
    ex.force_x_f32, ex.force_y_f32, ex.force_y_v = not x_v, False, 6
    a, yv = ex.build_args(sp, xin)
    a.wino_m = 46
    rc, name = _variant(lib, a)
    assert rc == 0 and "[V out]" in name and ("[V in]" in name) == x_v, (rc, name, lib.bsvd_last_error())
    yv.t.zero_()
    v = stale.probe_verdict(stale.lds_probe(_launcher(lib, a), lambda: yv.t))
    assert all(v.values()), ("producer", name, v)
    ex.force_x_f32, ex.force_y_v = False, 0
    for code in (6, 46):
        ra, ry = ex.build_args(sp, yv)
        ra.wino_m = code
        rc, rname = _variant(lib, ra)
        assert rc == 0 and "[V in]" in rname, (rc, rname)
        ry.zero_()
        runs = stale.lds_probe(_launcher(lib, ra), lambda: ry)
        v = stale.probe_verdict(runs)
        oex = OracleExecutor(st, double=True)
        final = oex.conv(sp, oex.conv(sp, xc))
        err = float((from_split(runs[0][0]).double() - final.double()).abs().max())
        print("STALE | y_v producer (x_v %s) -> x_v reader code %d, %dx%d | %s -> %s | %s | max-abs %.3e" % (x_v, code, H, W, name, rname, v, err))
        assert all(v.values()) and err < WINO_TIGHT * max(1.0, float(final.abs().max())), (rname, v, err)


@pytest.mark.parametrize("m,halos", [(6, "compact"), (6, "full"), (6, "none"), (2, "none")])
def test_transformed_domain_reader_with_transformed_halos_behind_poisoned_lds(m, halos):
    from bsvd_amd.schedule import Halo
    T, H, W = 2, 20, 17
    sp, st = _v_layer(128, 128, True, "relu6", 0)
    ex = _wino_exec(_Net(sp), st, "wino%d" % m)
    ex.force_x_f32, ex.force_y_v = False, 0
    rs = np.random.RandomState(H + W + len(halos))
    x = _randn(rs, T, H, W, 128)
    kw, okw = {}, {}
    if halos == "compact":
        hp, hn = _randn(rs, 1, H, W, sp.fold), _randn(rs, 1, H, W, sp.fold)
        okw = dict(halo_prev=Halo(hp[0], sp.fold, 0), halo_next=Halo(hn[0], sp.fold, 0))
        kw = dict(halo_prev=Halo(_to_v(hp.to(_dev()), m)[0], sp.fold, 0), halo_next=Halo(_to_v(hn.to(_dev()), m)[0], sp.fold, 0))
    elif halos == "full":
        full = _randn(rs, 1, H, W, 128)
        fv = _to_v(full.to(_dev()), m)[0]
        okw = dict(halo_prev=Halo(full[0], 128, sp.fold), halo_next=Halo(full[0], 128, 0))
        kw = dict(halo_prev=Halo(fv, 128, sp.fold), halo_next=Halo(fv, 128, 0))
    ref = OracleExecutor(st, double=True).conv(sp, x, **okw)
    a, y = ex.build_args(sp, _to_v(x.to(_dev()), m), **kw)
    a.wino_m = 40 + m
    rc, name = _variant(ex.lib, a)
    assert rc == 0 and "[V in]" in name, (rc, name, ex.lib.bsvd_last_error())
    y.zero_()
    runs = stale.lds_probe(_launcher(ex.lib, a), lambda: y)
    v = stale.probe_verdict(runs)
    err = float((from_split(runs[0][0]).double() - ref.double()).abs().max())
    print("STALE | F(%d,3) x_v reader, %s transformed halos | %s | %s | max-abs %.3e" % (m, halos, name, v, err))
    assert all(v.values()) and err < WINO_TIGHT, (v, err)


@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (1, 4, 12, 20)])
def test_frame_sigma_behind_poisoned_lds(shape):
    """histogram and finish on frames so small that most of the 4096 bins stay untouched: the bits of tests/sigma_model.py, clean and behind
    both patterns"""
    from bsvd_amd import _lib
    from bsvd_amd.engine import require_hip
    lib = require_hip()
    T, C, H, W = shape
    x = np.random.default_rng(H).uniform(0, 1, shape).astype(np.float32)
    d = torch.from_numpy(x).to(_dev())
    ws = torch.full((T, 4096), -1, dtype=torch.int32, device=_dev())
    out = torch.zeros(T, dtype=torch.float32, device=_dev())
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.bsvd_estimate_sigma(d.data_ptr(), T, 3, H, W, H, W, C * H * W, 1.0, 0.0, float(sigma_model.SIGMA_MAX), ws.data_ptr(),
                                           out.data_ptr(), stream), "bsvd_estimate_sigma")
    runs = stale.lds_probe(launch, lambda: (ws, out))
    want_s, want_h = sigma_model.estimate(x)
    assert all(stale.probe_verdict(runs).values()), stale.probe_verdict(runs)
    for h, s in runs:
        assert np.array_equal(h.numpy().view(np.uint32).astype(np.int64), want_h)
        assert np.array_equal(s.numpy().view(np.uint32), np.asarray(want_s, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ B. poisoned allocations under every schedule
# Every case: ``run(build())`` unpatched, then -- inside stale.poisoned_empty -- a FRESH model (packs, rings, plans, graphs rebuilt from poisoned
# memory) under fill 0x00 and under fill 0xFF.  The three results have the same bits and no NaN; where the schedule has a synchronous
# counterpart the suite already compares it with (the clip schedule; the frame_io calls around it), the unpatched result equals that too.

@pytest.fixture
def poisoned(monkeypatch):
    """stale.poisoned_empty bound to this test's monkeypatch"""
    return lambda fill: stale.poisoned_empty(monkeypatch, fill)


def test_wrapper_fills_device_and_pinned_memory_and_is_inert_while_capturing(poisoned):
    for fill in (0x00, 0xFF):
        with poisoned(fill):
            made = [torch.empty((3, 5), device=_dev()), torch.empty_like(torch.zeros(7, device=_dev())), torch.zeros(2, device=_dev()).new_empty((4, 4)),
                    torch.empty_strided((2, 3), (8, 2), device=_dev()), torch.empty(9, dtype=torch.uint8, pin_memory=True)]
            torch.cuda.synchronize()
            for t in made:
                raw = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage(), 0, (t.untyped_storage().nbytes(),), (1,))
                assert bool((raw == fill).all()), (fill, t.shape)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):          # (a fill -- and its synchronize -- inside a capture would end the capture with an error)
                y = torch.empty(16, device=_dev())
                y.fill_(2.0)
            g.replay()
            torch.cuda.synchronize()
            assert bool((y == 2.0).all())


def test_ring_slot_read_one_step_early_is_caught_on_the_device(poisoned, monkeypatch):
    """the first mutant of tests/test_stale_cpu.py inside the real engine on real rings: the comparison of part B has its teeth here too"""
    import bsvd_amd.stream_plan as SP
    from test_stale_cpu import _EarlyRecorder

    class Early(_EarlyRecorder):
        def __init__(self, eng):
            super().__init__(eng, eng.net.temp1["down0"].key)

    x = _clip("c32", SIZES[0]).to(_dev())
    outs = {}
    for mutant in (False, True):
        with monkeypatch.context() as mp:
            if mutant:
                mp.setattr(SP, "_Recorder", Early)
            for fill in (0x00, 0xFF):
                with stale.poisoned_empty(mp, fill):
                    m = _build("c32", precision="f16x3", stream_graphs=False)
                    outs[(mutant, fill)] = _per_frame(m, x).cpu()
                    m.release_stream_buffers()
    assert stale.same_bits(outs[(False, 0x00)], outs[(False, 0xFF)])
    assert not stale.same_bits(outs[(True, 0x00)], outs[(True, 0xFF)])


NETS = {
    "c32": dict(chns=[32, 64, 128], mid_ch=32, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=32),
    "c64": dict(chns=[64, 128, 256], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=64),
    "blind": dict(chns=[64, 128, 256], mid_ch=64, in_ch=4, out_ch=3, norm="none", act="relu", interm_ch=30, blind=True),      # pad channels
    "defaults, bn": dict(),                                                                                               # the constructor's own
}
SIZES = [(5, 16, 24), (5, 20, 28)]


@functools.lru_cache(maxsize=None)
def _weights(name):
    import bsvd_amd
    c = NETS[name]
    if c:
        st = seeded_state(bsvd_keys(c["chns"], c["mid_ch"], c["in_ch"], c["out_ch"], c["interm_ch"], c.get("blind", False)), 11)
        return {k: torch.as_tensor(v) for k, v in st.items()}
    torch.manual_seed(3)
    sd = {k: v.detach().clone() for k, v in bsvd_amd.BSVD(pretrain_ckpt=None).state_dict().items()}
    g = torch.Generator().manual_seed(4)
    for k, v in sd.items():          # BatchNorm statistics away from (0, 1): the fold into the packs does something
        if k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
    return sd


def _build(name, **kw):
    import bsvd_amd
    m = bsvd_amd.BSVD(pretrain_ckpt=None, **dict(NETS[name], **kw))
    m.load_state_dict(_weights(name))
    return m.to(_dev()).eval()


@functools.lru_cache(maxsize=None)
def _clip(name, size):
    T, H, W = size
    blind = NETS[name].get("blind", False)
    x = np.random.RandomState(T + H).uniform(0, 1, (T, 3 if blind else 4, H, W)).astype(np.float32)
    if not blind:
        x[:, 3] = 30 / 255.0
    return torch.from_numpy(x)


def _host(r):
    """a result as host arrays: tensors, numpy arrays, or lists of them"""
    if isinstance(r, (list, tuple)):
        return [a for e in r for a in _host(e)]
    return [r.detach().cpu().contiguous().numpy() if isinstance(r, torch.Tensor) else np.ascontiguousarray(r)]


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _under_both_fills(poisoned, build, run):
    """-> the unpatched result (host arrays), after asserting that both fills reproduce its bits"""
    def once():
        m = build()
        r = run(m)
        torch.cuda.synchronize()
        r = _host(r)
        if hasattr(m, "release_stream_buffers"):
            m.release_stream_buffers()
        return r
    want = once()
    got = []
    for fill in (0x00, 0xFF):
        with poisoned(fill):
            got.append(once())
    assert _same(got[0], got[1]), "fill 0x00 and fill 0xFF give different bits"
    assert _same(got[0], want), "the poisoned runs differ from the unpatched one"
    assert not any(np.isnan(a).any() for a in want if a.dtype.kind == "f")
    return want


def _per_frame(m, x):
    outs = [m.feedin_one_element(x[i:i + 1]) for i in range(x.shape[0])]
    while len(outs) < x.shape[0] + m.shift_num:
        outs.append(m.feedin_one_element(None))
    assert m.feedin_one_element(None) is None
    m.reset()
    return torch.cat(outs[m.shift_num:])


def _overlapped(m, x):
    outs = [m.feed_overlapped(x[i:i + 1]) for i in range(x.shape[0])]
    outs += [m.feed_overlapped(None) for _ in range(m.shift_num + 1)]
    outs.append(m.feed_overlapped(None, last=True))
    m.reset()
    outs = [o for o in outs if o is not None]
    assert len(outs) == x.shape[0]
    return torch.cat(outs)


CLIP_CASES = {
    "c32 fp32": ("c32", dict(precision="fp32")),
    "c32 f16x3": ("c32", dict(precision="f16x3")),
    "c32 f16": ("c32", dict(precision="f16")),
    "c32 direct": ("c32", dict(precision="f16x3", wide_conv="direct")),
    "c32 wino2": ("c32", dict(precision="f16x3", wide_conv="wino2")),
    "c32 wino6": ("c32", dict(precision="f16x3", wide_conv="wino6")),
    "c32 fuse_pairs": ("c32", dict(precision="f16x3", fuse_pairs=True)),
    "c32 wino2, f32_handover on": ("c32", dict(precision="f16x3", wide_conv="wino2", f32_handover=True)),
    "c32 wino2, f32_handover off": ("c32", dict(precision="f16x3", wide_conv="wino2", f32_handover=False)),
    "c32 wino6, v_handover": ("c32", dict(precision="f16x3", wide_conv="wino6", v_handover=True)),
    "c32 weight_scale auto": ("c32", dict(precision="f16x3", weight_scale="auto")),
    "c64 f16x3": ("c64", dict(precision="f16x3")),
    "c64 wino6, v_handover": ("c64", dict(precision="f16x3", wide_conv="wino6", v_handover=True)),
    "blind f16x3": ("blind", dict(precision="f16x3")),
    "blind fp32": ("blind", dict(precision="fp32")),
    "defaults, bn": ("defaults, bn", dict()),
}


@pytest.mark.parametrize("size", SIZES, ids=["5x16x24", "5x20x28"])
@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clip_schedule_on_poisoned_allocations(poisoned, case, size):
    name, kw = CLIP_CASES[case]
    x = _clip(name, size).to(_dev())
    _under_both_fills(poisoned, lambda: _build(name, **kw), lambda m: [m.clip_forward(x), m(x[None])[0]])


def _two_clips(m, x):
    a = _per_frame(m, x)
    for i in range(3):          # an unfinished stream, then reset(): the next clip starts from rings that hold its leftovers
        m.feedin_one_element(x[i:i + 1])
    m.reset()
    return [a, _per_frame(m, x[:2]), _per_frame(m, x)]


def _chunked(chunk, overlap):
    def run(m, x):
        m.stream_chunk, m.stream_overlap = chunk, overlap
        return [m.streaming_forward(c) for c in (x, x[:2], x)]          # (graphs: issued, captured, replayed)
    return run


STREAM_CASES = {
    "feedin_one_element": (dict(), lambda m, x: [_per_frame(m, x) for _ in range(3)]),
    "feedin_one_element, no graphs": (dict(stream_graphs=False), lambda m, x: [_per_frame(m, x) for _ in range(2)]),
    "feedin_one_element, allocating": (dict(stream_rings=False), lambda m, x: [_per_frame(m, x)]),
    "feed_overlapped": (dict(), lambda m, x: [_overlapped(m, x) for _ in range(3)]),
    "feed_overlapped, no graphs": (dict(stream_graphs=False), lambda m, x: [_overlapped(m, x)]),
    "two clips and a reset": (dict(), _two_clips),
    "two frames": (dict(), lambda m, x: [_per_frame(m, x[:2]), _overlapped(m, x[:1])]),
}
for _chunk in (1, 3, "auto"):
    for _ov in (True, False):
        STREAM_CASES["streaming_forward, chunk %s, overlap %s" % (_chunk, _ov)] = (dict(), _chunked(_chunk, _ov))
STREAM_CASES["streaming_forward, chunk 3, no graphs"] = (dict(stream_graphs=False), _chunked(3, True))
STREAM_NETS = {"c32 f16x3": ("c32", dict(precision="f16x3")), "c32 fp32": ("c32", dict(precision="fp32")),
               "c32 wino6 v_handover": ("c32", dict(precision="f16x3", wide_conv="wino6", v_handover=True)), "blind f16x3": ("blind", dict(precision="f16x3"))}
# every schedule on the c32 network in f16x3; the per-frame, the overlapped and one chunked schedule on the others
STREAM_RUNS = [(c, "c32 f16x3") for c in STREAM_CASES]
STREAM_RUNS += [(c, n) for n in list(STREAM_NETS)[1:] for c in ("feedin_one_element", "feed_overlapped", "streaming_forward, chunk 3, overlap True")]


@pytest.mark.parametrize("case,net", STREAM_RUNS, ids=["%s-%s" % cn for cn in STREAM_RUNS])
def test_stream_schedules_on_poisoned_allocations(poisoned, case, net):
    name, kw = STREAM_NETS[net]
    skw, run = STREAM_CASES[case]
    x = _clip(name, SIZES[len(case) % 2]).to(_dev())
    got = _under_both_fills(poisoned, lambda: _build(name, **dict(kw, **skw)), lambda m: run(m, x))
    ref, clip = _build(name, **kw), {}
    for g in got:                            # the existing comparison: every stream schedule == the clip schedule, bit for bit
        n = g.shape[0]                       # (every clip a case streams is the first n frames of x)
        if n not in clip:
            clip[n] = ref.clip_forward(x[:n]).cpu().numpy()
        assert g.tobytes() == clip[n].tobytes()


def _shards(build, x, world):
    """test_gpu_widths._two_shards for any number of ranks: one thread and one fresh model per rank on one device, compact halo slices handed
    over at a barrier"""
    from bsvd_amd.dist import shard_range
    from bsvd_amd.schedule import Halo
    T = x.shape[0]
    boxes, results, errors = {}, [None] * world, []
    barrier = threading.Barrier(world)

    def rank(r):
        try:
            torch.cuda.set_device(0)
            m = build()
            ex = m._executor(_dev())

            class TH:
                def start(self, sp, v):
                    fold = sp.fold
                    boxes[(r, sp.key)] = (ex.halo_pack(v[0], 0, fold), ex.halo_pack(v[-1], fold, fold))

                    class P:
                        def finish(self_p):
                            torch.cuda.synchronize()
                            barrier.wait()
                            prev = boxes[(r - 1, sp.key)][1] if r > 0 else None
                            nxt = boxes[(r + 1, sp.key)][0] if r + 1 < world else None
                            barrier.wait()
                            return (None if prev is None else Halo(prev, fold, 0), None if nxt is None else Halo(nxt, fold, 0))
                    return P()

                def __call__(self, sp, v):
                    return self.start(sp, v).finish()

            a, b = shard_range(T, world, r)
            results[r] = m.clip_forward(x[a:b], TH())
            torch.cuda.synchronize()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
            barrier.abort()

    th = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    return torch.cat(results)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", ["c32 f16x3", "c32 fp32", "c32 wino6, v_handover", "c64 wino6, v_handover"])
def test_sharded_clip_on_poisoned_allocations(poisoned, case, world):
    name, kw = CLIP_CASES[case]
    x = _clip(name, (7, 16, 24)).to(_dev())          # 7 frames: a shard of three frames takes the overlapped start / finish form
    build = lambda: _build(name, **kw)               # noqa: E731

    class Fabric:
        """stands where a model stands in _under_both_fills: every rank builds its own inside"""
    got = _under_both_fills(poisoned, Fabric, lambda _: _shards(build, x, world))
    assert got[0].tobytes() == build().clip_forward(x).cpu().numpy().tobytes()          # sharded == unsharded, bit for bit


def test_tsn_segmented_inference_on_poisoned_allocations(poisoned):
    """TSN + denoise_seq (segments, look-ahead, queued past slices as halos): the golden case of test_gpu_parity, fresh model per fill"""
    import bsvd_amd
    from bsvd_amd.arch import TSN
    from helpers import load_golden, maxabs
    g = load_golden("g10_mimo_segments")
    st = seeded_state([(str(k), tuple(int(v) for v in str(s_).split(","))) for k, s_ in zip(g["tsn_keys"], g["tsn_shapes"])], int(g["seed"]))
    T, psz, fbl = (int(v) for v in g["cfg_a"])
    seq = torch.from_numpy(g["seq_a"])
    nm = torch.full((T, 1) + tuple(seq.shape[-2:]), 30.0 / 255.0)

    def build():
        m = TSN(precision="fp32", num_segments=3, net2d_opt=dict(chns=[32, 64, 128], mid_ch=32, in_ch=4, out_ch=3, norm="none", act="relu6",
                                                                 interm_ch=32, blind=False))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
        return m.to(_dev()).eval()
    got = _under_both_fills(poisoned, build, lambda m: bsvd_amd.denoise_seq(seq, nm, psz, m, future_buffer_len=fbl))
    assert maxabs(got[0], g["den_a"]) < TOL


PIPE_CASES = [("rgb24", None, 16, 24, 30 / 255.0), ("rgb24", "reflect", 18, 26, "auto"), ("nv12", "reflect", 18, 26, 30 / 255.0), ("nv12", None, 16, 24, "auto"),
              ("yuv422p10le", "reflect", 18, 26, "auto"), ("yuv422p10le", None, 16, 24, 30 / 255.0)]
_PIPE_IDS = ["%s-%s-%dx%d-%s" % (f, p, h, w, "auto" if s == "auto" else "const") for f, p, h, w, s in PIPE_CASES]


def _pipe_frames(pix_fmt, n, H, W, seed):
    from test_gpu_sigma import _frames_for
    from test_gpu_yuv_formats import _frames
    return _frames(pix_fmt, n, H, W, seed) if pix_fmt == "yuv422p10le" else _frames_for(pix_fmt, n, H, W, seed)


def _pipe_sync(m, frames, pix_fmt, H, W, pad, sigma):
    """the synchronous path of test_gpu_sigma._sync / test_gpu_yuv_formats._direct on the same frames"""
    from bsvd_amd import frame_io as F
    if pix_fmt != "yuv422p10le":
        from test_gpu_sigma import _sync
        return _sync(m, frames, pix_fmt, H, W, pad, sigma)[0]
    dev = torch.from_numpy(frames.view(np.uint8).reshape(frames.shape[0], -1)).to(_dev())
    y = m.clip_forward(F.yuv_to_input(dev, H, W, pix_fmt, sigma=sigma, pad_to=F.network_size(H, W) if pad else None))
    return F.output_to_yuv(y, pix_fmt, crop_to=(H, W) if pad else None).cpu().numpy().view(frames.dtype).reshape(frames.shape)


@pytest.mark.parametrize("pix_fmt,pad,H,W,sigma", PIPE_CASES, ids=_PIPE_IDS)
def test_clip_pipeline_on_poisoned_allocations(poisoned, pix_fmt, pad, H, W, sigma):
    from bsvd_amd.pipeline import ClipPipeline
    clips = [_pipe_frames(pix_fmt, 3 + (i % 2), H, W, 21 + i) for i in range(3)]
    kw = {} if pix_fmt in ("rgb24", "nv12") else dict(frame_shape=(H, W))

    def run(m):
        return list(ClipPipeline(m, sigma=sigma, depth=2, pix_fmt=pix_fmt, pad=pad, **kw).run(iter(clips)))
    got = _under_both_fills(poisoned, lambda: _build("c32", precision="f16x3"), run)
    m = _build("c32", precision="f16x3")
    for g, c in zip(got, clips):
        assert np.array_equal(g, _pipe_sync(m, c, pix_fmt, H, W, pad, sigma))


@pytest.mark.parametrize("pix_fmt,pad,H,W,sigma", PIPE_CASES, ids=_PIPE_IDS)
def test_live_stream_on_poisoned_allocations(poisoned, pix_fmt, pad, H, W, sigma):
    from bsvd_amd.pipeline import LiveStream
    frames = _pipe_frames(pix_fmt, 5, H, W, 31)

    def run(m):
        live = LiveStream(m, sigma=sigma, depth=2, pix_fmt=pix_fmt, pad=pad, frame_shape=(H, W))
        outs = []
        for rep in range(2):          # the second stream runs on the first one's slots and graphs
            got = [r for r in (live.feed(fr) for fr in frames) if r is not None]
            got += live.flush()
            assert len(got) == len(frames)
            outs.append(np.stack(got))
        return outs
    got = _under_both_fills(poisoned, lambda: _build("c32", precision="f16x3"), run)
    want = _pipe_sync(_build("c32", precision="f16x3"), frames, pix_fmt, H, W, pad, sigma)
    assert all(np.array_equal(g, want) for g in got)


def test_output_to_yuv_without_out_on_poisoned_allocations(poisoned):
    """the surface it allocates: samples written, every byte between them zero, whatever the allocation held"""
    from bsvd_amd.frame_io import output_to_yuv
    from test_gpu_yuv_formats import _layouts
    H, W = 12, 20
    x = torch.from_numpy(np.random.RandomState(2).uniform(-0.1, 1.1, (2, 3, H, W)).astype(np.float32)).to(_dev())
    n = 0
    for pix_fmt in ("yuv420p", "uyvy422", "p210le", "yuv444p10le", "yuv422p10le"):
        for pitches, offsets, _ in _layouts(H, W, pix_fmt):
            n += 1
            _under_both_fills(poisoned, lambda: None, lambda _: output_to_yuv(x, pix_fmt, pitches=pitches, offsets=offsets))
    assert n >= 6
