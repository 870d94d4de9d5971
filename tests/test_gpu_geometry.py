"""The layer launches of the SHIPPED geometries -- 540 x 960 (clip and live stream), 480 x 856, 1080 x 1920 and the 2160 x 3840 the README
advertises -- held to the CPU models at sampled output pixels (tests/sampled_ref.py; tests/test_sampled_ref_cpu.py holds that harness to the
full-tensor models).  Every other comparison of a conv kernel with a high-precision reference runs on tensors of about 40 x 48 pixels; a fault
that is a property of position or grid size -- a seam class beyond the first tiles, the ragged last column of 214, the naturally chosen fat /
half-height / folded tile, an XCD range of thousands of tiles, a byte offset in the last octave below 2 GiB -- has nothing else to notice it.

Case table.  Derived from the product: for bsvd_c64 (non-blind and blind) and the c32-sized network every layer slot of netspec is walked at
every geometry, the BsvdConvArgs are the ones engine.HipExecutor.build_args fills for engine.PackedNet's defaults (tile_order by layer
parity, the plain-fp32 hand-over, the fused entry; no fat_min_wgs or tile override anywhere), bsvd_conv3x3_variant names the kernel, and ONE
case is kept per distinct (variant, T, H, W, Cin, Cout, stride, fold, epilogue, act, plain-fp32 output or pairs): a slot whose launch an earlier slot of the session
already checked prints that and returns.  The variant that runs is asserted to be the one the dry run named.  precision 'f16' keeps only the
cases whose variant differs from the f16x3 one in more than the tag (at these geometries: none); the direct form of the wide layers runs
once per geometry (bsvd_c64).  The fused pair and F(6,3) are no default launches of the product: their units are held to the full models on
the CPU (tests/test_sampled_ref_cpu.py) and the kernels to theirs on small shapes (tests/test_gpu_split_passes.py, tests/test_gpu_wino.py).

Per case, once with both halos as full neighbour frames and once with none (temporal layers):
  - the whole output, on the device: y lies inside a 0xFF-filled buffer with 1 MiB of guard on both sides; after the launch no 0xFFFFFFFF word
    is left in it (every element was written), every value is finite, padded channels are zero, both guards are intact;
  - walk independence: the other tile_order, and wino_m + 40 for the Winograd codes, are bit-equal over the whole tensor -- which carries
    the sampled verdict to the pixels that were not sampled, as far as an independent walk can;
  - sampled outputs against the model of the mode, with the margins the small-shape tests assert (nothing new): 'fp32' the bits of
    chain_exec.ChainExecutor; 'f16x3' split_model.needed <= M_DIRECT / M_WINO[m] against direct_three_pass / wino_model; 'f16' the same
    against f16_model.  Every output channel of a sampled pixel is compared, padded ones must be exact zeros in both halves.
Units per case: the mandatory classes of sampled_ref.sample_set (150 - 300), filled up with seeded interior positions to 2^24 / (Cin Cout)
units (at most 4096) -- about a second of model time per evaluation on the host (profiles/production_geometry.txt has the measured times).

The 4K cases (ids `4k-...`, bsvd_c64, T = 1) are a parametrisation of their own so that they can run alone and after the others; the largest,
128 -> 256 PixelShuffle + skip, holds 1.06 GB in, 2.12 GB skip and 2 x 2.12 GB out.  No rings, no whole network at 4K.
"""
import ctypes
import time
import zlib

import numpy as np
import pytest
import torch

import sampled_ref as R
import split_model as S
from chain_exec import assert_same_bits
from helpers import bsvd_keys
from seeded import seeded_state
from test_gpu_f16x3 import to_split

pytestmark = pytest.mark.gpu

NETS = {
    "c64": dict(chns=(64, 128, 256), mid=64, interm=64, act="relu6", blind=False, seed=11),
    "c64blind": dict(chns=(64, 128, 256), mid=64, interm=30, act="relu", blind=True, seed=21),
    "c32": dict(chns=(32, 64, 128), mid=32, interm=32, act="relu6", blind=False, seed=5),
}
GEOS = [("540x960xT2", 540, 960, 2), ("540x960xT1", 540, 960, 1), ("480x856xT2", 480, 856, 2), ("1080x1920xT1", 1080, 1920, 1)]
GEO_4K = ("4k", 2160, 3840, 1)
SLOTS = [("temp1", n) for n in ("inc0", "inc3", "down0", "d0c1", "d0c2", "down1", "d1c1", "d1c2", "u2c1", "u2c2", "up2", "u1c1", "u1c2", "up1",
                                "out0", "out3")] + [("temp2", "inc0"), ("temp2", "inc3"), ("temp2", "out3")]
SCALE = {"inc0": 0, "inc3": 0, "down0": 0, "out0": 0, "out3": 0, "d0c1": 1, "d0c2": 1, "down1": 1, "u1c1": 1, "u1c2": 1, "up1": 1,
         "d1c1": 2, "d1c2": 2, "u2c1": 2, "u2c2": 2, "up2": 2}
WIDE = ("d0c1", "d0c2", "d1c1", "d1c2", "u2c1", "u2c2", "up2", "u1c1", "u1c2", "up1")
MODES = [("fp32", "direct"), ("f16x3", "wino2"), ("f16", "wino2")]
UNIT_WORK = 2 ** 24
GUARD = 1 << 18             # floats: 1 MiB

_seen = {}                  # key of a launch -> id of the case that checked it
_rows = []


def _params(geos, nets):
    out = []
    for gname, H, W, T in geos:
        for net in nets:
            for prec, wide in MODES:
                out += [pytest.param(net, (H, W, T), prec, wide, blk, name, id="%s-%s-%s-%s.%s" % (gname, net, prec, blk, name))
                        for blk, name in SLOTS]
        out += [pytest.param("c64", (H, W, T), "f16x3", "direct", "temp1", name, id="%s-c64-f16x3-direct-temp1.%s" % (gname, name))
                for name in WIDE]
    return out


_execs = {}


def _dev():
    return torch.device("cuda", 0)


def _exec(net_name, prec, wide):
    from bsvd_amd.engine import HipExecutor, PackedNet
    from bsvd_amd.netspec import make_netspec
    k = (net_name, prec, wide)
    if k not in _execs:
        n = NETS[net_name]
        st = seeded_state(bsvd_keys(list(n["chns"]), n["mid"], 4, 3, n["interm"], blind=n["blind"]), n["seed"])
        net = make_netspec(n["chns"], n["mid"], 4, 3, n["act"], n["interm"], n["blind"])
        ex = HipExecutor(PackedNet(net, {k_: torch.as_tensor(v) for k_, v in st.items()}, _dev(), prec, wide))
        assert ex.fat_min_wgs == 0, "BSVD_FAT_MIN_WGS is set: this file is about the kernels production takes"
        _execs[k] = (net, st, ex)
    return _execs[k]


def _guarded(shape, dev):
    """an uninitialised-looking tensor of `shape` inside a 0xFF-filled buffer, 1 MiB of guard on both sides: (buffer, tensor)"""
    n = int(np.prod(shape))
    buf = torch.empty((n + 2 * GUARD) * 4, dtype=torch.uint8, device=dev).fill_(0xFF).view(torch.int32)
    return buf, buf[GUARD:GUARD + n].view(torch.float32).view(shape)


def _check_whole(buf, y, real_ch, f32, planar, what):
    n = y.numel()
    assert bool((buf[:GUARD] == -1).all()) and bool((buf[GUARD + n:] == -1).all()), "%s: a guard band was written" % what
    assert not bool((y.view(torch.int32) == -1).any()), "%s: an element of y was not written" % what
    v = y if f32 else y.view(torch.float16)
    assert bool(torch.isfinite(v).all()), "%s: a value of y is not finite" % what
    if not planar and real_ch < y.shape[-1] and (f32 or real_ch % 16 == 0):          # (a split16 chunk that is partly padding: the sampled check)
        assert not bool(y[..., real_ch:].view(torch.int32).any()), "%s: a padded channel of y is not zero" % what


def _variant(ex, a):
    buf = ctypes.create_string_buffer(128)
    assert ex.lib.bsvd_conv3x3_variant(ctypes.byref(a), buf, 128) == 0, ex.lib.bsvd_last_error()
    return buf.value.decode()


def _launch(ex, a):
    rc = ex.lib.bsvd_conv3x3(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, ex.lib.bsvd_last_error())
    torch.cuda.synchronize()


def _randn(shape, real, gen, split):
    """N(0,1) on the device from the seeded generator, padded channels zero; split: as the split16 container of those values"""
    x = torch.randn(shape, generator=gen, device=_dev())
    if real < shape[-1]:
        x[..., real:] = 0
    return to_split(x) if split else x


def check_slot(net_name, geo, prec, wide, blk, name, case_id):
    from bsvd_amd.netspec import out_hwc
    from bsvd_amd.schedule import Halo
    H0, W0, T = geo
    net, st, ex = _exec(net_name, prec, wide)
    S_ = getattr(net, blk)
    sp = S_[name]
    split = prec != "fp32"
    fused = split and blk == "temp1" and name in ("inc0", "inc3") and ex.fuse_head(S_)
    if fused and name == "inc0":
        print("%s: part of the fused entry (temp1.inc3's case)" % case_id)
        return
    H, W = H0, W0
    for _ in range(SCALE[name]):
        H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dev = _dev()
    entry = blk == "temp1" and name == "inc0" or fused
    sp_in = S_["inc0"] if fused else sp
    exit_ = blk == "temp2" and name == "out3"
    pk = ex.packed
    x_f32 = (not split) or entry or (sp.key in pk.f32_in and sp.key in pk.wino)
    y_f32 = (not split) or exit_ or sp.key in pk.f32_out
    # ---- shapes first (uninitialised tensors): the dry run names the kernel, and a launch that was already checked returns here
    x = torch.empty((T, sp_in.cin, H, W) if entry else (T, H, W, sp.cin_pad), device=dev)
    kw = {}
    Ho, Wo = (H - 1) // sp.stride + 1, (W - 1) // sp.stride + 1
    if sp.epilogue == R.EPI_PS_ADD:
        cq = sp.out_channels_pad
        kw = dict(extra=torch.empty((T, 2 * Ho, 2 * Wo, cq), device=dev), extra_pstride=cq, extra_cstride=1)
    elif sp.epilogue == R.EPI_RESID:
        if blk == "temp1":          # the block input: the planar network input
            kw = dict(extra=torch.empty((T, 4, H, W), device=dev), extra_pstride=1, extra_cstride=H * W)
        else:                       # temp1's output
            cm = S_["inc0"].cin_pad
            kw = dict(extra=torch.empty((T, H, W, cm), device=dev), extra_pstride=cm, extra_cstride=1)
    if exit_:
        kw["y_planar"] = (sp.cout, None)
    if entry:
        kw["x_planar"] = True
    if fused:
        kw["head"] = sp_in
    yshape = (T, sp.cout, H, W) if exit_ else (T,) + out_hwc(sp, H, W)
    buf, y = _guarded(yshape, dev)
    halo_forms = ["none"]
    if sp.tsm:
        hframes = [torch.empty((1, H, W, sp.cin_pad), device=dev) for _ in range(2)]
        halo_forms = ["frames", "none"]
    hkw = lambda form: {} if form == "none" else dict(halo_prev=Halo(hframes[0], sp.cin_pad, sp.fold), halo_next=Halo(hframes[1], sp.cin_pad, 0))
    a, _ = ex.build_args(sp, x, out=y, **kw, **hkw(halo_forms[0]))
    variant = _variant(ex, a)
    assert bool(a.x_f32) == (x_f32 and split and not entry) and bool(a.y_f32) == (y_f32 and split and not exit_), (variant, a.x_f32, a.y_f32)
    if prec == "f16":
        a3 = ex.lib_args_type().from_buffer_copy(a)
        a3.dtype = 2                # BSVD_F16X3
        v3 = _variant(ex, a3)
        if variant.replace("[f16]", "[f16x3]") == v3:
            print("%s: %s differs from %s in the tag only: the f16x3 case stands for it" % (case_id, variant, v3))
            return
    key = (variant, T, H, W, sp.cin_pad, sp.cout_pad, sp.stride, sp.fold, sp.epilogue, sp.act, sp.cin, sp.cout, bool(a.x_f32), bool(a.y_f32))
    if key in _seen:
        print("%s: same launch as %s (%s)" % (case_id, _seen[key], variant))
        return
    _seen[key] = case_id
    # ---- operands
    gen = torch.Generator(device=dev)
    gen.manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)
    if entry:
        x.copy_(torch.rand(x.shape, generator=gen, device=dev))
    else:
        x.copy_(_randn(x.shape, sp.cin, gen, not x_f32))
    if sp.tsm:
        for h in hframes:
            h.copy_(_randn(h.shape, sp.cin, gen, not x_f32))
    ecodec = "f32"
    if "extra" in kw:
        e = kw["extra"]
        if kw["extra_cstride"] != 1:
            e.copy_(torch.rand(e.shape, generator=gen, device=dev))
        else:
            real = sp.out_channels if sp.epilogue == R.EPI_PS_ADD else S_["inc0"].cin
            e.copy_(_randn(e.shape, real, gen, split))
            ecodec = "split" if split else "f32"
    assert not (split and variant.startswith("head_kernel")), "the shipped networks enter through the fused entry in the split modes"
    levels = R.tile_levels(variant)
    m = R.wino_m_of(variant)
    one_pass = "[f16]" in variant
    work = sp.cin_pad * sp.cout_pad * (3 if fused else 1)
    pos, mandatory = R.sample_set(Ho, Wo, T, levels, fold=sp.fold, cap=min(R.CAP, max(1, UNIT_WORK // work)), group=m or 1)
    w, b = st[sp.key + ".weight"], st[sp.key + ".bias"]
    for form in halo_forms:
        what = "%s [%s, halos %s]" % (case_id, variant, form)
        a, _ = ex.build_args(sp, x, out=y, **kw, **hkw(form))
        assert _variant(ex, a) == variant, (what, _variant(ex, a))
        buf.fill_(-1)
        _launch(ex, a)
        _check_whole(buf, y, sp.out_channels, y_f32, exit_, what)
        # ---- walk independence
        buf2, y2 = _guarded(yshape, dev)
        codes = [(a.tile_order ^ 1, a.wino_m)] + ([(a.tile_order, a.wino_m + 40)] if a.wino_m in (2, 6) else [])
        for order, code in codes:
            a2, _ = ex.build_args(sp, x, out=y2, **kw, **hkw(form))
            a2.tile_order, a2.wino_m = order, code
            buf2.fill_(-1)
            _launch(ex, a2)
            assert torch.equal(buf2, buf), "%s: tile_order %d / wino_m %d changes the result or writes a guard" % (what, order, code)
        del buf2, y2
        # ---- sampled outputs against the model of the mode
        t0 = time.perf_counter()
        g = {k_: v for k_, v in kw.items() if k_.startswith("extra")}
        u = R.gather_units(sp_in if fused else sp, x, pos, m=m, x_planar=entry, codec="f32" if x_f32 else "split", extra_codec=ecodec,
                           radius=2 if fused else 1, **({} if fused else g), **hkw(form))
        if fused:
            u.extra = None
        got, ghi, glo = R.gather_outputs(sp, y, u, codec="f32" if y_f32 else "split", y_planar=exit_)
        if ghi is not None and sp.out_channels_pad > sp.out_channels:
            assert not ghi[..., sp.out_channels:].any() and not glo[..., sp.out_channels:].any(), "%s: a padded channel is not zero" % what
        yp = kw.get("y_planar")
        if not split:
            model = R.eval_chain(st, sp, u, y_planar=yp)
            assert_same_bits(got.astype(np.float32), model, what)
            need, limit, err = 0.0, 0, 0.0
        else:
            if fused:
                model, err = R.eval_two_convs(sp_in, sp, u, st[sp_in.key + ".weight"], st[sp_in.key + ".bias"], w, b, one_pass=one_pass)
                limit = S.M_DIRECT
            elif m:
                model, err = R.eval_wino(sp, u, w, b, m, one_pass=one_pass)
                limit = S.M_WINO[m]
            else:
                model, err = R.eval_direct(sp, u, w, b, one_pass=one_pass, y_planar=yp)
                limit = S.M_DIRECT
            assert got.shape == model.shape, (got.shape, model.shape)
            need = S.needed(got, model, err)
        host = time.perf_counter() - t0
        last = lambda k_, v: int((u.pos[:, k_] == v).sum())
        vname = variant + ("[f32 out]" if split and a.y_f32 else "")
        row = ("%-58s %-52s %4dx%-4d T%d %3d->%-3d s%d fold %-2d epi %d %-5s halos %-6s units %4d (mandatory %3d; last row %3d, last col %3d, "
               "last pixel %d) needed %.3f of %d (yardstick %.2e) host %.1f s"
               % (case_id, vname, H, W, T, sp.cin_pad, sp.cout_pad, sp.stride, sp.fold, sp.epilogue, sp.act, form, len(pos), mandatory,
                  last(1, Ho - 1), last(2, (Wo - 1) // (m or 1) * (m or 1)),
                  int(((u.pos[:, 0] == T - 1) & (u.pos[:, 1] == Ho - 1) & (u.pos[:, 2] == (Wo - 1) // (m or 1) * (m or 1))).sum()),
                  need, limit, err, host))
        print(row)
        _rows.append(row)
        if split:
            assert float(np.abs(model).max()) > 0.1 and need <= limit, (what, need, limit)
    del buf, y, x
    torch.cuda.empty_cache()


@pytest.mark.parametrize("net_name,geo,prec,wide,blk,name", _params(GEOS, list(NETS)))
def test_layer_launch_at_a_shipped_geometry(net_name, geo, prec, wide, blk, name, request):
    check_slot(net_name, geo, prec, wide, blk, name, request.node.callspec.id)


@pytest.mark.parametrize("net_name,geo,prec,wide,blk,name", _params([GEO_4K], ["c64"]))
def test_layer_launch_at_4k(net_name, geo, prec, wide, blk, name, request):
    check_slot(net_name, geo, prec, wide, blk, name, request.node.callspec.id)
