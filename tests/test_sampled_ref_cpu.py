"""tests/sampled_ref.py held to the full-tensor models it wraps (no GPU).

  a  equivalence: on small tensors the atlas evaluation at EVERY pixel equals the full-tensor evaluation -- bit for bit for
     chain_exec.ChainExecutor (a sequential fmaf chain does not depend on the tensor's shape), within float64 rounding for the float64
     models (BLAS may block by shape).  Measured largest |atlas - full| / max(1, |full|) over all cases of this file: 0 -- with the
     torch / numpy of the recorded run every centre has the full tensor's bits (profiles/production_geometry.txt); asserted: F64_TOL = 2^-46 =
     1.4e-14, 64 ulp of float64, for a BLAS that sums a dot product in another order.  The weakest mutant (a Winograd unit one column
     off its group: the algorithm is shift-invariant, only the fp16 pairs of the transformed values move) differs by 4e-6.  The yardstick
     taken at the centres equals chain_err / wino_err of the full tensor (relative 1e-9) when every pixel is a centre.
  b  mutants of the harness: each must make the same comparison fail.
  c  coverage: for the tile levels of every product variant at every geometry of tests/test_gpu_geometry.py the sample set holds every
     mandatory class; the classes are computed here from (Ho, Wo, tile), not by the sampler.
"""
import numpy as np
import pytest
import torch

import sampled_ref as R
import split_model as S
from chain_exec import ChainExecutor, same_bits
from seeded import seeded_state
from bsvd_amd.netspec import ConvSpec
from bsvd_amd.schedule import Halo

F64_TOL = 2.0 ** -46
worst = {"rel": 0.0}


def _state(*sps):
    return seeded_state([kv for sp in sps for kv in ((sp.key + ".weight", (sp.cout, sp.cin, 3, 3)), (sp.key + ".bias", (sp.cout,)))], 7)


def _pad(t, c):
    return t if t.shape[-1] == c else torch.cat([t, t.new_zeros(t.shape[:-1] + (c - t.shape[-1],))], dim=-1)


def _q(t):
    """values an fp16 pair encodes exactly"""
    return torch.from_numpy(sum(S.pairs(t))).float()


# name, cin, cout, stride, tsm, act, epi, T, H, W, halos, extra
LAYERS = [
    ("plain 64", 64, 64, 1, False, "relu6", 0, 2, 21, 37, "none", None),
    ("padded 30->64", 30, 64, 1, False, "relu", 0, 2, 21, 37, "none", None),
    ("stride 2, odd size", 64, 128, 2, False, "relu6", 0, 2, 21, 37, "none", None),
    ("stride 2, even size", 64, 128, 2, False, "relu6", 0, 1, 12, 20, "none", None),
    ("fold 8, no halo", 64, 64, 1, True, "relu6", 0, 2, 21, 37, "none", None),
    ("fold 8, compact", 64, 64, 1, True, "relu6", 0, 2, 10, 19, "compact", None),
    ("fold 8, frames", 64, 64, 1, True, "relu", 0, 1, 10, 19, "full", None),
    ("fold 16, no halo, 3 frames", 128, 128, 1, True, "relu6", 0, 3, 10, 19, "none", None),
    ("fold 16, compact", 128, 128, 1, True, "relu6", 0, 2, 10, 19, "compact", None),
    ("fold 16, frames", 128, 128, 1, True, "relu6", 0, 2, 10, 19, "full", None),
    ("fold 16, next only", 128, 128, 1, True, "relu6", 0, 2, 10, 19, "next", None),
    ("fold 16, prev only", 128, 128, 1, True, "relu6", 0, 1, 10, 19, "prev", None),
    ("fold 32, frames", 256, 256, 1, True, "relu", 0, 1, 9, 13, "full", None),
    ("PS_ADD skip", 128, 256, 1, False, "none", 1, 2, 10, 19, "none", "skip"),
    ("PS_ADD no skip", 128, 256, 1, False, "none", 1, 1, 10, 19, "none", None),
    ("RESID nhwc base", 64, 64, 1, False, "none", 2, 2, 10, 19, "none", "nhwc"),
    ("RESID planar base, cout 3", 64, 3, 1, False, "none", 2, 2, 10, 19, "none", "planar"),
]
WINO_LAYERS = [c for c in LAYERS if c[1] >= 128 and c[3] == 1]


def _operands(case, split):
    name, cin, cout, stride, tsm, act, epi, T, H, W, halos, extra = case
    sp = ConvSpec("l", "l", cin, cout, stride, tsm, act, epi)
    st = _state(sp)
    rs = np.random.RandomState(zlib_seed(name))
    q = _q if split else (lambda t: t)
    draw = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    x = q(_pad(draw(T, H, W, cin), sp.cin_pad))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    kw = {}
    if extra == "skip":
        kw = dict(extra=q(_pad(draw(T, 2 * Ho, 2 * Wo, cout // 4), sp.out_channels_pad)), extra_pstride=sp.out_channels_pad, extra_cstride=1)
    elif extra == "nhwc":
        kw = dict(extra=q(draw(T, Ho, Wo, 16)), extra_pstride=16, extra_cstride=1)
    elif extra == "planar":
        kw = dict(extra=draw(T, 4, Ho, Wo), extra_pstride=1, extra_cstride=Ho * Wo)
    fold = sp.fold
    if halos == "compact":
        kw.update(halo_prev=Halo(q(draw(H, W, fold)), fold, 0), halo_next=Halo(q(draw(H, W, fold)), fold, 0))
    elif halos in ("full", "next", "prev"):
        fp, fn = q(_pad(draw(1, H, W, cin), sp.cin_pad)), q(_pad(draw(1, H, W, cin), sp.cin_pad))
        if halos != "next":
            kw["halo_prev"] = Halo(fp, sp.cin_pad, fold)
        if halos != "prev":
            kw["halo_next"] = Halo(fn, sp.cin_pad, 0)
    return sp, st, x, kw


def zlib_seed(name):
    import zlib
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def _enc(t):
    return S.container(*S.pairs(t))


def _units(sp, x, kw, split, m=0, mutate=None, extra_planar=False):
    """gather every unit of the small tensor; split: from split16 containers, as a GPU test would hold them"""
    T, H, W, _ = x.shape
    Ho, Wo = (H - 1) // sp.stride + 1, (W - 1) // sp.stride + 1
    g = dict(kw)
    codec = "split" if split else "f32"
    ecodec = codec
    if split:
        x = _enc(x)
        for k in ("halo_prev", "halo_next"):
            if k in g:
                g[k] = Halo(_enc(g[k].t), g[k].pstride, g[k].coff)
        if "extra" in g and g["extra_cstride"] == 1:
            g["extra"] = _enc(g["extra"])
        else:
            ecodec = "f32"
    return R.gather_units(sp, x, R.all_positions(T, Ho, Wo, m or 1), m=m, codec=codec, extra_codec=ecodec, mutate=mutate, **g)


def _full(sp, full, m=1):
    """full-tensor result [T, Ho', Wo', C] -> the layout of the units' centres [N, ny, nx, C] (zeros right of the image)"""
    full = S._np(full)
    k = 2 if sp.epilogue == 1 else 1
    T, Hy, Wy, C = full.shape
    Wo = Wy // k
    nq = (Wo + m - 1) // m
    p = np.zeros((T, Hy, nq * m * k, C), dtype=full.dtype)
    p[:, :, :Wy] = full
    return p.reshape(T, Hy // k, k, nq, m * k, C).transpose(0, 1, 3, 2, 4, 5).reshape(-1, k, m * k, C)


def _close(a, b, what):
    rel = float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
    if "[mutant" not in what:
        worst["rel"] = max(worst["rel"], rel)
    print("%s: atlas vs full, largest relative difference %.3e (all cases so far %.3e)" % (what, rel, worst["rel"]))
    return rel <= F64_TOL


# ------------------------------------------------------------------------------------------------------------------------- a  equivalence
@pytest.mark.parametrize("case", LAYERS, ids=lambda c: c[0])
def test_chain_on_the_atlas_has_the_bits_of_the_full_tensor(case):
    sp, st, x, kw = _operands(case, False)
    want = ChainExecutor(st).conv(sp, x, **kw)
    got = R.eval_chain(st, sp, _units(sp, x, kw, False))
    assert same_bits(got, _full(sp, want))
    assert np.array_equal(got.view(np.uint32), _full(sp, want).view(np.uint32)), "the sign of a zero differs"


@pytest.mark.parametrize("kind", ["head", "tail"])
def test_chain_on_the_atlas_planar_entry_and_exit(kind):
    rs = np.random.RandomState(3)
    T, H, W = 2, 10, 19
    if kind == "head":
        sp = ConvSpec("l", "l", 4, 64, 1, False, "relu6", 0)
        st = _state(sp)
        x = torch.from_numpy(rs.standard_normal((T, 4, H, W)).astype(np.float32))
        want = ChainExecutor(st).conv(sp, x, x_planar=True)
        u = R.gather_units(sp, x, R.all_positions(T, H, W), x_planar=True)
        got = R.eval_chain(st, sp, u)
    else:
        sp = ConvSpec("l", "l", 64, 3, 1, False, "none", 2)
        st = _state(sp)
        x = torch.from_numpy(rs.standard_normal((T, H, W, 64)).astype(np.float32))
        base = torch.from_numpy(rs.standard_normal((T, H, W, 16)).astype(np.float32))
        kw = dict(extra=base, extra_pstride=16, extra_cstride=1)
        want = ChainExecutor(st).conv(sp, x, y_planar=(3, (0.0, 1.0)), **kw).permute(0, 2, 3, 1)
        u = R.gather_units(sp, x, R.all_positions(T, H, W), **kw)
        got = R.eval_chain(st, sp, u, y_planar=(3, (0.0, 1.0)))
    assert np.array_equal(got.view(np.uint32), _full(sp, want.contiguous()).view(np.uint32))


@pytest.mark.parametrize("one_pass", [False, True], ids=["f16x3", "f16"])
@pytest.mark.parametrize("case", LAYERS, ids=lambda c: c[0])
def test_direct_model_on_the_atlas_equals_the_full_tensor(case, one_pass):
    import f16_model as F
    sp, st, x, kw = _operands(case, True)
    w, b = st["l.weight"], st["l.bias"]
    hv = lambda h, i: Halo(S.pairs(h.t)[i], h.pstride, h.coff)
    mk = {k: ((hv(v, 0), hv(v, 1)) if isinstance(v, Halo) else v) for k, v in kw.items()}
    xh, xl = S.pairs(x)
    want = (F.direct_one_pass if one_pass else S.direct_three_pass)(sp, xh, xl, w, b, **mk)
    model, err = R.eval_direct(sp, _units(sp, x, kw, True), w, b, one_pass=one_pass)
    assert _close(model, _full(sp, want), case[0])
    if one_pass:
        h0 = {k: (hv(v, 0) if isinstance(v, Halo) else v) for k, v in kw.items()}
        full_err = S.chain_err(sp, xh, S.pairs(w)[0], b, **h0)
    else:
        full_err = S.chain_err(sp, x.double(), w, b, **kw)
    assert abs(err - full_err) <= 1e-9 * full_err, (err, full_err)


@pytest.mark.parametrize("m", [2, 6])
@pytest.mark.parametrize("case", WINO_LAYERS, ids=lambda c: c[0])
def test_wino_model_on_the_atlas_equals_the_full_tensor(case, m):
    sp, st, x, kw = _operands(case, True)
    w, b = S.detie_wino_weights(st["l.weight"], m), st["l.bias"]
    want = S.wino_model(sp, x.double(), w, m, b, **kw)
    model, err = R.eval_wino(sp, _units(sp, x, kw, True, m=m), w, b, m)
    assert _close(model, _full(sp, want, m), "%s F(%d,3)" % (case[0], m))
    full_err = S.wino_err(sp, x.double(), w, m, b, **kw)
    assert abs(err - full_err) <= 1e-9 * full_err, (err, full_err)


def test_wino_one_pass_model_on_the_atlas_equals_the_full_tensor():
    import f16_model as F
    sp, st, x, kw = _operands(WINO_LAYERS[2], True)
    w, b = st["l.weight"], st["l.bias"]
    want = F.wino_one_pass(sp, x.double(), w, 2, b, **kw)
    model, _ = R.eval_wino(sp, _units(sp, x, kw, True, m=2), w, b, 2, one_pass=True)
    assert _close(model, _full(sp, want, 2), "F(2,3) one pass")


def _two_convs(kind, rs):
    T, H, W = 2, 10, 19
    if kind == "entry":
        a, b = ConvSpec("inc0", "a", 4, 64, 1, False, "relu6", 0), ConvSpec("inc3", "b", 64, 64, 1, False, "relu6", 0)
        x = torch.from_numpy(rs.standard_normal((T, 4, H, W)).astype(np.float32))
        xs = x.permute(0, 2, 3, 1).contiguous()
    elif kind == "entry 3-30":
        a, b = ConvSpec("inc0", "a", 3, 30, 1, False, "relu", 0), ConvSpec("inc3", "b", 30, 64, 1, False, "relu", 0)
        x = torch.from_numpy(rs.standard_normal((T, 3, H, W)).astype(np.float32))
        xs = x.permute(0, 2, 3, 1).contiguous()
    else:
        a, b = ConvSpec("out0", "a", 64, 64, 1, False, "relu6", 0), ConvSpec("out3", "b", 64, 3, 1, False, "none", 2)
        x = xs = _q(torch.from_numpy(rs.standard_normal((T, H, W, 64)).astype(np.float32)))
    return a, b, _state(a, b), x, xs, (T, H, W)


@pytest.mark.parametrize("kind", ["entry", "entry 3-30", "pair"])
def test_two_conv_model_on_the_atlas_equals_the_full_tensor(kind):
    rs = np.random.RandomState(11)
    a, b, st, x, xs, (T, H, W) = _two_convs(kind, rs)
    wa, ba, wb, bb = st["a.weight"], st["a.bias"], st["b.weight"], st["b.bias"]
    kw = {}
    if kind == "pair":
        kw = dict(extra=torch.from_numpy(rs.standard_normal((T, 4, H, W)).astype(np.float32)), extra_pstride=1, extra_cstride=H * W)
    mid = S.direct_three_pass(a, *S.pairs(xs), wa, ba)[..., :a.cout]
    pad = lambda t: np.concatenate([t, np.zeros(t.shape[:-1] + (b.cin_pad - a.cout,))], axis=-1)
    mh, ml = S.pairs(mid)
    want = S.direct_three_pass(b, pad(mh), pad(ml), wb, bb, **kw)
    pos = R.all_positions(T, H, W)
    if kind == "pair":
        u = R.gather_units(b, _enc(x), pos, codec="split", radius=2, **kw)
    else:
        u = R.gather_units(a, x, pos, x_planar=True, radius=2)
    model, err = R.eval_two_convs(a, b, u, wa, ba, wb, bb)
    assert _close(model, _full(b, want), kind)
    y1c, y1d = S.fp32_chain(a, sum(S.pairs(xs)), wa, ba)          # the yardstick of tests/test_gpu_split_passes.py (_pair_chain)
    y2c, _ = S.fp32_chain(b, y1c.float().double(), wb, bb, **kw)
    full_err = float((y2c - S.conv_f64(b, y1d, wb, bb, **kw)).abs().max())
    assert abs(err - full_err) <= 1e-9 * full_err, (err, full_err)
    # mutant: the tensor between the two convs keeps what the first conv made of the unit's zeros outside the image
    u.mutate = "fused_no_zero"
    bad, _ = R.eval_two_convs(a, b, u, wa, ba, wb, bb)
    assert not _close(bad, _full(b, want), kind + " [mutant: not zeroed]")


# --------------------------------------------------------------------------------------------------------------------------- b  mutants
def _case(name):
    return next(c for c in LAYERS if c[0] == name)


@pytest.mark.parametrize("mutate,name", [("col_off", "plain 64"), ("row_off", "plain 64"), ("col_off", "stride 2, odd size"),
                                         ("fold_swap", "fold 16, frames"), ("fold_swap", "fold 8, no halo"), ("no_border_zeros", "plain 64"),
                                         ("ps_swap", "PS_ADD skip"), ("ps_swap", "PS_ADD no skip")])
def test_mutants_of_the_gather_fail_the_bit_comparison(mutate, name):
    sp, st, x, kw = _operands(_case(name), False)
    want = _full(sp, ChainExecutor(st).conv(sp, x, **kw))
    assert same_bits(R.eval_chain(st, sp, _units(sp, x, kw, False)), want)
    assert not same_bits(R.eval_chain(st, sp, _units(sp, x, kw, False, mutate=mutate)), want)


def test_border_zeros_are_what_fails_without_them():
    """the clamped gather repeats the edge pixel: only units at the image's border change"""
    sp, st, x, kw = _operands(_case("plain 64"), False)
    want = _full(sp, ChainExecutor(st).conv(sp, x, **kw))
    u = _units(sp, x, kw, False, mutate="no_border_zeros")
    bad = (R.eval_chain(st, sp, u).view(np.uint32) != want.view(np.uint32)).any(axis=(1, 2, 3))
    T, H, W, _ = x.shape
    border = (u.pos[:, 1] == 0) | (u.pos[:, 1] == H - 1) | (u.pos[:, 2] == 0) | (u.pos[:, 2] == W - 1)
    assert bad.any() and not (bad & ~border).any() and bad[border].mean() > 0.9


@pytest.mark.parametrize("m", [2, 6])
@pytest.mark.parametrize("mutate", ["wino_misalign", "col_off", "row_off", "fold_swap", "no_border_zeros"])
def test_mutants_fail_the_winograd_comparison(mutate, m):
    sp, st, x, kw = _operands(_case("fold 16, frames"), True)
    w, b = S.detie_wino_weights(st["l.weight"], m), st["l.bias"]
    want = _full(sp, S.wino_model(sp, x.double(), w, m, b, **kw), m)
    model, _ = R.eval_wino(sp, _units(sp, x, kw, True, m=m, mutate=mutate), w, b, m)
    assert not _close(model, want, "F(%d,3) [mutant %s]" % (m, mutate))


@pytest.mark.parametrize("mutate,name", [("col_off", "plain 64"), ("fold_swap", "fold 16, compact"), ("ps_swap", "PS_ADD skip")])
def test_mutants_fail_the_float64_comparison(mutate, name):
    sp, st, x, kw = _operands(_case(name), True)
    w, b = st["l.weight"], st["l.bias"]
    hv = lambda h, i: Halo(S.pairs(h.t)[i], h.pstride, h.coff)
    mk = {k: ((hv(v, 0), hv(v, 1)) if isinstance(v, Halo) else v) for k, v in kw.items()}
    want = _full(sp, S.direct_three_pass(sp, *S.pairs(x), w, b, **mk))
    model, _ = R.eval_direct(sp, _units(sp, x, kw, True, mutate=mutate), w, b)
    assert not _close(model, want, "%s [mutant %s]" % (name, mutate))


def test_gathered_outputs_are_the_tensor_s():
    """gather_outputs reads y where the units' centres are: plain, PixelShuffle, planar, split16"""
    rs = np.random.RandomState(5)
    T, H, W = 2, 7, 11
    sp = ConvSpec("l", "l", 128, 256, 1, False, "none", 1)
    x = torch.zeros(T, H, W, 128)
    y = torch.from_numpy(rs.standard_normal((T, 2 * H, 2 * W, 64)).astype(np.float32))
    for m in (1, 2, 6):
        u = R.gather_units(sp, x, R.all_positions(T, H, W, m), m=0 if m == 1 else m)
        v, _, _ = R.gather_outputs(sp, y, u)
        assert np.array_equal(v, _full(sp, y.double(), m))
        v, h, l = R.gather_outputs(sp, _enc(_q(y)), u, codec="split")
        assert np.array_equal(v, _full(sp, _q(y).double(), m)) and np.array_equal(h + l, v)
    sp = ConvSpec("l", "l", 64, 3, 1, False, "none", 2)
    yp = torch.from_numpy(rs.standard_normal((T, 3, H, W)).astype(np.float32))
    u = R.gather_units(sp, torch.zeros(T, H, W, 64), R.all_positions(T, H, W))
    assert np.array_equal(R.gather_outputs(sp, yp, u, y_planar=True)[0], _full(sp, yp.permute(0, 2, 3, 1).double()))


# -------------------------------------------------------------------------------------------------------------------------- c  coverage
PRODUCT_VARIANTS = [
    "conv3x3_kernel<2,2,4,1,1>[f32]", "conv3x3_kernel<2,2,2,2,1>[f32]", "conv3x3_kernel<2,2,2,2,2>[f32]", "head_kernel<4>[f32]", "tail_kernel<3>[f32]",
    "conv3x3_kernel<2,2,4,1,1>[f16x3]", "conv3x3_kernel<4,1,2,2,1>[f16x3]", "conv3x3_kernel<2,1,4,1,1>[f16x3]", "conv3x3_kernel<4,1,1,4,2>[f16x3]",
    "conv3x3_kernel<4,2,2,2,1>[f16x3]", "conv3x3_kernel<2,2,2,2,1>[f16x3]",
    "winox_kernel<F(2,3),2x2>[f16x3]", "winox_kernel<F(2,3),2x2>[f16x3][8 rows]", "winox_kernel<F(6,3),1x2>[f16x3]", "winox_kernel<F(6,3),1x2>[f16x3][8 rows]",
]
GEOMETRIES = [(540, 960, 2), (540, 960, 1), (480, 856, 2), (1080, 1920, 1), (2160, 3840, 1)]


def _scales(H, W):
    """the conv output grids of a network at H x W: full, half and quarter resolution"""
    return [(H, W), ((H - 1) // 2 + 1, (W - 1) // 2 + 1), (((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1)]


@pytest.mark.parametrize("variant", PRODUCT_VARIANTS)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "%dx%dxT%d" % g)
def test_sample_set_holds_every_mandatory_class(variant, geo):
    levels = R.tile_levels(variant)
    m = R.wino_m_of(variant) or 1
    for fold in (0, 16):
        for Ho, Wo in _scales(geo[0], geo[1]):
            T = geo[2]
            pos, mandatory = R.sample_set(Ho, Wo, T, levels, fold=fold, cap=512, group=m)
            again, _ = R.sample_set(Ho, Wo, T, levels, fold=fold, cap=512, group=m)
            assert np.array_equal(pos, again) and mandatory <= len(pos) <= max(512, mandatory) <= R.CAP
            assert len({(f, y, x // m) for f, y, x in pos.tolist()}) == len(pos), "a unit twice"
            assert (pos >= 0).all() and (pos[:, 0] < T).all() and (pos[:, 1] < Ho).all() and (pos[:, 2] < Wo).all()
            # a unit covers the columns of its group
            cover = {(f, y, g) for f, y, x in pos.tolist() for g in range(x // m * m, min(x // m * m + m, Wo))}
            has = lambda f, y, x: (f, y, x) in cover
            for f in {0, T - 1}:                                                             # corners of the first and the last frame
                assert all(has(f, y, x) for y in (0, Ho - 1) for x in (0, Wo - 1))
            assert has(T - 1, Ho - 1, Wo - 1)                                                # the highest address of the launch
            last = [(y, x) for f, y, x in cover if f == T - 1]
            for edge in (lambda y, x: y == 0, lambda y, x: y == Ho - 1, lambda y, x: x == 0, lambda y, x: x == Wo - 1):
                assert sum(1 for y, x in last if edge(y, x)) >= min(8, Ho, Wo), "a run along every border"
            ys, xs = {y for y, _ in last}, {x for _, x in last}
            for th, tw in levels:                                                            # both sides of the three seams, both axes
                for n, t, have in ((Ho, th, ys), (Wo, tw, xs)):
                    want = set()
                    if t < n:
                        want |= {t - 1, t}                                                   # the first seam
                    if n // t >= 2:
                        want |= {(n // t - 1) * t - 1, (n // t - 1) * t}                     # the last seam between two full tiles
                    if n % t and n >= t:
                        want |= {n // t * t - 1, n // t * t}                                 # the seam before the ragged last tile
                    assert want <= have, (variant, th, tw, n, sorted(want - have))
                # ... and a seam CROSSING of the level: the four pixels around a tile corner
                if th < Ho and tw < Wo:
                    assert all(has(T - 1, y, x) for y in (th - 1, th) for x in (tw - 1, tw))
            th, tw = levels[0]                                                               # the last row band: first and last row, at a tile seam
            yb = (Ho - 1) // th * th
            for y in (yb, Ho - 1):
                assert has(T - 1, y, 0) and has(T - 1, y, Wo - 1) and (tw >= Wo or (has(T - 1, y, tw - 1) and has(T - 1, y, tw)))
                assert 2 * tw >= Wo or (has(T - 1, y, 2 * tw - 1) and has(T - 1, y, 2 * tw)), "the seam between two folded tile pairs"
            if fold and T > 1:                                                               # first AND last frame carry seam samples
                first = [(y, x) for f, y, x in cover if f == 0]
                assert len(first) >= 16 and any(y not in (0, Ho - 1) and x not in (0, Wo - 1) for y, x in first)
            assert len(pos) > mandatory or mandatory >= 512, "seeded interior positions fill the set up to the cap"


def test_the_cap_never_cuts_the_mandatory_classes():
    levels = R.tile_levels("winox_kernel<F(2,3),2x2>[f16x3]")
    full, mandatory = R.sample_set(135, 240, 2, levels, fold=32, cap=4096, group=2)
    cut, m2 = R.sample_set(135, 240, 2, levels, fold=32, cap=8, group=2)
    assert m2 == mandatory == len(cut) and np.array_equal(cut, full[:mandatory]) and len(full) == 4096
