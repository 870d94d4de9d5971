"""The variance-stabilising transform on the device (bsvd_amd/csrc/frame_vst.hip through frame_io.build_vst / vst_forward / vst_inverse and
the pipelines' ``vst=``): tables, forward and inverse bit for bit against tests/vst_model.py -- float4 and scalar paths, shared and
per-frame tables, with and without the filled plane, inside guard bands --, and ClipPipeline / LiveStream byte for byte against the same
steps run by hand through frame_io and ``clip_forward(cuts=...)``, each scene with its own table."""
import ctypes

import numpy as np
import pytest
import torch

import arena
import nlf_model as NM
import vst_model as V
from helpers import bsvd_keys
from seeded import seeded_state
from test_gpu_rgb import model      # noqa: F401 -- the small network of the RGB pipeline tests (a module-scoped fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
CURVES = V.curves()
FLOORS = (V.FLOOR_MIN, V.FLOOR, 0.05)
_TABLES = {}                                   # (curve name, floor) -> the model's table set: computed once, never written


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _model_tables(name, floor=V.FLOOR):
    if (name, floor) not in _TABLES:
        t = V.tables(CURVES[name], floor)
        t.setflags(write=False)
        _TABLES[(name, floor)] = t
    return _TABLES[(name, floor)]


# ---- build -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("floor", FLOORS)
def test_build_equals_the_model_bit_for_bit(floor):
    from bsvd_amd import frame_io as F
    names = sorted(CURVES)
    want = {n: _model_tables(n, floor) for n in names}
    for n in names:                                            # n = 1
        got = F.build_vst(torch.from_numpy(CURVES[n][None]).to(DEV), floor)
        assert tuple(got.shape) == (1, F.VST_TABLE_FLOATS)
        assert np.array_equal(_bits(got.cpu().numpy()[0]), _bits(want[n])), (n, floor)
        assert _bits(F.vst_sigma(got).cpu().numpy())[0] == _bits(want[n][V.SIGMA_AT])
    for trio in (names[:3], names[2:]):                        # n = 3 in one call
        got = F.build_vst(torch.from_numpy(np.stack([CURVES[n] for n in trio])).to(DEV), floor).cpu().numpy()
        for k, n in enumerate(trio):
            assert np.array_equal(_bits(got[k]), _bits(want[n])), (trio, n, floor)
    curve = F.NoiseCurve(CURVES["random"].tolist())            # the NoiseCurve form, and out=
    out = torch.full((1, F.VST_TABLE_FLOATS), float("nan"), device=DEV)
    assert F.build_vst(curve, floor, out=out) is out
    assert np.array_equal(_bits(out.cpu().numpy()[0]), _bits(want["random"]))


# ---- forward and inverse -----------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 3, 1, 1), (2, 4, 3, 5), (3, 4, 5, 7), (1, 4, 64, 96)]
FRAME_CURVES = ("from_model", "random", "step")


def _case(shape, per_frame, inverse):
    """-> (values fp32 [T,C,H,W], tables fp32 [1 | T, TABLE_FLOATS], expected planes 0 .. 2 fp32 [T,3,H,W], sigma' per frame)"""
    T, C, H, W = shape
    names = FRAME_CURVES[:T] if per_frame else FRAME_CURVES[1:2]
    tabs = np.stack([_model_tables(n) for n in names])
    x = np.empty(shape, f32)
    want = np.empty((T, 3, H, W), f32)
    for t in range(T):
        tab = tabs[t if per_frame else 0]
        G, R = tab[:V.KNOTS], tab[V.R_AT:]
        n = C * H * W
        v = (V.inverse_values(n, 100 + t, G) if inverse else V.test_values(n, 100 + t)).reshape(C, H, W)
        x[t] = v
        want[t] = V.inverse(v[:3], G, R) if inverse else V.forward(v[:3], G)
    sig = [tabs[t if per_frame else 0][V.SIGMA_AT] for t in range(T)]
    return x, tabs, want, sig


def _check(got, x, want, sig, fill, what):
    T, C = x.shape[:2]
    assert np.array_equal(_bits(got[:, :3]), _bits(want)), what
    if C > 3:
        for t in range(T):
            exp = np.full(x.shape[2:], sig[t], f32) if fill else x[t, 3]
            assert np.array_equal(_bits(got[t, 3]), _bits(exp)), (what, "plane 3 of frame %d" % t)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per_frame"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_forward_and_inverse_equal_the_model_bit_for_bit(shape, per_frame, inverse):
    from bsvd_amd import _lib
    from bsvd_amd import frame_io as F
    lib = _lib.load()
    T, C, H, W = shape
    x, tabs, want, sig = _case(shape, per_frame, inverse)
    tables = torch.from_numpy(tabs).to(DEV)
    fills = [False] if inverse else ([False, True] if C > 3 else [False])
    for fill in fills:
        apply = (lambda t: F.vst_inverse(t, tables)) if inverse else (lambda t: F.vst_forward(t, tables, fill_plane=fill))
        # a contiguous tensor at the allocation's base: the float4 path where Hp * Wp and the frame stride allow
        a = torch.from_numpy(x).to(DEV)
        assert apply(a) is a
        _check(a.cpu().numpy(), x, want, sig, fill, "aligned")
        # a contiguous slice one float into an allocation: the base is 4-byte but not 16-byte aligned -- the scalar path and the tails
        flat = torch.full((x.size + 1,), float("nan"), device=DEV)
        b = flat[1:].view(shape)
        b.copy_(torch.from_numpy(x))
        assert b.data_ptr() % 16 == 4 and b.is_contiguous()
        apply(b)
        _check(b.cpu().numpy(), x, want, sig, fill, "one float off")
        assert np.isnan(flat[:1].cpu().numpy()).all()
        # inside guard bands, frames apart by a slack of 4 (float4 where the plane allows) and of 3 (scalars): no byte outside is touched
        for slack in (4, 3):
            ptr, fs, h = arena.place(torch.from_numpy(x).to(DEV), slack)
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            stride = 1 if per_frame else 0
            if inverse:
                rc = lib.bsvd_vst_inverse(ptr, fs, T, H, W, tables.data_ptr(), stride, st)
            else:
                rc = lib.bsvd_vst_forward(ptr, T, H, W, fs, C - 1 if fill else -1, tables.data_ptr(), stride, st)
            torch.cuda.synchronize()
            assert rc == 0, lib.bsvd_last_error()
            _check(h.logical().cpu().numpy(), x, want, sig, fill, "arena, slack %d" % slack)
            assert h.slack_intact(), ("a byte outside the planes was written", slack, h.slack_damage())


def test_a_frame_stride_wider_than_the_planes_written_leaves_the_planes_behind_alone():
    """forward on a 5-plane tensor: without the fill planes 3 and 4 keep their bits, with it the LAST plane is the one written"""
    from bsvd_amd import frame_io as F
    tables = torch.from_numpy(_model_tables("random")[None].copy()).to(DEV)
    x = V.test_values(2 * 5 * 8 * 12, 9).reshape(2, 5, 8, 12)
    a = torch.from_numpy(x).to(DEV)
    F.vst_forward(a, tables, fill_plane=False)
    got = a.cpu().numpy()
    assert np.array_equal(_bits(got[:, 3:]), _bits(x[:, 3:]))
    G = _model_tables("random")[:V.KNOTS]
    assert np.array_equal(_bits(got[:, :3]), _bits(V.forward(x[:, :3], G)))
    F.vst_forward(a, tables, fill_plane=True)                 # the LAST plane is the filled one
    got = a.cpu().numpy()
    assert np.array_equal(_bits(got[:, 3]), _bits(x[:, 3])) and np.all(got[:, 4] == _model_tables("random")[V.SIGMA_AT])


def test_refusals_launch_nothing():
    from bsvd_amd import frame_io as F
    tables = torch.from_numpy(_model_tables("random")[None].copy()).to(DEV)
    x = torch.rand(2, 4, 4, 8, device=DEV)
    before = x.clone()
    two = tables.expand(3, -1).contiguous()
    for call in (lambda: F.vst_forward(x, two), lambda: F.vst_inverse(x, two), lambda: F.vst_forward(x[:, :3].contiguous(), tables),
                 lambda: F.vst_forward(x[:, :2].contiguous(), tables, fill_plane=False), lambda: F.vst_forward(x.half(), tables),
                 lambda: F.vst_forward(x, tables[:, :-1].contiguous()), lambda: F.vst_forward(x.cpu(), tables),
                 lambda: F.vst_forward(x[:, :, :, ::2], tables), lambda: F.build_vst(torch.rand(2, 15, device=DEV)),
                 lambda: F.build_vst(torch.rand(1, 16, device=DEV), floor=2.0 ** -11), lambda: F.build_vst(torch.rand(1, 16, device=DEV), floor=1.5),
                 lambda: F.build_vst(torch.rand(1, 16, device=DEV), floor=float("nan"))):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert torch.equal(x, before)


# ---- the pipelines -----------------------------------------------------------------------------------------------------------------------

SIZE = (30, 42)                   # no multiple of 4: pad='reflect' -> 32 x 44; one row of two 16 x 16 detector blocks
LENGTHS = (12, 11)                # two scenes: latency + depth + 3 = 23 frames at depth 2 with the lagged schedule
AB = ((NM.A, NM.B), (4 * NM.A, NM.B))          # the two scenes' noise: sigma(I) = sqrt(a I + b), a four times as large in the second
_FRAMES = {}
_EXPECTED = {}


def _frames(fmt):
    """23 frames [n,30,42,3|4] uint8, read-only: two scenes of flat 16 x 16 blocks with a ramp on top, each with signal-dependent noise of
    its own curve; bgra: alpha codes over the whole range"""
    if fmt not in _FRAMES:
        H, W = SIZE
        rs = np.random.default_rng(23)
        out, t = [], 0
        for (a, b), n, blocks in zip(AB, LENGTHS, ((0.25, 0.75, 0.5), (0.8, 0.2, 0.45))):
            clean = np.kron(np.array([blocks]), np.ones((32, 16)))[:H, :W] * 0.8 + 0.2 * np.linspace(0, 1, W)[None, :]
            clean = np.stack([clean, clean * 0.9 + 0.05, clean * 0.8 + 0.1])
            for _ in range(n):
                out.append(NM.poisson_gauss_u8(clean, seed=500 + t, a=a, b=b))
                t += 1
        rgb = np.stack(out).transpose(0, 2, 3, 1)                                  # [n,H,W,3]
        if fmt == "bgra":
            alpha = rs.integers(0, 256, rgb.shape[:3] + (1,)).astype(np.uint8)
            rgb = np.concatenate([rgb[..., ::-1], alpha], axis=-1)
        fr = np.ascontiguousarray(rgb)
        fr.setflags(write=False)
        _FRAMES[fmt] = fr
    return _FRAMES[fmt]


def _by_hand(m, fmt, fr, vst, cuts, strength=1.0, floor=V.FLOOR, blind=False):
    """the same steps through frame_io and clip_forward, no pipeline object: decode, the source's copy, curve(s), build, forward, the
    network, inverse, blend, encode -> (surfaces like fr, curves [n,16] or None, sigma' [n])"""
    from bsvd_amd import frame_io as F
    H, W = SIZE
    n = fr.shape[0]
    net = F.network_size(H, W)
    dev = torch.from_numpy(np.array(fr).reshape(n, -1)).to(DEV)
    sig0 = None if blind else 0.0
    alpha = None
    if fmt == "rgb24":
        x = F.frames_to_input(dev.view(n, H, W, 3), sig0, pad_to=net)
    else:
        x, alpha = F.rgb_to_input(dev, H, W, fmt, full_range=True, sigma=sig0, pad_to=net, return_alpha=True)
    src = x[:, :3].clone()
    starts = [0] + list(cuts)
    scene_of = [sum(1 for s in starts[1:] if s <= t) for t in range(n)]
    curves = None
    if isinstance(vst, str):
        c = F.estimate_noise_curve(x[starts].contiguous(), picture=(H, W))
        sets = F.build_vst(c, floor)
        tables = sets[scene_of].contiguous()
        curves = c.cpu().numpy()[scene_of]
    else:
        tables = F.build_vst(vst, floor)
    F.vst_forward(x, tables, fill_plane=not blind)
    y = m.clip_forward(x, **(dict(cuts=list(cuts)) if cuts else {})).float().contiguous()
    F.vst_inverse(y, tables)
    if strength != 1.0:
        F.blend_output(y, src, strength)
    if fmt == "rgb24":
        out = F.output_to_frames(y, crop_to=(H, W))
    else:
        out = F.output_to_rgb(y, fmt, full_range=True, crop_to=(H, W), alpha=alpha)
    torch.cuda.synchronize()
    sig = F.vst_sigma(tables).cpu().numpy()
    return out.cpu().numpy().reshape(fr.shape), curves, np.broadcast_to(sig, (n,)) if len(sig) == 1 else sig


def _vst_arg(kind):
    from bsvd_amd.frame_io import NoiseCurve
    return "scene" if kind == "scene" else NoiseCurve.from_model(*AB[0])


def _expected(m, fmt, kind):
    if (fmt, kind) not in _EXPECTED:
        _EXPECTED[(fmt, kind)] = _by_hand(m, fmt, _frames(fmt), _vst_arg(kind), [LENGTHS[0]])
    return _EXPECTED[(fmt, kind)]


def test_the_two_scenes_have_curves_far_apart(model):     # noqa: F811
    """what the pipeline tests rest on: the detector finds the one cut, and the scenes' tables differ enough that a frame transformed back
    with the other scene's set gives other bytes (shown with the ring mutant below)"""
    from bsvd_amd import frame_io as F
    fr = _frames("rgb24")
    x = F.frames_to_input(torch.from_numpy(fr.copy()).to(DEV), 0.0, pad_to=F.network_size(*SIZE))
    assert F.scene_cuts(x, picture=SIZE) == [LENGTHS[0]]
    _, curves, sig = _expected(model, "rgb24", "scene")
    assert sig[-1] > 1.3 * sig[0] and not np.array_equal(curves[0], curves[-1])


@pytest.mark.parametrize("kind", ["curve", "scene"])
@pytest.mark.parametrize("fmt", ["rgb24", "bgra"])
def test_clip_pipeline_equals_the_steps_by_hand(model, fmt, kind):     # noqa: F811
    from bsvd_amd.pipeline import ClipPipeline
    fr = _frames(fmt)
    want, _, _ = _expected(model, fmt, kind)
    pipe = ClipPipeline(model, pix_fmt=fmt, pad="reflect", cuts="auto", vst=_vst_arg(kind))
    got = list(pipe.run([fr, fr[:5]]))
    assert pipe.last_cuts == [] and got[0].shape == fr.shape and got[0].dtype == fr.dtype
    assert np.array_equal(got[0], want), "the clip differs from the steps by hand"
    assert np.array_equal(got[1], _by_hand(model, fmt, fr[:5], _vst_arg(kind), [])[0]), "the one-scene clip differs from the steps by hand"
    if fmt == "bgra":
        assert np.array_equal(got[0][..., 3], fr[..., 3])


LIVE = [("rgb24", 1, "manual", "scene"), ("bgra", 2, "manual", "scene"), ("rgb24", 2, "auto", "scene"), ("bgra", 1, "auto", "scene"),
        ("rgb24", 2, "manual", "curve")]


def _run_live(m, fmt, depth, cuts, kind, **kw):
    """the 23 frames (cut=True at the second scene, or cuts='auto'), flush(), four more frames, flush() -> the two streams' frames; per feed
    last_noise_curve and last_vst_sigma against the scene of the frame whose step the feed has waited for"""
    from bsvd_amd.pipeline import LiveStream
    fr = _frames(fmt)
    _, curves, sig = _expected(m, fmt, kind)
    live = LiveStream(m, depth=depth, pix_fmt=fmt, pad="reflect", cuts="auto" if cuts == "auto" else None, vst=_vst_arg(kind), **kw)
    assert live.last_vst_sigma is None and live.last_noise_curve is None
    outs = []
    for k, f in enumerate(fr):
        r = live.feed(f, cut=True) if (cuts == "manual" and k == LENGTHS[0]) else live.feed(f)
        if r is not None:
            outs.append(r)
        if cuts == "auto":
            assert bool(live.last_cut) == (k == LENGTHS[0])
        j = k - (depth - 1)
        if j >= 0:
            assert _bits(live.last_vst_sigma) == _bits(sig[j]), ("last_vst_sigma", k)
            if kind == "scene":
                assert np.array_equal(_bits(live.last_noise_curve), _bits(curves[j])), ("last_noise_curve", k)
            else:
                assert live.last_noise_curve is None
    outs += live.flush()
    assert len(outs) == len(fr)
    more = fr[LENGTHS[0]:LENGTHS[0] + 4]                       # a new stream on the same object: its first frame starts a scene
    outs2 = [r for r in (live.feed(f) for f in more) if r is not None] + live.flush()
    assert len(outs2) == 4
    return np.stack(outs), np.stack(outs2)


@pytest.mark.parametrize("fmt,depth,cuts,kind", LIVE, ids=["-".join(map(str, c)) for c in LIVE])
def test_live_stream_equals_the_steps_by_hand(model, fmt, depth, cuts, kind):     # noqa: F811
    fr = _frames(fmt)
    want, _, _ = _expected(model, fmt, kind)
    got, got2 = _run_live(model, fmt, depth, cuts, kind)
    bad = [t for t in range(len(fr)) if not np.array_equal(got[t], want[t])]
    assert not bad, ("frames differ from the by-hand clip result of their scene", bad)
    more = fr[LENGTHS[0]:LENGTHS[0] + 4]
    assert np.array_equal(got2, _by_hand(model, fmt, more, _vst_arg(kind), [])[0]), "the stream after flush() differs from the steps by hand"
    if fmt == "bgra":
        assert np.array_equal(got[..., 3], fr[..., 3])


def test_a_table_ring_one_set_behind_is_caught(model, monkeypatch):     # noqa: F811
    """the mutant: next_out hands every frame the set of the frame before it -- the first frame of the second scene is mapped back with the
    first scene's table, and the comparison with the by-hand result fails there"""
    from bsvd_amd import pipeline as P

    def next_out(self):
        if self.emitted >= self.fed:
            raise RuntimeError("table ring: frame %d comes out before it went in" % self.emitted)
        self.emitted += 1
        return self.buf[(self.emitted - 2) % self.buf.shape[0]]
    monkeypatch.setattr(P._TableRing, "next_out", next_out)
    want, _, _ = _expected(model, "rgb24", "scene")
    got, _ = _run_live(model, "rgb24", 2, "manual", "scene")
    bad = [t for t in range(len(want)) if not np.array_equal(got[t], want[t])]
    assert LENGTHS[0] in bad, bad


def _plain_by_hand(m, fr, sigma):
    """what the pipelines did before ``vst=`` existed: decode with the constant plane, the network, encode"""
    from bsvd_amd import frame_io as F
    x = F.frames_to_input(torch.from_numpy(fr.copy()).to(DEV), sigma, pad_to=F.network_size(*SIZE))
    out = F.output_to_frames(m.clip_forward(x).float().contiguous(), crop_to=SIZE)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_identity_and_exact_ends(model, monkeypatch):     # noqa: F811
    from bsvd_amd import pipeline as P
    from bsvd_amd.frame_io import NoiseCurve
    fr = _frames("rgb24")[:6]
    v = 12.0 / 255
    plain = _plain_by_hand(model, fr, v)
    # strength = 0 with vst='scene' on: the source bytes come back (the blend is in the picture's own domain)
    for make in (lambda **kw: list(P.ClipPipeline(model, pad="reflect", **kw).run([fr]))[0],
                 lambda **kw: _live_all(P.LiveStream(model, pad="reflect", depth=2, **kw), fr)):
        assert np.array_equal(make(vst="scene", strength=0.0), fr)
    # a flat curve and vst=None launch nothing of the transform and give the bytes of sigma=v
    def refuse(*a, **k):
        raise AssertionError("a transform kernel was asked for")
    for name in ("build_vst", "vst_forward", "vst_inverse"):
        monkeypatch.setattr(P, name, refuse)
    for make in (lambda **kw: list(P.ClipPipeline(model, pad="reflect", **kw).run([fr]))[0],
                 lambda **kw: _live_all(P.LiveStream(model, pad="reflect", depth=2, **kw), fr)):
        assert np.array_equal(make(sigma=v), plain)
        assert np.array_equal(make(sigma=v, vst=None), plain)
        assert np.array_equal(make(vst=NoiseCurve([v] * 16)), plain)


def _live_all(live, fr):
    outs = [r for r in (live.feed(f) for f in fr) if r is not None] + live.flush()
    return np.stack(outs)


def test_blind_model_gets_the_transform_and_no_plane():
    import bsvd_amd
    from bsvd_amd.pipeline import ClipPipeline, LiveStream
    st = seeded_state(bsvd_keys([32, 64, 128], 32, 4, 3, 32, True), 11)
    m = bsvd_amd.BSVD(chns=[32, 64, 128], mid_ch=32, in_ch=4, out_ch=3, norm="none", act="relu6", interm_ch=32, blind=True, pretrain_ckpt=None,
                      precision="f16x3")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    m = m.to(torch.device("cuda", 0))
    fr = _frames("rgb24")[:5]
    for kind in ("curve", "scene"):
        want = _by_hand(m, "rgb24", fr, _vst_arg(kind), [], blind=True)[0]
        assert np.array_equal(list(ClipPipeline(m, pad="reflect", vst=_vst_arg(kind)).run([fr]))[0], want)
        assert np.array_equal(_live_all(LiveStream(m, pad="reflect", depth=1, vst=_vst_arg(kind)), fr), want)
    plain = list(ClipPipeline(m, pad="reflect").run([fr]))[0]
    assert not np.array_equal(plain, want)                     # the transform did run
