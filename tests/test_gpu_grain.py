"""The film-grain model on the device (bsvd_amd/csrc/frame_grain.hip through frame_io.grain_stats / estimate_grain / apply_grain and the
pipelines' ``grain=``): the 256 integers of a frame and the synthesised grain bit for bit against tests/grain_model.py, the closed loop of
tests/grain_cases.py, and ClipPipeline / LiveStream byte for byte against the same steps run by hand through frame_io and
``clip_forward(cuts=...)``, each scene with the model measured on its own first frame."""
import ctypes

import numpy as np
import pytest
import torch

import grain_cases as C
import grain_model as G
from test_gpu_rgb import model      # noqa: F401 -- the small network of the RGB pipeline tests (a module-scoped fixture)
from test_gpu_vst import LENGTHS, SIZE, _frames, _live_all
from test_grain_cpu import noisy_pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _offset_copy(a, elems=1):
    """a device copy of ``a`` whose base is ``elems`` floats past a 16-byte boundary: the scalar paths"""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=DEV)
    t = buf[elems:elems + a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


# ---- the statistics --------------------------------------------------------------------------------------------------------------------------

def _stats_case(T, H, W, Hp, Wp, seed, channels=3, offset=False):
    from bsvd_amd import frame_io as F
    x, y = noisy_pair(T, Hp, Wp, seed=seed, special=H >= 4 and W >= 13)
    if (Hp, Wp) != (H, W):
        for a in (x, y):
            a[:, :, H:, :] = np.nan                                      # the pad region: counted, it would poison every sum
            a[:, :, :, W:] = np.nan
    want = G.stats(x, y, H, W)
    if channels > 3:                                                     # a slack stride: further planes behind the three
        x = np.concatenate([x, np.full((T, channels - 3, Hp, Wp), np.nan, f32)], axis=1)
    xd = _offset_copy(x) if offset else torch.from_numpy(x).to(DEV)
    yd = _offset_copy(y) if offset else torch.from_numpy(y).to(DEV)
    got = F.grain_stats(xd, yd, picture=(H, W)).cpu().numpy()
    assert got.dtype == np.int64 and got.shape == (T, 256)
    bad = np.argwhere(got != want)
    assert not len(bad), ("entries differ from the model (frame, index)", bad[:8].tolist())


@pytest.mark.parametrize("T,H,W,Hp,Wp,channels,offset", [
    (1, 4, 13, 4, 13, 3, False),            # a single anchor
    (1, 5, 14, 5, 14, 3, False),
    (1, 37, 53, 40, 56, 3, True),           # NaN in the pad region, bases that are not float4-aligned, two tile rows
    (3, 64, 96, 64, 96, 5, False),          # three frames, frames a slack stride apart
    (2, 70, 130, 72, 132, 3, False),        # three tile rows and columns, the last of each ragged
    (128, 9, 700, 9, 700, 3, False),        # the launch rule caps a frame's workgroups at 512 / frames = 4; 11 tiles: trips of 4, 4 and 3
])
def test_stats_equal_the_model_bit_for_bit(T, H, W, Hp, Wp, channels, offset):
    _stats_case(T, H, W, Hp, Wp, seed=H * W + T, channels=channels, offset=offset)


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_stats_zero_their_workspace(fill):
    from bsvd_amd import _lib
    from bsvd_amd import frame_io as F
    lib = F.require_hip()
    x, y = noisy_pair(2, 20, 40, seed=77)
    want = G.stats(x, y)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    ws = torch.full((2, 256 * 8), fill, dtype=torch.uint8, device=DEV)
    assert lib.bsvd_grain_stats_bytes(2) == ws.numel()
    w = F._luma_weights("bt709")
    _lib.check(lib.bsvd_grain_stats(xd.data_ptr(), 3 * 20 * 40, yd.data_ptr(), 3 * 20 * 40, 2, 20, 40, 20, 40, w, ws.data_ptr(),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "bsvd_grain_stats")
    assert np.array_equal(ws.cpu().numpy().view(np.int64).reshape(2, 256), want)


def test_stats_follow_the_matrix_and_refuse_bad_tensors():
    from bsvd_amd import frame_io as F
    x, y = noisy_pair(1, 16, 32, seed=5)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    got = F.grain_stats(xd, yd, matrix="bt601").cpu().numpy()
    assert np.array_equal(got, G.stats(x, y, w=G.weights("bt601")))
    for call in (lambda: F.grain_stats(xd, yd[:, :2].contiguous()), lambda: F.grain_stats(xd, yd[:, :, :8].contiguous()), lambda: F.grain_stats(xd.cpu(), yd),
                 lambda: F.grain_stats(xd, yd, picture=(3, 32)), lambda: F.grain_stats(xd, yd, picture=(16, 12)), lambda: F.grain_stats(xd, yd, picture=(17, 32)),
                 lambda: F.grain_stats(xd.half(), yd), lambda: F.grain_stats(xd, yd, matrix="bt0")):
        with pytest.raises(ValueError):
            call()


# ---- the synthesis ---------------------------------------------------------------------------------------------------------------------------

_SET = {}


def _set_model():
    from bsvd_amd import frame_io as F
    if "m" not in _SET:
        _SET["m"] = F.GrainModel.from_values(*C.set_model(), template_seed=C.TEMPLATE_SEED)
    return _SET["m"]


def _picture(T, Hp, Wp, seed):
    """[T,3,Hp,Wp] float32 over all sixteen levels, a little beyond [0, 1] at both ends"""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(-0.05, 1.05, Wp, dtype=f32)[None, None, None, :]
    return (ramp + rng.normal(0, 0.02, (T, 3, Hp, Wp))).astype(f32)


@pytest.mark.parametrize("T,Hp,Wp,frame0,offset", [(1, 4, 4, 0, False), (1, 33, 65, 0, False), (3, 96, 128, 0, False), (3, 96, 128, 5, False),
                                                   (2, 40, 72, 3, True)])
def test_apply_equals_the_model_bit_for_bit(T, Hp, Wp, frame0, offset):
    from bsvd_amd import frame_io as F
    m = _set_model()
    y = _picture(T, Hp, Wp, seed=Hp + Wp)
    want = G.apply(y, m.templates, m.std, 0.75, seed=11, frame0=frame0)
    yd = _offset_copy(y) if offset else torch.from_numpy(y).to(DEV)
    assert F.apply_grain(yd, m, amount=0.75, seed=11, frame0=frame0) is yd
    got = yd.cpu().numpy()
    bad = np.argwhere(_bits(got) != _bits(want))
    assert not len(bad), ("pixels differ from the model", len(bad), bad[:6].tolist())
    assert not np.array_equal(got, y)
    if frame0 == 5:                                                      # a frame's pattern follows its stream index, not its place in the call
        one = torch.from_numpy(y[2:3].copy()).to(DEV)
        F.apply_grain(one, m, amount=0.75, seed=11, frame0=7)
        assert np.array_equal(_bits(one.cpu().numpy()), _bits(want[2:3]))


def test_apply_of_nothing_keeps_every_byte():
    from bsvd_amd import frame_io as F
    y = _picture(1, 8, 16, seed=1)
    y[0, 0, 0, 0], y[0, 1, 1, 1] = np.nan, -0.0
    yd = torch.from_numpy(y).to(DEV)
    F.apply_grain(yd, _set_model(), amount=0.0)
    F.apply_grain(yd, F.GrainModel.from_values(0.0), amount=1.0)
    F.apply_grain(yd, F.GrainModel.from_values([[0.0] * 16] * 3, C.set_model()[1]))
    assert np.array_equal(_bits(yd.cpu().numpy()), _bits(y))
    for call in (lambda: F.apply_grain(yd, None), lambda: F.apply_grain(yd, _set_model(), amount=-1), lambda: F.apply_grain(yd, _set_model(), seed=2 ** 32),
                 lambda: F.apply_grain(yd, _set_model(), frame0=-1), lambda: F.apply_grain(torch.zeros(1, 4, 8, 16, device=DEV), _set_model()),
                 lambda: F.apply_grain(yd.cpu(), _set_model())):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(_bits(yd.cpu().numpy()), _bits(y))


def test_closed_loop_on_the_device():
    """grain from the known model onto flat frames on the device, measured back on the device, fitted on the host: 2 x the numpy model's own
    error (grain_cases: the device adds none, its sums are integers)"""
    from bsvd_amd import frame_io as F
    m = _set_model()
    y = torch.from_numpy(C.flat_frames()).to(DEV)
    x = F.apply_grain(y.clone(), m, seed=C.APPLY_SEED)
    got, pooled = F.estimate_grain(x, y, return_stats=True)
    e_std, e_acf = C.errors(got.std, got.ar)
    print("closed loop, device: std %.4f (bound %.4f), acf %.4f (bound %.4f)" % (e_std, C.STD_BOUND, e_acf, C.ACF_BOUND))
    assert e_std <= C.STD_BOUND and e_acf <= C.ACF_BOUND
    assert pooled[:16].sum() == len(C.LEVELS) * C.H * C.W and all(pooled[l] == C.H * C.W for l in C.LEVELS)


# ---- the pipelines ---------------------------------------------------------------------------------------------------------------------------

SIGMA = 12.0 / 255
_EXPECTED = {}


def _fixed():
    return _set_model()


def _by_hand(m, fmt, fr, grain, cuts, strength=1.0, dither=None, vst=None, amount=1.0, seed=0):
    """the same steps through frame_io and clip_forward, no pipeline object: decode, the source's copy, (the transform), the network, (its
    inverse), the blend, per scene the model measured on its first frame and the grain, encode -> (surfaces like fr, the models used)"""
    from bsvd_amd import frame_io as F
    H, W = SIZE
    n = fr.shape[0]
    net = F.network_size(H, W)
    dev = torch.from_numpy(np.array(fr).reshape(n, -1)).to(DEV)
    sig = 0.0 if vst is not None else SIGMA
    alpha = None
    if fmt == "rgb24":
        x = F.frames_to_input(dev.view(n, H, W, 3), sig, pad_to=net)
    else:
        x, alpha = F.rgb_to_input(dev, H, W, fmt, full_range=True, sigma=sig, pad_to=net, return_alpha=True)
    src = x[:, :3].clone()
    starts = [0] + list(cuts)
    if vst is not None:
        scene_of = [sum(1 for s in starts[1:] if s <= t) for t in range(n)]
        tables = F.build_vst(F.estimate_noise_curve(x[starts].contiguous(), picture=(H, W)))[scene_of].contiguous()
        F.vst_forward(x, tables)
    y = m.clip_forward(x, **(dict(cuts=list(cuts)) if cuts else {})).float().contiguous()
    if vst is not None:
        F.vst_inverse(y, tables)
    if strength != 1.0:
        F.blend_output(y, src, strength)
    models = []
    for a, b in zip(starts, starts[1:] + [n]):
        gm = F.estimate_grain(src[a:a + 1], y[a:a + 1], picture=(H, W)) if grain == "scene" else grain
        models.append(gm)
        F.apply_grain(y[a:b], gm, amount, seed, frame0=a)
    kw = dict(dither=dither, dither_seed=0, frame0=0) if dither else {}
    if fmt == "rgb24" and not dither:
        out = F.output_to_frames(y, crop_to=(H, W))
    else:
        out = F.output_to_rgb(y, fmt, full_range=True, crop_to=(H, W), alpha=alpha, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(fr.shape), models


# (name): format, grain, further pipeline keywords
ROWS = {
    "fixed": ("rgb24", "fixed", {}),
    "scene": ("rgb24", "scene", {}),
    "scene-strength-dither-alpha": ("bgra", "scene", dict(strength=0.6, dither="ordered")),
    "scene-vst": ("rgb24", "scene", dict(vst="scene")),
    "fixed-amount-seed-dither": ("bgra", "fixed", dict(grain_amount=0.5, grain_seed=9, dither="random")),
}


def _row(m, name, fr_slice=None):
    fmt, grain, kw = ROWS[name]
    key = (name, fr_slice)
    if key not in _EXPECTED:
        fr = _frames(fmt) if fr_slice is None else _frames(fmt)[fr_slice[0]:fr_slice[1]]
        _EXPECTED[key] = _by_hand(m, fmt, fr, _fixed() if grain == "fixed" else "scene", [LENGTHS[0]] if fr_slice is None else [],
                                  strength=kw.get("strength", 1.0), dither=kw.get("dither"), vst=kw.get("vst"),
                                  amount=kw.get("grain_amount", 1.0), seed=kw.get("grain_seed", 0))
    return _EXPECTED[key]


def _pipe_kw(name):
    fmt, grain, kw = ROWS[name]
    kw = dict(kw)
    if "vst" not in kw:
        kw["sigma"] = SIGMA
    return fmt, dict(pix_fmt=fmt, pad="reflect", grain=_fixed() if grain == "fixed" else "scene", **kw)


def _same_model(a, b):
    return np.array_equal(a.std, b.std) and np.array_equal(a.ar, b.ar)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_clip_pipeline_equals_the_steps_by_hand(model, name):     # noqa: F811
    from bsvd_amd.pipeline import ClipPipeline
    fmt, kw = _pipe_kw(name)
    fr = _frames(fmt)
    want, models = _row(model, name)
    pipe = ClipPipeline(model, cuts="auto", **kw)
    got = list(pipe.run([fr]))[0]
    assert pipe.last_cuts == [LENGTHS[0]] and got.shape == fr.shape and got.dtype == fr.dtype
    assert np.array_equal(got, want), "the clip differs from the steps by hand"
    assert _same_model(pipe.last_grain_model, models[-1])
    if ROWS[name][1] == "scene":
        assert not _same_model(models[0], models[1])
    if fmt == "bgra":
        assert np.array_equal(got[..., 3], fr[..., 3])
    # the grain did run: without it the bytes are others
    kw.pop("grain")
    plain = list(ClipPipeline(model, cuts="auto", **{k: v for k, v in kw.items() if not k.startswith("grain_")}).run([fr]))[0]
    assert not np.array_equal(plain, want)


LIVE = [("fixed", 2, "manual"), ("scene", 2, "manual"), ("scene", 1, "auto"), ("scene-strength-dither-alpha", 2, "auto"), ("scene-vst", 2, "manual"),
        ("fixed-amount-seed-dither", 1, "manual")]


@pytest.mark.parametrize("name,depth,cuts", LIVE, ids=["-".join(map(str, c)) for c in LIVE])
def test_live_stream_equals_the_steps_by_hand(model, name, depth, cuts):     # noqa: F811
    """the 23 frames (cut=True at the second scene, or cuts='auto'), flush(), four more frames, flush()"""
    from bsvd_amd.pipeline import LiveStream
    fmt, kw = _pipe_kw(name)
    fr = _frames(fmt)
    want, models = _row(model, name)
    live = LiveStream(model, depth=depth, cuts="auto" if cuts == "auto" else None, **kw)
    outs, seen = [], []
    for k, f in enumerate(fr):
        r = live.feed(f, cut=True) if (cuts == "manual" and k == LENGTHS[0]) else live.feed(f)
        if r is not None:
            outs.append(r)
        seen.append(live.last_grain_model)
    outs += live.flush()
    got = np.stack(outs)
    bad = [t for t in range(len(fr)) if not np.array_equal(got[t], want[t])]
    assert not bad, ("frames differ from the by-hand clip result of their scene", bad)
    assert _same_model(live.last_grain_model, models[-1])
    if ROWS[name][1] == "scene":
        assert seen[0] is None and _same_model(next(s for s in seen if s is not None), models[0])        # measured when the frame emerges
    if fmt == "bgra":
        assert np.array_equal(got[..., 3], fr[..., 3])
    a, b = LENGTHS[0], LENGTHS[0] + 4                            # a new stream on the same object: its first frame starts a scene, index 0
    got2 = _live_all(live, fr[a:b])
    assert np.array_equal(got2, _row(model, name, (a, b))[0]), "the stream after flush() differs from the steps by hand"


def test_a_source_ring_one_frame_behind_is_caught(model, monkeypatch):     # noqa: F811
    """the mutant: next_out hands every emerging frame the source of the frame before it -- the second scene's model is measured against a
    frame of the first scene, and the comparison with the by-hand result fails there"""
    from bsvd_amd import pipeline as P

    def next_out(self):
        if self.emitted >= self.fed:
            raise RuntimeError("source ring: frame %d comes out before it went in" % self.emitted)
        self.emitted += 1
        return self.buf[(self.emitted - 2) % self.buf.shape[0]]
    monkeypatch.setattr(P._SourceRing, "next_out", next_out)
    want, _ = _row(model, "scene")
    fr = _frames("rgb24")
    live = P.LiveStream(model, depth=2, **_pipe_kw("scene")[1])
    outs = [r for r in (live.feed(f, cut=(k == LENGTHS[0])) for k, f in enumerate(fr)) if r is not None] + live.flush()
    bad = [t for t in range(len(fr)) if not np.array_equal(outs[t], want[t])]
    assert LENGTHS[0] in bad, bad


def test_defaults_allocate_nothing_launch_nothing_and_keep_every_byte(model, monkeypatch):     # noqa: F811
    from bsvd_amd import pipeline as P
    fr = _frames("rgb24")[:6]

    def refuse(*a, **k):
        raise AssertionError("a grain kernel was asked for")
    for name in ("apply_grain", "estimate_grain"):
        monkeypatch.setattr(P, name, refuse)
    for make in (lambda **kw: P.ClipPipeline(model, sigma=SIGMA, pad="reflect", **kw), lambda **kw: P.LiveStream(model, sigma=SIGMA, pad="reflect", depth=2, **kw)):
        runs = []
        for kw in ({}, dict(grain=None, grain_amount=1.0, grain_seed=0)):
            p = make(**kw)
            runs.append(list(p.run([fr]))[0] if isinstance(p, P.ClipPipeline) else _live_all(p, fr))
            assert not p.grain.active and p.last_grain_model is None and getattr(p, "_source", None) is None
        assert np.array_equal(runs[0], runs[1])
