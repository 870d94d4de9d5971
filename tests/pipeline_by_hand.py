"""The expected bytes of the pipeline option matrix (tests/pipeline_matrix.py): coloured frames for every format of the matrix, the
synchronous composition of one stream or clip on the default stream -- ``*_to_input``, the noise estimate and its plane, ``scene_scores``,
``clip_forward``, ``blend_output``, ``output_to_*`` -- and the same composition over the numpy models, which anchors the first.  No pipeline
object is used here.  A superset of test_gpu_finish._by_hand: every format family of the matrix with its colour and pitch, every sigma
mode with its gain, and the per-frame estimates, curves and cut scores beside the bytes."""
import collections
import zlib

import numpy as np

import finish_model as FM
import nlf_model as NM
import pipeline_matrix as PM
import rgb_surface_model as R
import scene_model as SC
import sigma_model as SM
import yuv_model as Y2
import yuv_surface_model as YS

DEV = "cuda:0"
BITS = {"rgb24": 8, "nv12": 8, "p010": 10, "yuv420p": 8, "uyvy422": 8, "yuv444p10le": 10, "bgra": 8, "rgba64le": 16, "x2rgb10le": 10,
        "gbrap10le": 10, "rgb0": 8}
DARK = 0.3                        # the second scene's brightness relative to the first

Expected = collections.namedtuple("Expected", "out x y cuts sigma curves scores")
Expected.__doc__ = """out: the surfaces, an array like the frames; x: the network input (device); y: the network's own result before the blend
(device, fp32); cuts: the scene starts used; sigma: estimate_sigma per frame (float32 [n], sigma='auto' rows, gain applied) or None;
curves: estimate_noise_curve per frame (float32 [n,16], sigma='nlf' rows, gain applied) or None; scores: the cut score per frame"""


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
def frames(fmt, size, n, seed, dark_from=None, one_d=False):
    """n frames of ``fmt`` as the pipelines take them, [n, ...], read-only.  Three planes that differ (a ramp along the row, one down the
    column, one along the diagonal: R, G, B, or Y, Cb, Cr -- chroma away from neutral), Gaussian noise of a level of its own per frame
    (2 / 255 rising by 0.7 / 255 a frame), clipped, so that both ends of the code range are met (and planted in two corners, for the
    pictures too small to clip); alpha or filler codes over their whole range; from ``dark_from`` on a second scene, DARK times as bright.
    One RandomState per (format, size, seed)."""
    H, W = size
    rs = np.random.RandomState(zlib.crc32(("%s %dx%d %d" % (fmt, H, W, seed)).encode()))
    top = (1 << BITS[fmt]) - 1
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    yuv = fmt in PM.YUV420_2D + PM.YUV_1D
    clean = np.stack([xx, 1 - yy, (xx + yy) / 2] if not yuv else [0.1 + 0.8 * (xx + yy) / 2, 0.15 + 0.6 * xx, 0.8 - 0.5 * yy])
    codes = np.empty((n, 3, H, W), np.int64)
    for t in range(n):
        scene = clean.copy()
        if dark_from is not None and t >= dark_from:
            scene[:1 if yuv else 3] *= DARK
        v = scene + rs.normal(0, (2 + 0.7 * t) / 255.0, scene.shape)
        codes[t] = np.rint(np.clip(v, 0, 1) * top)
    codes[:, 0, 0, 0], codes[:, 0, -1, -1] = 0, top
    codes[:, 1, 0, -1], codes[:, 2, -1, 0] = top, 0
    fourth = rs.randint(0, top + 1, (n, H, W)).astype(np.int64)
    fourth[:, 0, 0], fourth[:, 0, 1] = 0, top
    if fmt in PM.YUV420_2D:
        sb = PM.sample_bytes(fmt)
        buf = Y2.pack(codes[:, 0], codes[:, 1, ::2, ::2], codes[:, 2, ::2, ::2], fmt, row_pitch=(W + PM.PITCH_EXTRA) * sb)
        out = buf.view("<u2" if sb == 2 else np.uint8).reshape(n, H * 3 // 2, W + PM.PITCH_EXTRA)
    elif fmt in PM.YUV_1D:
        f = YS.FORMATS[fmt]
        sy, sx = (2 if f.sub == 420 else 1), (1 if f.sub == 444 else 2)
        buf = YS.pack(codes[:, 0], codes[:, 1, ::sy, ::sx], codes[:, 2, ::sy, ::sx], fmt)
        out = buf.view("<u2" if f.bits > 8 else np.uint8).reshape(n, -1)
    else:
        buf = R.pack(codes[:, 0], codes[:, 1], codes[:, 2], fmt, fourth, junk=rs if fmt == "x2rgb10le" else None)
        f = R.FORMATS[fmt]
        natural = (H, W) if f.layout == "x2" else (len(f.order), H, W) if f.layout == "planar" else (H, W, len(f.order))
        out = buf.view(R.container(fmt)).reshape((n, -1) if one_d else (n,) + natural)
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


def as_bytes(a):
    """frames [n, ...] -> uint8 [n, frame bytes], a copy"""
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1).copy()


def alpha_of(fmt, a, size):
    """the alpha codes [n,H,W] of frames of an alpha format"""
    return R.unpack(as_bytes(a), size[0], size[1], fmt)[3]


def yuv_kw(row):
    c = PM.COLOURS[row["colour"]] or {}
    return dict(matrix=c.get("matrix", "bt709"), full_range=bool(c.get("full_range", False)), chroma="linear")


def rgb_full_range(row):
    return bool((PM.COLOURS[row["colour"]] or {}).get("full_range", True))


def luma_matrix(row):
    """the blend's luma weights: the stream's matrix for YUV formats, BT.709 for RGB ones"""
    return yuv_kw(row)["matrix"] if row["pix_fmt"] in PM.YUV420_2D + PM.YUV_1D else "bt709"


def dither_of(row):
    return None if row["dither"] == "none" else row["dither"]


# ---- on the device -----------------------------------------------------------------------------------------------------------------------
def by_hand(model, row, fr, size, cuts=None, frame0=0, want_cut=None):
    """row: a dict of the matrix; fr: its frames [n, ...]; size: (H, W) of the picture; cuts: None, the scene starts, or 'auto';
    frame0: the stream index of fr[0] for the random dither.  want_cut (cuts='auto'): must a cut be found?  Default: yes -- a row that
    finds none past frame 0 would pass without having tested a cut.  -> Expected"""
    import torch
    from bsvd_amd import frame_io as F
    fmt = row["pix_fmt"]
    H, W = size
    pad = PM.size_of(row)[1]
    pad_to, crop_to = (F.network_size(H, W), (H, W)) if pad else (None, None)
    n = fr.shape[0]
    dev = torch.from_numpy(as_bytes(fr)).to(DEV)
    s, gain = PM.sigma_of(row)
    mode = PM.SIGMAS[row["sigma"]][0]
    first = s if row["sigma"] == "const" else 0.0                # the per-frame modes: the plane is written below, from the converted frame
    alpha = None
    if fmt == "rgb24":
        x = F.frames_to_input(dev.view(n, H, W, 3), first, pad_to=pad_to)
    elif fmt in PM.YUV420_2D:
        x = F.yuv420_to_input(dev, H, W, fmt, sigma=first, row_pitch=(W + PM.PITCH_EXTRA) * PM.sample_bytes(fmt), pad_to=pad_to, **yuv_kw(row))
    elif fmt in PM.YUV_1D:
        x = F.yuv_to_input(dev, H, W, fmt, sigma=first, pad_to=pad_to, **yuv_kw(row))
    elif fmt in PM.ALPHA:
        x, alpha = F.rgb_to_input(dev, H, W, fmt, full_range=rgb_full_range(row), sigma=first, pad_to=pad_to, return_alpha=True)
    else:
        x = F.rgb_to_input(dev, H, W, fmt, full_range=rgb_full_range(row), sigma=first, pad_to=pad_to)
    sigma = curves = None
    if mode == "auto":
        est = F.estimate_sigma(x, picture=(H, W), gain=gain)
        F.fill_sigma_plane(x, est)
        sigma = est.cpu().numpy()
    elif mode == "nlf":
        c = F.estimate_noise_curve(x, picture=(H, W), gain=gain)
        F.fill_noise_map(x, c)
        curves = c.cpu().numpy()
    elif mode == "curve":
        F.fill_noise_map(x, torch.tensor(s.values, dtype=torch.float32, device=DEV).expand(n, len(s.values)).contiguous())
    sad, grid = F.scene_scores(x, picture=(H, W))
    scores, _ = F.cut_scores(sad.tolist(), grid.shape[1] * grid.shape[2])
    if isinstance(cuts, str):
        cuts = [t for t, v in enumerate(scores) if v >= F.CUT_THRESHOLD]
        if want_cut is None or want_cut:
            assert cuts and 0 not in cuts, ("the detector found no cut past frame 0: the row would pass vacuously", scores)
    cuts = list(cuts or [])
    y = model.clip_forward(x, **(dict(cuts=cuts) if cuts else {})).float().contiguous()
    net = y.clone()
    strength = PM.STRENGTHS[row["strength"]]
    if strength != 1.0:
        F.blend_output(y, x, strength, matrix=luma_matrix(row))
    dk = dict(dither=dither_of(row), dither_seed=PM.DITHER_SEED, frame0=frame0)
    if fmt == "rgb24" and dk["dither"] is None:
        out = F.output_to_frames(y, crop_to=crop_to)
    elif fmt in PM.YUV420_2D:
        out = F.output_to_yuv420(y, fmt, row_pitch=(W + PM.PITCH_EXTRA) * PM.sample_bytes(fmt), crop_to=crop_to, **yuv_kw(row), **dk)
    elif fmt in PM.YUV_1D:
        out = F.output_to_yuv(y, fmt, crop_to=crop_to, **yuv_kw(row), **dk)
    else:
        out = F.output_to_rgb(y, fmt, full_range=rgb_full_range(row) if fmt != "rgb24" else True, crop_to=crop_to, alpha=alpha, **dk)
    torch.cuda.synchronize()
    out = out.cpu().numpy().reshape(n, -1).view(fr.dtype).reshape(fr.shape)
    return Expected(out, x, net, cuts, sigma, curves, scores)


# ---- the same composition over the numpy models --------------------------------------------------------------------------------------------
def anchor(row, fr, size, exp, frame0=0):
    """exp (by_hand's) against the chain of the numpy models.  RGB formats: the decode, pad, noise plane, blend, dither and encode bit for
    bit and byte for byte.  YUV formats: the decode within 1e-6 and the codes equal except a step of 1 at a near-tie of the model -- the
    rule of the YUV kernels' own tests, whose models are float64 --; the noise plane, estimates, curves, cut scores and the blend bit for bit from the
    device's own decoded planes.  The encode side starts from the device's own y."""
    fmt = row["pix_fmt"]
    H, W = size
    pad = PM.size_of(row)[1]
    Hp, Wp = ((H + 3) // 4 * 4, (W + 3) // 4 * 4) if pad else (H, W)
    x = exp.x.cpu().numpy()
    raw = as_bytes(fr)
    rgb = fmt not in PM.YUV420_2D + PM.YUV_1D
    if rgb:
        want, _ = R.to_input(raw, H, W, fmt, rgb_full_range(row) if fmt != "rgb24" else True, pad_to=(Hp, Wp) if pad else None)
        assert np.array_equal(_bits(x[:, :3]), _bits(want)), "decode: the RGB surface model"
    else:
        kw = yuv_kw(row)
        if fmt in PM.YUV420_2D:
            Yc, Cb, Cr, _ = Y2.unpack(raw, H, W, fmt, (W + PM.PITCH_EXTRA) * PM.sample_bytes(fmt))
            want = Y2.decode(Yc, Cb, Cr, BITS[fmt], **kw)
        else:
            Yc, Cb, Cr, _ = YS.unpack(raw, H, W, fmt)
            want = YS.decode(Yc, Cb, Cr, fmt, **kw)
        want = YS.reflect_pad(want, Hp, Wp)
        assert np.abs(x[:, :3].astype(np.float64) - want).max() <= 1e-6, "decode: the YUV model"
        assert np.array_equal(_bits(x[:, :3]), _bits(YS.reflect_pad(x[:, :3, :H, :W], Hp, Wp))), "pad: mirror images of the picture"
    s, gain = PM.SIGMAS[row["sigma"]]
    if row["sigma"] == "const":
        assert np.array_equal(_bits(x[:, 3]), _bits(np.full(x[:, 3].shape, s, np.float32)))
    elif s == "auto":
        est = SM.estimate(x, (H, W), gain=gain)[0]
        assert np.array_equal(_bits(est), _bits(exp.sigma)), "sigma='auto': the estimator model"
        assert np.array_equal(_bits(x[:, 3]), _bits(np.broadcast_to(est[:, None, None], x[:, 3].shape)))
    elif s == "nlf":
        c = NM.estimate(x, (H, W), gain=gain)[0]
        assert np.array_equal(_bits(c), _bits(exp.curves)), "sigma='nlf': the curve model"
        assert np.array_equal(_bits(x[:, 3]), _bits(NM.noise_map(x, c))), "sigma='nlf': the map model"
    else:
        from bsvd_amd.frame_io import NoiseCurve
        c = np.tile(np.asarray(NoiseCurve.from_model(*PM.CURVE_AB).values, np.float32), (x.shape[0], 1))
        assert np.array_equal(_bits(x[:, 3]), _bits(NM.noise_map(x, c))), "sigma=NoiseCurve: the map model"
    want_cuts, want_scores = SC.cuts(x, picture=(H, W))
    assert list(want_scores) == list(exp.scores), "cut scores: the scene model"
    if row["cuts"] == "auto":
        assert want_cuts == exp.cuts, "cuts: the scene model"
    y = exp.y.cpu().numpy()
    sl, sc = (lambda v: v if isinstance(v, tuple) else (v, v))(PM.STRENGTHS[row["strength"]])
    if (sl, sc) != (1.0, 1.0):
        y = FM.blend(y, x[:, :3], sl, sc, FM.LUMA_W[luma_matrix(row)])
    got = as_bytes(exp.out)
    mode = dither_of(row)
    if rgb:
        alpha = alpha_of(fmt, fr, size) if fmt in PM.ALPHA else None
        want = FM.rgb_to_surface(y, fmt, rgb_full_range(row) if fmt != "rgb24" else True, crop_to=(H, W), alpha=alpha, mode=mode,
                                 seed=PM.DITHER_SEED, frame0=frame0)
        assert np.array_equal(got, want), "blend + dither + encode: the finish and RGB surface models"
    else:
        kw = yuv_kw(row)
        if fmt in PM.YUV420_2D:
            pitch = (W + PM.PITCH_EXTRA) * PM.sample_bytes(fmt)
            want, ties = FM.yuv420_codes(y[..., :H, :W], fmt, mode=mode, seed=PM.DITHER_SEED, frame0=frame0, **kw)
            planes = Y2.unpack(got, H, W, fmt, pitch)[:3]
            assert (got[~Y2.sample_mask(got.shape[0], H, W, fmt, pitch, got.shape[1])] == 0).all(), "pitch padding of a fresh surface is zero"
        else:
            want, ties = FM.yuv_codes(y[..., :H, :W], fmt, mode=mode, seed=PM.DITHER_SEED, frame0=frame0, **kw)
            planes = YS.unpack(got, H, W, fmt)[:3]
        assert FM.mismatches(planes, want, ties) == 0, "blend + dither + encode: the finish and YUV models"
