"""Which entry point of the library every call of bsvd_amd/frame_io.py and bsvd_amd/pipeline.py reaches, and with which scalar arguments:
the bytes are covered elsewhere, this is the trace.  ``frame_io.require_hip`` is replaced by a proxy that logs every call before it
forwards it -- the entry point's name, integers and floats as they are, the fields of by-reference structs and the float arrays by value,
and every other argument whose declared ``argtypes`` entry is a pointer (device memory, the stream) as "ptr" or "null" -- and the sequences
are held, exactly, to tests/golden/frame_io_calls.json.

The rows: every public decode and encode function plain, with ``pad_to`` / ``crop_to`` (also to the size the picture already has: the
pad / crop entry points are still the ones called), dither off and on, ``out=`` given and not, every kind of ``sigma`` and
``return_alpha`` / ``alpha=``, at T = 2 with a 6 x 14 picture inside 8 x 16 (the smallest that is even for 4:2:0, can be reflect-padded and
holds ``grain_stats``' W >= 13), for uint8 RGB, nv12, uyvy422, yuv420p10le and rgba; one call each of the estimate, vst, scene, blend and
grain functions; and two LiveStream and two ClipPipeline runs over 20 frames of 16 x 24 with the small network of the RGB pipeline
tests: the defaults (with the constant sigma the non-blind network needs), and bgra with pad='reflect', cuts='auto', vst='scene',
strength=(0.5, 1), dither='random' and grain='scene'.

The golden file is written by this module itself: BSVD_CALL_TRACE_WRITE=<path> records instead of comparing."""
import ctypes
import json
import numbers
import os

import numpy as np
import pytest
import torch

import pipeline_by_hand as BH
from test_gpu_rgb import model      # noqa: F401 -- the small network of the RGB pipeline tests (a module-scoped fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_io_calls.json")
WRITE = os.environ.get("BSVD_CALL_TRACE_WRITE")
DEV = "cuda:0"
T, PIC, NET = 2, (6, 14), (8, 16)
SIGMA = 30 / 255.0


# ---- the proxy ---------------------------------------------------------------------------------------------------------------------------
def _by_value(obj):
    if isinstance(obj, ctypes.Array):
        return [_by_value(v) for v in obj]
    if isinstance(obj, ctypes.Structure):
        return {name: _by_value(getattr(obj, name)) for name, *_ in obj._fields_}
    return obj


def _is_pointer(argtype):
    return argtype in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(argtype, type) and issubclass(argtype, ctypes._Pointer))


def _logged(arg, argtype):
    if hasattr(arg, "_obj"):                                # ctypes.byref(struct)
        return _by_value(arg._obj)
    if isinstance(arg, (ctypes.Array, ctypes.Structure)):
        return _by_value(arg)
    if _is_pointer(argtype):
        value = arg.value if isinstance(arg, ctypes.c_void_p) else arg
        return "ptr" if value else "null"
    if isinstance(arg, bool) or isinstance(arg, numbers.Integral):
        return int(arg)
    assert isinstance(arg, numbers.Real), (type(arg), argtype)
    return float(arg)


class _Proxy:
    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            assert len(args) == len(fn.argtypes), (name, len(args), len(fn.argtypes))
            self._log.append([name] + [_logged(a, t) for a, t in zip(args, fn.argtypes)])
            return fn(*args)
        return call


class _Trace:
    """rows of one section: ``with trace.row(name):`` logs the calls made inside under that name"""

    def __init__(self, monkeypatch):
        from bsvd_amd import frame_io
        self.rows, self._log = {}, None
        real = frame_io.require_hip
        monkeypatch.setattr(frame_io, "require_hip", lambda: _Proxy(real(), self._log) if self._log is not None else real())

    def row(self, name):
        trace = self

        class Row:
            def __enter__(self):
                assert name not in trace.rows, name
                trace._log = trace.rows[name] = []

            def __exit__(self, *exc):
                trace._log = None
        return Row()


# ---- the rows ----------------------------------------------------------------------------------------------------------------------------
def _sigmas():
    from bsvd_amd.frame_io import NoiseCurve
    return [("none", None, 1.0), ("float", SIGMA, 1.0), ("auto", "auto", 1.25), ("nlf", "nlf", 0.8),
            ("curve", NoiseCurve.from_model(2.0e-3, 1.0e-4), 1.0), ("list", [0.05, 0.1], 1.0),
            ("tensor", torch.tensor([0.05, 0.1], dtype=torch.float32, device=DEV), 1.0)]


def _surface(nbytes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (T, nbytes), dtype=torch.uint8, generator=g).to(DEV)


def _planes(C, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((T, C) + tuple(hw), generator=g).to(DEV)


GEOMETRIES = [("plain", NET, None), ("pad", PIC, NET), ("pad_same", NET, NET)]      # (name, the picture, pad_to / the tensor cropped from)
DITHER_KW = [("off", {}), ("ordered", dict(dither="ordered")), ("random", dict(dither="random", dither_seed=7, frame0=5))]
YUV_KW = dict(matrix="bt601", full_range=True, chroma="nearest")


def section_decode(tr):
    from bsvd_amd import frame_io as F
    for gname, (H, W), pad in GEOMETRIES:
        picture = pad is not None
        for sname, sigma, gain in _sigmas():
            tag = "%s-%s" % (gname, sname)
            u8 = _surface(H * W * 3, 1).view(T, H, W, 3)
            with tr.row("frames_to_input-" + tag):
                F.frames_to_input(u8, sigma, pad_to=pad, sigma_gain=gain)
            nv12 = _surface((F.yuv420_picture_bytes if picture else F.yuv420_frame_bytes)(H, W, "nv12"), 2)
            with tr.row("yuv420_to_input-nv12-" + tag):
                F.yuv420_to_input(nv12, H, W, "nv12", sigma=sigma, pad_to=pad, sigma_gain=gain, **YUV_KW)
            for fmt in ("uyvy422", "yuv420p10le"):
                with tr.row("yuv_to_input-%s-%s" % (fmt, tag)):
                    F.yuv_to_input(_surface(F.yuv_frame_bytes(H, W, fmt), 3), H, W, fmt, sigma=sigma, pad_to=pad, sigma_gain=gain, **YUV_KW)
            rgba = _surface(F.rgb_frame_bytes(H, W, "rgba"), 4)
            with tr.row("rgb_to_input-rgba-" + tag):
                F.rgb_to_input(rgba, H, W, "rgba", full_range=False, sigma=sigma, pad_to=pad, sigma_gain=gain)
            with tr.row("rgb_to_input-rgba-alpha-" + tag):
                F.rgb_to_input(rgba, H, W, "rgba", sigma=sigma, pad_to=pad, sigma_gain=gain, return_alpha=True)
            into = torch.empty((T, H, W), dtype=torch.uint8, device=DEV)
            with tr.row("rgb_to_input-rgba-alpha-into-" + tag):
                F.rgb_to_input(rgba, H, W, "rgba", sigma=sigma, pad_to=pad, sigma_gain=gain, return_alpha=into)
    H, W = NET
    with tr.row("frames_to_input-chw"):
        F.frames_to_input(_surface(3 * H * W, 5).view(T, 3, H, W), SIGMA, hwc=False)
    with tr.row("yuv420_to_input-nv12-row_pitch"):
        F.yuv420_to_input(_surface(F.yuv420_frame_bytes(H, W, "nv12", 32), 6), H, W, "nv12", sigma=SIGMA, row_pitch=32)
    with tr.row("yuv_to_input-yuv420p10le-pitches"):
        F.yuv_to_input(_surface(F.yuv_frame_bytes(H, W, "yuv420p10le", (64, 32, 32), (16, 0, 0)), 7), H, W, "yuv420p10le", sigma=SIGMA,
                       pitches=(64, 32, 32), offsets=(16, 0, 0))
    with tr.row("rgb_to_input-rgba-pitches"):
        F.rgb_to_input(_surface(F.rgb_frame_bytes(H, W, "rgba", (96,), (32,)), 8), H, W, "rgba", sigma=SIGMA, pitches=(96,), offsets=(32,))


def section_encode(tr):
    from bsvd_amd import frame_io as F
    y = _planes(3, NET, 11)
    for gname, (H, W), full in GEOMETRIES:
        crop = None if full is None else (H, W)
        picture = full is not None
        for hwc in (True, False):
            for bgr in (False, True):
                with tr.row("output_to_frames-%s-%s-%s" % (gname, "hwc" if hwc else "chw", "bgr" if bgr else "rgb")):
                    F.output_to_frames(y, hwc=hwc, rgb2bgr=bgr, crop_to=crop)
        alpha = torch.full((T, H, W), 77, dtype=torch.uint8, device=DEV)
        for dname, dkw in DITHER_KW:
            for given in (False, True):
                tag = "%s-%s-%s" % (gname, dname, "out" if given else "new")
                n = (F.yuv420_picture_bytes if picture else F.yuv420_frame_bytes)(H, W, "nv12")
                with tr.row("output_to_yuv420-nv12-" + tag):
                    F.output_to_yuv420(y, "nv12", crop_to=crop, out=torch.zeros((T, n + 16), dtype=torch.uint8, device=DEV) if given else None,
                                       **YUV_KW, **dkw)
                for fmt in ("uyvy422", "yuv420p10le"):
                    n = F.yuv_frame_bytes(H, W, fmt)
                    with tr.row("output_to_yuv-%s-%s" % (fmt, tag)):
                        F.output_to_yuv(y, fmt, crop_to=crop, out=torch.zeros((T, n + 16), dtype=torch.uint8, device=DEV) if given else None,
                                        **YUV_KW, **dkw)
                n = F.rgb_frame_bytes(H, W, "rgba")
                for aname, a in (("opaque", None), ("alpha", alpha)):
                    with tr.row("output_to_rgb-rgba-%s-%s" % (aname, tag)):
                        F.output_to_rgb(y, "rgba", full_range=a is None, crop_to=crop, alpha=a,
                                        out=torch.zeros((T, n + 16), dtype=torch.uint8, device=DEV) if given else None, **dkw)
    with tr.row("output_to_yuv420-nv12-row_pitch"):
        F.output_to_yuv420(y, "nv12", row_pitch=32)
    with tr.row("output_to_yuv-yuv420p10le-pitches"):
        F.output_to_yuv(y, "yuv420p10le", pitches=(64, 32, 32), offsets=(16, 0, 0))
    with tr.row("output_to_rgb-rgba-pitches"):
        F.output_to_rgb(y, "rgba", pitches=(96,), offsets=(32,), dither="ordered")


def section_side(tr):
    """one call each of the estimate, vst, scene, blend and grain functions"""
    from bsvd_amd import frame_io as F
    x, y = _planes(4, NET, 21), _planes(3, NET, 22)
    with tr.row("estimate_sigma"):
        s = F.estimate_sigma(x, picture=PIC, gain=1.25, clamp=(0.01, 0.2))
    with tr.row("fill_sigma_plane"):
        F.fill_sigma_plane(x, s)
    with tr.row("estimate_noise_curve"):
        curve, hist = F.estimate_noise_curve(x, picture=PIC, gain=0.8, clamp=(0.01, 0.2), min_count=3, return_hist=True)
    with tr.row("noise_curve_from_hist"):
        F.noise_curve_from_hist(hist, gain=0.8, clamp=(0.01, 0.2), min_count=3)
    with tr.row("fill_noise_map"):
        F.fill_noise_map(x, curve)
    with tr.row("build_vst"):
        tables = F.build_vst(curve, floor=0.01)
    with tr.row("build_vst-curve-out"):
        shared = F.build_vst(F.NoiseCurve.from_model(2.0e-3, 1.0e-4), out=torch.empty((1, F.VST_TABLE_FLOATS), dtype=torch.float32, device=DEV))
    with tr.row("vst_forward"):
        F.vst_forward(x, tables)
    with tr.row("vst_forward-shared-no-plane"):
        F.vst_forward(x, shared, fill_plane=False)
    with tr.row("vst_inverse"):
        F.vst_inverse(y, tables)
    big = _planes(4, (32, 48), 23)
    with tr.row("scene_scores"):
        _, grid = F.scene_scores(big, picture=(30, 42))
    with tr.row("scene_scores-prev-out"):
        F.scene_scores(big, picture=(30, 42), prev=grid[0], out=(torch.empty(T, dtype=torch.int64, device=DEV), torch.empty_like(grid)))
    with tr.row("scene_scores-no-block"):
        F.scene_scores(x, picture=PIC)
    with tr.row("scene_cuts"):
        F.scene_cuts(big, threshold=5.0, picture=(30, 42))
    with tr.row("blend_output"):
        F.blend_output(y, x, (0.4, 1.0), matrix="bt601")
    with tr.row("grain_stats"):
        F.grain_stats(x, y, picture=PIC, matrix="bt2020")
    with tr.row("estimate_grain"):
        F.estimate_grain(x, y, picture=PIC)
    with tr.row("apply_grain"):
        F.apply_grain(y, F.GrainModel.from_values([0.02, 0.01, 0.015]), amount=0.75, seed=9, frame0=3, matrix="bt601")
    with tr.row("apply_grain-nothing"):
        F.apply_grain(y, F.GrainModel.from_values(0.0))


PIPE_SIZE, PIPE_FRAMES, PIPE_CLIPS = (16, 24), 20, (8, 7, 5)
FULL = dict(pix_fmt="bgra", pad="reflect", cuts="auto", vst="scene", strength=(0.5, 1), dither="random", grain="scene")


def _pipeline(tr, m, name, live, fmt, kw):
    from bsvd_amd.pipeline import ClipPipeline, LiveStream
    fr = BH.frames(fmt, PIPE_SIZE, PIPE_FRAMES, seed=0, dark_from=PIPE_FRAMES // 2)
    with tr.row(name):
        if live:
            pipe = LiveStream(m, **kw)
            outs = [r for r in (pipe.feed(f) for f in fr) if r is not None] + pipe.flush()
        else:
            clips = np.split(fr, np.cumsum(PIPE_CLIPS)[:-1])
            outs = [f for clip in ClipPipeline(m, **kw).run(clips) for f in clip]
    assert len(outs) == PIPE_FRAMES
    torch.cuda.synchronize()


SECTIONS = {
    "decode": lambda tr, m: section_decode(tr),
    "encode": lambda tr, m: section_encode(tr),
    "side": lambda tr, m: section_side(tr),
    "live-defaults": lambda tr, m: _pipeline(tr, m, "LiveStream", True, "rgb24", dict(sigma=SIGMA)),
    "live-full": lambda tr, m: _pipeline(tr, m, "LiveStream", True, "bgra", FULL),
    "clip-defaults": lambda tr, m: _pipeline(tr, m, "ClipPipeline", False, "rgb24", dict(sigma=SIGMA)),
    "clip-full": lambda tr, m: _pipeline(tr, m, "ClipPipeline", False, "bgra", FULL),
}


def _dump(golden):
    """one call per line: a diff of the file reads as a diff of the trace"""
    lines = []
    for section in sorted(golden):
        rows = ["  %s: [\n%s\n  ]" % (json.dumps(name), ",\n".join("   " + json.dumps(call) for call in calls))
                for name, calls in golden[section].items()]
        lines.append(" %s: {\n%s\n }" % (json.dumps(section), ",\n".join(rows)))
    return "{\n%s\n}\n" % ",\n".join(lines)


@pytest.mark.parametrize("section", sorted(SECTIONS))
def test_calls_reach_the_entry_points_of_the_golden_trace(model, monkeypatch, section):     # noqa: F811
    tr = _Trace(monkeypatch)
    SECTIONS[section](tr, model)
    torch.cuda.synchronize()
    got = json.loads(json.dumps(tr.rows))                   # as the file holds them: tuples are lists
    assert got and all(calls or name.endswith("-nothing") for name, calls in got.items()), "a row made no call"
    if WRITE:
        golden = json.load(open(WRITE)) if os.path.exists(WRITE) else {}
        golden[section] = got
        with open(WRITE, "w") as f:
            f.write(_dump(golden))
        return
    want = json.load(open(GOLDEN))[section]
    assert list(got) == list(want), ("rows", sorted(set(got) ^ set(want)))
    for name in want:
        assert [c[0] for c in got[name]] == [c[0] for c in want[name]], ("entry points of row %s" % name, [c[0] for c in got[name]],
                                                                         [c[0] for c in want[name]])
        for k, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, ("row %s, call %d" % (name, k), g, w)
    assert got == want
