"""The noise-level estimate (bsvd_sigma_workspace_bytes, bsvd_estimate_sigma, bsvd_fill_sigma_plane, frame_io.estimate_sigma, the
``sigma='auto'`` of the ``*_to_input`` functions and the pipelines): what needs no device -- the numpy model against the true sigma on seeded
synthetic scenes (bounds: profiles/sigma_auto.txt), the model's mutants against the model on the GPU tests' inputs, every validation answer
of the three entry points with its text, the argument checks of frame_io and pipeline, and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest

import sigma_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_header_s():
    from bsvd_amd import _lib
    src = open(os.path.join(ROOT, "bsvd_amd", "csrc", "frame_sigma_items.h")).read()
    k = float.fromhex(re.search(r"SIGMA_K\s*=\s*(0x[0-9a-f.]+p[-+]?\d+)", src).group(1))
    assert k == M.K == _lib.SIGMA_K == 1.0 / (4096 * 6 * 0.6744897501960817)
    assert int(re.search(r"SIGMA_BINS\s*=\s*(\d+)", src).group(1)) == M.BINS == _lib.SIGMA_BINS
    assert int(re.search(r"SIGMA_BAND\s*=\s*(\d+)", src).group(1)) == M.BAND
    assert _lib.SIGMA_MAX == M.SIGMA_MAX == pytest.approx(1 / (6 * 0.6744897501960817))


# the bounds of profiles/sigma_auto.txt, section 1, in code units (/255): measured on the model at 64 x 96 over 8 noise seeds per cell, then
# widened to a rule -- one histogram step (0.25) + 4 % of sigma, where the widest cell measured was 0.22 + 1.4 %
@pytest.mark.parametrize("kind", ["smooth", "mixed", "texture"])
def test_model_against_the_true_sigma(kind):
    clean = M.scene(kind, 64, 96, 0)
    for sigma in (2, 5, 10, 20, 30):
        for seed in range(3):
            est = float(M.estimate(M.to_f32(M.noisy_u8(clean, sigma, seed))[None])[0][0]) * 255
            print("%s sigma %g seed %d: %.3f" % (kind, sigma, seed, est))
            assert abs(est - sigma) <= 0.25 + 0.04 * sigma, (kind, sigma, seed, est)
    est0 = float(M.estimate(M.to_f32(M.noisy_u8(clean, 0, 0))[None])[0][0]) * 255
    print("%s clean: %.3f" % (kind, est0))
    assert est0 <= 0.75                                            # the scene's own response: 0.01 (smooth), 0.26 (mixed), 0.50 (texture) measured
    for seed in range(3):                                          # clipping at 0 / 255 pulls the estimate down: 47.9 .. 50.9 measured
        est = float(M.estimate(M.to_f32(M.noisy_u8(clean, 50, seed))[None])[0][0]) * 255
        print("%s sigma 50 seed %d: %.3f" % (kind, seed, est))
        assert 47.0 <= est <= 51.5, (kind, seed, est)


def test_model_steps_and_edge_cases():
    x = M.to_f32(M.noisy_u8(M.scene("smooth", 64, 96, 0), 10, 0))[None]
    s, h = M.estimate(x)
    assert h.sum() == 3 * 62 * 94
    assert float(M.estimate(x, gain=2.0)[0][0]) == pytest.approx(2 * float(s[0]), rel=1e-6)
    assert M.estimate(x, clamp=(0.2, 0.21))[0][0] == np.float32(0.2) and M.estimate(x, clamp=(0.0, 0.01))[0][0] == np.float32(0.01)
    assert M.finish(np.zeros((1, 4096), np.int64), lo=0.03)[0] == np.float32(0.03)          # N = 0 gives lo
    one = np.zeros((1, 4096), np.int64)
    one[0, 100] = 7
    assert M.finish(one)[0] == np.float32(100.5 * M.K)
    two = np.zeros((1, 4096), np.int64)
    two[0, 10], two[0, 20] = 5, 5                                  # 2 cum[10] = 10 >= N = 10: the median sits at the end of bin 10
    assert M.finish(two)[0] == np.float32(11.0 * M.K)
    bad = x.copy()
    bad[0, 1, 5, 5] = np.nan
    assert M.estimate(bad)[1].sum() == h.sum() - 9


CASES = M.gpu_cases()


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_differs_on_the_gpu_tests_inputs(mutant):
    """the inputs of tests/test_gpu_sigma.py can tell the model from: a mask without its corner taps, border pixels included, the pad
    region sampled, frames pooled into one histogram, the mean instead of the median"""
    differs = []
    for name, (x, picture) in CASES.items():
        s0, h0 = M.estimate(x, picture)
        s1, h1 = M.estimate(x, picture, mutant=mutant)
        if not (np.array_equal(h0, h1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))):
            differs.append(name)
    print(mutant, "differs on", differs)
    assert differs
    if mutant == "pad_sampled":
        assert "pad_finite_37x53_in_40x56" in differs and "pad_scalar_5x6_in_7x9" in differs
    if mutant == "frames_pooled":
        assert "five_frames" in differs and "shape_2x12x20" in differs


def test_gpu_cases_cover_the_shapes_and_contents():
    shapes = {(x.shape, p) for x, p in CASES.values()}
    assert ((1, 4, 3, 3), None) in shapes and ((1, 4, 4, 4), None) in shapes and ((2, 4, 12, 20), None) in shapes
    assert ((2, 4, 40, 56), (37, 53)) in shapes
    for H in (M.BAND - 1, M.BAND, M.BAND + 1, 2 * M.BAND + 1):
        assert "height_%d" % H in CASES and "height_%d" % (H + 2) in CASES       # rows in all, and interior rows
    assert all("width_%d" % W in CASES for W in (3, 5, 8, 67))
    x = CASES["pad_nan_37x53_in_40x56"][0]
    assert np.isnan(x[:, 3]).all() and np.isnan(x[:, :, 37:]).all() and np.isnan(x[:, :, :, 53:]).all() and np.isfinite(x[:, :3, :37, :53]).all()
    dy = CASES["dyadic"][0][:, :3]
    assert (dy * 2 ** 20 == np.round(dy * 2 ** 20)).all()
    r = np.abs(M.response(dy)) * 4096
    assert (r == np.floor(r)).mean() > 0.1 and (r != np.floor(r)).any()           # on the bin edges, and beside them
    assert np.isnan(CASES["nan_inf"][0]).any() and np.isposinf(CASES["nan_inf"][0]).any() and np.isneginf(CASES["nan_inf"][0]).any()


# ---- the entry points' validation, without a device ----------------------------------------------------------------------------------------
def _lib_loaded():
    from bsvd_amd import _lib
    return _lib.load()


def _estimate(lib, **kw):
    a = dict(x=64, frames=2, channels=3, H=12, W=20, Hp=12, Wp=20, frame_stride=4 * 12 * 20, gain=1.0, lo=0.0, hi=0.25, workspace=64, sigma_out=64)
    a.update(kw)
    rc = lib.bsvd_estimate_sigma(a["x"], a["frames"], a["channels"], a["H"], a["W"], a["Hp"], a["Wp"], a["frame_stride"], a["gain"], a["lo"],
                                 a["hi"], a["workspace"], a["sigma_out"], None)
    return rc, lib.bsvd_last_error().decode()


ESTIMATE_REFUSALS = [
    (dict(x=None), "x is NULL"), (dict(workspace=None), "workspace is NULL"), (dict(sigma_out=None), "sigma_out is NULL"),
    (dict(x=66), "x must be 4-byte aligned"), (dict(workspace=66), "4-byte aligned"), (dict(sigma_out=65), "4-byte aligned"),
    (dict(frames=0), "frames = 0"), (dict(frames=65536), "frames = 65536"), (dict(channels=0), "channels = 0"),
    (dict(H=2), "H = 2 must be at least 3"), (dict(W=2), "W = 2 must be at least 3"), (dict(Hp=11), "Hp = 11 is below H = 12"),
    (dict(Wp=19), "Wp = 19 is below W = 20"), (dict(frame_stride=3 * 12 * 20 - 1), "frame_stride = 719"),
    (dict(H=46343, W=46343, Hp=46343, Wp=46343, frame_stride=4 * 46343 * 46343), "2^32 samples or more"),
    (dict(gain=0.0), "gain = 0"), (dict(gain=-1.0), "gain = -1"), (dict(gain=float("nan")), "gain = nan"), (dict(gain=float("inf")), "gain = inf"),
    (dict(lo=-0.1), "clamp [lo, hi]"), (dict(lo=0.3), "clamp [lo, hi]"), (dict(hi=float("inf")), "clamp [lo, hi]"), (dict(lo=float("nan")), "clamp [lo, hi]"),
]


@pytest.mark.parametrize("kw,text", ESTIMATE_REFUSALS, ids=[t for _, t in ESTIMATE_REFUSALS])
def test_estimate_sigma_refusals(kw, text):
    rc, msg = _estimate(_lib_loaded(), **kw)
    assert rc == -3 and msg.startswith("bsvd_estimate_sigma: ") and text in msg, (rc, msg)


FILL_REFUSALS = [
    (dict(x=None), "x is NULL"), (dict(sigma_dev=None), "sigma_dev is NULL"), (dict(x=66), "x must be 4-byte aligned"),
    (dict(sigma_dev=66), "sigma_dev must be 4-byte aligned"), (dict(frames=0), "frames = 0"), (dict(channels=0), "channels = 0"),
    (dict(Hp=0), "Hp = 0"), (dict(Wp=-4), "Wp = -4"), (dict(frame_stride=4 * 12 * 20 - 1), "frame_stride = 959"),
]


@pytest.mark.parametrize("kw,text", FILL_REFUSALS, ids=[t for _, t in FILL_REFUSALS])
def test_fill_sigma_plane_refusals(kw, text):
    lib = _lib_loaded()
    a = dict(x=64, frames=2, channels=3, Hp=12, Wp=20, frame_stride=4 * 12 * 20, sigma_dev=64)
    a.update(kw)
    rc = lib.bsvd_fill_sigma_plane(a["x"], a["frames"], a["channels"], a["Hp"], a["Wp"], a["frame_stride"], a["sigma_dev"], None)
    msg = lib.bsvd_last_error().decode()
    assert rc == -3 and msg.startswith("bsvd_fill_sigma_plane: ") and text in msg, (rc, msg)


def test_workspace_bytes_and_binding():
    from bsvd_amd import _lib
    lib = _lib_loaded()
    assert lib.bsvd_sigma_workspace_bytes(1) == 16384 and lib.bsvd_sigma_workspace_bytes(33) == 33 * 16384
    assert lib.bsvd_sigma_workspace_bytes(0) == -1 and lib.bsvd_sigma_workspace_bytes(-5) == -1
    assert {"bsvd_sigma_workspace_bytes", "bsvd_estimate_sigma", "bsvd_fill_sigma_plane"} <= set(_lib.EXPORTS)
    assert lib.bsvd_abi_version() == 12 and _lib.ABI_VERSION == 12                 # additive: found by symbol


# ---- frame_io / pipeline argument checks, without a device ---------------------------------------------------------------------------------
def test_sigma_argument_forms():
    import torch
    from bsvd_amd import frame_io as F
    assert F._sigma_mode(None) == ("const", None) and F._sigma_mode(0.1) == ("const", 0.1) and F._sigma_mode(np.float32(0.5)) == ("const", 0.5)
    assert F._sigma_mode("auto") == ("auto", None)
    assert F._sigma_mode([0.1, 0.2], 2) == ("host", [0.1, 0.2]) and F._sigma_mode(np.array([0.25, 0.5]), 2) == ("host", [0.25, 0.5])
    assert F._sigma_mode(torch.tensor([0.25, 0.5]), 2) == ("host", [0.25, 0.5])
    for bad in ("Auto", "estimate", ""):
        with pytest.raises(ValueError, match="'auto'"):
            F._sigma_mode(bad)
    for wrong in ([0.1, 0.2, 0.3], np.zeros(1), torch.zeros(5)):                   # wrong [T] length
        with pytest.raises(ValueError, match="per-frame values for 2 frames"):
            F._sigma_mode(wrong, 2)
    with pytest.raises(ValueError, match="float32"):
        F._sigma_mode(torch.zeros(2, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="float32"):
        F._sigma_mode(torch.zeros(2, 1), 2)
    with pytest.raises(ValueError, match="numbers"):
        F._sigma_mode(["a", "b"], 2)


@pytest.mark.parametrize("clamp", [(0.1, 0.05), (-0.1, 0.2), (0.0, float("inf")), (float("nan"), 0.1), 0.1, (0.1,), ("a", "b")])
def test_bad_clamp_is_refused_before_anything_else(clamp):
    from bsvd_amd.frame_io import estimate_sigma
    with pytest.raises(ValueError, match="clamp"):
        estimate_sigma(None, clamp=clamp)


@pytest.mark.parametrize("gain", [0, -1.0, float("inf"), float("nan"), "x"])
def test_bad_gain_is_refused(gain):
    from bsvd_amd.frame_io import estimate_sigma
    with pytest.raises(ValueError, match="sigma_gain"):
        estimate_sigma(None, gain=gain)


def test_estimate_sigma_refuses_what_is_no_device_tensor():
    import torch
    from bsvd_amd.frame_io import estimate_sigma, fill_sigma_plane
    for x in (None, torch.zeros(1, 4, 8, 8), torch.zeros(4, 8, 8)):
        with pytest.raises(ValueError, match="float32 device tensor"):
            estimate_sigma(x)
        with pytest.raises(ValueError, match="float32 device tensor"):
            fill_sigma_plane(x, torch.zeros(1))


class _Net:
    def __init__(self, c):
        self.net_in_ch = c


class _FakeModel:
    """what the constructors look at before they touch a device"""

    def __init__(self, c):
        self.net = _Net(c)

    def _device(self):
        raise AssertionError("the sigma check comes before the device")


@pytest.mark.parametrize("which", ["ClipPipeline", "LiveStream"])
def test_auto_with_a_blind_model_is_refused_at_construction(which):
    from bsvd_amd import pipeline
    cls = getattr(pipeline, which)
    with pytest.raises(ValueError, match="blind"):
        cls(_FakeModel(3), sigma="auto")
    with pytest.raises(ValueError, match="'auto'"):
        cls(_FakeModel(4), sigma="automatic")
    with pytest.raises(ValueError, match="sigma_gain"):
        cls(_FakeModel(4), sigma="auto", sigma_gain=0.0)
    with pytest.raises(ValueError, match="per-frame"):
        cls(_FakeModel(4), sigma=[0.1, 0.2])
    with pytest.raises(AssertionError, match="before the device"):           # a non-blind model passes the check and goes on
        cls(_FakeModel(4), sigma="auto", sigma_gain=1.5)


def test_tools_parse_sigma_auto():
    import importlib.util
    spec = importlib.util.spec_from_file_location("yuv_denoise", os.path.join(ROOT, "tools", "yuv_denoise.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_sigma("auto") == "auto" and mod.parse_sigma("30") == pytest.approx(30 / 255.0)
    with pytest.raises(Exception):
        mod.parse_sigma("car")
