"""The noise-level function (bsvd_nlf_workspace_bytes, bsvd_estimate_nlf, bsvd_finish_nlf, bsvd_fill_nlf_plane, frame_io.estimate_noise_curve /
fill_noise_map / NoiseCurve, ``sigma='nlf'`` of the ``*_to_input`` functions and the pipelines): what needs no device -- the numpy model's
internals, its mutants against it on the GPU tests' inputs, the model against the true curve on seeded synthetic signal-dependent noise
(bounds: profiles/noise_curve.txt), every validation answer of the entry points with its text, the argument checks of frame_io and pipeline."""
import os
import re

import numpy as np
import pytest

import nlf_model as M
import sigma_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = M.gpu_cases()
CURVES = M.curve_cases()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_constants_are_the_header_s():
    from bsvd_amd import _lib
    src = open(os.path.join(ROOT, "bsvd_amd", "csrc", "frame_nlf_items.h")).read()
    k = float.fromhex(re.search(r"NLF_K\s*=\s*(0x[0-9a-f.]+p[-+]?\d+)", src).group(1))
    assert k == M.K == _lib.NLF_K == 1.0 / (1024 * 6 * 0.6744897501960817) == 4 * S.K
    assert int(re.search(r"NLF_LEVELS\s*=\s*(\d+)", src).group(1)) == M.LEVELS == _lib.NLF_LEVELS == 16
    assert int(re.search(r"NLF_BINS\s*=\s*(\d+)", src).group(1)) == M.BINS == _lib.NLF_BINS == 1024
    assert M.MIN_COUNT == _lib.NLF_MIN_COUNT == 512 and M.SIGMA_MAX == S.SIGMA_MAX


# ---- model internals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_level_summed_histogram_is_the_scalar_estimate_s_in_fours(name):
    """both count the same samples, and floor(|r| * 1024) = floor(|r| * 4096) >> 2 up to the shared saturation"""
    x, picture = CASES[name]
    h = M.histogram(x, picture)
    assert h.shape == (x.shape[0], 16, 1024)
    assert np.array_equal(h.sum(1), S.histogram(x, picture).reshape(x.shape[0], 1024, 4).sum(2))


def test_model_steps_and_edge_cases():
    x, _ = CASES["flat"]
    h = M.histogram(x)
    assert h[0, 8, 0] == 3 * 22 * 38 and h.sum() == 3 * 22 * 38                    # box sum 4.5 -> level 8; r = 0 -> bin 0
    x, _ = CASES["checkerboard"]
    h = M.histogram(x)
    assert h[0, 7, 1023] + h[0, 8, 1023] == 3 * 22 * 38 and h[0, 7, 1023] > 0 and h[0, 8, 1023] > 0      # two levels, |r| = 4: the last bin
    assert M.levels_of(np.float32([np.inf, -np.inf, np.nan, -0.1, 0.0, 9.0, 100.0, 4.5])).tolist() == [15, 0, 0, 0, 0, 15, 15, 8]
    x, _ = CASES["nan_inf"]
    assert (M.histogram(x).sum((1, 2)) < 3 * 22 * 38).all()
    c, _ = M.estimate(x)
    assert np.isfinite(M.noise_map(x, c)).all()                                   # finite whatever the colour planes hold
    flat = np.full((x.shape[0], 16), 0.0421, np.float32)
    assert np.array_equal(_bits(M.noise_map(x, flat)), np.full((2, 24, 40), _bits(np.float32(0.0421))))
    x, _ = CASES["out_of_range"]
    assert (x[:, :3] < 0).any() and (x[:, :3] > 1).any()
    m = M.noise_map(x, M.estimate(x)[0])
    assert np.isfinite(m).all()


def test_curve_rules_of_the_model():
    h, kw = CURVES["min_count_boundary"]
    c = M.curve(h, **kw)[0]
    assert c[3] == np.float32(10.5 * M.K) and c[4] == c[3] and (c == c[3]).all()   # 99 < 100: level 4 is filled, level 3 alone is valid
    assert M.curve(h, min_count=99)[0][4] == np.float32(50.5 * M.K)
    h, kw = CURVES["tie_to_the_lower_level"]
    c = M.curve(h, **kw)[0]
    lo, hi = np.float32(20.5 * M.K), np.float32(80.5 * M.K)
    assert c.tolist() == [lo] * 5 + [hi] * 11
    h, kw = CURVES["no_valid_level_pooled"]
    c = M.curve(h, **kw)[0]
    assert (c == c[0]).all() and c[0] == M._value(h[0].sum(0), 1.0, 0.0, M.SIGMA_MAX)[0] and np.float32(30 * M.K) <= c[0] <= np.float32(31 * M.K)
    h, kw = CURVES["empty_gives_lo"]
    assert (M.curve(h, **kw)[0] == np.float32(0.0125)).all()
    h, kw = CURVES["gain_and_clamp"]
    c = M.curve(h, **kw)[0]
    assert c[2] == np.float32(max(20.5 * M.K * float(np.float32(1.37)), float(np.float32(0.01)))) and c[10] == np.float32(0.05)


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------
def _results(mutant):
    """everything the GPU tests compare with the device, under a mutant: histogram, curve and map of every case; curve of every hand-built histogram"""
    out = {}
    for name, (x, picture) in CASES.items():
        c, h = M.estimate(x, picture, mutant=mutant)
        out[name] = (h, _bits(c), _bits(M.noise_map(x, c, mutant=mutant)))
    for name, (h, kw) in CURVES.items():
        out["curve " + name] = (_bits(M.curve(h, mutant=mutant, **kw)),)
    return out


@pytest.fixture(scope="module")
def baseline():
    return _results(None)


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_differs_on_the_gpu_tests_inputs(baseline, mutant):
    """the inputs of tests/test_gpu_nlf.py can tell the model from: the centre pixel instead of the box, the level off by one, `>` for `>=` in
    the validity test, the tie to the higher level, the interpolation anchored at level edges, a contracted multiply-add in the interpolation"""
    got = _results(mutant)
    differs = [name for name in baseline if not all(np.array_equal(a, b) for a, b in zip(baseline[name], got[name]))]
    print(mutant, "differs on", differs)
    assert differs
    want = {"centre_pixel": "noisy_1x64x96", "level_off_by_one": "flat", "valid_gt": "curve min_count_boundary", "tie_high": "curve tie_to_the_lower_level",
            "lerp_edges": "noisy_5x64x96", "fma": "noisy_5x64x96"}[mutant]
    assert want in differs


# ---- accuracy against known truth ------------------------------------------------------------------------------------------------------------
# profiles/noise_curve.txt, section 1: the worst |curve - truth| in 8-bit code units measured on this model at 96 x 128 over seeds 0 .. 9, for
# the levels whose centre +- 3 sigma stays inside [0, 1]; the assertion is twice that
WORST = {"ramp": 1.634, "blocks": 1.838}


@pytest.mark.parametrize("kind", ["ramp", "blocks"])
def test_model_against_the_true_curve(kind):
    scored = M.scored_levels()
    assert scored.tolist() == list(range(1, 13))
    truth = M.true_curve()
    worst = 0.0
    for seed in range(10):
        x = S.to_f32(M.poisson_gauss_u8(M.nlf_scene(kind, 96, 128, seed), 1000 + seed))[None]
        c, valid = M.curve(M.histogram(x), return_valid=True)
        if kind == "ramp":
            assert valid.all(), (seed, valid)                                     # all sixteen levels valid on the ramp
        assert valid[0][scored].all()
        dev = np.abs(c[0].astype(np.float64) - truth)[scored] * 255
        print("%s seed %d: worst %.3f at level %d" % (kind, seed, dev.max(), scored[dev.argmax()]))
        worst = max(worst, dev.max())
    print("%s: worst deviation %.3f / 255 (recorded %.3f)" % (kind, worst, WORST[kind]))
    assert worst <= 2 * WORST[kind]


# the same record, section 2: worst |level value - the scalar estimate| of the same frame over the valid levels, seeds 0 .. 9, 96 x 128
AWGN_WORST = {("smooth", 10): 0.943, ("smooth", 25): 2.217, ("mixed", 10): 1.201, ("mixed", 25): 2.951}


@pytest.mark.parametrize("kind,sigma", sorted(AWGN_WORST))
def test_on_uniform_noise_every_valid_level_agrees_with_the_scalar_estimate(kind, sigma):
    worst = 0.0
    for seed in range(10):
        x = S.to_f32(S.noisy_u8(S.scene(kind, 96, 128, 0), sigma, seed))[None]
        c, valid = M.curve(M.histogram(x), return_valid=True)
        assert valid.sum() >= 8
        scalar = float(S.estimate(x)[0][0])
        worst = max(worst, float(np.abs(c[0][valid[0]].astype(np.float64) - scalar).max() * 255))
    print("%s sigma %d: worst |level - scalar| %.3f / 255 (recorded %.3f)" % (kind, sigma, worst, AWGN_WORST[(kind, sigma)]))
    assert worst <= 2 * AWGN_WORST[(kind, sigma)]


# ---- the entry points' validation, without a device ------------------------------------------------------------------------------------------
def _lib_loaded():
    from bsvd_amd import _lib
    return _lib.load()


def _estimate(lib, **kw):
    a = dict(x=64, frames=2, H=12, W=20, Hp=12, Wp=20, frame_stride=4 * 12 * 20, gain=1.0, lo=0.0, hi=0.25, min_count=512, workspace=64, curve_out=64)
    a.update(kw)
    rc = lib.bsvd_estimate_nlf(a["x"], a["frames"], a["H"], a["W"], a["Hp"], a["Wp"], a["frame_stride"], a["gain"], a["lo"], a["hi"], a["min_count"],
                               a["workspace"], a["curve_out"], None)
    return rc, lib.bsvd_last_error().decode()


ESTIMATE_REFUSALS = [
    (dict(x=None), "x is NULL"), (dict(workspace=None), "workspace is NULL"), (dict(curve_out=None), "curve_out is NULL"),
    (dict(x=66), "x must be 4-byte aligned"), (dict(workspace=66), "4-byte aligned"), (dict(curve_out=65), "4-byte aligned"),
    (dict(frames=0), "frames = 0"), (dict(frames=65536), "frames = 65536"),
    (dict(H=2), "H = 2 must be at least 3"), (dict(W=2), "W = 2 must be at least 3"), (dict(Hp=11), "Hp = 11 is below H = 12"),
    (dict(Wp=19), "Wp = 19 is below W = 20"), (dict(frame_stride=3 * 12 * 20 - 1), "frame_stride = 719"),
    (dict(H=46343, W=46343, Hp=46343, Wp=46343, frame_stride=4 * 46343 * 46343), "2^32 samples or more"),
    (dict(gain=0.0), "gain = 0"), (dict(gain=-1.0), "gain = -1"), (dict(gain=float("nan")), "gain = nan"), (dict(gain=float("inf")), "gain = inf"),
    (dict(lo=-0.1), "clamp [lo, hi]"), (dict(lo=0.3), "clamp [lo, hi]"), (dict(hi=float("inf")), "clamp [lo, hi]"), (dict(lo=float("nan")), "clamp [lo, hi]"),
    (dict(min_count=0), "min_count = 0"), (dict(min_count=-7), "min_count = -7"),
]


@pytest.mark.parametrize("kw,text", ESTIMATE_REFUSALS, ids=[t for _, t in ESTIMATE_REFUSALS])
def test_estimate_nlf_refusals(kw, text):
    rc, msg = _estimate(_lib_loaded(), **kw)
    assert rc == -3 and msg.startswith("bsvd_estimate_nlf: ") and text in msg, (rc, msg)


FINISH_REFUSALS = [
    (dict(workspace=None), "workspace is NULL"), (dict(curve_out=None), "curve_out is NULL"), (dict(workspace=66), "4-byte aligned"),
    (dict(frames=0), "frames = 0"), (dict(frames=65536), "frames = 65536"), (dict(gain=0.0), "gain = 0"), (dict(lo=0.3), "clamp [lo, hi]"),
    (dict(min_count=0), "min_count = 0"),
]


@pytest.mark.parametrize("kw,text", FINISH_REFUSALS, ids=[t for _, t in FINISH_REFUSALS])
def test_finish_nlf_refusals(kw, text):
    lib = _lib_loaded()
    a = dict(workspace=64, frames=2, gain=1.0, lo=0.0, hi=0.25, min_count=512, curve_out=64)
    a.update(kw)
    rc = lib.bsvd_finish_nlf(a["workspace"], a["frames"], a["gain"], a["lo"], a["hi"], a["min_count"], a["curve_out"], None)
    msg = lib.bsvd_last_error().decode()
    assert rc == -3 and msg.startswith("bsvd_finish_nlf: ") and text in msg, (rc, msg)


FILL_REFUSALS = [
    (dict(x=None), "x is NULL"), (dict(curve_dev=None), "curve_dev is NULL"), (dict(x=66), "x must be 4-byte aligned"),
    (dict(curve_dev=66), "curve_dev must be 4-byte aligned"), (dict(frames=0), "frames = 0"), (dict(frames=65536), "frames = 65536"),
    (dict(channels=2), "channels = 2 must be at least 3"), (dict(Hp=0), "Hp = 0"), (dict(Wp=-4), "Wp = -4"),
    (dict(frame_stride=4 * 12 * 20 - 1), "frame_stride = 959"),
]


@pytest.mark.parametrize("kw,text", FILL_REFUSALS, ids=[t for _, t in FILL_REFUSALS])
def test_fill_nlf_plane_refusals(kw, text):
    lib = _lib_loaded()
    a = dict(x=64, frames=2, channels=3, Hp=12, Wp=20, frame_stride=4 * 12 * 20, curve_dev=64)
    a.update(kw)
    rc = lib.bsvd_fill_nlf_plane(a["x"], a["frames"], a["channels"], a["Hp"], a["Wp"], a["frame_stride"], a["curve_dev"], None)
    msg = lib.bsvd_last_error().decode()
    assert rc == -3 and msg.startswith("bsvd_fill_nlf_plane: ") and text in msg, (rc, msg)


def test_workspace_bytes_and_binding():
    from bsvd_amd import _lib
    lib = _lib_loaded()
    assert lib.bsvd_nlf_workspace_bytes(1) == 65536 and lib.bsvd_nlf_workspace_bytes(33) == 33 * 65536
    assert lib.bsvd_nlf_workspace_bytes(0) == -1 and lib.bsvd_nlf_workspace_bytes(-5) == -1
    assert {"bsvd_nlf_workspace_bytes", "bsvd_estimate_nlf", "bsvd_finish_nlf", "bsvd_fill_nlf_plane"} <= set(_lib.EXPORTS)
    assert lib.bsvd_abi_version() == 12 and _lib.ABI_VERSION == 12                 # additive: found by symbol


# ---- frame_io / pipeline argument checks, without a device -----------------------------------------------------------------------------------
def test_sigma_argument_forms():
    from bsvd_amd import frame_io as F
    assert F._sigma_mode("nlf") == ("nlf", None)
    c = F.NoiseCurve([0.01 * (i + 1) for i in range(16)])
    kind, vals = F._sigma_mode(c, 5)
    assert kind == "curve" and vals == list(c.values) and len(vals) == 16
    assert F._sigma_mode("auto") == ("auto", None) and F._sigma_mode(None) == ("const", None) and F._sigma_mode(0.1) == ("const", 0.1)
    for bad in ("NLF", "curve", "nlf "):
        with pytest.raises(ValueError, match="'nlf'"):
            F._sigma_mode(bad)


def test_noise_curve_validation_and_from_model():
    from bsvd_amd.frame_io import NoiseCurve
    c = NoiseCurve(np.linspace(0.01, 0.1, 16))
    assert len(c.values) == 16 and all(isinstance(v, float) for v in c.values) and c == NoiseCurve(c.values) and "NoiseCurve" in repr(c)
    for bad in ([0.1] * 15, [0.1] * 17, [0.1] * 15 + [-0.01], [0.1] * 15 + [float("nan")], [0.1] * 15 + [float("inf")], ["a"] * 16, 0.1, None):
        with pytest.raises(ValueError, match="NoiseCurve"):
            NoiseCurve(bad)
    m = NoiseCurve.from_model(M.A, M.B)
    assert np.allclose(m.values, M.true_curve(), rtol=1e-12, atol=0)
    assert m.values[0] == pytest.approx(((20 / 255) ** 2 / 32 + (5 / 255) ** 2) ** 0.5)
    assert NoiseCurve.from_model(0.0, 0.04).values == (0.2,) * 16                  # no signal dependence: a flat curve
    assert NoiseCurve.from_model(1.0, -0.5).values[:8] == (0.0,) * 8               # max(a I + b, 0)
    with pytest.raises(ValueError, match="from_model"):
        NoiseCurve.from_model("a", 0.1)
    with pytest.raises(ValueError, match="NoiseCurve"):
        NoiseCurve.from_model(float("inf"), 0.1)


@pytest.mark.parametrize("min_count", [0, -1, 1.5, "x", None, 2 ** 31])
def test_bad_min_count_is_refused(min_count):
    from bsvd_amd.frame_io import estimate_noise_curve
    with pytest.raises(ValueError, match="min_count"):
        estimate_noise_curve(None, min_count=min_count)


def test_bad_clamp_and_gain_are_refused_before_anything_else():
    from bsvd_amd.frame_io import estimate_noise_curve, noise_curve_from_hist
    for fn in (estimate_noise_curve, noise_curve_from_hist):
        with pytest.raises(ValueError, match="clamp"):
            fn(None, clamp=(0.1, 0.05))
        with pytest.raises(ValueError, match="sigma_gain"):
            fn(None, gain=0)


def test_entry_functions_refuse_what_is_no_device_tensor():
    import torch
    from bsvd_amd.frame_io import estimate_noise_curve, fill_noise_map, noise_curve_from_hist
    for x in (None, torch.zeros(1, 4, 8, 8), torch.zeros(4, 8, 8)):
        with pytest.raises(ValueError, match="float32 device tensor"):
            estimate_noise_curve(x)
        with pytest.raises(ValueError, match="float32 device tensor"):
            fill_noise_map(x, torch.zeros(1, 16))
    with pytest.raises(ValueError, match="uint32 device tensor"):
        noise_curve_from_hist(torch.zeros(1, 16, 1024, dtype=torch.int32))


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
def test_nlf_with_a_blind_model_is_refused_at_construction(which):
    from bsvd_amd import pipeline
    from bsvd_amd.frame_io import NoiseCurve
    cls = getattr(pipeline, which)
    with pytest.raises(ValueError, match="blind"):
        cls(_FakeModel(3), sigma="nlf")
    with pytest.raises(ValueError, match="blind"):
        cls(_FakeModel(3), sigma=NoiseCurve([0.1] * 16))
    with pytest.raises(ValueError, match="'nlf'"):
        cls(_FakeModel(4), sigma="nlf2")
    with pytest.raises(ValueError, match="sigma_gain"):
        cls(_FakeModel(4), sigma="nlf", sigma_gain=0.0)
    for sigma in ("nlf", NoiseCurve([0.1] * 16)):
        with pytest.raises(AssertionError, match="before the device"):       # a non-blind model passes the check and goes on
            cls(_FakeModel(4), sigma=sigma, sigma_gain=1.5)


def test_tools_parse_sigma_nlf_and_noise_model():
    import importlib.util
    spec = importlib.util.spec_from_file_location("yuv_denoise", os.path.join(ROOT, "tools", "yuv_denoise.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_sigma("nlf") == "nlf" and mod.parse_sigma("auto") == "auto" and mod.parse_sigma("30") == pytest.approx(30 / 255.0)
    c = mod.parse_noise_model("1.5686,25")                                       # A = 400 / 255, B = 25: the model of the accuracy tests
    assert np.allclose(c.values, M.true_curve(), rtol=1e-4)
    for bad in ("1", "a,b", "1,2,3"):
        with pytest.raises(Exception):
            mod.parse_noise_model(bad)
