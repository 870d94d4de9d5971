"""tests/launch_shapes.py without a device: every case chosen for the GPU tests at capped grids qualifies under the restated launch rules and
stays inside its memory limit, the case table is complete, the small-shape GPU files are single-trip under the same restatement (the gap
the new file closes), the chunks of the launch-shape-independence check are single-trip, and the models themselves do not depend on how the
frames are chunked -- so that a difference between one call and its chunks on the device points at the kernel."""
import collections

import numpy as np
import pytest

import finish_model as F
import launch_shapes as L
import nlf_model as NM
import rgb_surface_model as R
import scene_model as SC
import sigma_model as SM
import vst_model as VM
import yuv_pad_model as P
import yuv_surface_model as S


def test_the_issue_numbers_follow_from_the_restatement():
    """the shipped geometries: trips of one 2160 x 3840 frame and of the headline clip's sigma estimate"""
    assert L.rule_u8_pad(1, 2160, 3840).items == 2073600 and 1 < L.trips(L.rule_u8_pad(1, 2160, 3840)) <= 2
    assert L.per_trip(L.rule_vst(1, 2160, 3840)) == 524288 and 3 < L.trips(L.rule_vst(1, 2160, 3840)) <= 4
    assert L.rule_sigma_hist(1, 2160, 3840).items == 777600 and L.per_trip(L.rule_sigma_hist(1, 2160, 3840)) == 262144
    l = L.rule_sigma_hist(10, 540, 960)
    assert (l.items, L.per_trip(l)) == (48960, 26112) and L.tail(l) % L.WAVE == 0 and L.tail(l) == 22848
    assert L.per_trip(L.rule_sigma_hist(257, 540, 960)) == 512
    assert L.per_trip(L.rule_scene_diff(32400)) == 16384


@pytest.mark.parametrize("c", L.SWEEP_CASES, ids=lambda c: c.id)
def test_sweep_case_qualifies(c):
    l = L.case_rule(c)
    assert L.trips(l) >= L.TRIPS_MIN and L.tail(l) % L.WAVE != 0 and L.cap_binds(l)
    assert not any(L.qualifies(L.case_rule(c, t)) for t in range(max(c.T - 16, 1), c.T)), "not the smallest frame count that qualifies"
    assert L.trips(l) < L.TRIPS_MIN + max(0.1, L.case_rule(c, 1).items / L.per_trip(l)), "more than a frame above the margin"
    assert max(L.case_bytes(c).values()) < L.GIB
    parts = L.chunks(lambda T: L.case_rule(c, T), c.T)
    assert parts[0][0] == 0 and parts[-1][1] == c.T and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    assert len(parts) >= 3 and all(L.cap_fraction(L.case_rule(c, hi - lo)) <= L.CHUNK_TRIPS for lo, hi in parts)


def test_the_sweep_table_is_complete():
    """one case per format and direction; every option value in at least two cases; both families in every translation unit"""
    ids = collections.Counter((c.entry, c.fmt, c.hwc) for c in L.SWEEP_CASES)
    assert set(ids.values()) == {1}
    for entry in ("yuv_in", "yuv_out"):
        assert sorted(c.fmt for c in L.SWEEP_CASES if c.entry == entry) == sorted(L.YUV_NAMES)
        assert set(L.YUV_NAMES) == set(S.FORMATS) | {"nv12", "p010"}
    for entry in ("rgb_in", "rgb_out"):
        assert sorted(c.fmt for c in L.SWEEP_CASES if c.entry == entry) == sorted(R.FORMATS)
    for entry in ("u8_in", "u8_out"):
        assert sorted((c.pad, c.hwc) for c in L.SWEEP_CASES if c.entry == entry) == [(False, False), (False, True), (True, False), (True, True)]
    yuv = [c for c in L.SWEEP_CASES if c.unit == "frame_yuv"]
    enc = [c for c in L.SWEEP_CASES if c.entry in ("yuv_out", "rgb_out")]
    surf = [c for c in L.SWEEP_CASES if c.unit in ("frame_yuv", "frame_rgb")]

    def at_least_twice(cases, field, values):
        n = collections.Counter(getattr(c, field) for c in cases)
        assert all(n[v] >= 2 for v in values), (field, n)
    at_least_twice(yuv, "chroma", L.CHROMAS)
    at_least_twice(yuv, "matrix", [m for m, _ in L.COLOURS])
    at_least_twice(surf, "full_range", [False, True])
    at_least_twice(surf, "pitched", [False, True])
    at_least_twice(L.SWEEP_CASES, "pad", [False, True])
    at_least_twice(enc, "dither", L.DITHERS)
    at_least_twice([c for c in L.SWEEP_CASES if c.entry == "yuv_out"], "dither", L.DITHERS)
    at_least_twice([c for c in L.SWEEP_CASES if c.entry == "rgb_out"], "dither", L.DITHERS)
    blends = [c.strength for c in L.SWEEP_CASES if c.entry == "blend"]
    assert (1.0, 1.0) in blends and (0.0, 0.0) in blends and sum(0 < s[0] < 1 and 0 < s[1] < 1 for s in blends) >= 2
    for unit in ("tensor_layout", "frame_yuv", "frame_rgb", "frame_finish"):
        assert {c.family for c in L.SWEEP_CASES if c.unit == unit} == set(L.FAMILIES), unit


@pytest.mark.parametrize("fc", L.FRAME_CASES, ids=lambda fc: fc.id)
def test_frame_case_is_what_its_regime_says(fc):
    l = L.frame_rule(fc)
    assert max(L.frame_bytes_of(fc).values()) < L.GIB
    if fc.regime == "collapsed" and fc.kernel != "scene":
        assert l.cap == 1 and L.qualifies(l) and L.trips(l) < L.TRIPS_MIN + 0.1
        assert fc.Hp != fc.Wp
        groups = (fc.W + 2) >> 2 if "hist" in fc.kernel else -(-fc.Wp // 4)
        assert groups % 64 not in (0, 1, 63)
        parts = L.chunks(lambda T: L.frame_rule(fc, T), fc.T)
        assert len(parts) >= 3 and all(L.cap_fraction(L.frame_rule(fc, hi - lo)) <= L.CHUNK_TRIPS for lo, hi in parts)
    parts = L.chunks(lambda T: L.frame_rule(fc, T), fc.T)                # every regime: at least three calls, none of them the whole
    assert len(parts) >= 3 and parts[0][0] == 0 and parts[-1][1] == fc.T and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    assert all(L.cap_fraction(L.frame_rule(fc, hi - lo)) <= L.CHUNK_TRIPS for lo, hi in parts)
    if fc.kernel == "scene":
        # the grid kernel has no loop: its cases are about blockIdx.y up to 65535 frames and 240-block rows; their diff launch is a single
        # trip, so the capped sweep of bsvd_scene_diff is what SCENE_DIFF_BLOCKS is for (test_gpu_launch_shapes.py runs those on the device)
        d = L.rule_scene_diff(l.items)
        assert l.cap is None and L.workgroups(l) == -(-l.items // 4) and L.single_trip(d) and not L.cap_binds(d)
        assert any(L.qualifies(L.rule_scene_diff(b)) for b in L.SCENE_DIFF_BLOCKS)
    if fc.regime == "headline":
        assert (fc.T, fc.H, fc.W) == (10, 540, 960)
        if fc.kernel in ("sigma_hist", "nlf_hist", "vst_forward", "vst_inverse", "fill_sigma"):
            assert L.trips(l) > 1 and L.cap_binds(l)                   # the shipped launch is already multi-trip
    if fc.regime == "max_frames":
        assert fc.T == (L.HIST_MAX_FRAMES if "hist" in fc.kernel else L.MAX_FRAMES) and (l.cap in (1, None))


def test_the_frame_table_is_complete_and_the_histogram_workspaces_are_why_4096():
    kernels = {"sigma_hist", "nlf_hist", "fill_sigma", "nlf_map", "vst_forward", "vst_inverse", "scene"}
    for regime in ("headline", "collapsed", "max_frames"):
        assert {fc.kernel for fc in L.FRAME_CASES if fc.regime == regime} == kernels
    assert any(fc.kernel == "scene" and fc.W // 16 == 240 for fc in L.FRAME_CASES)
    assert L.MAX_FRAMES * SM.BINS * 4 >= L.GIB - 4 * SM.BINS and L.MAX_FRAMES * NM.LEVELS * NM.BINS * 4 > 3.9 * L.GIB
    big = L.rule_scene_diff(L.SCENE_DIFF_BLOCKS[-1])
    assert L.qualifies(big) and L.trips(L.rule_scene_diff(16384)) == 1.0 and L.tail(L.rule_scene_diff(16385)) == 1


def test_the_small_shape_files_are_single_trip():
    """the gap: under the same restatement, the largest shapes of the existing GPU files (5 frames of 64 x 96, and their own case lists)
    run every loop once -- pinned, so that it shows if someone later shrinks the new shapes to these"""
    T, H, W = 5, 64, 96
    rules = [L.rule_u8_to_planar(T, H, W, cc=1), L.rule_planar_to_u8(T, H, W), L.rule_u8_pad(T, H, W), L.rule_yuv(T, H, W, 444), L.rule_rgb(T, H, W),
             L.rule_blend(T, H, W), L.rule_sigma_hist(T, H, W), L.rule_fill_sigma(T, H, W), L.rule_nlf_map(T, H, W), L.rule_vst(T, H, W),
             L.rule_scene_diff((H // 16) * (W // 16)), L.rule_scene_diff((64 // 16) * (96 // 16))]
    assert all(L.single_trip(l) and not L.cap_binds(l) for l in rules)
    for x, pic in list(SM.gpu_cases().values()) + list(NM.gpu_cases().values()):
        t, _, hp, wp = x.shape
        h, w = pic if pic is not None else (hp, wp)
        assert all(L.single_trip(l) for l in (L.rule_sigma_hist(t, h, w), L.rule_fill_sigma(t, hp, wp), L.rule_nlf_map(t, hp, wp), L.rule_vst(t, hp, wp)))
    for (h, w), (hp, wp) in list(P.HALF_ITEM_SIZES) + list(F.PICTURES):
        assert L.single_trip(L.rule_yuv(max(P.T, F.T), h, w, 444)) and L.single_trip(L.rule_blend(F.T, hp, wp))


# ---- the models are chunk-invariant at the new shapes -----------------------------------------------------------------------------------------
def _first(entry, **kw):
    return next(c for c in L.SWEEP_CASES if c.entry == entry and all(getattr(c, k) == v for k, v in kw.items()))


def _cat(a, b):
    if isinstance(a, tuple) or isinstance(a, list):
        return type(a)(_cat(x, y) for x, y in zip(a, b))
    return None if a is None else np.concatenate([a, b])


def _eq(a, b):
    if isinstance(a, (tuple, list)):
        return all(_eq(x, y) for x, y in zip(a, b))
    return (a is None and b is None) or np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


FULL = [_first("u8_in", pad=True), _first("u8_out", pad=True), _first("yuv_in", family="rows"), _first("yuv_out", dither="random"),
        _first("yuv_out", fmt="p010"), _first("rgb_in", family="rows"), _first("rgb_out", dither="random"), _first("rgb_out", dither="ordered"),
        _first("blend", strength=(0.4, 0.8))]


@pytest.mark.parametrize("c", FULL, ids=lambda c: c.id)
def test_sweep_models_do_not_depend_on_the_chunking(c):
    """model(all frames) == the concatenation of model(chunk) over the case's own chunks, with frame0 advanced for random dither
    (launch_shapes.model does that): one case per model function and dither mode, whole"""
    parts = L.chunks(lambda T: L.case_rule(c, T), c.T)
    got = L.model(c, *parts[0])
    for lo, hi in parts[1:]:
        got = _cat(got, L.model(c, lo, hi))
    assert _eq(got, L.model(c))


@pytest.mark.parametrize("c", L.SWEEP_CASES, ids=lambda c: c.id)
def test_every_sweep_model_joins_at_every_chunk_boundary(c):
    """every case, every boundary a of its own chunking: the model of frames a - 1 and a in one call is the model of a - 1 followed by the
    model of a (the models have no term across frames but the dither's frame index, so the boundaries are where a chunked call can differ)"""
    for a, _ in L.chunks(lambda T: L.case_rule(c, T), c.T)[1:]:
        assert _eq(L.model(c, a - 1, a + 1), _cat(L.model(c, a - 1, a), L.model(c, a, a + 1))), a


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("fc", [fc for fc in L.FRAME_CASES if fc.regime in ("collapsed", "max_frames") or fc.id == "scene-gw240"], ids=lambda fc: fc.id)
def test_frame_models_do_not_depend_on_the_chunking(fc, per_frame):
    """every frame kernel at its collapsed-cap case under the case's own chunking: the histograms and values, the filled planes, the VST with
    one table set and with a set per frame, the scene grid and its sums with the frame before a chunk as ``prev``"""
    parts = L.chunks(lambda T: L.frame_rule(fc, T), fc.T)
    assert len(parts) >= 3
    got = L.frame_model(fc, *parts[0], per_frame=per_frame)
    for lo, hi in parts[1:]:
        got = _cat(got, L.frame_model(fc, lo, hi, per_frame=per_frame))
    assert _eq(got, L.frame_model(fc, per_frame=per_frame))


def test_fma32_rounds_an_exact_tie_half_to_even():
    """found by blend-0.4-0.8 on the device (30 of 29 million elements): w_B = Kb of bt709, d_B = -0.5, and an inner sum that puts the exact
    result midway between two float32 values.  fmaf gives the even neighbour; the model's repair of its double rounding took the lower one"""
    f32 = np.float32
    a, b, c = f32(F.LUMA_W["bt709"][2]), f32(-0.5), f32(0.73954386)
    import fractions
    exact = fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c))
    got = F.fma32(np.array([a]), np.array([b]), np.array([c]))[0]
    lo, hi = np.nextafter(got, f32(-np.inf)), np.nextafter(got, f32(np.inf))
    d = abs(fractions.Fraction(float(got)) - exact)
    assert d <= abs(fractions.Fraction(float(lo)) - exact) and d <= abs(fractions.Fraction(float(hi)) - exact)
    if d in (abs(fractions.Fraction(float(lo)) - exact), abs(fractions.Fraction(float(hi)) - exact)):
        assert got.view(np.uint32) % 2 == 0
    c0 = next(c for c in L.SWEEP_CASES if c.id == "blend-0.4-0.8")
    y, x = L.values(c0.T, c0.Hp, c0.Wp)[67:68, :, 65:66, 33:34], L.values(c0.T, c0.Hp, c0.Wp, 4)[67:68, :, 65:66, 33:34]
    assert F.blend(y, x, 0.4, 0.8, F.LUMA_W["bt709"])[0, 1, 0, 0] == f32(0.42377573)
