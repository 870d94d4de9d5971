"""The variance-stabilising transform without a device: the properties of the numpy model (tests/vst_model.py) that the device is held to
bit for bit in tests/test_gpu_vst.py -- exact ends, ordering, sigma', the round trip of every code, monotonicity, special values, and that
the transformed frames of signal-dependent noise are as flat as the estimator can tell --, the mutants of the model, each failing one of
them, and the host logic of ``vst=``: the refusals and the table ring.

Measured figures (profiles/vst.txt): flattening, worst relative deviation from sigma' over the scored levels and eight seeds: transformed
frames 0.119, white-noise reference 0.099 (bound 1.5 x the reference = 0.148); spread max / min of the re-estimated curve 2.27 .. 2.52 raw,
1.09 .. 1.18 transformed.  Every 8-, 10-, 12- and 16-bit code survives the round trip for the five curves at the default floor."""
import os

import numpy as np
import pytest

import nlf_model as NM
import vst_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CURVES = V.curves()


# ---- properties, as functions of a model so that the mutants can be put through them ---------------------------------------------------

class Model:
    def __init__(self, mutant=None):
        self.mutant = mutant

    def build(self, c, floor=V.FLOOR):
        return V.build(c, floor, self.mutant)

    def forward(self, x, G):
        return V.forward(x, G, self.mutant)

    def inverse(self, y, G, R):
        return V.inverse(y, G, R, self.mutant)


FLOORS = (V.FLOOR_MIN, V.FLOOR, 0.05)             # the floors of the GPU build test


def check_ends_and_order(m):
    for name, c, floor in ((name, c, floor) for name, c in CURVES.items() for floor in FLOORS):
        G, R, sigma = m.build(c, floor)
        assert G.dtype == f32 and R.dtype == f32 and G.shape == (V.KNOTS,) and R.shape == (V.N,)
        assert G[0] == 0 and G[V.N] == 1, name
        assert np.all(np.diff(G.astype(np.float64)) > 0), name
        assert np.all(np.isfinite(R)) and np.all(R > 0), name
        want = V.harmonic_sigma(c, floor)
        assert abs(float(sigma) - want) <= np.spacing(f32(want)), (name, floor, sigma, want)
        # a knot's own value goes back to the knot exactly: y - G[k] = 0 leaves (float)k / 1024.  (Taken from the interval below, as a
        # `<` search would, it is (k - 1 + d * fl(1 / d)) / 1024, which is not k / 1024 for every d: knot 1 of the step curve at floor 0.05)
        assert np.array_equal(m.inverse(G[:V.N], G, R), (np.arange(V.N) / V.N).astype(f32)), (name, floor)


def check_round_trip(m, bits=(8, 10, 12, 16)):
    for name, c in CURVES.items():
        G, R, _ = m.build(c)
        for b in bits:
            top = 2 ** b - 1
            q = np.arange(top + 1)
            x = (q / top).astype(f32)
            back = m.inverse(m.forward(x, G), G, R)
            with np.errstate(invalid="ignore"):             # (a mutant's table may hold not-a-number)
                got = np.rint(np.nan_to_num(back.astype(np.float64), nan=-1.0, posinf=-1.0, neginf=-1.0) * top).astype(np.int64)
            assert np.array_equal(got, q), (name, b, int(np.count_nonzero(got != q)))


def check_monotone(m):
    codes = (np.arange(65536) / 65535).astype(f32)
    knots = np.sort(V.knot_values())
    for name, c in CURVES.items():
        G, _, _ = m.build(c)
        for x in (codes, knots):
            y = m.forward(x, G)
            assert np.all(np.diff(y.astype(np.float64)) >= 0), name


def check_flattening(m, seeds=range(8), report=None):
    """nlf_model's ramp at 96 x 128 with its Poisson-Gaussian noise, quantised to 8 bits, through the forward model with the true curve's
    tables: the re-estimated curve against sigma', beside the same estimator on the transformed clean scene plus white noise of sigma'"""
    H, W = 96, 128
    c = NM.true_curve().astype(f32)
    G, _, sigma = m.build(c)
    sigma = float(sigma)
    clean = NM.nlf_scene("ramp", H, W)
    tclean = m.forward(clean.astype(f32), G).astype(np.float64)
    worst, worst_ref, spreads = 0.0, 0.0, []
    for seed in seeds:
        raw = np.zeros((1, 4, H, W), f32)
        raw[0, :3] = NM.S.to_f32(NM.poisson_gauss_u8(clean, seed))
        est_raw = NM.estimate(raw)[0][0].astype(np.float64)
        tx = raw.copy()
        tx[0, :3] = m.forward(raw[0, :3], G)
        est = NM.estimate(tx)[0][0].astype(np.float64)
        ref = np.zeros((1, 4, H, W), f32)
        ref[0, :3] = (tclean + sigma * np.random.default_rng(seed).standard_normal(tclean.shape)).astype(f32)
        est_ref = NM.estimate(ref)[0][0].astype(np.float64)
        lv = np.arange(NM.LEVELS)
        scored = lv[(NM.CENTRES - 3 * sigma >= 0) & (NM.CENTRES + 3 * sigma <= 1)]     # centre +- 3 sigma' inside [0, 1], transformed domain
        assert len(scored) >= 8
        worst = max(worst, float(np.max(np.abs(est[scored] - sigma) / sigma)))
        worst_ref = max(worst_ref, float(np.max(np.abs(est_ref[scored] - sigma) / sigma)))
        s0 = NM.scored_levels()
        spread_raw = float(est_raw[s0].max() / est_raw[s0].min())
        spread_tx = float(est[s0].max() / est[s0].min())
        spreads.append((spread_raw, spread_tx))
        assert spread_raw > spread_tx, (seed, spread_raw, spread_tx)
    if report is not None:
        report.update(worst=worst, worst_ref=worst_ref, spreads=spreads, sigma=sigma)
    print("vst flattening: worst relative deviation %.4f (reference %.4f, bound %.4f); spreads raw / transformed %s"
          % (worst, worst_ref, 1.5 * worst_ref, ", ".join("%.2f / %.2f" % s for s in spreads)))
    assert worst <= 1.5 * worst_ref, (worst, worst_ref)


def test_ends_ordering_and_sigma():
    check_ends_and_order(Model())
    for floor in (V.FLOOR_MIN, 0.05, 1.0):
        for c in CURVES.values():
            G, R, sigma = V.build(c, floor)
            assert G[0] == 0 and G[-1] == 1 and np.all(np.diff(G.astype(np.float64)) > 0) and np.all(np.isfinite(R))
            assert floor * (1 - 1e-6) <= float(sigma) <= 1.0


def test_every_code_survives_the_round_trip():
    check_round_trip(Model())


def test_forward_is_monotone_over_codes_and_knots():
    check_monotone(Model())


def test_flat_curve_is_the_identity():
    G, R, sigma = V.build(CURVES["flat"])
    assert sigma == CURVES["flat"][0]
    assert np.array_equal(G, (np.arange(V.KNOTS) / V.N).astype(f32)) and np.all(R == V.N)
    x = V.test_values(4096, 3)
    ok = np.isfinite(x)
    assert np.array_equal(V.forward(x, G)[ok], x[ok]) and np.array_equal(V.inverse(x, G, R)[ok], x[ok])   # exact: every step is exact


def test_out_of_range_and_special_values_follow_the_formulas():
    for name, c in CURVES.items():
        G, R, _ = V.build(c)
        d0, d1 = f32(G[1] - G[0]), f32(G[V.N] - G[V.N - 1])
        # outside [0, 1]: the end intervals' lines
        lo = f32(-0.1)
        t = f32(lo * f32(1024))
        assert V.forward(lo, G) == f32(G[0] + f32(t * d0)) and V.forward(lo, G) < 0
        hi = f32(1.1)
        t = f32(f32(hi * f32(1024)) - f32(1023))
        assert V.forward(hi, G) == f32(G[V.N - 1] + f32(t * d1)) and V.forward(hi, G) > 1
        assert V.forward(f32(np.inf), G) == np.inf and V.forward(f32(-np.inf), G) == -np.inf
        assert np.isnan(V.forward(f32(np.nan), G)) and np.isnan(V.inverse(f32(np.nan), G, R))
        assert V.inverse(f32(np.inf), G, R) == np.inf and V.inverse(f32(-np.inf), G, R) == -np.inf
        z = V.forward(f32(-0.0), G)
        assert z == 0 and not np.signbit(z)                                       # G[0] + (-0 * d) = +0
        for sub in (f32(1e-40), f32(-1e-40), f32(1.4e-45)):
            y = V.forward(sub, G)
            assert y == f32(G[0] + f32(f32(sub * f32(1024)) * d0))
        # the inverse continues the end lines too.  The rounding of y (half a spacing) comes back multiplied by the end interval's
        # R / 1024 (up to 1 / floor-ish on a steep curve), beside the few roundings of the inverse's own operations
        for v, k in ((lo, 0), (hi, V.N - 1)):
            y = V.forward(v, G)
            back = V.inverse(y, G, R)
            tol = float(np.spacing(np.abs(y))) * float(R[k]) / V.N + 4 * float(np.spacing(f32(1.1)))
            assert abs(float(back) - float(v)) <= tol, (name, v, back, tol)
        assert V.inverse(f32(0), G, R) == 0 and V.inverse(f32(1), G, R) == 1


def test_no_index_leaves_the_table():
    """the model indexes with numpy, which would raise: every special value and far out-of-range value goes through"""
    G, R, _ = V.build(CURVES["step"])
    x = np.concatenate([V.SPECIALS, f32([1e30, -1e30, 3.4e38, -3.4e38, 1023.5 / 1024, 1.0 - 2 ** -24])])
    y = V.forward(x, G)
    V.inverse(y, G, R)
    V.inverse(x, G, R)


def test_flattening_against_the_white_noise_reference():
    check_flattening(Model())


# ---- the mutants: each fails at least one property ------------------------------------------------------------------------------------

def _fails(check, m):
    try:
        check(m)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutant", V.MUTANTS)
def test_each_mutant_fails_a_property(mutant):
    m = Model(mutant)
    failed = [name for name, check in (("ends", check_ends_and_order), ("round_trip", lambda mm: check_round_trip(mm, bits=(8, 16))),
                                       ("monotone", check_monotone), ("bits", check_bits_against_the_true_model)) if _fails(check, m)]
    print("mutant %s fails: %s" % (mutant, failed))
    assert failed, mutant
    if mutant != "fma":                                  # a contracted forward is a rounding difference: only the bit comparison sees it
        assert set(failed) - {"bits"}, (mutant, failed)


def check_bits_against_the_true_model(m):
    """what the GPU test does with the device in the model's place: tables, forward and inverse bit for bit on the GPU tests' values"""
    x = V.test_values(64 * 96 * 3, 7)
    for name, c, floor in ((name, c, floor) for name, c in CURVES.items() for floor in FLOORS[1:]):
        G, R, sigma = V.build(c, floor)
        g, r, s = m.build(c, floor)
        assert np.array_equal(G, g) and np.array_equal(R, r) and sigma == s, name
        assert np.array_equal(V.forward(x, G), m.forward(x, G), equal_nan=True), name
        y = V.inverse_values(64 * 96 * 3, 7, G)
        assert np.array_equal(V.inverse(y, G, R), m.inverse(y, G, R), equal_nan=True), name


def test_the_gpu_values_hold_the_specials_and_every_knot():
    x = V.test_values(64 * 96 * 3, 7)
    assert np.isnan(x).any() and np.isinf(x).any() and (x < 0).any() and (x > 1).any()
    assert set(V.knot_values().view(np.int32).tolist()) <= set(x.view(np.int32).tolist())
    G = V.build(CURVES["random"])[0]
    assert set(V.knot_values(G).view(np.int32).tolist()) <= set(V.inverse_values(64 * 96 * 3, 7, G).view(np.int32).tolist())


# ---- host logic without a device -------------------------------------------------------------------------------------------------------

class _Net:
    def __init__(self, ch):
        self.net_in_ch = ch


class _FakeModel:
    def __init__(self, ch=4):
        self.net = _Net(ch)


def test_vst_and_sigma_refusals():
    from bsvd_amd import frame_io, pipeline
    curve = frame_io.NoiseCurve.from_model(NM.A, NM.B)
    for cls in (pipeline.LiveStream, pipeline.ClipPipeline):
        for sigma in (0.1, "auto", "nlf", curve):
            with pytest.raises(ValueError, match="sigma must be None"):
                cls(_FakeModel(), sigma=sigma, vst=curve)
            with pytest.raises(ValueError, match="sigma must be None"):
                cls(_FakeModel(), sigma=sigma, vst="scene")
        with pytest.raises(ValueError, match="vst must be"):
            cls(_FakeModel(), vst="frame")
        with pytest.raises(ValueError, match="vst must be"):
            cls(_FakeModel(), vst=[0.1] * 16)
        for floor in (0.0, 2.0 ** -11, 1.5, float("nan"), float("inf"), None, "x"):
            with pytest.raises(ValueError, match="vst_floor"):
                cls(_FakeModel(), vst=curve, vst_floor=floor)


def test_vst_modes_without_a_device():
    from bsvd_amd import frame_io, pipeline
    curve = frame_io.NoiseCurve.from_model(NM.A, NM.B)
    v = pipeline._Vst(_FakeModel(4), None, frame_io.VST_FLOOR, 0.25, "x")
    assert not v.active and v.sigma_in == 0.25                                    # vst=None: the caller's sigma, untouched
    v = pipeline._Vst(_FakeModel(4), curve, frame_io.VST_FLOOR, None, "x")
    assert v.active and not v.scene and v.fills and v.sigma_in == 0.0
    v = pipeline._Vst(_FakeModel(3), "scene", frame_io.VST_FLOOR, None, "x")
    assert v.active and v.scene and not v.fills and v.sigma_in is None            # a blind model: no plane
    flat = frame_io.NoiseCurve([0.1] * 16)
    v = pipeline._Vst(_FakeModel(4), flat, frame_io.VST_FLOOR, None, "x")
    assert not v.active and f32(v.sigma_in) == f32(0.1)                           # the identity: sigma=<that value>, nothing launched
    low = frame_io.NoiseCurve([0.0] * 8 + [0.001] * 8)                            # all below the floor: flat after the clamp
    v = pipeline._Vst(_FakeModel(4), low, frame_io.VST_FLOOR, None, "x")
    assert not v.active and f32(v.sigma_in) == f32(frame_io.VST_FLOOR)
    assert frame_io.vst_identity(curve) is None
    assert pipeline._Vst(_FakeModel(3), flat, frame_io.VST_FLOOR, None, "x").sigma_in is None


def test_constants_match_the_model_and_the_header():
    from bsvd_amd import _lib, frame_io
    assert (_lib.VST_KNOTS, _lib.VST_SIGMA_AT, _lib.VST_R_AT, _lib.VST_TABLE_FLOATS) == (V.KNOTS, V.SIGMA_AT, V.R_AT, V.TABLE_FLOATS)
    assert frame_io.VST_FLOOR == V.FLOOR == 0.5 / 255 and _lib.VST_FLOOR_MIN == V.FLOOR_MIN
    assert {"bsvd_vst_build", "bsvd_vst_forward", "bsvd_vst_inverse"} <= set(_lib.EXPORTS)
    src = open(os.path.join(ROOT, "bsvd_amd", "csrc", "frame_vst_items.h")).read()
    assert "VST_N = 1024" in src and "VST_SIGMA_AT = VST_KNOTS" in src and "VST_R_AT = VST_KNOTS + 3" in src
    flags = open(os.path.join(ROOT, "bsvd_amd", "csrc", "sources.sh")).read()
    assert "frame_vst" in flags.split("BSVD_SRCS=")[1].split("\n")[0] and "frame_nlf|frame_vst) echo \"-ffp-contract=off\"" in flags


def test_error_codes_without_a_device():
    import ctypes
    from bsvd_amd import _lib
    lib = _lib.load()
    P = 4096                                                                      # an aligned, never dereferenced address

    def err(rc, *words):
        msg = lib.bsvd_last_error().decode()
        assert rc == -3 and all(w in msg for w in words), (rc, msg, words)

    B = lib.bsvd_vst_build
    err(B(None, 1, V.FLOOR, P, None), "bsvd_vst_build", "curves is NULL")
    err(B(P, 1, V.FLOOR, None, None), "tables is NULL")
    err(B(P + 2, 1, V.FLOOR, P, None), "4-byte aligned")
    err(B(P, 1, V.FLOOR, P + 1, None), "4-byte aligned")
    for n in (0, -1, 65536):
        err(B(P, n, V.FLOOR, P, None), "n = %d" % n)
    for floor in (0.0, 2.0 ** -11, 1.0001, float("nan"), float("inf"), -1.0):
        err(B(P, 1, floor, P, None), "floor")
    F = lib.bsvd_vst_forward
    err(F(None, 1, 4, 4, 64, 3, P, 0, None), "bsvd_vst_forward", "x is NULL")
    err(F(P + 1, 1, 4, 4, 64, 3, P, 0, None), "x must be 4-byte aligned")
    err(F(P, 1, 4, 4, 64, 3, None, 0, None), "tables is NULL")
    err(F(P, 1, 4, 4, 64, 3, P + 2, 0, None), "tables must be 4-byte aligned")
    for frames in (0, -3, 65536):
        err(F(P, frames, 4, 4, 64, 3, P, 0, None), "frames = %d" % frames)
    err(F(P, 1, 0, 4, 64, 3, P, 0, None), "Hp = 0")
    err(F(P, 1, 4, -1, 64, 3, P, 0, None), "Wp = -1")
    err(F(P, 1, 4, 4, 63, 3, P, 0, None), "frame_stride = 63", "4 planes")
    err(F(P, 1, 4, 4, 47, -1, P, 0, None), "frame_stride = 47", "3 planes")
    for fill in (0, 1, 2):
        err(F(P, 1, 4, 4, 64, fill, P, 0, None), "fill_plane = %d" % fill)
    err(F(P, 1, 4, 4, 64, 3, P, -1, None), "table_stride = -1")
    I = lib.bsvd_vst_inverse
    err(I(None, 48, 1, 4, 4, P, 0, None), "bsvd_vst_inverse", "y is NULL")
    err(I(P + 3, 48, 1, 4, 4, P, 0, None), "y must be 4-byte aligned")
    err(I(P, 48, 1, 4, 4, None, 0, None), "tables is NULL")
    err(I(P, 47, 1, 4, 4, P, 0, None), "y_frame_stride = 47")
    err(I(P, 48, 0, 4, 4, P, 0, None), "frames = 0")
    err(I(P, 48, 1, 0, 4, P, 0, None), "Hp = 0")
    err(I(P, 48, 1, 4, 0, P, 0, None), "Wp = 0")
    err(I(P, 48, 1, 4, 4, P, -2, None), "table_stride = -2")
    assert ctypes.sizeof(ctypes.c_float) == 4


# ---- the table ring: frame k's set meets frame k's output ------------------------------------------------------------------------------

def _ring_walk(make_ring, latency, scenes, flush_after):
    """a stand-in for the stream: every feed writes the scene's "table set" (its scene number in every float) into the ring's next slot and
    `latency` feeds later the frame's output is paired with the ring's next set; scene changes are cuts; after `flush_after` frames the
    tail is drained and the ring reset, then the walk goes on.  -> [(frame's scene, the scene of the set it met)]"""
    import torch
    ring = make_ring()
    met, pending = [], []

    def emit():
        met.append((pending.pop(0), int(ring.next_out()[0, 0])))

    for k, scene in enumerate(scenes):
        if k == flush_after:
            while pending:
                emit()
            ring.reset()
        ring.next_in().copy_(torch.full((1, V.TABLE_FLOATS), float(scene)))
        pending.append(scene)
        if len(pending) > latency:
            emit()
    while pending:
        emit()
    return met


def test_table_ring_pairs_every_frame_with_its_own_set():
    from bsvd_amd import pipeline
    latency, depth = 17, 1
    scenes = [0] * 5 + [1] * 9 + [2] * 30 + [3] * 4 + [4] * 25                  # cuts closer together and further apart than the latency
    met = _ring_walk(lambda: pipeline._TableRing(latency + depth, "cpu"), latency, scenes, flush_after=40)
    assert len(met) == len(scenes) and all(a == b for a, b in met)
    # the mutant: a ring one set short hands a frame the set of the frame `latency` feeds later -- another scene's, near every cut
    met = _ring_walk(lambda: pipeline._TableRing(latency + depth - 1, "cpu"), latency, scenes, flush_after=40)
    assert any(a != b for a, b in met)
    ring = pipeline._TableRing(3, "cpu")
    with pytest.raises(RuntimeError, match="before it went in"):
        ring.next_out()
