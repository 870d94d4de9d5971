"""The film-grain model without a device: the numpy model (tests/grain_model.py) that the device is held to bit for bit in
tests/test_gpu_grain.py -- its 256 integers against a brute-force double loop, their independence of how the frames are chunked, the
product's host fit (frame_io.grain_from_stats / grain_template) against the model's, the closed loop of tests/grain_cases.py --, the
mutants of the model, each failing its comparison, and the host logic: GrainModel, the refusals of the entry points and of the pipelines'
``grain=`` arguments.

Measured figures (profiles/film_grain.txt, section 1): closed loop at 192 x 256, five flat levels, template seed 0: recovered std within
0.0152 (relative) of the set value, implied autocorrelation within 0.0457 (absolute) of the set one; bounds 2 x these."""
import ctypes

import numpy as np
import pytest

import grain_cases as C
import grain_model as G

f32 = np.float32
_CACHE = {}


def noisy_pair(T, Hp, Wp, seed, special=True):
    """(x, y) [T,3,Hp,Wp]: a smooth result y, a source x = y + noise of a few levels' strength, with (special) differences that saturate
    q, a NaN and an inf pixel"""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(Hp), np.arange(Wp), indexing="ij")
    base = ((r * 3 + c * 5) % 97 / 96.0).astype(f32)
    y = np.stack([np.stack([base, base[::-1], base[:, ::-1]]) * f32(0.9 + 0.05 * t) for t in range(T)]).astype(f32)
    x = (y + rng.normal(0, 0.04, y.shape)).astype(f32)
    if special:
        x[0, 0, 1, 7] = f32(3.0)                      # saturates: n 4096 far beyond 2047
        x[0, 2, 2, 8] = f32(-2.5)
        x[0, 1, 0, 6] = f32(np.nan)                   # an anchor that is not counted
        x[-1, 0, 3, 9] = f32(np.inf)
        y[-1, 1, 2, 10] = f32(-np.inf)
    return x, y


def closed_loop():
    """the numpy model alone on the cases of grain_cases: -> (std error, acf error), computed once"""
    if "loop" not in _CACHE:
        std, ar = C.set_model()
        y = C.flat_frames()
        x = G.apply(y, G.template(ar, C.TEMPLATE_SEED), std, 1.0, seed=C.APPLY_SEED)
        pooled = G.stats(x, y).sum(axis=0)
        got = G.fit(pooled, len(C.LEVELS) * (C.H - 3) * (C.W - 12))
        _CACHE["loop"] = (pooled, got, C.errors(*got))
    return _CACHE["loop"]


# ---- the statistics --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,Hp,Wp", [(4, 13, 4, 13), (5, 14, 5, 14), (9, 21, 12, 24), (35, 70, 36, 72)])
def test_sums_equal_a_brute_force_double_loop(H, W, Hp, Wp):
    x, y = noisy_pair(2, Hp, Wp, seed=H * W)
    x[:, :, H:, :] = np.nan
    x[:, :, :, W:] = np.nan                            # the pad region is never looked at
    got = G.stats(x, y, H, W)
    for t in range(2):
        assert np.array_equal(got[t], G.stats_brute(x[t], y[t], H, W)), (H, W, t)
    assert np.all(got[:, 250:] == 0)
    assert got[:, G.N_AT:G.N_AT + 16].sum() == 2 * H * W - 3            # the three pixels with a non-finite n are not counted


def test_single_anchor_and_counts():
    x, y = noisy_pair(1, 4, 13, seed=3, special=False)
    st = G.stats(x, y)[0]
    l, q, counted = G.pixel_terms(x[0], y[0], G.weights())
    assert counted.all() and st[G.N_AT:G.N_AT + 16].sum() == 52
    for k in range(3):
        for i, (dy, dx) in enumerate(G.LAG_LIST):
            assert st[G.A_AT + G.LAGS * k + i] == q[k, 0, 6] * q[k, dy, 6 + dx]


def test_chunk_invariance():
    x, y = noisy_pair(5, 20, 40, seed=11)
    whole = G.stats(x, y, 19, 37)
    parts = np.concatenate([G.stats(x[a:b], y[a:b], 19, 37) for a, b in ((0, 1), (1, 4), (4, 5))])
    assert np.array_equal(whole, parts)
    from bsvd_amd import frame_io as F
    a = F.grain_from_stats(whole.sum(axis=0), 5 * 16 * 25, min_count=64)
    b = F.grain_from_stats(whole[::-1].copy()[[2, 0, 4, 1, 3]].sum(axis=0), 5 * 16 * 25, min_count=64)
    assert np.array_equal(a.std, b.std) and np.array_equal(a.ar, b.ar)


def test_quantisation_rule():
    w = G.weights()
    y = np.zeros((3, 1, 6), f32)
    x = y.copy()
    # equal differences in R, G, B: n0 = d (the weights sum to 1 within rounding), n1 = n2 ~ 0
    x[:, 0, :] = np.array([0.5 / 4096, 1.5 / 4096, 2.5 / 4096, -0.5 / 4096, 0.6, -0.6], f32)
    l, q, counted = G.pixel_terms(x, y, w)
    assert counted.all() and list(q[0, 0, 4:]) == [2047, -2047]
    n0 = G.luma(w, x[0], x[1], x[2])
    assert np.array_equal(q[0], np.rint(np.clip(n0 * f32(4096), -2047, 2047)).astype(np.int64))
    assert np.all(np.abs(q) <= 2047) and np.all(l == 0)
    # levels: luma(y) 16 floors, +inf -> 15, NaN and negatives -> 0
    assert list(G.level(np.array([0.0, 0.0624, 0.0626, 0.9999, 1.0, 7.0, np.inf, -0.1, -np.inf, np.nan], f32))) == [0, 0, 1, 15, 15, 15, 15, 0, 0, 0]


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------------

def test_lists_and_layout_match_the_library_constants():
    from bsvd_amd import _lib
    from bsvd_amd import frame_io as F
    assert F.GRAIN_LAG_LIST == G.LAG_LIST and F.GRAIN_TAP_LIST == G.TAP_LIST and len(G.LAG_LIST) == 46 and len(G.TAP_LIST) == 24
    assert (_lib.GRAIN_N_AT, _lib.GRAIN_S1_AT, _lib.GRAIN_S2_AT, _lib.GRAIN_A_AT, _lib.GRAIN_STATS) == (G.N_AT, G.S1_AT, G.S2_AT, G.A_AT, G.STATS)
    assert G.A_AT + 3 * G.LAGS == 250
    # every difference of two taps is a lag or a lag's mirror image
    for yi, xi in G.TAP_LIST:
        for yj, xj in G.TAP_LIST:
            G.lag_index(yi - yj, xi - xj)
    for name in ("bsvd_grain_stats_bytes", "bsvd_grain_stats", "bsvd_grain_apply"):
        assert name in _lib.EXPORTS


def test_host_fit_equals_the_model():
    from bsvd_amd import frame_io as F
    pooled, (std, ar), _ = closed_loop()
    anchors = len(C.LEVELS) * (C.H - 3) * (C.W - 12)
    m = F.grain_from_stats(pooled, anchors)
    assert np.allclose(m.std, std, rtol=1e-12, atol=0) and np.allclose(m.ar, ar, rtol=0, atol=1e-10)
    # levels without pixels take the nearest measured one, the lower on a tie
    assert m.std[0][0] == m.std[0][1] and m.std[0][2] == m.std[0][1] and m.std[0][3] == m.std[0][4] and m.std[0][15] == m.std[0][13]
    # no level reaches min_count: the pooled value everywhere; no pixels at all: zeros
    p = F.grain_from_stats(pooled, anchors, min_count=10 ** 9)
    assert np.all(p.std == p.std[:, :1]) and np.all(p.std > 0)
    z = F.grain_from_stats(np.zeros(256, np.int64), 1)
    assert z.is_zero and not z.ar.any()
    with pytest.raises(ValueError):
        F.grain_from_stats(np.zeros(255, np.int64), 1)
    with pytest.raises(ValueError):
        F.grain_from_stats(np.zeros(256, np.int64), 0)


def test_template_equals_the_pixel_by_pixel_recursion():
    from bsvd_amd import frame_io as F
    _, ar = C.set_model()
    ar[0, 1], ar[0, 2], ar[1, 9], ar[2, 23] = 0.1, -0.05, 0.03, 0.02           # taps of the row, of the rows above, the farthest one
    got = F.grain_template(ar, 5)
    assert got.dtype == f32 and got.shape == (3, 128, 128)
    assert np.allclose(got, G.template(ar, 5), rtol=0, atol=1e-5)
    assert np.allclose(got.astype(np.float64).std(axis=(1, 2)), 1.0, atol=1e-6)
    white = F.grain_template(np.zeros((3, 24)), 5)
    assert abs(float((white[0, :, 1:] * white[0, :, :-1]).mean())) < 0.03
    unstable = np.zeros((3, 24))
    unstable[:, 0] = 5.0                                                    # explodes: the white field stands in
    assert np.array_equal(F.grain_template(unstable, 5), white)


def test_solver_without_lapack():
    from bsvd_amd import frame_io as F
    rng = np.random.default_rng(0)
    A = rng.normal(size=(24, 24))
    M = A @ A.T + 0.1 * np.eye(24)
    b = rng.normal(size=24)
    assert np.allclose(F._solve(M, b), np.linalg.solve(M, b), rtol=1e-9, atol=1e-12)
    assert not F._solve(np.zeros((24, 24)), b).any()


# ---- the closed loop -------------------------------------------------------------------------------------------------------------------------

def test_closed_loop_of_the_model():
    _, _, (e_std, e_acf) = closed_loop()
    print("closed loop, numpy model: std %.4f (bound %.4f), acf %.4f (bound %.4f)" % (e_std, C.STD_BOUND, e_acf, C.ACF_BOUND))
    assert e_std <= C.STD_BOUND and e_acf <= C.ACF_BOUND
    # the recorded figures are this run's: the bounds were not set from anything else
    assert abs(e_std - C.MODEL_STD_ERR) < 5e-4 and abs(e_acf - C.MODEL_ACF_ERR) < 5e-4


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------

def test_mutants_fail_their_comparison():
    x, y = noisy_pair(1, 12, 24, seed=5)
    want = G.stats_brute(x[0], y[0], 11, 23)
    assert np.array_equal(G.stats(x, y, 11, 23)[0], want)
    for lag in (0, 6, 7, 45):
        assert not np.array_equal(G.stats(x, y, 11, 23, drop_lag=lag)[0], want), lag
    assert not np.array_equal(G.stats(x, y, 11, 23, anchor_shift=1)[0], want)          # an anchor window one column wide of the rule
    assert not np.array_equal(G.stats(x, y, 11, 23, level_from="x")[0], want)
    # block offsets that ignore the frame index: frames 0 and 5 of a stream get one pattern
    std, ar = C.set_model()
    tm = np.random.default_rng(1).normal(size=(3, 128, 128)).astype(f32)
    flat = np.full((1, 3, 40, 72), 0.5, f32)
    a, b = G.apply(flat, tm, std, seed=3, frame0=0), G.apply(flat, tm, std, seed=3, frame0=5)
    assert not np.array_equal(a, b)
    assert np.array_equal(G.apply(flat, tm, std, seed=3, frame0=0, ignore_frame=True), G.apply(flat, tm, std, seed=3, frame0=5, ignore_frame=True))
    two = G.apply(np.concatenate([flat, flat]), tm, std, seed=3, frame0=4)
    assert np.array_equal(two[1:], b) and not np.array_equal(two[:1], b)           # a frame's pattern follows its stream index


def test_apply_properties():
    std, _ = C.set_model()
    tm = np.random.default_rng(2).normal(size=(3, 128, 128)).astype(f32)
    y = np.full((1, 3, 33, 65), 0.5, f32)
    assert G.apply(y, tm, std, amount=0.0) is y and G.apply(y, tm, np.zeros((3, 16))) is y
    out = G.apply(y, tm, std, seed=9)
    # every block is a window of the templates: luma of the added noise / std is a template sample
    oy, ox = G.block_offsets(9, 0, np.array([0, 0, 1]), np.array([0, 2, 1]))
    assert np.all((oy >= 0) & (oy <= 96) & (ox >= 0) & (ox <= 96))
    all_oy, all_ox = G.block_offsets(1, 2, *np.meshgrid(np.arange(64), np.arange(64)))
    assert all_oy.min() == 0 and all_oy.max() == 96 and all_ox.min() == 0 and all_ox.max() == 96
    w = G.weights()
    d = out - y
    n0 = G.luma(w, d[0, 0], d[0, 1], d[0, 2])
    s0 = G.scale(G.luma(w, y[0, 0], y[0, 1], y[0, 2]), std.astype(f32))[0]
    assert np.allclose(n0[:32, :32] / s0[:32, :32], tm[0, oy[0]:oy[0] + 32, ox[0]:ox[0] + 32], atol=2e-3)
    assert np.allclose(n0[32:33, 32:64] / s0[32:33, 32:64], tm[0, oy[2]:oy[2] + 1, ox[2]:ox[2] + 32], atol=2e-3)


# ---- host logic ------------------------------------------------------------------------------------------------------------------------------

def test_grain_model_values():
    from bsvd_amd import frame_io as F
    m = F.GrainModel.from_values(0.02)
    assert m.std.shape == (3, 16) and np.all(m.std == 0.02) and not m.ar.any() and not m.is_zero
    m = F.GrainModel.from_values([0.02, 0.01, 0.0])
    assert np.all(m.std[1] == 0.01) and np.all(m.std[2] == 0)
    assert F.GrainModel.from_values(0.0).is_zero
    std, ar = C.set_model()
    m = F.GrainModel.from_values(std, ar, template_seed=4)
    assert m.templates is m.templates and not m.templates.flags.writeable and m.templates.shape == (3, 128, 128)
    for bad in ("x", [1, 2], np.zeros((3, 15)), -0.1, float("nan"), [[float("inf")] * 16] * 3):
        with pytest.raises(ValueError):
            F.GrainModel.from_values(bad)
    with pytest.raises(ValueError):
        F.GrainModel(std, np.zeros((3, 23)))
    assert F.check_grain(None) == (None, 1.0, 0) and F.check_grain("scene", 0.5, 7) == ("scene", 0.5, 7)
    for kw in (dict(grain="auto"), dict(grain=0.02), dict(grain=m, amount=-1), dict(grain=m, amount=float("nan")), dict(grain=m, amount="x"),
               dict(grain=m, seed=-1), dict(grain=m, seed=2 ** 32), dict(grain=m, seed=1.5)):
        with pytest.raises(ValueError):
            F.check_grain(**kw)


def test_pipelines_refuse_before_a_device_is_touched():
    from bsvd_amd import frame_io as F
    from bsvd_amd.pipeline import ClipPipeline, LiveStream

    class Stub:                                       # raises if the constructor gets as far as asking for the device
        def _device(self):
            raise AssertionError("the device was asked for")

    for cls in (ClipPipeline, LiveStream):
        for kw in (dict(grain="yes"), dict(grain=F.GrainModel.from_values(0.01), grain_amount=-0.5), dict(grain="scene", grain_seed=-3),
                   dict(grain_amount=float("inf"))):
            with pytest.raises(ValueError, match="grain"):
                cls(Stub(), **kw)


def test_refusals_without_a_device():
    from bsvd_amd import _lib
    lib = _lib.load()
    err = lambda: lib.bsvd_last_error().decode()
    assert lib.bsvd_grain_stats_bytes(3) == 3 * 256 * 8 and lib.bsvd_grain_stats_bytes(0) == -1
    w = (ctypes.c_float * 3)(0.2126, 0.7152, 0.0722)
    nanw = (ctypes.c_float * 3)(0.2126, float("nan"), 0.0722)
    P = 0x10000                                       # never dereferenced: every call below is refused before a launch
    ok = dict(x=P, xs=3 * 8 * 16, y=P, ys=3 * 8 * 16, frames=1, H=8, W=16, Hp=8, Wp=16, w=w, ws=P)
    call = lambda **kw: (lambda a: lib.bsvd_grain_stats(a["x"], a["xs"], a["y"], a["ys"], a["frames"], a["H"], a["W"], a["Hp"], a["Wp"], a["w"], a["ws"], None))({**ok, **kw})
    for kw, name in ((dict(x=None), "x is NULL"), (dict(y=None), "y is NULL"), (dict(w=None), "luma_w"), (dict(ws=None), "workspace"),
                     (dict(x=P + 2), "x must be 4-byte"), (dict(y=P + 1), "y must be 4-byte"), (dict(ws=P + 4), "workspace must be 8-byte"),
                     (dict(frames=0), "frames"), (dict(frames=65536), "frames"), (dict(H=3), "H = 3"), (dict(W=12), "W = 12"),
                     (dict(Hp=7), "Hp = 7"), (dict(Wp=15), "Wp = 15"), (dict(xs=3 * 8 * 16 - 1), "x_frame_stride"),
                     (dict(ys=3 * 8 * 16 - 1), "y_frame_stride"), (dict(w=nanw), "luma_w[1]")):
        assert call(**kw) == -3, kw
        assert name in err(), (kw, err())
    std = (ctypes.c_float * 48)(*([0.01] * 48))
    bad_std = (ctypes.c_float * 48)(*([0.01] * 47 + [float("inf")]))
    neg_std = (ctypes.c_float * 48)(*([-0.01] + [0.01] * 47))
    ok = dict(y=P, ys=3 * 8 * 16, frames=1, Hp=8, Wp=16, t=P, std=std, amount=1.0, w=w, inv=1.4, seed=0, f0=0)
    call = lambda **kw: (lambda a: lib.bsvd_grain_apply(a["y"], a["ys"], a["frames"], a["Hp"], a["Wp"], a["t"], a["std"], a["amount"], a["w"], a["inv"], a["seed"], a["f0"], None))({**ok, **kw})
    for kw, name in ((dict(y=None), "y is NULL"), (dict(t=None), "templates is NULL"), (dict(std=None), "std is NULL"), (dict(w=None), "luma_w"),
                     (dict(y=P + 2), "y must be 4-byte"), (dict(t=P + 2), "templates must be 4-byte"), (dict(frames=0), "frames"),
                     (dict(Hp=0), "Hp"), (dict(Wp=-1), "Wp"), (dict(ys=3 * 8 * 16 - 1), "y_frame_stride"), (dict(amount=float("nan")), "amount"),
                     (dict(amount=-1.0), "amount"), (dict(std=bad_std), "std[2][15]"), (dict(std=neg_std), "std[0][0]"), (dict(w=nanw), "luma_w[1]"),
                     (dict(inv=float("inf")), "inv_wg"), (dict(f0=-1), "frame0")):
        assert call(**kw) == -3, kw
        assert name in err(), (kw, err())
    # nothing to add: 0 and no launch (no device is needed to say so)
    zero = (ctypes.c_float * 48)()
    assert call(std=zero) == 0 and call(amount=0.0) == 0
