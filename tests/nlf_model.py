"""numpy model of the device's noise-level function (include/bsvd_hip.h, bsvd_estimate_nlf / bsvd_fill_nlf_plane;
bsvd_amd/csrc/frame_nlf_items.h), written from the definition line by line: fp32 adds in the stated order, an int64 histogram
[T, 16, 1024], the curve in integers and float64, the map in fp32 with the product rounded before the add.  The GPU tests hold the device's
histogram, curve and map to this model bit for bit.  The MUTANTS are the ways an implementation could plausibly differ;
tests/test_nlf_cpu.py shows that each one changes a result on the GPU tests' inputs."""
import numpy as np

import sigma_model as S

LEVELS, BINS = 16, 1024
K = 1.0 / (1024 * 6 * 0.6744897501960817)
SIGMA_MAX = BINS * K
MIN_COUNT = 512
BAND = S.BAND

f32 = np.float32
C169 = f32(16.0 / 9.0)
C1636 = f32(16.0 / 36.0)

MUTANTS = ("centre_pixel", "level_off_by_one", "valid_gt", "tie_high", "lerp_edges", "fma")


def box(p):
    """p: fp32 [..., h, w] -> the 3 x 3 box sum at the interior pixels, fp32 [..., h - 2, w - 2]:
    row = (x_w + x_c) + x_e per row, S = (row_n + row_c) + row_s"""
    p = np.asarray(p, f32)
    with np.errstate(all="ignore"):
        rows = (p[..., :, :-2] + p[..., :, 1:-1]) + p[..., :, 2:]
        return ((rows[..., :-2, :] + rows[..., 1:-1, :]) + rows[..., 2:, :]).astype(f32)


def levels_of(s):
    """fp32 box sums -> l = clamp(floor(S * 16/9), 0, 15); +inf gives 15, anything not >= 0 gives 0"""
    with np.errstate(all="ignore"):
        t = np.asarray(s, f32) * C169
        return np.where(t >= 15, 15, np.where(t >= 0, np.floor(np.where(t >= 0, np.minimum(t, 15), 0)), 0)).astype(np.int64)


def bins_of(r):
    """fp32 responses -> (q = min(floor(|r| * 1024), 1023), counted: r is finite)"""
    r = np.asarray(r, f32)
    ok = np.isfinite(r)
    with np.errstate(all="ignore"):
        t = np.abs(r) * f32(1024)
    q = np.minimum(np.floor(np.where(ok, t, 0)), BINS - 1).astype(np.int64)
    return q, ok


def histogram(x, picture=None, mutant=None):
    """x: fp32 [T, C >= 3, Hp, Wp] -> int64 [T, 16, 1024].  picture = (H, W): the top-left part of each plane that is sampled"""
    x = np.asarray(x, f32)
    T, C, Hp, Wp = x.shape
    H, W = picture if picture is not None else (Hp, Wp)
    assert 3 <= H <= Hp and 3 <= W <= Wp and C >= 3
    p = x[:, :3, :H, :W]
    q, ok = bins_of(S.response(p))
    with np.errstate(all="ignore"):
        s = (p[..., 1:-1, 1:-1] * f32(9)).astype(f32) if mutant == "centre_pixel" else box(p)
    lv = levels_of(s)
    if mutant == "level_off_by_one":
        lv = np.minimum(lv + 1, LEVELS - 1)
    key = lv * BINS + q
    hist = np.zeros((T, LEVELS * BINS), np.int64)
    for t in range(T):
        hist[t] = np.bincount(key[t][ok[t]], minlength=LEVELS * BINS)
    return hist.reshape(T, LEVELS, BINS)


def _value(h, gain, lo, hi):
    """one histogram of 1024 counts -> (fp32 value, N): sigma_model.finish with 1024 bins per unit"""
    N = int(h.sum())
    if N == 0:
        return f32(lo), 0
    cum = np.cumsum(h)
    k = int(np.argmax(2 * cum >= N))
    before = int(cum[k] - h[k])
    med = np.float64(k) + np.float64(N - 2 * before) / np.float64(2 * int(h[k]))
    s = med * np.float64(K)
    s = s * np.float64(gain)
    return f32(min(max(s, np.float64(lo)), np.float64(hi))), N


def curve(hist, gain=1.0, lo=0.0, hi=SIGMA_MAX, min_count=MIN_COUNT, mutant=None, return_valid=False):
    """int [T, 16, 1024] -> fp32 [T, 16]: the valid levels' own medians, the others filled from the nearest valid level (the lower one on a
    tie); no valid level: the pooled median everywhere"""
    hist = np.asarray(hist).astype(np.int64)
    gain, lo, hi = float(f32(gain)), float(f32(lo)), float(f32(hi))
    out = np.empty((hist.shape[0], LEVELS), f32)
    valid_all = np.zeros((hist.shape[0], LEVELS), bool)
    for t, h in enumerate(hist):
        own, valid = [], []
        for l in range(LEVELS):
            v, N = _value(h[l], gain, lo, hi)
            own.append(v)
            valid.append(N > min_count if mutant == "valid_gt" else N >= min_count)
        valid_all[t] = valid
        pooled = _value(h.sum(0), gain, lo, hi)[0]
        for l in range(LEVELS):
            out[t, l] = pooled
            for d in range(LEVELS):
                order = (l + d, l - d) if mutant == "tie_high" else (l - d, l + d)
                pick = [j for j in order if 0 <= j < LEVELS and valid[j]]
                if pick:
                    out[t, l] = own[pick[0]]
                    break
    return (out, valid_all) if return_valid else out


def estimate(x, picture=None, gain=1.0, clamp=(0.0, SIGMA_MAX), min_count=MIN_COUNT, mutant=None):
    """-> (curve fp32 [T, 16], hist int64 [T, 16, 1024])"""
    hist = histogram(x, picture, mutant)
    return curve(hist, gain, clamp[0], clamp[1], min_count, mutant), hist


def noise_map(x, c, mutant=None):
    """x: fp32 [T, C >= 3, Hp, Wp], c: fp32 [T, 16] -> fp32 [T, Hp, Wp]: box sums with replicate borders,
    u = ((S_R + S_B) + 2 S_G) * (16/36) - 0.5 clamped to [0, 15] (NaN: 0), i = min(int(u), 14), f = u - i, c[i] + f * (c[i+1] - c[i])"""
    x = np.asarray(x, f32)
    c = np.asarray(c, f32)
    T = x.shape[0]
    with np.errstate(all="ignore"):
        s = box(np.pad(x[:, :3], ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge"))
        mix = (s[:, 0] + s[:, 2]) + f32(2) * s[:, 1]
        u = mix * C1636
        if mutant != "lerp_edges":
            u = u - f32(0.5)
        u = np.where(u >= 15, f32(15), np.where(u >= 0, u, f32(0))).astype(f32)
        i = np.minimum(u.astype(np.int64), LEVELS - 2)
        f = (u - i.astype(f32)).astype(f32)
        t = np.arange(T)[:, None, None]
        c0, c1 = c[t, i], c[t, i + 1]
        d = (c1 - c0).astype(f32)
        if mutant == "fma":
            return (f.astype(np.float64) * d.astype(np.float64) + c0.astype(np.float64)).astype(f32)
        fd = (f * d).astype(f32)
        return (c0 + fd).astype(f32)


# ---------------------------------------------------------------------------------------------------
# signal-dependent noise: sigma(I) = sqrt(a I + b), quantised to 8 bits

A, B = (20.0 / 255) ** 2, (5.0 / 255) ** 2
CENTRES = (np.arange(LEVELS) + 0.5) / LEVELS


def true_curve(a=A, b=B):
    return np.sqrt(np.maximum(a * CENTRES + b, 0))


def scored_levels(a=A, b=B):
    """the levels whose centre +- 3 sigma stays inside [0, 1]: the clipped ends read low by construction"""
    s = true_curve(a, b)
    return np.nonzero((CENTRES - 3 * s >= 0) & (CENTRES + 3 * s <= 1))[0]


def nlf_scene(kind, H, W, seed=0):
    """clean RGB scene in [0,1], float64 [3, H, W]: 'ramp' (a horizontal ramp 0 .. 1 in every plane) or 'blocks' (flat 8 x 8 blocks, one grey
    value in [0, 1] per block)"""
    if kind == "ramp":
        return np.broadcast_to(np.linspace(0, 1, W)[None, None, :], (3, H, W)).copy()
    if kind == "blocks":
        rs = np.random.default_rng(seed)
        g = rs.uniform(0, 1, ((H + 7) // 8, (W + 7) // 8))
        return np.broadcast_to(np.kron(g, np.ones((8, 8)))[None, :H, :W], (3, H, W)).copy()
    raise ValueError(kind)


def poisson_gauss_u8(clean, seed=0, a=A, b=B):
    """clean [..] in [0,1] + noise of sigma(I) = sqrt(a I + b), rounded and clipped to uint8"""
    rs = np.random.default_rng(seed)
    v = clean + np.sqrt(np.maximum(a * clean + b, 0)) * rs.standard_normal(clean.shape)
    return np.clip(np.rint(v * 255.0), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_nlf.py (built here so that tests/test_nlf_cpu.py can show that each mutant differs on them)

def _noisy(T, H, W, seed, kind="mixed"):
    """[T, 4, H, W]: uint8-derived frames of one scene with signal-dependent noise; plane 3 (the noise-map plane) zero"""
    x = np.zeros((T, 4, H, W), f32)
    for t in range(T):
        x[t, :3] = S.to_f32(poisson_gauss_u8(S.scene(kind, H, W, seed + t), seed + 100 + t, a=A * (1 + t), b=B))
    return x


def gpu_cases():
    """name -> (x fp32 [T, 4, Hp, Wp], picture (H, W) or None)"""
    cases = {}
    cases["noisy_1x64x96"] = (_noisy(1, 64, 96, 1), None)
    cases["noisy_5x64x96"] = (_noisy(5, 64, 96, 2), None)
    pic = _noisy(2, 37, 50, 40)
    cases["pad_nan_37x50_in_40x52"] = (S._in_tensor(pic, 40, 52, np.nan), (37, 50))
    cases["pic_3x3"] = (_noisy(1, 3, 3, 3), None)
    cases["scalar_11x67"] = (_noisy(1, 11, 67, 4), None)                # a row that cannot move as float4; BAND + 1 interior rows
    cases["shape_2x12x20"] = (_noisy(2, 12, 20, 5), None)
    wide = _noisy(2, 24, 40, 6)
    wide[:, :3] = (wide[:, :3] * f32(1.6) - f32(0.3)).astype(f32)        # below 0 and above 1
    cases["out_of_range"] = (wide, None)
    bad = _noisy(2, 24, 40, 70)
    rs = np.random.default_rng(71)
    for v in (np.nan, np.inf, -np.inf):
        for _ in range(6):
            bad[rs.integers(2), rs.integers(3), rs.integers(24), rs.integers(40)] = v
    cases["nan_inf"] = (bad, None)
    flat = np.zeros((1, 4, 24, 40), f32)
    flat[:, :3] = f32(0.5)
    cases["flat"] = (flat, None)
    yy, xx = np.mgrid[0:24, 0:40]
    board = np.zeros((1, 4, 24, 40), f32)
    board[:, :3] = (f32(0.25) + f32(0.5) * ((yy + xx) & 1)).astype(f32)
    cases["checkerboard"] = (board, None)
    return cases


def curve_cases():
    """name -> (hist int64 [T, 16, 1024], dict of gain / lo / hi / min_count): hand-built histograms for the curve rules"""
    def h(*levels):
        a = np.zeros((1, LEVELS, BINS), np.int64)
        for l, k, n in levels:
            a[0, l, k] += n
        return a
    cases = {}
    # level 3 has exactly min_count samples (valid), level 4 one fewer (not valid: takes level 3's value, not its own)
    cases["min_count_boundary"] = (h((3, 10, 100), (4, 50, 99)), dict(min_count=100))
    # levels 2 and 6 valid with different values: level 4 is two away from both and takes the lower level's; 3 -> 2, 5 -> 6
    cases["tie_to_the_lower_level"] = (h((2, 20, 600), (6, 80, 600)), dict())
    cases["no_valid_level_pooled"] = (h((1, 10, 100), (7, 30, 100), (9, 40, 101)), dict())
    cases["empty_gives_lo"] = (h(), dict(lo=0.0125))
    cases["gain_and_clamp"] = (h((2, 20, 600), (6, 80, 600), (10, 300, 600)), dict(gain=1.37, lo=0.01, hi=0.05))
    two = np.concatenate([cases["tie_to_the_lower_level"][0], cases["no_valid_level_pooled"][0]])
    cases["two_frames"] = (two, dict())
    return cases
