"""numpy model of the device's noise-level estimate (include/bsvd_hip.h, bsvd_estimate_sigma; bsvd_amd/csrc/frame_sigma_items.h), written
from the definition line by line: fp32 adds in the stated order, an int64 histogram, the finish in integers and float64.  The GPU tests hold
the device's histogram and its fp32 sigma to this model bit for bit.  The MUTANTS are the ways an implementation could plausibly differ;
tests/test_sigma_cpu.py shows that each one changes the result on the GPU tests' inputs, i.e. that those inputs can tell."""
import numpy as np

BINS = 4096
K = 1.0 / (4096 * 6 * 0.6744897501960817)
SIGMA_MAX = BINS * K
BAND = 8                       # interior rows of one item of the device's histogram pass (SIGMA_BAND): the heights the GPU tests step around

f32 = np.float32


def response(p, corners=True):
    """p: fp32 [..., h, w] -> the mask's response at the interior pixels, fp32 [..., h - 2, w - 2]:
    r = (4 x_c - 2 ((x_n + x_s) + (x_w + x_e))) + ((x_nw + x_ne) + (x_sw + x_se))"""
    p = np.asarray(p, f32)
    c = p[..., 1:-1, 1:-1]
    n, s, w, e = p[..., :-2, 1:-1], p[..., 2:, 1:-1], p[..., 1:-1, :-2], p[..., 1:-1, 2:]
    nw, ne, sw, se = p[..., :-2, :-2], p[..., :-2, 2:], p[..., 2:, :-2], p[..., 2:, 2:]
    with np.errstate(all="ignore"):
        near = f32(4) * c - f32(2) * ((n + s) + (w + e))
        if not corners:
            return near.astype(f32)
        return (near + ((nw + ne) + (sw + se))).astype(f32)


def bins_of(r):
    """fp32 responses -> (bin of each, counted mask): q = min(floor(|r| * 4096), 4095); a response that is not finite is not counted"""
    r = np.asarray(r, f32)
    ok = np.isfinite(r)
    with np.errstate(all="ignore"):
        t = np.abs(r) * f32(4096)
    q = np.minimum(np.floor(np.where(ok, t, 0)), BINS - 1).astype(np.int64)
    return q, ok


def histogram(x, picture=None, channels=3, mutant=None):
    """x: fp32 [T, C, Hp, Wp] -> int64 [T, 4096].  picture = (H, W): the top-left part of each plane that is sampled (default: all of it)."""
    x = np.asarray(x, f32)
    T, C, Hp, Wp = x.shape
    H, W = picture if picture is not None else (Hp, Wp)
    if mutant == "pad_sampled":
        H, W = Hp, Wp
    assert 3 <= H <= Hp and 3 <= W <= Wp and channels <= C
    p = x[:, :channels, :H, :W]
    if mutant == "border_included":                                    # the border pixels too, with the picture repeated beyond its edge
        p = np.pad(p, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
    r = response(p, corners=mutant != "no_corners")
    q, ok = bins_of(r)
    hist = np.zeros((T, BINS), np.int64)
    for t in range(T):
        hist[t] = np.bincount(q[t][ok[t]], minlength=BINS)
    if mutant == "frames_pooled":
        hist[:] = hist.sum(0, keepdims=True)
    return hist


def finish(hist, gain=1.0, lo=0.0, hi=SIGMA_MAX):
    """int [T, 4096] -> fp32 [T]: N = sum, k = first bin with 2 cum[k] >= N, med = k + (N - 2 before) / (2 h[k]) in float64,
    sigma = med * K * gain clamped to [lo, hi] (the three taken as fp32 values), to fp32; N == 0 gives lo"""
    hist = np.asarray(hist).astype(np.int64)
    gain, lo, hi = float(f32(gain)), float(f32(lo)), float(f32(hi))
    out = np.empty(hist.shape[0], f32)
    for t, h in enumerate(hist):
        N = int(h.sum())
        if N == 0:
            out[t] = f32(lo)
            continue
        cum = np.cumsum(h)
        k = int(np.argmax(2 * cum >= N))
        before = int(cum[k] - h[k])
        med = np.float64(k) + np.float64(N - 2 * before) / np.float64(2 * int(h[k]))
        s = med * np.float64(K)
        s = s * np.float64(gain)
        out[t] = f32(min(max(s, np.float64(lo)), np.float64(hi)))
    return out


def estimate(x, picture=None, gain=1.0, clamp=(0.0, SIGMA_MAX), channels=3, mutant=None):
    """-> (sigma fp32 [T], hist int64 [T, 4096])"""
    hist = histogram(x, picture, channels, mutant)
    if mutant == "mean":                                               # Immerkaer's mean of |r| instead of the median, from the same bins
        centre = (np.arange(BINS) + 0.5) / 4096
        N = np.maximum(hist.sum(1), 1)
        s = (hist * centre).sum(1) / N * np.sqrt(np.pi / 2) / 6 * float(f32(gain))
        return np.clip(s, float(f32(clamp[0])), float(f32(clamp[1]))).astype(f32), hist
    return finish(hist, gain, clamp[0], clamp[1]), hist


MUTANTS = ("no_corners", "border_included", "pad_sampled", "frames_pooled", "mean")


# ---------------------------------------------------------------------------------------------------
# seeded synthetic scenes, uint8-quantised like a decoded frame

def scene(kind, H, W, seed=0):
    """clean RGB scene in [0,1], float64 [3, H, W]: 'smooth' (ramps), 'mixed' (ramps, an edge, a textured half), 'texture' (a fine two-dimensional sinusoid, 7 x 9 pixels a period)"""
    rs = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([0.2 + 0.6 * xx / max(W - 1, 1), 0.2 + 0.6 * yy / max(H - 1, 1), 0.8 - 0.3 * (xx + yy) / max(H + W - 2, 1)])
    if kind == "smooth":
        return ramp
    ph = rs.uniform(0, 2 * np.pi, (3, 2, 1, 1))
    tex = 0.5 + 0.05 * np.sin(0.9 * xx + ph[:, 0]) * np.sin(0.7 * yy + ph[:, 1])
    if kind == "texture":
        return np.clip(tex, 0, 1)
    if kind == "mixed":
        out = ramp.copy()
        out[:, :, W // 2:] = np.clip(tex[:, :, W // 2:], 0, 1)
        out[:, H // 3:H // 3 + 2, :] = 0.9
        return out
    raise ValueError(kind)


def noisy_u8(clean, sigma255, seed=0):
    """clean [.., H, W] in [0,1] + AWGN of sigma255 / 255, rounded and clipped to uint8"""
    rs = np.random.default_rng(seed)
    v = clean * 255.0 + sigma255 * rs.standard_normal(clean.shape)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def to_f32(u8):
    """uint8 codes -> the fp32 the conversion kernels make of them: code * (1 / 255) in fp32"""
    return (u8.astype(f32) * f32(1.0 / 255.0)).astype(f32)


# ---------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_sigma.py (built here so that tests/test_sigma_cpu.py can show that each mutant differs on them)

def _noisy(T, H, W, sigmas, seed, kind="mixed"):
    """[T, 4, H, W]: uint8-derived noisy frames of one scene, frame t at sigmas[t % len] / 255; plane 3 (the sigma plane) zero"""
    x = np.zeros((T, 4, H, W), f32)
    for t in range(T):
        x[t, :3] = to_f32(noisy_u8(scene(kind, H, W, seed + t), sigmas[t % len(sigmas)], seed + 100 + t))
    return x


def _in_tensor(pic, Hp, Wp, outside):
    """pic [T, 4, H, W] placed top-left in [T, 4, Hp, Wp]; everything else, and the whole sigma plane, is `outside` (a value or 'random')"""
    T, C, H, W = pic.shape
    if isinstance(outside, str):
        x = np.random.default_rng(H * 1000 + W).uniform(0, 1, (T, C, Hp, Wp)).astype(f32)
    else:
        x = np.full((T, C, Hp, Wp), outside, f32)
    x[:, :3, :H, :W] = pic[:, :3]
    return x


def gpu_cases():
    """name -> (x fp32 [T, 4, Hp, Wp], picture (H, W) or None).  Shapes: one sample per plane; 4 x 4; two frames; heights with BAND - 1, BAND,
    BAND + 1 and 2 BAND + 1 rows in all and as interior rows; widths around the float4 (67: a row that cannot move as float4); pictures inside
    larger tensors on the float4 and on the scalar path.  Contents: noisy frames at three sigma, a constant frame, a 0 / 1 checkerboard,
    dyadic values, NaN and +-Inf inside the picture, five different frames."""
    cases = {}
    for H, W in ((3, 3), (4, 4)):
        cases["shape_1x%dx%d" % (H, W)] = (_noisy(1, H, W, [10], 1), None)
    cases["shape_2x12x20"] = (_noisy(2, 12, 20, [10, 25], 2), None)
    for H in sorted({BAND - 1, BAND, BAND + 1, 2 * BAND + 1, BAND + 1, BAND + 2, BAND + 3, 2 * BAND + 3}):
        cases["height_%d" % H] = (_noisy(1, H, 20, [10], 3 + H), None)
    for W in (3, 5, 8, 67):
        cases["width_%d" % W] = (_noisy(1, 12, W, [10], 20 + W), None)
    pic = _noisy(2, 37, 53, [10, 30], 40)
    cases["pad_nan_37x53_in_40x56"] = (_in_tensor(pic, 40, 56, np.nan), (37, 53))
    cases["pad_finite_37x53_in_40x56"] = (_in_tensor(pic, 40, 56, "random"), (37, 53))
    cases["pad_scalar_5x6_in_7x9"] = (_in_tensor(_noisy(1, 5, 6, [10], 41), 7, 9, "random"), (5, 6))
    cases["noisy_three_sigma"] = (_noisy(3, 24, 40, [5, 30, 50], 50), None)
    const = np.zeros((1, 4, 24, 40), f32)
    const[:, :3] = f32(0.5)
    cases["constant"] = (const, None)
    yy, xx = np.mgrid[0:24, 0:40]
    board = np.zeros((1, 4, 24, 40), f32)
    board[:, :3] = ((yy + xx) & 1).astype(f32)
    cases["checkerboard"] = (board, None)
    dy = np.zeros((2, 4, 24, 40), f32)
    dy[:, :3] = (np.random.default_rng(60).integers(0, 1 << 14, (2, 3, 24, 40)) * 2.0 ** -14).astype(f32)
    dy[1, :3] = (dy[1, :3] * f32(2.0 ** -6)).astype(f32)            # |r| * 4096 around small integers too
    cases["dyadic"] = (dy, None)
    bad = _noisy(2, 24, 40, [10, 20], 70)
    rs = np.random.default_rng(71)
    for v in (np.nan, np.inf, -np.inf):
        for _ in range(6):
            bad[rs.integers(2), rs.integers(3), rs.integers(24), rs.integers(40)] = v
    cases["nan_inf"] = (bad, None)
    cases["five_frames"] = (_noisy(5, 24, 40, [2, 10, 20, 30, 40], 80, kind="texture"), None)
    cases["five_frames_again"] = (_noisy(5, 24, 40, [40, 5, 15, 25, 35], 90), None)
    return cases
