"""The film-grain model in numpy, written from the text of include/bsvd_hip.h (bsvd_grain_stats, bsvd_grain_apply) and of
frame_io.grain_from_stats / grain_template's docstrings, independent of the library: the per-pixel terms in np.float32 in the header's
order, the 256 integers of a frame, the fit (with numpy's solver where the product writes its elimination out), the template recursion
pixel by pixel, and the synthesis.  The test model of tests/test_grain_cpu.py and tests/test_gpu_grain.py.

``stats`` and ``apply`` take MUTANT switches -- a dropped lag, an anchor window one column wider than the rule, the level keyed on x instead
of y, block offsets that ignore the frame index -- which tests/test_grain_cpu.py shows the comparisons catch."""
import numpy as np

import finish_model as FM

f32 = np.float32
LEVELS, LAGS, TAPS, STATS = 16, 46, 24, 256
N_AT, S1_AT, S2_AT, A_AT = 0, 16, 64, 112
QSCALE, QMAX = f32(4096.0), 2047
TMPL, BLOCK, OFFSETS = 128, 32, 97
WARMUP, RIDGE = 16, 1e-3
LAG_LIST = [(0, dx) for dx in range(7)] + [(dy, dx) for dy in (1, 2, 3) for dx in range(-6, 7)]
TAP_LIST = [(0, dx) for dx in (1, 2, 3)] + [(dy, dx) for dy in (1, 2, 3) for dx in range(-3, 4)]
LUMA_W = FM.LUMA_W


def weights(matrix="bt709"):
    return tuple(f32(v) for v in LUMA_W[matrix])


def luma(w, R, G, B):
    """fmaf(w_B, B, fmaf(w_G, G, w_R * R))"""
    with np.errstate(all="ignore"):
        return FM.fma32(w[2], B, FM.fma32(w[1], G, (w[0] * np.asarray(R, f32)).astype(f32)))


def level(ly):
    with np.errstate(all="ignore"):
        t = (np.asarray(ly, f32) * f32(16.0)).astype(f32)
        return np.where(t >= 15, 15, np.where(t >= 0, np.floor(np.where(t >= 0, np.minimum(t, 15), 0)), 0)).astype(np.int64)


def pixel_terms(x, y, w, level_from="y"):
    """x, y [..., 3, H, W] float32 -> (l int64 [..., H, W], q int64 [..., 3, H, W], counted bool [..., H, W])"""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    with np.errstate(all="ignore"):
        d = (x - y).astype(f32)
        dR, dG, dB = d[..., 0, :, :], d[..., 1, :, :], d[..., 2, :, :]
        n0 = luma(w, dR, dG, dB)
        n = np.stack([n0, (dB - n0).astype(f32), (dR - n0).astype(f32)], axis=-3)
        src = y if level_from == "y" else x
        l = level(luma(w, src[..., 0, :, :], src[..., 1, :, :], src[..., 2, :, :]))
        counted = np.all(np.isfinite(n), axis=-3)
        t = (n * QSCALE).astype(f32)
        c = np.minimum(np.maximum(t, f32(-QMAX)), f32(QMAX))
        q = np.where(counted[..., None, :, :], np.rint(np.where(np.isfinite(c), c, 0)), 0).astype(np.int64)
    return l, q, counted


def stats(x, y, H=None, W=None, w=None, drop_lag=None, anchor_shift=0, level_from="y"):
    """x, y [T, >= 3, Hp, Wp] -> int64 [T, 256]; only the top-left H x W of the planes is looked at"""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    T, _, Hp, Wp = x.shape
    H, W = Hp if H is None else H, Wp if W is None else W
    w = weights() if w is None else w
    out = np.zeros((T, STATS), np.int64)
    for t in range(T):
        l, q, counted = pixel_terms(x[t, :3, :H, :W], y[t, :3, :H, :W], w, level_from)
        for lv in range(LEVELS):
            m = counted & (l == lv)
            out[t, N_AT + lv] = int(m.sum())
            for k in range(3):
                out[t, S1_AT + 16 * k + lv] = int(q[k][m].sum())
                out[t, S2_AT + 16 * k + lv] = int((q[k][m] ** 2).sum())
        c_lo, c_hi = 6, W - 7 + anchor_shift                                 # anchors 0 <= r <= H - 4, 6 <= c <= W - 7
        if anchor_shift:                                                     # (the mutant's window is wider: zeros beyond the picture)
            q = np.concatenate([q, np.zeros((3, H, anchor_shift), np.int64)], axis=2)
        for k in range(3):
            base = q[k, 0:H - 3, c_lo:c_hi + 1]
            for i, (dy, dx) in enumerate(LAG_LIST):
                if i == drop_lag:
                    continue
                out[t, A_AT + LAGS * k + i] = int((base * q[k, dy:dy + H - 3, c_lo + dx:c_hi + 1 + dx]).sum())
    return out


def stats_brute(x, y, H, W, w=None):
    """the same 256 integers of ONE frame [>= 3, Hp, Wp] by a double loop over the pixels, Python integers throughout"""
    w = weights() if w is None else w
    l, q, counted = pixel_terms(np.asarray(x, f32)[:3, :H, :W], np.asarray(y, f32)[:3, :H, :W], w)
    out = [0] * STATS
    for r in range(H):
        for c in range(W):
            if counted[r, c]:
                lv = int(l[r, c])
                out[N_AT + lv] += 1
                for k in range(3):
                    v = int(q[k, r, c])
                    out[S1_AT + 16 * k + lv] += v
                    out[S2_AT + 16 * k + lv] += v * v
            if r <= H - 4 and 6 <= c <= W - 7:
                for k in range(3):
                    v = int(q[k, r, c])
                    if v:
                        for i, (dy, dx) in enumerate(LAG_LIST):
                            out[A_AT + LAGS * k + i] += v * int(q[k, r + dy, c + dx])
    return np.array(out, np.int64)


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------------
def lag_index(dy, dx):
    if dy < 0 or (dy == 0 and dx < 0):
        dy, dx = -dy, -dx
    return LAG_LIST.index((dy, dx))


def fit(st, anchors, min_count=512):
    """pooled int64 [256] -> (std [3,16], ar [3,24]) in float64, numpy's solver for the 24 x 24 system"""
    st = np.asarray(st, np.int64)
    N = st[N_AT:N_AT + 16].astype(np.float64)
    std, ar = np.zeros((3, LEVELS)), np.zeros((3, TAPS))
    valid = [l for l in range(LEVELS) if N[l] >= min_count]
    for k in range(3):
        s1 = st[S1_AT + 16 * k:S1_AT + 16 * k + 16].astype(np.float64)
        s2 = st[S2_AT + 16 * k:S2_AT + 16 * k + 16].astype(np.float64)
        val = lambda n, a, b: 0.0 if n <= 0 else np.sqrt(max(b / n - (a / n) ** 2, 0.0)) / 4096.0
        for l in range(LEVELS):
            if valid:
                best = min(valid, key=lambda v: (abs(v - l), v))
                std[k, l] = val(N[best], s1[best], s2[best])
            else:
                std[k, l] = val(N.sum(), s1.sum(), s2.sum())
        R = st[A_AT + LAGS * k:A_AT + LAGS * (k + 1)].astype(np.float64) / float(anchors)
        if R[0] > 0:
            M = np.array([[R[lag_index(yi - yj, xi - xj)] for (yj, xj) in TAP_LIST] for (yi, xi) in TAP_LIST])
            M += RIDGE * R[0] * np.eye(TAPS)
            ar[k] = np.linalg.solve(M, np.array([R[lag_index(dy, dx)] for dy, dx in TAP_LIST]))
    return std, ar


def template(ar, seed=0):
    """float32 [3,128,128]: the raster recursion pixel by pixel over seeded white noise, warm-up border cut, / its own std"""
    ar = np.asarray(ar, np.float64).reshape(3, TAPS)
    rows, cols = TMPL + WARMUP, TMPL + 2 * WARMUP
    white = np.random.default_rng(seed).standard_normal((3, rows, cols))
    out = np.empty((3, TMPL, TMPL), f32)
    for k in range(3):
        g = np.zeros((rows + 3, cols + 6))
        taps = [(a, dy, dx) for a, (dy, dx) in zip(ar[k], TAP_LIST) if a != 0.0]
        for r in range(rows):
            for c in range(cols):
                v = white[k, r, c]
                for a, dy, dx in taps:
                    v += a * g[3 + r - dy, 3 + c - dx]
                g[3 + r, 3 + c] = v
        t = g[3 + WARMUP:, 3 + WARMUP:3 + WARMUP + TMPL]
        out[k] = (t / t.std()).astype(f32)
    return out


def acf(ar, n=256):
    """the autocorrelation an AR set implies, at the 24 taps: the inverse transform of 1 / |1 - sum a_j e^{-i w d_j}|^2 on an n x n grid"""
    ar = np.asarray(ar, np.float64).reshape(TAPS)
    k = np.zeros((n, n))
    k[0, 0] = 1.0
    for a, (dy, dx) in zip(ar, TAP_LIST):
        k[dy % n, dx % n] -= a
    S = 1.0 / np.abs(np.fft.fft2(k)) ** 2
    R = np.real(np.fft.ifft2(S))
    return np.array([R[dy % n, dx % n] / R[0, 0] for dy, dx in TAP_LIST])


# ---- the synthesis ---------------------------------------------------------------------------------------------------------------------------
def block_offsets(seed, frame, by, bx):
    """(oy, ox) int64 arrays for block index arrays by, bx of the frame with stream index ``frame``"""
    kf = FM.frame_key(seed, frame, 3)
    p = (np.asarray(bx, np.uint64) + np.asarray(by, np.uint64) * np.uint64(0x9e3779b1)) & np.uint64(0xffffffff)
    h = FM.fmix32(np.uint64(kf) ^ p)
    oy = ((h >> np.uint64(16)) * np.uint64(OFFSETS)) >> np.uint64(16)
    ox = ((h & np.uint64(0xffff)) * np.uint64(OFFSETS)) >> np.uint64(16)
    return oy.astype(np.int64), ox.astype(np.int64)


def scale(ly, std):
    """std [3,16] float32 at u = ly * 16 - 0.5 -> [3, ...] float32"""
    with np.errstate(all="ignore"):
        u = ((np.asarray(ly, f32) * f32(16.0)).astype(f32) - f32(0.5)).astype(f32)
        u = np.where(u >= 15, f32(15), np.where(u >= 0, u, f32(0))).astype(f32)
        i = np.minimum(u.astype(np.int64), 14)
        f = (u - i.astype(f32)).astype(f32)
        out = []
        for k in range(3):
            d = (std[k][i + 1] - std[k][i]).astype(f32)
            out.append((std[k][i] + (f * d).astype(f32)).astype(f32))
    return np.stack(out)


def apply(y, templates, std, amount=1.0, w=None, seed=0, frame0=0, ignore_frame=False):
    """y [T,3,Hp,Wp] float32 -> the frames with grain, float32; amount == 0 or an all-zero std: y itself, untouched"""
    y = np.asarray(y, f32)
    std = np.asarray(std, np.float64).astype(f32).reshape(3, LEVELS)
    amount = f32(amount)
    if amount == 0 or not std.any():
        return y
    w = weights() if w is None else w
    inv_wg = f32(1.0 / float(w[1]))
    templates = np.asarray(templates, f32)
    T, _, Hp, Wp = y.shape
    r, c = np.meshgrid(np.arange(Hp), np.arange(Wp), indexing="ij")
    out = y.copy()
    with np.errstate(all="ignore"):
        for t in range(T):
            oy, ox = block_offsets(seed, 0 if ignore_frame else frame0 + t, r >> 5, c >> 5)
            g = templates[:, oy + (r & 31), ox + (c & 31)]
            s = scale(luma(w, y[t, 0], y[t, 1], y[t, 2]), std)
            n = ((amount * s).astype(f32) * g).astype(f32)
            dR, dB = (n[2] + n[0]).astype(f32), (n[1] + n[0]).astype(f32)
            tt = ((w[0] * dR).astype(f32) + (w[2] * dB).astype(f32)).astype(f32)
            dG = ((n[0] - tt).astype(f32) * inv_wg).astype(f32)
            out[t, 0] = y[t, 0] + dR
            out[t, 1] = y[t, 1] + dG
            out[t, 2] = y[t, 2] + dB
    return out
