"""numpy model of the device's variance-stabilising transform (include/bsvd_hip.h, bsvd_vst_build / bsvd_vst_forward / bsvd_vst_inverse;
bsvd_amd/csrc/frame_vst_items.h), written from the definition line by line: the curve at the interval midpoints in fp32 with the product
rounded before the add, the build in float64 in ascending order with every operation rounded once, forward and inverse in fp32 with
separately rounded operations.  The GPU tests hold the device's tables, forward and inverse to this model bit for bit.  The MUTANTS are the
ways an implementation could plausibly differ; tests/test_vst_cpu.py shows that each one fails a property the true model has."""
import numpy as np

import nlf_model as NM

N = 1024
KNOTS = N + 1
SIGMA_AT, R_AT = KNOTS, KNOTS + 3
TABLE_FLOATS = R_AT + N
FLOOR = 0.5 / 255
FLOOR_MIN = 2.0 ** -10
LEVELS = NM.LEVELS

f32, f64 = np.float32, np.float64

MUTANTS = ("no_midpoint", "r_neighbour", "inverse_lt", "no_floor", "fma")


def midpoint_curve(c, floor=FLOOR, mutant=None):
    """c: 16 values -> s_j, fp32 [1024]: the curve at the interval midpoints, clamped to [floor, 1] (NaN: floor)"""
    c = np.asarray(c, f32)
    assert c.shape == (LEVELS,)
    j = np.arange(N).astype(f32)
    with np.errstate(all="ignore"):
        u = ((j if mutant == "no_midpoint" else j + f32(0.5)) * f32(16.0 / N) - f32(0.5)).astype(f32)
        u = np.where(u >= 15, f32(15), np.where(u >= 0, u, f32(0))).astype(f32)
        i = np.minimum(u.astype(np.int64), LEVELS - 2)
        f = (u - i.astype(f32)).astype(f32)
        d = (c[i + 1] - c[i]).astype(f32)
        fd = (f * d).astype(f32)
        s = (c[i] + fd).astype(f32)
        if mutant != "no_floor":
            s = np.where(s >= f32(floor), s, f32(floor)).astype(f32)
        s = np.where(s <= 1, s, f32(1)).astype(f32)
    return s


def build(c, floor=FLOOR, mutant=None):
    """c: 16 values -> (G fp32 [1025], R fp32 [1024], sigma' fp32)"""
    s = midpoint_curve(c, floor, mutant)
    with np.errstate(all="ignore"):
        w = f64(1.0) / s.astype(f64)
        F = np.zeros(N + 1, f64)
        acc = f64(0.0)
        for j in range(N):                      # ascending, one rounding per add (np.cumsum adds in this order too; the loop says so)
            F[j] = acc
            acc = acc + w[j]
        F[N] = acc
        G = (F / F[N]).astype(f32)
        R = (f64(1.0) / (G[1:].astype(f64) - G[:-1].astype(f64))).astype(f32)
        if mutant == "r_neighbour":
            R = np.concatenate([R[1:], R[-1:]])
        sigma = f32(f64(N) / F[N])
    return G, R, sigma


def tables(c, floor=FLOOR):
    """the device's layout of one table set, fp32 [TABLE_FLOATS]"""
    G, R, sigma = build(c, floor)
    t = np.zeros(TABLE_FLOATS, f32)
    t[:KNOTS], t[SIGMA_AT], t[R_AT:] = G, sigma, R
    return t


def forward(x, G, mutant=None):
    """x fp32 [...] -> fp32 [...]"""
    x = np.asarray(x, f32)
    G = np.asarray(G, f32)
    with np.errstate(all="ignore"):
        t = (x * f32(N)).astype(f32)
        k = np.where(t >= N - 1, N - 1, np.where(t >= 0, np.where(t >= 0, np.minimum(t, N - 1), 0).astype(np.int64), 0)).astype(np.int64)
        fr = (t - k.astype(f32)).astype(f32)
        g0 = G[k]
        d = (G[k + 1] - g0).astype(f32)
        if mutant == "fma":
            return (fr.astype(f64) * d.astype(f64) + g0.astype(f64)).astype(f32)
        fd = (fr * d).astype(f32)
        return (g0 + fd).astype(f32)


def inverse(y, G, R, mutant=None):
    """y fp32 [...] -> fp32 [...]"""
    y = np.asarray(y, f32)
    G, R = np.asarray(G, f32), np.asarray(R, f32)
    with np.errstate(all="ignore"):
        # the largest k in 0 .. 1023 with G[k] <= y; none (or NaN): 0
        side = "left" if mutant == "inverse_lt" else "right"
        k = np.searchsorted(G[:N], np.where(np.isnan(y), f32(-np.inf), y), side=side).astype(np.int64) - 1
        k = np.clip(k, 0, N - 1)
        d = (y - G[k]).astype(f32)
        p = (d * R[k]).astype(f32)
        s = (k.astype(f32) + p).astype(f32)
        return (s * f32(1.0 / N)).astype(f32)


def harmonic_sigma(c, floor=FLOOR):
    """float64 harmonic mean of the clamped curve over the 1024 midpoints, summed pairwise: what sigma' equals to fp32 rounding"""
    s = midpoint_curve(c, floor).astype(f64)
    return f64(N) / np.sum(f64(1.0) / s)


# ---------------------------------------------------------------------------------------------------
# the curves and values of the tests

def curves(seed=11):
    """name -> 16 fp32 values: flat, from_model (nlf_model's A, B), random, step (eight levels 0, eight SIGMA_MAX), all-zero"""
    rs = np.random.default_rng(seed)
    return {
        "flat": np.full(LEVELS, 10.0 / 255, f32),
        "from_model": NM.true_curve().astype(f32),
        "random": rs.uniform(0.0, NM.SIGMA_MAX, LEVELS).astype(f32),
        "step": np.concatenate([np.zeros(8), np.full(8, NM.SIGMA_MAX)]).astype(f32),
        "zero": np.zeros(LEVELS, f32),
    }


SPECIALS = np.array([-0.1, 1.1, np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0, 1e-40, -1e-40, 1.4e-45], f32)


def knot_values(G=None):
    """every knot j / 1024 (or, for the inverse, every knot value G[j]) and its two fp32 neighbours, fp32 [3 * 1025]"""
    k = (np.arange(KNOTS) / N).astype(f32) if G is None else np.asarray(G, f32)
    return np.concatenate([np.nextafter(k, f32(-np.inf)), k, np.nextafter(k, f32(np.inf))]).astype(f32)


def inverse_values(n, seed, G):
    """``test_values`` for the inverse of the table G: its own knot values +- 1 ulp stand where the knots j / 1024 +- 1 ulp stood"""
    return test_values(n, seed, G)


def test_values(n, seed, G=None):
    """fp32 [n]: uniform in [-0.1, 1.1] seeded with the special values and every knot +- 1 ulp (as many as fit)"""
    rs = np.random.default_rng(seed)
    v = rs.uniform(-0.1, 1.1, n).astype(f32)
    extra = np.concatenate([SPECIALS, knot_values(G)])
    rs.shuffle(extra[len(SPECIALS):])
    m = min(n, len(extra))
    at = rs.permutation(n)[:m]
    v[at] = extra[:m]
    return v
