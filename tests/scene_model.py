"""Numpy model of the scene-cut detector (csrc/frame_scene.hip, bsvd_amd.frame_io.scene_scores / scene_cuts), written from the
definition: integers throughout, the score in float64.  The GPU tests hold the device's grids and sums to it bit for bit."""
import numpy as np

import sigma_model

BLOCK = 16
L_MAX = 1020                    # qR + 2 qG + qB at q = 255


def grid(x, picture=None):
    """x: fp32 [T, C >= 3, Hp, Wp] -> int64 [T, GH, GW]: the sum of L = qR + 2 qG + qB over each full 16 x 16 block of the picture
    (H, W) = the top-left part of every plane; q = clamp(rint(255 v), 0, 255) with round-half-even, NaN -> 0"""
    x = np.asarray(x, np.float32)
    T, C, Hp, Wp = x.shape
    H, W = (Hp, Wp) if picture is None else picture
    GH, GW = H // BLOCK, W // BLOCK
    v = x[:, :3, :GH * BLOCK, :GW * BLOCK] * np.float32(255.0)
    q = np.clip(np.rint(np.where(np.isnan(v), np.float32(0), v)), 0, 255).astype(np.int64)
    L = q[:, 0] + 2 * q[:, 1] + q[:, 2]
    return L.reshape(T, GH, BLOCK, GW, BLOCK).sum(axis=(2, 4))


def sad(g, prev=None):
    """int64 [T]: sum |g[t] - g[t-1]|; ``prev`` stands in for the frame before g[0] (None: sad[0] = 0)"""
    g = np.asarray(g, np.int64)
    first = g[:1] if prev is None else np.asarray(prev, np.int64)[None]
    return np.abs(g - np.concatenate([first, g[:-1]])).reshape(g.shape[0], -1).sum(axis=1)


def mafd(sad_, blocks):
    return 100.0 * np.asarray(sad_, np.float64) / (blocks * BLOCK * BLOCK * L_MAX) if blocks else np.zeros(len(sad_))


def scores(mafd_, prev_mafd=0.0):
    """score[t] = min(mafd[t], |mafd[t] - mafd[t-1]|), mafd before the first pair taken as ``prev_mafd``"""
    m = np.asarray(mafd_, np.float64)
    before = np.concatenate([[prev_mafd], m[:-1]])
    return np.minimum(m, np.abs(m - before))


def cuts(x, threshold=10.0, picture=None):
    g = grid(x, picture)
    s = scores(mafd(sad(g), g.shape[1] * g.shape[2]))
    return [int(t) for t in np.nonzero(s >= threshold)[0]], s


def margin_clip(Hh=64, Ww=96, lengths=(4, 5, 4, 6, 4), seed=0, sigma255=50.0):
    """five scenes, each a random field constant on 16-pixel blocks, uint8 with white noise: ([T,4,H,W] fp32, starts).  A block's value is
    uniform in [0,1] and the same in the three planes: that is what the margin's derivation (E|a - b| = 1/3 at a cut, mafd ~ 33) describes.
    With a value of its own per plane L = R + 2G + B averages three of them and mafd at a cut is ~ 20 (measured 13.7 ... 22.2 at 32 x 48),
    too close to twice the threshold to serve as a clip with a margin."""
    rs = np.random.default_rng(seed)
    frames, starts, t = [], [], 0
    for n in lengths:
        starts.append(t)
        clean = np.kron(np.repeat(rs.uniform(0.0, 1.0, (1, Hh // 16, Ww // 16)), 3, axis=0), np.ones((16, 16)))
        for _ in range(n):
            f = np.zeros((4, Hh, Ww), np.float32)
            f[:3] = sigma_model.to_f32(sigma_model.noisy_u8(clean, sigma255, seed=1000 * seed + t))
            f[3] = np.float32(sigma255 / 255.0)
            frames.append(f)
            t += 1
    return np.stack(frames), starts
