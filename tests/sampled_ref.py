"""References of one fused layer at CHOSEN output pixels, for TESTS ONLY: plain torch / numpy indexing around the unchanged CPU models.

A 3 x 3 convolution is local, so what tests/chain_exec.py (the bits of the exact-fp32 mode), tests/split_model.py (the float64 models of
BSVD_F16X3, direct form and Winograd forms) and tests/f16_model.py (BSVD_F16) say of a 2160 x 3840 launch can be had at a few hundred of
its output pixels in seconds: tests/test_gpu_geometry.py holds the layer launches of the shipped geometries to them, and
tests/test_sampled_ref_cpu.py holds THIS module to the full-tensor models (equivalence at every pixel, mutants of the harness).

Unit.  What one reference evaluation needs around an output position (f, y, x) of the conv's own output grid (Ho x Wo; a PixelShuffle layer
writes the four sub-pixels (2y + sy, 2x + sx) of it): the (2r + 1)-row, (n + 2r)-column input neighbourhood with all Cin channels -- r = 1,
or 2 for the two-conv launches; n = 1, or the m outputs of a Winograd pixel group -- gathered with plain indexing from the launch's own
tensors (device or host) and brought to the host.  Channels come from frames f + 1 / f - 1 / f by the fold rule of include/bsvd_hip.h: the
neighbour frame inside the launch, else the halo (compact slice or full frame), else zeros.  Positions outside the image are WRITTEN as
zeros (gather with clamped indices, then mask).  The matching elements of `extra` come along: the skip values of the four sub-pixels
(PS_ADD), the base's leading channels (RESID).

Atlas.  The units lie side by side in one small NHWC tensor [1, 2r + 1, Wa, Cin], on which the model functions run UNCHANGED with a copy of
the layer's spec that has stride 1 and no temporal shift (the gather is done); only the centre outputs are read back.
  - stride 2: output (y, x) is the stride-1 centre of the neighbourhood around input (2y, 2x) -- the same nine taps, the same chain order.
  - direct form: unit i sits at atlas columns 3i .. 3i + 2 (5i .. 5i + 4 for r = 2), centre 3i + 1; units never read each other because each
    carries its whole neighbourhood, and the atlas's own zero padding is never read by a centre.
  - Winograd forms: a unit is a whole pixel group -- m outputs, m + 2 input columns -- at atlas column m (2i + 1), a multiple of m and two
    groups from its neighbours, so that the models' grouping from the image origin (split_model._wino: group q = columns q m ..) is the
    kernel's; groups at the image's ends carry their zeros, and outputs right of the image are not compared.
  - two-conv launches (fused entry head_w_packed, fused pair pre_w_packed; r = 2): the two model stages run separately and the tensor between
    them is ZEROED where it lies outside the image -- that is the contract ("zero outside the image"), and it is not what an atlas gives by
    itself: there the first conv has produced act(bias + ...) from the unit's zeros.
  - the yardsticks (split_model.fp32_chain, wino_fp32) run on the same atlas and their error is taken over the centre outputs only: never
    larger than split_model.chain_err / wino_err over the atlas, so the margins M_DIRECT / M_WINO are asked of no less.

Sample set.  `sample_set` is a seeded, deterministic function of (Ho, Wo, T, tile levels of the launched variant, fold): the corners of the
first and last frame, runs along the four borders, both sides of the first seam / the last seam between full tiles / the seam before the
ragged last tile of every tile level (workgroup tile, wave tile, MFMA tile, Winograd group: `tile_levels` reads them off the name
bsvd_conv3x3_variant gives) on both axes, the last row band (the folded band of the Winograd grid where Ho mod 16 is 1 .. 8), the last pixel
of the last frame, first and last frame where fold > 0, then seeded interior positions up to the cap.  The mandatory classes are never cut.
"""
import dataclasses
import re
import zlib
from types import SimpleNamespace

import numpy as np
import torch

import split_model as S

EPI_PLAIN, EPI_PS_ADD, EPI_RESID = 0, 1, 2
CAP = 4096                 # units per case, at most
MUTANTS = ("col_off", "row_off", "fold_swap", "no_border_zeros", "ps_swap", "wino_misalign", "fused_no_zero")

# ---------------------------------------------------------------------------------------------------------------------------------------
# tile levels of a variant, in pixels of the conv's output grid


def tile_levels(variant):
    """[(rows, columns)] of the tile levels of the kernel `variant` names (bsvd_conv3x3_variant), outermost first.
    conv3x3_kernel<MT,NT,WM,WN,S> (conv3x3_mfma.hip, ConvCfg): workgroup 2 MT WM x 16, wave 2 MT x 16, one 32-pixel MFMA tile 2 x 16.
    winox_kernel<F(m,3),..> (conv3x3_winox.hip, XCfg): workgroup 16 (8 with "[8 rows]") x 8 m, MFMA tile 4 x 8 m, pixel group 1 x m.
    head_kernel 4 x 64, tail_kernel 32 x 16 (tests/chain_exec.py)."""
    g = re.match(r"conv3x3_kernel<(\d+),(\d+),(\d+),(\d+),(\d+)>", variant)
    if g:
        mt, _, wm, _, _ = (int(v) for v in g.groups())
        return [(2 * mt * wm, 16), (2 * mt, 16), (2, 16)]
    g = re.match(r"winox_kernel<F\((\d),3\)", variant)
    if g:
        m = int(g.group(1))
        return [(8 if "[8 rows]" in variant else 16, 8 * m), (4, 8 * m), (1, m)]
    if variant.startswith("head_kernel"):
        return [(4, 64)]
    if variant.startswith("tail_kernel"):
        return [(32, 16)]
    raise ValueError("no tile table for %r" % variant)


def wino_m_of(variant):
    g = re.match(r"winox_kernel<F\((\d),3\)", variant)
    return int(g.group(1)) if g else 0


def seams(n, t):
    """the seams of an axis of n pixels under tiles of t: the first, the last between two full tiles, the one before the ragged last tile"""
    s = set()
    if t < n:
        s.add(t)
    k = n // t
    if k >= 2:
        s.add((k - 1) * t)
    if n % t and k >= 1:
        s.add(k * t)
    return sorted(s)


def seam_sides(n, t):
    return sorted({p for s in seams(n, t) for p in (s - 1, s)})


def sample_set(Ho, Wo, T, levels, fold=0, cap=CAP, seed=0, group=1):
    """(positions [N, 3] int64 of (f, y, x) on the conv's output grid, number of mandatory ones).  group = m: one position per Winograd
    pixel group (a unit is the whole group).  See the module docstring for the classes."""
    rs = np.random.RandomState(zlib.crc32(repr((Ho, Wo, T, tuple(levels), fold, seed)).encode()) & 0x7FFFFFFF)
    fl = T - 1
    pts = []
    for f in sorted({0, fl}):
        pts += [(f, 0, 0), (f, 0, Wo - 1), (f, Ho - 1, 0), (f, Ho - 1, Wo - 1)]
    pts.append((fl, Ho - 1, Wo - 1))
    for f in sorted({0, fl}) if fold else [fl]:
        Lx, Ly = min(8, Wo), min(8, Ho)
        x0, y0 = int(rs.randint(0, Wo - Lx + 1)), int(rs.randint(0, Ho - Ly + 1))
        for xs in (range(x0, x0 + Lx), range(Wo - Lx, Wo)):
            pts += [(f, 0, x) for x in xs] + [(f, Ho - 1, x) for x in xs]
        for ys in (range(y0, y0 + Ly), range(Ho - Ly, Ho)):
            pts += [(f, y, 0) for y in ys] + [(f, y, Wo - 1) for y in ys]
    for th, tw in levels:
        Ys, Xs = seam_sides(Ho, th), seam_sides(Wo, tw)
        xa, ya = [0, int(rs.randint(0, Wo)), Wo - 1], [0, int(rs.randint(0, Ho)), Ho - 1]
        pts += [(fl, y, x) for y in Ys for x in Xs + xa]
        pts += [(fl, y, x) for x in Xs for y in ya]
        if fold and fl:
            pts += [(0, y, x) for y in Ys for x in xa[1:2]] + [(0, y, x) for x in Xs for y in ya[1:2]]
    th, tw = levels[0]
    yb = (Ho - 1) // th * th
    for y in sorted({yb, Ho - 1}):
        pts += [(fl, y, x) for x in seam_sides(Wo, tw) + seam_sides(Wo, 2 * tw) + [0, Wo - 1]]
    key = lambda p: (p[0], p[1], p[2] // group)
    seen, out = set(), []
    for p in pts:
        if key(p) not in seen:
            seen.add(key(p))
            out.append(p)
    mandatory = len(out)
    tries = 0
    while len(out) < cap and tries < 8 * cap and len(seen) < T * Ho * ((Wo + group - 1) // group):
        p = (int(rs.randint(0, T)), int(rs.randint(0, Ho)), int(rs.randint(0, Wo)))
        tries += 1
        if key(p) not in seen:
            seen.add(key(p))
            out.append(p)
    return np.array(out, dtype=np.int64).reshape(-1, 3), mandatory


def all_positions(T, Ho, Wo, group=1):
    """every unit of a small tensor (the CPU equivalence tests)"""
    f, y, x = np.meshgrid(np.arange(T), np.arange(Ho), np.arange(0, Wo, group), indexing="ij")
    return np.stack([f.ravel(), y.ravel(), x.ravel()], axis=1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------------
# gathering units


def _decode(raw, codec):
    """gathered vectors [..., C] on any device -> (hi, lo) float64 numpy; codec 'f32': plain values, lo is None"""
    raw = raw.cpu()
    if codec == "f32":
        return raw.numpy().astype(np.float64), None
    return S.halves(raw)


def _take(src, iy, ix, inside):
    """src [H, W, C] (any strides); iy [N, R, 1], ix [N, 1, Q] input coordinates; inside [N, R, Q] -> [N, R, Q, C], zeros outside"""
    H, W = src.shape[:2]
    v = src[iy.clamp(0, H - 1).expand(-1, -1, ix.shape[2]), ix.clamp(0, W - 1).expand(-1, iy.shape[1], -1)]
    if inside is None:
        return v
    return torch.where(inside[..., None], v, torch.zeros((), dtype=v.dtype, device=v.device))


def _halo_frame(h, H, W, fold, which):
    """(tensor [H, W, Cx] of a Halo, first logical channel of the slice inside it).  Compact slice: pstride == fold, the slice is the tensor;
    a full frame: coff = fold (halo_prev) resp. 0 (halo_next) names the slice's channels."""
    t = h.t.reshape(H, W, h.pstride)
    if h.pstride == fold:
        assert h.coff == 0
        return t, 0
    assert h.coff == (fold if which == "prev" else 0), "a neighbour frame is passed with coff = fold resp. 0"
    return t, h.coff


def gather_units(sp, x, pos, *, m=0, halo_prev=None, halo_next=None, extra=None, extra_pstride=0, extra_cstride=1, x_planar=False,
                 codec="f32", extra_codec="f32", radius=1, mutate=None):
    """The units of output positions `pos` ([N, 3] of (f, y, x), conv output grid) of ONE launch of layer `sp` on input x ([T, H, W, Cin_pad],
    or planar [T, C, H, W]).  m: the Winograd form's group size (0: one output per unit).  codec: 'f32' (plain fp32 tensors) or 'split' (split16
    containers), extra_codec likewise.  Returns a namespace: pos (x moved to its group's first column), n (outputs per unit), r, hi / lo
    [N, 2r + 1, n + 2r, Cin_pad] float64 (lo None for 'f32'), valid [N, n] (outputs inside the image), extra [N, ny, nx, Ce] float64 or None,
    inside2 [N, 3, n + 2] (r == 2: where the tensor between the two convs lies inside the image)."""
    pos = torch.as_tensor(np.asarray(pos), dtype=torch.int64)
    dev = x.device
    n = m if m else 1
    r = radius
    if x_planar:
        T, C, H, W = x.shape
        frame = lambda f: x[f].permute(1, 2, 0)
    else:
        T, H, W, C = x.shape
        frame = lambda f: x[f]
    s = sp.stride
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    f, y = pos[:, 0], pos[:, 1]
    x0 = pos[:, 2] // n * n
    pos = torch.stack([f, y, x0], dim=1)
    iy = (y * s)[:, None, None] + torch.arange(-r, r + 1)[None, :, None]                    # [N, R, 1]
    ix = (x0 * s)[:, None, None] + torch.arange(-r, n + r)[None, None, :]                   # [N, 1, Q]   (stride 2 only with n == 1)
    if mutate == "col_off":
        ix = ix + 1
    if mutate == "row_off":
        iy = iy + 1
    inside = ((iy >= 0) & (iy < H)) & ((ix >= 0) & (ix < W))
    fold = sp.fold if sp.tsm else 0
    N, R, Q = pos.shape[0], 2 * r + 1, n + 2 * r
    hi = np.zeros((N, R, Q, C))
    lo = None if codec == "f32" else np.zeros((N, R, Q, C))
    iyd, ixd, ind = iy.to(dev), ix.to(dev), (None if mutate == "no_border_zeros" else inside.to(dev))
    for fr in sorted(set(int(v) for v in f)):
        sel = (f == fr).nonzero()[:, 0]
        seld = sel.to(dev)
        take = lambda src: _decode(_take(src, iyd[seld], ixd[seld], None if ind is None else ind[seld]), codec)
        h, l = take(frame(fr))
        if fold:
            nxt = (frame(fr + 1), 0) if fr + 1 < T else (None if halo_next is None else _halo_frame(halo_next, H, W, fold, "next"))
            prv = (frame(fr - 1), fold) if fr > 0 else (None if halo_prev is None else _halo_frame(halo_prev, H, W, fold, "prev"))
            ranges = {"next": slice(0, fold), "prev": slice(fold, 2 * fold)}
            if mutate == "fold_swap":
                ranges = {"prev": slice(0, fold), "next": slice(fold, 2 * fold)}
            for which, srcc in (("next", nxt), ("prev", prv)):
                dst = ranges[which]
                if srcc is None:
                    h[..., dst] = 0.0
                    if l is not None:
                        l[..., dst] = 0.0
                    continue
                sh, sl = take(srcc[0])
                h[..., dst] = sh[..., srcc[1]:srcc[1] + fold]
                if l is not None:
                    l[..., dst] = sl[..., srcc[1]:srcc[1] + fold]
        hi[sel.numpy()] = h
        if lo is not None:
            lo[sel.numpy()] = l
    u = SimpleNamespace(pos=pos.numpy(), n=n, r=r, hi=hi, lo=lo, Ho=Ho, Wo=Wo, T=T, extra=None, x_planar=x_planar,
                        valid=((x0[:, None] + torch.arange(n)[None, :]) < Wo).numpy(), inside2=None, mutate=mutate)
    if r == 2:
        my, mx = y[:, None, None] + torch.arange(-1, 2)[None, :, None], x0[:, None, None] + torch.arange(-1, n + 1)[None, None, :]
        u.inside2 = (((my >= 0) & (my < H)) & ((mx >= 0) & (mx < W))).numpy()
    if extra is not None and sp.epilogue in (EPI_PS_ADD, EPI_RESID):
        u.extra = _gather_extra(sp, extra, extra_pstride, extra_cstride, extra_codec, pos, n, Ho, Wo)
    return u


def _gather_extra(sp, extra, eps, ecs, codec, pos, n, Ho, Wo):
    """the epilogue's second operand at the units' outputs, decoded: PS_ADD [N, 2, 2n, cq] (skip laid out like y), RESID [N, 1, n, k]"""
    dev = extra.device
    f, y, x0 = pos[:, 0], pos[:, 1], pos[:, 2]
    fstride = extra[0].numel()
    flat = extra.reshape(-1)
    if sp.epilogue == EPI_PS_ADD:
        k = sp.cout // 4
        oy = (2 * y)[:, None, None] + torch.arange(2)[None, :, None]
        ox = (2 * x0)[:, None, None] + torch.arange(2 * n)[None, None, :]
        pix = oy * (2 * Wo) + ox.clamp(max=2 * Wo - 1)
    else:
        k = min(3, sp.cout)
        pix = (y[:, None, None] * Wo + (x0[:, None, None] + torch.arange(n)[None, None, :]).clamp(max=Wo - 1))
    base = f[:, None, None] * fstride + pix * eps                                           # [N, ny, nx]
    if ecs == 1:          # a pixel's channels are contiguous: whole vectors (a split16 container decodes per 16-channel chunk)
        idx = base[..., None] + torch.arange(eps)[None, None, None, :]
        h, l = _decode(flat[idx.to(dev)], codec)
        return (h if l is None else h + l)[..., :k]
    assert codec == "f32", "a planar base is plain fp32"
    idx = base[..., None] + (torch.arange(k) * ecs)[None, None, None, :]
    return flat[idx.to(dev)].cpu().numpy().astype(np.float64)


def gather_outputs(sp, y, u, codec="f32", y_planar=False):
    """the launch's results at the units' outputs, as stored: (values float64 [N, ny, nx, Cy], hi, lo of a split16 y or None, None).
    ny x nx = 1 x n, or 2 x 2n for a PixelShuffle layer; outputs right of the image read as zeros."""
    dev = y.device
    pos = torch.as_tensor(u.pos)
    f, yy, x0 = pos[:, 0], pos[:, 1], pos[:, 2]
    k = 2 if sp.epilogue == EPI_PS_ADD else 1
    oy = (k * yy)[:, None, None] + torch.arange(k)[None, :, None]
    ox = (k * x0)[:, None, None] + torch.arange(k * u.n)[None, None, :]
    ok = (ox < k * u.Wo).expand(-1, k, -1)
    ox = ox.clamp(max=k * u.Wo - 1)
    ff = f[:, None, None].expand(-1, k, k * u.n)
    src = y.permute(0, 2, 3, 1) if y_planar else y
    raw = src[ff.to(dev), oy.expand(-1, -1, k * u.n).to(dev), ox.expand(-1, k, -1).to(dev)]
    h, l = _decode(raw, codec)
    okn = ok.numpy()[..., None]
    if l is None:
        return np.where(okn, h, 0.0), None, None
    return np.where(okn, h + l, 0.0), np.where(okn, h, 0.0), np.where(okn, l, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the atlas


def _cols(u):
    """atlas column of every unit's first output, atlas width"""
    N = u.pos.shape[0]
    if u.n == 1 and u.r == 1:
        c = 3 * np.arange(N) + 1
        return c, 3 * N
    if u.n == 1:
        c = (2 * u.r + 1) * np.arange(N) + u.r
        return c, (2 * u.r + 1) * N
    assert u.r == 1
    c = u.n * (2 * np.arange(N) + 1) + (1 if u.mutate == "wino_misalign" else 0)
    return c, u.n * (2 * N + 3)


def atlas(u, part="hi"):
    """the units side by side: NHWC [1, 2r + 1, Wa, C] float64 (part 'hi' | 'lo' | 'sum')"""
    c, Wa = _cols(u)
    v = u.hi if part == "hi" else u.lo if part == "lo" else (u.hi if u.lo is None else u.hi + u.lo)
    N, R, Q, C = v.shape
    a = np.zeros((1, R, Wa, C))
    cols = c[:, None] + np.arange(-u.r, u.n + u.r)[None, :]                                  # [N, Q]
    a[0][:, cols.ravel()] = v.transpose(1, 0, 2, 3).reshape(R, N * Q, C)
    return a


def atlas_extra(sp, u):
    """(extra atlas laid out like the model's output on the atlas, extra_pstride) or (None, 0)"""
    if u.extra is None:
        return None, 0
    c, Wa = _cols(u)
    N, ny, nx, k = u.extra.shape
    R = 2 * u.r + 1
    if sp.epilogue == EPI_PS_ADD:
        e = np.zeros((1, 2 * R, 2 * Wa, k))
        cols = 2 * c[:, None] + np.arange(nx)[None, :]
        for sy in range(2):
            e[0, 2 * u.r + sy][cols.ravel()] = u.extra[:, sy].reshape(N * nx, k)
    else:
        e = np.zeros((1, R, Wa, k))
        cols = c[:, None] + np.arange(nx)[None, :]
        e[0, u.r][cols.ravel()] = u.extra[:, 0].reshape(N * nx, k)
    return e, k


def centres(sp, u, out, y_planar=False):
    """the centre outputs of a model's result on the atlas (NHWC, or NCHW with y_planar) -> [N, ny, nx, C], zeros right of the image"""
    out = out.detach().cpu().numpy() if isinstance(out, torch.Tensor) else np.asarray(out)
    if y_planar:
        out = out.transpose(0, 2, 3, 1)
    c, _ = _cols(u)
    k = 2 if sp.epilogue == EPI_PS_ADD else 1
    cols = k * c[:, None] + np.arange(k * u.n)[None, :]                                      # [N, nx]
    rows = k * u.r + np.arange(k)
    if u.mutate == "ps_swap" and k == 2:
        cols = cols.reshape(-1, u.n, 2)[..., ::-1].reshape(-1, 2 * u.n)
    v = out[0][rows[None, :, None], cols[:, None, :]]                                        # [N, ny, nx, C]
    ok = np.repeat(u.valid, k, axis=1)[:, None, :, None]
    return np.where(ok, v, 0.0)


def atlas_spec(sp):
    """the layer on the atlas: stride 1 (an output is the centre of its neighbourhood), no temporal shift (the gather is done)"""
    return dataclasses.replace(sp, stride=1, tsm=False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the models on the atlas


def eval_chain(st, sp, u, y_planar=None):
    """the exact-fp32 mode: chain_exec.ChainExecutor on the atlas -> the bits of the units' outputs, float32 [N, ny, nx, C]"""
    from chain_exec import ChainExecutor
    sp1 = atlas_spec(sp)
    a = torch.from_numpy(atlas(u).astype(np.float32))
    e, eps = atlas_extra(sp, u)
    kw = {}
    if e is not None:
        kw = dict(extra=torch.from_numpy(e.astype(np.float32)), extra_pstride=eps, extra_cstride=1)
    if u.x_planar:
        a = a[..., :sp.cin].permute(0, 3, 1, 2).contiguous()
        kw["x_planar"] = True
    if y_planar is not None:
        kw["y_planar"] = y_planar
    out = ChainExecutor(st).conv(sp1, a, **kw)
    return centres(sp, u, out, y_planar is not None).astype(np.float32)


def _kw_extra(sp, u):
    e, eps = atlas_extra(sp, u)
    return {} if e is None else dict(extra=e, extra_pstride=eps, extra_cstride=1)


def eval_direct(sp, u, w, b, one_pass=False, y_planar=None):
    """the direct form of the split modes on the atlas: (model at the centres, the float32 chain's error at the centres).
    one_pass: BSVD_F16 (f16_model.direct_one_pass; yardstick on the hi operands, as tests/test_gpu_f16.py has it)."""
    import f16_model as F
    sp1 = atlas_spec(sp)
    kw = _kw_extra(sp, u)
    if y_planar is not None:
        kw["y_planar"] = y_planar
    ah, al = atlas(u, "hi"), (atlas(u, "lo") if u.lo is not None else np.zeros_like(atlas(u, "hi")))
    if one_pass:
        model = F.direct_one_pass(sp1, ah, al, w, b, **kw)
        ca, cb = S.fp32_chain(sp1, ah, S.pairs(w)[0], b, **kw)
    else:
        model = S.direct_three_pass(sp1, ah, al, w, b, **kw)
        ca, cb = S.fp32_chain(sp1, ah + al, w, b, **kw)
    pl = y_planar is not None
    err = float(np.abs(centres(sp, u, ca, pl) - centres(sp, u, cb, pl)).max())
    return centres(sp, u, model, pl), err


def eval_wino(sp, u, w, b, m, one_pass=False):
    """a Winograd form on the atlas (x decoded: the kernel decodes before it transforms): (model at the centres, wino_fp32's error there)"""
    import f16_model as F
    assert u.n == m
    sp1 = atlas_spec(sp)
    kw = _kw_extra(sp, u)
    a = atlas(u, "sum")
    model = F.wino_one_pass(sp1, a, w, m, b, **kw) if one_pass else S.wino_model(sp1, a, w, m, b, **kw)
    ca, cb = S.wino_fp32(sp1, a, w, m, b, **kw)
    err = float(np.abs(centres(sp, u, ca) - centres(sp, u, cb)).max())
    return centres(sp, u, model), err


def _zero_outside(u, mid):
    """the tensor between the two convs of a fused launch, on the atlas [1, 5, Wa, C]: zero where it lies outside the image, and outside
    the 3 x (n + 2) window a unit's second conv reads"""
    c, _ = _cols(u)
    keep = np.zeros(mid.shape[1:3], dtype=bool)
    cols = c[:, None] + np.arange(-1, u.n + 1)[None, :]
    for a in range(3):
        keep[u.r - 1 + a, cols.ravel()] = (np.ones_like(u.inside2[:, a]) if u.mutate == "fused_no_zero" else u.inside2[:, a]).ravel()
    return np.where(keep[None, :, :, None], mid, 0.0)


def eval_two_convs(spa, spb, u, wa, ba, wb, bb, one_pass=False, y_planar=None):
    """fused entry / fused pair (r = 2): stage a, the tensor between re-split (zero outside the image), stage b; the yardstick is the two
    float32 chains of tests/test_gpu_split_passes.py (_pair_chain) at the centres.  spb's epilogue may be RESID / the planar exit."""
    import f16_model as F
    assert u.r == 2
    a1, b1 = atlas_spec(spa), atlas_spec(spb)
    kw = _kw_extra(spb, u)
    if y_planar is not None:
        kw["y_planar"] = y_planar
    ah, al = (atlas(u, "hi"), atlas(u, "lo")) if u.lo is not None else S.pairs(atlas(u, "hi"))      # planar fp32 input: split in the kernel
    stage = F.direct_one_pass if one_pass else S.direct_three_pass
    pad = lambda t: np.concatenate([t, np.zeros(t.shape[:-1] + (b1.cin_pad - t.shape[-1],))], axis=-1)
    mid = _zero_outside(u, S._np(stage(a1, ah, al, wa, ba)))[..., :spa.cout]
    mh, ml = S.pairs(mid)
    model = stage(b1, pad(mh), pad(ml), wb, bb, **kw)
    if one_pass:
        ca, cb = S.fp32_chain(b1, pad(mh), S.pairs(wb)[0], bb, **kw)
    else:
        y1c, y1d = S.fp32_chain(a1, ah + al, wa, ba)
        z = lambda t: pad(_zero_outside(u, S._np(t))[..., :spa.cout])
        ca, _ = S.fp32_chain(b1, z(y1c.float().double()), wb, bb, **kw)
        cb = S.conv_f64(b1, z(y1d), wb, bb, **kw)
    pl = y_planar is not None
    err = float(np.abs(centres(spb, u, ca, pl) - centres(spb, u, cb, pl)).max())
    return centres(spb, u, model, pl), err
