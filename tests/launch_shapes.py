"""The launch rules of the frame I/O kernels, restated in plain Python, and the shapes chosen from them for tests/test_gpu_launch_shapes.py.

Every frame I/O kernel is a grid-stride loop around an item body, launched with a capped grid.  The small-shape GPU tests never reach a cap:
every lane runs its loop once.  The cases here are the smallest at which, by the restatement below, a launch runs its loop at least
``TRIPS_MIN`` = 2.3 times, ends in a ragged trip (an item count that is no multiple of the 64 lanes of a wave) and, for the kernels whose
``blockIdx.y`` is the frame, is limited by the cap and not by the item count.

The grid of a launch cannot be observed from outside the library.  The margin is the defence against that: a restatement that is wrong by
up to a factor of two (rows per item, float4 against scalar items) still leaves the real kernel with a second trip, and the chunks of the
launch-shape-independence check are sized to HALF a trip, so they stay single-trip under the same error.

Two shape families.  'frames': many frames of a picture 69 x 126 (70 x 126 for 4:2:0) inside a 72 x 128 tensor for the pad / crop entry
points -- mirror images, rows ending in a 2-column part item -- and 72 x 124 for the plain ones.  'rows': rows 3836 wide, 35 (34) of them
inside 36 x 3840, or 36 x 3836 plain.  The plain uint8 kernels count elements, four planes with the constant channel: 72 x 123 and 33 x 3835.  A row of 3840 or of 128 columns is a whole number of half waves of items, so with an even row count
every total is a multiple of 64 and no trip is ragged: hence 3836 and 124 columns and the odd row counts.

The module needs numpy only (tests/test_launch_shapes_cpu.py runs it without a device): rules, cases, seeded inputs and the model calls."""
import collections
import functools
import itertools

import numpy as np

import finish_model as F
import nlf_model as NM
import rgb_surface_model as R
import scene_model as SC
import sigma_model as SM
import vst_model as VM
import yuv_model as M
import yuv_surface_model as S

f32 = np.float32
TRIPS_MIN = 2.3
WAVE = 64
GIB = 1 << 30
CHUNK_TRIPS = 0.5            # a chunk of the launch-shape-independence check is at most this much of one trip

# ---- the launch rules ------------------------------------------------------------------------------------------------------------------------
# items: of the launch (sweep kernels: frames are folded into the item index) or of one frame / one plane (per_frame: blockIdx.y = frame);
# lanes per workgroup; cap on the workgroups (None: no loop, the grid covers the items)
Launch = collections.namedtuple("Launch", "items lanes cap per_frame")

SWEEP_LANES = 256            # bsvd_internal.h launch_sweep: dim3(256)
SWEEP_MAX_WGS = 256 * 16     # bsvd_internal.h grid_for: `if (g > 256 * 16) g = 256 * 16`
SIGMA_BLOCK, SIGMA_MAX_WGS = 512, 512          # frame_sigma.hip enum; frame_nlf.hip NLF_BLOCK, NLF_MAX_WGS are the same numbers
FILL_LANES, FILL_MAX_WGS = 256, 4096           # frame_sigma.hip bsvd_fill_sigma_plane / frame_nlf.hip bsvd_fill_nlf_plane: `4096u / frames`
VST_BLOCK, VST_MAX_WGS = 256, 2048             # frame_vst.hip enum
SCENE_DIFF_THREADS, SCENE_DIFF_MAX_WGS = 256, 64   # frame_scene.hip enum
SCENE_WAVES = 4              # frame_scene.hip: one wave per block, four blocks per workgroup, no loop
BAND = 8                     # frame_sigma_items.h SIGMA_BAND; frame_nlf_items.h NLF_BAND = SIGMA_BAND


def _ceil(a, b):
    return -(-a // b)


def workgroups(l):
    g = max(_ceil(l.items, l.lanes), 1)
    return g if l.cap is None else max(min(g, l.cap), 1)


def per_trip(l):
    return workgroups(l) * l.lanes


def trips(l):
    return l.items / per_trip(l)


def tail(l):
    """items of the last trip"""
    return l.items - (_ceil(l.items, per_trip(l)) - 1) * per_trip(l)


def cap_binds(l):
    return l.cap is not None and _ceil(l.items, l.lanes) > l.cap


def qualifies(l):
    return trips(l) >= TRIPS_MIN and tail(l) % WAVE != 0 and cap_binds(l)


def cap_fraction(l):
    """items over the items of one trip of a grid AT its cap: at most 1 means a single trip whatever the grid"""
    return 0.0 if l.cap is None else l.items / (l.cap * l.lanes)


def single_trip(l):
    return trips(l) <= 1.0


def _sweep(items):
    return Launch(items, SWEEP_LANES, SWEEP_MAX_WGS, False)


def _frame_cap(max_wgs, T):
    return max(max_wgs // T, 1)                # `MAX_WGS / frames > 0 ? MAX_WGS / frames : 1` in every per-frame launch


def items_per_row(W):
    return (W + 3) >> 2                        # frame_items.h items_per_row


def rule_u8_to_planar(T, H, W, C=3, cc=1):
    return _sweep(T * (C + cc) * H * W)        # tensor_layout.hip bsvd_u8_to_planar: total = frames (C + const_channels) H W


def rule_planar_to_u8(T, H, W, C=3):
    return _sweep(T * C * H * W)               # tensor_layout.hip bsvd_planar_to_u8: total


def rule_u8_pad(T, H, W):
    return _sweep(T * H * items_per_row(W))    # tensor_layout.hip u8_pad_check: per_frame = H items_per_row(W); both directions


def rule_yuv(T, H, W, sub):
    item_rows = H >> 1 if sub == 420 else H    # frame_surface_items.h surf_item_rows; frame_yuv.hip plan_check: per_frame = item_rows items_per_row(W)
    return _sweep(T * item_rows * items_per_row(W))


def rule_rgb(T, H, W):
    return _sweep(T * H * items_per_row(W))    # frame_rgb.hip: per_frame = H items_per_row(W)


def rule_blend(T, Hp, Wp):
    plane = Hp * Wp                            # frame_finish.hip: g.per_frame = g.vec ? plane / 4 : plane (16-byte aligned tensors, strides % 4 == 0)
    return _sweep(T * (plane // 4 if Wp % 4 == 0 else plane))


def sigma_items(H, W, ch=3):
    return ch * _ceil(H - 2, BAND) * ((W + 2) >> 2)      # frame_sigma_items.h sigma_items = ch sigma_bands(H) sigma_groups(W)


def rule_sigma_hist(T, H, W):
    return Launch(sigma_items(H, W), SIGMA_BLOCK, _frame_cap(SIGMA_MAX_WGS, T), True)      # frame_sigma.hip bsvd_estimate_sigma


rule_nlf_hist = rule_sigma_hist                # frame_nlf.hip bsvd_estimate_nlf: sigma_items(g) with ch = 3, NLF_BLOCK = NLF_MAX_WGS = 512


def rule_fill_sigma(T, Hp, Wp):
    return Launch(_ceil(Hp * Wp, 4), FILL_LANES, _frame_cap(FILL_MAX_WGS, T), True)        # frame_sigma.hip bsvd_fill_sigma_plane: items = (n + 3) / 4


def rule_nlf_map(T, Hp, Wp):
    return Launch(_ceil(Hp, BAND) * _ceil(Wp, 4), FILL_LANES, _frame_cap(FILL_MAX_WGS, T), True)   # frame_nlf_items.h nlf_map_items


def rule_vst(T, Hp, Wp, C=4):
    plane = Hp * Wp                            # frame_vst.hip vst_launch: per_plane = vec ? plane / 4 : plane; one sweep per plane
    vec = plane % 4 == 0 and (C * plane) % 4 == 0
    return Launch(plane // 4 if vec else plane, VST_BLOCK, _frame_cap(VST_MAX_WGS, T), True)


def rule_scene_diff(blocks):
    return Launch(blocks, SCENE_DIFF_THREADS, SCENE_DIFF_MAX_WGS, True)                    # frame_scene.hip bsvd_scene_diff: gx capped at 64


def rule_scene_grid(H, W):
    return Launch((H // 16) * (W // 16), SCENE_WAVES, None, True)                          # frame_scene.hip bsvd_scene_grid: gx = ceil(blocks / 4), no loop


def smallest_T(rule):
    """the smallest frame count at which the sweep rule T -> Launch qualifies"""
    T = max(int(TRIPS_MIN * SWEEP_LANES * SWEEP_MAX_WGS / rule(1).items), 1)
    for T in range(T, T + 256):
        if qualifies(rule(T)):
            return T
    raise ValueError("no frame count near %d gives a ragged last trip: %r" % (T, rule(1)))


def chunk_frames(rule, T):
    """frames per chunk of the launch-shape-independence check: the most at which rule(chunk) is at most CHUNK_TRIPS of a trip, and at
    most 2 / 7 of the frames, so that every case -- those whose whole launch is below a trip too -- is split into at least four calls, the
    last one shorter than the others"""
    best = 1
    if rule(1).cap is None:                    # no loop in the kernel: any split is a different launch shape
        return _ceil(T, 4)
    for n in range(1, T + 1):
        l = rule(n)
        if l.items <= CHUNK_TRIPS * (l.cap if l.cap is not None else workgroups(l)) * l.lanes:
            best = n
        elif not l.per_frame:
            break
    return max(min(best, _ceil(2 * T, 7)), 1)


def chunks(rule, T):
    n = chunk_frames(rule, T)
    return [(a, min(a + n, T)) for a in range(0, T, n)]


# ---- the sweep cases -------------------------------------------------------------------------------------------------------------------------
SIGMA = 30 / 255.0
SEED, FRAME0 = 0x5eed1234, 5
COLOURS = list(itertools.product(["bt601", "bt709", "bt2020"], [False, True]))
CHROMAS = ["nearest", "linear"]
DITHERS = [None, "ordered", "random"]
FAMILIES = ["frames", "rows"]
STRENGTHS = [(1.0, 1.0), (0.0, 0.0), (0.4, 0.8), (0.75, 0.25)]
YUV_NAMES = sorted(S.FORMATS) + ["nv12", "p010"]          # nv12 / p010: the BsvdYuvDesc front (frame_io.yuv420_to_input / output_to_yuv420)
RGB_NAMES = sorted(R.FORMATS)

Case = collections.namedtuple("Case", "id unit entry fmt family pad pitched hwc chroma matrix full_range dither strength T H W Hp Wp")


def yuv_sub(fmt):
    return 420 if fmt in M.BITS else S.FORMATS[fmt].sub


def yuv_bits(fmt):
    return M.BITS[fmt] if fmt in M.BITS else S.FORMATS[fmt].bits


def case_rule(c, T=None):
    """the Launch of case c (at another frame count T)"""
    T = c.T if T is None else T
    if c.entry == "u8_in":
        return rule_u8_pad(T, c.H, c.W) if c.pad else rule_u8_to_planar(T, c.H, c.W)
    if c.entry == "u8_out":
        return rule_u8_pad(T, c.H, c.W) if c.pad else rule_planar_to_u8(T, c.H, c.W)
    if c.entry in ("yuv_in", "yuv_out"):
        return rule_yuv(T, c.H, c.W, yuv_sub(c.fmt))
    if c.entry in ("rgb_in", "rgb_out"):
        return rule_rgb(T, c.H, c.W)
    assert c.entry == "blend"
    return rule_blend(T, c.Hp, c.Wp)


def _geometry(family, pad, even_rows, plain_u8=False):
    """-> (H, W, Hp, Wp)"""
    if plain_u8:                               # element-wise kernels with a constant channel: 4 H W is ragged only with an odd width
        return (72, 123, 72, 123) if family == "frames" else (33, 3835, 33, 3835)    # 4 x 33 x 3835: a frame is under half a trip
    if family == "frames":
        return ((70 if even_rows else 69, 126, 72, 128) if pad else (72, 124, 72, 124))
    return ((34 if even_rows else 35, 3836, 36, 3840) if pad else (36, 3836, 36, 3836))


def _case(k, unit, entry, fmt, hwc=False, dither=None, strength=None, pad=None):
    """case number k of its translation unit: the options are dealt from the bits and residues of k"""
    family = FAMILIES[k & 1]
    pad = bool((k >> 1) & 1) if pad is None else pad
    matrix, full_range = COLOURS[k % 6]
    H, W, Hp, Wp = _geometry(family, pad, entry.startswith("yuv") and yuv_sub(fmt) == 420, entry.startswith("u8") and not pad)
    c = Case("%s-%s%s" % (entry, fmt, "-hwc" if hwc else ""), unit, entry, fmt, family, pad, bool((k >> 2) & 1), hwc, CHROMAS[(k >> 1 ^ k >> 3) & 1],
             matrix, full_range, dither, strength, 0, H, W, Hp, Wp)
    return c._replace(T=smallest_T(lambda T: case_rule(c, T)))


def _sweep_cases():
    out = []
    k = 0
    for entry in ("u8_in", "u8_out"):
        for pad, hwc in itertools.product([False, True], [False, True]):
            out.append(_case(k, "tensor_layout", entry, "pad" if pad else "plain", hwc=hwc, pad=pad))
            k += 1
    for k, (fmt, entry) in enumerate(itertools.product(YUV_NAMES, ("yuv_in", "yuv_out"))):
        k2 = k // 2 + (k & 1) * 5                                     # the two directions of a format get different options
        out.append(_case(k2, "frame_yuv", entry, fmt, dither=DITHERS[(k // 2) % 3] if entry == "yuv_out" else None))
    for k, (fmt, entry) in enumerate(itertools.product(RGB_NAMES, ("rgb_in", "rgb_out"))):
        k2 = k // 2 + (k & 1) * 3
        out.append(_case(k2, "frame_rgb", entry, fmt, dither=DITHERS[(k // 2 + 1) % 3] if entry == "rgb_out" else None))
    for k, s in enumerate(STRENGTHS):
        out.append(_case(k, "frame_finish", "blend", "s%g_%g" % s, strength=s, pad=False)._replace(id="blend-%g-%g" % s))
    assert len({c.id for c in out}) == len(out)
    return out


SWEEP_CASES = _sweep_cases()


def layout_yuv(c):
    """-> dict of the surface layout of a YUV case: pitches / offsets / stride (general surfaces) or row_pitch / stride (nv12, p010)"""
    if c.fmt in M.BITS:
        sb = 2 if c.fmt == "p010" else 1
        pitch = (c.W * sb + 63) // 64 * 64 + 64 if c.pitched else None
        return dict(row_pitch=pitch, stride=M.frame_bytes(c.H, c.W, c.fmt, pitch) + (128 if c.pitched else 0))
    if not c.pitched:
        return dict(pitches=None, offsets=None, stride=S.frame_bytes(c.H, c.W, c.fmt))
    pl = S.planes(c.H, c.W, c.fmt)             # the pitched layout of tests/test_gpu_yuv_formats.py
    pitches = [(rb + 63) // 64 * 64 + 64 + 2 * i for i, (_, rb) in enumerate(pl)]
    offsets, at = [], 66
    for i, (rows, _) in enumerate(pl):
        offsets.append(at)
        at += pitches[i] * rows + (34, 18, 0)[i]
    return dict(pitches=pitches, offsets=offsets, stride=S.frame_bytes(c.H, c.W, c.fmt, pitches, offsets) + 128)


def layout_rgb(c):
    if not c.pitched:
        return dict(pitches=None, offsets=None, stride=R.frame_bytes(c.H, c.W, c.fmt))
    pl = R.planes(c.H, c.W, c.fmt)             # the pitched layout of tests/test_gpu_rgb.py
    pitches = [(rb + 63) // 64 * 64 + 64 + 4 * i for i, (_, rb) in enumerate(pl)]
    offsets, at = [], 68
    for i, (rows, _) in enumerate(pl):
        offsets.append(at)
        at += pitches[i] * rows + (36, 20, 12, 0)[i]
    return dict(pitches=pitches, offsets=offsets, stride=R.frame_bytes(c.H, c.W, c.fmt, pitches, offsets) + 128)


def case_bytes(c):
    """name -> bytes of every device buffer of a sweep case"""
    planes = c.T * c.Hp * c.Wp * 4
    if c.entry in ("u8_in", "u8_out"):
        return {"u8": c.T * 3 * c.H * c.W, "fp32": planes * (4 if c.entry == "u8_in" else 3)}
    if c.entry == "blend":
        return {"y": planes * 3, "x": planes * 4}
    stride = (layout_yuv if c.entry.startswith("yuv") else layout_rgb)(c)["stride"]
    return {"surface": c.T * stride, "fp32": planes * (4 if c.entry.endswith("_in") else 3)}


# ---- seeded inputs (numpy; shared, never written) ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _random_words(T, H, W):
    """uint16 [4, T, H, W]: the pool every code array of one geometry is cut from"""
    return np.random.default_rng(1000 * H + W).integers(0, 1 << 16, (4, T, H, W), dtype=np.uint16)


def codes(T, H, W, bits, n=4, lo=0, hi=None):
    """frames [lo, hi) of n code arrays [T, H, W] over the full range of ``bits``"""
    w = _random_words(T, H, W)
    return [(w[i, lo:hi] >> (16 - bits)).astype(np.int64) for i in range(n)]


@functools.lru_cache(maxsize=2)
def values(T, Hp, Wp, C=3):
    """float32 [T, C, Hp, Wp]: uniform(-0.1, 1.1), with a tenth of the elements k / 510 (exact 0 and 1, rounding ties at 8 bits)"""
    rs = np.random.default_rng(7 * Hp + Wp + C)
    x = rs.random((T, C, Hp, Wp), dtype=f32) * f32(1.2) - f32(0.1)
    pick = rs.random((T, C, Hp, Wp), dtype=f32) < f32(0.1)
    x[pick] = (rs.integers(0, 511, int(pick.sum())) / 510.0).astype(f32)
    x.setflags(write=False)
    return x


def yuv_codes_of(c, lo=0, hi=None):
    hi = c.T if hi is None else hi
    ch, cw = S.chroma_shape(c.H, c.W, yuv_sub(c.fmt))
    Y, Cb, Cr = codes(c.T, c.H, c.W, yuv_bits(c.fmt), 3, lo, hi)
    return Y, Cb[:, :ch, :cw], Cr[:, :ch, :cw]


def yuv_surface_of(c, lo=0, hi=None):
    """the source surfaces of a yuv_in case, uint8 [frames, stride]: 0xFF in every byte that is no sample, junk in the ignored bits"""
    Y, Cb, Cr = yuv_codes_of(c, lo, hi)
    lay = layout_yuv(c)
    rs = np.random.RandomState(5)
    if c.fmt in M.BITS:
        return M.pack(Y, Cb, Cr, c.fmt, lay["row_pitch"], lay["stride"], fill=0xFF, low_bits=rs.randint(0, 64, (Y.shape[0], c.H * 3 // 2, c.W)))
    return S.pack(Y, Cb, Cr, c.fmt, lay["pitches"], lay["offsets"], lay["stride"], fill=0xFF, junk=rs)


def rgb_surface_of(c, lo=0, hi=None):
    hi = c.T if hi is None else hi
    r, g, b, a = codes(c.T, c.H, c.W, R.FORMATS[c.fmt].bits, 4, lo, hi)
    lay = layout_rgb(c)
    return R.pack(r, g, b, c.fmt, a, lay["pitches"], lay["offsets"], lay["stride"], fill=0xFF, junk=np.random.RandomState(6))


def alpha_of(c, lo=0, hi=None):
    """the alpha codes an rgb_out case writes (formats with alpha), in the container type"""
    hi = c.T if hi is None else hi
    return codes(c.T, c.H, c.W, R.FORMATS[c.fmt].bits, 4, lo, hi)[3].astype(R.container(c.fmt)) if R.has_alpha(c.fmt) else None


def u8_source_of(c, lo=0, hi=None):
    hi = c.T if hi is None else hi
    p = np.stack(codes(c.T, c.H, c.W, 8, 3, lo, hi), axis=1).astype(np.uint8)          # [T, 3, H, W]
    return np.ascontiguousarray(np.moveaxis(p, 1, -1)) if c.hwc else p


# ---- the models, on frames [lo, hi) of a case ---------------------------------------------------------------------------------------------------
def yuv_colour(c):
    return dict(matrix=c.matrix, full_range=c.full_range, chroma=c.chroma)


def model(c, lo=0, hi=None):
    """What frames [lo, hi) of the case's call give, by the model the format's small-shape test uses.
    u8_in / rgb_in: float32 [n, 4, Hp, Wp], the device's bits (rgb_in: a pair with the alpha codes or None).
    yuv_in: float64 [n, 3, Hp, Wp], the truth (the device is held to 1e-6 of it; its fourth plane to float32(SIGMA)).
    u8_out: uint8 frames.  rgb_out: uint8 [n, stride], the device's bytes, 0xA5 in every byte that is no sample.
    yuv_out: ([Y, Cb, Cr] codes, [near-tie masks]) for finish_model.mismatches.  blend: float32 [n, 3, Hp, Wp], the device's bits."""
    hi = c.T if hi is None else hi
    pad = (c.Hp, c.Wp)
    if c.entry == "u8_in":
        p = u8_source_of(c._replace(hwc=False), lo, hi)
        x = np.concatenate([p.astype(f32) / f32(255.0), np.full((hi - lo, 1, c.H, c.W), SIGMA, f32)], axis=1)
        return np.ascontiguousarray(R.reflect_pad(x, *pad))
    if c.entry == "u8_out":
        v = values(c.T, c.Hp, c.Wp)[lo:hi, :, :c.H, :c.W]
        q = np.rint(np.clip(v, f32(0), f32(1)) * f32(255.0)).astype(np.uint8)
        if c.chroma == "linear":                                       # the u8_out cases deal reverse_channels from the chroma slot
            q = q[:, ::-1]
        return np.ascontiguousarray(np.moveaxis(q, 1, -1)) if c.hwc else np.ascontiguousarray(q)
    if c.entry == "yuv_in":
        Y, Cb, Cr = yuv_codes_of(c, lo, hi)
        x = (M.decode(Y, Cb, Cr, M.BITS[c.fmt], dtype=np.float64, **yuv_colour(c)) if c.fmt in M.BITS
             else S.decode(Y, Cb, Cr, c.fmt, dtype=np.float64, **yuv_colour(c)))
        return S.reflect_pad(x, *pad)
    if c.entry == "yuv_out":
        v = values(c.T, c.Hp, c.Wp)[lo:hi, :, :c.H, :c.W]
        fn = F.yuv420_codes if c.fmt in M.BITS else F.yuv_codes
        return fn(v, c.fmt, mode=c.dither, seed=SEED, frame0=FRAME0 + lo, **yuv_colour(c))
    if c.entry == "rgb_in":
        lay = layout_rgb(c)
        return R.to_input(rgb_surface_of(c, lo, hi), c.H, c.W, c.fmt, c.full_range, lay["pitches"], lay["offsets"], pad_to=pad, const=SIGMA)
    if c.entry == "rgb_out":
        lay = layout_rgb(c)
        v = values(c.T, c.Hp, c.Wp)[lo:hi]
        kw = dict(full_range=c.full_range, pitches=lay["pitches"], offsets=lay["offsets"], frame_stride=lay["stride"], crop_to=(c.H, c.W),
                  alpha=alpha_of(c, lo, hi), fill=0xA5)
        if c.dither is None:
            return R.to_surface(v, c.fmt, **kw)
        return F.rgb_to_surface(v, c.fmt, mode=c.dither, seed=SEED, frame0=FRAME0 + lo, **kw)
    assert c.entry == "blend"
    y, x = values(c.T, c.Hp, c.Wp)[lo:hi], values(c.T, c.Hp, c.Wp, 4)[lo:hi]
    return F.blend(y, x, c.strength[0], c.strength[1], F.LUMA_W[c.matrix])


# ---- the kernels whose blockIdx.y is the frame ------------------------------------------------------------------------------------------------
# regime 'headline': the ClipPipeline call on the headline clip, 10 frames of 540 x 960 in the network's 544 x 960 planes.
# regime 'collapsed': so many frames that the cap is one workgroup per frame, with the smallest picture that then qualifies: not square,
#   a column-group count off every multiple of 64 (waves straddle band and row boundaries).
# regime 'max_frames': the largest accepted frame count, 65535, with the smallest legal picture; the two histogram kernels take 4096 frames:
#   their workspaces at 65535 frames are 65535 x 4096 x 4 bytes = 1.0 GiB and 65535 x 16 x 1024 x 4 bytes = 4.0 GiB = 4.3 x 10^9 bytes,
#   at and far past the 1 GiB a buffer of a case may have.
Frames = collections.namedtuple("Frames", "id kernel regime T H W Hp Wp C")
HEADLINE = (10, 540, 960, 544, 960)
MAX_FRAMES = 65535
HIST_MAX_FRAMES = 4096


def frame_rule(fc, T=None):
    T = fc.T if T is None else T
    return {"sigma_hist": lambda: rule_sigma_hist(T, fc.H, fc.W), "nlf_hist": lambda: rule_nlf_hist(T, fc.H, fc.W),
            "fill_sigma": lambda: rule_fill_sigma(T, fc.Hp, fc.Wp), "nlf_map": lambda: rule_nlf_map(T, fc.Hp, fc.Wp),
            "vst_forward": lambda: rule_vst(T, fc.Hp, fc.Wp, fc.C), "vst_inverse": lambda: rule_vst(T, fc.Hp, fc.Wp, fc.C),
            "scene": lambda: rule_scene_grid(fc.H, fc.W)}[fc.kernel]()


def _frame_cases():
    out = []
    for kernel in ("sigma_hist", "nlf_hist", "fill_sigma", "nlf_map", "vst_forward", "vst_inverse", "scene"):
        C = 3 if kernel == "vst_inverse" else 4
        out.append(Frames(kernel + "-headline", kernel, "headline", *HEADLINE, C))
    # collapsed cap: 512 / 300 = 1 workgroup of 512 items against 3 x 22 x 18 = 1188; 4096 / 2100 = 1 of 256 against 595 / 598; 2048 / 1100 = 1 against 595
    out += [Frames("sigma_hist-collapsed", "sigma_hist", "collapsed", 300, 171, 70, 172, 72, 4),
            Frames("nlf_hist-collapsed", "nlf_hist", "collapsed", 300, 171, 70, 172, 72, 4),
            Frames("fill_sigma-collapsed", "fill_sigma", "collapsed", 2100, 34, 70, 34, 70, 4),
            Frames("nlf_map-collapsed", "nlf_map", "collapsed", 2100, 100, 184, 100, 184, 4),
            Frames("vst_forward-collapsed", "vst_forward", "collapsed", 1100, 34, 70, 34, 70, 4),
            Frames("vst_inverse-collapsed", "vst_inverse", "collapsed", 1100, 34, 70, 34, 70, 3),
            Frames("scene-collapsed", "scene", "collapsed", 600, 48, 80, 50, 84, 4)]
    out += [Frames("sigma_hist-max_frames", "sigma_hist", "max_frames", HIST_MAX_FRAMES, 3, 3, 3, 3, 3),
            Frames("nlf_hist-max_frames", "nlf_hist", "max_frames", HIST_MAX_FRAMES, 3, 3, 3, 3, 3),
            Frames("fill_sigma-max_frames", "fill_sigma", "max_frames", MAX_FRAMES, 1, 1, 1, 1, 2),
            Frames("nlf_map-max_frames", "nlf_map", "max_frames", MAX_FRAMES, 1, 1, 1, 1, 4),
            Frames("vst_forward-max_frames", "vst_forward", "max_frames", MAX_FRAMES, 1, 1, 1, 1, 4),
            Frames("vst_inverse-max_frames", "vst_inverse", "max_frames", MAX_FRAMES, 1, 1, 1, 1, 3),
            Frames("scene-max_frames", "scene", "max_frames", MAX_FRAMES, 16, 16, 16, 16, 3),
            Frames("scene-gw240", "scene", "rows", 3, 32, 3840, 32, 3840, 3)]
    return out


FRAME_CASES = _frame_cases()
# one trip exactly; one item into the second; 2.44 trips with a tail of 7232 = 113 whole waves; and the same with a ragged tail of 7269
SCENE_DIFF_BLOCKS = (16384, 16385, 40000, 40037)


def frame_bytes_of(fc):
    b = {"x": fc.T * fc.C * fc.Hp * fc.Wp * 4}
    if fc.kernel == "sigma_hist":
        b["workspace"] = fc.T * SM.BINS * 4
    if fc.kernel == "nlf_hist":
        b["workspace"] = fc.T * NM.LEVELS * NM.BINS * 4
    if fc.kernel.startswith("vst"):
        b["tables"] = fc.T * VM.TABLE_FLOATS * 4 if fc.regime != "max_frames" else VM.TABLE_FLOATS * 4
    return b


POOL = 7                     # distinct frames of the large frame-capped inputs: frame t holds pool frame t % 7


@functools.lru_cache(maxsize=4)
def frame_pool(n, C, Hp, Wp, H, W, special):
    """float32 [n, C, Hp, Wp]: uint8-derived noisy ramps in the picture (sigma 2 .. 40 / 255 over the frames), uniform(0, 1) outside it and
    in plane 3.  special: frame 1 is constant 0.5 in the picture (every lane of a wave on bin 0), frame 2 has NaN and +-Inf in it."""
    rs = np.random.default_rng(31 * Hp + Wp + n)
    x = rs.random((n, C, Hp, Wp), dtype=f32)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([0.2 + 0.6 * xx / max(W - 1, 1), 0.2 + 0.6 * yy / max(H - 1, 1), 0.8 - 0.3 * (xx + yy) / max(H + W - 2, 1)])
    for t in range(n):
        sig = 2.0 + 38.0 * t / max(n - 1, 1)
        u8 = np.clip(np.rint(ramp * 255.0 + sig * rs.standard_normal(ramp.shape)), 0, 255).astype(np.uint8)
        x[t, :min(C, 3), :H, :W] = SM.to_f32(u8)[:min(C, 3)]
    if special and n > 2:
        x[1, :3, :H, :W] = f32(0.5)
        for k, v in enumerate((np.nan, np.inf, -np.inf) * 4):
            x[2, k % 3, rs.integers(H), rs.integers(W)] = v
    x.setflags(write=False)
    return x


def frame_input(fc):
    """-> (pool float32 [n, C, Hp, Wp], index int [T]): frame t of the case's tensor is pool[index[t]]"""
    n = fc.T if fc.T <= 16 else POOL
    pool = frame_pool(n, fc.C, fc.Hp, fc.Wp, fc.H, fc.W, fc.kernel.endswith("hist") and fc.regime != "max_frames")
    return pool, np.arange(fc.T) % n


@functools.lru_cache(maxsize=None)
def curve_pool(n=5):
    """float32 [n, 16]: vst_model's test curves (flat, sqrt(a I + b), random, a step, all zero)"""
    return np.stack(list(VM.curves().values())[:n]).astype(f32)


@functools.lru_cache(maxsize=None)
def table_pool(n=5):
    return np.stack([VM.tables(c) for c in curve_pool(n)])


def frame_picture(fc):
    return None if (fc.H, fc.W) == (fc.Hp, fc.Wp) else (fc.H, fc.W)


def sigma_values(fc):
    """the per-frame values a fill_sigma case writes"""
    return (np.arange(fc.T) % 251 / 251.0).astype(f32)


def set_index(fc, per_frame=True):
    """which curve (nlf_map) or table set (vst) of the pools frame t uses; not per_frame: set 1 for every frame"""
    return np.arange(fc.T) % len(curve_pool()) if per_frame else np.full(fc.T, 1)


def _by_pair(index, sets, fn):
    """fn(pool frame, set) -> array, evaluated once per distinct (frame, set) pair and dealt back to the frames"""
    key, inv = np.unique(index * 16 + sets, return_inverse=True)
    return np.stack([fn(k // 16, k % 16) for k in key])[inv]


def frame_model(fc, lo=0, hi=None, per_frame=True):
    """What frames [lo, hi) of a frame case give, by the model its small-shape test uses (every one bit for bit):
    sigma_hist / nlf_hist -> (values, int64 histograms); fill_sigma / nlf_map -> the written plane [n, Hp, Wp];
    vst_forward / vst_inverse -> planes 0 .. 2 [n, 3, Hp, Wp] (per_frame: a table set per frame);
    scene -> (grid, sad), the frame before ``lo`` standing in as ``prev``"""
    hi = fc.T if hi is None else hi
    pool, index = frame_input(fc)
    idx, pic = index[lo:hi], frame_picture(fc)
    if fc.kernel in ("sigma_hist", "nlf_hist"):
        v, h = (SM if fc.kernel == "sigma_hist" else NM).estimate(pool, pic)
        return v[idx], h[idx]
    if fc.kernel == "fill_sigma":
        return np.ascontiguousarray(np.broadcast_to(sigma_values(fc)[lo:hi, None, None], (hi - lo, fc.Hp, fc.Wp)))
    if fc.kernel == "nlf_map":
        return _by_pair(idx, set_index(fc)[lo:hi], lambda f, k: NM.noise_map(pool[f:f + 1], curve_pool()[k:k + 1])[0])
    tp = table_pool()
    if fc.kernel == "vst_forward":
        return _by_pair(idx, set_index(fc, per_frame)[lo:hi], lambda f, k: VM.forward(pool[f, :3], tp[k][:VM.KNOTS]))
    if fc.kernel == "vst_inverse":
        return _by_pair(idx, set_index(fc, per_frame)[lo:hi], lambda f, k: VM.inverse(pool[f, :3], tp[k][:VM.KNOTS], tp[k][VM.R_AT:]))
    assert fc.kernel == "scene"
    g = SC.grid(pool, pic)
    return g[idx], SC.sad(g[idx], g[index[lo - 1]] if lo else None)


def vst_sigma_plane(fc, per_frame=True):
    """the fourth plane vst_forward writes with fill_plane: sigma' of the frame's table set"""
    sig = table_pool()[set_index(fc, per_frame)][:, VM.SIGMA_AT]
    return np.ascontiguousarray(np.broadcast_to(sig[:, None, None], (fc.T, fc.Hp, fc.Wp)))
