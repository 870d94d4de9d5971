"""Host <-> device pipelining around the hot path (new component; SURVEY.md 8f-4 "frame I/O on device").

The reference moves every frame to the GPU synchronously on the compute stream (``x.cuda()``,
/root/reference/Experimental_root/archs/bsvd_arch.py:520) and brings fp32 results back with ``.cpu()`` after a
``torch.cuda.synchronize()`` (models/validation_seq_infer.py:28, denoising_model.py:187).  Here a sequence of clips
flows through three HIP streams so PCIe never idles the matrix cores:

    upload stream   : pinned uint8 frames -> HBM                      (4x fewer bytes than the reference's fp32 frames)
    compute stream  : bsvd_u8_to_planar -> BSVD forward -> bsvd_planar_to_u8   (all kernels of libbsvd_hip.so)
    download stream : uint8 result -> pinned host buffer

``depth`` slots of pinned staging memory form a ring; slot k is reused once its download has completed.  Results are
yielded in submission order.

The options of ``ClipPipeline`` and ``LiveStream`` are described here, once; the class docstrings say what differs per class: the
arrays taken and returned, latency, rings, and when the host waits.  Both check them in one order before anything touches a device,
and with the defaults both launch nothing new and give the bytes they gave.

``pix_fmt`` selects what crosses PCIe: 'rgb24' (the default, packed RGB uint8 [H,W,3]) or the YUV 4:2:0 surfaces video sources and
sinks speak, 'nv12' (uint8) and 'p010' (uint16, 10-bit code in the high bits), as arrays [H*3/2, pitch] -- the Y plane's H rows,
then the H/2 rows of interleaved CbCr; 1.5 (NV12) or 3 (P010) bytes per pixel each way instead of 3, converted by
``bsvd_yuv420_to_planar`` / ``bsvd_planar_to_yuv420`` where the uint8 kernels run for 'rgb24'.  The planar, 4:2:2 and 4:4:4 surfaces
('yuv420p', 'yuv420p10le', 'uyvy422', 'yuyv422', 'nv16', 'p210le', 'yuv422p', 'yuv422p10le', 'yuv444p', 'yuv444p10le'; ffmpeg's names)
cross as 1-D arrays of the tight frame's samples -- what ``ffmpeg -f rawvideo`` emits --, with ``frame_shape=(H, W)`` given at
construction, converted by ``bsvd_yuv_to_planar`` / ``bsvd_planar_to_yuv``.  The RGB surfaces of ``_lib.RGB_FORMATS`` besides 'rgb24'
('bgr24', 'rgba', 'bgra', 'argb', 'abgr', 'rgb0', 'bgr0', '0rgb', '0bgr', 'rgb48le', 'bgr48le', 'rgba64le', 'bgra64le', 'x2rgb10le',
'x2bgr10le', 'gbrp', 'gbrp10le', 'gbrp12le', 'gbrp16le', 'gbrap', 'gbrap10le', 'gbrap12le', 'gbrap16le') cross as self-describing
arrays -- packed [H,W,3|4] uint8 / uint16, [H,W] uint32 for the x2 words, planar [P,H,W] -- or as 1-D arrays of the tight frame's
samples with ``frame_shape``, converted by ``bsvd_rgb_to_planar`` / ``bsvd_planar_to_rgb``; ``colour`` may carry ``full_range`` only
(default True).  A format with alpha returns every frame with the alpha codes it came with, bit for bit: they wait on the device while
the frame is inside the network.

``pad`` selects what happens to a picture whose H or W is no multiple of 4 (the network has two 2x scales): None (the default) refuses
it; 'reflect' takes any size -- even H and W for the 4:2:0 surfaces -- and does what the reference's callers do around the model
(denoising_model.py, padding_input / crop_output): reflect-pad on the right and bottom up to the next multiples of 4, run the network at that
size, crop the result.  Pad and crop happen inside the conversion kernels (``frame_io``'s ``pad_to`` / ``crop_to``), so the staging buffers
and the PCIe transfers stay picture-sized and the results have the shape and dtype of what was fed.

``sigma`` is the noise level of the non-blind models' noise map: a float the caller knows, or 'auto' -- every frame's own estimate, computed
on the compute stream from the converted frame and written into its noise-map plane (``frame_io.estimate_sigma``; ``sigma_gain`` scales
it).  The host sees it only afterwards, as ``LiveStream.last_sigma``: 4 bytes that come down with the frame.  For sources whose noise depends
on the signal level: 'nlf' -- every frame's own noise-level function, sigma at sixteen levels of local intensity, and a per-pixel noise map
written from it (``frame_io.estimate_noise_curve`` / ``fill_noise_map``; ``LiveStream.last_noise_curve``: 64 bytes that come down with the
frame) -- or a ``frame_io.NoiseCurve`` the caller knows: the map is written from that curve and nothing is reported.  All but the float need a
non-blind model.  Nothing is known about the estimates on real footage (``frame_io.estimate_sigma`` / ``estimate_noise_curve``: what is
known), and YUV sources with subsampled chroma read low: ``sigma_gain`` scales every estimate.

``vst`` (with ``sigma=None``) is the remedy for signal-dependent noise that stays inside what the reference's checkpoints were trained on:
a variance-stabilising transform.  The colour planes are remapped by the curve's g(I) ~ integral dI / sigma(I) before the network
(``frame_io.build_vst`` / ``vst_forward``), the noise plane is the one sigma' the noise then has everywhere, and the result is mapped back
(``vst_inverse``) before the strength blend and the encoder.  A ``frame_io.NoiseCurve``: one table set for the stream; 'scene': the frame
that starts a scene gives the curve (``frame_io.estimate_noise_curve``, times ``sigma_gain``) and every later frame of the scene uses its
tables: a curve that drifts within a scene (auto-exposure) is not followed until the next cut.  A curve that is flat after the clamp to
[``vst_floor``, 1] is the identity: nothing is launched and the plane is written as sigma=<that value> writes it.  ``strength`` blends in the
picture's own domain, with the untransformed source (strength=0 still returns the source).  A blind model gets the transform and no plane.
No trained checkpoint has been run through it: its effect on denoising quality is not known, and nothing has been measured on real
footage (``frame_io.build_vst``: what is known).

``strength`` (a number or (luma, chroma), each in [0, 1]; default 1) is how much of the denoising to keep: the network's result is blended
with its own input on the device before it is encoded (``frame_io.blend_output``; luma weights: the stream's matrix for YUV formats, BT.709
for RGB ones, or ``luma_matrix``).  ``dither`` None | 'ordered' | 'random' with ``dither_seed``: dither at the encoder's quantiser
(``frame_io.output_to_*``); the random pattern depends on the frame's index in the stream.

``grain`` puts film grain back after denoising, as a MODEL instead of the removed signal that ``strength`` mixes back: a
``frame_io.GrainModel`` (its strength against brightness, its spatial correlation) the caller made, or 'scene' -- the first frame of every
scene to emerge has its source and result measured on the device (``frame_io.estimate_grain``: one host synchronisation per scene), and the
model fitted from it is synthesised onto that frame and every later frame of the scene (``frame_io.apply_grain``), after the inverse
transform and the strength blend and before the encoder and its dither; ``grain_amount`` (default 1) scales it, and the block offsets are
hashed from (``grain_seed``, the frame's index in the stream, the block).  With a strength below 1 the measured result is the blended one:
the model describes what is still missing.  ``last_grain_model``: the latest model.  No temporal pooling beyond the scene's first frame, no
overlap blending of grain blocks, nothing measured on real footage (``frame_io.estimate_grain``: what is known; the fit costs about the
figures of profiles/film_grain.txt).

``cuts`` is what the pipelines know about scene cuts: None (nothing: the footage is one scene, as before) or 'auto' -- every frame is scored
against the one before it on the device (``frame_io.scene_scores`` / ``scene_cuts``; ``cut_threshold``) and a frame that scores as a scene
start is fed with ``cut=True``: no temporal-fusion conv mixes the two scenes, nothing is flushed, latency is unchanged.  A caller who knows
the cuts says so per frame instead (``LiveStream.feed(frame, cut=True)``).  Nothing is known about the rule on real footage, the default
threshold has met none, and a cut one or two frames after another cut scores low (``frame_io.scene_cuts``: the rule and its blind spot).
"""
import collections

import numpy as np
import torch

from . import _lib
from .frame_io import (CUT_THRESHOLD, VST_FLOOR, VST_TABLE_FLOATS, GrainModel, NoiseCurve, _check_gain, _luma_weights, _sigma_mode, _yuv_desc, _yuv_surface,
                       apply_grain, blend_output, build_vst, check_cut_threshold, check_dither, check_grain, check_strength, check_vst_floor, cut_scores,
                       estimate_grain, estimate_noise_curve, fill_noise_map,
                       frames_to_input, network_size, output_to_frames, output_to_rgb, output_to_yuv, output_to_yuv420, rgb_frame_bytes, rgb_to_input,
                       scene_cuts, scene_scores, vst_forward, vst_identity, vst_inverse, vst_sigma, yuv420_frame_bytes, yuv420_picture_bytes,
                       yuv420_to_input, yuv_to_input)

Colour = collections.namedtuple("Colour", "matrix full_range chroma row_pitch width", defaults=("bt709", False, "linear", None, None))
Colour.__doc__ = """How a YUV surface is to be read and written: matrix 'bt601' | 'bt709' | 'bt2020', full_range (False = limited / "TV"
range), chroma 'nearest' | 'linear' (frame_io.yuv420_to_input), row_pitch in bytes (None = tight; otherwise it must be the arrays' row
length) and, for a pitch wider than the picture, its width W in samples (None = the arrays' row length)."""


# of one submitted array: picture size, shape of its bytes in the staging buffers, YUV row pitch (None = tight), and the size the network
# runs at: the picture's, or with pad='reflect' the next multiples of 4
_Geometry = collections.namedtuple("_Geometry", "h w staging row_pitch net_h net_w")

PADS = (None, "reflect")


def _check_pad(pad):
    if pad not in PADS:
        raise ValueError("pad %r: None (H and W must be multiples of 4) or 'reflect'" % (pad,))
    return pad


def _padded_size(h, w, what):
    """the network size of a picture under pad='reflect'; reflect needs a pad below the dimension, which rules out 1 and 2"""
    hp, wp = network_size(h, w)
    if hp - h >= h or wp - w >= w:
        raise ValueError("%s: a %d x %d picture cannot be reflect-padded to %d x %d (the pad must stay below the dimension)" % (what, h, w, hp, wp))
    return hp, wp


def _frame_shape(frame_shape):
    """``frame_shape`` -> (H, W) as ints; ValueError otherwise"""
    try:
        return int(frame_shape[0]), int(frame_shape[1])
    except (TypeError, ValueError, IndexError):
        raise ValueError("frame_shape: expected (H, W), got %r" % (frame_shape,)) from None


class _Format:
    """What the pixel-format adapters share.  ``pad``; ``geometry(a, clip)`` -> the ``_Geometry`` of a submitted array (each format's own);
    and one signature for every format, with or without alpha:
        to_input(dev_in, geom, sigma, sigma_gain, alpha=None) -> (x, alpha): the network input, and for a format with alpha the frames'
            alpha codes, a device tensor [T,H,W] -- written into ``alpha`` where one is given (a ring's plane), else a new one; without
            alpha in the format: None;
        to_output(y, geom, alpha=None, **dither) -> the surfaces, with those codes.
    ``pad_to`` / ``crop_to`` are given here, to the formats' ``_decode`` / ``_encode``: with pad='reflect' always, also for a picture that
    is a multiple of 4 already."""
    has_alpha = False

    def __init__(self, pad=None):
        self.pad = _check_pad(pad)

    def to_input(self, dev_in, geom, sigma, sigma_gain=1.0, alpha=None):
        return self._decode(dev_in, geom, alpha, sigma=sigma, sigma_gain=sigma_gain, pad_to=(geom.net_h, geom.net_w) if self.pad else None)

    def to_output(self, y, geom, alpha=None, **dither):
        return self._encode(y, geom, alpha, crop_to=(geom.h, geom.w) if self.pad else None, **dither)


class _Rgb24(_Format):
    """packed RGB uint8 [H,W,3]: staged as it comes, converted by bsvd_u8_to_planar / bsvd_planar_to_u8"""
    dtype = np.dtype(np.uint8)

    def geometry(self, a, clip):
        if a.dtype != np.uint8 or a.ndim != (4 if clip else 3) or a.shape[-1] != 3:
            raise ValueError("expected uint8 frames [T,H,W,3]" if clip else "expected one uint8 frame [H,W,3]")
        h, w = a.shape[-3], a.shape[-2]
        if self.pad:
            if h < 2 or w < 2:
                raise ValueError("expected frames of at least 2 x 2, got %d x %d" % (h, w))
            return _Geometry(h, w, tuple(a.shape), None, *_padded_size(h, w, "rgb24"))
        if h % 4 or w % 4:
            raise ValueError("H and W must be multiples of 4 (pad first: denoise.pad_to_multiple_of_4; or pad='reflect')")
        return _Geometry(h, w, tuple(a.shape), None, h, w)

    def _decode(self, dev_in, geom, alpha, sigma, **kw):
        return frames_to_input(dev_in, sigma, **kw), None

    def _encode(self, y, geom, alpha, crop_to, **dither):
        if dither.get("dither") is None:
            return output_to_frames(y, crop_to=crop_to)
        # dither: the RGB surface kernel, which gives the uint8 kernel's bits with dither off (the uint8 kernels have no dithered form)
        return output_to_rgb(y, "rgb24", crop_to=crop_to, **dither).view(y.shape[0], geom.h, geom.w, 3)


def _as_colour(colour):
    if colour is None:
        return Colour()
    if isinstance(colour, dict):
        unknown = set(colour) - set(Colour._fields)
        if unknown:
            raise ValueError("colour: unknown key(s) %s (known: %s)" % (sorted(unknown), ", ".join(Colour._fields)))
        return Colour(**colour)
    return Colour(*colour)


class _Yuv420(_Format):
    """NV12 (uint8) / P010 (uint16) arrays [H*3/2, pitch]: staged as the bytes of the surface, converted by bsvd_yuv420_to_planar /
    bsvd_planar_to_yuv420"""

    def __init__(self, pix_fmt, colour, pad=None):
        super().__init__(pad)
        colour = _as_colour(colour)
        self.pix_fmt, self.colour = pix_fmt, colour
        self.dtype = np.dtype(np.uint8 if pix_fmt == "nv12" else np.uint16)
        self.kw = dict(pix_fmt=pix_fmt, matrix=colour.matrix, full_range=bool(colour.full_range), chroma=colour.chroma)
        _yuv_desc(4, 4, row_pitch=None, **self.kw)               # a wrong name fails here, not at the first frame

    def geometry(self, a, clip):
        what = "%s %s [%sH*3/2,pitch]" % (self.pix_fmt, self.dtype.name, "T," if clip else "")
        if a.dtype != self.dtype or a.ndim != (3 if clip else 2):
            raise ValueError("expected %s, got %s %s" % (what, a.dtype, a.shape))
        rows, pitch = a.shape[-2], a.shape[-1]
        w = pitch if self.colour.width is None else int(self.colour.width)
        if self.pad:
            if rows <= 0 or rows % 3 or w <= 0 or w % 2:
                raise ValueError("expected %s with H and W even, got %s" % (what, a.shape))
        elif rows <= 0 or rows % 6 or w <= 0 or w % 4:
            raise ValueError("expected %s with H and W multiples of 4 (pad first: denoise.pad_to_multiple_of_4; or pad='reflect'), got %s" % (what, a.shape))
        if w > pitch:
            raise ValueError("%s: rows of %d samples are shorter than colour.width = %d" % (what, pitch, w))
        row_bytes = pitch * self.dtype.itemsize
        if self.colour.row_pitch is not None and self.colour.row_pitch != row_bytes:
            raise ValueError("%s: rows of %d bytes, colour.row_pitch says %d" % (what, row_bytes, self.colour.row_pitch))
        h = rows // 3 * 2
        net = _padded_size(h, w, what) if self.pad else (h, w)
        nbytes = (yuv420_picture_bytes if self.pad else yuv420_frame_bytes)(h, w, self.pix_fmt, row_bytes)
        return _Geometry(h, w, (a.shape[0], nbytes) if clip else (nbytes,), None if w == pitch else row_bytes, *net)

    def _decode(self, dev_in, geom, alpha, **kw):
        return yuv420_to_input(dev_in, geom.h, geom.w, row_pitch=geom.row_pitch, **self.kw, **kw), None

    def _encode(self, y, geom, alpha, **kw):
        return output_to_yuv420(y, row_pitch=geom.row_pitch, **self.kw, **kw)


class _YuvSurface(_Format):
    """the planar, 4:2:2 and 4:4:4 formats of _lib.YUV_FORMATS: 1-D arrays of the tight frame's samples (uint8; uint16 for the 10-bit
    formats) -- the bytes ``ffmpeg -f rawvideo`` emits --, converted by bsvd_yuv_to_planar / bsvd_planar_to_yuv.  A 1-D array does not
    say its picture size: frame_shape = (H, W) does, at construction."""

    def __init__(self, pix_fmt, colour, pad=None, frame_shape=None):
        super().__init__(pad)
        colour = _as_colour(colour)
        if colour.row_pitch is not None or colour.width is not None:
            raise ValueError("pix_fmt %r takes tight 1-D frames: colour.row_pitch / colour.width are for 'nv12' / 'p010' "
                             "(pitched surfaces: frame_io.yuv_to_input(pitches=))" % (pix_fmt,))
        if frame_shape is None:
            raise ValueError("pix_fmt %r frames are 1-D arrays of samples: give frame_shape=(H, W)" % (pix_fmt,))
        self.h, self.w = _frame_shape(frame_shape)
        self.pix_fmt, self.colour = pix_fmt, colour
        self.dtype = np.dtype(np.uint16 if _lib.YUV_FORMATS[pix_fmt][2] > 8 else np.uint8)
        self.kw = dict(pix_fmt=pix_fmt, matrix=colour.matrix, full_range=bool(colour.full_range), chroma=colour.chroma)
        self.nbytes = _yuv_surface(self.h, self.w, pitches=None, offsets=None, picture=bool(self.pad), **self.kw)[1]   # names and size fail here
        self.samples = self.nbytes // self.dtype.itemsize
        self.net = _padded_size(self.h, self.w, pix_fmt) if self.pad else (self.h, self.w)

    def geometry(self, a, clip):
        if a.dtype != self.dtype or a.ndim != (2 if clip else 1) or a.shape[-1] != self.samples:
            raise ValueError("expected %s %s [%s%d] (the tight %d x %d frame's samples), got %s %s"
                             % (self.pix_fmt, self.dtype.name, "T," if clip else "", self.samples, self.h, self.w, a.dtype, a.shape))
        return _Geometry(self.h, self.w, (a.shape[0], self.nbytes) if clip else (self.nbytes,), None, *self.net)

    def _decode(self, dev_in, geom, alpha, **kw):
        return yuv_to_input(dev_in, geom.h, geom.w, **self.kw, **kw), None

    def _encode(self, y, geom, alpha, **kw):
        return output_to_yuv(y, **self.kw, **kw)


class _RgbSurface(_Format):
    """the RGB surfaces of _lib.RGB_FORMATS but 'rgb24': self-describing arrays -- packed [H,W,3|4] uint8 / uint16, x2rgb10le / x2bgr10le
    [H,W] uint32, planar [P,H,W] -- or, with frame_shape=(H, W), 1-D arrays of the tight frame's samples (``ffmpeg -f rawvideo``'s bytes);
    staged as the tight surface's bytes, converted by bsvd_rgb_to_planar / bsvd_planar_to_rgb.  A format with alpha hands the frames' alpha
    codes from ``to_input`` to ``to_output`` as a device plane beside the tensor (``alpha=``): the pipelines keep it with its frame."""

    def __init__(self, pix_fmt, colour, pad=None, frame_shape=None):
        super().__init__(pad)
        if colour is None:
            colour = {}
        if not isinstance(colour, dict) or set(colour) - {"full_range"}:
            raise ValueError("colour: pix_fmt %r is RGB: a dict that may carry 'full_range' only (default True), got %r" % (pix_fmt, colour))
        self.pix_fmt, self.full_range = pix_fmt, bool(colour.get("full_range", True))
        layout, self.components, bits, _, fourth = _lib.RGB_FORMATS[pix_fmt]
        self.x2, self.planar = layout == _lib.RGB_PACKED_X2_10, layout == _lib.RGB_PLANAR
        self.has_alpha = fourth == _lib.FOURTH_ALPHA
        self.dtype = np.dtype(np.uint32 if self.x2 else np.uint16 if bits > 8 else np.uint8)
        self.per_pixel = 1 if self.x2 else self.components            # array elements per pixel
        self.hw = None
        if frame_shape is not None:
            self.hw = _frame_shape(frame_shape)
            self._size(*self.hw)                                      # a size the format cannot carry fails here, not at the first frame

    def _size(self, h, w):
        what = "%s %d x %d" % (self.pix_fmt, h, w)
        if self.pad:
            if h < 2 or w < 2:
                raise ValueError("expected frames of at least 2 x 2, got %d x %d" % (h, w))
            net = _padded_size(h, w, what)
        elif h <= 0 or w <= 0 or h % 4 or w % 4:
            raise ValueError("%s: H and W must be positive multiples of 4 (pad first: denoise.pad_to_multiple_of_4; or pad='reflect')" % what)
        else:
            net = (h, w)
        return net, rgb_frame_bytes(h, w, self.pix_fmt)

    def natural_shape(self, h, w):
        return (h, w) if self.x2 else (self.components, h, w) if self.planar else (h, w, self.components)

    def geometry(self, a, clip):
        shape = tuple(a.shape[1:]) if clip and a.ndim >= 1 else tuple(a.shape)
        hw = None
        if a.dtype == self.dtype and not (clip and a.ndim < 2):
            if len(shape) == 1:
                if self.hw is None:
                    raise ValueError("pix_fmt %r: a 1-D frame of samples does not say its picture size: give frame_shape=(H, W)" % (self.pix_fmt,))
                if shape[0] == self.hw[0] * self.hw[1] * self.per_pixel:
                    hw = self.hw
            elif self.x2 and len(shape) == 2:
                hw = shape
            elif self.planar and len(shape) == 3 and shape[0] == self.components:
                hw = shape[1:]
            elif not self.x2 and not self.planar and len(shape) == 3 and shape[2] == self.components:
                hw = shape[:2]
        if hw is None or (self.hw is not None and tuple(hw) != self.hw):
            raise ValueError("expected %s %s %s%s%s, got %s %s"
                             % (self.pix_fmt, self.dtype.name, "[T,...] of " if clip else "",
                                list(self.natural_shape(*(self.hw or ("H", "W")))),
                                " or the %d samples of the tight frame" % (self.hw[0] * self.hw[1] * self.per_pixel) if self.hw else "",
                                a.dtype, a.shape))
        h, w = int(hw[0]), int(hw[1])
        net, nbytes = self._size(h, w)
        return _Geometry(h, w, (a.shape[0], nbytes) if clip else (nbytes,), None, *net)

    def _decode(self, dev_in, geom, alpha, **kw):
        if not self.has_alpha:
            return rgb_to_input(dev_in, geom.h, geom.w, self.pix_fmt, full_range=self.full_range, **kw), None
        return rgb_to_input(dev_in, geom.h, geom.w, self.pix_fmt, full_range=self.full_range, return_alpha=True if alpha is None else alpha, **kw)

    def _encode(self, y, geom, alpha, **kw):
        return output_to_rgb(y, self.pix_fmt, full_range=self.full_range, alpha=alpha, **kw)


class _Ring:
    """What rides on the device beside a frame while the frame is inside LiveStream's network: ``slots`` entries (>= latency + depth),
    written in feed order and read in the order the frames come out -- the same order, through ``cut=True``, ``cuts='auto'`` and
    ``flush()``; an entry is written again ``slots`` feeds later, by when the step that read it has been waited for.  Allocated once with
    the stream's slots.  The subclasses say what an entry is and how the error names the ring."""
    what = None

    def __init__(self, slots, shape, dtype, device):
        self.buf = torch.empty((slots,) + shape, dtype=dtype, device=device)
        self.fed = self.emitted = 0

    def next_in(self):
        self.fed += 1
        return self.buf[(self.fed - 1) % self.buf.shape[0]]

    def next_out(self):
        if self.emitted >= self.fed:
            raise RuntimeError("%s ring: frame %d comes out before it went in" % (self.what, self.emitted))
        self.emitted += 1
        return self.buf[(self.emitted - 1) % self.buf.shape[0]]

    def reset(self):
        self.fed = self.emitted = 0


class _AlphaRing(_Ring):
    """frame k's alpha codes, a picture-sized plane [1,H,W] of the format's sample type"""
    what = "alpha"

    def __init__(self, planes, h, w, dtype, device):
        super().__init__(planes, (1, h, w), dtype, device)


class _SourceRing(_Ring):
    """for ``strength`` below 1 and grain='scene': frame k's three colour planes at network size, written by the decode's side; an entry
    is [1,3,Hp,Wp] fp32, what ``frame_io.blend_output`` takes as ``x``"""
    what = "source"

    def __init__(self, frames, h, w, device):
        super().__init__(frames, (1, 3, h, w), torch.float32, device)


class _TableRing(_Ring):
    """vst='scene': the table set frame k was transformed with, [1, VST_TABLE_FLOATS], mapped back with frame k's result"""
    what = "table"

    def __init__(self, sets, device):
        super().__init__(sets, (1, VST_TABLE_FLOATS), torch.float32, device)


class _Vst:
    """the pipelines' ``vst``: None, a NoiseCurve or 'scene', with ``vst_floor``.  Checked before anything touches a device.  ``active``:
    the transform runs; ``scene``: its curve is estimated at every scene start; ``fills``: the model has a noise plane for sigma';
    ``sigma_in``: what the decode is asked to put into that plane (the caller's ``sigma`` with vst=None: no kernel, no buffer and no
    argument more than before; the one value of a curve that is flat after the clamp, whose transform is the identity; otherwise 0,
    overwritten by the forward transform)."""

    def __init__(self, model, vst, vst_floor, sigma, what):
        self.floor = check_vst_floor(vst_floor)
        self.curve = self.shared = None
        self.active = self.scene = False
        self.sigma_in = sigma
        self.fills = False
        if vst is None:                                       # the defaults: the model is not looked at
            return
        if sigma is not None:
            raise ValueError("%s(vst=...): sigma must be None (the noise plane is the transform's sigma'), got %r" % (what, sigma))
        self.fills = model.net.net_in_ch != 3
        if isinstance(vst, NoiseCurve):
            flat = vst_identity(vst, self.floor)
            if flat is not None:                              # the identity: the constant plane of sigma=<that value>, nothing launched
                self.sigma_in = flat if self.fills else None
                return
            self.curve = vst
        elif isinstance(vst, str) and vst == "scene":
            self.scene = True
        else:
            raise ValueError("%s: vst must be None, a NoiseCurve or 'scene', got %r" % (what, vst))
        self.active = True
        self.sigma_in = 0.0 if self.fills else None

    def shared_tables(self, device):
        """vst=NoiseCurve: the stream's one table set [1, VST_TABLE_FLOATS], built at the first call"""
        if self.shared is None or self.shared.device != device:
            self.shared = build_vst(torch.tensor([self.curve.values], dtype=torch.float32).to(device), self.floor)
        return self.shared


class _Finish:
    """the pipelines' output finish: ``strength`` (a number or (luma, chroma)), ``dither`` / ``dither_seed``, the luma weights of the blend
    (``luma_matrix``: None = the stream's matrix for YUV formats, BT.709 for RGB ones).  Checked before anything touches a device.  With
    the defaults ``blends`` is False and ``dither_kw`` empty: no kernel, no buffer and no argument more than before."""

    def __init__(self, fmt, strength, dither, dither_seed, luma_matrix):
        self.strength = check_strength(strength)
        self.blends = self.strength != (1.0, 1.0)
        check_dither(dither, dither_seed)
        self.dither, self.seed = dither, int(dither_seed)
        colour = getattr(fmt, "colour", None)
        self.matrix = luma_matrix if luma_matrix is not None else colour.matrix if isinstance(colour, Colour) else "bt709"
        _luma_weights(self.matrix)
        self.emitted = 0                   # frames handed to the encoder since construction / the last flush: the dither's stream index

    def blend(self, y, x):
        return blend_output(y, x, self.strength, self.matrix)

    def dither_kw(self, frames):
        """the encoder's keywords for the next ``frames`` frames"""
        if self.dither is None:
            return {}
        f0, self.emitted = self.emitted, self.emitted + frames
        return dict(dither=self.dither, dither_seed=self.seed, frame0=f0)


class _Grain:
    """the pipelines' ``grain``: None, a GrainModel or 'scene', with ``grain_amount`` and ``grain_seed``; the luma weights are the
    finish's.  Checked before anything touches a device.  ``active``: grain is synthesised; ``scene``: its model is measured on the first
    frame of every scene to emerge; ``model``: the model in use; ``emitted``: the frames given grain since construction / the last flush,
    the stream index the block offsets are hashed from.  With the default nothing is allocated and nothing launched."""

    def __init__(self, grain, amount, seed, matrix):
        grain, self.amount, self.seed = check_grain(grain, amount, seed)
        self.active = grain is not None
        self.scene = isinstance(grain, str)
        self.model = grain if isinstance(grain, GrainModel) else None
        self.matrix = matrix
        self.emitted = 0

    def measure(self, src, y, picture):
        """the scene's model from its first frame: source and result [1,>=3,Hp,Wp]; the host waits for 2 KB of statistics here"""
        self.model = estimate_grain(src, y, picture=picture, matrix=self.matrix)
        return self.model

    def apply(self, y, frame0):
        return apply_grain(y, self.model, self.amount, self.seed, frame0, self.matrix)


def _pixel_format(pix_fmt, colour, pad=None, frame_shape=None):
    _check_pad(pad)
    if pix_fmt == "rgb24":
        if colour is not None:
            raise ValueError("colour describes a YUV surface; pix_fmt 'rgb24' takes none")
        return _Rgb24(pad)
    if pix_fmt in ("nv12", "p010"):
        return _Yuv420(pix_fmt, colour, pad)
    if pix_fmt in _lib.YUV_FORMATS:
        return _YuvSurface(pix_fmt, colour, pad, frame_shape)
    if isinstance(pix_fmt, str) and pix_fmt in _lib.RGB_FORMATS:
        return _RgbSurface(pix_fmt, colour, pad, frame_shape)
    raise ValueError("pix_fmt %r: one of 'rgb24', 'nv12', 'p010', %s" % (pix_fmt, ", ".join(repr(n) for n in sorted(set(_lib.YUV_FORMATS) | set(_lib.RGB_FORMATS) - {"rgb24"}))))


def _check_cuts_mode(cuts, cut_threshold, what):
    """the pipelines' ``cuts``: None or 'auto' -> (auto?, threshold).  Before anything touches a device."""
    if cuts is not None and not (isinstance(cuts, str) and cuts == "auto"):
        raise ValueError("%s: cuts must be None or 'auto' (known cuts: LiveStream.feed(frame, cut=True), BSVD.forward(cuts=[...])), got %r" % (what, cuts))
    return cuts is not None, check_cut_threshold(cut_threshold)


def _check_sigma(model, sigma, sigma_gain, what):
    """the pipelines' ``sigma``: None, a float, 'auto', 'nlf' or a NoiseCurve -- the last three need a noise-map channel to write into.
    Before anything touches a device."""
    if isinstance(sigma, str) or sigma is None or not hasattr(sigma, "__len__"):
        mode = _sigma_mode(sigma)[0]
    else:
        raise ValueError("%s: sigma must be None, a number, 'auto', 'nlf' or a NoiseCurve (per-frame values: frame_io.frames_to_input(sigma=[...]))" % what)
    if mode == "auto" and model.net.net_in_ch == 3:
        raise ValueError("%s(sigma='auto'): the model is blind (3 input channels): it has no noise map to estimate" % what)
    if mode in ("nlf", "curve") and model.net.net_in_ch == 3:
        raise ValueError("%s(sigma=%s): the model is blind (3 input channels): it has no noise map to write" % (what, "'nlf'" if mode == "nlf" else "NoiseCurve"))
    return _check_gain(sigma_gain)


_Side = collections.namedtuple("_Side", "dev pin")
# LiveStream's values that come down with a frame, each fp32: (name in ``_Slot.side``, length, the attribute that reports it once ``feed``
# has waited for the step, when the stream has it).  Written on the compute stream into ``dev``, copied to ``pin`` on the download stream
# behind the frame, read in ``_pop``: one value as a float, more as a list.
_SIDE_VALUES = (
    ("sigma", 1, "last_sigma", lambda live: live.auto_sigma),                                    # sigma='auto': the step's estimate
    ("curve", _lib.NLF_LEVELS, "last_noise_curve", lambda live: live.nlf_sigma or live.vst.scene),  # sigma='nlf' / vst='scene': the curve
    ("vsig", 1, "last_vst_sigma", lambda live: live.vst.active),                                 # vst=...: the frame's sigma'
)


class _Slot:
    def __init__(self):
        self.pin_in = self.pin_out = None
        self.dev_in = self.dev_out = None
        self.shape = None
        self.uploaded = torch.cuda.Event()
        self.computed = torch.cuda.Event()
        self.downloaded = torch.cuda.Event()
        self.ticket = None          # the in-flight clip occupying this slot
        self.side = {}                              # LiveStream: name -> _Side, the values of _SIDE_VALUES that come down beside the frame
        self.dev_alpha = None                       # ClipPipeline, formats with alpha: the clip's alpha plane [T,H,W], held like dev_out


class _Ticket:
    """One submitted clip: owns its slot until the download has been copied out of the pinned buffer."""

    def __init__(self, slot, dtype):
        self.slot, self.dtype, self.result = slot, dtype, None

    def finish(self):
        if self.slot is not None:
            self.slot.downloaded.synchronize()
            self.result = self.slot.pin_out.numpy().copy().view(self.dtype).reshape(self.slot.shape)
            self.slot.ticket = None
            self.slot = None
        return self.result


class _Pipeline:
    """What ClipPipeline and LiveStream share: the options of the module docstring, checked in one order before anything touches a
    device; the three streams; and the chain from the network's result to the surface."""

    def __init__(self, what, model, sigma, depth, pix_fmt, colour, pad, frame_shape, sigma_gain, cuts, cut_threshold, strength, dither,
                 dither_seed, luma_matrix, vst, vst_floor, grain, grain_amount, grain_seed):
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.auto_cuts, self.cut_threshold = _check_cuts_mode(cuts, cut_threshold, what)
        self.sigma_gain = _check_sigma(model, sigma, sigma_gain, what)
        self.vst = _Vst(model, vst, vst_floor, sigma, what)
        self.fmt = _pixel_format(pix_fmt, colour, pad, frame_shape)
        self.finish = _Finish(self.fmt, strength, dither, dither_seed, luma_matrix)
        self.grain = _Grain(grain, grain_amount, grain_seed, self.finish.matrix)
        self.last_grain_model = self.grain.model
        self.model, self.sigma, self.depth = model, sigma, depth
        self.device = model._device()
        if self.device.type != "cuda":
            raise RuntimeError("%s needs the model on a HIP device (model.cuda())" % what)
        with torch.cuda.device(self.device):
            self.up, self.comp, self.down = (torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream())
        self.count = 0

    def _emit(self, y, geom, tables, src, alpha, grain):
        """the chain behind the network, on the compute stream: the inverse transform with the table sets the frames went in with, the
        strength blend with their source ``src``, grain -- ``grain(y, src, geom)``: each pipeline's own, which knows its scenes --, the dither
        keywords, and the encoder with the frames' alpha codes"""
        y = y.float()
        if self.vst.active:
            y = vst_inverse(y.contiguous(), tables)
        if self.finish.blends:
            y = self.finish.blend(y.contiguous(), src)
        if self.grain.active:
            y = grain(y.contiguous(), src, geom)
        return self.fmt.to_output(y, geom, alpha=alpha, **self.finish.dither_kw(y.shape[0]))


class ClipPipeline(_Pipeline):
    """model: a bsvd_amd.BSVD on a HIP device; clips in, clips out, in submission order.  The options are the module docstring's (sigma:
    the noise std in [0,1] units for the constant noise map, None for a blind model); what is ClipPipeline's own:

    depth >= 2 overlaps the transfers of one clip with the forward of another.
    Clips are arrays [T,...] of what the module docstring says a frame of ``pix_fmt`` is: [T,H,W,3] uint8 for 'rgb24', [T,H*3/2,pitch] for
    'nv12' / 'p010', [T, n] tight samples with frame_shape=(H, W) for the planar, 4:2:2 and 4:4:4 YUV surfaces, [T,...] self-describing
    frames (or [T, n] with frame_shape) for the RGB surfaces; the results have the shape and dtype of what was submitted.  The alpha codes
    of a clip stay on the device beside the clip and come back with their frames.
    sigma='auto' / 'nlf': every frame of a clip gets its own estimate; nothing is reported to the host.
    cuts='auto': the scene starts of every clip are detected (``frame_io.scene_cuts`` at ``cut_threshold``) and handed to the model's
    forward, which runs every scene as a clip of its own.  The detection reads T integers back before the forward is enqueued: the host
    waits for the clip's upload and conversion there.  ``last_cuts``: the cuts of the most recent clip submitted.
    strength blends with the clip's own input; the frame index of dither='random' and of the grain pattern counts the frames submitted
    since construction.
    vst='scene' / grain='scene': the clip's scenes are its ``last_cuts`` with cuts='auto', otherwise the clip is one scene.  Each scene's
    curve is estimated from its first frame alone, and the table sets are per frame in one forward and one inverse launch.  The first
    frame of each scene is measured against the clip's own input for the grain model: the host waits once per scene."""

    def __init__(self, model, sigma=None, depth=2, pix_fmt="rgb24", colour=None, pad=None, frame_shape=None, sigma_gain=1.0, cuts=None,
                 cut_threshold=CUT_THRESHOLD, strength=1.0, dither=None, dither_seed=0, luma_matrix=None, vst=None, vst_floor=VST_FLOOR,
                 grain=None, grain_amount=1.0, grain_seed=0):
        super().__init__("ClipPipeline", model, sigma, depth, pix_fmt, colour, pad, frame_shape, sigma_gain, cuts, cut_threshold, strength, dither,
                         dither_seed, luma_matrix, vst, vst_floor, grain, grain_amount, grain_seed)
        self.last_cuts = None
        with torch.cuda.device(self.device):
            self.slots = [_Slot() for _ in range(depth)]
        self.pending = collections.deque()

    # ------------------------------------------------------------------------------------------------
    def submit(self, frames_u8):
        """frames_u8: numpy uint8 [T,H,W,3] (RGB); with pix_fmt 'nv12' / 'p010' uint8 / uint16 [T,H*3/2,pitch].  Enqueues upload +
        forward + download; returns immediately unless the ring is full (then it first drains the oldest clip into its result)."""
        frames_u8 = np.ascontiguousarray(frames_u8)
        geom = self.fmt.geometry(frames_u8, clip=True)
        slot = self.slots[self.count % len(self.slots)]
        self.count += 1
        if slot.ticket is not None:
            slot.ticket.finish()               # ring full: the oldest clip's result leaves the pinned buffer first
        with torch.cuda.device(self.device):
            if slot.shape != frames_u8.shape:
                slot.shape = frames_u8.shape
                slot.pin_in = torch.empty(geom.staging, dtype=torch.uint8).pin_memory()
                slot.pin_out = torch.empty(geom.staging, dtype=torch.uint8).pin_memory()
                slot.dev_in = torch.empty(geom.staging, dtype=torch.uint8, device=self.device)
            slot.pin_in.numpy()[...] = frames_u8.view(np.uint8).reshape(geom.staging)
            with torch.cuda.stream(self.up):
                slot.dev_in.copy_(slot.pin_in, non_blocking=True)
                slot.uploaded.record()
            with torch.cuda.stream(self.comp):
                self.comp.wait_event(slot.uploaded)
                # a format with alpha: the clip's alpha codes ride beside the clip, [T,H,W] on the device, held like dev_out
                x, slot.dev_alpha = self.fmt.to_input(slot.dev_in, geom, self.vst.sigma_in, self.sigma_gain)
                T, _, H, W = x.shape
                kw = {}
                if self.auto_cuts:
                    self.last_cuts = scene_cuts(x, self.cut_threshold, picture=(geom.h, geom.w))
                    kw = dict(cuts=self.last_cuts)
                src, tables = x, None
                if self.vst.active:
                    if self.finish.blends or self.grain.scene:
                        src = x[:, :3].clone()            # strength blends, and grain is measured, in the picture's own domain
                    tables = self._clip_tables(x, geom)
                    vst_forward(x, tables, fill_plane=self.vst.fills)
                if self.model._pick_mode(T, H, W) == "clip":
                    y = self.model.clip_forward(x, **kw)
                else:
                    y = self.model.streaming_forward(x, **kw)
                # held by the slot until its download completed
                slot.dev_out = self._emit(y, geom, tables, src, slot.dev_alpha, self._clip_grain)
                slot.computed.record()
            with torch.cuda.stream(self.down):
                self.down.wait_event(slot.computed)
                slot.pin_out.copy_(slot.dev_out, non_blocking=True)
                slot.downloaded.record()
        slot.ticket = _Ticket(slot, self.fmt.dtype)
        self.pending.append(slot.ticket)
        return slot.ticket

    def _clip_tables(self, x, geom):
        """the clip's table sets: the stream's one set (vst=NoiseCurve), or with vst='scene' one set per frame, [T, VST_TABLE_FLOATS]: each
        scene's tables, built from the curve of its first frame, repeated over its frames -- all of it on the device"""
        if not self.vst.scene:
            return self.vst.shared_tables(x.device)
        T = x.shape[0]
        starts = [0] + [int(c) for c in (self.last_cuts or []) if 0 < int(c) < T] if self.auto_cuts else [0]
        first = x if len(starts) == T else x[starts].contiguous()
        sets = build_vst(estimate_noise_curve(first, picture=(geom.h, geom.w), gain=self.sigma_gain), self.vst.floor)
        scene_of = [sum(1 for s in starts[1:] if s <= t) for t in range(T)]
        return sets if len(starts) == T else sets[scene_of].contiguous()

    def _clip_grain(self, y, src, geom):
        """grain onto the clip's result, in place: the caller's model, or with grain='scene' each scene's own, measured on its first frame"""
        T = y.shape[0]
        starts = [0] + [int(c) for c in (self.last_cuts or []) if 0 < int(c) < T] if self.auto_cuts and self.grain.scene else [0]
        for a, b in zip(starts, starts[1:] + [T]):
            if self.grain.scene:
                self.last_grain_model = self.grain.measure(src[a:a + 1], y[a:a + 1], (geom.h, geom.w))
            self.grain.apply(y[a:b], self.grain.emitted + a)
        self.grain.emitted += T
        return y

    def results(self):
        """Drains every clip submitted so far, in submission order."""
        while self.pending:
            yield self.pending.popleft().finish()

    def run(self, clips):
        """clips: iterable of uint8 [T,H,W,3] arrays (or of the pix_fmt's surfaces) -> generator of the denoised arrays of the same
        shape and dtype, in order, with up to ``depth`` clips in flight."""
        for clip in clips:
            if len(self.pending) == len(self.slots):
                yield self.pending.popleft().finish()
            self.submit(clip)
        yield from self.results()


class LiveStream(_Pipeline):
    """One live feed through the per-frame streaming API (``BSVD.feedin_one_element``, bsvd_arch.py:485-488) with uint8 frames
    on the host side: the streaming counterpart of ``ClipPipeline``.

        feed(frame)  : uint8 [H,W,3] (RGB) -> enqueues upload (uint8 over PCIe), ``bsvd_u8_to_planar``, one pipeline step (a
                       HIP-graph replay), ``bsvd_planar_to_u8`` and the download of whatever that step emitted on three HIP
                       streams, then waits for the step fed ``depth-1`` calls earlier and returns the frame it emitted (None
                       while the 16-step pipeline fills).
        flush()      : feeds the 16 + 1 ``None`` steps of the reference's ``streaming_forward`` tail (:530-544), returns the
                       remaining denoised frames in order and resets the stream.

    Frame k comes back ``model.shift_num`` (16) feeds after it went in -- the network's own latency -- plus ``depth-1``
    feeds of host pipelining (``depth=1``: every feed waits for its own step, lowest latency; ``depth>=2``: transfers of one
    step overlap the compute of the next, highest rate).  ``overlap_blocks`` (default: on for ``depth >= 2``) additionally lets
    DenBlock 2 run one step behind DenBlock 1 as a parallel graph branch (``BSVD.feed_overlapped``): one more feed of latency
    (``shift_num + depth`` in total), the single-frame launches of two independent chains share the chip.  Results keep
    submission order and are byte-identical in every mode.  Not re-entrant (one stream per instance, like the reference's
    module state).

    The options are the module docstring's; what is the stream's own:

    feed takes and returns one frame of ``pix_fmt`` as the module docstring describes it ([H*3/2,pitch] surfaces for 'nv12' / 'p010', 1-D
    tight samples for the planar, 4:2:2 and 4:4:4 YUV surfaces -- ``frame_shape`` is required --, self-describing arrays or, with
    ``frame_shape``, 1-D tight samples for the RGB surfaces); with pad='reflect' latency is the same and frames come back in the fed
    shape.  What waits on the device for frame k's result, ``latency`` feeds later, waits in a ring of ``latency + depth`` entries
    (``_Ring``), allocated with the slots, filled on the decode's side and consumed in order on the encode's, through ``cut=True``,
    cuts='auto' and ``flush()``; nothing is allocated per feed:
      alpha       a picture-sized plane of codes per entry: the frame returned for source frame k carries frame k's alpha bit for bit;
      strength    below 1 (and grain='scene'): frame k's three colour planes at network size, 3 fp32 planes per entry -- about 0.5 GB at
                  1080p --, blended with frame k's result when that emerges;
      vst='scene' the table set frame k was transformed with (8 KB per entry).

    sigma='auto' / 'nlf' run on the compute stream between the conversion and the pipeline step; latency, slot ring and stream order are
    what they are with a float.  ``last_sigma`` ('auto'; a float, [0,1] units), ``last_noise_curve`` ('nlf' and vst='scene'; sixteen
    values) and ``last_vst_sigma`` (vst): the values of the most recent input step ``feed`` has already waited for -- i.e. of the frame
    fed ``depth - 1`` calls ago --, None before that and None for what the stream does not estimate (sigma='nlf' leaves ``last_sigma``
    None); they come down on the download stream into the slot's pinned memory beside the frame and are never read earlier.

    Scene cuts.  ``feed(frame, cut=True)`` says that ``frame`` starts a new scene: no temporal-fusion conv mixes it with the frames before it
    (each side sees zeros for the other, as at a stream's ends), nothing is flushed and no feed returns None because of it.  The steps a cut
    passes through have launch plans of their own: batched launches at the first sighting, captured when the same ring phase recurs.
    cuts='auto' finds the cuts itself (``cut=True`` is refused then): the conversion, the two detector kernels (``frame_io.scene_scores``
    against the previous frame's grid, kept on the device) and an 8-byte copy run on the upload stream behind the frame's copy, and the host
    waits for them before it plans the step -- the step before is already enqueued, so ``depth >= 2`` keeps its overlap.  A frame whose score
    (``frame_io.scene_cuts``' rule, carried from frame to frame) reaches ``cut_threshold`` starts a scene.  ``last_cut_score`` /
    ``last_cut``: score and decision of the most recent frame fed.  ``flush()`` forgets the previous frame.  With cuts=None the stream order
    is what it always was.

    A scene starts with the first feed after construction or ``flush()``, a ``feed(frame, cut=True)`` frame, or a frame cuts='auto' flags.
    vst, on the compute stream: after the conversion, the source ring's copy of the untransformed planes and the cut decision come curve,
    build and forward, then the pipeline step; what emerges goes through the inverse, then the strength blend and the encoder.  A
    NoiseCurve: one table set for the stream, built once.  'scene': the frame that starts a scene gets its curve and a table set built
    from it, and every later frame of the scene uses that set.
    grain, on the compute stream: 'scene' notes whether a frame starts a scene when it is fed; when the first frame of a scene EMERGES,
    ``latency`` feeds later, its source (from the source ring) and its result are measured, the HOST WAITS for the 2 KB of statistics
    and fits the model -- once per scene --, and that model is used from that frame to the scene's last.
    The frame index of dither='random' and of the grain pattern counts the frames emitted since construction or the last ``flush()``."""

    def __init__(self, model, sigma=None, depth=2, overlap_blocks=None, frame_shape=None, pix_fmt="rgb24", colour=None, pad=None,
                 sigma_gain=1.0, cuts=None, cut_threshold=CUT_THRESHOLD, strength=1.0, dither=None, dither_seed=0, luma_matrix=None,
                 vst=None, vst_floor=VST_FLOOR, grain=None, grain_amount=1.0, grain_seed=0):
        """frame_shape: optional (H, W) of the frames to come (the picture, also with ``pad``) -- the overlap decision (and with it
        ``latency``) is then final at construction instead of at the first feed."""
        super().__init__("LiveStream", model, sigma, depth, pix_fmt, colour, pad, frame_shape, sigma_gain, cuts, cut_threshold, strength, dither,
                         dither_seed, luma_matrix, vst, vst_floor, grain, grain_amount, grain_seed)
        self.last_cut_score, self.last_cut = None, False
        self._grids = self._sad = self._pin_sad = None       # cuts='auto': two alternating grid buffers, the step's sum on the device and pinned
        self._have_prev, self._prev_mafd, self._n_scored = False, 0.0, 0
        self._tables = self._scene_tables = self._scene_curve = None    # vst='scene': the ring of table sets, the current scene's set and curve
        self._in_scene = False
        self.auto_sigma = isinstance(sigma, str) and sigma == "auto"
        self.nlf_sigma = isinstance(sigma, str) and sigma == "nlf"
        self._side = [row for row in _SIDE_VALUES if row[3](self)]     # the values this stream brings down beside its frames
        self.last_sigma = self.last_noise_curve = self.last_vst_sigma = None
        self._alpha = None                                    # formats with alpha: the ring of alpha planes (_AlphaRing), allocated with the slots
        self._source = None                                   # strength < 1 or grain='scene': the ring of source frames (_SourceRing), allocated with the slots
        self._scene_starts = collections.deque()             # grain='scene': per frame inside the network, does it start a scene?
        self._grain_in_scene = False
        self._overlap_wanted = (depth >= 2) if overlap_blocks is None else bool(overlap_blocks)
        self._overlap_explicit = overlap_blocks is not None
        self.overlap = self._overlap_wanted
        self._overlap_decided = not self._overlap_wanted     # nothing to decide without the lagged schedule
        self.slots, self.shape, self.geom = None, None, None
        self.inflight = collections.deque()          # (slot, has_output, has_sigma) in submission order
        model.reset()
        if frame_shape is not None:
            h, w = _frame_shape(frame_shape)
            self._decide_overlap(*(_padded_size(h, w, "frame_shape") if pad else (h, w)))

    @property
    def latency(self):
        """feeds between a frame going in and coming out: ``shift_num + depth - 1``, + 1 with the lagged two-branch schedule.  Final once
        ``latency_final`` is True -- from construction when ``frame_shape`` was given or overlap is off, else from the first feed (a default
        ``overlap_blocks=None`` falls back to the plain per-frame feed when the ring engine is not available for the frame size)."""
        return self.model.shift_num + self.depth - 1 + (1 if self.overlap else 0)

    @property
    def latency_final(self):
        return self._overlap_decided

    def _decide_overlap(self, h, w):
        """The lagged two-branch schedule needs the ring engine (stream_rings, planar edge layers, rings that fit the free HBM).  Decided
        once per stream, BEFORE its first frame touches the pipeline: a default (overlap_blocks=None) falls back to the plain per-frame
        feed -- one feed less latency, same frames --, an explicit overlap_blocks=True raises here with the stream still untouched (and
        the decision still open: a retried feed raises the same error again instead of failing half-way through a step).  flush() and a
        new frame size re-open the decision."""
        if self._overlap_decided:
            return
        if not self.model.overlap_available((self.model.net.net_in_ch, h, w)):
            if self._overlap_explicit:
                raise RuntimeError("LiveStream(overlap_blocks=True) needs the ring engine (stream_rings=True, planar edge layers, "
                                   "enough free HBM for the rings); use overlap_blocks=False")
            self.overlap = False
        self._overlap_decided = True

    def _reopen_overlap(self):
        self.overlap = self._overlap_wanted
        self._overlap_decided = not self._overlap_wanted

    def _alloc(self, shape, geom):
        self.shape, self.geom = shape, geom
        self.slots = []
        for _ in range(self.depth):                   # step k reuses the slot of step k - depth, which has been handed out
            s = _Slot()
            s.pin_in = torch.empty(geom.staging, dtype=torch.uint8).pin_memory()
            s.pin_out = torch.empty(geom.staging, dtype=torch.uint8).pin_memory()
            s.dev_in = torch.empty((1,) + geom.staging, dtype=torch.uint8, device=self.device)
            for name, n, _, _ in self._side:
                s.side[name] = _Side(torch.empty(n, dtype=torch.float32, device=self.device), torch.zeros(n, dtype=torch.float32).pin_memory())
            self.slots.append(s)
        if self.vst.scene:
            self._tables = _TableRing(self.latency + self.depth, self.device)
            self._scene_tables = torch.empty((1, VST_TABLE_FLOATS), dtype=torch.float32, device=self.device)
            self._scene_curve = torch.empty((1, _lib.NLF_LEVELS), dtype=torch.float32, device=self.device)
            self._in_scene = False
        if self.fmt.has_alpha:
            self._alpha = _AlphaRing(self.latency + self.depth, geom.h, geom.w, getattr(torch, self.fmt.dtype.name), self.device)
        self._source = _SourceRing(self.latency + self.depth, geom.net_h, geom.net_w, self.device) if self.finish.blends or self.grain.scene else None
        if self.auto_cuts:
            gh, gw = geom.h // 16, geom.w // 16
            self._grids = torch.zeros((2, 1, gh, gw), dtype=torch.int32, device=self.device)
            self._sad = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._pin_sad = torch.zeros(1, dtype=torch.int64).pin_memory()
            self._scored = torch.cuda.Event()
            self._forget_scene()

    def _forget_scene(self):
        self._have_prev, self._prev_mafd = False, 0.0

    def _detect(self, slot):
        """cuts='auto', on the upload stream behind the frame's copy: conversion, grid, difference against the previous frame's grid, 8 bytes
        to pinned memory; the host waits for them and decides.  -> (the network input, handed on to the compute stream; cut?)"""
        x = self._to_input(slot)
        x.record_stream(self.comp)
        cur = self._grids[self._n_scored % 2]
        prev = self._grids[(self._n_scored + 1) % 2][0] if self._have_prev else None
        scene_scores(x, picture=(self.geom.h, self.geom.w), prev=prev, out=(self._sad, cur))
        self._pin_sad.copy_(self._sad, non_blocking=True)
        self._scored.record()
        slot.uploaded.record()
        self._scored.synchronize()
        score, mafd = cut_scores([int(self._pin_sad[0])], cur.shape[1] * cur.shape[2], self._prev_mafd)
        self._n_scored += 1
        self._have_prev, self._prev_mafd = True, mafd[0]
        self.last_cut_score = score[0]
        self.last_cut = score[0] >= self.cut_threshold
        return x, self.last_cut

    def _to_input(self, slot):
        """the slot's frame -> the network input; a format with alpha leaves the frame's alpha codes in the ring's next plane"""
        sigma = 0.0 if self.nlf_sigma else self.vst.sigma_in
        x, _ = self.fmt.to_input(slot.dev_in, self.geom, sigma, self.sigma_gain, alpha=self._alpha.next_in() if self._alpha is not None else None)
        if self.nlf_sigma:                                   # what sigma='nlf' does inside to_input, with the curve kept for the host
            curve = estimate_noise_curve(x, picture=(self.geom.h, self.geom.w), gain=self.sigma_gain)
            fill_noise_map(x, curve)
            slot.side["curve"].dev.copy_(curve[0])
        if self._source is not None:
            self._source.next_in().copy_(x[:, :3])          # the frame's colour planes wait for its denoised self
        return x

    def _vst_forward(self, slot, x, cut):
        """vst=, on the compute stream behind the conversion, the source ring's copy and the cut decision: at a scene start ('scene') the
        curve and its table set; the frame's set into the ring; the forward transform.  The host waits for none of it."""
        if self.vst.scene:
            if cut or not self._in_scene:
                estimate = estimate_noise_curve(x, picture=(self.geom.h, self.geom.w), gain=self.sigma_gain)
                self._scene_curve.copy_(estimate)
                build_vst(self._scene_curve, self.vst.floor, out=self._scene_tables)
                self._in_scene = True
            tables = self._tables.next_in()
            tables.copy_(self._scene_tables)                 # frame k's set waits for frame k's result
            slot.side["curve"].dev.copy_(self._scene_curve[0])
        else:
            tables = self.vst.shared_tables(self.device)
        slot.side["vsig"].dev.copy_(vst_sigma(tables))
        vst_forward(x, tables, fill_plane=self.vst.fills)

    def _to_output(self, y):
        """what a step emitted -> the surface; frames come out in the order they went in, and so do their alpha planes"""
        tables = None
        if self.vst.active:
            tables = self._tables.next_out() if self.vst.scene else self.vst.shared_tables(self.device)
        src = self._source.next_out() if self._source is not None else None
        return self._emit(y, self.geom, tables, src, self._alpha.next_out() if self._alpha is not None else None, self._stream_grain)

    def _stream_grain(self, y, src, geom):
        """grain onto the frame that emerges, in place: the caller's model, or with grain='scene' the scene's own"""
        if self.grain.scene and self._scene_starts.popleft():        # the scene's first frame emerges: measure, wait, fit
            self.last_grain_model = self.grain.measure(src, y, (geom.h, geom.w))
        self.grain.apply(y, self.grain.emitted)
        self.grain.emitted += y.shape[0]
        return y

    def _pop(self):
        """oldest in-flight step -> its uint8 frame, or None if that step emitted nothing (pipeline fill)"""
        slot, has_out, has_sigma = self.inflight.popleft()
        slot.downloaded.synchronize()
        if has_sigma:
            for name, n, attr, _ in self._side:
                pin = slot.side[name].pin
                setattr(self, attr, float(pin[0]) if n == 1 else [float(v) for v in pin])
        return slot.pin_out.numpy().copy().view(self.fmt.dtype).reshape(self.shape) if has_out else None

    def _step(self, frame_u8, last=False, cut=False):
        if frame_u8 is not None:
            self._decide_overlap(self.geom.net_h, self.geom.net_w)
        slot = self.slots[self.count % len(self.slots)]
        self.count += 1
        with torch.cuda.device(self.device):
            x = None
            if frame_u8 is not None:
                slot.pin_in.numpy()[...] = frame_u8.view(np.uint8).reshape(self.geom.staging)
                with torch.cuda.stream(self.up):
                    slot.dev_in[0].copy_(slot.pin_in, non_blocking=True)
                    if self.auto_cuts:
                        x, cut = self._detect(slot)
                    else:
                        slot.uploaded.record()
            with torch.cuda.stream(self.comp):
                if frame_u8 is not None:
                    self.comp.wait_event(slot.uploaded)
                    if x is None:
                        x = self._to_input(slot)
                    if self.auto_sigma:
                        slot.side["sigma"].dev.copy_(x[0, -1, 0, :1])          # the plane holds the estimate: one element of it, device to device
                    if self.vst.active:
                        self._vst_forward(slot, x, cut)
                    if self.grain.scene:
                        self._scene_starts.append(bool(cut) or not self._grain_in_scene)
                        self._grain_in_scene = True
                kw = dict(cut=True) if cut else {}
                y = self.model.feed_overlapped(x, last=last, **kw) if self.overlap else self.model.feedin_one_element(x, **kw)
                if y is not None:
                    slot.dev_out = self._to_output(y)             # held by the slot until its download completed
                slot.computed.record()
            with torch.cuda.stream(self.down):
                self.down.wait_event(slot.computed)
                if y is not None:
                    slot.pin_out.copy_(slot.dev_out[0], non_blocking=True)
                if frame_u8 is not None:
                    for side in slot.side.values():
                        side.pin.copy_(side.dev, non_blocking=True)
                slot.downloaded.record()
        self.inflight.append((slot, y is not None, bool(self._side) and frame_u8 is not None))

    def _drain(self, keep, outs):
        while len(self.inflight) > keep:
            r = self._pop()
            if r is not None:
                outs.append(r)

    def feed(self, frame_u8, cut=False):
        """cut=True: this frame starts a new scene (refused with cuts='auto', which decides that itself)"""
        if cut and self.auto_cuts:
            raise ValueError("LiveStream(cuts='auto') finds the cuts itself: feed(frame, cut=True) is for streams constructed with cuts=None")
        frame_u8 = np.ascontiguousarray(frame_u8)
        geom = self.fmt.geometry(frame_u8, clip=False)
        if self.shape != frame_u8.shape:
            if self.inflight:
                raise ValueError("frame size changed mid-stream; flush() first")
            self._reopen_overlap()                    # the rings of another frame size may or may not fit
            self._alloc(frame_u8.shape, geom)
        self._step(frame_u8, cut=bool(cut))           # step k is in flight ...
        outs = []
        self._drain(self.depth - 1, outs)             # ... while step k - (depth-1) is waited for and handed out
        return outs[0] if outs else None

    def flush(self):
        """end of the feed: the 16 + 1 ``None`` steps of streaming_forward's tail, then everything in flight; returns the
        remaining frames, oldest first, and resets the stream"""
        outs = []
        if self.slots is None:
            return outs
        for _ in range(self.model.shift_num + 1):
            self._step(None)
            self._drain(self.depth - 1, outs)
        if self.overlap:                              # the lagging DenBlock-2 step of the last flush feed
            self._step(None, last=True)
        self._drain(0, outs)
        self.model.reset()
        self._forget_scene()
        if self._alpha is not None:
            self._alpha.reset()
        if self._source is not None:
            self._source.reset()
        if self._tables is not None:
            self._tables.reset()
        self._in_scene = False
        self.finish.emitted = 0
        self.grain.emitted = 0
        self._scene_starts.clear()
        self._grain_in_scene = False
        self._reopen_overlap()                        # the next stream decides again (free HBM may have changed)
        return outs
