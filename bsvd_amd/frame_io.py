"""uint8 frame I/O on the device: upload frames as uint8 (4x less PCIe traffic than fp32), build the
network input (RGB/255 + constant sigma map, the tensor ``temp_denoise`` hands to the model,
/root/reference/Experimental_root/models/validation_seq_infer.py:15-24) and turn the result into uint8 with the
reference's clamp + round (``tensor2img``, /root/reference/BasicSR/basicsr/utils/img_util.py:66,87-90) -- both on the GPU.

The same two steps for YUV 4:2:0 surfaces (NV12, P010), the formats decoders, capture cards and encoders speak:
``yuv420_to_input`` / ``output_to_yuv420`` (include/bsvd_hip.h, bsvd_yuv420_to_planar / bsvd_planar_to_yuv420; 1.5 or 3 bytes per
pixel over PCIe instead of RGB24's 3, and no colour conversion on the host).  And for the surfaces a pipeline meets besides those two --
planar 4:2:0, 4:2:2 (packed, semi-planar, planar) and planar 4:4:4, 8 and 10 bit, by ffmpeg's names (``_lib.YUV_FORMATS``):
``yuv_to_input`` / ``output_to_yuv`` (bsvd_yuv_to_planar / bsvd_planar_to_yuv), with a pitch and an offset per plane.

RGB as callers hold it who do not come through a video decoder (``_lib.RGB_FORMATS``, ffmpeg's names): packed 8 and 16 bit in any component
order with alpha or a filler, x2rgb10le / x2bgr10le, planar gbrp / gbrap at 8 to 16 bits -- ``rgb_to_input`` / ``output_to_rgb``
(bsvd_rgb_to_planar / bsvd_planar_to_rgb).  Alpha never meets the arithmetic: it comes out of ``rgb_to_input(return_alpha=True)`` as a
plane of codes and goes back in through ``output_to_rgb(alpha=)``.

Any picture size: the network needs H and W to be multiples of 4, and the reference's callers reflect-pad the fp32 tensor on the right and
bottom and crop the result (``denoise.pad_to_multiple_of_4`` / ``crop_padding`` here).  ``pad_to=(Hp, Wp)`` on the way in and
``crop_to=(H, W)`` on the way out do both inside the conversion kernels (bsvd_*_pad / bsvd_*_crop): the frames stay picture-sized uint8 /
YUV on the host and over PCIe.  ``network_size(H, W)`` is the (Hp, Wp) the pipelines use.  Without them every function is what it was.

The noise level: ``sigma`` is a float (the constant the caller knows, as before), ``'auto'`` (one estimate per frame, computed on the device
from the converted frame and written into that frame's noise-map plane -- ``estimate_sigma``; nothing crosses to the host and nothing waits
for it), a sequence of per-frame values, or a device tensor [T].  For sources whose noise depends on the signal level: ``'nlf'`` (a
noise-level function per frame, sigma at sixteen levels of local intensity, estimated on the device, and a per-pixel noise map written from
it -- ``estimate_noise_curve`` / ``fill_noise_map``) or a ``NoiseCurve`` the caller knows (``NoiseCurve.from_model(a, b)`` for a sensor's
Poisson-Gaussian parameters).  The same curve as a variance-stabilising transform, which keeps the constant noise plane the reference's
checkpoints were trained with: ``build_vst`` (the tables, on the device), ``vst_forward`` / ``vst_inverse`` (in place, around the network),
``vst_sigma`` -- the pipelines' ``vst=``.

Scene cuts: ``scene_scores`` (a 16 x 16 block grid of 8-bit luma sums per frame and its frame-to-frame difference, on the device, in
integers) and ``scene_cuts`` (the rule on top, on the host) find the frames that start a new scene, for the ``cuts=`` / ``cut=`` arguments of
the model's forward functions.  Untested on real footage.

The output finish: ``blend_output`` (the denoise strength: the network's result blended with its input, separate luma and chroma amounts,
in place, with exact ends) and ``dither=`` on ``output_to_yuv420`` / ``output_to_yuv`` / ``output_to_rgb`` (ordered or random dither at the
quantiser; a whole code is never moved) -- include/bsvd_hip.h, bsvd_blend_planar / BsvdDither.  The defaults call what was called before.

Film grain: ``estimate_grain`` (the statistics of the noise the network removed, taken on the device in integers -- ``grain_stats`` -- and
a model fitted to them on the host: ``GrainModel``, standard deviation against brightness and a spatial autoregression per component) and
``apply_grain`` (clean grain synthesised from a model onto the result, on the device) -- include/bsvd_hip.h, bsvd_grain_stats /
bsvd_grain_apply; the pipelines' ``grain=``.  Untested on real footage; no encoder has read the model."""
import ctypes

import numpy as np
import torch

from . import _lib
from .engine import require_hip


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def network_size(H, W):
    """-> (Hp, Wp): H and W rounded up to the next multiples of 4, the size the network runs a H x W picture at"""
    return (int(H) + 3) // 4 * 4, (int(W) + 3) // 4 * 4


def _call(device, name, *args):
    """the one way into the library's launching entry points: ``name(*args, stream)`` on ``device`` and torch's current stream there;
    a status other than 0 raises under that name"""
    lib = require_hip()
    with torch.cuda.device(device):
        _lib.check(getattr(lib, name)(*args, _stream()), name)


def _pair(v, what):
    try:
        a, b = v
        return int(a), int(b)
    except (TypeError, ValueError):
        raise ValueError("%s: expected a pair of ints, got %r" % (what, v)) from None


def _number(v, message, cast=float):
    """cast(v), or ValueError(message) for what is no number"""
    try:
        return cast(v)
    except (TypeError, ValueError):
        raise ValueError(message) from None


def _tensor(t, dtype, shape, device, message, contiguous=True):
    """the tensor-argument check: ``dtype`` (one, or a tuple of them), ``shape`` (None: any length), ``device`` (a torch.device, or 'cuda':
    any HIP device) and contiguity -> t; ValueError(message) otherwise"""
    if (not isinstance(t, torch.Tensor) or t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,))
            or (not t.is_cuda if device == "cuda" else t.device != device) or t.dim() != len(shape)
            or any(n is not None and s != n for s, n in zip(t.shape, shape)) or (contiguous and not t.is_contiguous())):
        raise ValueError(message)
    return t


# ---------------------------------------------------------------------------------------------------
# the noise level: estimated per frame on the device, or given per frame (include/bsvd_hip.h, bsvd_estimate_sigma / bsvd_fill_sigma_plane)

SIGMA_BINS = _lib.SIGMA_BINS
SIGMA_MAX = _lib.SIGMA_MAX          # where the estimate saturates: 1 / (6 * 0.6745) = 0.2471 (63 / 255)


def _check_clamp(clamp):
    """-> (lo, hi) floats with 0 <= lo <= hi, both finite; ValueError otherwise"""
    try:
        lo, hi = clamp
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError("clamp: expected a pair (lo, hi), got %r" % (clamp,)) from None
    if not (0.0 <= lo <= hi < float("inf")):
        raise ValueError("clamp %r: 0 <= lo <= hi, both finite" % (clamp,))
    return lo, hi


def _check_gain(gain):
    g = _number(gain, "sigma_gain: expected a positive number, got %r" % (gain,))
    if not (0.0 < g < float("inf")):
        raise ValueError("sigma_gain %r: must be positive and finite" % (gain,))
    return g


NLF_LEVELS = _lib.NLF_LEVELS
NLF_BINS = _lib.NLF_BINS
NLF_MIN_COUNT = _lib.NLF_MIN_COUNT


class NoiseCurve:
    """a noise-level function the caller knows: sigma ([0,1] units) at the centres (l + 0.5) / 16 of the sixteen intensity levels,
    for ``sigma=NoiseCurve(...)``: every frame's noise map is ``fill_noise_map`` of these values.  Sixteen finite numbers >= 0."""

    def __init__(self, values):
        try:
            vals = tuple(float(v) for v in values)
        except (TypeError, ValueError):
            raise ValueError("NoiseCurve: expected %d numbers, got %r" % (NLF_LEVELS, values)) from None
        if len(vals) != NLF_LEVELS:
            raise ValueError("NoiseCurve: expected %d values (one per intensity level), got %d" % (NLF_LEVELS, len(vals)))
        if not all(0.0 <= v < float("inf") for v in vals):
            raise ValueError("NoiseCurve: values must be finite and not negative, got %r" % (vals,))
        self.values = vals

    @classmethod
    def from_model(cls, a, b):
        """the Poisson-Gaussian sensor model: sigma(I) = sqrt(max(a I + b, 0)) at the level centres, I and sigma in [0,1] units"""
        a, b = (_number(v, "NoiseCurve.from_model: expected two numbers, got %r, %r" % (a, b)) for v in (a, b))
        return cls([max(a * (l + 0.5) / NLF_LEVELS + b, 0.0) ** 0.5 for l in range(NLF_LEVELS)])

    def __eq__(self, other):
        return isinstance(other, NoiseCurve) and self.values == other.values

    def __hash__(self):
        return hash(self.values)

    def __repr__(self):
        return "NoiseCurve(%r)" % (list(self.values),)


def _sigma_mode(sigma, T=None):
    """what ``sigma=`` asks for -> ('const', None | float) -- today's path --, ('auto', None), ('nlf', None), ('curve', [16 floats]),
    ('host', [T floats]) or ('device', tensor [T]).  Needs no device; T (when known) is checked against the length of per-frame values."""
    if sigma is None:
        return "const", None
    if isinstance(sigma, NoiseCurve):
        return "curve", list(sigma.values)
    if isinstance(sigma, str):
        if sigma == "nlf":
            return "nlf", None
        if sigma != "auto":
            raise ValueError("sigma %r: a number, 'auto', 'nlf', a NoiseCurve, a sequence of per-frame values or a device tensor [T]" % (sigma,))
        return "auto", None
    if isinstance(sigma, torch.Tensor) and sigma.dim() >= 1:
        if sigma.dim() != 1 or sigma.dtype != torch.float32:
            raise ValueError("sigma: a per-frame tensor must be float32 [T], got %s %s" % (sigma.dtype, tuple(sigma.shape)))
        if T is not None and sigma.shape[0] != T:
            raise ValueError("sigma: %d per-frame values for %d frames" % (sigma.shape[0], T))
        return ("device" if sigma.is_cuda else "host"), (sigma if sigma.is_cuda else [float(v) for v in sigma])
    if isinstance(sigma, (list, tuple)) or (not isinstance(sigma, torch.Tensor) and hasattr(sigma, "__len__") and hasattr(sigma, "__iter__")):
        try:
            vals = [float(v) for v in sigma]
        except (TypeError, ValueError):
            raise ValueError("sigma: per-frame values must be numbers, got %r" % (sigma,)) from None
        if T is not None and len(vals) != T:
            raise ValueError("sigma: %d per-frame values for %d frames" % (len(vals), T))
        return "host", vals
    return "const", float(sigma)


def _planes(x, what):
    return _tensor(x, torch.float32, (None,) * 4, "cuda", "%s: expected a contiguous float32 device tensor [T,C,H,W]" % what).shape


def estimate_sigma(x, picture=None, gain=1.0, clamp=(0.0, SIGMA_MAX), return_hist=False):
    """x: fp32 device tensor [T,C>=3,Hp,Wp], the tensor the ``*_to_input`` functions build -> fp32 device tensor [T]: one noise-level
    estimate per frame in [0,1] units, computed on the device, not synchronised with the host.  ``picture=(H, W)``: the top-left part of
    the planes that is the picture (``pad_to`` callers: the mirror images are not sampled); default: all of it.  The estimate: the
    Laplacian-difference mask [1 -2 1; -2 4 -2; 1 -2 1] over the interior pixels of the three colour planes, the median of its |response|
    from a 4096-bin histogram, / (6 * 0.6745); then ``* gain``, clamped to ``clamp``.  Bit-reproducible (integer counts; include/bsvd_hip.h
    states it operation by operation).  It saturates at ``SIGMA_MAX`` (63 / 255).  ``return_hist=True``: also the uint32 [T,4096] histograms.

    What is known: on synthetic frames with white Gaussian noise it is within 0.7 / 255 of the truth for sigma 2 .. 30 / 255 on
    frames of 64 x 96 and larger (profiles/sigma_auto.txt).  Nothing has been measured on real footage.  A YUV source with subsampled chroma gives correlated,
    chroma-smoothed RGB noise: the estimate reads LOW there, which is what ``gain`` is for."""
    lo, hi = _check_clamp(clamp)
    gain = _check_gain(gain)
    T, C, Hp, Wp = _planes(x, "estimate_sigma")
    if C < 3:
        raise ValueError("estimate_sigma: the estimate pools the three colour planes, x has %d" % C)
    H, W = (Hp, Wp) if picture is None else _pair(picture, "picture")
    hist = torch.empty((T, SIGMA_BINS), dtype=torch.int32, device=x.device)
    out = torch.empty((T,), dtype=torch.float32, device=x.device)
    _call(x.device, "bsvd_estimate_sigma", x.data_ptr(), T, 3, H, W, Hp, Wp, C * Hp * Wp, gain, lo, hi, hist.data_ptr(), out.data_ptr())
    return (out, hist.view(torch.uint32)) if return_hist else out


def fill_sigma_plane(x, sigma_dev):
    """x: fp32 device tensor [T,C,Hp,Wp]; its last plane of frame t becomes sigma_dev[t] (fp32 device tensor [T]), in place, on the device"""
    T, C, Hp, Wp = _planes(x, "fill_sigma_plane")
    _tensor(sigma_dev, torch.float32, (T,), x.device, "fill_sigma_plane: expected a contiguous float32 tensor [%d] on %s" % (T, x.device))
    if C < 2:
        raise ValueError("fill_sigma_plane: x has no plane behind its picture planes")
    _call(x.device, "bsvd_fill_sigma_plane", x.data_ptr(), T, C - 1, Hp, Wp, C * Hp * Wp, sigma_dev.data_ptr())
    return x


def _check_min_count(min_count):
    n = _number(min_count, "min_count: expected a positive integer, got %r" % (min_count,), int)
    if n != min_count or not (1 <= n < 2 ** 31):
        raise ValueError("min_count %r: must be a positive integer" % (min_count,))
    return n


def estimate_noise_curve(x, picture=None, gain=1.0, clamp=(0.0, SIGMA_MAX), min_count=NLF_MIN_COUNT, return_hist=False):
    """x: fp32 device tensor [T,C>=3,Hp,Wp], the tensor the ``*_to_input`` functions build -> fp32 device tensor [T,16]: the frame's
    noise-level function, sigma ([0,1] units) at sixteen levels of local intensity (level l: 3 x 3 box mean in [l/16, (l+1)/16)), computed
    on the device, not synchronised with the host.  The sample is ``estimate_sigma``'s (the Laplacian-difference response at the interior
    pixels of the picture in the three colour planes), binned by the 3 x 3 box sum of the same nine values; per level the median of
    |response| from a 1024-bin histogram, / (6 * 0.6745), ``* gain``, clamped to ``clamp``.  A level with fewer than ``min_count`` samples
    takes the value of the nearest level that has them (the lower one on a tie); if none has, every level gets the pooled estimate.
    Bit-reproducible (integer counts; include/bsvd_hip.h states it operation by operation).  No smoothing across levels and no temporal
    filter: both are left to the caller.  ``picture=(H, W)``: as for ``estimate_sigma``.  ``return_hist=True``: also the uint32
    [T,16,1024] histograms.

    What is known: on synthetic frames with sigma(I) = sqrt(a I + b) noise quantised to 8 bits the levels away from the clipped ends are
    within the bounds of profiles/noise_curve.txt.  Nothing has been measured on real footage, and a per-pixel noise map is outside what
    the reference's checkpoints were trained on (a constant plane): ``build_vst`` / the pipelines' ``vst=`` turn the same curve into a
    variance-stabilising transform, which keeps the constant plane."""
    lo, hi = _check_clamp(clamp)
    gain = _check_gain(gain)
    min_count = _check_min_count(min_count)
    T, C, Hp, Wp = _planes(x, "estimate_noise_curve")
    if C < 3:
        raise ValueError("estimate_noise_curve: the estimate pools the three colour planes, x has %d" % C)
    H, W = (Hp, Wp) if picture is None else _pair(picture, "picture")
    hist = torch.empty((T, NLF_LEVELS, NLF_BINS), dtype=torch.int32, device=x.device)
    out = torch.empty((T, NLF_LEVELS), dtype=torch.float32, device=x.device)
    _call(x.device, "bsvd_estimate_nlf", x.data_ptr(), T, H, W, Hp, Wp, C * Hp * Wp, gain, lo, hi, min_count, hist.data_ptr(), out.data_ptr())
    return (out, hist.view(torch.uint32)) if return_hist else out


def noise_curve_from_hist(hist, gain=1.0, clamp=(0.0, SIGMA_MAX), min_count=NLF_MIN_COUNT):
    """hist: uint32 (or int32) device tensor [T,16,1024], e.g. ``estimate_noise_curve(return_hist=True)`` histograms the caller has summed
    over frames -> fp32 device tensor [T,16]: the curve step of ``estimate_noise_curve`` alone"""
    lo, hi = _check_clamp(clamp)
    gain = _check_gain(gain)
    min_count = _check_min_count(min_count)
    _tensor(hist, (torch.uint32, torch.int32), (None, NLF_LEVELS, NLF_BINS), "cuda",
            "noise_curve_from_hist: expected a contiguous uint32 device tensor [T,%d,%d]" % (NLF_LEVELS, NLF_BINS))
    out = torch.empty((hist.shape[0], NLF_LEVELS), dtype=torch.float32, device=hist.device)
    _call(hist.device, "bsvd_finish_nlf", hist.data_ptr(), hist.shape[0], gain, lo, hi, min_count, out.data_ptr())
    return out


def fill_noise_map(x, curve):
    """x: fp32 device tensor [T,C>=4,Hp,Wp]; curve: fp32 device tensor [T,16] (``estimate_noise_curve``).  The last plane of frame t becomes
    that frame's per-pixel noise map, in place, on the device: at every pixel of the whole plane (the mirror margin of ``pad_to`` included)
    the 3 x 3 box means of R, G, B (replicate borders) mixed 1:2:1 give a position on the level axis, and the curve is interpolated linearly
    between the level centres.  A flat curve gives exactly that value everywhere; the map is finite whatever the colour planes hold."""
    T, C, Hp, Wp = _planes(x, "fill_noise_map")
    _tensor(curve, torch.float32, (T, NLF_LEVELS), x.device,
            "fill_noise_map: expected a contiguous float32 tensor [%d,%d] on %s" % (T, NLF_LEVELS, x.device))
    if C < 4:
        raise ValueError("fill_noise_map: x needs three colour planes and a plane behind them, it has %d" % C)
    _call(x.device, "bsvd_fill_nlf_plane", x.data_ptr(), T, C - 1, Hp, Wp, C * Hp * Wp, curve.data_ptr())
    return x


# ---------------------------------------------------------------------------------------------------
# the variance-stabilising transform of a noise curve (include/bsvd_hip.h, bsvd_vst_build / bsvd_vst_forward / bsvd_vst_inverse)

VST_KNOTS = _lib.VST_KNOTS
VST_TABLE_FLOATS = _lib.VST_TABLE_FLOATS
VST_FLOOR = _lib.VST_FLOOR


def check_vst_floor(floor):
    """``floor``: the least sigma the transform divides by, in [2^-10, 1] -> float; ValueError otherwise"""
    f = _number(floor, "vst_floor: expected a number in [2^-10, 1], got %r" % (floor,))
    if isinstance(floor, bool) or not (_lib.VST_FLOOR_MIN <= f <= 1.0):
        raise ValueError("vst_floor %r: must lie in [2^-10, 1] (the tables' knots stay apart and their reciprocals finite)" % (floor,))
    return f


def _vst_tables(tables, T, device, what):
    """a table tensor [1 | T, VST_TABLE_FLOATS] -> the table stride in sets (0: shared)"""
    message = ("%s: tables must be a contiguous float32 tensor [1,%d] (shared) or [%d,%d] (per frame) on %s (build_vst)"
               % (what, VST_TABLE_FLOATS, T, VST_TABLE_FLOATS, device))
    if _tensor(tables, torch.float32, (None, VST_TABLE_FLOATS), device, message).shape[0] not in (1, T):
        raise ValueError(message)
    return 0 if tables.shape[0] == 1 else 1


def build_vst(curve, floor=VST_FLOOR, out=None):
    """curve: a ``NoiseCurve`` (n = 1; ``device=`` of the current HIP device) or an fp32 device tensor [n,16] (``estimate_noise_curve``)
    -> fp32 device tensor [n, VST_TABLE_FLOATS]: the tables of the variance-stabilising transform of each curve, built on the device, not
    synchronised with the host.  With the curve clamped to [``floor``, 1] and interpolated between the level centres as ``fill_noise_map``
    does, g(I) ~ integral dI / sigma(I) at 1025 knots over [0, 1] (g(0) = 0, g(1) = 1), the reciprocal rise of every interval, and sigma'
    = the harmonic mean of the clamped curve: the one standard deviation the noise has after ``vst_forward`` (``vst_sigma``).  Built in
    double in a fixed order: bit-reproducible (include/bsvd_hip.h states it operation by operation).  ``out``: write into this tensor.

    What is known: on synthetic sigma(I) = sqrt(a I + b) noise the transformed frames are as flat as ``estimate_noise_curve`` can tell
    (profiles/vst.txt).  No trained checkpoint has been run through it: the effect on denoising quality has not been measured, and nothing
    has been measured on real footage.  The transform changes the tone curve the network sees."""
    floor = check_vst_floor(floor)
    if isinstance(curve, NoiseCurve):
        curve = torch.tensor([curve.values], dtype=torch.float32).to(out.device if out is not None else torch.device("cuda", torch.cuda.current_device()))
    message = "build_vst: expected a NoiseCurve or a contiguous float32 device tensor [n,%d]" % NLF_LEVELS
    n = _tensor(curve, torch.float32, (None, NLF_LEVELS), "cuda", message).shape[0]
    if n < 1:
        raise ValueError(message)
    if out is None:
        out = torch.empty((n, VST_TABLE_FLOATS), dtype=torch.float32, device=curve.device)
    elif _vst_tables(out, n, curve.device, "build_vst(out=)") != (0 if n == 1 else 1):
        raise ValueError("build_vst(out=): %d table sets for %d curves" % (out.shape[0], n))
    _call(curve.device, "bsvd_vst_build", curve.data_ptr(), n, floor, out.data_ptr())
    return out


def vst_sigma(tables):
    """tables: ``build_vst``'s [n, VST_TABLE_FLOATS] -> a device view [n] of the sigma' values (not synchronised with the host)"""
    if not isinstance(tables, torch.Tensor) or tables.dim() != 2 or tables.shape[1] != VST_TABLE_FLOATS:
        raise ValueError("vst_sigma: expected build_vst's tensor [n,%d]" % VST_TABLE_FLOATS)
    return tables[:, _lib.VST_SIGMA_AT]


def vst_forward(x, tables, fill_plane=True):
    """x: fp32 device tensor [T,C>=3,Hp,Wp], the tensor the ``*_to_input`` functions build; tables: ``build_vst``'s [1, ...] (one set for
    all frames) or [T, ...] (frame t uses set t).  In place, on the device: planes 0 .. 2 go through the forward transform (piecewise
    linear between the knots; values outside [0, 1] continue on the end intervals' lines, NaN stays NaN), and with ``fill_plane`` (needs
    C >= 4) every element of the last plane of frame t becomes that frame's sigma' -- the constant noise plane the reference's checkpoints
    were trained with.  ``fill_plane=False``: no plane is written (a blind model has none).  Returns ``x``."""
    T, C, Hp, Wp = _planes(x, "vst_forward")
    if C < 3:
        raise ValueError("vst_forward: the transform takes the three colour planes, x has %d" % C)
    if fill_plane and C < 4:
        raise ValueError("vst_forward(fill_plane=True): x needs a plane behind its colour planes, it has %d (a blind model: fill_plane=False)" % C)
    stride = _vst_tables(tables, T, x.device, "vst_forward")
    _call(x.device, "bsvd_vst_forward", x.data_ptr(), T, Hp, Wp, C * Hp * Wp, C - 1 if fill_plane else -1, tables.data_ptr(), stride)
    return x


def vst_inverse(y, tables):
    """y: fp32 device tensor [T,C>=3,Hp,Wp] (the network's output: C = 3); tables: as for ``vst_forward``.  Planes 0 .. 2 go back through
    the inverse transform, in place, on the device.  The inverse is the algebraic one: a nonlinear inverse of a denoised mean is biased
    where the curve bends sharply relative to sigma', and no unbiased-inverse correction is applied.  Returns ``y``."""
    T, C, Hp, Wp = _planes(y, "vst_inverse")
    if C < 3:
        raise ValueError("vst_inverse: the transform takes the three colour planes, y has %d" % C)
    stride = _vst_tables(tables, T, y.device, "vst_inverse")
    _call(y.device, "bsvd_vst_inverse", y.data_ptr(), C * Hp * Wp, T, Hp, Wp, tables.data_ptr(), stride)
    return y


def vst_identity(curve, floor=VST_FLOOR):
    """curve: a ``NoiseCurve`` -> the one value all sixteen levels have after the clamp to [floor, 1] (in fp32), as a float, or None.
    With one value the transform is the identity and sigma' is that value: the pipelines launch nothing then.  Needs no device."""
    import struct
    floor = check_vst_floor(floor)
    f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]
    vals = {min(max(f32(v), f32(floor)), 1.0) for v in curve.values}
    return vals.pop() if len(vals) == 1 else None


def _with_sigma(y, mode, picture, gain):
    """the shared second half of the ``*_to_input`` functions for per-frame sigma: y was converted with its sigma plane at 0;
    estimate (or upload) the T values, fill the plane -- or, for 'nlf' / a NoiseCurve, the T curves and the per-pixel map"""
    kind, val = mode
    if kind == "nlf":
        return fill_noise_map(y, estimate_noise_curve(y, picture=picture, gain=gain))
    if kind == "curve":
        return fill_noise_map(y, torch.tensor(val, dtype=torch.float32).to(y.device).expand(y.shape[0], NLF_LEVELS).contiguous())
    if kind == "auto":
        s = estimate_sigma(y, picture=picture, gain=gain)
    elif kind == "host":
        s = torch.tensor(val, dtype=torch.float32).to(y.device)
    else:
        if val.device != y.device:
            raise ValueError("sigma: the per-frame tensor is on %s, the frames on %s" % (val.device, y.device))
        s = val.contiguous()
    return fill_sigma_plane(y, s)


# ---------------------------------------------------------------------------------------------------
# scene cuts: a coarse luma grid per frame and its frame-to-frame difference on the device (include/bsvd_hip.h, bsvd_scene_grid /
# bsvd_scene_diff), the score and the decision on the host

SCENE_BLOCK = 16
SCENE_L_MAX = 1020            # qR + 2 qG + qB at q = 255
CUT_THRESHOLD = 10.0


def check_cut_threshold(threshold):
    t = _number(threshold, "cut_threshold: expected a positive number, got %r" % (threshold,))
    if isinstance(threshold, bool) or not (0.0 < t < float("inf")):
        raise ValueError("cut_threshold %r: must be positive and finite" % (threshold,))
    return t


def _scene_picture(x, picture, what):
    T, C, Hp, Wp = _planes(x, what)
    if C < 3:
        raise ValueError("%s: the score reads the three colour planes, x has %d" % (what, C))
    H, W = (Hp, Wp) if picture is None else _pair(picture, "picture")
    if not (0 <= H <= Hp and 0 <= W <= Wp):
        raise ValueError("%s: picture %r does not lie inside the %d x %d planes" % (what, picture, Hp, Wp))
    return T, C, Hp, Wp, H, W


def scene_scores(x, picture=None, prev=None, out=None):
    """x: fp32 device tensor [T,C>=3,Hp,Wp], the tensor the ``*_to_input`` functions build -> (sad, grid), device tensors, not synchronised
    with the host: ``grid`` int32 [T,GH,GW], the sum of L = qR + 2 qG + qB (q = the 8-bit code of a plane value) over every full 16 x 16
    block of the picture; ``sad`` int64 [T], sad[t] = sum |grid[t] - grid[t-1]| over the blocks.  ``prev`` (int32 [GH,GW], the grid of the
    frame before x[0]) stands in for grid[-1]; without it sad[0] = 0.  ``picture=(H, W)``: the top-left part of the planes that is the
    picture (the mirror images of a padded tensor and partial blocks are not counted).  Integer sums: bit-reproducible.
    ``out=(sad, grid)``: write into these tensors instead of new ones."""
    T, C, Hp, Wp, H, W = _scene_picture(x, picture, "scene_scores")
    GH, GW = H // SCENE_BLOCK, W // SCENE_BLOCK
    if prev is not None:
        _tensor(prev, torch.int32, (GH, GW), x.device, "scene_scores: prev must be a contiguous int32 tensor [%d,%d] on %s" % (GH, GW, x.device))
    if out is None:
        sad = torch.empty((T,), dtype=torch.int64, device=x.device)
        grid = torch.empty((T, GH, GW), dtype=torch.int32, device=x.device)
    else:
        sad, grid = out
        for t, dtype, shape in ((sad, torch.int64, (T,)), (grid, torch.int32, (T, GH, GW))):
            _tensor(t, dtype, shape, x.device, "scene_scores: out must be (int64 [%d], int32 [%d,%d,%d]) on %s" % (T, T, GH, GW, x.device))
    _call(x.device, "bsvd_scene_grid", x.data_ptr(), T, H, W, Hp, Wp, C * Hp * Wp, grid.data_ptr() if GH * GW else None)
    _call(x.device, "bsvd_scene_diff", grid.data_ptr() if GH * GW else None, None if prev is None or not GH * GW else prev.data_ptr(), T, GH * GW,
          sad.data_ptr())
    return sad, grid


def cut_scores(sad, blocks, prev_mafd=0.0):
    """host side of the rule, float64 from the integers: sad [T] ints, blocks = GH * GW -> (score [T], mafd [T]) as lists:
    mafd[t] = 100 sad[t] / (blocks * 256 * 1020) (the mean absolute block difference in percent of full scale),
    score[t] = min(mafd[t], |mafd[t] - mafd[t-1]|), mafd before the first pair = ``prev_mafd``"""
    full = float(blocks * SCENE_BLOCK * SCENE_BLOCK * SCENE_L_MAX)
    mafd = [100.0 * float(int(s)) / full if blocks else 0.0 for s in sad]
    score, before = [], float(prev_mafd)
    for m in mafd:
        score.append(min(m, abs(m - before)))
        before = m
    return score, mafd


def scene_cuts(x, threshold=CUT_THRESHOLD, picture=None):
    """x: fp32 device tensor [T,C>=3,Hp,Wp] -> the frame indices that start a new scene, a list of ints (what ``cuts=`` of the model's
    forward functions takes); one read-back of T integers.  The rule: ``scene_scores`` on the device, then on the host
    mafd[t] = 100 sad[t] / (GH GW 256 1020), score[t] = min(mafd[t], |mafd[t] - mafd[t-1]|) with mafd = 0 before the first pair; a cut is
    declared where score >= ``threshold``.  The difference term is what keeps motion, a pan or a fade -- many frames of similar mafd -- from
    reading as cuts.  (The rule and its default of 10 follow ffmpeg's ``scdet`` filter as remembered; nothing here depends on matching it.)

    What is known: on synthetic scenes of block-constant random fields with white noise of sigma 50 / 255 every scene start scores above 20
    and every other frame below 1.1 (tests/test_cuts_cpu.py).  Nothing has been measured on real footage, and the default threshold has not
    met any.  Known blind spot: a cut right behind another cut scores low, because mafd was already high one frame before -- on the
    same synthetic scenes (CPU model) back-to-back cuts, i.e. a one-frame scene, score 30.1 then 4.7, and the second is missed.  A cut TWO
    frames after another scored 34.5 there (mafd falls to the noise level in between); with real motion in the two-frame scene it will score
    lower -- take "one or two frames after a cut" as the blind spot.  A caller who knows the cuts passes them instead."""
    threshold = check_cut_threshold(threshold)
    T, C, Hp, Wp, H, W = _scene_picture(x, picture, "scene_cuts")
    sad, grid = scene_scores(x, picture=picture)
    score, _ = cut_scores(sad.tolist(), grid.shape[1] * grid.shape[2])
    return [t for t, s in enumerate(score) if s >= threshold]


# ---------------------------------------------------------------------------------------------------
# the output finish: denoise strength and dither (include/bsvd_hip.h, bsvd_blend_planar / BsvdDither)

DITHERS = (None, "ordered", "random")


def check_strength(strength):
    """``strength``: a number or a pair (luma, chroma), each in [0, 1] -> (s_luma, s_chroma) floats; ValueError otherwise"""
    try:
        if isinstance(strength, (tuple, list)):
            sl, sc = strength
        else:
            sl = sc = strength
        sl, sc = float(sl), float(sc)
    except (TypeError, ValueError):
        raise ValueError("strength: expected a number or a pair (luma, chroma), got %r" % (strength,)) from None
    if not (0.0 <= sl <= 1.0 and 0.0 <= sc <= 1.0):
        raise ValueError("strength %r: 0 <= strength <= 1 (1 = the network's result, 0 = the source), both finite" % (strength,))
    return sl, sc


def check_dither(dither, dither_seed=0, frame0=0):
    """``dither`` None | 'ordered' | 'random', ``dither_seed`` in [0, 2^32), ``frame0`` >= 0 -> (mode, seed, frame0); ValueError otherwise"""
    if dither is not None and not (isinstance(dither, str) and dither in DITHERS):
        raise ValueError("dither %r: None, 'ordered' or 'random'" % (dither,))
    seed, f0 = (_number(v, "dither_seed / frame0: expected ints, got %r / %r" % (dither_seed, frame0), int) for v in (dither_seed, frame0))
    if not 0 <= seed < 2 ** 32:
        raise ValueError("dither_seed %r: 0 <= seed < 2^32" % (dither_seed,))
    return _lib.DITHER[dither], seed, _stream_index(frame0, f0)


def _stream_index(frame0, f0):
    """``frame0`` as an int -> the same; ValueError outside [0, 2^62)"""
    if not 0 <= f0 < 2 ** 62:
        raise ValueError("frame0 %r: the stream index of the first frame, not negative" % (frame0,))
    return f0


def _dither_struct(dither, dither_seed, frame0):
    """-> a BsvdDither, or None with dither off (the existing entry point is called then)"""
    mode, seed, f0 = check_dither(dither, dither_seed, frame0)
    return _lib.BsvdDither(mode=mode, seed=seed, frame0=f0) if mode else None


def _luma_weights(matrix):
    """``matrix``: a name of ``_lib.MATRIX`` or three weights (Kr, Kg, Kb) in [0, 1] -> a ctypes float[3]"""
    if isinstance(matrix, str):
        if matrix not in _lib.LUMA_WEIGHTS:
            raise ValueError("matrix %r: one of %s, or three weights (Kr, Kg, Kb)" % (matrix, ", ".join(sorted(_lib.LUMA_WEIGHTS))))
        w = _lib.LUMA_WEIGHTS[matrix]
    else:
        try:
            w = tuple(float(v) for v in matrix)
        except (TypeError, ValueError):
            raise ValueError("matrix: a name of %s or three weights (Kr, Kg, Kb), got %r" % (sorted(_lib.LUMA_WEIGHTS), matrix)) from None
        if len(w) != 3 or not all(0.0 <= v <= 1.0 for v in w):
            raise ValueError("matrix %r: three weights (Kr, Kg, Kb), each in [0, 1]" % (matrix,))
    return (ctypes.c_float * 3)(*w)


def blend_output(y, x, strength, matrix="bt709"):
    """The denoise strength, in place on ``y``: y fp32 device tensor [T,3,Hp,Wp] (the network's output), x fp32 [T,3(+1),Hp,Wp] (the input
    it came from; only its first three planes are read).  ``strength``: a number or (luma, chroma), each in [0, 1]: 1 keeps the network's
    result, 0 returns the source; chroma mixes R, G and B alike, and luma moves the result along the luma of the removed noise (weights:
    the Kr, Kg, Kb of ``matrix``, a name or three numbers).  The ends are exact: (1, 1) leaves ``y``'s bits, (0, 0) gives ``x``'s.
    Returns ``y``.  (include/bsvd_hip.h, bsvd_blend_planar, states the arithmetic.)"""
    sl, sc = check_strength(strength)
    w = _luma_weights(matrix)
    _planes(y, "blend_output(y)")
    _planes(x, "blend_output(x)")
    if y.shape[1] != 3 or x.shape[1] < 3 or x.shape[0] != y.shape[0] or x.shape[2:] != y.shape[2:] or x.device != y.device:
        raise ValueError("blend_output: y [T,3,Hp,Wp] and x [T,3(+1),Hp,Wp] on one device, got %s and %s" % (tuple(y.shape), tuple(x.shape)))
    T, _, Hp, Wp = y.shape
    _call(y.device, "bsvd_blend_planar", y.data_ptr(), 3 * Hp * Wp, x.data_ptr(), x.shape[1] * Hp * Wp, T, Hp, Wp, sl, sc, w)
    return y


# ---------------------------------------------------------------------------------------------------
# film grain: the removed noise measured on the device, a model fitted on the host, clean grain synthesised on the device
# (include/bsvd_hip.h, bsvd_grain_stats / bsvd_grain_apply)

GRAIN_LEVELS, GRAIN_LAGS, GRAIN_TAPS, GRAIN_STATS = _lib.GRAIN_LEVELS, _lib.GRAIN_LAGS, _lib.GRAIN_TAPS, _lib.GRAIN_STATS
GRAIN_TMPL = _lib.GRAIN_TMPL
GRAIN_MIN_COUNT = _lib.GRAIN_MIN_COUNT
GRAIN_WARMUP = 16                   # rows above and columns on both sides of a template that the recursion runs through first
GRAIN_RIDGE = 1e-3                  # times R(0), on the diagonal of the Yule-Walker system
# the 46 lags (dy, dx) of bsvd_grain_stats in its order, and the 24 taps (dy, dx) of the causal lag-3 neighbourhood: tap i is the
# neighbour at (r - dy, c - dx) -- the three to the left in the row, then the rows above, nearest first, each from dx = -3 (right) to 3 (left)
GRAIN_LAG_LIST = [(0, dx) for dx in range(7)] + [(dy, dx) for dy in (1, 2, 3) for dx in range(-6, 7)]
GRAIN_TAP_LIST = [(0, dx) for dx in (1, 2, 3)] + [(dy, dx) for dy in (1, 2, 3) for dx in range(-3, 4)]
_GRAIN_LAG_AT = {lag: i for i, lag in enumerate(GRAIN_LAG_LIST)}


def _grain_lag_index(dy, dx):
    """R(-d) = R(d): the index of lag (dy, dx) or of its mirror image in ``GRAIN_LAG_LIST``"""
    if dy < 0 or (dy == 0 and dx < 0):
        dy, dx = -dy, -dx
    return _GRAIN_LAG_AT[(dy, dx)]


def _solve(M, b):
    """M a = b by Gaussian elimination with partial pivoting in float64, written out (no LAPACK); a singular system gives zeros"""
    n = len(b)
    A = np.array(M, dtype=np.float64).reshape(n, n).copy()
    v = np.array(b, dtype=np.float64).copy()
    for i in range(n):
        p = i + int(np.argmax(np.abs(A[i:, i])))
        if not abs(A[p, i]) > 0.0:
            return np.zeros(n)
        if p != i:
            A[[i, p]] = A[[p, i]]
            v[[i, p]] = v[[p, i]]
        f = A[i + 1:, i] / A[i, i]
        A[i + 1:] -= f[:, None] * A[i]
        v[i + 1:] -= f * v[i]
    a = np.zeros(n)
    for i in range(n - 1, -1, -1):
        a[i] = (v[i] - A[i, i + 1:] @ a[i + 1:]) / A[i, i]
    return a if np.all(np.isfinite(a)) else np.zeros(n)


def grain_template(ar, seed=0):
    """ar: [3][24] coefficients -> float32 [3,128,128]: one unit-variance grain template per component.  White Gaussian noise from
    ``numpy.random.default_rng(seed)`` over (128 + 16) x (128 + 32), the raster recursion g(r, c) = e(r, c) + sum_i a_i g(r - dy_i, c - dx_i)
    over ``GRAIN_TAP_LIST`` (zeros outside), the warm-up border of 16 rows above and 16 columns on both sides cut off, divided by its own
    standard deviation.  A recursion that does not stay finite (coefficients outside the stable region) gives the white field instead."""
    ar = np.asarray(ar, dtype=np.float64).reshape(3, GRAIN_TAPS)
    B, n = GRAIN_WARMUP, GRAIN_TMPL
    rows, cols = n + B, n + 2 * B
    white = np.random.default_rng(seed).standard_normal((3, rows, cols))
    out = np.empty((3, n, n), dtype=np.float32)
    for k in range(3):
        g = np.zeros((rows + 3, cols + 6))                 # three zero rows above, three zero columns on both sides
        a_row = ar[k, :3]
        with np.errstate(all="ignore"):
            for r in range(rows):
                acc = white[k, r].copy()
                for i, (dy, dx) in enumerate(GRAIN_TAP_LIST[3:], 3):
                    if ar[k, i] != 0.0:
                        acc += ar[k, i] * g[3 + r - dy, 3 - dx:3 - dx + cols]
                if np.any(a_row != 0.0):                   # the row's own three taps: a recursion along the row
                    line = g[3 + r]
                    a1, a2, a3 = (float(v) for v in a_row)
                    for c in range(cols):
                        line[3 + c] = acc[c] + a1 * line[2 + c] + a2 * line[1 + c] + a3 * line[c]
                else:
                    g[3 + r, 3:3 + cols] = acc
            t = g[3 + B:, 3 + B:3 + B + n]
            sd = float(t.std())
        if not (np.all(np.isfinite(t)) and 0.0 < sd < 1e6):
            t = white[k, B:, B:B + n]
            sd = float(t.std())
        out[k] = (t / sd).astype(np.float32)
    return out


class GrainModel:
    """A film-grain model in the components the statistics use -- 0: the luma of the noise, 1: B minus it, 2: R minus it.
    ``std`` [3][16]: the standard deviation ([0,1] units) at the centres (l + 0.5) / 16 of sixteen levels of the result's luma;
    ``ar`` [3][24]: the coefficients of a causal lag-3 autoregression over ``GRAIN_TAP_LIST`` (the grain's spatial correlation, its
    "size"); ``templates``: float32 [3,128,128], unit-variance fields synthesised from ``ar`` (``grain_template``; built when first asked
    for).  Plain numpy in float64.  ``from_values`` makes one by hand; ``estimate_grain`` / ``grain_from_stats`` measure one."""

    def __init__(self, std, ar=None, template_seed=0):
        try:
            s = np.array(std, dtype=np.float64)
            a = np.zeros((3, GRAIN_TAPS)) if ar is None else np.array(ar, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("GrainModel: std [3][%d] and ar [3][%d] numbers, got %r / %r" % (GRAIN_LEVELS, GRAIN_TAPS, std, ar)) from None
        if s.shape != (3, GRAIN_LEVELS) or not np.all(np.isfinite(s)) or np.any(s < 0):
            raise ValueError("GrainModel: std must be [3][%d] finite numbers >= 0" % GRAIN_LEVELS)
        if a.shape != (3, GRAIN_TAPS) or not np.all(np.isfinite(a)):
            raise ValueError("GrainModel: ar must be [3][%d] finite numbers" % GRAIN_TAPS)
        if np.any(s.astype(np.float32) > 3e38):
            raise ValueError("GrainModel: std must fit float32")
        self.std, self.ar, self.template_seed = s, a, int(template_seed)
        self._templates = None
        self._dev = {}

    @classmethod
    def from_values(cls, std, ar=None, template_seed=0):
        """std: one number (every component, every level), three numbers (one per component) or [3][16]; ar: None (white grain) or [3][24]"""
        try:
            s = np.array(std, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("GrainModel.from_values: std must be a number, three numbers or [3][%d], got %r" % (GRAIN_LEVELS, std)) from None
        if s.shape == ():
            s = np.full((3, GRAIN_LEVELS), float(s))
        elif s.shape == (3,):
            s = np.repeat(s[:, None], GRAIN_LEVELS, axis=1)
        return cls(s, ar, template_seed)

    @property
    def templates(self):
        if self._templates is None:
            self._templates = grain_template(self.ar, self.template_seed)
            self._templates.setflags(write=False)
        return self._templates

    @property
    def is_zero(self):
        return not bool((self.std.astype("float32") != 0).any())

    def device_templates(self, device):
        """the templates as a float32 tensor [3,128,128] on ``device``, uploaded once"""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.templates.copy()).to(device)
        return self._dev[key]

    def __repr__(self):
        return "GrainModel(std=%r, ar=%r)" % (self.std.tolist(), self.ar.tolist())


def grain_from_stats(stats, anchors, min_count=GRAIN_MIN_COUNT, template_seed=0):
    """stats: 256 integers (``estimate_grain(return_stats=True)``, summed over the frames to pool), anchors: the number of anchor
    positions they were taken over ((H - 3) (W - 12) per frame) -> ``GrainModel``.  The fit alone, in float64:
    std[k][l] = sqrt(max(sum q^2 / N - (sum q / N)^2, 0)) / 4096 for the levels with at least ``min_count`` pixels, the others filled
    from the nearest such level (the lower one on a tie; none: the value pooled over the levels, 0 without pixels);
    ar[k]: with R(d) = A[k][d] / anchors, the 24 x 24 system sum_j a_j R(d_i - d_j) = R(d_i) over ``GRAIN_TAP_LIST`` with
    ``GRAIN_RIDGE`` R(0) on the diagonal, solved by elimination; R(0) <= 0 gives zeros."""
    min_count = _check_min_count(min_count)
    st = np.asarray(stats)
    if st.shape != (GRAIN_STATS,) or st.dtype.kind not in "iu":
        raise ValueError("grain_from_stats: expected %d integers, got %s %s" % (GRAIN_STATS, st.dtype, st.shape))
    if int(anchors) < 1:
        raise ValueError("grain_from_stats: anchors %r must be positive" % (anchors,))
    st = st.astype(np.int64)
    N = st[_lib.GRAIN_N_AT:_lib.GRAIN_N_AT + GRAIN_LEVELS].astype(np.float64)
    std = np.zeros((3, GRAIN_LEVELS))
    ar = np.zeros((3, GRAIN_TAPS))
    valid = [l for l in range(GRAIN_LEVELS) if N[l] >= min_count]
    for k in range(3):
        s1 = st[_lib.GRAIN_S1_AT + 16 * k:_lib.GRAIN_S1_AT + 16 * k + 16].astype(np.float64)
        s2 = st[_lib.GRAIN_S2_AT + 16 * k:_lib.GRAIN_S2_AT + 16 * k + 16].astype(np.float64)

        def value(n, a, b):
            return 0.0 if n <= 0 else max(b / n - (a / n) ** 2, 0.0) ** 0.5 / _lib.GRAIN_QSCALE

        own = [value(N[l], s1[l], s2[l]) for l in range(GRAIN_LEVELS)]
        pooled = value(N.sum(), s1.sum(), s2.sum())
        for l in range(GRAIN_LEVELS):
            if not valid:
                std[k, l] = pooled
            else:
                std[k, l] = own[min(valid, key=lambda v: (abs(v - l), v))]
        R = st[_lib.GRAIN_A_AT + GRAIN_LAGS * k:_lib.GRAIN_A_AT + GRAIN_LAGS * (k + 1)].astype(np.float64) / float(anchors)
        if R[0] > 0.0:
            M = np.empty((GRAIN_TAPS, GRAIN_TAPS))
            for i, (yi, xi) in enumerate(GRAIN_TAP_LIST):
                for j, (yj, xj) in enumerate(GRAIN_TAP_LIST):
                    M[i, j] = R[_grain_lag_index(yi - yj, xi - xj)]
            M[np.diag_indices(GRAIN_TAPS)] += GRAIN_RIDGE * R[0]
            ar[k] = _solve(M, [R[_grain_lag_index(dy, dx)] for dy, dx in GRAIN_TAP_LIST])
    return GrainModel(std, ar, template_seed)


def grain_stats(x, y, picture=None, matrix="bt709"):
    """x (the source) fp32 device tensor [T,>=3,Hp,Wp], y (the result) [T,>=3,Hp,Wp] -> int64 device tensor [T,256]: the statistics of the
    removed noise x - y of every frame (include/bsvd_hip.h, bsvd_grain_stats, states them), not synchronised with the host.
    ``picture=(H, W)``: the top-left part of the planes that is the picture; default: all of it.  H >= 4, W >= 13."""
    w = _luma_weights(matrix)
    Tx, Cx, Hp, Wp = _planes(x, "grain_stats(x)")
    Ty, Cy, Hy, Wy = _planes(y, "grain_stats(y)")
    if Cx < 3 or Cy < 3 or (Tx, Hp, Wp) != (Ty, Hy, Wy) or x.device != y.device:
        raise ValueError("grain_stats: x [T,>=3,Hp,Wp] and y [T,>=3,Hp,Wp] on one device, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    H, W = (Hp, Wp) if picture is None else _pair(picture, "picture")
    out = torch.empty((Tx, GRAIN_STATS), dtype=torch.int64, device=x.device)
    _call(x.device, "bsvd_grain_stats", x.data_ptr(), Cx * Hp * Wp, y.data_ptr(), Cy * Hp * Wp, Tx, H, W, Hp, Wp, w, out.data_ptr())
    return out


def estimate_grain(x, y, picture=None, matrix="bt709", min_count=GRAIN_MIN_COUNT, return_stats=False):
    """x: the source, y: the denoised result, fp32 device tensors [T,>=3,Hp,Wp] -> ``GrainModel``: the grain the network removed, as a
    model.  The statistics are taken on the device (``grain_stats``: integers, bit-reproducible), pooled over the T frames and brought to
    the host -- ONE synchronisation --, where ``grain_from_stats`` fits standard deviations per luma level and an autoregression per
    component.  ``return_stats=True``: also the pooled int64 [256] (numpy).

    What is known: synthetic grain of a known model comes back within the figures of profiles/film_grain.txt.  Nothing has been measured
    on real footage, and no encoder has read the model (there is no AV1 / filmgrn1 table writer)."""
    min_count = _check_min_count(min_count)
    st = grain_stats(x, y, picture=picture, matrix=matrix)
    H, W = (x.shape[2], x.shape[3]) if picture is None else _pair(picture, "picture")
    pooled = st.sum(dim=0).cpu().numpy()
    model = grain_from_stats(pooled, x.shape[0] * (H - 3) * (W - 12), min_count)
    return (model, pooled) if return_stats else model


def check_grain(grain, amount=1.0, seed=0):
    """the pipelines' ``grain`` None | GrainModel | 'scene', ``grain_amount`` finite >= 0, ``grain_seed`` in [0, 2^32)
    -> (grain, amount, seed); ValueError otherwise.  Needs no device."""
    if grain is not None and not isinstance(grain, GrainModel) and not (isinstance(grain, str) and grain == "scene"):
        raise ValueError("grain %r: None, a GrainModel or 'scene'" % (grain,))
    a = _number(amount, "grain_amount: expected a number >= 0, got %r" % (amount,))
    if isinstance(amount, bool) or not (0.0 <= a < 3e38):
        raise ValueError("grain_amount %r: must be finite and not negative" % (amount,))
    s = _number(seed, "grain_seed: expected an int, got %r" % (seed,), int)
    if s != seed or not 0 <= s < 2 ** 32:
        raise ValueError("grain_seed %r: 0 <= seed < 2^32" % (seed,))
    return grain, a, s


def apply_grain(y, model, amount=1.0, seed=0, frame0=0, matrix="bt709"):
    """Synthetic grain from ``model`` (a ``GrainModel``) onto y, fp32 device tensor [T,3,Hp,Wp], in place over the whole planes: per
    32 x 32 block a window of the model's templates at an offset hashed from (seed, frame0 + t, block), scaled by ``amount`` times the
    model's standard deviation at the pixel's luma, turned from (luma, B - luma, R - luma) back into R, G, B with ``matrix``'s weights
    (include/bsvd_hip.h, bsvd_grain_apply, states the arithmetic).  ``frame0``: the stream index of the first frame -- the pattern of a
    frame depends on its index, not on how the stream was cut into calls.  ``amount=0`` or a model whose std is all zero: nothing is
    launched and y keeps its bytes.  No overlap blending of the blocks.  Returns ``y``."""
    if not isinstance(model, GrainModel):
        raise ValueError("apply_grain: model must be a GrainModel, got %r" % (model,))
    _, amount, seed = check_grain(model, amount, seed)
    f0 = _stream_index(frame0, _number(frame0, "frame0: expected an int, got %r" % (frame0,), int))
    w = _luma_weights(matrix)
    if not w[1] > 0.0:
        raise ValueError("apply_grain: matrix %r has no green weight to divide by" % (matrix,))
    T, C, Hp, Wp = _planes(y, "apply_grain")
    if C != 3:
        raise ValueError("apply_grain: y must have three planes, it has %d" % C)
    if amount == 0.0 or model.is_zero:
        return y
    std = (ctypes.c_float * (3 * GRAIN_LEVELS))(*[float(v) for v in model.std.reshape(-1)])
    inv_wg = ctypes.c_float(1.0 / float(w[1])).value
    _call(y.device, "bsvd_grain_apply", y.data_ptr(), 3 * Hp * Wp, T, Hp, Wp, model.device_templates(y.device).data_ptr(), std, amount, w, inv_wg,
          seed, f0)
    return y


# ---------------------------------------------------------------------------------------------------
# the two cores of the conversions: what the four ``*_to_input`` and the four ``output_to_*`` functions share

def _frames_of(buf):
    """T of a surface buffer [T, bytes], where its shape says so already (the length check of per-frame ``sigma`` values)"""
    return buf.shape[0] if isinstance(buf, torch.Tensor) and buf.dim() == 2 else None


def _decode(names, src, T, C, H, W, pad_to, sigma, sigma_gain, describe, head=()):
    """The decode core: ``src`` (the checked device tensor of T frames) -> fp32 [T, C(+1), Hp, Wp].  ``names``: the (plain, padded) entry
    points -- ``pad_to`` given, also to the size the picture has, takes the padded one; plain None: one entry point serves both.
    ``sigma`` / ``sigma_gain`` exist here alone: None or a number is the constant the entry point writes; every other kind converts with
    the plane at 0 and hands over to ``_with_sigma``.  ``describe()``, called once ``sigma`` is understood: the format's own checks ->
    (the arguments between the sizes and ``extra``, the alpha plane to return beside the tensor or None); ``head``: those before H, W."""
    mode = _sigma_mode(sigma, T)
    per_frame = mode[0] != "const"
    if per_frame:
        gain = _check_gain(sigma_gain)
    const = 0.0 if per_frame else sigma
    tail, alpha = describe()
    H, W = int(H), int(W)
    plain, padded = names
    Hp, Wp = (H, W) if pad_to is None else _pair(pad_to, "pad_to")
    sizes = (H, W) if pad_to is None and plain is not None else (H, W, Hp, Wp)
    extra = 0 if const is None else 1
    x = torch.empty((src.shape[0], C + extra, max(Hp, 0), max(Wp, 0)), dtype=torch.float32, device=src.device)
    _call(src.device, plain if len(sizes) == 2 else padded, src.data_ptr(), x.data_ptr(), src.shape[0], *head, *sizes, *tail, extra,
          float(const or 0.0))
    if per_frame:
        x = _with_sigma(x, mode, (H, W), gain)
    return x if alpha is None else (x, alpha)


def _encode(what, names, y, crop_to, describe, dith=None, out=None, zeroed=False, labels=("10-bit", "10-bit"), head=()):
    """The encode core: ``y`` (checked, fp32 [T,C,Hp,Wp]) -> the surfaces.  ``names``: the (plain, cropped, dithered) entry points -- a
    BsvdDither takes the dithered one, else ``crop_to`` given, also to the size ``y`` has, the cropped one; plain None: the cropped one
    serves both.  ``describe(T, H, W)``: the format's own checks for H x W surfaces -> (the descriptor whose frame_stride is the buffer's, or
    None; the bytes of a frame, or without a descriptor the shape of the result; 16-bit samples?; the arguments behind the sizes).
    ``out`` exists here alone: without it the result is allocated, ``zeroed`` where a pitch or an offset leaves bytes no kernel writes;
    with it, it is checked (``labels``: how ``_surface_buffer``'s messages name the format)."""
    plain, cropped, dithered = names
    T, _, Hp, Wp = y.shape
    H, W = (Hp, Wp) if crop_to is None else _pair(crop_to, "crop_to")
    desc, size, sixteen, tail = describe(T, H, W)
    y = y.contiguous()
    if out is None:
        out = (torch.zeros if zeroed else torch.empty)(size if desc is None else (T, size), dtype=torch.uint8, device=y.device)
    elif out.device != y.device:
        raise ValueError("%s: out is on %s, y on %s" % (what, out.device, y.device))
    if desc is not None:
        desc.frame_stride = _surface_buffer(out, T, size, sixteen, what + "(out=)", *labels)
    if dith is not None:
        name, sizes, tail = dithered, (Hp, Wp, H, W), tail + (ctypes.byref(dith),)
    elif crop_to is not None or plain is None:
        name, sizes = cropped, (Hp, Wp, H, W)
    else:
        name, sizes = plain, (H, W)
    _call(y.device, name, y.data_ptr(), out.data_ptr(), T, *head, *sizes, *tail)
    return out


def frames_to_input(frames_u8, sigma=None, hwc=True, pad_to=None, sigma_gain=1.0):
    """frames_u8: uint8 device tensor [T,H,W,3] (hwc) or [T,3,H,W] -> fp32 [T,3(+1),H,W] in [0,1]; with ``sigma`` (noise
    std in [0,1] units, e.g. 30/255) a constant noise-map channel is appended.  ``pad_to=(Hp, Wp)``: the result is [T,3(+1),Hp,Wp],
    reflect-padded on the right and bottom (F.pad(..., mode='reflect') of the unpadded result, bit for bit).  ``sigma='auto'``: the
    noise-map plane of frame t holds that frame's own estimate (``estimate_sigma`` of the picture, times ``sigma_gain``); a sequence or a
    device tensor [T]: the caller's per-frame values."""
    require_hip()                                           # without a device that is what the caller hears, whatever was passed
    x = _tensor(frames_u8, torch.uint8, (None,) * 4, "cuda", "expected a uint8 device tensor [T,H,W,C] or [T,C,H,W]", contiguous=False).contiguous()
    T, H, W, C = x.shape if hwc else (x.shape[0], x.shape[2], x.shape[3], x.shape[1])
    return _decode(("bsvd_u8_to_planar", "bsvd_u8_to_planar_pad"), x, T, C, H, W, pad_to, sigma, sigma_gain,
                   lambda: ((1 if hwc else 0,), None), head=(C,))


def output_to_frames(y, hwc=True, rgb2bgr=False, crop_to=None):
    """y: fp32 device tensor [T,C,H,W] -> uint8 [T,H,W,C] (or [T,C,H,W]): clamp [0,1], x255, round half to even.  ``crop_to=(H, W)``:
    the frames of ``y[..., :H, :W]``; the rows and columns beyond are not read."""
    require_hip()                                           # as in frames_to_input
    _tensor(y, torch.float32, (None,) * 4, "cuda", "expected a float32 device tensor [T,C,H,W]", contiguous=False)
    C = y.shape[1]

    def describe(T, H, W):
        return None, (T, max(H, 0), max(W, 0), C) if hwc else (T, C, max(H, 0), max(W, 0)), False, (1 if hwc else 0, 1 if rgb2bgr else 0)
    return _encode("output_to_frames", ("bsvd_planar_to_u8", "bsvd_planar_to_u8_crop", None), y, crop_to, describe, head=(C,))


def _yuv_desc(H, W, pix_fmt, matrix, full_range, chroma, row_pitch, picture=False):
    """-> (BsvdYuvDesc, frame_bytes); ValueError for a name or a size the library would refuse.  picture: a surface for the pad / crop
    entry points, whose H and W only need to be even"""
    for what, name, table in (("pix_fmt", pix_fmt, _lib.PIX_FMT), ("matrix", matrix, _lib.MATRIX), ("chroma", chroma, _lib.CHROMA)):
        if name not in table:
            raise ValueError("%s %r: one of %s" % (what, name, ", ".join(sorted(table))))
    desc = _lib.BsvdYuvDesc(pix_fmt=_lib.PIX_FMT[pix_fmt], matrix=_lib.MATRIX[matrix], full_range=1 if full_range else 0,
                            chroma=_lib.CHROMA[chroma], row_pitch=int(row_pitch or 0))
    lib = _lib.load()
    nbytes = (lib.bsvd_yuv420_picture_bytes if picture else lib.bsvd_yuv420_frame_bytes)(int(H), int(W), desc.pix_fmt, desc.row_pitch)
    if nbytes < 0:
        raise ValueError("yuv420 %s frame %d x %d with row_pitch %s: H and W must be positive %s and row_pitch (bytes%s) at least "
                         "W samples" % (pix_fmt, H, W, row_pitch, "and even" if picture else "multiples of 4", ", even" if pix_fmt == "p010" else ""))
    return desc, nbytes


def yuv420_frame_bytes(H, W, pix_fmt, row_pitch=None):
    """Bytes of one NV12 / P010 frame: ``row_pitch * H * 3 / 2`` (Y plane, then the interleaved CbCr plane of H/2 rows);
    ``row_pitch`` in bytes, None = tight (W samples)."""
    return _yuv_desc(H, W, pix_fmt, "bt709", False, "linear", row_pitch)[1]


def yuv420_picture_bytes(H, W, pix_fmt, row_pitch=None):
    """``yuv420_frame_bytes`` for the surfaces ``pad_to`` / ``crop_to`` take: H and W only need to be even."""
    return _yuv_desc(H, W, pix_fmt, "bt709", False, "linear", row_pitch, picture=True)[1]


def _surface_buffer(buf, T, nbytes, sixteen, what, callers="10-bit", frames="10-bit"):
    """a surface buffer [T, >= frame_bytes] -> its frame stride in bytes.  sixteen: 16-bit samples; callers / frames: how the two
    messages about them name the format ("P010" / "p010" for the 4:2:0 functions)"""
    _tensor(buf, torch.uint8, (None, None), "cuda",
            "%s: expected a contiguous uint8 device tensor [T, frame_bytes] (%s callers view their uint16 as bytes)" % (what, callers))
    if (T is not None and buf.shape[0] != T) or buf.shape[0] < 1 or buf.shape[1] < nbytes:
        raise ValueError("%s: shape %s, expected [%s, %d] (or longer rows: frames row-length bytes apart)"
                         % (what, tuple(buf.shape), "T" if T is None else T, nbytes))
    if sixteen and buf.shape[1] % 2:
        raise ValueError("%s: %s frames must be an even number of bytes apart, got %d" % (what, frames, buf.shape[1]))
    return buf.shape[1]


def yuv420_to_input(buf, H, W, pix_fmt="nv12", matrix="bt709", full_range=False, chroma="linear", sigma=None, row_pitch=None, pad_to=None,
                    sigma_gain=1.0):
    """buf: uint8 device tensor [T, frame_bytes] of NV12 / P010 frames (``yuv420_frame_bytes``; rows longer than one frame are
    frames that far apart) -> fp32 [T,3(+1),H,W] RGB, the tensor ``frames_to_input`` builds; with ``sigma`` the constant noise-map
    channel is appended.  matrix 'bt601' | 'bt709' | 'bt2020', limited or full range, chroma upsampling 'nearest' | 'linear'
    (MPEG-2 / H.264 / HEVC default siting).  The result is NOT clamped to [0,1]: the out-of-gamut values of a noisy source are
    information for a denoiser.  ``pad_to=(Hp, Wp)`` (Hp even, Wp a multiple of 4): H and W only need to be even (``yuv420_picture_bytes``)
    and the result is [T,3(+1),Hp,Wp]: the picture converted with its chroma clamped at the picture's own edges, then reflect-padded on
    the right and bottom.  ``sigma='auto'`` / a sequence / a device tensor [T] and ``sigma_gain``: as for ``frames_to_input``; the
    estimate is taken on the converted RGB, where 4:2:0 chroma has smoothed the noise of two planes: expect it to read low (``sigma_gain``)."""
    def describe():
        desc, nbytes = _yuv_desc(H, W, pix_fmt, matrix, full_range, chroma, row_pitch, picture=pad_to is not None)
        desc.frame_stride = _surface_buffer(buf, None, nbytes, pix_fmt == "p010", "yuv420_to_input", "P010", "p010")
        return (ctypes.byref(desc),), None
    return _decode(("bsvd_yuv420_to_planar", "bsvd_yuv420_to_planar_pad"), buf, _frames_of(buf), 3, H, W, pad_to, sigma, sigma_gain, describe)


def output_to_yuv420(y, pix_fmt="nv12", matrix="bt709", full_range=False, chroma="linear", row_pitch=None, out=None, crop_to=None,
                     dither=None, dither_seed=0, frame0=0):
    """y: fp32 device tensor [T,3,H,W] RGB -> uint8 [T, frame_bytes] NV12 / P010 frames: clamp [0,1], matrix, chroma downsampling
    ('nearest': mean of the 2x2 block; 'linear': rows averaged, [1 2 1]/4 over columns), scale, clamp to the legal codes, round half
    to even.  ``out``: the caller's buffer [T, >= frame_bytes] to write into -- pitch padding and the bytes between frames are left
    as they were; without it the result's padding is zero.  ``crop_to=(H, W)`` (even): the surfaces, H x W, of ``y[..., :H, :W]``; the
    rows and columns of ``y`` beyond reach no sample.  ``dither`` None | 'ordered' | 'random': a value in (-0.5, 0.5) code joins every
    scaled Y, Cb and Cr right before the clamp and the rounding (8 x 8 Bayer, static; or a hash of ``dither_seed``, the frame's stream index
    ``frame0 + t``, the component and the position) -- a whole code is never moved (include/bsvd_hip.h, BsvdDither)."""
    dith = _dither_struct(dither, dither_seed, frame0)
    _tensor(y, torch.float32, (None, 3, None, None), "cuda", "expected a float32 device tensor [T,3,H,W]", contiguous=False)

    def describe(T, H, W):
        desc, nbytes = _yuv_desc(H, W, pix_fmt, matrix, full_range, chroma, row_pitch, picture=crop_to is not None)
        return desc, nbytes, pix_fmt == "p010", (ctypes.byref(desc),)
    return _encode("output_to_yuv420", ("bsvd_planar_to_yuv420", "bsvd_planar_to_yuv420_crop", "bsvd_planar_to_yuv420_crop_d"), y, crop_to,
                   describe, dith, out, bool(row_pitch), ("P010", "p010"))


# ---------------------------------------------------------------------------------------------------
# planar, 4:2:2 and 4:4:4 surfaces (include/bsvd_hip.h, BsvdYuvSurface): the names of _lib.YUV_FORMATS, ffmpeg's

def _per_plane(v, what, planes, slots=3):
    """pitches / offsets: None, or up to ``planes`` non-negative ints (None or 0 = tight / directly behind the plane before) -> the
    ``slots`` values of the descriptor's array"""
    if v is None:
        return (0,) * slots
    try:
        v = [int(x or 0) for x in v]
    except TypeError:
        raise ValueError("%s: expected a sequence of up to %d ints, got %r" % (what, planes, v)) from None
    if len(v) > planes or any(x < 0 for x in v):
        raise ValueError("%s %r: the layout has %d plane(s); values must not be negative" % (what, v, planes))
    return tuple(v) + (0,) * (slots - len(v))


def yuv_planes(pix_fmt):
    """planes of a surface format: 3 (Y, Cb, Cr), 2 (Y, interleaved CbCr) or 1 (packed)"""
    if pix_fmt not in _lib.YUV_FORMATS:
        raise ValueError("pix_fmt %r: one of %s" % (pix_fmt, ", ".join(sorted(_lib.YUV_FORMATS))))
    return {_lib.LAYOUT_PLANAR: 3, _lib.LAYOUT_SEMIPLANAR: 2}.get(_lib.YUV_FORMATS[pix_fmt][1], 1)


def _yuv_surface(H, W, pix_fmt, matrix, full_range, chroma, pitches, offsets, picture):
    """-> (BsvdYuvSurface, frame_bytes); ValueError for a name or a size the library would refuse.  picture: a surface for the pad / crop
    entry points, whose H and W need not be multiples of 4"""
    planes = yuv_planes(pix_fmt)
    for what, name, table in (("matrix", matrix, _lib.MATRIX), ("chroma", chroma, _lib.CHROMA)):
        if name not in table:
            raise ValueError("%s %r: one of %s" % (what, name, ", ".join(sorted(table))))
    sub, layout, bits, high = _lib.YUV_FORMATS[pix_fmt]
    surf = _lib.BsvdYuvSurface(subsampling=sub, layout=layout, bits=bits, high_bits=high, matrix=_lib.MATRIX[matrix],
                               full_range=1 if full_range else 0, chroma=_lib.CHROMA[chroma])
    surf.pitch[:] = _per_plane(pitches, "pitches", planes)
    surf.offset[:] = _per_plane(offsets, "offsets", planes)
    H, W = int(H), int(W)
    if not picture and (H <= 0 or W <= 0 or H % 4 or W % 4):
        raise ValueError("%s frame %d x %d: H and W must be positive multiples of 4 (or use pad_to / crop_to)" % (pix_fmt, H, W))
    nbytes = _lib.load().bsvd_yuv_frame_bytes(H, W, ctypes.byref(surf))
    if nbytes < 0:
        raise ValueError("%s frame %d x %d with pitches %s, offsets %s: H and W must be at least 2%s, a pitch (bytes%s) at least its plane's row"
                         % (pix_fmt, H, W, pitches, offsets, {_lib.SUB_420: " and even", _lib.SUB_422: ", W even"}.get(sub, ""),
                            ", even" if bits > 8 else ""))
    return surf, nbytes


def yuv_frame_bytes(H, W, pix_fmt, pitches=None, offsets=None):
    """Bytes of one frame of a planar, 4:2:2 or 4:4:4 surface (``_lib.YUV_FORMATS``): the end of its last plane.  ``pitches``: bytes per
    row of each plane, None / 0 = tight; ``offsets``: byte offset of each plane from the frame start, None / 0 for planes 1 and 2 =
    directly behind the plane before.  Any picture size the format can carry (``pad_to`` / ``crop_to``)."""
    return _yuv_surface(H, W, pix_fmt, "bt709", False, "linear", pitches, offsets, picture=True)[1]


def yuv_to_input(buf, H, W, pix_fmt="yuv420p", matrix="bt709", full_range=False, chroma="linear", sigma=None, pitches=None, pad_to=None,
                 offsets=None, sigma_gain=1.0):
    """``yuv420_to_input`` for the planar, 4:2:2 and 4:4:4 surfaces (pix_fmt: one of ``_lib.YUV_FORMATS``): buf uint8 device tensor
    [T, frame_bytes] (``yuv_frame_bytes``) -> fp32 [T,3(+1),H,W] RGB, not clamped.  4:2:2 chroma is upsampled along the row only
    ('linear': co-sited with the even columns), 4:4:4 not at all.  ``pitches`` / ``offsets``: see ``yuv_frame_bytes``.  ``pad_to=(Hp, Wp)``
    (Wp a multiple of 4; Hp even for 4:2:0): any picture size the format can carry, reflect-padded on the right and bottom after
    conversion.  ``sigma='auto'`` / a sequence / a device tensor [T] and ``sigma_gain``: as for ``yuv420_to_input`` (with subsampled
    chroma the estimate reads low)."""
    def describe():
        surf, nbytes = _yuv_surface(H, W, pix_fmt, matrix, full_range, chroma, pitches, offsets, picture=pad_to is not None)
        surf.frame_stride = _surface_buffer(buf, None, nbytes, surf.bits > 8, "yuv_to_input")
        return (ctypes.byref(surf),), None
    return _decode(("bsvd_yuv_to_planar", "bsvd_yuv_to_planar_pad"), buf, _frames_of(buf), 3, H, W, pad_to, sigma, sigma_gain, describe)


def output_to_yuv(y, pix_fmt="yuv420p", matrix="bt709", full_range=False, chroma="linear", pitches=None, out=None, crop_to=None, offsets=None,
                  dither=None, dither_seed=0, frame0=0):
    """``output_to_yuv420`` for the planar, 4:2:2 and 4:4:4 surfaces: y fp32 device tensor [T,3,H,W] RGB -> uint8 [T, frame_bytes].
    4:2:2 chroma is filtered along the row only ('nearest': mean of the two columns; 'linear': [1 2 1]/4), 4:4:4 not at all.  ``out``: the
    caller's buffer [T, >= frame_bytes] -- pitch padding, the bytes between planes and between frames are left as they were; without it
    the result's padding is zero.  ``crop_to=(H, W)``: the surfaces of ``y[..., :H, :W]``.  ``dither`` / ``dither_seed`` / ``frame0``: as for
    ``output_to_yuv420``; subsampled chroma is dithered on the chroma grid."""
    dith = _dither_struct(dither, dither_seed, frame0)
    _tensor(y, torch.float32, (None, 3, None, None), "cuda", "expected a float32 device tensor [T,3,H,W]", contiguous=False)

    def describe(T, H, W):
        surf, nbytes = _yuv_surface(H, W, pix_fmt, matrix, full_range, chroma, pitches, offsets, picture=crop_to is not None)
        return surf, nbytes, surf.bits > 8, (ctypes.byref(surf),)
    return _encode("output_to_yuv", ("bsvd_planar_to_yuv", "bsvd_planar_to_yuv_crop", "bsvd_planar_to_yuv_crop_d"), y, crop_to, describe, dith, out,
                   bool(pitches or offsets))


# ---------------------------------------------------------------------------------------------------
# RGB surfaces (include/bsvd_hip.h, BsvdRgbSurface): the names of _lib.RGB_FORMATS, ffmpeg's

def rgb_planes(pix_fmt):
    """planes of an RGB surface format: 1 (packed) or 3 / 4 (gbrp* / gbrap*)"""
    if pix_fmt not in _lib.RGB_FORMATS:
        raise ValueError("pix_fmt %r: one of %s" % (pix_fmt, ", ".join(sorted(_lib.RGB_FORMATS))))
    layout, components = _lib.RGB_FORMATS[pix_fmt][:2]
    return components if layout == _lib.RGB_PLANAR else 1


def rgb_has_alpha(pix_fmt):
    rgb_planes(pix_fmt)
    return _lib.RGB_FORMATS[pix_fmt][4] == _lib.FOURTH_ALPHA


def rgb_sample_dtype(pix_fmt):
    """torch dtype of a sample's container (and of the alpha side plane): uint8, or uint16 for the formats above 8 bits"""
    rgb_planes(pix_fmt)
    return torch.uint8 if _lib.RGB_FORMATS[pix_fmt][2] == 8 else torch.uint16


def _rgb_surface(H, W, pix_fmt, full_range, pitches, offsets, picture):
    """-> (BsvdRgbSurface, frame_bytes); ValueError for a name or a size the library would refuse.  picture: a surface for pad_to / crop_to,
    whose H and W need not be multiples of 4"""
    planes = rgb_planes(pix_fmt)
    layout, components, bits, pos, fourth = _lib.RGB_FORMATS[pix_fmt]
    surf = _lib.BsvdRgbSurface(layout=layout, components=components, bits=bits, fourth=fourth, full_range=1 if full_range else 0)
    surf.pos[:] = pos
    surf.pitch[:] = _per_plane(pitches, "pitches", planes, 4)
    surf.offset[:] = _per_plane(offsets, "offsets", planes, 4)
    H, W = int(H), int(W)
    if not picture and (H <= 0 or W <= 0 or H % 4 or W % 4):
        raise ValueError("%s frame %d x %d: H and W must be positive multiples of 4 (or use pad_to / crop_to)" % (pix_fmt, H, W))
    lib = _lib.load()
    nbytes = lib.bsvd_rgb_frame_bytes(H, W, ctypes.byref(surf))
    if nbytes < 0:
        raise ValueError("%s frame %d x %d with pitches %s, offsets %s: %s" % (pix_fmt, H, W, pitches, offsets, lib.bsvd_last_error().decode()
                                                                               if H > 0 and W > 0 else "H and W must be positive"))
    return surf, nbytes


def rgb_frame_bytes(H, W, pix_fmt, pitches=None, offsets=None):
    """Bytes of one frame of an RGB surface (``_lib.RGB_FORMATS``): the end of its last plane.  ``pitches``: bytes per row of each plane,
    None / 0 = tight; ``offsets``: byte offset of each plane from the frame start, None / 0 for a later plane = directly behind the plane
    before.  Any picture size."""
    return _rgb_surface(H, W, pix_fmt, True, pitches, offsets, picture=True)[1]


def _alpha_plane(alpha, T, H, W, pix_fmt, device, what):
    dtype = rgb_sample_dtype(pix_fmt)
    return _tensor(alpha, dtype, (T, H, W), device, "%s: expected a contiguous %s tensor [%d,%d,%d] on %s" % (what, dtype, T, H, W, device))


def rgb_to_input(buf, H, W, pix_fmt, full_range=True, sigma=None, pitches=None, offsets=None, pad_to=None, sigma_gain=1.0, return_alpha=False):
    """buf: uint8 device tensor [T, frame_bytes] of RGB surfaces (``rgb_frame_bytes``; rows longer than one frame are frames that far
    apart; 16-bit callers view their uint16 as bytes) -> fp32 [T,3(+1),H,W] in R, G, B order, the tensor ``frames_to_input`` builds; with
    ``sigma`` the noise-map channel is appended.  pix_fmt: one of ``_lib.RGB_FORMATS`` (packed 8 / 16 bit in any component order with alpha
    or a filler, x2rgb10le / x2bgr10le, planar gbrp / gbrap at 8, 10, 12, 16 bits).  full_range (the default): code / (2^bits - 1); False:
    (code - 16 s) / (219 s).  NOT clamped.  ``pitches`` / ``offsets``: see ``rgb_frame_bytes``.  ``pad_to=(Hp, Wp)``: any picture size,
    reflect-padded on the right and bottom after conversion.  ``sigma='auto'`` / a sequence / a device tensor [T] and ``sigma_gain``: as for
    ``frames_to_input``.  ``return_alpha`` (formats with alpha): True -> (x, alpha), alpha the frames' alpha codes as they are, a device
    tensor [T,H,W] (uint8, uint16 above 8 bits), picture-sized also with ``pad_to``; a tensor of that shape: written into and returned."""
    if return_alpha is not False and not rgb_has_alpha(pix_fmt):
        raise ValueError("rgb_to_input(return_alpha=): pix_fmt %r carries no alpha" % (pix_fmt,))

    def describe():
        surf, nbytes = _rgb_surface(H, W, pix_fmt, full_range, pitches, offsets, picture=pad_to is not None)
        surf.frame_stride = _surface_buffer(buf, None, nbytes, surf.bits > 8, "rgb_to_input", "16-bit", "16-bit")
        alpha = None
        if return_alpha is True:
            alpha = torch.empty((buf.shape[0], int(H), int(W)), dtype=rgb_sample_dtype(pix_fmt), device=buf.device)
        elif return_alpha is not False:
            alpha = _alpha_plane(return_alpha, buf.shape[0], int(H), int(W), pix_fmt, buf.device, "rgb_to_input(return_alpha=)")
        return (ctypes.byref(surf), None if alpha is None else alpha.data_ptr()), alpha
    return _decode((None, "bsvd_rgb_to_planar"), buf, _frames_of(buf), 3, H, W, pad_to, sigma, sigma_gain, describe)


def output_to_rgb(y, pix_fmt, full_range=True, pitches=None, offsets=None, out=None, crop_to=None, alpha=None, dither=None, dither_seed=0,
                  frame0=0):
    """y: fp32 device tensor [T,3,H,W] (R, G, B) -> uint8 [T, frame_bytes] RGB surfaces: clamp [0,1], scale (+ 16 s at limited range), round
    half to even.  A filler sample is written as all ones.  ``alpha`` (formats with alpha): the codes to write, a device tensor [T,H,W]
    (uint8, uint16 above 8 bits; picture-sized also with ``crop_to``) -- what ``rgb_to_input(return_alpha=True)`` gave; None: the maximum
    code, opaque.  ``out``: the caller's buffer [T, >= frame_bytes] -- pitch padding, the bytes between planes and between frames are left
    as they were; without it the result's padding is zero.  ``crop_to=(H, W)``: the surfaces of ``y[..., :H, :W]``.  ``dither`` /
    ``dither_seed`` / ``frame0``: as for ``output_to_yuv420``, on R, G and B before the rounding; alpha and fillers are never dithered."""
    dith = _dither_struct(dither, dither_seed, frame0)
    if alpha is not None and not rgb_has_alpha(pix_fmt):
        raise ValueError("output_to_rgb(alpha=): pix_fmt %r carries no alpha" % (pix_fmt,))
    rgb_planes(pix_fmt)
    _tensor(y, torch.float32, (None, 3, None, None), "cuda", "expected a float32 device tensor [T,3,H,W]", contiguous=False)

    def describe(T, H, W):
        surf, nbytes = _rgb_surface(H, W, pix_fmt, full_range, pitches, offsets, picture=crop_to is not None)
        if alpha is not None:
            _alpha_plane(alpha, T, H, W, pix_fmt, y.device, "output_to_rgb(alpha=)")
        return surf, nbytes, surf.bits > 8, (ctypes.byref(surf), None if alpha is None else alpha.data_ptr())
    return _encode("output_to_rgb", (None, "bsvd_planar_to_rgb", "bsvd_planar_to_rgb_d"), y, crop_to, describe, dith, out, bool(pitches or offsets),
                   ("16-bit", "16-bit"))
