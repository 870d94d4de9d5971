#!/usr/bin/env python3
"""Denoises a raw YUV stream -- NV12 or P010 frames, or planar / 4:2:2 / 4:4:4 ones (yuv420p, yuv420p10le, uyvy422, yuyv422, nv16,
p210le, yuv422p, yuv422p10le, yuv444p, yuv444p10le), as any `-f rawvideo` producer pipes them -- through
bsvd_amd.pipeline.LiveStream(pix_fmt=...): surfaces over PCIe, colour conversion on the device, one graph-replayed pipeline step per
frame.  The same for raw RGB streams (the file name is older than they are): --pix-fmt bgr24, rgba, bgra, argb, abgr, rgb0, bgr0, 0rgb, 0bgr,
rgb48le, bgr48le, rgba64le, bgra64le, x2rgb10le, x2bgr10le, gbrp, gbrp10le / 12le / 16le, gbrap, gbrap10le / 12le / 16le (rgb24: tools/live_stream.py); full
range unless --limited-range; any size; the alpha of a frame comes out with that frame, bit for bit.  Prints one JSON line: frames, frames_per_s (whole run, host to host, file I/O and pipeline fill included), ms_per_feed p50 / p99 and
steady_frames_per_s (wall clock, reads and writes included) over the steady state, the second half of the feeds.

    python tools/yuv_denoise.py IN OUT --size 1920x1080 --pix-fmt nv12 --sigma 30 [--matrix bt709] [--full-range] [--chroma linear]
                                [--depth 2] [--ckpt model.pth]                IN / OUT: a file, or - for stdin / stdout
    python tools/yuv_denoise.py IN OUT --size 1920x1080 --sigma auto [--sigma-gain 1.0]      the noise level of every frame estimated on the
                                device (LiveStream(sigma='auto')); the JSON line then carries last_sigma, in 8-bit code units.  Untested on
                                real footage; with subsampled chroma the estimate reads low, which --sigma-gain corrects
    python tools/yuv_denoise.py IN OUT --size 1920x1080 --sigma nlf [--sigma-gain 1.0]       for noise that depends on the signal level: a
                                noise-level function per frame (sigma at sixteen levels of local intensity) estimated on the device and a
                                per-pixel noise map written from it (LiveStream(sigma='nlf')); the JSON line then carries last_noise_curve,
                                in 8-bit code units.  Untested on real footage, and outside what the reference's checkpoints were trained on
    python tools/yuv_denoise.py IN OUT --size 1920x1080 --noise-model A,B                    the same map from a sensor model the caller
                                knows, sigma(I) = sqrt(A I + B) with I and sigma in 8-bit code units (frame_io.NoiseCurve.from_model)
    python tools/yuv_denoise.py IN OUT --size 1920x1080 --vst scene [--sigma-gain 1.0] [--vst-floor 0.5] | --vst-model A,B
                                for noise that depends on the signal level, inside what the checkpoints were trained on: a
                                variance-stabilising transform around the network (LiveStream(vst=)).  Intensities are remapped so that the
                                noise has one standard deviation sigma' everywhere, the noise plane is that constant, the result is mapped
                                back.  scene: the curve is estimated on the device from the first frame of every scene (combine with --cuts
                                auto); --vst-model: from the sensor model sigma(I) = sqrt(A I + B), 8-bit code units.  --vst-floor: the
                                least sigma the transform divides by, 8-bit code units.  Instead of --sigma / --noise-model.  The JSON line
                                carries last_vst_sigma (and last_noise_curve for scene), in 8-bit code units.  The effect on denoising
                                quality is unmeasured (no trained checkpoint has been run through it); untested on real footage
    python tools/yuv_denoise.py IN OUT --size 1920x1080 --sigma 30 --cuts auto [--cut-threshold 10]      scene cuts detected on the device
                                (LiveStream(cuts='auto')): no frame is mixed with a frame of another scene; the JSON line then carries the
                                frame numbers found.  Untested on real footage; a cut one or two frames after another cut scores low
    python tools/yuv_denoise.py IN OUT --size 1920x1080 --sigma 30 --strength 0.7 | --strength 0.5,1.0  [--dither ordered|random] [--dither-seed N]
                                the output finish, on the device: how much of the denoising to keep (one amount, or luma,chroma: 0.5,1.0
                                keeps half the luma grain and removes all chroma noise), and dither at the quantiser (8 x 8 Bayer, or a
                                per-frame hash) against banding (LiveStream(strength=, dither=)).  The visual effect is unmeasured on real footage
    python tools/yuv_denoise.py IN OUT --size 1920x1080 --sigma 30 --grain scene | --grain STD[,STD_CHROMA]  [--grain-amount A] [--grain-seed N]
                                film grain after denoising, from a MODEL instead of the removed signal (LiveStream(grain=)).  scene: the
                                first frame of every scene to emerge is measured against its source on the device, a model (strength per
                                luma level, spatial correlation) is fitted on the host -- one synchronisation per scene; combine with
                                --cuts auto -- and clean grain is synthesised from it onto the scene's frames.  STD[,STD_CHROMA]: white
                                grain of that standard deviation (8-bit code units) in luma and in the two colour differences.  The JSON
                                line carries the last model's std curves (8-bit code units).  Nothing has been measured on real footage,
                                and no encoder has read the model

    ffmpeg -i in.mp4 -pix_fmt yuv420p -f rawvideo - | python tools/yuv_denoise.py - - --size 1920x1080 --sigma 30 | ffmpeg -f rawvideo ...
                                                                                  (--pix-fmt defaults to yuv420p, ffmpeg's own default)

The width and height must be even (4:2:2: the width; 4:4:4: neither); a size that is no multiple of 4 (854x480) is reflect-padded to the next one and cropped again on the
device (LiveStream(pad='reflect')), the files hold pictures of the size given.  Without --ckpt the weights are seeded random ones (rates, not pictures), like
tools/live_stream.py."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from bsvd_amd import _lib, frame_io


def read_frames(f, nbytes):
    while True:
        raw = f.read(nbytes)
        if len(raw) < nbytes:                      # end of the stream (a trailing partial frame is dropped)
            return
        yield raw


def parse_sigma(text):
    """--sigma: 'auto', 'nlf', or the noise std in 8-bit code units -> what LiveStream(sigma=) takes"""
    if text in ("auto", "nlf"):
        return text
    try:
        return float(text) / 255.0
    except ValueError:
        raise argparse.ArgumentTypeError("--sigma %r: a number (8-bit code units, e.g. 30), auto or nlf" % text) from None


def parse_noise_model(text):
    """--noise-model A,B: sigma(I) = sqrt(A I + B), I and sigma in 8-bit code units -> frame_io.NoiseCurve ([0,1] units: a = A / 255, b = B / 255^2)"""
    try:
        A, B = (float(p) for p in text.split(","))
        return frame_io.NoiseCurve.from_model(A / 255.0, B / 255.0 ** 2)
    except ValueError:
        raise argparse.ArgumentTypeError("--noise-model %r: A,B with sigma(I) = sqrt(A I + B) in 8-bit code units" % text) from None


def parse_strength(text):
    """--strength: S or S_LUMA,S_CHROMA, each in [0, 1] -> what LiveStream(strength=) takes"""
    try:
        v = tuple(float(p) for p in text.split(","))
        return frame_io.check_strength(v[0] if len(v) == 1 else v)
    except ValueError:
        raise argparse.ArgumentTypeError("--strength %r: S or S_LUMA,S_CHROMA, each in [0, 1]" % text) from None


def parse_grain(text):
    """--grain: 'scene', or STD[,STD_CHROMA] in 8-bit code units -> what LiveStream(grain=) takes"""
    if text == "scene":
        return text
    try:
        v = [float(p) / 255.0 for p in text.split(",")]
        if len(v) not in (1, 2):
            raise ValueError(text)
        return frame_io.GrainModel.from_values([v[0], v[-1], v[-1]])
    except ValueError:
        raise argparse.ArgumentTypeError("--grain %r: scene, or STD[,STD_CHROMA] in 8-bit code units, not negative" % text) from None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--size", required=True, help="WxH of the pictures, e.g. 1920x1080")
    ap.add_argument("--pix-fmt", default="yuv420p", choices=["nv12", "p010"] + sorted(_lib.YUV_FORMATS) + sorted(set(_lib.RGB_FORMATS) - {'rgb24'}))
    ap.add_argument("--sigma", type=parse_sigma, default=None, help="noise std in 8-bit code units (e.g. 30); auto: estimated per frame on the device; "
                    "nlf: a noise-level curve per frame and a per-pixel noise map")
    ap.add_argument("--noise-model", type=parse_noise_model, default=None, help="A,B instead of --sigma: sigma(I) = sqrt(A I + B) in 8-bit code units")
    ap.add_argument("--sigma-gain", type=float, default=1.0, help="factor on the estimate of --sigma auto / nlf and of --vst scene")
    ap.add_argument("--vst", default=None, choices=["scene"], help="instead of --sigma: variance-stabilising transform, the curve estimated at every scene start")
    ap.add_argument("--vst-model", type=parse_noise_model, default=None, help="A,B instead of --sigma: the transform of sigma(I) = sqrt(A I + B), 8-bit code units")
    ap.add_argument("--vst-floor", type=float, default=frame_io.VST_FLOOR * 255.0, help="the least sigma the transform divides by, 8-bit code units (default 0.5)")
    ap.add_argument("--cuts", default="none", choices=["none", "auto"], help="auto: scene cuts detected per frame on the device")
    ap.add_argument("--cut-threshold", type=float, default=frame_io.CUT_THRESHOLD, help="score at which --cuts auto declares a scene start")
    ap.add_argument("--matrix", default="bt709", choices=["bt601", "bt709", "bt2020"])
    ap.add_argument("--full-range", action="store_true")
    ap.add_argument("--limited-range", action="store_true", help="RGB formats: codes span [16 s, 235 s] instead of the full range")
    ap.add_argument("--chroma", default="linear", choices=["nearest", "linear"])
    ap.add_argument("--strength", type=parse_strength, default=(1.0, 1.0), help="S or S_LUMA,S_CHROMA in [0, 1]: how much of the denoising to keep (default 1)")
    ap.add_argument("--dither", default="none", choices=["none", "ordered", "random"], help="dither at the quantiser, on the device")
    ap.add_argument("--dither-seed", type=int, default=0, help="seed of --dither random")
    ap.add_argument("--grain", type=parse_grain, default=None, help="scene: a grain model measured at every scene start; STD[,STD_CHROMA]: white grain, 8-bit code units")
    ap.add_argument("--grain-amount", type=float, default=1.0, help="factor on the model's standard deviations (default 1)")
    ap.add_argument("--grain-seed", type=int, default=0, help="seed of the grain pattern")
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--precision", default="f16x3")
    a = ap.parse_args(argv)
    vst = a.vst if a.vst is not None else a.vst_model
    if a.vst is not None and a.vst_model is not None:
        ap.error("--vst scene and --vst-model exclude each other")
    if vst is not None:
        if a.sigma is not None or a.noise_model is not None:
            ap.error("--vst / --vst-model stand in for --sigma / --noise-model: the noise plane is the transform's own sigma'")
        try:
            vst_floor = frame_io.check_vst_floor(a.vst_floor / 255.0)
        except ValueError as e:
            ap.error("--vst-floor %r (8-bit code units): %s" % (a.vst_floor, e))
    elif (a.sigma is None) == (a.noise_model is None):
        ap.error("one of --sigma, --noise-model, --vst and --vst-model is required")
    if a.noise_model is not None:
        a.sigma = a.noise_model
    try:
        frame_io.check_grain(a.grain, a.grain_amount, a.grain_seed)
    except ValueError as e:
        ap.error("--grain-amount / --grain-seed: %s" % e)
    W, H = map(int, a.size.lower().split("x"))
    rgb = a.pix_fmt in _lib.RGB_FORMATS                  # the RGB formats: 1-D frames too
    surface = a.pix_fmt in _lib.YUV_FORMATS or rgb       # the 1-D frames of the planar / 4:2:2 / 4:4:4 formats
    if rgb:
        sub, bits = _lib.SUB_444, 32 if _lib.RGB_FORMATS[a.pix_fmt][0] == _lib.RGB_PACKED_X2_10 else _lib.RGB_FORMATS[a.pix_fmt][2]
    else:
        sub, bits = (_lib.YUV_FORMATS[a.pix_fmt][0], _lib.YUV_FORMATS[a.pix_fmt][2]) if surface else (_lib.SUB_420, 8 if a.pix_fmt == "nv12" else 10)
    if W <= 2 or H <= 2 or (W % 2 and sub != _lib.SUB_444) or (H % 2 and sub == _lib.SUB_420):
        ap.error("--size %s: at least 3x3; the width must be even for 4:2:0 and 4:2:2, the height for 4:2:0" % a.size)
    pad = "reflect" if W % 4 or H % 4 else None
    dtype = np.dtype(np.uint8 if bits == 8 else "<u4" if bits == 32 else "<u2")
    nbytes = frame_io.rgb_frame_bytes(H, W, a.pix_fmt) if rgb else frame_io.yuv_frame_bytes(H, W, a.pix_fmt) if surface else W * H * 3 // 2 * dtype.itemsize

    import torch
    import bsvd_amd
    from bsvd_amd.pipeline import LiveStream
    torch.manual_seed(1234)
    m = bsvd_amd.BSVD(chns=[64, 128, 256], mid_ch=64, norm="none", act="relu6", interm_ch=64, pretrain_ckpt=a.ckpt,
                      precision=a.precision).to(torch.device("cuda", 0)).eval()
    live = LiveStream(m, sigma=a.sigma, sigma_gain=a.sigma_gain, depth=a.depth, frame_shape=(H, W), pix_fmt=a.pix_fmt,
                      colour={"full_range": not a.limited_range} if rgb else {"matrix": a.matrix, "full_range": a.full_range, "chroma": a.chroma}, pad=pad,
                      cuts="auto" if a.cuts == "auto" else None, cut_threshold=a.cut_threshold,
                      strength=a.strength, dither=None if a.dither == "none" else a.dither, dither_seed=a.dither_seed,
                      **(dict(vst=vst, vst_floor=vst_floor) if vst is not None else {}),
                      **(dict(grain=a.grain, grain_amount=a.grain_amount, grain_seed=a.grain_seed) if a.grain is not None else {}))
    found = []
    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    fout = sys.stdout.buffer if a.output == "-" else open(a.output, "wb")
    n_in = n_out = 0
    ms, done = [], []                              # per feed: time inside feed(), clock when its iteration (read, feed, write) ended
    t0 = time.perf_counter()
    for raw in read_frames(fin, nbytes):
        frame = np.frombuffer(raw, dtype) if surface else np.frombuffer(raw, dtype).reshape(H * 3 // 2, W)
        t1 = time.perf_counter()
        r = live.feed(frame)
        ms.append((time.perf_counter() - t1) * 1e3)
        if live.last_cut:
            found.append(n_in)
        n_in += 1
        if r is not None:
            fout.write(r.tobytes())
            n_out += 1
        done.append(time.perf_counter())
    for r in live.flush():
        fout.write(r.tobytes())
        n_out += 1
    fout.flush()
    total = time.perf_counter() - t0
    assert n_out == n_in, (n_in, n_out)
    # steady state: the second half of the feeds, behind the pipeline fill and the first ring cycles' graph captures
    k = max(live.latency + 1, n_in // 2)
    steady = np.array(ms[k:] or ms or [0.0])
    res = {"frames": n_out, "frames_per_s": n_out / total if total > 0 else 0.0,
           "ms_per_feed": {"p50": float(np.percentile(steady, 50)), "p99": float(np.percentile(steady, 99))},
           "steady_frames_per_s": (n_in - k) / (done[-1] - done[k - 1]) if n_in > k >= 1 else 0.0,       # wall clock, reads and writes included
           "size": "%dx%d" % (W, H), "pix_fmt": a.pix_fmt, "depth": a.depth, "frame_latency_feeds": live.latency, "pad": pad,
           "sigma": a.sigma if isinstance(a.sigma, str) or a.sigma is None else "noise-model" if a.noise_model is not None else a.sigma * 255.0}
    if vst is not None:
        res["vst"] = "scene" if a.vst is not None else "model"
        res["vst_floor"] = a.vst_floor
        res["last_vst_sigma"] = None if live.last_vst_sigma is None else live.last_vst_sigma * 255.0
        if a.vst is not None:
            res["sigma_gain"] = a.sigma_gain
            res["last_noise_curve"] = None if live.last_noise_curve is None else [v * 255.0 for v in live.last_noise_curve]
    if a.sigma == "nlf":
        res["sigma_gain"] = a.sigma_gain
        res["last_noise_curve"] = None if live.last_noise_curve is None else [v * 255.0 for v in live.last_noise_curve]
    if a.noise_model is not None:
        res["last_noise_curve"] = [v * 255.0 for v in a.noise_model.values]
    if a.sigma == "auto":
        res["sigma_gain"] = a.sigma_gain
        res["last_sigma"] = None if live.last_sigma is None else live.last_sigma * 255.0
    if a.strength != (1.0, 1.0):
        res["strength"] = list(a.strength)
    if a.dither != "none":
        res["dither"] = a.dither
    if a.grain is not None:
        res["grain"] = "scene" if a.grain == "scene" else "model"
        res["grain_amount"] = a.grain_amount
        res["last_grain_std"] = None if live.last_grain_model is None else (live.last_grain_model.std * 255.0).tolist()
    if a.cuts == "auto":
        res["cut_threshold"] = a.cut_threshold
        res["cuts"] = found
    print(json.dumps(res), file=sys.stderr if a.output == "-" else sys.stdout, flush=True)
    return res


if __name__ == "__main__":
    main()
