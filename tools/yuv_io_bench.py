#!/usr/bin/env python3
"""The record behind profiles/yuv420_io.txt: the YUV 4:2:0 frame I/O kernels beside the uint8 RGB pair they stand next to.

  kernels : device time of bsvd_yuv420_to_planar / bsvd_planar_to_yuv420 (NV12 and P010, chroma 'linear', BT.709 limited) and of
            bsvd_u8_to_planar / bsvd_planar_to_u8 on the same 1080 x 1920 frames, one and ten per launch, in one process: HIP events
            around 200 launches after 20 warm-ups, three rounds interleaved, with the bytes each launch has to move.
            The pad / crop entry points (bsvd_*_pad / bsvd_*_crop) run beside them in the same rounds; --size HxW picks the picture
            (default 1080x1920).  With a size that is no multiple of 4 (480x854) the pad / crop entries take the picture and the tensor of the
            next multiples of 4, the existing YUV entries -- which cannot take the picture -- that network size (480x856), the existing uint8
            entries the picture.
  host    : tools/yuv_denoise.py (NV12 file in, file out) against tools/live_stream.py (RGB24) as child processes, alternating, twice.
  hostpad : the same two tools at 854x480 (pad='reflect') against 856x480, alternating, twice.

  formats : bsvd_yuv_to_planar / bsvd_planar_to_yuv on each of the ten planar / 4:2:2 / 4:4:4 surface formats beside the NV12 kernels, one
            frame per launch, same process, five rounds interleaved (the record behind profiles/yuv_formats.txt).
  hostfmt : tools/yuv_denoise.py on nv12, yuv420p and uyvy422 files at 1080p and 540 x 960, alternating, twice (same record).

    python tools/yuv_io_bench.py kernels|host|hostpad|all|formats|hostfmt [--size 1080x1920] [--out profiles/yuv420_io.txt]"""
import argparse, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def kernels(say, H=1080, W=1920):
    import torch
    from bsvd_amd.frame_io import network_size, yuv420_picture_bytes
    dev = torch.device("cuda", 0)
    sigma = 30 / 255.0
    Hn, Wn = network_size(H, W)
    say("kernels: %d x %d pictures (network size %d x %d) on %s; device time per launch, HIP events around 200 launches after 20 warm-ups, 3 rounds"
        % (H, W, Hn, Wn, torch.cuda.get_device_name(0)))
    say("%-44s %2s %10s %10s %10s %9s %8s" % ("launch", "T", "us (min)", "us (med)", "us (max)", "MB moved", "TB/s"))

    def timed(fn):
        for _ in range(20):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(200):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / 200

    import ctypes
    from bsvd_amd import _lib
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rs = np.random.RandomState(0)
    med = {}
    size = "%dx%d" % (H, W)
    nsize = "%dx%d" % (Hn, Wn)
    for T in (1, 10):
        # every launch below writes into preallocated memory
        rgb8 = torch.from_numpy(rs.randint(0, 256, (T, H, W, 3)).astype(np.uint8)).to(dev)
        o8 = torch.empty_like(rgb8)
        x4 = torch.rand((T, 4, H, W), device=dev)                 # picture-sized tensors: the existing uint8 entries
        y3 = torch.rand((T, 3, H, W), device=dev)
        x4n = torch.rand((T, 4, Hn, Wn), device=dev)              # network-sized: the pad / crop entries, the existing YUV entries
        y3n = torch.rand((T, 3, Hn, Wn), device=dev)
        px, pxn = T * H * W, T * Hn * Wn
        cases = [("bsvd_u8_to_planar (rgb24 hwc) %s" % size, "dec", lambda: lib.bsvd_u8_to_planar(rgb8.data_ptr(), x4.data_ptr(), T, 3, H, W, 1, 1, sigma, st), px * (3 + 16)),
                 ("bsvd_planar_to_u8 (rgb24 hwc) %s" % size, "enc", lambda: lib.bsvd_planar_to_u8(y3.data_ptr(), o8.data_ptr(), T, 3, H, W, 1, 0, st), px * (12 + 3)),
                 ("bsvd_u8_to_planar_pad (rgb24 hwc) %s" % size, "dec",
                  lambda: lib.bsvd_u8_to_planar_pad(rgb8.data_ptr(), x4n.data_ptr(), T, 3, H, W, Hn, Wn, 1, 1, sigma, st), px * 3 + pxn * 16),
                 ("bsvd_planar_to_u8_crop (rgb24 hwc) %s" % size, "enc",
                  lambda: lib.bsvd_planar_to_u8_crop(y3n.data_ptr(), o8.data_ptr(), T, 3, Hn, Wn, H, W, 1, 0, st), px * (12 + 3))]
        keep = []
        for fmt, bpp in (("nv12", 1.5), ("p010", 3.0)):
            surf_n = torch.from_numpy(rs.randint(0, 256, (T, yuv420_picture_bytes(Hn, Wn, fmt))).astype(np.uint8)).to(dev)
            surf = torch.from_numpy(rs.randint(0, 256, (T, yuv420_picture_bytes(H, W, fmt))).astype(np.uint8)).to(dev)
            out_n, out = torch.empty_like(surf_n), torch.empty_like(surf)
            d = _lib.BsvdYuvDesc(pix_fmt=_lib.PIX_FMT[fmt], matrix=_lib.MATRIX["bt709"], full_range=0, chroma=_lib.CHROMA["linear"])
            keep.append((surf, surf_n, out, out_n, d))
            cases.append(("bsvd_yuv420_to_planar (%s) %s" % (fmt, nsize), "dec",
                          lambda s=surf_n, d=d: lib.bsvd_yuv420_to_planar(s.data_ptr(), x4n.data_ptr(), T, Hn, Wn, ctypes.byref(d), 1, sigma, st), pxn * (bpp + 16)))
            cases.append(("bsvd_planar_to_yuv420 (%s) %s" % (fmt, nsize), "enc",
                          lambda o=out_n, d=d: lib.bsvd_planar_to_yuv420(y3n.data_ptr(), o.data_ptr(), T, Hn, Wn, ctypes.byref(d), st), pxn * (12 + bpp)))
            cases.append(("bsvd_yuv420_to_planar_pad (%s) %s" % (fmt, size), "dec",
                          lambda s=surf, d=d: lib.bsvd_yuv420_to_planar_pad(s.data_ptr(), x4n.data_ptr(), T, H, W, Hn, Wn, ctypes.byref(d), 1, sigma, st), px * bpp + pxn * 16))
            cases.append(("bsvd_planar_to_yuv420_crop (%s) %s" % (fmt, size), "enc",
                          lambda o=out, d=d: lib.bsvd_planar_to_yuv420_crop(y3n.data_ptr(), o.data_ptr(), T, Hn, Wn, H, W, ctypes.byref(d), st), px * (12 + bpp)))
        for name, _, fn, _ in cases:
            assert fn() == 0, name
        times = {name: [] for name, _, _, _ in cases}
        for _ in range(3):
            for name, _, fn, _ in cases:
                times[name].append(timed(fn))
        for name, kind, _, nbytes in cases:
            t = sorted(times[name])
            med[(name, T)] = (kind, t[1])
            say("%-44s %2d %10.1f %10.1f %10.1f %9.1f %8.2f" % (name, T, t[0], t[1], t[2], nbytes / 1e6, nbytes / t[1] / 1e6))
    say("ratio to the existing uint8 kernel of the same direction (median / median; the expectation for the YUV kernels is <= 1.10):")
    for (name, T), (kind, t) in med.items():
        if not name.startswith(("bsvd_u8_to_planar (", "bsvd_planar_to_u8 (")):
            ref = [v[1] for (n, tt), v in med.items() if tt == T and v[0] == kind and n.startswith(("bsvd_u8_to_planar (", "bsvd_planar_to_u8 ("))][0]
            say("  %-44s T=%2d  %.2f" % (name, T, t / ref))
    say("(every launch goes through the C ABI into preallocated tensors; MB moved = the bytes a launch must read + write, fp32 side + surface side)")


def host(say):
    say("host to host: tools/yuv_denoise.py (NV12, 288 frames from a file, depth 2) against tools/live_stream.py (RGB24, 96 frames, its depth-2 "
        "overlap_blocks row), alternating, twice; steady = wall-clock rate over the second half of the feeds (yuv_denoise.py, file reads and "
        "writes included) / 1 over the mean feed call of the third pass (live_stream.py, frames in memory)")
    with tempfile.TemporaryDirectory() as tmp:
        for size in ("1080x1920", "540x960"):
            H, W = map(int, size.split("x"))
            src = os.path.join(tmp, "in_%s.nv12" % size)
            with open(src, "wb") as f:
                rs = np.random.RandomState(0)
                for _ in range(288):
                    f.write(rs.randint(0, 256, H * W * 3 // 2, dtype=np.uint8).tobytes())
            for rep in range(2):
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "yuv_denoise.py"), src, os.path.join(tmp, "out.nv12"), "--size", "%dx%d" % (W, H),
                                    "--pix-fmt", "nv12", "--sigma", "30", "--depth", "2"], stdout=subprocess.PIPE, text=True, timeout=600, check=True)
                j = json.loads(r.stdout.strip().splitlines()[-1])
                say("  %s #%d nv12  yuv_denoise.py : steady %.1f frames/s, feed p50 %.2f ms, p99 %.2f ms (whole run with file I/O and pipeline fill: %.1f frames/s)"
                    % (size, rep, j["steady_frames_per_s"], j["ms_per_feed"]["p50"], j["ms_per_feed"]["p99"], j["frames_per_s"]))
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "live_stream.py"), "--size", size], stdout=subprocess.PIPE, text=True, timeout=600, check=True)
                rows = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
                j = [row for row in rows if row["depth"] == 2 and row["overlap_blocks"]][0]
                say("  %s #%d rgb24 live_stream.py : steady %.1f frames/s, feed p50 %.2f ms, p99 %.2f ms"
                    % (size, rep, j["host_to_host_fps_steady"], j["feed_call_ms"]["p50"], j["feed_call_ms"]["p99"]))


def hostpad(say):
    say("host to host with a picture that is no multiple of 4: tools/yuv_denoise.py (NV12, 288 frames from a file, depth 2) and tools/live_stream.py "
        "(RGB24, 96 frames, its depth-2 overlap_blocks row) at 854 x 480 (pad='reflect': padded to 856 x 480 and cropped on the device) against "
        "856 x 480 (no pad), alternating, twice; figures as in the host section")
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(2):
            for W, H in ((854, 480), (856, 480)):
                src = os.path.join(tmp, "in_%d.nv12" % W)
                if not os.path.exists(src):
                    with open(src, "wb") as f:
                        rs = np.random.RandomState(0)
                        for _ in range(288):
                            f.write(rs.randint(0, 256, H * W * 3 // 2, dtype=np.uint8).tobytes())
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "yuv_denoise.py"), src, os.path.join(tmp, "out.nv12"), "--size", "%dx%d" % (W, H),
                                    "--pix-fmt", "nv12", "--sigma", "30", "--depth", "2"], stdout=subprocess.PIPE, text=True, timeout=600, check=True)
                j = json.loads(r.stdout.strip().splitlines()[-1])
                say("  %dx%d #%d nv12  yuv_denoise.py : steady %.1f frames/s, feed p50 %.2f ms, p99 %.2f ms (whole run with file I/O and pipeline fill: %.1f frames/s)"
                    % (W, H, rep, j["steady_frames_per_s"], j["ms_per_feed"]["p50"], j["ms_per_feed"]["p99"], j["frames_per_s"]))
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "live_stream.py"), "--size", "%dx%d" % (H, W)], stdout=subprocess.PIPE, text=True,
                                   timeout=600, check=True)
                rows = [json.loads(l) for l in r.stdout.strip().splitlines() if l.startswith("{")]
                j = [row for row in rows if row["depth"] == 2 and row["overlap_blocks"]][0]
                say("  %dx%d #%d rgb24 live_stream.py : steady %.1f frames/s, feed p50 %.2f ms, p99 %.2f ms"
                    % (W, H, rep, j["host_to_host_fps_steady"], j["feed_call_ms"]["p50"], j["feed_call_ms"]["p99"]))


def formats(say, H=1080, W=1920):
    """the record behind profiles/yuv_formats.txt, kernels: bsvd_yuv_to_planar / bsvd_planar_to_yuv on each of the ten surface formats beside
    bsvd_yuv420_to_planar / bsvd_planar_to_yuv420 on NV12, one frame per launch, same process, rounds interleaved"""
    import ctypes
    import torch
    from bsvd_amd import _lib
    from bsvd_amd.frame_io import yuv420_frame_bytes, yuv_frame_bytes
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sigma = 30 / 255.0
    say("formats: %d x %d frames, one per launch, chroma 'linear', BT.709 limited, on %s; device us per launch (= per frame), HIP events around 200 "
        "launches after 20 warm-ups, 5 rounds interleaved over all rows" % (H, W, torch.cuda.get_device_name(0)))

    def timed(fn):
        for _ in range(20):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(200):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / 200

    rs = np.random.RandomState(0)
    x4 = torch.rand((1, 4, H, W), device=dev)
    y3 = torch.rand((1, 3, H, W), device=dev)
    px = H * W
    nb = yuv420_frame_bytes(H, W, "nv12")
    s0 = torch.from_numpy(rs.randint(0, 256, (1, nb)).astype(np.uint8)).to(dev)
    o0 = torch.empty_like(s0)
    d0 = _lib.BsvdYuvDesc(pix_fmt=_lib.PIX_FMT["nv12"], matrix=_lib.MATRIX["bt709"], full_range=0, chroma=_lib.CHROMA["linear"])
    keep = [s0, o0, d0]
    cases = [("bsvd_yuv420_to_planar (nv12)", "dec", lambda: lib.bsvd_yuv420_to_planar(s0.data_ptr(), x4.data_ptr(), 1, H, W, ctypes.byref(d0), 1, sigma, st), nb + px * 16),
             ("bsvd_planar_to_yuv420 (nv12)", "enc", lambda: lib.bsvd_planar_to_yuv420(y3.data_ptr(), o0.data_ptr(), 1, H, W, ctypes.byref(d0), st), nb + px * 12)]
    for fmt in sorted(_lib.YUV_FORMATS):
        sub, layout, bits, high = _lib.YUV_FORMATS[fmt]
        nb = yuv_frame_bytes(H, W, fmt)
        s = torch.from_numpy(rs.randint(0, 256, (1, nb)).astype(np.uint8)).to(dev)
        o = torch.empty_like(s)
        d = _lib.BsvdYuvSurface(subsampling=sub, layout=layout, bits=bits, high_bits=high, matrix=_lib.MATRIX["bt709"], full_range=0,
                                chroma=_lib.CHROMA["linear"])
        keep += [s, o, d]
        cases.append(("bsvd_yuv_to_planar (%s)" % fmt, "dec",
                      lambda s=s, d=d: lib.bsvd_yuv_to_planar(s.data_ptr(), x4.data_ptr(), 1, H, W, ctypes.byref(d), 1, sigma, st), nb + px * 16))
        cases.append(("bsvd_planar_to_yuv (%s)" % fmt, "enc",
                      lambda o=o, d=d: lib.bsvd_planar_to_yuv(y3.data_ptr(), o.data_ptr(), 1, H, W, ctypes.byref(d), st), nb + px * 12))
    for name, _, fn, _ in cases:
        assert fn() == 0, name
    times = {name: [] for name, _, _, _ in cases}
    for _ in range(5):
        for name, _, fn, _ in cases:
            times[name].append(timed(fn))
    ref = {kind: sorted(times[name])[2] for name, kind, _, _ in cases[:2]}
    say("%-38s %10s %10s %10s %9s %8s %9s" % ("launch", "us (min)", "us (med)", "us (max)", "MB moved", "TB/s", "/ nv12"))
    for name, kind, _, nbytes in cases:
        t = sorted(times[name])
        say("%-38s %10.1f %10.1f %10.1f %9.1f %8.2f %9.2f" % (name, t[0], t[2], t[4], nbytes / 1e6, nbytes / t[2] / 1e6, t[2] / ref[kind]))
    say("(MB moved = the bytes a launch must read + write, fp32 side + surface side; / nv12 = median over the NV12 kernel's of the same direction)")


def hostfmt(say, frames=192):
    """... and streams: tools/yuv_denoise.py host to host on nv12, yuv420p and uyvy422 files of the same size, alternating, twice"""
    say("host to host: tools/yuv_denoise.py (%d frames from a file, depth 2) with nv12, yuv420p and uyvy422, alternating, twice; steady = wall-clock "
        "rate over the second half of the feeds, file reads and writes included" % frames)
    from bsvd_amd.frame_io import yuv420_frame_bytes, yuv_frame_bytes
    with tempfile.TemporaryDirectory() as tmp:
        for size in ("1080x1920", "540x960"):
            H, W = map(int, size.split("x"))
            for fmt in ("nv12", "yuv420p", "uyvy422"):
                nb = yuv420_frame_bytes(H, W, fmt) if fmt == "nv12" else yuv_frame_bytes(H, W, fmt)
                with open(os.path.join(tmp, "in_%s.%s" % (size, fmt)), "wb") as f:
                    rs = np.random.RandomState(0)
                    for _ in range(frames):
                        f.write(rs.randint(0, 256, nb, dtype=np.uint8).tobytes())
            for rep in range(2):
                for fmt in ("nv12", "yuv420p", "uyvy422"):
                    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "yuv_denoise.py"), os.path.join(tmp, "in_%s.%s" % (size, fmt)),
                                        os.path.join(tmp, "out.yuv"), "--size", "%dx%d" % (W, H), "--pix-fmt", fmt, "--sigma", "30", "--depth", "2"],
                                       stdout=subprocess.PIPE, text=True, timeout=600, check=True)
                    j = json.loads(r.stdout.strip().splitlines()[-1])
                    say("  %s #%d %-8s: steady %.1f frames/s, feed p50 %.2f ms, p99 %.2f ms (whole run with file I/O and pipeline fill: %.1f frames/s)"
                        % (size, rep, fmt, j["steady_frames_per_s"], j["ms_per_feed"]["p50"], j["ms_per_feed"]["p99"], j["frames_per_s"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "host", "hostpad", "all", "formats", "hostfmt"])
    ap.add_argument("--size", default="1080x1920", help="HxW of the pictures of the kernels section")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="keep what --out already holds")
    a = ap.parse_args()
    lines = open(a.out).read().splitlines() if a.out and a.append and os.path.exists(a.out) else []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    if a.what in ("kernels", "all"):
        kernels(say, *map(int, a.size.lower().split("x")))
    if a.what in ("host", "all"):
        host(say)
    if a.what in ("hostpad", "all"):
        hostpad(say)
    if a.what == "formats":                       # the record of the planar / 4:2:2 / 4:4:4 surfaces: profiles/yuv_formats.txt
        formats(say, *map(int, a.size.lower().split("x")))
    if a.what == "hostfmt":
        hostfmt(say)
