#!/usr/bin/env python3
"""The record behind profiles/yuv420_io.txt: the YUV 4:2:0 frame I/O kernels beside the uint8 RGB pair they stand next to.

  kernels : device time of bsvd_yuv420_to_planar / bsvd_planar_to_yuv420 (NV12 and P010, chroma 'linear', BT.709 limited) and of
            bsvd_u8_to_planar / bsvd_planar_to_u8 on the same 1080 x 1920 frames, one and ten per launch, in one process: HIP events
            around 200 launches after 20 warm-ups, three rounds interleaved, with the bytes each launch has to move.
  host    : tools/yuv_denoise.py (NV12 file in, file out) against tools/live_stream.py (RGB24) as child processes, alternating, twice.

    python tools/yuv_io_bench.py kernels|host|all [--out profiles/yuv420_io.txt]"""
import argparse, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def kernels(say):
    import torch
    from bsvd_amd.frame_io import frames_to_input, yuv420_frame_bytes
    dev = torch.device("cuda", 0)
    H, W, sigma = 1080, 1920, 30 / 255.0
    say("kernels: %d x %d frames on %s; device time per launch, HIP events around 200 launches after 20 warm-ups, 3 rounds" % (H, W, torch.cuda.get_device_name(0)))
    say("%-34s %2s %10s %10s %10s %9s %8s" % ("launch", "T", "us (min)", "us (med)", "us (max)", "MB moved", "TB/s"))

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
    for T in (1, 10):
        rgb8 = torch.from_numpy(rs.randint(0, 256, (T, H, W, 3)).astype(np.uint8)).to(dev)
        x4 = frames_to_input(rgb8, sigma)                         # every launch below writes into preallocated memory
        y3 = x4[:, :3].contiguous()
        o8 = torch.empty_like(rgb8)
        px = T * H * W
        cases = [("bsvd_u8_to_planar (rgb24 hwc)", "dec", lambda: lib.bsvd_u8_to_planar(rgb8.data_ptr(), x4.data_ptr(), T, 3, H, W, 1, 1, sigma, st), px * (3 + 16)),
                 ("bsvd_planar_to_u8 (rgb24 hwc)", "enc", lambda: lib.bsvd_planar_to_u8(y3.data_ptr(), o8.data_ptr(), T, 3, H, W, 1, 0, st), px * (12 + 3))]
        keep = []
        for fmt, bpp in (("nv12", 1.5), ("p010", 3.0)):
            surf = torch.from_numpy(rs.randint(0, 256, (T, yuv420_frame_bytes(H, W, fmt))).astype(np.uint8)).to(dev)
            out = torch.empty_like(surf)
            d = _lib.BsvdYuvDesc(pix_fmt=_lib.PIX_FMT[fmt], matrix=_lib.MATRIX["bt709"], full_range=0, chroma=_lib.CHROMA["linear"])
            keep.append((surf, out, d))
            cases.append(("bsvd_yuv420_to_planar (%s)" % fmt, "dec",
                          lambda s=surf, d=d: lib.bsvd_yuv420_to_planar(s.data_ptr(), x4.data_ptr(), T, H, W, ctypes.byref(d), 1, sigma, st), px * (bpp + 16)))
            cases.append(("bsvd_planar_to_yuv420 (%s)" % fmt, "enc",
                          lambda o=out, d=d: lib.bsvd_planar_to_yuv420(y3.data_ptr(), o.data_ptr(), T, H, W, ctypes.byref(d), st), px * (12 + bpp)))
        for name, _, fn, _ in cases:
            assert fn() == 0, name
        times = {name: [] for name, _, _, _ in cases}
        for _ in range(3):
            for name, _, fn, _ in cases:
                times[name].append(timed(fn))
        for name, kind, _, nbytes in cases:
            t = sorted(times[name])
            med[(name, T)] = (kind, t[1])
            say("%-34s %2d %10.1f %10.1f %10.1f %9.1f %8.2f" % (name, T, t[0], t[1], t[2], nbytes / 1e6, nbytes / t[1] / 1e6))
    say("ratio to the uint8 kernel of the same direction (median / median; the expectation is <= 1.10):")
    for (name, T), (kind, t) in med.items():
        if "yuv420" in name:
            ref = [v[1] for (n, tt), v in med.items() if tt == T and v[0] == kind and "yuv420" not in n][0]
            say("  %-34s T=%2d  %.2f" % (name, T, t / ref))
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "host", "all"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    if a.what in ("kernels", "all"):
        kernels(say)
    if a.what in ("host", "all"):
        host(say)
