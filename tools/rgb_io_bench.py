#!/usr/bin/env python3
"""The measurements behind profiles/rgb_surfaces.txt.

    python tools/rgb_io_bench.py kernels [HxW]         workload for `rocprofv3 --kernel-trace --stats` (a run of its own): 30 decodes and
                                                       30 encodes of one HxW frame (default 1080x1920) for bgra, rgb48le, gbrp10le,
                                                       x2rgb10le and gbrp, and of bsvd_u8_to_planar / bsvd_planar_to_u8 in the same trace; prints the
                                                       bytes each kernel moves per frame, which with the trace's time per call gives bytes / us
    python tools/rgb_io_bench.py streams [--sizes 1920x1080,960x540]
                                                       host to host: tools/yuv_denoise.py --pix-fmt bgra and rgba64le against
                                                       tools/live_stream.py (RGB24, its depth 2 / overlap row), alternating twice, each a
                                                       process of its own; nothing more is started after a failure"""
import argparse, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

KERNEL_FORMATS = ("bgra", "rgb48le", "gbrp10le", "x2rgb10le", "gbrp")


def kernels(H, W):
    import torch
    from bsvd_amd import frame_io as F
    dev = torch.device("cuda", 0)
    rs = np.random.default_rng(0)
    y = torch.rand((1, 3, H, W), device=dev)
    fp32 = 3 * 4 * H * W
    u8 = torch.from_numpy(rs.integers(0, 256, (1, H, W, 3), dtype=np.uint8)).to(dev)
    for _ in range(30):
        F.frames_to_input(u8)
        F.output_to_frames(y)
    print("rgb24 (bsvd_u8_to_planar / bsvd_planar_to_u8): %d surface + %d fp32 = %d bytes per frame and direction" % (u8.numel(), fp32, u8.numel() + fp32))
    for name in KERNEL_FORMATS:
        n = F.rgb_frame_bytes(H, W, name)
        buf = torch.from_numpy(rs.integers(0, 256, (1, n), dtype=np.uint8)).to(dev)
        alpha = None
        for _ in range(30):
            if F.rgb_has_alpha(name):
                x, alpha = F.rgb_to_input(buf, H, W, name, return_alpha=True if alpha is None else alpha)
            else:
                x = F.rgb_to_input(buf, H, W, name)
            F.output_to_rgb(y, name, out=buf, alpha=alpha)
        side = 0 if alpha is None else alpha.numel() * alpha.element_size()
        print("%s: %d surface + %d fp32 + %d alpha plane = %d bytes per frame and direction" % (name, n, fp32, side, n + fp32 + side))
    torch.cuda.synchronize()


def _write_frames(path, nbytes, frames):
    rs = np.random.default_rng(1)
    pool = [rs.integers(0, 256, nbytes, dtype=np.uint8).tobytes() for _ in range(4)]
    with open(path, "wb") as f:
        for t in range(frames):
            f.write(pool[t % 4])


def streams(sizes):
    from bsvd_amd import frame_io as F
    tmp = tempfile.mkdtemp(prefix="rgb_io_")
    tool, live = os.path.join(ROOT, "tools", "yuv_denoise.py"), os.path.join(ROOT, "tools", "live_stream.py")
    for W, H in sizes:
        n = 72 if W * H > 1000000 else 200
        rows = [("rgb24 (live_stream.py)", None), ("bgra", "bgra"), ("rgba64le", "rgba64le")] * 2
        for i, (label, fmt) in enumerate(rows):
            if fmt is None:
                out = os.path.join(tmp, "live.json")
                cmd = [sys.executable, live, "--size", "%dx%d" % (H, W), "--frames", str(n), "--json", out]
            else:
                src = os.path.join(tmp, "%s_%dx%d.raw" % (fmt, W, H))
                if not os.path.exists(src):
                    _write_frames(src, F.rgb_frame_bytes(H, W, fmt), n)
                cmd = [sys.executable, tool, src, os.devnull, "--size", "%dx%d" % (W, H), "--sigma", "30", "--pix-fmt", fmt]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
            if p.returncode != 0:
                print("%dx%d %s: FAILED rc %d\n%s" % (W, H, label, p.returncode, p.stderr[-2000:]), flush=True)
                return 1                                    # nothing more is started on the device after a failure
            if fmt is None:
                r = [row for row in json.load(open(out))["rows"] if row["depth"] == 2 and row["overlap_blocks"]][0]
                print("%dx%d #%d %-24s: steady %7.2f frames/s (1 / mean feed), feed p50 %.2f ms, p99 %.2f ms, %d frames, third pass"
                      % (W, H, i, label, r["host_to_host_fps_steady"], r["feed_call_ms"]["p50"], r["feed_call_ms"]["p99"], n), flush=True)
            else:
                r = json.loads(p.stdout.strip().splitlines()[-1])
                print("%dx%d #%d %-24s: steady %7.2f frames/s (wall clock, file reads included), feed p50 %.2f ms, p99 %.2f ms, %d frames, first pass"
                      % (W, H, i, label, r["steady_frames_per_s"], r["ms_per_feed"]["p50"], r["ms_per_feed"]["p99"], r["frames"]), flush=True)
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["kernels", "streams"])
    ap.add_argument("size", nargs="?", default="1080x1920")
    ap.add_argument("--sizes", default="1920x1080,960x540")
    a = ap.parse_args()
    if a.mode == "kernels":
        H, W = map(int, a.size.lower().split("x"))
        return kernels(H, W)
    return streams([tuple(map(int, s.lower().split("x"))) for s in a.sizes.split(",")])


if __name__ == "__main__":
    sys.exit(main())
