#!/usr/bin/env python3
"""The measurements of profiles/scene_cuts.txt (scene cuts: LiveStream(cuts='auto'), feedin_one_element(cut=True)).

    python tools/scene_cuts_bench.py kernels HxW        workload for `rocprofv3 --kernel-trace --stats` (a run of its own): per frame the
                                                       conversion (bsvd_u8_to_planar) and the two detector kernels, 5 warm-ups + 30 launches
    python tools/scene_cuts_bench.py streams [--parent DIR] [--sizes 1920x1080,960x540]
                                                       tools/yuv_denoise.py as a child process per row, host to host, profiler off: --cuts auto
                                                       and --cuts none alternating twice on a one-scene file (what the detector costs), DIR's
                                                       own yuv_denoise.py (a checkout of the parent commit with its library built) in the same
                                                       alternation, then --cuts auto on a file with a cut every 30 frames (what cuts cost)
    python tools/scene_cuts_bench.py steps HxW         device events per feedin_one_element step for the 20 steps around a cut (first, second
                                                       and third sighting of its ring phase), and the flush-and-restart alternative

Frames are synthetic (grey fields constant on 16-pixel blocks, white noise): rates, not pictures."""
import argparse, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def _size(text):
    a, b = text.lower().split("x")
    return int(a), int(b)


def _model(torch):
    import bsvd_amd
    torch.manual_seed(1234)
    return bsvd_amd.BSVD(chns=[64, 128, 256], mid_ch=64, norm="none", act="relu6", interm_ch=64, pretrain_ckpt=None,
                         precision="f16x3").to(torch.device("cuda", 0)).eval()


def kernels(H, W):
    import torch
    from bsvd_amd import frame_io as F
    dev = torch.device("cuda", 0)
    rs = np.random.default_rng(0)
    u8 = [torch.from_numpy(rs.integers(0, 256, (1, H, W, 3), dtype=np.uint8)).to(dev) for _ in range(2)]
    prev = None
    for i in range(35):
        x = F.frames_to_input(u8[i % 2], 0.1)
        sad, grid = F.scene_scores(x, prev=prev)
        prev = grid[0]
    torch.cuda.synchronize()
    print("kernels %dx%d: 35 frames, last sad %d over %d blocks" % (H, W, int(sad[0]), grid[0].numel()))


def _write_yuv(path, W, H, frames, scene_len):
    """yuv420p: limited-range grey luma, a new block field every scene_len frames, 8 noise fields reused in turn; neutral chroma"""
    rs = np.random.default_rng(1)
    noise = [rs.normal(0.0, 30.0, (H, W)).astype(np.float32) for _ in range(8)]
    chroma = np.full(H * W // 2, 128, np.uint8).tobytes()
    with open(path, "wb") as f:
        for t in range(frames):
            if t % scene_len == 0:
                field = np.kron(rs.uniform(16.0, 235.0, ((H + 15) // 16, (W + 15) // 16)), np.ones((16, 16)))[:H, :W].astype(np.float32)
            f.write(np.clip(np.rint(field + noise[t % 8]), 16, 235).astype(np.uint8).tobytes())
            f.write(chroma)


def streams(sizes, parent):
    tmp = tempfile.mkdtemp(prefix="scene_cuts_")
    tool = os.path.join(ROOT, "tools", "yuv_denoise.py")
    for W, H in sizes:
        n = 120 if W * H > 1000000 else 300
        one, cut = os.path.join(tmp, "one_%dx%d.yuv" % (W, H)), os.path.join(tmp, "cut_%dx%d.yuv" % (W, H))
        _write_yuv(one, W, H, n, n)
        _write_yuv(cut, W, H, n, 30)
        rows = []
        for rep in range(2):
            rows += [("--cuts auto", tool, one, ["--cuts", "auto"]), ("--cuts none", tool, one, ["--cuts", "none"])]
            if parent:
                rows.append(("parent commit", os.path.join(parent, "tools", "yuv_denoise.py"), one, []))
        rows += [("--cuts auto, a cut every 30 frames", tool, cut, ["--cuts", "auto"]), ("--cuts none, a cut every 30 frames", tool, cut, ["--cuts", "none"])]
        for i, (name, exe, src, extra) in enumerate(rows):
            p = subprocess.run([sys.executable, exe, src, os.devnull, "--size", "%dx%d" % (W, H), "--sigma", "30"] + extra, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                print("%dx%d %s: FAILED rc %d\n%s" % (W, H, name, p.returncode, p.stderr[-2000:]), flush=True)
                return 1                                    # nothing more is started on the device after a failure
            r = json.loads(p.stdout.strip().splitlines()[-1])
            print("%dx%d #%d %-36s: steady %7.2f frames/s, feed p50 %.2f ms, p99 %.2f ms (whole run %.1f frames/s, %d frames)%s"
                  % (W, H, i, name, r["steady_frames_per_s"], r["ms_per_feed"]["p50"], r["ms_per_feed"]["p99"], r["frames_per_s"], r["frames"],
                     ", cuts %s" % r["cuts"] if "cuts" in r else ""), flush=True)
        os.remove(one)
        os.remove(cut)
    os.rmdir(tmp)
    return 0


def steps(H, W):
    import torch
    from bsvd_amd.stream_plan import RING_PERIOD
    m = _model(torch)
    dev = torch.device("cuda", 0)
    x = torch.rand((4, 1, 4, H, W), device=dev)
    cuts = [60, 60 + 3 * RING_PERIOD, 60 + 6 * RING_PERIOD]
    n = cuts[-1] + 30
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    host, stats = [], []
    for t in range(n):
        t0 = time.perf_counter()
        ev[t][0].record()
        m.feedin_one_element(x[t % 4], cut=t in cuts)
        ev[t][1].record()
        host.append((time.perf_counter() - t0) * 1e3)
        stats.append(dict(m._stream_eng.stats))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    steady = np.median(ms[40:58])
    print("steps %dx%d feedin_one_element, bsvd_c64 f16x3: steady-state step %.3f ms (device events, median of steps 40..57)" % (H, W, steady))
    for c, what in zip(cuts, ("first sighting of this cut phase (batched launches)", "second sighting (graph captures)", "third sighting (graph replays only)")):
        a, b = stats[c - 1], stats[c + 17]
        print("cut at step %d, %s: batch launches +%d, captures +%d, replays +%d over 18 steps" % (c, what, b["batch_launches"] - a["batch_launches"],
              b["graph_captures"] - a["graph_captures"], b["graph_replays"] - a["graph_replays"]))
        print("   device ms, steps %d..%d: %s" % (c - 2, c + 17, " ".join("%.2f" % v for v in ms[c - 2:c + 18])))
        print("   host ms in the call    : %s" % " ".join("%.2f" % v for v in host[c - 2:c + 18]))
        print("   sum over the 20 steps: %.2f ms device, %.2f ms above 20 steady steps" % (sum(ms[c - 2:c + 18]), sum(ms[c - 2:c + 18]) - 20 * steady))
    # the alternative: flush (shift_num + 1 feeds of None, the pending frames still come out), reset, refill (shift_num feeds without output)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(m.shift_num + 1):
        m.feedin_one_element(None)
    m.reset()
    quiet = 0
    while m.feedin_one_element(x[0]) is None:
        quiet += 1
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    print("flush and restart: %d feeds of None + reset + %d feeds without output before the next frame comes out: %.2f ms wall clock (host, synchronised), "
          "%.1f steady steps' worth" % (m.shift_num + 1, quiet, wall, wall / steady))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "streams", "steps"])
    ap.add_argument("size", nargs="?", default="540x960", help="HxW (kernels, steps)")
    ap.add_argument("--sizes", default="1920x1080,960x540", help="WxH,... (streams)")
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    if a.what == "kernels":
        return kernels(*_size(a.size))
    if a.what == "steps":
        return steps(*_size(a.size))
    return streams([_size(s) for s in a.sizes.split(",")], a.parent)


if __name__ == "__main__":
    sys.exit(main() or 0)
