#!/usr/bin/env python3
"""precision='f16' (one fp16 MFMA pass) beside 'f16x3' (three) on ONE box, in ONE process: the C1 clip [1,10,4,540,960] or, with
--workload c5, the 1080p per-frame stream of bench.py.  The modes ALTERNATE (--rounds, at least 2) so that a clock or thermal drift of
the box hits both; every leg is bench.py's timed loop -- W untimed steps, K timed steps between two synchronisations, the per-launch
events of the kernel table created before the timed region (bench.LaunchTimer.reserve), no event creation inside it.  Prints, per mode,
frames/s of every round, the per-kernel-variant milliseconds per step, and the max-abs of the mode's output against the engine's own
exact-fp32 output on the same clip; last line: one JSON record.

usage: tools/f16_fps.py [--workload c1|c5] [--steps K] [--warmup W] [--rounds R] [--frames F] [--wide-conv wino2|direct]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402

MODES = ("f16x3", "f16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c1", choices=["c1", "c5"])
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--wide-conv", default="auto")
    ap.add_argument("--modes", default=",".join(MODES), help="comma-separated subset of f16x3,f16 (one mode: a leg to set beside another build's)")
    args = ap.parse_args()
    if args.rounds < 2:
        ap.error("--rounds must be at least 2: the modes alternate")
    modes = tuple(args.modes.split(","))
    wl = bench.WORKLOADS[args.workload]
    frames = args.frames or wl["frames"]
    steps = args.steps or (30 if args.workload == "c1" else 2)
    warmup = args.warmup if args.warmup is not None else (3 if args.workload == "c1" else 1)
    dev = torch.device("cuda", 0)
    h, w, mode = wl["h"], wl["w"], wl["mode"]
    lq, nm = bench.synth_clip(frames, 100, dev, h, w)
    x = torch.cat([lq, nm], dim=2)[0].contiguous()
    models = {p: bench.build_model(dev, p, False, args.wide_conv) for p in modes + ("fp32",)}      # (same seed: the same weights)

    def make_step(m):
        if mode == "perframe":
            def per_frame():
                outs = []
                for k in range(frames + m.shift_num):
                    y = m.feedin_one_element(x[k:k + 1] if k < frames else None)
                    if y is not None:
                        outs.append(y)
                m.feedin_one_element(None)
                m.reset()
                return torch.cat(outs, dim=0)
            return per_frame
        return lambda: m.clip_forward(x)

    def kernel_table(m, step, timer, nsteps):
        if mode == "clip":
            agg = timer.summary()
        else:       # graph replays have no per-launch host call to bracket: one extra untimed pass, layer by layer (as bench.py does)
            for e in m._stream_engs.values():
                e.layerwise = True
            t = bench.LaunchTimer(m._executor(dev))
            step()
            t.reset()
            step()
            torch.cuda.synchronize()
            t.detach()
            agg, nsteps = t.summary(), 1
            for e in m._stream_engs.values():
                e.layerwise = False
        return {k: round(v["ms"] / nsteps, 4) for k, v in sorted(agg.items())}

    def leg(p):
        m = models[p]
        step = make_step(m)
        timer = bench.LaunchTimer(m._executor(dev)) if mode == "clip" else None
        for _ in range(warmup):
            if timer:
                timer.reset()
            y = step()
        if timer:
            timer.reserve(steps)
            timer.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            y = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if timer:
            timer.detach()
        return frames * steps / dt, kernel_table(m, step, timer, steps), y

    res = {p: {"fps": [], "kernels_ms_per_step": None, "max_abs_vs_fp32": None} for p in modes}
    with torch.no_grad():
        ref = make_step(models["fp32"])()
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for p in modes:
                fps, table, y = leg(p)
                res[p]["fps"].append(round(fps, 2))
                res[p]["kernels_ms_per_step"] = table
                res[p]["max_abs_vs_fp32"] = float((y - ref).abs().max())
                print("%s round %d %s: %.1f frames/s" % (args.workload, r, p, fps), flush=True)
    for p in modes:
        print("== %s: frames/s %s, max-abs vs the engine's exact fp32 %.3e (|out| max %.2f)" % (p, res[p]["fps"], res[p]["max_abs_vs_fp32"], float(ref.abs().max())))
        for k, v in res[p]["kernels_ms_per_step"].items():
            print("   %-64s %9.4f ms/step" % (k, v))
    if len(modes) == 2:
        a, b = (sum(res[p]["fps"]) / len(res[p]["fps"]) for p in modes)
        print("== %s / %s: %.3f x (mean of %d alternating rounds)" % (modes[1], modes[0], b / a, args.rounds))
    print(json.dumps({"tool": "f16_fps", "workload": args.workload, "frames": frames, "steps": steps, "warmup": warmup, "rounds": args.rounds,
                      "device": torch.cuda.get_device_name(dev), "lib": os.environ.get("BSVD_HIP_LIB", "in-tree"), "modes": res}))


if __name__ == "__main__":
    main()
