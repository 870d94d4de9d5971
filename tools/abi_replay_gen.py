#!/usr/bin/env python3
"""Records what the conv entry of libbsvd_hip.so answers to a fixed set of BsvdConvArgs: tests/golden/abi_replay.json, replayed by
tests/test_abi.py against the built library (return code, bsvd_last_error() text, dry-run kernel name: byte for byte).

usage: BSVD_HIP_LIB=<the library to record from> tools/abi_replay_gen.py [--out tests/golden/abi_replay.json]

Regenerate whenever the ABI changes ON PURPOSE, from the library that defines the new behaviour.  Everything but the batch case goes
through bsvd_conv3x3_variant, which validates and names without launching: no device needed.  The batch case (bsvd_conv3x3_batch with a bad
second element) has to launch its first element for real, so it is recorded only where a HIP device is present; without one the entry of
the existing fixture is carried over.

Cases = a hand-written table (one per set_error site of the conv path, next to the template it was derived from: its accepted
neighbour) + a seeded random product over the fields the checks read, thinned to PER_CLASS cases per outcome class (return code + text
with its numbers masked)."""
import argparse
import ctypes
import json
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bsvd_amd import _lib      # noqa: E402

F32, F16X3 = _lib.BSVD_F32, _lib.BSVD_F16X3
BIG = 1 << 26                   # a frame stride that holds any transformed frame of the shapes below
SEED, DRAWS, PER_CLASS = 20261018, 100000, 28

# fake, never dereferenced pointers: 256-byte aligned ones, +8 / +4 for the misaligned cases
BASE = dict(x=0x1000, y=0x2000, w_packed=0x3000, frames=2, H=16, W=16, Cin=64, Cout=64, stride=1)
HALO = dict(fold=16, halo_prev=0x8000, halo_prev_pstride=64, halo_next=0x9000, halo_next_pstride=64)
TEMPLATES = [
    dict(),                                                                                            # 0 direct fp32
    dict(dtype=F16X3),                                                                                 # 1 direct f16x3
    dict(dtype=F16X3, w_wino_packed=0x4000, wino_m=6),                                                 # 2 Winograd F(6,3)
    dict(dtype=F16X3, w_wino_packed=0x4000, wino_m=2),                                                 # 3 Winograd F(2,3)
    dict(dtype=F16X3, pre_w_packed=0x5000, pre_bias=0x5800, pre_cin=16),                               # 4 fused pair
    dict(dtype=F16X3, x_planar_ch=4, head_w_packed=0x6000, head_bias=0x6800),                          # 5 fused entry
    dict(x_planar_ch=3, Cin=16),                                                                       # 6 planar input, fp32 head
    dict(y_planar_ch=3, Cout=16),                                                                      # 7 planar output, fp32 tail
    dict(dtype=F16X3, y_planar_ch=3, Cout=16),                                                         # 8 planar output, f16x3
    dict(HALO),                                                                                        # 9 temporal shift, fp32
    dict(HALO, dtype=F16X3),                                                                           # 10 temporal shift, f16x3
    dict(HALO, dtype=F16X3, w_wino_packed=0x4000, wino_m=6),                                           # 11 temporal shift, Winograd
    dict(dtype=F16X3, w_wino_packed=0x4000, wino_m=6, x_v=6, y_v=6, x_frame_stride=BIG, y_frame_stride=BIG),   # 12 transformed in and out
    dict(epilogue=2, extra=0x7000, resid_ch=3),                                                        # 13 RESID
    dict(dtype=F16X3, epilogue=1, extra=0x7000, extra_cstride=1),                                      # 14 PS_ADD
    dict(dtype=F16X3, pre_w_packed=0x5000, pre_bias=0x5800, pre_cin=16, y_planar_ch=3, Cout=16),       # 15 fused pair into the exit
]

# one case per set_error site of the conv path (template, overrides); the template itself is the accepted neighbour and is replayed too
TABLE = [(t, {}) for t in range(len(TEMPLATES))] + [
    (0, {"_null": 1}), (0, {"_name_len": 4}), (0, {"_name_len": 8}),
    (0, dict(dtype=1)), (0, dict(dtype=7)),
    (0, dict(x=0)), (0, dict(y=0)), (0, dict(w_packed=0)), (0, dict(w_packed=0, w_wino_packed=0x4000)),
    (0, dict(frames=0)), (0, dict(H=0)), (0, dict(W=-1)),
    (0, dict(Cin=12)), (0, dict(Cout=0)), (0, dict(Cout=24)),
    (0, dict(stride=0)), (0, dict(stride=3)), (0, dict(stride=2)),
    (0, dict(fold=-1)), (0, dict(fold=40)), (0, dict(fold=32)),
    (0, dict(act=3)), (0, dict(act=-1)), (0, dict(act=2)),
    (0, dict(epilogue=3)), (0, dict(epilogue=-1)),
    (0, dict(epilogue=1, Cout=32)), (0, dict(epilogue=1, Cout=64)),
    (0, dict(epilogue=2)), (13, dict(resid_ch=-1)), (13, dict(resid_ch=65)), (13, dict(resid_ch=64)),
    (9, dict(halo_prev_pstride=0)), (9, dict(halo_next_pstride=-4)), (9, dict(halo_prev=0, halo_prev_pstride=0)),
    # the three scales
    (1, dict(out_scale="2.0")), (1, dict(out_scale="3.0")), (1, dict(out_scale="-2.0")), (1, dict(out_scale="inf")), (1, dict(out_scale="nan")),
    (1, dict(out_scale="1e-40")), (1, dict(out_scale="1.0")), (0, dict(out_scale="2.0")), (0, dict(out_scale="1.0")),
    (1, dict(head_out_scale="0.5")), (5, dict(head_out_scale="0.5")), (5, dict(head_out_scale="0.75")),
    (1, dict(pre_out_scale="4.0")), (4, dict(pre_out_scale="4.0")), (4, dict(pre_out_scale="nan")),
    (2, dict(out_scale="2.0")), (2, dict(out_scale="2.0", wino_m=12)), (2, dict(out_scale="2.0", wino_m=20)),
    (6, dict(dtype=F16X3, out_scale="2.0")), (5, dict(out_scale="2.0")),
    # x_v / y_v
    (1, dict(x_v=6)), (1, dict(y_v=6)), (0, dict(w_wino_packed=0x4000, wino_m=6, x_v=6)),
    (12, dict(x_v=2)), (12, dict(y_v=2)), (12, dict(wino_m=46)), (12, dict(x_f32=1)), (12, dict(y_f32=1)), (12, dict(epilogue=1)),
    (12, dict(HALO, halo_prev_pstride=24)), (12, dict(HALO, halo_next_coff=8)), (12, dict(HALO)),
    (12, dict(x_frame_stride=1024)), (12, dict(x_frame_stride=1024, frames=1)), (12, dict(y_frame_stride=1024)),
    (12, dict(H=4320, W=7680, Cin=256, Cout=256, x_frame_stride=1 << 40, y_frame_stride=1 << 40)), (12, dict(wino_m=3, x_v=3, y_v=3)), (12, dict(wino_m=2, x_v=2, y_v=2)),
    # x_f32 / y_f32
    (1, dict(x_f32=1)), (0, dict(x_f32=1)), (2, dict(x_f32=1)), (3, dict(x_f32=1)),
    (1, dict(y_f32=1)), (0, dict(y_f32=1)), (2, dict(y_f32=1)), (8, dict(y_f32=1)), (6, dict(dtype=F16X3, y_f32=1)),
    (13, dict(dtype=F16X3, y_f32=1)), (4, dict(y_f32=1)), (5, dict(y_f32=1)), (14, dict(y_f32=1)),
    (14, dict(y_f32=1, w_wino_packed=0x4000, wino_m=6)),
    # pack alignment
    (0, dict(w_packed=0x3008)), (2, dict(w_wino_packed=0x4004)),
    # Winograd form
    (2, dict(x_planar_ch=3)), (2, dict(head_w_packed=0x6000)), (2, dict(dtype=F32)), (2, dict(wino_m=4)), (2, dict(wino_m=12)), (2, dict(wino_m=3)),
    (2, dict(wino_m=0)), (2, dict(wino_m=42)), (2, dict(wino_m=46)), (2, dict(stride=2)), (2, dict(epilogue=2, extra=0x7000)), (2, dict(y_planar_ch=3)),
    (11, dict(fold=8)), (2, dict(x=0x1008)), (2, dict(x_frame_stride=6)), (11, dict(halo_prev=0x8004)), (11, dict(halo_next_coff=2)),
    (2, dict(Cout=48)), (14, dict(w_wino_packed=0x4000, wino_m=6)), (14, dict(w_wino_packed=0x4000, wino_m=6, extra_cstride=2)),
    (14, dict(w_wino_packed=0x4000, wino_m=6, extra=0, extra_cstride=2)),
    (2, dict(H=4320, W=7680, Cin=64)), (11, dict(H=2048, W=2048, halo_prev_pstride=256)), (11, dict(H=2048, W=2048, halo_next_pstride=256)),
    (2, dict(Cin=8192, Cout=8192)), (3, dict(y_v=2, y_frame_stride=BIG)), (2, dict(frames=2 ** 31 - 1, H=64, W=64)),
    # fused pair
    (4, dict(dtype=F32)), (4, dict(x_planar_ch=3)), (4, dict(head_w_packed=0x6000)), (4, dict(stride=2)), (4, dict(fold=16)), (4, dict(epilogue=1)),
    (4, dict(pre_cin=0)), (4, dict(pre_cin=24)), (4, dict(Cin=48)), (4, dict(Cin=128)), (4, dict(Cout=128)), (4, dict(Cin=32, Cout=16)),
    (4, dict(pre_act=3)), (4, dict(pre_act=-1)), (4, dict(pre_act=2)),
    (4, dict(pre_bias=0)), (4, dict(pre_w_packed=0x5008)), (4, dict(pre_bias=0x5804)), (4, dict(x=0x1008)), (4, dict(x_frame_stride=6)),
    (4, dict(H=4320, W=7680)), (4, dict(pre_cin=2 ** 24)), (4, dict(epilogue=2, extra=0x7000, resid_ch=3)),
    (15, dict(Cout=32)), (15, dict(y_planar_ch=5)), (15, dict(epilogue=2, extra=0x7000, resid_ch=4)), (15, dict(epilogue=2, extra=0x7000, resid_ch=3)),
    # planar edges, fused entry
    (6, dict(y_planar_ch=3)), (6, dict(stride=2)), (7, dict(fold=4)), (6, dict(H=32768, W=8192)), (7, dict(H=32768, W=8192)),
    (5, dict(dtype=F32)), (5, dict(x_planar_ch=5)), (5, dict(x_planar_ch=1)), (5, dict(x_planar_ch=3)), (5, dict(Cin=48)), (5, dict(Cout=128)),
    (5, dict(epilogue=2, extra=0x7000)), (5, dict(head_bias=0)), (5, dict(head_w_packed=0x6008)), (5, dict(head_bias=0x6804)),
    (5, dict(H=8192, W=8192, Cin=32, Cout=16)), (5, dict(H=4096, W=4096, Cin=32, Cout=32)), (5, dict(Cin=32, Cout=32)),
    (6, dict(Cin=32)), (6, dict(epilogue=2, extra=0x7000)), (6, dict(x_planar_ch=4)), (6, dict(x_planar_ch=5)), (6, dict(dtype=F16X3)),
    (7, dict(Cout=32)), (7, dict(epilogue=1, Cout=64)), (7, dict(epilogue=2, extra=0x7000, resid_ch=4)), (7, dict(epilogue=2, extra=0x7000, resid_ch=3)),
    (7, dict(y_planar_ch=5)), (7, dict(y_planar_ch=4)), (7, dict(y_planar_ch=1)), (8, dict(y_planar_ch=5)), (8, dict(y_planar_ch=1)),
    # the direct launcher's own refusals and names
    (1, dict(fold=12)), (1, dict(fold=8)), (1, dict(fold=8, Cout=128)), (1, dict(stride=2)), (1, dict(stride=2, fold=16)), (1, dict(x=0x1008)),
    (1, dict(x_frame_stride=6)), (10, dict(halo_prev_coff=2)), (10, dict(halo_next=0x9004)), (1, dict(H=4320, W=7680)), (1, dict(Cin=16384, Cout=16384)),
    (0, dict(fold=12)), (0, dict(fold=8)), (0, dict(x=0x1008)), (0, dict(H=4320, W=7680)), (0, dict(frames=2 ** 31 - 1, H=64, W=64)),
    (1, dict(frames=10, H=270, W=480, Cin=128, Cout=128)), (1, dict(frames=1, H=270, W=480, Cin=128, Cout=128)),
    (1, dict(frames=1, H=270, W=480, Cin=128, Cout=128, fat_min_wgs=1)), (0, dict(tile_order=1)),
]

# the random product: per field the 0 / legal values AND illegal ones
PTR = lambda p: [0, p, p + 8, p + 4]
SCALE = ["0.0", "1.0", "2.0", "0.5", "3.0", "-2.0", "inf", "nan", "1e-40"]
FIELDS = dict(
    dtype=[0, 2, 1, 7], Cin=[16, 32, 64, 128, 48, 12, 0, 96], Cout=[16, 32, 64, 128, 256, 48, 24, 0], stride=[1, 2, 0, 3],
    fold=[0, 8, 16, 32, 12, 4, -1, 40], act=[0, 1, 2, 3, -1], epilogue=[0, 1, 2, 3, -1],
    x_planar_ch=[0, 3, 4, 5, 1], y_planar_ch=[0, 1, 3, 4, 5],
    w_wino_packed=PTR(0x4000), wino_m=[0, 2, 6, 42, 46, 4, 12, 3, 14, 22], head_w_packed=PTR(0x6000), head_bias=PTR(0x6800),
    pre_w_packed=PTR(0x5000), pre_bias=PTR(0x5800), pre_cin=[0, 16, 64, 8, -16], pre_act=[0, 2, 3, -1],
    x_f32=[0, 1], y_f32=[0, 1], x_v=[0, 2, 6, 4], y_v=[0, 2, 6, 4],
    out_scale=SCALE, head_out_scale=SCALE, pre_out_scale=SCALE,
    halo_prev=PTR(0x8000), halo_next=PTR(0x9000), halo_prev_pstride=[0, 64, 16, 6, 62, -4], halo_next_pstride=[0, 64, 16, 6, 62, -4],
    halo_prev_coff=[0, 16, 4, 2], halo_next_coff=[0, 16, 4, 2],
    x=PTR(0x1000), y=[0, 0x2000], w_packed=PTR(0x3000), x_frame_stride=[0, 16384, 16386, BIG], y_frame_stride=[0, 1024, BIG],
    extra=[0, 0x7000], resid_ch=[0, 3, 4, 64, 65, -1], extra_cstride=[0, 1, 2],
    frames=[1, 2, 10, 0], H=[16, 135, 4320, 0], W=[16, 240, 7680, -1],
)


def apply(template, overrides):
    """-> (args or None, name_len) of one case"""
    if overrides.get("_null"):
        return None, 96
    a = _lib.BsvdConvArgs()
    for k, v in dict(BASE, **dict(template, **overrides)).items():
        if not k.startswith("_"):
            setattr(a, k, float(v) if isinstance(v, str) else v)
    return a, overrides.get("_name_len", 96)


def outcome(lib, buf, template, overrides):
    a, name_len = apply(template, overrides)
    rc = lib.bsvd_conv3x3_variant(ctypes.byref(a) if a is not None else None, buf, name_len)
    return [rc, lib.bsvd_last_error().decode() if rc < 0 else "", buf.value.decode() if name_len >= 8 else ""]


def record_batch(lib, previous):
    """bsvd_conv3x3_batch, a good first and a bad second element; the first one is launched, on real (zeroed) device tensors"""
    import torch
    if not torch.cuda.is_available():
        print("abi_replay_gen: no HIP device, the batch case is carried over from the existing fixture", file=sys.stderr)
        return previous
    first, second = dict(frames=1, H=8, W=8, Cin=16, Cout=16), dict(frames=1, H=8, W=8, Cin=12, Cout=16)
    x = torch.zeros(8 * 8 * 16, device="cuda")
    w, y = torch.zeros(16 * 9 * 16, device="cuda"), torch.zeros(8 * 8 * 16, device="cuda")
    arr = (_lib.BsvdConvArgs * 2)()
    for a, ov in zip(arr, (first, second)):
        for k, v in dict(BASE, **ov).items():
            setattr(a, k, v)
        a.x, a.w_packed, a.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    rc = lib.bsvd_conv3x3_batch(arr, 2, None)
    torch.cuda.synchronize()
    return dict(args=[first, second], rc=rc, error=lib.bsvd_last_error().decode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "abi_replay.json"))
    opt = ap.parse_args()
    if not os.environ.get("BSVD_HIP_LIB"):
        sys.exit("abi_replay_gen: set BSVD_HIP_LIB to the library to record from")
    lib, buf = _lib.load(), ctypes.create_string_buffer(96)
    rs = random.Random(SEED)
    draws = list(TABLE)
    names = sorted(FIELDS)
    for _ in range(DRAWS):
        ks = rs.sample(names, rs.randint(1, 5))
        draws.append((rs.randrange(len(TEMPLATES)), {k: rs.choice(FIELDS[k]) for k in ks}))
    outcomes, cases, per_class, seen = [], [], {}, set()
    for i, (t, ov) in enumerate(draws):
        key = json.dumps([t, ov], sort_keys=True)
        if key in seen:
            continue
        seen.add(key)
        out = outcome(lib, buf, TEMPLATES[t], ov)
        cls = (out[0], re.sub(r"-?\d+(\.\d+)?(e[+-]\d+)?", "#", out[1] + "|" + out[2]))
        per_class[cls] = per_class.get(cls, 0) + 1
        if i >= len(TABLE) and per_class[cls] > PER_CLASS:
            continue
        if out not in outcomes:
            outcomes.append(out)
        cases.append([t, ov, outcomes.index(out)])
    previous = json.load(open(opt.out)).get("batch") if os.path.exists(opt.out) else None
    fx = dict(base=BASE, templates=TEMPLATES, outcomes=outcomes, cases=cases, batch=record_batch(lib, previous))
    with open(opt.out, "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in fx.items()) + "\n}\n")
    codes = sorted({o[0] for o in outcomes if o[0] < 0})
    print("abi_replay_gen: %d cases (%d from the table), %d outcomes, %d classes, codes %s -> %s (%d bytes)"
          % (len(cases), len(TABLE), len(outcomes), len(per_class), codes, opt.out, os.path.getsize(opt.out)))


if __name__ == "__main__":
    main()
