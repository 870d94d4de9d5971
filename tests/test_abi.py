"""The C-ABI shared library loads and exports every symbol include/bsvd_hip.h declares; argument
validation works without touching a device (CPU-safe: no kernel is launched)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "bsvd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(bsvd_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported():
    from bsvd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 8
    for s in syms:
        assert hasattr(lib, s), "libbsvd_hip.so does not export %s" % s
    assert sorted(_lib.EXPORTS) == syms


def test_struct_layout_matches_header():
    from bsvd_amd import _lib
    lib = _lib.load()
    assert lib.bsvd_abi_version() == _lib.ABI_VERSION
    lib.bsvd_conv_args_size.restype = ctypes.c_int
    assert lib.bsvd_conv_args_size() == ctypes.sizeof(_lib.BsvdConvArgs)


def test_argument_validation_without_device():
    from bsvd_amd import _lib
    lib = _lib.load()
    assert lib.bsvd_conv3x3(None, None) == -1
    a = _lib.BsvdConvArgs()
    a.x = a.y = a.w_packed = 16
    a.frames, a.H, a.W, a.Cin, a.Cout, a.stride = 1, 8, 8, 12, 16, 1
    assert lib.bsvd_conv3x3(ctypes.byref(a), None) == -5 and b"multiples of 16" in lib.bsvd_last_error()
    a.Cin, a.stride = 16, 3
    assert lib.bsvd_conv3x3(ctypes.byref(a), None) == -6
    a.stride, a.fold = 1, 9
    assert lib.bsvd_conv3x3(ctypes.byref(a), None) == -7
    a.fold, a.dtype = 0, 7
    assert lib.bsvd_conv3x3(ctypes.byref(a), None) == -2
    assert lib.bsvd_packed_weight_elems(16, 64) == 16 * 9 * 64
    with pytest.raises(ValueError):
        _lib.check(-5, "x")


def test_variant_dry_run_reports_dispatch():
    """bsvd_conv3x3_variant validates like bsvd_conv3x3 and names the kernel instantiation, launching nothing."""
    from bsvd_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(96)

    def variant(**kw):
        a = _lib.BsvdConvArgs()
        a.x = a.y = a.w_packed = 256
        a.frames, a.H, a.W, a.Cin, a.Cout, a.stride = 10, 270, 480, 128, 128, 1
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.bsvd_conv3x3_variant(ctypes.byref(a), buf, 96)
        return rc, buf.value.decode()

    assert variant() == (0, "conv3x3_kernel<2,2,2,2,1>[f32]")
    assert variant(fold=16) == (0, "conv3x3_kernel<2,2,2,2,1>[f32]")
    assert variant(fold=12) == (0, "conv3x3_kernel<2,2,2,2,1>[f32][generic]")
    assert variant(dtype=_lib.BSVD_F16X3) == (0, "conv3x3_kernel<4,2,2,2,1>[f16x3]")
    assert variant(dtype=_lib.BSVD_F16X3, frames=1) == (0, "conv3x3_kernel<2,2,2,2,1>[f16x3]")     # small grid: thin tiles
    assert variant(Cout=64, H=540, W=960, Cin=64) == (0, "conv3x3_kernel<2,2,4,1,1>[f32]")
    assert variant(stride=2, Cin=64) == (0, "conv3x3_kernel<2,2,2,2,2>[f32]")
    assert variant(dtype=_lib.BSVD_F16X3, fold=12)[0] == -17 and b"fold 12" in lib.bsvd_last_error()
    # the split stride-2 tile (round 6: 128 px x 32 ch wave tiles) is a plain conv: a temporal shift on it is refused, never read from the wrong frames
    assert variant(dtype=_lib.BSVD_F16X3, stride=2, Cin=64) == (0, "conv3x3_kernel<4,1,1,4,2>[f16x3]")
    assert variant(dtype=_lib.BSVD_F16X3, stride=2, Cin=64, fold=16)[0] == -17 and b"plain convs" in lib.bsvd_last_error()
    # transformed-domain tensors are options of the Winograd form
    assert variant(dtype=_lib.BSVD_F16X3, x_v=6)[0] == -22 and variant(dtype=_lib.BSVD_F16X3, y_v=6)[0] == -22
    # the Winograd launcher's dispatch (expected names: the library as it was before the launcher became one table of codes)
    def wino(m, **kw):
        kw = dict(dict(dtype=_lib.BSVD_F16X3, w_wino_packed=256, wino_m=m, H=135, W=240, Cin=256, Cout=256), **kw)
        return variant(**kw)

    vfe = lib.bsvd_v_frame_elems(135, 240, 256, 6)
    assert wino(2) == (0, "winox_kernel<F(2,3),2x2>[f16x3]")                    # 10 frames: the 16-row tile
    assert wino(6) == (0, "winox_kernel<F(6,3),1x2>[f16x3]")
    assert wino(2, frames=1) == (0, "winox_kernel<F(2,3),2x2>[f16x3]")          # one frame: the folded 16-row grid is one round (240 + 16 workgroups)
    assert wino(6, frames=1) == (0, "winox_kernel<F(6,3),1x2>[f16x3]")          # 180 workgroups of 16 rows beat 340 of 8
    assert wino(6, frames=2) == (0, "winox_kernel<F(6,3),1x2>[f16x3][8 rows]")
    assert wino(2, frames=1, Cin=128, Cout=128) == (0, "winox_kernel<F(2,3),2x2>[f16x3][8 rows]")
    assert wino(6, frames=1, Cin=128, Cout=128) == (0, "winox_kernel<F(6,3),1x2>[f16x3][8 rows]")
    assert wino(42, frames=1, Cin=128, Cout=128) == (0, "winox_kernel<F(2,3),2x2>[f16x3]")      # 42 / 46: never the half-height tile
    assert wino(46, frames=1, Cin=128, Cout=128) == (0, "winox_kernel<F(6,3),1x2>[f16x3]")
    assert wino(42, frames=1) == (0, "winox_kernel<F(2,3),2x2>[f16x3]") and wino(46, frames=1) == (0, "winox_kernel<F(6,3),1x2>[f16x3]")
    assert wino(2, x_f32=1) == (0, "winox_kernel<F(2,3),2x2>[f16x3][f32 in]")
    assert wino(6, x_f32=1) == (0, "winox_kernel<F(6,3),1x2>[f16x3][f32 in]")
    assert wino(6, x_v=6, x_frame_stride=vfe) == (0, "winox_kernel<F(6,3),1x2>[f16x3][V in]")
    assert wino(2, x_v=2, frames=1) == (0, "winox_kernel<F(2,3),2x2>[f16x3][8 rows][V in]")      # a transformed-domain input never folds
    assert wino(6, y_v=6, y_frame_stride=vfe) == (0, "winox_kernel<F(6,3),1x2>[f16x3][V out]")
    assert wino(2, y_v=2, y_frame_stride=lib.bsvd_v_frame_elems(135, 240, 256, 2))[0] == -19 and b"F(6,3) only" in lib.bsvd_last_error()
    # the measurement codes are refused by the product library, and the message says where they live
    for m in (4, 12, 22, 32, 36, 52, 62):
        assert wino(m)[0] == -19 and b"measurement" in lib.bsvd_last_error(), m
    assert wino(3)[0] == -19 and wino(14)[0] == -19
    assert lib.bsvd_v_groups(240, 6) == 40 and lib.bsvd_v_groups(214, 6) == 40 and lib.bsvd_v_groups(50, 2) == 32 and lib.bsvd_v_groups(240, 5) == -1
    assert lib.bsvd_v_frame_elems(135, 240, 256, 6) == 135 * 5 * 16 * (8 * 32 + 8) * 4 + 135 * 5 * 4 * 256 and lib.bsvd_v_frame_elems(8, 8, 24, 6) == -1
    # a frame of 2 GiB or more cannot be addressed by the split kernel: the error says so (not "fold")
    assert variant(dtype=_lib.BSVD_F16X3, frames=1, H=4320, W=7680, Cin=64, Cout=64)[0] == -17
    assert b"2 GiB" in lib.bsvd_last_error() and b"4320 x 7680" in lib.bsvd_last_error()
    assert variant(frames=1, H=4320, W=7680, Cin=64, Cout=64) == (0, "conv3x3_kernel<2,2,4,1,1>[f32][generic]")
    assert variant(Cin=12)[0] == -5


def test_last_error_is_per_thread():
    """include/bsvd_hip.h: "no global state besides a thread-local error string".  Thread A fails 1000 dry runs (bsvd_conv3x3_variant launches
    nothing), each with a message only that call can have produced, and must read back its own; thread B, whose string holds the text of
    one failure of its own, makes valid calls beside it and must never see A's text: its string stays what it was."""
    import threading
    from bsvd_amd import _lib
    lib = _lib.load()
    N = 1000
    start = threading.Barrier(2)
    stop = threading.Event()
    failures = []

    def args(**kw):
        a = _lib.BsvdConvArgs()
        a.x = a.y = a.w_packed = 256
        a.frames, a.H, a.W, a.Cin, a.Cout, a.stride = 1, 8, 8, 64, 64, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def fails():
        buf = ctypes.create_string_buffer(96)
        start.wait(timeout=30)
        for i in range(N):
            if stop.is_set():
                return
            cin = 16 * i + 1 + i % 15                      # never a multiple of 16, another number in every call
            rc = lib.bsvd_conv3x3_variant(ctypes.byref(args(Cin=cin)), buf, 96)
            msg = lib.bsvd_last_error()
            assert rc == -5 and msg == b"bsvd_conv3x3: Cin=%d / Cout=64 must be positive multiples of 16 (pad channels)" % cin, (i, rc, msg)

    def succeeds():
        buf = ctypes.create_string_buffer(96)
        assert lib.bsvd_conv3x3_variant(ctypes.byref(args(stride=3)), buf, 96) == -6
        mine = lib.bsvd_last_error()
        assert mine == b"bsvd_conv3x3: stride 3"
        ok = args()
        start.wait(timeout=30)
        for i in range(N):
            if stop.is_set():
                return
            rc = lib.bsvd_conv3x3_variant(ctypes.byref(ok), buf, 96)
            msg = lib.bsvd_last_error()
            assert rc == 0 and buf.value.startswith(b"conv3x3_kernel<") and msg == mine, (i, rc, buf.value, msg)

    def guarded(fn):
        def run():
            try:
                fn()
            except BaseException as e:         # noqa: B036 -- collected and re-raised in the main thread
                failures.append(e)
                stop.set()
                start.abort()
        return run

    assert lib.bsvd_conv3x3_variant(ctypes.byref(args(stride=5)), ctypes.create_string_buffer(96), 96) == -6
    threads = [threading.Thread(target=guarded(f)) for f in (fails, succeeds)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads)
    if failures:
        raise failures[0]
    assert lib.bsvd_last_error() == b"bsvd_conv3x3: stride 5"          # the main thread's own string: untouched by both


def test_product_has_no_cpu_fallback():
    """Without a HIP device the product must fail loudly instead of computing on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import bsvd_amd
    m = bsvd_amd.BSVD(precision="fp32", norm="none", pretrain_ckpt=None)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(1, 2, 4, 8, 8))
    with pytest.raises(RuntimeError, match="HIP device"):
        m.feedin_one_element(torch.zeros(1, 4, 8, 8))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "bsvd_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "conv_ref" not in txt, f


def test_workspace_bytes_is_zero_and_validates():
    """bsvd_workspace_bytes: 0 for valid layers (no scratch in this ABI version), the conv's own error code otherwise."""
    from bsvd_amd import _lib
    lib = _lib.load()
    a = _lib.BsvdConvArgs()
    a.x = a.y = a.w_packed = 16
    a.frames, a.H, a.W, a.Cin, a.Cout, a.stride = 2, 8, 8, 64, 64, 1
    assert lib.bsvd_workspace_bytes(ctypes.byref(a)) == 0
    a.dtype = _lib.BSVD_F16X3
    assert lib.bsvd_workspace_bytes(ctypes.byref(a)) == 0
    a.Cin = 12
    assert lib.bsvd_workspace_bytes(ctypes.byref(a)) == -5
    assert lib.bsvd_workspace_bytes(None) == -1
    assert lib.bsvd_halo_unpack(None, None, 4, 16, 0, 8, 0, None) == -3
    assert lib.bsvd_halo_unpack(16, 16, 4, 16, 12, 8, 0, None) == -3        # c0 + n > C


# ---------------------------------------------------------------------------------------------------------------------------------------
# validation replay: tests/golden/abi_replay.json holds what the conv entry answered when the fixture was recorded (tools/abi_replay_gen.py)

REPLAY = os.path.join(ROOT, "tests", "golden", "abi_replay.json")
# every negative code the conv path can answer through bsvd_conv3x3_variant, read off the source the fixture was recorded from: -1 .. -13
# and -15 .. -23 of bsvd_abi.hip, with -17 and -19 coming out of the launchers as well (-14 is the fp32 head's launch, never a dry run)
REPLAY_CODES = set(range(-23, 0)) - {-14}


def _replay_args(fx, template, overrides):
    from bsvd_amd import _lib
    if overrides.get("_null"):
        return None
    a = _lib.BsvdConvArgs()
    for k, v in dict(fx["base"], **dict(fx["templates"][template], **overrides)).items():
        if not k.startswith("_"):
            setattr(a, k, float(v) if isinstance(v, str) else v)       # floats travel as text (inf and nan are no JSON)
    return a


def test_validation_replay():
    """Return code, bsvd_last_error() text and dry-run name of every recorded BsvdConvArgs: byte for byte what the fixture holds."""
    import json
    from bsvd_amd import _lib
    lib = _lib.load()
    fx = json.load(open(REPLAY))
    assert len(fx["cases"]) >= 2000
    buf = ctypes.create_string_buffer(96)
    codes, wrong = set(), []
    for template, overrides, oi in fx["cases"]:
        rc_exp, err_exp, name_exp = fx["outcomes"][oi]
        a = _replay_args(fx, template, overrides)
        name_len = overrides.get("_name_len", 96)
        buf.value = b"?"
        rc = lib.bsvd_conv3x3_variant(ctypes.byref(a) if a is not None else None, buf, name_len)
        got = [rc, lib.bsvd_last_error().decode() if rc < 0 else "", buf.value.decode() if name_len >= 8 else ""]
        if got != [rc_exp, err_exp, name_exp]:
            wrong.append((template, overrides, got, fx["outcomes"][oi]))
        codes.add(rc_exp)
    assert not wrong, "%d of %d cases differ, first: %r" % (len(wrong), len(fx["cases"]), wrong[:3])
    assert {c for c in codes if c < 0} == REPLAY_CODES and 0 in codes
    launcher = {(o[0], o[1].split(":")[1].strip()[:12]) for o in fx["outcomes"] if o[0] in (-17, -19)}
    assert (-17, "BSVD_F16X3 n") in launcher and (-19, "y_v is not a") in launcher      # ... and the launchers' own refusals are among them


@pytest.mark.gpu
def test_batch_replay_names_the_failing_layer():
    """bsvd_conv3x3_batch with a bad second element: the first one is launched (on real tensors), the message names layer 1 of 2."""
    import json
    import torch
    from bsvd_amd import _lib
    lib = _lib.load()
    fx = json.load(open(REPLAY))
    rec = fx["batch"]
    x, w, y = (torch.zeros(n, device="cuda") for n in (8 * 8 * 16, 16 * 9 * 16, 8 * 8 * 16))
    arr = (_lib.BsvdConvArgs * 2)()
    for a, ov in zip(arr, rec["args"]):
        for k, v in dict(fx["base"], **ov).items():
            setattr(a, k, v)
        a.x, a.w_packed, a.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    rc = lib.bsvd_conv3x3_batch(arr, 2, None)
    torch.cuda.synchronize()
    assert (rc, lib.bsvd_last_error().decode()) == (rec["rc"], rec["error"])
    assert rec["rc"] < 0 and rec["error"].startswith("bsvd_conv3x3_batch: layer 1 of 2: bsvd_conv3x3: ")
