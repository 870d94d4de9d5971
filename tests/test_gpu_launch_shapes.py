"""The frame I/O kernels at capped grids: every launch here runs its grid-stride loop more than twice and ends in a ragged trip, by the
restatement of the launch rules in tests/launch_shapes.py (which also says why the shapes are what they are).  Each case holds the whole
result to the numpy model its format's small-shape test uses, by that test's rule (bit for bit; 1e-6 of the float64 truth for the YUV
decoders; finish_model.mismatches with its tie rule for the YUV encoders), then asks for the same bytes from calls on chunks of frames that
are each a single trip (launch-shape independence, no allowance), and runs in tests/arena.py arenas pre-filled with 0x00 and with 0xFF."""
import ctypes
import time

import numpy as np
import pytest
import torch

import arena
import finish_model as F
import launch_shapes as L
import rgb_surface_model as R
import scene_model as SC
import yuv_model as M
import yuv_surface_model as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _libs():
    from bsvd_amd import _lib
    from bsvd_amd.engine import require_hip
    return _lib, require_hip()


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)          # the shared inputs are read-only arrays


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    """bit equality of two device tensors of one dtype"""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has reported one"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                             # noqa: BLE001
        pytest.exit("device error, stopping: %s" % e, returncode=3)


# ---- the sweep kernels -----------------------------------------------------------------------------------------------------------------------
def _inputs(c):
    """name -> device tensor of all T frames (frame-major, contiguous)"""
    if c.entry == "u8_in":
        return {"src": _dev(L.u8_source_of(c))}
    if c.entry == "yuv_in":
        return {"src": _dev(L.yuv_surface_of(c))}
    if c.entry == "rgb_in":
        return {"src": _dev(L.rgb_surface_of(c))}
    if c.entry == "blend":
        return {"src": _dev(L.values(c.T, c.Hp, c.Wp)), "x": _dev(L.values(c.T, c.Hp, c.Wp, 4))}
    d = {"src": _dev(L.values(c.T, c.Hp, c.Wp))}
    a = L.alpha_of(c) if c.entry == "rgb_out" else None
    if a is not None:
        d["alpha"] = _dev(a.view(np.uint8).reshape(c.T, c.H, -1))
    return d


def _out_shape(c, n):
    """(shape, dtype) of the logical output of n frames"""
    if c.entry in ("u8_in", "yuv_in", "rgb_in"):
        return (n, 4, c.Hp, c.Wp), torch.float32
    if c.entry == "u8_out":
        return ((n, c.H, c.W, 3) if c.hwc else (n, 3, c.H, c.W)), torch.uint8
    lay = L.layout_yuv(c) if c.entry == "yuv_out" else L.layout_rgb(c)
    return (n, lay["stride"]), torch.uint8


def _frame_bytes(shape, dtype):
    return int(np.prod(shape[1:])) * (4 if dtype == torch.float32 else 1)


def _launch(c, inp, lo, hi, dst, alpha_dst=None):
    """the case's entry point on frames [lo, hi) of its inputs, writing at device address ``dst``"""
    from bsvd_amd import frame_io as fio
    _lib, lib = _libs()
    n, src = hi - lo, inp["src"][lo:hi].data_ptr()
    H, W, Hp, Wp = c.H, c.W, c.Hp, c.Wp
    dith = fio._dither_struct(c.dither, L.SEED, L.FRAME0 + lo) if c.dither else None
    if c.entry == "u8_in":
        rc = (lib.bsvd_u8_to_planar_pad(src, dst, n, 3, H, W, Hp, Wp, int(c.hwc), 1, L.SIGMA, None) if c.pad
              else lib.bsvd_u8_to_planar(src, dst, n, 3, H, W, int(c.hwc), 1, L.SIGMA, None))
    elif c.entry == "u8_out":
        rev = int(c.chroma == "linear")
        rc = (lib.bsvd_planar_to_u8_crop(src, dst, n, 3, Hp, Wp, H, W, int(c.hwc), rev, None) if c.pad
              else lib.bsvd_planar_to_u8(src, dst, n, 3, H, W, int(c.hwc), rev, None))
    elif c.entry in ("yuv_in", "yuv_out"):
        lay = L.layout_yuv(c)
        semi = c.fmt in M.BITS
        if semi:
            s, _ = fio._yuv_desc(H, W, c.fmt, c.matrix, c.full_range, c.chroma, lay["row_pitch"], picture=c.pad)
        else:
            s, _ = fio._yuv_surface(H, W, c.fmt, c.matrix, c.full_range, c.chroma, lay["pitches"], lay["offsets"], picture=c.pad)
        s.frame_stride = lay["stride"]
        name = "bsvd_yuv420_to_planar" if semi else "bsvd_yuv_to_planar"
        back = "bsvd_planar_to_yuv420" if semi else "bsvd_planar_to_yuv"
        if c.entry == "yuv_in":
            rc = (getattr(lib, name + "_pad")(src, dst, n, H, W, Hp, Wp, ctypes.byref(s), 1, L.SIGMA, None) if c.pad
                  else getattr(lib, name)(src, dst, n, H, W, ctypes.byref(s), 1, L.SIGMA, None))
        elif dith is not None:
            rc = getattr(lib, back + "_crop_d")(src, dst, n, Hp, Wp, H, W, ctypes.byref(s), ctypes.byref(dith), None)
        elif c.pad:
            rc = getattr(lib, back + "_crop")(src, dst, n, Hp, Wp, H, W, ctypes.byref(s), None)
        else:
            rc = getattr(lib, back)(src, dst, n, H, W, ctypes.byref(s), None)
    elif c.entry in ("rgb_in", "rgb_out"):
        lay = L.layout_rgb(c)
        s, _ = fio._rgb_surface(H, W, c.fmt, c.full_range, lay["pitches"], lay["offsets"], picture=True)
        s.frame_stride = lay["stride"]
        if c.entry == "rgb_in":
            rc = lib.bsvd_rgb_to_planar(src, dst, n, H, W, Hp, Wp, ctypes.byref(s), alpha_dst, 1, L.SIGMA, None)
        else:
            al = inp["alpha"][lo:hi].data_ptr() if "alpha" in inp else None
            rc = (lib.bsvd_planar_to_rgb_d(src, dst, n, Hp, Wp, H, W, ctypes.byref(s), al, ctypes.byref(dith), None) if dith is not None
                  else lib.bsvd_planar_to_rgb(src, dst, n, Hp, Wp, H, W, ctypes.byref(s), al, None))
    else:
        raise AssertionError(c.entry)
    _lib.check(rc, c.id)


def _alpha_arena(c, fill):
    if c.entry != "rgb_in" or not R.has_alpha(c.fmt):
        return None
    return arena.reserve((c.T, c.H, c.W * min(R.sample_bytes(c.fmt), 2)), 0, fill=fill, device=DEV, dtype=torch.uint8)


def _run_sweep(c, inp):
    """-> (logical output, alpha or None) after checks 2 and 3"""
    shape, dtype = _out_shape(c, c.T)
    fb = _frame_bytes(shape, dtype)
    keep = {k: v.clone() for k, v in inp.items()}
    runs, alphas = [], []
    for fill in (0x00, 0xFF):
        a = arena.reserve(shape, 0, fill=fill, device=DEV, dtype=dtype)
        al = _alpha_arena(c, fill)
        _launch(c, inp, 0, c.T, a.ptr, None if al is None else al.ptr)
        torch.cuda.synchronize()
        runs.append(a)
        alphas.append(al)
    assert all(_same(inp[k], keep[k]) for k in inp), "the call wrote into an input"
    assert all(r.slack_intact() for r in runs), runs[0].slack_damage()
    out = [r.logical() for r in runs]
    if c.entry in ("yuv_out", "rgb_out"):                              # non-sample bytes keep the fill, samples are the same in both
        lay = L.layout_yuv(c) if c.entry == "yuv_out" else L.layout_rgb(c)
        if c.entry == "rgb_out":
            mask = R.sample_mask(1, c.H, c.W, c.fmt, lay["pitches"], lay["offsets"], lay["stride"])[0]
        elif c.fmt in M.BITS:
            mask = M.sample_mask(1, c.H, c.W, c.fmt, lay["row_pitch"], lay["stride"])[0]
        else:
            mask = S.sample_mask(1, c.H, c.W, c.fmt, lay["pitches"], lay["offsets"], lay["stride"])[0]
        m = _dev(mask)
        assert bool((out[0][:, ~m] == 0x00).all()) and bool((out[1][:, ~m] == 0xFF).all()), "a byte that is no sample was written"
        assert torch.equal(out[0][:, m], out[1][:, m]), "a sample was not written"
        out[1][:, ~m] = 0x00
    assert _same(out[0], out[1]), "an element of the output was not written"
    if alphas[0] is not None:
        assert all(a.slack_intact() for a in alphas) and torch.equal(alphas[0].logical(), alphas[1].logical())
    # check 2: chunks of frames, each a single trip, into a third arena
    parts = L.chunks(lambda T: L.case_rule(c, T), c.T)
    assert len(parts) >= 3 and all(L.cap_fraction(L.case_rule(c, hi - lo)) <= L.CHUNK_TRIPS for lo, hi in parts)
    a = arena.reserve(shape, 0, fill=0x00, device=DEV, dtype=dtype)
    al = _alpha_arena(c, 0x00)
    for lo, hi in parts:
        _launch(c, inp, lo, hi, a.ptr + lo * fb, None if al is None else al.ptr + lo * c.H * c.W * min(R.sample_bytes(c.fmt), 2))
    torch.cuda.synchronize()
    assert a.slack_intact()
    assert _same(a.logical(), out[0]), "one call and its single-trip chunks give different bytes"
    assert al is None or torch.equal(al.logical(), alphas[0].logical())
    return out[0].cpu().numpy(), None if alphas[0] is None else alphas[0].logical().cpu().numpy()


def _check_model(c, got, alpha):
    want = L.model(c)
    if c.entry == "u8_in":
        assert np.array_equal(_bits(got), _bits(want))
    elif c.entry == "u8_out":
        assert np.array_equal(got, want)
    elif c.entry == "yuv_in":
        assert (_bits(got[:, 3]) == np.float32(L.SIGMA).view(np.uint32)).all()
        worst = max(float(np.abs(got[a:a + 128, :3].astype(np.float64) - want[a:a + 128]).max()) for a in range(0, c.T, 128))
        print("%s: max-abs vs the float64 model %.3e" % (c.id, worst))
        assert worst <= 1e-6, worst
        for m in range(c.Hp - c.H):                                    # a pad element holds the bits of its mirror source
            assert np.array_equal(_bits(got[..., c.H + m, :]), _bits(got[..., c.H - 2 - m, :])), ("row", m)
        for m in range(c.Wp - c.W):
            assert np.array_equal(_bits(got[..., c.W + m]), _bits(got[..., c.W - 2 - m])), ("column", m)
    elif c.entry == "yuv_out":
        lay = L.layout_yuv(c)
        codes, ties = want
        near, total = sum(int(t.sum()) for t in ties), sum(t.size for t in ties)
        assert near <= 0.01 * total
        if c.fmt in M.BITS:
            planes = M.unpack(got, c.H, c.W, c.fmt, lay["row_pitch"])[:3]
        else:
            planes = S.unpack(got, c.H, c.W, c.fmt, lay["pitches"], lay["offsets"])
            assert planes[3] == 0, "ignored bits of a 10-bit word are not zero"
            planes = planes[:3]
        bad = F.mismatches(planes, codes, ties)
        print("%s: %d of %d samples at a near-tie, %d mismatches" % (c.id, near, total, bad))
        assert bad == 0, bad
    elif c.entry == "rgb_in":
        x, a = want
        assert not np.isnan(got).any() and np.array_equal(_bits(got), _bits(x))
        if a is not None:
            assert np.array_equal(alpha.reshape(c.T, c.H, -1).view(R.container(c.fmt)).reshape(c.T, c.H, c.W), a)
    elif c.entry == "rgb_out":
        lay = L.layout_rgb(c)
        mask = R.sample_mask(1, c.H, c.W, c.fmt, lay["pitches"], lay["offsets"], lay["stride"])[0]
        assert np.array_equal(got[:, mask], want[:, mask])


@pytest.mark.parametrize("c", [c for c in L.SWEEP_CASES if c.entry != "blend"], ids=lambda c: c.id)
def test_sweep_kernel_at_a_capped_grid(c):
    l = L.case_rule(c)
    assert L.qualifies(l) and max(L.case_bytes(c).values()) < L.GIB
    t0 = time.time()
    got, alpha = _run_sweep(c, _inputs(c))
    t1 = time.time()
    _check_model(c, got, alpha)
    print("%s: T x H x W = %d x %d x %d (%d x %d), items %d, trips %.3f, tail %d, device part %.2f s, model part %.2f s"
          % (c.id, c.T, c.H, c.W, c.Hp, c.Wp, l.items, L.trips(l), L.tail(l), t1 - t0, time.time() - t1))


@pytest.mark.parametrize("c", [c for c in L.SWEEP_CASES if c.entry == "blend"], ids=lambda c: c.id)
def test_blend_at_a_capped_grid(c):
    """bsvd_blend_planar is in place: y lives in an arena with slack between its frames, x in another; bit for bit the model, the same
    bits from single-trip chunks, and the ends exact: (1, 1) leaves y's bits, (0, 0) gives x's"""
    from bsvd_amd import frame_io as fio
    _lib, lib = _libs()
    l = L.case_rule(c)
    assert L.qualifies(l) and max(L.case_bytes(c).values()) < L.GIB
    y0, x0 = L.values(c.T, c.Hp, c.Wp), L.values(c.T, c.Hp, c.Wp, 4)
    w = fio._luma_weights(c.matrix)
    sl, sc = c.strength
    _, yfs, ya = arena.place(_dev(y0), 20)
    _, xfs, xa = arena.place(_dev(x0), 12)
    _lib.check(lib.bsvd_blend_planar(ya.ptr, yfs, xa.ptr, xfs, c.T, c.Hp, c.Wp, sl, sc, w, None), c.id)
    torch.cuda.synchronize()
    assert ya.slack_intact() and xa.slack_intact() and _same(xa.logical(), _dev(x0))
    whole = ya.logical()
    y = _dev(y0)
    x = _dev(x0)
    parts = L.chunks(lambda T: L.case_rule(c, T), c.T)
    assert len(parts) >= 3
    for lo, hi in parts:
        fio.blend_output(y[lo:hi], x[lo:hi], c.strength, matrix=c.matrix)
    assert _same(y, whole), "one call and its single-trip chunks give different bits"
    got = whole.cpu().numpy()
    want = L.model(c)
    bad = np.argwhere(_bits(got) != _bits(want))
    where = tuple(bad[0]) if len(bad) else None
    assert not np.isnan(got).any() and not len(bad), (len(bad), where, got[where], want[where], y0[where[0], :, where[2], where[3]],
                                                      x0[where[0], :3, where[2], where[3]])
    if c.strength == (1.0, 1.0):
        assert np.array_equal(_bits(got), _bits(y0))
    if c.strength == (0.0, 0.0):
        assert np.array_equal(_bits(got), _bits(x0[:, :3]))
    print("%s: T x Hp x Wp = %d x %d x %d, items %d, trips %.3f, tail %d" % (c.id, c.T, c.Hp, c.Wp, l.items, L.trips(l), L.tail(l)))


# ---- bsvd_scene_diff on synthetic grids ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("blocks", L.SCENE_DIFF_BLOCKS)
def test_scene_diff_on_synthetic_grids(blocks, with_prev):
    """three frames of `blocks` sums: random values with 0 and 261120 (= L_MAX x 256) side by side, against int64 numpy; the sad buffer
    holds garbage before the call"""
    _lib, lib = _libs()
    top = SC.L_MAX * 256
    rs = np.random.default_rng(blocks)
    g = rs.integers(0, top + 1, (3, blocks)).astype(np.int32)
    g[0, ::2], g[0, 1::2] = 0, top
    g[1, ::2], g[1, 1::2] = top, 0
    g[2, -70:] = np.where(np.arange(70) % 3 == 0, top, 0)
    prev = rs.integers(0, top + 1, blocks).astype(np.int32)
    prev[-3:] = (top, 0, top)
    want = SC.sad(g.astype(np.int64).reshape(3, 1, blocks), prev.astype(np.int64).reshape(1, blocks) if with_prev else None)
    gd, pd = _dev(g), _dev(prev)
    sad = torch.full((3,), -0x0123456789abcdef, dtype=torch.int64, device=DEV)
    _lib.check(lib.bsvd_scene_diff(gd.data_ptr(), pd.data_ptr() if with_prev else None, 3, blocks, sad.data_ptr(), None), "bsvd_scene_diff")
    assert np.array_equal(sad.cpu().numpy(), want), (sad.cpu().numpy(), want)
    assert torch.equal(gd, _dev(g)) and torch.equal(pd, _dev(prev))
    l = L.rule_scene_diff(blocks)
    print("scene_diff: blocks %d, trips %.3f, tail %d" % (blocks, L.trips(l), L.tail(l)))


# ---- the kernels whose blockIdx.y is the frame -----------------------------------------------------------------------------------------------
def _frames(fc):
    """-> (pool numpy, index numpy, x device tensor [T, C, Hp, Wp])"""
    pool, index = L.frame_input(fc)
    return pool, index, _dev(pool)[_dev(index)].contiguous()


def _parts(fc):
    """the chunks of check 2: at least three calls, each at most half a trip at its own cap"""
    parts = L.chunks(lambda T: L.frame_rule(fc, T), fc.T)
    assert len(parts) >= 3 and parts[0][0] == 0 and parts[-1][1] == fc.T and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    assert all(L.cap_fraction(L.frame_rule(fc, hi - lo)) <= L.CHUNK_TRIPS for lo, hi in parts)
    return parts


def _report(fc):
    l = L.frame_rule(fc)
    print("%s: T = %d, %d x %d (%d x %d), items %d, cap %s, trips %.3f, tail %d" % (fc.id, fc.T, fc.H, fc.W, fc.Hp, fc.Wp, l.items, l.cap, L.trips(l), L.tail(l)))


def _i32(pair):
    return pair[0], pair[1].view(torch.int32)


def _cases(kernel):
    return [fc for fc in L.FRAME_CASES if fc.kernel == kernel]


@pytest.mark.parametrize("fc", _cases("sigma_hist") + _cases("nlf_hist"), ids=lambda fc: fc.id)
def test_histogram_kernels(fc):
    from bsvd_amd import frame_io as fio
    pool, index, x = _frames(fc)
    pic = L.frame_picture(fc)
    keep = x.clone()
    if fc.kernel == "sigma_hist":
        fn = lambda t: _i32(fio.estimate_sigma(t, picture=pic, return_hist=True))
    else:
        fn = lambda t: _i32(fio.estimate_noise_curve(t, picture=pic, return_hist=True))
    want, hist = L.frame_model(fc)
    got, gh = fn(x)
    assert _same(x, keep)
    assert np.array_equal(gh.cpu().numpy().astype(np.int64), hist), "histogram"
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    parts = _parts(fc)
    assert len(parts) >= 3 and all(L.cap_fraction(L.frame_rule(fc, hi - lo)) <= L.CHUNK_TRIPS for lo, hi in parts)
    outs = [fn(x[lo:hi]) for lo, hi in parts]
    assert _same(torch.cat([o[0] for o in outs]), got) and _same(torch.cat([o[1] for o in outs]), gh), "chunks of frames give other bits"
    _report(fc)


def _in_place(fc, x, call, planes):
    """``call(ptr, frame_stride, T, lo)`` on x inside an arena with slack between the frames -> the logical tensor; and, through ``planes``
    (the written planes), the check that they do not depend on what they held"""
    outs = []
    for fill in (0.0, float("nan")):
        t = x.clone()
        t[:, planes] = fill
        _, fs, a = arena.place(t, 20)
        call(a.ptr, fs, fc.T, 0)
        torch.cuda.synchronize()
        assert a.slack_intact(), a.slack_damage()
        outs.append(a.logical())
    assert _same(outs[0][:, planes], outs[1][:, planes]), "an element of the written plane was not written"
    return outs[0]


@pytest.mark.parametrize("fc", _cases("fill_sigma") + _cases("nlf_map"), ids=lambda fc: fc.id)
def test_fill_kernels(fc):
    from bsvd_amd import frame_io as fio
    _lib, lib = _libs()
    pool, index, x = _frames(fc)
    last = fc.C - 1
    if fc.kernel == "fill_sigma":
        v = _dev(L.sigma_values(fc))
        call = lambda ptr, fs, T, lo: _lib.check(lib.bsvd_fill_sigma_plane(ptr, T, last, fc.Hp, fc.Wp, fs, v[lo:].data_ptr(), None), fc.id)
        fn = fio.fill_sigma_plane
    else:
        v = _dev(L.curve_pool()[L.set_index(fc)])
        call = lambda ptr, fs, T, lo: _lib.check(lib.bsvd_fill_nlf_plane(ptr, T, last, fc.Hp, fc.Wp, fs, v[lo:].data_ptr(), None), fc.id)
        fn = fio.fill_noise_map
    want = L.frame_model(fc)
    got = _in_place(fc, x, call, [last])
    assert _same(got[:, :last], x[:, :last]), "a plane that is only read was written"
    assert np.array_equal(_bits(got[:, last].cpu().numpy()), _bits(np.ascontiguousarray(want)))
    parts = _parts(fc)
    t = x.clone()
    for lo, hi in parts:
        fn(t[lo:hi], v[lo:hi])
    assert _same(t, got), "chunks of frames give other bits"
    _report(fc)


# (65535 table sets are 0.5 GiB of tables for one float per plane: at that frame count the shared set is the case)
@pytest.mark.parametrize("fc,per_frame_tables", [(fc, p) for fc in _cases("vst_forward") + _cases("vst_inverse") for p in (False, True)
                                                 if not (p and fc.regime == "max_frames")], ids=lambda v: v.id if hasattr(v, "id") else "sets" if v else "shared")
def test_vst_kernels(fc, per_frame_tables):
    from bsvd_amd import frame_io as fio
    _lib, lib = _libs()
    pool, index, x = _frames(fc)
    tp = L.table_pool()
    tables = _dev(tp[L.set_index(fc)] if per_frame_tables else tp[1:2])
    stride = 1 if per_frame_tables else 0
    want = L.frame_model(fc, per_frame=per_frame_tables)
    forward = fc.kernel == "vst_forward"
    fills = (True, False) if forward else (None,)
    for fill in fills:
        if forward:
            call = lambda ptr, fs, T, lo: _lib.check(lib.bsvd_vst_forward(ptr, T, fc.Hp, fc.Wp, fs, fc.C - 1 if fill else -1,
                                                                          tables[lo * stride:].data_ptr(), stride, None), fc.id)
            fn = lambda t, tb: fio.vst_forward(t, tb, fill_plane=fill)
        else:
            call = lambda ptr, fs, T, lo: _lib.check(lib.bsvd_vst_inverse(ptr, fs, T, fc.Hp, fc.Wp, tables[lo * stride:].data_ptr(), stride, None), fc.id)
            fn = fio.vst_inverse
        outs = []
        for f in (0x00, 0xFF):
            _, fs, a = arena.place(x, 20, fill=f)
            call(a.ptr, fs, fc.T, 0)
            torch.cuda.synchronize()
            assert a.slack_intact(), a.slack_damage()
            outs.append(a.logical())
        assert _same(outs[0], outs[1])
        got = outs[0]
        assert np.array_equal(_bits(got[:, :3].cpu().numpy()), _bits(want)), (fc.id, fill)
        if fill:
            assert np.array_equal(_bits(got[:, 3].cpu().numpy()), _bits(L.vst_sigma_plane(fc, per_frame_tables)))
        elif fc.C > 3:
            assert _same(got[:, 3:], x[:, 3:]), "fill_plane off: the fourth plane was written"
        t = x.clone()
        for lo, hi in _parts(fc):
            fn(t[lo:hi], tables[lo:hi] if per_frame_tables else tables)
        assert _same(t, got), "chunks of frames give other bits"
    _report(fc)


@pytest.mark.parametrize("fc", _cases("scene"), ids=lambda fc: fc.id)
def test_scene_scores(fc):
    from bsvd_amd import frame_io as fio
    pool, index, x = _frames(fc)
    pic = L.frame_picture(fc)
    keep = x.clone()
    sad, grid = fio.scene_scores(x, picture=pic)
    assert _same(x, keep)
    want, want_sad = L.frame_model(fc)
    assert np.array_equal(grid.cpu().numpy().astype(np.int64), want.reshape(grid.shape))
    assert np.array_equal(sad.cpu().numpy(), want_sad)
    sads, grids, prev = [], [], None
    for lo, hi in _parts(fc):
        s, g = fio.scene_scores(x[lo:hi], picture=pic, prev=prev)
        sads.append(s)
        grids.append(g)
        prev = g[-1].contiguous()
    assert _same(torch.cat(grids), grid) and _same(torch.cat(sads), sad), "chunks of frames give other sums"
    _report(fc)
