"""The arena harness (tests/arena.py) catches what it claims to catch -- shown on the CPU with a plain torch conv as the "kernel".

The kernel below sees what a HIP kernel sees: flat element buffers, the offset of frame 0 and frame strides (BsvdConvArgs.x / x_frame_stride,
y / y_frame_stride).  Three deliberately wrong variants restate the three classes of address error tests/test_gpu_strides.py looks for in the
HIP kernels; each must be flagged by the matching check of arena.verdict, and the correct variant must pass all of them."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import arena

T, H, W, C = 3, 5, 7, 4          # W = 7 on a tile of 4 pixels: a ragged last tile in every row
TILE = 4


def _weights():
    g = torch.Generator().manual_seed(5)
    return torch.randn(C, C, 3, 3, generator=g) * 0.2


def conv_kernel(xbuf, x0, x_fs, ybuf, y0, y_fs, w, variant="correct"):
    """y[f] = conv3x3(x[f], w), pad 1, NHWC, on flat buffers.  Rows are produced one at a time from the three input rows around them, in tiles
    of TILE pixels with a masked last tile -- the shape of the HIP kernels' address arithmetic.
      correct   selects zero for rows outside the frame, strides by x_fs / y_fs, masks the ragged tile
      tight     strides frames by H * W * C whatever the caller's frame stride says
      mulmask   loads row -1 / row H from memory (the neighbour frame's row in a tight clip) and multiplies it by a zero mask
      overrun   the ragged tile's mask is one pixel too wide"""
    tight = H * W * C
    xs, ys = (tight, tight) if variant == "tight" else (x_fs, y_fs)
    for f in range(T):
        for r in range(H):
            rows = []
            for dy in (-1, 0, 1):
                ok = 0 <= r + dy < H
                at = x0 + f * xs + (r + dy) * W * C
                if variant == "mulmask":
                    rows.append(xbuf[at:at + W * C].reshape(W, C) * (1.0 if ok else 0.0))
                else:
                    rows.append(xbuf[at:at + W * C].reshape(W, C) if ok else torch.zeros(W, C))
            band = torch.stack(rows).permute(2, 0, 1)[None]                               # [1, C, 3, W]
            out = F.conv2d(F.pad(band.double(), (1, 1, 0, 0)), w.double()).float()[0, :, 0].t()      # [W, C]
            for t0 in range(0, W, TILE):
                n = min(TILE, W - t0) + (1 if variant == "overrun" and t0 + TILE > W else 0)
                px = torch.cat([out, out[-1:]])[t0:t0 + n]                                # the overrun stores one more pixel's worth
                at = y0 + f * ys + (r * W + t0) * C
                ybuf[at:at + n * C] = px.reshape(-1)


def _reference(x, w):
    return F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), padding=1).permute(0, 2, 3, 1).float()


def _run(variant, x, w, slack):
    _, x_fs, hx = arena.place(x, slack)
    runs = []
    for fill in (0x00, 0xFF):
        hy = arena.reserve(x.shape, slack, fill=fill)
        conv_kernel(hx.typed(), hx.offset, x_fs, hy.typed(), hy.offset, hy.frame_stride, w, variant)
        runs.append(hy)
    return runs, hx


def _tight(variant, x, w):
    y = torch.zeros(x.numel())
    conv_kernel(x.reshape(-1).clone(), 0, H * W * C, y, 0, H * W * C, w, variant)
    return y.reshape(x.shape)


@pytest.fixture(scope="module")
def operands():
    g = torch.Generator().manual_seed(6)
    x, w = torch.randn(T, H, W, C, generator=g), _weights()
    return x, w, _reference(x, w)


def test_place_logical_round_trip_and_untouched_slack():
    g = torch.Generator().manual_seed(1)
    t = torch.randn(3, 4, 5, 6, generator=g)
    for slack in (0, 5, 20):
        ptr, fs, h = arena.place(t, slack)
        assert fs == 4 * 5 * 6 + slack and ptr == h.buf.data_ptr() + h.offset * 4 and h.offset >= fs
        assert h.buf.numel() == 4 * (2 * h.offset + 3 * fs)            # a guard of >= one frame stride on both sides
        assert arena.same_bits(h.logical(), t) and h.slack_intact()
        assert torch.isnan(h.typed()[~h.owned]).all()                   # 0xFF bytes: NaN as fp32 ...
        assert torch.isnan(h.buf.view(torch.float16)[:8].float()).all()  # ... and in both fp16 halves of a word
        assert ptr % 16 == 0
    hp, ps, co, h = arena.place_pixels(t[0], 6 + 16, 16)
    assert (ps, co) == (22, 16) and h.ptr - hp == 16 * 4 and arena.same_bits(h.logical(), t[0]) and h.slack_intact()
    assert int(h.owned.sum()) == t[0].numel()
    _, _, _, h4 = arena.place_pixels(t, 10, 0, frame_slack=20)
    assert h4.frame_stride == 4 * 5 * 10 + 20 and arena.same_bits(h4.logical(), t) and h4.slack_intact()
    assert arena.same_bits(arena.halo_slice(h.typed()[h.offset - 16:h.offset - 16 + 4 * 5 * 22], 22, 16, 6).reshape(4, 5, 6), t[0])


def test_slack_intact_sees_a_single_byte_and_ignores_logical_elements():
    h = arena.reserve((2, 3, 4), 20, fill=0xFF)
    assert h.slack_intact()
    h.view().fill_(1.0)
    assert h.slack_intact()
    h.buf[4 * (h.offset + 3 * 4) + 1] = 0                      # one byte of the first slack element behind frame 0
    assert not h.slack_intact() and h.slack_damage() == ([12], 1)
    h0 = arena.reserve((2, 3, 4), 0, fill=0x00)
    h0.typed()[h0.offset - 1] = 1.0                            # the last guard element in front of frame 0
    assert not h0.slack_intact() and h0.slack_damage() == ([-1], 1)


def test_rehome_moves_every_tensor_of_a_filled_struct():
    from bsvd_amd import _lib
    a = _lib.BsvdConvArgs()
    a.Cin, a.fold, a.extra_pstride, a.extra_cstride, a.frames = 32, 4, 8, 1, 2
    x, e = torch.randn(2, 3, 5, 32), torch.randn(2, 3, 5, 8)
    full = torch.randn(3, 5, 32)
    b, h = arena.rehome(a, x, (2, 3, 5, 16), extra=e, halo_prev=(full, 32, 4), halo_next=(full, 32, 0), extra_pstride=24,
                        halo_n=4, halo_layout="wide", y_fill=0x00)
    assert a.x is None and b.x == h["x"].ptr and b.x_frame_stride == 3 * 5 * 32 + 20
    assert b.y == h["y"].ptr and b.y_frame_stride == 3 * 5 * 16 + 20 and not h["y"].buf.any()
    assert (b.extra_pstride, b.extra_cstride, b.extra_frame_stride) == (24, 1, 3 * 5 * 24 + 20) and arena.same_bits(h["extra"].logical(), e)
    assert (b.halo_prev_pstride, b.halo_prev_coff, b.halo_next_pstride, b.halo_next_coff) == (48, 20, 48, 16)
    assert b.halo_prev == h["halo_prev"].hold_ptr and arena.same_bits(h["halo_prev"].logical(), full[..., 4:8])
    assert arena.same_bits(h["halo_next"].logical(), full[..., :4])
    assert ctypes.sizeof(b) == ctypes.sizeof(a) and b.Cin == 32
    b, h = arena.rehome(a, x, (2, 3, 5, 16), halo_prev=(full, 32, 4), halo_layout="frame")
    assert (b.halo_prev_pstride, b.halo_prev_coff) == (48, 20) and arena.same_bits(h["halo_prev"].logical(), full)


@pytest.mark.parametrize("slack", [20, 5])
def test_the_correct_kernel_passes_every_check(operands, slack):
    x, w, ref = operands
    runs, hx = _run("correct", x, w, slack)
    v = arena.verdict(runs, [hx], y_tight=_tight("correct", x, w), ref=ref, tol=1e-5)
    assert v == dict(written=True, no_nan=True, y_slack=True, inputs_intact=True, equals_tight=True, within_ref=True), v


def test_a_kernel_that_strides_by_the_tight_frame_is_flagged(operands):
    """... by the comparison with the tight launch and the reference (frames 1.. are read and written at the wrong place), by the NaN it reads
    from the slack, by the stores it leaves between the frames and by the logical elements it never writes"""
    x, w, ref = operands
    assert arena.same_bits(_tight("tight", x, w), _tight("correct", x, w))          # invisible to every test on tight tensors
    runs, hx = _run("tight", x, w, 20)
    v = arena.verdict(runs, [hx], y_tight=_tight("correct", x, w), ref=ref, tol=1e-5)
    assert not v["equals_tight"] and not v["within_ref"] and not v["y_slack"] and not v["written"] and not v["no_nan"], v
    assert v["inputs_intact"]


def test_a_kernel_that_masks_a_neighbour_row_by_multiplying_with_zero_is_flagged(operands):
    """exact on finite neighbours -- the tight clip of every other test -- and NaN once the neighbour is poisoned slack"""
    x, w, ref = operands
    tight_in_a_clip = torch.zeros(T * H * W * C + 2 * W * C)
    xin = torch.zeros_like(tight_in_a_clip)
    xin[W * C:-W * C] = x.reshape(-1)                                              # finite memory on both sides of the clip
    conv_kernel(xin, W * C, H * W * C, tight_in_a_clip, W * C, H * W * C, w, "mulmask")
    assert arena.same_bits(tight_in_a_clip[W * C:-W * C].reshape(x.shape), _tight("correct", x, w))
    runs, hx = _run("mulmask", x, w, 20)
    v = arena.verdict(runs, [hx], y_tight=_tight("correct", x, w), ref=ref, tol=1e-5)
    assert not v["no_nan"], v
    assert v["written"] and v["y_slack"] and v["inputs_intact"], v                 # its addresses are right: only the value check sees it


def test_a_kernel_that_stores_one_pixel_past_a_ragged_row_is_flagged(operands):
    """inside a frame the next row's first tile overwrites the stray pixel: the result is right everywhere and only the slack shows it"""
    x, w, ref = operands
    runs, hx = _run("overrun", x, w, 20)
    v = arena.verdict(runs, [hx], y_tight=_tight("correct", x, w), ref=ref, tol=1e-5)
    assert not v["y_slack"], v
    assert v["equals_tight"] and v["within_ref"] and v["no_nan"] and v["written"] and v["inputs_intact"], v
    dmg, n = runs[0].slack_damage()
    assert n == T * C and dmg[:C] == list(range(H * W * C, H * W * C + C))          # the C channels behind every frame's last row
