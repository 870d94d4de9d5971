"""Arenas for address tests: every tensor a kernel sees lives inside a larger byte-filled buffer that the TEST owns, so a wrong address lands
in memory the test inspects instead of in allocator slack nobody looks at (include/bsvd_hip.h, Conventions: strides are the caller's).

Pure torch, CPU and GPU.  A buffer is [guard | frame 0 | slack | frame 1 | slack | ... | guard] with every byte outside the logical elements
equal to ``fill``.  0xFF bytes are NaN as fp32 and NaN in both fp16 halves of a split16 word: an outside value that reaches a result shows
as NaN, an outside store shows in ``slack_intact()``, and a logical element the kernel never writes shows as a difference between a run on a
0x00 pre-filled and a run on a 0xFF pre-filled output arena."""
import ctypes

import torch

ALIGN = 64          # bytes: the base of frame 0 keeps the alignment of the allocation (vector paths need 16)


def _contig_strides(shape):
    st, n = [], 1
    for d in reversed(shape):
        st.append(n)
        n *= int(d)
    return tuple(reversed(st))


class Arena:
    """One strided logical tensor (``size`` / ``stride`` / ``offset`` in elements of ``dtype``) inside a byte buffer filled with ``fill``."""

    def __init__(self, size, stride, offset, nelem, fill, device, dtype=torch.float32):
        self.size, self.stride, self.offset = tuple(int(s) for s in size), tuple(int(s) for s in stride), int(offset)
        self.fill, self.dtype = int(fill), dtype
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((int(nelem) * self.itemsize,), self.fill, dtype=torch.uint8, device=device)
        self.owned = torch.zeros(int(nelem), dtype=torch.bool, device=device)         # True = a logical element
        self.owned.as_strided(self.size, self.stride, self.offset).fill_(True)
        assert int(self.owned.sum()) == self._numel(), "logical elements overlap"
        self.frame_stride = self.stride[0]
        self.pstride = self.coff = None

    def _numel(self):
        n = 1
        for s in self.size:
            n *= s
        return n

    def typed(self):
        return self.buf.view(self.dtype)

    def view(self):
        """the logical tensor, as a view into the arena"""
        return self.typed().as_strided(self.size, self.stride, self.offset)

    def logical(self):
        """the logical tensor back out of the arena (a contiguous copy)"""
        return self.view().clone()

    def write(self, t):
        self.view().copy_(t.to(self.buf.device))
        return self

    @property
    def ptr(self):
        """address of logical element 0"""
        return self.buf.data_ptr() + self.offset * self.itemsize

    @property
    def hold_ptr(self):
        """place_pixels: address of channel 0 of the HOLDING tensor's pixel 0 (what halo_* takes; the logical slice starts ``coff`` further)"""
        return self.ptr - (self.coff or 0) * self.itemsize

    def slack_intact(self):
        """True if every byte outside the logical elements still equals the fill"""
        same = (self.buf.view(-1, self.itemsize) == self.fill).all(dim=1)
        return bool((same | self.owned).all())

    def slack_damage(self):
        """element indices (relative to logical element 0) of damaged slack, for a failure message"""
        same = (self.buf.view(-1, self.itemsize) == self.fill).all(dim=1)
        bad = (~(same | self.owned)).nonzero().flatten()
        return [int(i) - self.offset for i in bad[:8]], int(bad.numel())


def _guard(frame_stride, guard_frames, itemsize):
    g = max(1, int(guard_frames)) * int(frame_stride)
    q = ALIGN // itemsize
    return (g + q - 1) // q * q


def reserve(shape, frame_slack, guard_frames=1, fill=0xFF, device="cpu", dtype=torch.float32):
    """An arena for a [T, ...] tensor whose logical elements hold the fill too (an output): guard of at least one frame stride, T frames
    ``tight + frame_slack`` elements apart (slack behind the last one as well), the same guard again."""
    shape = tuple(int(s) for s in shape)
    inner = _contig_strides(shape[1:])
    tight = 1
    for s in shape[1:]:
        tight *= s
    fs = tight + int(frame_slack)
    itemsize = torch.empty((), dtype=dtype).element_size()
    g = _guard(fs, guard_frames, itemsize)
    return Arena(shape, (fs,) + inner, g, g + shape[0] * fs + g, fill, device, dtype)


def place(t, frame_slack, guard_frames=1, fill=0xFF):
    """Copies a [T, ...] tensor into a fresh arena; returns (pointer of frame 0, frame stride in elements, handle)."""
    a = reserve(t.shape, frame_slack, guard_frames, fill, t.device, t.dtype).write(t)
    return a.ptr, a.frame_stride, a


def reserve_pixels(shape, pstride, coff, fill=0xFF, frame_slack=0, device="cpu", dtype=torch.float32):
    """An arena for a per-pixel strided tensor [H, W, C] or [T, H, W, C]: the C logical channels sit at [coff, coff + C) of a
    ``pstride``-channel holding tensor, every other channel holds the fill; frames (if any) H * W * pstride + frame_slack apart."""
    shape = tuple(int(s) for s in shape)
    C = shape[-1]
    assert 0 <= coff and coff + C <= pstride
    lead = shape[:-1]
    if len(shape) == 4:
        fs = shape[1] * shape[2] * pstride + int(frame_slack)
        stride = (fs, shape[2] * pstride, pstride, 1)
        n = shape[0] * fs
    else:
        npix = 1
        for s in lead:
            npix *= s
        fs = npix * pstride + int(frame_slack)
        stride = tuple(s * pstride for s in _contig_strides(lead)) + (1,)
        n = fs
    itemsize = torch.empty((), dtype=dtype).element_size()
    g = _guard(fs, 1, itemsize)
    a = Arena(shape, stride, g + coff, g + n + g, fill, device, dtype)
    a.frame_stride, a.pstride, a.coff = fs, int(pstride), int(coff)
    return a


def place_pixels(t, pstride, coff, fill=0xFF, frame_slack=0):
    """Copies a per-pixel tensor into a fresh holding tensor (see reserve_pixels); returns (pointer of the holding tensor, pstride, coff, handle)."""
    a = reserve_pixels(t.shape, pstride, coff, fill, frame_slack, t.device, t.dtype).write(t)
    return a.hold_ptr, a.pstride, a.coff, a


def copy_args(args):
    """a bitwise copy of a ctypes struct (BsvdConvArgs)"""
    b = type(args)()
    ctypes.memmove(ctypes.byref(b), ctypes.byref(args), ctypes.sizeof(args))
    return b


def halo_slice(t, pstride, coff, n):
    """the logical [pixels, n] slice of a halo given as (holding tensor, pstride, coff)"""
    flat = t.reshape(-1)
    return torch.as_strided(flat, (flat.numel() // pstride, n), (pstride, 1), flat.storage_offset() + coff).clone()


def rehome(args, x, y_shape, extra=None, halo_prev=None, halo_next=None, *, x_slack=20, y_slack=20, y_fill=0xFF, extra_slack=20,
           extra_pstride=None, halo_n=None, halo_layout=None, fill=0xFF):
    """A copy of filled BsvdConvArgs (HipExecutor.build_args) whose x, y, extra, halo_prev and halo_next -- with their stride fields -- point into
    arenas; returns (args, {name: handle}).

    x / extra / halo_*: the tensors of the tight launch (a halo as (tensor, pstride, coff)); y_shape: shape of the tight output ([T, ...];
    planar, NHWC or [T, frame elems] of a transformed tensor alike).  extra keeps args' (pstride, cstride) unless ``extra_pstride`` widens a
    cstride-1 tensor: its logical channels are then the first ``extra.shape[-1]`` of a holding tensor.  ``halo_layout``:
      None       keeps each halo's own holding tensor (moved as a whole);
      "frame"    puts a full neighbour frame behind 16 foreign channels (coff + 16);
      "wide"     puts the ``halo_n``-channel slices into Cin + 16 channel holding tensors at coff 16 + fold (prev) / 16 (next);
      "compact"  puts them into halo_n + 16 channel ones at coff 16."""
    b = copy_args(args)
    h = {}
    b.x, b.x_frame_stride, h["x"] = place(x, x_slack, fill=fill)
    h["y"] = reserve(y_shape, y_slack, fill=y_fill, device=x.device)
    b.y, b.y_frame_stride = h["y"].ptr, h["y"].frame_stride
    if extra is not None:
        if extra_pstride is not None:
            assert args.extra_cstride == 1
            a = reserve_pixels(extra.shape, extra_pstride, 0, fill, extra_slack, extra.device).write(extra)
            b.extra, b.extra_frame_stride, b.extra_pstride = a.ptr, a.frame_stride, extra_pstride
            h["extra"] = a
        else:
            b.extra, b.extra_frame_stride, h["extra"] = place(extra, extra_slack, fill=fill)
    for name, halo, wide_coff in (("halo_prev", halo_prev, 16 + args.fold), ("halo_next", halo_next, 16)):
        if halo is None:
            continue
        t, ps, co = halo
        if halo_layout is None:
            ptr, _, a = place(t.reshape(1, -1), 0, fill=fill)
        elif halo_layout == "frame":        # a full neighbour frame (pstride == Cin) behind 16 foreign channels
            assert ps == args.Cin
            ptr, ps, _, a = place_pixels(t.reshape(tuple(x.shape[-3:-1]) + (ps,)), ps + 16, 16, fill)
            co += 16
        else:
            sl = halo_slice(t, ps, co, halo_n).reshape(tuple(x.shape[-3:-1]) + (halo_n,))
            ps, co = (args.Cin + 16, wide_coff) if halo_layout == "wide" else (halo_n + 16, 16)
            ptr, _, _, a = place_pixels(sl, ps, co, fill)
        setattr(b, name, ptr)
        setattr(b, name + "_pstride", ps)
        setattr(b, name + "_coff", co)
        h[name] = a
    return b, h


def same_bits(a, b):
    """bit equality of two fp32 tensors (NaN == NaN of the same payload, +0 != -0)"""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def verdict(runs, inputs, y_tight=None, ref=None, tol=None, decode=None):
    """The checks of one re-homed case as {name: bool}.  ``runs``: the output handles of the launches on a 0x00 and on a 0xFF pre-filled
    arena; ``inputs``: the input handles; ``y_tight``: the tight launch's output (None: not comparable, e.g. another kernel instantiation);
    ``ref`` / ``tol``: a high-precision reference of the logical output and the bound on max |y - ref|; ``decode``: logical tensor -> values
    (split16 containers).
      written        both pre-fills give the same bits: every logical element of y is written
      equals_tight   each re-homed output has the tight launch's bits
      within_ref     each re-homed output is within tol of the reference
      no_nan         no outside value (all NaN) reached a result
      y_slack        no byte outside y's logical elements was written
      inputs_intact  the inputs are const"""
    outs = [r.logical() for r in runs]
    vals = [decode(o) if decode is not None else o for o in outs]
    v = {"written": all(same_bits(outs[0], o) for o in outs[1:]),
         "no_nan": not any(bool(torch.isnan(o).any()) for o in vals),
         "y_slack": all(r.slack_intact() for r in runs),
         "inputs_intact": all(i.slack_intact() for i in inputs)}
    if y_tight is not None:
        v["equals_tight"] = all(same_bits(o, y_tight.to(o.device)) for o in outs)
    if ref is not None:
        # (a NaN difference compares False: not within the bound)
        v["within_ref"] = all(bool(((o.double().cpu() - ref.double().cpu()).abs().max() < tol)) for o in vals)
    return v
