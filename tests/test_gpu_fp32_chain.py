"""The exact-fp32 mode (BSVD_F32) held to what include/bsvd_hip.h says of it ("Arithmetic of BSVD_F32"): the BITS of a stated fmaf chain.

  a  every kernel family of the mode, FAST and [generic], on N(0,1) data against the CPU model of the chain (oracle/chain_ref.c through
     tests/chain_exec.py), bit for bit; the family is resolved through bsvd_conv3x3_variant and its name asserted;
  b  the exact-integer probes of tests/test_fp32_chain_cpu.py through the same families against the double-accumulating oracle, bit for bit:
     on them every summation order gives the exact result, so this part asks nothing of the order and everything of the precision;
  c  a whole c32-sized network: the clip schedule on the GPU == schedule.bsvd_clip on the chain model == the stream schedule, bit for bit.

Bits are compared as fp32 patterns with -0 mapped to +0 (chain_exec.assert_same_bits, which also refuses NaN).  What a wrong kernel would do
to these assertions is shown on the CPU by the mutation tests of tests/test_fp32_chain_cpu.py; profiles/fp32_chain_bits.txt records which
chain each family matched on the MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from chain_exec import FAMILY_CASES, ChainExecutor, assert_same_bits, operands
from helpers import bsvd_keys, load_golden
from oracle_exec import OracleExecutor
from seeded import seeded_state
from test_gpu_parity import _dev, _gpu_exec, _module

pytestmark = pytest.mark.gpu


def _unaligned(t):
    """the same contiguous tensor 4 bytes off a 16-byte boundary: the exact-fp32 mode then runs its [generic] kernel (include/bsvd_hip.h)"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    off = 1 if buf.data_ptr() % 16 == 0 else (16 - buf.data_ptr() % 16) // 4 + 1
    u = buf[off:off + t.numel()].view(t.shape)
    u.copy_(t)
    assert u.is_contiguous() and u.data_ptr() % 16 == 4
    return u


def run_case(c, sp, net, st, x, kw):
    """case ``c`` on the GPU: (result, the kernel's name); the name carries what the case declares"""
    from bsvd_amd.schedule import Halo
    ex = _gpu_exec(net, st)
    xd = x.to(_dev())
    if c.generic and not (c.tsm and sp.fold % 4):
        xd = _unaligned(xd)
    kwd = {k: (Halo(v.t.to(_dev()), v.pstride, v.coff) if isinstance(v, Halo) else v.to(_dev()) if isinstance(v, torch.Tensor) else v)
           for k, v in kw.items()}
    a, y = ex.build_args(sp, xd, **kwd)
    a.tile_order = c.tile_order
    buf = ctypes.create_string_buffer(128)
    assert ex.lib.bsvd_conv3x3_variant(ctypes.byref(a), buf, 128) == 0, ex.lib.bsvd_last_error()
    name = buf.value.decode()
    assert c.expect in name and ("[generic]" in name) == c.generic, (c.name, name)
    rc = ex.lib.bsvd_conv3x3(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, ex.lib.bsvd_last_error())
    torch.cuda.synchronize()
    return y.cpu(), name


@pytest.mark.parametrize("c", FAMILY_CASES, ids=lambda c: c.name)
def test_family_has_the_bits_of_the_documented_chain(c):
    sp, net, st, x, kw = operands(c, "normal")
    got, name = run_case(c, sp, net, st, x, kw)
    print("%s: %s, tile_order %d" % (c.name, name, c.tile_order))
    assert_same_bits(got, ChainExecutor(st).conv(sp, x, **kw), "%s on %s" % (c.name, name))


@pytest.mark.parametrize("c", FAMILY_CASES, ids=lambda c: c.name)
def test_family_is_exact_on_the_integer_probe(c):
    sp, net, st, x, kw = operands(c, "integer")
    got, name = run_case(c, sp, net, st, x, kw)
    assert_same_bits(got, OracleExecutor(st, double=True).conv(sp, x, **kw), "%s on %s" % (c.name, name))


@pytest.mark.parametrize("T,H,W,blind", [(3, 8, 12, False), (2, 20, 28, False), (3, 8, 12, True)])
def test_whole_network_has_the_bits_of_the_chain(T, H, W, blind):
    """c32-sized network, the seeded state of golden g4_bsvd_small_T3 (blind: its sibling with a 3-channel input, interm_ch 30 and ReLU, the
    project's blind configuration): clip schedule on the GPU == schedule.bsvd_clip on ChainExecutor == stream schedule."""
    from bsvd_amd.netspec import make_netspec
    from bsvd_amd.schedule import bsvd_clip
    g = load_golden("g4_bsvd_small_T3")
    interm, act, cin = (30, "relu", 3) if blind else (32, "relu6", 4)
    st = seeded_state(bsvd_keys([32, 64, 128], 32, 4, 3, interm, blind=blind), int(g["seed"]))
    x = torch.from_numpy(np.random.RandomState(T * 100 + H).standard_normal((T, cin, H, W)).astype(np.float32))
    net = make_netspec([32, 64, 128], 32, 4, 3, act, interm, blind)
    cex = ChainExecutor(st)
    want = bsvd_clip(cex, net, x, x_planar=True, y_planar=(3, None))
    assert cex.launches == 32
    yc = _module([32, 64, 128], 32, interm, act, st, blind=blind, mode="clip")(x[None].to(_dev()))[0]
    assert_same_bits(yc, want, "clip schedule, T %d %dx%d blind %s" % (T, H, W, blind))
    ys = _module([32, 64, 128], 32, interm, act, st, blind=blind, mode="stream")(x[None].to(_dev()))[0]
    assert torch.equal(ys, yc)
    assert_same_bits(ys, want, "stream schedule")
