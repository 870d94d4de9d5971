"""The CPU model of the exact-fp32 mode (oracle/chain_ref.c, tests/chain_exec.py) checked on the CPU, and the conditions that make the GPU
comparisons of tests/test_gpu_fp32_chain.py mean something:

  sanity     on the layer and edge cases of test_gpu_parity.py the chain is within TOL of the double-accumulating oracle (measured: printed);
  probes     exact-integer operands on which EVERY summation order gives the exact result: the chain in both orders, the double oracle and an
             int64 evaluation have the same bits -- so a kernel compared with the oracle on them needs no tolerance;
  mutations  a chain that is wrong the way a kernel could be wrong fails the assertion the GPU tests make (chain_exec.assert_same_bits).
"""
import numpy as np
import pytest
import torch

from chain_exec import CHAIN_OF, FAMILY_CASES, ChainExecutor, assert_same_bits, family_of, operands, same_bits
from helpers import maxabs
from oracle import chain_ref as CR
from oracle_exec import OracleExecutor, _slice_from_halo
from test_gpu_parity import EDGE_CASES, LAYER_CASES, TOL, edge_operands, layer_operands

BOTH_ORDERS = ({f: (CR.ORDER_MFMA, 0) for f in CHAIN_OF}, {f: (CR.ORDER_EDGE, 0) for f in CHAIN_OF})


# ------------------------------------------------------------------------------------------------ sanity
@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_chain_is_within_tol_of_the_double_oracle_on_the_layer_cases(case):
    sp, net, st, x, extra, eps, halos = layer_operands(*case)
    oex, cex = OracleExecutor(st, double=True), ChainExecutor(st)
    for hp, hn in halos:
        err = maxabs(cex.conv(sp, x, hp, hn, extra, eps, 1).numpy(), oex.conv(sp, x, hp, hn, extra, eps, 1).numpy())
        print("layer case %s, halos %s: chain vs double oracle max-abs %.3e (TOL %.0e)" % (case, "none" if hp is None else hp.pstride, err, TOL))
        assert err < TOL


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_chain_is_within_tol_of_the_double_oracle_on_the_edge_cases(case):
    sp, net, st, x, kws = edge_operands(*case)
    oex, cex = OracleExecutor(st, double=True), ChainExecutor(st)
    for kw in kws:
        err = maxabs(cex.conv(sp, x, **kw).numpy(), oex.conv(sp, x, **kw).numpy())
        print("edge case %s %s: chain vs double oracle max-abs %.3e (TOL %.0e)" % (case, kw.get("y_planar"), err, TOL))
        assert err < TOL


# ------------------------------------------------------------------------------------------------ exact-integer probes
def exact_reference(c, sp, st, x, kw):
    """Case ``c`` on integer operands in int64 (units: 1, or 2^-20 for the scaled ReLU6 layers), returned as the executor's fp32 tensor together
    with the largest magnitude any step can reach -- which must stay below 2^24 for fp32 to hold every partial sum of every order."""
    unit = 2.0 ** -20 if c.act == "relu6" else 1.0
    T, H, W = c.T, c.H, c.W
    s, fold = c.stride, sp.fold

    def ints(t, u=unit):
        v = t.double().numpy() / u
        r = np.rint(v).astype(np.int64)
        assert np.array_equal(r.astype(np.float64), v), "operand is no integer multiple of the unit"
        return r

    v = ints(x if c.kind == "head" else x[..., :c.cin].permute(0, 3, 1, 2))            # [T,cin,H,W]
    g = v.copy()
    if fold:
        g[:, :2 * fold] = 0
        g[:-1, :fold] = v[1:, :fold]
        g[1:, fold:2 * fold] = v[:-1, fold:2 * fold]
        if kw.get("halo_next") is not None:
            g[-1, :fold] = ints(_slice_from_halo(kw["halo_next"], H * W, fold).t().reshape(fold, H, W))
        if kw.get("halo_prev") is not None:
            g[0, fold:2 * fold] = ints(_slice_from_halo(kw["halo_prev"], H * W, fold).t().reshape(fold, H, W))
    w, b = ints(torch.as_tensor(st["l.weight"]), 1.0), ints(torch.as_tensor(st["l.bias"]))
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    gp = np.zeros((T, c.cin, H + 2, W + 2), np.int64)
    gp[:, :, 1:-1, 1:-1] = g
    acc = np.zeros((T, c.cout, Ho, Wo), np.int64)
    absacc = np.zeros((T, c.cout, Ho, Wo), np.int64)
    for ky in range(3):
        for kx in range(3):
            win = gp[:, :, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s]
            acc += np.einsum("oc,tchw->tohw", w[:, :, ky, kx], win)
            absacc += np.einsum("oc,tchw->tohw", np.abs(w[:, :, ky, kx]), np.abs(win))
    peak = int(absacc.max()) + int(np.abs(b).max())            # bounds every partial sum of every order, bias first or last
    y = acc + b[None, :, None, None]
    peak = max(peak, int(np.abs(y).max()))
    if c.act != "none":
        y = np.maximum(y, 0)
    if c.act == "relu6":
        y = np.minimum(y, int(6 / unit))
    e = kw.get("extra")
    if c.epi == 1:
        cq = c.cout // 4
        y = y.reshape(T, cq, 2, 2, Ho, Wo).transpose(0, 1, 4, 2, 5, 3).reshape(T, cq, 2 * Ho, 2 * Wo)
        if e is not None:
            y = y + ints(e[..., :cq].permute(0, 3, 1, 2))
    elif c.epi == 2:
        k = min(3, c.cout)
        ef = e.reshape(-1)
        ev = torch.as_strided(ef, (T, Ho * Wo, k), (e[0].numel(), kw["extra_pstride"], kw["extra_cstride"]), storage_offset=ef.storage_offset())
        y[:, :k] = ints(ev.reshape(T, Ho, Wo, k).permute(0, 3, 1, 2)) - y[:, :k]
    peak = max(peak, int(np.abs(y).max()))
    yf = torch.from_numpy((y.astype(np.float64) * unit).astype(np.float32))
    if c.kind == "tail":
        return (yf if c.clamp is None else yf.clamp(*c.clamp)), peak
    out = torch.zeros((T,) + tuple(yf.shape[-2:]) + (sp.cout_pad // 4 if c.epi == 1 else sp.cout_pad,))
    out[..., :yf.shape[1]] = yf.permute(0, 2, 3, 1)
    return out, peak


@pytest.mark.parametrize("c", FAMILY_CASES, ids=lambda c: c.name)
def test_integer_probe_is_exact_in_every_order(c):
    sp, net, st, x, kw = operands(c, "integer")
    exact, peak = exact_reference(c, sp, st, x, kw)
    assert peak < 2 ** 24, peak
    oracle = OracleExecutor(st, double=True).conv(sp, x, **kw)
    assert same_bits(oracle, exact), "the double oracle's own result is not the exact one"
    for chain_of in BOTH_ORDERS + (None,):
        assert_same_bits(ChainExecutor(st, chain_of).conv(sp, x, **kw), oracle, "%s, chain %s" % (c.name, chain_of))
    real = exact[..., :c.cout] if c.kind != "tail" and c.epi != 1 else exact
    if c.act == "relu6":
        assert float(real.min()) == 0.0 and float(real.max()) == 6.0 and bool(((real > 0) & (real < 6)).any()), "outputs straddle 0 and 6"
    print("%s: peak partial sum %d < 2^24; oracle == int64 == chain in both orders, %d values" % (c.name, peak, exact.numel()))


# ------------------------------------------------------------------------------------------------ mutations
def _mutant_fails(what, sp, x, kw, st, flags, want):
    """the GPU tests' assertion, made of a chain with ``flags`` in the kernel's place, must fail"""
    fam = family_of(kw.get("x_planar", False), kw.get("y_planar"))
    order, f0 = CHAIN_OF[fam]
    got = ChainExecutor(st, {fam: (order, f0 ^ flags)}).conv(sp, x, **kw)
    with pytest.raises(AssertionError) as ei:
        assert_same_bits(got, want, what)
    print("mutation -> assertion fails as it must: %s" % str(ei.value)[:200])


PROBE_MUTATION_CASES = [c for c in FAMILY_CASES if c.name in ("narrow 64 relu6", "wide 128, full halos", "fold8, full halos",
                                                              "stride 2, 27x43", "head 4->64 relu6", "tail 3, NHWC base")]      # (not a clamped exit: [0, 1] hides the values)


@pytest.mark.parametrize("flag,name", [(CR.ROUND11, "operands at 11 bits"), (CR.DROP_TERM, "one (channel, tap) term dropped")])
@pytest.mark.parametrize("c", PROBE_MUTATION_CASES, ids=lambda c: c.name)
def test_lost_precision_or_a_lost_term_breaks_the_integer_probe(c, flag, name):
    sp, net, st, x, kw = operands(c, "integer")
    _mutant_fails("%s, %s" % (c.name, name), sp, x, kw, st, flag, OracleExecutor(st, double=True).conv(sp, x, **kw))


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_a_changed_order_or_bias_place_changes_bits_on_normal_data(case):
    """The two k of an MFMA swapped; (tap, chunk) for (chunk, tap); the bias in front of the chain: each changes at least one output's bits
    in every layer case in which it changes the chain at all.  With Cin <= 4 (one chunk, every second term of an MFMA a zero-padded channel)
    the first two are the same chain -- asserted too, so that the exemption is no larger than that."""
    cin = case[0]
    sp, net, st, x, extra, eps, halos = layer_operands(*case)
    hp, hn = halos[-1]
    kw = dict(halo_prev=hp, halo_next=hn, extra=extra, extra_pstride=eps, extra_cstride=1)
    want = ChainExecutor(st).conv(sp, x, **kw)
    for flag, name, changes in ((CR.SWAP_K, "k swapped", cin > 4), (CR.TAP_MAJOR, "(tap, chunk) order", cin > 16), (CR.BIAS_FIRST, "bias first", True)):
        if changes:
            _mutant_fails("%s, %s" % (case, name), sp, x, kw, st, flag, want)
        else:
            assert same_bits(ChainExecutor(st, flags=flag).conv(sp, x, **kw), want)


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_bias_place_changes_bits_in_the_edge_kernels(case):
    sp, net, st, x, kws = edge_operands(*case)
    _mutant_fails("%s, bias at the other end" % (case,), sp, x, kws[-1], st, CR.BIAS_FIRST, ChainExecutor(st).conv(sp, x, **kws[-1]))
