"""Which fmaf chain does each kernel family of the exact-fp32 mode reproduce bit for bit?  Needs the MI355X.

    python tools/fp32_chain_probe.py [OUT]        (default OUT: fp32_chain_bits.txt in the current directory)

Every case of tests/chain_exec.py FAMILY_CASES on N(0,1) data against oracle/chain_ref.c under the four forms the documentation leaves open
(k = 0 or 1 of an MFMA first, the bias behind or in front of the chain), its max-abs error and the model's against the double-accumulating
oracle, and the exact-integer probe against that oracle.  profiles/fp32_chain_bits.txt is this tool's output with a reading added."""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
from chain_exec import CHAIN_OF, FAMILY_CASES, ChainExecutor, family_of, operands, same_bits
from helpers import maxabs
from oracle import chain_ref as CR
from oracle_exec import OracleExecutor
from test_gpu_fp32_chain import run_case

VARIANTS = [("k=0 first, bias last", 0), ("k=1 first, bias last", CR.SWAP_K), ("k=0 first, bias first", CR.BIAS_FIRST),
            ("k=1 first, bias first", CR.SWAP_K | CR.BIAS_FIRST)]
OUT = sys.argv[1] if len(sys.argv) > 1 else "fp32_chain_bits.txt"
rows = collections.OrderedDict()
lines = []
for c in FAMILY_CASES:
    sp, net, st, x, kw = operands(c, "normal")
    got, name = run_case(c, sp, net, st, x, kw)
    fam = family_of(kw.get("x_planar", False), kw.get("y_planar"))
    order = CHAIN_OF[fam][0]
    ref = OracleExecutor(st, double=True).conv(sp, x, **kw)
    match = []
    cerr = None
    for vn, fl in VARIANTS:
        w = ChainExecutor(st, {fam: (order, fl)}).conv(sp, x, **kw)
        if fl == CHAIN_OF[fam][1]:
            cerr = maxabs(w.numpy(), ref.numpy())
        if same_bits(got, w):
            match.append(vn)
    gerr = maxabs(got.numpy(), ref.numpy())
    isp, inet, ist, ix, ikw = operands(c, "integer")
    ig, _ = run_case(c, isp, inet, ist, ix, ikw)
    iok = same_bits(ig, OracleExecutor(ist, double=True).conv(isp, ix, **ikw))
    line = "%-52s %-44s matches [%s]  gpu-vs-double %.3e  chain-vs-double %.3e  integer probe %s" % (c.name, name, "; ".join(match) or "NONE", gerr, cerr, "exact" if iok else "DIFFERS")
    print(line, flush=True)
    lines.append(line)
    rows.setdefault(name, []).append((c.name, tuple(match), gerr, cerr, iok))
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n\n")
    for name, rs in rows.items():
        common = [v for v, _ in VARIANTS if all(v in r[1] for r in rs)]
        f.write("%-48s cases %2d  common match: %s  integer probes exact: %s\n" % (name, len(rs), "; ".join(common) or "NONE", all(r[4] for r in rs)))
print("PROBE DONE")
