#!/bin/bash
# Digest of the instruction stream of every kernel of one build (compile-time: no GPU needed): is a source change a pure refactor?
# usage: [EXTRA_HIPCC_FLAGS=...] tools/isa_digest.sh [source ...]   (default: every product source)  -> per translation unit one line per kernel (demangled name, sha256 of its body
#        from its label to its .Lfunc_end) and a last line with the sha256 of the whole normalised assembly file
# Normalised: comment lines, .file / .ident / .loc / .section / .Ltmp* / .Lfunc* lines, trailing ";" comments and the lines naming
# __hip_cuid_<hash> (a hash of the source text) are dropped.  Same flags and sources as tools/kernel_resources.sh.
# ISA_DIGEST_MASK_ORDINAL=1: a body's local labels (.LBB<n>_<block>) lose <n>, the kernel's position in its file -- for a change that only
# reorders the kernels of a translation unit (the whole-file digest still sees the order).
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT=$(mktemp -d)
. "$ROOT/bsvd_amd/csrc/sources.sh"      # BSVD_SRCS, bsvd_src_flags: the list bsvd_amd/csrc/build.sh builds
SRCS="$BSVD_SRCS"
[ $# -gt 0 ] && SRCS="$*"
for src in $SRCS; do
  XF="$(bsvd_src_flags $src)"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$ROOT/include -I$ROOT/bsvd_amd/csrc -Wno-unused-function \
     $XF ${EXTRA_HIPCC_FLAGS} --cuda-device-only -S $ROOT/bsvd_amd/csrc/$src.hip -o $OUT/$src.s 2> $OUT/$src.log &
done
wait
rc=0
for src in $SRCS; do
  [ -s $OUT/$src.s ] || { echo "isa_digest: $src.hip did not compile" >&2; cat $OUT/$src.log >&2; rc=1; continue; }
  python3 - $src $OUT/$src.s ${ISA_DIGEST_KEEP:+$ISA_DIGEST_KEEP/$src.norm.s} <<'EOF' || rc=1
import hashlib, os, re, subprocess, sys
src, path = sys.argv[1], sys.argv[2]
raw = open(path).read().splitlines()
kernels = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', '\n'.join(raw), re.M))
DROP = ('.file', '.ident', '.loc', '.section', '.Ltmp', '.Lfunc')
norm, bodies, cur = [], [], None
for l in raw:
    s = l.strip()
    m = re.match(r'(\w+):', s)
    if m and m.group(1) in kernels: cur = (m.group(1), []); bodies.append(cur)
    if s.startswith('.Lfunc_end'): cur = None
    if not s or s.startswith(';') or s.startswith(DROP) or '__hip_cuid_' in s: continue
    l = re.sub(r'\s*;.*$', '', l.rstrip())
    if not l.strip(): continue
    norm.append(l)
    if cur is not None: cur[1].append((re.sub(r'\.LBB\d+_', '.LBB_', l) if os.environ.get('ISA_DIGEST_MASK_ORDINAL') else l).replace(cur[0], '<kernel>'))      # (its own symbol -- label, .amdhsa_kernel -- is not part of a body's digest)
sha = lambda ls: hashlib.sha256(('\n'.join(ls) + '\n').encode()).hexdigest()
names = subprocess.run(['c++filt'] + [n for n, _ in bodies], capture_output=True, text=True).stdout.splitlines() if bodies else []
print('== %s: %d kernels' % (src, len(bodies)))
for (n, b), d in zip(bodies, names):
    d = d.replace('bsvd::', '').replace('void ', '').replace('(ConvParams)', '')
    print('%-100s %6d lines %s' % (d[:100], len(b), sha(b)))
print('%-100s %6d lines %s' % (src + ' (whole file)', len(norm), sha(norm)))
if len(sys.argv) > 3: open(sys.argv[3], 'w').write('\n'.join(norm) + '\n')      # ISA_DIGEST_KEEP=<dir>: keep the normalised files (to diff)
EOF
done
rm -rf $OUT
exit $rc
