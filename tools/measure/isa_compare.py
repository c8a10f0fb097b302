#!/usr/bin/env python3
"""Compares the gfx950 code generation of the correlation family between two trees.

  isa_compare.py TREE_A TREE_B [--work DIR] [--jobs N] [--out TABLE]
                 [--patterns GLOB ...] [--extra-flags=FLAGS]

For each tree every unit of the family (csrc/sfm_xcorr*.hip, sfm_mfma*.hip,
sfm_fft_own.hip; another family with --patterns, its own build flags with
--extra-flags) is compiled to device assembly with the production flags, the
functions are matched by demangled name with the enclosing namespaces dropped, and
for each the instruction text (local label numbers and symbol namespaces
normalised, comments dropped) and the .amdhsa_ lines (registers, scratch, LDS) are
compared.  One line per function: `same`, or the size of the difference.  The exit
status is 0 only if both trees hold the same functions and all of them are `same`.
"""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '--offload-device-only', '-S']
PATTERNS = ('sfm_xcorr*.hip', 'sfm_mfma*.hip', 'sfm_fft_own.hip')
NAMESPACES = re.compile(r'\(anonymous namespace\)::|\bsfm::mfma::|\bsfm::')


def emit(tree, work, jobs, patterns, extra):
  csrc = os.path.join(tree, 'sofima_amd', 'csrc')
  units = sorted(u for p in patterns for u in glob.glob(os.path.join(csrc, p)))
  os.makedirs(work, exist_ok=True)

  def one(unit):
    out = os.path.join(work, os.path.basename(unit)[:-4] + '.s')
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(unit):
      subprocess.run(['hipcc'] + FLAGS + extra + [unit, '-o', out], check=True)
    return out

  with ThreadPoolExecutor(max_workers=jobs) as pool:
    return list(pool.map(one, units))


def demangle(names):
  names = sorted(names)
  out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True,
                       check=True).stdout.split('\n')
  return {m: NAMESPACES.sub('', d) for m, d in zip(names, out)}


def functions(paths):
  """{normalised name: (instruction lines, .amdhsa_ lines)} of a tree's assembly files."""
  raw = {}      # (file, mangled name) -> [body lines, amdhsa lines]
  for path in paths:
    name = None
    hsa = None
    for line in open(path):
      line = line.split(';')[0].rstrip()
      s = line.strip()
      if not s:
        continue
      m = re.match(r'\.type\s+(\S+),@function', s)
      if m:
        name = m.group(1)
        raw[path, name] = [[], []]
        continue
      if s.startswith('.amdhsa_kernel'):
        hsa = s.split()[1]
        continue
      if s.startswith('.end_amdhsa_kernel'):
        hsa = None
        continue
      if hsa is not None:
        raw[path, hsa][1].append(s)
        continue
      if name is None:
        continue
      if re.match(r'\.Lfunc_end\d+:', s):
        name = None
        continue
      if s == name + ':' or s.startswith(('.p2align', '.globl', '.section', '.text', '.protected',
                                          '.weak', '.hidden')):
        continue
      raw[path, name][0].append(s)
  symbols = {n for _, n in raw}
  for body, _ in raw.values():
    for s in body:
      symbols.update(re.findall(r'\b_Z\w+', s))
  plain = demangle(symbols)

  def norm(s):
    s = re.sub(r'\b_Z\w+', lambda m: '<' + plain[m.group(0)] + '>', s)
    # (.Lpost_getpc<n>, the label of a long branch, is numbered through the whole unit)
    s = re.sub(r'\.L(BB|tmp|func_begin|func_end|JTI|post_getpc)\d+', r'.L\1', s)
    return re.sub(r'\s+', ' ', s)

  # (a device function that is not inlined exists once per unit that calls it: one entry
  # if the copies agree, else one per unit)
  found = {}
  for (path, n), (body, hsa) in raw.items():
    found.setdefault(plain[n], {})[os.path.basename(path)] = ([norm(s) for s in body], hsa)
  out = {}
  for n, copies in found.items():
    if all(c == next(iter(copies.values())) for c in copies.values()):
      out[n] = next(iter(copies.values()))
    else:
      out.update({'%s [%s]' % (n, unit): c for unit, c in copies.items()})
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('tree_a')
  ap.add_argument('tree_b')
  ap.add_argument('--work', default='measure_out/isa_compare')
  ap.add_argument('--jobs', type=int, default=min(os.cpu_count() or 1, 16))
  ap.add_argument('--out', default=None)
  ap.add_argument('--patterns', nargs='+', default=list(PATTERNS))
  ap.add_argument('--extra-flags', default='')
  args = ap.parse_args()
  extra = args.extra_flags.split()
  fa = functions(emit(args.tree_a, os.path.join(args.work, 'a'), args.jobs, args.patterns, extra))
  fb = functions(emit(args.tree_b, os.path.join(args.work, 'b'), args.jobs, args.patterns, extra))
  rows = []
  bad = 0
  for name in sorted(set(fa) | set(fb)):
    if name not in fb:
      verdict = 'only in A'
    elif name not in fa:
      verdict = 'only in B'
    else:
      (ia, ha), (ib, hb) = fa[name], fb[name]
      parts = []
      if ia != ib:
        changed = sum(1 for d in difflib.unified_diff(ia, ib, lineterm='', n=0)
                      if d[:1] in '+-' and d[:3] not in ('+++', '---'))
        parts.append('%d of %d instruction lines differ' % (changed, len(ia)))
      if ha != hb:
        parts.append('.amdhsa_ differs: ' + ', '.join(sorted(set(ha) ^ set(hb))))
      verdict = '; '.join(parts) or 'same'
    bad += verdict != 'same'
    rows.append('%-9s %s' % (verdict if verdict == 'same' else 'DIFF', name) +
                ('' if verdict == 'same' else '\n          ' + verdict))
  text = ('# isa_compare.py: %d functions in A, %d in B, %d not the same\n' %
          (len(fa), len(fb), bad) + '\n'.join(rows) + '\n')
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text)
  sys.stdout.write(text)
  return 1 if bad else 0


if __name__ == '__main__':
  sys.exit(main())
