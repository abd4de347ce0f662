#!/usr/bin/env python
"""What the compiled Winograd kernels (csrc/wino_conv.hip) do with the weight stream and the window DMA, read from
their gfx950 assembly.  A tool, not a test: it prints, per kernel instance,

  weight loads   MFMAs between the issue of a transformed-weight load (buffer_load_dwordx4 into VGPRs) and the first
                 MFMA that reads its destination - the wait that covers the load stands in front of that MFMA.  Loads
                 inside the K loop only (the prologue's first loads are waited on before any MFMA by construction);
                 the scan follows the loop round its back edge.  min .. max over the loads.
  window DMA     MFMAs between the last LDS-DMA piece of a chunk's window (buffer_load_dwordx4 .. lds) and the first
                 s_waitcnt vmcnt(N) that forces the FIRST piece: vmcnt retires in order, so a wait forces the piece as
                 soon as N <= the loads issued behind it.  Loads and waits are taken in layout order; a load inside a
                 block that a forward branch can skip (the sixth piece, which one wave of four does not issue) is not
                 counted, which is the case of the wave with the fewest pieces - the other arm of such a branch holds
                 the same wait with the count one higher.
  registers      VGPRs, scratch bytes, occupancy (the compiler's resource summary), accumulation-register moves, and
                 the highest VGPR the COMPILER touches outside asm statements: the ring kernels keep their ring in
                 named registers above a budget (amdgpu_num_vgpr) that the compiler must stay under.

  python tools/wino_sched_report.py [--ablation]          compile csrc/wino_conv.hip with the Makefile's flags
  python tools/wino_sched_report.py --asm FILE.s          read an assembly file made earlier (e.g. of another commit)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'stereotracking_amd', 'csrc')
SHORT_BLOCK = 24   # lines: a forward branch over at most this much skips one conditional piece, not a whole window


def compile_asm(ablation):
    flags = subprocess.check_output(['make', '-s', '-C', CSRC, 'print-cxxflags'] + (['ABLATION=1'] if ablation else []),
                                    text=True).split()
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    out = os.path.join(tempfile.mkdtemp(prefix='wino_sched_'), 'wino_conv.s')
    subprocess.check_call([hipcc] + flags + ['-x', 'hip', '--cuda-device-only', '-S', os.path.join(CSRC, 'wino_conv.hip'),
                                              '-o', out], stderr=subprocess.DEVNULL)
    return out


def demangle(names):
    try:
        out = subprocess.check_output(['c++filt'] + names, text=True).split('\n')
        return [re.sub(r'\(anonymous namespace\)::|st::|\(.*$', '', o) for o in out[:len(names)]]
    except (OSError, subprocess.CalledProcessError):
        return names


def kernels(path):
    """[(mangled name, [instruction / label lines], {summary})] in file order."""
    out, cur = [], None
    for line in open(path):
        m = re.match(r'^(_Z\w+):\s*; @', line)
        if m:
            cur = (m.group(1), [], {})
            out.append(cur)
            continue
        if cur is None:
            continue
        m = re.match(r'^; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)', line)
        if m:
            cur[2][m.group(1)] = int(m.group(2))
            if m.group(1) == 'Occupancy':
                cur = None
            continue
        s = line.split(';')[0].rstrip() if not line.lstrip().startswith(';;#') else line.strip()
        if s.strip():
            cur[1].append(s.strip())
    return out


def regs(tok):
    m = re.match(r'v\[(\d+):(\d+)\]', tok)
    if m:
        return range(int(m.group(1)), int(m.group(2)) + 1)
    m = re.match(r'v(\d+)$', tok)
    return range(int(m.group(1)), int(m.group(1)) + 1) if m else range(0)


def analyse(lines):
    label = {l[:-1]: i for i, l in enumerate(lines) if re.match(r'^\.LBB\w+:$', l)}
    loops, skipped = [], set()
    for i, l in enumerate(lines):
        m = re.match(r'^s_c?branch\w*\s+(\.LBB\w+)$', l)
        if not m or m.group(1) not in label:
            continue
        t = label[m.group(1)]
        if t < i:
            loops.append((t, i))
        elif l.startswith('s_cbranch') and t - i <= SHORT_BLOCK:
            skipped.update(range(i + 1, t))
    def order(i):
        inside = [lp for lp in loops if lp[0] <= i <= lp[1]]
        if not inside:
            return None
        a, b = min(inside, key=lambda lp: lp[1] - lp[0])
        return list(range(i + 1, b + 1)) + list(range(a, i))
    is_mfma = lambda l: l.startswith('v_mfma')
    is_dma = lambda l: l.startswith('buffer_load') and l.endswith(' lds')
    is_wload = lambda l: l.startswith('buffer_load_dwordx4 v[') and not l.endswith(' lds') and 'offen' in l
    is_vm = lambda l: l.startswith(('buffer_load', 'buffer_store', 'global_load', 'global_store'))
    wl = []
    for i, l in enumerate(lines):
        if not is_wload(l) or order(i) is None:
            continue
        dst, n = set(regs(l.split()[1].rstrip(','))), 0
        for j in order(i):
            lj = lines[j]
            if is_mfma(lj):
                ops = [o.strip() for o in lj.split(None, 1)[1].split(',')]
                if set(regs(ops[2])) & dst:
                    wl.append(n)
                    break
                n += 1
            elif is_wload(lj) and set(regs(lj.split()[1].rstrip(','))) & dst:
                break   # overwritten before any MFMA read it (a clamped re-load behind the last step)
    dma, i = [], 0
    while i < len(lines):
        if not is_dma(lines[i]) or order(i) is None or i in skipped:
            i += 1
            continue
        seq = order(i)
        last = i   # the last piece of this window: pieces follow each other before the first wait
        for j in seq:
            if is_dma(lines[j]):
                last = j
            if re.match(r'^s_waitcnt.*vmcnt', lines[j]) or is_mfma(lines[j]):
                break
        younger, n, forced = 0, 0, None
        for j in seq:
            lj = lines[j]
            if is_vm(lj) and j not in skipped:
                younger += 1
            elif is_mfma(lj) and (j > last or j < i):
                n += 1
            m = re.match(r'^s_waitcnt.*vmcnt\((\d+)\)', lj)
            if m and younger >= int(m.group(1)):
                forced = n
                break
        dma.append(forced)
        i = max(last, i) + 1
    compiler_high, in_asm = -1, False
    for l in lines:
        if l.startswith(';;#ASMSTART'):
            in_asm = True
        elif l.startswith(';;#ASMEND'):
            in_asm = False
        elif not in_asm:
            for tok in re.findall(r'v\[\d+:\d+\]|v\d+', l):
                compiler_high = max(compiler_high, max(regs(tok), default=-1))
    return wl, dma, compiler_high, sum('v_accvgpr' in l for l in lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--asm', help='assembly file to read instead of compiling csrc/wino_conv.hip')
    ap.add_argument('--ablation', action='store_true', help='compile with ABLATION=1 (the tools build: every schedule)')
    args = ap.parse_args()
    ks = [k for k in kernels(args.asm or compile_asm(args.ablation)) if 'wino_conv3x3' in k[0] and 'persist' not in k[0]]
    names = demangle([k[0] for k in ks])
    print(f'{"kernel":58s} {"weight loads: MFMAs to cover":>29s} {"window DMA: MFMAs to force":>27s}  VGPRs  scratch  occ'
          f'  compiler<=  accvgpr')
    worst = 0
    for (_, lines, summ), name in zip(ks, names):
        wl, dma, high, acc = analyse(lines)
        w = f'{min(wl)} .. {max(wl)} ({len(wl)} loads)' if wl else '-'
        d = ('-' if not dma else 'never' if all(x is None for x in dma) else
             f'{min(x for x in dma if x is not None)} ({len(dma)} windows)')
        print(f'{name:58s} {w:>29s} {d:>27s}  {summ.get("NumVgprs", -1):5d}  {summ.get("ScratchSize", -1):7d}  '
              f'{summ.get("Occupancy", -1):3d}  v{high:<9d}  {acc:7d}')
        worst |= summ.get('ScratchSize', 0) != 0 or acc != 0
    return 1 if worst else 0


if __name__ == '__main__':
    sys.exit(main())
