"""Static view of one kernel: compiles a .hip file for gfx950 and prints, for the named kernel, the register and
spill counts of its metadata, its code size, and per barrier-delimited phase the instructions by class prefix.

    python tests/tools/kernel_isa_stats.py pysubstringsearch_amd/csrc/msd_sort.hip msd_local_fast_kernel [-DFLAG ...]

Classes (by mnemonic prefix only): v_ (vector ALU, lane moves included), s_ (scalar, branches and waits included),
ds_ (LDS), mem (global_/flat_/buffer_/scratch_), lane (v_readlane / v_writelane: scalar spills live there), br
(s_cbranch / s_branch), exec (s_*_saveexec: a lane mask put in force).  Phase k is what stands between the k-th and
the (k+1)-th s_barrier of the listing; code the compiler placed out of line is counted where it stands.  Needs hipcc
only, no GPU."""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
READELF = os.environ.get('READELF', '/opt/rocm/llvm/bin/llvm-readelf')
META = ('.sgpr_count', '.sgpr_spill_count', '.vgpr_count', '.vgpr_spill_count', '.private_segment_fixed_size',
        '.group_segment_fixed_size', '.max_flat_workgroup_size')
CLASSES = ('v_', 's_', 'ds_', 'mem', 'lane', 'br', 'exec')


def classify(op):
    out = []
    if op.startswith('v_'):
        out.append('v_')
        if op.startswith(('v_readlane', 'v_writelane')):
            out.append('lane')
    elif op.startswith('s_'):
        out.append('s_')
        if op.startswith(('s_cbranch', 's_branch')):
            out.append('br')
        if 'saveexec' in op:
            out.append('exec')
    elif op.startswith('ds_'):
        out.append('ds_')
    elif op.startswith(('global_', 'flat_', 'buffer_', 'scratch_')):
        out.append('mem')
    return out


def kernel_stats(asm, kernel):
    lines = asm.splitlines()
    label = re.compile(r'^(_Z\w*%s\w*):' % re.escape(kernel))
    start = next((i for i, ln in enumerate(lines) if label.match(ln)), None)
    if start is None:
        raise SystemExit(f'no kernel named *{kernel}* in the listing')
    symbol = label.match(lines[start]).group(1)
    phases = [dict.fromkeys(CLASSES, 0)]
    for ln in lines[start + 1:]:
        m = re.match(r'^\s+([a-z_0-9]+)', ln)
        if not m:
            continue
        op = m.group(1)
        if op == 's_barrier':
            phases.append(dict.fromkeys(CLASSES, 0))
        for c in classify(op):
            phases[-1][c] += 1
        if op == 's_endpgm':
            break
    meta = {}
    at = next(i for i, ln in enumerate(lines) if re.match(r'^\s+\.name:\s+%s\s*$' % re.escape(symbol), ln))
    lo = max(j for j in range(at) if lines[j].lstrip().startswith('- .'))            # this kernel's metadata entry ...
    hi = next((j for j in range(at + 1, len(lines)) if lines[j].lstrip().startswith('- .agpr_count')
               or lines[j].startswith('amdhsa.')), len(lines))
    for ln in lines[lo:hi]:
        m = re.match(r'^\s*-?\s*(\.\w+):\s+(\S+)', ln)
        if m and m.group(1) in META:
            meta[m.group(1)] = m.group(2)
    return symbol, meta, phases


def main():
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    src, kernel, flags = sys.argv[1], sys.argv[2], sys.argv[3:]
    base = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', *flags, '-x', 'hip', src]
    with tempfile.TemporaryDirectory() as d:
        s_path, o_path = os.path.join(d, 'k.s'), os.path.join(d, 'k.o')
        subprocess.run(base + ['-S', '-o', s_path], check=True, stderr=subprocess.DEVNULL)
        symbol, meta, phases = kernel_stats(open(s_path).read(), kernel)
        size = None
        if os.path.exists(READELF):
            subprocess.run(base + ['--no-gpu-bundle-output', '-c', '-o', o_path], check=True, stderr=subprocess.DEVNULL)
            syms = subprocess.run([READELF, '-sW', o_path], check=True, capture_output=True, text=True).stdout
            for ln in syms.splitlines():
                f = ln.split()
                if len(f) >= 8 and f[-1] == symbol and f[3] == 'FUNC':
                    size = int(f[2], 0)
    print(f'{src} {" ".join(flags)}'.rstrip())
    print(f'kernel {symbol}')
    for k in META:
        if k in meta:
            print(f'  {k[1:]:28s} {meta[k]}')
    if size is not None:
        print(f'  {"code_bytes":28s} {size}')
    print('  phase ' + ' '.join(f'{c:>6s}' for c in CLASSES))
    total = dict.fromkeys(CLASSES, 0)
    for i, ph in enumerate(phases):
        print(f'  {i:5d} ' + ' '.join(f'{ph[c]:6d}' for c in CLASSES))
        for c in CLASSES:
            total[c] += ph[c]
    print('  total ' + ' '.join(f'{total[c]:6d}' for c in CLASSES))


if __name__ == '__main__':
    main()
