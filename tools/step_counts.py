"""Static instruction counts of the fused kernel's unrolled steps, from the assembly `hipcc -S` writes (no GPU needed):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics --cuda-device-only -S -Iinclude -Itelescope_amd/csrc unit.hip -o unit.s
    python tools/step_counts.py unit.s [mangled-name substring, default ILi4ELi0ELi2ELi0E]

The text of one kernel is cut at its `s_barrier`s.  A piece that holds streaming loads (`buffer_load ... nt`) and LDS atomics is one
unrolled data-wave step (blocks the compiler laid out of line are counted with the piece they stand in); a piece with neither is
an exchange-wave step or start-up / tail code.  Per piece: VALU, SALU (without waits, barriers, nops and branches), branches, LDS
instructions (`ds_add_f64` among them) and clock reads (`s_memtime` / `s_memrealtime`).  Then the kernel's registers and scratch."""
import re
import sys


def kernel_text(lines, key):
    start = next(i for i, l in enumerate(lines) if re.match(r'^_Z10k_em_fused\S*:', l) and key in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    return lines[start].split(':')[0], lines[start + 1:end]


def classify(op):
    if op.startswith('s_cbranch') or op in ('s_branch', 's_setpc_b64'):
        return 'branch'
    if op in ('s_memtime', 's_memrealtime'):
        return 'clock'
    if op.startswith(('s_waitcnt', 's_barrier', 's_nop', 's_endpgm', 's_sleep', 's_setprio')):
        return 'other'
    if op.startswith('s_'):
        return 'salu'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith('v_'):
        return 'valu'
    if op.startswith(('buffer_', 'global_', 'flat_', 'scratch_')):
        return 'vmem'
    return 'other'


def main():
    path = sys.argv[1]
    key = sys.argv[2] if len(sys.argv) > 2 else 'ILi4ELi0ELi2ELi0E'
    lines = open(path).read().split('\n')
    name, body = kernel_text(lines, key)
    pieces, cur = [], []
    for l in body:
        t = l.strip()
        if not t or t.startswith(('.', ';')) or t.endswith(':'):
            continue
        op = t.split()[0]
        cur.append((op, t))
        if op == 's_barrier':
            pieces.append(cur)
            cur = []
    pieces.append(cur)
    print('%s: %d pieces between barriers' % (name, len(pieces)))
    print('%-6s %-9s %6s %6s %8s %5s %10s %6s %6s' % ('piece', 'kind', 'VALU', 'SALU', 'branches', 'ds_', 'ds_add_f64', 'vmem', 'clock'))
    for n, p in enumerate(pieces):
        c = dict(valu=0, salu=0, branch=0, lds=0, vmem=0, clock=0, other=0)
        for op, _ in p:
            c[classify(op)] += 1
        adds = sum(1 for op, _ in p if op == 'ds_add_f64')
        stream = sum(1 for op, t in p if op.startswith('buffer_load') and ' nt' in t)
        kind = 'data' if stream and adds else ('exchange' if c['vmem'] and not stream else '-')
        print('%-6d %-9s %6d %6d %8d %5d %10d %6d %6d' % (n, kind, c['valu'], c['salu'], c['branch'], c['lds'], adds, c['vmem'], c['clock']))
    for pat in (r'\.vgpr_count:\s+(\d+)', r'\.sgpr_count:\s+(\d+)', r'\.private_segment_fixed_size:\s+(\d+)', r'\.vgpr_spill_count:\s+(\d+)'):
        i = next(i for i, l in enumerate(lines) if '.name:' in l and name in l)
        m = next((re.search(pat, l) for l in lines[max(0, i - 20):i + 30] if re.search(pat, l)), None)
        print('%s %s' % (pat.split(':')[0].replace('\\', ''), m.group(1) if m else '?'))


if __name__ == '__main__':
    main()
