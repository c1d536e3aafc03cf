#!/usr/bin/env python3
"""Static loop census of a hipcc -S listing: for every loop the assembler comments mark (`Loop Header: Depth=N`), count the
instructions between the header label and the last backward branch to it, by class.  Used to see what sits inside the layer
loops of samsim_step_kernel (scratch traffic, SGPR-spill lane moves, FP64 VALU, memory).
usage: isa_loops.py kern.s <kernel-name-substring> [min_instructions]
       isa_loops.py --marks kern.s <kernel-name-substring>

--marks (listing built with -DSAMSIM_ISA_MARKS=1): the request lead of every marked loop.  For each loop that holds a mark
`*_ITER_BEGIN` or `*_REST_BEGIN` the loop's main path is walked twice round (see marks_report) with the in-order counter of
outstanding vector-memory operations the hardware keeps; every operation on that path counts, conditional stores included, as
it does for a wave that takes them.  Per request group (adjacent global loads) it prints where the `s_waitcnt vmcnt(N)` that
retires it sits, how many vector-memory operations and vector instructions were issued between the request and that wait, the
first instruction that reads a loaded register, and how many vector instructions lie between the wait and that reader.  A first
reader that is a `v_mov` is flagged COPY: the wait guards a register copy (a buffer rotation), not arithmetic -- the row is
waited for wherever the copy stands, however far away its first real use is."""
import re, sys, collections

REG = re.compile(r'\b([vs])(?:\[(\d+):(\d+)\]|(\d+))')

def regs_of(text):
    out = set()
    for m in REG.finditer(text):
        if m.group(1) != 'v': continue
        lo, hi = (int(m.group(2)), int(m.group(3))) if m.group(2) else (int(m.group(4)),) * 2
        out.update(range(lo, hi + 1))
    return out

def marks_report(body, label_at):
    """body: lines of one kernel.  A marked loop is the loop whose header the assembler's block comment names for the block that
    holds a `*_ITER_BEGIN` / `*_REST_BEGIN` mark; its main path is followed from the header: straight on through conditional
    branches (the `s_cbranch_execz` skips of empty regions, the exits and the back edges of inner loops), along `s_branch`, and
    back to the header on any branch that goes there.  Where the straight-on side of a branch is the rare one (the single-layer
    copy inside the down sweep's two-layer trip) the source marks it `*_RARE_BEGIN`, and the walk takes the branch instead."""
    def header_of(i):
        for j in range(i, -1, -1):
            m = re.match(r'^(\.LBB\d+_\d+):(.*)', body[j])
            if not m: continue
            if 'Loop Header' in ' '.join(body[j:j + 3]) and 'Inner Loop Header' not in ' '.join(body[j:j + 3]): return m.group(1)
            h = re.search(r'Header=(BB\d+_\d+)', m.group(2))
            if 'Inner Loop Header' in ' '.join(body[j:j + 3]): return m.group(1)
            return '.L' + h.group(1) if h else None
        return None
    seen = set()
    for i, l in enumerate(body):
        mk = re.search(r'; ISA_MARK (\S+_(?:ITER|REST)_BEGIN)', l)
        if not mk: continue
        lab = header_of(i)
        if lab is None or lab in seen or lab not in label_at: continue
        seen.add(lab)
        # the main path, twice round
        path, pc, rounds, steps, untaken = [], label_at[lab], 0, 0, []
        while rounds < 2 and steps < 200000:
            steps += 1
            l2 = body[pc]
            path.append((pc, rounds))
            m = re.match(r'^\s+(s_c?branch\S*)\s+(\.LBB\d+_\d+)', l2)
            nxt = pc + 1
            if re.search(r'; ISA_MARK \S+_RARE_BEGIN', l2) and untaken:
                # a region marked *_RARE_BEGIN is not on the main path: back to the last conditional branch passed, and take it
                keep, pc = untaken.pop()
                del path[keep:]
                continue
            if m and m.group(2) in label_at:
                if m.group(2) == lab: nxt = label_at[lab]
                elif label_at[m.group(2)] < label_at[lab] and m.group(1) == 's_branch' and ('Header=' + lab[2:] + ' ') in body[label_at[m.group(2)]]:
                    nxt = label_at[m.group(2)]               # the loop's tail, laid out in front of its header
                elif label_at[m.group(2)] <= pc: pass        # latch of an inner loop: its body is walked once
                elif m.group(1) == 's_branch': nxt = label_at[m.group(2)]
                else: untaken.append((len(path), label_at[m.group(2)]))
            if nxt == label_at[lab]: rounds += 1
            if nxt >= len(body): break
            pc = nxt
        if rounds < 2:
            print('loop %s (mark %s): the main path does not return to the header\n' % (lab, mk.group(1)))
            continue
        once = [pc for pc, r in path if r == 0]
        names = [m.group(1) for pc in once for m in [re.search(r'; ISA_MARK (\S+)', body[pc])] if m and not m.group(1).startswith(('U_GETT', 'NEWTON'))]
        scr = sum(1 for pc in once if re.match(r'^\s+scratch_', body[pc]))
        print('loop %s  header at line %d, %d lines on the main path  marks: %s  scratch accesses on the main path: %d' % (lab, label_at[lab], len(once), ' '.join(names), scr))
        queue = []      # outstanding vector-memory operations, oldest first: index of the request group, None for stores
        groups = []     # request groups
        open_reads = {} # vgpr -> group, loaded and not yet read
        seg = '(loop head)'
        last_load_pos = -10
        pos = 0
        notes = []
        for pc, rnd in path:
                l = body[pc]
                mk2 = re.search(r'; ISA_MARK (\S+)', l)
                if mk2 and not mk2.group(1).startswith(('U_GETT', 'NEWTON')): seg = mk2.group(1)
                m = re.match(r'^\s+([a-z_0-9]+)\s*(.*?)(?:;.*)?$', l)
                if not m or l.strip().startswith((';', '.')): continue
                op, args = m.group(1), m.group(2)
                pos += 1
                is_v = op.startswith('v_')
                is_ld = op.startswith(('global_load', 'buffer_load', 'scratch_load'))
                is_st = op.startswith(('global_store', 'buffer_store', 'scratch_store', 'global_atomic'))
                parts = args.split(',')
                dst = regs_of(parts[0]) if (is_v or is_ld) and parts else set()
                src = regs_of(','.join(parts[1:])) if (is_v or is_ld) else regs_of(args)
                if op.startswith(('v_fmac', 'v_readlane', 'v_cmp', 'v_readfirstlane')): src |= dst
                if op.startswith(('v_cmp', 'v_readlane', 'v_readfirstlane')): dst = set()
                for r in sorted(src):   # first reader of a loaded register
                    gidx = open_reads.get(r)
                    if gidx is None: continue
                    gr = groups[gidx]
                    if 'use_op' not in gr:
                        gr['use_op'], gr['use_seg'], gr['use_line'] = op, seg, pc
                        gr['valu_wait_to_use'] = gr['valu_seen'] - gr['valu_at_wait'] if 'valu_at_wait' in gr else 'NO WAIT'
                        gr['copy'] = op.startswith('v_mov')
                    for q in [q for q, v in open_reads.items() if v == gidx]: del open_reads[q]
                for r in dst: open_reads.pop(r, None)
                if is_v:
                    for gr in groups: gr['valu_seen'] += 1
                if is_ld or is_st:
                    for gr in groups:
                        if 'wait_line' not in gr: gr['vm_after'] += 1
                    gr = None
                    if op.startswith('global_load'):
                        if pos - last_load_pos <= 3 and groups and groups[-1]['open']:
                            gr = groups[-1]; gr['vm_after'] -= 1
                        else:
                            for g2 in groups: g2['open'] = False
                            gr = dict(line=pc, rnd=rnd, seg=seg, n=0, vm_after=0, valu_seen=0, open=True)
                            groups.append(gr)
                        gr['n'] += 1; last_load_pos = pos
                        for r in dst: open_reads[r] = len(groups) - 1
                    queue.append(len(groups) - 1 if gr is not None else None)
                w = re.search(r'vmcnt\((\d+)\)', args) if op == 's_waitcnt' else None
                if w:
                    keep = int(w.group(1))
                    while len(queue) > keep:
                        gidx = queue.pop(0)
                        if gidx is None or gidx in queue: continue
                        gr = groups[gidx]
                        if 'wait_line' not in gr:
                            gr['wait_line'], gr['wait_n'], gr['wait_seg'] = pc, keep, seg
                            gr['valu_to_wait'] = gr['valu_at_wait'] = gr['valu_seen']
        print('  %-8s %-14s %2s | %-8s %-14s %-9s %6s %8s | %-20s %-14s %7s' % ('request', 'after mark', 'n', 'wait', 'after mark', '', 'vm ops', 'v instr', 'first reader', 'after mark', 'v instr'))
        for gr in groups:
            if gr['rnd'] != 0: continue
            if 'wait_line' not in gr:
                print('  %-8d %-14s %2d | not retired by a counted wait within two trips' % (gr['line'], gr['seg'], gr['n']))
                continue
            print('  %-8d %-14s %2d | %-8d %-14s %-9s %6d %8d | %-20s %-14s %7s %s' % (
                gr['line'], gr['seg'], gr['n'], gr['wait_line'], gr['wait_seg'], 'vmcnt(%d)' % gr['wait_n'], gr['vm_after'], gr['valu_to_wait'],
                gr.get('use_op', '(none)'), gr.get('use_seg', ''), gr.get('valu_wait_to_use', ''), 'COPY of an outstanding row' if gr.get('copy') else ''))
        print()

def main():
    marks = '--marks' in sys.argv
    if marks: sys.argv.remove('--marks')
    path, kname = sys.argv[1], sys.argv[2]
    min_n = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    lines = open(path).read().split('\n')
    start = next(i for i, l in enumerate(lines) if l.startswith('_Z') and kname in l and l.split(':')[0].endswith(l.split(':')[0]) and ':' in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    body = lines[start:end]
    label_at = {}
    for i, l in enumerate(body):
        m = re.match(r'^(\.LBB\d+_\d+):', l)
        if m: label_at[m.group(1)] = i
    # backward branches
    loops = collections.defaultdict(int)
    for i, l in enumerate(body):
        m = re.match(r'^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)', l)
        if m and m.group(1) in label_at and label_at[m.group(1)] <= i:
            loops[m.group(1)] = max(loops[m.group(1)], i)
    if marks:
        marks_report(body, label_at)
        return
    def classify(op):
        if op.startswith('scratch_load'): return 'scr_ld'
        if op.startswith('scratch_store'): return 'scr_st'
        if op.startswith('global_load') or op.startswith('buffer_load'): return 'g_ld'
        if op.startswith('global_store') or op.startswith('buffer_store'): return 'g_st'
        if op.startswith('ds_'): return 'lds'
        if op.startswith('v_readlane') or op.startswith('v_writelane') or op.startswith('v_readfirstlane'): return 'lane'
        if op.startswith('v_') and 'f64' in op: return 'v_f64'
        if op.startswith('v_'): return 'v_other'
        if op.startswith('s_waitcnt'): return 'wait'
        if op.startswith('s_cbranch') or op.startswith('s_branch'): return 'branch'
        if op.startswith('s_'): return 's_alu'
        return 'other'
    rows = []
    for lab, last in loops.items():
        first = label_at[lab]
        cnt = collections.Counter()
        for l in body[first:last + 1]:
            m = re.match(r'^\s+([a-z_0-9]+)', l)
            if not m or l.strip().startswith(';') or l.strip().startswith('.'): continue
            cnt[classify(m.group(1))] += 1
        n = sum(cnt.values())
        hdr = body[first + 1] if first + 1 < len(body) else ''
        depth = re.search(r'Depth=(\d+)', ' '.join(body[first:first + 3]))
        rows.append((first, last, lab, n, cnt, depth.group(1) if depth else '?'))
    rows.sort()
    keys = ['v_f64', 'v_other', 's_alu', 'branch', 'wait', 'g_ld', 'g_st', 'scr_ld', 'scr_st', 'lane', 'lds']
    print('%-12s %7s %7s %3s %6s ' % ('label', 'line', 'end', 'd', 'n') + ' '.join('%7s' % k for k in keys))
    for first, last, lab, n, cnt, d in rows:
        if n < min_n: continue
        print('%-12s %7d %7d %3s %6d ' % (lab, first, last, d, n) + ' '.join('%7d' % cnt[k] for k in keys))
    tot = collections.Counter()
    for l in body:
        m = re.match(r'^\s+([a-z_0-9]+)', l)
        if not m or l.strip().startswith(';') or l.strip().startswith('.'): continue
        tot[classify(m.group(1))] += 1
    print('%-12s %7d %7d %3s %6d ' % ('TOTAL', 0, len(body), '', sum(tot.values())) + ' '.join('%7d' % tot[k] for k in keys))

if __name__ == '__main__':
    main()
