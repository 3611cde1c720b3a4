"""Static check of k_compat_wide's machine code (hipcc -S, no GPU needed).

k_compat_wide (phl_compat_wide.hip) keeps a 16-pixel x 512-label row in 128 accumulator registers and runs two
workgroups per CU; its pieces of the planes arrive by LDS-DMA with counted waits.  For every instance of the kernel
(NT = 9 .. 16 K chunks, softmax and logits epilogues) this script verifies:
  * no scratch and no AGPRs, at most 256 VGPRs (two waves per SIMD: the two workgroups of a CU);
  * each slot ends in its counted wait followed by the workgroup barrier: every s_barrier in the slot loop is preceded by
    an `s_waitcnt vmcnt(6)` or `vmcnt(8)` (what the slot may leave in flight: the next slot's six DMA units and the X
    loads issued behind them) -- a compiler-made vmcnt(0) in its place would mean the DMAs of the next slot are drained;
  * six DMA units (global_load_lds_dwordx4) per slot and the X loads behind them, not in front (the counts above
    assume that order).
The E0 loads are ordinary compiler-visible loads (no inline-assembly hidden loads), so there is no hidden-load discipline
to check.  Exit code 0 = ok.  Used by tests/test_compat_wide_host.py."""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(asm_text):
    problems, seen = [], set()
    for m in re.finditer(r'^(_ZN\S*k_compat_wideILi(\d+)ELb(\d)E\S*):[^\n]*\n(.*?)\.end_amdhsa_kernel', asm_text, re.S | re.M):
        name, nt, body = m.group(1), int(m.group(2)), m.group(4)
        seen.add((nt, int(m.group(3))))
        lines = [l.strip() for l in body.split('\n')]
        code = [l for l in lines if l and l[0] not in ';.' and not l.endswith(':')]
        nq = (2 * nt + 7) // 8
        head = [i for i, l in enumerate(code) if l.startswith('s_barrier')]
        # one prologue barrier, then one per slot of the (runtime) chunk loop: NQ slots in its body
        if len(head) != 1 + nq:
            problems.append(f'{name}: {len(head)} barriers, expected {1 + nq} (prologue + {nq} slots)')
            continue
        for b in head[1:]:
            prev = next((code[j] for j in range(b - 1, -1, -1) if code[j].startswith('s_waitcnt')), '')
            w = re.search(r'vmcnt\((\d+)\)', prev)
            if not w or int(w.group(1)) not in (6, 8):
                problems.append(f'{name}: slot barrier preceded by `{prev}`, expected the counted wait vmcnt(6) / vmcnt(8)')
        for k in range(nq):
            lo, hi = head[k], head[k + 1]
            seg = code[lo:hi]
            dma = [i for i, l in enumerate(seg) if l.startswith('global_load_lds_dwordx4')]
            xl = [i for i, l in enumerate(seg) if l.startswith('global_load_dwordx4')]
            if len(dma) != 6:
                problems.append(f'{name}: slot {k}: {len(dma)} DMA units, expected 6')
            if xl and dma and min(xl) < max(dma):
                problems.append(f'{name}: slot {k}: an X load issued in front of the slot\'s DMA units')
            if len(xl) not in (0, 2) or (k == 0) != (len(xl) == 2):
                problems.append(f'{name}: slot {k}: {len(xl)} X loads (expected 2 in the first slot of a chunk, 0 elsewhere)')
        meta = asm_text[m.end():m.end() + 6000]
        for key, limit in (('ScratchSize', 0), ('NumAgprs', 0), ('NumVgprs', 256)):
            v = re.search(r'; %s: (\d+)' % key, meta)
            if not v or int(v.group(1)) > limit:
                problems.append(f'{name}: {key} = {v.group(1) if v else "?"} (limit {limit})')
    want = {(nt, lg) for nt in range(9, 17) for lg in (0, 1)}
    if seen != want:
        problems.append(f'instances of k_compat_wide found: {sorted(seen)}, expected NT 9..16 x (softmax, logits)')
    return problems


def main():
    src = os.path.join(ROOT, 'depth-estimation_amd', 'csrc', 'phl_compat_wide.hip')
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'wide.s')
        cmd = ['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fPIC',
               '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.dirname(src), '-S', '--cuda-device-only', src, '-o', out]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        problems = check(open(out).read())
    for p in problems:
        print(p)
    print('k_compat_wide machine code:', 'FAILED' if problems else 'ok')
    return 1 if problems else 0


if __name__ == '__main__':
    sys.exit(main())
