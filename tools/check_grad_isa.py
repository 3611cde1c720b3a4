"""Static check of the backward kernels' machine code (phl_compat_grad.hip; hipcc -S, no GPU needed).

For every kernel of phl_compat_grad.hip (k_softmax_neg_grad in all its instances, k_compat_grad_x, k_compat_grad_mu,
k_compat_grad_mu_sum) this script verifies:
  * no scratch;
  * the register budget of its launch: VGPRs + AGPRs within what its workgroup size allows one workgroup per CU
    (k_compat_grad_mu: 1024 threads = four waves per SIMD, 128 registers; the others: 256 threads, 256 registers);
  * no float atomics (global_atomic_*_f32 / _f64, buffer_atomic_*_f32 / _f64): the weight gradient is reduced in a
    fixed order, so it is the same bit for bit on every run;
  * the products run on the f32-input matrix cores (v_mfma_f32_16x16x4_f32 in k_compat_grad_x and k_compat_grad_mu).
Exit code 0 = ok.  Used by tests/test_compat_grad_host.py."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_softmax_neg_grad": 256, "k_compat_grad_x": 256, "k_compat_grad_mu": 128, "k_compat_grad_mu_sum": 256}
MFMA = ("k_compat_grad_x", "k_compat_grad_mu")


def check(asm_text):
    problems, seen = [], {}
    for m in re.finditer(r'^(_Z\S*?(k_softmax_neg_grad|k_compat_grad_mu_sum|k_compat_grad_mu|k_compat_grad_x)\S*):[^\n]*\n(.*?)\.end_amdhsa_kernel',
                         asm_text, re.S | re.M):
        name, kern, body = m.group(1), m.group(2), m.group(3)
        seen[kern] = seen.get(kern, 0) + 1
        code = [l.strip() for l in body.split('\n')]
        code = [l for l in code if l and l[0] not in ';.' and not l.endswith(':')]
        atom = [l for l in code if re.match(r'(global|buffer|flat)_atomic_\w*_f(32|64)\b', l)]
        if atom:
            problems.append(f'{name}: float atomics: {atom[:2]}')
        if kern in MFMA and not any(l.startswith('v_mfma_f32_16x16x4') for l in code):
            problems.append(f'{name}: no v_mfma_f32_16x16x4_f32')
        meta = asm_text[m.end():m.end() + 6000]
        vals = {}
        for key in ('ScratchSize', 'NumVgprs', 'NumAgprs'):
            v = re.search(r'; %s: (\d+)' % key, meta)
            vals[key] = int(v.group(1)) if v else None
        if vals['ScratchSize'] != 0:
            problems.append(f'{name}: ScratchSize = {vals["ScratchSize"]}')
        regs = (vals['NumVgprs'] or 0) + (vals['NumAgprs'] or 0)
        if vals['NumVgprs'] is None or regs > KERNELS[kern]:
            problems.append(f'{name}: {regs} VGPR+AGPR (limit {KERNELS[kern]})')
    for kern in KERNELS:
        if kern not in seen:
            problems.append(f'{kern}: not found in the code object')
    if seen.get('k_softmax_neg_grad', 0) != 8:
        problems.append(f'k_softmax_neg_grad: {seen.get("k_softmax_neg_grad", 0)} instances, expected 8 (NV 1, 2 x logits x uniform)')
    return problems


def main():
    src = os.path.join(ROOT, 'depth-estimation_amd', 'csrc', 'phl_compat_grad.hip')
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'grad.s')
        cmd = ['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fPIC',
               '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.dirname(src), '-S', '--cuda-device-only', src, '-o', out]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        problems = check(open(out).read())
        if '-v' in sys.argv:
            text = open(out).read()
            for m in re.finditer(r'^(_Z\S*k_\w+?\S*):[^\n]*\n.*?\.end_amdhsa_kernel', text, re.S | re.M):
                meta = text[m.end():m.end() + 6000]
                v = {k: re.search(r'; %s: (\d+)' % k, meta) for k in ('NumVgprs', 'NumAgprs', 'ScratchSize', 'Occupancy')}
                print(m.group(1), {k: (x.group(1) if x else '?') for k, x in v.items()})
    for p in problems:
        print(p)
    print('phl_compat_grad.hip machine code:', 'FAILED' if problems else 'ok')
    return 1 if problems else 0


if __name__ == '__main__':
    sys.exit(main())
