"""mean_field_infer end to end at the reference's full-resolution call shape: 2048 x 1536 pixels, max_disp = w // 6 = 341
labels (crf/depth.py:40; padded to 344 inside), Charbonnier Mu, 5 iterations -- with the compatibility step on the wide
split kernel (PHL_COMPAT_ARITH=split, the default) and on the library route (PHL_COMPAT_ARITH=f32: rocBLAS GEMM + fused
softmax, what this shape ran on before k_compat_wide), alternating, same process.  Prints wall-clock ms per call.
Usage: python tools/mf_wide_time.py [iters] [reps]"""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'depth-estimation_amd')); sys.path.insert(0, ROOT)
import bench
from crf.crf_module import charbonneir, compatibility_matrix, mean_field_infer
from crf.gaussian_matrix import LatticeGaussian

H, W = 1536, 2048
L = W // 6
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device('cuda')
ref = torch.from_numpy(bench.synthetic_features(H, W).reshape(-1, 5)).to(dev)
g = torch.Generator(device=dev).manual_seed(0)
E0 = torch.rand((H * W, L), device=dev, generator=g) * 10
labels = torch.arange(L, dtype=torch.float32, device=dev)
Mu = compatibility_matrix(lambda a, b: charbonneir(a, b, 3), labels)
Wop = LatticeGaussian(ref)


def run(arith):
    os.environ['PHL_COMPAT_ARITH'] = arith
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Q = mean_field_infer(E0, Wop, Mu, iters)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, Q


res = {'split': [], 'f32': []}
out = {}
for arith in ('split', 'f32'):                  # warm-up: lattice cache, Mu^T / planes caches, clocks
    run(arith)
for _ in range(reps):
    for arith in ('split', 'f32'):
        ms, out[arith] = run(arith)
        res[arith].append(ms)
diff = float((out['split'] - out['f32']).abs().max())
print(f"mean_field_infer {W}x{H}, L={L}, {iters} iterations: wide split kernel {min(res['split']):.1f} ms "
      f"(all {[round(x, 1) for x in res['split']]}), library route {min(res['f32']):.1f} ms "
      f"(all {[round(x, 1) for x in res['f32']]}); max |Q_split - Q_f32| = {diff:.2e}")
