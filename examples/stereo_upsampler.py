#!/usr/bin/env python3
"""The reference's upsampler head on one MI355X (crf/mb_stereo_crf.py: CRFdepthUpsampler), on the synthetic stereo pair of
examples/stereo_crf.py: the known disparity, reduced ``--factor`` times and with a block of missing measurements, and the
left image at full resolution go through the head's forward, then one training step follows on the device.

    E0, labels = phl.nchw_scalar_unaries(disp_lowres, (H, W), 18, gamma, s)      -> phl_nchw_scalar_unaries, two launches
    depth      = CRFasRNN(charb(.05), niters=2, r, gchannels=3).expected_depth(img, None, energies=E0, labels=labels, values=labels)

    python examples/stereo_upsampler.py [--h 288 --w 384 --r 8 --factor 8] [--fused-step] [--fused-unaries] [--full-cov [--full-cov-grad]] [--bilinear [--bilinear-grad | --full-cov --bilinear-full-grad]]

--fused-step runs the training step with ``CRFdepthUpsampler(fused_grad=True, fused_step=True)``: W on phl.GuidedFilterFn
and everything between two W calls on phl.NchwStepTrain.  --fused-unaries passes ``fused_unaries=True``: where the head
runs its torch prologue (PHL_SCALAR_UNARIES=0 in the environment), CRFasRNN's ``-logits * mask`` is phl.nchw_confidence_unaries
and under autograd phl.NchwConfidenceUnaries; behind the fused prologue, which hands E0 over itself, it changes nothing.
--full-cov gives W the full covariance of the RGB guide
(``CRFdepthUpsampler(full_cov=True)``): the forward on phl.guided_filter(full_cov=True), the training step on the torch form --
or, with --full-cov-grad (``full_cov_grad=True``), on phl.GuidedFilterFullFn, the model's backward kernels.  --bilinear
gives W ``mode='bilinear', fused_bilinear=True``: coefficients interpolated from the half-resolution solve instead of
repeated over 2 x 2 blocks, the forward on phl.guided_filter_bilinear, the training step on the torch form -- or, with --bilinear-grad
(``bilinear_grad=True``), on phl.GuidedFilterBilinearFn, the mode's backward kernels; with --bilinear --full-cov the switch is
--bilinear-full-grad (``bilinear_full_grad=True``): phl.GuidedFilterBilinearFullFn.

Prints the mean absolute disparity error of the plain bilinear enlargement and of the head's output against the known
disparity, and the loss before and after the step.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-estimation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from stereo_crf import synthetic_pair  # noqa: E402


def run(h=288, w=384, r=8, factor=8, device="cuda", quiet=False, fused_step=False, full_cov=False, full_cov_grad=False,
        bilinear=False, bilinear_grad=False, bilinear_full_grad=False, fused_unaries=False):
    import torch
    import torch.nn.functional as F

    from crf.mb_stereo_crf import CRFdepthUpsampler

    left, _, truth = synthetic_pair(h, w)
    dev = torch.device(device)
    img = torch.from_numpy(left).to(dev).permute(2, 0, 1)[None].contiguous()
    truth = torch.from_numpy(truth).to(dev).float()[None, None]
    low = F.interpolate(truth, size=(h // factor, w // factor), mode="bilinear", align_corners=False)
    low[:, :, 2:6, 3:9] = 0                                                   # no measurement there
    net = CRFdepthUpsampler(r=r, niters=2, fused_grad=fused_step, fused_step=fused_step, full_cov=full_cov,
                            full_cov_grad=full_cov_grad, mode="bilinear" if bilinear else "nearest", fused_bilinear=bilinear,
                            bilinear_grad=bilinear_grad, bilinear_full_grad=bilinear_full_grad,
                            fused_unaries=fused_unaries).to(dev)
    torch.cuda.synchronize()
    t0 = time.time()
    with torch.no_grad():
        depth = net((low, img, None))
    torch.cuda.synchronize()
    dt = time.time() - t0
    plain = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)
    err_plain, err_head = float((plain - truth).abs().mean()), float((depth - truth).abs().mean())

    # one training step: L1 loss, gradients for charb's gamma and s (phl.NchwScalarUnaries and the loop's Mu) and for W
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    loss = (net((low, img, None)) - truth).abs().mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    before = float(loss.detach())
    with torch.no_grad():
        after = float((net((low, img, None)) - truth).abs().mean())
    if not quiet:
        print(f"{w}x{h} from {w // factor}x{h // factor}, 18 labels, guided-filter radius {r}: forward {dt * 1e3:.1f} ms on the device")
        print(f"mean |disparity error|: bilinear enlargement {err_plain:.3f} px, CRFdepthUpsampler {err_head:.3f} px")
        if fused_step:
            print("training step with fused_step=True: W, Mu and the softmax on the HIP kernels under autograd")
        print(f"one SGD step: loss {before:.4f} -> {after:.4f}; gamma.grad = {float(net.CRF.Mu.gamma.grad):.4g}, "
              f"s.grad = {float(net.CRF.Mu.s.grad):.4g}")
    return err_plain, err_head, before, after


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=288)
    ap.add_argument("--w", type=int, default=384)
    ap.add_argument("--r", type=int, default=8)
    ap.add_argument("--factor", type=int, default=8)
    ap.add_argument("--fused-step", action="store_true", help="the training step on phl.NchwStepTrain / phl.GuidedFilterFn")
    ap.add_argument("--fused-unaries", action="store_true",
                    help="-logits * confidence on phl.nchw_confidence_unaries (the head's torch prologue: PHL_SCALAR_UNARIES=0)")
    ap.add_argument("--full-cov", action="store_true", help="W with the full covariance of the RGB guide")
    ap.add_argument("--full-cov-grad", action="store_true", help="with --full-cov: train that W on phl.GuidedFilterFullFn")
    ap.add_argument("--bilinear", action="store_true", help="W interpolates its coefficients (mode='bilinear', fused_bilinear=True)")
    ap.add_argument("--bilinear-grad", action="store_true", help="with --bilinear: train that W on phl.GuidedFilterBilinearFn")
    ap.add_argument("--bilinear-full-grad", action="store_true",
                    help="with --bilinear --full-cov: train that W on phl.GuidedFilterBilinearFullFn")
    a = ap.parse_args()
    kw = dict(fused_step=a.fused_step, full_cov=a.full_cov, full_cov_grad=a.full_cov_grad, bilinear=a.bilinear,
              bilinear_grad=a.bilinear_grad, bilinear_full_grad=a.bilinear_full_grad, fused_unaries=a.fused_unaries)
    run(a.h, a.w, a.r, a.factor, **kw)     # first run of the process: library load, first launches, first allocations
    t1 = time.time()
    run(a.h, a.w, a.r, a.factor, quiet=True, **kw)
    print(f"the same again, warm: {(time.time() - t1) * 1e3:.1f} ms end to end (synthetic pair generated on the CPU included)")
