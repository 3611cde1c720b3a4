"""Golden vectors for the differentiable CRFasRNN path: one backward pass of the reference's own
``CRFasRNN(charb(3.0), niters=3)`` (crf_module.py:81-104) with the lattice W (``gm.BatchedAdjacency``) over the reference
engine, on two Tsukuba crops of 20 x 24 with L = 32 -- the recipe of generate.py's crfasrnn_nchw case, whose helpers this
script imports (generate.py itself is not changed).

    python tests/golden/generate_train.py      -> tests/golden/crfasrnn_train.npz

The guide is a TRAINABLE ijrgbGuide, so the reference's BatchedLatticeFilter takes its ref-gradient branch
(gaussian_matrix.py:395-419) rather than its source-only one.  Stored: the inputs (logits, img, labels), a fixed upstream
gradient g_out of the output logits, the output, and the gradients of the logits, charb.gamma, charb.s, s_ij and s_rgb."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import generate as gen  # noqa: E402


def crfasrnn_train():
    import torch

    torch.manual_seed(5)
    torch.set_num_threads(1)
    crf_module, gm = gen.import_reference_python()
    imL = gen.read_image(os.path.join(gen.REFERENCE, "Experiments", "imL.png"))
    g_ = torch.Generator().manual_seed(777)
    bs, L, hh, ww = 2, 32, 20, 24
    img = torch.from_numpy(np.stack([imL[60:60 + hh, 100:100 + ww], imL[150:150 + hh, 220:220 + ww]]).transpose(0, 3, 1, 2)).float()
    logits = (torch.randn(bs, L, hh, ww, generator=g_) * 2.0).requires_grad_(True)
    g_out = torch.randn(bs, L, hh, ww, generator=g_)
    lab = torch.arange(L).float()
    net = crf_module.CRFasRNN(crf_module.charb(3.0), niters=3)
    net.W = gm.BatchedAdjacency(num_threads=2)          # the lattice alternative the reference imports (:5) but does not wire in
    guide = crf_module.ijrgbGuide(trainable=True)
    out = net(guide(img), logits, labels=lab)
    (out * g_out).sum().backward()
    np.savez_compressed(os.path.join(HERE, "crfasrnn_train.npz"), img=img.numpy(), logits=logits.detach().numpy(),
                        labels=lab.numpy(), gamma=np.float32(3.0), s_ij=np.float32(0.1), s_rgb=np.float32(0.1),
                        niters=np.int64(3), g_out=g_out.numpy(), out=out.detach().numpy(), grad_logits=logits.grad.numpy(),
                        grad_gamma=net.Mu.gamma.grad.numpy(), grad_s=net.Mu.s.grad.numpy(),
                        grad_s_ij=guide.s_ij.grad.numpy(), grad_s_rgb=guide.s_rgb.grad.numpy())
    print("wrote crfasrnn_train.npz", dict(gamma=float(net.Mu.gamma.grad), s=float(net.Mu.s.grad), s_ij=float(guide.s_ij.grad),
                                           s_rgb=float(guide.s_rgb.grad), logits=float(logits.grad.abs().max())))


if __name__ == "__main__":
    assert gen.po.build_reference(), "reference engine not built"
    crfasrnn_train()
