"""Stereo refinement / upsampling heads built on CRFasRNN, mirroring the nn.Modules of the
reference's crf/mb_stereo_crf.py (:62-66 logits2average_depth, :68-102 CRFdepthRefiner and
CRFwUncertainty, :138-163 CRFdepthUpsampler).  API surface only: the reference instantiates them
with the guided-filter W (out of the lattice scope); ``lattice=True`` switches W to the
permutohedral BatchedAdjacency.  The other engine keywords (_ENGINE_KEYWORDS) go to CRFasRNN as they are; those of the
guided-filter W have their table in crf.guided._guided_route (``full_cov=True`` takes up to four guide channels on the
kernels, the upsampler's RGB guide among those).  The trainer classes (:14-60, :105-136) and ``__main__`` need the
un-vendored ``oil`` package and Middlebury data and are not mirrored."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from crf import crf_module
from crf.crf_module import CRFasRNN, charb


def logits2average_depth(logits, labels=None):
    """Expected label under softmax(logits): [bs, L, h, w] -> [bs, 1, h, w] (:62-66).

    fp32 CUDA logits with one label value per channel (crf_module._expect_routable) are one kernel that reads the logits
    once (phl.nchw_expected_value; phl.NchwExpectedValue when the logits ask for a gradient).  Everything else -- CPU,
    float64, labels per pixel or asking for a gradient, PHL_NCHW_STEP=0 -- is the torch lines below."""
    if crf_module._expect_routable(logits, labels):
        import phl

        if torch.is_grad_enabled() and logits.requires_grad:
            return phl.nchw_expected_value_fn(logits, None, labels, False)
        return phl.nchw_expected_value(logits, labels=labels, negate=False)
    probs = F.softmax(logits, dim=1)
    if labels is None:
        labels = torch.arange(probs.shape[1], dtype=torch.float32, device=probs.device)[None, :, None, None]
    return (probs * labels).sum(1, keepdim=True)


class _CoordConv(nn.Module):
    """3x3 convolution that also sees the normalised (i, j) pixel coordinates (stands in for the
    reference's oil ``conv2d(..., coords=True)``)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin + 2, cout, 3, padding=1)

    def forward(self, x):
        bs, _, h, w = x.shape
        ii = torch.linspace(-1, 1, h, device=x.device)[None, None, :, None].expand(bs, 1, h, w)
        jj = torch.linspace(-1, 1, w, device=x.device)[None, None, None, :].expand(bs, 1, h, w)
        return self.conv(torch.cat([x, ii, jj], dim=1))


# The keywords that the heads hand on to CRFasRNN as they are: its W and its routes (crf_module.CRFasRNN, crf.guided).
_ENGINE_KEYWORDS = ("lattice", "fused_grad", "fused_step", "full_cov", "full_cov_grad", "mode", "fused_bilinear", "bilinear_grad",
                    "bilinear_full_grad", "fused_unaries")


def _engine(args):
    """The CRFasRNN of a head, from the arguments of the head's constructor (its ``locals()``)."""
    return CRFasRNN(charb(args["gamma"]), niters=args["niters"], r=args["r"], eps=args["eps"], gchannels=args["d_guide"],
                    **{k: args[k] for k in _ENGINE_KEYWORDS})


class CRFdepthRefiner(nn.Module):
    def __init__(self, d_in=64, d_guide=16, r=15, niters=2, eps=1e-2, gamma=.05, lattice=False, fused_grad=False, fused_step=False,
                 full_cov=False, full_cov_grad=False, mode="nearest", fused_bilinear=False, bilinear_grad=False, *,
                 bilinear_full_grad=False, fused_unaries=False):
        super().__init__()
        self.CRF = _engine(locals())
        self.projection = nn.Conv2d(d_in, d_guide - 3, kernel_size=1)

    def _guide(self, imgrgb, features):
        return torch.cat((imgrgb, self.projection(features)), dim=1)

    def forward(self, inputs):
        logits, imgrgb, features = inputs
        return self.CRF.expected_depth(self._guide(imgrgb, features), logits)


class CRFwUncertainty(CRFdepthRefiner):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.uncertainty_net = nn.Sequential(_CoordConv(3, 16), nn.GroupNorm(4, 16), nn.ReLU(),
                                             _CoordConv(16, 16), nn.GroupNorm(4, 16), nn.ReLU(),
                                             _CoordConv(16, 1))          # log sigma, bs x 1 x h x w

    def forward(self, inputs):
        logits, imgrgb, features = inputs
        confidence = torch.exp(-self.uncertainty_net(imgrgb))
        return self.CRF.expected_depth(self._guide(imgrgb, features), logits, confidence), confidence


# PHL_SCALAR_UNARIES=0 keeps the upsampler's prologue on its torch lines (read once).  A switch of its own: the prologue
# is the same whether the loop behind it runs fused or plain (crf_module._NCHW_STEP).
_SCALAR_UNARIES = os.environ.get("PHL_SCALAR_UNARIES", "1") not in ("", "0")


def _scalar_unaries_routable(disp, mu):
    """What phl.nchw_scalar_unaries computes in place of CRFdepthUpsampler's prologue: a non-empty fp32 CUDA [B, 1, h, w]
    disparity that asks for no gradient (the kernel has none for it), and a ``charb`` Mu whose gamma and s are fp32 on the
    disparity's device."""
    if not (_SCALAR_UNARIES and torch.is_tensor(disp) and disp.is_cuda and disp.dtype == torch.float32 and disp.dim() == 4
            and disp.shape[1] == 1 and disp.numel() > 0 and not disp.requires_grad and isinstance(mu, charb)):
        return False
    return all(p.dtype == torch.float32 and p.device == disp.device and p.numel() == 1 for p in (mu.gamma, mu.s))


class CRFdepthUpsampler(nn.Module):
    def __init__(self, d_in=64, d_guide=3, r=15, niters=2, eps=1e-2, gamma=.05, lattice=False, fused_grad=False, fused_step=False,
                 full_cov=False, full_cov_grad=False, mode="nearest", fused_bilinear=False, bilinear_grad=False, *,
                 bilinear_full_grad=False, fused_unaries=False):
        super().__init__()
        self.CRF = _engine(locals())

    def forward(self, inputs):
        """fp32 CUDA inputs (_scalar_unaries_routable) get E0 and the labels from phl.nchw_scalar_unaries -- two launches,
        no read-back -- and hand E0 to the CRF as it is; under autograd phl.NchwScalarUnaries gives gamma and s their
        gradients.  Everything else is the torch lines below."""
        disp_lowres, img_highres, _ = inputs
        if _scalar_unaries_routable(disp_lowres, self.CRF.Mu):
            import phl

            mu = self.CRF.Mu
            fn = phl.nchw_scalar_unaries_fn if torch.is_grad_enabled() and (mu.gamma.requires_grad or mu.s.requires_grad) \
                else phl.nchw_scalar_unaries
            E0, labels = fn(disp_lowres, img_highres.shape[2:], 18, mu.gamma, mu.s)
            return self.CRF.expected_depth(img_highres, None, energies=E0, labels=labels, values=labels)
        up = F.interpolate(disp_lowres, size=img_highres.shape[2:], mode="bilinear", align_corners=False)
        labels = torch.linspace(0, float(up.max()), 18, device=up.device)
        logits = -10 * self.CRF.Mu.get_energies_from_scalar(up, labels[None, :, None, None])
        confidence = (up > 1e-2).float()
        return self.CRF.expected_depth(img_highres, logits, confidence=confidence, labels=labels, values=labels)
