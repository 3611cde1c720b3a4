"""Dense-CRF mean-field inference, mirroring the reference's crf/crf_module.py.

    Q <- softmax(-E0);  repeat niters:  E <- E0 + (W @ Q) @ Mu;  Q <- softmax(-E)

``W`` is any object with ``@`` -- for the lattice path a crf.gaussian_matrix.LatticeGaussian,
whose product is one splat -> blur -> slice on the MI355X lattice built ONCE for the fixed
reference features (the reference rebuilds it on every iteration).
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import phl
from crf.gaussian_matrix import BatchedAdjacency, BatchedGuidedAdjacency  # noqa: F401  (crf_module.py:5)
from crf.guided import _check_guided_keywords


def gaussian_weights_u(f):
    """Dense brute-force W = exp(-|fi-fj|^2) - I for tiny n (crf_module.py:17-20)."""
    sq = torch.cdist(f, f).pow(2)
    return torch.exp(-sq) - torch.eye(f.shape[0], device=f.device, dtype=f.dtype)


def gaussian_weights(f):
    """Symmetrically normalised version of gaussian_weights_u, minus I (crf_module.py:8-15)."""
    W = gaussian_weights_u(f)
    s = W.sum(1).rsqrt()
    return s[:, None] * W * s[None, :] - torch.eye(f.shape[0], device=f.device, dtype=f.dtype)


def lazy_W(f):
    """Row generator of the normalised dense affinity for an [h, w, c] numpy image (crf_module.py:22-30)."""
    def W(i, j):
        a = np.exp(-((f - f[i, j]) ** 2).sum(-1).reshape(-1))
        a = a / np.sqrt(a.sum() - 1)
        return a.reshape(f.shape[:2])
    return W


def charbonneir(a, b, gamma=.1):
    """Charbonnier label compatibility sqrt(gamma^2 + (a-b)^2) - gamma (crf_module.py:32-33)."""
    return torch.sqrt(gamma ** 2 + (a - b) ** 2) - gamma


def charbonneir2(a, b, gamma=3):
    return torch.sqrt(1 + ((a - b) / gamma) ** 2) - 1


def compatibility_matrix(compat, labels):
    """Mu[a, b] = compat(labels[a], labels[b]) (crf_module.py:38-39)."""
    return compat(labels[:, None], labels[None, :])


# ---- label counts the fused kernels cannot take as they are ------------------------------------------------------
# The reference takes max_disp = w // 6 (crf/depth.py:40): 231 labels at Middlebury's 1390 columns, 341 at 2048 -- rows
# that are not made of 16-byte pieces.  The device loop then runs on L rounded up (to a multiple of 4; to 256 when that is
# 32 labels away at most): the extra labels get an energy nothing else reaches, so their probability is exactly 0 in every
# iteration (exp underflows), their rows and columns of Mu are 0, W maps a zero column to a zero column -- the first L
# columns evolve exactly as without them.  One padded copy of E_0 on entry, one slice on exit.
_PAD_ENERGY = 1.0e30


def _label_pad(L):
    if L % 4 == 0:
        return L
    return 256 if 224 < L < 256 else (L + 3) // 4 * 4


def _pad_labels(E_0, Mu, differentiable=False, channel_major=False, structure=True):
    """(E_0, Mu, uniform) on the label count of the device loop (_label_pad): the energies of the extra labels are
    _PAD_ENERGY, Mu gets zero rows / columns, and uniform is the Potts-family structure of the ORIGINAL Mu (or False) for
    phl.compat_softmax -- None when nothing is padded.  E_0 [..., n, L] and Mu [L, L].
    differentiable: through autograd (F.pad: fresh tensors, Mu's graph kept); structure=False then skips the
    Potts-family test and its device -> host read (uniform None), for a caller that does not run phl.compat_softmax.
    Otherwise one padded copy of E_0 and the padded Mu cached per Mu (phl._mu_forms); channel_major: E_0 is an image's
    [L, n] (NCHW) plane, always transposed into a fresh pixel-major buffer by phl.copy2d."""
    L = E_0.shape[0] if channel_major else E_0.shape[-1]
    Lp = _label_pad(L)
    if differentiable:
        if Lp == L:
            return E_0, Mu, None
        uniform = (phl._mu_uniform(Mu.detach()) or False) if structure else None
        return F.pad(E_0, (0, Lp - L), value=_PAD_ENERGY), F.pad(Mu, (0, Lp - L, 0, Lp - L)), uniform
    if Lp == L and not channel_major:
        return E_0, Mu, None
    n = E_0.shape[1] if channel_major else E_0.shape[0]
    E0p = torch.empty((n, L), dtype=torch.float32, device=E_0.device) if Lp == L else \
        torch.full((n, Lp), _PAD_ENERGY, dtype=torch.float32, device=E_0.device)
    if channel_major:
        phl.copy2d(E0p[:, :L], E_0.t())
    else:
        E0p[:, :L] = E_0
    if Lp == L:
        return E0p, Mu, None
    return (E0p,) + phl._mu_forms(Mu).padded(Lp, E_0.device)


def _fused_ok(E_0, Mu):
    return (E_0.is_cuda and E_0.dtype == torch.float32 and E_0.dim() == 2 and E_0.stride(1) == 1
            and not (torch.is_grad_enabled() and (E_0.requires_grad or Mu.requires_grad)))


def _kernel_operand(X, device):
    """X as the fused kernels read it: a fp32 [n, L] device tensor with unit channel stride."""
    if X.is_cuda and X.dtype == torch.float32 and X.stride(1) == 1:
        return X
    return X.to(device, torch.float32).contiguous()


def mean_field_step(E_0, W, Mu, Q, out=None):
    """One iteration ``softmax(-(E_0 + (W @ Q) @ Mu))`` (crf_module.py:51-52) on the fused device path.

    ``W`` is an operator (``@``) or a callable.  The raw-pointer kernels below know nothing of autograd, so
    the caller must have established that no gradient flows (``mean_field_infer`` does)."""
    X = W(Q) if callable(W) and not hasattr(W, "__matmul__") else W @ Q
    return phl.compat_softmax(E_0, _kernel_operand(X, E_0.device), Mu, out=out)


def _device_loop(E_0, apply_W, Mu, niters, uniform=None, differentiable=False, logits=False, fused_grad=False):
    """``niters`` iterations Q <- softmax(-(E_0 + X @ Mu)), X = apply_W(Q), on the fused kernels from Q = softmax(-E_0).
    E_0, Mu, uniform: from _pad_labels.  logits: the last iteration returns -(E_0 + X @ Mu) instead.

    differentiable=False: the raw-pointer kernels, in place (out=Q): nothing is allocated per iteration.  When X first
    carries a graph (W itself is being differentiated), the raw-pointer kernels would drop it and overwrite a tensor W
    saved for backward: from there on the loop continues on the differentiable Functions (fused_grad) or on plain torch
    ops.  differentiable=True: phl.SoftmaxNegAdd / phl.CompatSoftmax, every tensor fresh -- nothing autograd saved is
    written again."""
    plain = False
    Q = phl.softmax_neg_add_fn(E_0) if differentiable else phl.softmax_neg_add(E_0)
    for it in range(niters):
        X = apply_W(Q)
        if not differentiable and torch.is_grad_enabled() and X.requires_grad:
            differentiable, plain = True, not fused_grad
        last = logits and it == niters - 1
        if plain:
            Q = -(E_0 + X @ Mu) if last else F.softmax(-(E_0 + X @ Mu), dim=1)
        elif differentiable:
            Q = phl.compat_softmax_fn(E_0, _kernel_operand(X, E_0.device), Mu, last, uniform)
        else:
            Q = phl.compat_softmax(E_0, _kernel_operand(X, E_0.device), Mu, out=Q, logits=last, uniform=uniform)
    return Q


def _fused_infer(E_0, apply_W, Mu, niters, differentiable=False, fused_grad=False):
    """_device_loop on the padded label count, Q [n, L] back."""
    L = E_0.shape[1]
    E0p, Mp, uniform = _pad_labels(E_0, Mu, differentiable)
    Q = _device_loop(E0p, apply_W, Mp, niters, uniform, differentiable, fused_grad=fused_grad and E0p.shape[1] <= 512)
    return Q if E0p.shape[1] == L else Q[:, :L].contiguous()


def mean_field_infer(E_0, W, Mu, niters=10, fused_grad=False):
    """[E_0] n x L unaries, [W] n x n operator, [Mu] L x L compatibility -> Q n x L (crf_module.py:41-53).

    On the GPU inference path everything of an iteration outside the lattice filter -- the compatibility
    product, the add, the negation and the softmax -- is ONE fused HIP kernel (phl.compat_softmax: fp32 MFMA
    tiles of X @ Mu with the softmax as epilogue, so neither G nor E ever exists in HBM).  With autograd
    (E_0, Mu, or anything W carries -- e.g. a LatticeGaussian whose ``ref`` requires grad) or CPU tensors
    the plain, differentiable torch ops run -- unless ``fused_grad=True``: then CUDA fp32 inputs keep the fused
    kernels under autograd too (phl.CompatSoftmax / phl.SoftmaxNegAdd, whose backward runs on the library's own
    kernels), and ``W @ Q`` keeps its own graph.  Without any gradient, ``fused_grad`` changes nothing."""
    differentiable = fused_grad and _fused_grad_ok(E_0, Mu)
    if differentiable or _fused_ok(E_0, Mu):
        return _fused_infer(E_0 if E_0.stride(1) == 1 else E_0.contiguous(), lambda Q: W @ Q, Mu, niters, differentiable,
                            fused_grad)
    if _staged_ok(E_0, W, Mu):
        return _mean_field_infer_staged(E_0, W, Mu, niters)
    Q = F.softmax(-E_0, dim=1)
    for _ in range(niters):
        Q = F.softmax(-(E_0 + (W @ Q) @ Mu), dim=1)
    return Q


def _fused_grad_ok(E_0, Mu):
    """The differentiable device loop: CUDA fp32 [n, L] unaries (at most 512 labels: the backward kernels' range), a fp32
    Mu, and a gradient asked of E_0 or Mu (a gradient that only W asks for is found in the device loop, at its first
    ``W @ Q``)."""
    return (E_0.is_cuda and E_0.dtype == torch.float32 and E_0.dim() == 2 and torch.is_tensor(Mu) and Mu.dtype == torch.float32
            and Mu.is_cuda and _label_pad(E_0.shape[1]) <= 512 and torch.is_grad_enabled() and (E_0.requires_grad or Mu.requires_grad))


def _staged_ok(E_0, W, Mu):
    """The notebook's own call shape (Experiments/DenseCrf.ipynb:142-152,173: CPU tensors, W = LatticeGaussian(ref) on
    the CPU, no autograd) -- everything the device loop needs can be staged once."""
    from crf.gaussian_matrix import LatticeGaussian

    if not (type(W) is LatticeGaussian and torch.is_tensor(W.ref) and torch.cuda.is_available()):
        return False
    no_grad = not (torch.is_grad_enabled() and (E_0.requires_grad or Mu.requires_grad or W.ref.requires_grad))
    return (no_grad and not E_0.is_cuda and E_0.dtype == torch.float32 and E_0.dim() == 2 and W.ref.dtype == torch.float32
            and Mu.dtype == torch.float32 and W.ref.dim() == 2 and W.ref.shape[0] == E_0.shape[0])


def _mean_field_infer_staged(E_0, W, Mu, niters):
    """CPU tensors in, CPU tensor out, the iterations on the device: E_0 crosses PCIe once (pinned pieces, phl.to_device),
    the lattice of ``W.ref`` is built once (cached per ``ref``), every iteration is one lattice filter with ``- Q`` fused
    and one fused compatibility + softmax kernel, and Q crosses PCIe once at the end -- instead of Q making the round
    trip inside every ``W @ Q`` with the compatibility product and the softmax on the host."""
    dev = W.ref.device if W.ref.is_cuda else torch.device("cuda", torch.cuda.current_device())
    lat = phl.lattice_for(W.ref.detach())                 # CPU ref: built on the current device; GPU ref: where it lives
    E0d = phl.to_device(E_0.detach().contiguous(), dev)
    X = torch.empty((E0d.shape[0], _label_pad(E0d.shape[1])), dtype=torch.float32, device=dev)
    Q = _fused_infer(E0d, lambda Q: lat.filter(Q, subtract_input=True, out=X), Mu.detach(), niters)
    return phl.to_host(Q)


def potts(num_classes):
    """1x1 conv holding the Potts compatibility 1 - I (crf_module.py:55-64)."""
    conv = nn.Conv2d(num_classes, num_classes, kernel_size=1, bias=False)
    with torch.no_grad():
        conv.weight.copy_((1 - torch.eye(num_classes))[..., None, None])
    return conv


def _mu_is_matrix(mu, L):
    """Whether ``mu`` is a compatibility module that is an [L, L] matrix: ``charb``, or a bias-free 1x1 conv (``potts``)."""
    return isinstance(mu, charb) or (isinstance(mu, nn.Conv2d) and mu.kernel_size == (1, 1) and mu.bias is None
                                     and mu.groups == 1 and mu.weight.shape[:2] == (L, L))


def _compat_matrix(mu, L, labels, device, detach=True):
    """[L, L] matrix M with ``mu(Q)[:, c] = sum_b M[b, c] Q[:, b]`` for a ``mu`` that is one (_mu_is_matrix); None for
    anything else.  detach=False keeps the graph to the module's parameters (the differentiable path of CRFasRNN)."""
    if not _mu_is_matrix(mu, L):
        return None
    if isinstance(mu, charb):
        return mu.matrix(L, labels, device, detach=detach)
    w = mu.weight.detach() if detach else mu.weight
    return w[:, :, 0, 0].t().to(device, torch.float32)          # conv: out[c] = sum_b w[c, b] q[b]


def _maybe_learnable(value, trainable):
    """A scalar hyper-parameter: nn.Parameter when it is to be trained, the plain number otherwise
    (the reference's ``nn.Parameter(torch.tensor(v)) if trainable else v`` idiom, crf_module.py:109-110)."""
    return nn.Parameter(torch.tensor(value)) if trainable else value


class charb(nn.Module):
    """Learnable Charbonnier compatibility applied as a 1x1 conv over label channels
    (crf_module.py:66-79): Mu(Q) = conv(Q, charbonneir(l_a, l_b, gamma)) * exp(s).
    Parameter names (``gamma``, ``s``) are the reference's, so its checkpoints load."""

    def __init__(self, gamma):
        super().__init__()
        self.register_parameter("gamma", nn.Parameter(torch.tensor(gamma)))
        self.register_parameter("s", nn.Parameter(torch.tensor(0.)))

    def _scale(self):
        return torch.exp(self.s)

    def forward(self, x, labels=None):
        if labels is None:          # the reference builds them with .cuda(); here they follow the input
            labels = torch.arange(x.shape[1], dtype=torch.float32, device=x.device)
        weight = compatibility_matrix(lambda p, q: charbonneir(q, p, self.gamma), labels)     # symmetric in (p, q)
        return F.conv2d(x, weight[..., None, None]) * self._scale()

    def matrix(self, L, labels=None, device=None, detach=True):
        """The same compatibility as a dense [L, L] matrix for pixel-major data: forward(x)[:, c] = (x @ M)[:, c].
        detach=False keeps the graph to ``gamma`` and ``s``."""
        if labels is None:
            labels = torch.arange(L, dtype=torch.float32, device=device)
        weight = compatibility_matrix(lambda p, q: charbonneir(q, p, self.gamma), labels.to(device))
        M = weight * self._scale()
        return (M.detach() if detach else M).t().contiguous()

    def get_energies_from_scalar(self, x, labels):
        return charbonneir(labels, x, self.gamma * labels.max()) * self._scale()


def _mean_field_nchw(E0, message, niters):
    """NCHW mean field: ``message(Q)`` returns the pairwise energy; gives the energy of the last iteration."""
    E, Q = E0, F.softmax(-E0, dim=1)
    for _ in range(niters):
        E = E0 + message(Q)
        Q = F.softmax(-E, dim=1)
    return E


# PHL_NCHW_STEP=0 keeps CRFasRNN's non-lattice W on the plain loop above (read once; the two loops side by side)
_NCHW_STEP = os.environ.get("PHL_NCHW_STEP", "1") not in ("", "0")


def _mean_field_nchw_step(E0, refs, W, niters, step, last):
    """The same iteration for any other W (the default guided filter), in the reference's order E = E0 + W(Mu(Q))
    (crf_module.py:97-99): ``Y = step(None, None)``, then per iteration ``G = W(Y, refs)`` and ``Y = step(G, Y)``, which
    may write over Y -- on the last one ``last(G)`` instead, which is what the loop gives.  Everything between two W
    calls -- the add, the negation, the softmax over the label channels and the compatibility product -- is the one
    channel-major kernel behind ``step``, so Q and E never exist in memory and nothing is transposed.  W is called once
    per iteration as the module it is, on whatever engine it picks, and keeps its own graph."""
    Y = step(None, None)
    for it in range(niters):
        G = W(Y, refs)
        if it == niters - 1:
            return last(G)
        Y = step(G, Y)


def _nchw_step_kernels(E0, M, uniform, expect, values):
    """(step, last) of _mean_field_nchw_step without autograd: phl.nchw_softmax_compat in place (out=Y: nothing is allocated
    per iteration), and the logits -(E0 + G) -- or with ``expect`` their expected label [B, 1, H, W] under ``values`` (None:
    0 .. L-1) straight from E0 and G, the logits never written.  uniform: M's Potts-family structure, or False."""
    if not uniform and M.shape[0] > phl.NCHW_PRODUCT_MAX_L:          # a general Mu above 256 labels: the 32-pixel tile
        step = lambda G, Y: phl.nchw_softmax_compat_wide(E0, G, M, out=Y)                      # noqa: E731
    else:
        step = lambda G, Y: phl.nchw_softmax_compat(E0, G, M, uniform=uniform, out=Y)          # noqa: E731
    if expect:
        return step, lambda G: phl.nchw_expected_value(E0, G, values, negate=True)
    return step, lambda G: phl.nchw_softmax_compat(E0, G, logits=True)


def _nchw_step_train_kernels(E0, M, expect, values):
    """(step, last) of _mean_field_nchw_step under autograd: phl.NchwStepTrain -- one kernel forward, one call backward (dE,
    and Mu's gradient through the differentiable M), which saves E0, G and M and nothing it computed, so no [B, L, H, W]
    intermediate of the step lives until the backward -- and the logits or phl.NchwExpectedValue, as above."""
    step = lambda G, Y: phl.nchw_step_train_fn(E0, G, M)                                       # noqa: E731
    if expect:
        return step, lambda G: phl.nchw_expected_value_fn(E0, G, values, True)
    return step, lambda G: -(E0 + G)


# The label ranges of the routes: each is the range of the kernels the route runs on.
_STEP_MAX_L = phl.NCHW_WIDE_MAX_L            # 512: the step route with a general Mu
_STEP_POTTS_MAX_L = phl.NCHW_UNIFORM_MAX_L   # 1024: the step route with a Mu of the Potts family
_STEP_GRAD_MAX_L = phl.NCHW_TRAIN_MAX_L      # 64: the step route under autograd
_LATTICE_GRAD_MAX_L = 512                    # the backward kernels of the lattice route, on _label_pad(L)


def _nchw_route(lattice, niters, e0_fp32_cuda, e0_4d, refs_fp32_cuda, grad, grad_w, fused_grad, fused_step, L, mu_matrix,
                mu_potts, step=True):
    """The route of one CRFasRNN call, from plain values:

        W        | preconditions                                                                         | route
        lattice  | niters > 0, E0 fp32 CUDA, no grad, Mu a matrix                                        | "lattice"
        lattice  | the same under grad, fused_grad, refs fp32 CUDA, _label_pad(L) <= 512                 | "lattice_grad"
        another  | step, niters > 0, E0 fp32 CUDA 4-D, no grad_w, Mu a matrix, L <= 512 (Potts: <= 1024) | "step"
        another  | the same head under grad_w, fused_step, L <= 64                                       | "step_grad"
        anything else                                                                                    | "plain"

    A lattice W (BatchedAdjacency) that misses its rows is "plain", never a step route.  grad: autograd records and E0,
    refs or a parameter of Mu asks for a gradient; grad_w: the same with W's parameters.  mu_potts decides only "step"
    between 513 and 1024 labels, so CRFasRNN._run reads it (phl._mu_uniform: one cached device -> host read per Mu) only
    where everything else already says "step".  step: the module switch _NCHW_STEP."""
    if not (niters > 0 and e0_fp32_cuda and mu_matrix):
        return "plain"
    if lattice:
        if not grad:
            return "lattice"
        return "lattice_grad" if fused_grad and refs_fp32_cuda and _label_pad(L) <= _LATTICE_GRAD_MAX_L else "plain"
    if not (step and e0_4d):
        return "plain"
    if not grad_w:
        return "step" if L <= (_STEP_POTTS_MAX_L if mu_potts else _STEP_MAX_L) else "plain"
    return "step_grad" if fused_step and L <= _STEP_GRAD_MAX_L else "plain"


def _expect_routable(logits, labels):
    """What phl.nchw_expected_value computes in place of ``(softmax(logits, 1) * labels).sum(1, keepdim=True)``: fp32 CUDA
    [B, L, H, W] logits, L >= 1, and labels that are None or a fp32 tensor on the logits' device with one value per label
    channel ([1, L, 1, 1] or [L, 1, 1]) that asks for no gradient.  PHL_NCHW_STEP=0 switches it off with the step."""
    if not (_NCHW_STEP and torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4
            and logits.shape[1] >= 1):
        return False
    if labels is None:
        return True
    L = logits.shape[1]
    return (torch.is_tensor(labels) and labels.dtype == torch.float32 and labels.device == logits.device
            and labels.dim() in (3, 4) and tuple(labels.shape[-3:]) == (L, 1, 1) and labels.numel() == L
            and not labels.requires_grad)


def _confidence_routable(logits, confidence):
    """What phl.nchw_confidence_unaries computes in place of ``-logits * confidence``: fp32 CUDA [B, L, H, W] logits and
    a fp32 [B, 1, H, W] confidence on the logits' device.  A scalar, a confidence per label, CPU tensors and float64 keep
    the torch line."""
    return (torch.is_tensor(logits) and torch.is_tensor(confidence) and logits.is_cuda and logits.dtype == torch.float32
            and logits.dim() == 4 and confidence.dtype == torch.float32 and confidence.device == logits.device
            and confidence.dim() == 4 and tuple(confidence.shape) == (logits.shape[0], 1) + tuple(logits.shape[2:]))


def _unaries(logits, confidence, fused):
    """E0 = -logits * confidence (crf_module.py:95-97).  fused (CRFasRNN's ``fused_unaries``) and _confidence_routable
    operands: one kernel that reads the logits once -- phl.NchwConfidenceUnaries where autograd records and the logits or
    the confidence ask for a gradient, which saves its two inputs and no ``-logits`` --, with the torch line's bits."""
    if confidence is None:
        return -logits
    if not (fused and _confidence_routable(logits, confidence)):
        return -logits * confidence
    if torch.is_grad_enabled() and (logits.requires_grad or confidence.requires_grad):
        return phl.nchw_confidence_unaries_fn(logits, confidence)
    return phl.nchw_confidence_unaries(logits, confidence)


_nchw_streams = {}


def _mean_field_nchw_fused(E0, refs, M, niters):
    """The same iteration for a lattice W, without autograd, the way the device wants it: one transpose to
    pixel-major [n, L] per image on entry, then per iteration ONE lattice filter with the ``- Q`` fused
    (phl_filter) and ONE fused compatibility-product + softmax kernel (phl_compat_softmax), and one transpose
    back at the end -- Q, G and E never make extra passes over HBM.  The reference evaluates
    W(Mu(Q)); here (W Q) Mu: W acts on pixels, Mu on labels, so they commute (fp32 rounding differs).

    Batch items are independent (the reference hands them to a process pool, gaussian_matrix.py:370-377): they are
    dealt over phl.batch_devices (the tensors' own GPU, or all GPUs with PHL_BATCH_DEVICES=all / CPU inputs), two
    side streams per device, so that image b+1's lattice build and transposes run under image b's iterations; both
    transposes go through the library's LDS-tiled phl_copy2d."""
    bs, L, h, w = E0.shape
    d = refs.shape[1]
    n = h * w
    if niters <= 0:
        return E0
    out = torch.empty_like(E0)
    home = E0.device
    devices = phl.batch_devices(E0)
    cur = torch.cuda.current_stream(home)
    used = []
    for b in range(bs):
        dev = devices[b % len(devices)]
        lane = (b // len(devices)) % 2
        st = _nchw_streams.get((dev, lane))
        if st is None:
            st = _nchw_streams[(dev, lane)] = torch.cuda.Stream(device=dev)
        st.wait_stream(cur)
        with torch.cuda.device(dev), torch.cuda.stream(st):
            e_b, r_b, Mb = E0[b], refs[b].detach(), M
            if dev != home:
                e_b, r_b, Mb = e_b.to(dev, non_blocking=True), r_b.to(dev, non_blocking=True), M.to(dev)
            e0, Mb, uniform = _pad_labels(e_b.reshape(L, n), Mb, channel_major=True)   # [L, n] channel-major -> [n, Lp]
            lat = phl.lattice_for(r_b.reshape(d, n).t(), device=dev)      # strided [n, d] view, no copy
            Q = _device_loop(e0, lambda Q: lat.filter(Q, subtract_input=True), Mb, niters, uniform, logits=True)
            if dev == home:
                phl.copy2d(out[b].reshape(L, n).t(), Q[:, :L])
            else:
                back = torch.empty((L, n), dtype=torch.float32, device=dev)
                phl.copy2d(back.t(), Q[:, :L])
                out[b].reshape(L, n).copy_(back, non_blocking=True)
            for t in (e0, Q, e_b, r_b):
                t.record_stream(st)
        used.append(st)
    for st in used:
        cur.wait_stream(st)
    return out


def _mean_field_nchw_grad(E0, refs, M, niters):
    """The NCHW iteration of CRFasRNN under autograd on the library's kernels, image by image pixel-major on the current
    stream: e0 = E0[b] as [n, L] (padded by _pad_labels where L is off the kernels' grid), Q = phl.SoftmaxNegAdd, then per
    iteration, in the reference's order E = E0 + W(Mu(Q)) (crf_module.py:97-99): Y = Q @ M (phl.CompatProduct, matrix
    cores), G = LatticeFilter(Y, ref_b) - Y with the guide's graph kept, Q = phl.SoftmaxNegAdd(e0, G) -- the logits
    -(e0 + G) on the last one -- and back to NCHW.  M is the differentiable compatibility matrix (gradients reach the Mu
    module).  W and Mu commute in the forward, not in the backward: the lattice filter is not exactly symmetric, its
    backward is the filter itself (LatticeFilter, as the reference's), so only this order gives Mu the reference's
    gradient; the (W Q) Mu order of mean_field_infer would give the exact gradient of the forward instead."""
    from crf.gaussian_matrix import LatticeFilter

    bs, L, h, w = E0.shape
    d, n = refs.shape[1], h * w
    E0p, Mp, _ = _pad_labels(E0.reshape(bs, L, n).transpose(1, 2), M, differentiable=True, structure=False)   # [bs, n, Lp]
    outs = []
    for b in range(bs):
        e0 = E0p[b].contiguous()
        ref_b = refs[b].reshape(d, n).t().contiguous()
        Q = phl.softmax_neg_add_fn(e0)
        for it in range(niters):
            Y = phl.compat_product_fn(Q, Mp)
            G = LatticeFilter.apply(Y, ref_b) - Y
            Q = -(e0 + G) if it == niters - 1 else phl.softmax_neg_add_fn(e0, G)
        outs.append(Q[:, :L].t().reshape(L, h, w))
    return torch.stack(outs)


class CRFasRNN(nn.Module):
    """Batched NCHW mean field (crf_module.py:81-104); returns logits -E of the LAST iteration.

    ``lattice=True`` selects the permutohedral W (BatchedAdjacency, the MI355X path); the default stays the reference's
    guided-filter W.  _nchw_route holds the table of routes: on fp32 CUDA tensors with a Mu that is a matrix (``charb``, a
    bias-free 1x1 conv), a call that autograd does not record runs on the fused kernels -- _mean_field_nchw_fused for the
    lattice W, _mean_field_nchw_step for any other (PHL_NCHW_STEP=0 in the environment switches that one off) -- and one
    it records does so on request: ``fused_grad=True`` for the lattice W (_mean_field_nchw_grad; it also puts the guided
    W itself on phl.GuidedFilterFn), ``fused_step=True`` for any other W.  ``full_cov``, ``full_cov_grad``, ``mode``,
    ``fused_bilinear``, ``bilinear_grad`` and ``bilinear_full_grad`` are the guided W's own keywords, handed on to it:
    crf.guided._guided_route holds the table of the routes they open, crf.guided._check_guided_keywords the rules between
    them.  Everything else -- CPU tensors, float64, another Mu, a label count out of a route's range -- is the plain NCHW
    loop, with the bits it always had.
    ``fused_unaries=True`` puts the unaries ``-logits * confidence`` of fp32 CUDA logits and a [B, 1, H, W] confidence
    (_confidence_routable) on phl.nchw_confidence_unaries, on every route and with the torch line's bits; recorded, on
    phl.NchwConfidenceUnaries, which keeps no ``-logits`` for the backward and sums the confidence's gradient in float64.
    ``expected_depth`` is ``logits2average_depth(forward(...))``, what every head of crf/mb_stereo_crf.py ends with; on
    the step routes the loop itself ends in the expected label, and the logits are never written."""

    def __init__(self, mu_init, niters=5, r=20, eps=1e-5, notrain_mu=False, gaussian=False, gchannels=1, lattice=False,
                 fused_grad=False, fused_step=False, full_cov=False, full_cov_grad=False, mode="nearest", fused_bilinear=False,
                 bilinear_grad=False, *, bilinear_full_grad=False, fused_unaries=False):
        super().__init__()
        guided = dict(full_cov=full_cov, full_cov_grad=full_cov_grad, mode=mode, fused_bilinear=fused_bilinear,
                      bilinear_grad=bilinear_grad, bilinear_full_grad=bilinear_full_grad)
        if lattice and (full_cov or mode != "nearest" or fused_bilinear or bilinear_grad or bilinear_full_grad):
            raise ValueError("CRFasRNN: full_cov, mode, fused_bilinear, bilinear_grad and bilinear_full_grad belong to the "
                             "guided-filter W; lattice=True has no covariance model and does not interpolate")
        # what a keyword needs; every other rule between the guided W's keywords is raised by its constructor
        _check_guided_keywords(**guided, needs_only=True)
        self.Mu, self.niters = mu_init, niters
        if notrain_mu:
            self.Mu.requires_grad_(False)
        # (fused_grad and the guided W: its box-window filter trains on phl.GuidedFilterFn; the Gaussian window has its own
        # backward, crf.guided.GaussianBlur, and ignores the flag)
        self.W = BatchedAdjacency() if lattice else BatchedGuidedAdjacency(gchannels, r, eps, gaussian=gaussian,
                                                                             fused_grad=fused_grad and not gaussian, **guided)
        self.fused_grad, self.fused_step, self.fused_unaries = fused_grad, fused_step, fused_unaries

    def forward(self, refs, logits, confidence=None, labels=None, energies=None):
        """refs [B, C, H, W], logits [B, L, H, W].  energies: the unaries E0 [B, L, H, W] themselves in place of
        ``-logits * confidence`` (logits and confidence must then be None), for a caller that has them already."""
        return self._run(refs, logits, confidence, labels, energies=energies)[0]

    def expected_depth(self, refs, logits, confidence=None, labels=None, values=None, energies=None):
        """``logits2average_depth(self(refs, logits, confidence, labels), values)`` [B, 1, H, W]: the expected value under
        the softmax of the returned logits.  values: None = 0 .. L-1, a tensor with one value per label ([L] or
        [1, L, 1, 1]), or anything ``probs * values`` broadcasts.  A tensor of fewer than four dimensions with exactly L
        elements always means one value per label -- also a [W] tensor when W == L, which ``probs * values`` alone would
        spread along the width; hand such values over as [1, 1, 1, W].  Where forward takes _mean_field_nchw_step, the
        loop itself ends with the expected value; everything else goes through forward.  energies: as in forward
        (``expected_depth(refs, None, energies=E0, ...)``)."""
        from crf.mb_stereo_crf import logits2average_depth

        unary = logits if energies is None else energies
        if torch.is_tensor(values) and values.dim() != 4 and values.numel() == unary.shape[1]:
            values = values.reshape(1, -1, 1, 1)
        out, done = self._run(refs, logits, confidence, labels, expect=_expect_routable(unary, values), values=values,
                              energies=energies)
        return out if done else logits2average_depth(out, values)

    def _run(self, refs, logits, confidence, labels, expect=False, values=None, energies=None):
        """(forward's logits, False) -- or, with ``expect`` on the _mean_field_nchw_step routes, (their expected label under
        ``values``, True).  energies: E0 itself, on every route.  Gathers what _nchw_route decides on, then dispatches."""
        if energies is not None and (logits is not None or confidence is not None):
            raise ValueError("CRFasRNN: energies are E0 itself; logits and confidence must be None with them")
        E0 = energies if energies is not None else _unaries(logits, confidence, self.fused_unaries)
        L, recording = E0.shape[1], torch.is_grad_enabled()
        grad = recording and (E0.requires_grad or refs.requires_grad or any(p.requires_grad for p in self.Mu.parameters()))
        facts = (isinstance(self.W, BatchedAdjacency), self.niters, E0.is_cuda and E0.dtype == torch.float32, E0.dim() == 4,
                 refs.is_cuda and refs.dtype == torch.float32, grad,
                 grad or (recording and any(p.requires_grad for p in self.W.parameters())), self.fused_grad, self.fused_step,
                 L, _mu_is_matrix(self.Mu, L))
        route = _nchw_route(*facts, mu_potts=True, step=_NCHW_STEP)
        if route in ("lattice", "lattice_grad"):                       # (every route but "plain" gives -E already)
            M = _compat_matrix(self.Mu, L, labels, E0.device, detach=route == "lattice")
            if route == "lattice":
                return _mean_field_nchw_fused(E0.contiguous(), refs, M, self.niters), False
            return _mean_field_nchw_grad(E0, refs, M, self.niters), False
        if route in ("step", "step_grad"):
            M = _compat_matrix(self.Mu, L, labels, E0.device, detach=route == "step")
            if route == "step":
                uniform = phl._mu_uniform(M) or False                  # the route's one read of Mu's structure, cached per Mu
                route = _nchw_route(*facts, mu_potts=bool(uniform), step=_NCHW_STEP)     # a general Mu above 512 labels: "plain"
            if route == "step":
                E0 = E0.contiguous()
                kernels = _nchw_step_kernels(E0, M, uniform, expect, values)
            elif route == "step_grad":
                kernels = _nchw_step_train_kernels(E0, M, expect, values)
            if route != "plain":
                return _mean_field_nchw_step(E0, refs, self.W, self.niters, *kernels), bool(expect)
        extra = () if labels is None else (labels,)
        return -_mean_field_nchw(E0, lambda Q: self.W(self.Mu(Q, *extra), refs), self.niters), False


class ijGuide(nn.Module):
    """Guide features (i, j) / sqrt(h^2 + w^2) / s_ij  (crf_module.py:116-123)."""

    def __init__(self, s_ij=.1, trainable=True):
        super().__init__()
        self.s_ij = _maybe_learnable(s_ij, trainable)

    def positions(self, x):
        bs, _, h, w = x.shape
        grid = np.mgrid[:h, :w] / np.sqrt(h ** 2 + w ** 2)
        return torch.from_numpy(grid).float().to(x.device)[None].expand(bs, -1, -1, -1) / self.s_ij

    def forward(self, x):
        return self.positions(x)


class ijrgbGuide(ijGuide):
    """Guide features (i, j)/s_ij ++ rgb/s_rgb (crf_module.py:106-114)."""

    def __init__(self, s_ij=.1, s_rgb=.1, trainable=True):
        super().__init__(s_ij, trainable)
        self.s_rgb = _maybe_learnable(s_rgb, trainable)

    def forward(self, x):
        return torch.cat([self.positions(x), x / self.s_rgb], dim=1)
