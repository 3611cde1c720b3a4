"""What the energy-range tests share (test_energy_regimes_cpu.py, test_gpu_energy_range.py): named energy regimes of the
sizes the workload feeds the softmax kernels, the accuracy rules the suite already has (re-exported or restated, no figure
changed), the checks that go with infinite and dominated energies, and a model of an fp32 accumulation started at E0.

Where the magnitudes come from: examples/stereo_crf.py feeds ``phl.cost_volume(...) * unary_weight``.  An AD cost over a
5x5 window and 3 channels with weight 4 is at most 300 for images in [0, 1] and at most 7.65e4 for 8-bit images.

Rules (``want`` is always the float64 torch form on the device, ``e_torch`` the fp32 torch form on the same operands):
    Q, logits and step products   e_hip <= max(2e-6 * max(1, |want|max), 2 * e_torch)     (_nchw_util.check_product)
    gradients                     e_hip <= 2 * e_torch + 2.5e-7 * |want|max               (test_compat_grad_parity)
    loops                         e_new <= 2 * e_old                                      (_nchw_util.report_loop)
A bound is never taken from the code under test.  Every pair of errors is printed as a ``[measured]`` line."""
import torch

from _nchw_util import check_product, report_loop  # noqa: F401  (re-exported: the rules of the step and of the loops)

OFFSET_REGIMES = ("offset_3e2", "offset_7.65e4", "offset_-7.65e4", "row_offsets", "ties")
REGIMES = OFFSET_REGIMES + ("dominated", "spread_120", "masked")
LOOP_REGIMES = ("offset_7.65e4", "row_offsets", "masked")
ROW_OFFSETS = (0.0, 1e2, -1e3, 1e4, -1e5, 7.65e4)
INF = float("inf")


def winners(n, L, device):
    """The winning label of every pixel of ``dominated``: p % L, and L - 1 for the last pixel, so that label 0 and label
    L - 1 win somewhere at every (n, L) with n >= 2, and every label where n >= L."""
    win = torch.arange(n, device=device) % L
    if n > 1:
        win[n - 1] = L - 1
    return win


def regimes(n, L, gen):
    """{name: fp32 [n, L] energies} on the generator's device, every regime built from ``base = 8 * rand``:
        offset_3e2, offset_7.65e4, offset_-7.65e4   base + c
        row_offsets   base + c_p, c_p drawn per pixel from ROW_OFFSETS (a tile-wide shift in place of a per-row one fails)
        ties          every entry 7.65e4
        dominated     base + 200 with label winners(n, L)[p] 200 lower: every other label underflows to exactly 0 in fp32
        spread_120    120 * rand: Q runs through the denormal range of exp2 down to 0
        masked        base with +inf at a random quarter of the entries, the whole of label 0 in the first third of the
                      pixels and of label L - 1 in the second third; one finite label per pixel is guaranteed
    A channel-major caller transposes (``nchw``).  L >= 2."""
    dev = gen.device
    rand = lambda *shape: torch.rand(shape, device=dev, generator=gen)                          # noqa: E731
    base = 8 * rand(n, L)
    out = {"offset_3e2": base + 3e2, "offset_7.65e4": base + 7.65e4, "offset_-7.65e4": base - 7.65e4}
    pick = torch.randint(0, len(ROW_OFFSETS), (n,), device=dev, generator=gen)
    out["row_offsets"] = base + torch.tensor(ROW_OFFSETS, device=dev)[pick][:, None]
    out["ties"] = torch.full((n, L), 7.65e4, device=dev)
    p = torch.arange(n, device=dev)
    dom = base + 200
    dom[p, winners(n, L, dev)] -= 200
    out["dominated"] = dom
    out["spread_120"] = 120 * rand(n, L)
    mask = rand(n, L) < 0.25
    a, b = n // 3, 2 * n // 3
    mask[:a, 0] = True
    mask[a:b, L - 1] = True
    keep = torch.randint(0, L - 1, (n,), device=dev, generator=gen)      # a label that stays finite: not 0 / L - 1 where forced
    keep[:a] += 1
    keep[b:] = torch.randint(0, L, (n - b,), device=dev, generator=gen)
    mask[p, keep] = False
    out["masked"] = torch.where(mask, torch.full_like(base, INF), base)
    assert tuple(out) == REGIMES
    return out


def nchw(E, B, H, W):
    """The pixel-major [B * H * W, L] regime as a contiguous channel-major [B, L, H, W] volume."""
    return E.reshape(B, H, W, E.shape[1]).permute(0, 3, 1, 2).contiguous()


def padded_rows(t, pad=4, poison=1e3):
    """A row-padded view of the [n, L] tensor t (row stride L + pad; the padding is poison)."""
    n, L = t.shape
    buf = torch.full((n, L + pad), poison, dtype=t.dtype, device=t.device)
    buf[:, :L] = t
    return buf[:, :L]


# ---- the rules ---------------------------------------------------------------------------------------------------------
def q_bound(want, e_torch):
    fin = want[torch.isfinite(want)]
    return max(2e-6 * max(1.0, float(fin.abs().max()) if fin.numel() else 0.0), 2 * e_torch)


def grad_bound(want, e_torch):
    return 2 * e_torch + 2.5e-7 * float(want.abs().max())


def max_err(got, want):
    """max|got - want| where the float64 ``want`` is finite -- (error, problem): ``got`` must be finite wherever ``want`` is,
    and equal to it (the same infinity) wherever it is not."""
    fin = torch.isfinite(want)
    problem = None
    if not bool(torch.isfinite(got[fin]).all()):
        problem = "not finite where the float64 reference is"
    elif not bool((got[~fin].double() == want[~fin]).all()):
        problem = "differs from the float64 reference where that is infinite"
    d = (got.double() - want)[fin].abs()
    d = d[torch.isfinite(d)]
    return (float(d.max()) if d.numel() else 0.0), problem


class Report:
    """Collects the failures of one test so that every ``[measured]`` line is printed before the test asserts."""

    def __init__(self):
        self.failures = []

    def fail(self, name, what):
        self.failures.append(f"{name}: {what}")

    def judge(self, name, got, ref32, want, bound=q_bound, chain=None, contract=False):
        """e_hip against the rule ``bound(want, e_torch)``.  chain: the same output computed from the fp32-accumulation
        model (chain_model); its error e_chain is printed, and with ``contract`` the rule is ``bound(want, e_chain)`` -- the
        documented contract of the kernels that accumulate on top of E0, at the offset regimes only.  Returns
        (e_hip, e_torch)."""
        e_hip, problem = max_err(got, want)
        e_torch, _ = max_err(ref32, want)
        lim, tag = bound(want, e_torch), ""
        if chain is not None:
            e_chain, _ = max_err(chain, want)
            tag = f"  e_chain = {e_chain:.3e}"
            if contract:                         # Q and logits: 2 * e_chain with no floor; gradients: their rule on e_chain
                lim = 2 * e_chain if bound is q_bound else bound(want, e_chain)
        print(f"[measured] {name}: e_hip = {e_hip:.3e}  e_torch = {e_torch:.3e}{tag}  bound = {lim:.3e}")
        if problem:
            self.fail(name, problem)
        if not e_hip <= lim:
            self.fail(name, f"e_hip {e_hip:.3e} > bound {lim:.3e} (e_torch {e_torch:.3e})")
        return e_hip, e_torch

    def exact(self, name, got, at, value):
        """``got`` is exactly ``value`` at the entries ``at``."""
        if not bool((got[at] == value).all()):
            self.fail(name, f"not exactly {value} at the masked entries")

    def one_hot(self, name, q, win, want, e_torch):
        """dominated: Q is the one-hot winner within the rule."""
        hot = torch.zeros_like(want).scatter_(1, win[:, None], 1.0)
        e = float((q.double() - hot).abs().max())
        if not (bool((q.argmax(1) == win).all()) and e <= q_bound(want, e_torch)):
            self.fail(name, f"not the one-hot winner (off by {e:.3e})")

    def done(self):
        assert not self.failures, "\n".join(self.failures)


def loop_judge(rep, name, new, old, want, chain=None, contract=False):
    """The rule of _nchw_util.report_loop, e_new <= 2 * e_old, where ``want`` is finite, with the infinities compared
    exactly (report_loop itself takes finite outputs only).  chain: the loop run on the accumulation model, its error
    printed; with ``contract`` the rule is e_new <= 2 * max(e_old, e_chain)."""
    e_new, problem = max_err(new, want)
    e_old, _ = max_err(old, want)
    lim, tag = 2 * e_old, ""
    if chain is not None:
        e_chain, _ = max_err(chain, want)
        tag = f"  e_chain = {e_chain:.3e}"
        if contract:
            lim = 2 * max(e_old, e_chain)
    print(f"[measured] {name}: e_new = {e_new:.3e}  e_old = {e_old:.3e}{tag}")
    if problem:
        rep.fail(name, problem)
    if not e_new <= lim:
        rep.fail(name, f"e_new {e_new:.3e} > {lim:.3e} (e_old {e_old:.3e})")
    return e_new, e_old


# ---- the accumulation model ----------------------------------------------------------------------------------------------
def _bf16_parts(t):
    """t = h + m + l exactly, each part a bf16 number taken by truncation (the split kernels' operands)."""
    def trunc(v):
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    h = trunc(t)
    m = trunc(t - h)
    return h, m, (t - h) - m


def chain_model(E0, X, Mu, group, split=False, inner=None):
    """E = E0 + X @ Mu as an fp32 accumulation STARTED AT E0, in plain torch: per step of ``group`` products a float64 fma
    rounded to fp32, so every step rounds at the magnitude of E0.  group = 1 is an fmaf chain in k order (k_compat_tail, and
    the f32 matrix cores of k_compat_softmax, which are bitwise that chain).  split: the bf16 matrix cores of
    k_compat_split -- both operands in three exact bf16 parts, six partial products per chunk of ``group`` = 32 in the
    kernel's order.  inner: the accumulator is rounded every ``inner`` products inside one instruction (default: once per
    instruction).  v_mfma_f32_16x16x32_bf16 on gfx950 behaves as inner = 8: over 12 cases (L = 132, 252, 256; offsets 3e2 and
    7.65e4, row offsets, ties) e_hip / e_chain is 0.96 .. 1.03 at 8 and 0.5 .. 3.5 at 32, 16, 4 and 2, and only at 8 does the
    model follow the kernel's Q itself (|Q_hip - Q_chain| five to ten times smaller than at any other value)."""
    acc = E0.clone()
    L = E0.shape[1]
    if split:
        xs, ms = [p.double() for p in _bf16_parts(X)], [p.double() for p in _bf16_parts(Mu)]
        terms = [(0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0)]             # (part of X, part of Mu): smallest terms first
    else:
        xs, ms, terms = [X.double()], [Mu.double()], [(0, 0)]
    inner = inner or group
    for k in range(0, L, group):
        for a, b in terms:
            for j in range(k, min(k + group, L), inner):
                hi = min(j + inner, k + group)
                acc = (acc.double() + xs[a][:, j:hi] @ ms[b][j:hi]).float()
    return acc
