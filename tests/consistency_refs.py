"""The float64 yardstick of the consistency loss (sf_consistency_loss), written from the definitions:
KL(Categorical_t || Categorical_s), KL(Normal_t || Normal_s) and the squared value difference between a target row and a
student row, summed over the members of a head list, meaned over the valid rows, with the target DETACHED; the gradient of
the student comes from torch autograd.  No formula of the kernel is copied: the categorical KL is written with
log_softmax, the normal KL with its closed form from variances, and tests/test_consistency_loss_cpu.py holds both against
torch.distributions.kl_divergence."""
import torch

SD_MIN, SD_MAX = 1e-4, 1e4  # the loss's clamp of a Box member's standard deviation (box_sd)


def member_slices(head_sizes):
    """[(kind, start, size)]: 'cat' with size logits, or 'box' with size D (2 D parameters [means | log_std])"""
    out, off = [], 0
    for nh in head_sizes:
        if nh > 0:
            out.append(("cat", off, int(nh)))
            off += int(nh)
        else:
            out.append(("box", off, -int(nh)))
            off += -2 * int(nh)
    return out


def num_params(head_sizes) -> int:
    return sum(nh if nh > 0 else -2 * nh for nh in head_sizes)


def row_kl(params_t: torch.Tensor, params_s: torch.Tensor, head_sizes) -> torch.Tensor:
    """[rows] KL(target || student) of the rows' action distributions, float64"""
    kl = params_t.new_zeros(params_t.shape[0], dtype=torch.float64)
    for kind, off, size in member_slices(head_sizes):
        if kind == "cat":
            lt = torch.log_softmax(params_t[:, off:off + size].double(), dim=-1)
            ls = torch.log_softmax(params_s[:, off:off + size].double(), dim=-1)
            kl = kl + (lt.exp() * (lt - ls)).sum(-1)
        else:
            mt, mss = params_t[:, off:off + size].double(), params_s[:, off:off + size].double()
            st = params_t[:, off + size:off + 2 * size].double().exp().clamp(SD_MIN, SD_MAX)
            ss = params_s[:, off + size:off + 2 * size].double().exp().clamp(SD_MIN, SD_MAX)
            # KL(N(mt, st^2) || N(ms, ss^2)) = log(ss / st) + (st^2 + (mt - ms)^2) / (2 ss^2) - 1/2
            kl = kl + (torch.log(ss / st) + (st ** 2 + (mt - mss) ** 2) / (2.0 * ss ** 2) - 0.5).sum(-1)
    return kl


def consistency_reference(heads_t: torch.Tensor, heads_s: torch.Tensor, valid: torch.Tensor, head_sizes, coeff_policy: float,
                          coeff_value: float, n_valid=None):
    """heads_* [rows, >= 1 + A] (column 0 the value, columns 1 .. A the action parameters); valid [rows] bool.  Returns a
    dict of float64 results: kl_sum, dv2_sum, kl_max, n_valid (over the valid rows), loss = (coeff_policy kl_sum +
    coeff_value dv2_sum) / n_valid, and g [rows, 1 + A] = d loss / d heads_s (zero rows where invalid).  n_valid: the
    divisor when it is not the number of valid rows (the learner's global count)"""
    A = num_params(head_sizes)
    t = heads_t[:, :1 + A].detach().double()
    s = heads_s[:, :1 + A].detach().double().clone().requires_grad_(True)
    w = valid.to(torch.float64)
    kl = row_kl(t[:, 1:], s[:, 1:], head_sizes)
    dv2 = (s[:, 0] - t[:, 0]) ** 2
    nv = float(w.sum()) if n_valid is None else float(n_valid)
    loss = (coeff_policy * (kl * w).sum() + coeff_value * (dv2 * w).sum()) / nv
    g, = torch.autograd.grad(loss, s)
    klv = kl.detach()[valid]
    return dict(kl_sum=float((kl.detach() * w).sum()), dv2_sum=float((dv2.detach() * w).sum()),
                kl_max=float(klv.max()) if klv.numel() else 0.0, n_valid=float(w.sum()), loss=float(loss.detach()), g=g,
                kl_rows=kl.detach())
