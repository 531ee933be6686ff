"""Torch restatement of the vector quantiser (taming.modules.vqvae.quantize.VectorQuantizer's public behaviour, which the reference
builds with beta = 0.25, ldm/models/autoencoder.py:45) and of the reverse steps that quantise their prediction of x_0.  Test
infrastructure: runs on whatever device its inputs live on, in the precision asked for.

  rows  = channels-last flattening of z [N, C, *sp]
  d[m,k] = sum_c z[m,c]^2 + sum_c E[k,c]^2 - 2 sum_c z[m,c] E[k,c];  idx[m] = argmin_k d[m,k], the first minimum on a tie
  quant = z + (E[idx] - z)           the straight-through expression, in that order
"""
import torch


def distances(rows, E, dtype=torch.float64):
    z, e = rows.to(dtype), E.to(dtype)
    return (z ** 2).sum(1, keepdim=True) + (e ** 2).sum(1)[None, :] - 2.0 * (z @ e.t())


def first_argmin(d):
    """Index of the FIRST minimum of every row, written out (no reliance on a library's tie rule)."""
    K = d.shape[1]
    dmin = d.min(1, keepdim=True).values
    ar = torch.arange(K, device=d.device)[None, :].expand_as(d)
    return torch.where(d == dmin, ar, torch.full_like(ar, K)).min(1).values


def quantise(rows, E, dtype=torch.float64, chunk=1024):
    """-> (idx int64 [M], ambiguous bool [M]): ambiguous rows are those whose two smallest distances differ by less than
    1e-4 * (1 + d_min) in `dtype` -- the only rows an fp32 kernel may resolve differently."""
    idx, amb = [], []
    for s in range(0, rows.shape[0], chunk):
        d = distances(rows[s:s + chunk], E, dtype)
        i = first_argmin(d)
        idx.append(i)
        if d.shape[1] > 1:
            two = torch.topk(d, 2, dim=1, largest=False).values
            amb.append((two[:, 1] - two[:, 0]) < 1e-4 * (1.0 + two[:, 0]))
        else:
            amb.append(torch.zeros_like(i, dtype=torch.bool))
    return torch.cat(idx), torch.cat(amb)


def straight_through(rows, E, idx):
    """z + (z_q - z), each operation rounded in the dtype of `rows`."""
    zq = E.to(rows.dtype)[idx]
    return rows + (zq - rows)


class RefVectorQuantizer(torch.nn.Module):
    """Stand-in for taming's class with its constructor, parameter name and return value, for importing the reference's VQModel."""

    def __init__(self, n_e, e_dim, beta=0.25, **unused):
        super().__init__()
        self.n_e, self.e_dim, self.beta = n_e, e_dim, beta
        self.embedding = torch.nn.Embedding(n_e, e_dim)
        self.embedding.weight.data.uniform_(-1.0 / n_e, 1.0 / n_e)

    def forward(self, z):
        zc = z.permute(0, 2, 3, 1).contiguous()
        rows = zc.view(-1, self.e_dim)
        idx, _ = quantise(rows, self.embedding.weight, rows.dtype)
        q = straight_through(rows, self.embedding.weight, idx).view(zc.shape).permute(0, 3, 1, 2).contiguous()
        return q, None, (None, None, idx.view(-1, 1))


def ddim_step_vq(x, eps, sc, E, noise=None, ancestral=False):
    """One reverse step on channels-last rows as separate fp32 torch ops, in the order gg_ddim_step_vq documents.  x, eps, noise fp32
    [M, C]; sc fp32[5]; E fp32 [n_embed, C] or None.  -> (x_prev, pred_x0 quantised, idx, ambiguous, pred_x0 before quantisation), on
    the device of x.  The three scalar square roots are the correctly rounded fp32 ones, as the kernel's sqrtf is: taken in fp64 and
    rounded to fp32 (53 bits are enough for that double rounding to be exact).  torch's own fp32 sqrt of such a scalar is not always
    correctly rounded (measured: it differs from the rounded fp64 root for a_t = 0.6132, 0.9983 and 0.05, and a root one ulp off
    moves most elements of the step).  The elementwise arithmetic runs on the CPU, whose fp32 `/` is the IEEE one."""
    dev = x.device
    x, eps, sc = x.detach().cpu(), eps.detach().cpu(), sc.detach().cpu().float()
    noise = None if noise is None else noise.detach().cpu()
    if ancestral:
        p = sc[0] * x - sc[1] * eps
    else:
        root = lambda v: v.double().sqrt().float()
        sqrt_at, sqrt_ap = root(sc[0]), root(sc[1])
        dirc = root(1.0 - sc[1] - sc[2] * sc[2])
        p = (x - sc[3] * eps) / sqrt_at.expand_as(x)            # a full tensor: a one-element divisor may be turned into a reciprocal
    idx = amb = None
    q = p
    if E is not None:
        E = E.detach().cpu()
        idx, amb = quantise(p, E)
        q = straight_through(p, E, idx)
    if ancestral:
        xn = sc[2] * q + sc[3] * x
    else:
        xn = sqrt_ap * q + dirc * eps
    if noise is not None:
        xn = xn + sc[4] * noise
    mv = lambda t: None if t is None else t.to(dev)
    return mv(xn), mv(q), mv(idx), mv(amb), mv(p)
