"""Helpers of the DPM-Solver++ tests (test_dpm_cpu.py, test_dpm_gpu.py): fp64 numpy restatements of the grid rule, of the coefficient rows
and of the solver's chain on an `eps(x, a)` callable, written from the formulas of Lu et al. 2022 (Algorithm 2) and not from the product
code; the Gaussian toy problem with its closed forms; and the step kernel's expression as separate fp32 torch ops."""
import numpy as np
import torch

SCHEDULES = [(0.0015, 0.0195), (0.00085, 0.012), (1e-4, 2e-2)]          # linear_start, linear_end
T = 1000


def alphas_cumprod(linear_start, linear_end, timesteps=T):
    """The "linear" beta schedule of the reference (util.py:21-24) in fp64, rounded to the fp32 table the samplers read."""
    betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas).astype(np.float32)


def lam(a):
    """lambda = log(alpha / sigma), in the issue's own form: the rows are compared after ONE fp32 rounding, which leaves no room for the
    last-bit differences between two fp64 spellings of it (h = lambda_t - lambda_s cancels most of their digits)."""
    a = np.asarray(a, dtype=np.float64)
    return np.log(np.sqrt(a) / np.sqrt(1.0 - a))


def ddim_timesteps(method, S, timesteps=T):
    """util.py:46-59, + 1."""
    if method == "uniform":
        return np.arange(0, timesteps, timesteps // S) + 1
    return (np.linspace(0, np.sqrt(timesteps * 0.8), S) ** 2).astype(int) + 1


def grid(method, S, ac):
    """Ascending unique DDPM indices of the chain's points."""
    if method != "logsnr":
        return np.asarray(sorted(set(int(t) for t in ddim_timesteps(method, S, len(ac)))), dtype=np.int64)
    l = lam(ac.astype(np.float64))
    picked = set()
    for k in range(S):
        target = l[-1] + (l[0] - l[-1]) * k / S
        best = min(range(len(l)), key=lambda j: (abs(l[j] - target), j))          # nearest lambda, the lower index on a tie
        picked.add(max(best, 1))
    return np.asarray(sorted(picked), dtype=np.int64)


def point_pairs(ts, ac):
    """[(a_s, a_t)] in sampling order, fp64 from the fp32 table: from ts[-1] down, the last step to DDPM index 0."""
    idx = [int(t) for t in ts[::-1]] + [0]
    a = ac.astype(np.float64)
    return [(a[idx[i]], a[idx[i + 1]]) for i in range(len(ts))]


def second_order(i, n, order, lower_order_final):
    return order == 2 and i > 0 and not (lower_order_final and n < 15 and i == n - 1)


def rows(ts, ac, order, lower_order_final):
    """fp64 [n, 6] rows {alpha_s, sigma_s, k_x, k_d, c0, c1} and the fp64 step sizes h."""
    pairs = point_pairs(ts, ac)
    n = len(pairs)
    out, hs = np.zeros((n, 6)), np.zeros(n)
    for i, (a_s, a_t) in enumerate(pairs):
        h = lam(a_t) - lam(a_s)
        hs[i] = h
        c0, c1 = 1.0, 0.0
        if second_order(i, n, order, lower_order_final):
            r = hs[i - 1] / h
            c0, c1 = 1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r)
        out[i] = [np.sqrt(a_s), np.sqrt(1.0 - a_s), np.sqrt(1.0 - a_t) / np.sqrt(1.0 - a_s), -np.sqrt(a_t) * np.expm1(-h), c0, c1]
    return out, hs


def chain(eps, x, ts, ac, order, lower_order_final=True):
    """The solver in fp64 on an eps(x, a) callable, straight from Algorithm 2 (no row table)."""
    pairs = point_pairs(ts, ac)
    n = len(pairs)
    p_prev = h_prev = None
    for i, (a_s, a_t) in enumerate(pairs):
        al_s, sg_s, al_t, sg_t = np.sqrt(a_s), np.sqrt(1.0 - a_s), np.sqrt(a_t), np.sqrt(1.0 - a_t)
        h = np.log(al_t / sg_t) - np.log(al_s / sg_s)
        p = (x - sg_s * eps(x, a_s)) / al_s
        D = p
        if second_order(i, n, order, lower_order_final):
            r = h_prev / h
            D = (1.0 + 1.0 / (2.0 * r)) * p - p_prev / (2.0 * r)
        x = sg_t / sg_s * x - al_t * np.expm1(-h) * D
        p_prev, h_prev = p, h
    return x


# ---- the Gaussian toy: data N(mu, s^2); x_t ~ N(alpha mu, alpha^2 s^2 + sigma^2), so eps and the probability-flow solution are closed forms
MU = 0.3


def toy_eps(s):
    def eps(x, a):
        al, sg = np.sqrt(a), np.sqrt(1.0 - a)
        return sg * (x - al * MU) / (a * s * s + (1.0 - a))            # -sigma * score of the marginal
    return eps


def toy_exact(x_start, a_start, a_end, s):
    """The probability-flow ODE of a Gaussian marginal keeps (x - mean) / std fixed."""
    std = lambda a: np.sqrt(a * s * s + (1.0 - a))
    return np.sqrt(a_end) * MU + std(a_end) * (x_start - np.sqrt(a_start) * MU) / std(a_start)


def toy_error(method, S, order, ac, s, x_T):
    ts = grid(method, S, ac)
    a = ac.astype(np.float64)
    got = chain(toy_eps(s), x_T.copy(), ts, ac, order)
    return float(np.abs(got - toy_exact(x_T, a[ts[-1]], a[0], s)).max())


# ---- the step kernel's expression, every product and sum its own fp32 torch op
def torch_step(x, out, hist, sc, flags):
    """-> (x_next, p): sc fp32[6] = {alpha_s, sigma_s, k_x, k_d, c0, c1}; hist enters only when c1 != 0."""
    t = sc[1] * out
    u = x - t
    p = u / sc[0]
    if flags & 1:
        p = out.clone()
    if flags & 2:
        p = torch.clamp(p, -1.0, 1.0)
    D = p
    if float(sc[5]) != 0.0:
        d0 = sc[4] * p
        d1 = sc[5] * hist
        D = d0 + d1
    n0 = sc[2] * x
    n1 = sc[3] * D
    return n0 + n1, p
