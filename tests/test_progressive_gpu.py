"""GPU suite for progressive sampling: gg_ddpm_step_x0 bit for bit against the same expression as separate fp32 torch ops (and against
gg_ddpm_step with no option set), gg_log_rows against permute + contiguous inside a log buffer, the logged lists of p_sample_loop,
progressive_denoising, DDPM, DDIM and PLMS against what the REFERENCE produced from the same tapes (tests/golden/progressive.npz,
make_golden_progressive.py; inputs and tapes are those of inpaint.npz), and the engine's bit-exact invariants.

Tolerances are those of the existing chain tests on this network (tests/test_inpaint_gpu.py, tests/test_hip_parity.py): ancestral 20 steps
and PLMS max < 1.5e-2, rms < 1e-2; DDIM 5 steps max < 2e-2, rms < 1.5e-2.  Every list entry is held to them, relative to that entry."""
import pytest
import torch

from progressive_ref import ddpm_small, ldm_small, logged, torch_step_x0
from util import T, gold, rel_err, rms_err

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SHAPE = (2, 4, 8, 8)
ANC = (1.5e-2, 1e-2)          # ancestral 20 steps (test_ancestral_inpainting_matches_reference_fixture), PLMS
DDIM = (2e-2, 1.5e-2)         # DDIM 5 steps (test_ddim_inpainting_matches_reference_fixture)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return gold("progressive")


@pytest.fixture(scope="module")
def ops_in(dev):
    """Inputs and tapes of the fixture: make_golden_progressive.py checks that it drew exactly what inpaint.npz holds."""
    gi = gold("inpaint")
    o = {k: T(gi[k]).float().to(dev) for k in ("c", "x_T", "x0", "mask_hole")}
    o["q"] = list(T(gi["q_tape"]).float().to(dev))
    o["step"] = list(T(gi["step_tape"]).float().to(dev))
    return o


@pytest.fixture(scope="module")
def small(dev):
    return ldm_small(1000).to(dev)


@pytest.fixture(scope="module")
def m20(dev):
    return ldm_small(20).to(dev)


def check_list(got, want, tol, what):
    """Every entry against the reference's, each relative to itself; the figures are printed before anything is asserted."""
    want = T(want).float()
    assert len(got) == want.shape[0], (what, len(got), want.shape[0])
    errs = []
    for j, e in enumerate(got):
        assert tuple(e.shape) == tuple(want[j].shape)
        errs.append((rel_err(e, want[j]), rms_err(e, want[j])))
    print(f"{what}: {len(got)} entries, worst max {max(e for e, _ in errs):.3e} rms {max(r for _, r in errs):.3e}; "
          + " ".join(f"[{j}] {e:.2e}/{r:.2e}" for j, (e, r) in enumerate(errs)))
    for j, (err, rms) in enumerate(errs):
        t = tol[j] if isinstance(tol, list) else tol          # a list: one (max, rms) bound per entry
        assert err < t[0] and rms < t[1], f"{what}[{j}]: max {err:.3e} rms {rms:.3e} (bound {t[0]:.1e} / {t[1]:.1e})"


# ------------------------------------------------------------------------------------------------ kernel: gg_ddpm_step_x0
SC = [1.0932451, 0.4417764, 0.2113977, 0.7840215, 0.0912346]


def step_case(dev, M, C, flags, stride, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(M, C, device=dev, generator=gen) * 1.5                      # |x_recon| crosses 1 on a good share of the elements
    out = torch.randn(M, stride, device=dev, generator=gen)
    noise = torch.randn(M, C, device=dev, generator=gen)
    return x, out, noise, torch.tensor(SC, device=dev)


@pytest.mark.parametrize("M", [1000, 2 ** 20 + 3], ids=["M1000", "M2^20+3"])
@pytest.mark.parametrize("C", [4, 3], ids=["C4_vector", "C3_scalar"])
@pytest.mark.parametrize("flags", [0, 1, 2, 3], ids=["eps", "x0", "eps_clip", "x0_clip"])
def test_step_kernel_is_bit_equal_to_the_torch_expression(dev, M, C, flags):
    from jointimagegeneration_amd import ops
    x0_, out, noise, sc = step_case(dev, M, C, flags, 32, M * 13 + C * 5 + flags)
    for with_noise in (True, False):
        want_x, want_p = torch_step_x0(x0_, out[:, :C], noise if with_noise else None, sc, flags)
        if flags & 2:
            assert bool((want_p.abs() == 1.0).any()) and bool((want_p.abs() < 1.0).any())
        for with_p0 in (True, False):
            for with_uin in (True, False):
                x = x0_.clone()
                p0 = torch.full((M, C), 9.0, device=dev) if with_p0 else None
                uin = torch.full((M, 32), 7.0, dtype=torch.bfloat16, device=dev) if with_uin else None      # pad lanes: a sentinel that must survive
                ops.ddpm_step_x0(x, out, sc, noise=noise if with_noise else None, predicts_x0=bool(flags & 1), clip=bool(flags & 2),
                                 pred_x0_out=p0, unet_in=uin)
                torch.cuda.synchronize()
                tag = (with_noise, with_p0, with_uin)
                assert torch.equal(x, want_x), tag
                if with_p0:
                    assert torch.equal(p0, want_p), tag
                if with_uin:
                    assert torch.equal(uin[:, :C], want_x.bfloat16()) and bool((uin[:, C:] == 7.0).all()), tag


@pytest.mark.parametrize("M", [1000, 2 ** 20 + 3], ids=["M1000", "M2^20+3"])
@pytest.mark.parametrize("C", [4, 3])
def test_step_kernel_without_options_is_bit_equal_to_gg_ddpm_step(dev, M, C):
    from jointimagegeneration_amd import ops
    x0_, out, noise, sc = step_case(dev, M, C, 0, 32, M + C)
    for nz in (noise, None):
        xa, xb = x0_.clone(), x0_.clone()
        ua, ub = (torch.full((M, 32), 7.0, dtype=torch.bfloat16, device=dev) for _ in range(2))
        ops.ddpm_step(xa, out, sc, noise=nz, unet_in=ua)
        ops.ddpm_step_x0(xb, out, sc, noise=nz, unet_in=ub)
        torch.cuda.synchronize()
        assert torch.equal(xa, xb) and torch.equal(ua, ub)


def test_step_kernel_misaligned_rows_take_the_fallback(dev):
    """x as a view offset by one row with C = 3 (12 bytes off any 16-byte boundary), and C = 4 rows at a one-float offset with a unet_in
    stride that is no multiple of 4: both must run the per-element loop and give the same bits."""
    from jointimagegeneration_amd import ops
    sc = torch.tensor(SC, device=dev)
    gen = torch.Generator(device=dev).manual_seed(77)
    M = 4099
    buf = torch.randn(M + 1, 3, device=dev, generator=gen)
    x, row0 = buf[1:], buf[0].clone()
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    out, noise = torch.randn(M, 5, device=dev, generator=gen), torch.randn(M, 3, device=dev, generator=gen)
    want_x, want_p = torch_step_x0(x.clone(), out[:, :3], noise, sc, 3)
    p0, uin = torch.empty(M, 3, device=dev), torch.full((M, 6), -3.0, dtype=torch.bfloat16, device=dev)
    ops.ddpm_step_x0(x, out, sc, noise=noise, predicts_x0=True, clip=True, pred_x0_out=p0, unet_in=uin)
    torch.cuda.synchronize()
    assert torch.equal(x, want_x) and torch.equal(p0, want_p) and torch.equal(uin[:, :3], want_x.bfloat16()) and bool((uin[:, 3:] == -3.0).all())
    assert torch.equal(buf[0], row0)                         # the row in front of the view is not touched
    flat = torch.randn(3, M * 4 + 1, device=dev, generator=gen)
    col0 = flat[:, 0].clone()
    x, noise, p0 = (flat[i, 1:].view(M, 4) for i in range(3))
    out = torch.randn(M, 4, device=dev, generator=gen)
    want_x, want_p = torch_step_x0(x.clone(), out, noise, sc, 2)
    uin = torch.full((M, 6), -3.0, dtype=torch.bfloat16, device=dev)
    ops.ddpm_step_x0(x, out, sc, noise=noise, clip=True, pred_x0_out=p0, unet_in=uin)
    torch.cuda.synchronize()
    assert torch.equal(x, want_x) and torch.equal(p0, want_p) and torch.equal(uin[:, :4], want_x.bfloat16()) and bool((uin[:, 4:] == -3.0).all())
    assert torch.equal(flat[:, 0], col0)


# ------------------------------------------------------------------------------------------------ kernel: gg_log_rows
@pytest.mark.parametrize("sp", [(5, 7), (3, 4, 5)], ids=["2d", "3d"])
@pytest.mark.parametrize("C", [3, 4])
def test_log_rows_fills_one_slot_and_leaves_its_neighbours(dev, sp, C):
    from jointimagegeneration_amd import ops
    N = 2
    gen = torch.Generator(device=dev).manual_seed(C + len(sp))
    state = torch.randn((N,) + sp + (C,), device=dev, generator=gen)
    log = torch.full((3, N, C) + sp, -5.0, device=dev)
    S = state.numel() // (N * C)
    ops.log_rows(state.view(N * S, C), N, log[1])
    torch.cuda.synchronize()
    nd = len(sp)
    assert torch.equal(log[1], state.permute((0, nd + 1) + tuple(range(1, nd + 1))).contiguous())
    assert bool((log[0] == -5.0).all()) and bool((log[2] == -5.0).all())
    with pytest.raises(ValueError, match="log_rows"):
        ops.log_rows(state.view(N * S, C), N, log[1, :1])


# ------------------------------------------------------------------------------------------------ chains against the reference
def test_p_sample_loop_log_every_3_matches_reference(dev, m20, ops_in, g):
    z, inter = m20.p_sample_loop(ops_in["c"], SHAPE, return_intermediates=True, x_T=ops_in["x_T"], verbose=False, log_every_t=3,
                                 noise_tape=ops_in["step"])
    assert len(inter) == 1 + len(logged(20, 3)) and torch.equal(inter[0], ops_in["x_T"]) and torch.equal(inter[-1], z)
    check_list(inter[1:], g["inter_loop3"], ANC, "p_sample_loop log_every_t=3")
    # the default keeps the two-entry list, with the same final tensor
    z2, two = m20.p_sample_loop(ops_in["c"], SHAPE, return_intermediates=True, x_T=ops_in["x_T"], verbose=False, noise_tape=ops_in["step"])
    assert len(two) == 2 and torch.equal(two[0], ops_in["x_T"]) and torch.equal(two[1], z2) and torch.equal(z2, z)


def test_progressive_denoising_matches_reference(dev, m20, ops_in, g):
    seen, imgs = [], []
    z, inter = m20.progressive_denoising(ops_in["c"], SHAPE, verbose=False, x_T=ops_in["x_T"], log_every_t=3, noise_tape=ops_in["step"],
                                         callback=seen.append, img_callback=lambda img, i: imgs.append((i, img)))
    check_list(inter, g["inter_prog3"], ANC, "progressive_denoising x0 predictions")
    check_list([z], T(g["z_prog3"])[None], ANC, "progressive_denoising img")
    assert seen == list(range(19, -1, -1)) and [i for i, _ in imgs] == seen
    assert all(tuple(im.shape) == SHAPE for _, im in imgs) and torch.equal(imgs[-1][1], z)
    # batch_size / per-sample shape, and the cut of the conditioning to the batch (ddpm.py:1130-1145)
    c3 = torch.cat([ops_in["c"], ops_in["c"][:1]])
    z_b, inter_b = m20.progressive_denoising(c3, SHAPE[1:], verbose=False, batch_size=2, x_T=ops_in["x_T"], log_every_t=3, noise_tape=ops_in["step"])
    assert torch.equal(z_b, z) and all(torch.equal(a, b) for a, b in zip(inter_b, inter))


def test_progressive_denoising_temperature_list_and_mask_matches_reference(dev, m20, ops_in, g):
    temps = [float(v) for v in g["temperature"]]
    z, inter = m20.progressive_denoising(ops_in["c"], SHAPE, verbose=False, x_T=ops_in["x_T"], log_every_t=10, temperature=temps,
                                         mask=ops_in["mask_hole"], x0=ops_in["x0"], noise_tape=ops_in["step"], mask_noise_tape=ops_in["q"])
    check_list(inter, g["inter_prog_temp_mask"], ANC, "progressive_denoising temperature list + mask, x0 predictions")
    check_list([z], T(g["z_prog_temp_mask"])[None], ANC, "progressive_denoising temperature list + mask, img")
    known = m20.sqrt_alphas_cumprod[0] * ops_in["x0"] + m20.sqrt_one_minus_alphas_cumprod[0] * ops_in["q"][19]
    assert float(((z - known) * ops_in["mask_hole"]).abs().max()) <= 1e-6


def test_clip_denoised_variant_of_latent_diffusion_matches_reference(dev, ops_in, g):
    m = ldm_small(20).to(dev)
    m.clip_denoised = True                                   # an attribute, as in the reference (ddpm.py:471)
    z, inter = m.progressive_denoising(ops_in["c"], SHAPE, verbose=False, x_T=ops_in["x_T"], log_every_t=10, noise_tape=ops_in["step"])
    assert all(float(e.abs().max()) <= 1.0 for e in inter)
    check_list(inter, g["inter_prog_clip"], ANC, "LatentDiffusion clip_denoised, x0 predictions")
    check_list([z], T(g["z_prog_clip"])[None], ANC, "LatentDiffusion clip_denoised, img")


def x0_bounds(measured):
    """Per-entry bounds of an x0-parameterised chain: the standard ancestral tolerance, or twice the error measured against the reference
    golden where that is larger (X0_MEASURED)."""
    return [(max(ANC[0], 2 * e), max(ANC[1], 2 * r)) for e, r in measured]


# Errors (max, rms) of the x0-parameterised chains against the reference golden, measured on an MI355X, per logged entry (timesteps 19,
# 10, 0).  These chains feed the UNet's output back as the state (posterior_mean_coef1 reaches 1 at t = 0), and on these random-weight
# networks they amplify a perturbation from step to step: the REFERENCE itself, run in fp32 on the CPU with nothing but its UNet weights
# rounded to bf16, moves by (5.9e-4, 1.4e-2, 5.3e-1) max / (5.2e-4, 1.0e-2, 3.1e-1) rms on the DDPM chain and by (7.3e-3, 9.4e-3, 2.5e-2)
# / (7.4e-3, 1.1e-2, 2.0e-2) on the LatentDiffusion one.  The eps-parameterised chains above stay inside the standard tolerance.
X0_MEASURED = {
    "prog_x0": [(9.54e-3, 1.01e-2), (1.15e-2, 1.42e-2), (2.40e-2, 2.09e-2)],
    "loop_x0_clip": [(7.47e-4, 6.64e-4), (8.05e-3, 6.73e-3), (4.78e-2, 2.69e-2)],
    "ddpm_x0": [(8.25e-4, 7.33e-4), (1.74e-2, 1.01e-2), (1.07, 4.10e-1)],
}


def test_x0_variants_of_latent_diffusion_match_reference(dev, ops_in, g):
    mx = ldm_small(20, parameterization="x0").to(dev)
    z, inter = mx.progressive_denoising(ops_in["c"], SHAPE, verbose=False, x_T=ops_in["x_T"], log_every_t=10, noise_tape=ops_in["step"])
    assert torch.equal(z, inter[-1])                         # t = 0: coef1 = 1, coef2 = 0, sigma = 0, so img is the last prediction
    check_list(inter, g["inter_prog_x0"], x0_bounds(X0_MEASURED["prog_x0"]), "LatentDiffusion x0 parameterisation, x0 predictions")
    check_list([z], T(g["z_prog_x0"])[None], x0_bounds(X0_MEASURED["prog_x0"][-1:]), "LatentDiffusion x0 parameterisation, img")
    mx.clip_denoised = True
    z, inter = mx.p_sample_loop(ops_in["c"], SHAPE, return_intermediates=True, x_T=ops_in["x_T"], verbose=False, log_every_t=10,
                                noise_tape=ops_in["step"])
    assert float(z.abs().max()) <= 1.0
    check_list(inter[1:], g["inter_loop_x0_clip"], x0_bounds(X0_MEASURED["loop_x0_clip"]), "LatentDiffusion x0 + clip, p_sample_loop")


@pytest.mark.parametrize("tag,kw", [("eps", {}), ("x0", dict(parameterization="x0"))])
def test_ddpm_matches_reference(dev, ops_in, g, tag, kw):
    d = ddpm_small(**kw).to(dev)
    assert d.clip_denoised is True
    z, inter = d.p_sample_loop(SHAPE, return_intermediates=True, x_T=ops_in["x_T"], noise_tape=ops_in["step"])
    assert len(inter) == 1 + len(logged(20, 10)) and torch.equal(inter[0], ops_in["x_T"]) and torch.equal(inter[-1], z)
    check_list(inter[1:], g[f"inter_ddpm_{tag}"], x0_bounds(X0_MEASURED["ddpm_x0"]) if tag == "x0" else ANC, f"DDPM {tag}")
    # clip_denoised bounds every prediction of x_0, and at t = 0 the posterior mean IS that prediction (coef1 = 1, coef2 = 0, sigma = 0):
    # whatever the chain amplified, the result lies in [-1, 1], as the reference's does
    assert bool(torch.isfinite(z).all()) and float(z.abs().max()) <= 1.0 and float(T(g[f"inter_ddpm_{tag}"])[-1].abs().max()) <= 1.0
    z2 = d.sample(batch_size=2, x_T=ops_in["x_T"], noise_tape=ops_in["step"])
    assert torch.equal(z2, z)


def sampler_run(s, ops_in, eta=0.0, **kw):
    if eta:
        kw["noise_tape"] = ops_in["step"][:5]
    return s.sample(S=5, batch_size=2, shape=(4, 8, 8), conditioning=ops_in["c"], verbose=False, x_T=ops_in["x_T"], eta=eta, **kw)


@pytest.mark.parametrize("name,eta,tol", [("ddim_eta0", 0.0, DDIM), ("ddim_eta1", 1.0, DDIM), ("plms", 0.0, ANC)])
@pytest.mark.parametrize("k", [1, 2])
def test_sampler_lists_match_reference(dev, small, ops_in, g, name, eta, tol, k):
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    s = (PLMSSampler if name == "plms" else DDIMSampler)(small)
    rows = [4 - index for index in logged(5, k)]             # rows of the stored log_every_t = 1 lists (entry j: index 4 - j)
    for call in range(3 if name == "ddim_eta0" else 1):       # eta 0: eager, captured, replayed
        z, inter = sampler_run(s, ops_in, eta, log_every_t=k)
        assert torch.equal(inter["x_inter"][0], ops_in["x_T"]) and torch.equal(inter["pred_x0"][0], ops_in["x_T"])
        assert torch.equal(inter["x_inter"][-1], z)
        check_list(inter["x_inter"][1:], g[f"xi_{name}"][rows], tol, f"{name} k={k} call {call} x_inter")
        check_list(inter["pred_x0"][1:], g[f"p0_{name}"][rows], tol, f"{name} k={k} call {call} pred_x0")


# ------------------------------------------------------------------------------------------------ engine invariants (bit for bit)
def lists_equal(a, b):
    return all(len(a[n]) == len(b[n]) and all(torch.equal(x, y) for x, y in zip(a[n], b[n])) for n in ("x_inter", "pred_x0"))


def test_logged_chain_captured_equals_eager_and_leaves_the_unlogged_graph(dev, small, ops_in):
    from jointimagegeneration_amd.ldm import DDIMSampler
    s = DDIMSampler(small)
    plain = [sampler_run(s, ops_in) for _ in range(3)]        # eager, capture, replay
    (key0, st0), = s._graphs.items()
    graph0 = st0["graph"]
    assert graph0 is not None and "log" not in st0
    se = DDIMSampler(small)
    se.use_graph = False
    z_e, inter_e = sampler_run(se, ops_in, log_every_t=2)
    for call in range(3):
        z, inter = sampler_run(s, ops_in, log_every_t=2)
        assert torch.equal(z, z_e) and lists_equal(inter, inter_e), call
        # the final z and the last pred_x0 are those of the unlogged call
        assert torch.equal(z, plain[0][0]) and torch.equal(inter["pred_x0"][-1], plain[0][1]["pred_x0"][1])
    logged_states = [st for key, st in s._graphs.items() if any(isinstance(e, tuple) and e and e[0] == "log" for e in key)]
    assert len(logged_states) == 1 and logged_states[0]["graph"] is not None and logged_states[0]["graph"] is not graph0
    assert ("log", (4, 2, 0)) in [e for key in s._graphs for e in key if isinstance(e, tuple)]
    # another interval is another state; an unlogged call afterwards replays the graph it had and returns identical tensors
    sampler_run(s, ops_in, log_every_t=1)
    z, inter = sampler_run(s, ops_in)
    assert s._graphs[key0] is st0 and st0["graph"] is graph0 and len(inter["x_inter"]) == 2
    assert torch.equal(z, plain[2][0]) and torch.equal(inter["pred_x0"][1], plain[2][1]["pred_x0"][1])
    # a chain with callbacks runs eagerly and gives the same bits
    seen, preds = [], []
    z_c, inter_c = sampler_run(s, ops_in, log_every_t=2, callback=seen.append, img_callback=lambda p, i: preds.append(p))
    assert seen == [0, 1, 2, 3, 4] and torch.equal(z_c, z_e) and lists_equal(inter_c, inter_e)
    assert torch.equal(preds[-1], inter_e["pred_x0"][-1]) and torch.equal(preds[0], inter_e["pred_x0"][1])


def traced(cls, model, run):
    """An unlogged eager chain whose callback copies the state's x and pred_x0 after every step: what a log entry has to equal."""
    s = cls(model)
    s.use_graph = False
    xs, ps = [], []

    def grab(i):
        st = next(v for v in s._graphs.values() if v.get("callbacks") is not None)
        shape = (st["N"],) + tuple(st["sp"]) + (st["Cx"],)
        back = (0, len(shape) - 1) + tuple(range(1, len(shape) - 1))
        xs.append(st["x"].view(shape).permute(back).contiguous())
        ps.append(st["pred_x0"].view(shape).permute(back).contiguous())
    z, _ = run(s, callback=grab)
    return z, xs, ps


def check_logged_against_trace(cls, model, run, x_T, steps, captured):
    """Logged lists (log_every_t 1 and 3) against the traced chain, entry by entry and bit for bit; three calls each, so that a
    capturable chain is also compared as a captured and as a replayed graph."""
    z_t, xs, ps = traced(cls, model, run)
    assert len(xs) == steps
    s = cls(model)
    for k in (1, 3):
        rows = [steps - 1 - index for index in logged(steps, k)]
        for call in range(3):
            z, inter = run(s, log_every_t=k)
            assert torch.equal(z, z_t), (k, call)
            assert len(inter["x_inter"]) == len(inter["pred_x0"]) == 1 + len(rows)
            assert torch.equal(inter["x_inter"][0], x_T) and torch.equal(inter["pred_x0"][0], x_T)
            for e, r in zip(inter["x_inter"][1:], rows):
                assert torch.equal(e, xs[r]), (k, call, r)
            for e, r in zip(inter["pred_x0"][1:], rows):
                assert torch.equal(e, ps[r]), (k, call, r)
    states = [st for key, st in s._graphs.items() if any(isinstance(e, tuple) and e and e[0] == "log" for e in key)]
    assert len(states) == 2 and all((st["graph"] is not None) == captured for st in states)


@pytest.mark.parametrize("case", ["guidance", "mask", "mask_eta", "plms_mask"])
def test_logged_entries_under_guidance_and_inpainting_equal_the_traced_chain(dev, small, ops_in, case):
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    kw = dict(guidance=dict(unconditional_guidance_scale=3.0, unconditional_conditioning=torch.zeros_like(ops_in["c"])),
              mask=dict(mask=ops_in["mask_hole"], x0=ops_in["x0"], mask_noise_tape=ops_in["q"][:5]),
              mask_eta=dict(mask=ops_in["mask_hole"], x0=ops_in["x0"], mask_noise_tape=ops_in["q"][:5], eta=0.6),
              plms_mask=dict(mask=ops_in["mask_hole"], x0=ops_in["x0"], mask_noise_tape=ops_in["q"][:5]))[case]
    cls = PLMSSampler if case == "plms_mask" else DDIMSampler
    check_logged_against_trace(cls, small, lambda s, **k: sampler_run(s, ops_in, **kw, **k), ops_in["x_T"], 5, captured=case == "mask")


def test_steps_are_the_schedules_own_count_when_S_does_not_divide_the_timesteps(dev, small, ops_in, g):
    """S = 15 on 1000 timesteps: the uniform schedule holds 16 steps, and the reference logs against those (ddim.py:136,160): its
    recorded indices start at 15.  (S = 3 would be the smallest such case, but its schedule ends at timestep 1000, which the reference
    cannot index either.)"""
    from jointimagegeneration_amd.ldm import DDIMSampler, make_ddim_timesteps
    assert make_ddim_timesteps("uniform", 15, 1000).shape[0] == 16
    for k in (1, 3, 100):
        assert g[f"idx_ddim_15_{k}"].tolist() == [-1] + logged(16, k) == g[f"idx_plms_15_{k}"].tolist()

    def run(s, **kw):
        return s.sample(S=15, batch_size=2, shape=(4, 8, 8), conditioning=ops_in["c"], verbose=False, x_T=ops_in["x_T"], **kw)
    check_logged_against_trace(DDIMSampler, small, run, ops_in["x_T"], 16, captured=True)
    z, inter = run(DDIMSampler(small), log_every_t=1)
    assert len(inter["x_inter"]) == 1 + 16 and torch.equal(inter["x_inter"][-1], z)
    _, xs, _ = traced(DDIMSampler, small, run)
    assert torch.equal(inter["x_inter"][1], xs[0])            # the entry after the first step


def test_logging_under_quantize_x0_and_patch_wise_sampling(dev, small, ops_in):
    from jointimagegeneration_amd.ldm import DDIMSampler, LatentDiffusion
    from util import AE_SMALL, LDM_SMALL, seeded
    loss = dict(target="torch.nn.Identity")
    vq = LatentDiffusion(first_stage_config=dict(target="ldm.models.autoencoder.VQModelInterface",
                                                 params=dict(embed_dim=4, n_embed=256, dims=2, ddconfig=dict(AE_SMALL), lossconfig=loss)),
                         cond_stage_config=dict(target="ldm.models.autoencoder.AutoencoderKL",
                                                params=dict(embed_dim=4, dims=2, ddconfig=dict(AE_SMALL, in_channels=2, out_ch=2), lossconfig=loss)),
                         unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(LDM_SMALL)),
                         linear_start=0.0015, linear_end=0.0195, timesteps=1000, image_size=8, channels=4, dims=2, first_stage_key="image",
                         cond_stage_key="mask", num_timesteps_cond=1)
    vq = seeded(vq, "ldm_pipe.").to(dev)
    check_logged_against_trace(DDIMSampler, vq, lambda s, **k: sampler_run(s, ops_in, quantize_x0=True, **k), ops_in["x_T"], 5, captured=True)
    # the logged predictions are the quantised ones: the first is the quantiser's output for the unquantised chain's first prediction
    # (the same x_T and eps; gg_ddim_step, not the head conv's epilogue, so that the prediction has gg_ddim_step_vq's bits)
    _, inter = sampler_run(DDIMSampler(vq), ops_in, quantize_x0=True, log_every_t=1)
    plain = DDIMSampler(vq)
    plain.use_graph, plain.fuse_ddim = False, False
    _, inter_p = sampler_run(plain, ops_in, log_every_t=1)
    assert torch.equal(inter["pred_x0"][1], vq.first_stage_model.quantize(inter_p["pred_x0"][1])[0])
    assert not torch.equal(inter["pred_x0"][1], inter_p["pred_x0"][1])
    # patch-wise: a 12 x 12 latent in 8 x 8 crops at stride 4
    gen = torch.Generator().manual_seed(12)
    c12, x12 = (torch.randn(2, 4, 12, 12, generator=gen).to(dev) for _ in range(2))

    def run(s, **kw):
        return s.sample(S=5, batch_size=2, shape=(4, 12, 12), conditioning=c12, verbose=False, x_T=x12, **kw)
    small.split_input_params = dict(ks=(8, 8), stride=(4, 4), vqf=4, patch_distributed_vq=True, tie_braker=False, clip_max_weight=0.5,
                                    clip_min_weight=0.01, clip_max_tie_weight=0.5, clip_min_tie_weight=0.01)
    key = small.cond_stage_key
    small.cond_stage_key = "segmentation"                    # a key whose concat conditioning is cut into crops (ddpm.py:930)
    try:
        check_logged_against_trace(DDIMSampler, small, run, x12, 5, captured=True)
    finally:
        del small.split_input_params
        small.cond_stage_key = key


def test_quantize_denoised_with_clip_and_with_an_x0_model(dev, ops_in):
    """quantize_denoised where gg_ddim_step_vq does not apply: the logged prediction is quantise(clamp(x_recon)) -- after clip and after
    quantisation (ddpm.py:1079-1082) -- and one step from x_T is the posterior mean of that prediction, bit for bit."""
    from jointimagegeneration_amd.ldm import LatentDiffusion
    from util import AE_SMALL, LDM_SMALL, seeded
    loss = dict(target="torch.nn.Identity")

    def build(**kw):
        m = LatentDiffusion(first_stage_config=dict(target="ldm.models.autoencoder.VQModelInterface",
                                                    params=dict(embed_dim=4, n_embed=256, dims=2, ddconfig=dict(AE_SMALL), lossconfig=loss)),
                            cond_stage_config=dict(target="ldm.models.autoencoder.AutoencoderKL",
                                                   params=dict(embed_dim=4, dims=2, ddconfig=dict(AE_SMALL, in_channels=2, out_ch=2), lossconfig=loss)),
                            unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(LDM_SMALL)),
                            linear_start=0.0015, linear_end=0.0195, timesteps=20, image_size=8, channels=4, dims=2, first_stage_key="image",
                            cond_stage_key="mask", num_timesteps_cond=1, **kw)
        return seeded(m, "ldm_pipe.").to(dev)
    for m, clip in ((build(), True), (build(parameterization="x0"), False), (build(parameterization="x0"), True)):
        m.clip_denoised = clip
        x_T = 1.5 * ops_in["x_T"]
        run = lambda **kw: m.progressive_denoising(ops_in["c"], SHAPE, verbose=False, x_T=x_T, noise_tape=ops_in["step"], **kw)
        _, plain = run(log_every_t=20)                        # the first entry: timestep 19, one step from x_T, not quantised
        z, inter = run(log_every_t=20, quantize_denoised=True)
        want = m.first_stage_model.quantize(plain[0])[0]
        assert torch.equal(inter[0], want) and not torch.equal(inter[0], plain[0])
        if clip and m.parameterization == "eps":
            assert float(plain[0].abs().max()) == 1.0         # the clip is active on this start latent
        # start_T = 1: the single step at t = 0, where the posterior mean is coef1 * x_recon + coef2 * x and sigma is 0
        z1, one = run(start_T=1, log_every_t=1, quantize_denoised=True)
        assert len(one) == 1 and torch.equal(z1, m.posterior_mean_coef1[0] * one[0] + m.posterior_mean_coef2[0] * x_T)
        z20, _ = run(log_every_t=20, quantize_denoised=True, mask=ops_in["mask_hole"], x0=ops_in["x0"], mask_noise_tape=ops_in["q"])
        assert bool(torch.isfinite(z20).all()) and bool(torch.isfinite(z).all())


def test_progressive_denoising_ends_in_the_img_of_p_sample_loop(dev, m20, ops_in):
    z = m20.p_sample_loop(ops_in["c"], SHAPE, x_T=ops_in["x_T"], verbose=False, noise_tape=ops_in["step"])
    z_p, inter = m20.progressive_denoising(ops_in["c"], SHAPE, verbose=False, x_T=ops_in["x_T"], log_every_t=20, noise_tape=ops_in["step"])
    assert torch.equal(z, z_p) and len(inter) == 2            # timesteps 19 and 0
    z_m = m20.p_sample_loop(ops_in["c"], SHAPE, x_T=ops_in["x_T"], verbose=False, noise_tape=ops_in["step"], mask=ops_in["mask_hole"],
                            x0=ops_in["x0"], mask_noise_tape=ops_in["q"])
    z_pm, _ = m20.progressive_denoising(ops_in["c"], SHAPE, verbose=False, x_T=ops_in["x_T"], log_every_t=20, noise_tape=ops_in["step"],
                                        mask=ops_in["mask_hole"], x0=ops_in["x0"], mask_noise_tape=ops_in["q"])
    assert torch.equal(z_m, z_pm)
    # start_T shortens the chain to its last timesteps
    z_s, inter_s = m20.progressive_denoising(ops_in["c"], SHAPE, verbose=False, x_T=ops_in["x_T"], start_T=5, log_every_t=2,
                                             noise_tape=ops_in["step"])
    assert len(inter_s) == len(logged(5, 2))
    assert torch.equal(z_s, m20.p_sample_loop(ops_in["c"], SHAPE, x_T=ops_in["x_T"], verbose=False, start_T=5, noise_tape=ops_in["step"]))


def test_progressive_noise_dropout_and_temperature_equal_the_same_ops_on_the_tape(dev, m20, ops_in):
    """As test_vq_gpu.py checks DDIM's: the run with noise_dropout equals the run on the tape that went through the same dropout (same
    device seed); a scalar temperature of 0.5 (an int-free power of two) equals the run on the pre-multiplied tape."""
    tape = ops_in["step"]

    def run(**kw):
        return m20.progressive_denoising(ops_in["c"], SHAPE, verbose=False, x_T=ops_in["x_T"], log_every_t=20, **kw)[0]
    torch.cuda.manual_seed(4321)
    z_d = run(noise_tape=tape, temperature=0.5, noise_dropout=0.3)
    torch.cuda.manual_seed(4321)
    dropped = [torch.nn.functional.dropout(n * 0.5, p=0.3) for n in tape]
    assert all(bool((d == 0).any()) for d in dropped)
    z_m = run(noise_tape=dropped)
    z_1 = run(noise_tape=tape)
    assert torch.equal(z_d, z_m) and not torch.equal(z_d, z_1)
    assert torch.equal(run(noise_tape=tape, temperature=1), z_1)                                  # an int temperature is accepted
    assert torch.equal(run(noise_tape=tape, temperature=0.5), run(noise_tape=[n * 0.5 for n in tape]))
    with pytest.raises(ValueError, match="temperature holds 3 values"):
        run(noise_tape=tape, temperature=[1.0, 1.0, 1.0])


def test_denoise_row_tiles_one_row_per_sample(dev, m20, ops_in):
    from jointimagegeneration_amd import ops, render
    _, inter = m20.progressive_denoising(ops_in["c"], SHAPE, verbose=False, x_T=ops_in["x_T"], log_every_t=10, noise_tape=ops_in["step"])
    row = m20.denoise_row(inter, value_range=(-1.0, 1.0))
    dec = torch.stack([m20.decode_first_stage(z) for z in inter])                  # n b c h w
    n, b = dec.shape[:2]
    Hg, Wg = ops.make_grid_extent(b * n, dec.shape[-2], dec.shape[-1], n, 2)
    assert row.dtype == torch.uint8 and tuple(row.shape) == (Hg, Wg, 3)
    order = torch.stack([dec[j, i] for i in range(b) for j in range(n)])           # (b n)
    want = render.make_grid((torch.clamp((order + 1.0) / 2.0, 0.0, 1.0) * 255.0).contiguous(), nrow=n)
    assert torch.equal(row, want)
    raw = m20.denoise_row(inter)                             # the default: the decoded values as they are, as in the reference
    assert torch.equal(raw, render.make_grid(order.contiguous(), nrow=n))


# ------------------------------------------------------------------------------------------------ entry point
def test_sample_diffusion_progress_png_end_to_end(dev, tmp_path, monkeypatch):
    """`sample_diffusion -v --progress-png --log-every-t 10` on the 20-timestep model: the NIfTI file as without the flag, and beside it
    the denoise row of the last generated slice (3 logged timesteps, one sample) as an 8-bit RGB PNG."""
    import os
    import struct
    import zlib
    from jointimagegeneration_amd import ops, sample_diffusion as sd
    m = ldm_small(20, use_ema=False).to(dev)
    (tmp_path / "m.yaml").write_text("model:\n  target: none\n")
    monkeypatch.setattr(sd, "load_model", lambda config, ckpt: (m, 7))
    monkeypatch.chdir(tmp_path)
    rows = []
    real = type(m).denoise_row
    monkeypatch.setattr(type(m), "denoise_row", lambda self, samples, **kw: rows.append((len(samples), real(self, samples, **kw))) or rows[-1][1])
    sd.main(["--config", str(tmp_path / "m.yaml"), "--slices", "4", "--size", "32", "-v", "--progress-png", "--log-every-t", "10"])
    out = tmp_path / "samples" / "00000007"
    assert sorted(os.listdir(out)) == ["sample_0000.nii.gz", "sample_progress.png"]
    assert len(rows) == 1 and rows[0][0] == len(logged(20, 10)) == 3
    Hg, Wg = ops.make_grid_extent(3, 32, 32, 3, 2)
    raw = (out / "sample_progress.png").read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", raw[16:24]) == (Wg, Hg)
    pos, idat = 8, b""
    while pos < len(raw):                                    # chunks: length, type, data, crc
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        if kind == b"IDAT":
            idat += raw[pos + 8:pos + 8 + n]
        pos += 12 + n
    pix = torch.frombuffer(bytearray(zlib.decompress(idat)), dtype=torch.uint8).view(Hg, 1 + 3 * Wg)[:, 1:].reshape(Hg, Wg, 3)
    assert torch.equal(pix, rows[0][1].cpu())
    # without the new flags the program writes what it wrote before
    sd.main(["--config", str(tmp_path / "m.yaml"), "--slices", "4", "--size", "32", "-v", "-l", str(tmp_path / "plain")])
    assert sorted(os.listdir(tmp_path / "plain" / "samples" / "00000007")) == ["sample_0000.nii.gz"]


def test_logging_works_with_3d_latents_and_eta(dev):
    """[N, C, D, H, W] latents (the dims = 3 UNet of the volumetric fixtures, no first stage): a logged eta = 0 chain, captured, equals
    the eager one and ends in the unlogged call's tensors; with eta > 0 and a mask the lists hold S + 1 volumes and end in z."""
    import json
    import os
    from jointimagegeneration_amd.ldm import DDIMSampler, LatentDiffusion
    from util import GOLD, seeded
    with open(os.path.join(GOLD, "ae3d_surface.json")) as f:
        meta = json.load(f)
    unet = dict(meta["unet3d"])
    m = LatentDiffusion(first_stage_config="__is_no_first_stage__", cond_stage_config=dict(target="ldm.modules.encoders.modules.IdentityEncoder"),
                        unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=unet), linear_start=0.0015,
                        linear_end=0.0195, timesteps=meta["timesteps"], image_size=6, channels=4, dims=3, use_ema=False,
                        first_stage_key="image", cond_stage_key="mask", num_timesteps_cond=1, conditioning_key="concat")
    m = seeded(m, "ldm3d.").to(dev)
    lat = (2, 4, 4, 6, 6)
    gen = torch.Generator().manual_seed(31)
    c = torch.randn((2, unet["in_channels"] - 4) + lat[2:], generator=gen).to(dev)
    x_T, x0 = (torch.randn(lat, generator=gen).to(dev) for _ in range(2))
    tape = [torch.randn(lat, generator=gen).to(dev) for _ in range(5)]

    def run(s, **kw):
        return s.sample(S=5, batch_size=2, shape=lat[1:], conditioning=c, verbose=False, x_T=x_T, dims=3, **kw)
    s, se = DDIMSampler(m), DDIMSampler(m)
    se.use_graph = False
    z_e, inter_e = run(se, log_every_t=2)
    z_u, inter_u = run(se)
    assert torch.equal(z_e, z_u) and torch.equal(inter_e["pred_x0"][-1], inter_u["pred_x0"][1])
    for call in range(3):                                    # eager, captured, replayed
        z, inter = run(s, log_every_t=2)
        assert torch.equal(z, z_e) and lists_equal(inter, inter_e), call
    assert [tuple(e.shape) for e in inter["x_inter"]] == [lat] * 4 and torch.equal(inter["x_inter"][-1], z)
    mask = (torch.rand((2, 1) + lat[2:], generator=gen) > 0.5).float().to(dev)
    z, inter = run(s, log_every_t=1, eta=0.7, noise_tape=tape, mask=mask, x0=x0, mask_noise_tape=tape)
    z2, inter2 = run(se, eta=0.7, noise_tape=tape, mask=mask, x0=x0, mask_noise_tape=tape)
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == 6 and torch.equal(inter["x_inter"][-1], z)
    assert torch.equal(z, z2) and torch.equal(inter["pred_x0"][-1], inter2["pred_x0"][1])
