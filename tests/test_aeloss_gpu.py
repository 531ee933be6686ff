"""GPU suite of the first stage's held-out objective (csrc/gg_patchgan.hip, jointimagegeneration_amd/aeloss.py, ldm.AutoencoderKL, ae_eval).

Exact part, no tolerance (the manner of tests/conv_exact.py regime D): activations in {+-1..+-4}, weights in {+-1..+-4}/8, alpha in
{+-0.5, +-1, +-2}, integer beta.  Every product and partial sum is a multiple of 1/8 below 2^24 / 16, acc * alpha and + beta are exact,
so the only rounding of the whole convolution is the LeakyReLU product y * fl32(0.2), rounded once: the fp32 output must equal
fl32(fp64 closed form) bit for bit, the bf16 output its round-to-nearest-even.

Bounds of the rest (every tol_<kind> is the largest distance of the reference's own fp32 value from the fp64 restatement,
recorded by tests/golden/make_golden_aeloss.py):
  reductions, fp32 discriminators, pixel / KL / nll terms   4 x tol_<kind>   (the project's rule of 7k: ATen and the kernel sum in
                                                                             different orders, both a few fp32 roundings from fp64)
  bf16 discriminator after L convolutions                   (1 + 1.5e-2)^L - 1, max-norm relative to max |value|   (1.5e-2: what
                                                                             tests/test_hip_parity.py holds one bf16 ops.conv to)
  scalar logs of a discriminator                            that bound times max |logit|   (mean, ReLU, softplus are 1-Lipschitz)
  LPIPS term                                                RTOL / BF16_BOUND of tests/test_lpips_gpu.py
combined linearly with the recorded weights."""
import contextlib
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aeloss_ref as A  # noqa: E402
import lpips_ref  # noqa: E402
from util import AE_SMALL, GOLD, seeded  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LPIPS_RTOL, LPIPS_BF16 = 2e-5, 2.26e-3        # RTOL, BF16_BOUND of tests/test_lpips_gpu.py
BF16_CONV = 1.5e-2                            # one bf16 ops.conv, tests/test_hip_parity.py
LOSS = "ldm.modules.losses.LPIPSWithDiscriminator"
LIMIT = 1 << 24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from jointimagegeneration_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "aeloss.npz")))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLD, "aeloss_surface.json")) as f:
        return json.load(f)


def relmax(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------------ exact convolutions
# name, kd, cin, cout, stride, (D, H, W)
EXACT = [
    ("d2_1to64_s2_16x20", 1, 1, 64, 2, (1, 16, 20)),
    ("d2_1to64_s2_17x21", 1, 1, 64, 2, (1, 17, 21)),
    ("d2_64to128_s2_9x11", 1, 64, 128, 2, (1, 9, 11)),
    ("d2_256to512_s1_3x4", 1, 256, 512, 1, (1, 3, 4)),             # output larger than input: every border tap padded
    ("d2_512to1_s1_4x5", 1, 512, 1, 1, (1, 4, 5)),                 # Cout_pad 32, one logical channel
    ("d3_1to64_s2_4x16x20", 4, 1, 64, 2, (4, 16, 20)),
    ("d3_64to128_s2_3x9x11", 4, 64, 128, 2, (3, 9, 11)),
    ("d3_512to64_s1_2x3x4", 4, 512, 64, 1, (2, 3, 4)),             # K = 64 x 512 products
]
NMAX = 3
_exact_cache = {}


def _signed(g, shape, hi):
    return torch.randint(1, hi + 1, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def exact_inputs(case):
    """(x [N, cin, D, H, W], w [cout, cin, kd, 4, 4], alpha [cout], beta [cout], acc fp64 [N, cout, Do, Ho, Wo]) with the preconditions
    asserted; built once per case and never changed."""
    name, kd, cin, cout, stride, sp = case
    if name not in _exact_cache:
        g = torch.Generator().manual_seed(sum(name.encode()))
        x = _signed(g, (NMAX, cin) + sp, 4)
        w = _signed(g, (cout, cin, kd, 4, 4), 4) / 8
        alpha = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=g)] * (torch.randint(0, 2, (cout,), generator=g).float() * 2 - 1)
        beta = torch.randint(-8, 9, (cout,), generator=g).float()
        K = cin * kd * 16
        assert bool((x != 0).all()) and bool((w != 0).all()) and float(x.abs().max()) <= 4 and float((w * 8).abs().max()) <= 4
        assert torch.equal(w * 8, (w * 8).round()) and torch.equal(x, x.to(torch.bfloat16).float()) and torch.equal(w, w.to(torch.bfloat16).float())
        assert (4 * K + 8) * 16 < LIMIT, f"{name}: the sums do not fit fp32"        # |acc| <= 2 K, |y| <= 4 K + 8, in quanta of 1/16 (alpha = 0.5)
        pad = (2 if kd == 4 else 0, 2, 2)
        acc = F.conv3d(x.double(), w.double(), None, stride=(stride if kd == 4 else 1, stride, stride), padding=pad)
        assert torch.equal(acc * 8, (acc * 8).round()) and float(acc.abs().max()) * 16 < LIMIT
        assert tuple(acc.shape[2:]) == ((sp[0] // stride + 1) if kd == 4 else sp[0], sp[1] // stride + 1, sp[2] // stride + 1)
        _exact_cache[name] = (x, w, alpha, beta, acc)
    return _exact_cache[name]


def closed_form(acc, alpha, beta, slope):
    """fp32 [N, Do, Ho, Wo, cout]: y = acc * alpha + beta (exact), LeakyReLU product rounded once to fp32."""
    y = acc.permute(0, 2, 3, 4, 1)
    if alpha is not None:
        y = y * alpha.double()
    y = y + beta.double()
    assert torch.equal(y, y.float().double())
    if slope != 1.0:
        y = torch.where(y >= 0, y, (y * float(np.float32(slope))).float().double())      # two fp32 factors: the fp64 product is exact
    return y.float()


@pytest.mark.parametrize("entry", ["bf16", "f32"])
@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_patch_conv_exact(dev, case, entry):
    from jointimagegeneration_amd import ops
    name, kd, cin, cout, stride, sp = case
    x, w, alpha, beta, acc = exact_inputs(case)
    cp = ops.pad32(cout)
    wk = w if kd == 4 else w[:, :, 0]

    def padded(v):
        out = torch.zeros(cp)
        out[:cout] = v
        return out.to(dev)
    for N in (1, NMAX):
        xd = x[:N].to(dev)
        if entry == "f32":
            with ops.fp32_validation():
                src, pw = ops.to_cl(xd), ops.pack_conv_weight(wk.to(dev), ops.pad32(cin))
            assert src.t.dtype == torch.float32 and pw.dtype == torch.float32
        else:
            src, pw = ops.to_cl(xd), ops.pack_conv_weight(wk.to(dev), ops.pad32(cin))
            assert src.t.dtype == torch.bfloat16 and pw.dtype == torch.bfloat16
        for use_alpha in (True, False):
            for slope in (0.2, 1.0):
                want = closed_form(acc[:N], alpha if use_alpha else None, beta, slope)
                for out_f32 in ((True,) if entry == "f32" else (True, False)):
                    got = ops.patch_conv(src, pw, padded(alpha) if use_alpha else None, padded(beta), cout, kd, stride, slope=slope, out_f32=out_f32)
                    t = got.t.cpu()
                    what = f"{name} {entry} N={N} alpha={use_alpha} slope={slope} out_f32={out_f32}"
                    assert tuple(t.shape) == tuple(want.shape[:-1]) + (cp,), what
                    assert not bool((t[..., cout:] != 0).any()), what + ": pad lanes"
                    exp = want if out_f32 else want.to(torch.bfloat16)
                    bad = (t[..., :cout] != exp) | torch.isnan(t[..., :cout].float())
                    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} differ, first {bad.nonzero()[:3].tolist()}"


# ------------------------------------------------------------------------------------------------ posterior kernels and reductions
def moment_rows(rows, seed):
    """fp32 channels-last moments [3, 1, 1, rows, 32] (C = 4: mean lanes 0..3, logvar lanes 4..7, the rest never read) with both clamp edges
    in every sample, and noise [3, 4, 1, 1, rows]."""
    g = torch.Generator().manual_seed(seed)
    mom = torch.randn((3, 1, 1, rows, 32), generator=g)
    for n in range(3):
        mom[n, 0, 0, 3 + n, 5], mom[n, 0, 0, rows - 2, 7], mom[n, 0, 0, rows // 2, 4] = -40.0, 25.0, 25.0
    return mom.contiguous(), torch.randn((3, 4, 1, 1, rows), generator=g)


def nc_moments(mom):
    """the [N, 2C, *sp] form the restatement takes"""
    return mom[..., :8].permute(0, 4, 1, 2, 3).double()


@pytest.mark.parametrize("rows", [35, 257, 4096])
def test_gauss_kl_and_sample_rows(dev, gold, rows):
    from jointimagegeneration_amd import ops
    mom, noise = moment_rows(rows, 5 + rows)
    md, nd = mom.to(dev), noise.to(dev)
    kl = ops.gauss_kl_rows(md, 4)
    assert kl.dtype == torch.float64 and tuple(kl.shape) == (3,) and torch.equal(kl, ops.gauss_kl_rows(md, 4))          # two runs, the same bits
    want = A.gauss_kl(nc_moments(mom))
    d = float(((kl.cpu() - want).abs() / want.abs()).max())
    print(f"gauss_kl_rows rows={rows}: distance {d:.3e} (bound {4 * float(gold['tol_kl']):.3e})")
    assert d <= 4 * float(gold["tol_kl"])
    z = ops.gauss_sample_rows(md, 4, nd)
    z_rows = torch.zeros((3, 1, 1, rows, 32), dtype=torch.bfloat16, device=dev)
    z32 = torch.full((3, 1, 1, rows, 32), 7.0, dtype=torch.float32, device=dev)
    ops.gauss_sample_rows(md, 4, nd, out=None, z_in=z_rows)
    z2 = ops.gauss_sample_rows(md, 4, nd, out=torch.empty_like(nd), z_in=z32)
    assert torch.equal(z, z2)
    zr = z.permute(0, 2, 3, 4, 1)
    assert torch.equal(z_rows[..., :4], zr.to(torch.bfloat16)) and not bool((z_rows[..., 4:] != 0).any())               # other lanes untouched
    assert torch.equal(z32[..., :4], zr) and bool((z32[..., 4:] == 7.0).all())
    wz = A.gauss_sample(nc_moments(mom), noise.double())
    d = relmax(z.cpu().numpy(), wz.numpy())
    print(f"gauss_sample_rows rows={rows}: distance {d:.3e} (bound {4 * float(gold['tol_sample']):.3e})")
    assert d <= 4 * float(gold["tol_sample"])


def test_gauss_sample_rows_exact_points_and_clamp_edges(dev, gold):
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(3)
    mom = torch.zeros((2, 1, 1, 70, 32))
    mom[..., :4] = torch.randn((2, 1, 1, 70, 4), generator=g)
    noise = torch.randn((2, 4, 1, 1, 70), generator=g)
    z = ops.gauss_sample_rows(mom.to(dev), 4, noise.to(dev)).cpu()
    assert torch.equal(z, mom[..., :4].permute(0, 4, 1, 2, 3) + noise)                                  # logvar 0: std is exactly 1
    mom[..., :4] = 0
    mom[0, ..., 4:8], mom[1, ..., 4:8] = -40.0, 25.0                                                    # clamped to -30 and 20
    z = ops.gauss_sample_rows(mom.to(dev), 4, noise.to(dev)).cpu().double()
    bound = 4 * float(gold["tol_sample"])
    for n, e in ((0, np.exp(-15.0)), (1, np.exp(10.0))):
        assert float(((z[n] - e * noise[n].double()).abs() / (e * noise[n].double().abs())).max()) <= bound


@pytest.mark.parametrize("rows", [35, 257, 4096])
def test_logit_stats(dev, gold, rows):
    from jointimagegeneration_amd import ops
    g = torch.Generator().manual_seed(11 + rows)
    l = torch.zeros((3, 1, 1, rows, 32))
    l[..., 0] = 0.4 + 1.5 * torch.randn((3, 1, 1, rows), generator=g)
    l[..., 1:] = 100.0                                                                                  # only lane 0 is a logit
    l[0, 0, 0, 0, 0], l[1, 0, 0, 1, 0] = 30.0, -30.0                                                    # beyond softplus's threshold
    ld = l.to(dev)
    got = ops.logit_stats(ld)
    assert got.dtype == torch.float64 and tuple(got.shape) == (5,) and torch.equal(got, ops.logit_stats(ld))
    want = A.logit_stats(l[..., 0].double().reshape(-1))
    d = float(((got.cpu() - want).abs() / want.abs()).max())
    print(f"logit_stats rows={rows}: distance {d:.3e} (bound {4 * float(gold['tol_logit']):.3e})")
    assert d <= 4 * float(gold["tol_logit"])


# ------------------------------------------------------------------------------------------------ discriminators against the restatement
def disc_sd(meta, dims, which, nl):
    interm = dims == 3 or which == "ct"
    return A.seeded_disc_state_dict(3 if which == "ct" else 2, 1, nl, interm, 1000 * dims + 100 * (which == "ct") + nl,
                                    meta["gains"][f"dims{dims}_{which}_layers{nl}"])


def frames(t, dims):
    n = t.shape[0] * t.shape[1]
    t = t.reshape((n, 1) + tuple(t.shape[2:]))
    return t.reshape((-1, 1) + tuple(t.shape[3:])) if dims == 3 else t


_restated = {}


def restated_blocks(gold, meta, dims, which, nl, tensor):
    """fp64 block outputs of a discriminator on the fixture's inputs ('x') or reconstructions ('y'), computed once."""
    key = (dims, which, nl, tensor)
    if key not in _restated:
        t = frames(torch.from_numpy(gold[f"{tensor}{dims}"]).double(), dims if which == "frame" else 2)
        _restated[key] = (t, A.disc_forward(t, disc_sd(meta, dims, which, nl), nl, dims == 3 or which == "ct"))
    return _restated[key]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("dims,which,nl", [(2, "frame", 3), (2, "frame", 2), (3, "frame", 3), (3, "ct", 3), (3, "ct", 2)])
def test_discriminator_blocks(dev, gold, meta, dims, which, nl, mode):
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.aeloss import NLayerDiscriminator, NLayerDiscriminator3D
    interm = dims == 3 or which == "ct"
    cls = NLayerDiscriminator3D if which == "ct" else NLayerDiscriminator
    disc = cls(1, n_layers=nl, getIntermFeat=interm).eval()
    disc.load_state_dict(disc_sd(meta, dims, which, nl))
    disc = disc.to(dev)
    y, want = restated_blocks(gold, meta, dims, which, nl, "y")
    yd = y.float().to(dev)
    with (ops.fp32_validation() if mode == "fp32" else contextlib.nullcontext()):
        res = disc(yd)
        blocks = [ops.from_cl(o, disc.DIMS) for o in disc.run_cl(ops.to_cl(yd))]        # every block, also where forward returns the logits alone
    logits, outs = (res[0], res[1]) if interm else (res, None)
    assert tuple(logits.shape) == tuple(want[-1].shape) and logits.dtype == torch.float32 and torch.equal(logits, blocks[-1])
    if interm:
        assert len(outs) == nl + 2 and all(torch.equal(a, b) for a, b in zip(outs, blocks))
    for L, (got, w) in enumerate(zip(blocks, want), 1):
        bound = 4 * float(gold["tol_block"]) if mode == "fp32" else (1 + BF16_CONV) ** L - 1
        d = relmax(got.cpu().numpy(), w.numpy())
        print(f"discriminator dims={dims} {which} layers={nl} {mode} block {L}: distance {d:.3e} (bound {bound:.3e})")
        assert d <= bound


# ------------------------------------------------------------------------------------------------ loss module, teacher-forced
def build_loss(gold, meta, case, dev):
    from jointimagegeneration_amd.aeloss import LPIPSWithDiscriminator
    from jointimagegeneration_amd.lpips import map_vgg_state_dict
    cfg, dims = case["cfg"], case["dims"]
    m = LPIPSWithDiscriminator(dims=dims, **cfg).eval()
    sd = dict(map_vgg_state_dict(lpips_ref.seeded_vgg_state_dict()))
    sd.update({f"lin{k}.model.1.weight": torch.from_numpy(gold[f"lin{k}"]).reshape(1, -1, 1, 1) for k in range(5)})
    m.perceptual_loss.load_state_dict(sd, strict=False)
    m.frame_discriminator.load_state_dict(disc_sd(meta, dims, "frame", cfg["disc_num_layers"]))
    if dims == 3:
        m.ct_discriminator.load_state_dict(disc_sd(meta, dims, "ct", cfg["disc_num_layers"]))
    return m.to(dev)


def key_bounds(gold, meta, case, mode):
    """Absolute bound per key of both dicts, from the docstring's rules, on the fp64 restatement's values."""
    cfg, dims, name = case["cfg"], case["dims"], case["name"]
    nl, pw = cfg["disc_num_layers"], cfg["perceptual_weight"]
    f0 = dict(zip(case["keys0"], gold[f"{name}_f64_0"]))
    f1 = dict(zip(case["keys1"], gold[f"{name}_f64_1"]))
    t_nll, t_kl, t_logit = (4 * float(gold[f"tol_{k}"]) for k in ("nll", "kl", "logit"))
    x, y = (torch.from_numpy(gold[f"{k}{dims}"]).double() for k in ("x", "y"))
    pix = float((x - y).abs().mean() if (dims == 2 or cfg["pixel_loss"] == "l1") else ((x - y) ** 2).mean())
    p_max = float(gold[f"p{dims}_f64"].max())                      # the LPIPS bounds are max-norm relative to the largest per-image value
    rec_b = t_nll * pix + (pw * (LPIPS_RTOL if mode == "fp32" else LPIPS_BF16) * p_max if pw > 0 else 0.0) + t_nll * abs(f0["val/rec_loss"])
    S = x[0, 0].numel()
    nll_b = S / np.exp(cfg["logvar_init"]) * rec_b + t_nll * abs(f0["val/nll_loss"]) if dims == 2 else rec_b
    kl_b = t_kl * abs(f0["val/kl_loss"])
    L = nl + 2
    block = 4 * float(gold["tol_block"]) if mode == "fp32" else (1 + BF16_CONV) ** L - 1
    disc_b = 0.0
    for which in (("frame",) if dims == 2 else ("frame", "ct")):
        for tensor in ("x", "y"):
            lmax = float(restated_blocks(gold, meta, dims, which, nl, tensor)[1][-1].abs().max())
            disc_b = max(disc_b, block * lmax)
    disc_b += t_logit * max(abs(v) for k, v in f1.items() if "logits" in k)
    factor = f0["val/disc_factor"]
    b = {"val/total_loss": nll_b + cfg["kl_weight"] * kl_b + t_nll * abs(f0["val/total_loss"]), "val/logvar": 0.0, "val/kl_loss": kl_b,
         "val/nll_loss": nll_b, "val/rec_loss": rec_b, "val/d_weight": 0.0, "val/disc_factor": 0.0, "val/g_loss": disc_b, "val/gan_feat_loss": 0.0,
         "val/disc_loss": factor * disc_b}
    b.update({k: disc_b for k in f1 if "logits" in k})
    return b


def case_ids():
    with open(os.path.join(GOLD, "aeloss_surface.json")) as f:
        return [c["name"] for c in json.load(f)["cases"]]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", case_ids())
def test_loss_module_teacher_forced(dev, gold, meta, name, mode):
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import DiagonalGaussianDistribution
    case = next(c for c in meta["cases"] if c["name"] == name)
    dims = case["dims"]
    m = build_loss(gold, meta, case, dev)
    x, y, mom = (torch.from_numpy(gold[f"{k}{dims}"]).to(dev) for k in ("x", "y", "mom"))

    def run():
        post = DiagonalGaussianDistribution(mom)
        l0, d0 = m(x, y, post, 0, case["step"], last_layer=None, split="val")
        l1, d1 = m(x, y, post, 1, case["step"], last_layer=None, split="val")
        return l0, d0, l1, d1
    if mode == "fp32":
        with ops.fp32_validation():
            l0, d0, l1, d1 = run()
    else:
        l0, d0, l1, d1 = run()
    assert list(d0) == case["keys0"] and list(d1) == case["keys1"]
    for v in list(d0.values()) + list(d1.values()) + [l0, l1]:
        assert v.is_cuda and v.dim() == 0 and v.dtype == torch.float32
    assert torch.equal(l0, d0["val/total_loss"]) and torch.equal(l1, d1["val/disc_loss"])
    assert float(d0["val/d_weight"]) == 0.0 and float(d0["val/disc_factor"]) == (1.0 if case["step"] >= meta["disc_start"] else 0.0)
    assert float(d0["val/logvar"]) == float(np.float32(case["cfg"]["logvar_init"]))
    bounds = key_bounds(gold, meta, case, mode)
    worst = {}
    for tag, d in (("0", d0), ("1", d1)):
        for (k, v), ref in zip(d.items(), gold[f"{name}_ref{tag}"]):
            err = abs(float(v) - float(ref))
            print(f"{name} {mode} {k}: got {float(v)!r} reference {float(ref)!r} |diff| {err:.3e} bound {bounds[k]:.3e}")
            if err > bounds[k]:
                worst[k] = (float(v), float(ref), err, bounds[k])
    assert not worst, worst


# ------------------------------------------------------------------------------------------------ whole path
def ae_with_loss(dims, dev):
    from jointimagegeneration_amd.ldm import AutoencoderKL
    if dims == 2:
        dd = dict(AE_SMALL)
    else:
        with open(os.path.join(GOLD, "ae3d_surface.json")) as f:
            dd = dict(json.load(f)["ae3d"])
    loss = dict(target=LOSS, params=dict(disc_start=3, kl_weight=1e-6, disc_in_channels=1, gan_feat_weight=0, dims=dims))
    m = seeded(AutoencoderKL(ddconfig=dd, lossconfig=loss, embed_dim=4, dims=dims), f"aeloss{dims}.")
    m.global_step = 3
    return m.to(dev)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("dims", [2, 3])
def test_whole_path_is_the_composition_of_its_parts(dev, meta, dims, mode):
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd.ldm import nc_to_rows
    m = ae_with_loss(dims, dev)
    g = torch.Generator().manual_seed(17 + dims)
    x = (torch.rand((2, 1) + ((32, 32) if dims == 2 else (4, 16, 16)), generator=g) * 2 - 1).to(dev)
    e = torch.randn(m.latent_shape(x.shape), generator=g).to(dev)
    with (ops.fp32_validation() if mode == "fp32" else contextlib.nullcontext()):
        rec, post = m(x, noise=e)
        assert tuple(rec.shape) == tuple(x.shape) and tuple(post.mean.shape) == tuple(e.shape)
        z = ops.gauss_sample_rows(nc_to_rows(m.encode(x).parameters).contiguous(), 4, e)
        assert torch.equal(rec, m.decode(z))
        assert torch.equal(m(x, sample_posterior=False)[0], m.decode(post.mode().contiguous()))
        logs = m.validation_losses(x, noise=e)
        _, d0 = m.loss(x, rec, post, 0, m.global_step, split="val")
        _, d1 = m.loss(x, rec, post, 1, m.global_step, split="val")
        assert m.validation_step({m.image_key: nc_to_rows(x).contiguous()}, 0).keys() == logs.keys()
        before = m.validation_losses(x, noise=e, global_step=2)
    ref_case = next(c for c in meta["cases"] if c["dims"] == dims)
    assert list(logs) == ref_case["keys0"] + ref_case["keys1"]                                          # the reference's key set
    for k, v in {**d0, **d1}.items():
        assert torch.equal(logs[k], v), k
        assert bool(torch.isfinite(v)), k
    assert float(logs["val/disc_factor"]) == 1.0 and float(before["val/disc_factor"]) == 0.0 and float(before["val/disc_loss"]) == 0.0
    assert float(logs["val/disc_loss"]) != 0.0 and float(logs["val/rec_loss"]) > 0.0


# ------------------------------------------------------------------------------------------------ ae_eval, in process
def test_ae_eval_writes_the_mean_of_the_per_batch_losses(dev, tmp_path):
    import yaml
    from jointimagegeneration_amd import ae_eval
    from jointimagegeneration_amd.io import write_nifti
    m = ae_with_loss(2, dev)
    params = dict(embed_dim=4, dims=2, image_key="image", ddconfig=dict(AE_SMALL),
                  lossconfig=dict(target=LOSS, params=dict(disc_start=3, kl_weight=1e-6, disc_in_channels=1, gan_feat_weight=0, dims=2)))
    (tmp_path / "ae.yaml").write_text(yaml.safe_dump(dict(model=dict(target="ldm.models.autoencoder.AutoencoderKL", params=params))))
    torch.save(dict(state_dict={k: v.cpu() for k, v in m.state_dict().items()}, global_step=5), tmp_path / "ae.ckpt")
    (tmp_path / "ct").mkdir()
    vol = (torch.rand((4, 32, 32), generator=torch.Generator().manual_seed(2)) * 2 - 1).numpy().astype(np.float32)
    write_nifti(str(tmp_path / "ct" / "case0.nii.gz"), vol)
    doc = ae_eval.main(["--config", str(tmp_path / "ae.yaml"), "--ckpt", str(tmp_path / "ae.ckpt"), "--ct", str(tmp_path / "ct"),
                        "--seed", "40", "--out", str(tmp_path / "metrics.json")])
    with open(tmp_path / "metrics.json") as f:
        assert json.load(f) == doc
    assert doc["global_step"] == 5 and doc["batches"] == 4 and doc["volumes"] == ["case0.nii.gz"]
    m.global_step = 5
    logs = []
    for i in range(4):
        x = torch.from_numpy(vol[i])[None, None].to(dev)
        e = torch.randn(m.latent_shape(x.shape), generator=torch.Generator().manual_seed(40 + i)).to(dev)
        logs.append(m.validation_losses(x, noise=e))
    for k in logs[0]:
        want = logs[0][k].double()
        for l in logs[1:]:
            want = want + l[k].double()
        assert doc[k] == float(want / 4), k
    assert float(doc["val/disc_factor"]) == 1.0 and doc["val/rec_loss"] > 0
