"""GPU suite of the cond stages: the gg_cond.hip kernels against torch on the CPU (bit for bit where the arithmetic is exact), the product
modules against the reference's recorded outputs (tests/golden/cond.npz, make_golden_cond.py), and the conditioning's way into the
samplers.  Bounds: see each test; measured values are printed and recorded in DESIGN.md 7h."""

import pytest
import torch
import torch.nn.functional as F

import cond_ref
from test_cond_cpu import TE, TOKEN_SHAPES, cond_ldm, embedder
from util import T, gold, rel_err, rms_err, seeded

pytestmark = pytest.mark.gpu
GG_BF16, GG_F32, GG_ERR_BAD_SHAPE = 0, 1, -1
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return gold("cond")


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ gg_embed_rows
def raw_embed(ids, tok, pos, T_len, bf16, stride, dev):
    """gg_embed_rows at the C-ABI into a sentinel-filled buffer with 64 elements of slack; returns (rc, rows [R, stride], slack)."""
    from jointimagegeneration_amd import _lib
    R = ids.numel()
    buf = torch.full((R * stride + 64,), SENTINEL, dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
    ids_d, tok_d = ids.to(dev).int().contiguous(), tok.to(dev)
    pos_d = pos.to(dev) if pos is not None else None
    rc = _lib.load().gg_embed_rows(ids_d.data_ptr(), R, T_len, tok_d.data_ptr(), tok.shape[0], tok.shape[1],
                                   pos_d.data_ptr() if pos is not None else None, pos.shape[0] if pos is not None else 0, buf.data_ptr(),
                                   GG_BF16 if bf16 else GG_F32, stride, stream())
    torch.cuda.synchronize()
    return rc, buf[:R * stride].view(R, stride).cpu(), buf[R * stride:].cpu()


@pytest.mark.parametrize("D", [32, 48, 100, 512])
def test_embed_rows_bit_for_bit(dev, D):
    """(tok[ids] + pos[t]) rounded to bf16 by torch, and the plain gather for fp32 out; pad lanes zero (16 at D = 48, 28 at D = 100,
    none at 32 and 512), the memory after the last row untouched."""
    from jointimagegeneration_amd import ops
    gen = torch.Generator().manual_seed(D)
    stride = ops.pad32(D)
    for V in (1, 97):
        tok, pos = torch.randn(V, D, generator=gen), torch.randn(20, D, generator=gen)
        for B in (1, 3):
            for T_len in (1, 7, 20):
                ids = torch.randint(0, V, (B, T_len), generator=gen)
                ids.view(-1)[0] = V - 1
                ids.view(-1)[-1] = 0
                if ids.numel() > 3:
                    ids.view(-1)[1] = ids.view(-1)[2]                                     # a repeat
                want = tok[ids] + pos[:T_len][None]
                rc, rows, slack = raw_embed(ids, tok, pos, T_len, True, stride, dev)
                assert rc == 0 and torch.equal(rows[:, :D], want.bfloat16().view(-1, D)), (V, B, T_len)
                assert bool((rows[:, D:] == 0).all()) and bool((slack == SENTINEL).all())
                rc, rows, slack = raw_embed(ids, tok, None, T_len, False, D, dev)         # fp32, no pos, dense rows: ClassEmbedder's call
                assert rc == 0 and torch.equal(rows, tok[ids].view(-1, D)) and bool((slack == SENTINEL).all())
                rc, rows, slack = raw_embed(ids, tok, pos, T_len, False, stride, dev)
                assert rc == 0 and torch.equal(rows[:, :D], want.view(-1, D)) and bool((rows[:, D:] == 0).all()) and bool((slack == SENTINEL).all())
                got = ops.embed_rows(ids.to(dev), tok.to(dev), pos.to(dev), bf16=True)
                assert tuple(got.shape) == (B, 1, 1, T_len, stride) and torch.equal(got.cpu().view(-1, stride)[:, :D], want.bfloat16().view(-1, D))


def test_embed_rows_out_of_range_ids_and_refusals(dev):
    from jointimagegeneration_amd import ops
    gen = torch.Generator().manual_seed(1)
    tok, pos = torch.randn(97, 48, generator=gen), torch.randn(20, 48, generator=gen)
    ids = torch.tensor([[5, -1, 96], [97, 0, 2 ** 31 - 1]])
    rc, rows, slack = raw_embed(ids, tok, pos, 3, True, 64, dev)
    ok = torch.tensor([True, False, True, False, True, False])
    want = (tok[ids.clamp(0, 96)] + pos[:3][None]).bfloat16().view(-1, 48)
    assert rc == 0 and torch.equal(rows[ok][:, :48], want[ok]) and bool((rows[~ok] == 0).all()) and bool((slack == SENTINEL).all())
    assert raw_embed(ids, tok, pos, 3, True, 40, dev)[0] == GG_ERR_BAD_SHAPE                # stride < D
    assert raw_embed(ids, tok, pos, 4, True, 64, dev)[0] == GG_ERR_BAD_SHAPE                # rows are not whole sequences
    assert raw_embed(torch.zeros(1, 21, dtype=torch.long), tok, pos, 21, True, 64, dev)[0] == GG_ERR_BAD_SHAPE        # T > P
    with pytest.raises(ValueError, match=r"\[-1, 96\].*\[0, 97\)"):
        ops.embed_rows(torch.tensor([[5, -1, 96]], device=dev), tok.to(dev), pos.to(dev))
    with pytest.raises(ValueError, match=r"\[0, 97\].*\[0, 97\)"):
        ops.embed_rows(torch.tensor([[0, 97]], device=dev), tok.to(dev), pos.to(dev))
    with pytest.raises(ValueError, match="sequence length 21 exceeds max_seq_len 20"):
        ops.embed_rows(torch.zeros(1, 21, dtype=torch.long, device=dev), tok.to(dev), pos.to(dev))


# ------------------------------------------------------------------------------------------------ gg_gelu
@pytest.mark.parametrize("n", [1, 7, 4099])
def test_gelu_within_one_bf16_ulp_of_fp64(dev, n):
    """Every output within one bf16 ulp (the spacing at the reference's magnitude) of the fp64 erf-GELU of the bf16 input; where the
    reference is zero (x = 0, and x = -40 where even fp64 underflows) the output is zero."""
    from jointimagegeneration_amd import ops
    from jointimagegeneration_amd import _lib
    special = torch.tensor([0.0, 2.0 ** -20, -2.0 ** -20, 0.5, -0.5, 8.0, -8.0, 40.0, -40.0])
    k = min(n, special.numel())
    worst = 0.0
    for start in range(special.numel() - k + 1):                      # n = 1: nine calls, one special value each; n = 4099: all in one
        x = 3.0 * torch.randn(n, generator=torch.Generator().manual_seed(n + start))
        x[:k] = special[start:start + k]
        x = x.bfloat16()
        got = ops.gelu(x.to(dev))
        buf = torch.full((n + 64,), SENTINEL, dtype=torch.bfloat16, device=dev)
        _lib.check(_lib.load().gg_gelu(x.to(dev).data_ptr(), n, buf.data_ptr(), stream()), "gg_gelu")
        torch.cuda.synchronize()
        assert torch.equal(buf[:n], got) and bool((buf[n:] == SENTINEL).all())
        ref = cond_ref.gelu_f64(x)
        ulps = (got.cpu().double() - ref).abs() / cond_ref.bf16_ulp(ref)
        worst = max(worst, float(ulps[ref != 0].max()) if bool((ref != 0).any()) else 0.0)
        assert bool((ulps[ref != 0] <= 1.0).all()) and bool((got.cpu().double()[ref == 0] == 0).all()), (start, x[:k])
    print(f"gg_gelu n = {n}: max error {worst:.3f} bf16 ulp")


# ------------------------------------------------------------------------------------------------ gg_layernorm_rows
@pytest.mark.parametrize("C_", [8, 48, 100, 200])
def test_layernorm_rows_over_logical_channels(dev, C_):
    """LayerNorm over C of rows pad32(C) apart against fp64 on the same bf16 inputs.  Bound: the one rounding to bf16 (half an ulp, at most
    2^-8 |y|) plus fp32 arithmetic on terms of size max|gamma| max|xhat| + max|beta| (1e-5 of it).  Pad lanes zero."""
    from jointimagegeneration_amd import ops
    gen = torch.Generator().manual_seed(C_)
    cp = ops.pad32(C_)
    gamma, beta = 1.0 + 0.1 * torch.randn(C_, generator=gen), 0.05 * torch.randn(C_, generator=gen)
    for rows in (1, 5, 9):
        x = torch.zeros(rows, 1, 1, 1, cp)
        x[..., :C_] = 2.0 * torch.randn(rows, 1, 1, 1, C_, generator=gen) + 0.5
        xb = x.bfloat16()
        got = ops.layernorm_rows(ops.CL(xb.to(dev), C_), gamma.to(dev), beta.to(dev), 1e-5).t.cpu()
        ref = F.layer_norm(xb[..., :C_].double(), (C_,), gamma.double(), beta.double(), 1e-5)
        err = (got[..., :C_].double() - ref).abs()
        xhat = F.layer_norm(xb[..., :C_].double(), (C_,), None, None, 1e-5)
        bound = 2.0 ** -8 * ref.abs() + 1e-5 * float(gamma.abs().max() * xhat.abs().max() + beta.abs().max())
        assert bool((err <= bound).all()), (rows, float((err - bound).max()))
        assert bool((got[..., C_:] == 0).all())


# ------------------------------------------------------------------------------------------------ gg_interpolate2d_f32
@pytest.mark.parametrize("mode", cond_ref.MODES)
def test_interpolate_exact_cases_bit_for_bit(dev, mode):
    """Integer-valued planes, multipliers with dyadic weights: bit for bit against F.interpolate on the CPU."""
    from jointimagegeneration_amd import ops
    for i, shape in enumerate(cond_ref.EXACT_SHAPES):
        x = cond_ref.exact_input(shape, seed=i)
        for s in cond_ref.exact_multipliers(mode):
            got = ops.interpolate2d(x.to(dev), s, mode).cpu()
            assert torch.equal(got, F.interpolate(x, scale_factor=s, mode=mode)), (shape, s)


@pytest.mark.parametrize("mode", cond_ref.MODES)
def test_interpolate_general_multipliers(dev, mode):
    """Random normal planes at multipliers whose weights round.  nearest: bit for bit.  Others: e = max |y - F.interpolate(x.double())|
    at most 4 e_torch32 + 2^-22 max|x|, e_torch32 being fp32 CPU torch's own error in the same case (FMA contraction and another valid
    fp32 order, not a wrong tap)."""
    from jointimagegeneration_amd import ops
    gen = torch.Generator().manual_seed(11)
    worst = 0.0
    for shape in ((2, 3, 13, 10), (1, 1, 12, 8), (1, 2, 67, 45)):
        x = torch.randn(shape, generator=gen)
        for s in cond_ref.GENERAL_MULTIPLIERS:
            got = ops.interpolate2d(x.to(dev), s, mode).cpu()
            t32 = F.interpolate(x, scale_factor=s, mode=mode)
            if mode == "nearest":
                assert torch.equal(got, t32), (shape, s)
                continue
            ref = F.interpolate(x.double(), scale_factor=s, mode=mode)
            e, e_t = float((got.double() - ref).abs().max()), float((t32.double() - ref).abs().max())
            print(f"gg_interpolate2d_f32 {mode} {shape} x {s}: e = {e:.3e}, e_torch32 = {e_t:.3e}")
            worst = max(worst, e)
            assert e <= 4 * e_t + 2.0 ** -22 * float(x.abs().max()), (shape, s, e, e_t)
    print(f"gg_interpolate2d_f32 {mode}: worst e = {worst:.3e}")


def test_interpolate_refusals(dev):
    from jointimagegeneration_amd import _lib, ops
    x = torch.zeros(1, 1, 4, 4, device=dev)
    with pytest.raises(NotImplementedError, match="trilinear"):
        ops.interpolate2d(x, 0.5, "trilinear")
    with pytest.raises(ValueError, match="extent of 0"):
        ops.interpolate2d(x, 0.2, "nearest")
    out = torch.zeros(16, device=dev)
    lib = _lib.load()
    assert lib.gg_interpolate2d_f32(x.data_ptr(), 1, 4, 4, 0, 2, 2.0, 2.0, 0, out.data_ptr(), stream()) == GG_ERR_BAD_SHAPE
    assert lib.gg_interpolate2d_f32(x.data_ptr(), 1, 4, 4, 2, 2, 2.0, 2.0, 4, out.data_ptr(), stream()) == GG_ERR_BAD_SHAPE
    assert lib.gg_interpolate2d_f32(x.data_ptr(), 1, 4, 4, 2, 2, 0.0, 2.0, 1, out.data_ptr(), stream()) == GG_ERR_BAD_SHAPE
    assert b"interpolate2d" in lib.gg_last_error()


# ------------------------------------------------------------------------------------------------ modules against the reference's outputs
def test_class_embedder_is_an_exact_copy(dev, g):
    from jointimagegeneration_amd import cond
    ce = seeded(cond.ClassEmbedder(16, 11), "cond_cls.").to(dev)
    z = ce({"class": T(g["cls_labels"]).to(dev)})
    assert z.dtype == torch.float32 and tuple(z.shape) == (4, 1, 16) and torch.equal(z.cpu(), T(g["cls_z"]))
    assert torch.equal(ce({"label": T(g["cls_labels"]).long().to(dev)}, key="label"), z)
    with pytest.raises(ValueError, match=r"\[0, 11\]"):
        ce({"class": torch.tensor([0, 11], device=dev)})


@pytest.mark.parametrize("name", ["te", "bert", "te64"])
def test_embedders_match_reference_fixture(dev, g, name):
    """bf16 network with fp32 accumulation: rel_err < 3e-2, the bound of the SpatialTransformer module test (test_hip_parity.py).
    te / bert: width 48 (padded rows, gg_layernorm_rows); te64: width 64 (whole rows, gg_layernorm)."""
    m, kw = embedder(name)
    m = m.to(dev)
    for b, t in TOKEN_SHAPES:
        tok = T(g[f"{name}_{b}x{t}_tokens"]).to(dev)
        z = m.encode(tok)
        want = T(g[f"{name}_{b}x{t}_z"])
        e = rel_err(z, want)
        print(f"{name} tokens [{b}, {t}]: rel_err {e:.3e}")
        assert z.dtype == torch.float32 and tuple(z.shape) == (b, t, kw["n_embed"]) and e < 3e-2
        assert torch.equal(m(tok.long()), z)                                     # int32 and int64 tokens, encode == forward


@pytest.mark.parametrize("method", cond_ref.MODES)
def test_spatial_rescaler_matches_reference_fixture(dev, g, method):
    """With channel_mapper (bf16 1x1 conv): rel_err < 3e-2.  Without: the interpolation bounds (nearest bit for bit; others
    4 e_torch32 + 2^-22 max|x| against fp64 torch, per stage inputs being the previous stage's outputs)."""
    from jointimagegeneration_amd import cond
    x = T(g["rs_x"])
    for bias in (False, True):
        m = seeded(cond.SpatialRescaler(n_stages=1, method=method, multiplier=0.5, in_channels=3, out_channels=5, bias=bias), f"cond_rs_{method}_b{int(bias)}.").to(dev)
        y = m.encode(x.to(dev))
        e = rel_err(y, T(g[f"rs_{method}_b{int(bias)}"]))
        print(f"SpatialRescaler {method} bias={bias}: rel_err {e:.3e}")
        assert tuple(y.shape) == (2, 5, 6, 5) and e < 3e-2
    plain = cond.SpatialRescaler(n_stages=2, method=method, multiplier=0.5).eval()
    y = plain(x.to(dev)).cpu()
    want = T(g[f"rs_{method}_plain2"])
    if method == "nearest":
        assert torch.equal(y, want)
        return
    mid64 = F.interpolate(x.double(), scale_factor=0.5, mode=method)
    ref = F.interpolate(mid64, scale_factor=0.5, mode=method)
    e, e_t = float((y.double() - ref).abs().max()), float((want.double() - ref).abs().max())
    print(f"SpatialRescaler {method} two stages: e = {e:.3e}, e_torch32 = {e_t:.3e}")
    assert e <= 4 * e_t + 2.0 ** -22 * float(x.abs().max())


# ------------------------------------------------------------------------------------------------ the conditioning's way into the samplers
@pytest.fixture(scope="module")
def chain_ldm(dev):
    m = cond_ldm(dict(target="ldm.modules.encoders.modules.TransformerEmbedder", params=dict(TE, device="cpu")))
    return seeded(m, "ldm_cond.").to(dev)


def test_ddim_chain_with_transformer_embedder_vs_reference(dev, g, chain_ldm):
    """3 DDIM steps, eta = 0, conditioning = get_learned_conditioning(tokens) of the product embedder, against the reference's chain.
    Metric and bound of the ddim_options fixture comparison (test_hip_parity.py, the unguided chain: max 2e-2, rms 1.5e-2 of the
    reference).  The captured chain equals the eager one bit for bit."""
    from jointimagegeneration_amd.ldm import DDIMSampler
    m = chain_ldm
    tok, x_T = T(g["chain_tokens"]).to(dev), T(g["chain_x_T"]).to(dev)
    c = m.get_learned_conditioning(tok)
    ec = rel_err(c, T(g["chain_c"]))
    assert tuple(c.shape) == (2, 7, 48) and ec < 3e-2
    s = DDIMSampler(m)
    run = lambda smp, cc: smp.sample(S=3, batch_size=2, shape=(4, 8, 8), conditioning=cc, verbose=False, x_T=x_T, dims=2, eta=0.0)[0]
    z = run(s, c)
    assert list(s.ddim_timesteps) == list(g["chain_ddim_timesteps"])
    e, r = rel_err(z, T(g["chain_z"])), rms_err(z, T(g["chain_z"]))
    print(f"cond chain: conditioning rel_err {ec:.3e}; z max {e:.3e} rms {r:.3e} (of the reference's)")
    assert e < 2e-2 and r < 1.5e-2
    zs = run(s, c.flip(0).contiguous())                                            # each sample under the other's context: the reference's too
    assert rel_err(zs, T(g["chain_z_swapped"])) < 2e-2 and rms_err(zs, T(g["chain_z_swapped"])) < 1.5e-2
    z2 = run(s, c)                                                                  # the captured graph, replayed on reloaded inputs
    assert any(st["graph"] is not None for st in s._graphs.values()) and torch.equal(z, z2)
    s_eager = DDIMSampler(m)
    s_eager.use_graph = False
    assert torch.equal(run(s_eager, c), z)


def test_context_reaches_plms_ancestral_guided_and_hybrid_sampling(dev, g, chain_ldm):
    """The [B, T, D] conditioning as cross-attention context in PLMSSampler, p_sample_loop, classifier-free guidance (ClassEmbedder, the
    null class as unconditional_conditioning) and under the hybrid key: every run is finite and depends on the context."""
    from jointimagegeneration_amd.ldm import DDIMSampler, PLMSSampler
    tok, x_T = T(g["chain_tokens"]).to(dev), T(g["chain_x_T"]).to(dev)
    c = chain_ldm.get_learned_conditioning(tok)
    other = c.flip(0).contiguous()
    differs = lambda a, b: bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and rms_err(a, b) > 1e-2
    plms = lambda cc: PLMSSampler(chain_ldm).sample(S=3, batch_size=2, shape=(4, 8, 8), conditioning=cc, verbose=False, x_T=x_T)[0]
    assert differs(plms(c), plms(other))
    m4 = seeded(cond_ldm(dict(target="ldm.modules.encoders.modules.TransformerEmbedder", params=dict(TE)), timesteps=4), "ldm_cond.").to(dev)
    tape = list(torch.randn(4, 2, 4, 8, 8, generator=torch.Generator().manual_seed(3)))
    anc = lambda cc: m4.p_sample_loop(cc, (2, 4, 8, 8), x_T=x_T, verbose=False, noise_tape=tape)
    assert differs(anc(c), anc(other))
    assert torch.equal(anc({"c_crossattn": [c]}), anc(c))
    # ClassEmbedder: dict input through get_learned_conditioning; guidance with the null class (the last one)
    mc = seeded(cond_ldm(dict(target="ldm.modules.encoders.modules.ClassEmbedder", params=dict(embed_dim=48, n_classes=11))), "ldm_cls.").to(dev)
    cc = mc.get_learned_conditioning({"class": torch.tensor([3, 7], device=dev)})
    uc = mc.get_learned_conditioning({"class": torch.tensor([10, 10], device=dev)})
    assert tuple(cc.shape) == (2, 1, 48) and torch.equal(cc.cpu(), mc.cond_stage_model.embedding.weight[[3, 7]][:, None].cpu())
    sc = DDIMSampler(mc)
    guided = sc.sample(S=3, batch_size=2, shape=(4, 8, 8), conditioning=cc, verbose=False, x_T=x_T, dims=2, unconditional_guidance_scale=3.0,
                       unconditional_conditioning=uc)[0]
    plain = sc.sample(S=3, batch_size=2, shape=(4, 8, 8), conditioning=cc, verbose=False, x_T=x_T, dims=2)[0]
    assert differs(guided, plain)
    # hybrid: a concat latent and the embedder's context in one dict
    mh = seeded(cond_ldm(dict(target="ldm.modules.encoders.modules.TransformerEmbedder", params=dict(TE)), key="hybrid", in_channels=8), "ldm_hyb.").to(dev)
    assert mh.model.conditioning_key == "hybrid"
    lat = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(4)).to(dev)
    ch = mh.get_learned_conditioning(tok)
    hyb = lambda ctx, l: DDIMSampler(mh).sample(S=3, batch_size=2, shape=(4, 8, 8), conditioning=dict(c_concat=[l], c_crossattn=[ctx]),
                                               verbose=False, x_T=x_T, dims=2)[0]
    base = hyb(ch, lat)
    assert differs(base, hyb(ch.flip(0).contiguous(), lat)) and differs(base, hyb(ch, lat.flip(0).contiguous()))


def test_a_second_guided_call_allocates_nothing_for_the_unconditional_inputs(dev, g, chain_ldm):
    """Classifier-free guidance on a full-size (not patch-wise) state: the unconditional UNet input and context are members of the
    state, made on the first guided call and refilled by the second, which leaves no byte behind and follows its new inputs."""
    from jointimagegeneration_amd.ldm import DDIMSampler
    tok, x_T = T(g["chain_tokens"]).to(dev), T(g["chain_x_T"]).to(dev)
    c = chain_ldm.get_learned_conditioning(tok)
    uc, uc2 = c.flip(0).contiguous(), (c * 0.5).contiguous()
    s = DDIMSampler(chain_ldm)
    run = lambda u: s.sample(S=3, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, dims=2, unconditional_guidance_scale=3.0,
                             unconditional_conditioning=u)[0]
    z = run(uc)
    assert len(s._graphs) == 1
    st = next(iter(s._graphs.values()))
    members = (st["cfg_unet_in"], st["cfg_ctx"].t)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    z2 = run(uc)
    torch.cuda.synchronize()
    same = torch.equal(z, z2)
    del z2
    assert torch.cuda.memory_allocated() == before and same
    assert st["cfg_unet_in"] is members[0] and st["cfg_ctx"].t is members[1]
    assert not torch.equal(run(uc2), z) and torch.equal(run(uc), z)                 # refilled: nothing of the other call is left in them
